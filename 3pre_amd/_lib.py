"""ctypes binding of lib/libpre3.so (the C ABI of include/pre3.h).

There is no CPU fallback: if the shared library is missing this module raises at import, and
every compute call raises Pre3Error when no HIP device is present.
"""
import ctypes as C
import os

import numpy as np

try:  # torch ships its own libamdhip64.so.7; load it first so both share ONE HIP runtime
    import torch  # noqa: F401
except Exception:  # pragma: no cover - torch is plumbing, not a requirement of the library
    torch = None

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PRE3_LIB") or os.path.join(_HERE, "lib", "libpre3.so")      # PRE3_LIB: A/B builds while tuning

if not os.path.exists(LIB_PATH):
    raise ImportError(
        "3pre_amd: %s is missing -- build it with `make -C 3pre_amd/csrc` (or __graft_entry__.build()); "
        "there is no CPU fallback for the HIP path" % LIB_PATH)

lib = C.CDLL(LIB_PATH)
lib.pre3_last_error.restype = C.c_char_p
lib.pre3_version.restype = C.c_char_p
lib.pre3_match_bench_create.restype = C.c_void_p
lib.pre3_match_bench_create_cls.restype = C.c_void_p
lib.pre3_hypothesis_support.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
lib.pre3_step.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_int, C.c_double, C.c_void_p]
lib.pre3_plane_fit.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
lib.pre3_plane_bench.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
lib.pre3_heading_from_scan.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
lib.pre3_step_predicted.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_int, C.c_double, C.c_void_p]
_P, _I, _D, _U = C.c_void_p, C.c_int, C.c_double, C.c_uint64
lib.pre3_ransac_seeded.argtypes = [_P, _U, _U, _I, _D, _I, _P, _P, _P, _P, _P]
lib.pre3_step_seeded.argtypes = [_P, _P, _I, _P, _P, _U, _U, _I, _D, _I, _D, _P, _P, _P]
lib.pre3_step_predicted_seeded.argtypes = [_P, _U, _U, _I, _D, _I, _D, _P, _P, _P]
lib.pre3_vo_ransac_seeded.argtypes = [_I, _I, _P, _P, _P, _I, _U, _U, _P, _P, _P, _P, _P, _P]
lib.pre3_vo_ransac_frames_seeded.argtypes = [_I, _I, _I, _P, _P, _P, _P, _P, _P, _I, _I, _P, _I, _P, _I, _P, _I, _U, _U, _P, _P, _P, _P, _P, _P, _P, _P]
lib.pre3_plane_fit_seeded.argtypes = [_I, _I, _I, _P, _P, _P, _P, _D, _I, _U, _U, _P, _P, _P, _P]
lib.pre3_heading_from_scan_seeded.argtypes = [_P, _I, _I, _P, _P, _P, _P, _D, _I, _U, _U, _I, _I, _P, _P, _P]
lib.pre3_candidate_order.argtypes = [_I, _I, _P, _I, _I, _U, _U, _P, _P]
lib.pre3_map_policy_seeded.argtypes = [_P, _I, _I, _D, _D, _I, _I, _P, _P, _P, _I, _I, _U, _U, _P, _P, _P, _P, _P, _P, _P]
lib.pre3_sr_gauss3.argtypes = [_D, _P]
lib.pre3_sr_frame_create.argtypes = [_P, _I, _I, _I]
lib.pre3_sr_frame_destroy.argtypes = [_P]
lib.pre3_sr_frame_load.argtypes = [_P, _I, _P, _P, _P, _P, _P]
lib.pre3_sr_frame_get.argtypes = [_P, _P, _P, _P, _P, _P, _P, _P]
lib.pre3_sr_frame_keypoints.argtypes = [_P, _I, _I, _I, _P, _I, _P, _P, _P, _P, _P, _P, _P]
lib.pre3_vo_pair_seeded.argtypes = [_P, _P, _D, _U, _U, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]
lib.pre3_map_policy_frames_seeded.argtypes = [_P, _P, _P, _D, _I, _I, _D, _D, _I, _I, _I, _U, _U, _P, _P, _P, _P, _P, _P, _P, _P, _P]
lib.pre3_plane_fit_frame.argtypes = [_P, _P, _D, _I, _P, _P, _P, _P]
lib.pre3_plane_fit_frame_seeded.argtypes = [_P, _P, _D, _I, _U, _U, _P, _P, _P, _P]
lib.pre3_heading_from_frame.argtypes = [_P, _P, _P, _D, _I, _P, _I, _I, _P, _P]
lib.pre3_heading_from_frame_seeded.argtypes = [_P, _P, _P, _D, _I, _U, _U, _I, _I, _P, _P, _P]
lib.pre3_set_scan_frame.argtypes = [_P, _P, _I]
lib.pre3_predict_pair_seeded.argtypes = [_P, _P, _P, _D, _U, _U, _P, _P]
lib.pre3_predict_cv.argtypes = [_P, _I, _D, _D, _D]
lib.pre3_set_process_noise.argtypes = [_P, _P]
lib.pre3_get_process_noise.argtypes = [_P, _P, _P]
lib.pre3_vo_cov.argtypes = [_I, _I, _P, _P, _P, _P, _P, _P, _P]
lib.pre3_vo_pair_cov_seeded.argtypes = [_P, _P, _D, _U, _U, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]
lib.pre3_predict_pair_cov_seeded.argtypes = [_P, _P, _P, _D, _U, _U, _P, _P, _P, _P]
lib.pre3_sift_plan_get.argtypes = [_I, _I, _P, _P, _P, _P, _P, _P, _P, _P]
lib.pre3_sr_frame_sift.argtypes = [_P, _P, _I, _I, _P, _P, _P, _P]
lib.pre3_sr_frame_gate.argtypes = [_P, _I, _P, _P, _P, _P, _P, _P]
lib.pre3_sr_frame_sift_level.argtypes = [_P, _I, _I, _I, _P]
lib.pre3_sr_frame_sift_refined.argtypes = [_P, _P, _P]
lib.pre3_sr_text_limits.argtypes = [_P, _P]
lib.pre3_sr_text_parse.argtypes = [_I, _P, C.c_size_t, _P, C.c_size_t, _P]
lib.pre3_sr_frame_load_text.argtypes = [_P, _I, _P, C.c_size_t, _P]
lib.pre3_sr_frame_set_compensation.argtypes = [_P, _I, _D]
lib.pre3_sr_frame_get_compensation.argtypes = [_P, _P, _P]
lib.pre3_sr_frame_bad_pixels.argtypes = [_P, _P, _P]
lib.pre3_sr_medfilt3.argtypes = [_I, _I, _I, _P, _I, _P]
lib.pre3_set_image.argtypes = [_P, _I, _I, _P]
lib.pre3_get_image.argtypes = [_P, _I, _I, _P]
lib.pre3_set_image_frame.argtypes = [_P, _P]
lib.pre3_set_patches.argtypes = [_P, _I, _I, _P, _P, _P, _P]
lib.pre3_get_patches.argtypes = [_P, _I, _I, _P, _P, _P, _P, _P]
lib.pre3_patch_cut.argtypes = [_P, _I, _I, _P]
lib.pre3_predict_patches.argtypes = [_P, _D, _P, _P]
lib.pre3_patch_search.argtypes = [_P, _D, _D, _I, _P, _P, _P, _P, _P, _P]
lib.pre3_patch_timing.argtypes = [_P, _P, _P]
lib.pre3_fast_detect.argtypes = [_P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P]
lib.pre3_fast_timing.argtypes = [_P, _P]
lib.pre3_init_feature_fast.argtypes = [_P, _P, _D, _I, _I, _I, _P, _I, _P]
lib.pre3_init_feature_fast_seeded.argtypes = [_P, _P, _D, _I, _I, _I, _U, _U, _P]
lib.pre3_init_features_fast_all.argtypes = [_P, _P, _D, _I, _I, _P, _P, _P, _P, _P]
lib.pre3_icp.argtypes = [_I, _P, _I, _P, _I, _D, _P, _P, _P, _P, _P, _P]
lib.pre3_icp_limits.argtypes = [_P]
lib.pre3_icp_frames.argtypes = [_P, _P, _I, _D, _P, _P, _P, _P, _P, _P, _P]
lib.pre3_icp_pair_seeded.argtypes = [_P, _P, _D, _U, _U, _I, _D, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]
lib.pre3_icp_nn_bench.argtypes = [_I, _P, _I, _P, _I, _I, _P]
lib.pre3_icp_cov.argtypes = [_I, _P, _I, _P, _I, _P, _I, _P, _P, _P, _P]
lib.pre3_icp_cov_limits.argtypes = [_P]
lib.pre3_icp_cov_bench.argtypes = [_I, _P, _I, _P, _I, _P, _I, _P, _I, _P]
lib.pre3_predict_icp_pair_seeded.argtypes = [_P, _P, _P, _D, _U, _U, _I, _D, _D, _I, _P, _P, _P, _P, _P, _P]
lib.pre3_icp_pair_cov_seeded.argtypes = [_P, _P, _D, _U, _U, _I, _D, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]
lib.pre3_epnp.argtypes = [_I, _P, _I, _I, _P, _P, _P]
lib.pre3_pnp_ransac.argtypes = [_I, _P, _I, _I, _P, _P, _I, _P, _D, _P, _P, _P, _P, _P]
lib.pre3_pnp_ransac_seeded.argtypes = [_I, _P, _I, _I, _P, _P, _I, _U, _U, _D, _P, _P, _P, _P, _P, _P]
lib.pre3_pnp_limits.argtypes = [_P]
lib.pre3_vo_pair_pnp_seeded.argtypes = [_P, _P, _D, _U, _U, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]
lib.pre3_pnp_bench.argtypes = [_I, _P, _I, _I, _P, _P, _I, _U, _U, _D, _I, _P]
lib.pre3_relocalise_seeded.argtypes = [_P, _D, _I, _U, _U, _D, _I, _I, _P, _P, _P, _P]
lib.pre3_reloc_limits.argtypes = [_P]
lib.pre3_pnp_refine.argtypes = [_I, _P, _I, _I, _P, _P, _P, _P, _I, _D, _P]
lib.pre3_pnp_ransac_refined_seeded.argtypes = [_I, _P, _I, _I, _P, _P, _I, _U, _U, _D, _P, _P, _P, _P, _P, _P, _I, _D, _P]
lib.pre3_relocalise_refined_seeded.argtypes = [_P, _D, _I, _U, _U, _D, _I, _I, _I, _D, _I, _P, _P, _P, _P]
lib.pre3_test_downdate.argtypes = [_P, _I, _P, _I]            # csrc/pre3_test_hooks.h, not include/pre3.h: not in EXPORTS
lib.pre3_test_factor_solve.argtypes = [_P, _I, _P, _P, _P, _I, _I, _P, _P]      # (the same)

F64, F32 = 0, 1
INVDEPTH, CARTESIAN = 0, 1
X_K_K, X_K_KM1 = 0, 1
FAST_MAX_CORNERS, FAST_MAX_ATTEMPTS = 8192, 10


class FastInitResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("attempts", C.c_int32), ("uv", C.c_int32 * 2), ("landmark", C.c_int32), ("pad", C.c_int32), ("rho", C.c_double),
                ("xyz", C.c_double * 3), ("centres", C.c_int32 * 20)]


class Cam(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("f", "Cx", "Cy", "k1", "k2", "nRows", "nCols")]


class Pre3Error(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libpre3 error %d: %s" % (code, msg))
        self.code = code


def check(rc):
    if rc != 0:
        raise Pre3Error(rc, lib.pre3_last_error().decode(errors="replace"))


def dptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def addr(a):
    """Address of a C-contiguous array as an int: 0.3 us through the buffer protocol instead of 2 us through ndarray.ctypes
    (the per-step wrapper overhead is GPU idle time); falls back for read-only or empty arrays."""
    try:
        return C.addressof(C.c_char.from_buffer(a))
    except (TypeError, ValueError, BufferError):
        return a.ctypes.data


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def device_count():
    return int(lib.pre3_device_count())


# every symbol include/pre3.h declares (checked by tests/test_abi.py against the header text)
EXPORTS = [
    "pre3_last_error", "pre3_device_count", "pre3_version", "pre3_create", "pre3_destroy", "pre3_sync", "pre3_set_cam",
    "pre3_set_map", "pre3_state_size", "pre3_set_state", "pre3_get_state", "pre3_get_landmarks", "pre3_get_marginal", "pre3_predict", "pre3_predict_dense", "pre3_project", "pre3_innovation",
    "pre3_get_landmark_fields", "pre3_window_gate", "pre3_set_measurements", "pre3_ransac", "pre3_hypothesis_support", "pre3_ransac_score",
    "pre3_ransac_select", "pre3_ransac_export", "pre3_ransac_import", "pre3_update_li", "pre3_rescue", "pre3_update_hi", "pre3_update_all", "pre3_update_rows", "pre3_heading_update", "pre3_plane_fit", "pre3_heading_from_scan", "pre3_plane_bench", "pre3_get_flags",
    "pre3_set_flags", "pre3_step", "pre3_step_all", "pre3_step_predicted", "pre3_set_option", "pre3_get_option", "pre3_map_delete", "pre3_map_add_inverse_depth", "pre3_map_inversedepth_2_cartesian", "pre3_map_management", "pre3_get_map", "pre3_set_book", "pre3_get_book", "pre3_map_policy", "pre3_set_descriptors", "pre3_get_descriptors", "pre3_set_scan", "pre3_ic_search", "pre3_vo_ransac", "pre3_vo_ransac_frames", "pre3_vo_bench", "pre3_update_ell", "pre3_siftmatch_f64", "pre3_siftmatch_f32", "pre3_siftmatch_u8",
    "pre3_siftmatch_i8", "pre3_siftmatch_partial", "pre3_siftmatch_merge", "pre3_match_shard_create", "pre3_match_shard_create_cls", "pre3_match_shard_run", "pre3_match_shard_merge",
    "pre3_match_shard_destroy", "pre3_release_scratch", "pre3_knn_f64", "pre3_timer_start",
    "pre3_timer_stop", "pre3_kernel_timing", "pre3_kernel_timing_read", "pre3_kernel_timing_info", "pre3_bench_downdate",
    "pre3_match_bench_create", "pre3_match_bench_create_cls", "pre3_match_bench_info", "pre3_match_bench_run", "pre3_match_bench_fetch", "pre3_match_bench_destroy",
    "pre3_comm_unique_id", "pre3_comm_create", "pre3_comm_destroy", "pre3_comm_info", "pre3_comm_set_timeout", "pre3_set_comm", "pre3_comm_init", "pre3_match_shard_set_comm",
    "pre3_ransac_sharded", "pre3_match_shard_match",
    "pre3_ransac_seeded", "pre3_step_seeded", "pre3_step_predicted_seeded", "pre3_vo_ransac_seeded", "pre3_vo_ransac_frames_seeded",
    "pre3_plane_fit_seeded", "pre3_heading_from_scan_seeded",
    "pre3_candidate_order", "pre3_map_policy_seeded",
    "pre3_sr_gauss3", "pre3_sr_frame_create", "pre3_sr_frame_destroy", "pre3_sr_frame_load", "pre3_sr_frame_get", "pre3_sr_frame_keypoints",
    "pre3_vo_pair_seeded", "pre3_map_policy_frames_seeded",
    "pre3_plane_fit_frame", "pre3_plane_fit_frame_seeded", "pre3_heading_from_frame", "pre3_heading_from_frame_seeded", "pre3_set_scan_frame",
    "pre3_predict_pair_seeded", "pre3_predict_cv",
    "pre3_set_process_noise", "pre3_get_process_noise", "pre3_vo_cov", "pre3_vo_pair_cov_seeded", "pre3_predict_pair_cov_seeded",
    "pre3_sift_plan_get", "pre3_sr_frame_sift", "pre3_sr_frame_gate", "pre3_sr_frame_sift_level", "pre3_sr_frame_sift_refined",
    "pre3_sr_text_limits", "pre3_sr_text_parse", "pre3_sr_frame_load_text",
    "pre3_sr_frame_set_compensation", "pre3_sr_frame_get_compensation", "pre3_sr_frame_bad_pixels", "pre3_sr_medfilt3",
    "pre3_set_image", "pre3_get_image", "pre3_set_image_frame", "pre3_set_patches", "pre3_get_patches", "pre3_patch_cut", "pre3_predict_patches",
    "pre3_patch_search", "pre3_patch_timing",
    "pre3_fast_detect", "pre3_fast_timing", "pre3_init_feature_fast", "pre3_init_feature_fast_seeded", "pre3_init_features_fast_all",
    "pre3_icp", "pre3_icp_limits", "pre3_icp_frames", "pre3_icp_pair_seeded", "pre3_icp_nn_bench",
    "pre3_icp_cov", "pre3_icp_cov_limits", "pre3_icp_cov_bench", "pre3_icp_pair_cov_seeded", "pre3_predict_icp_pair_seeded",
    "pre3_epnp", "pre3_pnp_ransac", "pre3_pnp_ransac_seeded", "pre3_pnp_limits", "pre3_pnp_bench", "pre3_vo_pair_pnp_seeded",
    "pre3_relocalise_seeded", "pre3_reloc_limits",
    "pre3_pnp_refine", "pre3_pnp_ransac_refined_seeded", "pre3_relocalise_refined_seeded",
]
