"""The live-block count of tests/test_gpu_regrow.py, in a process of its own (the counters are the process's; PRE3_TEST_HOOKS=1 arms the hook):

    PRE3_TEST_HOOKS=1 python tests/regrow_worker.py        -> one line on stdout: LIVEJSON {"base": [4 ints], "end": [4 ints], "peak": [4 ints]}

A warm-up creates what belongs to the process and stays (the pinned blocks of the stateless ICP and plane fit, the text parse's table), closes one
context and one frame handle and releases the scratch pool; `base` is read there.  Then an f32 and an f64 context at N = 8 and one frame handle touch
every block they can own (`peak` is read while they live); everything is closed, the pool released, and `end` is read."""
import ctypes as C
import importlib
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import plane_fit_ref as pr  # noqa: E402
import sr_frame_ref as sr  # noqa: E402

N, ROWS, COLS = 8, 24, 32


def live(lib):
    out = (C.c_int64 * 4)()
    assert lib.pre3_test_live_blocks(out) == 0
    return [int(v) for v in out]


def dat_text(fr):
    a = np.vstack([fr[k] for k in ("z", "x", "y", "amp", "conf")])
    buf = io.BytesIO()
    np.savetxt(buf, a, fmt="%.17g")
    return buf.getvalue()


def touch_frame(srm, rng):
    fr = sr.make_frame(ROWS, COLS, seed=3)
    f = srm.SrFrame(ROWS, COLS)
    f.load(fr, 1)
    frm = np.stack([rng.uniform(1, COLS, 40), rng.uniform(1, ROWS, 40), np.full(40, 2.0), np.zeros(40)])
    f.keypoints(frm, np.abs(rng.normal(0, 1, (128, 40))), 1)
    f.sift(want_arrays=False)
    f.load_text(dat_text(fr), 1)
    return f


def touch_context(pre3, synth, dtype, rng):
    cam = synth.CAM.copy()
    x, P, _ = synth.make_map(N, seed=5)
    f = pre3.EkfFilter(cam, np.zeros(N, np.int32), dtype=dtype, max_hyp=8, max_landmarks=N + 4)
    f.set_x_p_k_k(x, P)
    f.landmarks(); f.marginal([0, 3, 14])                                                   # the readers' two pairs
    H = np.zeros((2, f.n)); H[0, 0] = 1.0; H[1, 13] = 1.0
    f.update(H, None, [0.0, 0.0], [0.0, 0.0])                                               # the rows block
    xs, ys, zs, _ = pr.scene(0, 0.1)
    f.heading_from_scan(xs, ys, zs, pr.scene_draws(0, 65 * 71, 16))                         # the plane fit's work block
    f.set_descriptors(np.abs(rng.normal(0, 1, (128, N))))                                   # the IC group, the upload ring
    f.ekf_prediction(np.array([0, 0, 0, 1.0, 0, 0, 0]))
    f.load_scan(np.abs(rng.normal(0, 1, (128, 30))), np.stack([rng.uniform(1, 176, 30), rng.uniform(1, 144, 30), np.full(30, 2.0), np.zeros(30)]))
    f.matching_sift_based(1.5)
    f.set_x_p_k_k(x, P)
    im = rng.integers(0, 255, (int(cam[5]), int(cam[6]))).astype(np.uint8)
    f.set_image(im)                                                                         # the patch state, its image
    f.patch_cut(np.tile([[60, 50]], (N, 1)))
    f.ekf_prediction(np.array([0, 0, 0, 1.0, 0, 0, 0]))
    f.search_ic_matches_patch(300.0)
    f.fast_corner_detect_9(20)                                                              # the FAST state, its map
    f.set_x_p_k_k(x, P)
    f.set_book(np.zeros((N, 4), np.int32))                                                  # the book trio
    f.map_management_policy(5, np.array([[40.0, 50.0], [90.0, 70.0]]), np.array([[0.1, 0.1, 2.0], [0.2, -0.1, 3.0]]), min_features=N + 1)     # the policy pair, the map group, the map ring
    f.delete_features([0])
    return f


def main():
    pre3 = importlib.import_module("3pre_amd")
    synth = importlib.import_module("3pre_amd.synth")
    srm = importlib.import_module("3pre_amd.sr4000")
    vo = importlib.import_module("3pre_amd.vo")
    plane = importlib.import_module("3pre_amd.plane")
    lib = C.CDLL(pre3.LIB_PATH)
    lib.pre3_test_live_blocks.argtypes = [C.POINTER(C.c_int64)]
    rng = np.random.default_rng(11)
    # ---- warm-up: what the process keeps, and one context and one handle created and closed
    xs, ys, zs, _ = pr.scene(0, 0.1)
    plane.plane_fit(xs, ys, zs, pr.scene_draws(0, 65 * 71, 16))
    pts = rng.normal(0, 1, (3, 200))
    vo.icp_with_init(pts, pts + 0.01, 0.02)
    touch_frame(srm, rng).close()
    touch_context(pre3, synth, "f64", rng).close()
    lib.pre3_release_scratch()
    base = live(lib)
    # ---- every lazy group of two contexts and a handle
    held = [touch_context(pre3, synth, "f32", rng), touch_context(pre3, synth, "f64", rng), touch_frame(srm, rng)]
    peak = live(lib)
    for h in held:
        h.close()
    lib.pre3_release_scratch()
    print("LIVEJSON " + json.dumps(dict(base=base, peak=peak, end=live(lib))))


if __name__ == "__main__":
    main()
