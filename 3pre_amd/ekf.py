"""Host-side mirror of the reference's EKF interface for the hot path, over the C ABI (include/pre3.h).

Names, argument meaning and error behaviour follow the MATLAB functions they replace (paths under
matlab_code/ of the reference):

    EkfFilter                     <-> @ekf_filter/ekf_filter.m:27-89 (x_k_k, p_k_k, x_k_km1, p_k_km1, std_z ...)
      .ekf_prediction(u)          <-> @ekf_filter/ekf_prediction.m:29 -> predict_state_and_covariance.m:27
      .ekf_prediction_cv(dt, sigma_a, sigma_alpha, type)  <-> the same with the camera-only models (fv.m:64-106, dfv_by_dxv.m, func_Q.m)
      .search_IC_matches()        <-> search_IC_matches.m:31-44 (projection, Jacobians, S_i)
      .matching(k1, zc)           <-> matching_sift_based.m:119-134 (window gate on siftmatch's output)
      .ransac_hypotheses(hyp)     <-> ransac_hypotheses.m:27-85 (draws are an input: MATLAB's RNG is not reproducible)
      .ransac_hypotheses_seeded / .step_seeded / .step_predicted_seeded / .heading_from_scan_seeded
                                  <-> the same with the draws made on the device from (seed, seq) (select_random_match.m:40-51, ransac.m:142-176)
      .ekf_update_li_inliers()    <-> @ekf_filter/ekf_update_li_inliers.m:45-58
      .rescue_hi_inliers()        <-> @ekf_filter/rescue_hi_inliers.m:29-47
      .ekf_update_hi_inliers()    <-> @ekf_filter/ekf_update_hi_inliers.m:45-58
      .ekf_update_all()           <-> @ekf_filter/ekf_update_all.m:46-62
      .landmarks() / .marginal()  <-> plots_complete.m:161-237, inversedepth_2_cartesian.m:36-62 (what they read of x and P, without fetching P)
      .map_management_policy()    <-> map_management.m:27-79 with delete_features.m / update_features_info.m / initialize_features.m's policy
    update(x, P, H, R, z, h)      <-> update.m:27   (stateless drop-in: host arrays in, host arrays out)
    predict_state_and_covariance  <-> predict_state_and_covariance.m:27 (u passed explicitly instead of fv.m's disk read)

All compute runs in libpre3.so on the GPU; this module only marshals numpy arrays.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import Cam, Pre3Error, addr, check, dptr, f64, i32, lib

CHI2INV_2_95 = 5.9915          # rescue_hi_inliers.m:29


def _cam(cam):
    if isinstance(cam, dict):
        cam = [cam[k] for k in ("f", "Cx", "Cy", "k1", "k2", "nRows", "nCols")]
    return Cam(*[float(v) for v in cam])


class EkfFilter:
    """Device-resident filter state.  dtype: 'f64' or 'f32' (covariance path); geometry is always fp64."""

    def __init__(self, cam, lm_type, dtype="f32", device=0, max_hyp=1000, max_landmarks=None, std_z=1.0):
        lm_type = i32(lm_type)
        self.N = int(lm_type.shape[0])
        self.dtype = {"f64": _lib.F64, "f32": _lib.F32}[dtype]
        self.std_z = float(std_z)
        self._ctx = C.c_void_p()
        check(lib.pre3_create(C.byref(self._ctx), int(device), self.dtype, int(max_landmarks or max(self.N, 1)), int(max_hyp)))
        c = _cam(cam)
        check(lib.pre3_set_cam(self._ctx, C.byref(c)))
        self._image_shape = (int(c.nRows), int(c.nCols))     # the resident image has the camera's shape
        check(lib.pre3_set_map(self._ctx, self.N, dptr(lm_type)))
        self.n = int(lib.pre3_state_size(self._ctx))
        self.lm_type = lm_type
        self.m = 0
        self.meas_idx = np.zeros(0, np.int32)            # the installed measurements' landmarks (the flags of get_flags are in this order)
        self._st = np.zeros(8, np.int32)                 # pre3_step's statistics block (kept: the wrapper's time is GPU idle time)
        self._st_addr = self._st.ctypes.data

    def close(self):
        if getattr(self, "_ctx", None) and lib is not None:        # (lib is None while the interpreter shuts down)
            lib.pre3_destroy(self._ctx)
            self._ctx = None

    __del__ = close

    # ---- state (set_x_k_k.m / get_x_k_k.m ...)
    def set_x_p_k_k(self, x, P):
        x, P = f64(x), f64(P)
        check(lib.pre3_set_state(self._ctx, _lib.X_K_K, x.shape[0], dptr(x), dptr(P)))

    def set_x_p_k_km1(self, x, P):
        x, P = f64(x), f64(P)
        check(lib.pre3_set_state(self._ctx, _lib.X_K_KM1, x.shape[0], dptr(x), dptr(P)))

    def _get(self, which, want_P=True):
        x = np.empty(self.n)
        P = np.empty((self.n, self.n)) if want_P else None
        check(lib.pre3_get_state(self._ctx, which, self.n, dptr(x), dptr(P)))
        return x, P

    def get_x_k_k(self):
        return self._get(_lib.X_K_K, False)[0]

    def get_p_k_k(self):
        return self._get(_lib.X_K_K)[1]

    def get_x_k_km1(self):
        return self._get(_lib.X_K_KM1, False)[0]

    def get_p_k_km1(self):
        return self._get(_lib.X_K_KM1)[1]

    # ---- marginals without fetching P (pre3_get_landmarks / pre3_get_marginal)
    def landmarks(self, which=_lib.X_K_K, first=0, count=None):
        """The map as 3-D points with their uncertainty, as plots_complete.m:208-237 draws it (inversedepth2cartesian.m for the point,
        inversedepth_2_cartesian.m:58-62's J for its 3x3 covariance J P_ii J', inversedepth_2_cartesian.m:36-49's linearity index), for
        landmarks first .. first+count-1 (count None: to the end of the map).  Returns a dict of xyz (count, 3), cov_xyz (count, 3, 3),
        cov_native (count, 6, 6: the landmark's own block of P; a Cartesian landmark's 3x3 in the top-left corner, the rest 0) and linearity
        (count,: -1 for a Cartesian landmark).  A deferred HI update is completed first; a pending HI down-date is applied by the reading launch
        and stays pending (the filter's next step is not changed by the read)."""
        first = int(first)
        count = self.N - first if count is None else int(count)
        k = max(count, 0)
        xyz, cxyz = np.zeros((max(k, 1), 3)), np.zeros((max(k, 1), 3, 3))
        cnat, lin = np.zeros((max(k, 1), 6, 6)), np.zeros(max(k, 1))
        check(lib.pre3_get_landmarks(self._ctx, int(which), first, count, dptr(xyz), dptr(cxyz), dptr(cnat), dptr(lin)))
        return {"xyz": xyz[:k].copy(), "cov_xyz": cxyz[:k].copy(), "cov_native": cnat[:k].copy(), "linearity": lin[:k].copy()}

    def marginal(self, idx, which=_lib.X_K_K):
        """(x[idx], P[idx][:, idx]) for any index set (unsorted, repeats allowed): the pose plots_complete.m:161-164, 185 reads (idx 0..6),
        a landmark's block (plots_complete.m:208-237), P(rho, rho) of inversedepth_2_cartesian.m:41, or any pose-landmark cross term --
        without copying P to the host.  Same pending rule as landmarks()."""
        ix = i32(np.asarray(idx, dtype=np.int64).reshape(-1))
        k = int(ix.shape[0])
        x, P = np.zeros(max(k, 1)), np.zeros((max(k, 1), max(k, 1)))
        check(lib.pre3_get_marginal(self._ctx, int(which), k, dptr(ix), dptr(x), dptr(P)))
        return x[:k].copy(), P[:k, :k].copy()

    def pose(self, which=_lib.X_K_K):
        """marginal(range(7)): the camera position and quaternion x(1:7) and their 7x7 covariance (plots_complete.m:161-164, 185)."""
        return self.marginal(np.arange(7), which)

    # ---- other measurements on the resident current estimate (pre3_update_rows / pre3_heading_update)
    def update(self, H, R, z, h):
        """[x_k_k, p_k_k] = update(x_k_k, p_k_k, H, R, z, h) (update.m:27-56) in place on the device: H r x n (dense or scipy sparse, at most 16
        non-zeros per row), R r x r or None for eye(r).  Up to 16 rows: one sweep of P (rows_form() == 1); more: the general route."""
        z, h = f64(z).ravel(), f64(h).ravel()
        r = int(z.shape[0])
        if h.shape[0] != r:
            raise Pre3Error(-1, "update: z and h differ in length")
        if r == 0:
            check(lib.pre3_update_rows(self._ctx, 0, 1, None, None, None, None, None, None))
            return
        if H.shape != (r, self.n):
            raise Pre3Error(-1, "update: H must be %d x %d" % (r, self.n))
        width, nnz, col, val = _to_ell(H, self.n)
        if width > 16:
            raise Pre3Error(-1, "update: H has a row with %d non-zeros; the measurement rows of this filter have 13 (max 16)" % width)
        col, val = i32(col), f64(val)
        Rm = None if R is None else f64(R)
        if Rm is not None and Rm.shape != (r, r):
            raise Pre3Error(-1, "update: R must be %d x %d" % (r, r))
        check(lib.pre3_update_rows(self._ctx, r, width, dptr(nnz), dptr(col), dptr(val), dptr(Rm), dptr(z), dptr(h)))

    def ekf_heading_update(self, R_plane, strict_reference=True):
        """@ekf_filter/ekf_heading_update.m:27-52: corrects the camera's orientation from the rotation of a fitted plane, R_plane (3 x 3); the
        observation is its second column.  strict_reference=True keeps the reference's gate (it skips only when all seven angles of
        find_angle_bw_2_vecs exceed 4 degrees, quirk Q12); False skips when the angle between z and h exceeds 4 degrees.  Returns whether the
        update was applied (synchronises)."""
        Rp = np.asfortranarray(np.asarray(R_plane, dtype=np.float64))
        if Rp.shape != (3, 3):
            raise Pre3Error(-1, "ekf_heading_update: R_plane must be 3 x 3")
        Rc = f64(Rp.ravel(order="F"))
        applied = C.c_int32(0)
        check(lib.pre3_heading_update(self._ctx, dptr(Rc), int(bool(strict_reference)), C.byref(applied)))
        return bool(applied.value)

    def heading_from_scan(self, x_sr, y_sr, z_sr, draws, box=None, t=0.02, transpose=True, strict_reference=True, wait=True):
        """mono_slam.m:189-193 in one call: R_plane = plane_fit_to_data(step) on the range image (SR4000 coordinates, draws as for plane.plane_fit),
        then ekf_heading_update(filter, R_plane') (transpose=False: R_plane itself) -- fit, gate and update queued on the filter's stream, nothing
        read back in between.  A fit whose status is not 1 applies nothing.  wait=True synchronises and returns
        (applied, fit dict as plane.plane_fit's without counts / inliers); wait=False returns None at once."""
        from . import plane
        imgs = plane._images(x_sr, y_sr, z_sr)
        draws = i32(draws).reshape(-1, 3)
        args = (self._ctx, imgs[0].shape[0], imgs[0].shape[1], dptr(imgs[0]), dptr(imgs[1]), dptr(imgs[2]), dptr(plane._box(box)), float(t),
                draws.shape[0], dptr(draws), int(bool(transpose)), int(bool(strict_reference)))
        if not wait:
            check(lib.pre3_heading_from_scan(*args, None, None))
            return None
        applied, res = C.c_int32(0), plane.PlaneResult()
        check(lib.pre3_heading_from_scan(*args, C.byref(applied), C.byref(res)))
        return bool(applied.value), plane._result(res)

    def heading_from_scan_seeded(self, x_sr, y_sr, z_sr, seed, seq=0, n_draw=1001, box=None, t=0.02, transpose=True, strict_reference=True, wait=True,
                                 return_draws=False):
        """heading_from_scan with the draws made on the device from (seed, seq) (plane.plane_fit_seeded's rule): only the box
        crosses PCIe and nothing of the scan is needed on the host.  wait=False returns None at once, without any synchronisation."""
        from . import plane
        imgs = plane._images(x_sr, y_sr, z_sr)
        args = (self._ctx, imgs[0].shape[0], imgs[0].shape[1], dptr(imgs[0]), dptr(imgs[1]), dptr(imgs[2]), dptr(plane._box(box)), float(t),
                int(n_draw), int(seed), int(seq), int(bool(transpose)), int(bool(strict_reference)))
        if not wait:
            check(lib.pre3_heading_from_scan_seeded(*args, None, None, None))
            return None
        applied, res = C.c_int32(0), plane.PlaneResult()
        draws = np.zeros((max(int(n_draw), 1), 3), np.int32) if return_draws else None
        check(lib.pre3_heading_from_scan_seeded(*args, dptr(draws), C.byref(applied), C.byref(res)))
        out = plane._result(res)
        if return_draws:
            out["draws"] = draws
        return bool(applied.value), out

    def heading_from_frame(self, frame, draws, box=None, t=0.02, transpose=True, strict_reference=True, wait=True):
        """heading_from_scan with the range image taken from a resident sr4000.SrFrame: the box is gathered from its filtered
        planes on the device behind an event on the frame's stream; only the draw table crosses PCIe.  Bit-identical to heading_from_scan fed with
        frame.planes().  A non-finite coordinate inside the box applies nothing; with wait=True it raises Pre3Error with code -5 (.result: sta = 5)."""
        from . import plane
        draws = i32(draws).reshape(-1, 3)
        args = (self._ctx, frame._h, dptr(plane._box(box)), float(t), draws.shape[0], dptr(draws), int(bool(transpose)), int(bool(strict_reference)))
        if not wait:
            check(lib.pre3_heading_from_frame(*args, None, None))
            return None
        applied, res = C.c_int32(0), plane.PlaneResult()
        plane._check_frame(lib.pre3_heading_from_frame(*args, C.byref(applied), C.byref(res)), res)
        return bool(applied.value), plane._result(res)

    def heading_from_frame_seeded(self, frame, seed, seq=0, n_draw=1001, box=None, t=0.02, transpose=True, strict_reference=True, wait=True,
                                  return_draws=False):
        """heading_from_scan_seeded with the range image taken from a resident sr4000.SrFrame: nothing crosses PCIe on the way in, and wait=False
        returns None at once -- a frame.load() that follows stays behind the gather (the frame's stream waits for it)."""
        from . import plane
        args = (self._ctx, frame._h, dptr(plane._box(box)), float(t), int(n_draw), int(seed), int(seq), int(bool(transpose)), int(bool(strict_reference)))
        if not wait:
            check(lib.pre3_heading_from_frame_seeded(*args, None, None, None))
            return None
        applied, res = C.c_int32(0), plane.PlaneResult()
        draws = np.zeros((max(int(n_draw), 1), 3), np.int32) if return_draws else None
        plane._check_frame(lib.pre3_heading_from_frame_seeded(*args, dptr(draws), C.byref(applied), C.byref(res)), res)
        out = plane._result(res)
        if return_draws:
            out["draws"] = draws
        return bool(applied.value), out

    def rows_form(self):
        """PRE3_OPT_ROWS_FORM: 1 if the last update() / ekf_heading_update() took the single-sweep form, 0 the general route"""
        v = C.c_int(0)
        check(lib.pre3_get_option(self._ctx, 9, C.byref(v)))
        return int(v.value)

    def sync(self):
        check(lib.pre3_sync(self._ctx))

    def defer_hi_update(self, on=True):
        """PRE3_OPT_DEFER_HI: step() returns once the rescue stage is enqueued; the HI update is completed by the next call.
        step()'s n_hi then belongs to the previous step."""
        check(lib.pre3_set_option(self._ctx, 1, int(bool(on))))

    def k9_bf16x3(self, on=None):
        """PRE3_OPT_K9_BF16X3 (fp32 contexts): P <- P - W'W as a three-way bf16 split on the bf16 matrix cores (default) or, off,
        on the f32 MFMA.  Returns the setting in force."""
        if on is not None:
            check(lib.pre3_set_option(self._ctx, 2, int(bool(on))))
        v = C.c_int(0)
        check(lib.pre3_get_option(self._ctx, 2, C.byref(v)))
        return bool(v.value)

    def ic_search_was_ranked(self):
        """PRE3_OPT_IC_RANKED: whether the last matching_sift_based() matched on the matrix cores"""
        v = C.c_int(0)
        check(lib.pre3_get_option(self._ctx, 4, C.byref(v)))
        return bool(v.value)

    def ic_search_route(self):
        """PRE3_OPT_IC_ROUTE: 2 fused small-problem route, 1 ranked (matrix cores), 0 exact tiled kernel"""
        v = C.c_int(0)
        check(lib.pre3_get_option(self._ctx, 7, C.byref(v)))
        return int(v.value)

    def chol_persist(self, on=None):
        """PRE3_OPT_CHOL_PERSIST (fp32 contexts): update.m:32-33 -- the factorisation of S and W = L^-1 [HP | nu] -- as one persistent launch
        (default) or, off, one launch per 64-column panel.  Returns whether the persistent form is in effect."""
        if on is not None:
            check(lib.pre3_set_option(self._ctx, 3, int(bool(on))))
        v = C.c_int(0)
        check(lib.pre3_get_option(self._ctx, 3, C.byref(v)))
        return bool(v.value)

    def k9_overlap(self, on=None):
        """PRE3_OPT_K9_OVERLAP (fp32 contexts with the persistent factorisation): update.m:37's P - K*S*K' = P - sum_J W_J'W_J accumulated panel by
        panel inside the factorisation's launch, on the CUs it leaves idle (default); off: the down-date starts when the factorisation has
        finished.  Bit-identical results.  Returns the setting in force."""
        if on is not None:
            check(lib.pre3_set_option(self._ctx, 5, int(bool(on))))
        v = C.c_int(0)
        check(lib.pre3_get_option(self._ctx, 5, C.byref(v)))
        return bool(v.value)

    def pend_hi(self, on=None):
        """PRE3_OPT_PEND_HI (fp32 contexts with the persistent factorisation, together with defer_hi_update): the HI update's down-date of P is not
        launched behind the update but taken along by the next step's launches (prediction, H*P, the LI update's consumers): P is swept once per
        step.  Results agree with the default form to fp32 rounding.  Returns the setting in force."""
        if on is not None:
            check(lib.pre3_set_option(self._ctx, 8, int(bool(on))))
        v = C.c_int(0)
        check(lib.pre3_get_option(self._ctx, 8, C.byref(v)))
        return bool(v.value)

    def step_tail(self, on=None):
        """PRE3_OPT_STEP_TAIL (fp32 contexts): rescue_hi_inliers + ekf_update_hi_inliers (up to 32 landmarks) inside the LI update's persistent
        launch, P swept once per step; off (default: measured no faster on MI355X): as launches of their own behind it.  Same inlier sets, x / P equal to fp32 rounding.
        Returns the setting in force."""
        if on is not None:
            check(lib.pre3_set_option(self._ctx, 6, int(bool(on))))
        v = C.c_int(0)
        check(lib.pre3_get_option(self._ctx, 6, C.byref(v)))
        return bool(v.value)

    # ---- map management between steps (map_management.m:27-79); the policy is the caller's (map_management_policy: the device's)
    def _refresh_map(self):
        self.N = int(lib.pre3_get_map(self._ctx, None))
        t = np.zeros(max(self.N, 1), np.int32)
        lib.pre3_get_map(self._ctx, dptr(t))
        self.lm_type = t[:self.N].copy()
        self.n = int(lib.pre3_state_size(self._ctx))
        self.m = 0
        self.meas_idx = np.zeros(0, np.int32)

    def delete_features(self, del_idx):
        """delete_features.m:54-74 -> delete_a_feature.m:47-51 (0-based landmark indices)."""
        d = i32(sorted(int(v) for v in del_idx))
        check(lib.pre3_map_delete(self._ctx, int(d.shape[0]), dptr(d)))
        self._refresh_map()

    def add_features_inverse_depth(self, uvd, std_pxl, initial_rho):
        """add_features_inverse_depth.m:27-47; uvd is (k, 2) distorted pixels, initial_rho scalar or (k,)."""
        uvd = f64(uvd).reshape(-1, 2)
        rho = f64(np.broadcast_to(initial_rho, (uvd.shape[0],)))
        check(lib.pre3_map_add_inverse_depth(self._ctx, int(uvd.shape[0]), dptr(uvd), C.c_double(std_pxl), dptr(rho)))
        self._refresh_map()

    def inversedepth_2_cartesian(self, linearity_index_threshold=0.1):
        """inversedepth_2_cartesian.m:27-76; returns the per-landmark converted flags."""
        conv = np.zeros(max(self.N, 1), np.int32)
        check(lib.pre3_map_inversedepth_2_cartesian(self._ctx, C.c_double(linearity_index_threshold), dptr(conv)))
        conv = conv[:self.N].copy()
        self._refresh_map()
        return conv

    def map_management(self, del_idx=(), new_uvd=None, std_pxl=1.0, initial_rho=0.5, linearity_index_threshold=None):
        """map_management.m:27-79 as one call (delete_features, inversedepth_2_cartesian unless the threshold is None, the new features of
        initialize_features): one pass over the covariance.  Returns the per-landmark converted flags of the map before the call."""
        d = i32(sorted(int(v) for v in del_idx))
        uvd = f64(new_uvd).reshape(-1, 2) if new_uvd is not None else np.zeros((0, 2))
        rho = f64(np.broadcast_to(initial_rho, (uvd.shape[0],)))
        conv = np.zeros(max(self.N, 1), np.int32)
        n_before = self.N
        check(lib.pre3_map_management(self._ctx, int(d.shape[0]), dptr(d), C.c_double(-1.0 if linearity_index_threshold is None else linearity_index_threshold),
                                      dptr(conv), int(uvd.shape[0]), dptr(uvd), C.c_double(std_pxl), dptr(rho)))
        self._refresh_map()
        return conv[:n_before].copy()

    # ---- the policy half of map_management.m:27-79 on the device
    def set_book(self, book, first=0):
        """features_info bookkeeping: (count, 4) int rows {times_predicted, times_measured, init_frame, last_visible} for landmarks first..."""
        b = i32(np.asarray(book).reshape(-1, 4))
        check(lib.pre3_set_book(self._ctx, int(first), int(b.shape[0]), dptr(b)))

    def book(self):
        out = np.zeros((max(self.N, 1), 4), np.int32)
        check(lib.pre3_get_book(self._ctx, 0, self.N, dptr(out)))
        return out[:self.N].copy()

    def map_management_policy(self, step, cand_uv, cand_xyz, cand_desc=None, min_features=50, linearity_index_threshold=0.1, std_pxl=None,
                              strict_reference=True):
        """map_management.m:27-79 with its policy decided on the device: deletion (delete_features.m:31-49), counters (update_features_info.m),
        inversedepth_2_cartesian (threshold None: skipped) and the initialisation walk over the candidates in the given order
        (initialize_features.m:110-142).  cand_uv (K, 2) distorted pixels, cand_xyz (K, 3) camera-frame points, cand_desc (128, K) or None.
        Returns dict(deleted, accepted, converted, measured, target, examined, N)."""
        uv = f64(np.asarray(cand_uv, float).reshape(-1, 2))
        xyz = f64(np.asarray(cand_xyz, float).reshape(-1, 3))
        K = int(uv.shape[0])
        if xyz.shape[0] != K:
            raise ValueError("cand_uv and cand_xyz disagree on K")
        desc = None
        if cand_desc is not None:
            d = np.asarray(cand_desc, dtype=np.float64)
            desc = np.ascontiguousarray(d.T) if d.ndim == 2 and d.shape[0] == 128 and d.shape[1] == K else f64(d).reshape(K, 128)
        N0 = self.N
        dl, acc, conv = np.zeros(max(N0, 1), np.int32), np.zeros(max(K, 1), np.int32), np.zeros(max(N0, 1), np.int32)
        nd, na, st = C.c_int32(0), C.c_int32(0), np.zeros(4, np.int32)
        thr = -1.0 if linearity_index_threshold is None else float(linearity_index_threshold)
        check(lib.pre3_map_policy(self._ctx, int(step), int(min_features), C.c_double(thr), C.c_double(self.std_z if std_pxl is None else std_pxl),
                                  int(bool(strict_reference)), K, dptr(uv), dptr(xyz), dptr(desc), dptr(dl), C.byref(nd), dptr(acc), C.byref(na),
                                  dptr(conv), dptr(st)))
        self._refresh_map()
        return dict(deleted=dl[:nd.value].copy(), accepted=acc[:na.value].copy(), converted=conv[:N0].copy(), measured=int(st[0]),
                    target=int(st[1]), examined=int(st[2]), N=int(st[3]))

    def map_management_policy_seeded(self, step, cand_uv, cand_xyz, seed, seq=0, cand_desc=None, box=(176, 144), min_features=50,
                                     linearity_index_threshold=0.1, std_pxl=None, strict_reference=True):
        """map_management_policy with the candidates' order -- Weighted_Smpl_wo_replacement.m, the draw initialize_a_feature_sift_3.m:42-46 makes
        -- drawn on the device from (seed, seq) (synth.candidate_order's rule).  The candidates are given in any order;
        box = (BoxLimX(2), BoxLimY(2)).  Returns map_management_policy's dict plus order (K,): order[p] = the candidate at drawn position p;
        accepted holds indices into the arrays as given."""
        uv = f64(np.asarray(cand_uv, float).reshape(-1, 2))
        xyz = f64(np.asarray(cand_xyz, float).reshape(-1, 3))
        K = int(uv.shape[0])
        if xyz.shape[0] != K:
            raise ValueError("cand_uv and cand_xyz disagree on K")
        desc = None
        if cand_desc is not None:
            d = np.asarray(cand_desc, dtype=np.float64)
            desc = np.ascontiguousarray(d.T) if d.ndim == 2 and d.shape[0] == 128 and d.shape[1] == K else f64(d).reshape(K, 128)
        N0 = self.N
        dl, acc, conv = np.zeros(max(N0, 1), np.int32), np.zeros(max(K, 1), np.int32), np.zeros(max(N0, 1), np.int32)
        order = np.zeros(max(K, 1), np.int32)
        nd, na, st = C.c_int32(0), C.c_int32(0), np.zeros(4, np.int32)
        thr = -1.0 if linearity_index_threshold is None else float(linearity_index_threshold)
        check(lib.pre3_map_policy_seeded(self._ctx, int(step), int(min_features), thr, float(self.std_z if std_pxl is None else std_pxl),
                                         int(bool(strict_reference)), K, dptr(uv), dptr(xyz), dptr(desc), int(box[0]), int(box[1]), int(seed), int(seq),
                                         dptr(order), dptr(dl), C.byref(nd), dptr(acc), C.byref(na), dptr(conv), dptr(st)))
        self._refresh_map()
        return dict(deleted=dl[:nd.value].copy(), accepted=acc[:na.value].copy(), converted=conv[:N0].copy(), measured=int(st[0]),
                    target=int(st[1]), examined=int(st[2]), N=int(st[3]), order=order[:K].copy())

    def map_management_policy_frames_seeded(self, step, prev, cur, seed, seq=0, thresh=1.5, box=(176, 144), min_features=50,
                                            linearity_index_threshold=0.1, std_pxl=None, strict_reference=True):
        """map_management_policy_seeded with the candidates built on the device from two resident frames (sr4000.SrFrame; initialize_features.m:95-99,
        DESIGN.md section 22): matches = siftmatch(prev's kept descriptors, cur's kept descriptors, thresh), candidate c is prev's kept keypoint
        match[0, c] - 1 with its pixel, its rho (prev's last keypoints() call must have been gate 0) and its descriptor.  Returns
        map_management_policy_seeded's dict plus match (2, K), 1-based positions in the kept sets, and K; accepted holds candidate indices c."""
        n1 = max(int(prev.n_kept), 1)
        N0 = self.N
        dl, acc, conv = np.zeros(max(N0, 1), np.int32), np.zeros(n1, np.int32), np.zeros(max(N0, 1), np.int32)
        order, match = np.zeros(n1, np.int32), np.zeros((2, n1), order="F")
        K, nd, na, st = C.c_int32(0), C.c_int32(0), C.c_int32(0), np.zeros(4, np.int32)
        thr = -1.0 if linearity_index_threshold is None else float(linearity_index_threshold)
        check(lib.pre3_map_policy_frames_seeded(self._ctx, prev._h, cur._h, float(thresh), int(step), int(min_features), thr,
                                                float(self.std_z if std_pxl is None else std_pxl), int(bool(strict_reference)), int(box[0]), int(box[1]),
                                                int(seed), int(seq), C.byref(K), dptr(match), dptr(order), dptr(dl), C.byref(nd), dptr(acc), C.byref(na),
                                                dptr(conv), dptr(st)))
        self._refresh_map()
        K = K.value
        return dict(deleted=dl[:nd.value].copy(), accepted=acc[:na.value].copy(), converted=conv[:N0].copy(), measured=int(st[0]),
                    target=int(st[1]), examined=int(st[2]), N=int(st[3]), order=order[:K].copy(), match=match[:, :K].copy(order="F"), K=K)

    # ---- IC search on the device (search_IC_matches.m:31-44 + matching_sift_based.m:104-149)
    def set_descriptors(self, desc, first=0):
        """features_info(first+i).Descriptor; desc is (128, count) as MATLAB stores it (or (count, 128) C-order rows)."""
        desc = np.asarray(desc, dtype=np.float64)
        cols = np.ascontiguousarray(desc.T) if desc.shape[0] == 128 and desc.ndim == 2 else f64(desc)
        assert cols.ndim == 2 and cols.shape[1] == 128, "descriptors are 128-vectors"
        check(lib.pre3_set_descriptors(self._ctx, int(first), int(cols.shape[0]), dptr(cols)))

    def get_descriptors(self):
        out = np.zeros((max(self.N, 1), 128))
        check(lib.pre3_get_descriptors(self._ctx, 0, self.N, dptr(out)))
        return out[:self.N].T.copy()                     # (128, N) like [features_info.Descriptor]

    def load_scan(self, Descriptor_RAW, SCALE_ORIENT_POS_RAW):
        """SCAN_SIFT.Descriptor_RAW (128 x K2) and SCAN_SIFT.SCALE_ORIENT_POS_RAW (4 x K2) of SIFT_result%04d.mat."""
        d = np.ascontiguousarray(np.asarray(Descriptor_RAW, dtype=np.float64).reshape(128, -1).T)
        p = np.ascontiguousarray(np.asarray(SCALE_ORIENT_POS_RAW, dtype=np.float64).reshape(4, -1).T)
        assert d.shape[0] == p.shape[0], "Descriptor_RAW and SCALE_ORIENT_POS_RAW disagree on K2"
        check(lib.pre3_set_scan(self._ctx, int(d.shape[0]), dptr(d), dptr(p)))

    def set_scan_frame(self, frame, which=0):
        """load_scan from a resident sr4000.SrFrame: which=0 the raw set handed to its last keypoints() call (Descriptor_RAW /
        SCALE_ORIENT_POS_RAW, what matching_sift_based.m reads), which=1 the set that call kept.  One copy on the device, no wait."""
        check(lib.pre3_set_scan_frame(self._ctx, frame._h, int(which)))

    def matching_sift_based(self, thresh=1.5, strict_reference=True):
        """The whole IC-search stage in one call; the accepted matches become the measurement list."""
        N = max(self.N, 1)
        nm, m = C.c_int32(0), C.c_int32(0)
        meas, z, pairs = np.zeros(N, np.int32), np.zeros((N, 2)), np.zeros((N, 3), np.int32)
        check(lib.pre3_ic_search(self._ctx, C.c_double(thresh), int(bool(strict_reference)), C.byref(nm), C.byref(m), dptr(meas), dptr(z), dptr(pairs)))
        self.m = int(m.value)
        self.meas_idx = meas[:self.m].copy()
        return dict(meas_idx=meas[:self.m].copy(), z=z[:self.m].copy(), match_idx=pairs[:nm.value, :2].T.copy(),
                    accepted=pairs[:nm.value, 2].copy())

    # ---- the patch branch of the IC search (search_IC_matches.m:45-51: predict_features_appearance.m + matching.m)
    PATCH_STATUS = ("not_predicted", "no_patch", "zero_patch", "warp_outside", "no_candidate", "below_threshold", "matched", "warped")

    def set_image(self, im):
        """The frame the patch search reads: (nRows, nCols) uint8, the camera's shape.  Copied before the call returns, no wait."""
        im = np.asarray(im)
        assert im.ndim == 2 and im.dtype == np.uint8, "the image is a 2-D uint8 array"
        imf = np.asfortranarray(im)                       # column-major, as MATLAB stores it
        check(lib.pre3_set_image(self._ctx, int(im.shape[0]), int(im.shape[1]), imf.ctypes.data_as(C.c_void_p)))

    def get_image(self, shape):
        out = np.zeros(shape, np.uint8, order="F")
        check(lib.pre3_get_image(self._ctx, int(shape[0]), int(shape[1]), out.ctypes.data_as(C.c_void_p)))
        return out

    def set_image_frame(self, frame):
        """set_image from a resident sr4000.SrFrame's filtered image plane: converted on the device, nothing read back, no wait."""
        check(lib.pre3_set_image_frame(self._ctx, frame._h))

    def set_patches(self, patch, uv_init, r_wc, R_wc, first=0):
        """features_info(first+i).patch_when_initialized (count, 41, 41) uint8 indexed [i, row, column], uv_when_initialized (count, 2),
        r_wc_when_initialized (count, 3), R_wc_when_initialized (count, 3, 3).  The bank follows the map like the descriptor bank."""
        patch = np.asarray(patch)
        assert patch.dtype == np.uint8 and patch.ndim == 3 and patch.shape[1:] == (41, 41), "patches are (count, 41, 41) uint8"
        k = int(patch.shape[0])
        pb = np.ascontiguousarray(patch.transpose(0, 2, 1))            # each patch column-major
        uv, r = f64(np.asarray(uv_init, dtype=np.float64).reshape(k, 2)), f64(np.asarray(r_wc, dtype=np.float64).reshape(k, 3))
        R = np.ascontiguousarray(np.asarray(R_wc, dtype=np.float64).reshape(k, 3, 3).transpose(0, 2, 1))
        check(lib.pre3_set_patches(self._ctx, int(first), k, pb.ctypes.data_as(C.c_void_p), dptr(uv), dptr(r), dptr(R)))

    def patches(self, first=0, count=None):
        """The bank as dict(patch (count, 41, 41) uint8, uv_init, r_wc, R_wc (count, 3, 3), has_patch (count,) bool)."""
        count = self.N - int(first) if count is None else int(count)
        k = max(count, 1)
        pb, uv, r, R, has = np.zeros((k, 41, 41), np.uint8), np.zeros((k, 2)), np.zeros((k, 3)), np.zeros((k, 3, 3)), np.zeros(k, np.int32)
        check(lib.pre3_get_patches(self._ctx, int(first), count, pb.ctypes.data_as(C.c_void_p), dptr(uv), dptr(r), dptr(R), dptr(has)))
        return dict(patch=pb[:count].transpose(0, 2, 1).copy(), uv_init=uv[:count].copy(), r_wc=r[:count].copy(),
                    R_wc=R[:count].transpose(0, 2, 1).copy(), has_patch=has[:count].astype(bool))

    def patch_cut(self, uv, first=0):
        """add_feature_to_info_vector_my_version.m:33-41 on the device: 41 x 41 around the integer pixels uv (count, 2) = (column, row), 1-based,
        out of the resident image; r_wc and q2r(q) from the resident x_k_k."""
        uv = i32(np.asarray(uv).reshape(-1, 2))
        check(lib.pre3_patch_cut(self._ctx, int(first), int(uv.shape[0]), dptr(uv)))

    def predict_features_appearance(self, focal_over_d):
        """predict_features_appearance.m behind a projection at x_k_km1: (patches (N, 13, 13) indexed [i, row, column], status (N,))."""
        k = max(self.N, 1)
        out, st = np.zeros((k, 13, 13)), np.zeros(k, np.int32)
        check(lib.pre3_predict_patches(self._ctx, float(focal_over_d), dptr(out), dptr(st)))
        return out[:self.N].transpose(0, 2, 1).copy(), st[:self.N].copy()

    def search_ic_matches_patch(self, focal_over_d, corr_threshold=0.60, strict_reference=True):
        """search_IC_matches.m:31-51 on the patch branch in one call; the accepted landmarks become the measurement list.
        Returns meas_idx, z (m, 2), corr (N,), ncand (N,), status (N,: indices into PATCH_STATUS)."""
        k = max(self.N, 1)
        m = C.c_int32(0)
        meas, z, corr, ncand, st = np.zeros(k, np.int32), np.zeros((k, 2)), np.zeros(k), np.zeros(k, np.int32), np.zeros(k, np.int32)
        check(lib.pre3_patch_search(self._ctx, float(focal_over_d), float(corr_threshold), int(bool(strict_reference)), C.byref(m), dptr(meas), dptr(z),
                                    dptr(corr), dptr(ncand), dptr(st)))
        self.m = int(m.value)
        self.meas_idx = meas[:self.m].copy()
        return meas[:self.m].copy(), z[:self.m].copy(), corr[:self.N].copy(), ncand[:self.N].copy(), st[:self.N].copy()

    def patch_timing(self):
        """(k_patch_warp ms, k_patch_search ms) of the last search_ic_matches_patch under kernel timing."""
        a, b = C.c_double(0), C.c_double(0)
        check(lib.pre3_patch_timing(self._ctx, C.byref(a), C.byref(b)))
        return a.value, b.value

    # ---- FAST-9 corners on the resident image (fast_corner_detect_9.m, fast_nonmax.m; DESIGN.md section 30: the published segment test, not the
    # reference's learned tree)
    def _fast_detect(self, threshold, barrier, nonmax, box):
        if box is None:
            box = (0, 0) + tuple(self._image_shape)
        r0, c0, rows, cols = (int(v) for v in box)
        K = C.c_int32(0)
        uv, score = np.zeros((_lib.FAST_MAX_CORNERS, 2), np.int32), np.zeros(_lib.FAST_MAX_CORNERS, np.int32)
        check(lib.pre3_fast_detect(self._ctx, r0, c0, rows, cols, int(threshold), int(barrier), int(nonmax), C.byref(K), dptr(uv), dptr(score)))
        return uv[:K.value].copy(), score[:K.value].copy()

    def fast_corner_detect_9(self, threshold, box=None, barrier=None):
        """fast_corner_detect_9(im, threshold) on the resident image, or on box = (r0, c0, rows, cols) (0-based) of it taken as an image of its own:
        (K, 2) int32 corners (x, y) = (column, row), 1-based and relative to the box, x outer / y inner.  With a barrier: (corners, scores)."""
        uv, score = self._fast_detect(threshold, 0 if barrier is None else barrier, 0, box)
        return uv if barrier is None else (uv, score)

    def fast_nonmax(self, threshold, barrier, box=None):
        """fast_nonmax(im, barrier, fast_corner_detect_9(im, threshold)): (maxima (K, 2) int32, scores (K,) int32)."""
        return self._fast_detect(threshold, barrier, 1, box)

    FAST_STATUS = ("initialised", "no_box", "no_depth_nan", "no_depth_near", "no_depth_conf")

    def _fast_init_result(self, res):
        ok = res.status == 0
        if ok:
            self._refresh_map()
        tried = np.array(res.centres[:], np.int32).reshape(-1, 2)[:res.attempts].copy()
        found = res.status != 1
        return dict(status=int(res.status), attempts=int(res.attempts), uv=np.array(res.uv[:], np.int32) if found else None,
                    rho=float(res.rho) if ok else None, xyz=np.array(res.xyz[:]) if ok else None, landmark=int(res.landmark) if ok else None, centres=tried)

    def initialize_a_feature(self, frame, std_pxl, centres, strict_reference=True, threshold=10, barrier=20):
        """initialize_a_feature.m:27-215 on the FAST branch, one call and one wait (pre3_init_feature_fast): up to 10 attempts over the box centres
        `centres` (attempts, 2) = (row, column), 1-based; depth from the resident sr4000.SrFrame `frame`.  On status 0 ("initialised") the map has the
        new inverse-depth landmark (rho = 1 / df) and the bank its 41 x 41 patch, as after add_features_inverse_depth(uv, std_pxl, rho) and
        patch_cut(uv, first=N).  Returns dict(status (index into FAST_STATUS), attempts, uv (column, row), rho, xyz, landmark, centres tried)."""
        ce = i32(np.asarray(centres).reshape(-1, 2))
        res = _lib.FastInitResult()
        check(lib.pre3_init_feature_fast(self._ctx, frame._h, float(std_pxl), int(bool(strict_reference)), int(threshold), int(barrier), dptr(ce), int(ce.shape[0]),
                                         C.byref(res)))
        return self._fast_init_result(res)

    def initialize_a_feature_seeded(self, frame, std_pxl, seed, seq, strict_reference=True, threshold=10, barrier=20):
        """initialize_a_feature with its rand(2, 1) per attempt (:64) drawn on the device: Philox key [seed, 5], counter [attempt, 0, seq, 0]."""
        res = _lib.FastInitResult()
        check(lib.pre3_init_feature_fast_seeded(self._ctx, frame._h, float(std_pxl), int(bool(strict_reference)), int(threshold), int(barrier), int(seed), int(seq),
                                                C.byref(res)))
        return self._fast_init_result(res)

    def initialize_n_features_fast(self, frame, std_pxl, threshold=5, barrier=20):
        """initialize_n_features_FAST.m:55-145 (pre3_init_features_fast_all): every maximum of the image inside the 20-pixel band through the depth
        gate, the survivors added in scan order in one map call with one patch cut.  Returns dict(uv (K, 2) of all maxima, rho (K,), verdict (K,:
        0 = added, else an index into FAST_STATUS), n_added)."""
        K, n = C.c_int32(0), C.c_int32(0)
        uv, rho, ver = np.zeros((_lib.FAST_MAX_CORNERS, 2), np.int32), np.zeros(_lib.FAST_MAX_CORNERS), np.zeros(_lib.FAST_MAX_CORNERS, np.int32)
        check(lib.pre3_init_features_fast_all(self._ctx, frame._h, float(std_pxl), int(threshold), int(barrier), C.byref(K), C.byref(n), dptr(uv), dptr(rho), dptr(ver)))
        if n.value:
            self._refresh_map()
        return dict(uv=uv[:K.value].copy(), rho=rho[:K.value].copy(), verdict=ver[:K.value].copy(), n_added=int(n.value))

    def initialize_features_fast(self, frame, n, std_pxl, seed, seq0=0, max_calls=50, **kw):
        """initialize_features.m:110-142: initialize_a_feature until n features are in or max_calls calls are spent -- the bound the reference declares
        (max_attempts = 50, :106) and never applies.  Each new feature changes the next call's "is the box free" test, so this is a host loop with one
        wait per call; call k draws from (seed, seq0 + k).  A depth refusal counts as a spent call.  Returns the list of the calls' results."""
        out, added = [], 0
        for k in range(int(max_calls)):
            if added >= int(n):
                break
            r = self.initialize_a_feature_seeded(frame, std_pxl, seed, int(seq0) + k, **kw)
            added += r["status"] == 0
            out.append(r)
        return out

    def fast_timing(self):
        """ms of the launches of the last detector / initialisation call under kernel timing."""
        a = C.c_double(0)
        check(lib.pre3_fast_timing(self._ctx, C.byref(a)))
        return a.value

    # ---- step stages
    def ekf_prediction(self, u):
        u = f64(u)
        assert u.shape == (7,), "u = [dX(3); dq(4)]"
        check(lib.pre3_predict(self._ctx, dptr(u)))

    CV_TYPES = ("constant_velocity", "constant_orientation", "constant_position", "constant_position_and_orientation")

    def ekf_prediction_cv(self, dt, sigma_a, sigma_alpha, type="constant_velocity"):
        """predict_state_and_covariance.m with the camera-only models the fork switched off: no u -- the prediction comes from the
        v and omega the state carries.  State functions fv.m:64-87 / :98-106, F = dfv_by_dxv.m:38-116, Q = func_Q.m:41-54 with the acceleration noise
        (sigma_a dt)^2, (sigma_alpha dt)^2 (predict_state_and_covariance.m:89-90); dt is the reference's delta_t (:35: 0.1).  type: one of CV_TYPES (or
        its index); constant_position_and_orientation_location_noise is not built.  At omega = 0 exactly -- what ekf_prediction and the steps leave in
        x[10:13] -- dqomegadt_by_domega takes its limit where the reference has 0/0.  One launch, in place, nothing waited for."""
        t = self.CV_TYPES.index(type) if isinstance(type, str) and type in self.CV_TYPES else type
        if isinstance(t, str):
            raise Pre3Error(-1, "ekf_prediction_cv: type %r is not one of %s" % (type, ", ".join(self.CV_TYPES)))
        check(lib.pre3_predict_cv(self._ctx, int(t), float(dt), float(sigma_a), float(sigma_alpha)))

    def ekf_prediction_pair_seeded(self, prev, cur, seed, seq=0, thresh=1.5, wait=True):
        """fv.m:47 + predict_state_and_covariance.m in one call: vo.vo_pair_seeded between the keypoint records of the resident
        frames prev and cur (sr4000.SrFrame after keypoints()), then ekf_prediction with that pair's u = [T; R2q(R)] -- the identity motion unless
        sta == 1 -- read on the device: u never crosses PCIe.  Bit-identical to vo.vo_pair_seeded(prev, cur, seed, seq, thresh) followed by
        ekf_prediction(res["u"]).  wait=True: one host wait; returns dict(pnum, rst, sta, u, rot, trans, euler, n_support, n_iterations, best,
        error_mean, error_std, dist) as vo.vo_pair_seeded reports them.  wait=False: returns None at once, nothing is synchronised; a pair that
        vo_pair_seeded would refuse (no matched point beyond 0.4 m) is predicted with the identity motion and the next call that reads the device's
        error words raises Pre3Error with code -5 once."""
        from . import vo
        args = (self._ctx, prev._h, cur._h, float(thresh), int(seed), int(seq))
        if not wait:
            check(lib.pre3_predict_pair_seeded(*args, None, None))
            return None
        pnum, res = C.c_int32(0), vo.VoResult()
        check(lib.pre3_predict_pair_seeded(*args, C.byref(pnum), C.byref(res)))
        pnum = int(pnum.value)
        out = vo._result(res, None, None, None)
        for k in ("cnum", "state", "inliers"):             # the per-hypothesis tables stay on the device
            del out[k]
        out["pnum"], out["rst"] = pnum, (vo.vo_rst(pnum) if pnum >= 4 else 0)
        return out

    def ekf_prediction_pair_cov_seeded(self, prev, cur, seed, seq=0, thresh=1.5, wait=True):
        """ekf_prediction_pair_seeded with the pair's own covariance as this one prediction's process noise (predict_state_and_covariance.m:115,
        DESIGN.md section 27): vo.vo_pair_cov_seeded's extra launch behind the final fit, and the prediction takes that 7 x 7 block as Pn when its
        status is 1 and the pair's u is taken (sta == 1) -- else this filter's own noise (set_process_noise, or the constant).  u and Pn stay on the
        device; the filter's noise setting is unchanged afterwards.  wait=True: one host wait; the dict of ekf_prediction_pair_seeded plus cov_status
        and cov ((7, 7) on status 1, else None).  wait=False: returns None at once."""
        from . import vo
        args = (self._ctx, prev._h, cur._h, float(thresh), int(seed), int(seq))
        if not wait:
            check(lib.pre3_predict_pair_cov_seeded(*args, None, None, None, None))
            return None
        pnum, res, cov, status = C.c_int32(0), vo.VoResult(), np.zeros((7, 7)), C.c_int32(0)
        check(lib.pre3_predict_pair_cov_seeded(*args, C.byref(pnum), C.byref(res), dptr(cov), C.byref(status)))
        pnum = int(pnum.value)
        out = vo._result(res, None, None, None)
        for k in ("cnum", "state", "inliers"):
            del out[k]
        out["pnum"], out["rst"] = pnum, (vo.vo_rst(pnum) if pnum >= 4 else 0)
        out["cov_status"] = int(status.value)
        out["cov"] = cov if out["cov_status"] == 1 else None
        return out

    def ekf_prediction_icp_pair_seeded(self, prev, cur, seed, seq=0, thresh=1.5, stride=1, res=0.02, max_error=float("inf"), noise=0, wait=True):
        """ekf_prediction_pair_seeded with the dense ICP between the pair and the prediction: vo.icp_pair_cov_seeded's launches,
        then the prediction with u and Pn taken on the device.  u: the ICP's when the pair's is taken (sta == 1), the ICP ended with sta == 1, its u is
        finite and its error <= max_error; else the pair's; the identity when the pair is not taken.  noise: 0 this filter's own (set_process_noise, or
        the constant), 1 the pair's covariance as ekf_prediction_pair_cov_seeded takes it, 2 the ICP's closed-form covariance when the ICP's u is taken
        and its status is 1 (else as 1), 3 as 2 with this filter's own noise added to it entry by entry.  Mode 2 is optimistic -- it propagates sensor
        noise only --, mode 3 lets set_process_noise act as a floor.  The filter's noise setting is unchanged afterwards.
        wait=True: one host wait; the dict of ekf_prediction_pair_seeded plus cov_status / cov (the pair's), icp (dict(sta=0) when it did not run, else
        R, t, Rtot, ttot, u, error, sta, p, iters1, iters2, n_model, n_source, cov_status, cov) and taken = (which u: 0 identity, 1 pair, 2 ICP; which
        noise: 0 .. 3).  wait=False: returns None at once, nothing is synchronised."""
        from . import vo
        args = (self._ctx, prev._h, cur._h, float(thresh), int(seed), int(seq), int(stride), float(res), float(max_error), int(noise))
        if not wait:
            check(lib.pre3_predict_icp_pair_seeded(*args, None, None, None, None, None, None))
            return None
        pnum, res_, r = C.c_int32(0), vo.VoResult(), vo.IcpResult()
        cov, status, taken = np.zeros((2, 7, 7)), np.zeros(2, np.int32), np.zeros(2, np.int32)
        check(lib.pre3_predict_icp_pair_seeded(*args, C.byref(pnum), C.byref(res_), C.byref(r), dptr(cov), dptr(status), dptr(taken)))
        pnum = int(pnum.value)
        out = vo._result(res_, None, None, None)
        for k in ("cnum", "state", "inliers"):
            del out[k]
        out["pnum"], out["rst"] = pnum, (vo.vo_rst(pnum) if pnum >= 4 else 0)
        out["cov_status"] = int(status[0])
        out["cov"] = cov[0].copy() if out["cov_status"] == 1 else None
        if int(r.sta) == 0:
            icp = dict(sta=0)
        else:
            icp = dict(R=np.array(r.R).reshape(3, 3), t=np.array(r.t), Rtot=np.array(r.Rtot).reshape(3, 3), ttot=np.array(r.ttot), u=np.array(r.u),
                       error=float(r.error), sta=int(r.sta), p=int(r.p), iters1=int(r.iters1), iters2=int(r.iters2), n_model=int(r.n_model),
                       n_source=int(r.n_source))
        icp["cov_status"] = int(status[1])
        icp["cov"] = cov[1].copy() if icp["cov_status"] == 1 else None
        out["icp"], out["taken"] = icp, (int(taken[0]), int(taken[1]))
        return out

    RELOC_PN = np.diag([0.05 ** 2] * 3 + [0.02 ** 2] * 4)      # relocalise_seeded's default noise: 5 cm and 0.02 per quaternion entry, one sigma

    def relocalise_seeded(self, seed, seq=0, thresh=1.5, n_hyp=200, thr_px=2.0, undistort=True, min_support=12, Pn=None, wait=True):
        """Relocalise a lost filter (the project's own, the reference has none): replaces ekf_prediction on the frame on which the
        caller has judged the filter lost.  siftmatch of the whole map's descriptors against the loaded scan with no window gate, the camera pose by a
        seeded EPnP RANSAC (vo.pnp_ransac_seeded's launches) from the matched landmarks' 3-D points at x_k_k and the scan's pixels, then the prediction
        onto that pose with the wide noise Pn ((7, 7) over [dX; dq]; default RELOC_PN), so that P stays a consistent covariance; matching_sift_based and
        step* follow as after any prediction.  The pose is taken iff the refit ended with sta == 1 over at least min_support inliers; otherwise the
        identity motion is predicted under this filter's own noise.  Everything stays on the device; the filter's noise setting is unchanged.
        wait=True: one host wait; returns dict(pnp (vo.efficient_pnp's result dict of the refit), u (the increment applied), n_matches, n_corr, winner
        (-1: no hypothesis ran), taken, match_idx (2, n_matches) 0-based (k1, k2), inliers (n_corr,) 0/1 flags of the winner over the correspondences).
        wait=False: returns None at once, nothing is synchronised.  Pre3Error -4: no descriptors, no scan, or the covariance buffer holds the
        prediction; -1: fewer than 6 landmarks, n_hyp outside 1 .. 700, thresh or thr_px not positive and finite, min_support < 6, a bad Pn."""
        from . import vo
        Pn = f64(self.RELOC_PN if Pn is None else Pn)
        assert Pn.shape == (7, 7), "Pn is 7 x 7 over [dX(3); dq(4)]"
        args = (self._ctx, float(thresh), int(n_hyp), int(seed), int(seq), float(thr_px), int(bool(undistort)), int(min_support), dptr(Pn))
        if not wait:
            check(lib.pre3_relocalise_seeded(*args, None, None, None))
            return None
        N = max(self.N, 1)
        res, pairs, inl = vo.RelocResult(), np.zeros((N, 2), np.int32), np.zeros(N, np.int32)
        check(lib.pre3_relocalise_seeded(*args, C.byref(res), dptr(pairs), dptr(inl)))
        nm, nc = int(res.n_matches), int(res.n_corr)
        return dict(pnp=vo._pnp_dict(res.pnp), u=np.array(res.u), n_matches=nm, n_corr=nc, winner=int(res.winner), taken=int(res.taken),
                    match_idx=pairs[:nm].T.copy(), inliers=inl[:nc].copy())

    RELOC_NOISE = {"caller": 0, "pose": 1, "pose_floor": 2}

    def relocalise_refined_seeded(self, seed, seq=0, thresh=1.5, n_hyp=200, thr_px=2.0, undistort=True, min_support=12, n_iter=5, sigma_px=0.0, noise="pose",
                                  Pn=None, wait=True):
        """relocalise_seeded with the pose refined by Gauss-Newton on the reprojection error between the refit and the prediction (DESIGN.md section 37;
        vo.pnp_refine over the winner's inliers, n_iter steps), and the prediction's noise from the refined pose's own covariance.  Whether the pose is
        taken is relocalise_seeded's rule on the EPnP refit; u comes from the refinement when it took its pose (ref.sta == 1), else from the refit.
        noise: "caller" -- Pn, as relocalise_seeded; "pose" -- the refinement's covariance carried to the increment (Pn where the refinement left none);
        "pose_floor" -- the same plus Pn entry by entry.  The covariance treats the map points as exact (pixel noise only: sigma_px, or the a-posteriori
        estimate when 0) and is optimistic on a real map: "pose_floor" is the form to use there.
        wait=True: relocalise_seeded's dict plus ref (vo.pnp_refine's dict), Pn (7, 7) the noise the prediction used and noise_taken ("caller", "pose",
        "pose_floor", or "own": the pose not taken).  wait=False: None at once.  Pre3Error as relocalise_seeded, and -1 for n_iter outside 0 .. 10, a
        negative or non-finite sigma_px."""
        from . import vo
        Pn = f64(self.RELOC_PN if Pn is None else Pn)
        assert Pn.shape == (7, 7), "Pn is 7 x 7 over [dX(3); dq(4)]"
        mode = self.RELOC_NOISE[noise] if isinstance(noise, str) else int(noise)
        args = (self._ctx, float(thresh), int(n_hyp), int(seed), int(seq), float(thr_px), int(bool(undistort)), int(min_support), int(n_iter), float(sigma_px),
                mode, dptr(Pn))
        if not wait:
            check(lib.pre3_relocalise_refined_seeded(*args, None, None, None))
            return None
        N = max(self.N, 1)
        res, pairs, inl = vo.RelocRefinedResult(), np.zeros((N, 2), np.int32), np.zeros(N, np.int32)
        check(lib.pre3_relocalise_refined_seeded(*args, C.byref(res), dptr(pairs), dptr(inl)))
        b = res.base
        nm, nc = int(b.n_matches), int(b.n_corr)
        names = {v: k for k, v in self.RELOC_NOISE.items()}
        return dict(pnp=vo._pnp_dict(b.pnp), u=np.array(b.u), n_matches=nm, n_corr=nc, winner=int(b.winner), taken=int(b.taken),
                    match_idx=pairs[:nm].T.copy(), inliers=inl[:nc].copy(), ref=vo._pnp_refine_dict(res.ref), Pn=np.array(res.Pn).reshape(7, 7),
                    noise_taken=names.get(int(res.noise_taken), "own"))

    def set_process_noise(self, Pn=None):
        """predict_state_and_covariance.m:98-102: the 7 x 7 process noise Pn of every prediction this filter makes from now on (ekf_prediction, step*,
        ekf_prediction_pair_seeded); None returns to the reference's constant.  Must be finite, exactly symmetric and without a negative diagonal
        entry (Pre3Error -1, nothing changed).  set_x_p_k_k does not reset it."""
        if Pn is None:
            check(lib.pre3_set_process_noise(self._ctx, None))
            return
        Pn = f64(Pn)
        assert Pn.shape == (7, 7), "Pn is 7 x 7 over [dX(3); dq(4)]"
        check(lib.pre3_set_process_noise(self._ctx, dptr(Pn)))

    @property
    def process_noise(self):
        """(Pn (7, 7), source): the process noise in force and where it comes from -- "constant" (predict_state_and_covariance.m:98-102) or "caller" (set_process_noise)"""
        Pn, src = np.zeros((7, 7)), C.c_int(0)
        check(lib.pre3_get_process_noise(self._ctx, dptr(Pn), C.byref(src)))
        return Pn, ("caller" if src.value else "constant")

    def predict_camera_measurements(self, which=_lib.X_K_KM1, clear_first=True):
        """Also computes the Jacobians (calculate_derivatives.m) -- the reference always calls them as a pair."""
        check(lib.pre3_project(self._ctx, int(which), int(bool(clear_first))))

    def search_IC_matches(self):
        check(lib.pre3_project(self._ctx, _lib.X_K_KM1, 1))
        check(lib.pre3_innovation(self._ctx))

    def landmark_fields(self):
        N = self.N
        h, has_h = np.zeros((N, 2)), np.zeros(N, np.int32)
        Hc, Hl, S = np.zeros((N, 2, 7)), np.zeros((N, 2, 6)), np.zeros((N, 2, 2))
        check(lib.pre3_get_landmark_fields(self._ctx, dptr(h), dptr(has_h), dptr(Hc), dptr(Hl), dptr(S)))
        return dict(h=h, has_h=has_h, Hc=Hc, Hl=Hl, S=S)

    def matching(self, k1, zc, strict_reference=True):
        """Window gate on siftmatch's pairs: k1[c] = 0-based column of L1 (= c-th predicted landmark list entry
        matched), zc[c] = matched pixel.  Returns the accept flags; accepted candidates become measurements."""
        k1, zc = i32(k1), f64(zc)
        M = int(k1.shape[0])
        acc = np.zeros(M, np.int32)
        check(lib.pre3_window_gate(self._ctx, M, dptr(k1), dptr(zc), int(bool(strict_reference)), dptr(acc)))
        return acc

    def set_measurements(self, meas_idx, z):
        meas_idx, z = i32(meas_idx), f64(z)
        self.m = int(meas_idx.shape[0])
        self.meas_idx = meas_idx
        check(lib.pre3_set_measurements(self._ctx, self.m, dptr(meas_idx), dptr(z)))

    def ransac_hypotheses(self, hyp, threshold=None, early_exit=True):
        hyp = i32(hyp)
        n_draw, k = hyp.shape
        sup = np.zeros(n_draw, np.int32)
        li = np.zeros(max(self.m, 1), np.int32)
        st = np.zeros(4, np.int32)
        thr = self.std_z if threshold is None else float(threshold)     # ransac_hypotheses.m:33
        check(lib.pre3_ransac(self._ctx, n_draw, k, dptr(hyp), C.c_double(thr), int(bool(early_exit)), dptr(sup), dptr(li), dptr(st)))
        return dict(support=sup, li_mask=li[:self.m], best=int(st[0]), iters=int(st[1]), n_hyp=int(st[2]), max_support=int(st[3]))

    def ransac_hypotheses_seeded(self, seed, seq, n_draw, threshold=None, early_exit=True, return_hyp=True):
        """ransac_hypotheses with the table drawn on the device from (seed, seq) (select_random_match.m:40-51 on the library's counter-based
        stream); the dict also carries the table, `hyp` (n_draw, k), unless return_hyp=False."""
        n_draw = int(n_draw)
        sup, li, st = np.zeros(max(n_draw, 1), np.int32), np.zeros(max(self.m, 1), np.int32), np.zeros(4, np.int32)
        hyp, k = (np.zeros(max(n_draw, 1) * 3, np.int32) if return_hyp else None), C.c_int32(0)
        thr = self.std_z if threshold is None else float(threshold)
        check(lib.pre3_ransac_seeded(self._ctx, int(seed), int(seq), n_draw, thr, int(bool(early_exit)), dptr(hyp), C.byref(k), dptr(sup), dptr(li), dptr(st)))
        out = dict(support=sup[:n_draw], li_mask=li[:self.m], best=int(st[0]), iters=int(st[1]), n_hyp=int(st[2]), max_support=int(st[3]), k=int(k.value))
        if return_hyp:
            out["hyp"] = hyp[:n_draw * k.value].reshape(n_draw, k.value).copy()
        return out

    def ransac_score_shard(self, hyp, threshold, hyp_begin, hyp_end):
        """Score hypotheses [hyp_begin, hyp_end) only; returns (support_dev_ptr, mask_dev_ptr, mask_words)."""
        hyp = i32(hyp)
        n_draw, k = hyp.shape
        sp, mp, mw = C.c_void_p(), C.c_void_p(), C.c_int(0)
        check(lib.pre3_ransac_score(self._ctx, n_draw, k, dptr(hyp), C.c_double(float(threshold)), int(hyp_begin), int(hyp_end),
                                    C.byref(sp), C.byref(mp), C.byref(mw)))
        return sp.value, mp.value, mw.value

    def ransac_select(self, n_draw, k, early_exit=True, fetch=True):
        """fetch=False: only the four statistics come back (through the mailbox: no stream sync, no D2H of the supports / the mask); the
        winner's flags stay on the device for ekf_update_li_inliers"""
        st = np.zeros(4, np.int32)
        if not fetch:
            check(lib.pre3_ransac_select(self._ctx, int(n_draw), int(k), int(bool(early_exit)), None, None, dptr(st)))
            return dict(best=int(st[0]), iters=int(st[1]), n_hyp=int(st[2]), max_support=int(st[3]))
        sup = np.zeros(n_draw, np.int32)
        li = np.zeros(max(self.m, 1), np.int32)
        check(lib.pre3_ransac_select(self._ctx, int(n_draw), int(k), int(bool(early_exit)), dptr(sup), dptr(li), dptr(st)))
        return dict(support=sup, li_mask=li[:self.m], best=int(st[0]), iters=int(st[1]), n_hyp=int(st[2]), max_support=int(st[3]))

    def set_comm(self, comm):
        """attach a comm.Comm (None detaches): ransac_sharded_stream then runs its all-reduce on this filter's stream"""
        check(lib.pre3_set_comm(self._ctx, comm._h if comm is not None else None))
        self._comm = comm                                   # keeps the communicator alive as long as the filter borrows it

    def ransac_sharded_stream(self, hyp, threshold, early_exit=True, fetch=True):
        """pre3_ransac_sharded: ransac_hypotheses with the draws dealt to the communicator's ranks -- scoring, ncclAllReduce and selection
        on the library's stream, one wait; same dict as ransac_hypotheses, identical on every rank"""
        hyp = i32(hyp)
        n_draw, k = hyp.shape
        st = np.zeros(4, np.int32)
        if not fetch:
            check(lib.pre3_ransac_sharded(self._ctx, n_draw, k, dptr(hyp), C.c_double(float(threshold)), int(bool(early_exit)), None, None, dptr(st)))
            return dict(best=int(st[0]), iters=int(st[1]), n_hyp=int(st[2]), max_support=int(st[3]))
        sup = np.zeros(n_draw, np.int32)
        li = np.zeros(max(self.m, 1), np.int32)
        check(lib.pre3_ransac_sharded(self._ctx, n_draw, k, dptr(hyp), C.c_double(float(threshold)), int(bool(early_exit)), dptr(sup), dptr(li), dptr(st)))
        return dict(support=sup, li_mask=li[:self.m], best=int(st[0]), iters=int(st[1]), n_hyp=int(st[2]), max_support=int(st[3]))

    def test_stall(self, release):
        """test hook: 0 parks a kernel on the context's stream until test_stall(1) (a peer that stalls inside a collective)"""
        check(lib.pre3_test_stall(self._ctx, int(release)))

    def test_downdate(self, W, launches=1):
        """test hook (PRE3_TEST_HOOKS=1): P <- P - launches * W'W through the down-date launch alone; W is r x n.  Read P with get_p_k_k()."""
        W = f64(W)
        if W.ndim != 2 or W.shape[1] != self.n:
            raise ValueError("test_downdate: W must be r x %d" % self.n)
        check(lib.pre3_test_downdate(self._ctx, int(W.shape[0]), dptr(W), int(launches)))

    def test_factor_solve(self, S, B, nu, mode=0, predicted_prior=False):
        """test hook (PRE3_TEST_HOOKS=1): S = L L', L W = [B | nu] through the factorisation's launches alone (mode 0: P untouched) or with the
        down-date behind them as in an update (mode 1: read P with get_p_k_k()).  S is r x r, B r x n, nu r.  Returns (L, W): L r x r, lower triangle;
        W round_up(r, 64) x (n + 1), the nu column last."""
        S, B, nu = f64(S), f64(B), f64(nu)
        r = S.shape[0]
        if S.ndim != 2 or S.shape != (r, r) or B.shape != (r, self.n) or nu.shape != (r,):
            raise ValueError("test_factor_solve: S must be r x r, B r x %d, nu r" % self.n)
        L, W = np.zeros((r, r)), np.zeros(((r + 63) // 64 * 64, self.n + 1))
        check(lib.pre3_test_factor_solve(self._ctx, int(r), dptr(S), dptr(B), dptr(nu), int(mode), int(bool(predicted_prior)), dptr(L), dptr(W)))
        return L, W

    def ransac_export(self, n_draw, support_ptr, mask_ptr):
        check(lib.pre3_ransac_export(self._ctx, int(n_draw), C.c_void_p(support_ptr), C.c_void_p(mask_ptr)))

    def ransac_import(self, n_draw, support_ptr, mask_ptr):
        check(lib.pre3_ransac_import(self._ctx, int(n_draw), C.c_void_p(support_ptr), C.c_void_p(mask_ptr)))

    def ekf_update_li_inliers(self):
        check(lib.pre3_update_li(self._ctx))

    def rescue_hi_inliers(self, chi2=CHI2INV_2_95):
        hi = np.zeros(max(self.m, 1), np.int32)
        check(lib.pre3_rescue(self._ctx, C.c_double(chi2), dptr(hi)))
        return hi[:self.m]

    def ekf_update_hi_inliers(self):
        check(lib.pre3_update_hi(self._ctx))

    def ekf_update_all(self):
        check(lib.pre3_update_all(self._ctx))

    def set_flags(self, li=None, hi=None):
        li = None if li is None else i32(li)
        hi = None if hi is None else i32(hi)
        check(lib.pre3_set_flags(self._ctx, dptr(li), dptr(hi)))

    def get_flags(self):
        li, hi = np.zeros(max(self.m, 1), np.int32), np.zeros(max(self.m, 1), np.int32)
        check(lib.pre3_get_flags(self._ctx, dptr(li), dptr(hi)))
        return li[:self.m], hi[:self.m]

    def step(self, u, meas_idx, z, hyp, threshold=None, early_exit=True, chi2=CHI2INV_2_95):
        """One '1PRE' filter step (mono_slam.m:153-187)."""
        u, meas_idx, z, hyp = f64(u), i32(meas_idx), f64(z), i32(hyp)
        self.m = int(meas_idx.shape[0])
        self.meas_idx = meas_idx
        n_draw, k = hyp.shape
        st = self._st
        rc = lib.pre3_step(self._ctx, addr(u), self.m, addr(meas_idx), addr(z), n_draw, k, addr(hyp),
                           self.std_z if threshold is None else threshold, 1 if early_exit else 0, chi2, self._st_addr)
        if rc:
            check(rc)
        s = st.tolist()
        return dict(best=s[0], iters=s[1], n_hyp=s[2], max_support=s[3], n_li=s[4], n_hi=s[5])

    def step_all(self, u, meas_idx, z):
        """pre3_step_all -- mono_slam.m's 'PURE_EKF' branch (:153-162, :199): ekf_prediction, search_IC_matches' projection / Jacobians / S_i, the
        measurements, ekf_update_all, as one call (the same arithmetic as the four calls, fewer launches)"""
        u, meas_idx, z = f64(u), i32(meas_idx), f64(z)
        self.m = int(meas_idx.shape[0])
        self.meas_idx = meas_idx
        check(lib.pre3_step_all(self._ctx, dptr(u), self.m, dptr(meas_idx), dptr(z)))

    def step_predicted(self, hyp, threshold=None, early_exit=True, chi2=CHI2INV_2_95):
        """mono_slam.m:178-187 (RANSAC, LI update, rescue, HI update) behind ekf_prediction() and matching_sift_based() (or search_IC_matches()
        + set_measurements()): the installed measurements, pre3_step's device-driven launches."""
        hyp = i32(hyp)
        n_draw, k = hyp.shape
        rc = lib.pre3_step_predicted(self._ctx, n_draw, k, addr(hyp), self.std_z if threshold is None else threshold, 1 if early_exit else 0, chi2, self._st_addr)
        if rc:
            check(rc)
        s = self._st.tolist()
        return dict(best=s[0], iters=s[1], n_hyp=s[2], max_support=s[3], n_li=s[4], n_hi=s[5])

    def _seeded_out(self, n_draw, return_hyp):
        return (np.zeros(max(n_draw, 1) * 3, np.int32) if return_hyp else None), C.c_int32(0)

    def _seeded_result(self, n_draw, hyp, k):
        s = self._st.tolist()
        out = dict(best=s[0], iters=s[1], n_hyp=s[2], max_support=s[3], n_li=s[4], n_hi=s[5])
        if hyp is not None:
            out["hyp"] = hyp[:n_draw * k.value].reshape(n_draw, k.value).copy()
        return out

    def step_seeded(self, u, meas_idx, z, seed, seq, n_draw, threshold=None, early_exit=True, chi2=CHI2INV_2_95, return_hyp=False):
        """step() with the hypothesis table drawn on the device from (seed, seq): no table is built on the host or shipped.
        return_hyp=True also fetches the table (synchronises)."""
        u, meas_idx, z = f64(u), i32(meas_idx), f64(z)
        self.m = int(meas_idx.shape[0])
        self.meas_idx = meas_idx
        n_draw = int(n_draw)
        hyp, k = self._seeded_out(n_draw, return_hyp)
        rc = lib.pre3_step_seeded(self._ctx, addr(u), self.m, addr(meas_idx), addr(z), int(seed), int(seq), n_draw,
                                  self.std_z if threshold is None else threshold, 1 if early_exit else 0, chi2, dptr(hyp), C.byref(k), self._st_addr)
        if rc:
            check(rc)
        return self._seeded_result(n_draw, hyp, k)

    def step_predicted_seeded(self, seed, seq, n_draw, threshold=None, early_exit=True, chi2=CHI2INV_2_95, return_hyp=False):
        """step_predicted() with the table drawn on the device from (seed, seq)."""
        n_draw = int(n_draw)
        hyp, k = self._seeded_out(n_draw, return_hyp)
        rc = lib.pre3_step_predicted_seeded(self._ctx, int(seed), int(seq), n_draw, self.std_z if threshold is None else threshold,
                                            1 if early_exit else 0, chi2, dptr(hyp), C.byref(k), self._st_addr)
        if rc:
            check(rc)
        return self._seeded_result(n_draw, hyp, k)

    # ---- measurement hooks
    def timer_start(self):
        check(lib.pre3_timer_start(self._ctx))

    def timer_stop(self):
        ms = C.c_double(0)
        check(lib.pre3_timer_stop(self._ctx, C.byref(ms)))
        return ms.value

    def kernel_timing(self, enable):
        """True / 1: time every K9 launch; N > 1: one launch in N; False / 0: off."""
        check(lib.pre3_kernel_timing(self._ctx, int(enable)))

    def kernel_timing_read(self):
        """launches / total_ms / flops (SYRK count n(n+1)r) / bytes of the bracketed launches; fused = how many of them were launches of the
        persistent factorisation with the down-date inside, fact_flops = the factorisation + solve flops those also executed"""
        fu, ff = C.c_int(0), C.c_double(0)
        check(lib.pre3_kernel_timing_info(self._ctx, C.byref(fu), C.byref(ff)))
        n, ms, fl, by = C.c_int(0), C.c_double(0), C.c_double(0), C.c_double(0)
        check(lib.pre3_kernel_timing_read(self._ctx, C.byref(n), C.byref(ms), C.byref(fl), C.byref(by)))
        return dict(launches=n.value, total_ms=ms.value, flops=fl.value, bytes=by.value, fused=fu.value, fact_flops=ff.value)

    def bench_downdate(self, r, reps):
        ms = C.c_double(0)
        check(lib.pre3_bench_downdate(self._ctx, int(r), int(reps), C.byref(ms)))
        return ms.value


# ---------------------------------------------------------------------------------------------------
# stateless drop-ins
# ---------------------------------------------------------------------------------------------------
def _to_ell(H, n):
    """rows of H (dense r x n ndarray or scipy.sparse) -> (width, nnz[r], col[r*width], val[r*width])"""
    try:
        import scipy.sparse as sp
        if sp.issparse(H):
            H = H.tocsr()
            r = H.shape[0]
            nnz = np.diff(H.indptr).astype(np.int32)
            width = max(int(nnz.max()) if r else 1, 1)
            col = np.zeros((r, width), np.int32)
            val = np.zeros((r, width))
            for a in range(r):
                s, e = H.indptr[a], H.indptr[a + 1]
                col[a, :e - s] = H.indices[s:e]
                val[a, :e - s] = H.data[s:e]
            return width, nnz, col, val
    except ImportError:  # pragma: no cover
        pass
    H = np.asarray(H, dtype=np.float64)
    r = H.shape[0]
    nz = H != 0
    nnz = nz.sum(axis=1).astype(np.int32)
    width = max(int(nnz.max()) if r else 1, 1)
    col = np.zeros((r, width), np.int32)
    val = np.zeros((r, width))
    for a in range(r):
        idx = np.nonzero(nz[a])[0]
        col[a, :len(idx)] = idx
        val[a, :len(idx)] = H[a, idx]
    return width, nnz, col, val


def update(x_km1_k, p_km1_k, H, R, z, h, dtype="f64", device=0, want_K=True):
    """[x_k_k, p_k_k, K] = update(x_km1_k, p_km1_k, H, R, z, h)   (update.m:27).

    H: r x n (dense or scipy sparse, at most 16 non-zeros per row -- the reference's rows have 13);
    R: r x r or None for eye(r).  An empty z returns the inputs and K = 0 (update.m:50-55)."""
    x, P = f64(x_km1_k).ravel(), f64(p_km1_k)
    n = x.shape[0]
    z, h = f64(z).ravel(), f64(h).ravel()
    r = z.shape[0]
    xo, Po = np.empty(n), np.empty((n, n))
    if r == 0:
        check(lib.pre3_update_ell(int(device), {"f64": 0, "f32": 1}[dtype], n, 0, dptr(x), dptr(P), 1, None, None, None, None, None, None,
                                  dptr(xo), dptr(Po), None))
        return xo, Po, 0
    width, nnz, col, val = _to_ell(H, n)
    if width > 16:
        raise Pre3Error(-1, "update: H has a row with %d non-zeros; the measurement rows of this filter have 13 (max 16)" % width)
    col, val = i32(col), f64(val)
    Rm = None if R is None else f64(R)
    K = np.zeros((r, n)) if want_K else None
    check(lib.pre3_update_ell(int(device), {"f64": 0, "f32": 1}[dtype], n, r, dptr(x), dptr(P), width, dptr(nnz), dptr(col), dptr(val),
                              dptr(Rm), dptr(z), dptr(h), dptr(xo), dptr(Po), dptr(K)))
    return xo, Po, (K.T.copy() if want_K else None)       # K_out is n x r column-major == (r x n row-major)'


def predict_state_and_covariance(X_k, P_k, u, cam=None, dtype="f64", device=0):
    """[X_km1_k, P_km1_k] = predict_state_and_covariance(X_k, P_k, type, SD_A, SD_alpha) (predict_state_and_covariance.m:27) with
    u = [dX; dq] explicit (the .m file reads it from disk through fv.m:47).  Stateless: host arrays in, host arrays out
    (pre3_predict_dense).  `cam` is accepted for symmetry with the other mirrors and unused, as in the reference."""
    X_k, P_k, u = f64(X_k).ravel(), f64(P_k), f64(u).ravel()
    n = X_k.shape[0]
    if P_k.shape != (n, n) or u.shape[0] != 7:
        raise Pre3Error(-1, "predict_state_and_covariance: P must be %d x %d and u = [dX(3); dq(4)]" % (n, n))
    xo, Po = np.empty(n), np.empty((n, n))
    check(lib.pre3_predict_dense(int(device), {"f64": _lib.F64, "f32": _lib.F32}[dtype], n, dptr(X_k), dptr(P_k), dptr(u), dptr(xo), dptr(Po)))
    return xo, Po


def generate_state_vector_pattern(lm_type, has_z, z, n=None):
    """[state_vector_pattern, z_id, z_euc] = generate_state_vector_pattern(features_info, x) (generate_state_vector_pattern.m:29-53):
    lm_type[N] (0 inverse depth, 1 cartesian), has_z[N] (features_info(i).z non-empty), z[N][2].  Host bookkeeping (index arithmetic)."""
    lm_type = np.asarray(lm_type).astype(int)
    if n is None:
        n = 13 + int(np.sum(np.where(lm_type == _lib.INVDEPTH, 6, 3)))
    pat = np.zeros((n, 4))
    z_id, z_euc, pos = [], [], 13
    for i, t in enumerate(lm_type):
        if t == _lib.INVDEPTH:
            if has_z[i]:
                pat[pos:pos + 3, 0] = 1; pat[pos + 3:pos + 5, 1] = 1; pat[pos + 5, 2] = 1
                z_id.append(z[i])
            pos += 6
        else:
            if has_z[i]:
                pat[pos:pos + 3, 3] = 1
                z_euc.append(z[i])
            pos += 3
    return pat, np.array(z_id, float).reshape(-1, 2).T, np.array(z_euc, float).reshape(-1, 2).T


def compute_hypothesis_support_fast(xi, cam, state_vector_pattern, z_id, z_euc, threshold, device=0):
    """[hypothesis_support, positions_li_inliers_id, positions_li_inliers_euc] = compute_hypothesis_support_fast(xi, cam,
    state_vector_pattern, z_id, z_euc, threshold) (compute_hypothesis_support_fast.m:27).  z_id / z_euc are 2 x n as in MATLAB
    (empty arrays allowed); the masks come back as boolean vectors ([] for an empty class, as the reference returns)."""
    xi = f64(xi).ravel()
    n = xi.shape[0]
    pat = np.asfortranarray(np.asarray(state_vector_pattern, dtype=np.float64))
    if pat.shape != (n, 4):
        raise Pre3Error(-1, "compute_hypothesis_support_fast: state_vector_pattern must be %d x 4" % n)
    zi = np.asfortranarray(np.asarray(z_id, dtype=np.float64).reshape(2, -1)) if np.size(z_id) else np.zeros((2, 0), order="F")
    ze = np.asfortranarray(np.asarray(z_euc, dtype=np.float64).reshape(2, -1)) if np.size(z_euc) else np.zeros((2, 0), order="F")
    n_id, n_euc = zi.shape[1], ze.shape[1]
    sup = C.c_int32(0)
    pid, peu = np.zeros(max(n_id, 1), np.int32), np.zeros(max(n_euc, 1), np.int32)
    c = _cam(cam)
    check(lib.pre3_hypothesis_support(int(device), n, dptr(xi), C.addressof(c), dptr(pat), n_id, dptr(zi) if n_id else None, n_euc,
                                      dptr(ze) if n_euc else None, float(threshold), C.addressof(sup), dptr(pid), dptr(peu)))
    return int(sup.value), pid[:n_id].astype(bool), peu[:n_euc].astype(bool)
