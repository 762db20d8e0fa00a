"""Host-side mirror of the reference's visual-odometry RANSAC over the C ABI.

    vodometry_dr_ye.m:162-236            -> vo_ransac / vo_ransac_frames (all hypotheses, winner, final fit, statistics)
    ransac_dr_ye.m:28-46                 -> draw_hypotheses (the reference's own rejection rule, any numpy Generator)
    ransac_dr_ye.m:28-48                 -> vo_ransac_seeded / vo_ransac_frames_seeded (the same rule on the device, from (seed, seq))
    vodometry_dr_ye.m:171                -> vo_rst
    vodometry_dr_ye.m:139-236            -> vo_pair_seeded (siftmatch, rst and the RANSAC between two resident SR4000 frames, one call)
    Calculate_V_Omega_RANSAC_dr_ye.m:40-50 -> result["u"] = [T; R2q(R)], the argument of EkfFilter.ekf_prediction
    aux_code/cov_pose_shift_calc.m       -> cov_pose_shift_calc (the 7 x 7 covariance of [T; q] from the points' range and angle noise)
    aux_code/calc_cov_RANSAC_dr_ye.m:17-30 -> vo_cov, vo_pair_cov_seeded (the same from a pair's inliers, on the device behind the final fit)
    TestScripts/icp_with_init.m:34-120   -> icp_with_init, icp_frames, icp_pair_seeded (dense ICP seeded with a pose)

All compute runs in libpre3.so on the GPU; this module marshals numpy arrays and draws random numbers.
"""
import ctypes as C
from math import comb

import numpy as np

from ._lib import check, dptr, f64, i32, lib


class VoResult(C.Structure):
    _fields_ = [("rot", C.c_double * 9), ("trans", C.c_double * 3), ("euler", C.c_double * 3), ("u", C.c_double * 7),
                ("error_mean", C.c_double), ("error_std", C.c_double), ("dist", C.c_double),
                ("sta", C.c_int32), ("n_support", C.c_int32), ("n_iterations", C.c_int32), ("best", C.c_int32)]


def vo_rst(pnum):
    """rst = min(700, nchoosek(pnum, 4))  (vodometry_dr_ye.m:171)"""
    return min(700, comb(int(pnum), 4))


def draw_hypotheses(match, n_hyp, rng):
    """ransac_dr_ye.m:28-46, n_hyp times: positions num_rs(1:4) = round((pnum-1)*rand+1), redrawn while they repeat or share
    a keypoint -- including the reference's mixed-row comparisons in ind_dup3 (match(1,.) against match(2,.)).
    match: (2, pnum) keypoint numbers.  Returns 0-based positions (n_hyp, 4)."""
    m = np.asarray(match)
    pnum = m.shape[1]
    out = np.zeros((n_hyp, 4), np.int32)

    def rnd():
        return int(np.floor((pnum - 1) * rng.random() + 1 + 0.5)) - 1          # MATLAB round(), then 0-based

    def dup1(r):
        return m[0, r[0]] == m[0, r[1]] or m[1, r[0]] == m[1, r[1]]

    def dup2(r):
        return m[0, r[0]] == m[0, r[2]] or m[0, r[1]] == m[0, r[2]] or m[1, r[0]] == m[1, r[2]] or m[1, r[1]] == m[1, r[2]]

    def dup3(r):
        return (m[0, r[0]] == m[0, r[3]] or m[0, r[1]] == m[1, r[3]] or m[0, r[2]] == m[0, r[3]] or m[1, r[0]] == m[0, r[3]]
                or m[1, r[1]] == m[1, r[3]] or m[1, r[2]] == m[1, r[3]])

    for h in range(n_hyp):
        r = [rnd() for _ in range(4)]
        while r[1] == r[0] or dup1(r):
            r[1] = rnd()
        while r[2] == r[0] or r[2] == r[1] or dup2(r):
            r[2] = rnd()
        while r[3] == r[0] or r[3] == r[1] or r[3] == r[2] or dup3(r):
            r[3] = rnd()
        out[h] = r
    return out


def _result(res, cnum, state, inl):
    return dict(rot=np.array(res.rot).reshape(3, 3), trans=np.array(res.trans), euler=np.array(res.euler), u=np.array(res.u),
                error_mean=res.error_mean, error_std=res.error_std, dist=res.dist, sta=int(res.sta), n_support=int(res.n_support),
                n_iterations=int(res.n_iterations), best=int(res.best), cnum=cnum, state=state, inliers=inl)


def vo_ransac(pset1, pset2, draws, device=0):
    """pset1, pset2: (3, pnum) matched points of frame 1 / 2 (ransac_dr_ye.m:13-19); draws: (n_hyp, 4) 0-based."""
    p1, p2 = np.ascontiguousarray(f64(pset1).T), np.ascontiguousarray(f64(pset2).T)
    assert p1.shape == p2.shape and p1.shape[1] == 3
    draws = i32(draws).reshape(-1, 4)
    pnum, n_hyp = p1.shape[0], draws.shape[0]
    cnum, state, inl = np.zeros(n_hyp, np.int32), np.zeros(n_hyp, np.int32), np.zeros(max(pnum, 1), np.int32)
    res = VoResult()
    check(lib.pre3_vo_ransac(int(device), pnum, dptr(p1), dptr(p2), n_hyp, dptr(draws), dptr(cnum), dptr(state), dptr(inl), C.byref(res)))
    return _result(res, cnum, state, inl[:pnum])


def vo_ransac_frames(frm1, frm2, match, x1, y1, z1, x2, y2, z2, draws, device=0):
    """ransac_dr_ye's own argument list (frm: (>=2, K) SIFT frames, match: (2, pnum) 1-based, x/y/z: (rows, cols))."""
    imgs = [np.asfortranarray(f64(a)) for a in (x1, y1, z1, x2, y2, z2)]
    rows, cols = imgs[0].shape
    assert all(a.shape == (rows, cols) for a in imgs)
    f1, f2 = np.asfortranarray(f64(frm1)), np.asfortranarray(f64(frm2))
    assert f1.shape[0] == f2.shape[0] >= 2
    mt = np.asfortranarray(f64(match))
    pnum = mt.shape[1]
    draws = i32(draws).reshape(-1, 4)
    n_hyp = draws.shape[0]
    p1, p2 = np.zeros((max(pnum, 1), 3)), np.zeros((max(pnum, 1), 3))
    cnum, state, inl = np.zeros(n_hyp, np.int32), np.zeros(n_hyp, np.int32), np.zeros(max(pnum, 1), np.int32)
    res = VoResult()
    P = [a.ctypes.data_as(C.c_void_p) for a in imgs]
    check(lib.pre3_vo_ransac_frames(int(device), rows, cols, *P, f1.shape[0], f1.shape[1], f1.ctypes.data_as(C.c_void_p), f2.shape[1],
                                    f2.ctypes.data_as(C.c_void_p), pnum, mt.ctypes.data_as(C.c_void_p), n_hyp, dptr(draws), dptr(p1), dptr(p2),
                                    dptr(cnum), dptr(state), dptr(inl), C.byref(res)))
    out = _result(res, cnum, state, inl[:pnum])
    out["pset1"], out["pset2"] = p1[:pnum].T.copy(), p2[:pnum].T.copy()
    return out


def vo_ransac_seeded(pset1, pset2, match, seed, seq=0, n_hyp=None, device=0):
    """vo_ransac with the draws made on the device from (seed, seq) by ransac_dr_ye.m:28-48's rule.  match: (2, pnum)
    keypoint numbers; n_hyp None: vo_rst(pnum).  The dict also carries draws (n_hyp, 4) and capped (hypotheses a position of which hit the
    64-redraw cap)."""
    p1, p2 = np.ascontiguousarray(f64(pset1).T), np.ascontiguousarray(f64(pset2).T)
    assert p1.shape == p2.shape and p1.shape[1] == 3
    mt = np.asfortranarray(f64(match))
    pnum = p1.shape[0]
    assert mt.shape == (2, pnum)
    n_hyp = vo_rst(pnum) if n_hyp is None else int(n_hyp)
    nh = max(n_hyp, 1)
    draws, capped = np.zeros((nh, 4), np.int32), C.c_int32(0)
    cnum, state, inl = np.zeros(nh, np.int32), np.zeros(nh, np.int32), np.zeros(max(pnum, 1), np.int32)
    res = VoResult()
    check(lib.pre3_vo_ransac_seeded(int(device), pnum, dptr(p1), dptr(p2), mt.ctypes.data_as(C.c_void_p), n_hyp, int(seed), int(seq), dptr(draws),
                                    C.byref(capped), dptr(cnum), dptr(state), dptr(inl), C.byref(res)))
    out = _result(res, cnum[:n_hyp], state[:n_hyp], inl[:pnum])
    out["draws"], out["capped"] = draws[:n_hyp], int(capped.value)
    return out


def vo_ransac_frames_seeded(frm1, frm2, match, x1, y1, z1, x2, y2, z2, seed, seq=0, n_hyp=None, device=0):
    """vo_ransac_frames with the draws made on the device: the match list is read where the gather already has it."""
    imgs = [np.asfortranarray(f64(a)) for a in (x1, y1, z1, x2, y2, z2)]
    rows, cols = imgs[0].shape
    assert all(a.shape == (rows, cols) for a in imgs)
    f1, f2 = np.asfortranarray(f64(frm1)), np.asfortranarray(f64(frm2))
    assert f1.shape[0] == f2.shape[0] >= 2
    mt = np.asfortranarray(f64(match))
    pnum = mt.shape[1]
    n_hyp = vo_rst(pnum) if n_hyp is None else int(n_hyp)
    nh = max(n_hyp, 1)
    draws, capped = np.zeros((nh, 4), np.int32), C.c_int32(0)
    p1, p2 = np.zeros((max(pnum, 1), 3)), np.zeros((max(pnum, 1), 3))
    cnum, state, inl = np.zeros(nh, np.int32), np.zeros(nh, np.int32), np.zeros(max(pnum, 1), np.int32)
    res = VoResult()
    P = [a.ctypes.data_as(C.c_void_p) for a in imgs]
    check(lib.pre3_vo_ransac_frames_seeded(int(device), rows, cols, *P, f1.shape[0], f1.shape[1], f1.ctypes.data_as(C.c_void_p), f2.shape[1],
                                           f2.ctypes.data_as(C.c_void_p), pnum, mt.ctypes.data_as(C.c_void_p), n_hyp, int(seed), int(seq),
                                           dptr(draws), C.byref(capped), dptr(p1), dptr(p2), dptr(cnum), dptr(state), dptr(inl), C.byref(res)))
    out = _result(res, cnum[:n_hyp], state[:n_hyp], inl[:pnum])
    out["pset1"], out["pset2"] = p1[:pnum].T.copy(), p2[:pnum].T.copy()
    out["draws"], out["capped"] = draws[:n_hyp], int(capped.value)
    return out


def vo_pair_seeded(prev, cur, seed, seq=0, thresh=1.5):
    """vodometry_dr_ye.m:139-236 between the keypoint sets two resident frames hold (sr4000.SrFrame after keypoints()):
    siftmatch(des1, des2, thresh), rst = min(700, nchoosek(pnum, 4)) and the seeded RANSAC, all on the device.  The dict of vo_ransac_frames_seeded
    plus match (2, pnum) -- 1-based positions in the KEPT keypoint sets --, pnum and rst.  Fewer than four matches: sta = 4, u the identity, empty
    point sets, tables and inlier list."""
    return _pair_call(lib.pre3_vo_pair_seeded, prev, cur, seed, seq, thresh)


def _pair_call(fn, prev, cur, seed, seq, thresh, *extra):
    n1 = max(int(getattr(prev, "n_kept", 0)), 1)
    pnum, capped = C.c_int32(0), C.c_int32(0)
    match = np.zeros((2, n1), order="F")
    p1, p2 = np.zeros((n1, 3)), np.zeros((n1, 3))
    draws, cnum, state, inl = np.zeros((700, 4), np.int32), np.zeros(700, np.int32), np.zeros(700, np.int32), np.zeros(n1, np.int32)
    res = VoResult()
    check(fn(prev._h, cur._h, float(thresh), int(seed), int(seq), C.byref(pnum), dptr(match), dptr(p1), dptr(p2), dptr(draws),
             C.byref(capped), dptr(cnum), dptr(state), dptr(inl), C.byref(res), *extra))
    pnum = int(pnum.value)
    rst = vo_rst(pnum) if pnum >= 4 else 0
    out = _result(res, cnum[:rst].copy(), state[:rst].copy(), inl[:pnum if rst else 0].copy())
    out["pset1"], out["pset2"] = p1[:pnum if rst else 0].T.copy(), p2[:pnum if rst else 0].T.copy()
    out["draws"], out["capped"] = draws[:rst].copy(), int(capped.value)
    out["match"], out["pnum"], out["rst"] = match[:, :pnum].copy(order="F"), pnum, rst
    return out


def vo_pair_cov_seeded(prev, cur, seed, seq=0, thresh=1.5):
    """vo_pair_seeded with calc_cov_RANSAC_dr_ye.m:17-30 behind it on the device: one more launch behind the final fit, still one
    host wait.  The dict of vo_pair_seeded, bit for bit, plus cov_status (0 not computed: pnum < 4 or sta != 1; 1 valid; 2 unusable) and cov -- the
    (7, 7) covariance of u = [T; q] on status 1, else None."""
    cov, status = np.zeros((7, 7)), C.c_int32(0)
    out = _pair_call(lib.pre3_vo_pair_cov_seeded, prev, cur, seed, seq, thresh, dptr(cov), C.byref(status))
    out["cov_status"] = int(status.value)
    out["cov"] = cov if out["cov_status"] == 1 else None
    return out


def R2q(R):
    """R2q.m with Calculate_V_Omega_RANSAC_dr_ye.m:48's sign: the quaternion part of u = [T; R2q(R)] as k_vo_final forms it"""
    R = f64(R).reshape(3, 3)
    Tq = R[0, 0] + R[1, 1] + R[2, 2] + 1
    if Tq > 0.00000001:
        S = 2 * np.sqrt(Tq)
        a, b, c, d = 0.25 * S, (R[1, 2] - R[2, 1]) / S, (R[2, 0] - R[0, 2]) / S, (R[0, 1] - R[1, 0]) / S
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        S = 2 * np.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2])
        a, b, c, d = (R[1, 2] - R[2, 1]) / S, 0.25 * S, (R[0, 1] + R[1, 0]) / S, (R[2, 0] + R[0, 2]) / S
    elif R[1, 1] > R[2, 2]:
        S = 2 * np.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2])
        a, b, c, d = (R[2, 0] - R[0, 2]) / S, (R[0, 1] + R[1, 0]) / S, 0.25 * S, (R[1, 2] + R[2, 1]) / S
    else:
        S = 2 * np.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1])
        a, b, c, d = (R[0, 1] - R[1, 0]) / S, (R[2, 0] + R[0, 2]) / S, (R[1, 2] + R[2, 1]) / S, 0.25 * S
    return np.array([a, -b, -c, -d])


def vo_cov(pset1, pset2, u, inliers=None, device=0):
    """calc_cov_RANSAC_dr_ye.m:17-30, stateless: pset1, pset2 (3, pnum) = op_pset1, op_pset2; u = [trans; R2q(rot)]; inliers (pnum,) 0/1 or None
    (every point counts).  Returns dict(cov (7, 7) or None, status, n_inliers): status 0 not computed (pnum < 4), 1 valid, 2 unusable."""
    p1, p2 = np.ascontiguousarray(f64(pset1).T), np.ascontiguousarray(f64(pset2).T)
    assert p1.shape == p2.shape and p1.ndim == 2 and p1.shape[1] == 3
    pnum = p1.shape[0]
    u = f64(u).reshape(7)
    inl = None if inliers is None else i32(inliers).reshape(pnum)
    cov, status, n = np.zeros((7, 7)), C.c_int32(0), C.c_int32(0)
    check(lib.pre3_vo_cov(int(device), pnum, dptr(p1), dptr(p2), dptr(inl), dptr(u), dptr(cov), C.byref(status), C.byref(n)))
    st = int(status.value)
    return dict(cov=cov if st == 1 else None, status=st, n_inliers=int(n.value))


def cov_pose_shift_calc(Ya, Yb, R, T, device=0):
    """aux_code/cov_pose_shift_calc.m's signature over pre3_vo_cov: Ya, Yb (3, n) the matched inlier points of the two frames, R, T the fitted motion
    (Ya ~ R Yb + T).  Forms u = [T; R2q(R)] itself.  Returns the (7, 7) covariance of [T; q]; raises ValueError when it is not valid (fewer than four
    points, a singular fit, a non-finite coordinate).  The summed implicit-function form, not the .m file's per-point pinv."""
    u = np.concatenate([f64(T).reshape(3), R2q(R)])
    r = vo_cov(Ya, Yb, u, None, device)
    if r["status"] != 1:
        raise ValueError("cov_pose_shift_calc: status %d (0: fewer than four points, 2: singular fit or non-finite input)" % r["status"])
    return r["cov"]


class IcpResult(C.Structure):
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("Rtot", C.c_double * 9), ("ttot", C.c_double * 3), ("u", C.c_double * 7),
                ("error", C.c_double), ("sta", C.c_int32), ("p", C.c_int32), ("iters1", C.c_int32), ("iters2", C.c_int32),
                ("n_model", C.c_int32), ("n_source", C.c_int32), ("pad", C.c_int32)]


ICP_MAX_ITERATIONS = 62


def icp_limits():
    """dict(src_tile, chunk, pts_per_lane, iter_cap): the nearest-neighbour launch's source tile and model chunk, the source points a lane keeps in
    registers, and the iteration cap (pre3_icp_limits)"""
    out = np.zeros(4, np.int32)
    check(lib.pre3_icp_limits(dptr(out)))
    return dict(src_tile=int(out[0]), chunk=int(out[1]), pts_per_lane=int(out[2]), iter_cap=int(out[3]))


def _icp_seed(Rinit, Tinit):
    R = None if Rinit is None else np.ascontiguousarray(f64(Rinit).reshape(3, 3))
    T = None if Tinit is None else f64(Tinit).reshape(3).copy()
    return R, T


def _icp_result(r, corr, data2, log, pix=None):
    """the ICP's outputs as a dict; sta == 0 (not run): only sta"""
    sta = int(r.sta)
    if sta == 0:
        return dict(sta=0)
    p, n2, it = int(r.p), int(r.n_source), int(r.iters1) + int(r.iters2)
    out = dict(R=np.array(r.R).reshape(3, 3), t=np.array(r.t), Rtot=np.array(r.Rtot).reshape(3, 3), ttot=np.array(r.ttot), u=np.array(r.u),
               error=float(r.error), sta=sta, p=p, iters1=int(r.iters1), iters2=int(r.iters2), n_model=int(r.n_model), n_source=n2,
               corr=corr[:p].copy(), data2=data2[:n2].T.copy(), log=log[:it].copy())
    if pix is not None:
        out["corr_pix"] = pix[:p].copy()
    return out


def icp_with_init(data1, data2, res, Rinit=None, Tinit=None, device=0):
    """[R, t, corr, error, data2] = icp_with_init(data1, data2, res, Rinit, Tinit) (TestScripts/icp_with_init.m) on the device with the exact nearest
    neighbour in place of dsearchn's triangulation.  data1 (3, n1) the model, data2 (3, n2) the source.  Returns dict(R, t -- the accumulated
    registration of the seeded source --, Rtot = R Rinit, ttot = R Tinit + t, u = [ttot; R2q(Rtot)], corr (p, 3) = [model, source, D] 1-based,
    p, error, data2 (3, n2) registered, sta (1 ended by the reference's rule, 2 an iteration found fewer than three pairs), iters1, iters2,
    log (iterations, 3) = [phase, p, sum(D) / (p res)])."""
    d1, d2 = np.ascontiguousarray(f64(data1).T), np.ascontiguousarray(f64(data2).T)
    assert d1.ndim == 2 and d2.ndim == 2 and d1.shape[1] == 3 and d2.shape[1] == 3
    n1, n2 = d1.shape[0], d2.shape[0]
    R, T = _icp_seed(Rinit, Tinit)
    r = IcpResult()
    corr, out2, log = np.zeros((max(min(n1, n2), 1), 3)), np.zeros((max(n2, 1), 3)), np.zeros((ICP_MAX_ITERATIONS, 3))
    check(lib.pre3_icp(int(device), dptr(d1), n1, dptr(d2), n2, float(res), dptr(R), dptr(T), C.byref(r), dptr(corr), dptr(out2), dptr(log)))
    return _icp_result(r, corr, out2, log)


def _icp_frame_buffers(cur, stride):
    npix = cur.rows * cur.cols
    ncand = -(-cur.rows // max(int(stride), 1)) * -(-cur.cols // max(int(stride), 1))
    return np.zeros((ncand, 3)), np.zeros((ncand, 2), np.int32), np.zeros((ncand, 3)), np.zeros((ICP_MAX_ITERATIONS, 3)), npix


def icp_frames(prev, cur, res, Rinit=None, Tinit=None, stride=1):
    """icp_with_init between two resident frames (sr4000.SrFrame): the model every pixel of prev's filtered planes as [-x; -y; z] in column-major pixel
    order, the source cur's pixels at rows and columns 0, stride, ...; pixels with a non-finite coordinate or z <= 0 dropped on the device.  The dict of
    icp_with_init plus n_model, n_source (the kept counts) and corr_pix (p, 2): the 0-based column-major pixel of either side of every pair."""
    R, T = _icp_seed(Rinit, Tinit)
    corr, pix, out2, log, _ = _icp_frame_buffers(cur, stride)
    r = IcpResult()
    check(lib.pre3_icp_frames(prev._h, cur._h, int(stride), float(res), dptr(R), dptr(T), C.byref(r), dptr(corr), dptr(pix), dptr(out2), dptr(log)))
    return _icp_result(r, corr, out2, log, pix)


def icp_pair_seeded(prev, cur, seed, seq=0, thresh=1.5, stride=1, res=0.02):
    """vo_pair_seeded with icp_frames queued behind it on the same stream, seeded on the device with the pair's rot, trans: one host wait.  Returns
    (pair, icp): pair is vo_pair_seeded's dict, bit for bit; icp is icp_frames' dict, or dict(sta=0) when the pair did not end in sta == 1."""
    n1 = max(int(getattr(prev, "n_kept", 0)), 1)
    pnum, capped = C.c_int32(0), C.c_int32(0)
    match = np.zeros((2, n1), order="F")
    p1, p2 = np.zeros((n1, 3)), np.zeros((n1, 3))
    draws, cnum, state, inl = np.zeros((700, 4), np.int32), np.zeros(700, np.int32), np.zeros(700, np.int32), np.zeros(n1, np.int32)
    vres, r = VoResult(), IcpResult()
    corr, pix, out2, log, _ = _icp_frame_buffers(cur, stride)
    check(lib.pre3_icp_pair_seeded(prev._h, cur._h, float(thresh), int(seed), int(seq), int(stride), float(res), C.byref(pnum), dptr(match), dptr(p1),
                                   dptr(p2), dptr(draws), C.byref(capped), dptr(cnum), dptr(state), dptr(inl), C.byref(vres), C.byref(r), dptr(corr),
                                   dptr(pix), dptr(out2), dptr(log)))
    pnum = int(pnum.value)
    rst = vo_rst(pnum) if pnum >= 4 else 0
    pair = _result(vres, cnum[:rst].copy(), state[:rst].copy(), inl[:pnum if rst else 0].copy())
    pair["pset1"], pair["pset2"] = p1[:pnum if rst else 0].T.copy(), p2[:pnum if rst else 0].T.copy()
    pair["draws"], pair["capped"] = draws[:rst].copy(), int(capped.value)
    pair["match"], pair["pnum"], pair["rst"] = match[:, :pnum].copy(order="F"), pnum, rst
    return pair, _icp_result(r, corr, out2, log, pix)


def icp_cov_limits():
    """dict(pairs_per_workgroup, partials_per_thread): the pairs one workgroup of the partial-sum launch owns, and the partials a thread of the finishing
    workgroup adds at the largest supported p (pre3_icp_cov_limits); max_pairs = 256 x pairs_per_workgroup x partials_per_thread"""
    out = np.zeros(2, np.int32)
    check(lib.pre3_icp_cov_limits(dptr(out)))
    return dict(pairs_per_workgroup=int(out[0]), partials_per_thread=int(out[1]), max_pairs=256 * int(out[0]) * int(out[1]))


def icp_cov(data1, data2, corr, u, device=0):
    """The closed-form covariance of the ICP's u = [T; q] over its final pairs, stateless: data1 (3, n1) the model, data2 (3, n2)
    the ORIGINAL source (as icp_with_init took it), corr (p, 2) or icp_with_init's (p, 3): 1-based (model, source) rows, u the run's u.
    Returns dict(cov (7, 7) or None, status, n): status 0 not computed (p < 4), 1 valid, 2 unusable.  It propagates sensor noise only and is
    optimistic as a process noise."""
    d1, d2 = np.ascontiguousarray(f64(data1).T), np.ascontiguousarray(f64(data2).T)
    assert d1.ndim == 2 and d2.ndim == 2 and d1.shape[1] == 3 and d2.shape[1] == 3
    c = np.asarray(corr)
    c = np.ascontiguousarray(c.reshape(-1, c.shape[-1] if c.ndim == 2 else 2)[:, :2].astype(np.int32))
    u = f64(u).reshape(7)
    cov, status, n = np.zeros((7, 7)), C.c_int32(0), C.c_int32(0)
    check(lib.pre3_icp_cov(int(device), dptr(d1), d1.shape[0], dptr(d2), d2.shape[0], dptr(c), c.shape[0], dptr(u), dptr(cov), C.byref(status), C.byref(n)))
    st = int(status.value)
    return dict(cov=cov if st == 1 else None, status=st, n=int(n.value))


def icp_cov_bench(data1, data2, corr, u, reps=50, device=0):
    """milliseconds of icp_cov's two launches on resident operands (measurement only)"""
    d1, d2 = np.ascontiguousarray(f64(data1).T), np.ascontiguousarray(f64(data2).T)
    c = np.ascontiguousarray(np.asarray(corr)[:, :2].astype(np.int32))
    u = f64(u).reshape(7)
    ms = C.c_double(0)
    check(lib.pre3_icp_cov_bench(int(device), dptr(d1), d1.shape[0], dptr(d2), d2.shape[0], dptr(c), c.shape[0], dptr(u), int(reps), C.byref(ms)))
    return ms.value


def icp_pair_cov_seeded(prev, cur, seed, seq=0, thresh=1.5, stride=1, res=0.02):
    """icp_pair_seeded with both covariances behind it on the device, still one host wait.  Returns (pair, icp): the dicts of
    icp_pair_seeded, bit for bit; pair has vo_pair_cov_seeded's cov_status and cov besides, icp has cov_status (0 not computed: the ICP did not end in
    sta == 1, or p < 4; 1 valid; 2 unusable) and cov -- the (7, 7) covariance of icp["u"] on status 1, else None."""
    n1 = max(int(getattr(prev, "n_kept", 0)), 1)
    pnum, capped = C.c_int32(0), C.c_int32(0)
    match = np.zeros((2, n1), order="F")
    p1, p2 = np.zeros((n1, 3)), np.zeros((n1, 3))
    draws, cnum, state, inl = np.zeros((700, 4), np.int32), np.zeros(700, np.int32), np.zeros(700, np.int32), np.zeros(n1, np.int32)
    vres, r = VoResult(), IcpResult()
    corr, pix, out2, log, _ = _icp_frame_buffers(cur, stride)
    cov_p, st_p, cov_i, st_i = np.zeros((7, 7)), C.c_int32(0), np.zeros((7, 7)), C.c_int32(0)
    check(lib.pre3_icp_pair_cov_seeded(prev._h, cur._h, float(thresh), int(seed), int(seq), int(stride), float(res), C.byref(pnum), dptr(match), dptr(p1),
                                       dptr(p2), dptr(draws), C.byref(capped), dptr(cnum), dptr(state), dptr(inl), C.byref(vres), C.byref(r), dptr(corr),
                                       dptr(pix), dptr(out2), dptr(log), dptr(cov_p), C.byref(st_p), dptr(cov_i), C.byref(st_i)))
    pnum = int(pnum.value)
    rst = vo_rst(pnum) if pnum >= 4 else 0
    pair = _result(vres, cnum[:rst].copy(), state[:rst].copy(), inl[:pnum if rst else 0].copy())
    pair["pset1"], pair["pset2"] = p1[:pnum if rst else 0].T.copy(), p2[:pnum if rst else 0].T.copy()
    pair["draws"], pair["capped"] = draws[:rst].copy(), int(capped.value)
    pair["match"], pair["pnum"], pair["rst"] = match[:, :pnum].copy(order="F"), pnum, rst
    pair["cov_status"] = int(st_p.value)
    pair["cov"] = cov_p if pair["cov_status"] == 1 else None
    icp = _icp_result(r, corr, out2, log, pix)
    icp["cov_status"] = int(st_i.value)
    icp["cov"] = cov_i if icp["cov_status"] == 1 else None
    return pair, icp


# ---- the camera pose from 3-D / 2-D correspondences: EPnP and its RANSAC ------------------------------------------------------
class PnpResult(C.Structure):
    _fields_ = [("R", C.c_double * 9), ("T", C.c_double * 3), ("u", C.c_double * 7), ("err", C.c_double * 3),
                ("best", C.c_int32), ("sta", C.c_int32), ("n", C.c_int32), ("n_support", C.c_int32)]


class RelocResult(C.Structure):
    """pre3_reloc_result (include/pre3.h): EkfFilter.relocalise_seeded's result block"""
    _fields_ = [("pnp", PnpResult), ("u", C.c_double * 7), ("n_matches", C.c_int32), ("n_corr", C.c_int32), ("winner", C.c_int32), ("taken", C.c_int32)]


def _pnp_dict(r):
    return dict(R=np.array(r.R).reshape(3, 3), T=np.array(r.T), u=np.array(r.u), err=np.array(r.err), best=int(r.best), sta=int(r.sta), n=int(r.n),
                n_support=int(r.n_support))


def _pnp_args(Xw, U, cam):
    from ._lib import Cam
    xw, uv = f64(Xw), f64(U)
    assert xw.ndim == 2 and xw.shape[1] == 3 and uv.shape == (xw.shape[0], 2), "Xw is (n, 3) and U (n, 2): one correspondence a row"
    return xw, uv, Cam(*[float(v) for v in np.asarray(cam, np.float64).ravel()[:7]])


def pnp_limits():
    """dict(max_n, max_hyp) (pre3_pnp_limits)"""
    out = np.zeros(2, np.int32)
    check(lib.pre3_pnp_limits(dptr(out)))
    return dict(max_n=int(out[0]), max_hyp=int(out[1]))


def efficient_pnp(Xw, U, cam, undistort=False, device=0):
    """aux_code/EPnP_matlab/EPnP/efficient_pnp.m for kernel dimensions 1 to 3 on the device: Xw (n, 3) points, U (n, 2) pixels, cam = [f, Cx, Cy, k1,
    k2, nRows, nCols].  Returns R, T, Xc, best_solution in the reference's order (Xc = (R Xw' + T)', best_solution 1-based), plus the result dict:
    R, T, u (the VO pair's convention, what predict takes), err[3], best (0-based), sta (1 ok; 2 the best of three where the reference would go on
    to dimension 4, which is not built; -1 a non-finite intermediate), n.  undistort=True passes every pixel through undistort_fm_my_version.m's
    ten Newton steps first: the form to use on real frames."""
    xw, uv, c = _pnp_args(Xw, U, cam)
    r = PnpResult()
    check(lib.pre3_epnp(int(device), C.byref(c), int(bool(undistort)), xw.shape[0], dptr(xw), dptr(uv), C.byref(r)))
    d = _pnp_dict(r)
    return d["R"], d["T"], xw @ d["R"].T + d["T"], d["best"] + 1, d


def _pnp_ransac_out(n, n_hyp, want_hyp):
    return (np.zeros(n_hyp, np.int32), np.zeros(n_hyp, np.int32), np.zeros(n, np.int32), (PnpResult * n_hyp)() if want_hyp else None, PnpResult())


def _pnp_ransac_dict(sup, sta, inl, hyp, r, draws):
    d = _pnp_dict(r)
    d.update(support=sup, state=sta, inliers=inl, draws=draws, hyp=None if hyp is None else [_pnp_dict(h) for h in hyp])
    return d


def pnp_ransac(Xw, U, cam, draws, thr_px, undistort=False, hyp_results=False, device=0):
    """Six-point EPnP hypotheses from the table draws (n_hyp, 6), all scored over the n correspondences (an inlier: reprojection distance < thr_px and
    camera-frame z > 0), the winner by (largest support, smallest inlier distance sum, lowest index), and the EPnP refit over its inliers.  Returns
    the refit's dict (sta = 0 when the support is below six) with support, state, inliers (0/1 flags of the winner), draws and, on request, hyp."""
    xw, uv, c = _pnp_args(Xw, U, cam)
    dr = i32(draws).reshape(-1, 6)
    sup, sta, inl, hyp, r = _pnp_ransac_out(xw.shape[0], dr.shape[0], hyp_results)
    check(lib.pre3_pnp_ransac(int(device), C.byref(c), int(bool(undistort)), xw.shape[0], dptr(xw), dptr(uv), dr.shape[0], dptr(dr), float(thr_px), dptr(sup),
                              dptr(sta), dptr(inl), None if hyp is None else C.byref(hyp), C.byref(r)))
    return _pnp_ransac_dict(sup, sta, inl, hyp, r, dr)


def pnp_ransac_seeded(Xw, U, cam, n_hyp, thr_px, seed, seq=0, undistort=False, hyp_results=False, device=0):
    """pnp_ransac with the table drawn on the device (Philox stream 6, six distinct of n per hypothesis); bit-identical to pnp_ransac fed result["draws"]"""
    xw, uv, c = _pnp_args(Xw, U, cam)
    dr = np.zeros((max(int(n_hyp), 0), 6), np.int32)
    sup, sta, inl, hyp, r = _pnp_ransac_out(xw.shape[0], dr.shape[0], hyp_results)
    check(lib.pre3_pnp_ransac_seeded(int(device), C.byref(c), int(bool(undistort)), xw.shape[0], dptr(xw), dptr(uv), int(n_hyp), int(seed), int(seq), float(thr_px),
                                     dptr(dr), dptr(sup), dptr(sta), dptr(inl), None if hyp is None else C.byref(hyp), C.byref(r)))
    return _pnp_ransac_dict(sup, sta, inl, hyp, r, dr)


# ---- the pose refined by Gauss-Newton on the reprojection error, with its covariance -------------------------------------------
class PnpRefineResult(C.Structure):
    """pre3_pnp_refine_result (include/pre3.h)"""
    _fields_ = [("R", C.c_double * 9), ("T", C.c_double * 3), ("u", C.c_double * 7), ("cost", C.c_double * 11), ("cov6", C.c_double * 36), ("cov", C.c_double * 49),
                ("sigma2", C.c_double), ("sta", C.c_int32), ("n", C.c_int32), ("n_iter", C.c_int32), ("pad", C.c_int32)]


class RelocRefinedResult(C.Structure):
    """pre3_reloc_refined_result (include/pre3.h): EkfFilter.relocalise_refined_seeded's result block"""
    _fields_ = [("base", RelocResult), ("ref", PnpRefineResult), ("Pn", C.c_double * 49), ("noise_taken", C.c_int32), ("pad", C.c_int32)]


def _pnp_refine_dict(r):
    return dict(R=np.array(r.R).reshape(3, 3), T=np.array(r.T), u=np.array(r.u), cost=np.array(r.cost), cov6=np.array(r.cov6).reshape(6, 6),
                cov=np.array(r.cov).reshape(7, 7), sigma2=float(r.sigma2), sta=int(r.sta), n=int(r.n), n_iter=int(r.n_iter))


def pnp_refine(Xw, U, cam, R0, T0, n_iter=5, sigma_px=0.0, undistort=False, device=0):
    """Gauss-Newton on the reprojection error from the pose (R0, T0) (Xc = R Xw + T): exactly n_iter (0 .. 10) plain steps over the six pose parameters,
    the refined pose taken iff everything stayed finite, every point is in front of it and the cost fell; otherwise the input pose is kept.  Returns
    dict(R, T, u, cost (11,; r'r in px^2 before each step and after the last, NaN beyond n_iter), cov6 (6, 6) over (tau, omega), cov (7, 7) of u,
    sigma2, sta (1 refined pose taken; 2 input pose kept; -1 no covariance: R, T, u the input's, the covariances NaN), n, n_iter).  The covariance is
    sigma2 (J'J)^-1 with sigma2 = sigma_px^2, or cost / (2 n - 6) when sigma_px == 0.  It treats the 3-D points as exact -- pixel noise only -- and is
    optimistic for landmarks of a map."""
    xw, uv, c = _pnp_args(Xw, U, cam)
    r0, t0 = f64(R0).reshape(3, 3), f64(T0).reshape(3)
    r = PnpRefineResult()
    check(lib.pre3_pnp_refine(int(device), C.byref(c), int(bool(undistort)), xw.shape[0], dptr(xw), dptr(uv), dptr(r0), dptr(t0), int(n_iter), float(sigma_px),
                              C.byref(r)))
    return _pnp_refine_dict(r)


def pnp_ransac_refined_seeded(Xw, U, cam, n_hyp, thr_px, seed, seq=0, undistort=False, hyp_results=False, n_iter=5, sigma_px=0.0, device=0):
    """pnp_ransac_seeded with pnp_refine behind it on the device, over the winner's inliers from the refit's pose, still one host wait: the dict of
    pnp_ransac_seeded (bit-equal) plus ref, pnp_refine's dict (sta = 0 when the refit's sta is not 1 or 2)"""
    xw, uv, c = _pnp_args(Xw, U, cam)
    dr = np.zeros((max(int(n_hyp), 0), 6), np.int32)
    sup, sta, inl, hyp, r = _pnp_ransac_out(xw.shape[0], dr.shape[0], hyp_results)
    ref = PnpRefineResult()
    check(lib.pre3_pnp_ransac_refined_seeded(int(device), C.byref(c), int(bool(undistort)), xw.shape[0], dptr(xw), dptr(uv), int(n_hyp), int(seed), int(seq),
                                             float(thr_px), dptr(dr), dptr(sup), dptr(sta), dptr(inl), None if hyp is None else C.byref(hyp), C.byref(r),
                                             int(n_iter), float(sigma_px), C.byref(ref)))
    d = _pnp_ransac_dict(sup, sta, inl, hyp, r, dr)
    d["ref"] = _pnp_refine_dict(ref)
    return d


def vo_pair_pnp_seeded(prev, cur, seed, cam, seq=0, thresh=1.5, undistort=False):
    """vo_pair_seeded with RANSAC_CALC_VER2.m:191 behind it on the device: the EPnP of efficient_pnp over the pair's inliers --
    prev's range points (pset1) against cur's PIXELS, no depth of cur -- still one host wait.  The dict of vo_pair_seeded, bit for bit, plus pix2
    (2, pnum): cur's pixel of every match, and pnp: the result dict of efficient_pnp (u in the pair's convention, comparable with the pair's own u;
    sta = 0 and the identity when the pair's sta != 1 or it has fewer than six inliers).  On real frames pass undistort=True."""
    from ._lib import Cam
    c = Cam(*[float(v) for v in np.asarray(cam, np.float64).ravel()[:7]])
    n1 = max(int(getattr(prev, "n_kept", 0)), 1)
    pix, r = np.zeros((n1, 2)), PnpResult()
    fn = lambda a, b, th, sd, sq, *rest: lib.pre3_vo_pair_pnp_seeded(a, b, th, sd, sq, C.byref(c), int(bool(undistort)), *rest)      # noqa: E731
    out = _pair_call(fn, prev, cur, seed, seq, thresh, dptr(pix), C.byref(r))
    out["pix2"] = pix[:out["pnum"] if out["rst"] else 0].T.copy()
    out["pnp"] = _pnp_dict(r)
    return out


def pnp_bench(Xw, U, cam, n_hyp, thr_px, seed=1, seq=0, undistort=False, reps=20, device=0):
    """milliseconds of pnp_ransac_seeded's four launches on resident operands (measurement only)"""
    xw, uv, c = _pnp_args(Xw, U, cam)
    ms = C.c_double(0)
    check(lib.pre3_pnp_bench(int(device), C.byref(c), int(bool(undistort)), xw.shape[0], dptr(xw), dptr(uv), int(n_hyp), int(seed), int(seq), float(thr_px), int(reps),
                             C.byref(ms)))
    return ms.value


def icp_nn_bench(data1, data2, reps=20, device=0):
    """milliseconds of one nearest-neighbour launch on resident clouds (measurement only)"""
    d1, d2 = np.ascontiguousarray(f64(data1).T), np.ascontiguousarray(f64(data2).T)
    ms = C.c_double(0)
    check(lib.pre3_icp_nn_bench(int(device), dptr(d1), d1.shape[0], dptr(d2), d2.shape[0], int(reps), C.byref(ms)))
    return ms.value


def vo_bench(pset1, pset2, draws, reps=20, device=0):
    p1, p2 = np.ascontiguousarray(f64(pset1).T), np.ascontiguousarray(f64(pset2).T)
    draws = i32(draws).reshape(-1, 4)
    ms = C.c_double(0)
    check(lib.pre3_vo_bench(int(device), p1.shape[0], dptr(p1), dptr(p2), draws.shape[0], dptr(draws), int(reps), C.byref(ms)))
    return ms.value
