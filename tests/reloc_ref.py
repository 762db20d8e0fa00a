"""pre3_relocalise_seeded restated in numpy: the four stages over tests/epnp_ref.py's RANSAC, tests/pnp_draws_ref.py's draw
table and oracle/np_twin.py.  The project's own follow-up -- the reference has no relocalisation -- so this file restates the issue's rules, not an .m
file.  tests/test_reloc_host.py runs 3pre_amd/csrc/pre3_reloc.h on the host against select(); tests/test_gpu_relocalise.py the whole call."""
import numpy as np

import epnp_ref as ref
import pnp_draws_ref as dr
from oracle import np_twin as tw

IDENTITY_U = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])


# ---- stage 1: siftmatch(bank, scan) over every landmark --------------------------------------------------------------------------------------------
def match(bank, scan_desc, thresh):
    """bank (N, 128), scan_desc (K2, 128) -> pairs (M, 2) int32, 0-based (k1, k2) in ascending k1.  sift/siftmatch.c:97-122 in the double class: every
    pair's bins accumulated in order (np_twin.siftmatch sums them pairwise: the last bit may differ, and with it a tie), the first index on ties, the
    ratio test in float."""
    a, b = np.asarray(bank, np.float64), np.asarray(scan_desc, np.float64)
    acc = np.zeros((len(a), len(b)))
    for k in range(a.shape[1]):
        dlt = a[:, k][:, None] - b[:, k][None, :]
        acc = acc + dlt * dlt
    th = np.float32(thresh)
    pairs = []
    for k1 in range(len(a)):
        d = acc[k1]
        if len(d) == 0:
            continue
        best_i = int(np.argmin(d))                       # the first of equal minima
        best = d[best_i]
        second = np.min(np.delete(d, best_i)) if len(d) > 1 else np.inf
        if th * np.float32(best) <= np.float32(second):
            pairs.append((k1, best_i))
    return np.array(pairs, np.int32).reshape(-1, 2)


# ---- stage 2: the correspondences ------------------------------------------------------------------------------------------------------------------
def landmark_points(types, off, x):
    """(N, 3): inversedepth2cartesian.m for an inverse-depth landmark (a point at infinity when rho = 0), the state's own entries for a Cartesian one"""
    out = np.zeros((len(types), 3))
    with np.errstate(divide="ignore", invalid="ignore"):
        for i, (t, o) in enumerate(zip(types, off)):
            out[i] = x[o:o + 3] + (1.0 / x[o + 5]) * tw.m_dir(x[o + 3], x[o + 4]) if t == tw.INVDEPTH else x[o:o + 3]
    return out


def correspondences(pairs, xyz, scan_pos):
    """Xw (n_corr, 3), U (n_corr, 2) and the kept rows of pairs: a match whose point is not finite is left out, order kept.  scan_pos (K2, 4) is
    SCALE_ORIENT_POS_RAW', of which entries 0 and 1 are the pixel."""
    keep = np.array([bool(np.isfinite(xyz[k1]).all()) for k1, _ in pairs], bool).reshape(-1)
    kept = pairs[keep]
    return xyz[kept[:, 0]].reshape(-1, 3), np.asarray(scan_pos)[kept[:, 1], :2].reshape(-1, 2), keep


# ---- stage 4: the rule ------------------------------------------------------------------------------------------------------------------------------
def select(x7, sta, n_support, min_support, pnp_u):
    """(u, taken): pre3_reloc.h's reloc_select"""
    if not (sta == 1 and n_support >= min_support):
        return IDENTITY_U.copy(), 0
    r, q = np.asarray(x7[:3], np.float64), np.asarray(x7[3:7], np.float64)
    dX = tw.q2R(q).T @ (np.asarray(pnp_u[:3]) - r)
    dq = tw.qProd(q * np.array([1.0, -1.0, -1.0, -1.0]), np.asarray(pnp_u[3:7]))[0] / (q @ q)
    if dq[0] < 0:
        dq = -dq
    return np.concatenate([dX, dq]), 1


def predict_pose(x7, u):
    """predict_state_and_covariance.m:60-77 on the pose alone: r + R(q) u_r, q (x) u_q normalised"""
    q = tw.qProd(x7[3:7], u[3:7])[0]
    return np.concatenate([x7[:3] + tw.q2R(x7[3:7]) @ u[:3], q / np.linalg.norm(q)])


# ---- the chain --------------------------------------------------------------------------------------------------------------------------------------
def relocalise(types, off, x, bank, scan_desc, scan_pos, cam, seed, seq=0, thresh=1.5, n_hyp=200, thr_px=2.0, undistort=True, min_support=12):
    """dict(pairs, keep, Xw, U, n_matches, n_corr, ransac (epnp_ref.ransac's dict, None when n_corr < 6), draws, winner, pnp (the refit's dict or None),
    sta, n_support, u, taken, inliers (flags over the correspondences), pose (the predicted [r; q]))"""
    pairs = match(bank, scan_desc, thresh)
    Xw, U, keep = correspondences(pairs, landmark_points(types, off, x), scan_pos)
    n = len(Xw)
    out = dict(pairs=pairs, keep=keep, Xw=Xw, U=U, n_matches=len(pairs), n_corr=n, ransac=None, draws=None, winner=-1, pnp=None, sta=0, n_support=0,
               inliers=np.zeros(n, np.int32))
    if n >= 6:
        Uu = ref.undistort10(cam, U) if undistort else U
        draws = dr.draw_pnp(seed, seq, n, n_hyp)
        rs = ref.ransac(Xw, Uu, cam, draws, thr_px)
        out.update(ransac=rs, draws=draws, winner=rs["winner"], pnp=rs["res"], n_support=int(rs["support"][rs["winner"]]),
                   inliers=rs["flags"][rs["winner"]].astype(np.int32), Uu=Uu)
        out["sta"] = rs["res"]["sta"] if rs["res"] is not None else 0
    pnp_u = ref.pair_u(out["pnp"]["R"], out["pnp"]["T"]) if out["sta"] in (1, 2) else IDENTITY_U
    out["pnp_u"] = pnp_u
    out["u"], out["taken"] = select(x[:7], out["sta"], out["n_support"], min_support, pnp_u)
    out["pose"] = predict_pose(x[:7], out["u"])
    return out
