"""numpy restatement of the patch branch of search_IC_matches.m:45-51, written from the .m files and independent of the HIP code:
predict_features_appearance.m:34-53 + pred_patch_fc.m:27-85 (over rotate_with_dist_fc_c2c1.m, rotate_with_dist_fc_c1c2.m,
undistort_fm_my_version.m, distort_fm_my_version.m) and mex_files/CorePar_Ver1/matching.m:39-146 over corrcoef_partitioned.m:3-21.

Pixels are the reference's 1-based coordinates; images are (nRows, nCols) arrays indexed [row - 1, column - 1]; a stored patch is (41, 41)
indexed the same way.  corrcoef is numpy.corrcoef; the fork's mode is the literal partition loop; interp2 is linear with NaN outside."""
import warnings

import numpy as np

HALF_INIT, HALF_MATCH, CHI_095_2 = 20, 6, 5.9915
NOT_PREDICTED, NO_PATCH, ZERO_PATCH, WARP_OUTSIDE, NO_CANDIDATE, BELOW, MATCHED, WARPED = range(8)


def q2r(q):
    r, x, y, z = q
    return np.array([[r * r + x * x - y * y - z * z, 2 * (x * y - r * z), 2 * (z * x + r * y)],
                     [2 * (x * y + r * z), r * r - x * x + y * y - z * z, 2 * (y * z - r * x)],
                     [2 * (z * x - r * y), 2 * (y * z + r * x), r * r - x * x - y * y + z * z]])


def undistort(uvd, cam):
    """undistort_fm_my_version.m:56-81; uvd (2, n)"""
    xd, yd = (uvd[0] - cam["Cx"]) / cam["f"], (uvd[1] - cam["Cy"]) / cam["f"]
    rd = np.sqrt(xd * xd + yd * yd)
    ru = rd / (1 + cam["k1"] * rd ** 2 + cam["k2"] * rd ** 4)
    for _ in range(10):
        f1 = ru + cam["k1"] * ru ** 3 + cam["k2"] * ru ** 5 - rd
        f1p = 1 + 3 * cam["k1"] * ru ** 2 + 5 * cam["k2"] * ru ** 4
        ru = ru - f1 / f1p
    D = 1 + cam["k1"] * ru ** 2 + cam["k2"] * ru ** 4
    return np.stack([cam["f"] * xd / D + cam["Cx"], cam["f"] * yd / D + cam["Cy"]])


def distort(uv, cam):
    """distort_fm_my_version.m:52-61; uv (2, n)"""
    xu, yu = (uv[0] - cam["Cx"]) / cam["f"], (uv[1] - cam["Cy"]) / cam["f"]
    ru = np.sqrt(xu * xu + yu * yu)
    D = 1 + cam["k1"] * ru ** 2 + cam["k2"] * ru ** 4
    return np.stack([xu * D * cam["f"] + cam["Cx"], yu * D * cam["f"] + cam["Cy"]])


def _K(cam):
    return np.array([[cam["f"], 0, cam["Cx"]], [0, cam["f"], cam["Cy"]], [0, 0, 1.0]])


def _transfer(cam, uv, Hm):
    und = undistort(uv, cam)
    p = Hm @ np.vstack([und, np.ones((1, und.shape[1]))])
    return distort(p[:2] / p[2], cam)


def rotate_c1c2(cam, uv_c2, R, t, n, d):
    """rotate_with_dist_fc_c1c2.m:40-43; uv (2, n)"""
    K = _K(cam)
    return _transfer(cam, uv_c2, K @ (R - np.outer(t, n) / d) @ np.linalg.inv(K))


def rotate_c2c1(cam, uv_c1, R, t, n, d):
    """rotate_with_dist_fc_c2c1.m:41-50"""
    K = _K(cam)
    return _transfer(cam, uv_c1, np.linalg.inv(K @ (R - np.outer(t, n) / d) @ np.linalg.inv(K)))


def interp2_linear(V, xq, yq):
    """interp2(1:nx, 1:ny, V, xq, yq), linear: V[row = y - 1, column = x - 1]; NaN outside [1, nx] x [1, ny]"""
    ny, nx = V.shape
    V = V.astype(np.float64)
    out = np.full(xq.shape, np.nan)
    ok = (xq >= 1) & (xq <= nx) & (yq >= 1) & (yq <= ny)
    x, y = xq[ok], yq[ok]
    x0 = np.minimum(np.floor(x).astype(int), nx - 1)
    y0 = np.minimum(np.floor(y).astype(int), ny - 1)
    fx, fy = x - x0, y - y0
    v00, v10 = V[y0 - 1, x0 - 1], V[y0 - 1, x0]
    v01, v11 = V[y0, x0 - 1], V[y0, x0]
    top = v00 + fx * (v10 - v00)
    bot = v01 + fx * (v11 - v01)
    out[ok] = top + fy * (bot - top)
    return out


def landmark_xyz(x, lm_type, off):
    """predict_features_appearance.m:36-44 (inversedepth2cartesian.m)"""
    y = x[off:off + (6 if lm_type == 0 else 3)]
    if lm_type != 0:
        return y[:3].copy()
    theta, phi, rho = y[3], y[4], y[5]
    m = np.array([np.cos(phi) * np.sin(theta), -np.sin(phi), np.cos(phi) * np.cos(theta)])
    return y[:3] + m / rho


def pred_patch(cam, focal_over_d, h, patch, uv0, r0, R0, R_wk, r_wk, XYZ_w, want_coords=False):
    """pred_patch_fc.m:27-85 -> (status, patch (13, 13) [row, column]); status ZERO_PATCH / WARP_OUTSIDE / WARPED"""
    hw = HALF_MATCH
    if not (h[0] > hw and h[0] < cam["nCols"] - hw and h[1] > hw and h[1] < cam["nRows"] - hw):
        return (ZERO_PATCH, np.zeros((13, 13))) + ((None,) if want_coords else ())
    T1 = np.block([[R0, np.zeros((3, 1))], [np.zeros((1, 3)), np.ones((1, 1))]]) @ np.block([[np.eye(3), r0.reshape(3, 1)], [np.zeros((1, 3)), np.ones((1, 1))]])
    T2 = np.block([[R_wk, np.zeros((3, 1))], [np.zeros((1, 3)), np.ones((1, 1))]]) @ np.block([[np.eye(3), r_wk.reshape(3, 1)], [np.zeros((1, 3)), np.ones((1, 1))]])
    T1i = np.linalg.inv(T1)
    Hk = T1i @ T2
    n1 = -np.array([-(uv0[0] - cam["Cx"]), -(uv0[1] - cam["Cy"]), focal_over_d])
    n2 = -np.array([-(h[0] - cam["Cx"]), -(h[1] - cam["Cy"]), focal_over_d])
    n2 = Hk @ np.append(n2, 1.0)
    n2 = (n2 / n2[3])[:3]
    n1 = n1 / np.linalg.norm(n1)
    n2 = n2 / np.linalg.norm(n2)
    n = n1 + n2
    n = n / np.linalg.norm(n)
    Xk = T1i @ np.append(XYZ_w, 1.0)
    Xk = Xk / Xk[3]
    d = -n @ Xk[:3]
    R, t = Hk[:3, :3], Hk[:3, 3]
    c = rotate_c2c1(cam, np.asarray(uv0, dtype=np.float64).reshape(2, 1), R, t, n, d)[:, 0]
    us = c[0] - hw + np.arange(2 * hw + 1.0)
    vs = c[1] - hw + np.arange(2 * hw + 1.0)
    u_pred, v_pred = np.meshgrid(us, vs)                       # [row, column]
    uv = np.stack([u_pred.ravel(), v_pred.ravel()])
    back = rotate_c1c2(cam, uv, R, t, n, d)
    xs = (back[0] - (uv0[0] - HALF_INIT - 1)).reshape(13, 13)
    ys = (back[1] - (uv0[1] - HALF_INIT - 1)).reshape(13, 13)
    out = interp2_linear(patch, xs, ys)
    st = WARP_OUTSIDE if np.isnan(out).any() else WARPED
    return (st, out) + (((xs, ys),) if want_coords else ())


def candidates(h, S, nRows, nCols):
    """matching.m:61-62, :74-82 -> (list of (j, i) in scan order, the ellipse margin).  The margin is the smallest |nu' inv(S) nu - 5.9915| / 5.9915
    over the pixels of the box that pass :81-82's band test -- a pixel outside the band is rejected whatever the ellipse says (inf when there is none)."""
    invS = np.linalg.inv(S)
    hx, hy = int(np.ceil(5 * np.sqrt(S[0, 0]))), int(np.ceil(5 * np.sqrt(S[1, 1])))
    cx, cy = int(np.floor(h[0] + 0.5)), int(np.floor(h[1] + 0.5))        # MATLAB's round, h > 0
    js = np.arange(cx - hx, cx + hx + 1)
    i_s = np.arange(cy - hy, cy + hy + 1)
    J, I = np.meshgrid(js, i_s, indexing="ij")                 # j outer, i inner
    nu = np.stack([J - h[0], I - h[1]], axis=-1)
    q = np.einsum("...a,ab,...b->...", nu, invS, nu)
    band = (J > HALF_MATCH) & (J < nCols - HALF_MATCH) & (I > HALF_MATCH) & (I < nRows - HALF_MATCH)
    margin = float(np.min(np.abs(q[band] - CHI_095_2)) / CHI_095_2) if band.any() else np.inf
    keep = (q < CHI_095_2) & band
    return list(zip(J[keep].tolist(), I[keep].tolist())), margin


def _corrcoef(M):
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        return np.corrcoef(M, rowvar=False)


def corr_first_row(M, chunk=256):
    """corrcoef(M)(1, 2:end) without the K x K rest of the matrix: an entry of corrcoef depends on its two columns alone, so the columns are taken
    `chunk` at a time beside column 1"""
    K = M.shape[1] - 1
    v = np.zeros(K)
    for a in range(0, K, chunk):
        b = min(a + chunk, K)
        v[a:b] = np.atleast_2d(_corrcoef(M[:, [0] + list(range(a + 1, b + 1))]))[0, 1:]
    return v


def corrcoef_partitioned(M):
    """corrcoef_partitioned.m:3-21, literally: M (169, n) -> a column"""
    n = M.shape[1]
    sp = n // 100
    if sp == 0:
        return np.atleast_2d(_corrcoef(M))[1:, 0]
    parts = []
    for i in range(1, 101):
        cols = [0] + list(range((i - 1) * sp, i * sp))           # [1, (i-1)*sp+1 : i*sp], 0-based
        parts.append(np.atleast_2d(_corrcoef(M[:, cols]))[1:, 0])
    return np.concatenate(parts)


def _nanmax(v):
    """MATLAB's [m, i] = max(v): NaN ignored, the first maximum; all NaN -> (NaN, 0); empty -> (None, None)"""
    if v.size == 0:
        return None, None
    if np.all(np.isnan(v)):
        return np.nan, 0
    i = int(np.nanargmax(v))
    return float(v[i]), i


def closed_form_range(K, strict):
    """the candidates (0-based ordinals [lo, hi)) the mode's maximum is over, and the offset from the best ordinal to z's"""
    if not strict:
        return 0, K, 0
    n = K + 1
    if n < 100:
        return 1, K, -1
    return 0, 100 * (n // 100) - 1, 0


def match_one(im, pred, cands, thr, strict):
    """matching.m:68-123 for one landmark -> (accepted, z or None, maximum_correlation, gap between the best and the second best considered)"""
    K = len(cands)
    M = np.zeros((169, K + 1))
    M[:, 0] = pred.reshape(-1, order="F")
    for k, (j, i) in enumerate(cands):
        M[:, k + 1] = im[i - 7:i + 6, j - 7:j + 6].astype(np.float64).reshape(-1, order="F")
    if strict:
        cm = corrcoef_partitioned(M)                           # :102
        v = cm[1:]                                             # :118 correlation_matrix(2:end, 1)
    else:
        v = corr_first_row(M)                                  # :115 correlation_matrix(1, 2:end)
    mx, idx = _nanmax(v)
    gap = np.inf
    fin = np.sort(v[~np.isnan(v)])
    if fin.size >= 2:
        gap = float(fin[-1] - fin[-2])
    if mx is None or not (mx > thr):
        return False, None, (np.nan if mx is None else mx), gap
    # :123 z = match_candidates(:, index_maximum_correlation), 1-based index into the candidate list
    return True, cands[idx], mx, gap


def match_closed(im, pred, cands, thr, strict):
    """the same through the closed form of the fork's mode (what a kernel may use)"""
    K = len(cands)
    lo, hi, zoff = closed_form_range(K, strict)
    M = np.zeros((169, K + 1))
    M[:, 0] = pred.reshape(-1, order="F")
    for k, (j, i) in enumerate(cands):
        M[:, k + 1] = im[i - 7:i + 6, j - 7:j + 6].astype(np.float64).reshape(-1, order="F")
    v = corr_first_row(M)
    mx, idx = _nanmax(v[lo:hi]) if hi > lo else (None, None)
    if mx is None or not (mx > thr):
        return False, None, (np.nan if mx is None else mx)
    return True, cands[lo + idx + zoff], mx


def search(cam, focal_over_d, im, x, lm_type, lm_off, h, has_h, S, bank, thr, strict, closed=False):
    """search_IC_matches.m:45-51 for a whole map.  bank: dict(patch (N, 41, 41), uv_init (N, 2), r_wc (N, 3), R_wc (N, 3, 3), has_patch (N,)).
    Returns dict(status, ncand, corr, z (N, 2; NaN where unmatched), meas_idx, patches (N, 13, 13), pstatus, margin_ellipse, margin_gap, coords)."""
    N = len(lm_type)
    R_wk, r_wk = q2r(x[3:7]), x[0:3]
    out = dict(status=np.zeros(N, np.int32), ncand=np.zeros(N, np.int32), corr=np.full(N, np.nan), z=np.full((N, 2), np.nan),
               patches=np.zeros((N, 13, 13)), pstatus=np.zeros(N, np.int32), margin_ellipse=np.full(N, np.inf), margin_gap=np.full(N, np.inf),
               coords=[None] * N)
    for i in range(N):
        if not has_h[i]:
            out["status"][i] = out["pstatus"][i] = NOT_PREDICTED
            continue
        if not bank["has_patch"][i]:
            out["status"][i] = out["pstatus"][i] = NO_PATCH
            continue
        st, pp, co = pred_patch(cam, focal_over_d, h[i], bank["patch"][i], bank["uv_init"][i], bank["r_wc"][i], bank["R_wc"][i], R_wk, r_wk,
                                landmark_xyz(x, lm_type[i], lm_off[i]), want_coords=True)
        out["pstatus"][i], out["patches"][i], out["coords"][i] = st, pp, co
        cands, margin = candidates(h[i], S[i], int(cam["nRows"]), int(cam["nCols"]))
        out["ncand"][i], out["margin_ellipse"][i] = len(cands), margin
        if st != WARPED:
            out["status"][i] = st                              # every correlation is NaN
            continue
        if len(cands) == 0:
            out["status"][i] = NO_CANDIDATE
            continue
        if closed:
            ok, z, mx = match_closed(im, pp, cands, thr, strict)
        else:
            ok, z, mx, gap = match_one(im, pp, cands, thr, strict)
            out["margin_gap"][i] = gap
        out["corr"][i] = mx
        out["status"][i] = MATCHED if ok else BELOW
        if ok:
            out["z"][i] = z
    out["meas_idx"] = np.flatnonzero(out["status"] == MATCHED).astype(np.int32)
    return out
