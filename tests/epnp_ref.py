"""EPnP (Moreno-Noguer, Lepetit, Fua: "Accurate Non-Iterative O(n) Solution to the PnP Problem", ICCV 2007) restated in numpy, fp64, statement by
statement after the reference's aux_code/EPnP_matlab/EPnP/efficient_pnp.m:34-175 for kernel dimensions 1, 2 and 3, quirks included (DESIGN.md
section 35).  Dimension 4 (:129-169) is not restated: where the reference would enter it the answer is the best of the three with sta = 2.

    Xw (n, 3) world points, U (n, 2) pixels, cam = [f, Cx, Cy, k1, k2, nRows, nCols]; A = [f 0 Cx; 0 f Cy; 0 0 1]

The eigenvectors come from numpy.linalg.eigh (LAPACK) or from jacobi12, the cyclic Jacobi of 3pre_amd/csrc/pre3_pnp.h restated here, so that the CPU
suite can say what separates the two.  Also here: the conversion of (R, T) to the VO pair's convention, the two pixel maps of the distortion model,
and the RANSAC of pre3_pnp_ransac with the draw table as an input.
"""
import numpy as np

THRESHOLD_REPROJECTION_ERROR = 20.0          # efficient_pnp.m:37 -- pixels, whatever its comment says
DSQ = np.array([2.0, 2.0, 1.0, 2.0, 1.0, 1.0])          # define_distances_btw_control_points.m: pairs 12 13 14 23 24 34 of Cw = [e1; e2; e3; 0]
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
JACOBI_SWEEPS = 30


def cam_A(cam):
    f, Cx, Cy = float(cam[0]), float(cam[1]), float(cam[2])
    return np.array([[f, 0.0, Cx], [0.0, f, Cy], [0.0, 0.0, 1.0]])


def alphas(Xw):
    """compute_alphas.m with define_control_points.m's Cw = [e1; e2; e3; 0]: [x, y, z, 1 - x - y - z]"""
    Xw = np.asarray(Xw, np.float64)
    return np.column_stack([Xw[:, 0], Xw[:, 1], Xw[:, 2], 1.0 - Xw[:, 0] - Xw[:, 1] - Xw[:, 2]])


def compute_M(U, Alph, A):
    """compute_M_ver2.m:32-52"""
    n = Alph.shape[0]
    fu, fv, u0, v0 = A[0, 0], A[1, 1], A[0, 2], A[1, 2]
    M = np.zeros((2 * n, 12))
    for j in range(4):
        a = Alph[:, j]
        M[0::2, 3 * j] = a * fu
        M[0::2, 3 * j + 2] = a * (u0 - U[:, 0])
        M[1::2, 3 * j + 1] = a * fv
        M[1::2, 3 * j + 2] = a * (v0 - U[:, 1])
    return M


# ---- the cyclic Jacobi of pre3_pnp.h --------------------------------------------------------------------------------------------------------------
def jacobi_pair(r, k):
    """pair k (0..5) of round r (0..10): the round-robin schedule, six disjoint pairs a round, every pair once a sweep"""
    a, b = (11, r) if k == 0 else ((r + k) % 11, (r - k + 11) % 11)
    return (a, b) if a < b else (b, a)


def jacobi_angle(app, aqq, apq):
    if apq == 0.0:
        return 1.0, 0.0
    zeta = (aqq - app) / (2.0 * apq)
    t = (1.0 if zeta >= 0 else -1.0) / (abs(zeta) + np.sqrt(1.0 + zeta * zeta))
    c = 1.0 / np.sqrt(1.0 + t * t)
    return c, c * t


def jacobi_done(A):
    off = 0.0
    dia = 0.0
    for i in range(12):
        for j in range(12):
            if i == j:
                dia += A[i, j] * A[i, j]
            else:
                off += A[i, j] * A[i, j]
    return np.sqrt(off) <= 2.0 ** -52 * np.sqrt(dia)


def jacobi12(S):
    """eigenvalues ascending (the lower column first on ties) and their vectors as columns; also the sweeps run"""
    A = np.array(S, np.float64)
    V = np.eye(12)
    sweeps = 0
    with np.errstate(all="ignore"):
        while sweeps < JACOBI_SWEEPS and not jacobi_done(A):
            for r in range(11):
                pq = [jacobi_pair(r, k) for k in range(6)]
                cs = [jacobi_angle(A[p, p], A[q, q], A[p, q]) for p, q in pq]
                B = A.copy()
                W = V.copy()
                for (p, q), (c, s) in zip(pq, cs):                  # columns of A and V
                    B[:, p] = c * A[:, p] - s * A[:, q]
                    B[:, q] = s * A[:, p] + c * A[:, q]
                    W[:, p] = c * V[:, p] - s * V[:, q]
                    W[:, q] = s * V[:, p] + c * V[:, q]
                A = B.copy()
                for (p, q), (c, s) in zip(pq, cs):                  # rows of A
                    A[p, :] = c * B[p, :] - s * B[q, :]
                    A[q, :] = s * B[p, :] + c * B[q, :]
                for (p, q), (c, s) in zip(pq, cs):
                    if s != 0.0:
                        A[p, q] = 0.0
                        A[q, p] = 0.0
                V = W
            sweeps += 1
    w = np.diag(A).copy()
    order = sorted(range(12), key=lambda i: (w[i], i))
    return w[order], V[:, order], sweeps


def kernel(M, eig="lapack"):
    """kernel_noise.m:19-22: eig(M'M); column 0 belongs to the smallest eigenvalue"""
    MtM = M.T @ M
    if eig == "jacobi":
        w, V, _ = jacobi12(MtM)
        return w, V
    return np.linalg.eigh(MtM)


def fix_signs(K):
    """eig leaves the sign of a vector open, and where the z < 0 rule meets an Xc of mixed signs (a poor six-point sample) the reference's answer
    depends on it: negating such an Xc leaves it mixed.  Both this restatement and the device fix the sign first: the entry of largest magnitude
    (the lowest index on ties) is made positive."""
    K = np.array(K)
    for c in range(K.shape[1]):
        i = int(np.argmax(np.abs(K[:, c])))
        if K[i, c] < 0:
            K[:, c] = -K[:, c]
    return K


def sign_margin(K):
    """the smallest gap between the largest and the second largest magnitude among the entries of a (unit) kernel vector, over the columns of K: where
    it is small, two eigensolvers may pick different entries to make positive -- fix_signs' own edge"""
    a = -np.sort(-np.abs(np.asarray(K)), axis=0)
    return float((a[0] - a[1]).min())


# ---- efficient_pnp.m's pieces ---------------------------------------------------------------------------------------------------------------------
def norm_sign_scale(X, Alph, Xw):
    """compute_norm_sign_scaling_factor.m:26-61"""
    Cc_ = X.reshape(4, 3)
    Xc_ = Alph @ Cc_
    dist_w = np.sqrt(((Xw - Xw.mean(axis=0)) ** 2).sum(axis=1))
    dist_c = np.sqrt(((Xc_ - Xc_.mean(axis=0)) ** 2).sum(axis=1))
    with np.errstate(all="ignore"):
        sc = 1.0 / ((1.0 / (dist_c @ dist_c)) * (dist_c @ dist_w))
        Cc = Cc_ / sc
    Xc = Alph @ Cc
    if (Xc[:, 2] < 0).any():
        sc = -sc
        Xc = Xc * (-1)
    return Cc, Xc, sc


def getrotT(wpts, cpts):
    """efficient_pnp.m:179-205"""
    ccent, wcent = cpts.mean(axis=0), wpts.mean(axis=0)
    M = (cpts - ccent).T @ (wpts - wcent)
    U, _, Vt = np.linalg.svd(M)
    R = U @ Vt
    if np.linalg.det(R) < 0:
        R = -R
    return R, ccent - R @ wcent


def reprojection(Xw, U, R, T, A):
    """efficient_pnp.m:210-226: the mean pixel distance (no test on depth) and the per-point distances"""
    P = A @ np.column_stack([R, T])
    Urep_ = (P @ np.column_stack([Xw, np.ones(len(Xw))]).T).T
    with np.errstate(all="ignore"):
        d = np.sqrt((U[:, 0] - Urep_[:, 0] / Urep_[:, 2]) ** 2 + (U[:, 1] - Urep_[:, 1] / Urep_[:, 2]) ** 2)
    return d.sum() / len(Xw), d


def _diffs(K):
    return [K[3 * i:3 * i + 3] - K[3 * j:3 * j + 3] for i, j in PAIRS]


def constraint_2(Km1, Km2):
    """compute_constraint_distance_2param_6eq_3unk: row (i, j) = [d1.d1, 2 d1.d2, d2.d2]"""
    return np.array([[a @ a, 2 * (a @ b), b @ b] for a, b in zip(_diffs(Km1), _diffs(Km2))])


def constraint_3(Km1, Km2, Km3):
    """compute_constraint_distance_3param_6eq_6unk: columns 11, 2.12, 2.13, 22, 2.23, 33"""
    return np.array([[a @ a, 2 * (a @ b), 2 * (a @ c), b @ b, 2 * (b @ c), c @ c] for a, b, c in zip(_diffs(Km1), _diffs(Km2), _diffs(Km3))])


def _sign(v):
    return float(np.sign(v))


def epnp(Xw, U, cam, eig="lapack", flip=(1, 1, 1, 1)):
    """efficient_pnp.m:34-175 without dimension 4.  flip: the signs the four kernel vectors are multiplied by before use (the answer does not depend
    on them).  Returns a dict: R, T (Xc = R Xw + T), Xc, err[3] (NaN where a dimension was not computed), best (0-based), sta (1 ok; 2 the best of
    three where the reference would go on to dimension 4; -1 a non-finite intermediate), d (the per-point distances of the answer), w (eigenvalues),
    dim3 (whether dimension 3 was entered), sols (R, T per computed dimension)."""
    Xw, U = np.asarray(Xw, np.float64), np.asarray(U, np.float64)
    n = len(Xw)
    A = cam_A(cam)
    Alph = alphas(Xw)
    M = compute_M(U, Alph, A)
    err = np.full(3, np.nan)
    bad = dict(R=np.eye(3), T=np.zeros(3), Xc=np.zeros((n, 3)), err=err, best=0, sta=-1, d=np.full(n, np.nan), w=np.full(12, np.nan), dim3=False, sols=[])
    with np.errstate(all="ignore"):
        finite = np.isfinite(M.T @ M).all()
    if not finite:
        return bad
    w, V = kernel(M, eig)
    Km = fix_signs(V[:, 3::-1]) * np.asarray(flip, np.float64)[::-1]          # Km(:, end) = V(:, 1)
    sols = []

    def solve(X):
        Cc, Xc, sc = norm_sign_scale(X, Alph, Xw)
        if not np.isfinite(Xc).all():
            sols.append((np.full((3, 3), np.nan), np.full(3, np.nan), Xc, np.full(n, np.nan)))
            return np.nan
        R, T = getrotT(Xw, Xc)
        e, d = reprojection(Xw, U, R, T, A)
        sols.append((R, T, Xc, d))
        return e

    with np.errstate(all="ignore"):
        err[0] = solve(Km[:, 3])
        D = constraint_2(Km[:, 2], Km[:, 3])
        try:
            b = np.linalg.inv(D.T @ D) @ D.T @ DSQ
        except np.linalg.LinAlgError:
            b = np.full(3, np.nan)
        beta1 = np.sqrt(abs(b[0]))
        beta2 = np.sqrt(abs(b[2])) * _sign(b[1]) * _sign(b[0])
        err[1] = solve(beta1 * Km[:, 2] + beta2 * Km[:, 3])
        dim3 = False
        if np.isfinite(err[:2]).all() and err[:2].min() > THRESHOLD_REPROJECTION_ERROR:
            dim3 = True
            D = constraint_3(Km[:, 1], Km[:, 2], Km[:, 3])
            try:
                b = np.linalg.inv(D) @ DSQ
            except np.linalg.LinAlgError:
                b = np.full(6, np.nan)
            beta1 = np.sqrt(abs(b[0]))
            beta2 = np.sqrt(abs(b[3])) * _sign(b[1]) * _sign(b[0])
            beta3 = np.sqrt(abs(b[5])) * _sign(b[2]) * _sign(b[0])
            err[2] = solve(beta1 * Km[:, 1] + beta2 * Km[:, 2] + beta3 * Km[:, 3])
    nd = 3 if dim3 else 2
    finite = np.isfinite(err[:nd]).all() and all(np.isfinite(s[0]).all() and np.isfinite(s[1]).all() for s in sols)
    if not finite:
        bad.update(err=err, w=w, dim3=dim3, sols=sols)
        return bad
    best = int(np.argmin(err[:nd]))                                  # [min_err, best] = min(err): the first index on ties
    sta = 2 if dim3 and err[:nd].min() > THRESHOLD_REPROJECTION_ERROR else 1
    R, T, Xc, d = sols[best]
    used = Km[:, 1:] if dim3 else Km[:, 2:]                             # the vectors the computed dimensions read
    return dict(R=R, T=T, Xc=Xc, err=err, best=best, sta=sta, d=d, w=w, dim3=dim3, sols=sols, sign_margin=sign_margin(used))


# ---- the pair's convention ------------------------------------------------------------------------------------------------------------------------
def r2q_vo(R):
    """R2q.m as the VO front end applies it (Calculate_V_Omega_RANSAC_dr_ye.m:40-50): [a, -b, -c, -d]"""
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


def pair_u(R, T):
    """u = [-R'T; R2q(R')]: Xc = R Xw + T read as pset1 ~ rot pset2 + trans with pset1 = Xw, pset2 = Xc -- what pre3_predict takes"""
    return np.concatenate([-(R.T @ T), r2q_vo(R.T)])


# ---- the distortion model -------------------------------------------------------------------------------------------------------------------------
def distort(cam, U):
    """distort_fm_my_version.m:52-61"""
    f, Cx, Cy, k1, k2 = [float(v) for v in cam[:5]]
    xu, yu = (U[:, 0] - Cx) / f, (U[:, 1] - Cy) / f
    r2 = xu * xu + yu * yu
    D = 1 + k1 * r2 + k2 * r2 * r2
    return np.column_stack([xu * D * f + Cx, yu * D * f + Cy])


def undistort10(cam, Ud):
    """undistort_fm_my_version.m:56-81: ten Newton steps"""
    f, Cx, Cy, k1, k2 = [float(v) for v in cam[:5]]
    xd, yd = (Ud[:, 0] - Cx) / f, (Ud[:, 1] - Cy) / f
    rd = np.sqrt(xd * xd + yd * yd)
    ru = rd / (1 + k1 * rd ** 2 + k2 * rd ** 4)
    for _ in range(10):
        f1 = ru + k1 * ru ** 3 + k2 * ru ** 5 - rd
        ru = ru - f1 / (1 + 3 * k1 * ru ** 2 + 5 * k2 * ru ** 4)
    D = 1 + k1 * ru ** 2 + k2 * ru ** 4
    return np.column_stack([f * xd / D + Cx, f * yd / D + Cy])


# ---- the RANSAC of pre3_pnp_ransac ----------------------------------------------------------------------------------------------------------------
def ransac(Xw, U, cam, draws, thr_px, eig="lapack"):
    """Every row of draws (n_hyp, 6) is solved by epnp on its six correspondences and all n are scored under its answer: an inlier has a reprojection
    distance < thr_px and a camera-frame z > 0.  A hypothesis with a non-finite pose has support 0 and state -1.  The winner: the largest support,
    then the smallest sum of inlier distances, then the lowest index.  res: epnp over the winner's inliers (None below six)."""
    Xw, U = np.asarray(Xw, np.float64), np.asarray(U, np.float64)
    draws = np.asarray(draws)
    A = cam_A(cam)
    H, n = len(draws), len(Xw)
    support, state, dsum = np.zeros(H, np.int32), np.zeros(H, np.int32), np.zeros(H)
    flags, dist, zc, hyp = np.zeros((H, n), bool), np.full((H, n), np.nan), np.full((H, n), np.nan), []
    for h in range(H):
        r = epnp(Xw[draws[h]], U[draws[h]], cam, eig)
        hyp.append(r)
        state[h] = r["sta"]
        if r["sta"] == -1:
            continue
        _, d = reprojection(Xw, U, r["R"], r["T"], A)
        z = Xw @ r["R"][2] + r["T"][2]
        dist[h], zc[h] = d, z
        flags[h] = (d < thr_px) & (z > 0)
        support[h] = flags[h].sum()
        dsum[h] = d[flags[h]].sum()
    order = sorted(range(H), key=lambda h: (-int(support[h]), dsum[h], h))
    winner = order[0]
    inl = np.nonzero(flags[winner])[0]
    res = epnp(Xw[inl], U[inl], cam, eig) if len(inl) >= 6 else None
    return dict(support=support, state=state, dsum=dsum, flags=flags, dist=dist, z=zc, hyp=hyp, winner=winner, order=order, inliers=inl, res=res)


def guard_excluded(rs, thr_px, guard):
    """the hypotheses left out of the exact comparison, judged in the restatement alone: a point's distance within the guard of thr_px (or its z of 0),
    an err within it of 20, two err within it of each other, or the two largest magnitudes of a kernel vector it reads (unit vectors) within it of each
    other -- the edge of fix_signs.  Also: whether the winner ties with the runner-up within the guard."""
    H = len(rs["support"])
    out = np.zeros(H, bool)
    for h in range(H):
        if rs["state"][h] == -1:
            continue
        e = rs["hyp"][h]["err"]
        e = e[np.isfinite(e)]
        near = (np.abs(rs["dist"][h] - thr_px) <= guard).any() or (np.abs(rs["z"][h]) <= guard).any() or (np.abs(e - THRESHOLD_REPROJECTION_ERROR) <= guard).any()
        near = near or any(abs(e[i] - e[j]) <= guard for i in range(len(e)) for j in range(i))
        out[h] = near or rs["hyp"][h]["sign_margin"] <= guard
    w = rs["order"][0]
    tie = False
    if H > 1:
        r = rs["order"][1]
        tie = rs["support"][w] == rs["support"][r] and abs(rs["dsum"][w] - rs["dsum"][r]) <= guard * max(1, int(rs["support"][w]))
    return out, tie
