"""An independent numpy restatement of the VO pair's covariance (the issue's "mathematics" section): nothing here is taken from
3pre_amd/csrc/pre3_vocov.h.  The rotation is held as the tensor of its quadratic form, R_ij(q) = q' Q_ij q, so that its first and second derivatives
come from one table instead of hand-written columns.

    f_p = pset1(:, i), f_n = pset2(:, i), r_i = T + R(q) f_n - f_p, X = [T; q], E = sum_i 1/2 |r_i|^2 over the inliers
    H = sum H_i, M = sum B_i Sigma_i B_i', cov = H^-1 M H^-1, symmetrised; status 0 / 1 / 2 as the status rule says
"""
import numpy as np

SIGMA_R = 0.01 / 2                       # cov_pose_shift_calc.m:38
SIGMA_A = 0.24 * np.pi / 180 / 4
EPS = np.finfo(np.float64).eps


def _quadratic_form():
    Q = np.zeros((3, 3, 4, 4))

    def add(i, j, k, l, v):              # v * q_k * q_l into R_ij, stored symmetrically in (k, l)
        Q[i, j, k, l] += v / 2
        Q[i, j, l, k] += v / 2
    a, b, c, d = 0, 1, 2, 3
    for (i, j, terms) in (
            (0, 0, ((a, a, 1), (b, b, 1), (c, c, -1), (d, d, -1))), (0, 1, ((b, c, 2), (a, d, -2))), (0, 2, ((b, d, 2), (a, c, 2))),
            (1, 0, ((b, c, 2), (a, d, 2))), (1, 1, ((a, a, 1), (b, b, -1), (c, c, 1), (d, d, -1))), (1, 2, ((c, d, 2), (a, b, -2))),
            (2, 0, ((b, d, 2), (a, c, -2))), (2, 1, ((c, d, 2), (a, b, 2))), (2, 2, ((a, a, 1), (b, b, -1), (c, c, -1), (d, d, 1)))):
        for (k, l, v) in terms:
            add(i, j, k, l, v)
    return Q


QF = _quadratic_form()


def rot(q):
    return np.einsum("ijkl,k,l->ij", QF, q, q)


def drot(q):
    """(3, 3, 4): dR/dq_k"""
    return 2 * np.einsum("ijkl,l->ijk", QF, q)


D2ROT = 2 * QF                           # (3, 3, 4, 4): d2R / dq_k dq_l, constant


def residual(fp, fn, X):
    return X[:3] + rot(X[3:]) @ fn - fp


def energy(P1, P2, X):
    """E over the columns of P1, P2 (3, n)"""
    r = X[:3, None] + rot(X[3:]) @ P2 - P1
    return 0.5 * float(np.sum(r * r))


def point_terms(fp, fn, X):
    """H_i (7, 7), B_i (7, 6), r_i"""
    q = X[3:]
    R, dR = rot(q), drot(q)
    r = X[:3] + R @ fn - fp
    A = np.einsum("ijk,j->ik", dR, fn)                     # (3, 4)
    J = np.hstack([np.eye(3), A])
    H = J.T @ J
    H[3:, 3:] += np.einsum("i,ijkl,j->kl", r, D2ROT, fn)
    Bn = J.T @ R
    Bn[3:, :] += np.einsum("i,ijk->kj", r, dR)             # row 3 + k: r' dR/dq_k
    return H, np.hstack([-J.T, Bn]), r


class Math:
    """the transcendentals the point covariance uses; a subclass may move each result by a few ulp (tests/golden/make_vo_cov_tolerance.py)"""
    def atan2(self, y, x): return np.arctan2(y, x)
    def hypot(self, a, b): return np.hypot(a, b)
    def sin(self, a): return np.sin(a)
    def cos(self, a): return np.cos(a)
    def sqrt(self, a): return np.sqrt(a)


def point_cov(p, m=Math()):
    """cov_pose_shift_calc.m:24-40"""
    hxy = m.hypot(p[0], p[1])
    az, el, r = m.atan2(p[1], p[0]), m.atan2(p[2], hxy), m.hypot(hxy, p[2])
    ca, sa, ce, se = m.cos(az), m.sin(az), m.cos(el), m.sin(el)
    Js = np.array([[ce * ca, -r * ce * sa, -r * se * ca],
                   [ce * sa, r * ce * ca, -r * se * sa],
                   [se, 0.0, r * ce]])
    return Js @ np.diag([SIGMA_R ** 2, SIGMA_A ** 2, SIGMA_A ** 2]) @ Js.T


def chol7(H, m=Math()):
    """lower Cholesky factor, or None when a pivot is not above 7 eps times its original diagonal entry"""
    n = H.shape[0]
    L = np.zeros_like(H)
    for j in range(n):
        d = H[j, j] - np.dot(L[j, :j], L[j, :j])
        if not d > 7 * EPS * H[j, j]:
            return None
        L[j, j] = m.sqrt(d)
        for i in range(j + 1, n):
            L[i, j] = (H[i, j] - np.dot(L[i, :j], L[j, :j])) / L[j, j]
    return L


def sums(pset1, pset2, inliers, u, order=None, m=Math()):
    """H, M, n_inliers, finite"""
    P1, P2 = np.asarray(pset1, float), np.asarray(pset2, float)
    X = np.asarray(u, float)
    idx = [k for k in range(P1.shape[1]) if inliers is None or inliers[k]]
    if order is not None:
        idx = [idx[t] for t in order]
    H, M, finite = np.zeros((7, 7)), np.zeros((7, 7)), True
    for k in idx:
        fp, fn = P1[:, k], P2[:, k]
        if not (np.all(np.isfinite(fp)) and np.all(np.isfinite(fn))):
            finite = False
            continue
        Hi, Bi, _ = point_terms(fp, fn, X)
        S = np.zeros((6, 6))
        S[:3, :3], S[3:, 3:] = point_cov(fp, m), point_cov(fn, m)
        H += Hi
        M += Bi @ S @ Bi.T
    return H, M, len(idx), finite


def cov(pset1, pset2, inliers, u, order=None, solver="chol", m=Math()):
    """(cov (7, 7) or None, status, n_inliers) -- pre3_vo_cov's contract (pnum < 4: status 0)"""
    if np.asarray(pset1).shape[1] < 4:
        return None, 0, 0
    H, M, n, finite = sums(pset1, pset2, inliers, u, order, m)
    if not finite:
        return None, 2, n
    L = chol7(H, m)
    if L is None:
        return None, 2, n
    if solver == "chol":
        C = _tri_solve(L, _tri_solve(L, M).T).T
    else:
        X = np.linalg.solve(H, M)
        C = np.linalg.solve(H, X.T).T
    C = (C + C.T) / 2
    if not np.all(np.isfinite(C)):
        return None, 2, n
    return C, 1, n


def _tri_solve(L, B):
    """(L L')^-1 B by forward and back substitution"""
    n = L.shape[0]
    Y = np.array(B, float)
    for i in range(n):
        Y[i] = (Y[i] - L[i, :i] @ Y[:i]) / L[i, i]
    for i in range(n - 1, -1, -1):
        Y[i] = (Y[i] - L[i + 1:, i] @ Y[i + 1:]) / L[i, i]
    return Y


# ---- the status rule
def pair_takes_u(sta, pnum, bad, dist_ok):
    """predict_u_select's `take` (pre3_predictu.h): the pair's u is the prediction's increment"""
    return pnum >= 4 and bad == 0 and dist_ok != 0 and sta == 1


def predict_takes(sta, pnum, bad, dist_ok, status):
    """the prediction takes the pair's covariance as Pn"""
    return bool(pair_takes_u(sta, pnum, bad, dist_ok) and status == 1)


# ---- the committed cases (tests/golden/vo_cov_tolerance.json is measured on exactly these)
def r2q_u(R, T):
    """u = [T; q] with R(q) = R for a proper rotation: q = (a, -b, -c, -d) of R2q, as Calculate_V_Omega_RANSAC_dr_ye.m:40-50 forms it"""
    a = 0.5 * np.sqrt(1 + R[0, 0] + R[1, 1] + R[2, 2])
    S = 4 * a
    b, c, d = (R[1, 2] - R[2, 1]) / S, (R[2, 0] - R[0, 2]) / S, (R[0, 1] - R[1, 0]) / S
    return np.concatenate([T, [a, -b, -c, -d]])


def planted_case(seed, pnum, n_inliers, second_word_only=False):
    """a planted motion of 0.05 rad and 3 - 5 cm with 4 mm point noise on n_inliers points, interleaved with gross outliers the mask leaves out.
    Returns dict(pset1, pset2 (3, pnum), inliers (pnum,) int32, u (7,))"""
    rng = np.random.default_rng(seed)
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    th = 0.05
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    T = rng.uniform(0.03, 0.05, 3) * rng.choice([-1, 1], 3)
    P2 = np.vstack([rng.uniform(-1.5, 1.5, pnum), rng.uniform(-1.0, 1.0, pnum), rng.uniform(1.0, 4.0, pnum)])
    P1 = R @ P2 + T[:, None] + rng.normal(scale=0.004, size=(3, pnum))
    inl = np.zeros(pnum, np.int32)
    if second_word_only:
        pos = 64 + rng.choice(pnum - 64, n_inliers, replace=False)
    else:
        pos = rng.choice(pnum, n_inliers, replace=False)
    inl[pos] = 1
    out = inl == 0
    P1[:, out] += rng.uniform(0.3, 1.0, (3, int(out.sum()))) * rng.choice([-1, 1], (3, int(out.sum())))      # gross outliers
    return dict(pset1=P1, pset2=P2, inliers=inl, u=r2q_u(R, T))


# (seed, pnum, inliers, second word only): inlier counts 3, 4, 63, 64, 65; pnum 4, 65, 128, 129; one case with inliers only in the second mask word
CASES = [(1, 4, 3, False), (2, 4, 4, False), (3, 65, 63, False), (4, 65, 64, False), (5, 65, 65, False), (6, 128, 64, False), (7, 129, 65, False),
         (8, 129, 20, True), (9, 128, 4, False)]


def committed_cases():
    return [planted_case(*c) for c in CASES]
