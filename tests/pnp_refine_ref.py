"""The Gauss-Newton refinement of an EPnP pose on the reprojection error, its covariance and the two maps that carry it to the prediction, restated in
numpy over tests/epnp_ref.py (3pre_amd/csrc/pre3_pnpref.h and reloc_noise_from_pose of pre3_reloc.h).  The project's own follow-up
of sections 35 and 36: the reference's efficient_pnp_gauss.m:191-225 refines over the betas against control-point distances and yields no covariance.

    pose (R, T) with Xc = R Xw + T; perturbation d = (tau, omega) on the camera side: R <- E R, T <- E T + tau, E = exp([omega]x)
    r_i = [u - (Cx + f x/z); v - (Cy + f y/z)],  J_i = D [I3, -[Xc]x],  D = f [1/z 0 -x/z^2; 0 1/z -y/z^2]
    step: (J'J) d = J'r by a 6 x 6 Cholesky whose pivots must lie above 7 eps times their own diagonal entry
    taken iff n_iter >= 1, everything finite, every z > 0 at the refined pose and cost[n_iter] < cost[0]; else the input pose is kept
    cov6 = s^2 (J'J)^-1 at the pose the call ends on; s^2 = sigma_px^2, or cost / (2 n - 6) when sigma_px == 0
    cov7 = Jm cov6 Jm' for u = pair_u(R, T);  Pn = Jd cov7 Jd' for the increment reloc_select makes of u at x_k_k
"""
import numpy as np

import epnp_ref as ref

MAX_ITER = 10
EPS = 2.0 ** -52
SMALL_ANGLE2 = 1e-8           # theta^2 below this: the series of sin(t)/t and (1 - cos t)/t^2 to the t^4 term (their next terms are below 1e-19 of the value)
STA_NOT_COMPUTED, STA_TAKEN, STA_KEPT, STA_NO_COV = 0, 1, 2, -1


def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def exp_so3(w):
    w = np.asarray(w, np.float64)
    t2 = float(w @ w)
    if t2 < SMALL_ANGLE2:
        a, b = 1.0 - t2 / 6.0 + t2 * t2 / 120.0, 0.5 - t2 / 24.0 + t2 * t2 / 720.0
    else:
        t = np.sqrt(t2)
        a, b = np.sin(t) / t, (1.0 - np.cos(t)) / t2
    K = skew(w)
    return np.eye(3) + a * K + b * (K @ K)


def perturb(R, T, d):
    E = exp_so3(d[3:6])
    return E @ R, E @ T + np.asarray(d[:3], np.float64)


def project(cam, R, T, Xw):
    Xc = Xw @ R.T + T
    with np.errstate(all="ignore"):
        return np.column_stack([cam[1] + cam[0] * Xc[:, 0] / Xc[:, 2], cam[2] + cam[0] * Xc[:, 1] / Xc[:, 2]]), Xc


def jacobians(cam, R, T, Xw):
    """(n, 2, 6): d projection / d (tau, omega) at d = 0"""
    f = float(cam[0])
    Xc = Xw @ R.T + T
    x, y, z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
    J = np.zeros((len(Xw), 2, 6))
    with np.errstate(all="ignore"):
        J[:, 0] = f * np.column_stack([1 / z, 0 * z, -x / z ** 2, -x * y / z ** 2, 1 + x * x / z ** 2, -y / z])
        J[:, 1] = f * np.column_stack([0 * z, 1 / z, -y / z ** 2, -(1 + y * y / z ** 2), x * y / z ** 2, x / z])
    return J


def normal(cam, R, T, Xw, U):
    """(J'J, J'r, r'r, every z > 0 and everything finite)"""
    P, Xc = project(cam, R, T, Xw)
    r = (U - P).reshape(-1)
    J = jacobians(cam, R, T, Xw).reshape(-1, 6)
    with np.errstate(all="ignore"):
        H, g, c = J.T @ J, J.T @ r, float(r @ r)
    ok = bool((Xc[:, 2] > 0).all() and np.isfinite(H).all() and np.isfinite(g).all() and np.isfinite(c))
    return H, g, c, ok


def chol6(H):
    """the lower factor, or None where a pivot is not above 7 eps times its own diagonal entry"""
    n = len(H)
    L = np.zeros((n, n))
    ok = True
    with np.errstate(all="ignore"):
        for j in range(n):
            d = H[j, j] - L[j, :j] @ L[j, :j]
            if not d > 7 * EPS * H[j, j]:
                ok = False
            L[j, j] = np.sqrt(d)
            for i in range(j + 1, n):
                L[i, j] = (H[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    return L if ok else None


def chol_solve(L, b):
    y = np.linalg.solve(L, b)
    return np.linalg.solve(L.T, y)


def qL(p):
    """the left-multiplication matrix of qProd: qProd(p, q) = qL(p) q"""
    a, b, c, d = p
    return np.array([[a, -b, -c, -d], [b, a, -d, c], [c, d, a, -b], [d, -c, b, a]])


def pair_u_jac(R, T):
    """Jm (7, 6): d pair_u(E R, E T + tau) / d (tau, omega) at 0"""
    u = ref.pair_u(R, T)
    Jm = np.zeros((7, 6))
    Jm[:3, :3] = -R.T
    Jm[3:, 3:] = -0.5 * qL(u[3:7])[:, 1:4]
    return Jm


def sym(C):
    return (C + C.T) / 2


def cov_u(R, T, cov6):
    Jm = pair_u_jac(R, T)
    return sym(Jm @ cov6 @ Jm.T)


def q2R(q):
    """reloc_q2R (pre3_reloc.h): the homogeneous quadratic form, not normalised"""
    a, b, c, d = q
    return np.array([[a * a + b * b - c * c - d * d, 2 * b * c - 2 * a * d, 2 * b * d + 2 * a * c],
                     [2 * b * c + 2 * a * d, a * a - b * b + c * c - d * d, 2 * c * d - 2 * a * b],
                     [2 * b * d - 2 * a * c, 2 * c * d + 2 * a * b, a * a - b * b - c * c + d * d]])


def select_jac(x7):
    """Jd (7, 7): d reloc_select's increment / d u at x_k_k's pose (the hemisphere flip negates the lower block: Jd C Jd' does not see it)"""
    q = np.asarray(x7[3:7], np.float64)
    Jd = np.zeros((7, 7))
    Jd[:3, :3] = q2R(q).T
    Jd[3:, 3:] = qL(q * np.array([1.0, -1.0, -1.0, -1.0])) / (q @ q)
    return Jd


def noise_from_pose(x7, cov7):
    """reloc_noise_from_pose, operation for operation (products and sums in the header's order, none fused): equal bits"""
    Jd = select_jac(x7)
    q = np.asarray(x7[3:7], np.float64)
    n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
    Jd[3:, 3:] = qL(q * np.array([1.0, -1.0, -1.0, -1.0]))
    for i in range(3, 7):
        for k in range(3, 7):
            Jd[i, k] = Jd[i, k] / n2
    C = np.asarray(cov7, np.float64).reshape(7, 7)
    T1, M = np.zeros((7, 7)), np.zeros((7, 7))
    for i in range(7):
        for k in range(7):
            s = 0.0
            for t in range(7):
                s = s + Jd[i, t] * C[t, k]
            T1[i, k] = s
    for i in range(7):
        for k in range(7):
            s = 0.0
            for t in range(7):
                s = s + T1[i, t] * Jd[k, t]
            M[i, k] = s
    return (M + M.T) / 2


def refine(Xw, U, cam, R0, T0, n_iter, sigma_px=0.0, sta_in=1):
    """dict(R, T, u, cost (11, NaN beyond n_iter), cov6, cov (7 x 7), sigma2, sta, n, n_iter, steps (the largest |component| of every step), zmin)"""
    Xw, U = np.asarray(Xw, np.float64).reshape(-1, 3), np.asarray(U, np.float64).reshape(-1, 2)
    R0, T0 = np.asarray(R0, np.float64).reshape(3, 3), np.asarray(T0, np.float64).reshape(3)
    n = len(Xw)
    out = dict(R=R0.copy(), T=T0.copy(), u=ref.pair_u(R0, T0), cost=np.full(MAX_ITER + 1, np.nan), cov6=np.full((6, 6), np.nan), cov=np.full((7, 7), np.nan),
               sigma2=np.nan, sta=STA_NOT_COMPUTED, n=n, n_iter=n_iter, steps=[], zmin=np.nan)
    if sta_in not in (1, 2) or n < 6:
        return out
    R, T, ok = R0.copy(), T0.copy(), True
    with np.errstate(all="ignore"):
        for k in range(n_iter):
            H, g, c, _ = normal(cam, R, T, Xw, U)
            out["cost"][k] = c
            L = chol6(H)
            if L is None:
                ok = False
                d = np.zeros(6)
            else:
                d = chol_solve(L, g)
            out["steps"].append(float(np.abs(d).max()))
            R, T = perturb(R, T, d)
            ok = ok and bool(np.isfinite(R).all() and np.isfinite(T).all() and np.isfinite(c))
        H, g, c, front = normal(cam, R, T, Xw, U)
        out["cost"][n_iter] = c
        taken = n_iter >= 1 and ok and front and c < out["cost"][0]
        if not taken:
            R, T = R0.copy(), T0.copy()
            H, g, c, front = normal(cam, R, T, Xw, U)
        out["zmin"] = float((Xw @ R.T + T)[:, 2].min())
        L = chol6(H) if front else None
        if L is None:
            out["sta"] = STA_NO_COV
            return out
        Li = np.linalg.inv(L)
        s2 = sigma_px * sigma_px if sigma_px > 0 else c / (2 * n - 6)
        cov6 = sym(s2 * (Li.T @ Li))
        cov7 = cov_u(R, T, cov6)
        if not (np.isfinite(cov6).all() and np.isfinite(cov7).all()):
            out["sta"] = STA_NO_COV
            return out
    out.update(R=R, T=T, u=ref.pair_u(R, T), cov6=cov6, cov=cov7, sigma2=s2, sta=STA_TAKEN if taken else STA_KEPT, JtJ=H)
    return out


def pose_delta(R, T, Rt, Tt):
    """the (tau, omega) that carries (Rt, Tt) to (R, T): E = R Rt', tau = T - E Tt"""
    E = R @ Rt.T
    c = np.clip((np.trace(E) - 1) / 2, -1, 1)
    th = np.arccos(c)
    v = np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]]) / 2
    w = v if th < 1e-8 else v * th / np.sin(th)
    return np.concatenate([T - E @ Tt, w])
