"""CPU: the numpy truth of the marginal readers (pre3_get_landmarks / pre3_get_marginal) that tests/test_gpu_marginals.py
checks the device against.  inversedepth2cartesian.m (the point), inversedepth_2_cartesian.m:58-65 (its Jacobian J), inversedepth_2_cartesian.m:36-56
(the linearity index), plots_complete.m:208-237 (what is read of P: each landmark's own block, J P_ii J' for an inverse-depth one)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util  # noqa: E402


def m_vec(theta, phi):
    """m.m: the unit ray of azimuth theta, elevation phi"""
    cphi = np.cos(phi)
    return np.array([cphi * np.sin(theta), -np.sin(phi), cphi * np.cos(theta)])


def id2cart(y):
    """inversedepth2cartesian.m:29-38 for one 6-vector [x y z theta phi rho]"""
    return y[:3] + (1.0 / y[5]) * m_vec(y[3], y[4])


def id_jacobian(y):
    """inversedepth_2_cartesian.m:63-65: J = [I3, dm_dtheta / rho, dm_dphi / rho, -m / rho^2] (3 x 6)"""
    theta, phi, rho = y[3], y[4], y[5]
    dmt = np.array([np.cos(phi) * np.cos(theta), 0.0, -np.cos(phi) * np.sin(theta)])
    dmp = np.array([-np.sin(phi) * np.sin(theta), -np.cos(phi), -np.sin(phi) * np.cos(theta)])
    return np.hstack([np.eye(3), (dmt / rho)[:, None], (dmp / rho)[:, None], (-m_vec(theta, phi) / rho ** 2)[:, None]])


def linearity_index(X, P, o):
    """inversedepth_2_cartesian.m:41-56 for the inverse-depth landmark at 0-based offset o (the camera position is X(1:3))"""
    std_rho = np.sqrt(P[o + 5, o + 5])
    rho = X[o + 5]
    std_d = std_rho / rho ** 2
    x_c1, x_c2 = X[o:o + 3], X[:3]
    p = id2cart(X[o:o + 6])
    d_c2p = np.linalg.norm(p - x_c2)
    cos_alpha = ((p - x_c1) @ (p - x_c2)) / (np.linalg.norm(p - x_c1) * np.linalg.norm(p - x_c2))
    return 4 * std_d * cos_alpha / d_c2p


def landmark_truth(X, P, types, off):
    """what pre3_get_landmarks returns for every landmark: xyz (N, 3), cov_xyz (N, 3, 3), cov_native (N, 6, 6), linearity (N,)"""
    N = len(types)
    xyz, cxyz, cnat, lin = np.zeros((N, 3)), np.zeros((N, 3, 3)), np.zeros((N, 6, 6)), np.zeros(N)
    for i in range(N):
        o = int(off[i])
        if int(types[i]) == 0:
            B = P[o:o + 6, o:o + 6]
            J = id_jacobian(X[o:o + 6])
            xyz[i], cxyz[i], cnat[i], lin[i] = id2cart(X[o:o + 6]), J @ B @ J.T, B, linearity_index(X, P, o)
        else:
            xyz[i], cxyz[i], lin[i] = X[o:o + 3], P[o:o + 3, o:o + 3], -1.0
            cnat[i, :3, :3] = P[o:o + 3, o:o + 3]
    return {"xyz": xyz, "cov_xyz": cxyz, "cov_native": cnat, "linearity": lin}


def test_jacobian_matches_central_differences():
    rng = np.random.default_rng(3)
    d = util.load_sr4000()
    X = d["x_k_k"]
    for i in rng.choice(d["N"], 12, replace=False):
        y = X[13 + 6 * i:19 + 6 * i].copy()
        J = id_jacobian(y)
        Jn = np.zeros((3, 6))
        for c in range(6):
            h = 1e-6 * max(1.0, abs(y[c]))
            e = np.zeros(6)
            e[c] = h
            Jn[:, c] = (id2cart(y + e) - id2cart(y - e)) / (2 * h)
        assert np.abs(J - Jn).max() < 1e-6 * max(1.0, np.abs(J).max()), (i, np.abs(J - Jn).max())
    # a near and a far landmark, away from the fixture's values
    for y in (np.array([0.1, -0.2, 0.3, 0.4, -0.3, 2.0]), np.array([-1.0, 0.5, 2.0, -2.5, 1.1, 0.05])):
        Jn = np.stack([(id2cart(y + e) - id2cart(y - e)) / 2e-7 for e in np.eye(6) * 1e-7], 1)
        assert np.abs(id_jacobian(y) - Jn).max() < 1e-5 * np.abs(Jn).max()


def test_linearity_index_on_the_sr4000_fixture():
    """the index as the .m file spells it, against the same quantity written from the geometry: 4 sigma_d cos(alpha) / d, sigma_d the depth's
    standard deviation sigma_rho / rho^2, alpha the angle at the point between the ray from its anchor and the ray from the camera"""
    d = util.load_sr4000()
    for X, P in ((d["x_k_k"], d["p_k_k"]), (d["x_k_km1"], d["p_k_km1"])):
        idx = np.array([linearity_index(X, P, 13 + 6 * i) for i in range(d["N"])])
        assert np.isfinite(idx).all()
        for i in range(0, d["N"], 7):
            o = 13 + 6 * i
            p = id2cart(X[o:o + 6])
            u, v = p - X[o:o + 3], p - X[:3]
            alpha = np.arctan2(np.linalg.norm(np.cross(u, v)), u @ v)
            ref = 4 * (np.sqrt(P[o + 5, o + 5]) / X[o + 5] ** 2) * np.cos(alpha) / np.linalg.norm(v)
            assert abs(idx[i] - ref) <= 1e-12 * abs(ref) + 1e-300, (i, idx[i], ref)
    # landmark_truth agrees with the per-landmark functions and reads only each landmark's own block
    X, P = d["x_k_k"], d["p_k_k"]
    types, off = np.zeros(d["N"], int), 13 + 6 * np.arange(d["N"])
    t = landmark_truth(X, P, types, off)
    assert np.array_equal(t["cov_native"][5], P[43:49, 43:49]) and t["linearity"][5] == linearity_index(X, P, 43)
    cx = t["cov_xyz"]
    assert np.abs(cx - cx.transpose(0, 2, 1)).max() <= 1e-15 * np.abs(cx).max()
    assert (np.linalg.eigvalsh(cx) > 0).all()
