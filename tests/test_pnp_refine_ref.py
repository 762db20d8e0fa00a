"""CPU suite: tests/pnp_refine_ref.py, the numpy restatement of the Gauss-Newton refinement of an EPnP pose, its covariance and the two maps that carry
it to the prediction's noise -- the Jacobians against finite differences of the functions they linearise, the figures the
design quotes, and the rules."""
import numpy as np
import pytest

import epnp_ref as ref
import pnp_cases as pc
import pnp_refine_ref as gn
import reloc_cases as rc
import reloc_ref as rr

CAM = pc.fixture_cam()
H = 1e-6
RISING_START = np.array([0.78, -0.2, 1.88, -0.04, -0.4, 0.57])          # (tau, omega) from sr_scene(12, 1003)'s EPnP pose: found by a seeded search on the CPU


def central(fun, m):
    cols = []
    for j in range(m):
        d = np.zeros(m)
        d[j] = H
        cols.append((fun(d) - fun(-d)) / (2 * H))
    return np.stack(cols, axis=-1)


@pytest.fixture(scope="module")
def scene():
    Xw, U, _, R, T = pc.sr_scene(12, 1003)
    return Xw, U, R, T


def test_J_against_finite_differences_of_the_projection(scene):
    Xw, _, R, T = scene
    J = gn.jacobians(CAM, R, T, Xw)
    F = central(lambda d: gn.project(CAM, *gn.perturb(R, T, d), Xw)[0], 6)
    assert np.abs(F - J).max() <= 1e-8 * np.abs(J).max()


def test_Jm_against_finite_differences_of_pair_u(scene):
    _, _, R, T = scene
    for Rk, Tk in ((R, T), (pc.rot([2.0, -1.0, 0.5]) @ R, T + [0.3, -2.0, 1.0])):
        F = central(lambda d: ref.pair_u(*gn.perturb(Rk, Tk, d)), 6)
        assert np.abs(F - gn.pair_u_jac(Rk, Tk)).max() < 1e-8


def test_Jd_against_finite_differences_of_the_selection(scene):
    _, _, R, T = scene
    u = ref.pair_u(R, T)
    for x7 in (np.array([0.1, -0.2, 0.3, 0.9, 0.1, -0.3, 0.2]), np.array([1.0, 2.0, -1.0, -0.2, 0.7, 0.1, 0.6])):      # neither normalised; the second flips
        F = central(lambda d: rr.select(x7, 1, 20, 6, u + d)[0], 7)
        Jd = gn.select_jac(x7)
        flip = (gn.qL(x7[3:7] * [1, -1, -1, -1]) @ u[3:7])[0] < 0                  # the hemisphere flip negates the lower block
        Jd[3:] *= -1.0 if flip else 1.0
        assert np.abs(F - Jd).max() < 1e-8


def _noise_checks(Pn):
    """pre3_set_process_noise's three checks"""
    return bool(np.isfinite(Pn).all() and (np.diag(Pn) >= 0).all() and np.array_equal(Pn, Pn.T))


def test_cov7_has_the_null_vector_and_both_noises_pass_the_process_noise_checks(scene):
    Xw, U, _, _ = scene
    e = ref.epnp(Xw, U, CAM)
    g = gn.refine(Xw, U, CAM, e["R"], e["T"], 5)
    z = g["cov"] @ np.concatenate([np.zeros(3), g["u"][3:]])
    assert np.abs(z).max() <= 1e-15 * np.abs(g["cov"]).max()
    x7 = np.array([0.1, -0.2, 0.3, 0.9, 0.1, -0.3, 0.2])
    Pn = gn.noise_from_pose(x7, g["cov"])
    assert _noise_checks(g["cov"]) and _noise_checks(Pn)
    Jd = gn.select_jac(x7)
    assert np.abs(Pn - Jd @ g["cov"] @ Jd.T).max() <= 1e-15 * np.abs(Pn).max()
    assert np.linalg.matrix_rank(g["cov6"]) == 6 and np.linalg.matrix_rank(g["cov"], tol=1e-12 * np.abs(g["cov"]).max()) == 6


# n -> (iterations to a step below 1e-9, median camera-centre error of EPnP and after, mm, mean NEES): the design's table
FIGURES = {6: (5, 9.9, 1.8, 5.65), 8: (5, 4.3, 1.4, 5.93), 12: (4, 2.7, 1.0, 6.05), 40: (3, 1.09, 0.50, 6.07), 185: (3, 0.41, 0.23, 5.94)}


@pytest.mark.parametrize("n", sorted(FIGURES))
def test_two_hundred_scenes(n):
    iters, nees, e0, e1 = 0, [], [], []
    for s in range(200):
        Xw, U, _, R, T = pc.sr_scene(n, 1000 + s)
        e = ref.epnp(Xw, U, CAM)
        g = gn.refine(Xw, U, CAM, e["R"], e["T"], 10, 0.3)
        c = g["cost"]
        assert g["sta"] == 1 and g["zmin"] > 0
        assert (c[1:] <= c[:-1] * (1 + 1e-9)).all(), "a cost rose"
        iters = max(iters, next(i for i, v in enumerate(g["steps"]) if v < 1e-9) + 1)
        d = gn.pose_delta(g["R"], g["T"], R, T)
        nees.append(d @ g["JtJ"] @ d / 0.09)
        e0.append(pc.pose_error(e["R"], e["T"], R, T)[1])
        e1.append(pc.pose_error(g["R"], g["T"], R, T)[1])
    want = FIGURES[n]
    print("n = %d: %d iterations, EPnP %.2f mm, refined %.2f mm, mean NEES %.2f" % (n, iters, 1e3 * np.median(e0), 1e3 * np.median(e1), np.mean(nees)))
    assert iters <= 5 and iters == want[0]
    assert 5.0 <= np.mean(nees) <= 7.0 and abs(np.mean(nees) - want[3]) < 0.01
    assert abs(1e3 * np.median(e0) - want[1]) <= 0.06 * want[1] and abs(1e3 * np.median(e1) - want[2]) <= 0.06 * want[2]


# scene -> (inliers, cost before and after, EPnP's and the refined (degrees, mm), s in px, sigma of the camera centre along the camera's axes in mm): the design's table
RELOC = {"fixture_1": (139, 30.19, 29.06, (0.107, 4.8), (0.078, 0.65), 0.327, (1.4, 1.3, 1.3)),
         "fixture_2": (34, 8.13, 7.09, (0.267, 16.9), (0.077, 5.3), 0.338, (3.0, 2.4, 4.2)),
         "fixture_3": (139, 32.77, 28.85, (0.189, 10.3), (0.084, 2.6), 0.326, (1.2, 1.1, 1.1)),
         "n6": (6, 2.53, 0.013, (0.105, 56.0), (0.021, 1.6), 0.046, (0.8, 0.8, 1.6)),
         "n64_mixed": (48, 16.9, 10.7, (0.095, 6.7), (0.053, 2.0), 0.344, (0.6, 0.6, 1.4)),
         "n65_rho0": (49, 32.4, 9.0, (0.116, 8.2), (0.020, 3.5), 0.312, (0.4, 0.5, 1.5))}


def near(got, want):
    """the table's figures are rounded to two or three digits"""
    return abs(got - want) <= 0.06 * abs(want) + 1e-3


def reloc_refined(name, n_iter=5, sigma_px=0.0):
    w, sc = rc.restated(name), rc.scene(name)
    inl = np.nonzero(w["inliers"])[0]
    if w["pnp"] is None:
        return gn.refine(w["Xw"][inl], w["U"][inl], sc["cam"], np.eye(3), np.zeros(3), n_iter, sigma_px, sta_in=0), w, sc
    return gn.refine(w["Xw"][inl], w["Uu"][inl], sc["cam"], w["pnp"]["R"], w["pnp"]["T"], n_iter, sigma_px, w["sta"]), w, sc


@pytest.mark.parametrize("name", sorted(RELOC))
def test_the_relocalisation_scenes(name):
    g, w, sc = reloc_refined(name)
    want = RELOC[name]
    a0, d0 = rc.pose_error(w["pnp_u"], sc["truth"])
    a1, d1 = rc.pose_error(g["u"], sc["truth"])
    # the camera centre's sigmas along the CAMERA's axes: the tau block of cov6, which is R cov7[0:3, 0:3] R' because dr* = -R' tau
    sig = 1e3 * np.sqrt(np.diag(g["cov6"])[:3])
    assert np.abs(sig - 1e3 * np.sqrt(np.diag(g["R"] @ g["cov"][:3, :3] @ g["R"].T))).max() < 1e-9
    print("%s: %d inliers, cost %.3f -> %.3f, %.3f deg %.2f mm -> %.3f deg %.2f mm, s %.3f px, sigma %s mm" %
          (name, g["n"], g["cost"][0], g["cost"][5], a0, 1e3 * d0, a1, 1e3 * d1, np.sqrt(g["sigma2"]), np.round(sig, 2)))
    assert g["sta"] == 1 and g["n"] == want[0] and g["cost"][5] < g["cost"][0] and d1 < d0
    assert g["steps"][3] < 1e-9, "four iterations"
    assert near(g["cost"][0], want[1]) and near(g["cost"][5], want[2])
    assert near(a0, want[3][0]) and near(1e3 * d0, want[3][1]) and near(a1, want[4][0]) and near(1e3 * d1, want[4][1])
    # each of the three within the rounding of the table's digits: half a unit of the last one, 0.05 mm
    assert near(np.sqrt(g["sigma2"]), want[5]) and all(abs(s - t) <= 0.05 for s, t in zip(sig, want[6])), sig


def test_n5_is_not_computed():
    g, w, _ = reloc_refined("n5")
    assert w["pnp"] is None and g["sta"] == 0 and np.isnan(g["cost"]).all() and np.isnan(g["cov"]).all()


def test_equivariance_under_a_rigid_motion_of_the_world(scene):
    Xw, U, _, _ = scene
    e = ref.epnp(Xw, U, CAM)
    g = gn.refine(Xw, U, CAM, e["R"], e["T"], 5)
    Q, t = pc.rot([0.4, -1.1, 0.7]), np.array([2.0, -3.0, 0.5])
    Xm = Xw @ Q.T + t                                        # Xw' = Q Xw + t: the same camera points under R' = R Q', T' = T - R Q' t
    h = gn.refine(Xm, U, CAM, e["R"] @ Q.T, e["T"] - e["R"] @ Q.T @ t, 5)
    assert h["sta"] == g["sta"] == 1
    assert np.abs(h["R"] - g["R"] @ Q.T).max() < 1e-12 and np.abs(h["T"] - (g["T"] - g["R"] @ Q.T @ t)).max() < 1e-11
    assert np.abs(h["cost"][:6] - g["cost"][:6]).max() < 1e-9 and np.abs(h["cov6"] - g["cov6"]).max() <= 1e-8 * np.abs(g["cov6"]).max()


def test_no_iteration_keeps_the_pose_and_gives_its_covariance(scene):
    Xw, U, _, _ = scene
    e = ref.epnp(Xw, U, CAM)
    g = gn.refine(Xw, U, CAM, e["R"], e["T"], 0, 0.3)
    H, _, c, ok = gn.normal(CAM, e["R"], e["T"], Xw, U)
    assert g["sta"] == 2 and ok and np.array_equal(g["R"], e["R"]) and np.array_equal(g["T"], e["T"])
    assert g["cost"][0] == c and np.isnan(g["cost"][1:]).all() and g["sigma2"] == 0.3 * 0.3
    assert np.abs(g["cov6"] - 0.09 * np.linalg.inv(H)).max() <= 1e-10 * np.abs(g["cov6"]).max()
    assert gn.refine(Xw, U, CAM, e["R"], e["T"], 0)["sigma2"] == c / (2 * len(Xw) - 6)


def test_the_rules_by_hand(scene):
    Xw, U, R, T = scene
    e = ref.epnp(Xw, U, CAM)
    # a rising cost: from RISING_START a plain step overshoots (5e5 -> 3e7 px^2), the start is kept and its covariance given
    R0, T0 = gn.perturb(e["R"], e["T"], RISING_START)
    g = gn.refine(Xw, U, CAM, R0, T0, 1)
    assert g["sta"] == 2 and g["cost"][1] > 10 * g["cost"][0] and np.array_equal(g["R"], R0) and np.array_equal(g["T"], T0)
    assert np.isfinite(g["cov"]).all() and g["sigma2"] == g["cost"][0] / (2 * len(Xw) - 6)
    # a NaN coordinate, a point behind the camera at the pose the call ends on, all points equal (a refused pivot), a pose that was not computed
    bad = Xw.copy()
    bad[3, 1] = np.nan
    assert gn.refine(bad, U, CAM, e["R"], e["T"], 5)["sta"] == -1
    Xb = Xw.copy()
    Xb[2] = e["R"].T @ (np.array([0.1, 0.1, -1.0]) - e["T"])
    gb = gn.refine(Xb, U, CAM, e["R"], e["T"], 5)
    assert gb["sta"] == -1 and np.array_equal(gb["R"], e["R"]) and np.isnan(gb["cov"]).all()
    assert gn.refine(np.tile(Xw[:1], (12, 1)), U, CAM, e["R"], e["T"], 5)["sta"] == -1
    assert gn.refine(Xw, U, CAM, e["R"], e["T"], 5, sta_in=-1)["sta"] == 0 and gn.refine(Xw[:5], U[:5], CAM, e["R"], e["T"], 5)["sta"] == 0
