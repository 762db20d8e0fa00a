"""CPU suite: tests/epnp_ref.py, the numpy restatement of the reference's efficient_pnp.m (dimensions 1 to 3) that the device code is held to
 -- pinned on the solver's own input file, on the properties that hold it up without MATLAB, and on what separates its two
eigensolvers.  Also: the cases the GPU tests run leave out at most 2 % of a RANSAC's hypotheses, never the winner or the runner-up."""
import json
import os

import numpy as np
import pytest

import epnp_ref as ref
import pnp_cases as pc
import pnp_draws_ref as dr

HERE = os.path.dirname(os.path.abspath(__file__))
TAB = json.load(open(os.path.join(HERE, "golden", "pnp_tolerance.json")))


@pytest.fixture(scope="module")
def fx():
    d, kat = pc.fixture()
    return d, kat


def test_the_fixture_is_data_only_and_small(fx):
    d, kat = fx
    assert os.path.getsize(os.path.join(HERE, "golden", "epnp_input_data_noise.npz")) < 10 * 1024
    assert sorted(d) == ["A", "Rt", "Xcam", "Ximg_pix", "Ximg_pix_true", "Xworld"]
    assert d["Xworld"].shape == (50, 3) and d["Ximg_pix"].shape == (50, 2) and d["A"].shape == (3, 3) and d["Rt"].shape == (4, 4)
    assert np.array_equal(d["A"], [[800, 0, 320], [0, 800, 240], [0, 0, 1]])
    assert 12 < np.sqrt(((d["Ximg_pix"] - d["Ximg_pix_true"]) ** 2).sum(axis=1)).mean() < 14          # the file's noise: 13 px mean


def test_the_true_pixels_reproduce_the_camera_points(fx):
    d, kat = fx
    r = ref.epnp(d["Xworld"], d["Ximg_pix_true"], kat["cam"])
    got = d["Xworld"] @ r["R"].T + r["T"]
    print("|R Xw + T - Xcam| %.3e, err %s" % (np.abs(got - d["Xcam"]).max(), r["err"]))
    assert r["best"] == 0 and r["sta"] == 1 and np.isnan(r["err"][2])
    assert np.abs(got - d["Xcam"]).max() <= 1e-10 and np.abs(r["Xc"] - d["Xcam"]).max() <= 1e-10
    assert r["err"][0] <= 1e-10


def test_the_noisy_pixels_against_the_recorded_answer(fx):
    d, kat = fx
    r = ref.epnp(d["Xworld"], d["Ximg_pix"], kat["cam"])
    want = kat["noisy"]
    assert r["best"] == want["best"] == 0 and r["sta"] == want["sta"] == 1
    assert abs(want["err"][0] - 13.85) < 0.01 and abs(want["err"][1] - 25.87) < 0.01 and want["err"][2] is None and np.isnan(r["err"][2])
    for k in (0, 1):
        assert abs(r["err"][k] - want["err"][k]) <= 1e-6 * want["err"][k]


def test_dimension_three_is_reached_on_purpose():
    r = ref.epnp(*pc.outlier_sta2())
    assert r["dim3"] and r["best"] == 0 and r["sta"] == 2 and np.abs(r["err"] - [57.4, 75.3, 65.7]).max() < 0.05
    g = ref.epnp(*pc.dim3_good())                                    # seed pc.DIM3_GOOD_SEED = 47, found by pc.search_dim3_good() on the CPU
    assert g["dim3"] and g["best"] == 2 and g["sta"] == 1 and g["err"][2] < 15 and min(g["err"][:2]) > 22


CASES = ["fixture_noisy", "outlier_sta2", "dim3_good", "sr_6", "sr_65", "sr_257"]


@pytest.mark.parametrize("name", CASES)
def test_the_rotation_is_proper(name):
    r = ref.epnp(*pc.tolerance_cases()[name])
    for R, T, _, _ in r["sols"]:
        assert np.abs(R.T @ R - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1) < 1e-12


@pytest.mark.parametrize("name", CASES)
def test_negating_a_kernel_vector_changes_nothing(name):
    Xw, U, cam = pc.tolerance_cases()[name]
    r = ref.epnp(Xw, U, cam)
    assert all((s[2][:, 2] > 0).all() for s in r["sols"]), "no answer of mixed depth signs among these cases"
    for k in range(4):
        flip = [1, 1, 1, 1]
        flip[k] = -1
        f = ref.epnp(Xw, U, cam, flip=flip)
        assert np.abs(f["R"] - r["R"]).max() < 1e-12 and np.abs(f["T"] - r["T"]).max() < 1e-12 and (f["best"], f["sta"]) == (r["best"], r["sta"])
        fin = np.isfinite(r["err"])
        assert np.abs(f["err"][fin] - r["err"][fin]).max() <= 1e-9 * np.abs(r["err"][fin]).max()


def test_an_answer_of_mixed_depth_signs_does_depend_on_the_sign():
    """why fix_signs exists: the z < 0 rule negates a mixed-sign Xc into another mixed-sign Xc, so the vector's sign decides which of the two comes out"""
    Xw, U, cam = pc.behind()
    r = ref.epnp(Xw, U, cam)
    assert (r["sols"][0][2][:, 2] < 0).sum() == 29, "the rule fired: 29 of the 30 depths came out negative"
    f = ref.epnp(Xw, U, cam, flip=[-1, 1, 1, 1])
    assert (f["sols"][0][2][:, 2] < 0).sum() == 1 and abs(f["err"][0] - r["err"][0]) > 1


@pytest.mark.parametrize("seed", [165, 166])
def test_the_pose_follows_a_rigid_motion_of_the_camera(seed):
    """On noise-free pixels: the world moved by (Q, t) -- Xw' = Q'(Xw - t) -- under the same pixels needs R' = R Q, T' = T + R t.  Only the clean case is
    an assertion: the control points are not centred on the data, so with noisy pixels the two problems are different least-squares systems whose
    answers differ by the noise's conditioning, which bounds nothing."""
    cam = pc.fixture_cam()
    Xw, U, _, _, _ = pc.sr_scene(65, seed, noise=0.0)
    Q, t = pc.rot([0.3, -0.2, 0.5]), np.array([0.4, -0.1, 0.25])
    a, b = ref.epnp(Xw, U, cam), ref.epnp((Xw - t) @ Q, U, cam)
    assert a["sta"] == b["sta"] == 1
    assert np.abs(b["R"] - a["R"] @ Q).max() < 1e-9 and np.abs(b["T"] - (a["T"] + a["R"] @ t)).max() < 1e-9


@pytest.mark.parametrize("name", list(pc.tolerance_cases()))
def test_no_committed_case_sits_on_the_edge_of_the_sign_rule(name):
    r = ref.epnp(*pc.tolerance_cases()[name])
    assert r["sign_margin"] > 1e-3, "the two largest entries of a kernel vector are 1e-3 apart at least: no eigensolver orders them differently"


def test_the_pair_convention():
    Xw, U, _, R, T = pc.sr_scene(20, 3)
    u = ref.pair_u(R, T)
    q = u[3:]
    a, b, c, d = q
    Rq = np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)], [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                   [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]])
    Xc = Xw @ R.T + T
    assert np.abs(Xw - (Xc @ Rq.T + u[:3])).max() < 1e-12, "pset1 = rot pset2 + trans with pset1 = Xw, pset2 = Xc"


def test_the_two_pixel_maps_invert_each_other():
    g = np.random.default_rng(4)
    U = np.column_stack([g.uniform(0, 176, 200), g.uniform(0, 144, 200)])
    assert np.abs(ref.undistort10(pc.SR_CAM, ref.distort(pc.SR_CAM, U)) - U).max() < 1e-10
    moved = np.linalg.norm(ref.undistort10(pc.SR_CAM, np.array([[1.0, 1.0]])) - 1.0)
    print("the corner pixel moves by %.2f px" % moved)
    assert 5 < moved < 40


@pytest.mark.parametrize("name", list(pc.tolerance_cases()))
def test_jacobi_against_lapack(name):
    Xw, U, cam = pc.tolerance_cases()[name]
    M = ref.compute_M(U, ref.alphas(Xw), ref.cam_A(cam))
    w, V, sweeps = ref.jacobi12(M.T @ M)
    wl = np.linalg.eigh(M.T @ M)[0]
    assert sweeps <= 10 and np.abs(V.T @ V - np.eye(12)).max() < 1e-13
    assert np.abs(w - wl).max() <= 1e-12 * wl.max()
    a, b = ref.epnp(Xw, U, cam, eig="jacobi"), ref.epnp(Xw, U, cam)
    assert (a["best"], a["sta"], a["dim3"]) == (b["best"], b["sta"], b["dim3"])
    own = name in ("dim3_good", "fixture_true")
    assert max(np.abs(a["R"] - b["R"]).max(), np.abs(a["T"] - b["T"]).max()) <= (16 * TAB["cases"][name]["pose"] if own else TAB["tol_pose"])


def test_the_draw_rule():
    for n in (6, 7, 400):
        t = dr.draw_pnp(5, 2, n, 300)
        assert t.shape == (300, 6) and t.min() >= 0 and t.max() < n and all(len(set(r.tolist())) == 6 for r in t)
    assert np.array_equal(np.sort(dr.draw_pnp(5, 2, 6, 50), axis=1), np.tile(np.arange(6), (50, 1)))
    t = dr.draw_pnp(9, 0, 12, 6000)
    cnt = np.bincount(t.ravel(), minlength=12)
    assert np.abs(cnt / cnt.sum() - 1 / 12).max() < 0.006            # 36000 picks: sigma = 0.0015 per cell


@pytest.mark.parametrize("n_hyp", list(pc.RANSAC_SEEDS))
def test_the_ransac_cases_keep_clear_of_their_edges(n_hyp):
    """a bad seed fails here, not on the GPU: at most 2 % of the hypotheses within the guard of an edge, never the winner or the runner-up"""
    sc = pc.ransac_scene(n_hyp)
    assert len(sc["bad"]) == 10
    rs = ref.ransac(sc["Xw"], sc["U"], sc["cam"], sc["draws"], pc.THR_PX)
    skip, tie = ref.guard_excluded(rs, pc.THR_PX, TAB["guard"] * max(1.0, pc.THR_PX))
    assert not tie and skip.sum() <= 0.02 * n_hyp and not skip[rs["order"][0]] and (n_hyp == 1 or not skip[rs["order"][1]])
    assert TAB["hypotheses"][str(n_hyp)]["decide_differently"] == 0
    if n_hyp >= 64:
        assert rs["res"]["sta"] == 1 and not set(rs["inliers"].tolist()) & set(sc["bad"].tolist())
        ang, dist = pc.pose_error(rs["res"]["R"], rs["res"]["T"], sc["R"], sc["T"])
        assert ang < 1.0 and dist < 0.03
        j = ref.ransac(sc["Xw"], sc["U"], sc["cam"], sc["draws"][:64], pc.THR_PX, eig="jacobi")
        l = ref.ransac(sc["Xw"], sc["U"], sc["cam"], sc["draws"][:64], pc.THR_PX)
        assert np.array_equal(j["support"], l["support"]) and j["winner"] == l["winner"]
