"""GPU suite: pre3_epnp and the EPnP RANSAC (3pre_amd/csrc/pre3_pnp.hip) against tests/epnp_ref.py over LAPACK, to 16 times
what tests/golden/make_pnp_tolerance.py measured between the same header run on the host and that restatement; decisions exactly, outside the guard."""
import importlib
import json
import os

import numpy as np
import pytest

import epnp_ref as ref
import pnp_cases as pc
import pnp_draws_ref as dr

pytestmark = pytest.mark.gpu

vo = importlib.import_module("3pre_amd.vo")
_lib = importlib.import_module("3pre_amd._lib")
TAB = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pnp_tolerance.json")))


def rel(got, want):
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())


def close(got, want, name=None):
    """the device's answer against the restatement's: decisions equal, pose and err within 16 x the recorded floors (a case with a floor of its own:
    16 x that)"""
    own = TAB["cases"].get(name) if name in ("dim3_good", "fixture_true") else None
    tol_pose = 16 * own["pose"] if own else TAB["tol_pose"]
    tol_err = 16 * own["err"] if own else TAB["tol_err"]
    fin = np.isfinite(want["err"])
    dp = max(np.abs(got["R"] - want["R"]).max(), np.abs(got["T"] - want["T"]).max())
    de = rel(got["err"][fin], want["err"][fin])
    print("%s: pose %.3e (tol %.3e)  err %.3e (tol %.3e)  err %s best %d sta %d" % (name, dp, tol_pose, de, tol_err, got["err"], got["best"], got["sta"]))
    assert (got["best"], got["sta"]) == (want["best"], want["sta"])
    assert np.array_equal(np.isfinite(got["err"]), fin)
    assert dp <= tol_pose and de <= tol_err
    assert np.abs(got["u"] - ref.pair_u(got["R"], got["T"])).max() < 1e-12


def bits(r):
    return np.concatenate([r["R"].ravel(), r["T"], r["u"], r["err"]]).view(np.uint64).tolist() + [r["best"], r["sta"], r["n"], r["n_support"]]


@pytest.mark.parametrize("name", list(pc.tolerance_cases()))
def test_epnp_against_the_restatement(name):
    Xw, U, cam = pc.tolerance_cases()[name]
    want = ref.epnp(Xw, U, cam)
    R, T, Xc, best1, got = vo.efficient_pnp(Xw, U, cam)
    close(got, want, name)
    assert best1 == got["best"] + 1 and got["n"] == len(Xw) == got["n_support"]
    assert np.abs(Xc - (Xw @ R.T + T)).max() == 0
    if name == "outlier_sta2":
        assert got["sta"] == 2 and np.isfinite(got["err"]).all()
    if name == "dim3_good":
        assert got["sta"] == 1 and got["best"] == 2 and got["err"][2] < 20
    assert bits(vo.efficient_pnp(Xw, U, cam)[4]) == bits(got), "two runs differ"


def test_epnp_at_the_largest_n():
    n = vo.pnp_limits()["max_n"]
    assert n >= 144 * 176 and vo.pnp_limits()["max_hyp"] == 700
    Xw, U, _, R0, T0 = pc.sr_scene(n, 5)
    got = vo.efficient_pnp(Xw, U, pc.fixture_cam())[4]
    close(got, ref.epnp(Xw, U, pc.fixture_cam()), "sr_%d" % n)
    with pytest.raises(_lib.Pre3Error) as e:
        vo.efficient_pnp(np.zeros((n + 1, 3)), np.zeros((n + 1, 2)), pc.fixture_cam())
    assert e.value.code == -1


def test_undistorted_pixels_give_the_pose_of_the_clean_ones():
    cam = pc.SR_CAM
    Xw, U, _, _, _ = pc.sr_scene(65, 21, cam, fov=(0.3, 0.25))
    Ud = ref.distort(cam, U)
    assert np.abs(Ud - U).max() > 3, "the distortion moves pixels by several px on this set"
    clean = vo.efficient_pnp(Xw, U, cam, undistort=False)[4]
    und = vo.efficient_pnp(Xw, Ud, cam, undistort=True)[4]
    raw = vo.efficient_pnp(Xw, Ud, cam, undistort=False)[4]
    dp = max(np.abs(und["R"] - clean["R"]).max(), np.abs(und["T"] - clean["T"]).max())
    print("undistort: pose %.3e (tol %.3e); without it %.3e" % (dp, TAB["tol_pose"], np.abs(raw["T"] - clean["T"]).max()))
    assert (und["best"], und["sta"]) == (clean["best"], clean["sta"]) and dp <= TAB["tol_pose"]
    assert np.abs(raw["T"] - clean["T"]).max() > 1e-3
    close(und, ref.epnp(Xw, ref.undistort10(cam, Ud), cam), "undistort")


def test_one_point_behind_the_camera_fires_the_sign_rule():
    Xw, U, cam = pc.behind()
    want = ref.epnp(Xw, U, cam)
    assert (want["Xc"][:, 2] < 0).sum() == 29, "the rule fired in the restatement: the whole Xc was negated"
    close(vo.efficient_pnp(Xw, U, cam)[4], want, "behind")


@pytest.mark.parametrize("where", ["Xw", "U"])
def test_a_non_finite_coordinate_gives_sta_minus_one(where):
    Xw, U, _, _, _ = pc.sr_scene(70, 41)
    Xw, U = Xw.copy(), U.copy()
    if where == "Xw":
        Xw[69, 1] = np.nan
    else:
        U[3, 0] = np.inf
    got = vo.efficient_pnp(Xw, U, pc.fixture_cam())[4]
    assert got["sta"] == -1 and np.array_equal(got["u"], [0, 0, 0, 1, 0, 0, 0])
    assert ref.epnp(Xw, U, pc.fixture_cam())["sta"] == -1


def test_epnp_refusals():
    Xw, U, _, _, _ = pc.sr_scene(8, 1)
    cam = pc.fixture_cam()
    for bad in (lambda: vo.efficient_pnp(Xw[:5], U[:5], cam), lambda: vo.efficient_pnp(Xw, U, [0.0] + list(cam[1:])),
                lambda: vo.efficient_pnp(Xw, U, [-1.0] + list(cam[1:]))):
        with pytest.raises(_lib.Pre3Error) as e:
            bad()
        assert e.value.code == -1


# ---- the RANSAC ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_hyp", list(pc.RANSAC_SEEDS))
def test_ransac_against_the_restatement(n_hyp):
    sc = pc.ransac_scene(n_hyp)
    want = ref.ransac(sc["Xw"], sc["U"], sc["cam"], sc["draws"], pc.THR_PX)
    got = vo.pnp_ransac(sc["Xw"], sc["U"], sc["cam"], sc["draws"], pc.THR_PX, hyp_results=True)
    skip, tie = ref.guard_excluded(want, pc.THR_PX, TAB["guard"] * max(1.0, pc.THR_PX))
    assert not tie and not skip[want["order"][0]] and (n_hyp == 1 or not skip[want["order"][1]]) and skip.sum() <= 0.02 * n_hyp
    keep = ~skip
    print("n_hyp %d: %d left out; winner %d support %d" % (n_hyp, skip.sum(), want["winner"], want["support"][want["winner"]]))
    assert np.array_equal(got["support"][keep], want["support"][keep]) and np.array_equal(got["state"][keep], want["state"][keep])
    for h in np.nonzero(keep)[0]:
        assert got["hyp"][h]["best"] == want["hyp"][h]["best"] and got["hyp"][h]["n_support"] == want["support"][h]
    assert np.array_equal(got["inliers"].astype(bool), want["flags"][want["winner"]]), "another winner, or other flags"
    assert got["n_support"] == want["support"][want["winner"]] == got["n"]
    if want["res"] is None:
        assert got["sta"] == 0
        return
    close(got, want["res"], "ransac_%d" % n_hyp)
    # the restatement's own distance from the truth, measured here on the CPU, times two
    ang0, dist0 = pc.pose_error(want["res"]["R"], want["res"]["T"], sc["R"], sc["T"])
    ang, dist = pc.pose_error(got["R"], got["T"], sc["R"], sc["T"])
    print("truth: restatement %.4f deg %.4f m, device %.4f deg %.4f m" % (ang0, dist0, ang, dist))
    if n_hyp >= 64:
        assert ang0 < 1.0 and dist0 < 0.03
        assert ang <= 2 * ang0 and dist <= 2 * dist0


@pytest.mark.parametrize("n", [6, 7, 400])
def test_the_draw_table_against_its_restatement(n):
    Xw, U, _, _, _ = pc.sr_scene(n, 50 + n)
    got = vo.pnp_ransac_seeded(Xw, U, pc.fixture_cam(), 130, pc.THR_PX, seed=77, seq=9)
    want = dr.draw_pnp(77, 9, n, 130)
    assert np.array_equal(got["draws"], want)
    assert all(len(set(r.tolist())) == 6 for r in got["draws"]) and got["draws"].min() >= 0 and got["draws"].max() < n
    again = vo.pnp_ransac(Xw, U, pc.fixture_cam(), got["draws"], pc.THR_PX)
    assert bits(again) == bits(got) and np.array_equal(again["support"], got["support"]) and np.array_equal(again["state"], got["state"])
    assert np.array_equal(again["inliers"], got["inliers"])


def test_ransac_refusals_and_the_empty_support():
    sc = pc.ransac_scene(64)
    d = sc["draws"].copy()
    d[5, 3] = d[5, 0]
    cam = sc["cam"]
    for bad in (lambda: vo.pnp_ransac(sc["Xw"], sc["U"], cam, d, 2.0), lambda: vo.pnp_ransac(sc["Xw"], sc["U"], cam, sc["draws"], 0.0),
                lambda: vo.pnp_ransac(sc["Xw"], sc["U"], cam, sc["draws"], np.nan), lambda: vo.pnp_ransac_seeded(sc["Xw"], sc["U"], cam, 701, 2.0, seed=1),
                lambda: vo.pnp_ransac_seeded(sc["Xw"], sc["U"], cam, 0, 2.0, seed=1),
                lambda: vo.pnp_ransac(sc["Xw"], sc["U"], cam, np.where(sc["draws"] == 0, 40, sc["draws"]), 2.0)):
        with pytest.raises(_lib.Pre3Error) as e:
            bad()
        assert e.value.code == -1
    # no hypothesis reaches six inliers: nothing is refitted
    got = vo.pnp_ransac(sc["Xw"], sc["U"], cam, sc["draws"], 1e-4)
    want = ref.ransac(sc["Xw"], sc["U"], cam, sc["draws"], 1e-4)
    assert want["support"].max() < 6 and got["support"].max() < 6
    assert got["sta"] == 0 and got["n_support"] == got["support"].max() and np.array_equal(got["u"], [0, 0, 0, 1, 0, 0, 0])
