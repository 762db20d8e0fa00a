"""GPU suite: pre3_pnp_refine and pre3_pnp_ransac_refined_seeded (k_pnp_refine, 3pre_amd/csrc/pre3_pnp.hip) against
tests/pnp_refine_ref.py to 16 times what tests/golden/make_pnp_refine_tolerance.py measured between the same header run on the host and that
restatement; the decision exactly (the table leaves no case out); two runs and the two forms bit for bit."""
import ctypes as C
import importlib
import json
import os

import numpy as np
import pytest

import epnp_ref as ref
import pnp_cases as pc
import pnp_refine_ref as gn

pytestmark = pytest.mark.gpu

vo = importlib.import_module("3pre_amd.vo")
_lib = importlib.import_module("3pre_amd._lib")
TAB = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pnp_refine_tolerance.json")))
CAM = pc.fixture_cam()
SIZES = (6, 7, 63, 64, 65, 255, 256, 257, 513)      # the minimum (6 degrees of freedom), the wave's edge, the stride of 256
KEYS = ("pose", "u", "cost", "cov6", "cov7")
_CACHE = {}


def sr_case(n):
    """(Xw, the pixels as sums take them, the same pixels distorted, the restatement's EPnP pose)"""
    if n not in _CACHE:
        Xw, U, _, _, _ = pc.sr_scene(n, 100 + n)
        Ud = ref.distort(CAM, U)
        e = ref.epnp(Xw, U, CAM)
        _CACHE[n] = (Xw, U, Ud, ref.undistort10(CAM, Ud), e["R"], e["T"])
    return _CACHE[n]


def bits(r):
    return np.concatenate([r["R"].ravel(), r["T"], r["u"], r["cost"], r["cov6"].ravel(), r["cov"].ravel(), [r["sigma2"]]]).view(np.uint64).tolist() + \
        [r["sta"], r["n"], r["n_iter"]]


def rel_cov(got, want):
    d = np.sqrt(np.abs(np.diag(want)))
    return float((np.abs(got - want) / np.outer(d, d)).max())


def diffs(h, r):
    fin = np.isfinite(r["cost"])
    assert np.array_equal(np.isfinite(h["cost"]), fin)
    return dict(pose=float(max(np.abs(h["R"] - r["R"]).max(), np.abs(h["T"] - r["T"]).max())), u=float(np.abs(h["u"] - r["u"]).max()),
                cost=float((np.abs(h["cost"][fin] - r["cost"][fin]) / np.maximum(1.0, r["cost"][fin])).max()),
                cov6=rel_cov(h["cov6"], r["cov6"]), cov7=rel_cov(h["cov"], r["cov"]))


def within(df, what):
    print("%s: " % (what,) + "  ".join("%s %.2e (tol %.2e)" % (k, df[k], TAB["tol_" + k]) for k in KEYS))
    return all(df[k] <= TAB["tol_" + k] for k in KEYS)


@pytest.mark.parametrize("n", SIZES)
def test_against_the_restatement(pre3, n):
    Xw, U, Ud, Uu, R0, T0 = sr_case(n)
    for undistort in (False, True):
        for n_iter in (0, 1, 5, 10):
            for sigma in (0.0, 0.3):
                got = vo.pnp_refine(Xw, Ud if undistort else U, CAM, R0, T0, n_iter, sigma, undistort=undistort)
                want = gn.refine(Xw, Uu if undistort else U, CAM, R0, T0, n_iter, sigma)
                assert got["sta"] == want["sta"] == (2 if n_iter == 0 else 1) and (got["n"], got["n_iter"]) == (n, n_iter)
                assert within(diffs(got, want), "n %d undistort %d n_iter %d sigma %.1f" % (n, undistort, n_iter, sigma))
                assert np.array_equal(got["cov"], got["cov"].T) and np.array_equal(got["cov6"], got["cov6"].T)
                assert got["sigma2"] == (sigma * sigma if sigma else got["cost"][n_iter] / (2 * n - 6))
                if n_iter == 0:
                    assert np.array_equal(got["R"], R0) and np.array_equal(got["T"], T0)
                null = got["cov"] @ np.concatenate([np.zeros(3), got["u"][3:]])
                assert np.abs(null).max() <= 1e-14 * np.abs(got["cov"]).max()


@pytest.mark.parametrize("n", (6, 65, 513))
def test_two_runs_are_bit_equal(pre3, n):
    Xw, U, Ud, _, R0, T0 = sr_case(n)
    a, b = (vo.pnp_refine(Xw, Ud, CAM, R0, T0, 5, 0.0, undistort=True) for _ in range(2))
    assert bits(a) == bits(b) and a["sta"] == 1


def test_refusals(pre3):
    Xw, U, _, _, R0, T0 = sr_case(7)
    for kw in (dict(n_iter=-1), dict(n_iter=11), dict(sigma_px=-0.1), dict(sigma_px=np.nan), dict(sigma_px=np.inf)):
        with pytest.raises(pre3.Pre3Error) as e:
            vo.pnp_refine(Xw, U, CAM, R0, T0, **kw)
        assert e.value.code == -1
    with pytest.raises(pre3.Pre3Error) as e:
        vo.pnp_refine(Xw[:5], U[:5], CAM, R0, T0)
    assert e.value.code == -1
    cam, xw, uv, r0, t0, res = _lib.Cam(*CAM), _lib.f64(Xw), _lib.f64(U), _lib.f64(R0), _lib.f64(T0), vo.PnpRefineResult()
    ptr = _lib.dptr
    assert _lib.lib.pre3_pnp_refine(0, C.byref(cam), 0, 7, ptr(xw), ptr(uv), None, ptr(t0), 5, 0.0, C.byref(res)) == -1
    assert _lib.lib.pre3_pnp_refine(0, C.byref(cam), 0, 7, ptr(xw), ptr(uv), ptr(r0), None, 5, 0.0, C.byref(res)) == -1
    assert _lib.lib.pre3_pnp_refine(0, C.byref(cam), 0, 7, ptr(xw), ptr(uv), ptr(r0), ptr(t0), 5, 0.0, None) == -1
    assert _lib.lib.pre3_pnp_refine(0, None, 0, 7, ptr(xw), ptr(uv), ptr(r0), ptr(t0), 5, 0.0, C.byref(res)) == -1


def test_no_covariance_keeps_the_input(pre3):
    Xw, U, _, _, R0, T0 = sr_case(65)
    nan = Xw.copy()
    nan[40, 2] = np.nan
    behind = Xw.copy()
    behind[2] = R0.T @ (np.array([0.1, 0.1, -1.0]) - T0)
    for pts in (nan, behind, np.tile(Xw[:1], (65, 1))):           # a NaN coordinate, a depth <= 0, a refused pivot
        got = vo.pnp_refine(pts, U, CAM, R0, T0, 5)
        assert got["sta"] == -1 == gn.refine(pts, U, CAM, R0, T0, 5)["sta"]
        assert np.array_equal(got["R"], R0) and np.array_equal(got["T"], T0) and np.abs(got["u"] - ref.pair_u(R0, T0)).max() < 1e-15
        assert np.isnan(got["cov"]).all() and np.isnan(got["cov6"]).all() and np.isnan(got["sigma2"])


# ---- behind the RANSAC ----------------------------------------------------------------------------------------------------------------------------------
def pnp_bits(r):
    return np.concatenate([r["R"].ravel(), r["T"], r["u"], r["err"]]).view(np.uint64).tolist() + [r["best"], r["sta"], r["n"], r["n_support"]]


# tests/pnp_cases.py's ransac_scene(n_hyp, n) has tables for 1, 64, 65 and 700 hypotheses: 65 over 40 and over 200 correspondences, and 700
@pytest.mark.parametrize("n_hyp,n", ((65, 40), (65, 200), (700, 40)))
@pytest.mark.parametrize("undistort", (False, True))
def test_the_ransac_form(pre3, n_hyp, n, undistort):
    sc = pc.ransac_scene(n_hyp, n=n)
    U = ref.distort(sc["cam"], sc["U"]) if undistort else sc["U"]
    args = (sc["Xw"], U, sc["cam"], n_hyp, pc.THR_PX, sc["seed"], sc["seq"])
    plain = vo.pnp_ransac_seeded(*args, undistort=undistort, hyp_results=True)
    got = vo.pnp_ransac_refined_seeded(*args, undistort=undistort, hyp_results=True, n_iter=5, sigma_px=0.0)
    assert pnp_bits(got) == pnp_bits(plain) and [pnp_bits(a) for a in got["hyp"]] == [pnp_bits(b) for b in plain["hyp"]]
    for k in ("support", "state", "inliers", "draws"):
        assert np.array_equal(got[k], plain[k]), k
    inl = np.nonzero(got["inliers"])[0]
    alone = vo.pnp_refine(sc["Xw"][inl], U[inl], sc["cam"], got["R"], got["T"], 5, 0.0, undistort=undistort)
    assert bits(got["ref"]) == bits(alone), "ref differs from pre3_pnp_refine on the gathered inliers"
    Uu = ref.undistort10(sc["cam"], U) if undistort else U
    want = gn.refine(sc["Xw"][inl], Uu[inl], sc["cam"], got["R"], got["T"], 5, 0.0)
    assert got["sta"] == 1 and got["ref"]["sta"] == want["sta"] == 1 and got["ref"]["n"] == len(inl) == got["n_support"]
    assert within(diffs(got["ref"], want), "ransac n_hyp %d n %d undistort %d" % (n_hyp, n, undistort))
    e0, e1 = pc.pose_error(got["R"], got["T"], sc["R"], sc["T"])[1], pc.pose_error(got["ref"]["R"], got["ref"]["T"], sc["R"], sc["T"])[1]
    print("camera centre against the planted pose: EPnP %.2f mm, refined %.2f mm" % (1e3 * e0, 1e3 * e1))


def test_a_refit_that_was_not_computed_is_not_refined(pre3):
    sc = pc.ransac_scene(65)
    got = vo.pnp_ransac_refined_seeded(sc["Xw"], sc["U"], sc["cam"], 65, 1e-9, sc["seed"], sc["seq"])        # nothing within a nanopixel: support below six
    assert got["sta"] == 0 and got["n_support"] < 6 and got["ref"]["sta"] == 0
    assert np.isnan(got["ref"]["cost"]).all() and np.isnan(got["ref"]["cov"]).all() and np.array_equal(got["ref"]["u"], got["u"])
    with pytest.raises(pre3.Pre3Error) as e:
        vo.pnp_ransac_refined_seeded(sc["Xw"], sc["U"], sc["cam"], 65, 2.0, sc["seed"], sc["seq"], n_iter=11)
    assert e.value.code == -1
