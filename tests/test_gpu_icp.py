"""GPU: the dense ICP (pre3_icp) against the numpy restatement of icp_with_init.m (tests/icp_ref.py).

Per scene, first the restatement alone: the smallest |D - 2 res| over all iterations, the smallest gap between a source point's best and second-best d,
the smallest gap between the two best claimants of a model index and the smallest distance of a |e2 - e1| from res / 10000 must all be >= 1e-9 -- only
then do the integer results of two fp64 implementations have to agree.  Then: the iteration counts of both phases, p of every iteration, the final
pairs and the status identical; R, t, Rtot, ttot, u, error, D and the registered data2 within max(1e-12, 100 x spread), the spread being what the order
of the restatement's own sums moves on that scene (tests/golden/icp_tolerance.json, written by tests/golden/make_icp_tolerance.py).
Shapes: (3, 3), (257, 64), (1000, 777), (4097, 1500); from pre3_icp_limits one model chunk - 1 / + 0 / + 1 and two chunks + 1 against one source tile
- 1 / + 0 / + 1.  Three seeds each.  The restatement of a scene runs once per session and is shared."""
import ctypes as C
import functools
import importlib
import json
import os
import sys

import numpy as np
import pytest

import icp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_icp_tolerance as T  # noqa: E402

pytestmark = pytest.mark.gpu
vo = importlib.import_module("3pre_amd.vo")
_lib = importlib.import_module("3pre_amd._lib")
E_ARG, E_NUMERIC = -1, -5
TAB = json.load(open(os.path.join(ROOT, "tests", "golden", "icp_tolerance.json")))
LIMIT_SHAPES = R.limit_shapes(TAB["limits"]["src_tile"], TAB["limits"]["chunk"])
FLOATS = ("R", "t", "Rtot", "ttot", "u", "error", "data2")


@functools.lru_cache(maxsize=None)
def scene(n1, n2, seed):
    s = R.surface_scene(n1, n2, seed)
    return s, R.icp_with_init(s["data1"], s["data2"], s["res"], s["Rinit"], s["Tinit"])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_same_bits(a, b):
    for k in FLOATS + ("corr", "log"):
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    for k in ("sta", "p", "iters1", "iters2", "n_model", "n_source"):
        assert a[k] == b[k], k


def compare(got, want, tol, name):
    """integers identical, floats within tol; every figure printed before it is asserted"""
    worst = {k: float(np.abs(np.asarray(got[k]) - np.asarray(want[k])).max()) for k in FLOATS}
    if want["p"] and got["p"] == want["p"]:
        worst["D"] = float(np.abs(got["corr"][:, 2] - want["corr"][:, 2]).max())
        worst["log_e"] = float(np.abs(got["log"][:, 2] - want["log"][:, 2]).max()) if got["log"].shape == want["log"].shape else float("nan")
    print(name, "iterations", got["iters1"], got["iters2"], "p", got["p"], "sta", got["sta"], "tol %.2e" % tol, {k: "%.2e" % v for k, v in worst.items()})
    assert (got["sta"], got["iters1"], got["iters2"]) == (want["sta"], want["iters1"], want["iters2"])
    assert [int(v) for v in got["log"][:, 1]] == want["ps"] and [int(v) for v in got["log"][:, 0]] == [int(v) for v in want["log"][:, 0]]
    assert got["p"] == want["p"] and np.array_equal(got["corr"][:, :2], want["corr"][:, :2])
    for k, v in worst.items():
        assert v <= tol, (k, v, tol)


def test_the_limits_are_the_ones_the_scenes_were_built_for(pre3):
    lim = vo.icp_limits()
    assert (lim["src_tile"], lim["chunk"]) == (TAB["limits"]["src_tile"], TAB["limits"]["chunk"]) and lim["iter_cap"] == 62


@pytest.mark.parametrize("seed", R.SEEDS)
@pytest.mark.parametrize("shape", R.FIXED_SHAPES + LIMIT_SHAPES, ids=lambda s: "%dx%d" % s)
def test_against_the_restatement(pre3, shape, seed):
    assert pre3.device_count() >= 1
    s, want = scene(shape[0], shape[1], seed)
    assert R.margins_ok(want), want["margins"]                      # on the restatement alone, before anything is compared
    name = T.scene_name(shape[0], shape[1], seed)
    got = vo.icp_with_init(s["data1"], s["data2"], s["res"], s["Rinit"], s["Tinit"])
    assert (got["n_model"], got["n_source"]) == shape
    compare(got, want, T.tolerance(TAB, name), name)


def test_a_second_call_gives_the_same_bits(pre3):
    s, _ = scene(1000, 777, 1)
    a = vo.icp_with_init(s["data1"], s["data2"], s["res"], s["Rinit"], s["Tinit"])
    b = vo.icp_with_init(s["data1"], s["data2"], s["res"], s["Rinit"], s["Tinit"])
    assert_same_bits(a, b)
    s, _ = scene(LIMIT_SHAPES[3][0], LIMIT_SHAPES[3][1], 2)          # two chunks + 1: the merge of the partials
    assert_same_bits(vo.icp_with_init(s["data1"], s["data2"], s["res"], s["Rinit"], s["Tinit"]),
                     vo.icp_with_init(s["data1"], s["data2"], s["res"], s["Rinit"], s["Tinit"]))


def test_no_seed_is_the_identity_seed(pre3):
    s, _ = scene(257, 64, 1)
    a = vo.icp_with_init(s["data1"], s["data2"], s["res"])
    b = vo.icp_with_init(s["data1"], s["data2"], s["res"], np.eye(3), np.zeros(3))
    assert_same_bits(a, b)
    assert np.array_equal(a["Rtot"], a["R"]) and np.array_equal(a["ttot"], a["t"])


def test_fewer_than_three_pairs_is_status_two(pre3):
    model = np.array([[0.0, 1.0, 0.0, 5.0], [0.0, 0.0, 1.0, 5.0], [1.0, 1.0, 1.0, 9.0]])
    src = np.concatenate([model[:, :2] + 0.001, [[40.0], [40.0], [40.0]]], axis=1)
    want = R.icp_with_init(model, src, 0.01)
    got = vo.icp_with_init(model, src, 0.01)
    assert want["sta"] == R.FEW == got["sta"] and (got["iters1"], got["iters2"], got["p"]) == (1, 0, 2)
    assert np.array_equal(got["R"], np.eye(3)) and not got["t"].any() and got["error"] == 1000000.0
    assert np.array_equal(got["corr"], want["corr"]) and got["log"].tolist() == [[1.0, 2.0, 0.0]]
    assert np.array_equal(got["data2"], src)                          # nothing was applied
    # a later iteration: the transform accumulated so far stays
    s, _ = scene(257, 64, 1)
    far = s["data2"].copy()
    far[:, 3:] += 50.0                                                # three sources near the surface, the rest nowhere
    w2 = R.icp_with_init(s["data1"], far, s["res"], s["Rinit"], s["Tinit"])
    g2 = vo.icp_with_init(s["data1"], far, s["res"], s["Rinit"], s["Tinit"])
    assert (g2["sta"], g2["iters1"], g2["iters2"], g2["p"]) == (w2["sta"], w2["iters1"], w2["iters2"], w2["p"])
    assert np.abs(g2["R"] - w2["R"]).max() <= 1e-12 and np.abs(g2["t"] - w2["t"]).max() <= 1e-12


@pytest.mark.parametrize("where", ["model", "source"])
@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_a_non_finite_coordinate_is_a_numeric_error(pre3, where, value):
    s, _ = scene(257, 64, 1)
    d1, d2 = s["data1"].copy(), s["data2"].copy()
    (d1 if where == "model" else d2)[1, -1] = value
    with pytest.raises(pre3.Pre3Error) as e:
        vo.icp_with_init(d1, d2, s["res"], s["Rinit"], s["Tinit"])
    assert e.value.code == E_NUMERIC and "pre3_icp" in str(e.value)
    good = vo.icp_with_init(s["data1"], s["data2"], s["res"], s["Rinit"], s["Tinit"])       # the library goes on
    assert good["sta"] == 1


def test_argument_errors_are_refused_before_anything_is_queued(pre3):
    lib, dptr = _lib.lib, _lib.dptr
    pts = np.ascontiguousarray(scene(257, 64, 1)[0]["data1"].T)
    r = vo.IcpResult()
    r.sta = -7
    cases = (("n1 < 3", lambda: lib.pre3_icp(0, dptr(pts), 2, dptr(pts), 10, 0.1, None, None, C.byref(r), None, None, None)),
             ("n2 < 3", lambda: lib.pre3_icp(0, dptr(pts), 10, dptr(pts), 2, 0.1, None, None, C.byref(r), None, None, None)),
             ("res 0", lambda: lib.pre3_icp(0, dptr(pts), 10, dptr(pts), 10, 0.0, None, None, C.byref(r), None, None, None)),
             ("res < 0", lambda: lib.pre3_icp(0, dptr(pts), 10, dptr(pts), 10, -0.1, None, None, C.byref(r), None, None, None)),
             ("res nan", lambda: lib.pre3_icp(0, dptr(pts), 10, dptr(pts), 10, float("nan"), None, None, C.byref(r), None, None, None)),
             ("res inf", lambda: lib.pre3_icp(0, dptr(pts), 10, dptr(pts), 10, float("inf"), None, None, C.byref(r), None, None, None)),
             ("null model", lambda: lib.pre3_icp(0, None, 10, dptr(pts), 10, 0.1, None, None, C.byref(r), None, None, None)),
             ("null limits", lambda: lib.pre3_icp_limits(None)))
    for what, fn in cases:
        assert fn() == E_ARG, what
        assert b"pre3_icp" in lib.pre3_last_error(), what
    assert r.sta == -7
    # every output may be NULL
    assert lib.pre3_icp(0, dptr(pts), 257, dptr(pts), 64, 0.1, None, None, None, None, None, None) == 0
