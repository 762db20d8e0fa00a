"""GPU: the ICP's closed-form covariance (pre3_icp_cov) against the numpy restatement (tests/icp_cov_ref.py).

The scenes are tests/icp_ref.py's surface scenes at (257, 64), (1000, 777), (4097, 1500), seed 1.  Per scene, first the restatement alone: the ICP's
margins hold (only then do two fp64 implementations have to find the same pairs), the covariance's status is 1 and cond(H) < 2000.  Then the ICP runs
through pre3_icp, pre3_icp_cov on its pairs and its u, and the result is compared with the restatement fed the same pairs and u under the gate of
tests/golden/icp_cov_tolerance.json (16 x what the restatement alone moves under reordered sums and jittered transcendentals, relative to the
largest |cov| entry); a second call is bit-equal.
The largest scene's list is also cut to p = 4, 255, 256, 257, 513 and 256 x limits[1] + 1 = 1025 (the scene's 1219 pairs reach it)."""
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np
import pytest

import icp_cov_ref as ref
import icp_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_icp_cov_tolerance as T  # noqa: E402

pytestmark = pytest.mark.gpu
vo = importlib.import_module("3pre_amd.vo")
_lib = importlib.import_module("3pre_amd._lib")
E_ARG = -1
TAB = json.load(open(os.path.join(ROOT, "tests", "golden", "icp_cov_tolerance.json")))
U_ID = np.array([0, 0, 0, 1.0, 0, 0, 0])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check(got, d1, d2, corr, u, name):
    cr, sr, nr = ref.cov(d1, d2, corr, u)
    tol = T.tolerance(TAB, name)
    err = float(np.abs(got["cov"] - cr).max() / np.abs(cr).max()) if got["cov"] is not None else float("nan")
    print(name, "status", got["status"], "n", got["n"], "relative difference %.3e" % err, "gate %.3e" % tol)
    assert (got["status"], got["n"]) == (sr, nr) == (1, len(corr))
    assert np.array_equal(got["cov"], got["cov"].T)
    assert err <= tol


@pytest.mark.parametrize("shape", ref.SHAPES, ids=lambda s: "%dx%d" % s)
def test_against_the_restatement(pre3, shape):
    assert pre3.device_count() >= 1
    s, want = ref.scene(*shape)
    # on the restatement alone, before anything is compared
    assert icp_ref.margins_ok(want) and want["sta"] == 1, want["margins"]
    H = ref.sums(s["data1"], s["data2"], want["corr"], want["u"])[0]
    assert ref.cov(s["data1"], s["data2"], want["corr"], want["u"])[1] == 1 and np.linalg.cond(H) < 2000
    run = vo.icp_with_init(s["data1"], s["data2"], s["res"], s["Rinit"], s["Tinit"])
    assert run["sta"] == 1 and np.array_equal(run["corr"][:, :2], want["corr"][:, :2])
    name = ref.case_name(shape[0], shape[1], want["p"])
    got = vo.icp_cov(s["data1"], s["data2"], run["corr"], run["u"])
    check(got, s["data1"], s["data2"], run["corr"], run["u"], name)
    again = vo.icp_cov(s["data1"], s["data2"], run["corr"], run["u"])
    assert again["status"] == 1 and again["n"] == got["n"] and np.array_equal(bits(again["cov"]), bits(got["cov"]))


def test_the_limits_are_the_ones_the_cases_were_built_for(pre3):
    lim = vo.icp_cov_limits()
    assert (lim["pairs_per_workgroup"], lim["partials_per_thread"]) == (256, 4)
    assert 256 * lim["partials_per_thread"] + 1 == T.EXTRA_TRUNCATIONS[0] < ref.scene(*ref.SHAPES[-1])[1]["p"]       # a scene reaches it


@pytest.mark.parametrize("p", ref.TRUNCATIONS + T.EXTRA_TRUNCATIONS)
def test_truncated_lists(pre3, p):
    n1, n2 = ref.SHAPES[-1]
    s, want = ref.scene(n1, n2)
    corr = want["corr"][:p]
    assert len(corr) == p
    got = vo.icp_cov(s["data1"], s["data2"], corr, want["u"])
    check(got, s["data1"], s["data2"], corr, want["u"], ref.case_name(n1, n2, p))
    assert np.array_equal(bits(vo.icp_cov(s["data1"], s["data2"], corr, want["u"])["cov"]), bits(got["cov"]))


def test_the_status_rule(pre3):
    lib, dptr = _lib.lib, _lib.dptr
    n1, n2 = ref.SHAPES[0]
    s, want = ref.scene(n1, n2)
    corr, u = want["corr"], want["u"]
    assert vo.icp_cov(s["data1"], s["data2"], corr[:3], u) == dict(cov=None, status=0, n=0)
    good = vo.icp_cov(s["data1"], s["data2"], corr, u)
    paired_m, paired_s = set(corr[:, 0].astype(int) - 1), set(corr[:, 1].astype(int) - 1)
    free_m = next(i for i in range(n1) if i not in paired_m)
    free_s = next(i for i in range(n2) if i not in paired_s)
    # a NaN in a point no pair names changes nothing
    d1, d2 = s["data1"].copy(), s["data2"].copy()
    d1[0, free_m], d2[2, free_s] = np.nan, np.inf
    same = vo.icp_cov(d1, d2, corr, u)
    assert same["status"] == 1 and np.array_equal(bits(same["cov"]), bits(good["cov"]))
    # the same NaN in a paired point: status 2, cov untouched
    for side, row in (("model", 0), ("source", 1)):
        d1, d2 = s["data1"].copy(), s["data2"].copy()
        (d1 if side == "model" else d2)[1, int(corr[len(corr) // 2, row]) - 1] = np.nan
        c1, c2 = np.ascontiguousarray(d1.T), np.ascontiguousarray(d2.T)
        ci = np.ascontiguousarray(corr[:, :2].astype(np.int32))
        cov, st, n = np.full(49, -3.0), C.c_int32(-1), C.c_int32(-1)
        assert lib.pre3_icp_cov(0, dptr(c1), n1, dptr(c2), n2, dptr(ci), len(ci), dptr(u), dptr(cov), C.byref(st), C.byref(n)) == 0
        assert (st.value, n.value) == (2, len(ci)) and (cov == -3.0).all(), side
        assert ref.cov(d1, d2, corr, u)[1] == 2
    # three pairs on the optical axis and one more of them, the identity motion, zero residual (tests/test_vo_cov_ref.py's SINGULAR as a list of pairs)
    pts = np.array([[0, 0, 0, 0], [0, 0, 0, 5], [1, 2, 3, 4.0]])
    sing = np.array([[1, 1], [2, 2], [3, 3], [3, 3]])
    assert ref.cov(pts, pts, sing, U_ID)[1] == 2
    assert vo.icp_cov(pts, pts, sing, U_ID) == dict(cov=None, status=2, n=4)
    assert vo.icp_cov(s["data1"], s["data2"], corr, u)["status"] == 1                # the library goes on


def test_an_index_outside_its_cloud_is_an_argument_error(pre3):
    n1, n2 = ref.SHAPES[0]
    s, want = ref.scene(n1, n2)
    for row, col, v in ((0, 0, 0), (5, 0, n1 + 1), (want["p"] - 1, 1, n2 + 1), (7, 1, 0), (3, 0, -4)):
        corr = want["corr"][:, :2].copy()
        corr[row, col] = v
        with pytest.raises(pre3.Pre3Error) as e:
            vo.icp_cov(s["data1"], s["data2"], corr, want["u"])
        assert e.value.code == E_ARG and "pre3_icp_cov" in str(e.value)
