"""GPU: the covariance of a VO pair's increment from its inliers (k_vo_cov: pre3_vo_cov, pre3_vo_pair_cov_seeded).

pre3_vo_cov on the committed cases of tests/vo_cov_ref.py -- planted motions whose inliers are interleaved with masked-out gross outliers, inlier counts
3, 4, 63, 64, 65, pnum 4, 65, 128, 129, one case with inliers in the second mask word only -- against the numpy restatement under the gate of
tests/golden/vo_cov_tolerance.json (16 x the floor the restatement alone moves by, relative to the largest |cov| entry), a second call bit-equal; the
status rule's corners; and pre3_vo_pair_cov_seeded on the 36 x 45 pairs of tests/vo_pair_cases.py: every shared output byte for byte
pre3_vo_pair_seeded's, cov byte for byte pre3_vo_cov's on the call's own pset, inlier list and u."""
import importlib
import json
import os

import numpy as np
import pytest

import vo_cov_ref as ref
import vo_pair_cases as vp
from test_vo_cov_ref import SINGULAR

pytestmark = pytest.mark.gpu
srm = importlib.import_module("3pre_amd.sr4000")
vo = importlib.import_module("3pre_amd.vo")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATE = json.load(open(os.path.join(ROOT, "tests", "golden", "vo_cov_tolerance.json")))["tol"]
SEED, SEQ = 5, 0
SMALL_PAIRS = [n for n, spec in vp.CASES.items() if spec[0] == vp.SMALL]
PAIR_KEYS = ("rot", "trans", "euler", "u", "error_mean", "error_std", "dist", "sta", "n_support", "n_iterations", "best", "cnum", "state", "inliers",
             "pset1", "pset2", "draws", "capped", "match", "pnum", "rst")


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def references():
    """the restatement on the committed cases, once"""
    return [(c, ref.cov(c["pset1"], c["pset2"], c["inliers"], c["u"])) for c in ref.committed_cases()]


@pytest.mark.parametrize("i", range(len(ref.CASES)), ids=["seed%d_p%d_in%d%s" % (s, p, n, "_word2" if w else "") for s, p, n, w in ref.CASES])
def test_vo_cov_against_the_restatement_under_the_gate(pre3, references, i):
    c, (cr, sr_, nr) = references[i]
    got = vo.vo_cov(c["pset1"], c["pset2"], c["u"], c["inliers"])
    assert (got["status"], got["n_inliers"]) == (sr_, nr) == (1, ref.CASES[i][2])
    err = np.abs(got["cov"] - cr).max() / np.abs(cr).max()
    print(ref.CASES[i], "cov err %.3g of max |cov| (gate %.3g); sigma_T %.3g m" % (err, GATE, np.sqrt(np.diag(got["cov"])[:3]).mean()))
    assert err <= GATE
    assert same_bytes(got["cov"], got["cov"].T)
    again = vo.vo_cov(c["pset1"], c["pset2"], c["u"], c["inliers"])
    assert same_bytes(again["cov"], got["cov"]) and again["n_inliers"] == got["n_inliers"]
    # the mask matters: with the outliers counted the covariance is another one
    if c["inliers"].sum() < c["inliers"].size:
        every = vo.vo_cov(c["pset1"], c["pset2"], c["u"], None)
        assert every["n_inliers"] == c["inliers"].size and (every["status"] != 1 or not same_bytes(every["cov"], got["cov"]))


def test_the_status_rule_on_the_device(pre3, references):
    lib = importlib.import_module("3pre_amd._lib")
    import ctypes as C
    # three points on the optical axis, the identity motion: H's last pivot is exactly zero -> unusable, cov untouched
    p1, p2 = np.ascontiguousarray(SINGULAR["pset1"].T), np.ascontiguousarray(SINGULAR["pset2"].T)
    cov, st, n = np.full((7, 7), -3.0), C.c_int32(-1), C.c_int32(-1)
    lib.check(lib.lib.pre3_vo_cov(0, 4, lib.dptr(p1), lib.dptr(p2), lib.dptr(SINGULAR["inliers"]), lib.dptr(SINGULAR["u"]), lib.dptr(cov), C.byref(st), C.byref(n)))
    assert (st.value, n.value) == (2, 3) and np.all(cov == -3.0)
    # a NaN inlier coordinate -> unusable; the same NaN on a masked-out point is not looked at
    c = {k: np.array(v, copy=True) for k, v in references[2][0].items()}
    k_in, k_out = int(np.flatnonzero(c["inliers"])[5]), int(np.flatnonzero(c["inliers"] == 0)[0])
    c["pset2"][1, k_in] = np.nan
    assert vo.vo_cov(c["pset1"], c["pset2"], c["u"], c["inliers"])["status"] == 2
    c["pset2"][1, k_in] = references[2][0]["pset2"][1, k_in]
    c["pset1"][2, k_out] = np.nan
    ok = vo.vo_cov(c["pset1"], c["pset2"], c["u"], c["inliers"])
    assert ok["status"] == 1 and same_bytes(ok["cov"], vo.vo_cov(references[2][0]["pset1"], references[2][0]["pset2"], c["u"], c["inliers"])["cov"])
    # fewer than four points: not computed
    r = vo.vo_cov(c["pset1"][:, :3], c["pset2"][:, :3], c["u"], None)
    assert (r["status"], r["n_inliers"], r["cov"]) == (0, 0, None)
    # the .m file's signature: every point an inlier
    c0 = references[4][0]
    Rm = ref.rot(c0["u"][3:] / np.linalg.norm(c0["u"][3:]))
    got = vo.cov_pose_shift_calc(c0["pset1"], c0["pset2"], Rm, c0["u"][:3])
    want = ref.cov(c0["pset1"], c0["pset2"], None, np.r_[c0["u"][:3], vo.R2q(Rm)])[0]
    assert np.abs(got - want).max() <= GATE * np.abs(want).max()
    with pytest.raises(ValueError):
        vo.cov_pose_shift_calc(SINGULAR["pset1"][:, :3], SINGULAR["pset2"][:, :3], np.eye(3), np.zeros(3))


def resident(c):
    f1, f2 = srm.SrFrame(c["rows"], c["cols"]), srm.SrFrame(c["rows"], c["cols"])
    f1.load(c["fr1"], 1); f2.load(c["fr2"], 1)
    f1.keypoints(c["frm1"], c["des1"], 1); f2.keypoints(c["frm2"], c["des2"], 1)
    return f1, f2


@pytest.mark.parametrize("name", SMALL_PAIRS + ["no_consensus"])
def test_vo_pair_cov_seeded_is_the_pair_call_plus_vo_cov(pre3, name):
    c = dict(vp.make_pair(36, 45, 33, 65, 12, seed=40, outliers=1.0, drop1=2), expect_pnum=12) if name == "no_consensus" else vp.case(name)
    f1, f2 = resident(c)
    with f1, f2:
        base = vo.vo_pair_seeded(f1, f2, SEED, SEQ)
        got = vo.vo_pair_cov_seeded(f1, f2, SEED, SEQ)
        again = vo.vo_pair_cov_seeded(f1, f2, SEED, SEQ)
        after = vo.vo_pair_seeded(f1, f2, SEED, SEQ)             # (the plain call's layout of the work block, behind a call with the other one)
    assert base["pnum"] == c["expect_pnum"]
    for k in PAIR_KEYS:
        assert same_bytes(np.asarray(got[k]), np.asarray(base[k])), k
        assert same_bytes(np.asarray(after[k]), np.asarray(base[k])), k
    print(name, "pnum sta n_support cov_status =", got["pnum"], got["sta"], got["n_support"], got["cov_status"])
    assert again["cov_status"] == got["cov_status"]
    if got["pnum"] < 4 or got["sta"] != 1:
        assert got["cov_status"] == 0 and got["cov"] is None          # pnum < 4, no consensus (sta = 4): not computed
        return
    assert got["cov_status"] in (1, 2)
    alone = vo.vo_cov(got["pset1"], got["pset2"], got["u"], got["inliers"])
    assert alone["status"] == got["cov_status"] and alone["n_inliers"] == got["n_support"]
    if got["cov_status"] == 1:
        assert same_bytes(got["cov"], alone["cov"]) and same_bytes(again["cov"], got["cov"])
        cr, sr_, _ = ref.cov(got["pset1"], got["pset2"], got["inliers"], got["u"])
        if sr_ == 1 and np.linalg.cond(ref.sums(got["pset1"], got["pset2"], got["inliers"], got["u"])[0]) < 1e4:      # (the gate is measured below that)
            assert np.abs(got["cov"] - cr).max() <= GATE * np.abs(cr).max()
