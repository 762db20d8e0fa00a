"""GPU: the dense ICP on two resident SR4000 frames (pre3_icp_frames, pre3_icp_pair_seeded).

The frames are tests/icp_frame_cases.py's: a smooth surface seen from two poses, a few raw pixels NaN and a few behind the camera.
  stride 8 (about 400 sources against the full model): against the numpy restatement (tests/icp_ref.py) on the same compacted points, under
      tests/test_gpu_icp.py's rules -- margins first, integers identical, floats within max(1e-12, 100 x spread) of tests/golden/icp_tolerance.json;
  stride 1 (25 thousand against 25 thousand) is not compared with the restatement, which would take minutes: it is bit-equal to pre3_icp fed the
      compacted points (device against device), bit-equal to itself on a second run, and ends with status 1;
  pre3_icp_pair_seeded: the pair's outputs bit-equal to pre3_vo_pair_seeded's, the ICP's bit-equal to pre3_icp_frames fed that pair's rot, trans; a
      pair with fewer than four matches gives ICP status 0 and leaves every ICP output untouched."""
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np
import pytest

import icp_frame_cases as F
import icp_ref as R
import vo_pair_cases as vp
from test_gpu_icp import assert_same_bits, compare
from test_gpu_vo_pair import SEED, SEQ, assert_same_result, resident
from test_sr_frame_ref import same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_icp_tolerance as T  # noqa: E402

pytestmark = pytest.mark.gpu
srm = importlib.import_module("3pre_amd.sr4000")
vo = importlib.import_module("3pre_amd.vo")
_lib = importlib.import_module("3pre_amd._lib")
E_ARG, E_STATE = -1, -4
TAB = json.load(open(os.path.join(ROOT, "tests", "golden", "icp_tolerance.json")))


@pytest.fixture(scope="module")
def frames():
    sc = F.make_frames()
    f1, f2 = srm.SrFrame(F.ROWS, F.COLS), srm.SrFrame(F.ROWS, F.COLS)
    f1.load(sc["fr1"], F.MODE); f2.load(sc["fr2"], F.MODE)
    x1, y1, z1, _ = f1.planes(); x2, y2, z2, _ = f2.planes()
    yield sc, f1, f2, (x1, y1, z1, x2, y2, z2)
    f1.close(); f2.close()


def check_pixels(out, cl):
    assert (out["n_model"], out["n_source"]) == (cl["model"].shape[1], cl["source"].shape[1])
    m, s = out["corr"][:, 0].astype(int) - 1, out["corr"][:, 1].astype(int) - 1
    assert np.array_equal(out["corr_pix"][:, 0], cl["mpix"][m]) and np.array_equal(out["corr_pix"][:, 1], cl["spix"][s])


def test_stride_8_against_the_restatement(pre3, frames):
    sc, f1, f2, planes = frames
    cl = F.clouds(*planes, 8)
    ref = F.restated_clouds(sc, 8)                                  # the scene the tolerance was measured on
    assert same_bits(cl["model"], ref["model"]) and same_bits(cl["source"], ref["source"])
    n_bad = 9 * (len(F.NAN_PIXELS) + len(F.BEHIND_PIXELS))
    assert F.ROWS * F.COLS - n_bad <= cl["model"].shape[1] < F.ROWS * F.COLS and 380 <= cl["source"].shape[1] <= 18 * 22
    want = R.icp_with_init(cl["model"], cl["source"], F.RES, sc["Rinit"], sc["Tinit"])
    assert R.margins_ok(want), want["margins"]
    got = vo.icp_frames(f1, f2, F.RES, sc["Rinit"], sc["Tinit"], stride=8)
    check_pixels(got, cl)
    compare(got, want, T.tolerance(TAB, "frames_stride8"), "frames_stride8")
    assert_same_bits(got, vo.icp_with_init(cl["model"], cl["source"], F.RES, sc["Rinit"], sc["Tinit"]))


def test_stride_1_is_the_stateless_call_on_the_compacted_points_bit_for_bit(pre3, frames):
    sc, f1, f2, planes = frames
    cl = F.clouds(*planes, 1)
    got = vo.icp_frames(f1, f2, F.RES, sc["Rinit"], sc["Tinit"], stride=1)
    print("stride 1: n", got["n_model"], got["n_source"], "iterations", got["iters1"], got["iters2"], "p", got["p"], "error", got["error"])
    assert got["sta"] == 1
    check_pixels(got, cl)
    assert_same_bits(got, vo.icp_with_init(cl["model"], cl["source"], F.RES, sc["Rinit"], sc["Tinit"]))
    assert_same_bits(got, vo.icp_frames(f1, f2, F.RES, sc["Rinit"], sc["Tinit"], stride=1))
    assert np.abs(got["data2"] - R.apply(got["R"], got["t"], R.apply(sc["Rinit"], sc["Tinit"], cl["source"]))).max() < 1e-9


def test_the_pair_call_is_the_pair_followed_by_icp_frames(pre3, orc):
    c = vp.case("p13")
    f1, f2, _, _ = resident(c)
    with f1, f2:
        base = vo.vo_pair_seeded(f1, f2, SEED, SEQ)
        pair, icp = vo.icp_pair_seeded(f1, f2, SEED, SEQ, stride=2, res=0.2)
        assert base["sta"] == 1 and base["pnum"] == 13
        assert np.array_equal(pair["match"], base["match"]) and pair["pnum"] == base["pnum"]
        assert_same_result(pair, base)
        direct = vo.icp_frames(f1, f2, 0.2, base["rot"], base["trans"], stride=2)
        print("pair: icp sta", icp["sta"], "iterations", icp["iters1"], icp["iters2"], "p", icp["p"])
        assert icp["sta"] in (1, 2) and icp["iters1"] >= 1
        assert_same_bits(icp, direct)
        assert np.array_equal(icp["corr_pix"], direct["corr_pix"])
        again_pair, again = vo.icp_pair_seeded(f1, f2, SEED, SEQ, stride=2, res=0.2)
        assert_same_result(again_pair, base)
        assert_same_bits(again, icp)


def test_fewer_than_four_matches_leave_the_icp_outputs_untouched(pre3, orc):
    lib, dptr = _lib.lib, _lib.dptr
    c = vp.case("p3")
    f1, f2, _, _ = resident(c)
    with f1, f2:
        base = vo.vo_pair_seeded(f1, f2, SEED, SEQ)
        pair, icp = vo.icp_pair_seeded(f1, f2, SEED, SEQ, stride=2, res=0.2)
        assert base["pnum"] == 3 and pair["pnum"] == 3 and pair["sta"] == 4 and np.array_equal(pair["match"], base["match"])
        assert icp == dict(sta=0)
        r, vres, pn = vo.IcpResult(), vo.VoResult(), C.c_int32(0)
        C.memset(C.byref(r), 0x5A, C.sizeof(r))
        corr, pix, d2, log = np.full((900, 3), -3.0), np.full((900, 2), -3, np.int32), np.full((900, 3), -3.0), np.full((62, 3), -3.0)
        assert lib.pre3_icp_pair_seeded(f1._h, f2._h, 1.5, SEED, SEQ, 2, 0.2, C.byref(pn), None, None, None, None, None, None, None, None, C.byref(vres),
                                        C.byref(r), dptr(corr), dptr(pix), dptr(d2), dptr(log)) == 0
        assert pn.value == 3 and vres.sta == 4 and r.sta == 0
        assert bytes(r)[:256] == b"\x5a" * 256 and r.p == 0x5A5A5A5A
        assert (corr == -3.0).all() and (pix == -3).all() and (d2 == -3.0).all() and (log == -3.0).all()


def test_refusals_leave_the_handles_usable(pre3, frames):
    lib = _lib.lib
    sc, f1, f2, _ = frames
    r = vo.IcpResult()
    r.sta = -7

    def call(p, q, stride=8, res=F.RES):
        return lib.pre3_icp_frames(p, q, stride, res, None, None, C.byref(r), None, None, None, None)

    with srm.SrFrame(F.ROWS, F.COLS + 1) as other, srm.SrFrame(F.ROWS, F.COLS) as empty:
        other.load({k: np.asfortranarray(np.pad(v, ((0, 0), (0, 1)), mode="edge")) for k, v in sc["fr2"].items()}, F.MODE)
        for what, fn, want in (("null prev", lambda: call(None, f2._h), E_ARG), ("null cur", lambda: call(f1._h, None), E_ARG),
                               ("prev == cur", lambda: call(f1._h, f1._h), E_ARG), ("sizes differ", lambda: call(f1._h, other._h), E_ARG),
                               ("stride 0", lambda: call(f1._h, f2._h, 0), E_ARG), ("stride < 0", lambda: call(f1._h, f2._h, -2), E_ARG),
                               ("res 0", lambda: call(f1._h, f2._h, 8, 0.0), E_ARG), ("res nan", lambda: call(f1._h, f2._h, 8, float("nan"))
                                                                                      , E_ARG),
                               ("res inf", lambda: call(f1._h, f2._h, 8, float("inf")), E_ARG), ("nothing loaded", lambda: call(f1._h, empty._h), E_STATE)):
            rc = fn()
            assert rc == want, (what, rc)
            assert want == E_STATE or b"pre3_icp_frames" in lib.pre3_last_error(), what
    assert r.sta == -7
    a = vo.icp_frames(f1, f2, F.RES, sc["Rinit"], sc["Tinit"], stride=16)
    assert call(f1._h, f2._h, 16) == 0 and r.sta in (1, 2)           # every array output NULL, no seed
    assert_same_bits(a, vo.icp_frames(f1, f2, F.RES, sc["Rinit"], sc["Tinit"], stride=16))
