"""GPU: the pair form of EPnP (pre3_vo_pair_pnp_seeded) -- RANSAC_CALC_VER2.m:191 in place: the VO pair's launches with the EPnP
refit over the pair's inliers behind them, prev's range points against cur's pixels.  Every output shared with pre3_vo_pair_seeded is that call's bit
for bit, the EPnP result is pre3_epnp's on the gathered arrays bit for bit, and on a pinhole-consistent pair the pose is held to twice the distance
from the truth that tests/epnp_ref.py has on the same arrays.  tests/test_gpu_vo_pair.py's frames are imported, not edited."""
import ctypes as C
import importlib

import numpy as np
import pytest

import epnp_ref as ref
import pnp_cases as pc
import pnp_frame_cases as F
import vo_pair_cases as vp
from test_gpu_pnp import bits as pnp_bits
from test_gpu_vo_pair import SEED, SEQ, assert_same_result, bits, resident

pytestmark = pytest.mark.gpu
vo = importlib.import_module("3pre_amd.vo")
_lib = importlib.import_module("3pre_amd._lib")
E_ARG, E_STATE = -1, -4
CAM = pc.fixture_cam()
IDENTITY = [0, 0, 0, 1, 0, 0, 0]


def both(c):
    f1, f2, k1, k2 = resident(c)
    with f1, f2:
        plain = vo.vo_pair_seeded(f1, f2, SEED, SEQ)
        out = vo.vo_pair_pnp_seeded(f1, f2, SEED, CAM, SEQ)
        again = vo.vo_pair_pnp_seeded(f1, f2, SEED, CAM, SEQ)
    return plain, out, again, k2


def assert_shared_outputs_equal(out, plain):
    assert out["pnum"] == plain["pnum"] and out["rst"] == plain["rst"] and np.array_equal(out["match"], plain["match"])
    if plain["rst"]:
        assert_same_result(out, plain)
    else:
        assert out["sta"] == plain["sta"] == 4 and np.array_equal(out["u"], plain["u"])


@pytest.mark.parametrize("name", ["p13", "p64", "p65"])
def test_shared_outputs_and_the_refit_are_bit_equal_to_their_own_calls(name):
    plain, out, again, k2 = both(vp.case(name))
    assert_shared_outputs_equal(out, plain)
    inl = np.nonzero(out["inliers"])[0]
    print(name, "pnum", out["pnum"], "support", len(inl), "pair sta", out["sta"], "pnp sta", out["pnp"]["sta"], "err", out["pnp"]["err"])
    assert out["pix2"].shape == (2, out["pnum"])
    assert np.array_equal(bits(out["pix2"]), bits(k2["frames"][:2, out["match"][1].astype(int) - 1])), "cur's kept uv at match(2, :)"
    assert out["sta"] == 1 and len(inl) >= 6 and out["pnp"]["n"] == len(inl) == out["pnp"]["n_support"]
    alone = vo.efficient_pnp(out["pset1"][:, inl].T, out["pix2"][:, inl].T, CAM)[4]
    assert pnp_bits(out["pnp"]) == pnp_bits(alone), "the refit behind the pair is pre3_epnp on the gathered arrays"
    assert pnp_bits(again["pnp"]) == pnp_bits(out["pnp"]) and np.array_equal(bits(again["pix2"]), bits(out["pix2"]))


def test_the_pinhole_consistent_pair():
    c = F.pinhole_pair()
    plain, out, again, k2 = both(c)
    assert_shared_outputs_equal(out, plain)
    inl = np.nonzero(out["inliers"])[0]
    assert out["pnum"] == F.K and out["sta"] == 1 and out["pnp"]["sta"] == 1
    bad_prev = set(np.nonzero(np.isin(out["match"][1].astype(int) - 1, c["corrupt"]))[0].tolist())
    assert len(bad_prev) == F.N_CORRUPT and not bad_prev & set(inl.tolist()), "the corrupted depths are outliers of the 3-D / 3-D fit"
    Xw, U = out["pset1"][:, inl].T, out["pix2"][:, inl].T
    assert pnp_bits(out["pnp"]) == pnp_bits(vo.efficient_pnp(Xw, U, CAM)[4])
    R0, T0 = F.truth_RT(c)
    want = ref.epnp(Xw, U, CAM)
    ang0, dist0 = pc.pose_error(want["R"], want["T"], R0, T0)
    ang, dist = pc.pose_error(out["pnp"]["R"], out["pnp"]["T"], R0, T0)
    ang3, dist3 = pc.pose_error(out["rot"].T, -out["rot"].T @ out["trans"], R0, T0)
    # recorded, not compared with each other: nobody has measured which of the two is nearer the truth in general
    print("against the truth: EPnP %.3e deg %.3e m (restatement %.3e deg %.3e m); the pair's 3-D / 3-D fit %.3e deg %.3e m" % (ang, dist, ang0, dist0, ang3, dist3))
    assert np.isfinite([ang, dist]).all() and ang <= 2 * ang0 and dist <= 2 * dist0
    assert np.abs(out["pnp"]["u"] - ref.pair_u(out["pnp"]["R"], out["pnp"]["T"])).max() < 1e-12
    assert np.abs(out["pnp"]["u"] - out["u"]).max() < 1e-3, "the two increments are in one convention"


def test_refusals_and_a_pair_below_six_inliers(pre3):
    c = vp.case("p13")
    f1, f2, k1, k2 = resident(c)
    fresh = importlib.import_module("3pre_amd.sr4000").SrFrame(c["rows"], c["cols"])
    with f1, f2, fresh:
        fresh.load(c["fr2"], 1)                                     # loaded, no keypoint call yet
        for what, fn, want in (("prev == cur", lambda: vo.vo_pair_pnp_seeded(f1, f1, SEED, CAM, SEQ), E_ARG),
                               ("no keypoint record", lambda: vo.vo_pair_pnp_seeded(fresh, f2, SEED, CAM, SEQ), E_STATE),
                               ("f == 0", lambda: vo.vo_pair_pnp_seeded(f1, f2, SEED, [0.0] + list(CAM[1:]), SEQ), E_ARG),
                               ("f < 0", lambda: vo.vo_pair_pnp_seeded(f1, f2, SEED, [-800.0] + list(CAM[1:]), SEQ), E_ARG)):
            with pytest.raises(pre3.Pre3Error) as e:
                fn()
            assert e.value.code == want, what
        r = vo.PnpResult()
        pnum = C.c_int32(0)
        from3 = _lib.lib.pre3_vo_pair_pnp_seeded(f1._h, f2._h, 1.5, SEED, SEQ, None, 0, C.byref(pnum), None, None, None, None, None, None, None, None, None, None, C.byref(r))
        assert from3 == E_ARG, "a null camera"
    for name in ("p3", "p5"):                                        # fewer than four matches; five matches: at most five inliers
        plain, out, again, _ = both(vp.case(name))
        assert_shared_outputs_equal(out, plain)
        assert out["pnp"]["sta"] == 0 and np.array_equal(out["pnp"]["u"], IDENTITY) and np.array_equal(out["pnp"]["R"], np.eye(3))
        assert out["n_support"] < 6


def test_vodometry_frames_pnp_on_two_dat_files(tmp_path):
    """the same scan twice: every keypoint has its match, the motion is the identity, and the pose from prev's points and cur's pixels comes out
    finite and in the pair's convention; every output of vodometry_frames is there bit for bit"""
    from test_gpu_sift import _texture_planes
    from test_gpu_vo_pair import _write_dat
    srm = importlib.import_module("3pre_amd.sr4000")
    d1, d2 = tmp_path / "d1_0001.dat", tmp_path / "d1_0002.dat"
    _write_dat(d1, _texture_planes(1)); _write_dat(d2, _texture_planes(1))
    plain = srm.vodometry_frames(str(d1), str(d2), 5, 0)
    out = srm.vodometry_frames_pnp(str(d1), str(d2), 5, pc.SR_CAM, 0)
    assert np.array_equal(out["kept1"], plain["kept1"]) and out["pnum"] == plain["pnum"] > 100
    assert_shared_outputs_equal(out, plain)
    inl = np.nonzero(out["inliers"])[0]
    assert out["pnp"]["n"] == len(inl) and out["pnp"]["sta"] in (1, 2) and np.isfinite(out["pnp"]["u"]).all()
    alone = vo.efficient_pnp(out["pset1"][:, inl].T, out["pix2"][:, inl].T, pc.SR_CAM, undistort=True)[4]
    assert pnp_bits(out["pnp"]) == pnp_bits(alone)
