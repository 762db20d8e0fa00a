"""GPU: the VO front end between two resident SR4000 frames in one call (pre3_vo_pair_seeded).

Expected values come from code that is not under test, three ways:
  the CPU oracle chain -- oracle.siftmatch on the kept descriptors gives the match list (exact, order included); oracle.vo_gather on SrFrame.planes()
      the point sets (bit-equal); oracle.vo_ransac on them with the returned draws gives cnum, the inlier set, best, n_iterations and sta exactly and
      the transform, Euler angles, u and the error statistics within tests/test_gpu_vo.py's tolerances for the same kernels (1e-12; 1e-13 for the
      statistics: fp64 on both sides, different summation trees); tests/draws_ref.py's rule gives the draw table and the capped count;
  the parent's own chain -- vo_ransac_frames_seeded fed the oracle's match list, the read-back planes, the kept frames, n_hyp = rst and the same
      (seed, seq): draws, capped, cnum, state, inliers and every field of the result bit for bit (the same code in the same order);
  the planted motion, once at 144 x 176: sta == 1 and rot within the 1e-9 of R that test_vo_frames_entry uses.
The pairs are tests/vo_pair_cases.py's; tests/test_vo_pair_ref.py checks on the CPU that each lands on the pnum it names.  No test feeds the device an
out-of-range pixel or index: the host checks refuse them first."""
import ctypes as C
import importlib

import numpy as np
import pytest

import draws_ref
import vo_pair_cases as vp
from test_gpu_sr_frame import _write_dat
from test_gpu_vo import _compare
from test_sr_frame_ref import same_bits

pytestmark = pytest.mark.gpu
srm = importlib.import_module("3pre_amd.sr4000")
vo = importlib.import_module("3pre_amd.vo")
_lib = importlib.import_module("3pre_amd._lib")
E_ARG, E_STATE, E_NUMERIC = -1, -4, -5
SEED, SEQ = 20261018, 3
RES_FIELDS = ("rot", "trans", "euler", "u", "error_mean", "error_std", "dist", "sta", "n_support", "n_iterations", "best")


def resident(c, which=(1, 2)):
    """the case's two frames loaded in mode 1 with gate 1 run on each: (f1, f2, k1, k2)"""
    f1, f2 = srm.SrFrame(c["rows"], c["cols"]), srm.SrFrame(c["rows"], c["cols"])
    f1.load(c["fr%d" % which[0]], 1); f2.load(c["fr%d" % which[1]], 1)
    k1 = f1.keypoints(c["frm%d" % which[0]], c["des%d" % which[0]], 1)
    k2 = f2.keypoints(c["frm%d" % which[1]], c["des%d" % which[1]], 1)
    return f1, f2, k1, k2


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_same_result(a, b):
    """every output of two runs of the same arithmetic, bit for bit"""
    for k in ("draws", "cnum", "state", "inliers"):
        assert np.array_equal(a[k], b[k]), k
    assert a["capped"] == b["capped"]
    for k in RES_FIELDS:
        assert np.array_equal(bits(a[k]), bits(b[k])), (k, a[k], b[k])
    for k in ("pset1", "pset2"):
        assert np.array_equal(bits(a[k]), bits(b[k])), k


def assert_no_solution(out):
    """vodometry_dr_ye.m:152-160"""
    assert (out["sta"], out["n_support"], out["n_iterations"], out["rst"]) == (4, 0, 0, 0)
    assert np.array_equal(out["u"], [0, 0, 0, 1, 0, 0, 0]) and not out["rot"].any() and not out["trans"].any()
    assert out["draws"].shape == (0, 4) and out["cnum"].size == 0 and out["inliers"].size == 0


def check_case(c, orc):
    f1, f2, k1, k2 = resident(c)
    with f1, f2:
        assert np.array_equal(k1["keep_idx"], c["kept1"]) and np.array_equal(k2["keep_idx"], c["kept2"])
        out = vo.vo_pair_seeded(f1, f2, SEED, SEQ)
        mt, _ = orc.siftmatch(np.asfortranarray(k1["descriptors"]), np.asfortranarray(k2["descriptors"]), vp.THRESH)
        pnum = mt.shape[1]
        print(c["name"], "n1 n2 pnum rst capped sta =", c["n1"], c["n2"], pnum, out["rst"], out["capped"], out["sta"])
        assert pnum == c["expect_pnum"]
        assert out["pnum"] == pnum and out["match"].shape == mt.shape and np.array_equal(out["match"], mt)
        again = vo.vo_pair_seeded(f1, f2, SEED, SEQ)
        assert np.array_equal(again["match"], out["match"])
        if pnum < 4:
            assert_no_solution(out); assert_no_solution(again)
            return out, None
        rst = vo.vo_rst(pnum)
        assert out["rst"] == rst and out["draws"].shape == (rst, 4)
        x1, y1, z1, _ = f1.planes(); x2, y2, z2, _ = f2.planes()
        p1, p2 = orc.vo_gather(x1, y1, z1, k1["frames"], mt[0]), orc.vo_gather(x2, y2, z2, k2["frames"], mt[1])
        assert same_bits(out["pset1"], p1) and same_bits(out["pset2"], p2)
        draws, capped, _ = draws_ref.draw_vo(SEED, SEQ, mt, rst)
        assert np.array_equal(out["draws"], draws) and out["capped"] == capped
        _compare(out, orc.vo_ransac(p1, p2, out["draws"]), orc)
        parent = vo.vo_ransac_frames_seeded(k1["frames"], k2["frames"], mt, x1, y1, z1, x2, y2, z2, SEED, SEQ, n_hyp=rst)
        assert_same_result(out, parent)
        assert_same_result(again, out)
        return out, parent


@pytest.mark.parametrize("name", [n for n in sorted(vp.CASES) if n != "p129"])
def test_pair_against_the_oracle_chain_and_the_parent_chain(pre3, orc, name):
    assert pre3.device_count() >= 1
    c = vp.case(name)
    out, parent = check_case(c, orc)
    if name == "n5x1_shared":
        assert out["capped"] == 5 == parent["capped"] and len(set(out["match"][1])) == 1      # every hypothesis shares the one cur keypoint
    if name == "p4":
        assert out["rst"] == 1 and out["best"] == 0 and sorted(out["draws"][0]) == [0, 1, 2, 3]
    if name == "p12_dup":
        d = c["dup"]
        pos1 = {int(k): i + 1 for i, k in enumerate(c["kept1"])}
        pos2 = {int(k): i + 1 for i, k in enumerate(c["kept2"])}
        got = {int(p): int(q) for p, q in out["match"].T}
        assert got[pos1[d["exact_prev"]]] == pos2[d["exact_cur"]] < pos2[d["exact_copy"]]      # distance 0 to both: accepted, the first index kept
        assert pos1[d["noisy_prev"]] not in got                                                  # best == second > 0: rejected


def test_the_planted_motion_at_full_size(pre3, orc):
    c = vp.case("p129")
    out, parent = check_case(c, orc)
    assert out["rst"] == 700 and out["sta"] == 1 and out["n_support"] >= 80
    assert np.abs(out["rot"] - c["R"]).max() < 1e-9 and np.abs(out["trans"] - c["T"]).max() < 1e-9
    assert np.abs(out["u"][:3] - c["T"]).max() < 1e-9 and np.abs(out["u"][3:] - orc.R2q(c["R"])).max() < 1e-9


def test_shared_keypoints_make_the_draw_rule_redraw(pre3, orc):
    """two prev keypoints on one cur keypoint among 20 matches: the shared-keypoint redraw fires, capped equals the parent chain's"""
    c = vp.make_pair(36, 45, 40, 40, 20, seed=41, drop1=3, drop2=3)
    a, b = c["planted"]
    c["des1"][:, a[1]] = c["des1"][:, a[0]]                        # a[1] now matches a[0]'s partner too
    c["name"], c["expect_pnum"] = "two_on_one", 20
    out, parent = check_case(c, orc)
    m2 = out["match"][1]
    assert len(set(m2)) == 19
    first = np.stack([[draws_ref.vo_position(20, draws_ref.uniform(draws_ref.draw_block(SEED, draws_ref.STREAM_VO, h, 0, SEQ)[p])) for p in range(4)]
                      for h in range(out["rst"])])
    assert (first != out["draws"]).any()                           # some position was redrawn
    for r in out["draws"]:
        assert len(set(r)) == 4 and len({m2[r[0]], m2[r[1]], m2[r[2]]}) == 3
    assert out["capped"] == parent["capped"]


def test_no_point_beyond_40_cm_is_a_numeric_error_and_the_handles_stay_usable(pre3, orc):
    c = vp.make_pair(36, 45, 33, 65, 12, seed=21, near=True, drop1=2)
    f1, f2, k1, k2 = resident(c)
    with f1, f2:
        with pytest.raises(pre3.Pre3Error) as e:
            vo.vo_pair_seeded(f1, f2, SEED, SEQ)
        assert e.value.code == E_NUMERIC
        # the same handles, a new pair: load + keypoints on both, then the new result
        good = vp.case("p13")
        f1.load(good["fr1"], 1); f2.load(good["fr2"], 1)
        f1.keypoints(good["frm1"], good["des1"], 1); f2.keypoints(good["frm2"], good["des2"], 1)
        out = vo.vo_pair_seeded(f1, f2, SEED, SEQ)
    g1, g2, _, _ = resident(good)
    with g1, g2:
        fresh = vo.vo_pair_seeded(g1, g2, SEED, SEQ)
    assert out["pnum"] == 13 and np.array_equal(out["match"], fresh["match"])
    assert_same_result(out, fresh)


def test_load_and_keypoints_on_prev_give_the_new_result(pre3, orc):
    a, b = vp.case("p13"), vp.case("p12")
    f1, f2, _, _ = resident(a)
    with f1, f2:
        first = vo.vo_pair_seeded(f1, f2, SEED, SEQ)
        # a stale record: prev holds a new frame whose keypoints have not been run
        f1.load(b["fr1"], 1)
        with pytest.raises(pre3.Pre3Error) as e:
            vo.vo_pair_seeded(f1, f2, SEED, SEQ)
        assert e.value.code == E_STATE
        f1.keypoints(b["frm1"], b["des1"], 1)
        f2.load(b["fr2"], 1); f2.keypoints(b["frm2"], b["des2"], 1)
        second = vo.vo_pair_seeded(f1, f2, SEED, SEQ)
    g1, g2, _, _ = resident(b)
    with g1, g2:
        fresh = vo.vo_pair_seeded(g1, g2, SEED, SEQ)
    assert first["pnum"] == 13 and second["pnum"] == 12 and np.array_equal(second["match"], fresh["match"])
    assert_same_result(second, fresh)


def test_argument_and_state_errors_leave_both_handles_unchanged(pre3, orc):
    lib, dptr = _lib.lib, _lib.dptr
    c = vp.case("p13")
    f1, f2, k1, k2 = resident(c)
    res, pn = vo.VoResult(), C.c_int32(-7)

    def call(p, q, thresh=1.5):
        return lib.pre3_vo_pair_seeded(p, q, thresh, SEED, SEQ, C.byref(pn), None, None, None, None, None, None, None, None, C.byref(res))

    with f1, f2, srm.SrFrame(36, 46) as other, srm.SrFrame(36, 45) as empty, srm.SrFrame(36, 45) as nd64, srm.SrFrame(36, 45) as fresh:
        before = vo.vo_pair_seeded(f1, f2, SEED, SEQ)
        planes = [f.planes() for f in (f1, f2)]
        other.load({k: (None if v is None else np.asfortranarray(np.pad(v, ((0, 0), (0, 1)), mode="edge"))) for k, v in c["fr2"].items()}, 1)
        other.keypoints(c["frm2"], c["des2"], 1)
        nd64.load(c["fr2"], 1); nd64.keypoints(c["frm2"], c["des2"][:64], 1)
        fresh.load(c["fr2"], 1)                                     # loaded, no keypoint call yet
        # (each call is made inside the loop: pre3_last_error belongs to the call just made)
        for what, fn, want in (("null prev", lambda: call(None, f2._h), E_ARG), ("null cur", lambda: call(f1._h, None), E_ARG),
                               ("prev == cur", lambda: call(f1._h, f1._h), E_ARG), ("sizes differ", lambda: call(f1._h, other._h), E_ARG),
                               ("ND != 128 on cur", lambda: call(f1._h, nd64._h), E_ARG), ("ND != 128 on prev", lambda: call(nd64._h, f2._h), E_ARG),
                               ("thresh 0", lambda: call(f1._h, f2._h, 0.0), E_ARG), ("thresh < 0", lambda: call(f1._h, f2._h, -1.5), E_ARG),
                               ("thresh nan", lambda: call(f1._h, f2._h, float("nan")), E_ARG), ("thresh inf", lambda: call(f1._h, f2._h, float("inf")), E_ARG),
                               ("nothing loaded", lambda: call(f1._h, empty._h), E_STATE), ("no keypoint record", lambda: call(fresh._h, f2._h), E_STATE)):
            rc = fn()
            assert rc == want, (what, rc)
            assert want == E_STATE or b"pre3_vo_pair_seeded" in lib.pre3_last_error(), (what, lib.pre3_last_error())
        assert pn.value == -7                                        # nothing was written
        for f, (x, y, z, conf) in zip((f1, f2), planes):
            gx, gy, gz, gc = f.planes()
            assert same_bits(gx, x) and same_bits(gy, y) and same_bits(gz, z) and same_bits(gc, conf)
        after = vo.vo_pair_seeded(f1, f2, SEED, SEQ)                # the keypoint records are the ones from before
        assert np.array_equal(after["match"], before["match"])
        assert_same_result(after, before)
        # an empty record is valid: K == 0 on cur gives pnum = 0
        f2.keypoints(np.zeros((4, 0)), np.zeros((128, 0)), 1)
        assert_no_solution(vo.vo_pair_seeded(f1, f2, SEED, SEQ))
        # optional outputs may all be NULL
        f2.keypoints(c["frm2"], c["des2"], 1)
        assert lib.pre3_vo_pair_seeded(f1._h, f2._h, 1.5, SEED, SEQ, None, None, None, None, None, None, None, None, None, None) == 0
        assert call(f1._h, f2._h) == 0 and pn.value == 13
        for k in ("sta", "n_support", "n_iterations", "best"):
            assert getattr(res, k) == before[k]


def test_vodometry_dr_ye_on_two_dat_files_equals_the_direct_call(pre3, orc, tmp_path):
    c = vp.make_pair(144, 176, 60, 70, 40, seed=31, drop1=8, drop2=5)
    d1, d2 = tmp_path / "d1_0001.dat", tmp_path / "d1_0002.dat"
    _write_dat(d1, c["fr1"]); _write_dat(d2, c["fr2"])
    out = srm.vodometry_dr_ye(str(d1), str(d2), (c["frm1"], c["des1"]), (c["frm2"], c["des2"]), SEED, SEQ)
    c["rows"], c["cols"] = 144, 176
    f1, f2, k1, k2 = resident(c)
    with f1, f2:
        direct = vo.vo_pair_seeded(f1, f2, SEED, SEQ)
    assert np.array_equal(out["kept1"], k1["keep_idx"]) and np.array_equal(out["kept2"], k2["keep_idx"])
    assert out["pnum"] == 40 and np.array_equal(out["match"], direct["match"])
    assert_same_result(out, direct)
    T, q, R, sta = srm.calculate_v_omega(str(d1), str(d2), (c["frm1"], c["des1"]), (c["frm2"], c["des2"]), SEED, SEQ)
    assert sta == 1 and np.array_equal(T, direct["u"][:3]) and np.array_equal(q, direct["u"][3:]) and np.array_equal(R, direct["rot"])
    assert np.abs(R - c["R"]).max() < 1e-9
