"""GPU: map management's candidate build and policy from two resident frames in one call (pre3_map_policy_frames_seeded).

Primary yardstick, exact: the parent's own chain on a twin context -- SrFrame.keypoints(gate 0) read back, pre3_siftmatch_f64 on the kept descriptors,
the gather of initialize_features.m:97-99 in numpy, map_management_policy_seeded -- against which match, K, order, the lists, stats, the book, the
descriptor bank, x and P are compared bit for bit.  That parity rests on rho: the parent recomputes it on the host as 1 / sqrt(x*x + y*y + z*z) of the
read-back xyz, the new call takes the keypoint stage's own; every case first asserts that the two are the same bits.
Secondary, exact: lists, stats and the book against the CPU restatement chain of tests/test_frame_policy_ref.py (restatement (a) of section 20,
oracle.siftmatch, cand_order_ref, map_policy_ref), whose margins that file asserts for every case -- nothing is skipped here.
No test feeds the device an out-of-range pixel or index: the host checks refuse them first."""
import ctypes as C
import importlib

import numpy as np
import pytest

import frame_policy_cases as fp
from test_frame_policy_ref import chain
from test_gpu_map_policy import _filter
from test_gpu_sr_frame import _write_dat

pytestmark = pytest.mark.gpu
srm = importlib.import_module("3pre_amd.sr4000")
_lib = importlib.import_module("3pre_amd._lib")
E_ARG, E_STATE, E_NUMERIC = -1, -4, -5
SEED, SEQ = fp.SEED, fp.SEQ


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def resident(c, fr1=None):
    """the case's two frames loaded in mode 0, gate 0 on prev and the case's gate on cur: (f1, f2, k1, k2)"""
    f1, f2 = srm.SrFrame(c["rows"], c["cols"]), srm.SrFrame(c["rows"], c["cols"])
    f1.load(c["fr1"] if fr1 is None else fr1, fp.MODE); f2.load(c["fr2"], fp.MODE)
    return f1, f2, f1.keypoints(c["frm1"], c["des1"], 0), f2.keypoints(c["frm2"], c["des2"], c["gate_cur"])


def bank0(c):
    """descriptors of the map before the call: the survivors carry theirs through the re-layout"""
    return np.random.default_rng(c["N"]).integers(0, 255, (128, c["N"])).astype(float)


def context(pre3, c, dtype):
    f = _filter(pre3, c["cam"], c["N"], c["x"], c["P"], dtype, c["cap"], c["meas"], c["li"], c["hi"], c["book"])
    if c["N"]:
        f.set_descriptors(bank0(c))
    return f


def state(pre3, f):
    try:
        desc = f.get_descriptors() if f.N else None
    except pre3.Pre3Error as e:                                      # no descriptor has ever been set: the same on both twins
        assert e.code == E_STATE
        desc = "unset"
    return dict(N=f.N, types=f.lm_type.copy(), book=f.book(), x=f.get_x_k_k(), P=f.get_p_k_k(), desc=desc)


def same_state(a, b):
    assert a["N"] == b["N"] and np.array_equal(a["types"], b["types"]) and np.array_equal(a["book"], b["book"])
    assert np.array_equal(bits(a["x"]), bits(b["x"])) and np.array_equal(bits(a["P"]), bits(b["P"]))
    if isinstance(a["desc"], str) or isinstance(b["desc"], str) or a["desc"] is None or b["desc"] is None:
        assert type(a["desc"]) is type(b["desc"]) and (not isinstance(a["desc"], str) or a["desc"] == b["desc"])
    else:
        assert np.array_equal(bits(a["desc"]), bits(b["desc"]))


def same_result(a, b):
    for k in ("deleted", "accepted", "converted", "order"):
        assert np.array_equal(a[k], b[k]), k
    assert all(a[k] == b[k] for k in ("measured", "target", "examined", "N"))
    if "match" in b:
        assert a["K"] == b["K"] and np.array_equal(bits(a["match"]), bits(b["match"]))


def kwargs(c, strict):
    return dict(min_features=c["min_features"], linearity_index_threshold=0.1, std_pxl=1.0, strict_reference=strict)


def parent_chain(pre3, g, c, k1, k2, strict):
    """what a caller of pre3_map_policy_seeded does today, on context g"""
    if k1["descriptors"].shape[1] and k2["descriptors"].shape[1]:
        mt = pre3.siftmatch(k1["descriptors"], k2["descriptors"], fp.THRESH)
    else:
        mt = np.zeros((2, 0))
    uv, xyz, desc = fp.gather(k1, mt)
    out = g.map_management_policy_seeded(c["step"], uv, xyz, SEED, SEQ, cand_desc=desc, **kwargs(c, strict))
    out.update(match=mt, K=mt.shape[1], desc=desc)
    return out


def assert_rho_identity(k1):
    x, y, z = k1["xyz"]
    assert np.array_equal(bits(k1["rho"]), bits(1 / np.sqrt(x * x + y * y + z * z))), "keypoints()['rho'] is not 1 / sqrt(sum xyz^2) bit for bit on the device"


def run_case(pre3, orc, name, dtype, strict):
    ch = chain(name, orc)
    c = ch["c"]
    f1, f2, k1, k2 = resident(c)
    with f1, f2:
        assert np.array_equal(k1["keep_idx"], c["kept1"]) and np.array_equal(k2["keep_idx"], c["kept2"])
        assert_rho_identity(k1)
        f, g = context(pre3, c, dtype), context(pre3, c, dtype)
        pred = f.landmark_fields()["has_h"] if c["N"] else np.zeros(0, np.int32)
        ref = parent_chain(pre3, g, c, k1, k2, strict)
        out = f.map_management_policy_frames_seeded(c["step"], f1, f2, SEED, SEQ, fp.THRESH, **kwargs(c, strict))
        print(name, dtype, strict, "n1 n2 K examined accepted deleted N =", c["n1"], c["n2"], out["K"], out["examined"], len(out["accepted"]), len(out["deleted"]), out["N"])
        assert out["K"] == c["expect_pnum"] == ch["match"].shape[1] and np.array_equal(out["match"], ch["match"])
        same_result(out, ref)
        sf, sg = state(pre3, f), state(pre3, g)
        same_state(sf, sg)
        n_s = c["N"] - len(out["deleted"])
        if len(out["accepted"]):
            assert np.array_equal(sf["desc"][:, n_s:], ref["desc"][:, out["accepted"]])
            assert np.array_equal(sf["desc"][:, n_s:], c["des1"][:, c["kept1"][out["match"][0].astype(int) - 1][out["accepted"]]])
        if n_s and not isinstance(sf["desc"], str):
            assert np.array_equal(sf["desc"][:, :n_s], np.delete(bank0(c), out["deleted"], axis=1))
        # the CPU restatement chain: lists, stats and the book exact
        r = fp.restated_policy(c, ch["uv"], ch["xyz"], pred, strict, dtype)
        rr = r["ref"]
        assert r["margin_ok"]
        assert np.array_equal(out["order"], r["order"]) and np.array_equal(out["accepted"], r["accepted"])
        assert np.array_equal(out["deleted"], rr["deleted"]) and np.array_equal(out["converted"], rr["converted"])
        assert (out["measured"], out["target"], out["examined"]) == (rr["measured"], rr["T"], rr["examined"])
        assert out["N"] == f.N == c["N"] - len(rr["deleted"]) + len(rr["accepted"]) and np.array_equal(sf["book"], rr["book"])
        fp.check_ending(c, rr, out["K"], strict)
        f.close(); g.close()
    return out, sf


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("name", sorted(fp.CASES))
def test_frames_call_is_the_parent_chain_bit_for_bit(pre3, orc, name, strict, dtype):
    assert pre3.device_count() >= 1
    run_case(pre3, orc, name, dtype, strict)


@pytest.mark.parametrize("name", ["p63", "p129"])
def test_a_second_call_on_a_fresh_twin_is_bit_equal(pre3, orc, name):
    a, sa = run_case(pre3, orc, name, "f32", True)
    b, sb = run_case(pre3, orc, name, "f32", True)
    same_result(a, b); same_state(sa, sb)


def test_a_nan_y_at_a_matched_keypoint_is_a_numeric_error_and_changes_nothing(pre3, orc):
    ch = chain("p63", orc)
    c = ch["c"]
    a, _ = c["planted"]
    r0, c0 = int(round(c["frm1"][1, a[3]])) - 1, int(round(c["frm1"][0, a[3]])) - 1
    bad = {k: (None if v is None else v.copy(order="F")) for k, v in c["fr1"].items()}
    bad["y"][r0, c0] = np.nan                                       # the filtered y of that pixel is NaN, its x is not: the depth gate keeps it
    f1, f2, k1, k2 = resident(c, bad)
    with f1, f2:
        assert np.array_equal(k1["keep_idx"], c["kept1"]) and np.isnan(k1["rho"]).sum() == 1
        f, g = context(pre3, c, "f64"), context(pre3, c, "f64")
        before = state(pre3, f)
        for _ in range(2):                                           # (the second call: both records are still there and still the same)
            with pytest.raises(pre3.Pre3Error) as e:
                f.map_management_policy_frames_seeded(c["step"], f1, f2, SEED, SEQ, fp.THRESH, **kwargs(c, True))
            assert e.value.code == E_NUMERIC and "pre3_map_policy_frames_seeded" in str(e.value)
            same_state(state(pre3, f), before)
            assert f1.n_kept == c["n1"] and f2.n_kept == c["n2"]
        # a following valid call on the same context and handles
        f1.load(c["fr1"], fp.MODE)
        k1 = f1.keypoints(c["frm1"], c["des1"], 0)
        out = f.map_management_policy_frames_seeded(c["step"], f1, f2, SEED, SEQ, fp.THRESH, **kwargs(c, True))
        ref = parent_chain(pre3, g, c, k1, k2, True)
        same_result(out, ref); same_state(state(pre3, f), state(pre3, g))
        assert out["K"] == 63
        f.close(); g.close()


def test_load_and_keypoints_on_prev_right_after_the_call(pre3, orc):
    """the release event: the descriptor copy out of prev's keypoint block is queued on the context's stream when the call returns; a load and a
    keypoint call on prev right behind it must not overwrite what it reads"""
    ch, other = chain("p129_0", orc), fp.case("p129")
    c = ch["c"]
    f1, f2, k1, k2 = resident(c)
    with f1, f2:
        f, g = context(pre3, c, "f32"), context(pre3, c, "f32")
        out = f.map_management_policy_frames_seeded(c["step"], f1, f2, SEED, SEQ, fp.THRESH, **kwargs(c, False))
        f1.load(other["fr1"], fp.MODE)
        f1.keypoints(other["frm1"], other["des1"], 0)
        f2.load(other["fr2"], fp.MODE)
        ref = parent_chain(pre3, g, c, k1, k2, False)
        same_result(out, ref); same_state(state(pre3, f), state(pre3, g))
        assert len(out["accepted"]) == 30
        # prev now holds the other frame and its record; cur's record is stale
        with pytest.raises(pre3.Pre3Error) as e:
            f.map_management_policy_frames_seeded(c["step"] + 1, f1, f2, SEED, SEQ, fp.THRESH, **kwargs(c, False))
        assert e.value.code == E_STATE
        f.close(); g.close()


def test_argument_and_state_errors_leave_everything_unchanged(pre3, orc):
    lib = _lib.lib
    ch = chain("p20", orc)
    c = ch["c"]
    f1, f2, k1, k2 = resident(c)
    rows, cols = c["rows"], c["cols"]
    Kout, nd, na = C.c_int32(-7), C.c_int32(-7), C.c_int32(-7)

    def call(ctx, p, q, thresh=1.5, mf=50, box=(176, 144), std=1.0, thr=0.1):
        return lib.pre3_map_policy_frames_seeded(ctx, p, q, thresh, c["step"], mf, thr, std, 1, box[0], box[1], SEED, SEQ, C.byref(Kout), None, None, None,
                                                 C.byref(nd), None, C.byref(na), None, None)

    with f1, f2, srm.SrFrame(rows, cols + 1) as other, srm.SrFrame(rows, cols) as empty, srm.SrFrame(rows, cols) as nd64, \
            srm.SrFrame(rows, cols) as fresh, srm.SrFrame(rows, cols) as gate1, srm.SrFrame(rows, cols) as stale:
        f, g = context(pre3, c, "f64"), context(pre3, c, "f64")
        unbooked = pre3.EkfFilter(c["cam"], np.zeros(c["N"], np.int32), dtype="f64", max_landmarks=c["cap"])
        unbooked.set_x_p_k_k(c["x"], c["P"])
        before = state(pre3, f)
        planes = [h.planes() for h in (f1, f2)]
        other.load({k: (None if v is None else np.asfortranarray(np.pad(v, ((0, 0), (0, 1)), mode="edge"))) for k, v in c["fr2"].items()}, fp.MODE)
        other.keypoints(c["frm2"], c["des2"], 0)
        nd64.load(c["fr2"], fp.MODE); nd64.keypoints(c["frm2"], c["des2"][:64], 0)
        fresh.load(c["fr2"], fp.MODE)                                # loaded, no keypoint call yet
        gate1.load(c["fr1"], fp.MODE); gate1.keypoints(c["frm1"], c["des1"], 1)
        stale.load(c["fr1"], fp.MODE); stale.keypoints(c["frm1"], c["des1"], 0); stale.load(c["fr1"], fp.MODE)
        x = f._ctx
        # (each call is made inside the loop: pre3_last_error belongs to the call just made)
        for what, fn, want in (("null context", lambda: call(None, f1._h, f2._h), E_ARG), ("null prev", lambda: call(x, None, f2._h), E_ARG),
                               ("null cur", lambda: call(x, f1._h, None), E_ARG), ("prev == cur", lambda: call(x, f1._h, f1._h), E_ARG),
                               ("sizes differ", lambda: call(x, f1._h, other._h), E_ARG), ("ND != 128 on cur", lambda: call(x, f1._h, nd64._h), E_ARG),
                               ("ND != 128 on prev", lambda: call(x, nd64._h, f2._h), E_ARG), ("gate 1 on prev", lambda: call(x, gate1._h, f2._h), E_ARG),
                               ("thresh 0", lambda: call(x, f1._h, f2._h, 0.0), E_ARG), ("thresh nan", lambda: call(x, f1._h, f2._h, float("nan")), E_ARG),
                               ("thresh inf", lambda: call(x, f1._h, f2._h, float("inf")), E_ARG), ("min_features", lambda: call(x, f1._h, f2._h, mf=1025), E_ARG),
                               ("min_features < 0", lambda: call(x, f1._h, f2._h, mf=-1), E_ARG), ("box 0", lambda: call(x, f1._h, f2._h, box=(0, 144)), E_ARG),
                               ("box sigma 0", lambda: call(x, f1._h, f2._h, box=(176, 2)), E_ARG), ("std nan", lambda: call(x, f1._h, f2._h, std=float("nan")), E_ARG),
                               ("threshold inf", lambda: call(x, f1._h, f2._h, thr=float("inf")), E_ARG),
                               ("nothing loaded", lambda: call(x, f1._h, empty._h), E_STATE), ("no keypoint record", lambda: call(x, fresh._h, f2._h), E_STATE),
                               ("stale record", lambda: call(x, stale._h, f2._h), E_STATE), ("no book", lambda: call(unbooked._ctx, f1._h, f2._h), E_STATE)):
            rc = fn()
            assert rc == want, (what, rc, lib.pre3_last_error())
            assert want == E_STATE or what == "null context" or b"pre3_map_policy_frames_seeded" in lib.pre3_last_error(), (what, lib.pre3_last_error())
        assert (Kout.value, nd.value, na.value) == (-7, -7, -7)      # nothing was written
        same_state(state(pre3, f), before)
        assert np.array_equal(unbooked.get_x_k_k(), c["x"]) and unbooked.N == c["N"]
        for h, (px, py, pz, pc) in zip((f1, f2), planes):
            gx, gy, gz, gc = h.planes()
            assert np.array_equal(bits(gx), bits(px)) and np.array_equal(bits(gy), bits(py)) and np.array_equal(bits(gz), bits(pz)) and np.array_equal(bits(gc), bits(pc))
        # the records are the ones from before: the call still equals the parent chain; every optional output may be NULL
        assert call(x, f1._h, f2._h) == 0 and Kout.value == 20
        f._refresh_map()
        ref = parent_chain(pre3, g, c, k1, k2, True)
        assert (nd.value, na.value) == (len(ref["deleted"]), len(ref["accepted"]))
        same_state(state(pre3, f), state(pre3, g))
        f.close(); g.close(); unbooked.close()


def test_initialize_features_frames_on_two_dat_files_equals_the_direct_call(pre3, orc, tmp_path):
    ch = chain("p129", orc)
    c = ch["c"]
    d1, d2 = tmp_path / "d1_0001.dat", tmp_path / "d1_0002.dat"
    _write_dat(d1, c["fr1"]); _write_dat(d2, c["fr2"])
    f, g = context(pre3, c, "f32"), context(pre3, c, "f32")
    out = srm.initialize_features_frames(f, c["step"], str(d1), str(d2), (c["frm1"], c["des1"]), (c["frm2"], c["des2"]), SEED, SEQ, fp.THRESH,
                                         **kwargs(c, True))
    f1, f2, k1, k2 = resident(c)
    with f1, f2:
        direct = g.map_management_policy_frames_seeded(c["step"], f1, f2, SEED, SEQ, fp.THRESH, **kwargs(c, True))
    assert np.array_equal(out["kept_prev"], k1["keep_idx"]) and np.array_equal(out["kept_cur"], k2["keep_idx"])
    same_result(out, direct); same_state(state(pre3, f), state(pre3, g))
    assert out["K"] == 129 and np.array_equal(out["cand_idx"], c["kept1"][direct["match"][0].astype(int) - 1])
    f.close(); g.close()
