"""GPU: sift_vedal made on the device in a resident frame's keypoint block (pre3_sift.hip) against the numpy restatement
tests/sift_ref.py, which is fed the library's own plan (pre3_sift_plan_get: the taps the launches use).

Bit for bit: every level of gss and dogss (pre3_sr_frame_sift_level), the four counts per octave, the refined (x, y, s) of every octave and their order
(pre3_sr_frame_sift_refined), x and y of every frame.  Equal: K and the number of orientations per refined point.  Within tests/golden/sift_tolerance.json
(16 x a floor measured on the CPU with the restatement alone): sigma, theta, the descriptor entries.
Shapes: 69 x 85 (odd both ways, four octaves, the last narrower than its filter), 37 x 45 in double interpolation, the real 144 x 176 after a load."""
import ctypes as C
import importlib

import numpy as np
import pytest

import sift_ref as R
import sr_frame_ref as sr
from test_sift_ref import compare, same_bits, tolerance

pytestmark = pytest.mark.gpu
srm = importlib.import_module("3pre_amd.sr4000")
vo = importlib.import_module("3pre_amd.vo")
matcher = importlib.import_module("3pre_amd.matcher")
_lib = importlib.import_module("3pre_amd._lib")
E_ARG, E_STATE, E_NOMEM = -1, -4, -6
_CASE, _FRAME = {}, {}


def teardown_module(module):
    """the shared handles (a scale space and pinned memory each) are closed with the module"""
    for v in list(_CASE.values()) + list(_FRAME.values()):
        v[0].close()
    _CASE.clear(); _FRAME.clear()


def lib_plan(M, N):
    """the restatement's plan with the library's own bits in it"""
    got, pl = srm.sift_plan(M, N), R.plan(M, N)
    pl["sigma0"], pl["pow2"] = got["sigma0"], [float(v) for v in got["pow2"]]
    pl["lev"] = [[(float(got["sigma"][o, l]), int(got["W"][o, l]), [float(v) for v in got["taps"][o, l, :2 * got["W"][o, l] + 1]] if got["W"][o, l] else [])
                  for l in range(R.NLEV)] for o in range(got["O"])]
    return pl


def case(shape, strict):
    """one device run on a committed image and the restatement of it, computed once and shared; the handle stays open for the level reads"""
    key = (shape, strict)
    if key not in _CASE:
        I = R.make_image(*shape)
        f = srm.SrFrame(*shape)
        _CASE[key] = (f, f.sift(I, int(strict), one_based=False), R.sift_vedal(I, strict, pl=lib_plan(*shape)), I)
    return _CASE[key]


def loaded_frame(seed):
    """a 144 x 176 frame of synthetic planes whose amplitude is a texture, loaded in mode 1; the device set, and the restatement on SrFrame.image()"""
    if seed not in _FRAME:
        fr = sr.make_frame(144, 176, seed=seed, conf=True)
        fr["amp"] = np.asfortranarray((R.make_image(144, 176, seed=40 + seed) / 255.0) ** 2 * 9000.0 + 1.0)
        f = srm.SrFrame(144, 176).load(fr, srm.MODE_DR_YE)
        got = f.sift()
        _FRAME[seed] = (f, fr, got, R.sift_vedal(f.image().astype(np.float64), True, pl=lib_plan(144, 176)))
    return _FRAME[seed]


CASES = (((69, 85), True), ((37, 45), False))


@pytest.mark.parametrize("shape,strict", CASES)
def test_every_level_of_the_scale_space_is_bit_equal(shape, strict):
    f, got, ref, _ = case(shape, strict)
    for o in range(ref["plan"]["O"]):
        for l in range(R.NLEV):
            assert same_bits(f.sift_level(o, l), ref["gss"][o][:, :, l]), ("gss", o, l)
        for l in range(R.NDOG):
            assert same_bits(f.sift_level(o, l, dog=True), ref["dogss"][o][:, :, l]), ("dogss", o, l)


@pytest.mark.parametrize("shape,strict", CASES)
def test_counts_order_and_refined_points(shape, strict):
    f, got, ref, _ = case(shape, strict)
    assert np.array_equal(got["counts"], ref["counts"])
    assert got["K"] == ref["frames"].shape[1] > 0
    want = np.concatenate([np.vstack([q, np.full((1, q.shape[1]), float(o))]) for o, q in enumerate(ref["refined"])], 1)
    assert same_bits(f.sift_refined(), want)                          # (x, y, s, octave) of every refined point, with or without an orientation
    assert same_bits(got["frames"][:2], ref["frames"][:2])            # 2^(o - 1) x the refined (x, y), every orientation of a point in a row
    # the orientation multiplicities: runs of equal (x, y) inside an octave
    xy = got["frames"][:2].T
    runs = np.diff(np.flatnonzero(np.r_[True, np.any(xy[1:] != xy[:-1], axis=1), True]))
    assert np.array_equal(runs, np.concatenate(ref["npeaks"])[np.concatenate(ref["npeaks"]) > 0])


@pytest.mark.parametrize("shape,strict", CASES)
def test_sigma_theta_and_descriptors_within_the_tolerance(shape, strict):
    f, got, ref, _ = case(shape, strict)
    compare(got, ref, tolerance(), "device %s" % (shape,))


@pytest.mark.parametrize("shape,strict", CASES)
def test_two_runs_are_bit_equal_and_one_based_adds_one(shape, strict):
    f, got, ref, I = case(shape, strict)
    again = f.sift(I, int(strict), one_based=True)
    assert same_bits(again["descriptors"], got["descriptors"]) and same_bits(again["frames"][2:], got["frames"][2:])
    assert same_bits(again["frames"][:2], got["frames"][:2] + 1.0)
    assert np.array_equal(again["counts"], got["counts"])


def test_the_frames_own_image_equals_the_restatement_on_it():
    f, fr, got, ref = loaded_frame(1)
    assert np.array_equal(got["counts"], ref["counts"]) and got["K"] == ref["frames"].shape[1] > 100
    want = np.concatenate([np.vstack([q, np.full((1, q.shape[1]), float(o))]) for o, q in enumerate(ref["refined"])], 1)
    assert same_bits(f.sift_refined(), want)
    one = dict(frames=ref["frames"] + np.array([[1.0], [1.0], [0.0], [0.0]]), descriptors=ref["descriptors"])      # SIFT_extract_save.m:55-56
    compare(got, one, tolerance(), "device 144 x 176, image = NULL")
    # siftmatch of the device descriptors against the restatement's pairs every keypoint with itself
    m = matcher.siftmatch(got["descriptors"], ref["descriptors"], 1.5)
    assert np.array_equal(m[0], np.arange(1, got["K"] + 1)) and np.array_equal(m[1], m[0])


@pytest.mark.parametrize("gate", [0, 1])
def test_gate_is_bit_identical_to_keypoints_fed_with_the_same_set(gate):
    f, fr, got, _ = loaded_frame(1)
    a = f.gate(gate)
    with srm.SrFrame(144, 176) as g:
        g.load(fr, srm.MODE_DR_YE)
        b = g.keypoints(got["frames"], got["descriptors"], gate)
    assert 0 < len(a["keep_idx"]) <= got["K"]
    for k in b:
        assert a[k].shape == b[k].shape and same_bits(a[k].astype(np.float64), b[k].astype(np.float64)), k


def test_vo_pair_is_bit_identical_whether_the_sets_were_made_or_uploaded():
    f1, fr1, got1, _ = loaded_frame(1)
    f2, fr2, got2, _ = loaded_frame(2)
    f1.gate(1); f2.gate(1)
    a = vo.vo_pair_seeded(f1, f2, 5, 0, 1.5)
    with srm.SrFrame(144, 176) as g1, srm.SrFrame(144, 176) as g2:
        g1.load(fr1, srm.MODE_DR_YE); g2.load(fr2, srm.MODE_DR_YE)
        g1.keypoints(got1["frames"], got1["descriptors"], 1); g2.keypoints(got2["frames"], got2["descriptors"], 1)
        b = vo.vo_pair_seeded(g1, g2, 5, 0, 1.5)
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k


def test_error_paths():
    I = R.make_image(37, 45)
    K = C.c_int32(0)

    def rc(h, img, strict):
        return _lib.lib.pre3_sr_frame_sift(h, _lib.dptr(img), strict, 1, C.byref(K), None, None, None)
    with srm.SrFrame(37, 45) as f:
        assert rc(None, I, 1) == E_ARG
        assert _lib.lib.pre3_sr_frame_sift(f._h, _lib.dptr(I), 1, 1, None, None, None, None) == E_ARG
        assert rc(f._h, None, 1) == E_STATE                            # image == NULL before the first load
        bad = I.copy(order="F"); bad[3, 4] = np.nan
        assert rc(f._h, bad, 0) == E_ARG
        bad[3, 4] = 7.5
        assert rc(f._h, bad, 1) == E_ARG and rc(f._h, bad, 0) == 0
        bad[3, 4] = 256.0
        assert rc(f._h, bad, 1) == E_ARG
        out = np.zeros((74, 90), order="F")
        assert _lib.lib.pre3_sr_frame_sift_level(f._h, 9, 0, 0, _lib.dptr(out)) == E_ARG
        assert _lib.lib.pre3_sr_frame_sift_level(f._h, 0, 5, 1, _lib.dptr(out)) == E_ARG
        n = C.c_int32(0)
        assert _lib.lib.pre3_sr_frame_gate(f._h, 0, C.byref(n), None, None, None, None, None) == E_STATE      # no frame loaded
    with srm.SrFrame(7, 45) as f:
        assert rc(f._h, np.zeros((7, 45), order="F"), 1) == E_ARG      # O would be < 1
    with srm.SrFrame(37, 45) as f:
        out = np.zeros((74, 90), order="F")
        assert _lib.lib.pre3_sr_frame_sift_level(f._h, 0, 0, 0, _lib.dptr(out)) == E_STATE


def test_a_load_after_sift_makes_the_record_stale():
    fr = sr.make_frame(37, 45, seed=3, conf=True)
    with srm.SrFrame(37, 45) as f:
        f.load(fr, srm.MODE_XYZ)
        assert f.sift(want_arrays=False)["K"] >= 0
        f.gate(0)
        f.load(fr, srm.MODE_XYZ)
        with pytest.raises(_lib.Pre3Error) as e:
            f.gate(0)
        assert e.value.code == E_STATE


def test_sift_extract_frame_uploads_nothing_and_feeds_set_scan_frame():
    f, fr, got, _ = loaded_frame(2)
    scan = srm.sift_extract_frame(f, 2)
    assert scan["SCALE_ORIENT_POS_RAW"].shape == (4, got["K"]) and scan["XYZ_DATA"].shape[1] == len(scan["keep_idx"]) > 0
    assert same_bits(scan["Descriptor"], scan["Descriptor_RAW"][:, scan["keep_idx"]])


def test_the_ic_search_takes_the_device_made_scan(pre3, orc, sr4000):
    """pre3_set_scan_frame (which = 0: the raw set, 1: the gated one) behind sift() + gate() against pre3_set_scan fed with sift()'s own output"""
    from test_gpu_scan_frame import _context, _pos4, _reset, _same, _search
    fh, fr, got, _ = loaded_frame(1)
    kept = fh.gate(0)
    f, x, P, bank, h = _context(pre3, orc, sr4000, "fixture_f64")
    bank = np.asfortranarray(got["descriptors"][:, :bank.shape[1]])   # the map's descriptors are the scan's first ones: the ranking finds them
    for which, des, frm in ((0, got["descriptors"], got["frames"]), (1, kept["descriptors"], kept["frames"])):
        _reset(f, x, P, bank)
        f.load_scan(des, _pos4(frm))
        ref = _search(f)
        _reset(f, x, P, bank)
        f.set_scan_frame(fh, which)
        _same(_search(f), ref)
    f.close()


def test_gate_refuses_a_set_of_another_shape():
    """a keypoints() upload of 6-entry frames leaves a record gate()'s outputs are not sized for"""
    fr = sr.make_frame(37, 45, seed=3, conf=True)
    frm, des = sr.make_keypoints(20, 37, 45, ldf=6, ND=128, seed=1, specials=False)
    with srm.SrFrame(37, 45) as f:
        f.load(fr, srm.MODE_XYZ)
        f.keypoints(frm, des, 0)
        with pytest.raises(_lib.Pre3Error) as e:
            f.gate(0)
        assert e.value.code == E_ARG
        f.keypoints(frm[:4], des[:32], 0)
        with pytest.raises(_lib.Pre3Error) as e:
            f.gate(0)
        assert e.value.code == E_ARG
        a = f.keypoints(frm[:4], des, 0)                              # (4, K) and (128, K): the gate runs over the uploaded set
        b = f.gate(0)
        for k in a:
            assert same_bits(a[k].astype(np.float64), b[k].astype(np.float64)), k


def _patch_image(M, N):
    """a flat image with the 69 x 85 texture in its middle: few keypoints, so that the restatement of a large image stays quick"""
    I = np.full((M, N), 128.0, order="F")
    I[M // 2 - 34:M // 2 + 35, N // 2 - 42:N // 2 + 43] = R.make_image(69, 85)
    return I


def test_more_keypoints_than_the_cap_leave_an_empty_record_and_a_usable_handle():
    """512 x 512 of the dense texture: 10551 refined points (below the candidate cap), 13382 keypoints (above PRE3_SR_MAX_KEYPOINTS), counted on the CPU
    with the header built for the host.  PRE3_E_NOMEM after the wait, K_out = 0, gate() keeps nothing; the next sift() on the handle is right."""
    M = N = 512
    fr = sr.make_frame(M, N, seed=4, conf=True)
    K = C.c_int32(-1)
    counts = np.zeros((32, 4), np.int32)
    with srm.SrFrame(M, N) as f:
        f.load(fr, srm.MODE_XYZ)
        dense = R.fine_texture(M, N)
        assert _lib.lib.pre3_sr_frame_sift(f._h, _lib.dptr(dense), 0, 1, C.byref(K), None, None, _lib.dptr(counts)) == E_NOMEM
        assert K.value == 0 and counts[:, 2].sum() == 10551 and counts[:, 3].sum() == 13382
        assert len(f.gate(0)["keep_idx"]) == 0
        n = C.c_int32(0)
        assert _lib.lib.pre3_sr_frame_sift_refined(f._h, C.byref(n), None) == E_STATE
        I = _patch_image(M, N)
        got, ref = f.sift(I, 1, one_based=False), R.sift_vedal(I, True, pl=lib_plan(M, N))
        assert np.array_equal(got["counts"], ref["counts"]) and got["K"] == ref["frames"].shape[1] > 50
        compare(got, ref, tolerance(), "device 512 x 512 after an overflow")
        assert len(f.gate(0)["keep_idx"]) > 0


def test_more_refined_points_than_the_candidate_cap():
    """1100 x 1100 of the dense texture: 50711 refined points, above PRE3_SIFT_MAX_CANDIDATES (counted on the CPU with the header built for the host)"""
    M = N = 1100
    K = C.c_int32(-1)
    counts = np.zeros((32, 4), np.int32)
    with srm.SrFrame(M, N) as f:
        dense = R.fine_texture(M, N)
        assert _lib.lib.pre3_sr_frame_sift(f._h, _lib.dptr(dense), 0, 1, C.byref(K), None, None, _lib.dptr(counts)) == E_NOMEM
        assert K.value == 0 and counts[:, 2].sum() == 50711
        I = R.make_image(69, 85)
    with srm.SrFrame(69, 85) as f:                                    # (the library is as usable as before)
        assert f.sift(I, 1)["K"] == case((69, 85), True)[1]["K"]


def _texture_planes(seed):
    fr = sr.make_frame(144, 176, seed=seed, conf=True)
    fr["amp"] = np.asfortranarray((R.make_image(144, 176, seed=40 + seed) / 255.0) ** 2 * 9000.0 + 1.0)
    return fr


def test_vodometry_frames_on_two_dat_files_equals_the_host_fed_twin(tmp_path):
    from test_gpu_vo_pair import _write_dat, assert_same_result
    d1, d2 = tmp_path / "d1_0001.dat", tmp_path / "d1_0002.dat"
    _write_dat(d1, _texture_planes(1)); _write_dat(d2, _texture_planes(1))      # the same scan twice: every keypoint has its match
    out = srm.vodometry_frames(str(d1), str(d2), 5, 0)
    sets = []
    for d in (d1, d2):
        with srm.SrFrame(144, 176) as f:
            f.load(srm.load_dat(str(d)), srm.MODE_DR_YE)
            s = f.sift()
            sets.append((s["frames"], s["descriptors"]))
    twin = srm.vodometry_dr_ye(str(d1), str(d2), sets[0], sets[1], 5, 0)
    assert np.array_equal(out["kept1"], twin["kept1"]) and np.array_equal(out["kept2"], twin["kept2"])
    assert out["pnum"] == twin["pnum"] > 100 and np.array_equal(out["match"], twin["match"])
    assert_same_result(out, twin)


def test_initialize_features_scans_on_two_dat_files_equals_the_host_fed_twin(pre3, orc, tmp_path):
    import frame_policy_cases as fp
    from test_gpu_frame_policy import SEED, SEQ, _write_dat, chain, context, kwargs, same_result, same_state, state
    c = chain("p129", orc)["c"]
    d1, d2 = tmp_path / "d1_0001.dat", tmp_path / "d1_0002.dat"
    _write_dat(d1, _texture_planes(1)); _write_dat(d2, _texture_planes(1))
    sets = []
    for d in (d1, d2):
        with srm.SrFrame(144, 176) as f:
            f.load(srm.load_dat(str(d)), srm.MODE_XYZ)
            s = f.sift()
            sets.append((s["frames"], s["descriptors"]))
    f, g = context(pre3, c, "f32"), context(pre3, c, "f32")
    out = srm.initialize_features_scans(f, c["step"], str(d1), str(d2), SEED, SEQ, fp.THRESH, **kwargs(c, True))
    twin = srm.initialize_features_frames(g, c["step"], str(d1), str(d2), sets[0], sets[1], SEED, SEQ, fp.THRESH, **kwargs(c, True))
    assert np.array_equal(out["kept_prev"], twin["kept_prev"]) and np.array_equal(out["kept_cur"], twin["kept_cur"])
    same_result(out, twin); same_state(state(pre3, f), state(pre3, g))
    assert out["K"] > 100 and np.array_equal(out["cand_idx"], twin["cand_idx"])
    f.close(); g.close()
