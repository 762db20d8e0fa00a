"""GPU: the SR4000 frame conditioned on the device (k_sr_maxima, k_sr_condition, k_sr_keypoints) against the numpy restatement
tests/sr_frame_ref.py (a), which is fed the library's own pre3_sr_gauss3 weights.

Everything is compared EXACTLY: the filtered planes, the image, xyz and rho bit for bit (NaN sets equal, every other entry the same 64 bits), imax and
cmax as values, keep_idx / n_kept / frames / descriptors as arrays.  The kernels add the nine products in the restatement's order with no contraction,
and fp64 sqrt and division are correctly rounded on both sides, so no tolerance is needed.  Sizes: smaller than the 16 x 16 tile, one pixel past it
(17), several tiles with a ragged edge (70), the real 144 x 176.  No test feeds the device an out-of-range pixel: the host check refuses it first."""
import ctypes as C
import importlib

import numpy as np
import pytest

import sr_frame_ref as sr
from test_sr_frame_ref import same_bits

pytestmark = pytest.mark.gpu
srm = importlib.import_module("3pre_amd.sr4000")
plane = importlib.import_module("3pre_amd.plane")
scanio = importlib.import_module("3pre_amd.scanio")
_lib = importlib.import_module("3pre_amd._lib")

SIZES = ((1, 1), (1, 5), (5, 1), (3, 3), (17, 70), (144, 176))
K_SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 2048, 8192)      # a wave and its edges; one workgroup of 256 and its edges; 8 workgroups; the cap (32)
E_ARG, E_STATE = -1, -4
_W, _KP = {}, {}


def weights(mode):
    """the library's own bits, as the conditioning launch uses them"""
    if mode not in _W:
        _W[mode] = srm.gauss3(2.0 if mode == 0 else 1.0).T.ravel()
        _W[mode].setflags(write=False)
    return _W[mode]


def kp_case(mode):
    """the keypoint frame and its restatement, computed once per mode and shared"""
    if mode not in _KP:
        fr = sr.make_keypoint_frame(weights(mode), mode)
        _KP[mode] = (fr, sr.condition(fr, mode, weights(mode)))
    return _KP[mode]


def assert_frame(f, ref):
    x, y, z, conf = f.planes()
    for got, k in ((x, "x"), (y, "y"), (z, "z")):
        assert same_bits(got, ref[k]), k
    assert np.array_equal(f.image(), ref["img"].astype(np.uint8))
    imax, cmax = f.maxima()
    assert imax == ref["imax"] and (cmax == ref["cmax"] or (np.isnan(cmax) and np.isnan(ref["cmax"])))
    if ref["conf"] is None:
        assert conf is None
    else:
        assert same_bits(conf, ref["conf"])


def assert_keypoints(got, ref, gate):
    assert np.array_equal(got["keep_idx"], ref["keep_idx"]) and got["keep_idx"].dtype == np.int32
    assert np.array_equal(got["frames"], ref["frames"]) and np.array_equal(got["descriptors"], ref["descriptors"])
    if gate == 0:
        assert same_bits(got["xyz"], ref["xyz"]) and same_bits(got["rho"], ref["rho"])


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", SIZES)
def test_planes_image_and_maxima_are_bit_equal(pre3, shape, mode):
    assert pre3.device_count() >= 1
    fr = sr.make_frame(*shape)
    ref = sr.condition(fr, mode, weights(mode))
    with srm.SrFrame(*shape) as f:
        assert_frame(f.load(fr, mode), ref)
        assert not np.isnan(f.planes()[0]).any()
        if shape == (144, 176):
            assert ref["img"].max() > 100 and (fr["amp"] > sr.SATURATED).sum() > 50 and ref["imax"] < 30000.0


@pytest.mark.parametrize("mode", [0, 1])
def test_planted_nan_pixels(pre3, mode):
    fr = sr.make_frame(17, 70, seed=1)
    fr["x"][8, 30] = np.nan                                        # interior: on no tile edge
    fr["x"][15, 16] = np.nan                                       # next to the tile boundaries at row 16 and column 16
    fr["y"][0, 40] = np.nan; fr["y"][9, 69] = np.nan               # on an edge
    fr["z"][0, 0] = np.nan; fr["z"][16, 69] = np.nan               # in a corner
    fr["z"][5, 5] = -0.0
    ref = sr.condition(fr, mode, weights(mode))
    assert np.isnan(ref["x"]).sum() == 18 and np.isnan(ref["y"]).sum() == 12 and np.isnan(ref["z"]).sum() == 8
    with srm.SrFrame(17, 70) as f:
        assert_frame(f.load(fr, mode), ref)


@pytest.mark.parametrize("mode", [0, 1])
def test_amplitude_cases(pre3, mode):
    with srm.SrFrame(17, 70) as f:
        fr = sr.make_frame(17, 70, seed=2)                         # some pixels above 65000, one at 0
        assert (fr["amp"] > sr.SATURATED).any() and (fr["amp"] == 0).any()
        assert_frame(f.load(fr, mode), sr.condition(fr, mode, weights(mode)))
        fr["amp"][:] = 65001.0 + np.arange(17 * 70).reshape(17, 70) % 500      # every pixel saturated: imax = 0, 0 / 0 -> uint8(NaN) = 0
        f.load(fr, mode)
        assert f.maxima()[0] == 0.0 and not f.image().any()
        assert_frame(f, sr.condition(fr, mode, weights(mode)))
        fr["amp"][:] = 0.0                                         # a black frame
        f.load(fr, mode)
        assert f.maxima()[0] == 0.0 and not f.image().any()
        fr["amp"][:] = 65000.0                                     # exactly at the threshold: not saturated
        f.load(fr, mode)
        assert f.maxima()[0] == 65000.0
        assert_frame(f, sr.condition(fr, mode, weights(mode)))
        assert f.image()[8, 30] == 255


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("case", ["all_nan", "one_nan", "none"])
def test_confidence_cases(pre3, mode, case):
    fr = sr.make_frame(17, 70, seed=3)
    if case == "all_nan":
        fr["conf"][:] = np.nan
    elif case == "one_nan":
        fr["conf"][np.unravel_index(np.argmax(fr["conf"]), fr["conf"].shape)] = np.nan       # the largest entry: cmax is the second largest
    else:
        fr["conf"] = None
    ref = sr.condition(fr, mode, weights(mode))
    assert np.isnan(ref["cmax"]) == (case != "one_nan")
    frm, des = sr.make_keypoints(300, 17, 70, seed=5)
    with srm.SrFrame(17, 70) as f:
        assert_frame(f.load(fr, mode), ref)
        assert_keypoints(f.keypoints(frm, des, 0), sr.keypoints(ref, frm, des, 0), 0)
        if case == "none":
            with pytest.raises(pre3.Pre3Error) as e:
                f.keypoints(frm, des, 1)
            assert e.value.code == E_ARG and "confidence" in str(e.value)
        else:
            assert_keypoints(f.keypoints(frm, des, 1), sr.keypoints(ref, frm, des, 1), 1)      # all NaN: no comparison is true, all are kept
        if case == "all_nan":
            assert len(f.keypoints(frm, des, 1)["keep_idx"]) == 300


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("K", K_SIZES)
def test_keypoints_both_gates(pre3, K, mode):
    fr, ref = kp_case(mode)
    frm, des = sr.make_keypoints(K, seed=mode)
    with srm.SrFrame() as f:
        f.load(fr, mode)
        for gate in (0, 1):
            want = sr.keypoints(ref, frm, des, gate)
            got = f.keypoints(frm, des, gate)
            assert_keypoints(got, want, gate)
            again = f.keypoints(frm, des, gate)                    # a second identical call is bit-equal
            assert all(same_bits(got[k], again[k]) for k in got if k != "keep_idx") and np.array_equal(got["keep_idx"], again["keep_idx"])
            if K >= 63:
                assert 0 < len(want["keep_idx"]) < K
        if K >= 21:
            k0, k1 = set(f.keypoints(frm, des, 0)["keep_idx"].tolist()), set(f.keypoints(frm, des, 1)["keep_idx"].tolist())
            assert not k0 & {0, 1, 2} and {0, 1, 2} <= k1          # confidence exactly 0.5 cmax: <= drops, < keeps
            assert {3, 4, 5} <= k0 and not k0 & {6, 7, 8}          # range exactly 0.4 kept, the double below dropped
            assert not k0 & {9, 10, 11} and {12, 13, 14} <= k0     # a NaN x dropped, a NaN y alone kept


@pytest.mark.parametrize("ldf,ND", [(2, 0), (3, 5), (4, 128), (5, 6)])
def test_frame_and_descriptor_widths(pre3, ldf, ND):
    """odd widths take the 8-byte copy, even ones the 16-byte copy; ND = 0 copies no descriptor"""
    fr, ref = kp_case(0)
    frm, des = sr.make_keypoints(700, ldf=ldf, ND=ND, seed=9)
    with srm.SrFrame() as f:
        f.load(fr, 0)
        for gate in (0, 1):
            assert_keypoints(f.keypoints(frm, des if ND else None, gate), sr.keypoints(ref, frm, des, gate), gate)


@pytest.mark.parametrize("K", [600, 8192])
def test_all_kept_none_kept_and_only_the_last_kept(pre3, K):
    fr, ref = kp_case(1)
    good, bad = (sr.PX_GOOD[1] + 1.0, sr.PX_GOOD[0] + 1.0), (sr.PX_BAD[1] + 1.0, sr.PX_BAD[0] + 1.0)
    frm, des = sr.make_keypoints(K, specials=False, seed=11)
    with srm.SrFrame() as f:
        f.load(fr, 1)
        for gate in (0, 1):
            frm[0], frm[1] = good
            out = f.keypoints(frm, des, gate)
            assert np.array_equal(out["keep_idx"], np.arange(K)) and np.array_equal(out["descriptors"], des)
            assert_keypoints(out, sr.keypoints(ref, frm, des, gate), gate)
            frm[0], frm[1] = bad
            out = f.keypoints(frm, des, gate)
            assert len(out["keep_idx"]) == 0 and out["frames"].shape == (4, 0) and out["descriptors"].shape == (128, 0)
            frm[0, K - 1], frm[1, K - 1] = good                    # the last keypoint of the last workgroup
            out = f.keypoints(frm, des, gate)
            assert out["keep_idx"].tolist() == [K - 1] and np.array_equal(out["descriptors"][:, 0], des[:, K - 1])
            assert_keypoints(out, sr.keypoints(ref, frm, des, gate), gate)


def test_a_second_load_replaces_the_frame(pre3):
    fa, ra = kp_case(0)
    fb = sr.make_frame(144, 176, seed=21)
    rb = sr.condition(fb, 1, weights(1))
    frm, des = sr.make_keypoints(700, seed=2)
    with srm.SrFrame() as f:
        f.load(fa, 0)
        assert_keypoints(f.keypoints(frm, des, 0), sr.keypoints(ra, frm, des, 0), 0)
        f.load(fb, 1)                                              # another frame, the other mode
        assert_frame(f, rb)
        for gate in (0, 1):
            assert_keypoints(f.keypoints(frm, des, gate), sr.keypoints(rb, frm, des, gate), gate)
        f.load(fa, 0).load(fb, 1).load(fa, 0)                      # queued back to back: the staging block is not overwritten under a transfer
        assert_frame(f, ra)


def test_calls_before_a_load_are_state_errors(pre3):
    lib = _lib.lib
    frm, des = sr.make_keypoints(4, 17, 70)
    with srm.SrFrame(17, 70) as f:
        for call in (f.planes, f.image, f.maxima, lambda: f.keypoints(frm, des, 0)):
            with pytest.raises(pre3.Pre3Error) as e:
                call()
            assert e.value.code == E_STATE
    h = C.c_void_p()
    for rows, cols in ((0, 5), (5, 0), (-1, -1)):
        assert lib.pre3_sr_frame_create(C.byref(h), 0, rows, cols) == E_ARG and not h
    assert lib.pre3_sr_frame_create(None, 0, 5, 5) == E_ARG
    assert lib.pre3_sr_frame_destroy(None) == 0


def test_every_argument_error_leaves_the_frame_readable_and_unchanged(pre3):
    lib, dptr = _lib.lib, _lib.dptr
    rows, cols = 17, 70
    fr = sr.make_frame(rows, cols, seed=4)
    ref = sr.condition(fr, 0, weights(0))
    frm, des = sr.make_keypoints(40, rows, cols, seed=1)
    want = sr.keypoints(ref, frm, des, 0)
    n = C.c_int32(-7)
    idx = np.full(64, -7, np.int32)
    with srm.SrFrame(rows, cols) as f:
        f.load(fr, 0)
        z, x, y, amp, conf = (np.asfortranarray(fr[k]) for k in ("z", "x", "y", "amp", "conf"))

        def load(mode=0, z=z, x=x, y=y, amp=amp, conf=conf):
            return lib.pre3_sr_frame_load(f._h, mode, dptr(z), dptr(x), dptr(y), dptr(amp), dptr(conf))

        def bad_amp(v):
            a = amp.copy(order="F"); a[3, 7] = v
            return a

        def kp(gate=0, ldf=4, K=40, frm=frm, ND=128, des=des, n_kept=n, h=None):
            return lib.pre3_sr_frame_keypoints(f._h if h is None else h, gate, ldf, K, dptr(frm), ND, dptr(des),
                                               None if n_kept is None else C.byref(n_kept), dptr(idx), None, None, None, None)

        def moved(u=None, v=None):
            g = frm.copy(order="F")
            if u is not None:
                g[0, 17] = u
            if v is not None:
                g[1, 17] = v
            return g

        errors = [lambda: load(mode=2), lambda: load(mode=-1), lambda: load(z=None), lambda: load(x=None), lambda: load(y=None), lambda: load(amp=None),
                  lambda: load(amp=bad_amp(-1.0)), lambda: load(amp=bad_amp(np.nan)), lambda: load(amp=bad_amp(np.inf)),
                  lambda: lib.pre3_sr_frame_load(None, 0, dptr(z), dptr(x), dptr(y), dptr(amp), None),
                  lambda: kp(gate=2), lambda: kp(gate=-1), lambda: kp(K=-1), lambda: kp(K=8193), lambda: kp(ldf=1), lambda: kp(ND=-1),
                  lambda: kp(frm=None), lambda: kp(des=None), lambda: kp(n_kept=None), lambda: kp(h=C.c_void_p()),
                  lambda: kp(frm=moved(u=np.nan)), lambda: kp(frm=moved(v=np.inf)), lambda: kp(frm=moved(u=0.49)), lambda: kp(frm=moved(u=cols + 0.5)),
                  lambda: kp(frm=moved(v=0.0)), lambda: kp(frm=moved(v=rows + 0.5)), lambda: kp(frm=moved(u=-3.0)), lambda: kp(frm=moved(v=1e300))]
        for i, call in enumerate(errors):
            assert call() == E_ARG, i
            assert b"pre3_sr_frame" in lib.pre3_last_error()
            assert (idx == -7).all()                               # nothing was launched or written
            assert_frame(f, ref)
            assert_keypoints(f.keypoints(frm, des, 0), want, 0)
        assert lib.pre3_sr_frame_get(f._h, None, None, None, None, None, None, None) == 0
        assert kp(K=0, frm=None, des=None) == 0 and n.value == 0   # K = 0 launches nothing
        assert kp(frm=moved(u=0.5, v=rows + 0.49)) == 0 and n.value >= 0      # the outermost legal positions
        # a frame without a confidence map: gate 1 and a confidence read-back are argument errors, the frame stays
        f.load(dict(fr, conf=None), 0)
        ref2 = sr.condition(dict(fr, conf=None), 0, weights(0))
        assert kp(gate=1) == E_ARG
        assert lib.pre3_sr_frame_get(f._h, None, None, None, None, dptr(np.zeros((rows, cols), order="F")), None, None) == E_ARG
        assert_frame(f, ref2)


def _write_dat(path, fr, timestamp=None):
    a = np.vstack([fr[k] for k in ("z", "x", "y", "amp")] + ([fr["conf"]] if fr["conf"] is not None else []))
    if timestamp is not None:
        a = np.vstack([a, np.r_[timestamp, np.zeros(a.shape[1] - 1)]])
    np.savetxt(path, a, fmt="%.17g")


def test_a_dat_frame_through_the_plane_fit(pre3, tmp_path):
    """read_xyz_sr4000 on a synthetic .dat frame of a tilted floor -> plane_fit_seeded, against the same fit on the restatement's planes"""
    rng = np.random.default_rng(6)
    r, c = np.mgrid[0:144, 0:176]
    fr = sr.make_frame(144, 176, seed=30)
    fr["x"] = np.asfortranarray((88.0 - c) * 0.012 + rng.normal(0, 0.002, c.shape))
    fr["y"] = np.asfortranarray((72.0 - r) * 0.012 + rng.normal(0, 0.002, c.shape))
    fr["z"] = np.asfortranarray(2.5 + 1.3 * fr["y"] + 0.1 * fr["x"] + rng.normal(0, 0.003, c.shape))      # a tilted floor
    path = tmp_path / "d1_0012.dat"
    _write_dat(path, fr, timestamp=99.5)
    x, y, z, conf, ts = srm.read_xyz_sr4000(str(path), with_timestamp=True)
    ref = sr.condition(fr, 0, weights(0))
    assert same_bits(x, ref["x"]) and same_bits(y, ref["y"]) and same_bits(z, ref["z"]) and np.array_equal(conf, fr["conf"]) and ts == 99.5
    a = plane.plane_fit_seeded(x, y, z, 20261018, 3, n_draw=200)
    b = plane.plane_fit_seeded(ref["x"], ref["y"], ref["z"], 20261018, 3, n_draw=200)
    assert a["sta"] == 1 and a["n_inliers"] > 1000
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    # the other readers on the same file
    assert np.array_equal(srm.read_image_sr4000(str(path)), ref["img"].astype(np.uint8))
    r1 = sr.condition(fr, 1, weights(1))
    x1, y1, z1, c1, img1 = srm.read_sr4000_data_dr_ye(str(path))
    assert same_bits(x1, r1["x"]) and same_bits(y1, r1["y"]) and same_bits(z1, r1["z"]) and np.array_equal(img1, r1["img"].astype(np.uint8))
    assert img1.dtype == np.uint8 and np.array_equal(c1, fr["conf"])


def test_sift_extract_and_confidence_filtering(pre3, tmp_path):
    fr, ref = kp_case(0)
    frm, des = sr.make_keypoints(300, seed=4)
    with srm.SrFrame() as f:
        f.load(fr, 0)
        scan = srm.sift_extract(frm, des, f, 12)
        f2, d2 = srm.confidence_filtering(frm, des, f)
    w0, w1 = sr.keypoints(ref, frm, des, 0), sr.keypoints(ref, frm, des, 1)
    assert np.array_equal(f2, w1["frames"]) and np.array_equal(d2, w1["descriptors"])
    assert scan["idxScan"] == 12 and np.array_equal(scan["Image"], ref["img"].astype(np.uint8))
    assert np.array_equal(scan["Descriptor_RAW"], des) and np.array_equal(scan["SCALE_ORIENT_POS_RAW"], frm)
    assert np.array_equal(scan["Descriptor"], w0["descriptors"]) and np.array_equal(scan["SCALE_ORIENT_POS"], w0["frames"])
    assert same_bits(scan["XYZ_DATA"], w0["xyz"])
    path = str(tmp_path / "SIFT_result0012.mat")
    scanio.save_sift_result(path, scan)
    back = scanio.load_sift_result(path)
    assert same_bits(back["XYZ_DATA"], w0["xyz"]) and np.array_equal(back["Descriptor"], w0["descriptors"])
