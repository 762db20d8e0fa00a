"""GPU: low-confidence pixels compensated by a 3 x 3 median on the resident frame (pre3_sr_frame_set_compensation, pre3_sr_frame_bad_pixels,
pre3_sr_medfilt3) against the numpy statement tests/sr_median_ref.py (a), which is fed the library's own pre3_sr_gauss3 weights (host only, pinned against the
closed form by tests/test_sr_frame_ref.py).

There are no tolerances: a median is a selection and the Gaussian behind it is the arithmetic section 20 pins.  Equal means equal as values (-0 equals
+0) with NaNs in the same places (sr_median_ref.same); "bit for bit" means sr_frame_ref's NaN sets and bits.  One 144 x 176 case; everything else runs
at (1, 1), (1, 5), (5, 1), (2, 2), (3, 3) and (17, 70), which crosses the tile rows 15 | 16 and the tile columns at 16, 32, 48 and 64."""
import importlib
import io

import numpy as np
import pytest

import sr_frame_ref as sr
import sr_median_ref as mr

pytestmark = pytest.mark.gpu
srm = importlib.import_module("3pre_amd.sr4000")
plane = importlib.import_module("3pre_amd.plane")
_lib = importlib.import_module("3pre_amd._lib")
E_ARG, E_STATE = -1, -4
KEYS = ("x", "y", "z", "img")
W = {mode: srm.gauss3(2.0 if mode == 0 else 1.0).T.ravel() for mode in (0, 1)}      # the library's own pre3_sr_gauss3 weights, as section 20's suite feeds (a)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64)))


def state(f):
    x, y, z, _ = f.planes()
    return dict(x=x, y=y, z=z, img=f.image().astype(np.float64))


def check_frame(f, ref, what=""):
    got = state(f)
    for k in KEYS:
        assert mr.same(got[k], ref[k]), (what, k)
    imax, cmax = f.maxima()
    assert imax == ref["imax"] and (cmax == ref["cmax"] or (np.isnan(cmax) and np.isnan(ref["cmax"]))), what
    return got


# ---- 1. pre3_sr_medfilt3 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("padding", ["zeros", "symmetric"])
@pytest.mark.parametrize("shape", mr.SIZES)
def test_medfilt3_against_the_numpy_statement(shape, padding):
    rng = np.random.default_rng(13 * shape[0] + shape[1])
    a = rng.normal(0.0, 3.0, shape)
    u = np.floor(rng.uniform(0, 256, shape))
    for p in (a, u, u.astype(np.uint8)):
        got = srm.medfilt2(p, padding)
        assert got.shape == shape and got.dtype == np.float64 and mr.same(got, mr.medfilt3(p, padding))
    if shape == (17, 70):
        for px in ((8, 30), (15, 16), (16, 47), (0, 40), (9, 69), (16, 69), (0, 0)):     # interior, beside tile boundaries, on edges, in corners
            a[px] = np.nan
        ref = mr.medfilt3(a, padding)
        assert np.isnan(ref).sum() > 30 and mr.same(srm.medfilt2(a, padding), ref)
        assert np.isnan(srm.medfilt2(np.full(shape, np.nan), padding)).all()


def test_medfilt3_argument_errors():
    a, out = np.zeros((3, 4), order="F"), np.full((3, 4), 7.0, order="F")
    rc = _lib.lib.pre3_sr_medfilt3
    assert rc(0, 3, 4, None, 0, _lib.dptr(out)) == E_ARG and rc(0, 3, 4, _lib.dptr(a), 0, None) == E_ARG
    for padding in (-1, 2):
        assert rc(0, 3, 4, _lib.dptr(a), padding, _lib.dptr(out)) == E_ARG
    for r, c in ((0, 4), (3, 0), (-3, 4), (3, -1), (1 << 14, (1 << 12) + 1)):
        assert rc(0, r, c, _lib.dptr(a), 0, _lib.dptr(out)) == E_ARG
    assert (out == 7.0).all()
    with pytest.raises(ValueError):
        srm.medfilt2(a, "replicate")
    assert rc(0, 3, 4, _lib.dptr(a), 1, _lib.dptr(out)) == 0 and not out.any()


# ---- 2. frames in modes 0 and 1 under forms 1 and 2 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [mr.BADPIXEL, mr.IMAGE_MEDIAN])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", mr.SIZES)
def test_frames_against_the_numpy_statement(shape, mode, form):
    rows, cols = shape
    w = W[mode]
    fr, n_bad = mr.planted_frame(rows, cols, seed=mode)
    with srm.SrFrame(rows, cols) as f, srm.SrFrame(rows, cols) as f0:
        f.set_compensation(form, mr.CUTOFF)
        # the planted pixels: corners, edges, rows and columns 15 .. 17, the 2 x 2 block, confidence == cutoff and NaN
        ref = mr.condition(fr, mode, w, form)
        f.load(fr, mode)
        check_frame(f, ref, "planted")
        assert f.bad_pixels() == (form, n_bad if form == mr.BADPIXEL else 0) and ref["n_bad"] == f.bad_pixels()[1]
        assert same_bits(f.planes()[3], fr["conf"])                          # the confidence map as loaded
        if shape == (17, 70) and form == mr.BADPIXEL:
            bad, block, at_cutoff, nan_conf = mr.planted_pixels(rows, cols)
            mask = mr.bad_mask(fr["conf"], mr.CUTOFF, shape)
            assert fr["conf"][at_cutoff] == mr.CUTOFF and np.isnan(fr["conf"][nan_conf]) and not mask[at_cutoff] and not mask[nan_conf]
            seq = dict(fr)                                                    # the test's data tells the rule from a sequential replacement
            for k in ("x", "y", "z"):
                seq[k] = mr.compensate_sequential(fr[k], fr["conf"], mr.CUTOFF)
                assert any(seq[k][p] != mr.compensate(fr[k], fr["conf"], mr.CUTOFF)[p] for p in block), k
            seq["conf"] = None
            wrong = sr.condition(seq, mode, w)
            got = state(f)
            assert all(not mr.same(got[k], wrong[k]) for k in ("x", "y", "z"))
        # every pixel bad
        allbad = dict(fr)
        allbad["conf"] = np.zeros((rows, cols), order="F")                   # all below the cut-off
        allbad["conf"][0, 0] = np.nextafter(mr.CUTOFF, 0.0)
        ref = mr.condition(allbad, mode, w, form)
        f.load(allbad, mode)
        check_frame(f, ref, "every pixel bad")
        assert f.bad_pixels() == (form, rows * cols if form == mr.BADPIXEL else 0)
        # no pixel bad: under form 1 the form-0 load of the same planes, bit for bit
        good = dict(fr)
        good["conf"] = np.asfortranarray(np.maximum(np.nan_to_num(fr["conf"], nan=mr.CUTOFF), mr.CUTOFF))
        good["conf"][0, 0] = mr.CUTOFF                                       # exactly the cut-off: not bad
        f.load(good, mode)
        f0.load(good, mode)
        check_frame(f, mr.condition(good, mode, w, form), "no pixel bad")
        assert f.bad_pixels() == (form, 0) and f0.bad_pixels() == (0, 0)
        if form == mr.BADPIXEL:
            a, b = state(f), state(f0)
            assert all(same_bits(a[k], b[k]) for k in KEYS)
        # no confidence map: form 1 is a no-op, form 2 still filters the image
        bare = dict(fr)
        bare["conf"] = None
        f.load(bare, mode)
        f0.load(bare, mode)
        check_frame(f, mr.condition(bare, mode, w, form), "no confidence map")
        assert f.bad_pixels() == (form, 0)
        a, b = state(f), state(f0)
        assert all(same_bits(a[k], b[k]) for k in ("x", "y", "z"))
        if form == mr.BADPIXEL:
            assert same_bits(a["img"], b["img"])
        elif shape == (17, 70):
            assert not mr.same(a["img"], b["img"])


def test_the_144_by_176_frame():
    fr, n_bad = mr.planted_frame(144, 176, seed=5)
    fr["x"][14, 89] = np.nan                                                 # in the window of the planted pixel (15, 88): its compensated x is NaN
    with srm.SrFrame() as f:
        f.set_compensation(srm.COMP_BADPIXEL, mr.CUTOFF)
        f.load(fr, srm.MODE_DR_YE)
        check_frame(f, mr.condition(fr, 1, W[1], mr.BADPIXEL))
        assert f.bad_pixels() == (1, n_bad) and n_bad > 20
        f.set_compensation(srm.COMP_IMAGE_MEDIAN)
        f.load(fr, srm.MODE_XYZ)
        check_frame(f, mr.condition(fr, 0, W[0], mr.IMAGE_MEDIAN))
        assert f.bad_pixels() == (2, 0)


# ---- 3. form 0 after the setter has been set and cleared ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_form_0_after_set_and_clear_is_the_untouched_handle(mode):
    fr, _ = mr.planted_frame(17, 70, seed=7)
    fr["y"][4, 4] = np.nan
    with srm.SrFrame(17, 70) as f, srm.SrFrame(17, 70) as f0:
        f0.load(fr, mode)
        assert f.compensation == (0, 1.0) == f0.compensation
        f.set_compensation(srm.COMP_BADPIXEL, 5.0).load(fr, mode)
        f.set_compensation(srm.COMP_IMAGE_MEDIAN).load(fr, mode)
        f.set_compensation(srm.COMP_NONE).load(fr, mode)
        a, b = state(f), state(f0)
        assert all(same_bits(a[k], b[k]) for k in KEYS)
        assert f.maxima() == f0.maxima() and f.bad_pixels() == (0, 0) == f0.bad_pixels()
        ref = sr.condition(fr, mode, W[mode])                               # and both are section 20's frame
        assert all(same_bits(a[k], ref[k]) for k in KEYS)


# ---- 4. the setting applies only to later loads -------------------------------------------------------------------------------------------------------
def test_the_setting_applies_to_later_loads_only():
    rows, cols, mode = 17, 70, 1
    fr, n_bad = mr.planted_frame(rows, cols, seed=2)
    refs = {form: mr.condition(fr, mode, W[mode], form) for form in (0, 1, 2)}
    with srm.SrFrame(rows, cols) as f:
        with pytest.raises(srm.Pre3Error) as e:
            f.bad_pixels()
        assert e.value.code == E_STATE
        f.load(fr, mode)
        before = state(f)
        f.set_compensation(srm.COMP_BADPIXEL, mr.CUTOFF)
        assert f.compensation == (1, mr.CUTOFF) and f.bad_pixels() == (0, 0)       # the resident frame is as it was
        after = state(f)
        assert all(same_bits(before[k], after[k]) for k in KEYS)
        # three loads queued back to back, the setting changed between them: each comes out under its own
        for order in ((1, 2, 0), (2, 0, 1), (0, 1, 2)):
            for form in order:
                f.set_compensation(form, mr.CUTOFF).load(fr, mode)
            check_frame(f, refs[order[-1]], order)
            assert f.bad_pixels() == (order[-1], n_bad if order[-1] == 1 else 0)
        for form in (1, 2, 0, 2, 1):
            f.set_compensation(form, mr.CUTOFF).load(fr, mode)
            check_frame(f, refs[form], form)
            assert f.bad_pixels() == (form, n_bad if form == 1 else 0)
        # another cut-off is another frame
        f.set_compensation(1, 0.0).load(fr, mode)
        assert f.bad_pixels() == (1, 0)
        check_frame(f, refs[0])
        # the setter's argument errors leave the setting unchanged
        f.set_compensation(1, 12.5)
        rc = _lib.lib.pre3_sr_frame_set_compensation
        assert rc(None, 0, 1.0) == E_ARG
        for form, cutoff in ((3, 1.0), (-1, 1.0), (1, float("nan")), (1, float("inf")), (1, float("-inf"))):
            assert rc(f._h, form, cutoff) == E_ARG
            assert f.compensation == (1, 12.5)
        assert _lib.lib.pre3_sr_frame_get_compensation(None, None, None) == E_ARG and _lib.lib.pre3_sr_frame_bad_pixels(None, None, None) == E_ARG
        assert rc(f._h, 2, float("nan")) == 0 and f.compensation[0] == 2            # the cut-off matters to form 1 only


# ---- 5. load_text under form 1 ------------------------------------------------------------------------------------------------------------------------
def frame_text(fr):
    buf = io.BytesIO()
    np.savetxt(buf, np.vstack([fr[k] for k in ("z", "x", "y", "amp", "conf")]), fmt="%.17g")
    return buf.getvalue()


@pytest.mark.parametrize("mode", [0, 1])
def test_load_text_under_form_1(mode):
    rows, cols = 17, 70
    fr, n_bad = mr.planted_frame(rows, cols, seed=4)
    text = frame_text(fr)
    with srm.SrFrame(rows, cols) as f, srm.SrFrame(rows, cols) as g:
        f.set_compensation(srm.COMP_BADPIXEL, mr.CUTOFF)
        g.set_compensation(srm.COMP_BADPIXEL, mr.CUTOFF)
        f.load_text(text, mode)
        g.load(srm.load_dat(io.BytesIO(text), rows), mode)
        a, b = state(f), state(g)
        assert all(a[k].tobytes() == b[k].tobytes() for k in KEYS)
        assert f.bad_pixels() == (1, n_bad) == g.bad_pixels() and f.maxima()[0] == g.maxima()[0]
        check_frame(f, mr.condition(fr, mode, W[mode], mr.BADPIXEL))
        # a refused text leaves the previous frame, its form and its count -- whatever the setting has become
        f.set_compensation(srm.COMP_IMAGE_MEDIAN)
        for bad in (b"1d5" + text[text.index(b" "):], text + b"1 2 3\n", b""):
            with pytest.raises(srm.Pre3Error) as e:
                f.load_text(bad, mode)
            assert e.value.code == E_ARG
            assert f.bad_pixels() == (1, n_bad)
            c = state(f)
            assert all(a[k].tobytes() == c[k].tobytes() for k in KEYS)
        f.load_text(text, mode)
        assert f.bad_pixels() == (2, 0)
        check_frame(f, mr.condition(fr, mode, W[mode], mr.IMAGE_MEDIAN))


# ---- 6. consumers read what was compensated -----------------------------------------------------------------------------------------------------------
def flying_floor(rows=48, cols=64, seed=11):
    """a tilted floor with flying pixels: confidence 0, range off by metres"""
    rng = np.random.default_rng(seed)
    r, c = np.mgrid[0:rows, 0:cols]
    fr = sr.make_frame(rows, cols, seed=seed)
    x = (cols / 2.0 - c) * 0.012 + rng.normal(0, 0.002, c.shape)
    y = (rows / 2.0 - r) * 0.012 + rng.normal(0, 0.002, c.shape)
    z = 2.5 + 1.3 * y + 0.1 * x + rng.normal(0, 0.003, c.shape)
    conf = 1000.0 + np.floor(rng.uniform(0, 30000, c.shape))
    fly = rng.random(c.shape) < 0.08
    z[fly] += rng.uniform(1.0, 4.0, int(fly.sum()))
    conf[fly] = 0.0
    fr.update(x=np.asfortranarray(x), y=np.asfortranarray(y), z=np.asfortranarray(z), conf=np.asfortranarray(conf))
    return fr, int(fly.sum())


def same_fit(a, b):
    assert set(a) == set(b)
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


def test_the_plane_fit_reads_the_compensated_planes():
    fr, n_fly = flying_floor()
    box = (2, 46, 2, 62)
    ref = mr.condition(fr, 0, W[0], mr.BADPIXEL, 1.0)
    with srm.SrFrame(48, 64) as f:
        f.set_compensation(srm.COMP_BADPIXEL, 1.0).load(fr, 0)
        assert f.bad_pixels() == (1, n_fly) and n_fly > 100
        got = plane.plane_fit_frame_seeded(f, 20261020, 3, n_draw=300, box=box)
        same_fit(got, plane.plane_fit_seeded(ref["x"], ref["y"], ref["z"], 20261020, 3, n_draw=300, box=box))
        f.set_compensation(srm.COMP_NONE).load(fr, 0)
        plain = plane.plane_fit_frame_seeded(f, 20261020, 3, n_draw=300, box=box)
    assert got["sta"] == 1
    assert got["n_inliers"] != plain["n_inliers"] or np.asarray(got["B"]).tobytes() != np.asarray(plain["B"]).tobytes()
    assert got["n_inliers"] > plain["n_inliers"]                             # the flying pixels smeared by the Gaussian are outliers of the floor


def test_sift_reads_the_median_filtered_image():
    rows, cols = 48, 64
    rng = np.random.default_rng(3)
    fr = sr.make_frame(rows, cols, seed=8)
    r, c = np.mgrid[0:rows, 0:cols]
    tex = 9000.0 + 7000.0 * np.sin(r / 3.1) * np.cos(c / 2.3) + 4000.0 * (((r // 6) + (c // 7)) % 2)
    fr["amp"] = np.asfortranarray(np.floor(tex + rng.uniform(0, 1500, tex.shape)))
    fr["amp"][rng.random(tex.shape) < 0.03] = 0.0                           # salt the median removes
    ref = mr.condition(fr, 1, W[1], mr.IMAGE_MEDIAN)
    with srm.SrFrame(rows, cols) as f, srm.SrFrame(rows, cols) as g:
        f.set_compensation(srm.COMP_IMAGE_MEDIAN).load(fr, 1)
        assert mr.same(f.image(), ref["img"]) and not mr.same(ref["img"], sr.condition(fr, 1, W[1])["img"])
        a = f.sift()
        b = g.sift(image=ref["img"])
    assert a["K"] == b["K"] > 0 and np.array_equal(a["counts"], b["counts"])
    assert a["frames"].tobytes() == b["frames"].tobytes() and a["descriptors"].tobytes() == b["descriptors"].tobytes()


# ---- 7. the Python mirrors ----------------------------------------------------------------------------------------------------------------------------
def test_compensate_badpixel_soonhac_mirror():
    fr, n_bad = mr.planted_frame(17, 70, seed=6)
    img = sr.normalise(fr["amp"], sr.maxima(fr["amp"], fr["conf"])[0]).astype(np.uint8)
    i2, x2, y2, z2, c2 = srm.compensate_badpixel_soonhac(img, fr["x"], fr["y"], fr["z"], fr["conf"], mr.CUTOFF)
    assert i2.dtype == np.uint8 and c2 is fr["conf"]
    for got, p in ((i2, img), (x2, fr["x"]), (y2, fr["y"]), (z2, fr["z"])):
        assert mr.same(got, mr.compensate(p, fr["conf"], mr.CUTOFF))
    assert (x2 != fr["x"]).sum() == n_bad


@pytest.fixture(scope="module")
def dat_file(tmp_path_factory):
    fr, n_bad = mr.planted_frame(144, 176, seed=9, cutoff=1.0)              # the reference's cut-off: confidence 0 is bad
    path = tmp_path_factory.mktemp("sr_median") / "d1_0007.dat"
    path.write_bytes(frame_text(fr))
    return str(path), fr, n_bad


def test_read_image_sr4000_dr_ye_mirror(dat_file):
    path, fr, _ = dat_file
    im = srm.read_image_sr4000_dr_ye(path)
    assert im.dtype == np.uint8 and mr.same(im, mr.condition(fr, 0, W[0], mr.IMAGE_MEDIAN)["img"])
    assert not np.array_equal(im, srm.read_image_sr4000(path))
    assert np.array_equal(srm.read_image_sr4000(path, compensation=(srm.COMP_IMAGE_MEDIAN, 1.0)), im)


def test_read_sr4000_data_dr_ye_with_line_44_switched_on(dat_file):
    path, fr, n_bad = dat_file
    ref = mr.condition(fr, 1, W[1], mr.BADPIXEL, 1.0)
    assert ref["n_bad"] == n_bad > 20
    x, y, z, conf, img = srm.read_sr4000_data_dr_ye(path, compensation=(srm.COMP_BADPIXEL, 1.0))
    for got, k in ((x, "x"), (y, "y"), (z, "z"), (img, "img")):
        assert mr.same(got, ref[k]), k
    assert same_bits(conf, fr["conf"])
    x0 = srm.read_sr4000_data_dr_ye(path)[0]
    assert same_bits(x0, sr.condition(fr, 1, W[1])["x"]) and not mr.same(x0, x)
    xd = srm.read_sr4000_data_dr_ye(path, parse="device", compensation=(srm.COMP_BADPIXEL, 1.0))[0]
    assert x.tobytes() == xd.tobytes()
    xz = srm.read_xyz_sr4000(path, compensation=(srm.COMP_BADPIXEL, 1.0))
    assert mr.same(xz[2], mr.condition(fr, 0, W[0], mr.BADPIXEL, 1.0)["z"])
