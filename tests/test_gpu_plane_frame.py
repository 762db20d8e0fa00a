"""GPU: the floor-plane fit and the heading update fed from a resident SR4000 frame (pre3_plane_fit_frame[_seeded], pre3_heading_from_frame[_seeded];
DESIGN.md section 23).  The oracle is always the existing entry point fed with the planes SrFrame.planes() reads back -- plane_fit[_seeded],
heading_from_scan_seeded -- and the contract is bit-identity: every integer and every double."""
import ctypes as C
import importlib

import numpy as np
import pytest

import plane_fit_ref as pr
import sr_frame_ref as sr
from test_gpu_plane_fit import _fixture_filter, _turned, _types

pytestmark = pytest.mark.gpu
plane = importlib.import_module("3pre_amd.plane")
srm = importlib.import_module("3pre_amd.sr4000")
synth = importlib.import_module("3pre_amd.synth")
_lib = importlib.import_module("3pre_amd._lib")

# the smallest box the 40-row rule admits (the whole frame); an interior box over more than one 16 x 16 filter tile; the reference's box (19 workgroups of
# the crop, the last one partial)
CASES = [((41, 3), (1, 41, 1, 3)), ((48, 20), (3, 46, 2, 19)), ((144, 176), None)]
N_DRAWS = (1, 8, 65, 1001)


def npts_of(box):
    b = box or pr.DEFAULT_BOX
    return (b[1] - b[0] + 1) * (b[3] - b[2] + 1)


def floor(rows, cols, seed, outl=0.15):
    """the tilted floor of tests/test_gpu_sr_frame.py at any size, a fraction outl of the pixels displaced in z (sta 1 and 2 both occur)"""
    rng = np.random.default_rng(seed)
    r, c = np.mgrid[0:rows, 0:cols]
    fr = sr.make_frame(rows, cols, seed=seed)
    x = (cols / 2.0 - c) * 0.012 + rng.normal(0, 0.002, c.shape)
    y = (rows / 2.0 - r) * 0.012 + rng.normal(0, 0.002, c.shape)
    z = 2.5 + 1.3 * y + 0.1 * x + rng.normal(0, 0.003, c.shape)
    z = z + (rng.random(c.shape) < outl) * rng.uniform(-0.5, 0.5, c.shape)
    fr["x"], fr["y"], fr["z"] = (np.asfortranarray(a) for a in (x, y, z))
    return fr


def same_fit(a, b):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k             # (no NaN in a result: array_equal is bit-equality up to the sign of zero)
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape,box", CASES)
def test_the_fit_is_bit_equal_to_the_fit_on_the_read_back_planes(pre3, shape, box, mode):
    stas = set()
    with srm.SrFrame(*shape) as f:
        f.load(floor(*shape, seed=5), mode)
        x, y, z, _ = f.planes()
        for n_draw in N_DRAWS:
            ref = plane.plane_fit_seeded(x, y, z, 20261018, n_draw, n_draw=n_draw, box=box)
            got = plane.plane_fit_frame_seeded(f, 20261018, n_draw, n_draw=n_draw, box=box)
            same_fit(got, ref)
            same_fit(plane.plane_fit_frame_seeded(f, 20261018, n_draw, n_draw=n_draw, box=box), got)      # a second call
            draws = pr.scene_draws(3, npts_of(box), n_draw)
            ref_t = plane.plane_fit(x, y, z, draws, box=box)
            got_t = plane.plane_fit_frame(f, draws, box=box)
            same_fit(got_t, ref_t)
            same_fit(plane.plane_fit_frame(f, draws, box=box), got_t)
            assert got["sta"] in (1, 2) and got_t["sta"] in (1, 2) and got["n_inliers"] >= 3
            stas |= {got["sta"], got_t["sta"]}
        x2, y2, z2, _ = f.planes()
        assert np.array_equal(x, x2) and np.array_equal(y, y2) and np.array_equal(z, z2)                   # the handle's planes are only read
    if shape != (41, 3):
        assert stas == {1, 2}


def test_plane_fit_to_data_mirror(pre3):
    with srm.SrFrame() as f:
        f.load(floor(144, 176, seed=9), 0)
        x, y, z, _ = f.planes()
        same_fit(srm.plane_fit_to_data(f, 7, 2, n_draw=200), plane.plane_fit_seeded(x, y, z, 7, 2, n_draw=200))


@pytest.mark.parametrize("mode", [0, 1])
def test_non_finite_points(pre3, mode):
    shape, box = (48, 20), (3, 46, 2, 19)
    clean = floor(*shape, seed=11)
    draws = pr.scene_draws(4, npts_of(box), 65)

    def with_nan(*pix):
        fr = dict(clean)
        fr["x"] = clean["x"].copy()
        for r, c in pix:
            fr["x"][r, c] = np.nan
        return fr

    def refused(f, seeded):
        with pytest.raises(pre3.Pre3Error) as e:
            plane.plane_fit_frame_seeded(f, 1, 2, n_draw=65, box=box) if seeded else plane.plane_fit_frame(f, draws, box=box)
        assert e.value.code == -5 and "not finite" in str(e.value)
        r = e.value.result
        assert r["sta"] == 5 and r["best"] == -1 and r["n_trials"] == 0 and r["n_inliers"] == 0
        assert not r["B"].any() and not r["R"].any()

    with srm.SrFrame(*shape) as f:
        # a raw NaN two pixels above the box (0-based row 0; the box starts at row 2): its filtered patch ends one pixel above the box
        f.load(with_nan((0, 5)), mode)
        x, y, z, _ = f.planes()
        assert np.isnan(x[1, 5]) and not np.isnan(x[2:46, 1:19]).any()
        same_fit(plane.plane_fit_frame_seeded(f, 1, 2, n_draw=65, box=box), plane.plane_fit_seeded(x, y, z, 1, 2, n_draw=65, box=box))
        same_fit(plane.plane_fit_frame(f, draws, box=box), plane.plane_fit(x, y, z, draws, box=box))
        # one pixel above: the filter carries it into the box's first row
        f.load(with_nan((1, 5)), mode)
        x = f.planes()[0]
        assert np.isnan(x[2, 5]) and not np.isnan(x[3:46, 1:19]).any()
        refused(f, True); refused(f, False)
        # the box's first and last point
        f.load(with_nan((2, 1), (45, 18)), mode)
        refused(f, True); refused(f, False)
        # a clean frame afterwards: the flag word is cleared per call
        f.load(clean, mode)
        x, y, z, _ = f.planes()
        same_fit(plane.plane_fit_frame_seeded(f, 1, 2, n_draw=65, box=box), plane.plane_fit_seeded(x, y, z, 1, 2, n_draw=65, box=box))
        same_fit(plane.plane_fit_frame(f, draws, box=box), plane.plane_fit(x, y, z, draws, box=box))


def test_argument_and_state_errors_leave_the_handle_unchanged(pre3):
    with srm.SrFrame() as f:
        with pytest.raises(pre3.Pre3Error) as e:                                   # nothing loaded yet
            plane.plane_fit_frame_seeded(f, 1)
        assert e.value.code == -4
        f.load(floor(144, 176, seed=2), 0)
        before = f.planes()[:3]
        ref = plane.plane_fit_frame_seeded(f, 5, 1, n_draw=65)
        good = pr.scene_draws(0, 65 * 71, 8)
        bad_draw = good.copy(); bad_draw[3, 1] = 65 * 71
        for kw in (dict(box=(80, 145, 50, 120)), dict(box=(0, 60, 50, 120)), dict(box=(80, 144, 50, 177)), dict(box=(100, 138, 50, 120)),      # 39 rows
                   dict(n_draw=0), dict(n_draw=1002), dict(t=0.0), dict(t=-1.0), dict(t=float("nan"))):
            with pytest.raises(pre3.Pre3Error) as e:
                plane.plane_fit_frame_seeded(f, 5, 1, **{"n_draw": 65, **kw})
            assert e.value.code == -1, kw
        for kw in (dict(draws=bad_draw), dict(draws=-good), dict(draws=good, box=(80, 145, 50, 120)), dict(draws=good, t=0.0), dict(draws=np.zeros((0, 3), np.int32))):
            with pytest.raises(pre3.Pre3Error) as e:
                plane.plane_fit_frame(f, **kw)
            assert e.value.code == -1, kw
        res = plane.PlaneResult()
        assert _lib.lib.pre3_plane_fit_frame(f._h, None, 0.02, 8, None, None, None, C.byref(res)) == -1      # a null table
        assert _lib.lib.pre3_plane_fit_frame(f._h, None, 0.02, 8, _lib.dptr(good), None, None, None) == -1   # a null result
        small = pr.scene_draws(0, 40 * 71, 8)
        same_fit(plane.plane_fit_frame(f, small, box=(100, 139, 50, 120)), plane.plane_fit(*before, small, box=(100, 139, 50, 120)))      # 40 rows pass
        after = f.planes()[:3]
        assert all(np.array_equal(a, b) for a, b in zip(before, after))
        same_fit(plane.plane_fit_frame_seeded(f, 5, 1, n_draw=65), ref)


# ---- the heading update ---------------------------------------------------------------------------------------------------------------------------
def _synth8(pre3):
    x0, P0, _ = synth.make_map(8, None)
    f = pre3.EkfFilter(synth.CAM, _types(8), dtype="f32", max_hyp=8)
    f.set_x_p_k_k(x0, P0)
    x0, P0 = f._get(0)
    return f, x0, P0


def _scene_frame(seed, outl=0.1):
    x, y, z, _ = pr.scene(seed, outl)
    fr = sr.make_frame(144, 176, seed=seed)
    fr["x"], fr["y"], fr["z"] = (np.asfortranarray(a) for a in (x, y, z))
    return fr


def _aimed(filt, x0, P0, R, deg=1.5):
    """the filter's quaternion deg degrees from R2q(R'): the gate lets the update through"""
    x = x0.copy()
    x[3:7] = _turned(R.T, deg)
    filt.set_x_p_k_k(x, P0)
    return filt._get(0)


@pytest.mark.parametrize("ctx", ["fixture_f64", "synth_f32"])
def test_heading_from_frame(pre3, sr4000, ctx):
    filt, x0, P0 = _fixture_filter(pre3, sr4000) if ctx == "fixture_f64" else _synth8(pre3)
    if ctx == "fixture_f64":
        filt.set_x_p_k_k(x0, P0)
    with srm.SrFrame() as f:
        f.load(_scene_frame(1), 0)
        x, y, z, _ = f.planes()
        fit = plane.plane_fit_seeded(x, y, z, 77, 4)
        assert fit["sta"] == 1
        xs, Ps = _aimed(filt, x0, P0, fit["R"])
        for strict in (True, False):
            filt.set_x_p_k_k(xs, Ps)
            a_ref, r_ref = filt.heading_from_scan_seeded(x, y, z, 77, 4, strict_reference=strict, return_draws=True)
            x_ref, P_ref = filt._get(0)
            assert a_ref and np.abs(x_ref[3:7] - xs[3:7]).max() > 0                # the oracle's update was applied
            filt.set_x_p_k_k(xs, Ps)
            a, r = filt.heading_from_frame_seeded(f, 77, 4, strict_reference=strict, return_draws=True)
            xg, Pg = filt._get(0)
            assert a == a_ref and filt.rows_form() == 1
            same_fit(r, r_ref)
            assert xg.tobytes() == x_ref.tobytes() and Pg.tobytes() == P_ref.tobytes()
        # a supplied table, transpose off, and a gate that returns (10 degrees off)
        draws = pr.scene_draws(1, 65 * 71, 200)
        for deg, tr in ((1.5, True), (1.5, False), (10.0, True)):
            xs2, Ps2 = _aimed(filt, x0, P0, fit["R"] if tr else fit["R"].T, deg)
            a_ref, r_ref = filt.heading_from_scan(x, y, z, draws, transpose=tr)
            x_ref, P_ref = filt._get(0)
            filt.set_x_p_k_k(xs2, Ps2)
            a, r = filt.heading_from_frame(f, draws, transpose=tr)
            xg, Pg = filt._get(0)
            assert a == a_ref == (deg < 4.0)
            same_fit(r, r_ref)
            assert xg.tobytes() == x_ref.tobytes() and Pg.tobytes() == P_ref.tobytes()
        # a flagged box: PRE3_E_NUMERIC, x and P bit-unchanged, and the next update works
        bad = _scene_frame(1)
        bad["z"] = bad["z"].copy(); bad["z"][100, 80] = np.nan
        f.load(bad, 0)
        filt.set_x_p_k_k(xs, Ps)
        xa, Pa = filt._get(0)
        with pytest.raises(pre3.Pre3Error) as e:
            filt.heading_from_frame_seeded(f, 77, 4)
        assert e.value.code == -5 and e.value.result["sta"] == 5
        xb, Pb = filt._get(0)
        assert xa.tobytes() == xb.tobytes() and Pa.tobytes() == Pb.tobytes()
        assert filt.heading_from_frame_seeded(f, 77, 4, wait=False) is None       # the no-wait form skips on the device
        xb, Pb = filt._get(0)
        assert xa.tobytes() == xb.tobytes() and Pa.tobytes() == Pb.tobytes()
        f.load(_scene_frame(1), 0)
        filt.set_x_p_k_k(xs, Ps)
        a_ref, r_ref = filt.heading_from_scan_seeded(x, y, z, 77, 4)
        x_ref, P_ref = filt._get(0)
        filt.set_x_p_k_k(xs, Ps)
        a, r = filt.heading_from_frame_seeded(f, 77, 4)
        xg, Pg = filt._get(0)
        assert a and a_ref
        same_fit(r, r_ref)
        assert xg.tobytes() == x_ref.tobytes() and Pg.tobytes() == P_ref.tobytes()
    filt.close()


def test_a_load_straight_after_the_no_wait_form_stays_behind_the_crop(pre3):
    """load(A), heading_from_frame_seeded(wait=False), load(B) at once, then x and P: the fit of A (the handle's stream waits for the release event)"""
    filt, x0, P0 = _synth8(pre3)
    A, B = _scene_frame(1), _scene_frame(2, 0.5)
    B["z"] = np.asfortranarray(B["z"] + 0.4 * B["x"])                               # another plane altogether
    with srm.SrFrame() as f:
        f.load(A, 0)
        x, y, z, _ = f.planes()
        fit = plane.plane_fit_seeded(x, y, z, 3, 9)
        assert fit["sta"] == 1
        xs, Ps = _aimed(filt, x0, P0, fit["R"])
        a_ref, _ = filt.heading_from_scan_seeded(x, y, z, 3, 9)
        x_ref, P_ref = filt._get(0)
        assert a_ref and np.abs(x_ref[3:7] - xs[3:7]).max() > 0
        for _ in range(3):
            f.load(A, 0)
            filt.set_x_p_k_k(xs, Ps)
            assert filt.heading_from_frame_seeded(f, 3, 9, wait=False) is None
            f.load(B, 0)
            xg, Pg = filt._get(0)
            assert xg.tobytes() == x_ref.tobytes() and Pg.tobytes() == P_ref.tobytes()
        xb = f.planes()[0]
        f.load(B, 0)
        assert np.array_equal(xb, f.planes()[0])                                    # and B arrived whole
    filt.close()


def _synth4(pre3):
    x0, P0, _ = synth.make_map(4, None)
    f = pre3.EkfFilter(synth.CAM, _types(4), dtype="f32", max_hyp=8)
    f.set_x_p_k_k(x0, P0)
    return f, *f._get(0)


@pytest.mark.parametrize("feed", ["host", "frame"])
def test_a_larger_box_straight_after_the_no_wait_form_replaces_the_work_block_in_stream_order(pre3, feed):
    """The context's work block is grown, and zeroed, on the context's stream.  On a 64 x 48 image: the no-wait form with the smallest box (rows 1..41,
    columns 1..3: 123 points, 8 draws), at once the waiting form with the whole image, which replaces the block while the first call may still be
    queued.  State, covariance, applied and the result block are bit-equal to a fresh context given the same two calls with a sync() between them.
    The scene is fitted with sta = 1 in both boxes from either feed (tests/plane_fit_ref.py on the raw and on the conditioned planes)."""
    small, full = (1, 41, 1, 3), (1, 64, 1, 48)
    x, y, z, _ = pr.scene(1, 0.0)
    fr = sr.make_frame(64, 48, seed=1)
    fr["x"], fr["y"], fr["z"] = (np.asfortranarray(a[70:134, 64:112]) for a in (x, y, z))
    d_small, d_full = pr.scene_draws(2, npts_of(small), 8), pr.scene_draws(3, npts_of(full), 8)
    with srm.SrFrame(64, 48) as f:
        f.load(fr, 1)
        if feed == "host":
            def fit(box, draws):
                return plane.plane_fit(fr["x"], fr["y"], fr["z"], draws, box=box)

            def heading(filt, box, draws, wait):
                return filt.heading_from_scan(fr["x"], fr["y"], fr["z"], draws, box=box, wait=wait)
        else:
            def fit(box, draws):
                return plane.plane_fit_frame(f, draws, box=box)

            def heading(filt, box, draws, wait):
                return filt.heading_from_frame(f, draws, box=box, wait=wait)
        first, second = fit(small, d_small), fit(full, d_full)
        assert first["sta"] == 1 and second["sta"] == 1
        got = []
        for between in (False, True):
            filt, x0, P0 = _synth4(pre3)                                            # a fresh context: no work block yet
            _aimed(filt, x0, P0, second["R"])
            assert heading(filt, small, d_small, False) is None
            if between:
                filt.sync()
            a, r = heading(filt, full, d_full, True)
            got.append((a, r, *filt._get(0)))
            filt.close()
    (a, r, xg, Pg), (a_ref, r_ref, x_ref, P_ref) = got
    assert a and a_ref and r["sta"] == 1
    same_fit(r, r_ref)
    same_fit(r, {k: second[k] for k in r})
    assert xg.tobytes() == x_ref.tobytes() and Pg.tobytes() == P_ref.tobytes()


def test_errors_of_the_context_form(pre3):
    filt, x0, P0 = _synth8(pre3)
    good = pr.scene_draws(0, 65 * 71, 8)
    bad_draw = good.copy(); bad_draw[0, 0] = 65 * 71
    with srm.SrFrame() as f:
        with pytest.raises(pre3.Pre3Error) as e:                                   # nothing loaded yet
            filt.heading_from_frame_seeded(f, 1)
        assert e.value.code == -4
        f.load(_scene_frame(0), 0)
        before = f.planes()[:3]
        for kw in (dict(box=(80, 145, 50, 120)), dict(box=(100, 138, 50, 120)), dict(n_draw=0), dict(n_draw=1002), dict(t=0.0), dict(t=-2.0)):
            with pytest.raises(pre3.Pre3Error) as e:
                filt.heading_from_frame_seeded(f, 1, 0, **{"n_draw": 65, **kw})
            assert e.value.code == -1, kw
        with pytest.raises(pre3.Pre3Error) as e:
            filt.heading_from_frame(f, bad_draw)
        assert e.value.code == -1
        assert _lib.lib.pre3_heading_from_frame(filt._ctx, None, None, 0.02, 8, _lib.dptr(good), 1, 1, None, None) == -1      # a null handle
        assert _lib.lib.pre3_heading_from_frame(None, f._h, None, 0.02, 8, _lib.dptr(good), 1, 1, None, None) == -1          # a null context
        x1, P1 = filt._get(0)
        assert x1.tobytes() == x0.tobytes() and P1.tobytes() == P0.tobytes()
        assert all(np.array_equal(a, b) for a, b in zip(before, f.planes()[:3]))
        filt.set_x_p_k_km1(x0, P0)                                                  # the prediction in the covariance buffer
        with pytest.raises(pre3.Pre3Error) as e:
            filt.heading_from_frame(f, good)
        assert e.value.code == -4
    filt.close()


def test_a_handle_on_another_device_is_refused(pre3):
    if pre3.device_count() < 2:
        pytest.skip("one device: the device mismatch needs two")
    filt, x0, P0 = _synth8(pre3)
    with srm.SrFrame(device=1) as f1:
        f1.load(_scene_frame(0), 0)
        with pytest.raises(pre3.Pre3Error) as e:
            filt.heading_from_frame(f1, pr.scene_draws(0, 65 * 71, 8))
        assert e.value.code == -1 and "device" in str(e.value)
        with pytest.raises(pre3.Pre3Error) as e:
            filt.set_scan_frame(f1)
        assert e.value.code == -1 and "device" in str(e.value)
    x1, P1 = filt._get(0)
    assert x1.tobytes() == x0.tobytes() and P1.tobytes() == P0.tobytes()
    filt.close()
