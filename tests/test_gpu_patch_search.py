"""GPU: the patch branch of the IC search (pre3_patch_search, pre3_predict_patches, the patch bank) against the numpy restatement
tests/patch_match_ref.py, fed with the h, has_h and S read back through pre3_get_landmark_fields and the x_k_km1 read back from the same context.

Tolerances (derived, not measured).  Patches: 1e-8 grey levels -- the sample coordinates come from about 60 operations on magnitudes <= 200 px
(<= 1.5e-12 px), the bilinear slope is <= 255 per pixel on two axes, a factor 10 in hand.  corr: 1e-7 -- that bound over a template standard deviation
of >= 5 grey levels (asserted), the same factor in hand.  Everything else is equal exactly; the restatement's margins (ellipse, best - second best)
must be >= 1e-6 for every landmark, so none is left out of the comparison.  The ellipse margin is taken over the pixels of the box that pass
matching.m:81-82's band test: a pixel outside the band is no candidate whatever the ellipse says, and the box of a window that is the whole image
reaches far outside it.

S >= R = I, so a landmark that is searched always has K >= 2 (the ellipse's radius is at least 2.4 px): K = 0 and K = 1 occur on the device only for
landmarks in the border band (zero patch), whose candidates are still counted; the modes' K <= 1 rules are covered on the CPU.  On 60 x 80 no window
can exceed the LDS staging limit (16 KiB > 80 x 60 bytes); 144 x 176 has a window on each side of it."""
import importlib

import numpy as np
import pytest

import patch_cases as pc
import patch_match_ref as ref

pytestmark = pytest.mark.gpu
_lib = importlib.import_module("3pre_amd._lib")
Pre3Error = _lib.Pre3Error
THR = 0.60
_CACHE = {}


def _filter(pre3, sc, dtype, extra=6, patches=True, image="imB", km1=True):
    N = len(sc["types"])
    f = pre3.EkfFilter(pc.cam_list(sc["cam"]), sc["types"], dtype=dtype, max_hyp=16, max_landmarks=N + extra)
    (f.set_x_p_k_km1 if km1 else f.set_x_p_k_k)(sc["x"], sc["P"])
    if image:
        f.set_image(sc[image])
    if patches and N:
        b, has = sc["bank"], sc["bank"]["has_patch"]
        runs, i = [], 0
        while i < N:                                            # (landmarks without a patch are left out: set in runs)
            if has[i]:
                j = i
                while j < N and has[j]:
                    j += 1
                runs.append((i, j))
                i = j
            else:
                i += 1
        for a, e in runs:
            f.set_patches(b["patch"][a:e], b["uv_init"][a:e], b["r_wc"][a:e], b["R_wc"][a:e], first=a)
    return f


def _scene(orc, name):
    if name not in _CACHE:
        shape = (144, 176) if "176" in name else (60, 80)
        if name.startswith("win"):
            _CACHE[name] = pc.build_scene(orc, shape[0], shape[1], pc.spec_windows(*shape), seed=11)
        else:
            n = int(name.split("_")[0][1:])
            _CACHE[name] = pc.build_scene(orc, shape[0], shape[1], pc.spec_random(np.random.default_rng(3 + n), shape[0], shape[1], n, cart_every=3), seed=12 + n)
    return _CACHE[name]


SCENES = ["win_176", "win_80", "n70_176", "n3_80", "n1_176"]


def _device_reference(f, sc, strict, key):
    """the restatement on what the device holds; computed once per (scene, dtype, mode)"""
    if key not in _CACHE:
        lf = f.landmark_fields()
        _CACHE[key] = (pc.reference(sc, sc["imB"], THR, strict, h=lf["h"], has_h=lf["has_h"], S=lf["S"], x=f.get_x_k_km1()), lf)
    return _CACHE[key]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", SCENES)
def test_patches_and_search(pre3, orc, name, dtype):
    sc = _scene(orc, name)
    N = len(sc["types"])
    f = _filter(pre3, sc, dtype)
    got = {s: f.search_ic_matches_patch(pc.FD_FORK, THR, strict_reference=bool(s)) for s in (0, 1)}
    patches, pst = f.predict_features_appearance(pc.FD_FORK)
    for strict in (0, 1):
        r, lf = _device_reference(f, sc, strict, (name, dtype, strict))
        print(name, dtype, "strict", strict, "margins", r["margin_ellipse"].min(), r["margin_gap"].min(), "ncand", r["ncand"].tolist()[:20])
        assert r["margin_ellipse"].min() >= 1e-6 and r["margin_gap"].min() >= 1e-6
        for co in r["coords"]:
            if co is not None:
                for a in co:
                    assert min(np.abs(a - 1).min(), np.abs(a - 41).min()) >= 1e-6
        w = r["pstatus"] == ref.WARPED
        if w.any():
            assert r["patches"][w].reshape(w.sum(), -1).std(axis=1)[[not s.get("flat_patch") for s, k in zip(sc["spec"], w) if k]].min() >= 5.0
        # 1. the warped patches
        if strict == 0:
            assert np.array_equal(pst, r["pstatus"])
            assert np.array_equal(np.isnan(patches), np.isnan(r["patches"]))
            d = np.abs(np.nan_to_num(patches) - np.nan_to_num(r["patches"])).max() if N else 0.0
            print(name, dtype, "max patch difference", d)
            assert d <= 1e-8
        # 2. the search
        meas, z, corr, ncand, st = got[strict]
        assert np.array_equal(st, r["status"]) and np.array_equal(ncand, r["ncand"])
        assert np.array_equal(meas, r["meas_idx"]) and f.m == len(r["meas_idx"])
        assert np.array_equal(z, r["z"][r["meas_idx"]])
        assert np.array_equal(np.isnan(corr), np.isnan(r["corr"]))
        ok = ~np.isnan(corr)
        dc = np.abs(corr[ok] - r["corr"][ok]).max() if ok.any() else 0.0
        print(name, dtype, "strict", strict, "max corr difference", dc)
        assert dc <= 1e-7
    if name == "win_176":
        r = _CACHE[(name, dtype, 1)][0]
        K = r["ncand"]
        assert ((K >= 2) & (K <= 98)).any() and ((K >= 99) & (K <= 199)).any() and (K >= 200).any() and (K > 256).any() and (K == 0).any() and (K == 1).any()
        for st_ in (ref.NOT_PREDICTED, ref.NO_PATCH, ref.ZERO_PATCH, ref.WARP_OUTSIDE, ref.BELOW, ref.MATCHED):
            assert (r["status"] == st_).any()
    f.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_empty_map(pre3, orc, dtype):
    sc = pc.build_scene(orc, 144, 176, [], seed=1)
    f = _filter(pre3, sc, dtype)
    meas, z, corr, ncand, st = f.search_ic_matches_patch(pc.FD_FORK, THR)
    assert len(meas) == 0 and f.m == 0 and len(st) == 0
    f.close()


def test_planted_shift_end_to_end(pre3, orc):
    """set_image, patch_cut, a prediction that leaves the pose where it was, set_image of the shifted image, the search in mode 0"""
    rng = np.random.default_rng(9)
    sp = [dict(uv=(float(rng.integers(30, 146)), float(rng.integers(30, 114))), S=pc.S_of(rng.uniform(2, 4)), depth=rng.uniform(4, 12), cartesian=(i % 3 == 2))
          for i in range(24)]
    sc = pc.build_scene(orc, 144, 176, sp, seed=31, moved=False)
    sx, sy = 3, -2
    imB = pc.shift_image(sc["imA"], sx, sy, np.random.default_rng(2))
    uv = np.array([s["uv"] for s in sp], np.int32)
    for dtype in ("f64", "f32"):
        f = _filter(pre3, sc, dtype, patches=False, image="imA", km1=False)
        f.patch_cut(uv)
        bank = f.patches()
        assert bank["has_patch"].all() and np.array_equal(bank["uv_init"], uv) and np.array_equal(bank["patch"], np.stack([pc.cut_patch(sc["imA"], u) for u in uv]))
        assert np.array_equal(bank["r_wc"], np.tile(sc["x"][0:3], (len(sp), 1))) and np.abs(bank["R_wc"] - ref.q2r(sc["x"][3:7])).max() == 0
        f.ekf_prediction(np.array([0, 0, 0, 1.0, 0, 0, 0]))
        f.set_image(imB)
        meas, z, corr, ncand, st = f.search_ic_matches_patch(pc.FD_FORK, THR, strict_reference=False)
        lf = f.landmark_fields()
        inside = []
        for i in range(len(sp)):
            cands, _ = ref.candidates(lf["h"][i], lf["S"][i], 144, 176)
            if (int(uv[i][0]) + sx, int(uv[i][1]) + sy) in cands:
                inside.append(i)
        assert len(inside) >= 10
        for i in inside:
            assert st[i] == ref.MATCHED and i in meas
            assert np.array_equal(z[list(meas).index(i)], uv[i] + [sx, sy])
        f.close()


def test_bank_follows_the_map(pre3, orc):
    sc = _scene(orc, "n70_176")
    N = len(sc["types"])
    b = sc["bank"]
    f = _filter(pre3, sc, "f64", km1=False)
    g = _filter(pre3, sc, "f64", patches=False, image=None, km1=False)          # never sets a patch or an image
    dele = [2, 5, 9]
    uvd = np.array([[60.0, 50.0], [100.0, 80.0]])
    for q in (f, g):
        q.delete_features(dele)
        q.add_features_inverse_depth(uvd, 1.0, 0.5)
    keep = [i for i in range(N) if i not in dele]
    got = f.patches()
    assert got["has_patch"].tolist() == [True] * len(keep) + [False, False]
    assert np.array_equal(got["patch"][:len(keep)], b["patch"][keep]) and np.array_equal(got["uv_init"][:len(keep)], b["uv_init"][keep])
    assert np.array_equal(got["r_wc"][:len(keep)], b["r_wc"][keep]) and np.array_equal(got["R_wc"][:len(keep)], b["R_wc"][keep])
    assert not got["patch"][len(keep):].any()
    assert np.array_equal(f.get_x_k_k(), g.get_x_k_k()) and np.array_equal(f.get_p_k_k(), g.get_p_k_k())
    with pytest.raises(Pre3Error) as e:
        g.patches()
    assert e.value.code == -4
    f.ekf_prediction(np.array([0, 0, 0, 1.0, 0, 0, 0]))
    st = f.search_ic_matches_patch(pc.FD_FORK, THR)[4]
    assert (st[len(keep):] == ref.NO_PATCH).all() and (st[:len(keep)] >= ref.ZERO_PATCH).all()
    f.close()
    g.close()
    # ... until patch_cut
    f = _filter(pre3, sc, "f64", km1=False)
    f.add_features_inverse_depth(uvd, 1.0, 0.5)
    f.patch_cut(uvd.astype(np.int32), first=N)
    assert f.patches()["has_patch"].all()
    f.close()


def test_set_image_frame(pre3, orc):
    srm = importlib.import_module("3pre_amd.sr4000")
    rng = np.random.default_rng(4)
    sc = _scene(orc, "n1_176")
    planes = dict(z=rng.uniform(0.5, 5, (144, 176)), x=rng.uniform(-2, 2, (144, 176)), y=rng.uniform(-2, 2, (144, 176)),
                  amp=rng.uniform(0, 30000, (144, 176)), conf=rng.uniform(0, 1, (144, 176)))
    f = _filter(pre3, sc, "f64", image=None)
    g = _filter(pre3, sc, "f64", image=None)
    with srm.SrFrame(144, 176) as fh:
        fh.load(planes)
        f.set_image_frame(fh)
        a = f.get_image((144, 176))
        img = fh.image()
        fh.feed_image(g)
        assert np.array_equal(g.get_image((144, 176)), a)
    assert img.dtype == np.uint8 and img.std() > 1
    g.set_image(img)
    assert np.array_equal(a, img) and np.array_equal(g.get_image((144, 176)), a)
    f.close()
    g.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_into_the_step(pre3, orc, dtype):
    sc = _scene(orc, "n70_176")
    f = _filter(pre3, sc, dtype, km1=False)
    g = _filter(pre3, sc, dtype, patches=False, image=None, km1=False)
    for q in (f, g):
        q.ekf_prediction_cv(0.1, 0.007, 0.007)
    meas, z, corr, ncand, st = f.search_ic_matches_patch(pc.FD_FORK, THR)
    assert len(meas) >= 10
    g.search_IC_matches()
    g.set_measurements(meas, z)
    sf = f.step_predicted_seeded(77, 1, 16)
    sg = g.step_predicted_seeded(77, 1, 16)
    assert np.array_equal(f.get_x_k_k(), g.get_x_k_k()) and np.array_equal(f.get_p_k_k(), g.get_p_k_k())
    assert sf["n_li"] == sg["n_li"] and sf["n_li"] > 0
    f.close()
    g.close()


def _raises(code, fn, *a, **k):
    with pytest.raises(Pre3Error) as e:
        fn(*a, **k)
    assert e.value.code == code, e.value


def test_refusals(pre3, orc):
    import ctypes as C
    sc = _scene(orc, "n3_80")
    lib = _lib.lib
    # no image
    f = _filter(pre3, sc, "f64", image=None)
    _raises(-4, f.search_ic_matches_patch, pc.FD_FORK)
    # wrong shape
    _raises(-1, f.set_image, np.zeros((80, 60), np.uint8))
    _raises(-1, f.set_image, np.zeros((144, 176), np.uint8))
    f.set_image(sc["imB"])
    # a NULL m_out
    assert lib.pre3_patch_search(f._ctx, pc.FD_FORK, THR, 1, None, None, None, None, None, None) == -1
    # first + count > N
    b = sc["bank"]
    _raises(-1, f.set_patches, b["patch"], b["uv_init"], b["r_wc"], b["R_wc"], first=1)
    _raises(-1, f.patch_cut, np.array([[30, 30]], np.int32), first=3)
    # usable afterwards
    meas, z, corr, ncand, st = f.search_ic_matches_patch(pc.FD_FORK, THR)
    assert len(st) == 3
    f.close()
    # no prediction: the covariance buffer holds (x_k_k, p_k_k)
    f = _filter(pre3, sc, "f64", km1=False)
    _raises(-4, f.search_ic_matches_patch, pc.FD_FORK)
    # uv too near the border in patch_cut (nothing queued: the bank is as it was)
    before = f.patches()
    for uv in ([20, 30], [30, 20], [61, 30], [30, 41]):
        _raises(-1, f.patch_cut, np.array([uv], np.int32))
    f.patch_cut(np.array([[21, 21], [60, 40]], np.int32), first=1)
    after = f.patches()
    assert np.array_equal(before["patch"][0], after["patch"][0]) and np.array_equal(after["uv_init"][1:], [[21, 21], [60, 40]])
    f.ekf_prediction(np.array([0, 0, 0, 1.0, 0, 0, 0]))
    assert len(f.search_ic_matches_patch(pc.FD_FORK, THR)[4]) == 3
    f.close()
