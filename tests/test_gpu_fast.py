"""GPU: FAST-9 corners on the resident image and the patch-feature initialisation from them (pre3_fast_detect, pre3_init_feature_fast[_seeded],
pre3_init_features_fast_all) against the numpy restatement tests/fast_ref.py and the fixture tests/golden/fast_lab_crop.npz (what
the reference's decision tree computes on a crop where it and the segment test agree).

Every comparison is exact equality of integers, lists in order.  rho and xyz equal pre3_sr_frame_keypoints' gate-0 outputs on the same pixel bit for
bit; x, P, the map and the patch bank equal, bit for bit, a twin context fed the same list through add_features_inverse_depth and patch_cut."""
import importlib
import os

import numpy as np
import pytest

import fast_ref as fr
import patch_cases as pc

pytestmark = pytest.mark.gpu
_lib = importlib.import_module("3pre_amd._lib")
Pre3Error = _lib.Pre3Error
HERE = os.path.dirname(os.path.abspath(__file__))
_CACHE = {}


def fixture():
    if "fx" not in _CACHE:
        _CACHE["fx"] = dict(np.load(os.path.join(HERE, "golden", "fast_lab_crop.npz")))
    return _CACHE["fx"]


def image(name):
    """crop: the fixture's; blur_RxC: seeded blurred noise; noise_RxC: seeded white noise; seven: a flat image with one planted corner"""
    if name not in _CACHE:
        if name == "crop":
            im = fixture()["image"]
        elif name == "seven":
            im = np.full((144, 176), 100, np.uint8)
            for dx, dy in fr.RING:
                im[50 + dy, 60 + dx] = 200
        else:
            kind, shape = name.split("_")
            R, Cn = (int(v) for v in shape.split("x"))
            rng = np.random.default_rng(R * 1000 + Cn)
            # (blurred noise at a sixth of the contrast: at full contrast nearly every pixel of it is a corner)
            im = (pc.smooth_image(rng, R, Cn) // 6 + 60).astype(np.uint8) if kind == "blur" else rng.integers(0, 256, (R, Cn)).astype(np.uint8)
        _CACHE[name] = np.ascontiguousarray(im)
    return _CACHE[name]


def bare_filter(pre3, shape, dtype="f64", cap=4):
    """a context with the camera of that shape, no landmarks, (x_k_k, p_k_k) set"""
    f = pre3.EkfFilter(pc.cam_list(pc.make_cam(*shape)), np.zeros(0, np.int32), dtype=dtype, max_hyp=16, max_landmarks=cap)
    x = np.zeros(13)
    x[3] = 1.0
    f.set_x_p_k_k(x, np.eye(13) * 1e-4)
    return f


def adjacent_pairs(c):
    s = {tuple(p) for p in c.tolist()}
    return sum(1 for (x, y) in s for dx, dy in ((1, -1), (1, 0), (1, 1), (0, 1)) if (x + dx, y + dy) in s)


def check_detector(f, im, box, threshold, barrier):
    """both lists on one rectangle; returns the maxima and their scores.  A list longer than the capacity is PRE3_E_NOMEM, whatever else is asked"""
    r0, c0, rows, cols = box
    ruv, rsc = fr.detect(im, threshold, barrier, 0, r0, c0, rows, cols)
    if len(ruv) > _lib.FAST_MAX_CORNERS:
        _raises(-6, f.fast_corner_detect_9, threshold, box=box)
    else:
        uv, sc = f.fast_corner_detect_9(threshold, box=box, barrier=barrier)
        assert uv.dtype == np.int32 and np.array_equal(uv, ruv) and np.array_equal(sc, rsc), (box, threshold, barrier, len(uv), len(ruv))
        assert np.array_equal(f.fast_corner_detect_9(threshold, box=box), ruv)
    mx, ms = f.fast_nonmax(threshold, barrier, box=box)
    rmx, rms = fr.detect(im, threshold, barrier, 1, r0, c0, rows, cols)
    assert np.array_equal(mx, rmx) and np.array_equal(ms, rms), (box, threshold, barrier, len(mx), len(rmx))
    return mx, ms


PAIRS = [(10, 20), (5, 20), (20, 20)]
# whole image; a 61 x 41 box; column counts one more / one less than a multiple of the strip width (8) from an origin that is no strip boundary of the
# image, odd row counts; one strip; rows and columns at the minimum
BOXES_144 = [(0, 0, 144, 176), (20, 30, 61, 41), (5, 5, 37, 33), (7, 3, 39, 31), (1, 13, 29, 8), (90, 100, 7, 40), (3, 2, 50, 7), (0, 0, 144, 9), (83, 135, 61, 41)]


@pytest.mark.parametrize("name", ["crop", "blur_144x176", "noise_144x176"])
def test_detector_equals_the_restatement(pre3, name):
    im = image(name)
    f = bare_filter(pre3, im.shape)
    f.set_image(im)
    zero_max = pairs = 0
    for box in BOXES_144:
        for t, b in PAIRS + ([(30, 20)] if name.startswith("noise") else []):
            mx, ms = check_detector(f, im, box, t, b)
            zero_max += int((ms == 0).sum())
            pairs += adjacent_pairs(mx)
    if name == "noise_144x176":
        n30 = len(fr.fast_corner_detect_9(im, 30))
        print(name, "corners at threshold 30:", n30)
        assert n30 >= 1000                                   # thousands of corners, many ties
    print(name, "score-0 maxima", zero_max, "adjacent pairs of maxima", pairs)
    assert pairs >= 1 and (zero_max >= 1 or name.startswith("noise"))      # both quirks of fast_nonmax.m:87-92 are in the inputs (white noise scores high)
    f.close()


def test_detector_240x320(pre3):
    im = image("blur_240x320")
    f = bare_filter(pre3, im.shape)
    f.set_image(im)
    for box in [(0, 0, 240, 320), (20, 20, 200, 280), (11, 9, 201, 65), (100, 250, 61, 41)]:
        for t, b in PAIRS:
            check_detector(f, im, box, t, b)
    n5, n10 = len(fr.fast_corner_detect_9(im, 5)), len(fr.fast_corner_detect_9(im, 10))
    assert n5 > _lib.FAST_MAX_CORNERS >= n10 > 1000          # the whole image at 5 is over the capacity (checked as a status above), at 10 under it
    f.close()


def test_one_candidate_pixel(pre3):
    im = image("seven")
    f = bare_filter(pre3, im.shape)
    f.set_image(im)
    for nonmax in (0, 1):
        uv, sc = f._fast_detect(10, 20, nonmax, (47, 57, 7, 7))              # the planted corner is the rectangle's one candidate
        assert uv.tolist() == [[4, 4]] and sc.tolist() == [16 * 80]
        uv, sc = f._fast_detect(10, 20, nonmax, (80, 80, 7, 7))              # flat
        assert uv.shape == (0, 2) and sc.shape == (0,)
        # one pixel off: the ring leaves the rectangle's candidate; the rectangle is an image of its own, so nothing outside it is read
        uv, _ = f._fast_detect(10, 20, nonmax, (48, 57, 7, 7))
        assert np.array_equal(uv, fr.detect(im, 10, 20, nonmax, 48, 57, 7, 7)[0])
    check_detector(f, im, (47, 57, 7, 7), 10, 20)
    f.close()


def test_the_pin_to_the_reference(pre3):
    """the device's corners on the crop are the reference tree's (tests/golden/make_fast_fixtures.py), at 10, 20 and 30, and fast_nonmax's maxima"""
    fx = fixture()
    f = bare_filter(pre3, (144, 176))
    f.set_image(fx["image"])
    for t in (10, 20, 30):
        assert np.array_equal(f.fast_corner_detect_9(t), fx["corners_%d" % t])
    mx, ms = f.fast_nonmax(10, 20)
    assert np.array_equal(mx, fx["maxima_10_20"]) and np.array_equal(ms, fx["maxima_scores_10_20"])
    assert len(mx) == 96 and int((ms == 0).sum()) == 16 and adjacent_pairs(mx) == 7
    f.close()


def _raises(code, fn, *a, **k):
    with pytest.raises(Pre3Error) as e:
        fn(*a, **k)
    assert e.value.code == code, e.value


def test_capacity_is_a_status(pre3):
    im = image("noise_200x200")
    want = fr.fast_corner_detect_9(im, 5)
    assert len(want) > _lib.FAST_MAX_CORNERS                                 # the raw list does not fit ...
    f = bare_filter(pre3, im.shape)
    f.set_image(im)
    _raises(-6, f.fast_corner_detect_9, 5)
    mx, ms = f.fast_nonmax(5, 20)                                            # ... the context stays usable: the suppressed list fits
    rmx, rms = fr.fast_nonmax(im, 5, 20)
    assert len(rmx) <= _lib.FAST_MAX_CORNERS and np.array_equal(mx, rmx) and np.array_equal(ms, rms)
    got = f.fast_corner_detect_9(40)
    assert np.array_equal(got, fr.fast_corner_detect_9(im, 40))
    f.close()


def test_argument_errors(pre3):
    im = image("crop")
    f = bare_filter(pre3, im.shape)
    _raises(-4, f.fast_corner_detect_9, 10)                                  # no image
    f.set_image(im)
    for box in [(-1, 0, 20, 20), (0, -1, 20, 20), (0, 0, 145, 176), (0, 0, 144, 177), (140, 0, 7, 7), (0, 170, 7, 7), (0, 0, 6, 20), (0, 0, 20, 6), (0, 0, 2 ** 31 - 1, 7)]:
        _raises(-1, f.fast_corner_detect_9, 10, box=box)
    _raises(-1, f.fast_corner_detect_9, -1)
    _raises(-1, f.fast_nonmax, 10, -1)
    assert _lib.lib.pre3_fast_detect(f._ctx, 0, 0, 144, 176, 10, 20, 1, None, None, None) == -1
    assert np.array_equal(f.fast_corner_detect_9(10), fixture()["corners_10"])          # usable afterwards
    f.close()


# ---- initialize_a_feature --------------------------------------------------------------------------------------------------------------------------
def base_planes(shape, seed=5):
    rng = np.random.default_rng(seed)
    return dict(z=rng.uniform(1.0, 5.0, shape), x=rng.uniform(-2, 2, shape), y=rng.uniform(-2, 2, shape), amp=rng.uniform(100, 30000, shape),
                conf=rng.uniform(0.8, 1.0, shape))


def ref_planes(frame):
    x, y, z, conf = frame.planes()
    return dict(x=x, y=y, z=z, conf=conf, cmax=frame.maxima()[1])


def gate0_of(frame, uv):
    """pre3_sr_frame_keypoints' gate-0 outputs at one pixel"""
    k = frame.keypoints(np.array([[float(uv[0])], [float(uv[1])]]), gate=0)
    return (k["rho"][0], k["xyz"][:, 0]) if len(k["rho"]) else (None, None)


def landmark_scene(orc, uvs):
    """landmarks the camera at x_k_k sees at the given pixels (144 x 176)"""
    key = ("scene", tuple(map(tuple, uvs)))
    if key not in _CACHE:
        _CACHE[key] = pc.build_scene(orc, 144, 176, [dict(uv=(float(u), float(v)), S=pc.S_of(2.0), depth=6.0 + i) for i, (u, v) in enumerate(uvs)], seed=21, moved=False)
    return _CACHE[key]


def scene_filter(pre3, sc, dtype, extra=4):
    f = pre3.EkfFilter(pc.cam_list(sc["cam"]), sc["types"], dtype=dtype, max_hyp=16, max_landmarks=len(sc["types"]) + extra)
    f.set_x_p_k_k(sc["x"], sc["P"])
    f.set_image(fixture()["image"])
    return f


def uv_pred_of(f):
    f.predict_camera_measurements(which=_lib.X_K_K)
    lf = f.landmark_fields()
    return lf["h"][lf["has_h"] != 0]


def same_context(f, g, new=None):
    assert f.N == g.N and np.array_equal(f.lm_type, g.lm_type)
    assert np.array_equal(f.get_x_k_k(), g.get_x_k_k()) and np.array_equal(f.get_p_k_k(), g.get_p_k_k())
    if new:
        a, b = f.patches(first=new[0], count=new[1]), g.patches(first=new[0], count=new[1])
        assert a["has_patch"].all()
        for k in a:
            assert np.array_equal(a[k], b[k]), k
    for q in (f, g):
        q.ekf_prediction(np.array([0.01, 0, 0.02, 1.0, 0, 0, 0]))
    ra, rb = f.search_ic_matches_patch(pc.FD_FORK, 0.6), g.search_ic_matches_patch(pc.FD_FORK, 0.6)
    for a, b in zip(ra, rb):
        assert np.array_equal(a, b, equal_nan=True)


def boxes():
    fx = fixture()
    has = fx["box_first"][:, 0] > 0
    return fx["box_centres"][has], fx["box_centres"][~has]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_initialize_a_feature_walks_the_attempts(pre3, orc, dtype):
    srm = importlib.import_module("3pre_amd.sr4000")
    im = fixture()["image"]
    full, empty = boxes()
    assert len(empty) == 526
    # three landmarks at the centres of three boxes with corners; a fourth box with corners far from all of them
    c1, c2, c3 = (60, 50), (85, 90), (70, 125)
    for c in (c1, c2, c3):
        assert fr.box_first_maximum(im, c) is not None
    sc = landmark_scene(orc, [(c[1], c[0]) for c in (c1, c2, c3)])
    free = next(tuple(c) for c in full if all(abs(c[0] - o[0]) > 31 or abs(c[1] - o[1]) > 21 for o in (c1, c2, c3))
                and all(abs(c[1] - o[0]) > 31 or abs(c[0] - o[1]) > 21 for o in (c1, c2, c3)))
    with srm.SrFrame(144, 176) as fh:
        fh.load(base_planes((144, 176)))
        planes = ref_planes(fh)
        cases = {
            "first": ([free] + [c1] * 9, False, 1, fr.INITIALISED),
            "fourth": ([c1, c2, c3, free, free], False, 4, fr.INITIALISED),
            "none_free": ([c1, c2, c3, c1, c2, c3, c1, c2, c3, c1], False, 10, fr.NO_BOX),
            "empty_boxes": ([tuple(c) for c in empty[:10]], False, 10, fr.NO_BOX),
            "empty_then_first": ([tuple(c) for c in empty[100:102]] + [free], True, 3, fr.INITIALISED),
        }
        for name, (centres, strict, attempts, status) in cases.items():
            f, g = scene_filter(pre3, sc, dtype), scene_filter(pre3, sc, dtype)
            want = fr.initialize_a_feature(im, planes, uv_pred_of(g), centres, strict)
            assert (want["attempts"], want["status"]) == (attempts, status), (name, want)
            got = f.initialize_a_feature(fh, 1.0, centres, strict_reference=strict)
            assert (got["status"], got["attempts"]) == (want["status"], want["attempts"]), (name, got, want)
            assert np.array_equal(got["centres"], np.array(centres)[:attempts])
            if status == fr.INITIALISED:
                rho, xyz = gate0_of(fh, want["uv"])
                assert tuple(got["uv"]) == want["uv"] and got["rho"] == rho == want["rho"] and np.array_equal(got["xyz"], xyz) and got["landmark"] == 3
                g.add_features_inverse_depth(np.array([got["uv"]], dtype=np.float64), 1.0, got["rho"])
                g.patch_cut(np.array([got["uv"]], np.int32), first=3)
                same_context(f, g, new=(3, 1))
            else:
                assert got["uv"] is None and f.N == 3
                assert np.array_equal(f.get_x_k_k(), g.get_x_k_k()) and np.array_equal(f.get_p_k_k(), g.get_p_k_k())
            f.close()
            g.close()


def test_both_forms_of_the_box_test_pick_different_attempts(pre3, orc):
    srm = importlib.import_module("3pre_amd.sr4000")
    im = fixture()["image"]
    c1, c2 = (60, 120), (88, 60)
    assert fr.box_first_maximum(im, c1) is not None and fr.box_first_maximum(im, c2) is not None
    sc = landmark_scene(orc, [(c1[1], c1[0])])               # a landmark at the centre of box 1: inside with the axes matched, outside as written
    with srm.SrFrame(144, 176) as fh:
        fh.load(base_planes((144, 176)))
        planes = ref_planes(fh)
        seen = {}
        for strict in (True, False):
            f = scene_filter(pre3, sc, "f64")
            want = fr.initialize_a_feature(im, planes, uv_pred_of(f), [c1, c2], strict)
            got = f.initialize_a_feature(fh, 1.0, [c1, c2], strict_reference=strict)
            assert (got["status"], got["attempts"], tuple(got["uv"])) == (want["status"], want["attempts"], want["uv"])
            seen[strict] = got["attempts"]
            f.close()
        assert seen == {True: 1, False: 2}


def test_depth_refusals_end_the_call(pre3):
    srm = importlib.import_module("3pre_amd.sr4000")
    im = fixture()["image"]
    full, empty = boxes()
    centres = [tuple(empty[0]), tuple(full[40]), tuple(full[400])]
    u, v = fr.box_first_maximum(im, centres[1])
    for kind, status in (("nan", fr.NO_DEPTH_NAN), ("near", fr.NO_DEPTH_NEAR), ("conf", fr.NO_DEPTH_CONF)):
        p = base_planes((144, 176))
        blk = (slice(v - 4, v + 3), slice(u - 4, u + 3))
        if kind == "nan":
            p["x"][v - 1, u - 1] = np.nan
        elif kind == "near":
            for k in "xyz":
                p[k][blk] = 0.05
        else:
            p["conf"][blk] = 0.1
        with srm.SrFrame(144, 176) as fh:
            fh.load(p)
            f = bare_filter(pre3, (144, 176))
            f.set_image(im)
            want = fr.initialize_a_feature(im, ref_planes(fh), np.zeros((0, 2)), centres)
            assert (want["status"], want["attempts"]) == (status, 2), (kind, want)
            got = f.initialize_a_feature(fh, 1.0, centres)
            assert (got["status"], got["attempts"], tuple(got["uv"])) == (status, 2, (u, v)) and got["rho"] is None and f.N == 0
            assert gate0_of(fh, (u, v))[0] is None                     # the keypoint gate refuses the same pixel
            f.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_empty_map_and_seeded_form(pre3, dtype):
    srm = importlib.import_module("3pre_amd.sr4000")
    im = fixture()["image"]
    with srm.SrFrame(144, 176) as fh:
        fh.load(base_planes((144, 176)))
        planes = ref_planes(fh)
        tried = []
        for seq in (0, 1, 7):
            centres = fr.seeded_centres(91, seq, 144, 176)
            tried.append(centres.tolist())
            f, g, t = bare_filter(pre3, (144, 176), dtype), bare_filter(pre3, (144, 176), dtype), bare_filter(pre3, (144, 176), dtype)
            for q in (f, g, t):
                q.set_image(im)
            want = fr.initialize_a_feature(im, planes, np.zeros((0, 2)), centres)
            a = f.initialize_a_feature_seeded(fh, 1.0, 91, seq)
            b = g.initialize_a_feature(fh, 1.0, centres)
            assert a["status"] == b["status"] == want["status"] == fr.INITIALISED and a["attempts"] == b["attempts"] == want["attempts"]
            assert tuple(a["uv"]) == tuple(b["uv"]) == want["uv"] and a["rho"] == b["rho"] == want["rho"] and a["landmark"] == 0
            assert np.array_equal(a["centres"], centres[:a["attempts"]]) and np.array_equal(a["centres"], b["centres"])
            t.add_features_inverse_depth(np.array([a["uv"]], dtype=np.float64), 1.0, a["rho"])
            t.patch_cut(np.array([a["uv"]], np.int32), first=0)
            same_context(f, t, new=(0, 1))
            for q in (f, g, t):
                q.close()
        assert tried[0] != tried[1] and tried[1] != tried[2]
    # the host loop of initialize_features.m:110-142 with its declared bound
    with srm.SrFrame(144, 176) as fh:
        fh.load(base_planes((144, 176)))
        f = bare_filter(pre3, (144, 176), dtype, cap=8)
        f.set_image(im)
        res = f.initialize_features_fast(fh, 3, 1.0, 5, seq0=10, max_calls=50)
        assert sum(r["status"] == 0 for r in res) == 3 and f.N == 3 and len(res) <= 50 and f.patches()["has_patch"].all()
        assert len(f.initialize_features_fast(fh, 3, 1.0, 5, seq0=100, max_calls=2)) <= 2
        f.close()


def test_init_argument_errors(pre3):
    srm = importlib.import_module("3pre_amd.sr4000")
    im = fixture()["image"]
    with srm.SrFrame(144, 176) as fh, srm.SrFrame(60, 80) as small, srm.SrFrame(144, 176) as unloaded:
        fh.load(base_planes((144, 176)))
        small.load(base_planes((60, 80)))
        f = bare_filter(pre3, (144, 176), cap=1)
        ok = [(60, 60)]
        _raises(-4, f.initialize_a_feature, fh, 1.0, ok)                               # no image
        f.set_image(im)
        _raises(-4, f.initialize_a_feature, unloaded, 1.0, ok)
        _raises(-1, f.initialize_a_feature, small, 1.0, ok)
        for bad in ([(50, 60)], [(93, 60)], [(60, 40)], [(60, 135)], [(60, 60)] * 11, np.zeros((0, 2))):
            _raises(-1, f.initialize_a_feature, fh, 1.0, bad)
        _raises(-1, f.initialize_a_feature, fh, float("nan"), ok)
        _raises(-1, f.initialize_a_feature, fh, 1.0, ok, threshold=-2)
        assert f.N == 0
        assert f.initialize_a_feature(fh, 1.0, [(92, 134), (51, 41), (70, 70)])["status"] in (0, 1)      # the corners of the range are accepted
        if f.N == 1:
            _raises(-6, f.initialize_a_feature, fh, 1.0, ok)                           # no room for one more
        f.close()
    g = bare_filter(pre3, (60, 80))
    g.set_image(np.zeros((60, 80), np.uint8))
    with srm.SrFrame(60, 80) as small:
        small.load(base_planes((60, 80)))
        _raises(-1, g.initialize_a_feature_seeded, small, 1.0, 1, 1)                   # no room for a box centre
    g.close()


# ---- initialize_n_features_fast ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_initialize_n_features_fast(pre3, orc, dtype):
    srm = importlib.import_module("3pre_amd.sr4000")
    im = fixture()["image"]
    p = base_planes((144, 176))
    p["x"][:, 60:75] = np.nan                                # a band of NaN ...
    p["conf"][100:115, :] = 0.05                             # ... a band of low confidence ...
    for k in "xyz":
        p[k][30:40, 120:140] = 0.02                          # ... and a near patch
    sc = landmark_scene(orc, [(40, 40), (120, 100)])
    with srm.SrFrame(144, 176) as fh:
        fh.load(p)
        planes = ref_planes(fh)
        uv, verdict, rho = fr.initialize_n_features_fast(im, planes)
        keep = verdict == fr.GATE_KEPT
        print("maxima", len(uv), "kept", int(keep.sum()), "verdicts", np.bincount(verdict, minlength=5).tolist())
        assert all((verdict == s).any() for s in (fr.GATE_KEPT, fr.NO_DEPTH_NAN, fr.NO_DEPTH_NEAR, fr.NO_DEPTH_CONF)) and keep.sum() >= 20
        n = int(keep.sum())
        f, g = scene_filter(pre3, sc, dtype, extra=n), scene_filter(pre3, sc, dtype, extra=n)
        got = f.initialize_n_features_fast(fh, 1.0)
        assert got["n_added"] == n and np.array_equal(got["uv"], uv) and np.array_equal(got["verdict"], verdict)
        assert np.array_equal(got["rho"][keep], rho[keep]) and not got["rho"][~keep].any()
        k = fh.keypoints(np.asfortranarray(uv.T.astype(np.float64)), gate=0)
        assert np.array_equal(k["keep_idx"], np.nonzero(keep)[0]) and np.array_equal(k["rho"], got["rho"][keep])
        g.add_features_inverse_depth(uv[keep].astype(np.float64), 1.0, rho[keep])
        g.patch_cut(uv[keep], first=2)
        same_context(f, g, new=(2, n))
        f.close()
        g.close()
        # not enough room: refused before the map is touched
        f = scene_filter(pre3, sc, dtype, extra=n - 1)
        x0, P0 = f.get_x_k_k(), f.get_p_k_k()
        _raises(-6, f.initialize_n_features_fast, fh, 1.0)
        assert f.N == 2 and np.array_equal(f.get_x_k_k(), x0) and np.array_equal(f.get_p_k_k(), P0)
        f.close()


# ---- nothing that exists changes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_a_step_is_what_it_was(pre3, orc, dtype):
    """two contexts through prediction, patch search and a seeded step; one of them runs the detector in between (it owns no state of the step): x, P
    and the statistics agree bit for bit, as they do for a context that never makes the calls"""
    rng = np.random.default_rng(8)
    sc = pc.build_scene(orc, 144, 176, pc.spec_random(rng, 144, 176, 40, cart_every=3), seed=52)
    out = []
    for use in (False, True):
        f = pre3.EkfFilter(pc.cam_list(sc["cam"]), sc["types"], dtype=dtype, max_hyp=16, max_landmarks=46)
        f.set_x_p_k_k(sc["x"], sc["P"])
        f.set_image(sc["imB"])
        b = sc["bank"]
        f.set_patches(b["patch"], b["uv_init"], b["r_wc"], b["R_wc"])
        if use:
            f.fast_corner_detect_9(60)
        f.ekf_prediction_cv(0.1, 0.007, 0.007)
        if use:
            f.fast_nonmax(10, 20)
        meas, z = f.search_ic_matches_patch(pc.FD_FORK, 0.6)[:2]
        if use:
            f.fast_nonmax(5, 20, box=(20, 20, 104, 136))
        st = f.step_predicted_seeded(77, 1, 16)
        out.append((meas, z, f.get_x_k_k(), f.get_p_k_k(), st["n_li"], st["n_hi"]))
        f.close()
    assert len(out[0][0]) >= 10
    for a, b in zip(*out):
        assert np.array_equal(a, b)
