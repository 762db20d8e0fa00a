"""GPU: the floor-plane fit on the device -- pre3_plane_fit (plane.plane_fit) and pre3_heading_from_scan (EkfFilter.heading_from_scan), DESIGN.md
section 17 -- against the numpy restatement of plane_fit_to_data.m in tests/plane_fit_ref.py and, for the update, oracle/np_twin.update fed with the
restatement's R (tests/test_heading_ref.heading_update).

Integers (the score of every draw, winner, trial count, inlier mask, status) must be identical; N to 1e-12 relative; B, R, p_orig, p_ray to 1e-12 (the
tolerance tests/test_gpu_vo.py uses for transforms).  Each scene first asserts on the restatement alone that no point of a trial that happened lies
within 1e-9 of the inlier distance, so that integer equality cannot hinge on a rounding.  The heading update keeps the tolerances of
tests/test_gpu_update_rows.py: 1e-12 x scale on fp64 contexts, 2e-5 x scale on fp32."""
import ctypes as C
import importlib

import numpy as np
import pytest

import plane_fit_ref as pr
from oracle import np_twin as tw
from test_heading_ref import R2q, axis_rot, heading_update

pytestmark = pytest.mark.gpu
synth = importlib.import_module("3pre_amd.synth")
plane = importlib.import_module("3pre_amd.plane")
_lib = importlib.import_module("3pre_amd._lib")

SCENES = [(seed, outl) for seed in range(4) for outl in (0.1, 0.5, 0.7)]
NPTS = 65 * 71


def _same(g, r, margin=1e-9):
    assert r["margin"] >= margin, r["margin"]
    assert np.array_equal(g["counts"], r["counts"])
    assert (g["best"], g["n_trials"], g["n_inliers"], g["sta"]) == (r["best"], r["n_trials"], r["n_inliers"], r["sta"])
    assert np.array_equal(g["inliers"], r["inliers"])
    assert abs(g["N"] - r["N"]) <= 1e-12 * abs(r["N"]), (g["N"], r["N"])
    for k in ("B", "R", "p_orig", "p_ray"):
        assert np.abs(g[k] - r[k]).max() <= 1e-12, (k, np.abs(g[k] - r[k]).max())


@pytest.mark.parametrize("seed,outl", SCENES)
def test_the_twelve_scenes(pre3, seed, outl):
    x, y, z, _ = pr.scene(seed, outl)
    draws = pr.scene_draws(seed, NPTS)
    g, r = plane.plane_fit(x, y, z, draws), pr.plane_fit(x, y, z, draws)
    assert r["sta"] == 1
    _same(g, r)
    g2 = plane.plane_fit(x, y, z, draws)                      # the same bits on every run
    assert all(np.array_equal(g[k], g2[k]) for k in g)


def test_a_second_box_and_too_few_draws(pre3):
    x, y, z, _ = pr.scene(2, 0.7)
    box = (60, 140, 30, 150)
    draws = pr.scene_draws(2, 81 * 121)
    _same(plane.plane_fit(x, y, z, draws, box=box), pr.plane_fit(x, y, z, draws, box))
    d8 = pr.scene_draws(2, NPTS)[:8]
    g, r = plane.plane_fit(x, y, z, d8), pr.plane_fit(x, y, z, d8)
    assert r["sta"] == 2 and r["n_trials"] == 8
    _same(g, r)


def test_degenerate_draws(pre3):
    x, y, z, _ = pr.scene(1, 0.5)
    draws = pr.scene_draws(1, NPTS)
    # zeros behind a first trial that raised N count as trials
    d = draws.copy()
    d[1] = (5, 5, 9)
    d[2] = (7, 7, 7)
    g, r = plane.plane_fit(x, y, z, d), pr.plane_fit(x, y, z, d)
    assert r["counts"][1] == 0 and r["counts"][2] == 0 and r["n_trials"] > 3 and r["sta"] == 1
    _same(g, r)
    # in front of everything: N is still 1 after the first trial, the loop ends without a solution (ransac.m:224)
    d = draws.copy()
    d[0] = (5, 5, 9)
    g, r = plane.plane_fit(x, y, z, d), pr.plane_fit(x, y, z, d)
    assert (r["sta"], r["n_trials"], r["best"]) == (0, 1, -1)
    _same(g, r)
    # every draw degenerate
    d = np.repeat(np.arange(40, dtype=np.int32)[:, None], 3, 1)
    g, r = plane.plane_fit(x, y, z, d), pr.plane_fit(x, y, z, d)
    assert r["sta"] == 0 and not r["counts"].any() and r["margin"] == np.inf
    _same(g, r)
    assert not g["inliers"].any() and not g["R"].any() and not g["B"].any()


def test_a_tiny_inlier_distance_keeps_the_three_sample_points(pre3):
    x, y, z, _ = pr.scene(3, 0.1)
    draws = pr.scene_draws(3, NPTS)
    g, r = plane.plane_fit(x, y, z, draws, t=1e-9), pr.plane_fit(x, y, z, draws, t=1e-9)
    assert r["n_inliers"] == 3 and r["n_trials"] == 1001 and r["best"] == 0 and r["sta"] == 1
    assert sorted(np.nonzero(r["inliers"])[0]) == sorted(draws[0])
    # the sample points are at |d| ~ 1e-16, i.e. 1e-9 from the bound, and nothing else may come closer than 1e-12: d is three products and two
    # sums of numbers below 8, so its rounding error stays under 1e-14 and an integer cannot hinge on it
    _same(g, r, margin=1e-12)


def test_a_ray_parallel_to_the_plane(pre3):
    x, y, z, nrm = pr.scene(0, 0.1)
    x, y, z = x.copy(), y.copy(), z.copy()
    draws = pr.scene_draws(0, NPTS)
    # p_ray's pixel: row 80 + 32 - 20, column 50 + 35 (1-based).  First an outlier far from the floor, so that the fitted plane does not depend on it;
    # then a point of the same kind whose ray runs along that plane (the parallel test's tolerance is 1e-5)
    x[91, 84], y[91, 84], z[91, 84] = 0.0, -5.0, 1.0
    B = pr.plane_fit(x, y, z, draws)["B"]
    v = np.cross(B[:3], [1.0, 0.0, 0.0])
    v = 2.0 * v / np.linalg.norm(v)
    x[91, 84], y[91, 84], z[91, 84] = -v[0], -v[1], v[2]
    g, r = plane.plane_fit(x, y, z, draws), pr.plane_fit(x, y, z, draws)
    assert r["sta"] == 3 and np.abs(r["p_ray"] - v).max() == 0 and np.abs(r["B"]).max() > 0 and not r["R"].any()
    _same(g, r)


def _raw(x, y, z, draws, box=None, t=0.02, n_draw=None, rows=None, cols=None, res=True, null=None):
    imgs = [np.asfortranarray(a, dtype=np.float64) for a in (x, y, z)]
    d = _lib.i32(draws)
    p = [_lib.dptr(a) for a in imgs] + [_lib.dptr(d)]
    if null is not None:
        p[null] = None
    r = plane.PlaneResult()
    return _lib.lib.pre3_plane_fit(0, imgs[0].shape[0] if rows is None else rows, imgs[0].shape[1] if cols is None else cols, p[0], p[1], p[2],
                                   None if box is None else _lib.dptr(_lib.i32(box)), t, len(d) if n_draw is None else n_draw, p[3], None, None,
                                   C.byref(r) if res else None)


def test_argument_errors(pre3):
    x, y, z, _ = pr.scene(0, 0.1)
    draws = pr.scene_draws(0, NPTS, 16)
    assert _raw(x, y, z, draws) == 0
    for k in range(4):
        assert _raw(x, y, z, draws, null=k) == -1                                # a null pointer
    assert _raw(x, y, z, draws, res=False) == -1
    for box in ((0, 144, 50, 120), (80, 145, 50, 120), (80, 144, 50, 177), (90, 80, 50, 120), (80, 144, 60, 50)):
        assert _raw(x, y, z, draws, box=box) == -1                               # outside the image, or empty
    assert _raw(x, y, z, draws, rows=100) == -1                                  # the default box in an image of 100 rows
    assert _raw(x, y, z, np.zeros((4, 3), np.int32), box=(80, 80, 50, 51)) == -1     # two points
    assert _raw(x, y, z, np.zeros((4, 3), np.int32), box=(80, 118, 50, 120)) == -1   # 39 rows: p_ray's row, floor(39 / 2) + 1 - 20 = 0, is outside the box
    assert _raw(x, y, z, np.zeros((4, 3), np.int32), box=(80, 119, 50, 120)) == 0    # 40 rows: row 1
    bad = draws.copy()
    bad[3, 1] = NPTS
    assert _raw(x, y, z, bad) == -1
    bad[3, 1] = -1
    assert _raw(x, y, z, bad) == -1
    assert _raw(x, y, z, draws, n_draw=0) == -1
    assert _raw(x, y, z, pr.scene_draws(0, NPTS, 1002)) == -1
    assert _raw(x, y, z, draws, t=0.0) == -1 and _raw(x, y, z, draws, t=-1.0) == -1 and _raw(x, y, z, draws, t=float("nan")) == -1
    for img in range(3):
        for v in (np.nan, np.inf):
            a = [x.copy(), y.copy(), z.copy()]
            a[img][100, 60] = v                                                  # inside the box
            assert _raw(a[0], a[1], a[2], draws) == -1
            a = [x.copy(), y.copy(), z.copy()]
            a[img][10, 10] = v                                                   # outside it: not looked at
            assert _raw(a[0], a[1], a[2], draws) == 0
    with pytest.raises(pre3.Pre3Error) as e:
        plane.plane_fit(x, y, z, bad)
    assert e.value.code == -1 and "draws" in str(e.value)


# ---- the fit feeding the heading update -------------------------------------------------------------------------------------------------------------
def _types(N):
    return np.zeros(N, np.int32)


def _turned(R_plane, deg, axis=(1.0, 0.0, 0.4)):
    """a quaternion whose heading h = q2R(q)(:, 2) is about deg degrees from R_plane(:, 2)"""
    q = R2q(R_plane @ axis_rot(axis, deg))
    return q / np.linalg.norm(q)


def _fixture_filter(pre3, d):
    f = pre3.EkfFilter(d["cam"], _types(d["N"]), dtype="f64", max_hyp=8, std_z=d["std_z"])
    return f, d["x_k_k"].copy(), d["p_k_k"]


def _synth_filter(pre3, N=500):
    x0, P0, _ = synth.make_map(N, None)
    f = pre3.EkfFilter(synth.CAM, _types(N), dtype="f32", max_hyp=8)
    f.set_x_p_k_k(x0, P0)
    x0, P0 = f._get(0)
    return f, x0, P0


def _heading_case(f, x0, P0, scan, draws, r, deg, tol, strict, expect):
    """the filter's quaternion deg degrees from R2q(R'), then the scan: against the twin fed with the restatement's R"""
    Rp = r["R"].T
    x0 = x0.copy()
    x0[3:7] = _turned(Rp if r["sta"] == 1 else np.eye(3), deg)
    f.set_x_p_k_k(x0, P0)
    x0, P0 = f._get(0)
    applied, fit = f.heading_from_scan(*scan, draws, strict_reference=strict)
    assert f.rows_form() == 1
    assert (fit["sta"], fit["best"], fit["n_trials"], fit["n_inliers"]) == (r["sta"], r["best"], r["n_trials"], r["n_inliers"])
    assert np.abs(fit["R"] - r["R"]).max() <= 1e-12
    x, P = f._get(0)
    assert applied == expect
    if not expect:
        assert np.array_equal(x, x0) and np.array_equal(P, P0)
        if r["sta"] == 1:
            assert heading_update(x0, P0, Rp, strict)[2] is False
        return
    xt, Pt, at = heading_update(x0, P0, Rp, strict)
    assert at
    sc = np.abs(Pt).max()
    assert np.array_equal(P, P.T)
    assert np.abs(P - Pt).max() <= tol * sc, np.abs(P - Pt).max() / sc
    assert np.abs(x - xt).max() <= tol * max(1.0, np.abs(xt).max()), np.abs(x - xt).max()
    assert np.abs(x[3:7] - x0[3:7]).max() > 0


@pytest.mark.parametrize("ctx", ["fixture_f64", "synth_f32"])
def test_heading_from_scan(pre3, sr4000, ctx):
    f, x0, P0 = _fixture_filter(pre3, sr4000) if ctx == "fixture_f64" else _synth_filter(pre3)
    tol = 1e-12 if ctx == "fixture_f64" else 2e-5
    x, y, z, _ = pr.scene(1, 0.5)
    draws = pr.scene_draws(1, NPTS)
    r = pr.plane_fit(x, y, z, draws)
    assert r["sta"] == 1 and r["margin"] >= 1e-9
    for strict in (True, False):
        _heading_case(f, x0, P0, (x, y, z), draws, r, 1.5, tol, strict, True)
        _heading_case(f, x0, P0, (x, y, z), draws, r, 10.0, tol, strict, False)      # the plane 10 degrees off: the gate returns
    # fits that are not sta == 1 apply nothing: too few draws (2), no inlier (0), axes undefined (3)
    x7, y7, z7, _ = pr.scene(2, 0.7)
    d8 = pr.scene_draws(2, NPTS)[:8]
    r2 = pr.plane_fit(x7, y7, z7, d8)
    assert r2["sta"] == 2
    x0b = x0.copy()
    x0b[3:7] = _turned(r2["R"].T, 1.5)                                               # (the update WOULD apply with this R)
    f.set_x_p_k_k(x0b, P0)
    xa, Pa = f._get(0)
    applied, fit = f.heading_from_scan(x7, y7, z7, d8, strict_reference=False)
    xb, Pb = f._get(0)
    assert not applied and fit["sta"] == 2 and np.abs(fit["R"] - r2["R"]).max() <= 1e-12
    assert np.array_equal(xa, xb) and np.array_equal(Pa, Pb)
    dz = np.repeat(np.arange(10, dtype=np.int32)[:, None], 3, 1)
    _heading_case(f, x0, P0, (x, y, z), dz, pr.plane_fit(x, y, z, dz), 1.5, tol, False, False)
    f.close()


def test_errors_of_the_context_form(pre3):
    f, x0, P0 = _synth_filter(pre3, 100)
    x, y, z, _ = pr.scene(0, 0.1)
    draws = pr.scene_draws(0, NPTS, 16)
    bad = draws.copy()
    bad[0, 0] = NPTS
    with pytest.raises(pre3.Pre3Error) as e:
        f.heading_from_scan(x, y, z, bad)
    assert e.value.code == -1
    x1, P1 = f._get(0)
    assert np.array_equal(x0, x1) and np.array_equal(P0, P1)
    f.set_x_p_k_km1(x0, P0)                                                          # the prediction in the covariance buffer
    with pytest.raises(pre3.Pre3Error) as e:
        f.heading_from_scan(x, y, z, draws)
    assert e.value.code == -4
    f.close()


def _rotation_onto(a, b):
    """the rotation about a x b that takes the unit vector a to the unit vector b"""
    ax = np.cross(a, b)
    return axis_rot(ax, np.degrees(np.arctan2(np.linalg.norm(ax), a @ b)))


def test_queued_behind_a_step_without_a_wait(pre3, orc):
    """defer_hi_update + pend_hi, a step, the scan queued with nothing read back, a second step: equal to the chain that fits with plane_fit, reads R
    on the host and calls ekf_heading_update.  The scene's points are turned as one rigid body (the fit follows: it knows no preferred direction) so
    that the fitted normal lies 1.5 degrees from the heading the first step leaves, and the update is applied."""
    N, N_HYP = 500, 200
    thr = synth.HEADLINE["threshold"]
    seq = synth.make_sequence(N, 2, N_HYP, motion_noise=synth.HEADLINE["motion_noise"])
    s0, s1 = seq["steps"]
    types, off, _ = orc.landmark_table(np.zeros(N, int))
    ref = tw.step(types, off, seq["cam"], seq["x0"], seq["P0"], s0["u"], s0["meas_idx"], s0["z"], s0["hyp"], thr, early_exit=False)
    h1 = tw.q2R(ref["x_kk"][3:7])[:, 1]
    h1 = h1 / np.linalg.norm(h1)
    x, y, z, _ = pr.scene(3, 0.5)
    draws = pr.scene_draws(3, NPTS)
    r = pr.plane_fit(x, y, z, draws)
    perp = np.cross(h1, [0.3, 0.5, 0.8])
    Q = _rotation_onto(r["R"][:, 1], axis_rot(perp, 1.5) @ h1)
    p = np.einsum("ij,jrc->irc", Q, np.stack([-x, -y, z]))
    x, y, z = -p[0], -p[1], p[2]
    r = pr.plane_fit(x, y, z, draws)
    assert r["sta"] == 1 and r["margin"] >= 1e-9
    a7 = np.degrees(np.arccos(np.clip(h1 @ r["R"][:, 1], -1, 1)))
    assert 1.0 < a7 < 2.0, a7

    def run(fused):
        f = pre3.EkfFilter(seq["cam"], _types(N), dtype="f32", max_hyp=N_HYP)
        f.defer_hi_update(True)
        assert f.pend_hi(True)
        f.set_x_p_k_k(seq["x0"], seq["P0"])
        st = [f.step(s0["u"], s0["meas_idx"], s0["z"], s0["hyp"], threshold=thr, early_exit=False)]
        if fused:
            assert f.heading_from_scan(x, y, z, draws, transpose=False, strict_reference=False, wait=False) is None
            applied = None
            mid = None
        else:
            g = plane.plane_fit(x, y, z, draws)
            before = f.get_x_k_k()
            applied = f.ekf_heading_update(g["R"], strict_reference=False)
            mid = (before, f.get_x_k_k())
        st.append(f.step(s1["u"], s1["meas_idx"], s1["z"], s1["hyp"], threshold=thr, early_exit=False))
        out = (f.get_flags(), f.get_x_k_k(), f.get_p_k_k(), st, applied, mid)
        f.close()
        return out

    fa, xa, Pa, sa, _, _ = run(True)
    fb, xb, Pb, sb, applied, mid = run(False)
    assert applied
    # (the update did something in the host chain: the heading moved towards the plane's normal)
    ang = [np.degrees(np.arccos(np.clip(tw.q2R(xm[3:7])[:, 1] @ r["R"][:, 1], -1, 1))) for xm in mid]
    assert ang[1] < ang[0] < 4.0, ang
    assert sa == sb
    assert all(np.array_equal(u, v) for u, v in zip(fa, fb))
    sc = np.abs(Pb).max()
    assert np.isfinite(Pa).all()
    assert np.abs(Pa - Pb).max() <= 2e-5 * sc, np.abs(Pa - Pb).max() / sc
    assert np.abs(xa - xb).max() <= 2e-5 * max(1.0, np.abs(xb).max()), np.abs(xa - xb).max()
