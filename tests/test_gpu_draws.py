"""GPU: the three seeded draw tables (pre3_draws.hip) against the Python-integer restatement in tests/draws_ref.py, and every
seeded entry point against its unseeded sibling fed with the restatement's table.

Tables are compared integer for integer; the siblings' outputs bit for bit (np.array_equal on floats, == on integers): behind the table the seeded
call launches exactly what the unseeded one launches.  The plane scenes first assert, on the restatement alone, that no collinearity decision sits
within 1e3 eps of the threshold; the VO lists that no position needed more than 32 redraws, half the cap."""
import ctypes as C
import importlib

import numpy as np
import pytest

import draws_ref as dr
import plane_fit_ref as pr
from test_heading_ref import axis_rot
from test_vo_oracle import scene as vo_scene

pytestmark = pytest.mark.gpu
synth = importlib.import_module("3pre_amd.synth")
plane = importlib.import_module("3pre_amd.plane")
vo = importlib.import_module("3pre_amd.vo")
_lib = importlib.import_module("3pre_amd._lib")

SEED, SEQ = 0x9E3779B97F4A7C15, 41          # (a seed with the top bit set: the words are unsigned all the way)
N_MAP = 480
M_SIZES = (0, 1, 3, 4, 5, 65, 400)
DRAW_SIZES = (1, 63, 64, 65, 200, 1000)
_REF_1P = {}


def ref_1p(seed, seq, m, n_draw):
    """the restatement's 1-point table, computed once per case and shared"""
    key = (seed, seq, m, n_draw)
    if key not in _REF_1P:
        _REF_1P[key] = dr.draw_1p(seed, seq, m, n_draw)
        _REF_1P[key].setflags(write=False)
    return _REF_1P[key]


# ---- 1-point ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table_filter(pre3):
    """a predicted, projected N = 480 map whose first 400 visible landmarks can be installed as measurements"""
    x0, P0, _ = synth.make_map(N_MAP)
    uv, vis = synth.pixels(x0[:7], x0[13:].reshape(N_MAP, 6))
    cand = np.nonzero(vis)[0].astype(np.int32)
    assert len(cand) >= max(M_SIZES)
    f = pre3.EkfFilter(synth.CAM, np.zeros(N_MAP, np.int32), dtype="f32", max_hyp=max(DRAW_SIZES))
    f.set_x_p_k_km1(x0, P0)
    f.search_IC_matches()
    yield f, cand, uv
    f.close()


@pytest.mark.parametrize("m", M_SIZES)
def test_one_point_tables(table_filter, m):
    f, cand, uv = table_filter
    f.set_measurements(cand[:m], uv[cand[:m]])
    for n_draw in DRAW_SIZES:
        out = f.ransac_hypotheses_seeded(SEED, SEQ, n_draw, threshold=1.0, early_exit=False)
        ref = ref_1p(SEED, SEQ, m, n_draw)
        assert out["k"] == ref.shape[1] == (3 if m > 3 else 1)
        assert np.array_equal(out["hyp"], ref), (m, n_draw)
        if m > 0:
            # the scoring behind the table is pre3_ransac's
            plain = f.ransac_hypotheses(ref, threshold=1.0, early_exit=False)
            assert np.array_equal(out["support"], plain["support"]) and np.array_equal(out["li_mask"], plain["li_mask"])
            assert all(out[k] == plain[k] for k in ("best", "iters", "n_hyp", "max_support"))
        else:
            assert out["best"] == -1 and (out["support"] == -1).all()


def test_one_point_stream_is_a_function_of_seed_and_seq(table_filter):
    f, cand, uv = table_filter
    f.set_measurements(cand[:65], uv[cand[:65]])
    a = f.ransac_hypotheses_seeded(SEED, SEQ, 200)["hyp"]
    assert np.array_equal(a, f.ransac_hypotheses_seeded(SEED, SEQ, 200)["hyp"])
    b = f.ransac_hypotheses_seeded(SEED, SEQ + 1, 200)["hyp"]
    c = f.ransac_hypotheses_seeded(SEED + 1, SEQ, 200)["hyp"]
    assert not np.array_equal(a, b) and not np.array_equal(a, c) and not np.array_equal(b, c)
    assert np.array_equal(b, ref_1p(SEED, SEQ + 1, 65, 200)) and np.array_equal(c, ref_1p(SEED + 1, SEQ, 65, 200))


def _state(f):
    li, hi = f.get_flags()
    return f.get_x_k_k(), f.get_p_k_k(), li.copy(), hi.copy()


def _same_state(a, b):
    assert all(np.array_equal(u, v) for u, v in zip(a, b))


def test_step_predicted_seeded_on_the_snapshot(pre3, sr4000):
    g = sr4000
    m = len(g["meas_idx"])
    ref = ref_1p(SEED, 3, m, 40)
    res = []
    for seeded in (True, False):
        f = pre3.EkfFilter(g["cam"], np.zeros(g["N"], np.int32), dtype="f64", max_hyp=64, std_z=g["std_z"])
        f.set_x_p_k_km1(g["x_k_km1"], g["p_k_km1"])
        f.search_IC_matches()
        f.set_measurements(g["meas_idx"], g["z"][g["meas_idx"]])
        if seeded:
            st = f.step_predicted_seeded(SEED, 3, 40, return_hyp=True)
            assert np.array_equal(st.pop("hyp"), ref)
        else:
            st = f.step_predicted(ref)
        res.append((st, _state(f)))
        f.close()
    assert res[0][0] == res[1][0] and res[0][0]["n_li"] > 0
    _same_state(res[0][1], res[1][1])


@pytest.mark.parametrize("pend", [False, True])
def test_chained_seeded_steps_on_a_synthetic_map(pre3, pend):
    """three chained steps, N = 120, fp32: step_predicted_seeded behind ekf_prediction + search_IC_matches + set_measurements, and step_seeded, against
    step_predicted / step given the restatement's tables -- also with the HI update deferred and its down-date pending across the step boundary"""
    N, N_HYP = 120, 60
    seq = synth.make_sequence(N, 3, N_HYP, seed=77, motion_noise=2.5)

    def run(form):
        f = pre3.EkfFilter(seq["cam"], np.zeros(N, np.int32), dtype="f32", max_hyp=N_HYP)
        if pend:
            f.defer_hi_update(True)
            assert f.pend_hi(True)
        f.set_x_p_k_k(seq["x0"], seq["P0"])
        sts = []
        for t, s in enumerate(seq["steps"]):
            m = len(s["meas_idx"])
            assert m > 3
            ref = ref_1p(SEED, t, m, N_HYP)
            if form.startswith("predicted"):
                f.ekf_prediction(s["u"])
                f.search_IC_matches()
                f.set_measurements(s["meas_idx"], s["z"])
                sts.append(f.step_predicted_seeded(SEED, t, N_HYP, threshold=1.0, early_exit=False) if form.endswith("seeded")
                           else f.step_predicted(ref, threshold=1.0, early_exit=False))
            elif form == "step_seeded":
                sts.append(f.step_seeded(s["u"], s["meas_idx"], s["z"], SEED, t, N_HYP, threshold=1.0, early_exit=False))
            else:
                sts.append(f.step(s["u"], s["meas_idx"], s["z"], ref, threshold=1.0, early_exit=False))
        out = (sts, _state(f))
        f.close()
        return out

    for a, b in (("predicted_seeded", "predicted"), ("step_seeded", "step")):
        ra, rb = run(a), run(b)
        assert ra[0] == rb[0], (a, ra[0], rb[0])
        assert sum(s["n_li"] for s in ra[0]) > 0
        _same_state(ra[1], rb[1])


# ---- VO --------------------------------------------------------------------------------------------------------------------------------------------
VO_CASES = {4: (21, 5), 5: (21, 5), 9: (21, 5), 60: (21, 5)}          # pnum -> (scene seed, draw seed), chosen on the CPU: no cap, at most 32 redraws


def vo_case(pnum):
    """a scene of tests/test_vo_oracle.py whose match list has a third of its matches (pnum // 3 of them) on one frame-1 keypoint"""
    rng, R, T, p1, p2, match, bad = vo_scene(pnum, VO_CASES[pnum][0], outliers=0.2)
    match = match.astype(np.float64)
    g = pnum // 3
    match[0, :g] = match[0, 0]
    return p1, p2, match


def _vo_same(a, b):
    for k in ("rot", "trans", "euler", "u", "cnum", "state", "inliers"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("error_mean", "error_std", "dist", "sta", "n_support", "n_iterations", "best"):
        assert a[k] == b[k], k


@pytest.mark.parametrize("pnum", sorted(VO_CASES))
def test_vo_draws_and_results(pre3, pnum):
    p1, p2, match = vo_case(pnum)
    n_hyp, seed = vo.vo_rst(pnum), VO_CASES[pnum][1]
    ref, capped, most = dr.draw_vo(seed, SEQ, match, n_hyp)
    assert capped == 0 and most <= dr.VO_MAX_REDRAWS // 2, (capped, most)
    out = vo.vo_ransac_seeded(p1, p2, match, seed, SEQ)
    assert np.array_equal(out["draws"], ref) and out["capped"] == 0
    _vo_same(out, vo.vo_ransac(p1, p2, ref))


def test_vo_cap(pre3):
    """every match on one frame-1 keypoint: no second position is admissible; each position stops after 64 redraws and the call returns"""
    p1, p2, match = vo_case(9)
    match[0, :] = 7.0
    ref, capped, most = dr.draw_vo(3, 0, match, 50)
    assert capped == 50 and most == dr.VO_MAX_REDRAWS
    out = vo.vo_ransac_seeded(p1, p2, match, 3, 0, n_hyp=50)
    assert out["capped"] == 50 and np.array_equal(out["draws"], ref)
    _vo_same(out, vo.vo_ransac(p1, p2, ref))


def test_vo_frames_seeded(pre3):
    rng = np.random.default_rng(13)
    rows, cols, K, pnum = 144, 176, 40, 9
    img = [rng.uniform(-1, 1, (rows, cols)), rng.uniform(-1, 1, (rows, cols)), rng.uniform(0.8, 4.0, (rows, cols))]
    frm1 = np.stack([rng.uniform(1, cols, K), rng.uniform(1, rows, K)])
    frm2 = np.stack([rng.uniform(1, cols, K), rng.uniform(1, rows, K)])
    match = np.stack([rng.permutation(K)[:pnum] + 1.0, rng.permutation(K)[:pnum] + 1.0])
    match[0, :3] = match[0, 0]
    ref, capped, most = dr.draw_vo(5, 2, match, vo.vo_rst(pnum))
    assert capped == 0 and most <= dr.VO_MAX_REDRAWS // 2
    out = vo.vo_ransac_frames_seeded(frm1, frm2, match, *img, *img, 5, 2)
    assert np.array_equal(out["draws"], ref) and out["capped"] == 0
    plain = vo.vo_ransac_frames(frm1, frm2, match, *img, *img, ref)
    _vo_same(out, plain)
    assert np.array_equal(out["pset1"], plain["pset1"]) and np.array_equal(out["pset2"], plain["pset2"])


# ---- plane -----------------------------------------------------------------------------------------------------------------------------------------
SMALL_BOX = (60, 99, 80, 87)                # 40 x 8
PLANE_MARGIN = 1e3


def zero_scene():
    """scene 1 with 30 % of the pixels an invalid return (all-zero, as the SR4000 reports one): repeated points, so collinear triples occur"""
    x, y, z, _ = pr.scene(1, 0.1)
    dead = np.random.default_rng(9).random(x.shape) < 0.3
    x, y, z = x.copy(), y.copy(), z.copy()
    x[dead] = 0.0; y[dead] = 0.0; z[dead] = 0.0
    return x, y, z


def _plane_same(a, b):
    for k in ("B", "R", "p_orig", "p_ray", "counts", "inliers"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("N", "sta", "n_inliers", "n_trials", "best"):
        assert a[k] == b[k], k


@pytest.mark.parametrize("box", [None, SMALL_BOX], ids=["default_box", "box_40x8"])
@pytest.mark.parametrize("n_draw", [1, 8, 1001])
def test_plane_draws_and_fit(pre3, box, n_draw):
    x, y, z, _ = pr.scene(2, 0.5)
    XYZ = plane.crop_points(x, y, z, box)[3]
    ref, most, margin = dr.draw_plane(SEED, SEQ, XYZ, n_draw)
    assert margin >= PLANE_MARGIN and most == 0, (margin, most)
    out = plane.plane_fit_seeded(x, y, z, SEED, SEQ, n_draw, box=box)
    assert np.array_equal(out["draws"], ref)
    _plane_same(out, plane.plane_fit(x, y, z, ref, box=box))


def test_plane_redraws_on_invalid_returns(pre3):
    """Three points of which two are the same invalid return give a cross product of exactly zero, whatever the rounding (every difference and every
    product pair is then bit-equal): those decisions do not sit on a rounding edge, and draw_plane_margins reports them apart.  Every other decision
    must keep the 1e3 eps distance."""
    x, y, z = zero_scene()
    XYZ = plane.crop_points(x, y, z)[3]
    assert 0.25 < (np.abs(XYZ).sum(0) == 0).mean() < 0.35
    ref, most, margin = dr.draw_plane(SEED, SEQ, XYZ, 1001)
    margin_distinct, n_repeated = dr.draw_plane_margins(SEED, SEQ, XYZ, 1001)
    assert most >= 1 and n_repeated > 0 and margin == 1.0          # (norm == 0 exactly: |0 - eps| / eps)
    assert margin_distinct >= PLANE_MARGIN, margin_distinct
    out = plane.plane_fit_seeded(x, y, z, SEED, SEQ, 1001)
    assert np.array_equal(out["draws"], ref)
    _plane_same(out, plane.plane_fit(x, y, z, ref))


def _rotation_onto(a, b):
    ax = np.cross(a, b)
    return axis_rot(ax, np.degrees(np.arctan2(np.linalg.norm(ax), a @ b)))


def _q2R(q):
    return synth.q2r(q)


def test_heading_from_scan_seeded_queued_between_two_steps(pre3):
    """defer_hi_update + pend_hi, a step, the scan queued with nothing read back, a second step: bit-equal to the same chain with heading_from_scan
    given the restatement's draws.  The scene is turned as one rigid body so that the fitted normal lies 1.5 degrees from the heading the first step
    leaves and the update is applied (checked on a third, waiting filter)."""
    N, N_HYP = 120, 60
    seq = synth.make_sequence(N, 2, N_HYP, seed=77, motion_noise=2.5)
    s0, s1 = seq["steps"]

    def start():
        f = pre3.EkfFilter(seq["cam"], np.zeros(N, np.int32), dtype="f32", max_hyp=N_HYP)
        f.defer_hi_update(True)
        assert f.pend_hi(True)
        f.set_x_p_k_k(seq["x0"], seq["P0"])
        f.step(s0["u"], s0["meas_idx"], s0["z"], s0["hyp"], threshold=1.0, early_exit=False)
        return f

    f = start()
    h1 = _q2R(f.get_x_k_k()[3:7])[:, 1]
    h1 = h1 / np.linalg.norm(h1)
    x, y, z, _ = pr.scene(3, 0.5)
    r = plane.plane_fit_seeded(x, y, z, SEED, SEQ)
    Q = _rotation_onto(r["R"][:, 1], axis_rot(np.cross(h1, [0.3, 0.5, 0.8]), 1.5) @ h1)
    p = np.einsum("ij,jrc->irc", Q, np.stack([-x, -y, z]))
    x, y, z = -p[0], -p[1], p[2]
    ref, most, margin = dr.draw_plane(SEED, SEQ, plane.crop_points(x, y, z)[3], 1001)
    assert margin >= PLANE_MARGIN
    applied, fit = f.heading_from_scan_seeded(x, y, z, SEED, SEQ, transpose=False, strict_reference=False, return_draws=True)
    assert applied and fit["sta"] == 1 and np.array_equal(fit["draws"], ref)
    f.close()

    def run(seeded):
        f = start()
        if seeded:
            assert f.heading_from_scan_seeded(x, y, z, SEED, SEQ, transpose=False, strict_reference=False, wait=False) is None
        else:
            assert f.heading_from_scan(x, y, z, ref, transpose=False, strict_reference=False, wait=False) is None
        st = f.step(s1["u"], s1["meas_idx"], s1["z"], s1["hyp"], threshold=1.0, early_exit=False)
        out = (st, _state(f))
        f.close()
        return out

    a, b = run(True), run(False)
    assert a[0] == b[0]
    _same_state(a[1], b[1])


# ---- argument errors -------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_context_unchanged(pre3, table_filter):
    f, cand, uv = table_filter
    f.set_measurements(cand[:65], uv[cand[:65]])
    before = f.ransac_hypotheses_seeded(SEED, SEQ, 64, early_exit=False)
    x_before = f.get_x_k_km1()
    lib, ctx = _lib.lib, f._ctx
    st = np.zeros(8, np.int32)
    E_ARG = -1
    for n_draw in (0, -1, max(DRAW_SIZES) + 1):
        assert lib.pre3_ransac_seeded(ctx, 1, 1, n_draw, 1.0, 0, None, None, None, None, _lib.dptr(st)) == E_ARG
        assert lib.pre3_step_predicted_seeded(ctx, 1, 1, n_draw, 1.0, 0, 5.9915, None, None, _lib.dptr(st)) == E_ARG
        u = np.array([0, 0, 0, 1.0, 0, 0, 0])
        assert lib.pre3_step_seeded(ctx, _lib.dptr(u), 0, None, None, 1, 1, n_draw, 1.0, 0, 5.9915, None, None, _lib.dptr(st)) == E_ARG
    assert lib.pre3_ransac_seeded(None, 1, 1, 8, 1.0, 0, None, None, None, None, None) == E_ARG
    assert lib.pre3_step_seeded(ctx, None, 0, None, None, 1, 1, 8, 1.0, 0, 5.9915, None, None, None) == E_ARG
    assert lib.pre3_step_seeded(ctx, _lib.dptr(u), 2, None, None, 1, 1, 8, 1.0, 0, 5.9915, None, None, None) == E_ARG
    # the plane range and its required pointers, stateless and on the context
    x, y, z, _ = pr.scene(0, 0.1)
    imgs = plane._images(x, y, z)
    res = plane.PlaneResult()
    P = [_lib.dptr(a) for a in imgs]
    for n_draw in (0, 1002):
        assert lib.pre3_plane_fit_seeded(0, 144, 176, *P, None, 0.02, n_draw, 1, 1, None, None, None, C.byref(res)) == E_ARG
        assert lib.pre3_heading_from_scan_seeded(ctx, 144, 176, *P, None, 0.02, n_draw, 1, 1, 1, 1, None, None, None) == E_ARG
    assert lib.pre3_plane_fit_seeded(0, 144, 176, *P, None, 0.02, 8, 1, 1, None, None, None, None) == E_ARG
    assert lib.pre3_plane_fit_seeded(0, 144, 176, None, P[1], P[2], None, 0.02, 8, 1, 1, None, None, None, C.byref(res)) == E_ARG
    assert lib.pre3_heading_from_scan_seeded(None, 144, 176, *P, None, 0.02, 8, 1, 1, 1, 1, None, None, None) == E_ARG
    assert lib.pre3_heading_from_scan_seeded(ctx, 144, 176, P[0], None, P[2], None, 0.02, 8, 1, 1, 1, 1, None, None, None) == E_ARG
    # VO: fewer than four matches, null required pointers
    p1, p2, match = vo_case(9)
    a1, a2, mt = np.ascontiguousarray(p1.T), np.ascontiguousarray(p2.T), np.asfortranarray(match)
    vres = vo.VoResult()
    assert lib.pre3_vo_ransac_seeded(0, 3, _lib.dptr(a1), _lib.dptr(a2), _lib.dptr(mt), 1, 1, 1, None, None, None, None, None, C.byref(vres)) == E_ARG
    assert lib.pre3_vo_ransac_seeded(0, 9, _lib.dptr(a1), _lib.dptr(a2), None, 8, 1, 1, None, None, None, None, None, C.byref(vres)) == E_ARG
    assert lib.pre3_vo_ransac_seeded(0, 9, None, _lib.dptr(a2), _lib.dptr(mt), 8, 1, 1, None, None, None, None, None, C.byref(vres)) == E_ARG
    assert lib.pre3_vo_ransac_seeded(0, 9, _lib.dptr(a1), _lib.dptr(a2), _lib.dptr(mt), 0, 1, 1, None, None, None, None, None, C.byref(vres)) == E_ARG
    img = np.asfortranarray(np.ones((144, 176)))
    fr = np.asfortranarray(np.ones((2, 12)))
    I = [_lib.dptr(img)] * 6
    assert lib.pre3_vo_ransac_frames_seeded(0, 144, 176, *I, 2, 12, _lib.dptr(fr), 12, _lib.dptr(fr), 3, _lib.dptr(mt), 1, 1, 1,
                                            None, None, None, None, None, None, None, C.byref(vres)) == E_ARG
    assert lib.pre3_vo_ransac_frames_seeded(0, 144, 176, *I, 2, 12, _lib.dptr(fr), 12, _lib.dptr(fr), 9, None, 8, 1, 1,
                                            None, None, None, None, None, None, None, C.byref(vres)) == E_ARG
    # the context is as it was: the same measurements, the same prediction, the same round
    assert f.m == 65 and np.array_equal(f.get_x_k_km1(), x_before)
    after = f.ransac_hypotheses_seeded(SEED, SEQ, 64, early_exit=False)
    assert all(np.array_equal(before[k], after[k]) for k in before)
