"""GPU: measurement updates on the resident current estimate -- pre3_update_rows / pre3_heading_update (EkfFilter.update / .ekf_heading_update,
DESIGN.md section 15) against oracle/np_twin.update (fp64) and the numpy truth of ekf_heading_update.m in tests/test_heading_ref.py.

On fp32 contexts the twin starts from the x / P read back from the device just before the call, so that the rounding of the input to fp32 is not
counted as error.  Up to 16 rows the call takes the single-sweep form (PRE3_OPT_ROWS_FORM = 1), above that the general route (0)."""
import importlib

import numpy as np
import pytest

from oracle import np_twin as tw
from test_heading_ref import axis_rot, heading_angles, heading_rows, heading_update

pytestmark = pytest.mark.gpu
synth = importlib.import_module("3pre_amd.synth")
_lib = importlib.import_module("3pre_amd._lib")

SMALL, LARGE = (1, 3, 8, 16), (17, 64, 130)


def _types(N):
    return np.zeros(N, np.int32)


def _rows(n, r, rng, dense_R):
    """r rows of 13 non-zeros: the pose block (even rows; odd rows: 3 position columns only) and one landmark's 6 columns from a small pool, so
    that columns repeat across rows; scaled so that H P H' is of the order of R"""
    N = (n - 13) // 6
    pool = rng.choice(N, size=max(2, r // 3), replace=False)
    H = np.zeros((r, n))
    for a in range(r):
        cols = list(range(7)) if a % 2 == 0 else [0, 1, 2]
        o = 13 + 6 * int(pool[a % len(pool)])
        cols += list(range(o, o + 6))
        H[a, cols] = rng.normal(0, 30.0, len(cols))
    R = None
    if dense_R:
        B = rng.normal(0, 0.3, (r, r))
        R = B @ B.T + 0.5 * np.eye(r)
    h = rng.normal(0, 1.0, r)
    z = h + rng.normal(0, 0.5, r)
    return H, R, z, h


def _check(f, H, R, z, h, tol, form):
    x0, P0 = f._get(0)
    xt, Pt, _ = tw.update(x0, P0, H, np.eye(len(z)) if R is None else R, z, h)
    f.update(H, R, z, h)
    assert f.rows_form() == form
    x, P = f._get(0)
    sc = np.abs(Pt).max()
    assert np.isfinite(P).all() and np.isfinite(x).all()
    if form == 1:
        assert np.array_equal(P, P.T)                                        # update.m:38, exactly (the single-sweep form's own property)
    assert np.abs(P - Pt).max() <= tol * sc, (len(z), np.abs(P - Pt).max() / sc)
    assert np.abs(x - xt).max() <= tol * max(1.0, np.abs(xt).max()), (len(z), np.abs(x - xt).max())
    assert np.abs(x - x0).max() > 0                                          # (it did something)


def _synth_filter(pre3, N, dtype="f32", seed=None):
    x0, P0, _ = synth.make_map(N, seed)
    f = pre3.EkfFilter(synth.CAM, _types(N), dtype=dtype, max_hyp=8)
    f.set_x_p_k_k(x0, P0)
    return f


def test_generic_rows_on_the_sr4000_fixture_fp64(pre3, sr4000):
    d = sr4000
    f = pre3.EkfFilter(d["cam"], _types(d["N"]), dtype="f64", max_hyp=8, std_z=d["std_z"])
    rng = np.random.default_rng(11)
    for k, r in enumerate(SMALL + LARGE):
        f.set_x_p_k_k(d["x_k_k"], d["p_k_k"])
        _check(f, *_rows(d["n"], r, rng, dense_R=k % 2 == 1), tol=1e-12, form=1 if r <= 16 else 0)
    f.close()


def test_generic_rows_on_a_synthetic_map_fp32(pre3):
    f = _synth_filter(pre3, 500)
    x0, P0 = f._get(0)
    rng = np.random.default_rng(12)
    for k, r in enumerate(SMALL + LARGE):
        f.set_x_p_k_k(x0, P0)
        _check(f, *_rows(f.n, r, rng, dense_R=k % 2 == 0), tol=2e-5, form=1 if r <= 16 else 0)
    # two calls in a row: the second starts from what the first left on the device
    H, R, z, h = _rows(f.n, 5, rng, dense_R=False)
    _check(f, H, R, z, h, tol=2e-5, form=1)
    _check(f, H, R, z + 0.1, h, tol=2e-5, form=1)
    f.close()


@pytest.mark.parametrize("r", [3, 16])
def test_generic_rows_at_n2000_fp32(pre3, r):
    f = _synth_filter(pre3, 2000)
    _check(f, *_rows(f.n, r, np.random.default_rng(13 + r), dense_R=r == 16), tol=2e-5, form=1)
    f.close()


def test_zero_rows_and_what_else_stays(pre3):
    """r = 0 is bit-exact; flags, per-landmark fields and the map are what the step left; marginal() reads what get_state reads"""
    N = 300
    seq = synth.make_sequence(N, 1, 100, motion_noise=synth.HEADLINE["motion_noise"])
    f = pre3.EkfFilter(seq["cam"], _types(N), dtype="f32", max_hyp=100)
    f.set_x_p_k_k(seq["x0"], seq["P0"])
    s = seq["steps"][0]
    f.step(s["u"], s["meas_idx"], s["z"], s["hyp"], threshold=synth.HEADLINE["threshold"], early_exit=False)
    x0, P0 = f._get(0)
    f.update(np.zeros((0, f.n)), None, np.zeros(0), np.zeros(0))
    x1, P1 = f._get(0)
    assert np.array_equal(x0, x1) and np.array_equal(P0, P1)
    flags, fields = f.get_flags(), f.landmark_fields()
    mp = np.zeros(N, np.int32)
    assert _lib.lib.pre3_get_map(f._ctx, _lib.dptr(mp)) == N
    H, R, z, h = _rows(f.n, 8, np.random.default_rng(14), dense_R=True)
    f.update(H, R, z, h)
    assert f.rows_form() == 1
    flags2, fields2 = f.get_flags(), f.landmark_fields()
    mp2 = np.zeros(N, np.int32)
    assert _lib.lib.pre3_get_map(f._ctx, _lib.dptr(mp2)) == N
    assert all(np.array_equal(a, b) for a, b in zip(flags, flags2))
    assert all(np.array_equal(fields[k], fields2[k]) for k in fields)
    assert np.array_equal(mp, mp2)
    idx = np.array([0, 3, 6, 13, 14, 20, f.n - 1, 5])
    xm, Pm = f.marginal(idx)
    x2, P2 = f._get(0)
    assert np.array_equal(xm, x2[idx]) and np.array_equal(Pm, P2[np.ix_(idx, idx)])
    assert not np.array_equal(P2, P1)
    f.close()


def _raw(f, r, width, nnz, col, val, R=None, z=None, h=None):
    z = np.zeros(max(r, 1)) if z is None else z
    h = np.zeros(max(r, 1)) if h is None else h
    return _lib.lib.pre3_update_rows(f._ctx, r, width, _lib.dptr(_lib.i32(nnz)), _lib.dptr(_lib.i32(col)), _lib.dptr(_lib.f64(val)),
                                     _lib.dptr(R), _lib.dptr(_lib.f64(z)), _lib.dptr(_lib.f64(h)))


def test_errors(pre3):
    f = _synth_filter(pre3, 100)
    x0, P0 = f._get(0)
    # 17 non-zeros, a column outside [0, n), r above the row capacity: PRE3_E_ARG before anything runs
    assert _raw(f, 1, 17, [17], np.arange(17), np.ones(17)) == -1
    assert _raw(f, 1, 16, [2], [0, f.n] + [0] * 14, np.ones(16)) == -1
    assert _raw(f, 1, 16, [2], [-1, 3] + [0] * 14, np.ones(16)) == -1
    big = 100000
    assert _raw(f, big, 1, np.zeros(big), np.zeros(big), np.zeros(big), z=np.zeros(big), h=np.zeros(big)) == -1
    assert _raw(f, -1, 1, [0], [0], [0.0]) == -1
    x1, P1 = f._get(0)
    assert np.array_equal(x0, x1) and np.array_equal(P0, P1)
    # the prediction in the covariance buffer: PRE3_E_STATE
    f.set_x_p_k_km1(x0, P0)
    with pytest.raises(pre3.Pre3Error) as e:
        f.update(np.eye(3, f.n), None, np.zeros(3), np.zeros(3))
    assert e.value.code == -4
    with pytest.raises(pre3.Pre3Error) as e:
        f.ekf_heading_update(np.eye(3))
    assert e.value.code == -4
    f.close()


def test_indefinite_S_leaves_x_and_P_and_reports(pre3):
    """a row of zeros with R = 0: S is not positive definite.  The next reader returns PRE3_E_NUMERIC; a heading update that synchronises
    (applied_out) reports it once and clears it -- its gate returns here -- after which get_state shows x and P bit-unchanged"""
    f = _synth_filter(pre3, 100, dtype="f64")
    x0, P0 = f._get(0)
    H = np.zeros((2, f.n))
    H[0, 0] = 1.0
    f.update(H, np.zeros((2, 2)), np.zeros(2), np.zeros(2))
    assert f.rows_form() == 1
    with pytest.raises(pre3.Pre3Error) as e:
        f._get(0)
    assert e.value.code == -5
    with pytest.raises(pre3.Pre3Error) as e:
        f.pose()
    assert e.value.code == -5
    Rp = tw.q2R(x0[3:7]) @ axis_rot([1, 0, 0], 10.0)           # 10 degrees from h, h on the y axis: the intent gate returns
    with pytest.raises(pre3.Pre3Error) as e:
        f.ekf_heading_update(Rp, strict_reference=False)
    assert e.value.code == -5
    x1, P1 = f._get(0)
    assert np.array_equal(x0, x1) and np.array_equal(P0, P1)
    f.close()


# ---- the heading update ---------------------------------------------------------------------------------------------------------------------------
def _heading_case(f, Rp, strict, tol):
    x0, P0 = f._get(0)
    xt, Pt, at = heading_update(x0, P0, Rp, strict)
    applied = f.ekf_heading_update(Rp, strict)
    assert f.rows_form() == 1
    x, P = f._get(0)
    assert applied == at
    if not at:
        assert np.array_equal(x, x0) and np.array_equal(P, P0)
        return
    sc = np.abs(Pt).max()
    assert np.array_equal(P, P.T)
    assert np.abs(P - Pt).max() <= tol * sc, np.abs(P - Pt).max() / sc
    assert np.abs(x - xt).max() <= tol, np.abs(x - xt).max()
    assert np.abs(x[3:7] - x0[3:7]).max() > 0


@pytest.mark.parametrize("deg", [1.5, 3.0])
def test_heading_on_the_fixture_fp64_and_a_synthetic_map_fp32(pre3, sr4000, deg):
    d = sr4000
    f = pre3.EkfFilter(d["cam"], _types(d["N"]), dtype="f64", max_hyp=8, std_z=d["std_z"])
    for strict in (True, False):
        f.set_x_p_k_k(d["x_k_k"], d["p_k_k"])
        _heading_case(f, tw.q2R(d["x_k_k"][3:7]) @ axis_rot([1.0, 0.2, 0.4], deg), strict, 1e-10)
    f.close()
    f = _synth_filter(pre3, 500)
    x0, P0 = f._get(0)
    x0[3:7] = tw.qProd(x0[3:7], np.array([np.cos(0.1), 0.0, np.sin(0.1), 0.0]))[0]      # (not the identity)
    f.set_x_p_k_k(x0, P0)
    _heading_case(f, tw.q2R(x0[3:7]) @ axis_rot([0.3, 0.1, 1.0], deg), True, 2e-5)
    f.close()


def test_heading_near_aligned_on_fp32(pre3):
    """0.2 degrees: S's smallest eigenvalue is some 1e-5 of its largest; the fp64 small-rank algebra holds it on an fp32 context"""
    f = _synth_filter(pre3, 500)
    x0, _ = f._get(0)
    _heading_case(f, tw.q2R(x0[3:7]) @ axis_rot([1.0, 0.0, 0.5], 0.2), True, 2e-5)
    f.close()


def test_heading_gate_on_the_device(pre3):
    f = _synth_filter(pre3, 200, dtype="f64")
    x0, P0 = f._get(0)
    # the camera's y axis far from every world axis and the plane 10 degrees from it: both modes return
    qf = np.array([np.cos(0.4), np.sin(0.4) / np.sqrt(2), 0.0, np.sin(0.4) / np.sqrt(2)])
    x1 = x0.copy()
    x1[3:7] = qf
    Rp = tw.q2R(qf) @ axis_rot([1, 0, 0], 10.0)
    a = heading_angles(Rp[:, 1], heading_rows(qf)[0])
    assert (a > 4).all()
    for strict in (True, False):
        f.set_x_p_k_k(x1, P0)
        _heading_case(f, Rp, strict, 1e-10)
    # the camera's y axis on the world's y axis, the plane 6 degrees off: only the intent mode returns (quirk Q12)
    x2 = x0.copy()
    x2[3:7] = [1.0, 0.0, 0.0, 0.0]
    Rp = axis_rot([1, 0, 0], 6.0)
    f.set_x_p_k_k(x2, P0)
    _heading_case(f, Rp, False, 1e-10)
    f.set_x_p_k_k(x2, P0)
    _heading_case(f, Rp, True, 1e-10)
    f.close()


# ---- with the headline's options --------------------------------------------------------------------------------------------------------------------
def test_headline_chain_with_heading_updates_between_the_steps(pre3):
    N, N_HYP, WARM = 500, 200, 2
    thr = synth.HEADLINE["threshold"]
    seq = synth.make_sequence(N, WARM + 3, N_HYP, motion_noise=synth.HEADLINE["motion_noise"])
    types = _types(N)
    off = 13 + 6 * np.arange(N)
    x, P = seq["x0"], seq["P0"]
    for s in seq["steps"][:WARM]:
        ref = tw.step(types, off, seq["cam"], x, P, s["u"], s["meas_idx"], s["z"], s["hyp"], thr, early_exit=False)
        x, P = ref["x_kk"], ref["P_kk"]
    f = pre3.EkfFilter(seq["cam"], types, dtype="f32", max_hyp=N_HYP)
    f.defer_hi_update(True)
    assert f.pend_hi(True)
    f.set_x_p_k_k(x, P)
    for k, s in enumerate(seq["steps"][WARM:]):
        ref = tw.step(types, off, seq["cam"], x, P, s["u"], s["meas_idx"], s["z"], s["hyp"], thr, early_exit=False)
        st = f.step(s["u"], s["meas_idx"], s["z"], s["hyp"], threshold=thr, early_exit=False)
        r = ref["ransac"]
        assert (st["best"], st["max_support"], st["n_li"]) == (r["best"], r["max_support"], int(ref["li"].sum()))
        x, P = ref["x_kk"], ref["P_kk"]
        if k < 2:
            Rp = tw.q2R(x[3:7]) @ axis_rot([0.5, 0.2, 1.0], 1.5 + k)
            x, P, applied = heading_update(x, P, Rp, True)
            assert f.ekf_heading_update(Rp, True) == applied
    flags, xg, Pg = f.get_flags(), f.get_x_k_k(), f.get_p_k_k()
    f.close()
    assert np.array_equal(flags[0], ref["li"]) and np.array_equal(flags[1], ref["hi"])
    sc = np.abs(ref["P_kk"]).max()
    assert np.abs(Pg - ref["P_kk"]).max() < 1e-3 * sc, np.abs(Pg - ref["P_kk"]).max() / sc
    assert np.abs(xg - ref["x_kk"]).max() < 1e-4, np.abs(xg - ref["x_kk"]).max()
