"""PRE3_OPT_PEND_HI against the numpy twin (fp64), one step at a time -- the form bench.py's headline times.  Under PEND_HI the HI update's down-date
P - W~'W~ is not launched; the next step carries it (k_predict transforms W~, k_ell_HP_build_mb subtracts (H W~')W~, the persistent launch's consumers
take W~ as the panels in front of panel 0, k_hi_fused updates x as x + W~'(L^-1 nu)).  tests/test_gpu_pend_hi.py compares that form with the default
GPU form at 3e-4 of P's scale; the LI update's own fp32 noise (about 1e-4 of the scale) hides errors of the carried terms there.

What is observed between steps must not send the trajectory down the flush path: EkfFilter.marginal() applies the pending rows inside its own launch and
leaves them pending (tests/test_gpu_marginals.py), step()'s statistics are exact (best, max_support, n_li; with the HI update deferred, n_hi is the
previous step's).  get_flags / get_x_k_k / get_p_k_k / landmark_fields run only after the last step."""
import functools
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
synth = importlib.import_module("3pre_amd.synth")
N, N_HYP = 500, 200
THR = synth.HEADLINE["threshold"]
MOTION = synth.HEADLINE["motion_noise"]


def _table(types):
    types = np.asarray(types, np.int32)
    dims = np.where(types == 0, 6, 3)
    return types, 13 + np.concatenate([[0], np.cumsum(dims)[:-1]]).astype(int)


def _filter(pre3, cam, types, x, P):
    f = pre3.EkfFilter(cam, np.asarray(types, np.int32), dtype="f32", max_hyp=N_HYP, std_z=1.0)
    f.defer_hi_update(True)                                  # as bench.py runs the headline
    assert f.pend_hi(True)
    f.set_x_p_k_k(x, P)
    return f


def _read(f):
    return f.marginal(np.arange(f.n))                        # (leaves the pending down-date pending)


def _step(f, s, u=None, z=None):
    return f.step(s["u"] if u is None else u, s["meas_idx"], s["z"] if z is None else z, s["hyp"], threshold=THR, early_exit=False)


def _same_stats(st, ref, n_hi_before):
    r = ref["ransac"]
    assert (st["best"], st["max_support"], st["n_li"]) == (r["best"], r["max_support"], int(ref["li"].sum()))
    if n_hi_before is not None:
        assert st["n_hi"] == n_hi_before                      # (deferred: the previous step's count)


def _one_update(xg, Pg, ref, what):
    """the tolerances of one fp32 step at N = 500 (tests/test_gpu_fullsize.py)"""
    sc = np.abs(ref["P_kk"]).max()
    assert np.isfinite(Pg).all(), what
    assert np.abs(Pg - ref["P_kk"]).max() < 3e-4 * sc, (what, np.abs(Pg - ref["P_kk"]).max() / sc)
    assert np.abs(xg - ref["x_kk"]).max() < 2e-5, (what, np.abs(xg - ref["x_kk"]).max())


def _cov_rel(A, B, Pd):
    """max over (i, j) of |A - B|_ij / sqrt(Pd_ii Pd_jj), over the states whose variance in Pd is not negligible: the Jnorm pass leaves the
    quaternion's own direction with a variance some 1e-8 of the largest (update.m:42-46)"""
    d = np.diag(Pd)
    ok = d > 1e-6 * d.max()
    return (np.abs(A - B)[np.ix_(ok, ok)] / np.sqrt(np.outer(d[ok], d[ok]))).max()


# ---- 1. the headline chain ------------------------------------------------------------------------------------------------------------------------
WARM, STEPS = 2, 4


def _headline_chain(pre3, observe):
    """bench.py's headline sequence: WARM steps on the twin only, then STEPS chained GPU steps.  observe = False: the twin chained on its own state,
    the final state compared; observe = True: the state read with marginal() after every step, the twin stepped once from it"""
    from oracle import np_twin as tw
    seq = synth.make_sequence(N, WARM + STEPS, N_HYP, motion_noise=MOTION)
    types, off = _table(np.zeros(N))
    x, P = seq["x0"], seq["P0"]
    for s in seq["steps"][:WARM]:
        ref = tw.step(types, off, seq["cam"], x, P, s["u"], s["meas_idx"], s["z"], s["hyp"], THR, early_exit=False)
        x, P = ref["x_kk"], ref["P_kk"]
    f = _filter(pre3, seq["cam"], types, x, P)
    n_hi, rescued = None, []
    for k, s in enumerate(seq["steps"][WARM:]):
        ref = tw.step(types, off, seq["cam"], x, P, s["u"], s["meas_idx"], s["z"], s["hyp"], THR, early_exit=False)
        st = _step(f, s)
        _same_stats(st, ref, n_hi)
        n_hi = int(ref["hi"].sum())
        rescued.append(n_hi)
        if observe:
            x, P = _read(f)
            _one_update(x, P, ref, ("step", k))
        else:
            x, P = ref["x_kk"], ref["P_kk"]
    out = dict(flags=f.get_flags(), x=f.get_x_k_k(), P=f.get_p_k_k(), ref=ref, rescued=rescued)
    f.close()
    return out


def test_headline_chain_with_the_pending_downdate_matches_the_twin(pre3):
    a = _headline_chain(pre3, observe=False)
    assert min(a["rescued"]) > 0 and min(a["rescued"]) <= 32 < max(a["rescued"]), a["rescued"]      # one and two pending panels both occur
    ref = a["ref"]
    assert np.array_equal(a["flags"][0], ref["li"]) and np.array_equal(a["flags"][1], ref["hi"])
    sc = np.abs(ref["P_kk"]).max()
    assert np.abs(a["P"] - ref["P_kk"]).max() < 1e-3 * sc, np.abs(a["P"] - ref["P_kk"]).max() / sc      # STEPS accumulated fp32 updates
    assert np.abs(a["x"] - ref["x_kk"]).max() < 1e-4, np.abs(a["x"] - ref["x_kk"]).max()
    b = _headline_chain(pre3, observe=True)
    assert b["rescued"] == a["rescued"]
    assert np.array_equal(b["x"], a["x"]) and np.array_equal(b["P"], a["P"])      # the reads between the steps did not change the trajectory
    assert all(np.array_equal(u, v) for u, v in zip(a["flags"], b["flags"]))


# ---- 2. the rescued-landmark sweep ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _step0(n_hi, mixed=False):
    """step 0 of the N = 500 headline-noise sequence from its prior, with exactly n_hi rescued landmarks (tests/test_gpu_tail.py); mixed: every third
    landmark converted to Cartesian first (tests/test_gpu_hi_fused.py)"""
    from oracle import np_twin as tw
    from test_gpu_tail import _with_n_rescued
    from test_gpu_hi_fused import _convert
    seq = synth.make_sequence(N, 2, N_HYP, motion_noise=MOTION)
    types = np.zeros(N, np.int32)
    x0, P0 = seq["x0"], seq["P0"]
    if mixed:
        types[::3] = 1
        x0, P0 = _convert(tw, x0, P0, types)
    types, off = _table(types)
    z0, ref0 = _with_n_rescued(tw, types, off, seq, seq["steps"][0], n_hi, x0=x0, P0=P0)
    return seq, types, off, x0, P0, z0, ref0


@pytest.mark.parametrize("n_hi", [1, 18, 32, 33, 48, 64])
def test_rescued_landmarks_left_pending_and_carried_match_the_twin(pre3, n_hi):
    """step 0 rescues n_hi landmarks (1 .. 32: one pending panel, 33 .. 64: two) and leaves its down-date pending; step 1 carries it.  Both
    against the twin, step 1 from the state marginal() shows after step 0"""
    from oracle import np_twin as tw
    seq, types, off, x0, P0, z0, ref0 = _step0(n_hi)
    s0, s1 = seq["steps"]
    f = _filter(pre3, seq["cam"], types, x0, P0)
    _same_stats(_step(f, s0, z=z0), ref0, None)
    x, P = _read(f)
    _one_update(x, P, ref0, "step 0")
    ref1 = tw.step(types, off, seq["cam"], x, P, s1["u"], s1["meas_idx"], s1["z"], s1["hyp"], THR, early_exit=False)
    _same_stats(_step(f, s1), ref1, n_hi)
    x, P = _read(f)
    _one_update(x, P, ref1, "step 1")
    li, hi = f.get_flags()
    f.close()
    assert np.array_equal(li, ref1["li"]) and np.array_equal(hi, ref1["hi"])


# ---- 3. the quiet carry step ----------------------------------------------------------------------------------------------------------------------
def _rotation(deg, axis):
    a, v = np.radians(deg) / 2, np.asarray(axis, float)
    return np.concatenate([[np.cos(a)], np.sin(a) * v / np.linalg.norm(v)])


QUIET_ROT = _rotation(2.0, [0.3, 1.0, 0.2])


@pytest.mark.parametrize("mixed", [False, True], ids=["invdepth", "mixed"])
@pytest.mark.parametrize("n_hi", [1, 32, 33, 64])
def test_quiet_step_carries_the_pending_downdate_through_the_prediction(pre3, n_hi, mixed):
    """step k rescues n_hi landmarks; step k+1 turns the camera by 2 degrees and has every measurement 300 px off.  Its HI set is empty, and its LI
    set holds only what compute_hypothesis_support_fast.m:33-110 counts for any hypothesis -- the inverse-depth measurements within the threshold of
    the smallest residual (one or two landmarks here).  P_{k+1|k+1} is then the prediction of P - W~'W~ (Qq1 and Jn on W~'s columns 3..6) behind
    that small update, and S_i is H (P - W~'W~) H' + I at the prediction: both against the twin from the state marginal() shows after step k,
    P relative to the predicted standard deviations, where the LI update's noise does not hide the carried terms.

    Measured on MI355X over the eight cases: e_P (max |dP_ij| / sqrt(P_ii P_jj), P_ii from the twin's P_{k+1|k}) <= 1.6e-5 on the inverse-depth map,
    <= 1.5e-6 on the mixed one; the 13 x 13 camera block <= 3.5e-7 of its largest entry; S_i <= 8.6e-9 of its norm; x <= 3.1e-6.  Computed with the
    twin on the same steps, k_predict leaving W~ untransformed (P_{k+1|k} wrong by F D F' - D, D the HI down-date) moves e_P by 2.4e-4 (one rescued
    landmark, mixed map) to 26, the camera block by 7.4e-6 to 0.83, S_i by 4.8e-5 to 7.0e-4.  The tolerances sit between the two."""
    from oracle import np_twin as tw
    seq, types, off, x0, P0, z0, ref0 = _step0(n_hi, mixed)
    s0, s1 = seq["steps"]
    u = np.array(s1["u"], float)
    u[3:7] = QUIET_ROT
    z1 = np.array(s1["z"], float) + 300.0
    f = _filter(pre3, seq["cam"], types, x0, P0)
    _same_stats(_step(f, s0, z=z0), ref0, None)
    x, P = _read(f)
    ref = tw.step(types, off, seq["cam"], x, P, u, s1["meas_idx"], z1, s1["hyp"], THR, early_exit=False)
    assert int(ref["hi"].sum()) == 0 and int(ref["li"].sum()) <= 2
    _same_stats(_step(f, s1, u=u, z=z1), ref, n_hi)
    xg, Pg = f.get_x_k_k(), f.get_p_k_k()
    S = f.landmark_fields()["S"]
    li, hi = f.get_flags()
    f.close()
    assert np.array_equal(li, ref["li"]) and np.array_equal(hi, ref["hi"])
    e_P = _cov_rel(Pg, ref["P_kk"], ref["P_km1"])
    cam = np.s_[:13, :13]
    e_cam = np.abs(Pg[cam] - ref["P_kk"][cam]).max() / np.abs(ref["P_kk"][cam]).max()
    vis = np.nonzero(np.abs(ref["S"]).max(axis=(1, 2)) > 0)[0]
    e_S = (np.abs(S[vis] - ref["S"][vis]).max(axis=(1, 2)) / np.linalg.norm(ref["S"][vis], axis=(1, 2))).max()
    e_x = np.abs(xg - ref["x_kk"]).max()
    assert e_P < 5e-5, e_P                                 # measured <= 1.6e-5; M1: >= 2.4e-4
    assert e_cam < 1.5e-6, e_cam                           # measured <= 3.5e-7; M1: >= 7.4e-6
    assert e_S < 1e-7, e_S                                 # measured <= 8.6e-9; M1: >= 4.8e-5
    assert e_x < 2e-5, e_x                                 # measured <= 3.1e-6 (one update's tolerance)
