"""GPU: a process noise the caller sets on a context (pre3_set_process_noise / pre3_get_process_noise).

A random SPD Pn on the four contexts tests/test_gpu_predict_pair.py uses (N = 0 fp64, N = 8 fp32, N = 41 fp32 and fp64): pre3_predict and the prediction
inside pre3_step_seeded (a step without measurements: update.m:50-55 changes nothing) against oracle/np_twin.py's predict with its process_noise
replaced by that Pn, within the tolerances that file uses against the oracle at equal u (X 1e-14, P 1e-13 / 2e-6 of max |P| -- here u is the same
array on both sides, so the 6 d / 352 d terms for a differing u are granted but not needed); get returns what was set; set(None) followed by a
prediction is byte-equal to a fresh context's and to the oracle's constant-noise prediction within the same tolerances (the parity route of
tests/test_gpu_synth.py); NaN, asymmetric and negative-diagonal inputs are refused with x, P and the setting unchanged; and one N = 120 fp32 case with
PRE3_OPT_DEFER_HI + PRE3_OPT_PEND_HI: setting the noise flushes nothing, the pending down-date is carried and the next step is the chain's."""
import importlib

import numpy as np
import pytest

from oracle import np_twin
from test_gpu_predict_pair import CONTEXTS, P_TOL, X_TOL, same_bytes, start_state

pytestmark = pytest.mark.gpu
synth = importlib.import_module("3pre_amd.synth")
E_ARG = -1
U = np.array([0.02, -0.015, 0.03, 0.9990482215818578, 0.025, -0.03, 0.015])
U[3:] /= np.linalg.norm(U[3:])


def random_spd(seed):
    """SPD with the constant's scale: sigmas of millimetres and of 1e-3 in q, and full correlations"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((7, 7))
    S = A @ A.T / 7 + 0.5 * np.eye(7)
    d = np.r_[np.full(3, 4e-3), np.full(4, 1.5e-3)]
    Pn = d[:, None] * S * d[None, :]
    return (Pn + Pn.T) / 2


PN = random_spd(31)


@pytest.fixture(scope="module")
def contexts(pre3):
    cache = {}

    def get(kind):
        if kind not in cache:
            N, dtype = CONTEXTS[kind]
            x0, P0 = start_state(N)
            fa, fb = (pre3.EkfFilter(synth.CAM, np.zeros(N, np.int32), dtype=dtype, max_hyp=8) for _ in range(2))
            fa.set_x_p_k_k(x0, P0)
            xr, Pr = fa._get(0)
            cache[kind] = dict(fa=fa, fb=fb, x0=xr, P0=Pr, dtype=dtype)
        return cache[kind]

    yield get
    for d in cache.values():
        d["fa"].close(); d["fb"].close()


@pytest.mark.parametrize("kind", sorted(CONTEXTS))
def test_a_set_noise_is_the_predictions_noise(pre3, contexts, kind, monkeypatch):
    k = contexts(kind)
    fa, fb, x0, P0 = k["fa"], k["fb"], k["x0"], k["P0"]
    fresh_Pn, src = fb.process_noise
    assert src == "constant" and np.abs(fresh_Pn - np_twin.process_noise()).max() < 1e-20
    # the constant-noise prediction of an untouched context: the reference for "back to the constant", and itself against the twin
    fb.set_x_p_k_k(x0, P0); fb.ekf_prediction(U)
    xc, Pc = fb._get(1)
    xt, Pt = np_twin.predict(x0, P0, U)
    assert np.abs(xc - xt).max() < X_TOL and np.abs(Pc - Pt).max() < P_TOL[k["dtype"]] * np.abs(Pt).max()
    # set, get, predict
    fa.set_process_noise(PN)
    got, src = fa.process_noise
    assert src == "caller" and same_bytes(got, PN)
    fa.set_x_p_k_k(x0, P0)                                  # (does not reset the setting)
    assert fa.process_noise[1] == "caller"
    fa.ekf_prediction(U)
    xa, Pa = fa._get(1)
    monkeypatch.setattr(np_twin, "process_noise", lambda: PN.copy())
    xr, Pr = np_twin.predict(x0, P0, U)
    ex, eP = np.abs(xa - xr).max(), np.abs(Pa - Pr).max() / np.abs(Pr).max()
    print(kind, "predict: x err %.3g  P err %.3g of max |P|" % (ex, eP))
    assert ex < X_TOL and eP < P_TOL[k["dtype"]]
    assert not same_bytes(Pa[:7, :7], Pc[:7, :7]) and same_bytes(Pa[7:, 7:], Pc[7:, 7:]) and same_bytes(Pa[:7, 7:], Pc[:7, 7:])      # Q enters the pose block only
    # the prediction inside a step: no measurements, so the step is its prediction
    fa.set_x_p_k_k(x0, P0)
    fa.step_seeded(U, np.zeros(0, np.int32), np.zeros((0, 2)), 9, 0, 1)
    xs, Ps = fa._get(0)
    ex, eP = np.abs(xs - xr).max(), np.abs(Ps - Pr).max() / np.abs(Pr).max()
    print(kind, "step_seeded: x err %.3g  P err %.3g of max |P|" % (ex, eP))
    assert ex < X_TOL and eP < P_TOL[k["dtype"]]
    # back to the constant: byte-equal to the context nothing was ever set on
    fa.set_process_noise(None)
    got, src = fa.process_noise
    assert src == "constant" and same_bytes(got, fresh_Pn)
    fa.set_x_p_k_k(x0, P0); fa.ekf_prediction(U)
    xb, Pb = fa._get(1)
    assert same_bytes(xb, xc) and same_bytes(Pb, Pc)


def test_bad_noise_is_refused_with_everything_unchanged(pre3, contexts):
    k = contexts("n8_f32")
    fa, x0, P0 = k["fa"], k["x0"], k["P0"]
    fa.set_process_noise(PN)
    fa.set_x_p_k_k(x0, P0)
    nan, asym, neg = PN.copy(), PN.copy(), PN.copy()
    nan[2, 5] = nan[5, 2] = np.nan
    asym[1, 4] = np.nextafter(asym[1, 4], 1.0)
    neg[6, 6] = -neg[6, 6]
    inf = PN.copy(); inf[0, 0] = np.inf
    for bad in (nan, asym, neg, inf):
        with pytest.raises(pre3.Pre3Error) as e:
            fa.set_process_noise(bad)
        assert e.value.code == E_ARG
        got, src = fa.process_noise
        assert src == "caller" and same_bytes(got, PN)
    xk, Pk = fa._get(0)
    assert same_bytes(xk, x0) and same_bytes(Pk, P0)
    zero_diag = PN.copy(); zero_diag[:, 3] = 0; zero_diag[3, :] = 0          # a zero diagonal entry is not negative: accepted
    fa.set_process_noise(zero_diag)
    assert same_bytes(fa.process_noise[0], zero_diag)
    fa.set_process_noise(None)
    # refused on a context nothing was set on: still the constant
    with pytest.raises(pre3.Pre3Error):
        fa.set_process_noise(nan)
    assert fa.process_noise[1] == "constant"


def test_pending_work_is_carried_under_a_set_noise(pre3):
    """fp32, PRE3_OPT_DEFER_HI + PRE3_OPT_PEND_HI (the N = 120 set-up of tests/test_gpu_pend_hi.py): step 0 leaves a HI update deferred and its down-date
    pending.  One context has the noise set before the step, the other between the step and the prediction -- the call flushes nothing, so both carry
    the same pending rows through the same prediction -- and a third predicts with the constant: P differs from it."""
    N, n_hyp = 120, 60
    seq = synth.make_sequence(N, 2, n_hyp, seed=77, motion_noise=2.5)
    s0, s1 = seq["steps"]
    filt = []
    for _ in range(3):
        f = pre3.EkfFilter(seq["cam"], np.zeros(N, np.int32), dtype="f32", max_hyp=n_hyp, std_z=1.0)
        f.defer_hi_update(True)
        assert f.pend_hi(True)
        filt.append(f)
    fa, fb, fc = filt

    def front(f, when):
        if when == "before":
            f.set_process_noise(PN)
        f.set_x_p_k_k(seq["x0"], seq["P0"])
        st = f.step(s0["u"], s0["meas_idx"], s0["z"], s0["hyp"], threshold=1.0, early_exit=False)
        if when == "between":
            f.set_process_noise(PN)
        f.ekf_prediction(s1["u"])
        return st

    # step 0 itself predicts with the noise in force: "between" runs it with the constant, so the two are compared from the prediction on a common
    # start -- set the noise before step 0 on both, once more between on one of them
    sa = front(fa, "before")
    fb.set_process_noise(PN)
    sb = front(fb, "between")
    sc = front(fc, "never")
    assert sa == sb
    (xa, Pa), (xb, Pb), (xc, Pc) = fa._get(1), fb._get(1), fc._get(1)
    assert same_bytes(xa, xb) and same_bytes(Pa, Pb) and np.isfinite(Pa).all()
    assert not same_bytes(Pa, Pc)
    front(fa, "before"); front(fb, "between")
    out = []
    for f in (fa, fb):
        f.search_IC_matches(); f.set_measurements(s1["meas_idx"], s1["z"])
        st = f.step_predicted(s1["hyp"], threshold=1.0, early_exit=False)
        li, hi = f.get_flags()
        out.append((st, li.copy(), hi.copy(), f.get_x_k_k(), f.get_p_k_k()))
    (sta_, lia, hia, xa, Pa), (stb, lib_, hib, xb, Pb) = out
    print("next step:", sta_)
    assert sta_["n_hi"] > 0                                     # the deferred HI update of step 0 was pending when the noise was set
    assert sta_ == stb and np.array_equal(lia, lib_) and np.array_equal(hia, hib)
    assert same_bytes(xa, xb) and same_bytes(Pa, Pb)
    assert fa.process_noise[1] == "caller"
    for f in filt:
        f.close()
