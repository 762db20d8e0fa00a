"""GPU: pre3_predict_cv -- the prediction with the camera-only motion models, one launch (k_predict_cv) -- against the numpy
restatement tests/cv_model_ref.py.  Sizes: N in {0, 1, 41, 85} inverse-depth landmarks (n = 13: the corner only; 19: one partial block; 259: just
past one block of 256 columns; 523: three blocks) and a mixed inverse-depth / Cartesian map, every context with max_landmarks > N so that ld != n.

Tolerances of the parity tests are those tests/test_gpu_synth.py::test_predict_parity grants the existing prediction: |dx| < 1e-14, |dP| < 1e-13 (fp64)
and 2e-6 (fp32) of max |P|."""
import importlib

import numpy as np
import pytest

import cv_model_ref as cvm
from test_oracle import _mixed_problem

pytestmark = pytest.mark.gpu
synth = importlib.import_module("3pre_amd.synth")

DT, SIGMA_A, SIGMA_ALPHA = 0.1, 0.007, 0.007          # predict_state_and_covariance.m:35; mono_slam.m:76-85
TOL_X, TOL_P = 1e-14, {"f64": 1e-13, "f32": 2e-6}
CASES = [("id", 0), ("id", 1), ("id", 41), ("id", 85), ("mixed", 30)]
VIEW_POSE = np.array([0.01, -0.02, 0.015, 0.999, 0.02, -0.01, 0.015, 0.05, -0.03, 0.04, 0.02, -0.015, 0.025])                   # at the map's origin, looking along it
POSE = np.array([0.4, -0.7, 1.3, 0.93, 0.21, -0.17, 0.24, 0.4, -0.3, 0.25, 0.31, -0.22, 0.41])     # q, v and omega well away from 0


def _problem(kind, N, pose=POSE):
    if kind == "mixed":
        types, x, P, cam = _mixed_problem(seed=4, N=N)
    elif N == 0:
        rng = np.random.default_rng(8)
        A = rng.standard_normal((13, 13)) * 0.01
        types, x, P, cam = np.zeros(0, np.int32), np.zeros(13), A @ A.T + 1e-6 * np.eye(13), synth.CAM.copy()
    else:
        x, P, _ = synth.make_map(N, seed=50 + N)
        types, cam = np.zeros(N, np.int32), synth.CAM.copy()
    x = x.copy()
    x[0:13] = pose
    x[3:7] /= np.linalg.norm(x[3:7])
    return types, x, P, cam


@pytest.fixture(scope="module")
def problems():
    """every (kind, N) problem once, shared and left unchanged"""
    out = {}
    for kind, N in CASES:
        types, x, P, cam = _problem(kind, N)
        for a in (types, x, P, cam):
            a.setflags(write=False)
        out[(kind, N)] = (types, x, P, cam)
    return out


def _filter(pre3, types, cam, dtype, **kw):
    return pre3.EkfFilter(cam, types, dtype=dtype, max_hyp=kw.pop("max_hyp", 8), max_landmarks=len(types) + 3, std_z=1.0, **kw)


def _assert_parity(xg, Pg, xr, Pr, dtype, what=""):
    ex, eP = np.abs(xg - xr).max(), np.abs(Pg - Pr).max() / np.abs(Pr).max()
    print("%s %s: |dx| = %.3g, |dP| / max|P| = %.3g" % (what, dtype, ex, eP))
    assert np.isfinite(xg).all() and np.isfinite(Pg).all()
    assert ex < TOL_X
    assert eP < TOL_P[dtype]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("kind,N", CASES, ids=["%s%d" % c for c in CASES])
def test_parity_and_what_must_not_move(pre3, problems, kind, N, dtype):
    """(1) all four types against the restatement; (2) x[13:] and P[13:, 13:] byte-equal to what the context held, the returned P exactly symmetric"""
    types, x, P, cam = problems[(kind, N)]
    f = _filter(pre3, types, cam, dtype)
    for type in range(4):
        f.set_x_p_k_k(x, P)
        x0, P0 = f.get_x_k_k(), f.get_p_k_k()                       # in the context's dtype
        if dtype == "f64":
            assert np.array_equal(x0, x) and np.array_equal(P0, P)
        f.ekf_prediction_cv(DT, SIGMA_A, SIGMA_ALPHA, type=cvm.TYPES[type])
        xg, Pg = f.get_x_k_km1(), f.get_p_k_km1()
        xr, Pr = cvm.predict(x0, P0, DT, SIGMA_A, SIGMA_ALPHA, type)
        _assert_parity(xg, Pg, xr, Pr, dtype, "%s N=%d type %d" % (kind, N, type))
        assert xg[13:].tobytes() == x0[13:].tobytes()
        assert Pg[13:, 13:].tobytes() == P0[13:, 13:].tobytes()
        assert np.array_equal(Pg, Pg.T)
    f.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_omega_zero_and_the_state_the_forks_prediction_leaves(pre3, problems, dtype):
    """(3) omega = 0 exactly: finite, and the restatement's limit form within the parity tolerances -- set by hand for all four types, and as pre3_predict
    leaves it (x[7:13] = exact zeros) for type 0"""
    types, x, P, cam = problems[("id", 41)]
    f = _filter(pre3, types, cam, dtype)
    xz = x.copy()
    xz[10:13] = 0.0
    for type in range(4):
        f.set_x_p_k_k(xz, P)
        P0 = f.get_p_k_k()
        f.ekf_prediction_cv(DT, SIGMA_A, SIGMA_ALPHA, type=type)
        xr, Pr = cvm.predict(xz, P0, DT, SIGMA_A, SIGMA_ALPHA, type)
        _assert_parity(f.get_x_k_km1(), f.get_p_k_km1(), xr, Pr, dtype, "omega = 0, type %d" % type)
    f.set_x_p_k_k(x, P)
    f.ekf_prediction(np.array([0.01, -0.02, 0.015, 0.9999, 0.004, -0.003, 0.002]))
    x1, P1 = f.get_x_k_km1(), f.get_p_k_km1()
    assert np.array_equal(x1[7:13], np.zeros(6))
    f.set_x_p_k_k(x1, P1)
    f.ekf_prediction_cv(DT, SIGMA_A, SIGMA_ALPHA)
    xr, Pr = cvm.predict(x1, P1, DT, SIGMA_A, SIGMA_ALPHA, cvm.CV)
    _assert_parity(f.get_x_k_km1(), f.get_p_k_km1(), xr, Pr, dtype, "behind pre3_predict")
    f.close()


@pytest.mark.parametrize("dtype,pend", [("f64", False), ("f32", False), ("f32", True)], ids=["f64", "f32", "f32-defer-pend"])
def test_the_pending_pass_runs_in_front(pre3, dtype, pend):
    """(4) one step (N = 40), then predict_cv: whatever the step left deferred or pending -- the HI update, its down-date, the update.m:42-46 pass --
    belongs in front of the prediction.  Against a second context that ran the same step, then get_state, then the restatement.  (A pass that landed
    behind the prediction would rescale rows / columns 3..6 by the update's 1 / |q| once more and project them along the wrong quaternion: small
    against max |P|, so it is the fp64 case that decides.)"""
    N = 40
    seq = synth.make_sequence(N, 1, 16, seed=77, sigma_z=0.6)
    types, s = np.zeros(N, np.int32), seq["steps"][0]
    out = []
    for predict in (True, False):
        f = _filter(pre3, types, seq["cam"], dtype, max_hyp=16)
        if pend:
            f.defer_hi_update(True)
            assert f.pend_hi(True)
        f.set_x_p_k_k(seq["x0"], seq["P0"])
        f.step(s["u"], s["meas_idx"], s["z"], s["hyp"], threshold=1.0, early_exit=True)
        if predict:
            f.ekf_prediction_cv(DT, SIGMA_A, SIGMA_ALPHA)
            out.append((f.get_x_k_km1(), f.get_p_k_km1()))
        else:
            out.append((f.get_x_k_k(), f.get_p_k_k()))
        f.close()
    (xg, Pg), (xk, Pk) = out
    xr, Pr = cvm.predict(xk, Pk, DT, SIGMA_A, SIGMA_ALPHA, cvm.CV)
    _assert_parity(xg, Pg, xr, Pr, dtype, "behind a step")


def test_v_and_omega_live(pre3):
    """(5) behind an update, type 0 carries x_k_k[7:13] into x_k_km1[7:13] byte for byte, and they are not zero"""
    types, x, P, cam = _problem("id", 41, pose=VIEW_POSE)          # a pose that sees the map
    f = _filter(pre3, types, cam, "f64")
    f.set_x_p_k_km1(x, P)
    f.search_IC_matches()
    fld = f.landmark_fields()
    vis = np.nonzero(fld["has_h"])[0].astype(np.int32)
    assert len(vis) >= 8
    rng = np.random.default_rng(3)
    f.set_measurements(vis, fld["h"][vis] + rng.normal(0, 0.4, (len(vis), 2)))
    f.ekf_update_all()
    xk = f.get_x_k_k()
    assert not np.array_equal(xk[7:13], x[7:13])                   # the update moved them
    f.ekf_prediction_cv(DT, SIGMA_A, SIGMA_ALPHA, type="constant_velocity")
    x1 = f.get_x_k_km1()
    assert x1[7:13].tobytes() == xk[7:13].tobytes() and np.all(x1[7:13] != 0)
    f.close()


# ---- (6) three chained frames of predict_cv -> search_IC_matches -> set_measurements -> step_predicted against step_cv
CHAIN_N, CHAIN_HYP, CHAIN_SEED = 40, 24, 0
GATE = 5.9915


def chain_sequence(seed, N=CHAIN_N, frames=3, n_hyp=CHAIN_HYP):
    """a truth that moves at constant velocity, its pixels with noise and outliers, and the RANSAC draws"""
    x0, P0, x_true = synth.make_map(N, seed=seed)
    rng = np.random.default_rng(seed + 7)
    v, om = np.array([0.05, -0.03, 0.04]), np.array([0.02, -0.015, 0.025])
    x0 = x0.copy()
    x0[7:10], x0[10:13] = v + rng.normal(0, 0.003, 3), om + rng.normal(0, 0.003, 3)
    pose, Y = x_true[0:7].copy(), x_true[13:].reshape(N, 6)
    steps = []
    for _ in range(frames):
        pose[0:3] = pose[0:3] + v * DT
        pose[3:7] = cvm.qprod(pose[3:7], cvm.v2q(om * DT))
        pose[3:7] /= np.linalg.norm(pose[3:7])
        uv, vis = synth.pixels(pose, Y)
        cand = np.nonzero(vis)[0]
        pick = np.sort(rng.choice(cand, size=min(int(0.8 * N), len(cand)), replace=False)).astype(np.int32)
        z = uv[pick] + rng.normal(0, 0.5, (len(pick), 2))
        out_pos = rng.choice(len(pick), size=len(pick) // 5, replace=False)
        z[out_pos] = np.stack([rng.uniform(1, 175, len(out_pos)), rng.uniform(1, 143, len(out_pos))], 1)
        steps.append(dict(meas_idx=pick, z=z, hyp=synth.draw_hypotheses(rng, len(pick), n_hyp)))
    return dict(x0=x0, P0=P0, steps=steps, cam=synth.CAM.copy())


def chain_reference(seq, N=CHAIN_N):
    """step_cv over the frames from its own state, and how far each frame is from a decision that rounding could turn: the number of evaluated
    hypotheses that share the best support, and the distance of the nearest rescue chi2 from the gate"""
    types, off = np.zeros(N, np.int32), 13 + 6 * np.arange(N)
    x, P, refs = seq["x0"], seq["P0"], []
    for s in seq["steps"]:
        r = cvm.step_cv(types, off, seq["cam"], x, P, DT, SIGMA_A, SIGMA_ALPHA, s["meas_idx"], s["z"], s["hyp"], 1.0, early_exit=True)
        sup = r["ransac"]["support"]
        r["n_best"] = int((sup == r["ransac"]["max_support"]).sum())
        r["gate_margin"] = float(np.abs(r["gate_d2"] - GATE).min()) if len(r["gate_d2"]) else np.inf
        refs.append(r)
        x, P = r["x_kk"], r["P_kk"]
    return refs


def test_three_chained_frames_against_step_cv(pre3):
    """fp64, N = 40, each side from its own state: LI set, HI set and RANSAC winner exact, x and P within what the fp64 chained tests of
    tests/test_gpu_synth.py grant (1e-10, 1e-11 of max |P|).  The seed was chosen on the CPU so that the restatement alone has no support tie and no
    chi2 within 1e-6 of the gate; that is asserted here."""
    seq = chain_sequence(CHAIN_SEED)
    refs = chain_reference(seq)
    for r in refs:
        assert r["n_best"] == 1, "support tie in the restatement"
        assert r["gate_margin"] > 1e-6, "a chi2 value within 1e-6 of the gate in the restatement"
    assert sum(int(r["hi"].sum()) for r in refs) > 0 and all(int(r["li"].sum()) > 8 for r in refs)
    f = _filter(pre3, np.zeros(CHAIN_N, np.int32), seq["cam"], "f64", max_hyp=CHAIN_HYP)
    f.set_x_p_k_k(seq["x0"], seq["P0"])
    for k, (s, ref) in enumerate(zip(seq["steps"], refs)):
        f.ekf_prediction_cv(DT, SIGMA_A, SIGMA_ALPHA)
        f.search_IC_matches()
        f.set_measurements(s["meas_idx"], s["z"])
        st = f.step_predicted(s["hyp"], threshold=1.0, early_exit=True)
        li, hi = f.get_flags()
        assert np.array_equal(li, ref["li"]), "frame %d: LI set differs" % k
        assert np.array_equal(hi, ref["hi"]), "frame %d: HI set differs" % k
        r = ref["ransac"]
        assert (st["best"], st["iters"], st["n_hyp"], st["max_support"]) == (r["best"], r["iters"], r["n_hyp"], r["max_support"])
        xg, Pg = f.get_x_k_k(), f.get_p_k_k()
        ex, eP = np.abs(xg - ref["x_kk"]).max(), np.abs(Pg - ref["P_kk"]).max() / np.abs(ref["P_kk"]).max()
        print("frame %d: |dx| = %.3g, |dP| / max|P| = %.3g, v = %s, omega = %s" % (k, ex, eP, xg[7:10], xg[10:13]))
        assert ex < 1e-10 and eP < 1e-11
        assert np.all(xg[7:13] != 0)
    f.close()


# ---- (7) refusals
def _state_of(f, Pre3Error):
    """x, P and the flags as a caller can see them: each estimate, or the error code that says it is not there"""
    out = []
    for get in (f.get_x_k_k, f.get_p_k_k, f.get_x_k_km1, f.get_p_k_km1):
        try:
            out.append(get().tobytes())
        except Pre3Error as e:
            out.append(e.code)
    return out


BAD_ARGS = [(DT, SIGMA_A, SIGMA_ALPHA, -1), (DT, SIGMA_A, SIGMA_ALPHA, 4), (0.0, SIGMA_A, SIGMA_ALPHA, 0), (-0.1, SIGMA_A, SIGMA_ALPHA, 0),
            (np.inf, SIGMA_A, SIGMA_ALPHA, 0), (np.nan, SIGMA_A, SIGMA_ALPHA, 0), (DT, -1e-3, SIGMA_ALPHA, 0), (DT, np.nan, SIGMA_ALPHA, 0),
            (DT, np.inf, SIGMA_ALPHA, 0), (DT, SIGMA_A, -1e-3, 0), (DT, SIGMA_A, np.nan, 0), (DT, SIGMA_A, np.inf, 0)]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_refusals_leave_the_context_as_it_was(pre3, problems, dtype):
    types, x, P, cam = problems[("id", 1)]
    f = _filter(pre3, types, cam, dtype)
    f.set_x_p_k_k(x, P)
    before = _state_of(f, pre3.Pre3Error)
    assert before[2] == -4 and before[3] == -4                      # no predicted estimate yet
    for dt, sa, sal, type in BAD_ARGS:
        with pytest.raises(pre3.Pre3Error) as e:
            f.ekf_prediction_cv(dt, sa, sal, type=type)
        assert e.value.code == -1, (dt, sa, sal, type)
        assert _state_of(f, pre3.Pre3Error) == before
    with pytest.raises(pre3.Pre3Error) as e:
        f.ekf_prediction_cv(DT, SIGMA_A, SIGMA_ALPHA, type="constant_position_and_orientation_location_noise")      # not built
    assert e.value.code == -1 and _state_of(f, pre3.Pre3Error) == before
    # without (x_k_k, p_k_k): PRE3_E_STATE, on a context that holds the predicted estimate only
    f.set_x_p_k_km1(x, P)
    before = _state_of(f, pre3.Pre3Error)
    assert before[1] == -4
    with pytest.raises(pre3.Pre3Error) as e:
        f.ekf_prediction_cv(DT, SIGMA_A, SIGMA_ALPHA)
    assert e.value.code == -4 and _state_of(f, pre3.Pre3Error) == before
    # and a sigma of zero is not an error
    f.set_x_p_k_k(x, P)
    f.ekf_prediction_cv(DT, 0.0, 0.0)
    assert np.isfinite(f.get_p_k_km1()).all()
    f.close()
