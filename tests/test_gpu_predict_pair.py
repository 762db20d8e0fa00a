"""GPU: the prediction fed from a resident VO pair, u never leaving the device (pre3_predict_pair_seeded).

The contract is bit identity with the chain that exists without it -- vo.vo_pair_seeded(prev, cur) followed by EkfFilter.ekf_prediction(res["u"]) on a
second context with the same start: x_k_km1, P, pnum and every field of the result, byte for byte, with and without the host wait, twice.  Independently
of the device chain, x and P are compared with oracle.predict fed the u of the restatement / oracle chain (tests/vo_pair_cases.py's restated_chain,
tests/draws_ref.py's draws, oracle.vo_ransac: the oracle_pair recipe of tests/test_vo_pair_ref.py).

Tolerances of the oracle comparison.  Given equal u, tests/test_gpu_synth.py::test_predict_parity grants |dx| < 1e-14 and |dP| < 1e-13 (fp64) / 2e-6
(fp32) of max |P|.  The device's u differs from the oracle's by d <= 1e-12 per entry (tests/test_gpu_vo.py::_compare).  x: the position moves by at
most sqrt(3) d (a row of a rotation has 1-norm <= sqrt(3)); an entry of q x u_q by sum |q_i| d <= 2 d, and the normalisation adds at most
|xo_i| * ||d xo||_2 / |xo|^2 <= 4 d: 6 d in all, so X_TOL = 1e-14 + 6e-12.  P: rows 3..6 are Jn Qq1 P -- sixteen products per entry, every factor
at most 1 in magnitude for a unit quaternion; Qq1's entries are u_q's (change d), Jn's are quadratic in xo over |xo|^3 with gradient at most 5 per
entry (change <= 5 * 2 d): (1 + 10) d per product, 176 d per entry, twice that for the 4 x 4 block where the congruence acts on both sides:
352 d <= 4e-10 of max |P| on top of the equal-u tolerance.  The process noise term does not depend on u."""
import ctypes as C
import importlib

import numpy as np
import pytest

import draws_ref
import sr_frame_ref as sr
import vo_pair_cases as vp

pytestmark = pytest.mark.gpu
srm = importlib.import_module("3pre_amd.sr4000")
vo = importlib.import_module("3pre_amd.vo")
synth = importlib.import_module("3pre_amd.synth")
_lib = importlib.import_module("3pre_amd._lib")
E_ARG, E_STATE, E_NUMERIC = -1, -4, -5
SEED, SEQ = 5, 0
W1 = sr.gauss3(1.0)
IDENTITY = np.array([0, 0, 0, 1.0, 0, 0, 0])
RES_FIELDS = ("rot", "trans", "euler", "u", "error_mean", "error_std", "dist", "sta", "n_support", "n_iterations", "best", "pnum", "rst")
D_U = 1e-12
X_TOL = 1e-14 + 6 * D_U
P_TOL = {"f64": 1e-13 + 352 * D_U, "f32": 2e-6 + 352 * D_U}

# name -> (the pair, the sta its chain must end in)
PAIRS = {
    "p0": (lambda: vp.case("p0"), 4), "p3": (lambda: vp.case("p3"), 4), "p4": (lambda: vp.case("p4"), 1), "p13": (lambda: vp.case("p13"), 1),
    "p64": (lambda: vp.case("p64"), 1), "n5x1_shared": (lambda: vp.case("n5x1_shared"), 1),
    "no_consensus": (lambda: dict(vp.make_pair(36, 45, 33, 65, 12, seed=40, outliers=1.0, drop1=2), expect_pnum=12), 4),
}
CONTEXTS = {"n0_f64": (0, "f64"), "n8_f32": (8, "f32"), "n41_f32": (41, "f32"), "n41_f64": (41, "f64")}


def near_pair():
    return vp.make_pair(36, 45, 33, 65, 12, seed=21, near=True, drop1=2)


def resident(c):
    f1, f2 = srm.SrFrame(c["rows"], c["cols"]), srm.SrFrame(c["rows"], c["cols"])
    f1.load(c["fr1"], 1); f2.load(c["fr2"], 1)
    f1.keypoints(c["frm1"], c["des1"], 1); f2.keypoints(c["frm2"], c["des2"], 1)
    return f1, f2


def start_state(N):
    """a start with a turned camera and non-zero velocities (nothing the prediction multiplies is a structural zero)"""
    if N == 0:
        rng = np.random.default_rng(13)
        A = rng.standard_normal((13, 13)) * 0.01
        x0, P0 = np.zeros(13), A @ A.T + 1e-6 * np.eye(13)
        P0 = (P0 + P0.T) / 2
    else:
        x0, P0, _ = synth.make_map(N, None)
    x0[0:3] = [0.3, -0.2, 0.1]
    x0[3:7] = np.array([0.98, 0.1, -0.12, 0.05]) / np.linalg.norm([0.98, 0.1, -0.12, 0.05])
    x0[7:13] = 0.3
    return x0, P0


@pytest.fixture(scope="module")
def pair_data(orc):
    """per pair, once: the case, its two resident frames, the device chain's result, and the u of the restatement / oracle chain"""
    cache = {}

    def get(name):
        if name not in cache:
            make, want_sta = PAIRS[name]
            c = make()
            f1, f2 = resident(c)
            res = vo.vo_pair_seeded(f1, f2, SEED, SEQ)
            ch = vp.restated_chain(c, orc, W1)
            pnum = ch["match"].shape[1]
            u_orc = IDENTITY
            if pnum >= 4:
                draws, _, _ = draws_ref.draw_vo(SEED, SEQ, ch["match"], vo.vo_rst(pnum))
                ref = orc.vo_ransac(ch["p1"], ch["p2"], draws)
                assert ref["sta"] == want_sta, (name, ref["sta"])
                if ref["sta"] == 1:
                    u_orc = np.r_[ref["trans"], orc.R2q(ref["rot"])]
            print(name, "pnum rst sta =", res["pnum"], res["rst"], res["sta"])
            # a case that drifts fails here instead of silently testing nothing
            assert res["pnum"] == pnum == c["expect_pnum"] and res["sta"] == want_sta, (name, res["pnum"], res["sta"])
            cache[name] = dict(c=c, f1=f1, f2=f2, res=res, u_orc=u_orc)
        return cache[name]

    yield get
    for d in cache.values():
        d["f1"].close(); d["f2"].close()


@pytest.fixture(scope="module")
def contexts(pre3):
    """per context kind, once: two filters (the chain's and the new call's) and the start as the device holds it"""
    cache = {}

    def get(kind):
        if kind not in cache:
            N, dtype = CONTEXTS[kind]
            x0, P0 = start_state(N)
            fa, fb = (pre3.EkfFilter(synth.CAM, np.zeros(N, np.int32), dtype=dtype, max_hyp=8) for _ in range(2))
            fa.set_x_p_k_k(x0, P0)
            xr, Pr = fa._get(0)                          # (fp32: P0 as rounded on its way in)
            cache[kind] = dict(fa=fa, fb=fb, x0=xr, P0=Pr, dtype=dtype, n=13 + 6 * N)
        return cache[kind]

    yield get
    for d in cache.values():
        d["fa"].close(); d["fb"].close()


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_same_result(got, res):
    for k in RES_FIELDS:
        assert same_bytes(np.asarray(got[k]), np.asarray(res[k])), (k, got[k], res[k])


def chain(f, x0, P0, f1, f2):
    """what exists without the new call: the pair, its 56 bytes to the host and back by value"""
    f.set_x_p_k_k(x0, P0)
    res = vo.vo_pair_seeded(f1, f2, SEED, SEQ)
    f.ekf_prediction(res["u"])
    return res, f._get(1)


@pytest.mark.parametrize("kind", sorted(CONTEXTS))
@pytest.mark.parametrize("name", sorted(PAIRS))
def test_bit_identity_with_the_chain_and_the_oracle_prediction(pre3, orc, pair_data, contexts, name, kind):
    d, k = pair_data(name), contexts(kind)
    fa, fb, x0, P0 = k["fa"], k["fb"], k["x0"], k["P0"]
    if kind.startswith("n41"):
        assert k["n"] == 259 and -(-k["n"] // 256) == 2        # two prediction blocks, three columns in the second
    res, (xa, Pa) = chain(fa, x0, P0, d["f1"], d["f2"])
    assert_same_result(res, d["res"])
    # the waiting form
    fb.set_x_p_k_k(x0, P0)
    got = fb.ekf_prediction_pair_seeded(d["f1"], d["f2"], SEED, SEQ)
    assert_same_result(got, res)
    xb, Pb = fb._get(1)
    assert same_bytes(xb, xa) and same_bytes(Pb, Pa)
    # the form that does not wait, then a second identical call
    for _ in range(2):
        fb.set_x_p_k_k(x0, P0)
        assert fb.ekf_prediction_pair_seeded(d["f1"], d["f2"], SEED, SEQ, wait=False) is None
        xc, Pc = fb._get(1)
        assert same_bytes(xc, xa) and same_bytes(Pc, Pa)
    # the prediction has happened as far as the context's flags go: x_k_k is still there, P holds the prediction
    assert same_bytes(fb.get_x_k_k(), x0)
    with pytest.raises(pre3.Pre3Error) as e:
        fb.get_p_k_k()
    assert e.value.code == E_STATE
    # the oracle, independently of the device chain
    xr, Pr = orc.predict(x0, P0, d["u_orc"])
    ex, eP = np.abs(xb - xr).max(), np.abs(Pb - Pr).max() / np.abs(Pr).max()
    print(name, kind, "x err %.3g  P err %.3g of max |P|" % (ex, eP))
    assert ex < X_TOL and eP < P_TOL[k["dtype"]]
    if d["res"]["sta"] != 1:
        assert same_bytes(res["u"], IDENTITY)                    # the chain fed the identity, +0 everywhere: the rule's own identity is the same bytes


def test_a_pending_hi_downdate_is_carried_as_the_chain_carries_it(pre3, pair_data):
    """fp32, PRE3_OPT_DEFER_HI + PRE3_OPT_PEND_HI (the N = 120 set-up of tests/test_gpu_pend_hi.py): one step leaves a HI update deferred and its
    down-date pending; the prediction completes the one and transforms the other's rows, from the pair as from the chain"""
    N, n_hyp = 120, 60
    seq = synth.make_sequence(N, 2, n_hyp, seed=77, motion_noise=2.5)
    d = pair_data("p13")
    s0, s1 = seq["steps"]
    filt = []
    for _ in range(2):
        f = pre3.EkfFilter(seq["cam"], np.zeros(N, np.int32), dtype="f32", max_hyp=n_hyp, std_z=1.0)
        f.defer_hi_update(True)
        assert f.pend_hi(True)
        filt.append(f)
    fa, fb = filt

    def front(f, pair_call):
        f.set_x_p_k_k(seq["x0"], seq["P0"])
        st = f.step(s0["u"], s0["meas_idx"], s0["z"], s0["hyp"], threshold=1.0, early_exit=False)
        if pair_call:
            assert f.ekf_prediction_pair_seeded(d["f1"], d["f2"], SEED, SEQ, wait=False) is None
        else:
            f.ekf_prediction(vo.vo_pair_seeded(d["f1"], d["f2"], SEED, SEQ)["u"])
        return st

    # x and P behind the prediction (the read completes what is pending)
    sa, sb = front(fa, False), front(fb, True)
    assert sa == sb
    (xa, Pa), (xb, Pb) = fa._get(1), fb._get(1)
    assert same_bytes(xa, xb) and same_bytes(Pa, Pb) and np.isfinite(Pa).all()
    # the next step takes the pending rows along: its statistics, its LI / HI sets and its estimate
    front(fa, False); front(fb, True)
    out = []
    for f in (fa, fb):
        f.search_IC_matches(); f.set_measurements(s1["meas_idx"], s1["z"])
        st = f.step_predicted(s1["hyp"], threshold=1.0, early_exit=False)
        li, hi = f.get_flags()
        out.append((st, li.copy(), hi.copy(), f.get_x_k_k(), f.get_p_k_k()))
    (sta_, lia, hia, xa, Pa), (stb, lib_, hib, xb, Pb) = out
    print("next step:", sta_)
    assert sta_["n_hi"] > 0                                     # (under PRE3_OPT_DEFER_HI: the count of step 0's deferred HI update -- it was pending)
    assert sta_ == stb and np.array_equal(lia, lib_) and np.array_equal(hia, hib)
    assert same_bytes(xa, xb) and same_bytes(Pa, Pb)
    fa.close(); fb.close()


def test_refused_pairs_predict_with_the_identity_and_report_once(pre3, pair_data, contexts):
    k = contexts("n41_f32")
    fa, fb, x0, P0 = k["fa"], k["fb"], k["x0"], k["P0"]
    fa.set_x_p_k_k(x0, P0); fa.ekf_prediction(IDENTITY)
    xi, Pi = fa._get(1)
    f1, f2 = resident(near_pair())
    with f1, f2:
        with pytest.raises(pre3.Pre3Error) as e:
            vo.vo_pair_seeded(f1, f2, SEED, SEQ)
        assert e.value.code == E_NUMERIC
        chain_msg = str(e.value)
        # the waiting form: the chain's code and message, the context holding the identity prediction and usable
        fb.set_x_p_k_k(x0, P0)
        with pytest.raises(pre3.Pre3Error) as e:
            fb.ekf_prediction_pair_seeded(f1, f2, SEED, SEQ)
        assert e.value.code == E_NUMERIC and str(e.value) == chain_msg
        xb, Pb = fb._get(1)
        assert same_bytes(xb, xi) and same_bytes(Pb, Pi)
        # the form that does not wait: OK, then PRE3_E_NUMERIC once from the next reader of the error words
        fb.set_x_p_k_k(x0, P0)
        assert fb.ekf_prediction_pair_seeded(f1, f2, SEED, SEQ, wait=False) is None
        with pytest.raises(pre3.Pre3Error) as e:
            fb._get(1)
        assert e.value.code == E_NUMERIC and "pre3_predict_pair_seeded" in str(e.value) and "0.4 m" in str(e.value)
        xb, Pb = fb._get(1)
        assert same_bytes(xb, xi) and same_bytes(Pb, Pi)
        # a clean pair afterwards on the same handles and context: the word and the header are cleared per call
        good = vp.case("p13")
        f1.load(good["fr1"], 1); f2.load(good["fr2"], 1)
        f1.keypoints(good["frm1"], good["des1"], 1); f2.keypoints(good["frm2"], good["des2"], 1)
        res, (xa, Pa) = chain(fa, x0, P0, f1, f2)
        assert res["sta"] == 1
        for wait in (True, False):
            fb.set_x_p_k_k(x0, P0)
            got = fb.ekf_prediction_pair_seeded(f1, f2, SEED, SEQ, wait=wait)
            if wait:
                assert_same_result(got, res)
            xb, Pb = fb._get(1)
            assert same_bytes(xb, xa) and same_bytes(Pb, Pa)
    assert_same_result(res, pair_data("p13")["res"])


def test_a_load_into_cur_right_behind_the_call_stays_behind_the_read_of_u(pre3, pair_data, contexts):
    k = contexts("n41_f64")
    fa, fb, x0, P0 = k["fa"], k["fb"], k["x0"], k["P0"]
    d, other = pair_data("p13"), vp.case("p12")
    _, (xa, Pa) = chain(fa, x0, P0, d["f1"], d["f2"])
    A, B = resident(d["c"])
    with A, B:
        fb.set_x_p_k_k(x0, P0)
        assert fb.ekf_prediction_pair_seeded(A, B, SEED, SEQ, wait=False) is None
        B.load(other["fr2"], 1)
        B.keypoints(other["frm2"], other["des2"], 1)
        A.load(other["fr1"], 1)
        xb, Pb = fb._get(1)
    assert same_bytes(xb, xa) and same_bytes(Pb, Pa)


def test_an_empty_keypoint_record_is_a_result(pre3, pair_data, contexts):
    k = contexts("n8_f32")
    fa, fb, x0, P0 = k["fa"], k["fb"], k["x0"], k["P0"]
    fa.set_x_p_k_k(x0, P0); fa.ekf_prediction(IDENTITY)
    xi, Pi = fa._get(1)
    c = pair_data("p13")["c"]
    A, B = resident(c)
    with A, B:
        B.keypoints(np.zeros((4, 0)), np.zeros((128, 0)), 1)
        for wait in (True, False):
            fb.set_x_p_k_k(x0, P0)
            got = fb.ekf_prediction_pair_seeded(A, B, SEED, SEQ, wait=wait)
            if wait:
                assert (got["pnum"], got["rst"], got["sta"], got["n_support"]) == (0, 0, 4, 0) and same_bytes(got["u"], IDENTITY)
            xb, Pb = fb._get(1)
            assert same_bytes(xb, xi) and same_bytes(Pb, Pi)


def test_argument_and_state_errors_leave_context_and_handles_unchanged(pre3, pair_data, contexts):
    lib = _lib.lib
    k = contexts("n8_f32")
    fa, fb, x0, P0 = k["fa"], k["fb"], k["x0"], k["P0"]
    d = pair_data("p13")
    c, f1, f2 = d["c"], d["f1"], d["f2"]
    res, pn = vo.VoResult(), C.c_int32(-7)
    fb.set_x_p_k_k(x0, P0)

    def call(ctx, p, q, thresh=1.5):
        return lib.pre3_predict_pair_seeded(ctx, p, q, thresh, SEED, SEQ, C.byref(pn), C.byref(res))

    with srm.SrFrame(36, 46) as other, srm.SrFrame(36, 45) as empty, srm.SrFrame(36, 45) as nd64, srm.SrFrame(36, 45) as fresh:
        other.load({k_: (None if v is None else np.asfortranarray(np.pad(v, ((0, 0), (0, 1)), mode="edge"))) for k_, v in c["fr2"].items()}, 1)
        other.keypoints(c["frm2"], c["des2"], 1)
        nd64.load(c["fr2"], 1); nd64.keypoints(c["frm2"], c["des2"][:64], 1)
        fresh.load(c["fr2"], 1)                                     # loaded, no keypoint call yet
        ctx = fb._ctx
        cases = [("null context", lambda: call(None, f1._h, f2._h), E_ARG), ("null prev", lambda: call(ctx, None, f2._h), E_ARG),
                 ("null cur", lambda: call(ctx, f1._h, None), E_ARG), ("prev == cur", lambda: call(ctx, f1._h, f1._h), E_ARG),
                 ("sizes differ", lambda: call(ctx, f1._h, other._h), E_ARG), ("ND != 128 on cur", lambda: call(ctx, f1._h, nd64._h), E_ARG),
                 ("ND != 128 on prev", lambda: call(ctx, nd64._h, f2._h), E_ARG), ("thresh 0", lambda: call(ctx, f1._h, f2._h, 0.0), E_ARG),
                 ("thresh nan", lambda: call(ctx, f1._h, f2._h, float("nan")), E_ARG), ("thresh inf", lambda: call(ctx, f1._h, f2._h, float("inf")), E_ARG),
                 ("nothing loaded", lambda: call(ctx, f1._h, empty._h), E_STATE), ("no keypoint record", lambda: call(ctx, fresh._h, f2._h), E_STATE)]
        if pre3.device_count() >= 2:
            with srm.SrFrame(36, 45, device=1) as g1, srm.SrFrame(36, 45, device=1) as g2:
                g1.load(c["fr1"], 1); g2.load(c["fr2"], 1)
                g1.keypoints(c["frm1"], c["des1"], 1); g2.keypoints(c["frm2"], c["des2"], 1)
                rc = call(ctx, g1._h, g2._h)
                assert rc == E_ARG and b"device" in lib.pre3_last_error()
        for what, fn, want in cases:
            rc = fn()
            assert rc == want, (what, rc)
        assert pn.value == -7                                        # nothing was written
        xk, Pk = fb._get(0)
        assert same_bytes(xk, x0) and same_bytes(Pk, P0)             # the context still holds (x_k_k, p_k_k)
        # pre3_predict's state requirement: a context whose covariance buffer holds the prediction
        fb.ekf_prediction(IDENTITY)
        xp, Pp = fb._get(1)
        assert call(ctx, f1._h, f2._h) == E_STATE and pn.value == -7
        xq, Pq = fb._get(1)
        assert same_bytes(xq, xp) and same_bytes(Pq, Pp)
    assert_same_result(vo.vo_pair_seeded(f1, f2, SEED, SEQ), d["res"])      # the keypoint records are the ones from before
