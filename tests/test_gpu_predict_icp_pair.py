"""GPU: both covariances behind the ICP-refined pair (pre3_icp_pair_cov_seeded) and the prediction fed from it on the device
(pre3_predict_icp_pair_seeded).

pre3_icp_pair_cov_seeded: every output it shares with pre3_icp_pair_seeded byte for byte, the pair's covariance equal to pre3_vo_pair_cov_seeded's, the
ICP's equal to pre3_icp_cov fed the two clouds gathered through corr_pix, this call's pairs and icp["u"].

pre3_predict_icp_pair_seeded: bit identity of x_k_km1 and P with the chain on a second context -- vo.icp_pair_cov_seeded -> the selection rule restated
in tests/icp_cov_ref.py -> set_process_noise(the taken Pn) when one is taken -> ekf_prediction(the taken u) -> the previous setting restored --, in
f32 and f64 contexts, for noise 0 .. 3, with max_error = inf and one that rejects the ICP, on a constant and on a caller-set context noise, waiting and
not waiting, with taken_out in every case.  The pairs are tests/vo_pair_cases.py's small ones (36 x 45; bit identity needs no meaningful geometry):
sta == 1, pnum < 4, no consensus, a refused one; an ICP that ends with sta = 2 (a res no pair satisfies); and one reduced-size pair built as
tests/icp_frame_cases.py builds its frames, with planted keypoints, on which the ICP's u is really taken."""
import ctypes as C
import importlib

import numpy as np
import pytest

import icp_cov_ref as ref
import vo_pair_cases as vp
from icp_pair_cases import planted_pair
from test_gpu_predict_pair import CONTEXTS, IDENTITY, PAIRS, near_pair, resident, same_bytes, start_state
from test_gpu_process_noise import PN

pytestmark = pytest.mark.gpu
srm = importlib.import_module("3pre_amd.sr4000")
vo = importlib.import_module("3pre_amd.vo")
synth = importlib.import_module("3pre_amd.synth")
_lib = importlib.import_module("3pre_amd._lib")
E_ARG, E_STATE, E_NUMERIC = -1, -4, -5
SEED, SEQ = 5, 0
ROWS, COLS = 36, 45
ICP_KW = dict(stride=2, res=0.2)                    # the small random pairs: tests/test_gpu_icp_frames.py's setting
PLANTED_KW = dict(stride=1, res=0.09)               # about twice the pixel spacing of the reduced surface frames
REJECT = 1e-9                                       # an error no run reaches: sum(D) / (p res) of real pairs
PAIR_FIELDS = ("rot", "trans", "euler", "u", "error_mean", "error_std", "dist", "sta", "n_support", "n_iterations", "best", "pnum", "rst")
ICP_FIELDS = ("R", "t", "Rtot", "ttot", "u", "error", "sta", "p", "iters1", "iters2", "n_model", "n_source")


# name -> (the pair, the ICP's arguments, what the rule must take as u with max_error = inf)
CASES = {
    "planted": (planted_pair, PLANTED_KW, ref.U_ICP),
    "p13": (PAIRS["p13"][0], ICP_KW, None),                                     # random clouds: whatever the ICP ends with, the chain decides
    "p13_icp_few": (PAIRS["p13"][0], dict(stride=2, res=1e-7), ref.U_PAIR),     # no pair within 2 res: the ICP ends with sta = 2
    "p3": (PAIRS["p3"][0], ICP_KW, ref.U_IDENTITY),
    "no_consensus": (PAIRS["no_consensus"][0], ICP_KW, ref.U_IDENTITY),
}
KINDS = ("n8_f32", "n41_f64")


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(name):
        if name not in cache:
            make, kw, _ = CASES[name]
            c = make()
            f1, f2 = resident(c)
            pair, icp = vo.icp_pair_cov_seeded(f1, f2, SEED, SEQ, **kw)
            print(name, "pnum sta cov_status =", pair["pnum"], pair["sta"], pair["cov_status"], "| icp sta p error cov_status =", icp["sta"], icp.get("p"),
                  icp.get("error"), icp["cov_status"])
            assert pair["pnum"] == c["expect_pnum"]
            cache[name] = dict(c=c, f1=f1, f2=f2, kw=kw, pair=pair, icp=icp)
        return cache[name]

    yield get
    for d in cache.values():
        d["f1"].close(); d["f2"].close()


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


def same_dict(a, b, fields):
    for k in fields:
        assert same_bytes(np.asarray(a[k]), np.asarray(b[k])), (k, a[k], b[k])


def same_cov(a, b):
    assert a["cov_status"] == b["cov_status"] and (a["cov"] is None) == (b["cov"] is None) and (a["cov"] is None or same_bytes(a["cov"], b["cov"]))


def same_icp(a, b):
    assert a["sta"] == b["sta"]
    if a["sta"] != 0:
        same_dict(a, b, ICP_FIELDS)


# ---- pre3_icp_pair_cov_seeded
@pytest.mark.parametrize("name", ["planted", "p13", "p13_icp_few", "p3"])
def test_the_pair_cov_call_is_the_three_calls_it_stands_for(pre3, cases, name):
    d = cases(name)
    f1, f2, kw, pair, icp = d["f1"], d["f2"], d["kw"], d["pair"], d["icp"]
    base_pair, base_icp = vo.icp_pair_seeded(f1, f2, SEED, SEQ, **kw)
    same_dict(pair, base_pair, PAIR_FIELDS + ("draws", "cnum", "state", "inliers", "pset1", "pset2", "match"))
    assert pair["capped"] == base_pair["capped"]
    same_icp(icp, base_icp)
    if icp["sta"] != 0:
        same_dict(icp, base_icp, ("corr", "corr_pix", "data2", "log"))
    same_cov(pair, vo.vo_pair_cov_seeded(f1, f2, SEED, SEQ))
    if icp["sta"] != 1 or icp["p"] < 4:
        assert icp["cov_status"] == 0 and icp["cov"] is None
    else:
        x1, y1, z1, _ = f1.planes(); x2, y2, z2, _ = f2.planes()
        m, s = icp["corr_pix"][:, 0], icp["corr_pix"][:, 1]
        d1 = np.stack([-x1.ravel(order="F")[m], -y1.ravel(order="F")[m], z1.ravel(order="F")[m]])
        d2 = np.stack([-x2.ravel(order="F")[s], -y2.ravel(order="F")[s], z2.ravel(order="F")[s]])
        k = np.arange(1, icp["p"] + 1)
        direct = vo.icp_cov(d1, d2, np.stack([k, k], axis=1), icp["u"])
        assert direct["n"] == icp["p"]
        same_cov(icp, dict(cov_status=direct["status"], cov=direct["cov"]))
    again_pair, again_icp = vo.icp_pair_cov_seeded(f1, f2, SEED, SEQ, **kw)
    same_cov(again_pair, pair); same_cov(again_icp, icp); same_icp(again_icp, icp)


def test_the_planted_pair_really_takes_the_icp(cases):
    d = cases("planted")
    pair, icp = d["pair"], d["icp"]
    assert pair["sta"] == 1 and pair["cov_status"] == 1 and icp["sta"] == 1 and icp["cov_status"] == 1 and icp["p"] >= 256
    assert np.isfinite(icp["u"]).all() and REJECT < icp["error"] < np.inf
    few = cases("p13_icp_few")["icp"]
    assert few["sta"] == 2 and few["cov_status"] == 0


# ---- pre3_predict_icp_pair_seeded
def rule(pair, icp, max_error, noise):
    icp_sta = icp["sta"]
    finite = icp_sta != 0 and bool(np.isfinite(icp["u"]).all())
    return ref.select(pair["sta"], pair["pnum"], 0, 1, icp_sta, finite, icp.get("error", 0.0), max_error, noise, pair["cov_status"], icp["cov_status"])[:2]


def predict_with(f, x0, P0, u, Pn):
    """one prediction with Pn (None: the setting as it is) as the noise, the setting restored: (x_k_km1, P)"""
    f.set_x_p_k_k(x0, P0)
    before, src = f.process_noise
    if Pn is not None:
        f.set_process_noise(Pn)
    f.ekf_prediction(u)
    f.set_process_noise(before if src == "caller" else None)
    return f._get(1)


def chain(f, x0, P0, f1, f2, kw, max_error, noise):
    """(pair, icp, taken, (x, P)).  One case has no chain: mode 3 on a context that runs on the constant.  The constant's quaternion block as the
    launch builds it is symmetric only to the last place (Pn(6,3) != Pn(3,6)), so pre3_set_process_noise refuses cov_icp + constant; there the state
    is None and the caller checks the prediction against mode 2's plus the constant's own contribution instead."""
    pair, icp = vo.icp_pair_cov_seeded(f1, f2, SEED, SEQ, **kw)
    ut, nt = rule(pair, icp, max_error, noise)
    before, src = f.process_noise
    u = IDENTITY if ut == ref.U_IDENTITY else pair["u"] if ut == ref.U_PAIR else icp["u"]
    Pn = None if nt == ref.NOISE_CONTEXT else ref.taken_pn(nt, before, pair["cov"], icp["cov"])
    if nt == ref.NOISE_ICP_FLOOR and src == "constant":
        assert not np.array_equal(before, before.T) and np.abs(before - before.T).max() <= 4 * np.finfo(float).eps * np.abs(before).max()
        return pair, icp, (ut, nt), None
    return pair, icp, (ut, nt), predict_with(f, x0, P0, u, Pn)


P_GRANT = {"f64": 1e-13, "f32": 2e-6}               # of max |P|, given equal inputs: tests/test_gpu_synth.py::test_predict_parity's grant


def check_floor_on_the_constant(f, x0, P0, icp, got_x, got_P, dtype):
    """mode 3 over the constant: x and everything outside the pose block are mode 2's bytes; the pose block is mode 2's plus what the constant alone adds
    (the prediction with the constant minus the prediction with a zero noise), Q = G Pn G' being linear in Pn"""
    x2, P2 = predict_with(f, x0, P0, icp["u"], icp["cov"])
    _, Pc = predict_with(f, x0, P0, icp["u"], None)
    _, Pz = predict_with(f, x0, P0, icp["u"], np.zeros((7, 7)))
    assert same_bytes(got_x, x2) and same_bytes(got_P[7:, 7:], P2[7:, 7:]) and same_bytes(got_P[:7, 7:], P2[:7, 7:]) and same_bytes(got_P[7:, :7], P2[7:, :7])
    want = P2[:7, :7].astype(np.float64) + (Pc[:7, :7].astype(np.float64) - Pz[:7, :7])
    err = np.abs(got_P[:7, :7] - want).max() / np.abs(P2).max()
    print("mode 3 over the constant: pose block differs by %.2e of max |P| (grant %.0e)" % (err, 4 * P_GRANT[dtype]))
    assert err <= 4 * P_GRANT[dtype]                # four predictions enter the figure


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_bit_identity_with_the_chain(pre3, cases, contexts, name, kind):
    d, k = cases(name), contexts(kind)
    fa, fb, x0, P0 = k["fa"], k["fb"], k["x0"], k["P0"]
    f1, f2, kw = d["f1"], d["f2"], d["kw"]
    seen = set()
    try:
        for own in ("constant", "caller"):
            for f in (fa, fb):
                f.set_process_noise(PN if own == "caller" else None)
            for max_error in (float("inf"), REJECT):
                for noise in (0, 1, 2, 3):
                    pair, icp, taken, state = chain(fa, x0, P0, f1, f2, kw, max_error, noise)
                    same_dict(pair, d["pair"], PAIR_FIELDS); same_icp(icp, d["icp"])
                    fb.set_x_p_k_k(x0, P0)
                    got = fb.ekf_prediction_icp_pair_seeded(f1, f2, SEED, SEQ, max_error=max_error, noise=noise, **kw)
                    print(name, kind, own, "max_error", max_error, "noise", noise, "taken", got["taken"])
                    assert got["taken"] == taken
                    same_dict(got, pair, PAIR_FIELDS); same_cov(got, pair)
                    same_icp(got["icp"], icp); same_cov(got["icp"], icp)
                    xb, Pb = fb._get(1)
                    if state is None:
                        check_floor_on_the_constant(fa, x0, P0, icp, xb, Pb, k["dtype"])
                        xa, Pa = xb, Pb                                  # the form that does not wait gives the waiting form's bytes
                    else:
                        xa, Pa = state
                        assert same_bytes(xb, xa) and same_bytes(Pb, Pa)
                    fb.set_x_p_k_k(x0, P0)
                    assert fb.ekf_prediction_icp_pair_seeded(f1, f2, SEED, SEQ, max_error=max_error, noise=noise, wait=False, **kw) is None
                    xc, Pc = fb._get(1)                                  # pre3_get_state behind the call that did not wait
                    assert same_bytes(xc, xa) and same_bytes(Pc, Pa)
                    Pn_now, src = fb.process_noise                       # the setting is the one from before
                    assert src == own and (own == "constant" or same_bytes(Pn_now, PN))
                    if max_error == REJECT:
                        assert taken[0] != ref.U_ICP
                    seen.add(taken)
        want_u = CASES[name][2]
        if want_u is not None:
            assert want_u in {t[0] for t in seen}, seen
        if name == "planted":                                            # every pairing the rule can give with a pair that is taken
            assert seen == {(2, 0), (2, 1), (2, 2), (2, 3), (1, 0), (1, 1)}, seen
        if name in ("p3", "no_consensus"):
            assert seen == {(0, 0)}, seen
    finally:
        fa.set_process_noise(None); fb.set_process_noise(None)


def test_the_taken_noise_shows_in_the_pose_block_only(pre3, cases, contexts):
    d, k = cases("planted"), contexts("n41_f64")
    fb, x0, P0 = k["fb"], k["x0"], k["P0"]
    out = {}
    for noise in (0, 1, 2, 3):
        fb.set_x_p_k_k(x0, P0)
        got = fb.ekf_prediction_icp_pair_seeded(d["f1"], d["f2"], SEED, SEQ, noise=noise, **d["kw"])
        assert got["taken"] == (2, noise)
        out[noise] = fb._get(1)
    for noise in (1, 2, 3):
        (x, P), (x0_, P0_) = out[noise], out[0]
        assert same_bytes(x, x0_) and not same_bytes(P[:7, :7], P0_[:7, :7]) and same_bytes(P[7:, 7:], P0_[7:, 7:]) and same_bytes(P[:7, 7:], P0_[:7, 7:])
    # mode 3 adds the context's noise to mode 2's: every diagonal entry of the pose block is larger
    assert (np.diag(out[3][1])[:7] > np.diag(out[2][1])[:7]).all()


def test_a_pending_hi_downdate_is_carried_as_the_chain_carries_it(pre3, cases, contexts):
    """tests/test_gpu_predict_pair.py's set-up: fp32, PRE3_OPT_DEFER_HI + PRE3_OPT_PEND_HI, one step leaves a HI update deferred and its down-date pending"""
    N, n_hyp = 120, 60
    seq = synth.make_sequence(N, 2, n_hyp, seed=77, motion_noise=2.5)
    d = cases("planted")
    s0 = seq["steps"][0]
    filt = []
    for _ in range(2):
        f = pre3.EkfFilter(seq["cam"], np.zeros(N, np.int32), dtype="f32", max_hyp=n_hyp, std_z=1.0)
        f.defer_hi_update(True)
        assert f.pend_hi(True)
        filt.append(f)
    fa, fb = filt
    for f in filt:
        f.set_process_noise(PN)                                          # mode 3 over a caller-set noise: the chain exists (see chain())
        f.set_x_p_k_k(seq["x0"], seq["P0"])
    sa = fa.step(s0["u"], s0["meas_idx"], s0["z"], s0["hyp"], threshold=1.0, early_exit=False)
    sb = fb.step(s0["u"], s0["meas_idx"], s0["z"], s0["hyp"], threshold=1.0, early_exit=False)
    assert sa == sb
    pair, icp = vo.icp_pair_cov_seeded(d["f1"], d["f2"], SEED, SEQ, **d["kw"])
    assert rule(pair, icp, float("inf"), 3) == (2, 3)
    fa.set_process_noise(ref.taken_pn(3, PN, pair["cov"], icp["cov"]))
    fa.ekf_prediction(icp["u"])
    fa.set_process_noise(PN)
    assert fb.ekf_prediction_icp_pair_seeded(d["f1"], d["f2"], SEED, SEQ, noise=3, wait=False, **d["kw"]) is None
    (xa, Pa), (xb, Pb) = fa._get(1), fb._get(1)
    assert same_bytes(xa, xb) and same_bytes(Pa, Pb) and np.isfinite(Pa).all()
    fa.close(); fb.close()


def test_refused_pairs_predict_with_the_identity_and_report_once(pre3, contexts):
    k = contexts("n41_f64")
    fa, fb, x0, P0 = k["fa"], k["fb"], k["x0"], k["P0"]
    fa.set_x_p_k_k(x0, P0); fa.ekf_prediction(IDENTITY)
    xi, Pi = fa._get(1)
    f1, f2 = resident(near_pair())
    with f1, f2:
        with pytest.raises(pre3.Pre3Error) as e:
            vo.icp_pair_cov_seeded(f1, f2, SEED, SEQ, **ICP_KW)
        assert e.value.code == E_NUMERIC
        chain_msg = str(e.value)
        fb.set_x_p_k_k(x0, P0)
        with pytest.raises(pre3.Pre3Error) as e:
            fb.ekf_prediction_icp_pair_seeded(f1, f2, SEED, SEQ, noise=2, **ICP_KW)
        assert e.value.code == E_NUMERIC and str(e.value) == chain_msg
        xb, Pb = fb._get(1)
        assert same_bytes(xb, xi) and same_bytes(Pb, Pi)
        fb.set_x_p_k_k(x0, P0)
        assert fb.ekf_prediction_icp_pair_seeded(f1, f2, SEED, SEQ, noise=2, wait=False, **ICP_KW) is None
        with pytest.raises(pre3.Pre3Error) as e:
            fb._get(1)
        assert e.value.code == E_NUMERIC and "0.4 m" in str(e.value)
        xb, Pb = fb._get(1)
        assert same_bytes(xb, xi) and same_bytes(Pb, Pi)


def test_handles_reloaded_right_behind_the_call_stay_behind_its_reads(pre3, cases, contexts):
    k = contexts("n41_f64")
    fa, fb, x0, P0 = k["fa"], k["fb"], k["x0"], k["P0"]
    d, other = cases("planted"), vp.case("p12")
    _, _, taken, (xa, Pa) = chain(fa, x0, P0, d["f1"], d["f2"], d["kw"], float("inf"), 2)
    assert taken == (2, 2)
    A, B = resident(d["c"])
    with A, B:
        fb.set_x_p_k_k(x0, P0)
        assert fb.ekf_prediction_icp_pair_seeded(A, B, SEED, SEQ, noise=2, wait=False, **d["kw"]) is None
        B.load(other["fr2"], 1)
        B.keypoints(other["frm2"], other["des2"], 1)
        A.load(other["fr1"], 1)
        # a second run into the same blocks, queued while the first prediction may still be reading them
        A.keypoints(other["frm1"], other["des1"], 1)
        xb, Pb = fb._get(1)
        assert same_bytes(xb, xa) and same_bytes(Pb, Pa)
        fb.set_x_p_k_k(x0, P0)
        assert fb.ekf_prediction_icp_pair_seeded(A, B, SEED, SEQ, noise=3, wait=False, **ICP_KW) is None
        fb._get(1)


def test_an_empty_keypoint_record_is_a_result(pre3, cases, contexts):
    k = contexts("n8_f32")
    fa, fb, x0, P0 = k["fa"], k["fb"], k["x0"], k["P0"]
    fa.set_x_p_k_k(x0, P0); fa.ekf_prediction(IDENTITY)
    xi, Pi = fa._get(1)
    A, B = resident(cases("p13")["c"])
    with A, B:
        B.keypoints(np.zeros((4, 0)), np.zeros((128, 0)), 1)
        for wait in (True, False):
            fb.set_x_p_k_k(x0, P0)
            got = fb.ekf_prediction_icp_pair_seeded(A, B, SEED, SEQ, noise=3, wait=wait, **ICP_KW)
            if wait:
                assert (got["pnum"], got["sta"], got["taken"], got["icp"]["sta"], got["cov_status"], got["icp"]["cov_status"]) == (0, 4, (0, 0), 0, 0, 0)
            xb, Pb = fb._get(1)
            assert same_bytes(xb, xi) and same_bytes(Pb, Pi)


def test_argument_and_state_errors_leave_everything_unchanged(pre3, cases, contexts):
    lib = _lib.lib
    k = contexts("n8_f32")
    fb, x0, P0 = k["fb"], k["x0"], k["P0"]
    d = cases("p13")
    f1, f2 = d["f1"], d["f2"]
    res, r, pn = vo.VoResult(), vo.IcpResult(), C.c_int32(-7)
    cov, cst, tk = np.full((2, 49), -3.0), np.full(2, -7, np.int32), np.full(2, -7, np.int32)
    r.sta = -7
    fb.set_process_noise(PN)
    fb.set_x_p_k_k(x0, P0)

    def call(ctx, p, q, thresh=1.5, stride=2, rs=0.2, max_error=float("inf"), noise=0):
        return lib.pre3_predict_icp_pair_seeded(ctx, p, q, thresh, SEED, SEQ, stride, rs, max_error, noise, C.byref(pn), C.byref(res), C.byref(r),
                                                _lib.dptr(cov), _lib.dptr(cst), _lib.dptr(tk))

    ctx = fb._ctx
    with srm.SrFrame(ROWS, COLS) as empty:
        bad = [("null context", lambda: call(None, f1._h, f2._h), E_ARG), ("null prev", lambda: call(ctx, None, f2._h), E_ARG),
               ("null cur", lambda: call(ctx, f1._h, None), E_ARG), ("prev == cur", lambda: call(ctx, f1._h, f1._h), E_ARG),
               ("thresh 0", lambda: call(ctx, f1._h, f2._h, 0.0), E_ARG), ("stride 0", lambda: call(ctx, f1._h, f2._h, stride=0), E_ARG),
               ("res 0", lambda: call(ctx, f1._h, f2._h, rs=0.0), E_ARG), ("res nan", lambda: call(ctx, f1._h, f2._h, rs=float("nan")), E_ARG),
               ("max_error 0", lambda: call(ctx, f1._h, f2._h, max_error=0.0), E_ARG), ("max_error < 0", lambda: call(ctx, f1._h, f2._h, max_error=-1.0), E_ARG),
               ("max_error nan", lambda: call(ctx, f1._h, f2._h, max_error=float("nan")), E_ARG), ("noise -1", lambda: call(ctx, f1._h, f2._h, noise=-1), E_ARG),
               ("noise 4", lambda: call(ctx, f1._h, f2._h, noise=4), E_ARG), ("nothing loaded", lambda: call(ctx, f1._h, empty._h), E_STATE)]
        for what, fn, want in bad:
            assert fn() == want, what
        assert pn.value == -7 and r.sta == -7 and (cov == -3.0).all() and (cst == -7).all() and (tk == -7).all()
        xk, Pk = fb._get(0)
        assert same_bytes(xk, x0) and same_bytes(Pk, P0)
        assert fb.process_noise[1] == "caller" and same_bytes(fb.process_noise[0], PN)
        fb.ekf_prediction(IDENTITY)
        xp, Pp = fb._get(1)
        assert call(ctx, f1._h, f2._h) == E_STATE and pn.value == -7
        xq, Pq = fb._get(1)
        assert same_bytes(xq, xp) and same_bytes(Pq, Pp)
    fb.set_process_noise(None)
    pair, icp = vo.icp_pair_cov_seeded(f1, f2, SEED, SEQ, **d["kw"])          # the handles are the ones from before
    same_dict(pair, d["pair"], PAIR_FIELDS); same_icp(icp, d["icp"])
