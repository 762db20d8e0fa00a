"""GPU: the prediction fed from a resident VO pair with the pair's own covariance as its process noise (pre3_predict_pair_cov_seeded; DESIGN.md
section 27).

The contract is bit identity with the chain on a second context: vo.vo_pair_cov_seeded(prev, cur) -> (cov_status == 1 and sta == 1:
set_process_noise(cov)) -> ekf_prediction(res["u"]) -> the previous setting restored.  x_k_km1, P, pnum, every field of the result, cov and its status,
byte for byte, waiting, not waiting, and a second time.  Pairs with sta == 1 (the pair's Pn is taken: P differs from the constant-noise prediction in
the pose block and nowhere else), with pnum < 4, and the no-consensus pair (fallback: byte-equal to pre3_predict_pair_seeded); a context with a
caller-set noise falls back to that, not to the constant; the setting is unchanged afterwards; argument and state errors leave everything unchanged."""
import ctypes as C
import importlib

import numpy as np
import pytest

from test_gpu_predict_pair import CONTEXTS, PAIRS, RES_FIELDS, resident, same_bytes, start_state
from test_gpu_process_noise import PN

pytestmark = pytest.mark.gpu
srm = importlib.import_module("3pre_amd.sr4000")
vo = importlib.import_module("3pre_amd.vo")
synth = importlib.import_module("3pre_amd.synth")
_lib = importlib.import_module("3pre_amd._lib")
E_ARG, E_STATE = -1, -4
SEED, SEQ = 5, 0
NAMES = ["p3", "p4", "p13", "p64", "no_consensus"]


@pytest.fixture(scope="module")
def pairs():
    cache = {}

    def get(name):
        if name not in cache:
            c = PAIRS[name][0]()
            f1, f2 = resident(c)
            cache[name] = dict(c=c, f1=f1, f2=f2, res=vo.vo_pair_cov_seeded(f1, f2, SEED, SEQ), want_sta=PAIRS[name][1])
            assert cache[name]["res"]["sta"] == PAIRS[name][1] and cache[name]["res"]["pnum"] == c["expect_pnum"]
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


def assert_same_result(got, res):
    for k in RES_FIELDS + ("cov_status",):
        assert same_bytes(np.asarray(got[k]), np.asarray(res[k])), (k, got[k], res[k])
    assert (got["cov"] is None) == (res["cov"] is None) and (got["cov"] is None or same_bytes(got["cov"], res["cov"]))


def chain(f, x0, P0, f1, f2):
    f.set_x_p_k_k(x0, P0)
    res = vo.vo_pair_cov_seeded(f1, f2, SEED, SEQ)
    before, src = f.process_noise
    if res["cov_status"] == 1 and res["sta"] == 1:
        f.set_process_noise(res["cov"])
    f.ekf_prediction(res["u"])
    f.set_process_noise(before if src == "caller" else None)
    return res, f._get(1)


@pytest.mark.parametrize("own", ["constant", "caller"])
@pytest.mark.parametrize("kind", sorted(CONTEXTS))
@pytest.mark.parametrize("name", NAMES)
def test_bit_identity_with_the_chain(pre3, pairs, contexts, name, kind, own):
    d, k = pairs(name), contexts(kind)
    fa, fb, x0, P0 = k["fa"], k["fb"], k["x0"], k["P0"]
    for f in (fa, fb):
        f.set_process_noise(PN if own == "caller" else None)
    try:
        res, (xa, Pa) = chain(fa, x0, P0, d["f1"], d["f2"])
        assert_same_result(res, d["res"])
        fb.set_x_p_k_k(x0, P0)
        got = fb.ekf_prediction_pair_cov_seeded(d["f1"], d["f2"], SEED, SEQ)
        assert_same_result(got, res)
        xb, Pb = fb._get(1)
        assert same_bytes(xb, xa) and same_bytes(Pb, Pa)
        for _ in range(2):
            fb.set_x_p_k_k(x0, P0)
            assert fb.ekf_prediction_pair_cov_seeded(d["f1"], d["f2"], SEED, SEQ, wait=False) is None
            xc, Pc = fb._get(1)
            assert same_bytes(xc, xa) and same_bytes(Pc, Pa)
        # the setting is the one from before
        Pn_now, src = fb.process_noise
        assert src == own and (own == "constant" or same_bytes(Pn_now, PN))
        # against pre3_predict_pair_seeded, which predicts with the context's own noise
        fb.set_x_p_k_k(x0, P0)
        fb.ekf_prediction_pair_seeded(d["f1"], d["f2"], SEED, SEQ)
        xo, Po = fb._get(1)
        assert same_bytes(xo, xb)                                  # the noise does not enter x
        taken = res["cov_status"] == 1 and res["sta"] == 1
        print(name, kind, own, "pnum sta cov_status =", res["pnum"], res["sta"], res["cov_status"], "taken" if taken else "fallback")
        if taken:
            assert not same_bytes(Pb[:7, :7], Po[:7, :7]) and same_bytes(Pb[7:, 7:], Po[7:, 7:]) and same_bytes(Pb[:7, 7:], Po[:7, 7:])
        else:
            assert res["cov_status"] == 0 and same_bytes(Pb, Po)   # pnum < 4, no consensus: the context's own noise -- caller-set, or the constant
    finally:
        fa.set_process_noise(None); fb.set_process_noise(None)


def test_the_pairs_cover_the_three_kinds(pairs):
    st = {n: (pairs(n)["res"]["pnum"], pairs(n)["res"]["sta"], pairs(n)["res"]["cov_status"]) for n in NAMES}
    assert st["p3"][0] < 4 and st["p3"][2] == 0
    assert st["no_consensus"][1] == 4 and st["no_consensus"][2] == 0
    assert any(s == 1 and cs == 1 for _, s, cs in st.values()), st


def test_argument_and_state_errors_leave_everything_unchanged(pre3, pairs, contexts):
    lib = _lib.lib
    k = contexts("n8_f32")
    fb, x0, P0 = k["fb"], k["x0"], k["P0"]
    d = pairs("p13")
    f1, f2 = d["f1"], d["f2"]
    res, pn, cst, cov = vo.VoResult(), C.c_int32(-7), C.c_int32(-7), np.full((7, 7), -3.0)
    fb.set_process_noise(PN)
    fb.set_x_p_k_k(x0, P0)

    def call(ctx, p, q, thresh=1.5):
        return lib.pre3_predict_pair_cov_seeded(ctx, p, q, thresh, SEED, SEQ, C.byref(pn), C.byref(res), _lib.dptr(cov), C.byref(cst))

    ctx = fb._ctx
    with srm.SrFrame(36, 45) as empty:
        cases = [("null context", lambda: call(None, f1._h, f2._h), E_ARG), ("null prev", lambda: call(ctx, None, f2._h), E_ARG),
                 ("null cur", lambda: call(ctx, f1._h, None), E_ARG), ("prev == cur", lambda: call(ctx, f1._h, f1._h), E_ARG),
                 ("thresh 0", lambda: call(ctx, f1._h, f2._h, 0.0), E_ARG), ("thresh nan", lambda: call(ctx, f1._h, f2._h, float("nan")), E_ARG),
                 ("nothing loaded", lambda: call(ctx, f1._h, empty._h), E_STATE)]
        for what, fn, want in cases:
            assert fn() == want, what
        assert (pn.value, cst.value) == (-7, -7) and np.all(cov == -3.0)
        xk, Pk = fb._get(0)
        assert same_bytes(xk, x0) and same_bytes(Pk, P0)
        assert fb.process_noise[1] == "caller" and same_bytes(fb.process_noise[0], PN)
        fb.ekf_prediction([0, 0, 0, 1.0, 0, 0, 0])
        xp, Pp = fb._get(1)
        assert call(ctx, f1._h, f2._h) == E_STATE and pn.value == -7
        xq, Pq = fb._get(1)
        assert same_bytes(xq, xp) and same_bytes(Pq, Pp)
    fb.set_process_noise(None)
    assert_same_result(vo.vo_pair_cov_seeded(f1, f2, SEED, SEQ), d["res"])
