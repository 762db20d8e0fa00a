"""GPU: the candidates' weighted order drawn on the device (k_cand_keys, k_cand_rank) against the restatement
tests/cand_order_ref.py, and pre3_map_policy_seeded against pre3_map_policy fed with the restatement's permuted arrays.

Keys are compared to 1e-12 relative (the project's bound for fp64 device geometry against numpy, section 17: log1p * exp is a few ulp); the order is
compared EXACTLY, twice: against the stable argsort of the device's own keys (no rounding edge at all), and against the restatement's order on inputs
whose smallest relative gap between adjacent sorted keys is asserted first to be at least 1e-9, a thousand times the key tolerance.  The siblings'
outputs are compared bit for bit: behind the two new launches the seeded call launches what the unseeded one launches."""
import ctypes as C
import importlib

import numpy as np
import pytest

import cand_order_ref as cr
from test_gpu_map_policy import _case, _filter

pytestmark = pytest.mark.gpu
synth = importlib.import_module("3pre_amd.synth")
_lib = importlib.import_module("3pre_amd._lib")

KEY_RTOL, MIN_GAP = 1e-12, 1e-9
SEEDS = ((0x9E3779B97F4A7C15, 41), (3, 1 << 40))          # (a seed with the top bit set and a seq beyond 32 bits: the words are unsigned all the way)
K_SIZES = (1, 5, 63, 64, 65, 256, 257, 700, 8192)          # one wave, its edges; one / two workgroups of k_cand_rank's 64 i; the tile of 1024 j; the cap
E_ARG = -1
_REF = {}


def _uv(K):
    rng = np.random.default_rng(1000 + K)
    return np.stack([rng.uniform(3, 173, K), rng.uniform(3, 141, K)], 1)


def ref_keys(K, seed, seq, box=cr.BOX):
    """the restatement's keys and order, computed once per case and shared; the input condition is asserted here, loudly"""
    key = (K, seed, seq, box)
    if key not in _REF:
        k = cr.keys(_uv(K), seed, seq, box)
        assert np.isfinite(k).all() and not np.isnan(k).any()      # the invariant the rank kernel relies on: no NaN for finite uv
        gap = cr.min_relative_gap(k)
        assert gap >= MIN_GAP, "K=%d seed=%d seq=%d: adjacent keys %g apart (relative): choose other pixels" % (K, seed, seq, gap)
        o = cr.order_of_keys(k)
        k.setflags(write=False); o.setflags(write=False)
        _REF[key] = (k, o)
    return _REF[key]


@pytest.mark.parametrize("K", K_SIZES)
def test_stateless_order_against_the_restatement(pre3, K):
    assert pre3.device_count() >= 1
    for seed, seq in SEEDS:
        rk, ro = ref_keys(K, seed, seq)
        o, k = synth.candidate_order(_uv(K), seed, seq, return_keys=True)
        rel = np.abs(k / rk - 1).max()
        print("K=%d seed=%#x seq=%d: max relative key error %.3g" % (K, seed, seq, rel))
        assert not np.isnan(k).any() and rel < KEY_RTOL, rel
        assert np.array_equal(o, cr.order_of_keys(k))                # exactly the stable argsort of the device's own keys
        assert np.array_equal(o, ro)
        assert sorted(o.tolist()) == list(range(K))


def test_an_odd_box_rounds_half_away_from_zero(pre3):
    box = (175, 141)                                               # mean (88, 71), sigma (29, 24): 70.5 -> 71, 23.5 -> 24
    rk, ro = ref_keys(257, 5, 6, box)
    o, k = synth.candidate_order(_uv(257), 5, 6, box=box, return_keys=True)
    assert np.abs(k / rk - 1).max() < KEY_RTOL and np.array_equal(o, ro)
    assert not np.array_equal(k, synth.candidate_order(_uv(257), 5, 6, box=(176, 144), return_keys=True)[1])


def test_repeats_are_bit_equal_and_seq_changes_the_order(pre3):
    uv = _uv(700)
    seed, seq = SEEDS[0]
    o, k = synth.candidate_order(uv, seed, seq, return_keys=True)
    for _ in range(3):
        o2, k2 = synth.candidate_order(uv, seed, seq, return_keys=True)
        assert np.array_equal(o, o2) and np.array_equal(k, k2)
    assert np.array_equal(o, synth.candidate_order(uv, seed, seq))                 # keys_out = NULL
    assert not np.array_equal(o, synth.candidate_order(uv, seed, seq + 1))
    assert not np.array_equal(o, synth.candidate_order(uv, seed + 1, seq))
    assert synth.candidate_order(np.zeros((0, 2)), seed, seq).shape == (0,)        # K = 0: OK, nothing written


def test_duplicate_pixels_and_extreme_keys(pre3):
    uv = np.tile(_uv(65), (4, 1))                                  # every pixel four times: distinct streams, distinct keys
    uv[7] = [1e6, 72.0]                                            # absurdly far: key +inf
    uv[200] = [1e6, 72.0]
    seed, seq = SEEDS[1]
    o, k = synth.candidate_order(uv, seed, seq, return_keys=True)
    rk = cr.keys(uv, seed, seq)
    assert k[7] == np.inf and k[200] == np.inf and not np.isnan(k).any()
    fin = np.isfinite(rk)
    assert np.array_equal(np.isfinite(k), fin) and np.abs(k[fin] / rk[fin] - 1).max() < KEY_RTOL
    assert np.array_equal(o, cr.order_of_keys(k))
    assert o[-2:].tolist() == [7, 200]                             # equal keys (+inf) break by index
    assert sorted(o.tolist()) == list(range(260))


def test_every_argument_error_of_the_stateless_call(pre3):
    lib = _lib.lib
    uv = np.ascontiguousarray(_uv(8))
    order = np.full(8, -7, np.int32)
    bad = np.ascontiguousarray(uv.copy()); bad[3, 1] = np.nan
    inf = np.ascontiguousarray(uv.copy()); inf[0, 0] = np.inf
    big = np.ones((8193, 2))
    cases = [(-1, uv, 176, 144), (8193, big, 176, 144), (8, uv, 0, 144), (8, uv, 176, -3), (8, uv, 2, 144), (8, uv, 176, 2), (8, None, 176, 144),
             (8, bad, 176, 144), (8, inf, 176, 144)]
    for K, a, w, h in cases:
        rc = lib.pre3_candidate_order(0, K, _lib.dptr(a), w, h, 1, 1, _lib.dptr(order) if K <= 8 else None, None)
        assert rc == E_ARG, (K, w, h)
        assert b"pre3_candidate_order" in lib.pre3_last_error()
        assert (order == -7).all()                                 # nothing was launched or written
    assert lib.pre3_candidate_order(0, 8, _lib.dptr(uv), 176, 144, 1, 1, None, None) == E_ARG
    assert lib.pre3_candidate_order(0, 0, None, 176, 144, 1, 1, None, None) == 0
    assert lib.pre3_candidate_order(0, 8, _lib.dptr(uv), 3, 3, 1, 1, _lib.dptr(order), None) == 0      # the smallest legal box: sigma 1
    assert sorted(order.tolist()) == list(range(8))


# ---- the context call against its sibling -----------------------------------------------------------------------------------------------------------
def _ref_order(cand_uv, seed, seq):
    k = cr.keys(cand_uv, seed, seq)
    assert not np.isnan(k).any() and (len(k) < 2 or cr.min_relative_gap(k) >= MIN_GAP)
    return cr.order_of_keys(k)


def _same_as_sibling(pre3, dtype, N, K, strict, cap, mf, seed, seq):
    x, P, cam, step, book, meas, li, hi, cand_uv, cand_xyz, cand_desc = _case(N, K, 7 + N + K, cap)
    o = _ref_order(cand_uv, seed, seq)
    f = _filter(pre3, cam, N, x, P, dtype, cap, meas, li, hi, book)
    g = _filter(pre3, cam, N, x, P, dtype, cap, meas, li, hi, book)
    kw = dict(min_features=mf, linearity_index_threshold=0.1, std_pxl=1.0, strict_reference=strict)
    out = f.map_management_policy_seeded(step, cand_uv, cand_xyz, seed, seq, cand_desc=cand_desc, **kw)
    ref = g.map_management_policy(step, cand_uv[o], cand_xyz[o], cand_desc[:, o], **kw)
    assert np.array_equal(out["order"], o)
    assert np.array_equal(out["deleted"], ref["deleted"]) and np.array_equal(out["converted"], ref["converted"])
    assert all(out[k] == ref[k] for k in ("measured", "target", "examined", "N"))
    assert np.array_equal(out["accepted"], o[ref["accepted"]])       # the caller's indices: the drawn positions mapped through the order
    assert f.N == g.N and np.array_equal(f.lm_type, g.lm_type)
    assert np.array_equal(f.book(), g.book())
    assert np.array_equal(f.get_x_k_k(), g.get_x_k_k()) and np.array_equal(f.get_p_k_k(), g.get_p_k_k())
    if f.N:
        assert np.array_equal(f.get_descriptors(), g.get_descriptors())
    n_s = N - len(out["deleted"])
    if len(out["accepted"]):
        assert np.array_equal(f.get_descriptors()[:, n_s:], cand_desc[:, out["accepted"]])
    f.close(); g.close()
    return out


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("N,K", [(N, K) for N in (0, 30, 120) for K in (5, 65, 300)])
@pytest.mark.parametrize("strict", [True, False])
def test_seeded_policy_is_its_sibling_on_the_permuted_arrays(pre3, dtype, N, K, strict):
    seed, seq = SEEDS[(N + K) % 2]
    out = _same_as_sibling(pre3, dtype, N, K, strict, N + 40, 50, seed, seq + N)
    if K == 5:
        # T exceeds the admissible candidates: the walk exhausts the drawn order
        assert out["target"] > 5 and out["examined"] == K and len(out["accepted"]) < out["target"]
    if N == 0 and K == 300:
        assert len(out["accepted"]) > 3 and not np.array_equal(out["accepted"], np.sort(out["accepted"]))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_seeded_policy_at_capacity(pre3, dtype):
    N, K = 30, 65
    out = _same_as_sibling(pre3, dtype, N, K, False, N + 3, 50, *SEEDS[0])
    assert out["N"] == N - len(out["deleted"]) + len(out["accepted"]) == N + 3      # the additions stopped at the capacity ...
    assert out["target"] > len(out["accepted"]) and out["examined"] < K               # ... not at the target, nor at the end of the order


def test_three_chained_frames_are_the_unseeded_chain(pre3):
    """seeded policy -> prediction -> measurements -> pre3_step_predicted_seeded over three frames at N = 120 (fp32, the HI update deferred and its
    down-date pending across the frame boundary), against the same chain with pre3_map_policy fed the restatement's permuted candidates.  The book
    deletes nothing, so the sequence's measurement indices stay valid; the walk adds landmarks behind them."""
    N, N_HYP, K, cap = 120, 60, 300, 200
    seq = synth.make_sequence(N, 3, N_HYP, seed=77, motion_noise=2.5)
    cam = seq["cam"]
    seed = SEEDS[0][0]
    rng = np.random.default_rng(8)
    frames = []
    for t in range(3):
        uv = np.stack([rng.uniform(3, cam[6] - 3, K), rng.uniform(3, cam[5] - 3, K)], 1)
        xyz = np.c_[rng.normal(0, 0.3, (K, 2)), rng.uniform(1.0, 4.0, K)]
        frames.append((uv, xyz, rng.integers(0, 255, (128, K)).astype(float), _ref_order(uv, seed, 3 + t)))

    def run(seeded):
        f = pre3.EkfFilter(cam, np.zeros(N, np.int32), dtype="f32", max_hyp=N_HYP, max_landmarks=cap)
        f.defer_hi_update(True)
        assert f.pend_hi(True)
        f.set_x_p_k_k(seq["x0"], seq["P0"])
        f.set_book(np.tile([0, 0, 2, 2], (N, 1)))
        outs = []
        for t, s in enumerate(seq["steps"]):
            uv, xyz, desc, o = frames[t]
            kw = dict(min_features=100, linearity_index_threshold=0.1, std_pxl=1.0)
            if seeded:
                out = f.map_management_policy_seeded(3 + t, uv, xyz, seed, 3 + t, cand_desc=desc, **kw)
                assert np.array_equal(out.pop("order"), o)
            else:
                out = f.map_management_policy(3 + t, uv[o], xyz[o], desc[:, o], **kw)
                out["accepted"] = o[out["accepted"]]
            f.ekf_prediction(s["u"])
            f.search_IC_matches()
            f.set_measurements(s["meas_idx"], s["z"])
            st = f.step_predicted_seeded(seed, t, N_HYP, threshold=1.0, early_exit=False)
            outs.append((out, st))
        li, hi = f.get_flags()
        state = (f.get_x_k_k(), f.get_p_k_k(), li.copy(), hi.copy(), f.book(), f.get_descriptors(), f.lm_type.copy())
        f.close()
        return outs, state

    (oa, sa), (ob, sb) = run(True), run(False)
    for (pa, ta), (pb, tb) in zip(oa, ob):
        assert ta == tb
        assert all(np.array_equal(pa[k], pb[k]) for k in pa), (pa, pb)
    assert all(np.array_equal(u, v) for u, v in zip(sa, sb))
    assert sum(len(p["accepted"]) for p, _ in oa) > 0 and all(len(p["deleted"]) == 0 for p, _ in oa)


def test_argument_errors_leave_the_context_and_the_book_unchanged(pre3):
    N = 15
    x, P, _ = synth.make_map(N, seed=4)
    f = pre3.EkfFilter(synth.CAM, np.zeros(N, np.int32), dtype="f64", max_landmarks=N + 2)
    f.set_x_p_k_k(x, P)
    with pytest.raises(pre3.Pre3Error) as e:                       # no book
        f.map_management_policy_seeded(3, [[10.0, 10.0]], [[0, 0, 1.0]], 1, 1)
    assert e.value.code == -4                                      # PRE3_E_STATE
    book = np.tile([1, 1, 2, 2], (N, 1))
    f.set_book(book)
    x0, P0 = f.get_x_k_k(), f.get_p_k_k()
    ok_uv, ok_xyz = [[10.0, 10.0]], [[0, 0, 1.0]]
    for uv, xyz, box in (([[np.nan, 10.0]], ok_xyz, (176, 144)), (ok_uv, [[0, 0, 0.0]], (176, 144)), (ok_uv, [[np.inf, 0, 1.0]], (176, 144)),
                         (ok_uv, ok_xyz, (0, 144)), (ok_uv, ok_xyz, (176, -1)), (ok_uv, ok_xyz, (2, 144)), (ok_uv, ok_xyz, (176, 2)),
                         (np.ones((8193, 2)), np.ones((8193, 3)), (176, 144))):
        with pytest.raises(pre3.Pre3Error) as e:
            f.map_management_policy_seeded(3, uv, xyz, 1, 1, box=box)
        assert e.value.code == E_ARG and "pre3_map_policy_seeded" in str(e.value)
    with pytest.raises(pre3.Pre3Error) as e:
        f.map_management_policy_seeded(3, ok_uv, ok_xyz, 1, 1, min_features=1025)
    assert e.value.code == E_ARG
    assert np.array_equal(f.get_x_k_k(), x0) and np.array_equal(f.get_p_k_k(), P0) and np.array_equal(f.book(), book) and f.N == N
    out = f.map_management_policy_seeded(3, np.zeros((0, 2)), np.zeros((0, 3)), 1, 1, min_features=0)      # K = 0 draws nothing
    assert out["order"].shape == (0,) and len(out["accepted"]) == 0
    f.close()
