"""GPU: the marginal readers pre3_get_landmarks / pre3_get_marginal (EkfFilter.landmarks / .marginal / .pose) -- what
plots_complete.m:161-237 and inversedepth_2_cartesian.m:36-62 read of x and P, without copying P to the host.  Against get_state on the SR4000
fixture (fp64 bit for bit, fp32 as stored) and the numpy truth of tests/test_marginals_ref.py; on the headline's chained steps with the HI update
deferred and its down-date pending (PRE3_OPT_PEND_HI), a read between the steps must not change the filter's trajectory by a bit, and must see
P - W~'W~."""
import importlib

import numpy as np
import pytest

from test_marginals_ref import landmark_truth

pytestmark = pytest.mark.gpu
synth = importlib.import_module("3pre_amd.synth")


def _offsets(types):
    off, o = np.zeros(len(types), int), 13
    for i, t in enumerate(types):
        off[i] = o
        o += 6 if int(t) == 0 else 3
    return off


def _blocks(P, types, off):
    out = np.zeros((len(types), 6, 6))
    for i, (t, o) in enumerate(zip(types, off)):
        d = 6 if int(t) == 0 else 3
        out[i, :d, :d] = P[o:o + d, o:o + d]
    return out


def _rel(a, b, axes):
    """max over landmarks of |a - b| relative to each landmark's own scale (the largest entry of b's block)"""
    sc = np.maximum(np.abs(b).max(axis=axes), 1e-300)
    return (np.abs(a - b).max(axis=axes) / sc).max()


def _sr4000_filter(pre3, d, dtype, which):
    f = pre3.EkfFilter(d["cam"], np.zeros(d["N"], np.int32), dtype=dtype, max_hyp=8, std_z=d["std_z"])
    if which == 0:
        f.set_x_p_k_k(d["x_k_k"], d["p_k_k"])
    else:
        f.set_x_p_k_km1(d["x_k_km1"], d["p_k_km1"])
    return f


@pytest.mark.parametrize("which", [0, 1])
def test_sr4000_fp64_blocks_are_those_of_P_and_the_geometry_is_the_reference(pre3, which):
    import util
    d = util.load_sr4000()
    f = _sr4000_filter(pre3, d, "f64", which)
    X, P = (d["x_k_k"], d["p_k_k"]) if which == 0 else (d["x_k_km1"], d["p_k_km1"])
    L = f.landmarks(which)
    xv, Pv = f.pose(which)
    xg, Pg = f._get(which)
    f.close()
    types, off = np.zeros(d["N"], int), _offsets(np.zeros(d["N"], int))
    assert L["xyz"].shape == (d["N"], 3) and L["cov_xyz"].shape == (d["N"], 3, 3) and L["cov_native"].shape == (d["N"], 6, 6)
    assert np.array_equal(L["cov_native"], _blocks(Pg, types, off))
    assert np.array_equal(xv, xg[:7]) and np.array_equal(Pv, Pg[:7, :7])
    t = landmark_truth(X, P, types, off)
    assert _rel(L["xyz"], t["xyz"], 1) < 1e-12
    assert _rel(L["cov_xyz"], t["cov_xyz"], (1, 2)) < 1e-12
    assert (np.abs(L["linearity"] - t["linearity"]) / np.abs(t["linearity"])).max() < 1e-12
    assert np.array_equal(L["cov_xyz"], L["cov_xyz"].transpose(0, 2, 1))


def test_sr4000_fp32_blocks_are_the_stored_fp32_entries(pre3):
    import util
    d = util.load_sr4000()
    types, off = np.zeros(d["N"], int), _offsets(np.zeros(d["N"], int))
    for which, X, P in ((0, d["x_k_k"], d["p_k_k"]), (1, d["x_k_km1"], d["p_k_km1"])):
        f = _sr4000_filter(pre3, d, "f32", which)
        L = f.landmarks(which)
        xv, Pv = f.pose(which)
        f.close()
        P32 = P.astype(np.float32).astype(np.float64)
        assert np.array_equal(L["cov_native"], _blocks(P32, types, off))
        assert np.array_equal(xv, X[:7]) and np.array_equal(Pv, P32[:7, :7])
        t = landmark_truth(X, P32, types, off)
        assert _rel(L["cov_xyz"], t["cov_xyz"], (1, 2)) < 1e-12


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_mixed_map_cartesian_landmarks_and_the_conversion_decision(pre3, dtype):
    import util
    d = util.load_sr4000()
    f = _sr4000_filter(pre3, d, dtype, 0)
    lin0 = f.landmarks()["linearity"]
    thr = float(np.quantile(lin0, 0.4))                   # about 40 % of the landmarks convert
    conv = f.inversedepth_2_cartesian(thr)
    assert 0 < conv.sum() < d["N"]
    if dtype == "f64":
        assert np.array_equal(conv.astype(bool), lin0 < thr)       # the reader's index is the number the conversion compares
    L = f.landmarks()
    xg, Pg = f.get_x_k_k(), f.get_p_k_k()
    types = f.lm_type.copy()
    f.close()
    assert np.array_equal(types == 1, conv.astype(bool))
    off = _offsets(types)
    cart = np.nonzero(types == 1)[0]
    assert np.array_equal(L["linearity"][cart], -np.ones(len(cart)))
    assert np.array_equal(L["xyz"][cart], np.stack([xg[o:o + 3] for o in off[cart]]))
    assert np.array_equal(L["cov_xyz"][cart], np.stack([Pg[o:o + 3, o:o + 3] for o in off[cart]]))
    assert np.array_equal(L["cov_native"], _blocks(Pg, types, off))          # Cartesian: 3x3 top-left, the rest 0
    idl = np.nonzero(types == 0)[0]
    t = landmark_truth(xg, Pg, types, off)
    assert _rel(L["xyz"][idl], t["xyz"][idl], 1) < 1e-12
    assert _rel(L["cov_xyz"][idl], t["cov_xyz"][idl], (1, 2)) < 1e-12
    assert (L["linearity"][idl] >= thr).all()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("k", [1, 7, 50, 1024])
def test_marginal_on_random_index_sets(pre3, dtype, k):
    import util
    d = util.load_sr4000()
    f = _sr4000_filter(pre3, d, dtype, 0)
    xg, Pg = f.get_x_k_k(), f.get_p_k_k()
    rng = np.random.default_rng(k)
    idx = rng.integers(0, d["n"], k)
    if k > 1:
        idx[rng.choice(k, min(k, 5), replace=False)] = rng.integers(0, 7, min(k, 5))       # pose entries: cross terms
    if k > 7:
        idx[-3:] = idx[:3]                                                                 # repeats
    xv, Pv = f.marginal(idx)
    f.close()
    assert Pv.shape == (k, k)
    assert np.array_equal(xv, xg[idx]) and np.array_equal(Pv, Pg[np.ix_(idx, idx)])


def _headline(N=500, steps=4, n_hyp=200, n_rescued=None):
    from oracle import np_twin as tw
    import oracle as orc
    from test_gpu_tail import _with_n_rescued
    seq = synth.make_sequence(N, steps, n_hyp, motion_noise=synth.HEADLINE["motion_noise"])
    z0 = None
    if n_rescued is not None:
        types, off, n = orc.landmark_table(np.zeros(N, int))
        z0, _ = _with_n_rescued(tw, types, off, seq, seq["steps"][0], n_rescued)      # step 0 rescues exactly n_rescued landmarks
    return seq, z0


def _chain(pre3, seq, z0, n_hyp, pend, read=None):
    N = seq["x0"].shape[0] - 13
    N //= 6
    f = pre3.EkfFilter(seq["cam"], np.zeros(N, np.int32), dtype="f32", max_hyp=n_hyp, std_z=1.0)
    f.defer_hi_update(True)
    assert f.pend_hi(pend) == pend
    f.set_x_p_k_k(seq["x0"], seq["P0"])
    stats, reads = [], []
    for i, s in enumerate(seq["steps"]):
        z = z0 if (i == 0 and z0 is not None) else s["z"]
        st = f.step(s["u"], s["meas_idx"], z, s["hyp"], threshold=synth.HEADLINE["threshold"], early_exit=False)
        stats.append(tuple(sorted(st.items())))
        if read is not None:
            reads.append(read(f))
    out = (f.get_flags(), f.get_x_k_k(), f.get_p_k_k(), stats, reads)
    f.close()
    return out


@pytest.mark.parametrize("n_rescued", [1, 33, 64])
def test_reading_between_steps_does_not_perturb_the_filter(pre3, n_rescued):
    n_hyp = 200
    seq, z0 = _headline(n_rescued=n_rescued)
    a = _chain(pre3, seq, z0, n_hyp, True, read=lambda f: (f.pose(), f.landmarks()))
    b = _chain(pre3, seq, z0, n_hyp, True)
    assert a[3] == b[3]
    assert any(dict(s)["n_hi"] > 0 for s in b[3])
    assert dict(b[3][1])["n_hi"] == n_rescued                         # (deferred: step 1 reports step 0's count)
    assert all(np.array_equal(u, v) for u, v in zip(a[0], b[0]))
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def _read_then_flush(idx):
    def read(f):
        L, (xv, Pv) = f.landmarks(), f.marginal(idx)
        xp, Pp = f.pose()
        x, P = f.get_x_k_k(), f.get_p_k_k()                           # completes what is pending
        L2, (xv2, Pv2) = f.landmarks(), f.marginal(idx)
        return L, xv, Pv, xp, Pp, x, P, L2, xv2, Pv2
    return read


@pytest.mark.parametrize("n_rescued", [1, 33, 64])
def test_the_pending_downdate_is_applied_by_the_reading_launch(pre3, n_rescued):
    n_hyp = 200
    seq, z0 = _headline(n_rescued=n_rescued)
    N = 500
    rng = np.random.default_rng(n_rescued)
    n = 13 + 6 * N
    idx = np.concatenate([np.arange(7), rng.integers(0, n, 43), [3, 5, 13 + 6 * 7 + 5]])
    rng.shuffle(idx)
    *_, reads = _chain(pre3, seq, z0, n_hyp, True, read=_read_then_flush(idx))
    types, off = np.zeros(N, int), _offsets(np.zeros(N, int))
    for L, xv, Pv, xp, Pp, x, P, L2, xv2, Pv2 in reads:
        sc = np.abs(P).max()
        assert np.abs(L["cov_native"] - _blocks(P, types, off)).max() < 1e-5 * sc
        assert np.abs(Pv - P[np.ix_(idx, idx)]).max() < 1e-5 * sc and np.array_equal(xv, x[idx])
        assert np.abs(Pp - P[:7, :7]).max() < 1e-5 * sc and np.array_equal(xp, x[:7])
        t = landmark_truth(x, P, types, off)
        assert _rel(L["cov_xyz"], t["cov_xyz"], (1, 2)) < 1e-4
        assert np.array_equal(L["xyz"], L2["xyz"])                      # x is final once the deferred update is complete
        # nothing pending any more: the stored fp32 entries
        assert np.array_equal(L2["cov_native"], _blocks(P, types, off))
        assert np.array_equal(Pv2, P[np.ix_(idx, idx)]) and np.array_equal(xv2, x[idx])


def test_deferred_hi_update_without_the_pending_form(pre3):
    """defer_hi_update(True) only: the read completes the deferred update and leaves its rows/cols 3..6 pass to the next prediction's launch, applying
    it itself -- value for value as k_jnorm_P then stores it"""
    n_hyp = 200
    seq, z0 = _headline(n_rescued=18)
    N, n = 500, 13 + 6 * 500
    idx = np.concatenate([np.arange(13), [13, 20, n - 1], np.arange(6, 2, -1)])
    *_, reads = _chain(pre3, seq, z0, n_hyp, False, read=_read_then_flush(idx))
    types, off = np.zeros(N, int), _offsets(np.zeros(N, int))
    for L, xv, Pv, xp, Pp, x, P, L2, *_ in reads:
        assert np.array_equal(L["cov_native"], _blocks(P, types, off))
        assert np.array_equal(Pv, P[np.ix_(idx, idx)]) and np.array_equal(xv, x[idx])
        assert np.array_equal(Pp, P[:7, :7]) and np.array_equal(xp, x[:7])
        assert np.array_equal(L["xyz"], L2["xyz"]) and np.array_equal(L["cov_xyz"], L2["cov_xyz"])
    # the chain with reads is the chain without
    a = _chain(pre3, seq, z0, n_hyp, False, read=lambda f: (f.pose(), f.landmarks()))
    b = _chain(pre3, seq, z0, n_hyp, False)
    assert a[3] == b[3] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_errors(pre3):
    import util
    d = util.load_sr4000()
    f = _sr4000_filter(pre3, d, "f64", 0)
    for bad in (lambda: f.landmarks(which=2), lambda: f.marginal([0], which=-1)):
        with pytest.raises(pre3.Pre3Error) as e:
            bad()
        assert e.value.code == -1
    for bad in (lambda: f.landmarks(first=d["N"] - 2, count=3), lambda: f.landmarks(first=-1, count=1), lambda: f.marginal([0, d["n"]]),
                lambda: f.marginal([-1])):
        with pytest.raises(pre3.Pre3Error) as e:
            bad()
        assert e.value.code == -1
    assert f.landmarks(first=d["N"], count=0)["xyz"].shape == (0, 3)
    f.set_x_p_k_km1(d["x_k_km1"], d["p_k_km1"])                 # the buffer now holds p_k_km1
    with pytest.raises(pre3.Pre3Error) as e:
        f.landmarks(which=0)
    assert e.value.code == -4 and "other estimate" in str(e.value)
    with pytest.raises(pre3.Pre3Error) as e:
        f.pose(which=0)
    assert e.value.code == -4
    assert f.landmarks(which=1)["xyz"].shape == (d["N"], 3)
    f.close()
    # N = 0: no landmarks, the pose is read as get_state reads it
    seq = synth.make_sequence(4, 1, 8, seed=3)
    f = pre3.EkfFilter(seq["cam"], np.zeros(0, np.int32), dtype="f32", max_hyp=8)
    f.set_x_p_k_k(seq["x0"][:13], seq["P0"][:13, :13])
    L = f.landmarks()
    assert L["xyz"].shape == (0, 3) and L["linearity"].shape == (0,)
    xv, Pv = f.pose()
    assert np.array_equal(xv, f.get_x_k_k()[:7]) and np.array_equal(Pv, f.get_p_k_k()[:7, :7])
    f.close()
