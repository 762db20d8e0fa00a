"""CPU checks of tests/map_congruence_ref.py (the sparse fp64 restatement of map management's congruence) against the numpy twin and the
C oracle, the input conditions of every case of tests/test_gpu_map_blocks.py, and the measured basis of the fp64 gate (printed)."""
import importlib

import numpy as np
import pytest

import map_congruence_ref as mc
from oracle import np_twin as tw

synth = importlib.import_module("3pre_amd.synth")
G64 = mc.gate("f64")


def _small(orc, N, mixed, seed):
    """A small map; mixed: every third landmark converted by the C oracle first."""
    x, P, _ = synth.make_map(N, seed)
    types = np.zeros(N, np.int32)
    cam = np.array(synth.CAM, float)
    if mixed:
        x, P, types, conv = orc.map_convert(types, x, mc.make_convertible(P, range(1, N, 3)), 1e-3)
        assert 0 < conv.sum() < N
    return types, x, P, cam


def _check(rm, P, Pref, xref, what):
    out, bound = rm.apply(P)
    assert out.shape == Pref.shape, what
    cp = rm.both_copied
    assert np.array_equal(out[cp], rm.copied_from(P)[cp]) and np.array_equal(out[cp], Pref[cp]), what
    w, at = mc.worst(out, Pref, bound, rm.computed)
    assert w <= G64, "%s: %.2f u at %s" % (what, w / mc.U["f64"], at)
    assert np.abs(rm.x_new - xref).max() < 1e-13, what
    return w


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("N", [12, 36, 40])
def test_restatement_against_twin_and_oracle(orc, N, mixed):
    types, x, P, cam = _small(orc, N, mixed, 50 + N)
    off, n = mc.offsets(types)
    # deletion: an exact selection
    dele = [0, N // 2, N // 2 + 1, N - 1]
    rm = mc.RowMap(types, x, P, del_idx=dele)
    assert rm.both_copied.all()
    for ref in (orc.map_delete(types, off, x, P, dele), tw.map_delete(types, off, x, P, dele)):
        assert np.array_equal(rm.apply(P)[0], ref[1]) and np.array_equal(rm.x_new, ref[0]) and np.array_equal(rm.types_new, ref[2])
    # conversion: some inverse-depth landmarks made convertible on top of what converts by itself
    inv = np.nonzero(types == 0)[0][::3]
    Pc = P.copy()
    for i in inv:
        Pc[off[i] + 5, :] *= 1e-3; Pc[:, off[i] + 5] *= 1e-3
    rm = mc.RowMap(types, x, Pc, threshold=0.1)
    assert rm.rel_dist.min() > 1e-6 and rm.conv[inv].all() and rm.conv.sum() < N
    for name, ref in (("oracle", orc.map_convert(types, x, Pc, 0.1)), ("twin", tw.map_convert(types, x, Pc, 0.1))):
        assert np.array_equal(rm.conv, ref[3]) and np.array_equal(rm.types_new, ref[2])
        _check(rm, Pc, ref[1], ref[0], "convert vs " + name)
    # addition
    uvd, rho = mc.new_features(3, 5)
    rm = mc.RowMap(types, x, P, uvd=uvd, rho=rho, cam=cam, std_pxl=1.0)
    assert np.array_equal(rm.lm_src, np.r_[np.arange(N), [-1] * 3]) and len(rm.D) == 3
    for name, ref in (("oracle", orc.map_add(x, P, cam, uvd, 1.0, rho)), ("twin", tw.map_add(x, P, cam, uvd, 1.0, rho))):
        _check(rm, P, ref[1], ref[0], "add vs " + name)
        assert np.array_equal(rm.apply(P)[0][:n, :n], P)


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("N", [12, 36, 40])
def test_composed_map_equals_the_three_in_sequence(orc, N, mixed):
    """map_management's one A (delete + convert + add) against delete, convert, add one after the other: the copies bit for bit, the
    computed entries to the gate (the entries pairing a converted landmark with a new one associate differently), also against the oracle."""
    types, x, P, cam = _small(orc, N, mixed, 70 + N)
    off, n = mc.offsets(types)
    inv = np.nonzero(types == 0)[0][::3]
    P = P.copy()
    for i in inv:
        P[off[i] + 5, :] *= 1e-3; P[:, off[i] + 5] *= 1e-3
    dele = [2, int(inv[1]), N - 1]
    uvd, rho = mc.new_features(3, 6)
    one = mc.RowMap(types, x, P, del_idx=dele, threshold=0.1, uvd=uvd, rho=rho, cam=cam)
    assert one.conv[dele].sum() == 0 and 0 < one.conv.sum() < N
    out, bound = one.apply(P)
    r1 = mc.RowMap(types, x, P, del_idx=dele)
    P1 = r1.apply(P)[0]
    r2 = mc.RowMap(r1.types_new, r1.x_new, P1, threshold=0.1)
    P2 = r2.apply(P1)[0]
    r3 = mc.RowMap(r2.types_new, r2.x_new, P2, uvd=uvd, rho=rho, cam=cam)
    P3 = r3.apply(P2)[0]
    kept = [i for i in range(N) if i not in dele]
    assert np.array_equal(one.conv[kept], r2.conv) and np.array_equal(one.types_new, r3.types_new)
    assert np.abs(one.x_new - r3.x_new).max() < 1e-13
    x1, Q1, t1 = orc.map_delete(types, off, x, P, dele)
    x2, Q2, t2, _ = orc.map_convert(t1, x1, Q1, 0.1)
    x3, Q3 = orc.map_add(x2, Q2, cam, uvd, 1.0, rho)
    for ref in (P3, Q3):
        cp = one.both_copied
        assert np.array_equal(out[cp], ref[cp]) and np.array_equal(out[cp], one.copied_from(P)[cp])
        w, at = mc.worst(out, ref, bound, one.computed)
        assert w <= G64, "%.2f u at %s" % (w / mc.U["f64"], at)
    assert np.abs(one.x_new - x3).max() < 1e-13


def _conditions(rm, N, named, dele=()):
    assert 0 < rm.conv.sum() < N
    assert rm.conv[named].all(), "named landmarks that do not convert: %s" % [i for i in named if not rm.conv[i]]
    assert rm.conv[list(dele)].sum() == 0
    assert rm.rel_dist.min() > 1e-6, "a linearity index sits %.1e (relative) from the threshold" % rm.rel_dist.min()
    same, cross = mc.group_properties(rm)
    assert same and cross


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("size", ["A", "B"])
def test_input_conditions_of_the_conversion_cases(size, dtype):
    N, x0, P0, cam, named = mc.conversion_case(size)
    assert set(mc.straddlers(size)) <= set(named) and {0, N - 1} <= set(named)
    for s, edge in zip(mc.straddlers(size), (1024, 2048)):
        assert 13 + 6 * s < edge <= 13 + 6 * s + 5                         # its six columns straddle the block boundary
    rm = mc.RowMap(np.zeros(N, np.int32), x0, mc.as_stored(P0, dtype), threshold=mc.THRESHOLD)
    _conditions(rm, N, named)


@pytest.mark.parametrize("size,dtype", [("A", "f32"), ("B", "f64"), ("C", "f32")])
def test_input_conditions_of_the_management_cases(size, dtype):
    N, x0, P0, cam, dele, named, uvd, rho = mc.management_case(size)
    cap = mc.SIZES[size][1]
    assert 168 in dele and N - len(dele) + len(uvd) == cap          # (the additions fill the map up to its capacity exactly)
    if size != "A":
        assert 339 in named
    rm = mc.RowMap(np.zeros(N, np.int32), x0, mc.as_stored(P0, dtype), del_idx=dele, threshold=mc.THRESHOLD, uvd=uvd, rho=rho, cam=cam, std_pxl=mc.STD_PXL)
    _conditions(rm, N, named, dele)
    assert len(rm.types_new) == cap


def test_fp64_gate_basis(orc):
    """The measured basis of the fp64 gate: the largest disagreement, in units of bound, between the C oracle and `apply` over the fp64
    cases of tests/test_gpu_map_blocks.py (conversion and addition at A and B, the one-call management at A and B; size C runs in fp32 only)."""
    worst = {}
    for size in ("A", "B"):
        N, x0, P0, cam, named = mc.conversion_case(size)
        types = np.zeros(N, np.int32)
        rm = mc.RowMap(types, x0, P0, threshold=mc.THRESHOLD)
        xo, Po, to, co = orc.map_convert(types, x0, P0, mc.THRESHOLD)
        assert np.array_equal(co, rm.conv)
        out, bound = rm.apply(P0)
        assert np.array_equal(out[rm.both_copied], Po[rm.both_copied])
        worst["convert " + size] = mc.worst(out, Po, bound, rm.computed)[0]
        N, x0, P0, cam = mc.base_map(size)
        for k in sorted({1, 6, mc.SIZES[size][1] - N}):
            uvd, rho = mc.new_features(k, 300 + k)
            rm = mc.RowMap(types, x0, P0, uvd=uvd, rho=rho, cam=cam, std_pxl=mc.STD_PXL)
            xo, Po = orc.map_add(x0, P0, cam, uvd, mc.STD_PXL, rho)
            out, bound = rm.apply(P0)
            assert np.array_equal(out[rm.both_copied], Po[rm.both_copied])
            worst["add %d %s" % (k, size)] = mc.worst(out, Po, bound, rm.computed)[0]
    for size in ("A", "B"):
        N, x0, P0, cam, dele, named, uvd, rho = mc.management_case(size)
        types = np.zeros(N, np.int32)
        rm = mc.RowMap(types, x0, P0, del_idx=dele, threshold=mc.THRESHOLD, uvd=uvd, rho=rho, cam=cam, std_pxl=mc.STD_PXL)
        x1, Q1, t1 = orc.map_delete(types, mc.offsets(types)[0], x0, P0, dele)
        x2, Q2, t2, _ = orc.map_convert(t1, x1, Q1, mc.THRESHOLD)
        x3, Q3 = orc.map_add(x2, Q2, cam, uvd, mc.STD_PXL, rho)
        out, bound = rm.apply(P0)
        assert np.array_equal(out[rm.both_copied], Q3[rm.both_copied]) and np.abs(rm.x_new - x3).max() < 1e-13
        worst["management " + size] = mc.worst(out, Q3, bound, rm.computed)[0]
    u = mc.U["f64"]
    for k, v in worst.items():
        print("fp64 disagreement, C oracle vs apply, %-14s %.3f u" % (k + ":", v / u))
    basis = max(worst.values()) / u
    print("fp64 gate basis: %.3f u (recorded %.2f u); gate = max(32, 8 x recorded) = %.1f u" % (basis, mc.F64_BASIS_U, mc.GATE_U["f64"]))
    assert basis <= mc.F64_BASIS_U, "the recorded basis of the fp64 gate (%.2f u) is below what is measured here (%.3f u)" % (mc.F64_BASIS_U, basis)
