"""CPU suite: the restatements, inputs and gates that tests/test_gpu_k9_alone.py holds the down-date kernels to (tests/k9_ref.py,
tests/golden/k9_tolerance.json).  No device, no library: what is checked here is that the yardstick itself is sound -- the exact class is
exact in every form, the gate comes from the plain restatement and is reproduced, the emulation of the bf16 form passes it and each of its
three mutants misses it by at least a factor of two where the plan requires that (r <= 64)."""
import importlib
import json
import os
import sys

import numpy as np
import pytest

import k9_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATES = json.load(open(os.path.join(ROOT, "tests", "golden", "k9_tolerance.json")))


@pytest.fixture(scope="module")
def gen():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    return importlib.import_module("make_k9_tolerance")


@pytest.fixture(scope="module")
def table(gen):
    """emulation and mutants on every committed f32 accuracy input, computed once"""
    return gen.emulation_table(GATES)


def test_the_restated_sizes():
    assert [R.state_size(N) for N, _ in R.SHAPES] == [61, 67, 127, 133, 259, 133]
    assert [R.ld_of(c) for _, c in R.SHAPES] == [128, 128, 128, 256, 384, 384] and R.ld_of(468) == 2944 and R.ld_of(340) == 2176
    assert [R.nst_of(r) for r in R.ROWS] == [4, 4, 4, 4, 4, 6, 6, 8, 10] and R.nst_of(192) == 12 and R.nst_of(518) == 34
    assert R.tiles128(468, 256) == (256, 20 * 3) and R.tiles128(41, 256) == (6, 0) and R.tiles128(460, 256)[1] == 0
    assert R.tiles64(340) == 595 and 2 * 256 < 595 <= 5 * 256
    assert R.admitted(20, R.ROWS) == list(R.ROWS[:-1]) and R.admitted(41, R.ROWS) == list(R.ROWS) and R.rcap_of(41) == 192


def test_every_group_has_its_cases():
    seen = set()
    for g, dt in R.GROUPS:
        cs = R.group_cases(g, dt)
        assert cs and all(R.round_up(c["r"], 64) <= R.rcap_of(c["cap"]) and c["n"] == R.state_size(c["N"]) for c in cs)
        assert {c["cls"] for c in cs} == {"exact", "acc"}
        seen |= {(g, c["r"], c["launches"]) for c in cs}
    assert {r for g, r, L in seen if g == "default"} == set(R.ROWS) | {192}
    assert {(r, L) for g, r, L in seen if g == "persist"} == {(1, 1), (1, 3), (65, 1), (65, 3), (129, 1), (129, 3)}
    assert {r for g, r, L in seen if g in ("small_tiles", "f64_1t16")} == {33, 65}
    assert sorted(R.accuracy_keys()) == sorted(GATES["cases"])


def test_the_exact_class_stays_below_2_to_the_24_and_every_restatement_hits_it():
    done = set()
    for g, dt in R.GROUPS:
        for c in R.group_cases(g, dt):
            k = (c["n"], c["r"], c["launches"], c["planes"])
            if c["cls"] != "exact" or k in done:
                continue
            done.add(k)
            P0, W = R.inputs(c)
            assert R.exact_bound(P0, W, c["launches"]) < 2 ** 24, k
            assert np.array_equal(W, np.rint(W)) and np.array_equal(P0, np.rint(P0)) and np.array_equal(P0, P0.T)
            assert np.abs(W).max() <= (255 if c["planes"] == 1 else 511)
            a, b, cc = R.split3(W)
            if c["planes"] == 1:
                assert not b.any() and not cc.any()
            else:
                assert c["r"] <= 64 and (np.abs(W[np.abs(W) > 255]) % 2 == 1).all() and b.any() and not cc.any()
            want = R.exact(P0, W, c["launches"])
            if c["n"] > 300 and c["planes"] == 1 and c["r"] == 65:
                continue                                                   # (the large inputs: one of each state size is enough for the restatements)
            assert np.array_equal(R.plain(P0, W, c["launches"], "f32"), want), k
            assert np.array_equal(R.emulate_b3(P0, W, c["launches"]), want), k
            if c["n"] < 300:
                assert np.array_equal(R.plain(P0, W, c["launches"], "f64"), want), k
    assert len(done) >= 80


def test_bf16_rounds_to_nearest_even_and_the_split_is_exact():
    x = np.array([1.0, 1.00390625, 1.01171875, 257.0, 259.0, -1.00390625, 0.0, 1.0078125], np.float32)     # 1 + 2^-8: a tie, to even (down); 1 + 3 * 2^-8: a tie, up
    assert R.bf16_rne(x).tolist() == [1.0, 1.0, 1.015625, 256.0, 260.0, -1.0, 0.0, 1.0078125]
    w = np.random.default_rng(3).standard_normal(4096).astype(np.float32) * np.float32(37.0)
    a, b, c = R.split3(w)
    for p in (a, b, c):
        assert not (p.view(np.uint32) & 0xFFFF).any()
    assert np.array_equal(a.astype(np.float64) + b + c, w.astype(np.float64))                          # 8 + 8 + 8 bits: nothing of an f32 is lost


def test_the_two_wide_references_agree():
    P0, W = R.accuracy_case(67, 33, 3, "f64")
    hi, lo = R.exact_wide(P0, W, 3)
    h2, l2 = R.exact_wide(P0, W, 3, force_error_free=True)
    den = R.denominator(P0, W, 3)
    assert (np.abs((hi - h2) + (lo - l2)) <= 0.1 * R.U64 * den).all()
    assert (np.abs(hi - R.exact(P0, W, 3)) <= 40 * R.U64 * den).all() and (np.abs(lo) <= R.U64 * np.abs(hi)).all()


def test_norm_err_leaves_no_entry_out():
    P0, W = R.accuracy_case(61, 2, 1, "f32")
    want = R.exact(P0, W, 1)
    den = R.denominator(P0, W, 1)
    assert R.norm_err(want, P0, W, 1, R.U32) == (0.0, 0.0)
    for i, j in ((0, 0), (60, 60), (0, 60), (60, 0), (17, 44)):
        got = want.copy()
        got[i, j] += 3.0 * R.U32 * den[i, j]
        mx, rms = R.norm_err(got, P0, W, 1, R.U32)
        assert abs(mx - 3.0) < 1e-6 and abs(rms - 3.0 / 61) < 1e-6
    zero_cols = np.nonzero(~W.any(axis=0))[0]
    assert len(zero_cols) == 2 and (np.abs(P0[zero_cols]) > 0).all()          # the rows of P0 the device must hand back untouched
    assert sum(1 for k in range(2) if not W[k].any()) == 1


def test_the_committed_tolerance_is_reproduced(gen):
    assert GATES["factor"] == gen.FACTOR == 6
    got = gen.measure()["cases"]
    assert sorted(got) == sorted(GATES["cases"])
    for k, w in GATES["cases"].items():
        g = got[k]
        rel = 1e-6 if w["dtype"] == "f32" else 0.1        # (f64: the wide reference is long double here and error-free sums elsewhere, 2^-11 u apart)
        for f in ("plain_max", "plain_rms"):
            assert abs(g[f] - w[f]) <= rel * w[f], (k, f, g[f], w[f])
        assert w["gate_max"] == min(6 * w["plain_max"], w["r"] + 8) and w["gate_rms"] == min(6 * w["plain_rms"], w["r"] + 8)
        assert 0 < w["plain_rms"] <= w["plain_max"] and w["gate_max"] <= w["r"] + 8, k


def test_the_emulation_passes_the_gate_and_every_mutant_misses_it_twofold(table):
    assert len(table) >= 50 and set(R.MUTANTS) == {"no(0,2)", "no(1,1)", "no third plane"}
    n_small = 0
    for k, row in table.items():
        g = GATES["cases"][k]
        mx, rms = row["emulation"]
        assert mx <= g["gate_max"] and rms <= g["gate_rms"], (k, mx, rms, g)
        if g["r"] > 64:
            continue
        n_small += 1
        for name in R.MUTANTS:
            mx, rms = row[name]
            assert mx >= 2 * g["gate_max"] and rms >= 2 * g["gate_rms"], (k, name, mx, rms, g)
    assert n_small >= 30
