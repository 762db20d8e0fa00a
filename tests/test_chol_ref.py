"""CPU suite: the restatements, inputs and gates that tests/test_gpu_chol_alone.py holds the factorisation and solve to (tests/chol_ref.py,
tests/golden/chol_tolerance.json).  No device, no library: what is checked here is that the yardstick itself is sound -- the exact class is
exact in every restatement and inside its bounds, the gate comes from `plain` and `blocked` and is reproduced, `blocked` does not leave
`plain`'s figures, the emulation of the persistent form passes the gate and each of its three mutants misses it at least twofold."""
import importlib
import json
import os
import sys

import numpy as np
import pytest

import chol_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATES = json.load(open(os.path.join(ROOT, "tests", "golden", "chol_tolerance.json")))
SMALL = 192                 # the rows up to which every case is redone here; of the larger ones, one per dtype


@pytest.fixture(scope="module")
def gen():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    return importlib.import_module("make_chol_tolerance")


def test_the_restated_sizes_and_form_selection():
    assert [R.state_size(N) for N, _ in R.CONTEXTS] == [31, 133, 589, 253]
    assert [R.ld_of(c) for _, c in R.CONTEXTS] == [128, 640, 640, 3200] and [R.rcap_of(c) for _, c in R.CONTEXTS] == [128, 256, 256, 1152]
    assert R.ldw_of(520) // 32 == 102 and R.ldw_of(520) // 64 == 51
    assert all(R.round_up(r, 64) <= R.rcap_of(cap) for (N, cap), rows in R.ROWS.items() for r in rows)
    assert [R.early_panel(r) for r in (56, 57, 120, 121, 64, 1, 1000)] == [56, 0, 56, 0, 0, 1, 40]
    assert R.cholp_takes(16, 520, 256) and not R.cholp_takes(17, 520, 256) and not R.cholp_takes(1, 96, 256) and R.cholp_takes(1, 96, 256, True)
    assert R.cholp_takes(2, 8, 256) and not R.cholp_takes(3, 8, 256) and R.cholp_stride(14, 256) == 8 and R.cholp_stride(14, 104) == 7 and R.cholp_stride(14, 8) == 0
    # the trailing sweeps on 256 CUs with PRE3_CHOL_TRAIL_SPLIT=1: 11 panels stay under the threshold (504 tiles against 512), 15 and 16 do not
    assert R.trail_plan(11, 520, 256, 1, 4) == ([], {}, []) and R.trail_plan(11, 520, 256, 1, 1) == ([], {}, [])
    assert R.trail_plan(15, 520, 256, 1, 1) == ([1, 2, 3, 4], {}, [])
    assert R.trail_plan(15, 520, 256, 1, 4) == ([], {1: 1, 2: 2, 3: 3, 4: 4, 5: 1, 6: 2, 7: 3, 8: 4}, [3, 7])
    assert R.trail_plan(16, 520, 256, 1, 4)[1] == {J: (4 if J % 4 == 0 else J % 4) for J in range(1, 9)} and R.trail_plan(16, 520, 256, 1, 4)[2] == [3, 7]
    assert R.trail_plan(16, 520, 256, 4, 4) == ([], {}, [])


def test_every_group_has_its_cases():
    rows = {g: {c["r"] for c in R.group_cases(g, "f32")} for g in ("cholp", "cholp1", "step", "trail")}
    assert rows["step"] == {1, 7, 8, 9, 56, 57, 63, 64, 65, 120, 121, 127, 128, 129, 192, 768, 832, 1000, 1024, 1025, 1152}
    assert rows["cholp"] == {65, 120, 121, 127, 128, 129, 192, 768, 832, 1000, 1024} and rows["cholp1"] == {1, 7, 8, 9, 56, 57, 63, 64}
    assert rows["trail"] == {704, 960, 1024}
    for g in rows:
        cs = R.group_cases(g, "f32")
        assert {c["cls"] for c in cs} == {"exact", "acc"} and all(c["n"] == R.state_size(c["N"]) for c in cs)
        assert {c["r"] for c in cs if c["cls"] == "exact"} == {r for r in rows[g] if r <= R.EXACT_MAX_R}
        assert {(c["r"], c["kappa"]) for c in cs if c["cls"] == "acc"} == {(r, k) for r in rows[g] for k in R.KAPPAS}
    assert sorted(R.accuracy_keys()) == sorted(GATES["cases"])


def test_the_exact_class_keeps_its_bounds_and_every_restatement_hits_it():
    done = 0
    for c in R.group_cases("step", "f32") + R.group_cases("trail", "f32"):
        if c["cls"] != "exact":
            continue
        S, B, nu, L0, W0 = R.exact_case(c["n"], c["r"])
        b = R.exact_bounds(L0, W0)
        assert b["sums"] < 2 ** 24 and b["operands"] < 2 ** 16, (c, b)
        r = c["r"]
        assert np.array_equal(np.diag(L0), np.ones(r)) and np.array_equal(L0, np.tril(L0)) and np.array_equal(L0, np.rint(L0))
        off = L0 - R.block_inverse(R.block_inverse(L0))
        assert np.abs(off).max(initial=0) <= 2 and np.abs(W0).max() <= 255 and np.array_equal(W0, np.rint(W0))
        assert np.array_equal(S, L0 @ L0.T) and np.array_equal(np.concatenate([B, nu[:, None]], axis=1), L0 @ W0)
        assert (~W0[:, :-1].any(axis=0)).sum() >= 2
        for M in (R.block_inverse(L0),):
            assert set(np.unique(M)) <= {-1.0, 0.0, 1.0}
        a, bb, cc = R.split3(np.concatenate([S.ravel(), B.ravel(), nu, W0.ravel(), L0.ravel()]))
        assert not cc.any()                                                 # two bf16 planes hold every operand
        if r <= SMALL or r == 832:
            for dt in ("f32", "f64") if r <= SMALL else ("f32",):
                for f in (R.plain, R.blocked):
                    L, W = f(S, B, nu, dt)
                    assert np.array_equal(L, L0) and np.array_equal(W, W0), (c, f.__name__, dt)
            if r <= SMALL:
                L, W = R.emulate_cholp(S, B, nu)
                assert np.array_equal(L, L0) and np.array_equal(W, W0), c
        assert R.judge(c, L0, np.concatenate([W0, np.zeros((R.round_up(r, 64) - r, c["n"] + 1))]), {}) == ([], {})
        done += 1
    assert done >= 30


def test_the_wide_product_is_finer_than_fp64_entry_by_entry():
    rng = np.random.default_rng(4)
    A = rng.standard_normal((40, 300)) * np.logspace(-6, 6, 300) * np.logspace(3, -3, 40)[:, None]
    B = rng.standard_normal((300, 30)) * np.logspace(5, -5, 300)[:, None]
    hi, lo, left = R.wide_matmul(A, B)
    ld = np.longdouble
    ref = A.astype(ld) @ B.astype(ld)
    den = np.abs(A) @ np.abs(B)
    assert (np.abs((hi.astype(ld) - ref) + lo).astype(np.float64) <= 2.0 ** -60 * den + 300 * 2.0 ** -64 * den).all()     # (long double itself: 64 bits)
    assert (left <= 2.0 ** -60 * den).all()


def test_the_figures_leave_no_entry_out_and_hold_the_zero_rule():
    S, B, nu = R.accuracy_case(31, 9, 10, "f32")
    L, W = R.plain(S, B, nu, "f32")
    base, bad = R.figures(L, W, S, B, nu, "f32")
    assert not bad and all(0 < base[k] < 20 for k in R.FIGS)
    zc = np.nonzero(~B.any(axis=0))[0]
    assert len(zc) == 2 and not W[:, zc].any()
    for i, j in ((0, 0), (8, 8), (8, 0), (4, 2)):
        L2 = L.copy(); L2[i, j] *= 1 + 1e-3
        assert R.figures(L2, W, S, B, nu, "f32")[0]["e1_max"] > 1e3
    for i, j in ((0, 0), (8, 31), (8, 0), (0, 31), (5, 17)):
        if j in zc:
            continue
        W2 = W.copy(); W2[i, j] *= 1 + 1e-3
        assert R.figures(L, W2, S, B, nu, "f32")[0]["e2_max"] > 1e3
    L2 = L.copy(); L2[2, 7] = 1e9                                               # above the diagonal: not judged
    assert R.figures(L2, W, S, B, nu, "f32")[0] == base
    W2 = W.copy(); W2[3, zc[0]] = 1e-30
    assert R.figures(L, W2, S, B, nu, "f32")[1]                                    # a zero column must come back as zeros
    c = dict(N=3, cap=8, n=31, r=9, cls="acc", kappa=10, dtype="f32")
    Wp = np.concatenate([W, np.zeros((55, 32))])
    assert R.judge(c, L, Wp, GATES["cases"])[0] == []
    Wp[20, 3] = 1e-20
    assert R.judge(c, L, Wp, GATES["cases"])[0]                                   # the padded rows of W must be zero


def _redone(key):
    g = GATES["cases"][key]
    return g["r"] <= SMALL or key in ("n253_r832_k1000_f32", "n253_r832_k10_f64")


def test_the_committed_tolerance_is_reproduced_and_blocked_stays_inside_plain(gen):
    assert GATES["factor"] == gen.FACTOR == 6
    n = 0
    for key, w in GATES["cases"].items():
        for f in R.FIGS:
            assert w["gate"][f] == 6 * max(w["plain"][f], w["blocked"][f]) and 0 < w["plain"][f] and 0 < w["blocked"][f]
        assert w["plain"]["e1_rms"] <= w["plain"]["e1_max"] and w["plain"]["e2_rms"] <= w["plain"]["e2_max"]
        # blocked does not leave plain's figures: from two panels on it is inside all four.  Below, where M_J is one rounding more among few (three
        # against two at r = 1), its RMS stays within that ratio of 1.5 and its maxima -- over as few as 32 entries -- within 3, twice that
        for f in R.FIGS:
            lim = 1.0 if w["r"] >= 120 else (3.0 if f.endswith("max") else 1.5)
            assert w["blocked"][f] <= lim * w["plain"][f], (key, f, w["blocked"][f], w["plain"][f])
        if not _redone(key):
            continue
        n += 1
        got = gen.measure_one(w["n"], w["r"], w["kappa"], w["dtype"])
        # plain is elementwise arithmetic on a reproducible input; blocked in f32 rounds fp64 matrix products once, and a BLAS that sums in another
        # order may flip one of those roundings (the fp64 cases go through the error-free product)
        for which, rel in (("plain", 1e-6), ("blocked", 1e-6 if w["dtype"] == "f64" else 1e-2)):
            for f in R.FIGS:
                assert abs(got[which][f] - w[which][f]) <= rel * w[which][f], (key, which, f, got[which][f], w[which][f])
    assert n >= 100


def test_the_emulation_passes_the_gate_and_every_mutant_misses_it_twofold():
    seen, n = set(), 0
    for key, w in GATES["cases"].items():
        if w["dtype"] != "f32" or w["r"] > SMALL:
            continue
        S, B, nu = R.accuracy_case(w["n"], w["r"], w["kappa"], "f32")
        L, W = R.emulate_cholp(S, B, nu)
        fig, bad = R.figures(L, W, S, B, nu, "f32")
        assert not bad and all(fig[f] <= w["gate"][f] for f in R.FIGS), (key, fig, w["gate"])
        for name, kw in R.mutants(w["r"], w["n"]).items():
            Lm, Wm = R.emulate_cholp(S, B, nu, **kw)
            fm, _ = R.figures(Lm, Wm, S, B, nu, "f32")
            assert max(fm[f] / w["gate"][f] for f in R.FIGS) >= 2, (key, name, fm, w["gate"])
            seen.add(name)
        n += 1
    assert n >= 40 and seen == {"strips drop (0,2)", "tile misses a rank-64 update", "strip misses L(J,K) W_K"}
