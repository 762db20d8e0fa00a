"""The factorisation and solve of the graded update -- update.m:32-33, S = L L' and W = L^-1 [HP | nu] -- on their own, entry by entry, in every form.

Every other check of these kernels goes through a whole update or step and holds P to 1e-4 .. 3e-4 of max|P| and x to 1e-5, or compares one
form's digest with another's.  A strip that skips one L(J,K) W_K block, a row that misses one rank-64 update of one tile or a dropped plane
product passes that wherever max|P| is set elsewhere, and the f32 image of L and the bf16 planes of W the factorisation writes were compared
with nothing.  Here the test hook EkfFilter.test_factor_solve hands an S, B and nu of the test's own to launch_chol_solve and nothing else
runs (mode 0), or only the down-date behind it (mode 1).  Per case (tests/chol_ref.py):

  * exact class (unit-triangular integer L0, integer W0, every sum below 2^24, every matrix-core operand below 2^16): L and W equal L0 and W0
    bit for bit, in either dtype;
  * accuracy class (cond(S) about 2e4 and 2e6): E1 = |L L' - S| / (u |L||L|') over the lower triangle and E2 = |L W - [B | nu]| / (u |L||W|) over
    every entry, from the device's own L and W, inside the gate of tests/golden/chol_tolerance.json on maximum and RMS -- 6 x the larger of the
    two CPU restatements' figures; a zero column of B comes back as zeros;
  * rows r .. r_pad-1 of W are zero, and mode 0 leaves P bitwise untouched;
  * mode 1: P from the consumers inside k_cholp, from k_downdate_b3 on the planes the strips wrote and from the pinned K9 on k_split_w's planes of
    the same W are bitwise equal; likewise for the launch-per-panel form's planes (chol_store_w_strip).

r sits on either side of the chain's 8-row sub-panel, of the `early` rule (at most 56 real rows in the last panel), of the panel edges, of the
strips' ring of 11 plane blocks (12 and 13 panels), at CP_MAX_NRB = 16 panels and beyond it.  Measured figures: profiles/chol_alone_accuracy.txt.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import chol_ref as R
import chol_worker as K
import k9_ref as K9

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESULTS = []                # (form, result) of every case that ran, for the report
TRIPLES = []                # (context, r, what) of the mode-1 comparisons


@pytest.fixture(autouse=True)
def _test_hooks_on(monkeypatch):
    """the hook is inert unless the environment enables it (3pre_amd/csrc/pre3_test_hooks.h)"""
    monkeypatch.setenv("PRE3_TEST_HOOKS", "1")


@pytest.fixture(scope="module", autouse=True)
def _report():
    """CHOL_ALONE_REPORT=<file>: the measured figures of every accuracy case, next to the restatements' (profiles/chol_alone_accuracy.txt is one)"""
    yield
    path = os.environ.get("CHOL_ALONE_REPORT")
    if path and RESULTS:
        with open(path, "w") as fh:
            fh.write("# factorisation and solve alone: E1 = |L L' - S|_ij / (u (|L||L|')_ij), lower triangle; E2 = |L W - [B | nu]|_ij / (u (|L||W|)_ij), every entry;\n")
            fh.write("# u = 2^-24 (f32) / 2^-53 (f64); max / RMS per figure.  plain, blocked: the CPU restatements (tests/chol_ref.py); gate = 6 x the larger\n")
            fh.write("# %-38s %4s %5s %5s %4s   %-27s   %-27s   %-27s   %-27s\n" % ("form", "n", "r", "kappa", "type", "device E1 max/rms E2 max/rms", "plain", "blocked", "gate"))
            g = K.gates()
            for form, res in RESULTS:
                c = res["case"]
                if c["cls"] == "acc" and res["fig"]:
                    q = g[R.key_of(c)]
                    cols = ["  ".join("%6.2f" % d[k] for k in R.FIGS) for d in (res["fig"], q["plain"], q["blocked"], q["gate"])]
                    fh.write("  %-38s %4d %5d %5d %4s   %s   %s   %s   %s\n" % (form, c["n"], c["r"], c["kappa"], c["dtype"], cols[0], cols[1], cols[2], cols[3]))
            n_exact = sum(1 for _, r in RESULTS if r["case"]["cls"] == "exact")
            fh.write("# exact class: %d cases, %d bit-equal to L0 and W0\n" % (n_exact, sum(1 for _, r in RESULTS if r["case"]["cls"] == "exact" and not r["bad"])))
            fh.write("# mode 0: P bitwise untouched in %d of %d cases\n" % (sum(1 for _, r in RESULTS if "mode 0 changed P" not in r["bad"]), len(RESULTS)))
            for t in TRIPLES:
                fh.write("# mode 1: N=%d cap=%d r=%d  %s\n" % t)


def _num_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _check(form, results, n_min):
    for res in results:
        print(form, K.describe(res))
        RESULTS.append((form, res))
    assert len(results) >= n_min, "only %d cases ran" % len(results)
    assert {r["case"]["cls"] for r in results} == {"exact", "acc"}
    bad = [K.describe(r) for r in results if r["bad"]]
    assert not bad, "%d of %d cases:\n" % (len(bad), len(results)) + "\n".join(bad)


def _ids(s):
    return "N%d_cap%d" % s


@pytest.mark.parametrize("shape", R.CONTEXTS, ids=_ids)
def test_the_persistent_form(pre3, shape):
    """k_cholp: crit, rows and strips in one launch, 2 .. 16 panels, and one panel through predicted_prior (what an update of the predicted state takes)"""
    cus = _num_cus()
    for group in ("cholp", "cholp1"):
        for c in R.group_cases(group, "f32"):
            if (c["N"], c["cap"]) == shape and not R.cholp_takes(R.round_up(c["r"], 64) // 64, c["cap"], cus, group == "cholp1"):
                pytest.skip("%d CUs: crit and the rows of %d panels do not fit, launch_chol_solve takes the launch-per-panel form" % (cus, R.round_up(c["r"], 64) // 64))
    _check("k_cholp", K.run_form(pre3, "k_cholp", (shape,), cus), 9)


@pytest.mark.parametrize("shape", R.CONTEXTS, ids=_ids)
@pytest.mark.parametrize("form", ["k_chol_step<float> with planes", "k_chol_step<float>", "k_chol_step<double>"])
def test_the_launch_per_panel_forms(pre3, form, shape):
    """PRE3_OPT_CHOL_PERSIST off: k_chol_step<float> with the bf16 planes (pending updates and trailing tiles from planes, chol_store_w_strip);
    PRE3_OPT_K9_BF16X3 off: without them; fp64 contexts: k_chol_step<double>.  The `early` instantiation takes the last panel of r = 1 .. 9, 56, 120 and 1000;
    17 and 18 panels run with PRE3_OPT_CHOL_PERSIST on and still come here."""
    rows = R.ROWS[shape]
    assert any(R.early_panel(r) for r in rows) and any(not R.early_panel(r) for r in rows)
    _check(form, K.run_form(pre3, form, (shape,), _num_cus()), 9)


@pytest.mark.parametrize("knobs", R.TRAIL_KNOBS, ids=lambda k: "P%d_T128_%d" % k)
def test_the_trailing_sweeps(knobs):
    """PRE3_CHOL_TRAIL_SPLIT=1 in a child process (the switches are read once): with PRE3_CHOL_TRAIL_P=1 the trailing updates of 15 and 16 panels go out
    as k_chol_trail_b3 launches of their own; with 4, panels 1 .. 8 bring their own column up to date from 1 .. 4 pending panels and a sweep of four
    panels follows panels 3 and 7 -- k_chol_trail_b3l (PRE3_CHOL_TRAIL_T128=2) or k_chol_trail_b3 (0).  (11 panels stay below the threshold on 256 CUs:
    504 tiles against 512; they run under the same switches in the panels' own launches.)"""
    cus, (p, t128) = _num_cus(), knobs
    plans = [R.trail_plan(r // 64, R.BIG[1], cus, 1, p) for r in R.TRAIL_ROWS]
    if p == 1 and not (plans[1][0] and plans[2][0]):
        pytest.skip("%d CUs: no trailing update of 15 or 16 panels exceeds %d tiles" % (cus, 2 * cus))
    if p == 4 and not (set(plans[2][1].values()) == {1, 2, 3, 4} and plans[1][2] and plans[2][2]):
        pytest.skip("%d CUs: the panels of 15 and 16 are not grouped in fours" % cus)
    env = dict(os.environ, PRE3_TEST_HOOKS="1", PRE3_CHOL_TRAIL_SPLIT="1", PRE3_CHOL_TRAIL_P=str(p), PRE3_CHOL_TRAIL_T128=str(t128))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "chol_worker.py"), "trail", str(cus)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("CHOLJSON ")]
    assert len(lines) == 1, r.stdout[-2000:]
    _check("trailing sweeps P=%d T128=%d" % knobs, json.loads(lines[0][9:]), 9)


def _same(a, b):
    return "bit-equal" if np.array_equal(a, b) else "%d entries differ, by up to %.3g of max|P|" % (int((a != b).sum()), float(np.abs(a - b).max() / np.abs(a).max()))


@pytest.mark.parametrize("shape", R.MODE1_CONTEXTS, ids=_ids)
def test_the_planes_the_factorisation_writes_feed_the_down_date(pre3, shape):
    """mode 1: (a) consumers inside k_cholp, (b) k_downdate_b3 behind it on the strips' planes, (c) the pinned K9 (test_downdate) on k_split_w's planes of
    the W read back from (b); then (b'), (c') with the launch-per-panel form's planes.  One live context: a second one takes the consumers out."""
    N, cap = shape
    cus, kappa, worst = _num_cus(), 1000, []
    f = K.open_context(pre3, N, cap, "k_cholp")
    assert f.k9_overlap() is True or f.k9_overlap() == 1
    x0 = K9.x0_of(N)
    for r in [r for r in R.MODE1_ROWS if R.round_up(r, 64) <= R.rcap_of(cap)]:
        nrb = R.round_up(r, 64) // 64
        assert R.cholp_takes(nrb, cap, cus, nrb == 1)
        S, B, nu = R.accuracy_case(f.n, r, kappa, "f32")
        P0 = K.mode1_prior(f.n, r, kappa)
        got = {}
        for name, persist, overlap in (("a", True, True), ("b", True, False), ("b'", False, True)):
            assert f.chol_persist(persist) == persist
            f.k9_overlap(overlap)
            f.set_x_p_k_k(x0, P0)
            L, W = f.test_factor_solve(S, B, nu, mode=1, predicted_prior=nrb == 1)
            got[name] = (f.get_p_k_k(), W)
            assert not W[r:].any() and np.isfinite(W).all()
            if name != "a":
                f.set_x_p_k_k(x0, P0)
                f.test_downdate(W[:r, :f.n])
                got[name.replace("b", "c")] = (f.get_p_k_k(), W)
        f.chol_persist(True); f.k9_overlap(True)
        assert np.array_equal(got["a"][1], got["b"][1])                       # the same launch but for the consumers: the same W
        for x, y in (("a", "b"), ("b", "c"), ("b'", "c'")):
            what = "(%s) = (%s): %s" % (x, y, _same(got[x][0], got[y][0]))
            print(shape, r, what)
            TRIPLES.append((N, cap, r, what))
            if not np.array_equal(got[x][0], got[y][0]):
                worst.append("r=%d %s" % (r, what))
        # and the down-date did what it says, on the device's own W: inside the worst-case bound of an r-term sum in f32 (the cap of the K9 gate;
        # the kernel's own gate is test_gpu_k9_alone.py's)
        assert K9.norm_err(got["b"][0], P0, got["b"][1][:r, :f.n], 1, K9.U32)[0] <= r + 8
    f.close()
    assert not worst, "\n".join(worst)


def test_the_hook_refuses_what_it_must(pre3, monkeypatch):
    """PRE3_E_ARG before anything is touched: P is read back, and the call that follows returns what the call in front returned, bit for bit"""
    N, cap = 20, 96
    f = K.open_context(pre3, N, cap, "k_cholp")
    P0 = K.prior(f.n, "f32")
    f.set_x_p_k_k(K9.x0_of(N), P0)
    S, B, nu = R.accuracy_case(f.n, 65, 10, "f32")
    L1, W1 = f.test_factor_solve(S, B, nu)
    rcap = R.rcap_of(cap)

    def poisoned(a, at, v):
        a = a.copy(); a[at] = v
        return a
    big = rcap + 1
    refused = [(np.eye(big), np.ones((big, f.n)), np.ones(big), 0), (poisoned(S, (3, 2), np.nan), B, nu, 0), (S, poisoned(B, (64, 7), np.inf), nu, 0),
               (S, B, poisoned(nu, 0, np.nan), 0), (poisoned(S, (0, 0), 1e300), B, nu, 0), (S, B, nu, 2)]
    for Sb, Bb, nb, mode in refused:
        with pytest.raises(pre3.Pre3Error) as e:
            f.test_factor_solve(Sb, Bb, nb, mode=mode)
        assert e.value.code == -1                                             # PRE3_E_ARG
        assert np.array_equal(f.get_p_k_k(), P0)
    for Sb, Bb, nb in ((S, B[:, :-1], nu), (S[:, :-1], B, nu), (S, B, nu[:-1]), (S[:0, :0], B[:0], nu[:0])):
        with pytest.raises((ValueError, pre3.Pre3Error)):
            f.test_factor_solve(Sb, Bb, nb)
    monkeypatch.delenv("PRE3_TEST_HOOKS", raising=False)
    with pytest.raises(pre3.Pre3Error) as e:
        f.test_factor_solve(S, B, nu)
    assert e.value.code == -4                                                 # PRE3_E_STATE: the hooks are off
    monkeypatch.setenv("PRE3_TEST_HOOKS", "1")
    assert np.array_equal(f.get_p_k_k(), P0)
    L2, W2 = f.test_factor_solve(S, B, nu)
    assert np.array_equal(L1, L2) and np.array_equal(W1, W2)
    Sx, Bx, nx = R.exact_case(f.n, rcap)[:3]                                  # the largest r the context admits
    L, W = f.test_factor_solve(Sx, Bx, nx)
    assert R.judge(dict(n=f.n, r=rcap, cls="exact"), L, W, {})[0] == []
    f.close()
