"""Writes tests/golden/chol_tolerance.json: the gates of tests/test_gpu_chol_alone.py, measured on the CPU with the two restatements
`plain` and `blocked` of tests/chol_ref.py alone -- never with the device, and never with the emulation of the persistent form.

Per committed accuracy input (chol_ref.accuracy_keys(): state size n, rows r, kappa, dtype) the file records the four figures of either
restatement -- max and RMS of E1 = |L L' - S| / (u |L||L|') over the lower triangle and of E2 = |L W - [B | nu]| / (u |L||W|) over every
entry, u = 2^-24 (f32) or 2^-53 (f64) -- and the device's gate: FACTOR x the larger of the two restatements' figures, each of the four on its own.

FACTOR = 6.  The argument is about the kernels' arithmetic where the restatements do least work, r = 1, in worst-case bounds (u = one correctly
rounded operation; an operation good to one ulp is off by up to 2 u):

  * E1.  plain: l = sqrt(s), one rounding, |l^2 - s| <= 2 u l^2.  The chains (chol_chain, pre3_chain_async.h) take l = s * v_rsq(s): 2 u for the
    raw v_rsq_f32, one for the product, |l^2 - s| <= 6 u l^2.  Ratio 3.
  * E2.  blocked, the larger restatement at r = 1: l (1 u), M = 1 / l (1 u), w = M b rounded once (1 u): |l w - b| <= 3 u |l||w|.  The persistent
    form: l as above (3 u), M = v_rsq(s) (2 u), so |l M - 1| <= 5 u; w = M b as six plane products -- the three roundings of the plane split lose
    nothing (8 + 8 + 8 bits hold an f32), the three dropped products (1,2), (2,1), (2,2) are at most 2^-24, 2^-24 and 2^-32 of |M||b|, together
    2 u, and the accumulator is rounded after each of the five products that follow the first: 5 u.  12 u against 3 u: ratio 4.  The
    launch-per-panel forms substitute in the chain, w = b * v_rsq(s): |l v_rsq(s) - 1| <= 5 u and the product's rounding, 6 u against 3 u: ratio 2.
    fp64 contexts refine v_rcp / v_rsq by Newton steps to within an ulp: the same counts.
  * From there the ratio falls.  Per rank-64 update of an entry plain rounds 128 times (a product and a subtraction per column), the matrix-core
    forms 24 times (six products in each of four k-steps, accumulated from zero in f32) and once in the subtraction; the order of the 16 terms
    inside one matrix-core product does not enter (they are exact products of bf16 values summed into a wider accumulator).  The one rounding more
    that goes through M_J -- L(i,J) = A(i,J) M_J' instead of a substitution -- is what `blocked` restates, and the gate takes the larger of the
    two restatements for exactly that reason; on these inputs blocked stays inside plain from two panels on; below, its RMS stays within
    1.5 x (three roundings against two at r = 1) and its maxima within 3 x (tests/test_chol_ref.py asserts all of it).

So the worst-case ratio is 4, met at the smallest r; 4 itself would leave nothing for comparing two measured maxima (over n + 1 entries at r = 1 --
and E1 has ONE entry there), so the gate keeps the headroom of a factor 1.5 that the down-date's gate keeps: 6.  It is one number for every case
and both dtypes, it is not fitted to a device run, and tests/test_chol_ref.py shows what it still catches: each of the three mutants of the
emulation lands at least twice outside it.

    python tests/golden/make_chol_tolerance.py          (rewrites the file; tests/test_chol_ref.py checks that it is reproduced)"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import chol_ref as R  # noqa: E402

FACTOR = 6


def measure_one(n, r, kappa, dtype):
    S, B, nu = R.accuracy_case(n, r, kappa, dtype)
    out = dict(n=n, r=r, kappa=kappa, dtype=dtype)
    for name, f in (("plain", R.plain), ("blocked", R.blocked)):
        L, W = f(S, B, nu, dtype)
        fig, bad = R.figures(L, W, S, B, nu, dtype)
        assert not bad, (name, bad)
        out[name] = fig
    out["gate"] = {k: FACTOR * max(out["plain"][k], out["blocked"][k]) for k in R.FIGS}
    return out


def measure(keys=None):
    return dict(factor=FACTOR, cases={key: measure_one(*v) for key, v in sorted((keys or R.accuracy_keys()).items())})


if __name__ == "__main__":
    out = measure()
    with open(os.path.join(HERE, "chol_tolerance.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("%-22s %-34s %-34s" % ("case", "plain  E1 max/rms  E2 max/rms", "blocked"))
    for key, c in out["cases"].items():
        print("%-22s %-34s %-34s" % (key, "  ".join("%6.2f" % c["plain"][k] for k in R.FIGS), "  ".join("%6.2f" % c["blocked"][k] for k in R.FIGS)))
