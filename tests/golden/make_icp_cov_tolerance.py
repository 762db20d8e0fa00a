"""Writes tests/golden/icp_cov_tolerance.json: the floor of the ICP's closed-form covariance, measured on the CPU with the
restatement alone (tests/icp_cov_ref.py over tests/vo_cov_ref.py, on tests/icp_ref.py's own ICP run) -- never with the code under test.

The recipe is tests/golden/make_vo_cov_tolerance.py's.  On every committed case (icp_cov_ref.committed_cases: the three surface scenes' final lists and
the truncations of the largest one, 256 x limits[1] + 1 = 1025 among them) the restatement runs once as it is and TRIALS times with every atan2 / hypot
/ sin / cos / sqrt result moved by a random -2 .. +2 ulp, the pairs summed in a random order, and H^-1 taken by the Cholesky factor and by
numpy.linalg.solve in turn.  A case's floor is the largest difference of a covariance entry relative to the largest |cov| entry of that case.

The gate of a case is FACTOR x max(its own floor, the floor over the three full lists).  The floor scales with cond(H) -- the two solves --, and a list
cut to a handful of pairs is far worse conditioned than a full one, so one figure for all would either hide an error on the full lists or fail the
short ones; the full lists' floor stands under every case so that twelve trials' luck on one case cannot shrink its gate below the common level.
The factor covers what the jitter model leaves out: the device library's own ulp bounds where they exceed 2, the fixed tree of the two launches, and
the order inside the per-point products.  The generator asserts cond(H) < 2000 on the full lists (the issue's bound; 360 - 411 measured).

    python tests/golden/make_icp_cov_tolerance.py          (rewrites the file; tests/test_icp_cov_ref.py checks that it is reproduced)"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import icp_cov_ref as R  # noqa: E402
from make_vo_cov_tolerance import Jitter  # noqa: E402

FACTOR = 16
TRIALS = 12
JITTER_SEED, SHUFFLE_SEED = 505, 606
COND_MAX_FULL = 2000.0
EXTRA_TRUNCATIONS = (1025,)                         # 256 x pre3_icp_cov_limits()[1] + 1; the GPU test checks that the library still says 4


def measure():
    jit, shuf = np.random.default_rng(JITTER_SEED), np.random.default_rng(SHUFFLE_SEED)
    cases, full = {}, len(R.SHAPES)
    for i, (name, d1, d2, corr, u) in enumerate(R.committed_cases(EXTRA_TRUNCATIONS)):
        H = R.sums(d1, d2, corr, u)[0]
        cond = float(np.linalg.cond(H))
        if i < full:
            assert cond < COND_MAX_FULL, "%s has cond(H) = %g" % (name, cond)
        base, status, n = R.cov(d1, d2, corr, u)
        assert status == 1 and n == len(corr), (name, status)
        floor = 0.0
        for t in range(TRIALS):
            other, st, _ = R.cov(d1, d2, corr, u, order=shuf.permutation(n), solver=("chol", "solve")[t % 2], m=Jitter(jit))
            assert st == 1
            floor = max(floor, float(np.abs(other - base).max() / np.abs(base).max()))
        cases[name] = dict(p=int(n), cond=cond, floor=floor, sigma_T_mm=[float(v) for v in 1000 * np.sqrt(np.diag(base)[:3])])
    names = list(cases)
    floor_full = max(cases[k]["floor"] for k in names[:full])
    for k in names:
        cases[k]["tol"] = FACTOR * max(cases[k]["floor"], floor_full)
    return dict(factor=FACTOR, trials=TRIALS, jitter_seed=JITTER_SEED, shuffle_seed=SHUFFLE_SEED, floor_full=floor_full, full=names[:full], cases=cases)


def tolerance(tab, name):
    return float(tab["cases"][name]["tol"])


if __name__ == "__main__":
    out = measure()
    with open(os.path.join(HERE, "icp_cov_tolerance.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))
