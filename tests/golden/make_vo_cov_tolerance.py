"""Writes tests/golden/vo_cov_tolerance.json: the floor of the VO pair's covariance, measured on the CPU with the restatement
alone (tests/vo_cov_ref.py) -- never with the code under test.

On every committed case (vo_cov_ref.CASES) the restatement runs once as it is and TRIALS times with every atan2 / hypot / sin / cos / sqrt result moved
by a random -2 .. +2 ulp, the inliers summed in a random order, and H^-1 taken by the Cholesky factor and by numpy.linalg.solve in turn.  The floor is
the largest difference of a covariance entry, relative to the largest |cov| entry of its case; the GPU gate is FACTOR x that floor.  The factor covers
what the jitter model leaves out: the device library's own ulp bounds where they exceed 2, the butterfly's summation tree, and the order inside the
per-point products.  The floor scales with cond(H) (the two solves), so the generator asserts that every committed case stays below 1e4.

    python tests/golden/make_vo_cov_tolerance.py          (rewrites the file; tests/test_vo_cov_ref.py checks that it is reproduced)"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import vo_cov_ref as R  # noqa: E402

FACTOR = 16
TRIALS = 12
JITTER_SEED, SHUFFLE_SEED = 303, 404
COND_MAX = 1e4


class Jitter(R.Math):
    def __init__(self, rng):
        self.rng = rng

    def _j(self, v):
        v = np.float64(v)
        return v + int(self.rng.integers(-2, 3)) * np.spacing(np.abs(v)) if np.isfinite(v) and v != 0 else v

    def atan2(self, y, x): return self._j(np.arctan2(y, x))
    def hypot(self, a, b): return self._j(np.hypot(a, b))
    def sin(self, a): return self._j(np.sin(a))
    def cos(self, a): return self._j(np.cos(a))
    def sqrt(self, a): return self._j(np.sqrt(a))


def measure():
    jit, shuf = np.random.default_rng(JITTER_SEED), np.random.default_rng(SHUFFLE_SEED)
    floor, conds = 0.0, []
    for c in R.committed_cases():
        H = R.sums(c["pset1"], c["pset2"], c["inliers"], c["u"])[0]
        conds.append(float(np.linalg.cond(H)))
        assert conds[-1] < COND_MAX, "a committed case has cond(H) = %g" % conds[-1]
        base, status, n = R.cov(c["pset1"], c["pset2"], c["inliers"], c["u"])
        assert status == 1
        for t in range(TRIALS):
            other, st, _ = R.cov(c["pset1"], c["pset2"], c["inliers"], c["u"], order=shuf.permutation(n), solver=("chol", "solve")[t % 2], m=Jitter(jit))
            assert st == 1
            floor = max(floor, float(np.abs(other - base).max() / np.abs(base).max()))
    return dict(factor=FACTOR, floor=floor, tol=FACTOR * floor, trials=TRIALS, jitter_seed=JITTER_SEED, shuffle_seed=SHUFFLE_SEED,
                cases=[list(map(int, c)) for c in R.CASES], cond_max=max(conds))


if __name__ == "__main__":
    out = measure()
    with open(os.path.join(HERE, "vo_cov_tolerance.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))
