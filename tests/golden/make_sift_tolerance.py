"""Writes tests/golden/sift_tolerance.json: the floor of the toleranced outputs of the SIFT extractor (theta, sigma and the descriptor entries),
measured on the CPU with the restatement alone (tests/sift_ref.py) -- never with the code under test.

The restatement runs once as it is and once with every transcendental result moved by a random -2 .. +2 ulp of its own format and every histogram
summed in a random sample order (float32 for the descriptor).  D_theta, D_sigma (relative) and D_des are the largest differences over the committed test
images; the tolerance is FACTOR x that floor.  The factor covers what the jitter model leaves out: contraction inside the float sample arithmetic and
the device library's own ulp bounds where they exceed 2.  One sample put into the wrong bin moves a descriptor entry by ~1e-3: orders of magnitude more.

    python tests/golden/make_sift_tolerance.py          (rewrites the file; tests/test_sift_ref.py checks that it is reproduced)"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import sift_ref as R  # noqa: E402

FACTOR = 16
CASES = [((69, 85), True), ((144, 176), True), ((37, 45), False)]
JITTER_SEED, SHUFFLE_SEED = 101, 202


def measure():
    d_theta = d_sigma = d_des = 0.0
    for shape, strict in CASES:
        I = R.make_image(*shape)
        a = R.sift_vedal(I, strict)
        b = R.sift_vedal(I, strict, jitter=np.random.default_rng(JITTER_SEED), shuffle=np.random.default_rng(SHUFFLE_SEED))
        assert a["frames"].shape == b["frames"].shape and a["frames"].shape[1] > 0, "the jitter changed a discrete decision: pick another seed"
        assert np.array_equal(a["frames"][:2], b["frames"][:2])
        d_theta = max(d_theta, float(np.abs(a["frames"][3] - b["frames"][3]).max()))
        d_sigma = max(d_sigma, float((np.abs(a["frames"][2] - b["frames"][2]) / a["frames"][2]).max()))
        d_des = max(d_des, float(np.abs(a["descriptors"] - b["descriptors"]).max()))
    return dict(factor=FACTOR, floor_theta=d_theta, floor_sigma_rel=d_sigma, floor_des=d_des, tol_theta=FACTOR * d_theta,
                tol_sigma_rel=FACTOR * d_sigma, tol_des=FACTOR * d_des, cases=[[list(s), bool(t)] for s, t in CASES],
                jitter_seed=JITTER_SEED, shuffle_seed=SHUFFLE_SEED)


if __name__ == "__main__":
    out = measure()
    with open(os.path.join(HERE, "sift_tolerance.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))
