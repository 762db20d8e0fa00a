"""Writes tests/golden/icp_tolerance.json: what the order of reg()'s sums moves in the dense ICP's results, measured on the CPU with
the restatement alone (tests/icp_ref.py) -- never with the code under test.

Every scene of tests/test_gpu_icp.py and the stride-8 scene of tests/test_gpu_icp_frames.py runs twice: with the sums of the means, of K and of sum(D)
taken forward, and taken in reverse.  The integers of the two runs must agree (the iteration counts, p of every iteration, the final pairs, the status);
the spread is the largest absolute difference over R, t, Rtot, ttot, u, error, the D column and the registered data2.  The GPU suites allow
max(1e-12, FACTOR x spread) per scene: 1e-12 is the project's tolerance for transforms (tests/test_gpu_vo.py), the factor covers a different svd and
a different summation tree.  The scenes that depend on the library's limits are built from the constants of 3pre_amd/csrc/pre3_icp.h, which the file
records; the GPU suite checks them against pre3_icp_limits.

    python tests/golden/make_icp_tolerance.py [scene ...]        (no argument: rewrites the file; tests/test_icp_ref.py re-measures two scenes)"""
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import icp_ref as R  # noqa: E402

FACTOR, FLOOR = 100, 1e-12
FLOAT_KEYS = ("R", "t", "Rtot", "ttot", "u", "error", "data2")


def header_limits():
    txt = open(os.path.join(os.path.dirname(os.path.dirname(HERE)), "3pre_amd", "csrc", "pre3_icp.h")).read()
    val = {k: int(v) for k, v in re.findall(r"constexpr int (ICP_PTS|ICP_NN_THREADS|ICP_CHUNK) = (\d+);", txt)}
    return dict(src_tile=val["ICP_NN_THREADS"] * val["ICP_PTS"], chunk=val["ICP_CHUNK"])


def scene_name(n1, n2, seed):
    return "%dx%d_s%d" % (n1, n2, seed)


def all_scenes(lim):
    return [(n1, n2, s) for (n1, n2) in tuple(R.FIXED_SHAPES) + R.limit_shapes(lim["src_tile"], lim["chunk"]) for s in R.SEEDS]


def spread(data1, data2, res, Rinit, Tinit):
    a = R.icp_with_init(data1, data2, res, Rinit, Tinit, sums="forward")
    b = R.icp_with_init(data1, data2, res, Rinit, Tinit, sums="reversed")
    assert (a["sta"], a["iters1"], a["iters2"], a["ps"]) == (b["sta"], b["iters1"], b["iters2"], b["ps"])
    assert np.array_equal(a["corr"][:, :2], b["corr"][:, :2])
    sp = max(float(np.abs(np.asarray(a[k]) - np.asarray(b[k])).max()) for k in FLOAT_KEYS)
    if len(a["corr"]):
        sp = max(sp, float(np.abs(a["corr"][:, 2] - b["corr"][:, 2]).max()))
    return sp


def measure_scene(n1, n2, seed):
    s = R.surface_scene(n1, n2, seed)
    return spread(s["data1"], s["data2"], s["res"], s["Rinit"], s["Tinit"])


def measure_frames(stride=8):
    import icp_frame_cases as F
    sc = F.make_frames()
    cl = F.restated_clouds(sc, stride)
    return spread(cl["model"], cl["source"], F.RES, sc["Rinit"], sc["Tinit"])


def tolerance(tab, name):
    return max(tab["floor"], tab["factor"] * tab["spread"][name])


if __name__ == "__main__":
    lim = header_limits()
    only = set(sys.argv[1:])
    out = dict(factor=FACTOR, floor=FLOOR, limits=lim, seeds=list(R.SEEDS), spread={})
    for (n1, n2, seed) in all_scenes(lim):
        name = scene_name(n1, n2, seed)
        if only and name not in only:
            continue
        out["spread"][name] = measure_scene(n1, n2, seed)
        print(name, out["spread"][name], flush=True)
    if not only or "frames_stride8" in only:
        out["spread"]["frames_stride8"] = measure_frames()
        print("frames_stride8", out["spread"]["frames_stride8"])
    if not only:
        with open(os.path.join(HERE, "icp_tolerance.json"), "w") as fh:
            json.dump(out, fh, indent=1, sort_keys=True)
            fh.write("\n")
