#!/usr/bin/env python
"""Time the dense ICP between two resident 144 x 176 frames: tests/icp_frame_cases.py's pair, vo.icp_frames at stride 1, 2 and 4.

Per stride: host wall time per call (one host wait each; median and quartiles over --reps calls behind --warmup warmed ones), the iterations the run
took and the time per iteration, and the nearest-neighbour launch alone on the same compacted clouds (vo.icp_nn_bench: back-to-back launches between
two events).  Every call queues all 62 iterations' launches, those behind the end of the run return at once: `floor_ms` is the same call on a pair
that ends in its first iteration, the cost of the queued launches alone.  Next to them the numpy restatement's wall time for the same call
(tests/icp_ref.py; stride 4 by default, --restate-stride 0 skips it): the only baseline there is.  No target is set.

    python tools/time_icp.py [--reps 20] [--warmup 3] [--restate-stride 4] [--out profiles/icp_timing.json]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import icp_frame_cases as F  # noqa: E402
import icp_ref as R  # noqa: E402


def quartiles(ts):
    q1, med, q3 = np.percentile(np.asarray(ts) * 1e3, [25, 50, 75])
    return dict(median_ms=round(float(med), 4), q1_ms=round(float(q1), 4), q3_ms=round(float(q3), 4), n=len(ts))


def timed(fn, warmup, reps):
    for _ in range(warmup):
        out = fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return out, quartiles(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--restate-stride", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_timing.json"))
    a = ap.parse_args()
    pre3 = importlib.import_module("3pre_amd")
    srm, vo = pre3.sr4000, importlib.import_module("3pre_amd.vo")
    assert pre3.device_count() >= 1, "needs a HIP device"
    sc = F.make_frames()
    res = dict(rows=F.ROWS, cols=F.COLS, res=F.RES, reps=a.reps, warmup=a.warmup, limits=vo.icp_limits(), strides={})
    with srm.SrFrame(F.ROWS, F.COLS) as f1, srm.SrFrame(F.ROWS, F.COLS) as f2:
        f1.load(sc["fr1"], F.MODE); f2.load(sc["fr2"], F.MODE)
        x1, y1, z1, _ = f1.planes(); x2, y2, z2, _ = f2.planes()
        for stride in (1, 2, 4):
            cl = F.clouds(x1, y1, z1, x2, y2, z2, stride)
            out, q = timed(lambda: vo.icp_frames(f1, f2, F.RES, sc["Rinit"], sc["Tinit"], stride=stride), a.warmup, a.reps)
            # the same launches with a seed that puts the source nowhere near the model: the run ends in its first iteration (p < 3)
            _, qf = timed(lambda: vo.icp_frames(f1, f2, F.RES, sc["Rinit"], sc["Tinit"] + 1000.0, stride=stride), a.warmup, a.reps)
            it = out["iters1"] + out["iters2"]
            row = dict(n_model=out["n_model"], n_source=out["n_source"], sta=out["sta"], iterations=it, p=out["p"], call=q, floor=qf,
                       ms_per_iteration=round((q["median_ms"] - qf["median_ms"]) / max(it - 1, 1), 4),
                       nn_launch_ms=round(vo.icp_nn_bench(cl["model"], cl["source"], reps=50), 4))
            if stride == a.restate_stride:
                t0 = time.perf_counter()
                want = R.icp_with_init(cl["model"], cl["source"], F.RES, sc["Rinit"], sc["Tinit"])
                row["restatement_s"] = round(time.perf_counter() - t0, 3)
                row["restatement_iterations"] = want["iters1"] + want["iters2"]
            res["strides"][str(stride)] = row
            print("stride", stride, json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
