#!/usr/bin/env python
"""Time the SR4000 frame conditioning at 144 x 176 against the host path it replaces.

    device: SrFrame.load followed by a cmax read-back (a get that synchronises), and the keypoint stage (gate 0, 128-double descriptors) at K = 300, 2048
    host:   tests/sr_frame_ref.py's independent form (b) on the same box -- scipy.ndimage.correlate for the four planes, the line-by-line keypoint loop

Reports the median and quartiles over --reps calls behind --warmup warmed ones and writes profiles/sr_frame_timing.json.  There is no gate on these
numbers: at 25 k pixels the launches sit near the launch floor; the thing to read is the ratio to the host path.

    python tools/time_sr_frame.py [--reps 200] [--warmup 20] [--out profiles/sr_frame_timing.json]
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
import sr_frame_ref as sr  # noqa: E402


def quartiles(ts):
    q1, med, q3 = np.percentile(np.asarray(ts) * 1e6, [25, 50, 75])
    return dict(median_us=round(float(med), 2), q1_us=round(float(q1), 2), q3_us=round(float(q3), 2), n=len(ts))


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return quartiles(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sr_frame_timing.json"))
    a = ap.parse_args()
    pre3 = importlib.import_module("3pre_amd")
    srm = pre3.sr4000
    assert pre3.device_count() >= 1, "needs a HIP device"
    res = dict(rows=144, cols=176, reps=a.reps, warmup=a.warmup, device={}, host={}, ratio_host_over_device={})
    for mode in (0, 1):
        w = srm.gauss3(2.0 if mode == 0 else 1.0).T.ravel()
        fr = sr.make_keypoint_frame(w, mode)
        f = srm.SrFrame()

        def load():
            f.load(fr, mode)
            f.maxima()

        res["device"]["load_mode%d" % mode] = timed(load, a.reps, a.warmup)
        res["host"]["load_mode%d" % mode] = timed(lambda: sr.condition(fr, mode, w, filt=sr.filter_scipy), max(a.reps // 4, 5), 2)
        cond = sr.condition(fr, mode, w)
        for K in (300, 2048):
            frm, des = sr.make_keypoints(K, seed=mode)
            res["device"]["keypoints_mode%d_K%d" % (mode, K)] = timed(lambda: f.keypoints(frm, des, 0), a.reps, a.warmup)
            res["host"]["keypoints_mode%d_K%d" % (mode, K)] = timed(lambda: sr.depth_gate_loop(cond, frm, des), max(a.reps // 20, 3), 1)
        f.close()
    for k, d in res["device"].items():
        res["ratio_host_over_device"][k] = round(res["host"][k]["median_us"] / d["median_us"], 2)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
