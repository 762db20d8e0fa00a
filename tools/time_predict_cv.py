#!/usr/bin/env python
"""Time the camera-only prediction (pre3_predict_cv) against the odometry prediction (pre3_predict: k_predict without riders), on
one build and one context.

    sync:        EkfFilter.sync() with nothing queued                                   (the floor of the wait itself)
    predict:     EkfFilter.ekf_prediction(u); sync()                                    (one launch: 4 rows of P per column)
    predict_cv:  EkfFilter.ekf_prediction_cv(dt, sigma_a, sigma_alpha); sync()          (one launch: 13 rows of P per column)

on an N = 500 fp32 context (n = 3013).  The legs are alternated call by call behind --warmup warmed ones, each from the same (x_k_k, p_k_k) installed
outside the timed region (that call synchronises: every leg starts from an idle device); host wall time per call, median and quartiles over --reps
calls; the clocks as found.  The expectation is the same few-microsecond class for both launches -- both sit near the small-launch floor --; it is an
expectation, not a gate.

    python tools/time_predict_cv.py [--reps 100] [--warmup 10] [--out profiles/predict_cv_timing.json]
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


def quartiles(ts):
    q1, med, q3 = np.percentile(np.asarray(ts) * 1e6, [25, 50, 75])
    return dict(median_us=round(float(med), 2), q1_us=round(float(q1), 2), q3_us=round(float(q3), 2), n=len(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--N", type=int, default=500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict_cv_timing.json"))
    a = ap.parse_args()
    pre3 = importlib.import_module("3pre_amd")
    synth = importlib.import_module("3pre_amd.synth")
    assert pre3.device_count() >= 1, "needs a HIP device"
    N = a.N
    x0, P0, _ = synth.make_map(N, None)
    x0 = x0.copy()
    x0[7:13] = [0.05, -0.03, 0.04, 0.02, -0.015, 0.025]
    u = np.array([0.004, -0.003, 0.002, 1.0, 0.0008, -0.0006, 0.0009])
    u[3:] /= np.linalg.norm(u[3:])
    f = pre3.EkfFilter(synth.CAM, np.zeros(N, np.int32), dtype="f32", max_hyp=8)

    def leg_predict():
        f.ekf_prediction(u)
        f.sync()

    def leg_predict_cv():
        f.ekf_prediction_cv(0.1, 0.007, 0.007)
        f.sync()

    forms = dict(sync=f.sync, predict=leg_predict, predict_cv=leg_predict_cv)
    ts = {k: [] for k in forms}
    for r in range(a.warmup + a.reps):
        for k, fn in forms.items():
            f.set_x_p_k_k(x0, P0)
            t0 = time.perf_counter()
            fn()
            if r >= a.warmup:
                ts[k].append(time.perf_counter() - t0)
    f.close()
    t = {k: quartiles(v) for k, v in ts.items()}
    res = dict(N=N, n=13 + 6 * N, dtype="f32", reps=a.reps, warmup=a.warmup, timing=t,
               predict_cv_extra_us=round(t["predict_cv"]["median_us"] - t["predict"]["median_us"], 2),
               note="host wall time of call + stream wait; the sync leg is the wait alone")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
