#!/usr/bin/env python
"""Time the VO pair call and the prediction pair with and without the pair's covariance, on one build and one context.

    pair / pair_cov:        vo.vo_pair_seeded(prev, cur)  /  vo.vo_pair_cov_seeded(prev, cur)                 (one host wait each)
    predict / predict_cov:  EkfFilter.ekf_prediction_pair_seeded(prev, cur)  /  .ekf_prediction_pair_cov_seeded(prev, cur), both waiting

at the pairs p64 (36 x 45) and p129 (144 x 176) of tests/vo_pair_cases.py, on an N = 200 fp32 context.  The four legs are alternated call by call
behind --warmup warmed ones, the prediction legs each from the same (x_k_k, p_k_k) installed outside the timed region; host wall time per call, median
and quartiles over --reps calls; the clocks as found.  The expectation is one more launch floor (k_vo_cov, one wave) on the *_cov legs; it is an
expectation, not a gate.

    python tools/time_vo_cov.py [--reps 200] [--warmup 20] [--out profiles/vo_cov_timing.json]
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
import vo_pair_cases as vp  # noqa: E402


def quartiles(ts):
    q1, med, q3 = np.percentile(np.asarray(ts) * 1e6, [25, 50, 75])
    return dict(median_us=round(float(med), 2), q1_us=round(float(q1), 2), q3_us=round(float(q3), 2), n=len(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vo_cov_timing.json"))
    a = ap.parse_args()
    pre3 = importlib.import_module("3pre_amd")
    srm, vo, synth = pre3.sr4000, importlib.import_module("3pre_amd.vo"), importlib.import_module("3pre_amd.synth")
    assert pre3.device_count() >= 1, "needs a HIP device"
    N, seed, seq = 200, 7, 1
    x0, P0, _ = synth.make_map(N, None)
    f = pre3.EkfFilter(synth.CAM, np.zeros(N, np.int32), dtype="f32", max_hyp=8)
    res = dict(N=N, dtype="f32", reps=a.reps, warmup=a.warmup, cases={})
    for name in ("p64", "p129"):
        c = vp.case(name)
        f1, f2 = srm.SrFrame(c["rows"], c["cols"]), srm.SrFrame(c["rows"], c["cols"])
        f1.load(c["fr1"], 1); f2.load(c["fr2"], 1)
        f1.keypoints(c["frm1"], c["des1"], 1); f2.keypoints(c["frm2"], c["des2"], 1)
        forms = dict(pair=lambda: vo.vo_pair_seeded(f1, f2, seed, seq), pair_cov=lambda: vo.vo_pair_cov_seeded(f1, f2, seed, seq),
                     predict=lambda: f.ekf_prediction_pair_seeded(f1, f2, seed, seq), predict_cov=lambda: f.ekf_prediction_pair_cov_seeded(f1, f2, seed, seq))
        first = forms["pair_cov"]()
        ts = {k: [] for k in forms}
        for r in range(a.warmup + a.reps):
            for k, fn in forms.items():
                f.set_x_p_k_k(x0, P0)                   # (synchronises: every leg starts from an idle device and the same state)
                t0 = time.perf_counter()
                fn()
                if r >= a.warmup:
                    ts[k].append(time.perf_counter() - t0)
        t = {k: quartiles(v) for k, v in ts.items()}
        res["cases"][name] = dict(rows=c["rows"], cols=c["cols"], n1=c["n1"], n2=c["n2"], pnum=c["pnum"], n_support=first["n_support"],
                                  cov_status=first["cov_status"], timing=t,
                                  pair_cov_extra_us=round(t["pair_cov"]["median_us"] - t["pair"]["median_us"], 2),
                                  predict_cov_extra_us=round(t["predict_cov"]["median_us"] - t["predict"]["median_us"], 2))
        f1.close(); f2.close()
    f.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
