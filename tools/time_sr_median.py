#!/usr/bin/env python
"""Time the frame conditioning under the bad-pixel compensation at 144 x 176.

    SrFrame.load followed by one synchronisation (a maxima read-back) on ONE handle, in both modes, under form 0 (none), form 2 (the image's median) and
    form 1 (bad pixels) at 0 %, 5 % and 100 % bad pixels.

The legs are alternated call by call behind --warmup warmed rounds; a host clock around work that ends in a synchronise; median and quartiles over
--reps calls; the clocks as found.  The form-0 figure of the same run is the yardstick.  The expectation is a record, not a gate: the compensated launch
stays near the small-launch floor the form-0 launch sits at, so load remains dominated by the 1 MB staged transfer.

    python tools/time_sr_median.py [--reps 200] [--warmup 20] [--out profiles/sr_median_timing.json]
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

CUTOFF = 1.0


def quartiles(ts):
    q1, med, q3 = np.percentile(np.asarray(ts) * 1e6, [25, 50, 75])
    return dict(median_us=round(float(med), 2), q1_us=round(float(q1), 2), q3_us=round(float(q3), 2), n=len(ts))


def with_bad(fr, fraction, seed):
    """the frame with `fraction` of its confidences below the cut-off (0) and the rest above it"""
    out = dict(fr)
    conf = np.asfortranarray(np.maximum(fr["conf"], CUTOFF))
    conf[np.random.default_rng(seed).random(conf.shape) < fraction] = 0.0
    out["conf"] = conf
    return out, int((conf < CUTOFF).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sr_median_timing.json"))
    a = ap.parse_args()
    pre3 = importlib.import_module("3pre_amd")
    srm = pre3.sr4000
    assert pre3.device_count() >= 1, "needs a HIP device"
    res = dict(rows=144, cols=176, reps=a.reps, warmup=a.warmup, cutoff=CUTOFF, what="SrFrame.load + maxima() (one synchronisation), wall clock",
               load={}, n_bad={}, ratio_over_form0={})
    base = sr.make_frame(144, 176, seed=1)
    f = srm.SrFrame()
    for mode in (0, 1):
        legs = []
        for name, form, fraction in (("form0", 0, 0.0), ("form2", 2, 0.0), ("form1_bad0", 1, 0.0), ("form1_bad5", 1, 0.05), ("form1_bad100", 1, 1.0)):
            fr, n_bad = with_bad(base, fraction, seed=mode)
            legs.append(("mode%d_%s" % (mode, name), form, fr))
            res["n_bad"]["mode%d_%s" % (mode, name)] = n_bad if form == 1 else 0
        ts = {name: [] for name, _, _ in legs}
        for it in range(a.warmup + a.reps):
            for name, form, fr in legs:
                f.set_compensation(form, CUTOFF)
                t0 = time.perf_counter()
                f.load(fr, mode)
                f.maxima()
                dt = time.perf_counter() - t0
                if it >= a.warmup:
                    ts[name].append(dt)
                assert it > 0 or f.bad_pixels() == (form, res["n_bad"][name])
        for name, _, _ in legs:
            res["load"][name] = quartiles(ts[name])
        for name, _, _ in legs:
            res["ratio_over_form0"][name] = round(res["load"][name]["median_us"] / res["load"]["mode%d_form0" % mode]["median_us"], 3)
    f.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
