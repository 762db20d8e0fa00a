"""ms per 144 x 176 frame for the SIFT set made on the device (SrFrame.sift) alone, and for sift + gate + the VO pair, next to the same chain with
the two sets uploaded from the host (SrFrame.keypoints).  Wall-clock around calls that wait; medians over --reps after --warmup.

    python tools/time_sift_frame.py [--reps 30] [--warmup 5]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import sift_ref as R  # noqa: E402
import sr_frame_ref as sr  # noqa: E402

srm = importlib.import_module("3pre_amd.sr4000")
vo = importlib.import_module("3pre_amd.vo")


def planes(seed):
    fr = sr.make_frame(144, 176, seed=seed, conf=True)
    fr["amp"] = np.asfortranarray((R.make_image(144, 176, seed=40 + seed) / 255.0) ** 2 * 9000.0 + 1.0)
    return fr


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    f1, f2 = srm.SrFrame().load(planes(1), srm.MODE_DR_YE), srm.SrFrame().load(planes(2), srm.MODE_DR_YE)
    s1, s2 = f1.sift(), f2.sift()

    def device_chain():
        for f in (f1, f2):
            f.sift(want_arrays=False); f.gate(1)
        vo.vo_pair_seeded(f1, f2, 5, 0, 1.5)

    def host_chain():
        f1.keypoints(s1["frames"], s1["descriptors"], 1); f2.keypoints(s2["frames"], s2["descriptors"], 1)
        vo.vo_pair_seeded(f1, f2, 5, 0, 1.5)
    out = dict(K=[s1["K"], s2["K"]], sift_ms=median_ms(lambda: f1.sift(want_arrays=False), a.reps, a.warmup),
               sift_with_arrays_ms=median_ms(lambda: f1.sift(), a.reps, a.warmup),
               two_frames_sift_gate_vo_ms=median_ms(device_chain, a.reps, a.warmup), two_frames_upload_gate_vo_ms=median_ms(host_chain, a.reps, a.warmup))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
