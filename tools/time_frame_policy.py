#!/usr/bin/env python
"""Time map management's candidate build and policy from two resident frames against the chain it replaces, on a 144 x 176 pair
and a map of N = 500 landmarks (fp32), at (n1, n2) = (300, 280) and (2048, 2048) kept keypoints.

    frames: EkfFilter.map_management_policy_frames_seeded(step, prev, cur, seed, seq) -- one call, one host wait
    chain:  what the same result took before it, from the same two resident frames with their keypoint records: prev's kept frames, descriptors and
            xyz and cur's kept descriptors read back (SrFrame.keypoints; cur's through the same call), pre3.siftmatch on the kept descriptors, the
            gather in numpy, EkfFilter.map_management_policy_seeded
    frames_with_keypoints: the two keypoint calls followed by the frames call (the chain's read-back IS the keypoint call: this is the like-for-like line)

Each timed call starts from the same filter state (map, x, P, book re-installed and the stream drained before the clock starts) and ends with the
context drained.  The forms are alternated call by call behind --warmup warmed ones; wall clock (perf_counter) and the span between two events on the
context's stream (pre3_timer_start / _stop: it includes the stream's idle time while the host works), median and quartiles over --reps calls; the clocks
as found.  Both forms give the same bits (tests/test_gpu_frame_policy.py); the tool checks the lists once.  No gate on these numbers.

    python tools/time_frame_policy.py [--reps 100] [--warmup 10] [--out profiles/frame_policy_timing.json]
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

pre3 = importlib.import_module("3pre_amd")
synth = importlib.import_module("3pre_amd.synth")
_lib = importlib.import_module("3pre_amd._lib")
SEED, SEQ, STEP, N = 7, 1, 25, 500


def quartiles(ts):
    q1, med, q3 = np.percentile(np.asarray(ts) * 1e6, [25, 50, 75])
    return dict(median_us=round(float(med), 2), q1_us=round(float(q1), 2), q3_us=round(float(q3), 2), n=len(ts))


def one_size(n1, n2, pnum, reps, warmup):
    srm = pre3.sr4000
    c = vp.make_pair(144, 176, n1, n2, pnum, seed=13 + n1, drop1=40, drop2=30)
    rng = np.random.default_rng(n1)
    x, P, _ = synth.make_map(N, seed=N)
    book = np.stack([rng.integers(0, 8, N), rng.integers(0, 8, N), rng.integers(3, STEP, N), rng.integers(3, STEP, N)], 1).astype(np.int32)
    f = pre3.EkfFilter(synth.CAM, np.zeros(N, np.int32), dtype="f32", max_landmarks=N + 100)
    f1, f2 = srm.SrFrame(), srm.SrFrame()
    f1.load(c["fr1"], 0); f2.load(c["fr2"], 0)
    kw = dict(min_features=50, linearity_index_threshold=0.1, std_pxl=1.0)

    def reset():
        t = np.zeros(N, np.int32)
        _lib.check(_lib.lib.pre3_set_map(f._ctx, N, _lib.dptr(t)))
        f._refresh_map()
        f.set_x_p_k_k(x, P)
        f.set_book(book)
        f.sync()

    def keypoints():
        return f1.keypoints(c["frm1"], c["des1"], 0), f2.keypoints(c["frm2"], c["des2"], 0)

    def frames():
        return f.map_management_policy_frames_seeded(STEP, f1, f2, SEED, SEQ, 1.5, **kw)

    def frames_with_keypoints():
        keypoints()
        return frames()

    def chain():
        k1, k2 = keypoints()
        mt = pre3.siftmatch(k1["descriptors"], k2["descriptors"], 1.5)
        idx = mt[0].astype(np.int64) - 1
        out = f.map_management_policy_seeded(STEP, k1["frames"][:2, idx].T, k1["xyz"][:, idx].T, SEED, SEQ, cand_desc=k1["descriptors"][:, idx], **kw)
        out["match"] = mt
        return out

    reset(); ref = chain()
    reset(); got = frames_with_keypoints()
    assert np.array_equal(got["match"], ref["match"]) and all(np.array_equal(got[k], ref[k]) for k in ("deleted", "accepted", "order")), "the two forms disagree"
    forms = dict(frames=frames, frames_with_keypoints=frames_with_keypoints, chain=chain)
    wall, span = {k: [] for k in forms}, {k: [] for k in forms}
    for i in range(warmup + reps):
        for k, fn in forms.items():
            reset()
            f.timer_start()
            t0 = time.perf_counter()
            fn()
            f.sync()
            dt = time.perf_counter() - t0
            ms = f.timer_stop()
            if i >= warmup:
                wall[k].append(dt); span[k].append(ms * 1e-3)
    res = dict(N=N, n1=c["n1"], n2=c["n2"], pnum=int(got["K"]), n_deleted=int(len(got["deleted"])), n_accepted=int(len(got["accepted"])), examined=got["examined"],
               wall={k: quartiles(v) for k, v in wall.items()}, event_span={k: quartiles(v) for k, v in span.items()})
    res["ratio_chain_over_frames_with_keypoints"] = round(res["wall"]["chain"]["median_us"] / res["wall"]["frames_with_keypoints"]["median_us"], 2)
    f1.close(); f2.close(); f.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_policy_timing.json"))
    a = ap.parse_args()
    assert pre3.device_count() >= 1, "needs a HIP device"
    res = dict(rows=144, cols=176, reps=a.reps, warmup=a.warmup, sizes=[one_size(300, 280, 129, a.reps, a.warmup), one_size(2048, 2048, 700, a.reps, a.warmup)])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
