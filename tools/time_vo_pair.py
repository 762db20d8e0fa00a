#!/usr/bin/env python
"""Time the VO front end between two resident SR4000 frames on a 144 x 176 pair with about 300 kept keypoints per frame.

    pair:   vo.vo_pair_seeded(prev, cur, seed, seq) -- one call, one host wait
    chain:  what the same result took before it: SrFrame.keypoints (gate 1) read-back on both frames -> pre3.siftmatch on the kept descriptors ->
            SrFrame.planes() of both frames -> vo.vo_ransac_frames_seeded with n_hyp = rst worked out on the host
    pair_with_keypoints: the two keypoint calls followed by the pair call (the chain's keypoint stage is part of its time; this is the like-for-like line)

The two forms are alternated call by call behind --warmup warmed ones; median and quartiles over --reps calls; the clocks as found.  Both forms give
the same bits (tests/test_gpu_vo_pair.py); the tool checks the match list and u once.  No gate on these numbers.

    python tools/time_vo_pair.py [--reps 200] [--warmup 20] [--out profiles/vo_pair_timing.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vo_pair_timing.json"))
    a = ap.parse_args()
    pre3 = importlib.import_module("3pre_amd")
    srm, vo = pre3.sr4000, importlib.import_module("3pre_amd.vo")
    assert pre3.device_count() >= 1, "needs a HIP device"
    c = vp.make_pair(144, 176, 300, 280, 129, seed=13, drop1=40, drop2=30)
    f1, f2 = srm.SrFrame(), srm.SrFrame()
    f1.load(c["fr1"], 1); f2.load(c["fr2"], 1)
    seed, seq = 7, 1

    def keypoints():
        return f1.keypoints(c["frm1"], c["des1"], 1), f2.keypoints(c["frm2"], c["des2"], 1)

    def pair():
        return vo.vo_pair_seeded(f1, f2, seed, seq)

    def pair_with_keypoints():
        keypoints()
        return pair()

    def chain():
        k1, k2 = keypoints()
        mt = pre3.siftmatch(k1["descriptors"], k2["descriptors"], 1.5)
        x1, y1, z1, _ = f1.planes(); x2, y2, z2, _ = f2.planes()
        return vo.vo_ransac_frames_seeded(k1["frames"], k2["frames"], mt, x1, y1, z1, x2, y2, z2, seed, seq, n_hyp=vo.vo_rst(mt.shape[1])), mt

    ref, mt = chain()
    got = pair_with_keypoints()
    assert np.array_equal(got["match"], mt) and np.array_equal(got["u"], ref["u"]) and np.array_equal(got["cnum"], ref["cnum"]), "the two forms disagree"
    forms = dict(pair=pair, pair_with_keypoints=pair_with_keypoints, chain=chain)
    for _ in range(a.warmup):
        for fn in forms.values():
            fn()
    ts = {k: [] for k in forms}
    for _ in range(a.reps):
        for k, fn in forms.items():
            t0 = time.perf_counter()
            fn()
            ts[k].append(time.perf_counter() - t0)
    res = dict(rows=144, cols=176, n1=c["n1"], n2=c["n2"], pnum=int(got["pnum"]), rst=int(got["rst"]), reps=a.reps, warmup=a.warmup,
               timing={k: quartiles(v) for k, v in ts.items()})
    res["ratio_chain_over_pair_with_keypoints"] = round(res["timing"]["chain"]["median_us"] / res["timing"]["pair_with_keypoints"]["median_us"], 2)
    res["ratio_chain_over_pair"] = round(res["timing"]["chain"]["median_us"] / res["timing"]["pair"]["median_us"], 2)
    f1.close(); f2.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
