#!/usr/bin/env python
"""Time the patch branch of the IC search (pre3_patch_search) at N = 500 on 144 x 176 and 240 x 320 with S of sigma 2 .. 4 px:
the per-call time, the two kernels' times under pre3_kernel_timing, and the numpy restatement's time on the CPU beside them.
Writes profiles/patch_search_timing.json.  Gates nothing."""
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle as orc          # noqa: E402
import patch_cases as pc      # noqa: E402

pre3 = importlib.import_module("3pre_amd")


def run(shape, N=500, reps=50, dtype="f32"):
    rng = np.random.default_rng(17)
    sc = pc.build_scene(orc, shape[0], shape[1], pc.spec_random(rng, shape[0], shape[1], N, sig=(2.0, 4.0)), seed=18)
    f = pre3.EkfFilter(pc.cam_list(sc["cam"]), sc["types"], dtype=dtype, max_hyp=16, max_landmarks=N)
    f.set_x_p_k_km1(sc["x"], sc["P"])
    f.set_image(sc["imB"])
    b = sc["bank"]
    f.set_patches(b["patch"], b["uv_init"], b["r_wc"], b["R_wc"])
    out = {"shape": list(shape), "N": N, "dtype": dtype}
    for strict in (0, 1):
        for _ in range(5):
            res = f.search_ic_matches_patch(pc.FD_FORK, 0.6, strict_reference=bool(strict))
        f.sync()
        t0 = time.perf_counter()
        for _ in range(reps):
            f.search_ic_matches_patch(pc.FD_FORK, 0.6, strict_reference=bool(strict))
        call_us = (time.perf_counter() - t0) / reps * 1e6
        f.kernel_timing(1)
        kw, ks = [], []
        for _ in range(10):
            f.search_ic_matches_patch(pc.FD_FORK, 0.6, strict_reference=bool(strict))
            a, s = f.patch_timing()
            kw.append(a * 1e3)
            ks.append(s * 1e3)
        f.kernel_timing(0)
        t0 = time.perf_counter()
        lf = f.landmark_fields()
        r = pc.reference(sc, sc["imB"], 0.6, strict, h=lf["h"], has_h=lf["has_h"], S=lf["S"], x=f.get_x_k_km1())
        cpu_ms = (time.perf_counter() - t0) * 1e3
        out["strict_%d" % strict] = dict(call_us=call_us, k_patch_warp_us=float(np.median(kw)), k_patch_search_us=float(np.median(ks)),
                                         numpy_restatement_ms=cpu_ms, matched=int(len(res[0])), candidates_mean=float(res[3].mean()),
                                         same_matches_as_restatement=bool(np.array_equal(res[0], r["meas_idx"])))
    f.close()
    return out


if __name__ == "__main__":
    orc.build()
    res = {"runs": [run((144, 176)), run((240, 320))]}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "patch_search_timing.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))
