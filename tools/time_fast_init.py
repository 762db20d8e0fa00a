#!/usr/bin/env python
"""Time FAST-9 corners and the patch-feature initialisation on the device (pre3_fast_detect, pre3_init_feature_fast_seeded,
pre3_init_features_fast_all) at 144 x 176 (the fixture's crop of a real image) and 240 x 320 (the crop tiled) with a map of 50
landmarks: the per-call time, the launches' event-bracketed time under pre3_kernel_timing, and the numpy restatement (tests/fast_ref.py) on one
core beside them.
Writes profiles/fast_init_timing.json.  Gates nothing."""
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
import fast_ref as fr         # noqa: E402
import patch_cases as pc      # noqa: E402

pre3 = importlib.import_module("3pre_amd")
srm = importlib.import_module("3pre_amd.sr4000")
_lib = importlib.import_module("3pre_amd._lib")


def med(v):
    return float(np.median(v))


def run(shape, N=50, dtype="f32"):
    rng = np.random.default_rng(23)
    sc = pc.build_scene(orc, shape[0], shape[1], pc.spec_random(rng, shape[0], shape[1], N), seed=24, moved=False)
    crop = np.load(os.path.join(ROOT, "tests", "golden", "fast_lab_crop.npz"))["image"]
    im = np.ascontiguousarray(np.tile(crop, (2, 2))[:shape[0], :shape[1]])
    planes = dict(z=rng.uniform(1.0, 5.0, shape), x=rng.uniform(-2, 2, shape), y=rng.uniform(-2, 2, shape), amp=rng.uniform(100, 30000, shape),
                  conf=rng.uniform(0.8, 1.0, shape))
    out = {"shape": list(shape), "N": N, "dtype": dtype}

    def ctx(extra):
        f = pre3.EkfFilter(pc.cam_list(sc["cam"]), sc["types"], dtype=dtype, max_hyp=16, max_landmarks=N + extra)
        f.set_x_p_k_k(sc["x"], sc["P"])
        f.set_image(im)
        return f

    with srm.SrFrame(*shape) as fh:
        fh.load(planes)
        x, y, z, conf = fh.planes()
        rp = dict(x=x, y=y, z=z, conf=conf, cmax=fh.maxima()[1])
        # ---- the detector on the whole image: suppressed list at (10, 20) and at (5, 20)
        f = ctx(0)
        for t in (10, 5):
            for _ in range(5):
                got = f.fast_nonmax(t, 20)
            f.sync()
            t0 = time.perf_counter()
            for _ in range(50):
                f.fast_nonmax(t, 20)
            call_us = (time.perf_counter() - t0) / 50 * 1e6
            f.kernel_timing(1)
            k = []
            for _ in range(10):
                f.fast_nonmax(t, 20)
                k.append(f.fast_timing() * 1e3)
            f.kernel_timing(0)
            t0 = time.perf_counter()
            ref = fr.fast_nonmax(im, t, 20)
            cpu_ms = (time.perf_counter() - t0) * 1e3
            out["fast_detect_t%d" % t] = dict(call_us=call_us, k_fast_strip_emit_us=med(k), numpy_restatement_ms=cpu_ms, maxima=int(len(got[0])),
                                              corners=int(len(fr.fast_corner_detect_9(im, t))), same_as_restatement=bool(np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])))
        f.close()
        # ---- initialize_a_feature, seeded: the call (projection + k_fast_box + the wait, then the map call and the patch cut queued behind it)
        f = ctx(40)
        calls, kern, stats = [], [], []
        for seq in range(36):
            timed = seq >= 24
            f.kernel_timing(1 if timed else 0)
            f.sync()
            t0 = time.perf_counter()
            r = f.initialize_a_feature_seeded(fh, 1.0, 7, seq)
            dt = (time.perf_counter() - t0) * 1e6
            if timed:
                kern.append(f.fast_timing() * 1e3)
            elif seq >= 4:
                calls.append(dt)
            stats.append(r["status"])
        f.kernel_timing(0)
        f.sync()
        f.predict_camera_measurements(which=_lib.X_K_K)
        lf = f.landmark_fields()
        t0 = time.perf_counter()
        fr.initialize_a_feature(im, rp, lf["h"][lf["has_h"] != 0], fr.seeded_centres(7, 99, *shape))
        cpu_ms = (time.perf_counter() - t0) * 1e3
        out["init_feature_fast_seeded"] = dict(call_us=med(calls), k_fast_box_us=med(kern), numpy_restatement_ms=cpu_ms, initialised=int(sum(s == 0 for s in stats)), calls=len(stats))
        f.close()
        # ---- initialize_n_features_fast: a fresh context per call (every call fills the map)
        t0 = time.perf_counter()
        uv, verdict, rho = fr.initialize_n_features_fast(im, rp)
        cpu_ms = (time.perf_counter() - t0) * 1e3
        n = int((verdict == 0).sum())
        calls, kern = [], []
        for rep in range(6):
            f = ctx(n)
            f.kernel_timing(1 if rep >= 3 else 0)
            f.sync()
            t0 = time.perf_counter()
            got = f.initialize_n_features_fast(fh, 1.0)
            f.sync()
            dt = (time.perf_counter() - t0) * 1e6
            (kern if rep >= 3 else calls).append(f.fast_timing() * 1e3 if rep >= 3 else dt)
            f.close()
        out["init_features_fast_all"] = dict(call_and_queued_work_us=med(calls[1:]), k_fast_strip_emit_gate_us=med(kern), numpy_restatement_ms=cpu_ms, maxima=int(len(uv)), added=n,
                                             same_as_restatement=bool(np.array_equal(got["uv"], uv) and got["n_added"] == n))
    return out


if __name__ == "__main__":
    orc.build()
    res = {"runs": [run((144, 176)), run((240, 320))]}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "fast_init_timing.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))
