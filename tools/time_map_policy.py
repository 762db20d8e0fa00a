"""Time pre3_map_policy against pre3_map_management with the same lists, and the per-step cost of the rescue-visibility
rider on a booked context.

    python tools/time_map_policy.py [--out profiles/map_policy_timing.json] [--reps 5]

Wall-clock times per call (median over reps; each rep restores the map, the state and the book first).  For device times run it under
`rocprofv3 --kernel-trace --stats -- python tools/time_map_policy.py` and read k_policy_* / k_book_vis / k_map_one in the stats file."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pre3 = importlib.import_module("3pre_amd")
synth = importlib.import_module("3pre_amd.synth")
_lib = importlib.import_module("3pre_amd._lib")


def _reset(f, N, x, P, book):
    t = np.zeros(N, np.int32)
    _lib.check(_lib.lib.pre3_set_map(f._ctx, N, _lib.dptr(t)))
    f._refresh_map()
    f.set_x_p_k_k(x, P)
    f.set_book(book)
    f.sync()


def policy_vs_management(N, K, reps):
    rng = np.random.default_rng(N + K)
    x, P, _ = synth.make_map(N, seed=N)
    cam = synth.CAM
    step = 25
    book = np.stack([rng.integers(0, 8, N), rng.integers(0, 8, N), rng.integers(3, step, N), rng.integers(3, step, N)], 1).astype(np.int32)
    W, H = cam[6], cam[5]
    uv = np.stack([rng.uniform(3, W - 3, K), rng.uniform(3, H - 3, K)], 1)
    xyz = np.tile([0.0, 0.0, 2.0], (K, 1)) * rng.uniform(0.5, 2.0, (K, 1))
    f = pre3.EkfFilter(cam, np.zeros(N, np.int32), dtype="f32", max_landmarks=N + 100)
    tp, tm, out = [], [], None
    for _ in range(reps):
        _reset(f, N, x, P, book)
        t0 = time.perf_counter()
        out = f.map_management_policy(step, uv, xyz, min_features=50, linearity_index_threshold=0.1)
        f.sync()
        tp.append(time.perf_counter() - t0)
    rho = 1.0 / np.linalg.norm(xyz, axis=1)
    for _ in range(reps):
        _reset(f, N, x, P, book)
        t0 = time.perf_counter()
        f.map_management(out["deleted"], uv[out["accepted"]], std_pxl=1.0, initial_rho=rho[out["accepted"]], linearity_index_threshold=0.1)
        f.sync()
        tm.append(time.perf_counter() - t0)
    f.close()
    return dict(N=N, K=K, policy_us=1e6 * float(np.median(tp)), map_management_us=1e6 * float(np.median(tm)), n_deleted=int(len(out["deleted"])),
                n_accepted=int(len(out["accepted"])), examined=out["examined"], target=out["target"])


def rider(steps=40, warm=5):
    N, n_hyp = 500, 200
    seq = synth.make_sequence(N, warm + steps, n_hyp, motion_noise=synth.HEADLINE["motion_noise"])
    res = {}
    for booked in (False, True):
        f = pre3.EkfFilter(seq["cam"], np.zeros(N, np.int32), dtype="f32", max_hyp=n_hyp)
        f.set_x_p_k_k(seq["x0"], seq["P0"])
        if booked:
            f.set_book(np.tile([0, 0, 2, 2], (N, 1)))
        for s in seq["steps"][:warm]:
            f.step(s["u"], s["meas_idx"], s["z"], s["hyp"], threshold=synth.HEADLINE["threshold"])
        f.sync()
        t0 = time.perf_counter()
        for s in seq["steps"][warm:]:
            f.step(s["u"], s["meas_idx"], s["z"], s["hyp"], threshold=synth.HEADLINE["threshold"])
        f.sync()
        res["booked" if booked else "unbooked"] = 1e6 * (time.perf_counter() - t0) / steps
        f.close()
    res["rider_us_per_step_wall"] = res["booked"] - res["unbooked"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    out = dict(calls=[policy_vs_management(N, K, a.reps) for N in (500, 2000) for K in (300, 700)], rider_step_us=rider())
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(txt + "\n")


if __name__ == "__main__":
    main()
