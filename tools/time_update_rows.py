"""What the in-place updates of the resident estimate cost (pre3_update_rows / pre3_heading_update):
  (a) device time per call (HIP events on the context's stream around 50 warmed calls; the heading update: median of brackets of 3 calls from a
      fresh state) of the heading update, of update() with r = 16 rows (the
      single-sweep form) and with r = 17 (the general route), at N = 500 and N = 2000 in fp32 and at N = 200 in fp64;
  (b) the bytes of P the single-sweep form reads and writes per call, over the call's time, against 6.0 TB/s of achievable HBM bandwidth;
  (c) with --profile: rocprofv3 --kernel-trace --stats of the same calls, from a run of its own (this script with --trace-only as the child).
Writes <out>/update_rows_timing.json and, with --profile, <out>/update_rows_kernel_stats.txt.

    python tools/time_update_rows.py [--out profiles] [--profile]
"""
import argparse
import glob
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

pre3 = importlib.import_module("3pre_amd")
synth = importlib.import_module("3pre_amd.synth")
_lib = importlib.import_module("3pre_amd._lib")
HBM = 6.0e12
REPS = 50
HEAD_BATCH = 3
CASES = ((500, "f32"), (2000, "f32"), (200, "f64"))


def _filter(N, dtype):
    x0, P0, _ = synth.make_map(N)
    f = pre3.EkfFilter(synth.CAM, np.zeros(N, np.int32), dtype=dtype, max_hyp=8)
    f.set_x_p_k_k(x0, P0)
    return f


def _ell(n, r, seed):
    """r rows of 13 non-zeros (pose block + one landmark), in the ELL form of the C ABI, with eye(r)"""
    rng = np.random.default_rng(seed)
    N = (n - 13) // 6
    nnz, col, val = np.full(r, 13, np.int32), np.zeros((r, 16), np.int32), np.zeros((r, 16))
    for a in range(r):
        o = 13 + 6 * int(rng.integers(N))
        col[a, :13] = list(range(7)) + list(range(o, o + 6))
        val[a, :13] = rng.normal(0, 30.0, 13)
    h = rng.normal(0, 1.0, r)
    return nnz, col, val, h + rng.normal(0, 0.5, r), h


def _timed(f, call, reps=REPS):
    for _ in range(5):
        call()
    f.timer_start()
    for _ in range(reps):
        call()
    return f.timer_stop() * 1e3 / reps                        # us per call


def _sweep_bytes(n, esz):
    """what k_rows_sweep moves: the upper-triangle 64 x 64 tiles read, every tile written (the mirror images off the diagonal)"""
    nT = -(-n // 64)
    t = nT * (nT + 1) // 2
    return t * 4096 * esz, (2 * t - nT) * 4096 * esz


def measure():
    out = {}
    for N, dtype in CASES:
        f = _filter(N, dtype)
        n, esz = f.n, 8 if dtype == "f64" else 4
        x0 = f.get_x_k_k()
        # The heading update from a fresh state, HEAD_BATCH calls per bracket: repeated heading updates collapse P's quaternion block within a few
        # calls (the numpy twin does the same), after which S is singular and the sweep returns early -- that would time nothing.  Planes 1.5
        # degrees either side of the camera, alternated.  (One event bracket costs ~12 us of stream time: ~2 us per call here.)
        Rps = [_lib.f64((synth.q2r(x0[3:7]) @ _rot(d)).ravel(order="F")) for d in (1.5, -1.5)]
        P0 = f.get_p_k_k()
        ts = []
        for b in range(REPS // HEAD_BATCH + 1):
            f.set_x_p_k_k(x0, P0)
            f.timer_start()
            for i in range(HEAD_BATCH):
                _lib.check(_lib.lib.pre3_heading_update(f._ctx, _lib.dptr(Rps[i % 2]), 1, None))
            t = f.timer_stop() * 1e3 / HEAD_BATCH
            f.get_x_k_k()                                     # (reads the device's error words: raises if an update found S not positive definite)
            if b > 0:                                         # (the first batch warms up)
                ts.append(t)
        res = {"n": n}
        res["heading_update_us"] = round(float(np.median(ts)), 1)
        f.set_x_p_k_k(x0, P0)
        for r in (16, 17):
            nnz, col, val, z, h = _ell(n, r, 7 + r)
            args = (f._ctx, r, 16, _lib.dptr(nnz), _lib.dptr(col), _lib.dptr(val), None, _lib.dptr(z), _lib.dptr(h))
            res["update_r%d_us" % r] = round(_timed(f, lambda: _lib.check(_lib.lib.pre3_update_rows(*args))), 1)
            res["update_r%d_form" % r] = f.rows_form()
            f.get_x_k_k()
        rd, wr = _sweep_bytes(n, esz)
        full = 2.0 * n * n * esz
        t16 = res["update_r16_us"] * 1e-6
        res["sweep_bytes_read"], res["sweep_bytes_written"] = rd, wr
        res["r16_sweep_GBps"] = round((rd + wr) / t16 / 1e9, 1)
        res["r16_time_at_6TBps_of_2n2_us"] = round(full / HBM * 1e6, 1)
        res["r16_over_2n2_at_6TBps"] = round(t16 / (full / HBM), 2)
        res["r16_beats_r17"] = res["update_r16_us"] < res["update_r17_us"]
        f.close()
        out["N=%d %s" % (N, dtype)] = res
        print(N, dtype, json.dumps(res), flush=True)
    return out


def _rot(deg):
    t = np.radians(deg)
    return np.array([[1, 0, 0], [0, np.cos(t), -np.sin(t)], [0, np.sin(t), np.cos(t)]])


def trace_only():
    """the calls alone, for rocprofv3 (--profile runs this as its child)"""
    for N, dtype in CASES:
        f = _filter(N, dtype)
        Rps = [_lib.f64(_rot(d).ravel(order="F")) for d in (1.5, -1.5)]
        for r in (16, 17):
            nnz, col, val, z, h = _ell(f.n, r, 7 + r)
            for _ in range(10):
                _lib.check(_lib.lib.pre3_update_rows(f._ctx, r, 16, _lib.dptr(nnz), _lib.dptr(col), _lib.dptr(val), None, _lib.dptr(z), _lib.dptr(h)))
        x0, P0 = f._get(0)
        for b in range(4):
            f.set_x_p_k_k(x0, P0)
            for i in range(HEAD_BATCH):
                _lib.check(_lib.lib.pre3_heading_update(f._ctx, _lib.dptr(Rps[i % 2]), 1, None))
            f.get_x_k_k()
        f.sync()
        f.close()


def profile(out_dir):
    tmp = os.path.join(out_dir, "_rocprof_update_rows")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "update_rows", "--", sys.executable, os.path.abspath(__file__), "--trace-only"]
    subprocess.run(cmd, check=True, timeout=600)
    csvs = sorted(glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True))
    assert csvs, "rocprofv3 wrote no kernel_stats.csv under %s" % tmp
    txt = open(csvs[-1]).read()
    print(txt, flush=True)
    with open(os.path.join(out_dir, "update_rows_kernel_stats.txt"), "w") as fh:
        fh.write("# rocprofv3 --kernel-trace --stats of tools/time_update_rows.py --trace-only: per case (N = 500 f32, 2000 f32, 200 f64) 10 x update() with\n")
        fh.write("# r = 16 (k_rows_hp + k_rows_sweep), 10 x with r = 17 (the general route), 4 x 3 heading updates from a fresh state; every kernel of the run\n")
        fh.write(txt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--profile", action="store_true", help="(c) only: the rocprofv3 pass")
    ap.add_argument("--trace-only", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.trace_only:
        trace_only()
        return
    os.makedirs(args.out, exist_ok=True)
    if args.profile:
        profile(args.out)
        return
    props = {}
    try:
        import torch
        props = {"device": torch.cuda.get_device_name(0)}
    except Exception:                                        # pragma: no cover
        pass
    res = {"measured": True, "box": props, "reps": REPS, "cases": measure()}
    with open(os.path.join(args.out, "update_rows_timing.json"), "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
