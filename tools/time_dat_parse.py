"""What the device parse of a .dat frame buys (pre3_sr_frame_load_text), at 144 x 176 with a confidence map and the timestamp row
(721 lines of 176 tokens), for the three number formats .dat writers use (%.6f, %.7e = MATLAB's save -ascii, %.16e = save -ascii -double):
  (A) the host parse: numpy.loadtxt on the file's bytes, then SrFrame.load, then a synchronise;
  (B) SrFrame.load_text on the same bytes, then a synchronise;
alternated in one process on one handle, the order swapped every round; a host clock around work that ends in a synchronise; median and quartiles of
CALLS calls each after WARMUP rounds.  numpy.loadtxt's own share of (A) is reported too.  The gate: (B)'s median below (A)'s for every format.
  with --profile: rocprofv3 --kernel-trace --memory-copy-trace --stats of 10 load_text calls per format, in a run of its own (this script with
  --trace-only as the child): the three parse kernels, the two conditioning kernels and the copies.
Writes <out>/dat_parse_timing.json and, with --profile, <out>/dat_parse_kernel_stats.txt.

    python tools/time_dat_parse.py [--out profiles] [--profile]
"""
import argparse
import glob
import importlib
import io
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

srm = importlib.import_module("3pre_amd.sr4000")
_lib = importlib.import_module("3pre_amd._lib")
ROWS, COLS, CALLS, WARMUP = 144, 176, 30, 5
FORMATS = ("%.6f", "%.7e", "%.16e")


def frame_text(fmt, seed=0):
    """a synthetic frame of realistic values: metres for z, x, y, 16-bit amplitudes and confidences, the timestamp row"""
    rng = np.random.default_rng(seed)
    z, x, y = rng.uniform(0.5, 4.0, (ROWS, COLS)), rng.uniform(-1.5, 1.5, (ROWS, COLS)), rng.uniform(-1.0, 1.0, (ROWS, COLS))
    amp, conf = np.floor(rng.uniform(0.0, 30000.0, (ROWS, COLS))), np.floor(rng.uniform(0.0, 65535.0, (ROWS, COLS)))
    a = np.vstack([z, x, y, amp, conf, np.r_[1234567.875, np.zeros(COLS - 1)]])
    buf = io.BytesIO()
    np.savetxt(buf, a, fmt=fmt)
    return buf.getvalue()


def sync(f):
    _lib.check(_lib.lib.pre3_sr_frame_get(f._h, None, None, None, None, None, None, None))      # nothing copied: the stream's synchronise alone


def host_path(f, text):
    a = np.loadtxt(io.BytesIO(text), dtype=np.float64, ndmin=2)
    d = {k: np.asfortranarray(a[i * ROWS:(i + 1) * ROWS]) for i, k in enumerate(("z", "x", "y", "amp", "conf"))}
    f.load(d, srm.MODE_XYZ)
    sync(f)


def device_path(f, text):
    f.load_text(text, srm.MODE_XYZ)
    sync(f)


def quartiles(ms):
    q = np.percentile(ms, [25, 50, 75])
    return dict(q25_ms=float(q[0]), median_ms=float(q[1]), q75_ms=float(q[2]))


def measure():
    out = {}
    with srm.SrFrame(ROWS, COLS) as f:
        for fmt in FORMATS:
            text = frame_text(fmt)
            t = {"host": [], "device": [], "loadtxt": []}
            for r in range(WARMUP + CALLS):
                order = (("host", host_path), ("device", device_path)) if r % 2 == 0 else (("device", device_path), ("host", host_path))
                for name, call in order:
                    t0 = time.perf_counter()
                    call(f, text)
                    t[name].append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                np.loadtxt(io.BytesIO(text), dtype=np.float64, ndmin=2)
                t["loadtxt"].append((time.perf_counter() - t0) * 1e3)
            res = {k: quartiles(v[WARMUP:]) for k, v in t.items()}
            res["bytes"] = len(text)
            res["ratio_host_over_device"] = res["host"]["median_ms"] / res["device"]["median_ms"]
            res["gate_device_below_host"] = bool(res["device"]["median_ms"] < res["host"]["median_ms"])
            out[fmt] = res
    return out


def trace_only():
    with srm.SrFrame(ROWS, COLS) as f:
        for fmt in FORMATS:
            text = frame_text(fmt)
            for _ in range(10):
                device_path(f, text)


def profile(out_dir):
    tmp = os.path.join(out_dir, "_rocprof_dat_parse")
    cmd = ["rocprofv3", "--kernel-trace", "--memory-copy-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "dat_parse", "--", sys.executable,
           os.path.abspath(__file__), "--trace-only"]
    subprocess.run(cmd, check=True, timeout=600)
    with open(os.path.join(out_dir, "dat_parse_kernel_stats.txt"), "w") as fh:
        fh.write("# rocprofv3 --kernel-trace --memory-copy-trace --stats of tools/time_dat_parse.py --trace-only: 10 x SrFrame.load_text per format\n")
        fh.write("# (%s) at 144 x 176 with a confidence map and the timestamp row, one handle\n" % ", ".join(FORMATS))
        for kind in ("kernel_stats", "memory_copy_stats"):
            csvs = sorted(glob.glob(os.path.join(tmp, "**", "*%s.csv" % kind), recursive=True))
            assert csvs or kind != "kernel_stats", "rocprofv3 wrote no kernel_stats.csv under %s" % tmp
            for c in csvs[-1:]:
                txt = open(c).read()
                print(txt, flush=True)
                fh.write("# %s\n%s" % (kind, txt))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--profile", action="store_true", help="the rocprofv3 pass only")
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
    res = {"measured": True, "box": props, "shape": [ROWS, COLS], "calls": CALLS, "warmup": WARMUP, "results": measure()}
    print(json.dumps(res, indent=1))
    with open(os.path.join(args.out, "dat_parse_timing.json"), "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
