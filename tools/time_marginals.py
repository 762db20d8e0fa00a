"""What the marginal readers (pre3_get_landmarks / pre3_get_marginal) cost, against get_p_k_k():
  (a) wall time of landmarks(), pose(), marginal() of one landmark block and get_p_k_k() at N = 500 and N = 2000, fp32;
  (b) headline-sequence steps/s (synth.HEADLINE, defer_hi_update + pend_hi, 200 steps) with a pose() + landmarks() read behind every step, and without;
  (c) with --profile: one rocprofv3 --kernel-trace --stats line per new kernel, from a run of its own (this script with --trace-only as the child).
Writes <out>/marginals_timing.json and, with --profile, <out>/marginals_kernel_stats.txt.

    python tools/time_marginals.py [--out profiles] [--profile]
"""
import argparse
import glob
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

pre3 = importlib.import_module("3pre_amd")
synth = importlib.import_module("3pre_amd.synth")


def _filter(N, seed=1):
    seq = synth.make_sequence(N, 1, 8, seed=seed)
    f = pre3.EkfFilter(seq["cam"], np.zeros(N, np.int32), dtype="f32", max_hyp=8)
    f.set_x_p_k_k(seq["x0"], seq["P0"])
    return f


def _wall(fn, reps):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    ts = np.array(ts) * 1e6
    return {"median_us": round(float(np.median(ts)), 1), "min_us": round(float(ts.min()), 1), "reps": reps}


def reads(Ns=(500, 2000)):
    out = {}
    for N in Ns:
        f = _filter(N)
        blk = 13 + 6 * (N // 2) + np.arange(6)
        out["N=%d" % N] = {
            "n": 13 + 6 * N,
            "landmarks()": _wall(lambda: f.landmarks(), 50),
            "pose()": _wall(lambda: f.pose(), 50),
            "marginal(one landmark block)": _wall(lambda: f.marginal(blk), 50),
            "get_p_k_k()": _wall(lambda: f.get_p_k_k(), 10 if N > 1000 else 20),
        }
        f.close()
        print(N, json.dumps(out["N=%d" % N]), flush=True)
    return out


def headline(steps=200, warm=5, rounds=2):
    N, n_hyp = 500, 200
    seq = synth.make_sequence(N, steps + warm, n_hyp, motion_noise=synth.HEADLINE["motion_noise"])
    thr = synth.HEADLINE["threshold"]
    res = {"without reads": [], "pose() + landmarks() behind every step": []}
    for _ in range(rounds):                                  # (alternated: the two forms see the same box state)
        for form in res:
            f = pre3.EkfFilter(seq["cam"], np.zeros(N, np.int32), dtype="f32", max_hyp=n_hyp, std_z=thr)
            f.set_x_p_k_k(seq["x0"], seq["P0"])
            assert f.pend_hi(True)
            f.defer_hi_update(True)
            read = form != "without reads"
            for s in seq["steps"][:warm]:
                f.step(s["u"], s["meas_idx"], s["z"], s["hyp"], threshold=thr, early_exit=False)
            f.sync()
            t = time.perf_counter()
            for s in seq["steps"][warm:]:
                f.step(s["u"], s["meas_idx"], s["z"], s["hyp"], threshold=thr, early_exit=False)
                if read:
                    f.pose()
                    f.landmarks()
            f.sync()
            el = time.perf_counter() - t
            f.close()
            res[form].append(round(steps / el, 1))
    out = {k: {"steps_per_s": v, "best": max(v)} for k, v in res.items()}
    print(json.dumps(out), flush=True)
    return out


def trace_only():
    """the readers alone, for rocprofv3 (--profile runs this as its child)"""
    for N in (500, 2000):
        f = _filter(N)
        blk = 13 + 6 * (N // 2) + np.arange(6)
        for _ in range(20):
            f.landmarks()
            f.pose()
            f.marginal(blk)
        f.close()


def profile(out_dir):
    tmp = os.path.join(out_dir, "_rocprof_marginals")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "marginals", "--", sys.executable, os.path.abspath(__file__), "--trace-only"]
    subprocess.run(cmd, check=True, timeout=600)
    csvs = sorted(glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True))
    assert csvs, "rocprofv3 wrote no kernel_stats.csv under %s" % tmp
    lines = open(csvs[-1]).read().splitlines()
    keep = [lines[0]] + [ln for ln in lines[1:] if "k_read_landmarks" in ln or "k_read_marginal" in ln]
    txt = "\n".join(keep) + "\n"
    print(txt, flush=True)
    with open(os.path.join(out_dir, "marginals_kernel_stats.txt"), "w") as fh:
        fh.write("# rocprofv3 --kernel-trace --stats of tools/time_marginals.py --trace-only: 20 x (landmarks(), pose(), marginal(one landmark block)) at N = 500 and\n")
        fh.write("# at N = 2000 (fp32, nothing pending); the readers' kernels only\n")
        fh.write(txt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--profile", action="store_true", help="(c) only: the rocprofv3 pass")
    ap.add_argument("--trace-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--steps", type=int, default=200)
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
    res = {"measured": True, "box": props,
           "reads_fp32": reads(), "headline_%d_steps" % args.steps: headline(args.steps)}
    with open(os.path.join(args.out, "marginals_timing.json"), "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
