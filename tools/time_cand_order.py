"""What the candidates' weighted order costs on the device and saves on the host (k_cand_keys, k_cand_rank), at K = 300 / 700 /
8192 candidates on an N = 500 fp32 map:
  map_management_policy_seeded  next to  a host draw (numpy weights + Generator.choice without replacement, the Plackett-Luce draw a caller would
  write) + the permutation of the three candidate arrays + map_management_policy.
The two forms are alternated in one process from the same restored state (the seeded one first on even rounds); wall times are reported as median and
quartiles over the rounds, with the host draw + permutation's own share.  With --profile: rocprofv3 --kernel-trace --stats of the seeded calls from
runs of their own, one per K (this script with --trace-only K as the child); the two kernels' device times are taken from its table and added to the JSON.
Writes <out>/cand_order_timing.json and, with --profile, <out>/cand_order_kernel_stats.txt.

    python tools/time_cand_order.py [--out profiles] [--profile]
"""
import argparse
import csv
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
_lib = importlib.import_module("3pre_amd._lib")
ROUNDS, WARM = 30, 4
SEED = 2024
SIZES = (300, 700, 8192)
N_MAP, STEP = 500, 25
BOX = (176, 144)


def _q(v):
    v = np.asarray(v, dtype=float)
    return {"median": round(float(np.median(v)), 1), "q25": round(float(np.percentile(v, 25)), 1), "q75": round(float(np.percentile(v, 75)), 1)}


def _setup(K):
    rng = np.random.default_rng(N_MAP + K)
    x, P, _ = synth.make_map(N_MAP, seed=N_MAP)
    cam = synth.CAM
    book = np.stack([rng.integers(0, 8, N_MAP), rng.integers(0, 8, N_MAP), rng.integers(3, STEP, N_MAP), rng.integers(3, STEP, N_MAP)], 1).astype(np.int32)
    uv = np.stack([rng.uniform(3, cam[6] - 3, K), rng.uniform(3, cam[5] - 3, K)], 1)
    xyz = np.tile([0.0, 0.0, 2.0], (K, 1)) * rng.uniform(0.5, 2.0, (K, 1))
    desc = rng.integers(0, 255, (K, 128)).astype(float)
    f = pre3.EkfFilter(cam, np.zeros(N_MAP, np.int32), dtype="f32", max_landmarks=N_MAP + 100)
    return f, x, P, book, uv, xyz, desc


def _reset(f, x, P, book):
    t = np.zeros(N_MAP, np.int32)
    _lib.check(_lib.lib.pre3_set_map(f._ctx, N_MAP, _lib.dptr(t)))
    f._refresh_map()
    f.set_x_p_k_k(x, P)
    f.set_book(book)
    f.sync()


def host_draw(rng, uv):
    """Weighted_Smpl_wo_replacement.m as a caller writes it in numpy"""
    du, dv = (uv[:, 0] - 88.0) / 29.0, (uv[:, 1] - 72.0) / 24.0
    w = np.exp(-0.5 * (du * du + dv * dv))
    return rng.choice(len(w), size=len(w), replace=False, p=w / w.sum())


def policy_forms(K, rounds=ROUNDS):
    f, x, P, book, uv, xyz, desc = _setup(K)
    rng = np.random.default_rng(1)
    kw = dict(min_features=50, linearity_index_threshold=0.1)
    ts, th, td = [], [], []
    for r in range(-WARM, rounds):
        for which in ((0, 1) if r % 2 == 0 else (1, 0)):
            _reset(f, x, P, book)
            t0 = time.perf_counter()
            if which == 0:
                f.map_management_policy_seeded(STEP, uv, xyz, SEED, r + WARM, cand_desc=desc, box=BOX, **kw)
                f.sync()
                if r >= 0:
                    ts.append((time.perf_counter() - t0) * 1e6)
            else:
                o = host_draw(rng, uv)
                a, b, d = uv[o], xyz[o], desc[o]
                t1 = time.perf_counter()
                f.map_management_policy(STEP, a, b, d, **kw)
                f.sync()
                if r >= 0:
                    th.append((time.perf_counter() - t0) * 1e6); td.append((t1 - t0) * 1e6)
    f.close()
    return {"seeded_wall_us": _q(ts), "host_draw_wall_us": _q(th), "of_which_host_draw_and_permutation_us": _q(td),
            "host_minus_seeded_us": _q(np.array(th) - np.array(ts))}


def trace_only(K):
    f, x, P, book, uv, xyz, desc = _setup(K)
    for s in range(10):
        _reset(f, x, P, book)
        f.map_management_policy_seeded(STEP, uv, xyz, SEED, s, cand_desc=desc, box=BOX, min_features=50, linearity_index_threshold=0.1)
    f.sync()
    f.close()
    for s in range(10):
        synth.candidate_order(uv, SEED, s, box=BOX)


def profile(out_dir):
    dev, texts = {}, []
    for K in SIZES:
        tmp = os.path.join(out_dir, "_rocprof_cand_order_%d" % K)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "cand_order", "--", sys.executable, os.path.abspath(__file__),
               "--trace-only", str(K)]
        subprocess.run(cmd, check=True, timeout=300)
        csvs = sorted(glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True))
        assert csvs, "rocprofv3 wrote no kernel_stats.csv under %s" % tmp
        txt = open(csvs[-1]).read()
        print(txt, flush=True)
        texts.append("# K = %d\n%s" % (K, txt))
        dev[str(K)] = {}
        for row in csv.DictReader(open(csvs[-1])):
            name = row.get("Name", "")
            for k in ("k_cand_keys", "k_cand_rank", "k_policy_prefilter", "k_policy_walk"):
                if k in name:
                    dev[str(K)][k] = {"calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 2), "min_us": round(float(row["MinNs"]) / 1e3, 2),
                                      "max_us": round(float(row["MaxNs"]) / 1e3, 2)}
    with open(os.path.join(out_dir, "cand_order_kernel_stats.txt"), "w") as fh:
        fh.write("# rocprofv3 --kernel-trace --stats of tools/time_cand_order.py --trace-only K: 10 x map_management_policy_seeded (N = 500 fp32) and\n")
        fh.write("# 10 x synth.candidate_order, K candidates each; one run per K\n")
        fh.write("\n".join(texts))
    path = os.path.join(out_dir, "cand_order_timing.json")
    res = json.load(open(path)) if os.path.exists(path) else {"measured": True, "results": {}}
    res["kernel_device_us"] = dev
    with open(path, "w") as fh:
        json.dump(res, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--profile", action="store_true", help="the rocprofv3 pass only")
    ap.add_argument("--trace-only", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.trace_only:
        trace_only(args.trace_only)
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
    res = {"measured": True, "box": props, "rounds": ROUNDS, "N": N_MAP,
           "results": {"K%d" % K: policy_forms(K, ROUNDS if K < 8192 else 12) for K in SIZES}}
    path = os.path.join(args.out, "cand_order_timing.json")
    if os.path.exists(path):
        old = json.load(open(path))
        if "kernel_device_us" in old:
            res["kernel_device_us"] = old["kernel_device_us"]
    print(json.dumps(res, indent=1))
    with open(path, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
