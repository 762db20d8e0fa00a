"""What the seeded draw tables cost and save (pre3_draws.hip), at the reference's sizes:
  1-point  200 draws at N = 500 / 400 measurements: step_predicted_seeded next to synth.draw_hypotheses + step_predicted
  VO       rst = 700 at pnum = 60:                  vo_ransac_seeded      next to vo.draw_hypotheses + vo_ransac
  plane    1001 draws on the default 65 x 71 box:   plane_fit_seeded      next to plane.draw_plane_hypotheses + plane_fit
Per RANSAC the two call forms are alternated in one process from the same state (the seeded one first on even rounds) and the wall times reported as
median and quartiles over the rounds, with the host draws' own share.  With --profile: rocprofv3 --kernel-trace --stats of the seeded calls from a
run of its own (this script with --trace-only as the child); the draw kernels' device times are taken from its table and added to the JSON.
Writes <out>/seeded_draws_timing.json and, with --profile, <out>/seeded_draws_kernel_stats.txt.

    python tools/time_seeded_draws.py [--out profiles] [--profile]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import plane_fit_ref as pr  # noqa: E402

pre3 = importlib.import_module("3pre_amd")
synth = importlib.import_module("3pre_amd.synth")
plane = importlib.import_module("3pre_amd.plane")
vo = importlib.import_module("3pre_amd.vo")
ROUNDS, WARM = 30, 4
SEED = 2024


def _q(v):
    v = np.asarray(v, dtype=float)
    return {"median": round(float(np.median(v)), 1), "q25": round(float(np.percentile(v, 25)), 1), "q75": round(float(np.percentile(v, 75)), 1)}


def _alternate(seeded, host, rounds=ROUNDS):
    """seeded() -> wall us; host() -> (wall us, us of it spent drawing on the host)"""
    ts, th, td = [], [], []
    for r in range(-WARM, rounds):
        order = (0, 1) if r % 2 == 0 else (1, 0)
        for which in order:
            if which == 0:
                v = seeded()
                if r >= 0:
                    ts.append(v)
            else:
                v, d = host()
                if r >= 0:
                    th.append(v); td.append(d)
    return {"seeded_wall_us": _q(ts), "host_draws_wall_us": _q(th), "of_which_host_draws_us": _q(td), "host_minus_seeded_us": _q(np.array(th) - np.array(ts))}


def _one_point_setup(N=500, M=400, n_draw=200):
    x0, P0, _ = synth.make_map(N)
    uv, vis = synth.pixels(x0[:7], x0[13:].reshape(N, 6))
    idx = np.nonzero(vis)[0][:M].astype(np.int32)
    f = pre3.EkfFilter(synth.CAM, np.zeros(N, np.int32), dtype="f32", max_hyp=n_draw)
    f.set_x_p_k_km1(x0, P0)
    f.sync()
    return f, x0, P0, idx, uv[idx], n_draw


def one_point():
    f, x0, P0, idx, z, n_draw = _one_point_setup()
    rng = np.random.default_rng(1)
    seq = [0]

    def prep():
        f.set_x_p_k_km1(x0, P0)
        f.search_IC_matches()
        f.set_measurements(idx, z)
        f.sync()

    def seeded():
        prep()
        seq[0] += 1
        t0 = time.perf_counter()
        f.step_predicted_seeded(SEED, seq[0], n_draw, threshold=1.0, early_exit=False)
        f.sync()
        return (time.perf_counter() - t0) * 1e6

    def host():
        prep()
        t0 = time.perf_counter()
        hyp = synth.draw_hypotheses(rng, len(idx), n_draw)
        t1 = time.perf_counter()
        f.step_predicted(hyp, threshold=1.0, early_exit=False)
        f.sync()
        t2 = time.perf_counter()
        return (t2 - t0) * 1e6, (t1 - t0) * 1e6

    out = _alternate(seeded, host)
    f.close()
    return out


def _vo_setup(pnum=60):
    from test_vo_oracle import scene
    rng, R, T, p1, p2, match, bad = scene(pnum, 3)
    return rng, p1, p2, match


def vo_ransac():
    rng, p1, p2, match = _vo_setup()
    seq = [0]

    def seeded():
        seq[0] += 1
        t0 = time.perf_counter()
        vo.vo_ransac_seeded(p1, p2, match, SEED, seq[0])
        return (time.perf_counter() - t0) * 1e6

    def host():
        t0 = time.perf_counter()
        d = vo.draw_hypotheses(match, vo.vo_rst(match.shape[1]), rng)
        t1 = time.perf_counter()
        vo.vo_ransac(p1, p2, d)
        t2 = time.perf_counter()
        return (t2 - t0) * 1e6, (t1 - t0) * 1e6

    return _alternate(seeded, host)


def plane_fit():
    x, y, z, _ = pr.scene(1, 0.5)
    XYZ = plane.crop_points(x, y, z)[3]
    rng = np.random.default_rng(2)
    seq = [0]

    def seeded():
        seq[0] += 1
        t0 = time.perf_counter()
        plane.plane_fit_seeded(x, y, z, SEED, seq[0])
        return (time.perf_counter() - t0) * 1e6

    def host():
        t0 = time.perf_counter()
        d = plane.draw_plane_hypotheses(XYZ, 1001, rng)
        t1 = time.perf_counter()
        plane.plane_fit(x, y, z, d)
        t2 = time.perf_counter()
        return (t2 - t0) * 1e6, (t1 - t0) * 1e6

    return _alternate(seeded, host, rounds=12)              # (the host draws alone take tens of milliseconds a round)


def trace_only():
    f, x0, P0, idx, z, n_draw = _one_point_setup()
    for s in range(10):
        f.set_x_p_k_km1(x0, P0)
        f.search_IC_matches()
        f.set_measurements(idx, z)
        f.step_predicted_seeded(SEED, s, n_draw, threshold=1.0, early_exit=False)
    f.sync()
    f.close()
    rng, p1, p2, match = _vo_setup()
    for s in range(10):
        vo.vo_ransac_seeded(p1, p2, match, SEED, s)
    x, y, zz, _ = pr.scene(1, 0.5)
    for s in range(10):
        plane.plane_fit_seeded(x, y, zz, SEED, s)


def profile(out_dir):
    tmp = os.path.join(out_dir, "_rocprof_seeded_draws")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "seeded_draws", "--", sys.executable, os.path.abspath(__file__), "--trace-only"]
    subprocess.run(cmd, check=True, timeout=600)
    csvs = sorted(glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True))
    assert csvs, "rocprofv3 wrote no kernel_stats.csv under %s" % tmp
    txt = open(csvs[-1]).read()
    print(txt, flush=True)
    with open(os.path.join(out_dir, "seeded_draws_kernel_stats.txt"), "w") as fh:
        fh.write("# rocprofv3 --kernel-trace --stats of tools/time_seeded_draws.py --trace-only: 10 x step_predicted_seeded (N = 500 fp32, 400 measurements, 200 draws),\n")
        fh.write("# 10 x vo_ransac_seeded (pnum = 60, rst = 700), 10 x plane_fit_seeded (default box, 1001 draws)\n")
        fh.write(txt)
    dev = {}
    for row in csv.DictReader(open(csvs[-1])):
        name = row.get("Name", "")
        for k in ("k_draw_1p", "k_draw_vo", "k_draw_plane"):
            if k in name:
                dev[k] = {"calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 2), "min_us": round(float(row["MinNs"]) / 1e3, 2),
                          "max_us": round(float(row["MaxNs"]) / 1e3, 2)}
    path = os.path.join(out_dir, "seeded_draws_timing.json")
    res = json.load(open(path)) if os.path.exists(path) else {"measured": True, "results": {}}
    res["draw_kernel_device_us"] = dev
    with open(path, "w") as fh:
        json.dump(res, fh, indent=1)


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
    res = {"measured": True, "box": props, "rounds": ROUNDS,
           "results": {"one_point_200_draws_N500_m400": one_point(), "vo_rst700_pnum60": vo_ransac(), "plane_1001_draws_default_box": plane_fit()}}
    path = os.path.join(args.out, "seeded_draws_timing.json")
    if os.path.exists(path):
        old = json.load(open(path))
        if "draw_kernel_device_us" in old:
            res["draw_kernel_device_us"] = old["draw_kernel_device_us"]
    print(json.dumps(res, indent=1))
    with open(path, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
