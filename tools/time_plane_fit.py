"""What the floor-plane fit costs (pre3_plane_fit / pre3_heading_from_scan):
  (a) device time per fit (pre3_plane_bench: HIP events around 50 warmed calls -- upload of the box from pinned memory + k_plane_score + k_plane_fit)
      with 1001 draws at the default box (4615 points) and at the full image (25 344 points);
  (b) wall time at N = 500 fp32 of heading_from_scan (nothing read back, then one sync) next to the separate sequence plane_fit -> host ->
      ekf_heading_update (no applied_out, then one sync), alternated in the same process from the same state, median and quartiles over the rounds;
  (c) the numpy restatement's time on the default box (tests/plane_fit_ref.py; a restatement -- MATLAB is not available -- for context only);
  (d) with --profile: rocprofv3 --kernel-trace --stats of the same calls, from a run of its own (this script with --trace-only as the child).
Writes <out>/plane_fit_timing.json and, with --profile, <out>/plane_fit_kernel_stats.txt.

    python tools/time_plane_fit.py [--out profiles] [--profile]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import plane_fit_ref as pr  # noqa: E402

pre3 = importlib.import_module("3pre_amd")
synth = importlib.import_module("3pre_amd.synth")
plane = importlib.import_module("3pre_amd.plane")
REPS, ROUNDS = 50, 40


def _scene():
    x, y, z, _ = pr.scene(1, 0.5)
    return x, y, z


def _filter(N=500):
    x0, P0, _ = synth.make_map(N)
    f = pre3.EkfFilter(synth.CAM, np.zeros(N, np.int32), dtype="f32", max_hyp=8)
    f.set_x_p_k_k(x0, P0)
    return f, x0, P0


def _pair(f, x0, P0, x, y, z, draws):
    """one round: both sequences from the same state, the fused one first on even rounds"""
    def fused():
        f.heading_from_scan(x, y, z, draws, strict_reference=False, wait=False)
        f.sync()

    def separate():
        g = plane.plane_fit(x, y, z, draws)
        if g["sta"] == 1:
            Rc = np.ascontiguousarray(g["R"].T.ravel(order="F"))
            pre3._lib.check(pre3._lib.lib.pre3_heading_update(f._ctx, pre3._lib.dptr(Rc), 0, None))
        f.sync()

    out = {}
    for name, call in (("fused", fused), ("separate", separate)):
        f.set_x_p_k_k(x0, P0)
        f.sync()
        t0 = time.perf_counter()
        call()
        out[name] = (time.perf_counter() - t0) * 1e6
    return out


def measure():
    x, y, z = _scene()
    res = {}
    for name, box, npts in (("default_box_4615", None, 65 * 71), ("full_image_25344", (1, 144, 1, 176), 144 * 176)):
        draws = pr.scene_draws(1, npts)
        res["plane_fit_device_us_" + name] = round(plane.plane_bench(x, y, z, draws, box=box, reps=REPS) * 1e3, 1)
    draws = pr.scene_draws(1, 65 * 71)
    r = pr.plane_fit(x, y, z, draws)
    f, x0, P0 = _filter()
    x0 = x0.copy()
    from test_heading_ref import R2q, axis_rot
    q = R2q(r["R"].T @ axis_rot([1.0, 0.0, 0.4], 1.5))
    x0[3:7] = q / np.linalg.norm(q)                           # the update applies: both sequences sweep P
    for _ in range(5):
        _pair(f, x0, P0, x, y, z, draws)
    ts = [_pair(f, x0, P0, x, y, z, draws) for _ in range(ROUNDS)]
    f.close()
    for k in ("fused", "separate"):
        v = np.array([t[k] for t in ts])
        res["heading_%s_wall_us" % k] = {"median": round(float(np.median(v)), 1), "q25": round(float(np.percentile(v, 25)), 1), "q75": round(float(np.percentile(v, 75)), 1)}
    d = np.array([t["separate"] - t["fused"] for t in ts])
    res["separate_minus_fused_us"] = {"median": round(float(np.median(d)), 1), "q25": round(float(np.percentile(d, 25)), 1), "q75": round(float(np.percentile(d, 75)), 1)}
    t0 = time.perf_counter()
    for _ in range(3):
        pr.plane_fit(x, y, z, draws)
    res["numpy_restatement_all_1001_draws_ms"] = round((time.perf_counter() - t0) / 3 * 1e3, 1)
    res["n_trials_of_the_scene"] = r["n_trials"]
    return res


def trace_only():
    x, y, z = _scene()
    draws = pr.scene_draws(1, 65 * 71)
    for _ in range(10):
        plane.plane_fit(x, y, z, draws)
    dfull = pr.scene_draws(1, 144 * 176)
    for _ in range(10):
        plane.plane_fit(x, y, z, dfull, box=(1, 144, 1, 176))
    f, x0, P0 = _filter()
    for _ in range(10):
        f.set_x_p_k_k(x0, P0)
        f.heading_from_scan(x, y, z, draws, strict_reference=False, wait=False)
    f.sync()
    f.close()


def profile(out_dir):
    tmp = os.path.join(out_dir, "_rocprof_plane_fit")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "plane_fit", "--", sys.executable, os.path.abspath(__file__), "--trace-only"]
    subprocess.run(cmd, check=True, timeout=600)
    csvs = sorted(glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True))
    assert csvs, "rocprofv3 wrote no kernel_stats.csv under %s" % tmp
    txt = open(csvs[-1]).read()
    print(txt, flush=True)
    with open(os.path.join(out_dir, "plane_fit_kernel_stats.txt"), "w") as fh:
        fh.write("# rocprofv3 --kernel-trace --stats of tools/time_plane_fit.py --trace-only: 10 x plane_fit at the default box (4615 points), 10 x at the full\n")
        fh.write("# image (25 344 points), 1001 draws each; 10 x heading_from_scan at N = 500 fp32 (pull + k_plane_score + k_plane_fit + k_rows_hp + k_rows_sweep)\n")
        fh.write(txt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--profile", action="store_true", help="(d) only: the rocprofv3 pass")
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
    res = {"measured": True, "box": props, "reps": REPS, "rounds": ROUNDS, "results": measure()}
    print(json.dumps(res, indent=1))
    with open(os.path.join(args.out, "plane_fit_timing.json"), "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
