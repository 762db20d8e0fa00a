#!/usr/bin/env python
"""Time EPnP and its RANSAC on the device.

The stateless vo.efficient_pnp call -- upload, one launch of k_pnp_solve, one wait: host wall time -- at n = 50 (the solver's own input file), 400
and 25 344 (every pixel of a 144 x 176 frame), next to tests/epnp_ref.py (numpy over LAPACK) on the same host for scale.  The RANSAC's four
launches (k_pnp_draw, k_pnp_hyp, k_pnp_select, k_pnp_solve over the winner's list) on resident operands between two device events, warmed
(vo.pnp_bench), at n = 400, n_hyp = 700, with and without the undistortion; next to it the waiting call.  The pair form (vo.vo_pair_pnp_seeded) against
vo.vo_pair_seeded alone on tests/pnp_frame_cases.py's pair, the two alternated in one process, host wall time of the waiting calls.  No target is set: nothing in an earlier
version does this work.

    python tools/time_pnp.py [--reps 20] [--warmup 3] [--out profiles/pnp_timing.json]
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
import epnp_ref as ref  # noqa: E402
import pnp_cases as pc  # noqa: E402


def quartiles(ts):
    q1, med, q3 = np.percentile(np.asarray(ts) * 1e3, [25, 50, 75])
    return dict(median_ms=round(float(med), 4), q1_ms=round(float(q1), 4), q3_ms=round(float(q3), 4), n=len(ts))


def timed(fn, warmup, reps):
    ts = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            ts.append(time.perf_counter() - t0)
    return quartiles(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pnp_timing.json"))
    a = ap.parse_args()
    pre3 = importlib.import_module("3pre_amd")
    vo = importlib.import_module("3pre_amd.vo")
    assert pre3.device_count() >= 1, "needs a HIP device"
    cam = pc.fixture_cam()
    res = dict(reps=a.reps, warmup=a.warmup, limits=vo.pnp_limits(), epnp={}, ransac={})
    d, _ = pc.fixture()
    sets = {"50": (d["Xworld"], d["Ximg_pix"])}
    for n in (400, 144 * 176):
        Xw, U, _, _, _ = pc.sr_scene(n, 7)
        sets[str(n)] = (Xw, U)
    for name, (Xw, U) in sets.items():
        row = dict(stateless_call=timed(lambda: vo.efficient_pnp(Xw, U, cam), a.warmup, a.reps),
                   stateless_call_undistort=timed(lambda: vo.efficient_pnp(Xw, U, pc.SR_CAM, undistort=True), a.warmup, a.reps),
                   numpy_restatement=timed(lambda: ref.epnp(Xw, U, cam), 1, 5))
        res["epnp"][name] = row
        print("epnp n", name, json.dumps(row), flush=True)
    Xw, U, _, _, _ = pc.sr_scene(400, 8)
    g = np.random.default_rng(9)
    U = U.copy()
    U[:100] = np.column_stack([g.uniform(0, cam[6], 100), g.uniform(0, cam[5], 100)])
    Xs, Us, _, _, _ = pc.sr_scene(400, 8, pc.SR_CAM, fov=(0.3, 0.25))
    Us[:100] = np.column_stack([g.uniform(0, 176, 100), g.uniform(0, 144, 100)])
    Us = ref.distort(pc.SR_CAM, Us)
    for und in (False, True):
        c = pc.SR_CAM if und else cam
        if und:
            Xw, U = Xs, Us
        got = vo.pnp_ransac_seeded(Xw, U, c, 700, pc.THR_PX, seed=3, undistort=und)
        row = dict(n=400, n_hyp=700, support=got["n_support"], sta=got["sta"],
                   four_launches_ms=round(vo.pnp_bench(Xw, U, c, 700, pc.THR_PX, seed=3, undistort=und, reps=50), 5),
                   waiting_call=timed(lambda: vo.pnp_ransac_seeded(Xw, U, c, 700, pc.THR_PX, seed=3, undistort=und), a.warmup, a.reps))
        res["ransac"]["undistort" if und else "plain"] = row
        print("ransac undistort", und, json.dumps(row), flush=True)
    # the pair form against pre3_vo_pair_seeded alone on tests/pnp_frame_cases.py's pair, the two alternated in one process; host wall time of the
    # waiting calls (each ends in its one wait, so the difference is the two launches behind the pair's and the larger transfer)
    import pnp_frame_cases as F
    srm = pre3.sr4000
    c = F.pinhole_pair()
    with srm.SrFrame(F.ROWS, F.COLS) as f1, srm.SrFrame(F.ROWS, F.COLS) as f2:
        f1.load(c["fr1"], 1); f2.load(c["fr2"], 1)
        f1.keypoints(c["frm1"], c["des1"], 1); f2.keypoints(c["frm2"], c["des2"], 1)
        ts = {"vo_pair_seeded": [], "vo_pair_pnp_seeded": []}
        for i in range(a.warmup + a.reps):
            for name, fn in (("vo_pair_seeded", lambda: vo.vo_pair_seeded(f1, f2, 5, 0)), ("vo_pair_pnp_seeded", lambda: vo.vo_pair_pnp_seeded(f1, f2, 5, cam, 0))):
                t0 = time.perf_counter()
                got = fn()
                if i >= a.warmup:
                    ts[name].append(time.perf_counter() - t0)
        res["pair"] = dict(case="pnp_frame_cases.pinhole_pair()", pnum=got["pnum"], support=got["n_support"], pnp_sta=got["pnp"]["sta"],
                           **{k: quartiles(v) for k, v in ts.items()})
        print("pair", json.dumps(res["pair"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
