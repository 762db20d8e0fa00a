#!/usr/bin/env python
"""Time the Gauss-Newton refinement of DESIGN.md section 37 as what it adds to the calls it rides behind, in one session.

Two pairs, alternated in one process so that both see the same machine:
  vo.pnp_ransac_refined_seeded  against  vo.pnp_ransac_seeded       (stateless: uploads, the launches, one copy back; a host clock round the call)
  EkfFilter.relocalise_refined_seeded  against  relocalise_seeded   (wait=False; "host free" until the call returns, "drained" until a sync() behind it)
on tests/reloc_cases.py's fixture scene 1 (N = 185; its correspondences for the stateless pair) and the N = 2000 map of tools/time_relocalise.py.  The
difference of two medians is the added launch (and, in the refined relocalisation, the 49-lane noise stage inside the prediction's launch); each row
carries its quartiles, so the spread can be set against that difference.  No target is set and the timing is not a pass condition: nothing in an
earlier version does this work.

    python tools/time_pnp_refine.py [--reps 30] [--warmup 3] [--big 2000] [--n-iter 5] [--out profiles/pnp_refine_timing.json]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import reloc_cases as rc  # noqa: E402
from time_relocalise import PN, big_scene, quartiles  # noqa: E402


def correspondences(pre3, f, sc):
    """the chain's own gather: what the relocaliser hands its RANSAC"""
    xyz = f.landmarks()["xyz"]
    m = pre3.siftmatch(f.get_descriptors(), sc["scan_desc"].T, 1.5).astype(np.int64) - 1
    pairs = m.T.reshape(-1, 2)
    kept = pairs[np.isfinite(xyz[pairs[:, 0]]).all(axis=1)]
    return np.ascontiguousarray(xyz[kept[:, 0]]), np.ascontiguousarray(sc["scan_pos"][kept[:, 1], :2])


def measure(pre3, vo, sc, dtype, warmup, reps, n_iter):
    f = pre3.EkfFilter(sc["cam"], sc["types"], dtype=dtype, max_hyp=16)
    f.set_descriptors(sc["bank"].T)
    f.load_scan(sc["scan_desc"].T, sc["scan_pos"].T)
    f.set_x_p_k_k(sc["x"], sc["P"])
    Xw, U = correspondences(pre3, f, sc)
    kw = dict(seed=sc["seed"], seq=sc["seq"], thresh=1.5, n_hyp=sc["n_hyp"], thr_px=sc["thr_px"], undistort=True, min_support=sc["min_support"], Pn=PN)
    rkw = dict(kw, n_iter=n_iter, sigma_px=0.0, noise="pose_floor")
    pargs = (Xw, U, sc["cam"], sc["n_hyp"], sc["thr_px"], sc["seed"], sc["seq"])
    out = dict(N=int(len(sc["types"])), K2=int(len(sc["scan_desc"])), n_corr=int(len(Xw)), n_hyp=int(sc["n_hyp"]), dtype=dtype, n_iter=n_iter)
    names = ("ransac", "ransac_refined", "reloc_host_free", "reloc_drained", "reloc_refined_host_free", "reloc_refined_drained")
    ts = {k: [] for k in names}
    for i in range(warmup + reps):
        for which in ("ransac", "ransac_refined"):
            f.sync()
            t0 = time.perf_counter()
            if which == "ransac":
                vo.pnp_ransac_seeded(*pargs, undistort=True)
            else:
                vo.pnp_ransac_refined_seeded(*pargs, undistort=True, n_iter=n_iter)
            t1 = time.perf_counter()                      # (the call ends in its copy back: the stream is drained)
            if i >= warmup:
                ts[which].append(t1 - t0)
        for which in ("reloc", "reloc_refined"):
            f.set_x_p_k_k(sc["x"], sc["P"])
            f.sync()
            t0 = time.perf_counter()
            if which == "reloc":
                f.relocalise_seeded(wait=False, **kw)
            else:
                f.relocalise_refined_seeded(wait=False, **rkw)
            t1 = time.perf_counter()
            f.sync()
            t2 = time.perf_counter()
            if i >= warmup:
                ts[which + "_host_free"].append(t1 - t0)
                ts[which + "_drained"].append(t2 - t0)
    f.set_x_p_k_k(sc["x"], sc["P"])
    res = f.relocalise_refined_seeded(**rkw)
    out.update(support=res["pnp"]["n_support"], taken=res["taken"], ref_sta=res["ref"]["sta"], noise_taken=res["noise_taken"],
               cost=[float(v) for v in res["ref"]["cost"][:n_iter + 1]], **{k: quartiles(v) for k, v in ts.items()})
    out["added_ms"] = dict(ransac=round(out["ransac_refined"]["median_ms"] - out["ransac"]["median_ms"], 4),
                           reloc_drained=round(out["reloc_refined_drained"]["median_ms"] - out["reloc_drained"]["median_ms"], 4))
    f.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--big", type=int, default=2000)
    ap.add_argument("--n-iter", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pnp_refine_timing.json"))
    a = ap.parse_args()
    pre3 = importlib.import_module("3pre_amd")
    vo = importlib.import_module("3pre_amd.vo")
    assert pre3.device_count() >= 1, "needs a HIP device"
    res = dict(reps=a.reps, warmup=a.warmup, clock="host perf_counter; drained = a sync() behind the last call; the stateless pair ends in its own copy back", rows=[])
    for sc, dtype in ((rc.scene("fixture_1"), "f32"), (big_scene(a.big), "f32")):
        row = measure(pre3, vo, sc, dtype, a.warmup, a.reps, a.n_iter)
        row["scene"] = sc["name"]
        print(json.dumps(row))
        res["rows"].append(row)
    with open(a.out, "w") as fo:
        json.dump(res, fo, indent=1)
        fo.write("\n")


if __name__ == "__main__":
    main()
