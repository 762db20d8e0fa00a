#!/usr/bin/env python
"""Time EkfFilter.relocalise_seeded against the chain joined by hand from the calls it fuses, in one session.

The chain: landmarks(), siftmatch on get_descriptors() and the scan, a gather of the finite matches, vo.pnp_ransac_seeded, set_process_noise(Pn) when
the pose is taken, ekf_prediction(u), the noise setting restored -- four host waits, and the map, the bank and the correspondences over PCIe and back.
Two sizes: tests/reloc_cases.py's fixture scene (N = 185, K2 = 245, n_hyp = 200) and a map of 3pre_amd/synth.py with N = 2000 against a scan of its
visible landmarks plus 200 distractors (K2 is recorded in the result; 2022 at the default seed), n_hyp = 700.  The chain forms its increment from the
pose the scene was built with (x[0:7], known to the caller): it reads no state back, as the call does not.  For each, two host clocks: "host free" -- until the last call has returned (the call: wait=False) -- and "stream drained" -- until a
sync() behind it has returned.  The filter's state is put back between repetitions outside the clock.  No target is set: nothing in an earlier version
does this work, and the timing is not a pass condition.

    python tools/time_relocalise.py [--reps 20] [--warmup 3] [--big 2000] [--out profiles/relocalise_timing.json]
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
import reloc_cases as rc  # noqa: E402

PN = np.diag([0.05 ** 2] * 3 + [0.02 ** 2] * 4)


def quartiles(ts):
    q1, med, q3 = np.percentile(np.asarray(ts) * 1e3, [25, 50, 75])
    return dict(median_ms=round(float(med), 4), q1_ms=round(float(q1), 4), q3_ms=round(float(q3), 4), n=len(ts))


def big_scene(N, K2_extra=200, seed=5):
    """a map of N inverse-depth landmarks seen from a pose 0.1 m / 0.1 rad away: the visible landmarks' descriptors in the scan, a quarter of the pixels
    replaced, K2_extra distractors"""
    synth = importlib.import_module("3pre_amd.synth")
    g = np.random.default_rng(seed)
    x0, P0, _ = synth.make_map(N, seed=seed)
    pose = rc.moved_pose(x0[:7], g, 0.1, 0.1)
    uv, vis = synth.pixels(pose, x0[13:].reshape(N, 6), synth.CAM)
    seen = np.nonzero(vis)[0]
    bank = rc.descriptors(g, N)
    sd, sp, _, _ = rc.build_scan(g, synth.CAM, bank, seen, uv[seen], K2_extra, 0.25)
    return dict(name="synth_%d" % N, types=np.zeros(N, np.int32), x=x0, P=P0, bank=bank, scan_desc=sd, scan_pos=sp, cam=synth.CAM, seed=3, seq=1, n_hyp=700,
                thr_px=2.0, min_support=12)


def chain(pre3, vo, f, sc, kw):
    xyz = f.landmarks()["xyz"]
    m = pre3.siftmatch(f.get_descriptors(), sc["scan_desc"].T, kw["thresh"]).astype(np.int64) - 1
    pairs = m.T.reshape(-1, 2)
    kept = pairs[np.isfinite(xyz[pairs[:, 0]]).all(axis=1)]
    r = vo.pnp_ransac_seeded(xyz[kept[:, 0]], sc["scan_pos"][kept[:, 1], :2], sc["cam"], kw["n_hyp"], kw["thr_px"], kw["seed"], kw["seq"], undistort=kw["undistort"])
    taken = r["sta"] == 1 and r["n_support"] >= kw["min_support"]
    u = np.array([0.0, 0, 0, 1, 0, 0, 0])
    if taken:
        import reloc_ref as rr
        u = rr.select(sc["x"][:7], r["sta"], r["n_support"], kw["min_support"], r["u"])[0]
        f.set_process_noise(kw["Pn"])
    f.ekf_prediction(u)
    f.set_process_noise(None)
    return int(taken), len(kept)


def measure(pre3, vo, sc, dtype, warmup, reps):
    f = pre3.EkfFilter(sc["cam"], sc["types"], dtype=dtype, max_hyp=16)
    f.set_descriptors(sc["bank"].T)
    f.load_scan(sc["scan_desc"].T, sc["scan_pos"].T)
    kw = dict(seed=sc["seed"], seq=sc["seq"], thresh=1.5, n_hyp=sc["n_hyp"], thr_px=sc["thr_px"], undistort=True, min_support=sc["min_support"], Pn=PN)
    out = dict(N=int(len(sc["types"])), K2=int(len(sc["scan_desc"])), n_hyp=int(sc["n_hyp"]), dtype=dtype)
    ts = {k: [] for k in ("call_host_free", "call_drained", "chain_host_free", "chain_drained")}
    for i in range(warmup + reps):
        for which in ("call", "chain"):                      # alternated: both see the same machine
            f.set_x_p_k_k(sc["x"], sc["P"])
            f.sync()
            t0 = time.perf_counter()
            if which == "call":
                f.relocalise_seeded(wait=False, **kw)
            else:
                out["taken"], out["n_corr"] = chain(pre3, vo, f, sc, kw)
            t1 = time.perf_counter()
            f.sync()
            t2 = time.perf_counter()
            if i >= warmup:
                ts[which + "_host_free"].append(t1 - t0)
                ts[which + "_drained"].append(t2 - t0)
    f.set_x_p_k_k(sc["x"], sc["P"])
    res = f.relocalise_seeded(**kw)
    assert (res["taken"], res["n_corr"]) == (out["taken"], out["n_corr"]), "the call and the chain disagree"
    out.update(support=res["pnp"]["n_support"], n_matches=res["n_matches"], **{k: quartiles(v) for k, v in ts.items()})
    f.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--big", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relocalise_timing.json"))
    a = ap.parse_args()
    pre3 = importlib.import_module("3pre_amd")
    vo = importlib.import_module("3pre_amd.vo")
    assert pre3.device_count() >= 1, "needs a HIP device"
    res = dict(reps=a.reps, warmup=a.warmup, clock="host perf_counter; drained = a sync() behind the last call", rows=[])
    for sc, dtype, reps in ((rc.scene("fixture_1"), "f32", a.reps), (rc.scene("fixture_1"), "f64", a.reps), (big_scene(a.big), "f32", max(a.reps // 2, 1))):
        row = measure(pre3, vo, sc, dtype, a.warmup, reps)
        row["scene"] = sc["name"]
        print(json.dumps(row))
        res["rows"].append(row)
    with open(a.out, "w") as fo:
        json.dump(res, fo, indent=1)
        fo.write("\n")


if __name__ == "__main__":
    main()
