"""What the consumers of a resident SR4000 frame save: wall time of the host-fed sequence -- the parent's only way to do the
same work -- next to the frame form, alternated in the same process from the same state, median and quartiles over the rounds:
  (a) SrFrame.planes() -> heading_from_scan_seeded   against  heading_from_frame_seeded      (default box, N = 500 fp32, one sync at the end)
  (b) SrFrame.planes() -> plane_fit_seeded           against  plane_fit_frame_seeded         (default box, 1001 draws)
  (c) load_scan (pre3_set_scan) of the host arrays   against  set_scan_frame(which = 0)      (K2 = 600; one sync at the end)
Writes <out>/frame_consumers_timing.json.

    python tools/time_frame_consumers.py [--out profiles]
"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import plane_fit_ref as pr  # noqa: E402
import sr_frame_ref as sr  # noqa: E402

pre3 = importlib.import_module("3pre_amd")
synth = importlib.import_module("3pre_amd.synth")
plane = importlib.import_module("3pre_amd.plane")
srm = importlib.import_module("3pre_amd.sr4000")
ROUNDS, WARM = 40, 5
SEED, K2 = 20261018, 600


def _frame():
    x, y, z, _ = pr.scene(1, 0.1)
    fr = sr.make_frame(144, 176, seed=1)
    fr["x"], fr["y"], fr["z"] = (np.asfortranarray(a) for a in (x, y, z))
    return fr


def _stats(v):
    v = np.asarray(v)
    return {"median": round(float(np.median(v)), 1), "q25": round(float(np.percentile(v, 25)), 1), "q75": round(float(np.percentile(v, 75)), 1)}


def _alternate(calls, before):
    """calls: {name: callable}; every round runs each once, the order flipped on odd rounds; before() restores the state and drains the queues"""
    names = list(calls)
    ts = {k: [] for k in names}
    for r in range(-WARM, ROUNDS):
        for k in (names if r % 2 == 0 else names[::-1]):
            before()
            t0 = time.perf_counter()
            calls[k]()
            dt = (time.perf_counter() - t0) * 1e6
            if r >= 0:
                ts[k].append(dt)
    out = {k + "_wall_us": _stats(ts[k]) for k in names}
    out["%s_minus_%s_us" % (names[0], names[1])] = _stats(np.array(ts[names[0]]) - np.array(ts[names[1]]))
    return out


def measure():
    res = {}
    fh = srm.SrFrame().load(_frame(), 0)
    x, y, z, _ = fh.planes()
    fit = plane.plane_fit_seeded(x, y, z, SEED, 0)
    # (a) the heading update at N = 500 fp32, the quaternion 1.5 degrees from the fit so that both sequences sweep P
    from test_heading_ref import R2q, axis_rot
    x0, P0, _ = synth.make_map(500)
    f = pre3.EkfFilter(synth.CAM, np.zeros(500, np.int32), dtype="f32", max_hyp=8)
    q = R2q(fit["R"].T @ axis_rot([1.0, 0.0, 0.4], 1.5))
    x0 = x0.copy()
    x0[3:7] = q / np.linalg.norm(q)

    def reset():
        f.set_x_p_k_k(x0, P0)
        f.sync()

    def host_fed():
        xs, ys, zs, _ = fh.planes()
        f.heading_from_scan_seeded(xs, ys, zs, SEED, 0, strict_reference=False, wait=False)
        f.sync()

    def from_frame():
        f.heading_from_frame_seeded(fh, SEED, 0, strict_reference=False, wait=False)
        f.sync()

    res["a_heading_N500_f32"] = _alternate({"host_fed": host_fed, "frame": from_frame}, reset)
    # (b) the stateless fit
    res["b_plane_fit"] = _alternate({"host_fed": lambda: plane.plane_fit_seeded(*fh.planes()[:3], SEED, 0), "frame": lambda: plane.plane_fit_frame_seeded(fh, SEED, 0)},
                                    lambda: None)
    res["fit_of_the_scene"] = {k: fit[k] for k in ("sta", "n_trials", "n_inliers")}
    # (c) the scan
    frm, des = sr.make_keypoints(K2, seed=2)
    fh.keypoints(frm, des, srm.GATE_DEPTH)
    pos = np.zeros((4, K2))
    pos[:min(4, frm.shape[0])] = frm[:4]
    f.set_x_p_k_km1(x0, P0)
    res["c_set_scan_K2_600"] = _alternate({"host_fed": lambda: (f.load_scan(des, pos), f.sync()), "frame": lambda: (f.set_scan_frame(fh, 0), f.sync())}, f.sync)
    f.close()
    fh.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    props = {}
    try:
        import torch
        props = {"device": torch.cuda.get_device_name(0)}
    except Exception:                                        # pragma: no cover
        pass
    res = {"measured": True, "box": props, "rounds": ROUNDS, "warm_up_rounds": WARM, "results": measure()}
    print(json.dumps(res, indent=1))
    with open(os.path.join(args.out, "frame_consumers_timing.json"), "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
