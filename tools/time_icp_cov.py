#!/usr/bin/env python
"""Time the ICP's closed-form covariance and the prediction fed from the ICP-refined pair.

Part 1, the two launches alone: tests/icp_frame_cases.py's 144 x 176 pair at the strides of tools/time_icp.py (1, 2, 4).  vo.icp_frames gives the final
pairs and u; the two clouds are gathered through corr_pix and vo.icp_cov_bench runs k_icp_cov_part + k_icp_cov_fin back to back between two events.
Next to it the host wall time of the stateless vo.icp_cov call (upload, two launches, one wait).

Part 2, the prediction call against the waiting chain, in the same session: tests/icp_pair_cases.py's planted pair at 144 x 176.  The chain is
vo.icp_pair_cov_seeded (one wait) -> the rule on the host -> set_process_noise -> ekf_prediction(u) -> the setting restored; the call is
EkfFilter.ekf_prediction_icp_pair_seeded, not waiting.  Both are timed to the point where the host is free again, and again with the context's stream
drained behind them (EkfFilter.sync), noise mode 3 over a caller-set noise.  No target is set; nothing in an earlier version does this work.

    python tools/time_icp_cov.py [--reps 20] [--warmup 3] [--out profiles/icp_cov_timing.json]
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
import icp_cov_ref as ref  # noqa: E402
import icp_frame_cases as F  # noqa: E402
from icp_pair_cases import planted_pair  # noqa: E402

SEED, SEQ = 5, 0


def quartiles(ts):
    q1, med, q3 = np.percentile(np.asarray(ts) * 1e3, [25, 50, 75])
    return dict(median_ms=round(float(med), 4), q1_ms=round(float(q1), 4), q3_ms=round(float(q3), 4), n=len(ts))


def timed(fn, warmup, reps, before=None):
    ts = []
    for i in range(warmup + reps):
        if before:
            before()
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            ts.append(time.perf_counter() - t0)
    return quartiles(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_cov_timing.json"))
    a = ap.parse_args()
    pre3 = importlib.import_module("3pre_amd")
    srm, vo, synth = pre3.sr4000, importlib.import_module("3pre_amd.vo"), importlib.import_module("3pre_amd.synth")
    assert pre3.device_count() >= 1, "needs a HIP device"
    res = dict(rows=F.ROWS, cols=F.COLS, reps=a.reps, warmup=a.warmup, limits=vo.icp_cov_limits(), strides={})
    sc = F.make_frames()
    with srm.SrFrame(F.ROWS, F.COLS) as f1, srm.SrFrame(F.ROWS, F.COLS) as f2:
        f1.load(sc["fr1"], F.MODE); f2.load(sc["fr2"], F.MODE)
        x1, y1, z1, _ = f1.planes(); x2, y2, z2, _ = f2.planes()
        for stride in (1, 2, 4):
            out = vo.icp_frames(f1, f2, F.RES, sc["Rinit"], sc["Tinit"], stride=stride)
            m, s = out["corr_pix"][:, 0], out["corr_pix"][:, 1]
            d1 = np.stack([-x1.ravel(order="F")[m], -y1.ravel(order="F")[m], z1.ravel(order="F")[m]])
            d2 = np.stack([-x2.ravel(order="F")[s], -y2.ravel(order="F")[s], z2.ravel(order="F")[s]])
            k = np.arange(1, out["p"] + 1)
            corr = np.stack([k, k], axis=1)
            c = vo.icp_cov(d1, d2, corr, out["u"])
            row = dict(p=out["p"], sta=out["sta"], status=c["status"], partials=-(-out["p"] // 256),
                       sigma_T_mm=[round(float(v), 4) for v in 1000 * np.sqrt(np.diag(c["cov"])[:3])] if c["status"] == 1 else None,
                       two_launches_ms=round(vo.icp_cov_bench(d1, d2, corr, out["u"], reps=200), 5),
                       stateless_call=timed(lambda: vo.icp_cov(d1, d2, corr, out["u"]), a.warmup, a.reps))
            res["strides"][str(stride)] = row
            print("stride", stride, json.dumps(row), flush=True)

    c = planted_pair(F.ROWS, F.COLS, K=120)
    N = 41
    x0, P0, _ = synth.make_map(N, None)
    Pn = np.diag([1e-5] * 3 + [1e-6] * 4)
    pred = {}
    with srm.SrFrame(F.ROWS, F.COLS) as f1, srm.SrFrame(F.ROWS, F.COLS) as f2:
        f1.load(c["fr1"], 1); f2.load(c["fr2"], 1)
        f1.keypoints(c["frm1"], c["des1"], 1); f2.keypoints(c["frm2"], c["des2"], 1)
        for dtype in ("f32", "f64"):
            for stride in (1, 2, 4):
                kw = dict(stride=stride, res=F.RES)
                f = pre3.EkfFilter(synth.CAM, np.zeros(N, np.int32), dtype=dtype, max_hyp=8)
                f.set_process_noise(Pn)
                taken = []

                def reset():
                    f.set_x_p_k_k(x0, P0); f.sync()

                def chain(drain):
                    pair, icp = vo.icp_pair_cov_seeded(f1, f2, SEED, SEQ, **kw)
                    finite = icp["sta"] != 0 and bool(np.isfinite(icp["u"]).all())
                    ut, nt, _ = ref.select(pair["sta"], pair["pnum"], 0, 1, icp["sta"], finite, icp.get("error", 0.0), np.inf, 3, pair["cov_status"], icp["cov_status"])
                    if nt:
                        f.set_process_noise(ref.taken_pn(nt, Pn, pair["cov"], icp["cov"]))
                    f.ekf_prediction([0, 0, 0, 1, 0, 0, 0] if ut == 0 else pair["u"] if ut == 1 else icp["u"])
                    f.set_process_noise(Pn)
                    taken.append((ut, nt))
                    if drain:
                        f.sync()

                def call(drain):
                    f.ekf_prediction_icp_pair_seeded(f1, f2, SEED, SEQ, noise=3, wait=False, **kw)
                    if drain:
                        f.sync()

                row = dict(chain_host_free=timed(lambda: chain(False), a.warmup, a.reps, reset), call_host_free=timed(lambda: call(False), a.warmup, a.reps, reset),
                           chain_drained=timed(lambda: chain(True), a.warmup, a.reps, reset), call_drained=timed(lambda: call(True), a.warmup, a.reps, reset))
                reset()
                got = f.ekf_prediction_icp_pair_seeded(f1, f2, SEED, SEQ, noise=3, **kw)
                row.update(taken=list(got["taken"]), chain_taken=list(taken[-1]), pnum=got["pnum"], icp_p=got["icp"].get("p"), icp_sta=got["icp"]["sta"])
                pred["%s_stride%d" % (dtype, stride)] = row
                print(dtype, "stride", stride, json.dumps(row), flush=True)
                f.close()
    res["prediction"] = dict(n_landmarks=N, noise=3, pair="icp_pair_cases.planted_pair(144, 176, K=120)", cases=pred)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
