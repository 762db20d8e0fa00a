"""Runs one group of tests/k9_ref.py's cases through the test hook EkfFilter.test_downdate (K9 alone on the caller's W) and judges them.
tests/test_gpu_k9_alone.py calls run_group() in its own process for the forms the library picks by itself, and starts this file as a child
process for the two forms PRE3_K9_FORM forces (the switch is read once per process):

    PRE3_TEST_HOOKS=1 PRE3_K9_FORM=2 python tests/k9_worker.py persist        -> one JSON line on stdout: [{case, bad, fig}, ...]
"""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import k9_ref as R  # noqa: E402

CAM = [250.0, 90, 70, 0, 0, 144, 176]
MFMA_F32 = ("f32_1t", "persist", "forced_1t")            # groups whose f32 contexts run the f32-MFMA forms (PRE3_OPT_K9_BF16X3 off)


def gates():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "k9_tolerance.json")))["cases"]


def run_group(pre3, group, dtype, shapes=None):
    """every case of (group, dtype) [on the (N, cap) in `shapes`], one context per (N, cap): [dict(case=..., bad=[...], fig={...})]"""
    g, out, f, at = gates(), [], None, None
    for c in R.group_cases(group, dtype):
        if shapes is not None and (c["N"], c["cap"]) not in shapes:
            continue
        if at != (c["N"], c["cap"]):
            if f is not None:
                f.close()
            at = (c["N"], c["cap"])
            f = pre3.EkfFilter(CAM, np.zeros(c["N"], np.int32), dtype=dtype, max_hyp=4, max_landmarks=c["cap"])
            assert f.n == c["n"]
            if dtype == "f32":
                assert f.k9_bf16x3(False if group in MFMA_F32 else None) == (group not in MFMA_F32)
        P0, W = R.inputs(c)
        f.set_x_p_k_k(R.x0_of(c["N"]), P0)
        f.test_downdate(W, c["launches"])
        bad, fig = R.judge(c, f.get_p_k_k(), g)
        out.append(dict(case=c, bad=bad, fig=fig))
    if f is not None:
        f.close()
    return out


def describe(res):
    c, fig = res["case"], res["fig"]
    what = "exact/%d" % c["planes"] if c["cls"] == "exact" else "acc: max %.3f rms %.3f u (plain %.3f / %.3f)" % (fig.get("max", np.nan), fig.get("rms", np.nan),
                                                                                                             fig.get("plain_max", np.nan), fig.get("plain_rms", np.nan))
    return "%s N=%d cap=%d r=%d launches=%d  %s%s" % (c["dtype"], c["N"], c["cap"], c["r"], c["launches"], what, "  FAILED: " + "; ".join(res["bad"]) if res["bad"] else "")


if __name__ == "__main__":
    pre3 = importlib.import_module("3pre_amd")
    res = []
    for dt in ("f32", "f64"):
        res += run_group(pre3, sys.argv[1], dt)
    print("K9JSON " + json.dumps(res))
