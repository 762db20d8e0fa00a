"""Runs groups of tests/chol_ref.py's cases through the test hook EkfFilter.test_factor_solve (factorisation and solve alone on the caller's
S, B, nu) and judges them.  tests/test_gpu_chol_alone.py calls run_form() in its own process for the forms a context option selects, and starts
this file as a child process for the trailing sweeps, whose switches are read once per process:

    PRE3_TEST_HOOKS=1 PRE3_CHOL_TRAIL_SPLIT=1 PRE3_CHOL_TRAIL_P=4 PRE3_CHOL_TRAIL_T128=2 python tests/chol_worker.py trail
        -> one JSON line on stdout: [{case, bad, fig}, ...]
"""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import chol_ref as R  # noqa: E402
import k9_ref as K9  # noqa: E402

CAM = [250.0, 90, 70, 0, 0, 144, 176]
# form -> (dtype, the groups of chol_ref.group_cases it runs, PRE3_OPT_CHOL_PERSIST, PRE3_OPT_K9_BF16X3)
FORMS = {
    "k_cholp": ("f32", ("cholp", "cholp1"), True, True),
    "k_chol_step<float> with planes": ("f32", ("step",), False, True),
    "k_chol_step<float>": ("f32", ("step",), False, False),
    "k_chol_step<double>": ("f64", ("step",), False, False),
    "trailing sweeps": ("f32", ("trail",), False, True),
}


def gates():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "chol_tolerance.json")))["cases"]


def prior(n, dtype):
    """a covariance for mode 0 to leave alone: symmetric, every entry non-zero, values of the dtype"""
    rng = np.random.default_rng([11, 3, n])
    a = rng.standard_normal((n, n))
    return (K9._sym(a) + n * np.eye(n)).astype(R.DT[dtype]).astype(np.float64)


def mode1_prior(n, r, kappa):
    """P0 by k9_ref.accuracy_case's recipe, P0 = 1.5 W'W + 1 % noise, around the W that `plain` solves for: P0 - W'W is comparable with W'W in every entry"""
    S, B, nu = R.accuracy_case(n, r, kappa, "f32")
    W = R.plain(S, B, nu, "f32")[1][:, :n]
    rng = np.random.default_rng([11, 4, n, r, kappa])
    G = W.T @ W
    g = np.diag(G).copy()
    g[g == 0] = g[g > 0].min()
    D = 0.01 * np.sqrt(np.outer(g, g)) * K9._sym(rng.standard_normal((n, n)))
    return K9._sym(1.5 * G + D).astype(np.float32).astype(np.float64)


def open_context(pre3, N, cap, form):
    dtype, _, persist, b3 = FORMS[form]
    f = pre3.EkfFilter(CAM, np.zeros(N, np.int32), dtype=dtype, max_hyp=4, max_landmarks=cap)
    assert f.n == R.state_size(N)
    if dtype == "f32":
        assert f.k9_bf16x3(b3) == b3
        assert f.chol_persist(persist) == (persist and b3)
    return f


def run_form(pre3, form, shapes=None, num_cus=256):
    """every case of a form [on the (N, cap) in `shapes`], one context at a time, mode 0: [dict(case=..., bad=[...], fig={...})]"""
    dtype, groups, persist, _ = FORMS[form]
    g, out, f, at, P0 = gates(), [], None, None, None
    for group in groups:
        for c in R.group_cases(group, dtype):
            if shapes is not None and (c["N"], c["cap"]) not in shapes:
                continue
            if at != (c["N"], c["cap"]):
                if f is not None:
                    f.close()
                at = (c["N"], c["cap"])
                f = open_context(pre3, c["N"], c["cap"], form)
                P0 = prior(f.n, dtype)
                f.set_x_p_k_k(K9.x0_of(c["N"]), P0)
            nrb = R.round_up(c["r"], 64) // 64
            if form == "k_cholp":
                assert R.cholp_takes(nrb, c["cap"], num_cus, group == "cholp1"), (c, "the sizes do not select k_cholp")
            elif nrb > 16 and dtype == "f32":
                f.chol_persist(True)                                  # 17 and 18 panels: the launch-per-panel form even with the option on
                assert not R.cholp_takes(nrb, c["cap"], num_cus)
            S, B, nu = R.inputs(c)
            L, W = f.test_factor_solve(S, B, nu, mode=0, predicted_prior=group == "cholp1")
            if form != "k_cholp" and nrb > 16 and dtype == "f32":
                f.chol_persist(persist)
            bad, fig = R.judge(c, L, W, g)
            if not np.array_equal(f.get_p_k_k(), P0):
                bad.append("mode 0 changed P")
            out.append(dict(case=c, bad=bad, fig=fig))
    if f is not None:
        f.close()
    return out


def describe(res):
    c, fig = res["case"], res["fig"]
    what = "exact" if c["cls"] == "exact" else "acc k=%d: E1 %.2f / %.2f  E2 %.2f / %.2f u" % ((c["kappa"],) + tuple(fig.get(k, np.nan) for k in R.FIGS))
    return "%s N=%d cap=%d r=%d  %s%s" % (c["dtype"], c["N"], c["cap"], c["r"], what, "  FAILED: " + "; ".join(res["bad"]) if res["bad"] else "")


if __name__ == "__main__":
    pre3 = importlib.import_module("3pre_amd")
    form = {"trail": "trailing sweeps"}[sys.argv[1]]
    print("CHOLJSON " + json.dumps(run_form(pre3, form, num_cus=int(sys.argv[2]))))
