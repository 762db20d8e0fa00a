"""tests/golden/pnp_refine_tolerance.json: what separates 3pre_amd/csrc/pre3_pnpref.h (and reloc_noise_from_pose of pre3_reloc.h) run on the host
(tests/pnp_refine_host_main.cpp) from tests/pnp_refine_ref.py, both started from the restatement's EPnP pose, on the committed cases: tests/pnp_cases.py's
sr_scene(n, 100 + n) at n = 6, 7, 63, 64, 65, 255, 256, 257, 513 and the winners' inlier sets of tests/reloc_cases.py's scenes, n_iter = 5.

    python tests/golden/make_pnp_refine_tolerance.py

Floors: the largest absolute difference in R and T (pose) and in u; cost as |difference| / max(1 px^2, value); cov6, cov7 and Pn entry by entry as
|difference| / sqrt(C_ii C_jj) (cov7's and Pn's quaternion block has a zero direction, not a zero diagonal).  The GPU tests allow `factor` = 16 times
each: device and host run one source, but the device build contracts products and sums into fma and has its own sin and cos.
The one decision -- whether the refined pose is taken -- is compared only where cost[0] - cost[end] >= 1e-6 cost[0], outside any rounding; a case that
does not is recorded under `left_out` and at most one may be.
"""
import json
import os
import shutil
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path.insert(0, TESTS)
sys.path.insert(0, ROOT)

FACTOR = 16
N_ITER = 5
SR_SIZES = (6, 7, 63, 64, 65, 255, 256, 257, 513)
REC = 9 + 3 + 7 + 11 + 36 + 49 + 1 + 1 + 49
KEYS = ("pose", "u", "cost", "cov6", "cov7", "pn")
X7 = np.array([0.3, -0.2, 0.1, 0.8, 0.2, -0.4, 0.1])           # the pose Pn is evaluated at for the cases that have no filter (not normalised, on purpose)


def build_host(d, sanitize=False):
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        return None, False
    exe = os.path.join(d, "pnp_refine_host_main")
    base = [cxx, "-O1", "-g", "-std=c++17", "-I", os.path.join(ROOT, "3pre_amd", "csrc"), os.path.join(TESTS, "pnp_refine_host_main.cpp"), "-o", exe]
    if sanitize:
        san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
        if san.returncode == 0:
            return exe, True
    subprocess.check_call(base)
    return exe, False


def run_host(exe, d, cases):
    """cases: list of dict(Xw, U (pixels as the sums take them), cam, R0, T0, n_iter, sigma_px, sta_in, x7) -> list of dicts"""
    payload = [struct.pack("<i", len(cases))]
    for c in cases:
        Xw, U = np.ascontiguousarray(c["Xw"], np.float64).reshape(-1, 3), np.ascontiguousarray(c["U"], np.float64).reshape(-1, 2)
        head = struct.pack("<4i4d", len(Xw), int(c["n_iter"]), int(c.get("sta_in", 1)), 0, float(c["cam"][0]), float(c["cam"][1]), float(c["cam"][2]),
                           float(c.get("sigma_px", 0.0)))
        x7 = np.asarray(c.get("x7", X7), np.float64)
        payload.append(head + np.ascontiguousarray(c["R0"], np.float64).tobytes() + np.ascontiguousarray(c["T0"], np.float64).tobytes() + x7.tobytes()
                       + Xw.tobytes() + U.tobytes())
    fi, fo = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    with open(fi, "wb") as f:
        f.write(b"".join(payload))
    r = subprocess.run([exe, fi, fo], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw = np.fromfile(fo, np.float64).reshape(len(cases), REC)
    return [dict(R=v[:9].reshape(3, 3), T=v[9:12], u=v[12:19], cost=v[19:30], cov6=v[30:66].reshape(6, 6), cov=v[66:115].reshape(7, 7), sigma2=v[115],
                 sta=int(v[116]), Pn=v[117:166].reshape(7, 7)) for v in raw]


def rel_cov(got, want):
    d = np.sqrt(np.abs(np.diag(want)))
    return float((np.abs(got - want) / np.outer(d, d)).max())


def diffs(h, r, pn_want=None):
    """the six differences of an answer h (host or device) and the restatement's r; pn_want: the restated Pn, where there is one to compare"""
    fin = np.isfinite(r["cost"])
    assert np.array_equal(np.isfinite(h["cost"]), fin)
    out = dict(pose=float(max(np.abs(h["R"] - r["R"]).max(), np.abs(h["T"] - r["T"]).max())), u=float(np.abs(h["u"] - r["u"]).max()),
               cost=float((np.abs(h["cost"][fin] - r["cost"][fin]) / np.maximum(1.0, r["cost"][fin])).max()),
               cov6=rel_cov(h["cov6"], r["cov6"]), cov7=rel_cov(h["cov"], r["cov"]))
    out["pn"] = rel_cov(h["Pn"], pn_want) if pn_want is not None else 0.0
    return out


def decided(r):
    """the taking decision lies outside rounding"""
    c = r["cost"]
    return c[0] - c[r["n_iter"]] >= 1e-6 * c[0]


def cases():
    """name -> the host case dict (its pixels undistorted where the scene asks for it) with the restatement's EPnP pose as the start"""
    import epnp_ref as ref
    import pnp_cases as pc
    import reloc_cases as rc
    out = {}
    for n in SR_SIZES:
        Xw, U, _, _, _ = pc.sr_scene(n, 100 + n)
        e = ref.epnp(Xw, U, pc.fixture_cam())
        out["sr_%d" % n] = dict(Xw=Xw, U=U, cam=pc.fixture_cam(), R0=e["R"], T0=e["T"], n_iter=N_ITER, sigma_px=0.0, sta_in=e["sta"], x7=X7)
    for name in rc.names():
        w, sc = rc.restated(name), rc.scene(name)
        if w["pnp"] is None:
            continue
        inl = np.nonzero(w["inliers"])[0]
        out["reloc_" + name] = dict(Xw=w["Xw"][inl], U=w["Uu"][inl], cam=sc["cam"], R0=w["pnp"]["R"], T0=w["pnp"]["T"], n_iter=N_ITER, sigma_px=0.0,
                                    sta_in=w["sta"], x7=sc["x"][:7])
    return out


def restate(c):
    import pnp_refine_ref as gn
    r = gn.refine(c["Xw"], c["U"], c["cam"], c["R0"], c["T0"], c["n_iter"], c["sigma_px"], c["sta_in"])
    return r, (gn.noise_from_pose(c["x7"], r["cov"]) if r["sta"] in (1, 2) else None)


def measure():
    with tempfile.TemporaryDirectory() as d:
        exe, _ = build_host(d)
        assert exe is not None, "no host C++ compiler"
        named = cases()
        hs = run_host(exe, d, list(named.values()))
    rec, floors, left_out = {}, {k: 0.0 for k in KEYS}, []
    for (name, c), h in zip(named.items(), hs):
        r, pn = restate(c)
        assert r["sta"] in (1, 2) and h["sta"] in (1, 2), "no covariance on %s" % name
        if r["sta"] == 1 and not decided(r):
            left_out.append(name)
        else:
            assert h["sta"] == r["sta"], "the host build and the restatement decide differently on %s" % name
        if h["sta"] != r["sta"]:
            continue
        df = diffs(h, r, pn)
        rec[name] = dict(n=len(c["Xw"]), sta=r["sta"], **df)
        for k in KEYS:
            floors[k] = max(floors[k], df[k])
    assert len(left_out) <= 1, left_out
    tab = {"factor": FACTOR, "n_iter": N_ITER, "left_out": left_out, "cases": rec}
    for k in KEYS:
        tab["floor_" + k] = floors[k]
        tab["tol_" + k] = FACTOR * floors[k]
    return tab


if __name__ == "__main__":
    tab = measure()
    with open(os.path.join(HERE, "pnp_refine_tolerance.json"), "w") as f:
        json.dump(tab, f, indent=1)
        f.write("\n")
    print(json.dumps(tab, indent=1))
