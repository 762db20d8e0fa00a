"""tests/golden/pnp_tolerance.json: what separates the Jacobi eigensolver of 3pre_amd/csrc/pre3_pnp.h, run on the host (tests/pnp_host_main.cpp), from
tests/epnp_ref.py over LAPACK on the committed cases of tests/pnp_cases.py -- the whole-set cases and every hypothesis of the RANSAC scenes.

    python tests/golden/make_pnp_tolerance.py

Three floors: the largest absolute difference in R and T (T in metres; the scenes are 1-7 m deep, the long-lens case 60 m), in err and in a
per-point reprojection distance, these two as |difference| / max(1 px, value) (rel()).  The GPU tests allow `factor` = 16 times each: device and
host run one source, but the device build contracts products and sums into fma where the host build does not, a few last-place differences amplified by the same conditioning.  `guard` is
64 times the distance floor: decisions the restatement takes nearer than that to their edge are left out of the exact comparison.
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

FACTOR, GUARD_FACTOR = 16, 64
# dim3_good is ill-conditioned on purpose (a near-planar scene 60 m away under a 16000 px lens, 3 px noise: what it takes for dimension 3 to be entered
# and to end below 20): its one- and two-vector answers have err in the thousands of pixels and move by 1e-6 of that between the two eigensolvers.  It
# is held to 16 times its own record, and kept out of the floors every other case is held to.
# fixture_true is noise-free: its two-vector answer has beta2 = sqrt(|b(3)|) with b(3) zero but for rounding (1e-11 here), and the square root of rounding
# noise is 3e-6 -- err(2) = 9e-6 px IS that noise, and moves by a third of itself between the two eigensolvers while the pose moves by 3e-14.  It too is
# held to 16 times its own record, so that every other case's err is held to the floor the noisy cases give.
OWN_FLOOR = ("dim3_good", "fixture_true")
REC = 9 + 3 + 7 + 3 + 4 + 12


def build_host(d, sanitize=False):
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        return None, False
    exe = os.path.join(d, "pnp_host_main")
    base = [cxx, "-O1", "-g", "-std=c++17", "-I", os.path.join(ROOT, "3pre_amd", "csrc"), os.path.join(TESTS, "pnp_host_main.cpp"), "-o", exe]
    if sanitize:
        san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
        if san.returncode == 0:
            return exe, True
    subprocess.check_call(base)
    return exe, False


def run_host(exe, d, cases):
    """cases: list of (Xw, U, cam) -> list of dicts"""
    payload = [struct.pack("<i", len(cases))]
    for Xw, U, cam in cases:
        Xw, U = np.ascontiguousarray(Xw, np.float64), np.ascontiguousarray(U, np.float64)
        payload.append(struct.pack("<2i3d", len(Xw), 0, float(cam[0]), float(cam[1]), float(cam[2])) + Xw.tobytes() + U.tobytes())
    fi, fo = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    with open(fi, "wb") as f:
        f.write(b"".join(payload))
    r = subprocess.run([exe, fi, fo], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw = np.fromfile(fo, np.float64)
    out, o = [], 0
    for Xw, U, cam in cases:
        n = len(Xw)
        v = raw[o:o + REC]
        out.append(dict(R=v[:9].reshape(3, 3), T=v[9:12], u=v[12:19], err=v[19:22], best=int(v[22]), sta=int(v[23]), dim3=bool(v[24]), sweeps=int(v[25]),
                        w=v[26:38], d=raw[o + REC:o + REC + n]))
        o += REC + n
    assert o == len(raw)
    return out


def rel(got, want):
    """the largest |got - want| / max(1, |want|): pixels for a value below one pixel, a fraction above it -- a poor six-point sample has an err of
    1e5 px, which moves in its sixth digit"""
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())


def diffs(h, r):
    """(pose, err, distance) differences of a host answer and the restatement's; None where the two decide differently or one is not finite"""
    if h["sta"] != r["sta"] or h["best"] != r["best"] or h["dim3"] != r["dim3"] or r["sta"] == -1:
        return None
    fin = np.isfinite(r["err"])
    return (max(np.abs(h["R"] - r["R"]).max(), np.abs(h["T"] - r["T"]).max()), rel(h["err"][fin], r["err"][fin]), rel(h["d"], r["d"]))


def measure():
    import epnp_ref as ref
    import pnp_cases as pc
    with tempfile.TemporaryDirectory() as d:
        exe, _ = build_host(d)
        assert exe is not None, "no host C++ compiler"
        named = pc.tolerance_cases()
        whole = run_host(exe, d, list(named.values()))
        rec = {}
        floors = np.zeros(3)
        for (name, (Xw, U, cam)), h in zip(named.items(), whole):
            r = ref.epnp(Xw, U, cam)
            df = diffs(h, r)
            assert df is not None, "the host build and the restatement decide differently on %s" % name
            rec[name] = {"n": len(Xw), "pose": df[0], "err": df[1], "dist": df[2], "sweeps": h["sweeps"]}
            if name not in OWN_FLOOR:
                floors = np.maximum(floors, df)
        hyp = {}
        for n_hyp in pc.RANSAC_SEEDS:
            sc = pc.ransac_scene(n_hyp)
            hs = run_host(exe, d, [(sc["Xw"][dr], sc["U"][dr], sc["cam"]) for dr in sc["draws"]])
            worst, differ = np.zeros(3), 0
            for dr, h in zip(sc["draws"], hs):
                df = diffs(h, ref.epnp(sc["Xw"][dr], sc["U"][dr], sc["cam"]))
                if df is None:
                    differ += 1
                else:
                    worst = np.maximum(worst, df)
            hyp[str(n_hyp)] = {"pose": worst[0], "err": worst[1], "dist": worst[2], "decide_differently": differ}
            floors = np.maximum(floors, worst)
    return {"factor": FACTOR, "guard_factor": GUARD_FACTOR, "floor_pose": floors[0], "floor_err": floors[1], "floor_dist": floors[2],
            "tol_pose": FACTOR * floors[0], "tol_err": FACTOR * floors[1], "tol_dist": FACTOR * floors[2], "guard": GUARD_FACTOR * floors[2],
            "cases": rec, "hypotheses": hyp}


if __name__ == "__main__":
    tab = measure()
    with open(os.path.join(HERE, "pnp_tolerance.json"), "w") as f:
        json.dump(tab, f, indent=1)
        f.write("\n")
    print(json.dumps(tab, indent=1))
