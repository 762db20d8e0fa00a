"""CPU: the ICP's closed-form covariance and the rule by which the prediction takes u and Pn from a refined pair.
3pre_amd/csrc/pre3_predicticp.h and pre3_icpcov.h compiled for the host (tests/icp_cov_host_main.cpp, with the address and undefined-behaviour
sanitizers where the compiler has them) against the restatement tests/icp_cov_ref.py: the selection rule over its whole grid; the tree of partial sums
of the two launches, restated on one thread with vc_add_point, at p = 3, 4, 255, 256, 257, 1219 under the committed gate; the gate reproduced; the new
symbols declared, exported and mirrored."""
import ctypes as C
import importlib
import inspect
import itertools
import json
import os
import re
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

import icp_cov_ref as ref
import icp_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_icp_cov_tolerance as T  # noqa: E402

TAB = json.load(open(os.path.join(ROOT, "tests", "golden", "icp_cov_tolerance.json")))
SYMBOLS = {"pre3_icp_cov": 11, "pre3_icp_cov_limits": 1, "pre3_icp_cov_bench": 10,"pre3_icp_pair_cov_seeded": 26, "pre3_predict_icp_pair_seeded": 16}
MEX_SRC = os.path.join(ROOT, "mex", "ekf_ctx_gateway.c")


def test_the_symbols_are_declared_exported_and_mirrored(pre3):
    txt = open(os.path.join(ROOT, "include", "pre3.h")).read()
    declared = set(re.findall(r"PRE3_API\s+[\w\s\*]+?\b(pre3_\w+)\s*\(", txt))
    _lib = importlib.import_module("3pre_amd._lib")
    so = C.CDLL(pre3.LIB_PATH)
    for sym, nargs in SYMBOLS.items():
        assert sym in declared, "include/pre3.h does not declare %s" % sym
        assert hasattr(so, sym), "libpre3.so does not export %s" % sym
        assert sym in _lib.EXPORTS and len(getattr(_lib.lib, sym).argtypes) == nargs, sym
    vo = importlib.import_module("3pre_amd.vo")
    assert list(inspect.signature(vo.icp_cov).parameters) == ["data1", "data2", "corr", "u", "device"]
    assert list(inspect.signature(vo.icp_pair_cov_seeded).parameters) == list(inspect.signature(vo.icp_pair_seeded).parameters)
    out = np.zeros(2, np.int32)
    assert _lib.lib.pre3_icp_cov_limits(_lib.dptr(out)) == 0 and out.tolist() == [256, 4]          # no device is touched
    assert _lib.lib.pre3_icp_cov_limits(None) == -1
    for k, v in (("CONTEXT", ref.NOISE_CONTEXT), ("PAIR", ref.NOISE_PAIR), ("ICP", ref.NOISE_ICP), ("ICP_FLOOR", ref.NOISE_ICP_FLOOR)):      # the noise modes
        assert re.search(r"#define\s+PRE3_%s\s+%d\b" % ("NOISE_" + k, v), txt), k
    ekf, srm = (importlib.import_module("3pre_amd." + m) for m in ("ekf", "sr4000"))
    assert list(inspect.signature(ekf.EkfFilter.ekf_prediction_icp_pair_seeded).parameters) == [
        "self", "prev", "cur", "seed", "seq", "thresh", "stride", "res", "max_error", "noise", "wait"]

    class Recorder:
        def __getattr__(self, name):
            return lambda *a: (name,) + a
    assert srm.ekf_prediction_frames_icp(Recorder(), 5, {3: "A", 4: "B"}, 1, noise=3)[:3] == ("ekf_prediction_icp_pair_seeded", "A", "B")
    assert srm.ekf_prediction_frames_icp(Recorder(), 5, {3: "A", 4: "B"}, 1, noise=3)[-2:] == (3, True)
    assert srm.ekf_prediction_frames_icp(Recorder(), 2, {}, 1) is None                           # fv.m:41-48: the identity frames
    assert _lib.lib.pre3_predict_icp_pair_seeded(None, None, None, 1.5, 1, 0, 1, 0.02, float("inf"), 0, None, None, None, None, None, None) == -1


def test_the_gateway_has_the_new_commands():
    src = open(MEX_SRC).read()
    for cmd, entry in (("icp_cov", "pre3_icp_cov("), ("predict_icp_pair", "pre3_predict_icp_pair_seeded(")):
        assert '!strcmp(cmd, "%s")' % cmd in src and entry in src


def test_argument_errors_come_before_a_device_is_touched(pre3):
    _lib = importlib.import_module("3pre_amd._lib")
    lib, dptr = _lib.lib, _lib.dptr
    pts, u, cov, st = np.ones((5, 3)), np.array([0, 0, 0, 1.0, 0, 0, 0]), np.full(49, 7.0), C.c_int32(7)
    good = np.array([[1, 1], [2, 2], [3, 3], [4, 4]], np.int32)
    for what, corr in (("model index 0", [[0, 1]]), ("model index n1 + 1", [[6, 1]]), ("source index 0", [[1, 0]]), ("source index n2 + 1", [[1, 6]]),
                       ("the last row", [[1, 1], [2, 2], [3, 3], [4, 4], [5, -1]])):
        c = np.array(corr, np.int32)
        assert lib.pre3_icp_cov(0, dptr(pts), 5, dptr(pts), 5, dptr(c), len(c), dptr(u), dptr(cov), C.byref(st), None) == -1, what
        assert b"pre3_icp_cov" in lib.pre3_last_error()
    assert lib.pre3_icp_cov(0, None, 5, dptr(pts), 5, dptr(good), 4, dptr(u), dptr(cov), C.byref(st), None) == -1
    assert lib.pre3_icp_cov(0, dptr(pts), 5, dptr(pts), 5, None, 4, dptr(u), dptr(cov), C.byref(st), None) == -1
    assert lib.pre3_icp_cov(0, dptr(pts), 5, dptr(pts), 5, dptr(good), -1, dptr(u), dptr(cov), C.byref(st), None) == -1
    assert lib.pre3_icp_cov(0, dptr(pts), 5, dptr(pts), 5, dptr(good), 256 * 256 * 4 + 1, dptr(u), dptr(cov), C.byref(st), None) == -1
    assert lib.pre3_icp_cov(0, dptr(pts), 5, dptr(pts), 5, dptr(good), 4, None, dptr(cov), C.byref(st), None) == -1
    assert lib.pre3_icp_cov(0, dptr(pts), 5, dptr(pts), 5, dptr(good), 4, dptr(u), dptr(cov), None, None) == -1
    assert st.value == 7 and (cov == 7.0).all()


def test_the_scenes_hold_their_margins_and_are_well_conditioned():
    """on the restatement alone: only then do the pairs of two fp64 implementations have to agree, and only then does the gate mean anything"""
    for n1, n2 in ref.SHAPES:
        s, r = ref.scene(n1, n2)
        assert icp_ref.margins_ok(r) and r["sta"] == 1, (n1, n2, r["margins"])
        H, M, n, finite = ref.sums(s["data1"], s["data2"], r["corr"], r["u"])
        cov, status, _ = ref.cov(s["data1"], s["data2"], r["corr"], r["u"])
        print(n1, n2, "p", n, "cond(H) %.1f" % np.linalg.cond(H), "sigma_T mm", 1000 * np.sqrt(np.diag(cov)[:3]))
        assert finite and status == 1 and np.linalg.cond(H) < 2000
        assert np.all(np.linalg.eigvalsh(cov) > -1e-12 * np.abs(cov).max())
    assert [ref.scene(*sh)[1]["p"] for sh in ref.SHAPES] == [57, 499, 1219]


def test_the_committed_tolerance_is_reproduced():
    got = T.measure()
    assert list(got["cases"]) == list(TAB["cases"]) or set(got["cases"]) == set(TAB["cases"])
    assert got["factor"] == TAB["factor"] == 16 and got["full"] == TAB["full"]
    for k, w in TAB["cases"].items():
        g = got["cases"][k]
        assert g["p"] == w["p"] and abs(g["cond"] - w["cond"]) <= 1e-6 * w["cond"]
        # (another libm or LAPACK build moves every trial by its own last ulps: a small factor, not a percentage)
        assert w["floor"] / 4 <= g["floor"] <= w["floor"] * 4, k
        assert w["tol"] == 16 * max(w["floor"], TAB["floor_full"])
    assert TAB["floor_full"] == max(TAB["cases"][k]["floor"] for k in TAB["full"])
    assert max(TAB["cases"][k]["cond"] for k in TAB["full"]) < 2000


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("icp_cov_host")
    exe = d / "icp_cov_host_main"
    base = [cxx, "-O1", "-g", "-std=c++17", "-I", os.path.join(ROOT, "3pre_amd", "csrc"), os.path.join(ROOT, "tests", "icp_cov_host_main.cpp"), "-o", str(exe)]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if san.returncode != 0:                                  # a compiler without the sanitizers' runtimes: the same program without them
        subprocess.check_call(base)

    def run(payload):
        fi, fo = d / "in.bin", d / "out.bin"
        fi.write_bytes(payload)
        r = subprocess.run([str(exe), str(fi), str(fo)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        return fo.read_bytes()
    return run


STA, PNUM, BAD, DIST_OK = (0, 1, 2), (3, 4, 12), (0, 1), (0, 1)
ICP_STA, FINITE, ERR = (0, 1, 2, 3), (0, 1), ((0.5, 1.0), (1.0, 1.0), (1.5, 1.0), (1e6, float("inf")), (float("nan"), float("inf")))
COV_STATUS, NOISE = (0, 1, 2), (0, 1, 2, 3)


def test_the_selection_rule_header_against_its_restatement_over_the_whole_grid(host_exe):
    grid = list(itertools.product(STA, PNUM, BAD, DIST_OK, ICP_STA, FINITE, ERR, NOISE, COV_STATUS, COV_STATUS))
    rec = b"".join(struct.pack("<10i2d", g[0], g[1], g[2], g[3], g[4], g[5], g[7], g[8], g[9], 0, g[6][0], g[6][1]) for g in grid)
    out = np.frombuffer(host_exe(struct.pack("<2i", 0, len(grid)) + rec), np.int32).reshape(len(grid), 4)
    seen = set()
    for g, o in zip(grid, out):
        sta, pnum, bad, dist_ok, icp_sta, finite, (err, max_err), noise, cps, cis = g
        u_taken, noise_taken, refusal = ref.select(sta, pnum, bad, dist_ok, icp_sta, bool(finite), err, max_err, noise, cps, cis)
        assert (int(o[0]), int(o[1]), int(o[2])) == (refusal, u_taken, noise_taken), g
        assert int(o[3]) == u_taken, "the u that comes out is the one reported: %r" % (g,)
        seen.add((u_taken, noise_taken))
    # every combination the rule can give: the identity and the pair's u never come with the ICP's noise
    assert seen == {(0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2), (2, 3)}


def _tree(host_exe, d1, d2, corr, u):
    P1, P2 = ref.gather(d1, d2, corr) if len(corr) else (np.zeros((3, 0)), np.zeros((3, 0)))
    pts = np.ascontiguousarray(np.concatenate([P1.T, P2.T], axis=1))
    rec = host_exe(struct.pack("<2i", 1, len(corr)) + pts.tobytes() + np.asarray(u, np.float64).tobytes())
    status, n = struct.unpack("<2i", rec[:8])
    return status, n, np.frombuffer(rec[8:], np.float64).reshape(7, 7)


@pytest.mark.parametrize("p", [4, 255, 256, 257, 1219])
def test_the_tree_of_partial_sums_against_the_restatement(host_exe, p):
    n1, n2 = ref.SHAPES[-1]
    s, r = ref.scene(n1, n2)
    corr = r["corr"][:p, :2]
    assert len(corr) == p
    status, n, cov = _tree(host_exe, s["data1"], s["data2"], corr, r["u"])
    cr, sr, nr = ref.cov(s["data1"], s["data2"], corr, r["u"])
    tol = T.tolerance(TAB, ref.case_name(n1, n2, p))
    err = np.abs(cov - cr).max() / np.abs(cr).max()
    print("p", p, "relative difference %.3e" % err, "gate %.3e" % tol)
    assert (status, n) == (sr, nr) == (1, p)
    assert np.array_equal(cov, cov.T)
    assert err <= tol


def test_the_tree_gives_the_status_rule(host_exe):
    n1, n2 = ref.SHAPES[0]
    s, r = ref.scene(n1, n2)
    assert _tree(host_exe, s["data1"], s["data2"], r["corr"][:3, :2], r["u"])[:2] == (0, 0) and ref.cov(s["data1"], s["data2"], r["corr"][:3], r["u"])[1] == 0
    bad = s["data2"].copy()
    bad[1, int(r["corr"][5, 1]) - 1] = np.nan
    status, n, cov = _tree(host_exe, s["data1"], bad, r["corr"][:, :2], r["u"])
    assert (status, n) == (2, r["p"]) and not cov.any() and ref.cov(s["data1"], bad, r["corr"], r["u"])[1] == 2
    # three pairs on the optical axis and one off it, the identity motion, zero residual: tests/test_vo_cov_ref.py's SINGULAR, as a list of pairs
    pts = np.array([[0, 0, 0, 0], [0, 0, 0, 5], [1, 2, 3, 4.0]])
    corr = np.array([[1, 1], [2, 2], [3, 3], [3, 3]])
    status, n, cov = _tree(host_exe, pts, pts, corr, np.array([0, 0, 0, 1.0, 0, 0, 0]))
    assert (status, n) == (2, 4) and not cov.any() and ref.cov(pts, pts, corr, np.array([0, 0, 0, 1.0, 0, 0, 0]))[1] == 2
