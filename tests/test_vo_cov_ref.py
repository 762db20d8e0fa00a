"""CPU: the VO pair's covariance and the caller-set process noise.  The restatement tests/vo_cov_ref.py against central finite
differences of E; 3pre_amd/csrc/pre3_vocov.h compiled for the host (tests/vo_cov_host_main.cpp) against that restatement -- the status rule over the
whole grid, the polynomial per-point terms within 1e-13 of the largest entry, the exactly singular case; the new symbols declared, exported and
mirrored; the MEX commands."""
import ctypes as C
import importlib
import inspect
import itertools
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import vo_cov_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"pre3_set_process_noise": 2, "pre3_get_process_noise": 3, "pre3_vo_cov": 9, "pre3_vo_pair_cov_seeded": 17, "pre3_predict_pair_cov_seeded": 10}
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
    ekf, srm, vo = (importlib.import_module("3pre_amd." + m) for m in ("ekf", "sr4000", "vo"))

    def params(fn):
        return list(inspect.signature(fn).parameters)

    assert params(ekf.EkfFilter.set_process_noise) == ["self", "Pn"]
    assert isinstance(ekf.EkfFilter.process_noise, property)
    assert params(ekf.EkfFilter.ekf_prediction_pair_cov_seeded) == ["self", "prev", "cur", "seed", "seq", "thresh", "wait"]
    assert params(vo.cov_pose_shift_calc)[:4] == ["Ya", "Yb", "R", "T"]
    assert params(vo.vo_pair_cov_seeded) == params(vo.vo_pair_seeded)
    assert params(srm.ekf_prediction_frames_cov) == params(srm.ekf_prediction_frames)

    class Recorder:
        def __getattr__(self, name):
            return lambda *a: (name,) + a
    assert srm.ekf_prediction_frames_cov(Recorder(), 5, {3: "A", 4: "B"}, 1)[:3] == ("ekf_prediction_pair_cov_seeded", "A", "B")
    assert srm.ekf_prediction_frames(Recorder(), 5, {3: "A", 4: "B"}, 1)[:3] == ("ekf_prediction_pair_seeded", "A", "B")
    assert srm.ekf_prediction_frames_cov(Recorder(), 2, {}, 1) is None          # fv.m:41-48: the identity frames


def _fd_cases():
    rng = np.random.default_rng(11)
    for _ in range(6):
        q = np.array([1.0, 0, 0, 0]) + rng.normal(scale=0.05, size=4)        # not normalised: R(q) is the homogeneous form
        X = np.concatenate([rng.normal(scale=0.05, size=3), q])
        fn = np.array([rng.uniform(-1.5, 1.5), rng.uniform(-1, 1), rng.uniform(1, 4)])
        fp = ref.rot(q) @ fn + X[:3] + rng.normal(scale=0.02, size=3)        # a residual of centimetres, so that the second-derivative terms count
        yield fp, fn, X


def test_H_i_and_B_i_are_the_second_derivatives_of_E():
    """central differences of E = 1/2 |r|^2 in X (H_i) and of dE/dX in the points (B_i); E is a quartic in X and quadratic in the points, so a step of
    1e-4 leaves a truncation error of h^2 E''''/12 ~ 1e-8 on entries of size 1 - 70, and rounding eps E / h^2 ~ 1e-9"""
    h = 1e-4
    for fp, fn, X in _fd_cases():
        Hi, Bi, r = ref.point_terms(fp, fn, X)
        E = lambda x, a=fp, b=fn: ref.energy(a[:, None], b[:, None], x)
        Hfd = np.zeros((7, 7))
        for a in range(7):
            for b in range(7):
                ea, eb = np.eye(7)[a] * h, np.eye(7)[b] * h
                Hfd[a, b] = (E(X + ea + eb) - E(X + ea - eb) - E(X - ea + eb) + E(X - ea - eb)) / (4 * h * h)
        assert np.abs(Hfd - Hi).max() < 1e-6 * np.abs(Hi).max(), np.abs(Hfd - Hi).max()
        assert np.array_equal(Hi, Hi.T) or np.abs(Hi - Hi.T).max() < 1e-14 * np.abs(Hi).max()

        def grad(a, b):                                   # dE/dX = J' r, itself checked against E's first differences below
            q = X[3:]
            J = np.hstack([np.eye(3), np.einsum("ijk,j->ik", ref.drot(q), b)])
            return J.T @ ref.residual(a, b, X)
        gfd = np.array([(E(X + np.eye(7)[a] * h) - E(X - np.eye(7)[a] * h)) / (2 * h) for a in range(7)])
        # (truncation h^2 E3 / 6 with the third derivative E3 = 3 r1 r2 <= 3 (2 |f|)^2 ~ 200 at |f| ~ 4 m: 3e-7)
        assert np.abs(gfd - grad(fp, fn)).max() < 1e-6
        Bfd = np.zeros((7, 6))
        for s in range(3):
            e = np.eye(3)[s] * h
            Bfd[:, s] = (grad(fp + e, fn) - grad(fp - e, fn)) / (2 * h)
            Bfd[:, 3 + s] = (grad(fp, fn + e) - grad(fp, fn - e)) / (2 * h)
        assert np.abs(Bfd - Bi).max() < 1e-8 * np.abs(Bi).max(), np.abs(Bfd - Bi).max()


def test_the_committed_cases_are_well_conditioned_and_give_sane_sigmas():
    sig = {}
    for c, spec in zip(ref.committed_cases(), ref.CASES):
        H, M, n, finite = ref.sums(c["pset1"], c["pset2"], c["inliers"], c["u"])
        assert finite and n == spec[2]
        assert np.linalg.cond(H) < 1e4, (spec, np.linalg.cond(H))
        cov, status, _ = ref.cov(c["pset1"], c["pset2"], c["inliers"], c["u"])
        assert status == 1 and np.all(np.linalg.eigvalsh(cov) > -1e-12 * np.abs(cov).max())
        sig[spec[2]] = np.sqrt(np.diag(cov)[:3]).mean()
    assert sig[3] > sig[65] and 1e-4 < sig[65] < 5e-3 and sig[3] < 0.1, sig          # more inliers, a tighter T; millimetres, as the constant's 3.3 mm


def test_the_committed_tolerance_is_reproduced():
    import json
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    gen = importlib.import_module("make_vo_cov_tolerance")
    got, want = gen.measure(), json.load(open(os.path.join(ROOT, "tests", "golden", "vo_cov_tolerance.json")))
    assert got["cases"] == want["cases"] and got["factor"] == want["factor"] == 16
    # (another libm or LAPACK build moves every trial by its own last ulps: the maximum over 108 trials stays within a small factor, not a percentage)
    assert want["floor"] / 4 <= got["floor"] <= want["floor"] * 4 and want["tol"] == 16 * want["floor"]
    assert want["cond_max"] < 1e4


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("vo_cov_host")
    exe = d / "vo_cov_host_main"
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "3pre_amd", "csrc"), os.path.join(ROOT, "tests", "vo_cov_host_main.cpp"), "-o", str(exe)])

    def run(payload):
        fi, fo = d / "in.bin", d / "out.bin"
        fi.write_bytes(payload)
        subprocess.run([str(exe), str(fi), str(fo)], check=True, timeout=60)
        return fo.read_bytes()
    return run


STA, PNUM, BAD, DIST_OK, STATUS = (-1, 0, 1, 2, 4), (0, 3, 4, 12), (0, 1, 2, 3), (0, 1), (0, 1, 2)


def test_the_status_rule_header_against_its_restatement_over_the_whole_grid(host_exe):
    grid = list(itertools.product(STA, PNUM, BAD, DIST_OK, STATUS))
    out = np.frombuffer(host_exe(struct.pack("<2i", 0, len(grid)) + b"".join(struct.pack("<5i", *g) for g in grid)), np.int32).reshape(len(grid), 3)
    taken = 0
    for g, o in zip(grid, out):
        computes, takes = ref.pair_takes_u(*g[:4]), ref.predict_takes(*g)
        assert (bool(o[0]), bool(o[1])) == (bool(computes), takes), g
        assert bool(o[0]) == bool(o[2]), "a covariance is computed exactly for the pairs whose u predict_u_select takes: %r" % (g,)
        taken += takes
    assert taken == 2 * 1 * 1 * 1 * 1          # sta == 1, pnum in (4, 12), bad == 0, dist_ok == 1, status == 1


def test_the_headers_per_point_terms_against_the_restatement(host_exe):
    cases = list(_fd_cases())
    c0 = ref.committed_cases()[3]
    cases += [(c0["pset1"][:, k], c0["pset2"][:, k], c0["u"]) for k in range(0, 65, 7)]
    rec = host_exe(struct.pack("<2i", 1, len(cases)) + b"".join(np.concatenate(c).astype(np.float64).tobytes() for c in cases))
    out = np.frombuffer(rec, np.float64).reshape(len(cases), 49 + 42 + 3 + 18)
    for (fp, fn, X), o in zip(cases, out):
        Hi, Bi, r = ref.point_terms(fp, fn, X)
        assert np.abs(o[:49].reshape(7, 7) - Hi).max() <= 1e-13 * np.abs(Hi).max()         # polynomials: no transcendentals
        assert np.abs(o[49:91].reshape(7, 6) - Bi).max() <= 1e-13 * np.abs(Bi).max()
        assert np.abs(o[91:94] - r).max() <= 1e-13 * max(np.abs(fp).max(), np.abs(fn).max())
        for C9, p in ((o[94:103], fp), (o[103:112], fn)):           # sin / cos / atan2 / hypot of two libms: a few ulp of entries of the largest one's size
            Cr = ref.point_cov(p)
            assert np.abs(C9.reshape(3, 3) - Cr).max() <= 1e-12 * np.abs(Cr).max()


def _mode2(host_exe, c):
    pnum = c["pset1"].shape[1]
    payload = struct.pack("<2i", 2, pnum) + np.ascontiguousarray(c["pset1"].T).tobytes() + np.ascontiguousarray(c["pset2"].T).tobytes()
    payload += np.asarray(c["inliers"], np.int32).tobytes() + np.asarray(c["u"], np.float64).tobytes()
    rec = host_exe(payload)
    status, n = struct.unpack("<2i", rec[:8])
    return status, n, np.frombuffer(rec[8:], np.float64).reshape(7, 7)


SINGULAR = dict(pset1=np.array([[0, 0, 0, 0], [0, 0, 0, 5], [1, 2, 3, 4.0]]), pset2=np.array([[0, 0, 0, 0], [0, 0, 0, 5], [1, 2, 3, 4.0]]),
                inliers=np.array([1, 1, 1, 0], np.int32), u=np.array([0, 0, 0, 1.0, 0, 0, 0]))


def test_the_headers_whole_covariance_on_the_host(host_exe):
    tol = float(__import__("json").load(open(os.path.join(ROOT, "tests", "golden", "vo_cov_tolerance.json")))["floor"]) * 16
    for c in ref.committed_cases():
        status, n, cov = _mode2(host_exe, c)
        cr, sr, nr = ref.cov(c["pset1"], c["pset2"], c["inliers"], c["u"])
        assert (status, n) == (sr, nr) == (1, int(c["inliers"].sum()))
        assert np.array_equal(cov, cov.T)
        assert np.abs(cov - cr).max() <= tol * np.abs(cr).max(), np.abs(cov - cr).max() / np.abs(cr).max()


def test_three_collinear_points_are_unusable_on_the_host(host_exe):
    """three points on the optical axis, the identity motion, zero residual: the rotation about that axis moves nothing, row and column q_d of H are
    exactly zero, every product and sum in front of that pivot is exact, and the pivot is exactly 0 <= 7 eps * 0"""
    status, n, cov = _mode2(host_exe, SINGULAR)
    assert (status, n) == (2, 3) and not cov.any()
    assert ref.cov(SINGULAR["pset1"], SINGULAR["pset2"], SINGULAR["inliers"], SINGULAR["u"])[1] == 2
    bad = {k: np.array(v, copy=True) for k, v in ref.committed_cases()[2].items()}
    bad["pset2"][1, int(np.flatnonzero(bad["inliers"])[5])] = np.nan
    assert _mode2(host_exe, bad)[0] == 2 and ref.cov(bad["pset1"], bad["pset2"], bad["inliers"], bad["u"])[1] == 2
    few = {k: (v[:, :3] if v.ndim == 2 else v[:3] if k == "inliers" else v) for k, v in ref.committed_cases()[0].items()}
    assert _mode2(host_exe, few)[0] == 0 and ref.cov(few["pset1"], few["pset2"], few["inliers"], few["u"])[1] == 0


def test_set_process_noise_refuses_before_a_device_is_touched(pre3):
    _lib = importlib.import_module("3pre_amd._lib")
    assert _lib.lib.pre3_set_process_noise(None, None) == -1 and _lib.lib.pre3_get_process_noise(None, None, None) == -1
    st = C.c_int32(7)
    assert _lib.lib.pre3_vo_cov(0, -1, None, None, None, None, None, C.byref(st), None) != 0 and st.value == 7


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_the_gateway_with_the_new_commands_passes_the_compiler_front_end():
    src = open(MEX_SRC).read()
    for cmd in ("process_noise", "vo_cov", "predict_pair_cov"):
        assert '!strcmp(cmd, "%s")' % cmd in src
    r = subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-Wextra", "-Werror=implicit-function-declaration", "-Werror=incompatible-pointer-types",
                        "-Werror=int-conversion", "-I", os.path.join(ROOT, "tests", "mex_api_decl"), "-I", os.path.join(ROOT, "include"), MEX_SRC],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
