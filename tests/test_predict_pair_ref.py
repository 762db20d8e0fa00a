"""CPU: the prediction fed from a resident VO pair.  The new symbol is declared, exported and mirrored; pre3_predictu.h (the rule
k_predict's device form evaluates: which increment, and which pairs are refused) compiled for the host against a restatement written here, bit for
bit over the whole grid of result blocks; fv.m:41-48's index rule; the argument errors that return before a device is touched; the MEX command."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "pre3_predict_pair_seeded"
MEX_SRC = os.path.join(ROOT, "mex", "ekf_ctx_gateway.c")


def test_the_symbol_is_declared_exported_and_mirrored(pre3):
    txt = open(os.path.join(ROOT, "include", "pre3.h")).read()
    declared = set(re.findall(r"PRE3_API\s+[\w\s\*]+?\b(pre3_\w+)\s*\(", txt))
    assert SYMBOL in declared, "include/pre3.h does not declare %s" % SYMBOL
    assert hasattr(C.CDLL(pre3.LIB_PATH), SYMBOL), "libpre3.so does not export %s" % SYMBOL
    _lib = importlib.import_module("3pre_amd._lib")
    assert SYMBOL in _lib.EXPORTS and len(getattr(_lib.lib, SYMBOL).argtypes) == 8
    ekf, srm = (importlib.import_module("3pre_amd." + m) for m in ("ekf", "sr4000"))

    def params(fn):
        return list(inspect.signature(fn).parameters)

    assert params(ekf.EkfFilter.ekf_prediction_pair_seeded) == ["self", "prev", "cur", "seed", "seq", "thresh", "wait"]
    assert params(srm.ekf_prediction_frames) == ["filt", "step", "frames", "seed", "seq", "thresh", "wait"]
    sig = inspect.signature(ekf.EkfFilter.ekf_prediction_pair_seeded).parameters
    assert (sig["seq"].default, sig["thresh"].default, sig["wait"].default) == (0, 1.5, True)


HOST_PROGRAM = r"""
#include <cstdio>
#include "pre3_predictu.h"
using namespace pre3;
// stdin: records of int32 sta, pnum, bad, dist_ok | 7 doubles u_in;  stdout: per record 7 doubles u_out | the refusal code | its error word, as doubles
int main()
{
    int32_t h[4]; double u[7];
    while (fread(h, 4, 4, stdin) == 4) {
        if (fread(u, 8, 7, stdin) != 7) return 2;
        double o[9] = { 7, 7, 7, 7, 7, 7, 7, 7, 7 };
        const int rf = predict_u_select(h[0], h[1], h[2], h[3], u, o);
        o[7] = rf; o[8] = pu_word_refusal(pu_error_word(rf)) == rf ? pu_error_word(rf) : -1;
        if (fwrite(o, 8, 9, stdout) != 9) return 3;
    }
    // with fewer than four matches the block must not be read at all: a null u_in has to do
    double o[7];
    if (predict_u_select(0, 3, 0, 0, nullptr, o) != PU_OK || predict_u_select(4, 12, 0, 1, nullptr, o) != PU_OK) return 4;
    return 0;
}
"""

STA, PNUM, BAD, DIST_OK = (-1, 0, 1, 2, 4), (0, 3, 4, 12), (0, 1, 2), (0, 1)
U_DISTINCT = np.array([0.25, -1.5, 3.0, 0.8, -0.1, 0.2, -0.3])
IDENTITY = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
OK, REFUSED_BAD, REFUSED_NEAR = 0, 1, 2


def rule(sta, pnum, bad, dist_ok, u_in):
    """The restatement.  pre3_vo_pair_seeded's order: fewer than four matches is a result whatever else the header says; then the bad flags
    (PRE3_E_HIP there), then the 0.4 m check (PRE3_E_NUMERIC); a pair that passes gives its u when sta == 1 and the identity motion otherwise
    (Calculate_V_Omega_RANSAC_dr_ye.m:41-50)."""
    if pnum < 4:
        return IDENTITY, OK
    if bad != 0:
        return IDENTITY, REFUSED_BAD
    if dist_ok == 0:
        return IDENTITY, REFUSED_NEAR
    return (u_in if sta == 1 else IDENTITY), OK


@pytest.fixture(scope="module")
def rule_exe(tmp_path_factory):
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("predictu_host")
    src, exe = d / "predictu_host.cpp", d / "predictu_host"
    src.write_text(HOST_PROGRAM)
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "3pre_amd", "csrc"), str(src), "-o", str(exe)])
    return str(exe)


def run_rule(exe, cases):
    inp = b"".join(struct.pack("<4i", *c[:4]) + np.asarray(c[4], np.float64).tobytes() for c in cases)
    r = subprocess.run([exe], input=inp, stdout=subprocess.PIPE, check=True)
    return np.frombuffer(r.stdout, np.float64).reshape(len(cases), 9)


@pytest.mark.parametrize("u_in", [U_DISTINCT, np.zeros(7)], ids=["distinct", "zero_block"])
def test_the_rule_header_against_the_restatement_over_the_whole_grid(rule_exe, u_in):
    cases = [(s, p, b, d, u_in) for s, p, b, d in itertools.product(STA, PNUM, BAD, DIST_OK)]
    assert len(cases) == 120
    got = run_rule(rule_exe, cases)
    for c, g in zip(cases, got):
        u_ref, rf = rule(*c)
        assert np.array_equal(g[:7].view(np.uint64), np.asarray(u_ref, np.float64).view(np.uint64)), c[:4]
        assert int(g[7]) == rf, c[:4]
        # the error word of a refusal is neither zero nor the factorisation's 1, and maps back to its refusal
        assert int(g[8]) == (1 + rf) and (rf == OK or int(g[8]) not in (0, 1)), c[:4]


def test_the_named_cases(rule_exe):
    zero = np.zeros(7)
    got = run_rule(rule_exe, [(0, 0, 0, 0, zero), (0, 3, 0, 0, zero), (4, 12, 0, 0, U_DISTINCT), (1, 12, 0, 0, U_DISTINCT), (4, 12, 0, 1, U_DISTINCT),
                              (1, 12, 0, 1, U_DISTINCT), (1, 12, 2, 1, U_DISTINCT), (1, 3, 1, 0, U_DISTINCT)])
    ident = IDENTITY.view(np.uint64)
    for k in (0, 1):                                   # pnum < 4 with the block still the zeros of the memset: identity (u[3] = 1, not 0), no refusal
        assert np.array_equal(got[k, :7].view(np.uint64), ident) and got[k, 7] == OK
    for k in (2, 3):                                   # pnum >= 4, dist_ok = 0: identity and refusal
        assert np.array_equal(got[k, :7].view(np.uint64), ident) and got[k, 7] == REFUSED_NEAR
    assert np.array_equal(got[4, :7].view(np.uint64), ident) and got[4, 7] == OK           # no consensus with pnum >= 4
    assert np.array_equal(got[5, :7].view(np.uint64), U_DISTINCT.view(np.uint64)) and got[5, 7] == OK
    assert np.array_equal(got[6, :7].view(np.uint64), ident) and got[6, 7] == REFUSED_BAD
    assert np.array_equal(got[7, :7].view(np.uint64), ident) and got[7, 7] == OK           # pnum < 4 comes first


def test_fv_pair():
    srm = importlib.import_module("3pre_amd.sr4000")
    assert [srm.fv_pair(s) for s in (1, 2, 3, 4, 100)] == [None, None, (1, 2), (2, 3), (98, 99)]


def test_ekf_prediction_frames_follows_fv_pair():
    """the dispatch of fv.m:41-48, with a stand-in for the filter: no device"""
    srm = importlib.import_module("3pre_amd.sr4000")

    class Filt:
        def __init__(self):
            self.calls = []

        def ekf_prediction(self, u):
            self.calls.append(("identity", list(u)))

        def ekf_prediction_pair_seeded(self, prev, cur, seed, seq, thresh, wait):
            self.calls.append(("pair", prev, cur, seed, seq, thresh, wait))
            return "result"

    f = Filt()
    frames = {k: "frame%d" % k for k in range(1, 6)}
    assert srm.ekf_prediction_frames(f, 2, frames, 9) is None
    assert srm.ekf_prediction_frames(f, 3, frames, 9, seq=3, wait=False) == "result"
    assert srm.ekf_prediction_frames(f, 5, frames, 9) == "result"
    assert f.calls == [("identity", [0, 0, 0, 1, 0, 0, 0]), ("pair", "frame1", "frame2", 9, 3, 1.5, False), ("pair", "frame3", "frame4", 9, 0, 1.5, True)]


def test_null_arguments_and_one_handle_twice_are_refused_before_a_device_is_touched(pre3):
    """these return on the first checks, with or without a HIP device; the non-null arguments are never dereferenced on the way"""
    lib = importlib.import_module("3pre_amd._lib").lib
    vo = importlib.import_module("3pre_amd.vo")
    res, pnum = vo.VoResult(), C.c_int32(7)
    block = (C.c_char * 64)()                           # stands for a context / a handle: an address that is not null
    a, b = C.addressof(block), C.addressof(block) + 32
    assert lib.pre3_predict_pair_seeded(None, a, b, 1.5, 5, 0, C.byref(pnum), C.byref(res)) == -1
    assert b"null context" in lib.pre3_last_error()
    for prev, cur in ((None, b), (a, None), (None, None)):
        assert lib.pre3_predict_pair_seeded(a, prev, cur, 1.5, 5, 0, None, None) == -1
        assert b"null handle" in lib.pre3_last_error()
    assert lib.pre3_predict_pair_seeded(a, b, b, 1.5, 5, 0, C.byref(pnum), C.byref(res)) == -1
    assert b"same handle" in lib.pre3_last_error() and SYMBOL.encode() in lib.pre3_last_error()
    assert pnum.value == 7 and bytes(block) == b"\0" * 64


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_the_gateway_with_predict_pair_passes_the_compiler_front_end():
    r = subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-Wextra", "-Werror=implicit-function-declaration", "-Werror=incompatible-pointer-types",
                        "-Werror=int-conversion", "-I", os.path.join(ROOT, "tests", "mex_api_decl"), "-I", os.path.join(ROOT, "include"), MEX_SRC],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]


def test_predict_pair_is_dispatched_to_its_entry_point():
    txt = open(MEX_SRC).read()
    m = re.search(r'strcmp\(cmd, "predict_pair"\)\) \{(.*?)\n    \}', txt, re.S)
    assert m, "pre3_mex('predict_pair') is not dispatched"
    assert SYMBOL + "(g_ctx, g_sr_prev, g_sr" in m.group(1)
    assert "pre3_mex('predict_pair'" in txt[:txt.index("#include")]            # and listed in the table of the file's header comment
