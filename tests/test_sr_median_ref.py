"""CPU: the 3 x 3 median and the bad-pixel compensation in front of the frame's Gaussian.  The numpy statement
tests/sr_median_ref.py (a) against scipy's median_filter (b); pre3_sr.h compiled for the host into a stand-alone program -- sr_median9 on all 512
zero/one windows (the 0-1 principle: a compare-exchange network that selects the fifth smallest of every 0/1 input does so for every input), on seeded
windows with repeated values and with NaNs, the predicate at its edge, and a whole 17 x 70 frame through the compensated conditioning against (a); the
symbols declared and exported.

There are no tolerances: a median is a selection and the Gaussian behind it is the arithmetic section 20 pins bit for bit.  Equal means equal as values
(-0 equals +0) with NaNs in the same places."""
import ctypes as C
import importlib
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import sr_frame_ref as sr
import sr_median_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pre3_sr_frame_set_compensation", "pre3_sr_frame_get_compensation", "pre3_sr_frame_bad_pixels", "pre3_sr_medfilt3")


def test_the_symbols_are_declared_and_exported(pre3):
    txt = open(os.path.join(ROOT, "include", "pre3.h")).read()
    declared = set(re.findall(r"PRE3_API\s+[\w\s\*]+?\b(pre3_\w+)\s*\(", txt))
    lib = C.CDLL(pre3.LIB_PATH)
    for name in SYMBOLS:
        assert name in declared, "include/pre3.h does not declare %s" % name
        assert hasattr(lib, name), "libpre3.so does not export %s" % name
        assert name in pre3._lib.EXPORTS
    for name, value in (("PRE3_SR_COMP_NONE", 0), ("PRE3_SR_COMP_BADPIXEL", 1), ("PRE3_SR_COMP_IMAGE_MEDIAN", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), txt), name
    srm = importlib.import_module("3pre_amd.sr4000")
    assert (srm.COMP_NONE, srm.COMP_BADPIXEL, srm.COMP_IMAGE_MEDIAN) == (0, 1, 2)
    for name in ("medfilt2", "compensate_badpixel_soonhac", "read_image_sr4000_dr_ye"):
        assert hasattr(srm, name), name
    for name in ("set_compensation", "compensation", "bad_pixels"):
        assert hasattr(srm.SrFrame, name), name
    # host only: the setter's null-handle check needs no device
    assert lib.pre3_sr_frame_set_compensation(None, 0, C.c_double(1.0)) == -1
    assert lib.pre3_sr_medfilt3(0, 3, 3, None, 0, None) == -1


def test_the_mex_gateway_has_the_three_commands():
    """source only (tests/test_mex_syntax.py puts the file through the compiler's front end): the commands are there and call the entry points"""
    txt = open(os.path.join(ROOT, "mex", "ekf_ctx_gateway.c")).read()
    for cmd, entry in (("sr_compensation", "pre3_sr_frame_set_compensation"), ("sr_bad_pixels", "pre3_sr_frame_bad_pixels"), ("medfilt3", "pre3_sr_medfilt3")):
        at = txt.index('!strcmp(cmd, "%s")' % cmd)
        assert entry + "(" in txt[at:txt.index("return;", at)], cmd


@pytest.mark.parametrize("padding", ["symmetric", "zeros"])
@pytest.mark.parametrize("shape", mr.SIZES + ((144, 176),))
def test_the_numpy_statement_agrees_with_scipy(shape, padding):
    rng = np.random.default_rng(100 * shape[0] + shape[1])
    for a in (rng.normal(0.0, 3.0, shape), np.floor(rng.uniform(0, 256, shape)), np.floor(rng.uniform(0, 4, shape))):
        got, ref = mr.medfilt3(a, padding), mr.medfilt3_scipy(a, padding)
        assert not np.isnan(got).any() and np.array_equal(got, ref)
    if padding == "symmetric":                                # a 1-row or 1-column image mirrors onto itself
        one = np.array([[5.0]])
        assert mr.medfilt3(one, "symmetric")[0, 0] == 5.0 and mr.medfilt3(one, "zeros")[0, 0] == 0.0


def test_the_planted_frame_is_what_the_gpu_suite_needs():
    w = sr.gauss3(1.0)
    fr, n_bad = mr.planted_frame(17, 70, seed=1)
    bad, block, at_cutoff, nan_conf = mr.planted_pixels(17, 70)
    mask = mr.bad_mask(fr["conf"], mr.CUTOFF, (17, 70))
    assert n_bad == len(bad) == int(mask.sum()) and len(block) == 4 and all(mask[p] for p in block)
    assert fr["conf"][at_cutoff] == mr.CUTOFF and not mask[at_cutoff] and np.isnan(fr["conf"][nan_conf]) and not mask[nan_conf]
    for p in ((0, 0), (0, 69), (16, 0), (16, 69), (15, 3), (16, 35), (3, 15), (3, 16), (3, 17), (15, 15), (16, 16)):
        assert mask[p], p
    # every median is taken on the plane as loaded: in the 2 x 2 block the result differs from a sequential replacement
    for k in ("x", "y", "z"):
        a, s = mr.compensate(fr[k], fr["conf"], mr.CUTOFF), mr.compensate_sequential(fr[k], fr["conf"], mr.CUTOFF)
        assert any(a[p] != s[p] for p in block), k
        assert a[at_cutoff] == fr[k][at_cutoff] and a[nan_conf] == fr[k][nan_conf]
    ref = mr.condition(fr, 1, w, mr.BADPIXEL)
    none = mr.condition(fr, 1, w, mr.NONE)
    assert ref["n_bad"] == n_bad and none["n_bad"] == 0 and not mr.same(ref["z"], none["z"]) and not mr.same(ref["img"], none["img"])
    assert sr.condition(fr, 1, w)["z"].tobytes() == none["z"].tobytes()
    assert not mr.same(mr.condition(fr, 0, w, mr.IMAGE_MEDIAN)["img"], none["img"])


HOST_PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "pre3_sr.h"
using namespace pre3;
// stdin: int32 op, then
//   op 0: int32 N | p[9 N]                                        -> sr_median9 of each window
//   op 1: int32 N | (conf, cutoff, has_conf)[N]                   -> sr_is_bad as 0 / 1
//   op 2: int32 rows, cols, mode, has_conf, form | cutoff | w[9] | z, x, y, amp, (conf) column-major -> x, y, z, img | n_bad
//   op 3: int32 rows, cols, padding | A column-major              -> medfilt2(A, [3 3]) through sr_medfilt_pixel
static bool rd(void *p, size_t n) { return fread(p, 8, n, stdin) == n; }
static bool ri(int32_t *p, size_t n) { return fread(p, 4, n, stdin) == n; }
int main()
{
    int32_t op;
    if (!ri(&op, 1)) return 2;
    std::vector<double> out;
    if (op == 0 || op == 1) {
        int32_t N;
        if (!ri(&N, 1)) return 2;
        const int per = op == 0 ? 9 : 3;
        std::vector<double> in((size_t)per * N);
        if (!rd(in.data(), in.size())) return 3;
        for (int k = 0; k < N; ++k)
            out.push_back(op == 0 ? sr_median9(&in[9 * (size_t)k]) : (sr_is_bad(in[3 * (size_t)k + 2] != 0.0, in[3 * (size_t)k], in[3 * (size_t)k + 1]) ? 1.0 : 0.0));
    } else if (op == 3) {
        int32_t h[3];
        if (!ri(h, 3)) return 2;
        const int rows = h[0], cols = h[1];
        std::vector<double> A((size_t)rows * cols);
        if (!rd(A.data(), A.size())) return 3;
        for (int c = 0; c < cols; ++c) for (int r = 0; r < rows; ++r) out.push_back(sr_medfilt_pixel(A.data(), rows, cols, r, c, h[2]));
    } else {
        int32_t h[5];
        if (!ri(h, 5)) return 2;
        const int rows = h[0], cols = h[1], mode = h[2], has_conf = h[3], form = h[4];
        const size_t n = (size_t)rows * cols;
        double cutoff, w[9];
        std::vector<double> raw(5 * n), U(n);
        if (!rd(&cutoff, 1) || !rd(w, 9) || !rd(raw.data(), (has_conf ? 5 : 4) * n)) return 3;
        const double *Z = raw.data(), *X = Z + n, *Y = X + n, *A = Y + n, *Cf = has_conf ? A + n : nullptr;
        double imax = 0.0, n_bad = 0.0;
        for (size_t i = 0; i < n; ++i) if (A[i] <= SR_SATURATED && A[i] > imax) imax = A[i];
        for (size_t i = 0; i < n; ++i) { U[i] = sr_norm_pixel(A[i], imax); if (form == SR_COMP_BADPIXEL && sr_is_bad(has_conf != 0, has_conf ? Cf[i] : 0.0, cutoff)) n_bad += 1.0; }
        out.resize(4 * n);
        for (int pl = 0; pl < 4; ++pl) {
            const double *P = pl == 0 ? X : (pl == 1 ? Y : (pl == 2 ? Z : U.data()));
            const int pform = (form == SR_COMP_IMAGE_MEDIAN && pl < 3) ? SR_COMP_NONE : form;      // form 2 leaves x, y, z as loaded
            for (int c = 0; c < cols; ++c) for (int r = 0; r < rows; ++r) {
                double p[9];
                for (int dj = 0; dj < 3; ++dj) for (int di = 0; di < 3; ++di) {
                    int gr = r + di - 1, gc = c + dj - 1;
                    const bool in = gr >= 0 && gr < rows && gc >= 0 && gc < cols;
                    double v = 0.0;
                    if (in || mode == 1) {
                        gr = gr < 0 ? 0 : (gr >= rows ? rows - 1 : gr); gc = gc < 0 ? 0 : (gc >= cols ? cols - 1 : gc);
                        v = sr_comp_pixel(P, Cf, rows, cols, gr, gc, pform, cutoff);
                    }
                    p[3 * dj + di] = v;
                }
                const double s = sr_tap9(w, p);
                out[pl * n + (size_t)c * rows + r] = pl == 3 ? matlab_uint8(s) : s;
            }
        }
        out.push_back(n_bad);
    }
    return fwrite(out.data(), 8, out.size(), stdout) == out.size() ? 0 : 4;
}
"""


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("sr_median_host")
    src, exe = d / "sr_median_host.cpp", d / "sr_median_host"
    src.write_text(HOST_PROGRAM)
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "3pre_amd", "csrc"),
                           str(src), "-o", str(exe), "-lm"])
    return str(exe)


def run(exe, head, *arrays):
    inp = head + b"".join(np.ascontiguousarray(a, dtype=np.float64).tobytes() for a in arrays)
    return np.frombuffer(subprocess.run([exe], input=inp, stdout=subprocess.PIPE, check=True).stdout, np.float64)


def median9_host(exe, windows):
    windows = np.ascontiguousarray(windows, dtype=np.float64)
    return run(exe, struct.pack("<2i", 0, len(windows)), windows)


def test_median9_on_all_512_zero_one_windows(host_exe):
    w = ((np.arange(512)[:, None] >> np.arange(9)) & 1).astype(np.float64)
    got = median9_host(host_exe, w)
    assert np.array_equal(got, (w.sum(1) >= 5).astype(np.float64))          # the fifth smallest of nine 0/1 values is 1 iff at least five are 1


def test_median9_on_seeded_windows_with_repeats_and_nans(host_exe):
    rng = np.random.default_rng(9)
    w = np.concatenate([rng.normal(0, 10, (2000, 9)), np.floor(rng.uniform(0, 4, (2000, 9))), np.floor(rng.uniform(0, 256, (2000, 9))),
                        np.tile(rng.normal(0, 1, (50, 1)), (1, 9)), rng.permuted(np.tile(np.r_[-np.inf, np.inf, 0.0, -0.0, 1.0, 1.0, 2.0, 2.0, 3.0], (200, 1)), axis=1)])
    assert np.array_equal(median9_host(host_exe, w), np.sort(w, axis=1)[:, 4])
    one = rng.normal(0, 1, (9, 9))
    one[np.arange(9), np.arange(9)] = np.nan                                 # one NaN, at each position of the window in turn
    assert np.isnan(median9_host(host_exe, one)).all()
    assert np.isnan(median9_host(host_exe, np.full((1, 9), np.nan))).all()
    few = rng.normal(0, 1, (100, 9))
    few[rng.random((100, 9)) < 0.3] = np.nan
    assert np.array_equal(np.isnan(median9_host(host_exe, few)), np.isnan(few).any(1))


def test_the_predicate_at_its_edge(host_exe):
    c = 7.25
    below, above = np.nextafter(c, 0.0), np.nextafter(c, 10.0)
    cases = np.array([[c, c, 1], [below, c, 1], [above, c, 1], [np.nan, c, 1], [-np.inf, c, 1], [below, c, 0], [-np.inf, c, 0], [0.0, 1.0, 1], [1.0, 1.0, 1]])
    got = run(host_exe, struct.pack("<2i", 1, len(cases)), cases)
    assert got.tolist() == [0, 1, 0, 0, 1, 0, 0, 1, 0]


@pytest.mark.parametrize("padding", ["zeros", "symmetric"])
@pytest.mark.parametrize("shape", mr.SIZES)
def test_the_headers_window_rule_built_for_the_host(host_exe, shape, padding):
    rng = np.random.default_rng(7 * shape[0] + shape[1])
    a = np.asfortranarray(rng.normal(0, 3, shape))
    if shape == (17, 70):
        for px in ((8, 30), (15, 16), (0, 40), (16, 69)):                   # interior, beside a tile boundary, on an edge, in a corner
            a[px] = np.nan
    got = run(host_exe, struct.pack("<4i", 3, shape[0], shape[1], {"zeros": 0, "symmetric": 1}[padding]), a.ravel(order="F"))
    assert mr.same(got.reshape(shape, order="F"), mr.medfilt3(a, padding))


@pytest.mark.parametrize("conf", [True, False])
@pytest.mark.parametrize("form", [mr.BADPIXEL, mr.IMAGE_MEDIAN])
@pytest.mark.parametrize("mode", [0, 1])
def test_a_whole_frame_through_the_host_compiled_compensation(host_exe, mode, form, conf):
    rows, cols = 17, 70
    w = sr.gauss3(2.0 if mode == 0 else 1.0)
    fr, n_bad = mr.planted_frame(rows, cols, seed=3)
    fr["x"][9, 33] = np.nan; fr["z"][0, 1] = np.nan; fr["y"][16, 68] = -0.0      # a NaN beside planted pixels: (8, 35)'s window misses it, (0, 0)'s holds z's
    if not conf:
        fr["conf"] = None
    planes = [fr[k] for k in ("z", "x", "y", "amp")] + ([fr["conf"]] if conf else [])
    got = run(host_exe, struct.pack("<6i", 2, rows, cols, mode, int(conf), form), np.array([mr.CUTOFF]), w, *[p.ravel(order="F") for p in planes])
    n = rows * cols
    ref = mr.condition(fr, mode, w, form)
    assert got.size == 4 * n + 1
    for i, k in enumerate(("x", "y", "z", "img")):
        assert mr.same(got[i * n:(i + 1) * n].reshape(rows, cols, order="F"), ref[k]), k
    assert got[4 * n] == ref["n_bad"] == (n_bad if conf and form == mr.BADPIXEL else 0)
    none = mr.condition(fr, mode, w, mr.NONE)
    if form == mr.BADPIXEL and not conf:                      # without a confidence map nothing is bad: the uncompensated frame
        for k in ("x", "y", "z", "img"):
            assert mr.same(ref[k], none[k]), k
    else:
        assert not mr.same(ref["img"], none["img"])
        assert mr.same(ref["z"], none["z"]) == (form == mr.IMAGE_MEDIAN)
