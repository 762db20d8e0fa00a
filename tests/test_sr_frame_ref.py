"""CPU: the SR4000 frame conditioning.  The numpy restatement tests/sr_frame_ref.py (a) against its independent form (b) --
scipy's correlate and the line-by-line keypoint loops; the library's Gaussian weights against the closed form; MATLAB's round and uint8 at their
edges; pre3_sr.h compiled for the host against the restatement, bit for bit; the symbols declared and exported; load_dat round trips.

Bounds.  (a) and (b) add the same nine products in different orders: each sum carries at most 8 roundings of relative size 2^-53 of the running sum,
which never exceeds S = sum_k w_k |p_k|, so two orders differ by less than 16 * 2^-53 * S = 1.8e-15 S in the worst case and a few 1e-16 S in
practice; the bound is the issue's 1e-15, taken relative to S (relative to the pixel itself it would be unbounded where x or y cancel to zero).
The weights: exp is within 1 ulp in both libms, the sum and the quotient add one rounding each: 4 ulp."""
import ctypes as C
import importlib
import math
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import sr_frame_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.220446049250313e-16
PLANE_RTOL = 1e-15
SYMBOLS = ("pre3_sr_gauss3", "pre3_sr_frame_create", "pre3_sr_frame_destroy", "pre3_sr_frame_load", "pre3_sr_frame_get", "pre3_sr_frame_keypoints")


def same_bits(a, b):
    """equal NaN sets, every other entry bit-equal (a NaN's sign and payload are not part of MATLAB's value)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64)))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", [(1, 1), (3, 3), (17, 70), (144, 176)])
def test_restatement_agrees_with_the_independent_form(shape, mode):
    w = sr.gauss3(2.0 if mode == 0 else 1.0)
    fr = sr.make_frame(*shape)
    a, b = sr.condition(fr, mode, w), sr.condition(fr, mode, w, filt=sr.filter_scipy)
    for k in ("x", "y", "z"):
        S = sr.filter9(np.abs(fr[k]), w, mode)
        rel = (np.abs(a[k] - b[k]) / S).max()
        print(shape, mode, k, "max |a - b| / S = %.3g" % rel)
        assert rel < PLANE_RTOL, (k, rel)
    # the image: the sums agree to the same bound; an input condition keeps them off the rounding edges, so the uint8 values agree exactly
    u = sr.normalise(fr["amp"], a["imax"])
    sa, sb = sr.filter9(u, w, mode), sr.filter_scipy(u, w, mode)
    assert (np.abs(sa - sb) / np.maximum(sr.filter9(np.abs(u), w, mode), 1e-300)).max() < PLANE_RTOL
    assert np.abs(sa - np.floor(sa) - 0.5).min() > 1e-9
    assert np.array_equal(a["img"], b["img"]) and a["img"].min() >= 0 and a["img"].max() <= 255
    assert (a["imax"], a["cmax"]) == (b["imax"], b["cmax"])
    if shape[0] < 3:
        return
    K = 300
    frm, des = sr.make_keypoints(K, shape[0], shape[1], seed=mode)
    if shape == (144, 176):
        fr = sr.make_keypoint_frame(w, mode)
        a = sr.condition(fr, mode, w)
    g0, l0 = sr.keypoints(a, frm, des, 0), sr.depth_gate_loop(a, frm, des)
    g1, l1 = sr.keypoints(a, frm, des, 1), sr.confidence_filtering_loop(a, frm, des)
    for g, l in ((g0, l0), (g1, l1)):
        assert np.array_equal(g["keep_idx"], l["keep_idx"])
        assert np.array_equal(g["frames"], l["frames"]) and np.array_equal(g["descriptors"], l["descriptors"])
    assert 0 < len(g0["keep_idx"]) < K and 0 < len(g1["keep_idx"]) < K
    assert same_bits(g0["xyz"], l0["xyz"])
    ok = ~np.isnan(g0["rho"])
    assert np.array_equal(ok, ~np.isnan(l0["rho"])) and np.abs(g0["rho"][ok] / l0["rho"][ok] - 1).max() < 4 * EPS      # 1 / df against 1 / norm (nrm2)
    if shape == (144, 176):
        # the planted pixels do what they were planted for (keypoints 0 .. 20: seven pixels, three positions each)
        k0, k1 = set(g0["keep_idx"].tolist()), set(g1["keep_idx"].tolist())
        assert a["conf"][sr.PX_CONF_EQ] == 0.5 * a["cmax"] and not k0 & {0, 1, 2} and {0, 1, 2} <= k1      # <= drops, < keeps
        assert a["z"][sr.PX_R04] == 0.4 and {3, 4, 5} <= k0                                                # a range of exactly 0.4 is kept
        assert a["z"][sr.PX_RBELOW] == np.nextafter(0.4, 0) and not k0 & {6, 7, 8}
        assert np.isnan(a["x"][sr.PX_NANX]) and not k0 & {9, 10, 11}
        assert np.isnan(a["y"][sr.PX_NANY]) and not np.isnan(a["x"][sr.PX_NANY]) and {12, 13, 14} <= k0    # a NaN y alone survives
        assert np.isnan(g0["rho"][g0["keep_idx"].tolist().index(12)])
        assert {15, 16, 17} <= k0 and not (k0 | k1) & {18, 19, 20}


def test_weights_against_the_closed_form(pre3):
    srm = importlib.import_module("3pre_amd.sr4000")
    for sigma in (1.0, 2.0, 0.7):
        w = srm.gauss3(sigma).T.ravel()
        ref = sr.gauss3(sigma)
        assert np.abs(w / ref - 1).max() <= 4 * EPS, np.abs(w / ref - 1).max()
        s = 0.0
        for v in w:
            s = s + v
        assert abs(s - 1) <= 2 * EPS and abs(math.fsum(w) - 1) <= 2 * EPS, (s - 1, math.fsum(w) - 1)
        G = w.reshape(3, 3)
        assert np.array_equal(G, G.T) and G[1, 1] == w.max() and w[0] == w[2] == w[6] == w[8] and w[1] == w[3] == w[5] == w[7]
        assert w.min() > EPS * w.max()                               # fspecial's eps * max branch never fires
    lib = pre3._lib.lib
    buf = np.zeros(9)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.pre3_sr_gauss3(bad, pre3._lib.dptr(buf)) == -1
    assert lib.pre3_sr_gauss3(1.0, None) == -1


def test_matlab_round_and_uint8_at_their_edges():
    v = np.array([0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 254.5, 255.5, -0.4, 0.49999999999999994, 143.49999999999997, 300.0, -7.0, np.nan])
    r = sr.matlab_round(v)
    assert r[:-1].tolist() == [1, -1, 2, -2, 3, -3, 255, 256, 0, 0, 143, 300, -7] and np.isnan(r[-1])
    assert round(2.5) == 2                                          # (Python's round is not MATLAB's)
    u = sr.matlab_uint8(v)
    assert u.tolist() == [1, 0, 2, 0, 3, 0, 255, 255, 0, 0, 143, 255, 0, 0]
    assert not np.signbit(u).any()
    assert [sr._round1(x) for x in v[:-1]] == r[:-1].tolist()


HOST_PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "pre3_sr.h"
using namespace pre3;
// stdin: int32 rows, cols, mode, has_conf, K, P | w[9] | z, x, y, amp, (conf) column-major | u[K], v[K] | probes[P]
// stdout: x, y, z, img | imax, cmax | keep0[K], keep1[K], xyz[3K], rho[K] | round[P], uint8[P]
static bool rd(void *p, size_t n) { return fread(p, 8, n, stdin) == n; }
int main()
{
    int32_t h[6];
    if (fread(h, 4, 6, stdin) != 6) return 2;
    const int rows = h[0], cols = h[1], mode = h[2], has_conf = h[3], K = h[4], P = h[5];
    const size_t n = (size_t)rows * cols;
    double w[9];
    std::vector<double> raw(5 * n), kp(2 * (size_t)K), pr(P), out;
    if (!rd(w, 9) || !rd(raw.data(), (has_conf ? 5 : 4) * n) || !rd(kp.data(), 2 * (size_t)K) || !rd(pr.data(), P)) return 3;
    const double *Z = raw.data(), *X = Z + n, *Y = X + n, *A = Y + n, *Cf = A + n;
    double imax = 0.0, cmax = NAN;
    for (size_t i = 0; i < n; ++i) { if (A[i] <= SR_SATURATED && A[i] > imax) imax = A[i]; if (has_conf) cmax = sr_nanmax(cmax, Cf[i]); }
    std::vector<double> f(4 * n);
    for (int c = 0; c < cols; ++c) for (int r = 0; r < rows; ++r)
        for (int pl = 0; pl < 4; ++pl) {
            double p[9];
            for (int dj = 0; dj < 3; ++dj) for (int di = 0; di < 3; ++di) {
                int gr = r + di - 1, gc = c + dj - 1;
                const bool in = gr >= 0 && gr < rows && gc >= 0 && gc < cols;
                double v = 0.0;
                if (in || mode == 1) {
                    gr = gr < 0 ? 0 : (gr >= rows ? rows - 1 : gr); gc = gc < 0 ? 0 : (gc >= cols ? cols - 1 : gc);
                    const size_t g = (size_t)gc * rows + gr;
                    v = pl == 0 ? X[g] : (pl == 1 ? Y[g] : (pl == 2 ? Z[g] : sr_norm_pixel(A[g], imax)));
                }
                p[3 * dj + di] = v;
            }
            const double s = sr_tap9(w, p);
            f[pl * n + (size_t)c * rows + r] = pl == 3 ? matlab_uint8(s) : s;
        }
    out = f;
    out.push_back(imax); out.push_back(cmax);
    std::vector<double> k0(K), k1(K), xyz(3 * (size_t)K), rho(K);
    for (int k = 0; k < K; ++k) {
        const int r = (int)matlab_round(kp[K + k]) - 1, c = (int)matlab_round(kp[k]) - 1;
        const size_t g = (size_t)c * rows + r;
        const double xf = f[g], yf = f[n + g], zf = f[2 * n + g], df = sr_range(xf, yf, zf);
        k0[k] = sr_gate_depth(xf, df, has_conf != 0, has_conf ? Cf[g] : 0.0, cmax) ? 1.0 : 0.0;
        k1[k] = has_conf && sr_gate_confidence(Cf[g], cmax) ? 1.0 : 0.0;
        xyz[3 * k] = -xf; xyz[3 * k + 1] = -yf; xyz[3 * k + 2] = zf; rho[k] = 1.0 / df;
    }
    out.insert(out.end(), k0.begin(), k0.end()); out.insert(out.end(), k1.begin(), k1.end());
    out.insert(out.end(), xyz.begin(), xyz.end()); out.insert(out.end(), rho.begin(), rho.end());
    for (int i = 0; i < P; ++i) out.push_back(matlab_round(pr[i]));
    for (int i = 0; i < P; ++i) out.push_back(matlab_uint8(pr[i]));
    return fwrite(out.data(), 8, out.size(), stdout) == out.size() ? 0 : 4;
}
"""


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("sr_host")
    src, exe = d / "sr_host.cpp", d / "sr_host"
    src.write_text(HOST_PROGRAM)
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "3pre_amd", "csrc"),
                           str(src), "-o", str(exe), "-lm"])
    return str(exe)


@pytest.mark.parametrize("conf", [True, False])
@pytest.mark.parametrize("mode", [0, 1])
def test_the_headers_functions_built_for_the_host(host_exe, mode, conf):
    rows, cols, K = 17, 70, 300
    w = sr.gauss3(2.0 if mode == 0 else 1.0)
    fr = sr.make_frame(rows, cols, seed=3, conf=conf)
    fr["x"][3, 50] = np.nan; fr["y"][12, 20] = np.nan; fr["z"][0, 0] = np.nan; fr["x"][16, 69] = -0.0
    if conf:
        fr["conf"][8, 40] = 0.5 * sr.CMAX; fr["conf"][2, 2] = np.nan
    frm, des = sr.make_keypoints(K, rows, cols, seed=mode)
    for i, (r, c) in enumerate(((3, 50), (12, 20), (8, 40), (2, 2), (0, 0), (16, 69))):
        frm[0, 2 * i], frm[1, 2 * i] = c + 1.0, r + 1.0
        frm[0, 2 * i + 1], frm[1, 2 * i + 1] = c + 0.5, r + 0.5
    probes = np.array([0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 254.5, 255.5, -0.4, 0.49999999999999994, 300.0, -7.0, np.nan])
    planes = [fr[k] for k in ("z", "x", "y", "amp")] + ([fr["conf"]] if conf else [])
    inp = struct.pack("<6i", rows, cols, mode, int(conf), K, len(probes)) + w.tobytes() + b"".join(p.tobytes(order="F") for p in planes) \
        + np.ascontiguousarray(frm[0]).tobytes() + np.ascontiguousarray(frm[1]).tobytes() + probes.tobytes()
    got = np.frombuffer(subprocess.run([host_exe], input=inp, stdout=subprocess.PIPE, check=True).stdout, np.float64)
    n = rows * cols
    ref = sr.condition(fr, mode, w)
    assert got.size == 4 * n + 2 + 6 * K + 2 * len(probes)
    for i, k in enumerate(("x", "y", "z", "img")):
        assert same_bits(got[i * n:(i + 1) * n].reshape(rows, cols, order="F"), ref[k]), k
    assert np.isnan(ref["x"]).sum() == 9 and np.isnan(ref["z"]).sum() == 4
    assert got[4 * n] == ref["imax"] and (got[4 * n + 1] == ref["cmax"] if conf else np.isnan(got[4 * n + 1]))
    o = 4 * n + 2
    k0, k1, xyz, rho = got[o:o + K] == 1.0, got[o + K:o + 2 * K] == 1.0, got[o + 2 * K:o + 5 * K].reshape(K, 3).T, got[o + 5 * K:o + 6 * K]
    r0 = sr.keypoints(ref, frm, des, 0)
    assert np.array_equal(np.flatnonzero(k0), r0["keep_idx"]) and 0 < k0.sum() < K
    assert same_bits(xyz[:, k0], r0["xyz"]) and same_bits(rho[k0], r0["rho"])
    if conf:
        assert np.array_equal(np.flatnonzero(k1), sr.keypoints(ref, frm, des, 1)["keep_idx"]) and 0 < k1.sum() < K
        assert not k0[4] and not k0[5] and k1[4] and k1[5]            # the pixel at exactly half the largest confidence
    o += 6 * K
    assert same_bits(got[o:o + len(probes)], sr.matlab_round(probes)) and same_bits(got[o + len(probes):], sr.matlab_uint8(probes))


def test_the_symbols_are_declared_and_exported(pre3):
    txt = open(os.path.join(ROOT, "include", "pre3.h")).read()
    declared = set(re.findall(r"PRE3_API\s+[\w\s\*]+?\b(pre3_\w+)\s*\(", txt))
    lib = C.CDLL(pre3.LIB_PATH)
    for name in SYMBOLS:
        assert name in declared, "include/pre3.h does not declare %s" % name
        assert hasattr(lib, name), "libpre3.so does not export %s" % name
    assert re.search(r"#define\s+PRE3_SR_MAX_KEYPOINTS\s+8192\b", txt) and "typedef struct pre3_sr_frame pre3_sr_frame;" in txt
    srm = importlib.import_module("3pre_amd.sr4000")
    assert pre3.sr4000 is srm and pre3.SrFrame is srm.SrFrame
    for name in ("load_dat", "SrFrame", "read_xyz_sr4000", "read_image_sr4000", "read_sr4000_data_dr_ye", "confidence_filtering", "sift_extract"):
        assert hasattr(srm, name), name
    internal = open(os.path.join(ROOT, "3pre_amd", "csrc", "pre3_internal.h")).read()
    assert "sr_frame_view" in internal


def test_without_a_device_the_handle_fails_loudly(pre3):
    if pre3.device_count() > 0:
        pytest.skip("a HIP device is present")
    with pytest.raises(pre3.Pre3Error) as e:
        pre3.SrFrame()
    assert e.value.code == -2 and "no CPU fallback" in str(e.value)
    with pytest.raises(pre3.Pre3Error) as e:
        pre3.SrFrame(0, 5)
    assert e.value.code == -1                                        # argument errors come first


@pytest.mark.parametrize("n_rows", [721, 720, 576])
def test_load_dat_round_trip(pre3, tmp_path, n_rows):
    fr = sr.make_frame(144, 176, seed=n_rows)
    a = np.vstack([fr[k] for k in ("z", "x", "y", "amp", "conf")])
    if n_rows == 721:
        a = np.vstack([a, np.r_[1234567.25, np.zeros(175)]])
    a = a[:n_rows]
    path = tmp_path / ("d1_%04d.dat" % 7)
    np.savetxt(path, a, fmt="%.17g")
    d = pre3.load_dat(str(path))
    for k in ("z", "x", "y", "amp"):
        assert d[k].shape == (144, 176) and d[k].flags.f_contiguous and np.array_equal(d[k], fr[k])
    if n_rows >= 720:
        assert np.array_equal(d["conf"], fr["conf"])
    else:
        assert d["conf"] is None
    assert d["timestamp"] == (1234567.25 if n_rows == 721 else -1.0)
    short = tmp_path / "short.dat"
    np.savetxt(short, a[:100], fmt="%.17g")
    with pytest.raises(ValueError):
        pre3.load_dat(str(short))
