"""CPU: the numpy restatement of sift_vedal (tests/sift_ref.py) against independent forms, the arithmetic of 3pre_amd/csrc/pre3_sift.h built for the
host (tests/sift_host_main.cpp) against the restatement, pre3_sift_plan_get against math.exp-made taps, the decision margins of the committed test
images, the tolerance file, and the new symbols.

Bit for bit: the plan, every Gaussian level (so doubleSize in both forms, the tap sums, halveSize), the counts, the refined points and their order.
Within tests/golden/sift_tolerance.json: sigma, theta, the descriptors."""
import importlib
import json
import math
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

import sift_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
CASES = (((69, 85), True), ((144, 176), True), ((37, 45), False))
_REF = {}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def reference(shape, strict):
    """the restatement's result for a committed image, computed once and shared (read-only)"""
    key = (tuple(shape), bool(strict))
    if key not in _REF:
        m = {}
        _REF[key] = (R.sift_vedal(R.make_image(*shape), strict, margins=m), m)
    return _REF[key]


def tolerance():
    with open(os.path.join(ROOT, "tests", "golden", "sift_tolerance.json")) as fh:
        return json.load(fh)


def test_smoothing_against_a_dense_edge_continued_operator():
    rng = np.random.default_rng(0)
    I = np.asfortranarray(rng.random((18, 22)) * 255)                  # narrower than the filter: W = 13
    lev = R.taps(R.plan(144, 176)["lev"][0][5][0])
    assert lev[1] == 13

    def op(n):
        T = np.zeros((n, n))
        for i in range(n):
            for t, g in enumerate(lev[2]):
                T[i, min(max(i - lev[1] + t, 0), n - 1)] += g
        return T
    want = op(18) @ I @ op(22).T
    assert np.abs(R.imsmooth(I, lev) - want).max() <= 1e-12


def test_extrema_against_a_maximum_filter():
    ref, _ = reference((69, 85), True)
    D = ref["dogss"][0]
    M, N, L = D.shape
    stack = np.stack([D[1 + dy:M - 1 + dy, 1 + dx:N - 1 + dx, 1 + ds:L - 1 + ds] for ds in (-1, 0, 1) for dx in (-1, 0, 1) for dy in (-1, 0, 1)])
    v = D[1:-1, 1:-1, 1:-1]
    strict_max = (stack.max(0) == v) & ((stack == v).sum(0) == 1) & (v >= 0.8 * R.THRESH)
    y, x, s = np.nonzero(strict_max)
    assert np.array_equal(np.sort((y + 1) + (x + 1) * M + (s + 1) * M * N), R.siftlocalmax(D, 0.8 * R.THRESH))
    assert len(y) > 20


def test_elimination_against_numpy_solve():
    rng = np.random.default_rng(1)
    for _ in range(20):
        Q = rng.standard_normal((3, 3))
        H = -(Q @ Q.T + 3 * np.eye(3)) * 0.1                          # a maximum; isotropic enough to pass the edge test
        H[0, 1] = H[1, 0] = 0.2 * H[0, 1]
        off = rng.uniform(-0.4, 0.4, 3)                               # (x, y, s)
        g = np.indices((9, 9, 5)).astype(np.float64)                  # D[y, x, s]
        d = np.stack([g[1] - 4 - off[0], g[0] - 4 - off[1], g[2] - 2 - off[2]])
        D = np.asfortranarray(5.0 + 0.5 * np.einsum("i...,ij,j...->...", d, H, d))
        got = R.refine_one(D, 4, 4, 2)
        grad = H @ (-off)                                             # at the centre sample
        want = np.linalg.solve(H, -grad)
        assert got is not None
        assert np.allclose([got[0] - 4, got[1] - 4, got[2] - R.SMIN - 2], want, rtol=0, atol=1e-9)


@pytest.mark.parametrize("shape,strict", CASES)
def test_descriptors_are_unit_vectors_clipped_once(shape, strict):
    ref, _ = reference(shape, strict)
    d = ref["descriptors"]
    assert d.shape[1] == ref["counts"][:, 3].sum() > 0
    assert np.all(d >= 0)
    nrm = np.sqrt((d * d).sum(0))
    assert np.all(np.abs(nrm[nrm > 0] - 1) < 1e-5)
    c = np.sqrt(np.minimum(1.0, 0.04 / np.maximum(d.max(0), 1e-30) ** 2))      # ||clipped||, if anything was clipped
    assert np.all(d.max(0) <= 0.2 / np.maximum(c, 0.2) * (1 + 1e-5))


@pytest.mark.parametrize("shape,strict", CASES)
def test_decision_margins_of_the_committed_images(shape, strict):
    ref, m = reference(shape, strict)
    assert set(m) == {"orient_W", "orient_bin", "peak", "desc_W"}
    for k, v in m.items():
        assert v >= 1e-9, (k, v)


def test_the_shapes_exercise_what_they_are_meant_to():
    ref, _ = reference((69, 85), True)
    assert [g.shape[:2] for g in ref["gss"]] == [(138, 170), (69, 85), (35, 43), (18, 22)]
    assert np.all(ref["counts"][:3, 1] > 0)                            # keypoints survive the boundary discard in octaves 0-2
    assert 2 * ref["plan"]["lev"][3][5][1] + 1 > 22                    # the last octave is narrower than its filter
    assert np.any(np.concatenate(ref["npeaks"]) > 1)                   # some keypoint has two orientations
    ref, _ = reference((144, 176), True)
    assert len(ref["gss"]) == 5


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("sift_host") / "sift_host"
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "3pre_amd", "csrc"),
                           os.path.join(ROOT, "tests", "sift_host_main.cpp"), "-o", str(exe), "-lm"])
    return str(exe)


def run_host(exe, I, strict, d):
    M, N = I.shape
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    with open(fin, "wb") as fh:
        fh.write(struct.pack("<3i", M, N, int(strict)) + np.asfortranarray(I).tobytes(order="F"))
    subprocess.check_call([exe, fin, fout])
    b, p = open(fout, "rb").read(), 4
    O, = struct.unpack_from("<i", b, 0)
    gss = []
    for _ in range(O):
        m, n = struct.unpack_from("<2i", b, p)
        gss.append(np.frombuffer(b, np.float64, m * n * 6, p + 8).reshape((m, n, 6), order="F"))
        p += 8 + m * n * 48
    nc, = struct.unpack_from("<i", b, p)
    cand = np.frombuffer(b, np.float64, nc * 4, p + 4).reshape(nc, 4)
    p += 4 + nc * 32
    K, = struct.unpack_from("<i", b, p)
    fd = np.frombuffer(b, np.float64, K * 132, p + 4).reshape(K, 132)
    counts = np.frombuffer(b, np.int32, 4 * O, p + 4 + K * 132 * 8).reshape(O, 4)
    return dict(gss=gss, cand=cand, frames=fd[:, :4].T, descriptors=fd[:, 4:].T, counts=counts)


def compare(got, ref, tol, what=""):
    """frames (4, K) 0-based and descriptors (128, K) against the restatement: x, y bit for bit, sigma, theta and the descriptors within `tol`"""
    assert got["frames"].shape == ref["frames"].shape, what
    assert same_bits(got["frames"][:2], ref["frames"][:2]), what
    ds = (np.abs(got["frames"][2] - ref["frames"][2]) / ref["frames"][2]).max()
    dt = np.abs(got["frames"][3] - ref["frames"][3]).max()
    dd = np.abs(got["descriptors"] - ref["descriptors"]).max()
    print("%s sigma %.3g (tol %.3g) theta %.3g (tol %.3g) descriptors %.3g (tol %.3g)" % (what, ds, tol["tol_sigma_rel"], dt, tol["tol_theta"], dd,
                                                                                          tol["tol_des"]))
    assert ds <= tol["tol_sigma_rel"] and dt <= tol["tol_theta"] and dd <= tol["tol_des"], (what, ds, dt, dd)


@pytest.mark.parametrize("shape,strict", CASES)
def test_the_headers_functions_built_for_the_host(host_exe, tmp_path, shape, strict):
    ref, _ = reference(shape, strict)
    got = run_host(host_exe, R.make_image(*shape), strict, str(tmp_path))
    assert len(got["gss"]) == len(ref["gss"])
    for o, (a, b) in enumerate(zip(got["gss"], ref["gss"])):
        assert same_bits(a, b), "octave %d" % o
    assert np.array_equal(got["counts"], ref["counts"])
    want = np.concatenate([np.vstack([q, np.full((1, q.shape[1]), float(o))]) for o, q in enumerate(ref["refined"])], 1).T
    assert same_bits(got["cand"], want)
    compare(got, ref, tolerance(), "host %s" % (shape,))


def test_double_size_leaves_the_last_row_and_column_zero_and_saturates():
    I = np.asfortranarray(np.full((4, 5), 255.0))
    J = R.double_size(I, True)
    assert np.all(J[-1] == 0) and np.all(J[:, -1] == 0)
    assert J[1, 1] == 255.0 and J[1, 0] == 255.0                      # 4 x uint8(63.75) = 256 saturates; 2 x uint8(127.5) = 256 too
    assert R.double_size(I, False)[1, 1] == 255.0
    I[:] = 1.0
    assert R.double_size(I, True)[1, 1] == 0.0 and R.double_size(I, True)[1, 0] == 2.0      # uint8(0.25) = 0; uint8(0.5) = 1
    assert R.double_size(I, False)[1, 1] == 1.0


@pytest.mark.parametrize("shape", [c[0] for c in CASES])
def test_plan_get_against_taps_made_with_math_exp(shape):
    srm = importlib.import_module("3pre_amd.sr4000")
    got, want = srm.sift_plan(*shape), R.plan(*shape)
    assert got["O"] == want["O"] and list(got["rows"]) == want["rows"] and list(got["cols"]) == want["cols"]
    assert got["sigma0"] == want["sigma0"] and same_bits(got["pow2"], want["pow2"])
    for o in range(want["O"]):
        for l in range(R.NLEV):
            s, W, g = want["lev"][o][l]
            assert got["sigma"][o, l] == s and got["W"][o, l] == W
            assert same_bits(got["taps"][o, l, :len(g)], g) and not got["taps"][o, l, len(g):].any()
    assert want["O"] == int(math.floor(math.log2(min(shape)))) - 2


def test_plan_get_refuses_an_image_without_an_octave():
    srm = importlib.import_module("3pre_amd.sr4000")
    lib = importlib.import_module("3pre_amd._lib")
    with pytest.raises(lib.Pre3Error) as e:
        srm.sift_plan(7, 100)
    assert e.value.code == -1


def test_the_tolerance_file_is_reproduced_by_its_builder():
    """the settings exactly; the floors within a factor of two (they pass through numpy's vectorised float32 exp / sin / arctan2, whose last bits differ
    between builds and SIMD targets, and a floor is the largest of a few thousand such differences); every tolerance is factor x its floor"""
    import make_sift_tolerance
    got, want = make_sift_tolerance.measure(), tolerance()
    assert set(got) == set(want)
    for k in ("factor", "cases", "jitter_seed", "shuffle_seed"):
        assert got[k] == want[k], k
    assert want["factor"] == 16
    for k in ("theta", "sigma_rel", "des"):
        assert want["tol_" + k] == want["factor"] * want["floor_" + k]
        assert 0.5 * want["floor_" + k] <= got["floor_" + k] <= 2.0 * want["floor_" + k], (k, got["floor_" + k], want["floor_" + k])


def _rot_points():
    """refined points of octave 0 of the 69 x 85 image, moved onto a 1/64 grid (so that N - 1 - x is exact in float32 too), and the octave"""
    ref, _ = reference((69, 85), True)
    q = np.round(ref["refined"][0] * 64.0) / 64.0
    return ref["gss"][0], q, ref["plan"]["sigma0"]


def test_a_rotated_octave_turns_the_orientation_histogram_by_nine_bins():
    """siftormx on np.rot90 of an octave: the pixel (x, y) goes to (y, N - 1 - x), a gradient (gx, gy) to (gy, -gx), so every sample's angle is the
    original's minus pi / 2 and the 36-bin histogram moves by exactly nine bins -- an independent check of the angle convention, the window and the
    binning.  The histogram is compared BEFORE the smoother: siftormx.c:209-217 smooths in place, bin 35 reads the new bin 0, so the reference's
    own orientations are not equivariant (they move by up to 0.06 rad here).  Bound: the bins are sums of <= 1700 positive terms taken
    in another order, 1700 x 2^-53 relative to the largest bin."""
    G, q, sigma0 = _rot_points()
    Gr = np.asfortranarray(np.rot90(G, 1, axes=(0, 1)))
    N = G.shape[1]
    worst = 0.0
    for x, y, s in q.T:
        ha, hb = [], []
        R.orient_one(G, x, y, s, sigma0, raw=ha)
        R.orient_one(Gr, y, N - 1 - x, s, sigma0, raw=hb)
        ha, hb = np.array(ha), np.array(hb)
        assert ha.max() > 0 and np.abs(np.roll(ha, -5) - hb).max() > 1e-3 * ha.max()      # another shift is told apart
        worst = max(worst, np.abs(np.roll(ha, -9) - hb).max() / ha.max())
    print("orientation histograms of %d points under a quarter turn: %.3g (bound %.3g)" % (q.shape[1], worst, 1700 * 2.0 ** -53))
    assert q.shape[1] > 80 and worst <= 1700 * 2.0 ** -53


def test_a_rotated_octave_gives_the_same_or_the_permuted_descriptor():
    """siftdescriptor on np.rot90 of an octave.  With theta0 turned along (theta0 - pi / 2) the descriptor is the same; with theta0 kept, the patch is
    a quarter turn on in the keypoint's frame: (nx, ny) -> (ny, -nx) and theta0 - angle grows by pi / 2, so entry (t, bx, by) of Lowe's layout
    t + 8 (bx + 4 by) moves to ((t + 2) mod 8, by, 3 - bx).  This pins the bin layout and the sign of -angle + theta0 independently of the header."""
    G, q, sigma0 = _rot_points()
    Gr = np.asfortranarray(np.rot90(G, 1, axes=(0, 1)))
    N = G.shape[1]
    t, bx, by = np.meshgrid(np.arange(8), np.arange(4), np.arange(4), indexing="ij")
    src, dst = (t + 8 * (bx + 4 * by)).ravel(), (((t + 2) % 8) + 8 * (by + 4 * (3 - bx))).ravel()
    tol, same, perm = tolerance()["tol_des"], 0.0, 0.0
    th0 = np.float64(np.float32(0.7))                                  # exact in float32, so that the turned angle is the only new rounding
    for x, y, s in q.T[:40]:
        d = R.descriptor_one(G, x, y, s, th0, sigma0)
        assert d.max() > 0.05
        same = max(same, np.abs(R.descriptor_one(Gr, y, N - 1 - x, s, th0 - np.pi / 2 + R.TWO_PI, sigma0) - d).max())
        p = np.zeros(128)
        p[dst] = d[src]
        perm = max(perm, np.abs(R.descriptor_one(Gr, y, N - 1 - x, s, th0, sigma0) - p).max())
        assert np.abs(p - d).max() > 1e-2                              # the permutation is not the identity on this descriptor
    print("descriptors under a quarter turn: same %.3g, permuted %.3g (tol %.3g)" % (same, perm, tol))
    assert same <= tol and perm <= tol


def test_new_symbols_are_declared_and_exported():
    lib = importlib.import_module("3pre_amd._lib")
    header = open(os.path.join(ROOT, "include", "pre3.h")).read()
    for name in ("pre3_sift_plan_get", "pre3_sr_frame_sift", "pre3_sr_frame_gate", "pre3_sr_frame_sift_level", "pre3_sr_frame_sift_refined"):
        assert "PRE3_API int %s(" % name in header and name in lib.EXPORTS
        assert getattr(lib.lib, name) is not None


def test_without_a_device_the_new_calls_report_it():
    lib = importlib.import_module("3pre_amd._lib")
    srm = importlib.import_module("3pre_amd.sr4000")
    if lib.device_count() > 0:
        return                                                         # with a device the calls are tests/test_gpu_sift.py's
    with pytest.raises(lib.Pre3Error) as e:
        srm.sift_vedal(R.make_image(37, 45), 0)
    assert e.value.code == -2
