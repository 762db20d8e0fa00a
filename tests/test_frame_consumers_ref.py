"""CPU: the consumers of a resident SR4000 frame -- the plane fit, the heading update and the IC search's scan.  The new symbols
are declared, exported and mirrored; pre3_planecrop.h (the index arithmetic of k_plane_crop) compiled for the host against a numpy restatement of
plane_pack, bit for bit, with its non-finite flag; the argument errors that return before a device is touched."""
import ctypes as C
import importlib
import inspect
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from test_sr_frame_ref import same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pre3_plane_fit_frame", "pre3_plane_fit_frame_seeded", "pre3_heading_from_frame", "pre3_heading_from_frame_seeded", "pre3_set_scan_frame")
DEFAULT_BOX = (80, 144, 50, 120)
# (rows, cols), box: the smallest box the 40-row rule admits; an interior box that straddles row 16 and column 16; the reference's
CASES = [((41, 3), (1, 41, 1, 3)), ((48, 20), (3, 46, 2, 19)), ((144, 176), DEFAULT_BOX)]


def test_the_symbols_are_declared_exported_and_mirrored(pre3):
    txt = open(os.path.join(ROOT, "include", "pre3.h")).read()
    declared = set(re.findall(r"PRE3_API\s+[\w\s\*]+?\b(pre3_\w+)\s*\(", txt))
    lib = C.CDLL(pre3.LIB_PATH)
    _lib = importlib.import_module("3pre_amd._lib")
    for name in SYMBOLS:
        assert name in declared, "include/pre3.h does not declare %s" % name
        assert hasattr(lib, name), "libpre3.so does not export %s" % name
        assert name in _lib.EXPORTS and getattr(_lib.lib, name).argtypes is not None, name
    assert re.search(r"\b5 \(the \*_frame forms only\)", txt), "sta = 5 is documented in pre3_plane_result's comment"
    plane, ekf, srm = (importlib.import_module("3pre_amd." + m) for m in ("plane", "ekf", "sr4000"))

    def params(fn):
        return list(inspect.signature(fn).parameters)

    assert params(plane.plane_fit_frame) == ["frame", "draws", "box", "t"]
    assert params(plane.plane_fit_frame_seeded) == ["frame", "seed", "seq", "n_draw", "box", "t"]
    assert params(ekf.EkfFilter.heading_from_frame) == ["self", "frame", "draws", "box", "t", "transpose", "strict_reference", "wait"]
    assert params(ekf.EkfFilter.heading_from_frame_seeded) == ["self", "frame", "seed", "seq", "n_draw", "box", "t", "transpose", "strict_reference", "wait",
                                                               "return_draws"]
    assert params(ekf.EkfFilter.set_scan_frame) == ["self", "frame", "which"]
    assert params(srm.plane_fit_to_data)[:3] == ["frame", "seed", "seq"]
    assert pre3.plane_fit_frame is plane.plane_fit_frame and pre3.plane_fit_frame_seeded is plane.plane_fit_frame_seeded


HOST_PROGRAM = r"""
#include <cstdio>
#include <vector>
#include "pre3_planecrop.h"
using namespace pre3;
// stdin: int32 rows, cols, row0, row1, col0, col1 (the box, 1-based inclusive) | x, y, z column-major
// stdout: [X | Y | Z] of the box | the flag as a double
int main()
{
    int32_t h[6];
    if (fread(h, 4, 6, stdin) != 6) return 2;
    const size_t n = (size_t)h[0] * h[1];
    std::vector<double> p(3 * n);
    if (fread(p.data(), 8, 3 * n, stdin) != 3 * n) return 3;
    const PlaneCrop b{ h[0], h[2] - 1, h[4] - 1, h[3] - h[2] + 1, h[5] - h[4] + 1 };
    const int npts = b.nr * b.nc;
    std::vector<double> out(3 * (size_t)npts + 1, 7.0);
    int flag = 0;
    for (int k = npts - 1; k >= 0; --k) flag |= plane_crop_point(b, k, p.data(), p.data() + n, p.data() + 2 * n, out.data()) ? 1 : 0;
    out[3 * (size_t)npts] = flag;
    return fwrite(out.data(), 8, out.size(), stdout) == out.size() ? 0 : 4;
}
"""


@pytest.fixture(scope="module")
def crop_exe(tmp_path_factory):
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("crop_host")
    src, exe = d / "crop_host.cpp", d / "crop_host"
    src.write_text(HOST_PROGRAM)
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "3pre_amd", "csrc"), str(src), "-o", str(exe), "-lm"])
    return str(exe)


def plane_pack(x, y, z, box):
    """pre3_plane.hip's plane_pack restated: the box column-major, X = -x, Y = -y, Z = z, as [X | Y | Z]"""
    r0, r1, c0, c1 = box
    return np.concatenate([(-x[r0 - 1:r1, c0 - 1:c1]).ravel(order="F"), (-y[r0 - 1:r1, c0 - 1:c1]).ravel(order="F"), z[r0 - 1:r1, c0 - 1:c1].ravel(order="F")])


def run_crop(exe, x, y, z, box):
    rows, cols = x.shape
    inp = struct.pack("<6i", rows, cols, *box) + b"".join(np.asarray(p, np.float64).tobytes(order="F") for p in (x, y, z))
    got = np.frombuffer(subprocess.run([exe], input=inp, stdout=subprocess.PIPE, check=True).stdout, np.float64)
    return got[:-1], int(got[-1])


def planes(shape, seed):
    rng = np.random.default_rng(seed)
    x, y, z = (rng.normal(0, 2.0, shape) for _ in range(3))
    x[0, 0] = -0.0; y[-1, -1] = 0.0; z[shape[0] // 2, shape[1] // 2] = 5e-324      # signed zeros and a denormal keep their bits
    return x, y, z


@pytest.mark.parametrize("shape,box", CASES)
def test_the_crop_header_against_plane_pack(crop_exe, shape, box):
    x, y, z = planes(shape, shape[0])
    got, flag = run_crop(crop_exe, x, y, z, box)
    ref = plane_pack(x, y, z, box)
    assert got.size == ref.size == 3 * (box[1] - box[0] + 1) * (box[3] - box[2] + 1)
    assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)) and flag == 0


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("shape,box", CASES)
def test_the_flag_is_set_exactly_by_a_non_finite_point_of_the_box(crop_exe, shape, box, bad):
    r0, r1, c0, c1 = box
    rows, cols = shape
    inside = [(r0 - 1, c0 - 1), (r1 - 1, c1 - 1), ((r0 + r1) // 2 - 1, (c0 + c1) // 2 - 1), (r0 - 1, c1 - 1), (r1 - 1, c0 - 1)]
    # the pixel just outside each of the four edges, where the frame has one
    outside = [(r, c) for r, c in ((r0 - 2, c0 - 1), (r1, c1 - 1), (r0 - 1, c0 - 2), (r1 - 1, c1)) if 0 <= r < rows and 0 <= c < cols]
    assert len(outside) == (0 if box == (1, rows, 1, cols) else (3 if shape == (144, 176) else 4))      # (the default box ends on the last row)
    for pl in range(3):
        for r, c in inside:
            p = list(planes(shape, 1))
            p[pl] = p[pl].copy(); p[pl][r, c] = bad
            got, flag = run_crop(crop_exe, *p, box)
            assert flag == 1 and same_bits(got, plane_pack(*p, box)), (pl, r, c)
        for r, c in outside:
            p = list(planes(shape, 1))
            p[pl] = p[pl].copy(); p[pl][r, c] = bad
            got, flag = run_crop(crop_exe, *p, box)
            assert flag == 0 and np.array_equal(got.view(np.uint64), plane_pack(*p, box).view(np.uint64)), (pl, r, c)


def test_null_arguments_are_refused_before_a_device_is_touched(pre3):
    """these return on the first check, with or without a HIP device"""
    lib = importlib.import_module("3pre_amd._lib").lib
    plane = importlib.import_module("3pre_amd.plane")
    res, draws = plane.PlaneResult(), np.zeros(3, np.int32)
    d = draws.ctypes.data_as(C.c_void_p)
    assert lib.pre3_plane_fit_frame(None, None, 0.02, 1, d, None, None, C.byref(res)) == -1
    assert b"null" in lib.pre3_last_error()
    assert lib.pre3_plane_fit_frame_seeded(None, None, 0.02, 1, 1, 0, None, None, None, C.byref(res)) == -1
    assert lib.pre3_heading_from_frame(None, None, None, 0.02, 1, d, 1, 1, None, None) == -1
    assert lib.pre3_heading_from_frame_seeded(None, None, None, 0.02, 1, 1, 0, 1, 1, None, None, None) == -1
    assert lib.pre3_set_scan_frame(None, None, 0) == -1
