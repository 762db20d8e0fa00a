"""CPU: the .dat text rules.  tests/dattext_ref.py -- bytes.split, float() -- is the restatement; 3pre_amd/csrc/pre3_dattext.h
built for the host (tests/dattext_host_main.cpp: the three launches as loops, the header's own summaries, fold, conversion, status rules and table)
is checked against it, the restatement itself against numpy.loadtxt and against expectations written out by hand.

Bit for bit, NaNs equal to NaNs: every converted double against float(token).  Required: n_undecided == 0 over the whole corpus, no token excluded.
Equal: status, rows, cols, the bad token's row, column and byte offset; the 128-bit table rows against Python's integers."""
import ctypes as C
import inspect
import io
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import dattext_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD = "<9iqd2i"
LAYOUTS = (b"1 2\r\n3 4\r\n", b"1\t2\n3\t\t4\n", b"   1 2   \n 3 4 \n", b"1 2\n\n \t \n3 4\n\n\n", b"1 2\n3 4", b"7", b"\n\n7\n",
           b"1.5 -2 3e2 .25 5.\n6 7 8 9 10\r\n-0.0 inf -Inf NaN 1e+05\n11 12 13 14 15.0000000000000000001")
# text -> (status, bad_row, bad_col, bad_offset), written out by hand
REFUSALS = {b"1d5": (1, 0, 0, 0), b"1,2": (1, 0, 0, 0), b"% c": (1, 0, 0, 0), b"--1": (1, 0, 0, 0), b"1e": (1, 0, 0, 0), b".": (1, 0, 0, 0),
            b"+": (1, 0, 0, 0), b"1D5": (1, 0, 0, 0), b"# 1": (1, 0, 0, 0), b"infinity": (1, 0, 0, 0), b"1_0": (1, 0, 0, 0), b"0x10": (1, 0, 0, 0),
            b"1 \x00 2\n": (1, 0, 1, 2), b"1 2\n3 1,2\n": (1, 1, 1, 6), b" 1 2\r\n 3 4e\r\n": (1, 1, 1, 9),
            b"1 2 3\n4 5\n6 7 8\n": (2, 1, 2, 10), b"1 2\n3 4 5\n": (2, 1, 2, 8), b"1 2\n3 4\n5": (2, 2, 1, 9), b"1\n2 x\n": (2, 1, 1, 4),
            b"": (6, -1, -1, -1), b" \t\r\n \n": (6, -1, -1, -1)}


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("dattext_host") / "dattext_host"
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "3pre_amd", "csrc"),
                           os.path.join(ROOT, "tests", "dattext_host_main.cpp"), "-o", str(exe), "-lm"])
    return str(exe)


def run_host(exe, text, lanes=256, plane_rows=0, frame_cols=0):
    """the host program's result in the restatement's form (values column-major as the library returns them, reshaped here)"""
    b = subprocess.run([exe, "parse", str(lanes), str(plane_rows), str(frame_cols)], input=bytes(text), stdout=subprocess.PIPE, check=True).stdout
    h = struct.unpack_from(HEAD, b, 0)
    r = dict(zip(("status", "rows", "cols", "has_conf", "has_timestamp", "n_tokens", "n_undecided", "bad_row", "bad_col", "bad_offset", "timestamp",
                  "n_exact"), h))
    v = np.frombuffer(b, np.float64, h[12], struct.calcsize(HEAD))
    if r["status"] != 0:
        r["values"] = None
    elif plane_rows:
        r["values"] = v.reshape((-1, frame_cols, plane_rows)).transpose(0, 2, 1)
    else:
        r["values"] = v.reshape((r["rows"], r["cols"]), order="F")
    return r


def assert_same_result(got, want):
    for k in ("status", "rows", "cols", "has_conf", "has_timestamp", "n_tokens", "n_undecided", "bad_row", "bad_col", "bad_offset"):
        assert got[k] == want[k], (k, got[k], want[k])
    assert got["timestamp"] == want["timestamp"]
    assert (got["values"] is None) == (want["values"] is None)
    if want["values"] is not None:
        assert R.same_bits(got["values"], want["values"])


def test_the_corpus_bit_for_bit_with_nothing_undecided(host_exe):
    tokens = R.corpus()
    text, want = R.as_matrix(tokens, 40)
    assert len(tokens) >= 240000 and sum(len(t.replace(b".", b"").split(b"e")[0].lstrip(b"+-0")) > 19 for t in tokens) > 15000
    got = run_host(host_exe, text)
    assert got["status"] == 0 and got["n_undecided"] == 0 and got["n_tokens"] == want.size
    assert R.same_bits(got["values"], want)
    assert got["n_exact"] > 100            # tokens of more than 19 digits between two doubles: the exact comparison is exercised


def test_the_required_spellings_and_extremes_are_in_the_corpus():
    tokens = set(R.corpus(n_random=10))
    for t in (b"-0.0", b"+5", b".5", b"5.", b"1e+05", b"inf", b"-Inf", b"NaN", b"1.7976931348623157e308", b"2.2250738585072014e-308",
              b"4.9406564584124654e-324", b"2.2250738585072009e-308"):
        assert t in tokens
    assert np.signbit(float(b"-0.0")) and R.TOKEN.match(b"-0.0")
    assert all(R.TOKEN.match(t) for t in tokens)


def test_the_power_table_against_python_integers(host_exe):
    b = subprocess.run([host_exe, "table"], stdout=subprocess.PIPE, check=True).stdout
    T = np.frombuffer(b, np.uint64).reshape(651, 2)
    for q in (-342, -28, -27, -1, 0, 27, 55, 308):
        assert (int(T[q + 342, 0]), int(T[q + 342, 1])) == R.table_row(q), q
    assert all((int(T[q + 342, 0]), int(T[q + 342, 1])) == R.table_row(q) for q in range(-342, 309))
    assert R.table_row(0) == (1 << 63, 0) and R.table_row(-1) == (0xCCCCCCCCCCCCCCCC, 0xCCCCCCCCCCCCCCCD)


@pytest.mark.parametrize("lanes", [1, 2, 3, 256])
def test_layouts(host_exe, lanes):
    """lanes: 16-byte lanes per chunk -- small chunks put every kind of boundary inside these short texts"""
    for text in LAYOUTS:
        want = R.parse(text)
        assert want["status"] == 0
        assert_same_result(run_host(host_exe, text, lanes), want)
        for k in (1, 15, 16, 17, 33):                             # shifted against the lanes and the chunks
            assert_same_result(run_host(host_exe, b" " * k + text, lanes), R.parse(b" " * k + text))


def test_the_restatement_reads_what_numpy_loadtxt_reads():
    for text in LAYOUTS:
        assert R.same_bits(R.parse(text)["values"], np.loadtxt(io.BytesIO(text), dtype=np.float64, ndmin=2))


@pytest.mark.parametrize("text", sorted(REFUSALS))
def test_refusals(host_exe, text):
    status, row, col, off = REFUSALS[text]
    want = R.parse(text)
    assert (want["status"], want["bad_row"], want["bad_col"], want["bad_offset"]) == (status, row, col, off)
    for lanes in (1, 2, 256):
        assert_same_result(run_host(host_exe, text, lanes), want)


def test_a_long_random_text_over_many_small_chunks(host_exe):
    rng = np.random.default_rng(5)
    toks = R.corpus(seed=7, n_random=3000)[:3000]
    rows = [b" " * rng.integers(0, 3) + (b" " * rng.integers(1, 40)).join(toks[i:i + 6]) + (b"\r\n", b"\n", b" \n\n")[rng.integers(3)]
            for i in range(0, 3000, 6)]
    text = b"".join(rows)
    want = R.parse(text)
    assert want["status"] == 0 and want["values"].shape == (500, 6)
    for lanes in (1, 2, 5, 256):
        assert_same_result(run_host(host_exe, text, lanes), want)


def frame_text(rows, cols, lines, amp=None):
    rng = np.random.default_rng(rows + lines)
    a = rng.standard_normal((lines, cols)) * 3
    a[3 * rows:4 * rows] = np.abs(a[3 * rows:4 * rows]) * 1000
    a[0, 0] = np.nan
    if amp is not None:
        a[3 * rows + 1, 1] = amp
    buf = io.BytesIO()
    np.savetxt(buf, a, fmt="%.17g")
    return buf.getvalue()


def test_a_frame_in_its_three_forms_and_its_refusals(host_exe):
    rows, cols = 3, 4
    for lines in (4 * rows, 5 * rows, 5 * rows + 1):
        text = frame_text(rows, cols, lines)
        want = R.parse(text, rows, cols)
        assert (want["status"], want["has_conf"], want["has_timestamp"]) == (0, int(lines >= 5 * rows), int(lines == 5 * rows + 1))
        assert want["values"].shape == (5 if lines >= 5 * rows else 4, rows, cols)
        for lanes in (1, 256):
            assert_same_result(run_host(host_exe, text, lanes, rows, cols), want)
    for text, status in ((frame_text(rows, cols, 5 * rows, amp=-1.0), R.AMPLITUDE), (frame_text(rows, cols, 5 * rows, amp=np.inf), R.AMPLITUDE),
                         (frame_text(rows, cols, 5 * rows, amp=np.nan), R.AMPLITUDE), (frame_text(rows, cols, 5 * rows - 1), R.SHAPE),
                         (frame_text(rows, cols + 1, 4 * rows), R.SHAPE), (frame_text(rows, cols, 5 * rows + 2), R.SHAPE),
                         (frame_text(rows, cols, 4 * rows) + b"1 2\n", R.RAGGED)):
        want = R.parse(text, rows, cols)
        assert want["status"] == status
        assert_same_result(run_host(host_exe, text, 2, rows, cols), want)
    assert R.parse(frame_text(rows, cols, 4 * rows, amp=-0.0), rows, cols)["status"] == 0      # -0 is no negative amplitude (the host check's rule)


def test_the_new_symbols(pre3):
    txt = open(os.path.join(ROOT, "include", "pre3.h")).read()
    lib = C.CDLL(pre3.LIB_PATH)
    for name in ("pre3_sr_text_limits", "pre3_sr_text_parse", "pre3_sr_frame_load_text"):
        assert "PRE3_API int %s(" % name in txt and name in pre3._lib.EXPORTS and hasattr(lib, name)
    chunk, top = C.c_int32(0), C.c_int64(0)
    assert lib.pre3_sr_text_limits(C.byref(chunk), C.byref(top)) == 0 and chunk.value % 16 == 0 and top.value >= 3 * 1024 * 1024
    srm = pre3.sr4000
    assert C.sizeof(srm.TextInfo) == 56 and [f[0] for f in srm.TextInfo._fields_][:3] == ["status", "rows", "cols"]
    for fn in (srm.read_xyz_sr4000, srm.read_image_sr4000, srm.read_sr4000_data_dr_ye, srm.vodometry_frames, srm.initialize_features_scans):
        assert inspect.signature(fn).parameters["parse"].default == "host"
    with pytest.raises(ValueError):
        srm.read_xyz_sr4000("nowhere.dat", parse="gpu")
