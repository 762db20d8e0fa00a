"""GPU: SR4000 .dat text parsed on the device (pre3_dattext.hip) against the plain-Python restatement tests/dattext_ref.py
(bytes.split, float()) and against the host parse it stands in for (numpy.loadtxt -> SrFrame.load).

Bit for bit, NaNs equal to NaNs: every double pre3_sr_text_parse returns; planes(), image(), maxima(), has_conf and the timestamp of a frame loaded
from text against the same file through load_dat and SrFrame.load; every output of vodometry_frames(parse="device") against parse="host".
Equal: every field of the info block of a refused text."""
import ctypes as C
import importlib
import io
import re

import numpy as np
import pytest

import dattext_ref as R
import sr_frame_ref as sr

pytestmark = pytest.mark.gpu
srm = importlib.import_module("3pre_amd.sr4000")
_lib = importlib.import_module("3pre_amd._lib")
E_ARG, E_NOMEM = -1, -6
INFO_FIELDS = ("status", "rows", "cols", "has_conf", "has_timestamp", "n_tokens", "n_undecided", "bad_row", "bad_col", "bad_offset")
REFUSALS = (b"1d5", b"1 2\n3 1,2\n", b"% c\n1 2\n", b"--1", b"1e", b".", b"1 \x00 2\n", b"1 2 3\n4 5\n6 7 8\n", b"1 2\n3 4 5\n", b"1 2\n3 4\n5", b"", b" \t\r\n \n")
TOKENS = re.compile(rb"[^ \t\r\n]+")
_CORPUS = {}


def corpus_matrix():
    """the CPU corpus as a 40-column text and what float() makes of it, computed once and shared (read-only)"""
    if not _CORPUS:
        _CORPUS["m"] = R.as_matrix(R.corpus(), 40)
    return _CORPUS["m"]


def raw_parse(text, cap=None, fill=-7.25):
    """pre3_sr_text_parse as it is: (return code, info dict, the caller's array as the call left it)"""
    info = srm.TextInfo()
    cap = (len(text) + 1) // 2 if cap is None else cap
    out = np.full(max(cap, 1), fill)
    rc = _lib.lib.pre3_sr_text_parse(0, text, len(text), _lib.dptr(out), cap, C.byref(info))
    return rc, info.as_dict(), out


def assert_parses_like_the_restatement(text):
    want = R.parse(text)
    assert want["status"] == R.OK
    got, info = srm.loadtxt_device(text)
    assert (info["status"], info["rows"], info["cols"], info["n_tokens"], info["n_undecided"]) == (0,) + want["values"].shape + (want["values"].size, 0)
    assert R.same_bits(got, want["values"])


def test_the_corpus_as_a_40_column_matrix():
    text, want = corpus_matrix()
    chunk, top = srm.text_limits()
    assert 3 * chunk < len(text) <= top and want.size >= 200000
    got, info = srm.loadtxt_device(text)
    assert info["n_undecided"] == 0 and (info["rows"], info["cols"]) == want.shape
    assert R.same_bits(got, want)


def boundary_text(chunk):
    """five columns of tokens of varying length over more than three chunks, \\r\\n line ends, padded with spaces so that a token, a \\r\\n pair and a
    run of spaces each lie across a chunk boundary"""
    rng = np.random.default_rng(11)
    forms = (b"%.6f", b"%.7e", b"%.16e", b"%d")
    rows = []
    while sum(len(r) for r in rows) < 3 * chunk + 400:
        rows.append(b" ".join(forms[k] % (int(v) if k == 3 else v) for v, k in zip(rng.standard_normal(5) * 1000, rng.integers(0, 4, 5))) + b"\r\n")
    text = b"".join(rows)
    starts = [m.start() for m in TOKENS.finditer(text) if m.end() - m.start() >= 3]
    s0 = max(s for s in starts if s <= chunk - 2)
    text = b" " * (chunk - 1 - s0) + text                     # a token starts on the last byte of chunk 0
    r0 = text.rindex(b"\r\n", 0, 2 * chunk - 1)
    text = text[:r0] + b" " * (2 * chunk - 1 - r0) + text[r0:]      # \r ends chunk 1, \n starts chunk 2
    g0 = text.rindex(b" ", 0, 3 * chunk - 3)
    text = text[:g0] + b" " * (3 * chunk + 3 - g0) + text[g0:]      # a run of spaces from chunk 2 into chunk 3
    return text


def test_tokens_a_crlf_pair_and_a_run_of_spaces_across_chunk_boundaries():
    chunk, _ = srm.text_limits()
    text = boundary_text(chunk)
    assert len(text) > 3 * chunk
    assert text[chunk - 2:chunk - 1] in (b" ", b"\n") and TOKENS.fullmatch(text[chunk - 1:chunk + 1])
    assert text[2 * chunk - 1:2 * chunk + 1] == b"\r\n"
    assert text[3 * chunk - 4:3 * chunk + 3] == b" " * 7
    assert_parses_like_the_restatement(text)


def test_every_alignment_of_the_16_byte_loads():
    body = b"1.5 -2 3e2 .25 5.\n6 7 8 9 10\r\n-0.0 inf -Inf NaN 1e+05\n11 12 13 14 15.0000000000000000001"
    want = R.parse(body)["values"]
    assert want.shape == (4, 5)
    for k in range(64):
        got, info = srm.loadtxt_device(b" " * k + body)
        assert R.same_bits(got, want), k


def test_a_text_that_ends_in_a_token_at_its_last_byte():
    chunk, _ = srm.text_limits()
    for n in (chunk, chunk + 1, 16, 17, 1):
        text = (b"12 " * n)[:n - 1] + b"7"
        assert len(text) == n and text[-1:] == b"7"
        assert_parses_like_the_restatement(text)


def test_layouts():
    for text in (b"1 2\r\n3 4\r\n", b"1\t2\n3\t\t4\n", b"   1 2   \n 3 4\n", b"1 2\n\n \t \n3 4\n\n\n", b"1 2\n3 4", b"7", b"\n\n7\n"):
        assert_parses_like_the_restatement(text)


@pytest.mark.parametrize("text", REFUSALS)
def test_refusals_leave_out_untouched(text):
    want = R.parse(text)
    assert want["status"] != R.OK
    rc, info, out = raw_parse(text, cap=16)
    assert rc == E_ARG
    assert {k: info[k] for k in INFO_FIELDS} == {k: want[k] for k in INFO_FIELDS}
    assert np.all(out == -7.25)
    with pytest.raises(srm.Pre3Error, match=srm.TEXT_STATUS[want["status"]]):
        srm.loadtxt_device(text)


def test_the_expected_statuses_of_the_refusals():
    got = [R.parse(t)["status"] for t in REFUSALS]
    assert got == [R.BAD] * 7 + [R.RAGGED] * 3 + [R.EMPTY] * 2


def test_cap_one_short_is_nomem():
    text = b"1 2 3\n4 5 6\n"
    rc, info, out = raw_parse(text, cap=5)
    assert rc == E_NOMEM and (info["rows"], info["cols"], info["n_tokens"]) == (2, 3, 6) and np.all(out == -7.25)
    rc, info, out = raw_parse(text, cap=6)
    assert rc == 0 and np.array_equal(out, [1, 4, 2, 5, 3, 6])


# ---- pre3_sr_frame_load_text against load_dat + SrFrame.load

def frame_text(rows, cols, blocks, seed=0, edit=None):
    """the .dat text of a synthetic frame: blocks = 4 (no confidence map), 5, or 6 (5 and the timestamp row); edit(fr) changes the planes first"""
    fr = sr.make_frame(rows, cols, seed=seed, conf=blocks >= 5)
    fr["z"][rows // 2, cols // 3] = np.nan
    if edit:
        edit(fr)
    a = np.vstack([fr[k] for k in ("z", "x", "y", "amp")] + ([fr["conf"]] if blocks >= 5 else []))
    if blocks == 6:
        a = np.vstack([a, np.r_[1234567.875, np.zeros(cols - 1)]])
    buf = io.BytesIO()
    np.savetxt(buf, a, fmt="%.17g")
    return buf.getvalue()


def frame_state(f):
    return f.planes() + (f.image(),) + f.maxima() + (f.has_conf,)


def same_state(a, b):
    return all((u is None and v is None) or R.same_bits(u, v) for u, v in zip(a, b))


def host_twin(text, rows, cols, mode):
    with srm.SrFrame(rows, cols) as f:
        d = srm.load_dat(io.BytesIO(text), rows)
        f.load(d, mode)
        return frame_state(f), d["timestamp"]


@pytest.mark.parametrize("shape", [(4, 5), (17, 16), (144, 176)])
def test_a_frame_loaded_from_text_equals_the_host_parsed_twin(shape):
    rows, cols = shape
    with srm.SrFrame(rows, cols) as f:
        for blocks in (4, 5, 6):
            text = frame_text(rows, cols, blocks, seed=blocks)
            for mode in (srm.MODE_XYZ, srm.MODE_DR_YE):
                want, stamp = host_twin(text, rows, cols, mode)
                r = f.load_text(text, mode)
                assert r == dict(has_conf=blocks >= 5, timestamp=stamp, rows=(blocks if blocks < 6 else 5) * rows + (blocks == 6))
                got = frame_state(f)
                assert same_state(got, want), (blocks, mode)
                assert np.isnan(got[2]).any()                      # the NaN planted in z came through


def _negative(fr):
    fr["amp"][1, 2] = -1.0


def _infinite(fr):
    fr["amp"][3, 1] = np.inf


def test_refused_files_leave_the_frame_and_its_keypoint_record_alone():
    rows, cols = 17, 16
    good = frame_text(rows, cols, 5, seed=9)
    lines = good.split(b"\n")
    ragged = b"\n".join(lines[:7] + [lines[7] + b" 1"] + lines[8:])
    cases = ((frame_text(rows, cols, 5, seed=1, edit=_negative), R.AMPLITUDE), (frame_text(rows, cols, 5, seed=2, edit=_infinite), R.AMPLITUDE),
             (ragged, R.RAGGED), (b"\n".join(lines[:5 * rows - 1]) + b"\n", R.SHAPE), (frame_text(rows, cols + 1, 5), R.SHAPE),
             (frame_text(rows + 1, cols, 6), R.SHAPE), (b"1d5" + good[good.index(b" "):], R.BAD), (b"", R.EMPTY))
    rng = np.random.default_rng(3)
    frm = np.asfortranarray(np.vstack([rng.uniform(1, cols, 12), rng.uniform(1, rows, 12), rng.uniform(1, 3, 12), rng.uniform(-3, 3, 12)]))
    des = np.asfortranarray(rng.random((128, 12)))
    with srm.SrFrame(rows, cols) as f:
        f.load_text(good, srm.MODE_XYZ)
        kept = f.keypoints(frm, des, srm.GATE_DEPTH)
        before = frame_state(f)
        for text, status in cases:
            want = R.parse(text, rows, cols)
            assert want["status"] == status
            with pytest.raises(srm.Pre3Error, match=srm.TEXT_STATUS[status]) as e:
                f.load_text(text, srm.MODE_DR_YE)
            assert e.value.code == E_ARG and {k: e.value.info[k] for k in INFO_FIELDS} == {k: want[k] for k in INFO_FIELDS}
            assert same_state(frame_state(f), before)
            again = f.gate(srm.GATE_DEPTH)                         # the record of the frame that is still there
            assert all(R.same_bits(again[k], kept[k]) for k in ("frames", "descriptors", "xyz", "rho")) and np.array_equal(again["keep_idx"], kept["keep_idx"])


def test_vodometry_frames_parsed_on_the_device_equals_the_host_parsed_run(tmp_path):
    from test_gpu_sift import _texture_planes
    from test_gpu_vo_pair import _write_dat, assert_same_result
    d1, d2 = tmp_path / "d1_0001.dat", tmp_path / "d1_0002.dat"
    _write_dat(d1, _texture_planes(1)); _write_dat(d2, _texture_planes(1))      # the same scan twice: every keypoint has its match
    host = srm.vodometry_frames(str(d1), str(d2), 5, 0, parse="host")
    dev = srm.vodometry_frames(str(d1), str(d2), 5, 0, parse="device")
    assert np.array_equal(dev["kept1"], host["kept1"]) and np.array_equal(dev["kept2"], host["kept2"])
    assert dev["pnum"] == host["pnum"] > 100 and np.array_equal(dev["match"], host["match"])
    assert_same_result(dev, host)
    with pytest.raises(ValueError):
        srm.vodometry_frames(str(d1), str(d2), 5, 0, parse="gpu")
