"""The .dat text rules of 3pre_amd/csrc/pre3_dattext.h restated in plain Python, independent of the header's arithmetic:
bytes.split per line, float() per token, the shape and status rules.  parse(text, plane_rows=0, frame_cols=0) -> dict(status, rows, cols, has_conf,
has_timestamp, n_tokens, n_undecided, bad_row, bad_col, bad_offset, timestamp, values) -- values: the matrix (rows, cols), or for a frame the
(4 or 5, plane_rows, frame_cols) planes in file order z, x, y, amplitude, confidence; None unless status == 0."""
import math
import re

import numpy as np

OK, BAD, RAGGED, SHAPE, UNDECIDED, AMPLITUDE, EMPTY = range(7)
TOKEN = re.compile(rb"[+-]?(?:(?:[0-9]+(?:\.[0-9]*)?|\.[0-9]+)(?:[eE][+-]?[0-9]+)?|[iI][nN][fF]|[nN][aA][nN])\Z")
GAP = re.compile(rb"[^ \t\r]+")


def lines_of(text):
    """[(tokens, offsets)] of the non-empty lines: a row ends at \\n or at the end of the text; space, tab and \\r separate"""
    out, pos = [], 0
    for line in bytes(text).split(b"\n"):
        found = [(m.group(), pos + m.start()) for m in GAP.finditer(line)]
        if found:
            out.append(([t for t, _ in found], [o for _, o in found]))
        pos += len(line) + 1
    return out


def parse(text, plane_rows=0, frame_cols=0, cap=None):
    text = bytes(text)
    rows = lines_of(text)
    n = sum(len(t) for t, _ in rows)
    cols = len(rows[0][0]) if rows else 0
    r = dict(status=OK, rows=len(rows), cols=cols, has_conf=0, has_timestamp=0, n_tokens=n, n_undecided=0, bad_row=-1, bad_col=-1, bad_offset=-1,
             timestamp=-1.0, values=None)
    if cap is None:
        cap = (5 * plane_rows + 1) * frame_cols if plane_rows else (len(text) + 1) // 2
    if n == 0:
        r["status"] = EMPTY
        return r
    if n > cap:
        r["status"] = SHAPE
        return r
    for i, (toks, offs) in enumerate(rows):
        if len(toks) != cols:                                  # the first extra token, or where the next row starts too early
            nxt = rows[i + 1][1][0] if i + 1 < len(rows) else len(text)
            r.update(status=RAGGED, bad_row=i, bad_col=min(len(toks), cols), bad_offset=offs[cols] if len(toks) > cols else nxt)
            return r
    for i, (toks, offs) in enumerate(rows):
        for j, t in enumerate(toks):
            if not TOKEN.match(t):
                r.update(status=BAD, bad_row=i, bad_col=j, bad_offset=offs[j])
                return r
    a = np.array([[float(t) for t in toks] for toks, _ in rows], dtype=np.float64)
    if not plane_rows:
        r["values"] = a
        return r
    if cols != frame_cols or len(rows) not in (4 * plane_rows, 5 * plane_rows, 5 * plane_rows + 1):
        r["status"] = SHAPE
        return r
    r["has_conf"] = int(len(rows) >= 5 * plane_rows)
    r["has_timestamp"] = int(len(rows) == 5 * plane_rows + 1)
    if r["has_timestamp"]:
        r["timestamp"] = float(a[5 * plane_rows, 0])
    amp = a[3 * plane_rows:4 * plane_rows]
    if not all(math.isfinite(v) and v >= 0 for v in amp.ravel()):
        r["status"] = AMPLITUDE
        return r
    r["values"] = a[:(5 if r["has_conf"] else 4) * plane_rows].reshape(-1, plane_rows, frame_cols)
    return r


def same_bits(a, b):
    """bit-equal doubles, every NaN equal to every NaN"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb]))


def table_row(q):
    """(high, low) of the power-of-five table at q, from Python's integers"""
    if q >= 0:
        c = 5 ** q
        while c < 1 << 127:
            c *= 2
    else:
        p, z = 5 ** -q, 0
        while (1 << z) < p:
            z += 1
        c = (1 << (z + 127 if q >= -27 else 2 * z + 128)) // p + 1
    while c >= 1 << 128:
        c //= 2
    return c >> 64, c & ((1 << 64) - 1)


def corpus(seed=20260, n_random=200000):
    """the token corpus of the conversion tests, as a list of bytes: seeded random tokens of 1-19 and of more than 19 digits over the whole exponent
    range, the four printf forms of .dat writers, exact halfway integers, the extremes, and the spellings the grammar allows"""
    rng = np.random.default_rng(seed)
    out = []
    nd = rng.integers(1, 20, n_random)
    qs = rng.integers(-342, 309, n_random)
    kind = rng.integers(0, 10, n_random)
    big = rng.integers(0, 1 << 63, n_random, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n_random).astype(np.uint64)
    val = rng.standard_normal(n_random) * 10.0 ** rng.integers(-3, 5, n_random)
    for i in range(n_random):
        k = kind[i]
        if k <= 2:                                             # 1-19 digits, any exponent
            d = str(int(big[i]))[:nd[i]]
            out.append(("%se%d" % (d, qs[i])).encode())
        elif k == 3:                                           # a random 64-bit w
            out.append(("%de%d" % (int(big[i]), min(int(qs[i]), 289))).encode())
        elif k == 4:                                           # more than 19 digits, a point somewhere
            d = str(int(big[i])) + str(int(big[(i + 1) % n_random]))[:int(nd[i]) + 1]
            cut = int(nd[i]) % len(d)
            out.append(("%s.%se%d" % (d[:cut], d[cut:], max(int(qs[i]), -330) - cut + 1)).encode())
        elif k == 5:
            out.append(b"%.6f" % val[i])
        elif k == 6:
            out.append(b"%.7e" % val[i])
        elif k == 7:
            out.append(b"%.16e" % val[i])
        elif k == 8:
            out.append(b"%d" % int(val[i]))
        else:                                                  # subnormals and the edge of overflow
            out.append(("%se%d" % (str(int(big[i]))[:nd[i]], int(rng.integers(-342, -300)) if i & 1 else int(rng.integers(285, 309)))).encode())
    for i in range(40000):                                     # (2 m + 1) * 2^e < 2^64: exactly between two doubles once it has more than 53 bits
        m = int(rng.integers(1 << 52, 1 << 53))
        e = int(rng.integers(0, 10))
        out.append(b"%d" % ((2 * m + 1) << e))
    for i in range(2000):                                      # the same ties with digits behind them: just above, and all zeros
        m = int(rng.integers(1 << 52, 1 << 53))
        out.append(b"%d.%s" % ((2 * m + 1) << int(rng.integers(0, 10)), b"0" * 30 + (b"1" if i & 1 else b"0")))
    out += [b"1.7976931348623157e308", b"1.7976931348623158e308", b"1.7976931348623159e308", b"2.2250738585072014e-308", b"2.2250738585072011e-308",
            b"4.9406564584124654e-324", b"2.4703282292062327e-324", b"2.4703282292062328e-324", b"2.2250738585072009e-308", b"1e309", b"1e-400",
            b"-0.0", b"+5", b".5", b"5.", b"1e+05", b"inf", b"-Inf", b"NaN", b"+nan", b"-INF", b"0", b"-0", b"0e999", b"00012.5000", b"1E5", b"-.25e-1",
            b"9007199254740993", b"9007199254740992.99999999999999999999", b"0." + b"0" * 400 + b"1e400", b"1" + b"0" * 400 + b"e-400",
            b"123456789012345678901234567890123456789012345678901234567890", b"0.1000000000000000055511151231257827021181583404541015625",
            b"0.500000000000000166533453693773481063544750213623046875", b"1.00000000000000011102230246251565404236316680908203125",
            b"1.00000000000000011102230246251565404236316680908203124", b"1.00000000000000011102230246251565404236316680908203126"]
    return out


def as_matrix(tokens, cols):
    """the tokens as a text of `cols` columns (padded with zeros) and the (rows, cols) matrix float() makes of it"""
    tokens = list(tokens) + [b"0"] * (-len(tokens) % cols)
    rows = [tokens[i:i + cols] for i in range(0, len(tokens), cols)]
    return b"\n".join(b" ".join(r) for r in rows) + b"\n", np.array([[float(t) for t in r] for r in rows], dtype=np.float64)
