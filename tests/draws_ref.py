"""The seeded draw tables restated in Python integers: the Philox4x64-10 block, the bounded integer, the uniform double,
three-distinct-of-m and the three rejection rules, with the library's counter / key conventions.  No numpy arithmetic on the words: every 64-bit
product is a Python integer.  tests/test_draws_ref.py pins block() against numpy.random.Philox; tests/test_gpu_draws.py compares the device tables
with these, integer for integer.

    key     = [seed, stream]                stream 1: 1-point RANSAC, 2: VO 4-point RANSAC, 3: floor-plane RANSAC
    counter = [index, attempt, seq, 0]      index: hypothesis; attempt: redraw number (0 = first draw); seq: the caller's frame / step number
"""
import math

import numpy as np

M64 = (1 << 64) - 1
PHILOX_M0, PHILOX_M1 = 0xD2E7470EE14C6C93, 0xCA5A826395121157
PHILOX_W0, PHILOX_W1 = 0x9E3779B97F4A7C15, 0xBB67AE8584CAA73B
STREAM_1P, STREAM_VO, STREAM_PLANE = 1, 2, 3
VO_MAX_REDRAWS = 64          # per position; the reference loops for ever (ransac_dr_ye.m:28-46)
PLANE_MAX_ATTEMPTS = 100     # ransac.m:122 maxDataTrials
EPS = 2.220446049250313e-16


def block(counter, key):
    """Philox4x64-10: 4 x uint64 from counter[4], key[2]"""
    c0, c1, c2, c3 = [int(v) & M64 for v in counter]
    k0, k1 = [int(v) & M64 for v in key]
    for r in range(10):
        if r:
            k0, k1 = (k0 + PHILOX_W0) & M64, (k1 + PHILOX_W1) & M64
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> 64) ^ c1 ^ k0, p1 & M64, (p0 >> 64) ^ c3 ^ k1, p0 & M64
    return [c0, c1, c2, c3]


def draw_block(seed, stream, index, attempt, seq):
    return block([index, attempt, seq, 0], [seed, stream])


def bounded(w, rng):
    """an integer in [0, rng): the high 64 bits of w * rng (no rejection; bias <= rng / 2^64)"""
    return (int(w) * int(rng)) >> 64


def uniform(w):
    """a double in [0, 1): the top 53 bits"""
    return (int(w) >> 11) * 2.0 ** -53


def three_distinct(m, w0, w1, w2):
    """randperm(m)(1:3)'s distribution from three words: ranks j0 in [0,m), j1 in [0,m-1), j2 in [0,m-2), each later one shifted past the
    earlier picks in ascending order"""
    i0 = bounded(w0, m)
    i1 = bounded(w1, m - 1)
    if i1 >= i0:
        i1 += 1
    i2 = bounded(w2, m - 2)
    lo, hi = (i0, i1) if i0 < i1 else (i1, i0)
    if i2 >= lo:
        i2 += 1
    if i2 >= hi:
        i2 += 1
    return i0, i1, i2


# ---- select_random_match.m:40-51 -------------------------------------------------------------------------------------------------------------------
def draw_1p(seed, seq, m, n_draw):
    """(n_draw, k) int32: k = 3 when m > 3, else 1; m == 0: one column of zeros (synth.draw_hypotheses).  attempt is always 0."""
    if m == 0:
        return np.zeros((n_draw, 1), np.int32)
    k = 3 if m > 3 else 1
    out = np.zeros((n_draw, k), np.int32)
    for h in range(n_draw):
        w = draw_block(seed, STREAM_1P, h, 0, seq)
        out[h] = three_distinct(m, w[0], w[1], w[2]) if k == 3 else (bounded(w[0], m),)
    return out


# ---- ransac_dr_ye.m:28-48 --------------------------------------------------------------------------------------------------------------------------
def vo_position(pnum, u):
    """round((pnum - 1) * u + 1), MATLAB rounding, then 0-based"""
    return int(math.floor(((pnum - 1) * u + 1.0) + 0.5)) - 1


def vo_bad(m, r, p):
    """whether position p (1..3) of r must be redrawn: it repeats an earlier position or ind_dup<p> fires (vo.draw_hypotheses' predicates, the
    mixed-row comparisons of ind_dup3 included)"""
    if p == 1:
        return bool(r[1] == r[0] or m[0][r[0]] == m[0][r[1]] or m[1][r[0]] == m[1][r[1]])
    if p == 2:
        return bool(r[2] == r[0] or r[2] == r[1] or m[0][r[0]] == m[0][r[2]] or m[0][r[1]] == m[0][r[2]] or m[1][r[0]] == m[1][r[2]] or m[1][r[1]] == m[1][r[2]])
    return bool(r[3] == r[0] or r[3] == r[1] or r[3] == r[2] or m[0][r[0]] == m[0][r[3]] or m[0][r[1]] == m[1][r[3]] or m[0][r[2]] == m[0][r[3]]
                or m[1][r[0]] == m[0][r[3]] or m[1][r[1]] == m[1][r[3]] or m[1][r[2]] == m[1][r[3]])


def vo_rule(match, n_hyp, uniforms):
    """The rule on any source of uniforms: uniforms(h, p, a) is the number behind position p of hypothesis h at attempt a.  Returns
    (draws (n_hyp, 4) int32, capped hypotheses, largest attempt used)."""
    m = [[v for v in row] for row in np.asarray(match).tolist()]
    pnum = len(m[0])
    out = np.zeros((n_hyp, 4), np.int32)
    capped, most = 0, 0
    for h in range(n_hyp):
        r = [vo_position(pnum, uniforms(h, p, 0)) for p in range(4)]
        cap = False
        for p in (1, 2, 3):
            a = 0
            while vo_bad(m, r, p) and a < VO_MAX_REDRAWS:
                a += 1
                r[p] = vo_position(pnum, uniforms(h, p, a))
            most = max(most, a)
            cap = cap or vo_bad(m, r, p)
        capped += int(cap)
        out[h] = r
    return out, capped, most


def draw_vo(seed, seq, match, n_hyp):
    """The first draws are words 0..3 of block(h, 0); the redraw of position p at attempt a >= 1 is word p of block(h, a).  A position stops after
    VO_MAX_REDRAWS redraws and keeps its last value; a hypothesis one of whose positions is still inadmissible then counts as capped."""
    cache = {}

    def uniforms(h, p, a):
        if (h, a) not in cache:
            if len(cache) > 4096:
                cache.clear()
            cache[(h, a)] = draw_block(seed, STREAM_VO, h, a, seq)
        return uniform(cache[(h, a)][p])

    return vo_rule(match, n_hyp, uniforms)


# ---- ransac.m:142-176 ------------------------------------------------------------------------------------------------------------------------------
def collinear_norm(X, Y, Z, i1, i2, i3):
    """norm(cross(p2 - p1, p3 - p1)) with every product and sum rounded on its own (iscolinear.m:62), as the kernel evaluates it"""
    a = (X[i2] - X[i1], Y[i2] - Y[i1], Z[i2] - Z[i1])
    b = (X[i3] - X[i1], Y[i3] - Y[i1], Z[i3] - Z[i1])
    n0 = a[1] * b[2] - a[2] * b[1]
    n1 = a[2] * b[0] - a[0] * b[2]
    n2 = a[0] * b[1] - a[1] * b[0]
    return math.sqrt(n0 * n0 + n1 * n1 + n2 * n2)


def draw_plane(seed, seq, XYZ, n_draw):
    """XYZ (3, npts): the cropped points as k_plane_score sees them.  Per attempt three distinct of npts; redrawn while the points are collinear,
    at most PLANE_MAX_ATTEMPTS attempts, the last one kept.  Returns (draws (n_draw, 3) int32, largest attempt number used,
    smallest |norm - eps| / eps met)."""
    P = np.asarray(XYZ, dtype=np.float64)
    X, Y, Z = P[0].tolist(), P[1].tolist(), P[2].tolist()
    npts = len(X)
    out = np.zeros((n_draw, 3), np.int32)
    most, margin = 0, math.inf
    for h in range(n_draw):
        for a in range(PLANE_MAX_ATTEMPTS):
            w = draw_block(seed, STREAM_PLANE, h, a, seq)
            ind = three_distinct(npts, w[0], w[1], w[2])
            nrm = collinear_norm(X, Y, Z, *ind)
            margin = min(margin, abs(nrm - EPS) / EPS)
            if not nrm < EPS:
                break
        most = max(most, a)
        out[h] = ind
    return out, most, margin


def draw_plane_margins(seed, seq, XYZ, n_draw):
    """The same walk as draw_plane, split by whether a sample repeats a point (two of its three points equal coordinate for coordinate -- an invalid
    SR4000 return is all-zero).  Such a sample's cross product is exactly zero in any rounding: a difference of equal numbers is +0 and the two
    products of every component are then equal bit for bit; asserted here.  Returns (smallest |norm - eps| / eps over the samples of three different
    points, number of samples with a repeated point)."""
    P = np.asarray(XYZ, dtype=np.float64)
    X, Y, Z = P[0].tolist(), P[1].tolist(), P[2].tolist()
    npts = len(X)
    margin, repeated = math.inf, 0
    for h in range(n_draw):
        for a in range(PLANE_MAX_ATTEMPTS):
            w = draw_block(seed, STREAM_PLANE, h, a, seq)
            ind = three_distinct(npts, w[0], w[1], w[2])
            nrm = collinear_norm(X, Y, Z, *ind)
            pts = {(X[i], Y[i], Z[i]) for i in ind}
            if len(pts) < 3:
                repeated += 1
                assert nrm == 0.0
            else:
                margin = min(margin, abs(nrm - EPS) / EPS)
            if not nrm < EPS:
                break
    return margin, repeated
