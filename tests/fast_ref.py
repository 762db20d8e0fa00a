"""FAST-9 corners and the patch-feature initialisation policy restated in numpy: the segment test of the FAST papers
(Rosten and Drummond, ICCV 2005 / ECCV 2006: 9 contiguous pixels of the 16-pixel ring all > centre + t or all < centre - t), fast_nonmax.m:61-100,
initialize_a_feature.m:55-194, initialize_n_features_FAST.m:55-145 and gate 0 of inittialize_depth_my_version.m:40-45,74-92.  Integer arithmetic on
the byte image: every list is exact.  This is NOT the learned decision tree the reference ships as fast_corner_detect_9.m; the two agree on the
fixture's crop at thresholds 10, 20 and 30 (tests/golden/make_fast_fixtures.py re-derives that) and differ elsewhere -- section 30 has the counts.

An image is a (nRows, nCols) array; a corner is (x, y) = (column, row), 1-based, and lists run x outer, y inner: ascending column-major index.
"""
import math

import numpy as np

import draws_ref as dr

# fast_nonmax.m:44-59: (dx, dy) of ring pixel k; consecutive k are neighbours on the circle, 15 next to 0
RING = ((0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3))
MAX_ATTEMPTS = 10                        # initialize_a_feature.m:34
BOX_SEMI = (30, 20)                      # :35-36: rows, columns
EXCLUDED_BAND = 21                       # :33
STREAM_FAST = 5                          # key = [seed, 5], counter = [attempt, 0, seq, 0]; words 0, 1 -> u1, u2
INITIALISED, NO_BOX, NO_DEPTH_NAN, NO_DEPTH_NEAR, NO_DEPTH_CONF = 0, 1, 2, 3, 4
GATE_KEPT = 0                            # per-maximum verdicts of initialize_n_features_fast: GATE_KEPT or one of the NO_DEPTH_* above


def rotl16(m, k):
    m = np.asarray(m, dtype=np.uint32)
    return ((m << np.uint32(k)) | (m >> np.uint32(16 - k))) & np.uint32(0xFFFF)


def has_run9(m):
    """whether the 16-bit ring mask holds 9 circularly contiguous set bits -- rotate-and-AND: runs of 2, 4, 8, then 9"""
    m = np.asarray(m, dtype=np.uint32)
    r2 = m & rotl16(m, 1)
    r4 = r2 & rotl16(r2, 2)
    r8 = r4 & rotl16(r4, 4)
    return (r8 & rotl16(m, 8)) != 0


def has_run9_loop(m):
    """the same, literally: some start s with bits s, s+1, .., s+8 (mod 16) all set"""
    m = int(m)
    return any(all((m >> ((s + j) & 15)) & 1 for j in range(9)) for s in range(16))


def ring_stack(im):
    """(16, nRows - 6, nCols - 6) ring values of the candidates (rows, columns 4 .. size - 3, 1-based) and their centres"""
    a = np.asarray(im).astype(np.int32)
    R, C = a.shape
    assert R >= 7 and C >= 7
    ring = np.stack([a[3 + dy:R - 3 + dy, 3 + dx:C - 3 + dx] for dx, dy in RING])
    return ring, a[3:R - 3, 3:C - 3]


def masks(im, threshold):
    """bright and dark 16-bit masks of every candidate (strict > and <, fast_corner_detect_9.m:61-63)"""
    ring, c = ring_stack(im)
    w = (np.uint32(1) << np.arange(16, dtype=np.uint32))[:, None, None]
    bright = ((ring > c + threshold) * w).sum(axis=0).astype(np.uint32)
    dark = ((ring < c - threshold) * w).sum(axis=0).astype(np.uint32)
    return bright, dark


def corner_map(im, threshold):
    b, d = masks(im, threshold)
    out = np.zeros(np.asarray(im).shape, bool)
    out[3:-3, 3:-3] = has_run9(b) | has_run9(d)
    return out


def _list(mask):
    """(K, 2) int32 (x, y), 1-based, x outer / y inner"""
    xs, ys = np.nonzero(mask.T)
    return np.stack([xs + 1, ys + 1], axis=1).astype(np.int32)


def fast_corner_detect_9(im, threshold):
    return _list(corner_map(im, threshold))


def score_map(im, cmap, barrier):
    """fast_nonmax.m:70-75 at the corners of cmap, 0 elsewhere"""
    ring, c = ring_stack(im)
    pos = np.maximum(ring - (c + barrier), 0).sum(axis=0)
    neg = np.maximum(c - barrier - ring, 0).sum(axis=0)
    s = np.zeros(np.asarray(im).shape, np.int64)
    s[3:-3, 3:-3] = np.maximum(pos, neg)
    return np.where(cmap, s, 0)


def nonmax_map(im, cmap, barrier):
    """fast_nonmax.m:87-92: a corner whose score is >= all eight neighbours' (ties and score-0 corners are kept)"""
    s = score_map(im, cmap, barrier)
    R, C = s.shape
    keep = cmap.copy()
    inner = s[3:R - 3, 3:C - 3]
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                keep[3:R - 3, 3:C - 3] &= inner >= s[3 + dy:R - 3 + dy, 3 + dx:C - 3 + dx]
    return keep, s


def fast_nonmax(im, threshold, barrier):
    """fast_nonmax(im, barrier, fast_corner_detect_9(im, threshold)): the maxima and their scores"""
    keep, s = nonmax_map(im, corner_map(im, threshold), barrier)
    c = _list(keep)
    return c, s[c[:, 1] - 1, c[:, 0] - 1].astype(np.int32)


def detect(im, threshold, barrier, nonmax, r0=0, c0=0, rows=None, cols=None):
    """pre3_fast_detect on the rectangle [r0, r0 + rows) x [c0, c0 + cols) (0-based), taken as an image of its own: (uv (K, 2), score (K,))"""
    a = np.asarray(im)
    sub = a[r0:r0 + (a.shape[0] - r0 if rows is None else rows), c0:c0 + (a.shape[1] - c0 if cols is None else cols)]
    if nonmax:
        return fast_nonmax(sub, threshold, barrier)
    cmap = corner_map(sub, threshold)
    c = _list(cmap)
    return c, score_map(sub, cmap, barrier)[c[:, 1] - 1, c[:, 0] - 1].astype(np.int32)


# ---- initialize_a_feature.m ---------------------------------------------------------------------------------------------------------------------
def matlab_round(v):
    """MATLAB's round for v >= 0 (halves up; v - floor(v) is exact, so 0.49999999999999994 rounds to 0)"""
    f = math.floor(v)
    return int(f) + (1 if v - f >= 0.5 else 0)


def centre_ranges(nRows, nCols):
    """:65-68 with BoxLimX = [1 nCols], BoxLimY = [1 nRows]: (row range, row offset, column range, column offset)"""
    return (nRows - 1) - 2 * EXCLUDED_BAND - 2 * BOX_SEMI[0], EXCLUDED_BAND + BOX_SEMI[0], (nCols - 1) - 2 * EXCLUDED_BAND - 2 * BOX_SEMI[1], EXCLUDED_BAND + BOX_SEMI[1]


def box_centre(u1, u2, nRows, nCols):
    rr, ro, cr, co = centre_ranges(nRows, nCols)
    return matlab_round(u1 * rr) + ro, matlab_round(u2 * cr) + co


def seeded_centres(seed, seq, nRows, nCols, attempts=MAX_ATTEMPTS):
    """(attempts, 2) int32 (row centre, column centre)"""
    out = np.zeros((attempts, 2), np.int32)
    for a in range(attempts):
        w = dr.block([a, 0, seq, 0], [seed, STREAM_FAST])
        out[a] = box_centre(dr.uniform(w[0]), dr.uniform(w[1]), nRows, nCols)
    return out


def all_centres(nRows, nCols):
    """every centre the policy can draw: (rr + 1) * (cr + 1) boxes"""
    rr, ro, cr, co = centre_ranges(nRows, nCols)
    return [(ro + i, co + j) for i in range(rr + 1) for j in range(cr + 1)]


def features_in_box(uv_pred, centre, strict_reference):
    """:164-174.  uv_pred (k, 2) = (u, v) = (column, row) of the landmarks that have an h.  strict_reference: u against the ROW centre +/- 30 and v
    against the COLUMN centre +/- 20, as written; else the axes matched.  Strict inequalities."""
    uv = np.asarray(uv_pred, dtype=np.float64).reshape(-1, 2)
    if uv.shape[0] == 0:
        return False
    a, b = (uv[:, 0], uv[:, 1]) if strict_reference else (uv[:, 1], uv[:, 0])
    return bool(((a > centre[0] - BOX_SEMI[0]) & (a < centre[0] + BOX_SEMI[0]) & (b > centre[1] - BOX_SEMI[1]) & (b < centre[1] + BOX_SEMI[1])).any())


def box_first_maximum(im, centre, threshold=10, barrier=20):
    """the first maximum of the 61 x 41 box at centre (row, column), in image coordinates (u, v), or None (:93-105, :152-157)"""
    r0, c0 = centre[0] - BOX_SEMI[0] - 1, centre[1] - BOX_SEMI[1] - 1
    c, _ = detect(im, threshold, barrier, 1, r0, c0, 2 * BOX_SEMI[0] + 1, 2 * BOX_SEMI[1] + 1)
    return None if c.shape[0] == 0 else (int(c[0, 0]) + c0, int(c[0, 1]) + r0)


def gate0(planes, u, v):
    """inittialize_depth_my_version.m:40-45,74-92 at pixel (u, v): (verdict, rho, xyz).  planes = dict(x, y, z (nRows, nCols) filtered, conf or None,
    cmax)"""
    xf, yf, zf = float(planes["x"][v - 1, u - 1]), float(planes["y"][v - 1, u - 1]), float(planes["z"][v - 1, u - 1])
    if xf != xf:
        return NO_DEPTH_NAN, None, None
    df = math.sqrt((xf * xf + yf * yf) + zf * zf)
    if df < 0.4:
        return NO_DEPTH_NEAR, None, None
    if planes.get("conf") is not None and float(planes["conf"][v - 1, u - 1]) <= 0.5 * planes["cmax"]:
        return NO_DEPTH_CONF, None, None
    return GATE_KEPT, 1.0 / df, (-xf, -yf, zf)


def initialize_a_feature(im, planes, uv_pred, centres, strict_reference=True, threshold=10, barrier=20):
    """:55-194 over a table of centres: dict(status, attempts, uv, rho, xyz)"""
    used = 0
    for centre in np.asarray(centres).reshape(-1, 2).tolist()[:MAX_ATTEMPTS]:
        used += 1
        first = box_first_maximum(im, centre, threshold, barrier)
        if first is None or features_in_box(uv_pred, centre, strict_reference):
            continue
        verdict, rho, xyz = gate0(planes, *first)
        return dict(status=INITIALISED if verdict == GATE_KEPT else verdict, attempts=used, uv=first, rho=rho, xyz=xyz)
    return dict(status=NO_BOX, attempts=used, uv=None, rho=None, xyz=None)


def initialize_n_features_fast(im, planes, threshold=5, barrier=20, band=20):
    """initialize_n_features_FAST.m:55-145: the maxima of the image inside the band, each through gate 0: (uv (K, 2), verdict (K,), rho (K,))"""
    a = np.asarray(im)
    c, _ = detect(a, threshold, barrier, 1, band, band, a.shape[0] - 2 * band, a.shape[1] - 2 * band)
    uv = c + band
    verdict, rho = np.zeros(len(uv), np.int32), np.full(len(uv), np.nan)
    for k, (u, v) in enumerate(uv.tolist()):
        verdict[k], r, _ = gate0(planes, u, v)
        if r is not None:
            rho[k] = r
    return uv.astype(np.int32), verdict, rho
