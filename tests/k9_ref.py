"""K9 alone: plain-numpy restatements of the down-date P <- P - W'W, the seeded inputs and the case lists of tests/test_k9_ref.py (CPU),
tests/test_gpu_k9_alone.py (device) and tests/golden/make_k9_tolerance.py (the gate).  Nothing here touches the library.

    exact        P0 - launches * W'W to (far) below the unit roundoff it is measured in
    plain        the same sums in the context's dtype, one row of W at a time, P rounded after every launch: what "f32 accuracy" means
    emulate_b3   the bf16 form restated: three round-to-nearest-even bf16 planes of W, the six plane products of a 16-row stage in the
                 kernel's order, f32 accumulation, P rounded to f32 once per launch.  The tests' own tool (and the carrier of the mutants).
    norm_err     |got - exact|_ij / (u (|P0|_ij + launches (|W|'|W|)_ij)), max and RMS over ALL n x n entries

Two input classes.  Exact: integer W and P0 chosen so that every product, partial sum and result is an integer below 2^24 -- every form in either
dtype must return exact() bit for bit.  Accuracy: columns of W spread over three decades, P0 = 1.5 launches W'W + 1 % noise, so that P is
comparable with the product in every entry and nothing hides behind a large prior.

Two departures from the letter of the plan, both forced by the inputs themselves:
  * the two zero columns of an accuracy W have G_ii = 0; their rows of the noise D take the smallest positive G_ii instead, so that the
    denominator of norm_err stays positive there (the device must return those rows of P0 untouched: error 0);
  * r = 1 has no zero row (W would be zero altogether).
"""
import functools
import math

import numpy as np

U32, U64 = 2.0 ** -24, 2.0 ** -53
SIX = ((0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0))           # B3_MFMAS' order (pre3_update.hip)
MUTANTS = {
    "no(0,2)": tuple(p for p in SIX if p != (0, 2)),
    "no(1,1)": tuple(p for p in SIX if p != (1, 1)),
    "no third plane": tuple(p for p in SIX if 2 not in p),
}
LIMIT = 2 ** 24


def round_up(a, b):
    return (a + b - 1) // b * b


# ---- the library's sizes (pre3_create, launch_downdate), restated
def state_size(N):
    return 13 + 6 * N


def ld_of(cap):
    return round_up(13 + 6 * cap, 128)


def rcap_of(cap):
    return round_up(2 * cap, 64) + 64


def nst_of(r):
    """k-stages of 16 rows k_downdate_b3 runs"""
    return min(round_up(r, 64) // 16, max(4, 2 * -(-r // 32)))


def tiles128(cap, num_cus):
    """(large 128x128 tiles, 64x64 tiles from split left-overs) of k_downdate_b3's list"""
    nt = ld_of(cap) // 128
    total = nt * (nt + 1) // 2
    n_big = total if total <= num_cus else total // num_cus * num_cus
    left, small, n_diag = total - n_big, 0, nt
    for _ in range(left):                                        # diagonal tiles first: three small tiles each, four off the diagonal
        if n_diag > 0:
            small += 3; n_diag -= 1
        else:
            small += 4
    return n_big, small


def tiles64(cap):
    nt = ld_of(cap) // 64
    return nt * (nt + 1) // 2


def x0_of(N):
    """a valid state of N inverse-depth landmarks: identity attitude, rho = 0.5"""
    x = np.zeros(state_size(N))
    x[3] = 1.0
    x[13 + 5::6] = 0.5
    return x


# ---- inputs
def _sym(a):
    u = np.triu(a)
    return u + np.triu(a, 1).T


@functools.lru_cache(maxsize=None)
def exact_case(n, r, launches, planes):
    """(P0, W): integers; |w| <= 255 (planes = 1: one bf16 plane) or <= 511 with odd values above 255 in every column (planes = 2)"""
    rng = np.random.default_rng([9, 1, n, r, launches, planes])
    budget = (LIMIT - 1001) // (3 * launches)                    # sum_k w_k^2 per column: 3 L sum + 1000 < 2^24 bounds |P0| + L |W|'|W|
    nbig = min(2, r) if planes == 2 else 0
    budget -= nbig * 511 * 511
    wmax = min(255, math.isqrt(budget // max(1, r - nbig)))
    assert wmax >= 100
    W = rng.integers(-wmax, wmax + 1, (r, n)).astype(np.float64)
    for j in range(n if nbig else 0):
        rows = rng.choice(r, nbig, replace=False)
        W[rows, j] = (257 + 2 * rng.integers(0, 128, nbig)) * rng.choice((-1.0, 1.0), nbig)
    D = _sym(rng.integers(-1000, 1001, (n, n)).astype(np.float64))
    P0 = 2.0 * launches * (W.T @ W) + D
    assert exact_bound(P0, W, launches) < LIMIT and np.array_equal(P0, P0.T) and (planes == 1 or (np.abs(W) > 255).any())
    for a in (P0, W):
        a.setflags(write=False)
    return P0, W


def exact_bound(P0, W, launches):
    """an upper bound of every product, partial sum (in any order) and result of the exact class"""
    return float((np.abs(P0) + launches * (np.abs(W).T @ np.abs(W))).max())


@functools.lru_cache(maxsize=None)
def accuracy_case(n, r, launches, dtype):
    """(P0, W), both holding values of `dtype` ('f32' / 'f64') in float64 arrays"""
    t = {"f32": np.float32, "f64": np.float64}[dtype]
    rng = np.random.default_rng([9, 2, n, r, launches, 32 if dtype == "f32" else 64])
    W = rng.standard_normal((r, n)) * np.logspace(-2, 1, n)[None, :]
    W[:, rng.choice(n, 2, replace=False)] = 0.0
    if r >= 2:
        W[int(rng.integers(0, r)), :] = 0.0
    W = W.astype(t).astype(np.float64)
    G = W.T @ W
    g = np.diag(G).copy()
    g[g == 0] = g[g > 0].min()
    D = 0.01 * np.sqrt(np.outer(g, g)) * _sym(rng.standard_normal((n, n)))
    P0 = _sym(1.5 * launches * G + D).astype(t).astype(np.float64)
    assert np.array_equal(P0, P0.T) and (np.abs(P0) + launches * (np.abs(W).T @ np.abs(W))).min() > 0, "norm_err's denominator must be positive"
    for a in (P0, W):
        a.setflags(write=False)
    return P0, W


# ---- the restatements
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah = ca - (ca - a); al = a - ah
    bh = cb - (cb - b); bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def exact_wide(P0, W, launches, force_error_free=False):
    """P0 - launches W'W as an unevaluated sum hi + lo of two doubles: np.longdouble where it is wider than double, else error-free sums"""
    n = P0.shape[0]
    if np.finfo(np.longdouble).nmant > 52 and not force_error_free:
        G = np.zeros((n, n), np.longdouble)
        Wl = W.astype(np.longdouble)
        for k in range(W.shape[0]):
            G += np.multiply.outer(Wl[k], Wl[k])
        E = P0.astype(np.longdouble) - launches * G
        hi = E.astype(np.float64)
        return hi, (E - hi).astype(np.float64)
    hi, lo = np.zeros((n, n)), np.zeros((n, n))
    for k in range(W.shape[0]):
        p, e = _two_prod(W[k][:, None], W[k][None, :])
        hi, e2 = _two_sum(hi, p)
        lo += e + e2
    t, e = _two_prod(hi, float(launches))
    rh, e2 = _two_sum(np.asarray(P0, np.float64), -t)
    return _two_sum(rh, e2 - e - launches * lo)


def exact(P0, W, launches):
    """P0 - launches W'W in fp64 (exact for the exact class; 2^-29 of an f32 ulp off otherwise)"""
    return P0 - launches * (W.T @ W)


def plain(P0, W, launches, dtype):
    t = {"f32": np.float32, "f64": np.float64}[dtype]
    P, Wd = P0.astype(t), W.astype(t)
    for _ in range(launches):
        s = np.zeros(P.shape, t)
        for k in range(Wd.shape[0]):
            s += np.multiply.outer(Wd[k], Wd[k])
        P = P - s
    assert P.dtype == t
    return P.astype(np.float64)


def bf16_rne(x):
    """float32 -> the nearest bf16 (ties to even), as float32"""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return ((b + (((b >> 16) & 1) + 0x7FFF)) & 0xFFFF0000).view(np.float32)


def split3(W):
    """the three planes of k_split_w: each the bf16 of the running residual (the residuals are exact in f32)"""
    x = np.ascontiguousarray(W, np.float32)
    a = bf16_rne(x)
    r1 = x - a
    b = bf16_rne(r1)
    return a, b, bf16_rne(r1 - b)


def emulate_b3(P0, W, launches, pairs=SIX):
    r, n = W.shape
    nst = nst_of(r)
    planes = []
    for p in split3(W):
        q = np.zeros((16 * nst, n))
        q[:r] = p
        planes.append(q)
    P = P0.astype(np.float32)
    for _ in range(launches):
        acc = np.zeros((n, n), np.float32)
        for s in range(nst):
            k = slice(16 * s, 16 * s + 16)
            for pa, pb in SIX:
                if (pa, pb) in pairs:                            # one MFMA: 16 exact products summed, added to the f32 accumulator
                    acc = (acc.astype(np.float64) + planes[pa][k].T @ planes[pb][k]).astype(np.float32)
        P = P - acc
    assert P.dtype == np.float32
    return P.astype(np.float64)


def denominator(P0, W, launches):
    return np.abs(P0) + launches * (np.abs(W).T @ np.abs(W))


def norm_err(got, P0, W, launches, u):
    """(max, RMS) of |got - exact| / (u (|P0| + launches |W|'|W|)) over every entry of the n x n block"""
    den = denominator(P0, W, launches)
    assert den.shape == got.shape and (den > 0).all()
    if u == U64:
        hi, lo = exact_wide(P0, W, launches)
        d = np.abs((got - hi) - lo)
    else:
        d = np.abs(got - exact(P0, W, launches))
    e = d / (u * den)
    return float(e.max()), float(np.sqrt(np.mean(e * e)))


# ---- the cases
SHAPES = ((8, 8), (9, 9), (19, 19), (20, 20), (41, 41), (20, 60))            # (N, cap): n = 61, 67, 127, 133, 259 (ld = 384), 133 in ld = 384
ROWS = (1, 2, 31, 33, 64, 65, 96, 97, 129)                                    # nst = 4, 4, 4, 4, 4, 6, 6, 8, 10
MULTI = ((20, 20), (41, 41), (20, 60))                                        # the shapes that also run three launches
FORCED = ((20, 20), (41, 41), (20, 60))                                       # PRE3_K9_FORM children ((20, 60): the only n = 133 that admits r = 129)
SMALL_TILES, ONE_TILE_16 = (468, 468), (340, 340)                             # ld = 2944: 256 + 20 split tiles on 256 CUs; ld = 2176: 595 tiles of 64 x 64


def admitted(cap, rows):
    """the hook refuses round_up(r, 64) above the context's row capacity: r = 129 needs cap >= 33"""
    return [r for r in rows if round_up(r, 64) <= rcap_of(cap)]


def _classes(r):
    return [("exact", 1)] + ([("exact", 2)] if r <= 64 else []) + [("acc", 0)]


def _case(N, cap, r, launches, cls, dtype):
    return dict(N=N, cap=cap, n=state_size(N), r=r, launches=launches, cls=cls[0], planes=cls[1], dtype=dtype)


def group_cases(group, dtype):
    """the cases of one form: 'default' (k_downdate_b3 / k_downdate_1t<double,32,8>), 'small_tiles', 'f32_1t', 'f64_1t16', 'persist', 'forced_1t'"""
    out = []
    if group == "default":
        for N, cap in SHAPES:
            rows = admitted(cap, ROWS) + ([rcap_of(cap)] if (N, cap) == (41, 41) else [])
            out += [_case(N, cap, r, 1, c, dtype) for r in rows for c in _classes(r)]
            if (N, cap) in MULTI:
                out += [_case(N, cap, r, 3, c, dtype) for r in admitted(cap, (2, 65, 129)) for c in (("exact", 1), ("acc", 0))]
    elif group in ("small_tiles", "f64_1t16"):
        N, cap = SMALL_TILES if group == "small_tiles" else ONE_TILE_16
        out = [_case(N, cap, r, 1, c, dtype) for r in (33, 65) for c in _classes(r)]
    elif group == "f32_1t":
        out = [_case(N, cap, r, 1, c, dtype) for N, cap in SHAPES for r in admitted(cap, (1, 64, 65, 129)) for c in _classes(r)]
    elif group in ("persist", "forced_1t"):
        out = [_case(N, cap, r, L, c, dtype) for N, cap in FORCED for r in admitted(cap, (1, 65, 129)) for L in ((1, 3) if group == "persist" else (1,))
               for c in (("exact", 1), ("acc", 0))]
    else:
        raise KeyError(group)
    return out


GROUPS = (("default", "f32"), ("default", "f64"), ("small_tiles", "f32"), ("f32_1t", "f32"), ("f64_1t16", "f64"),
          ("persist", "f32"), ("persist", "f64"), ("forced_1t", "f32"), ("forced_1t", "f64"))


def key_of(c):
    return "n%d_r%d_L%d_%s" % (c["n"], c["r"], c["launches"], c["dtype"])


def accuracy_keys():
    """every accuracy input a device test uses, once: {key: (n, r, launches, dtype)}"""
    keys = {}
    for g, dt in GROUPS:
        for c in group_cases(g, dt):
            if c["cls"] == "acc":
                keys[key_of(c)] = (c["n"], c["r"], c["launches"], c["dtype"])
    return keys


def inputs(c):
    return accuracy_case(c["n"], c["r"], c["launches"], c["dtype"]) if c["cls"] == "acc" else exact_case(c["n"], c["r"], c["launches"], c["planes"])


def judge(c, got, gates):
    """what the device tests assert of one case; returns (list of failures, figures)"""
    P0, W = inputs(c)
    bad, fig = [], {}
    if not np.isfinite(got).all():
        return ["not finite"], fig
    if not np.array_equal(got, got.T):
        bad.append("not bitwise symmetric (%d entries)" % int((got != got.T).sum()))
    if c["cls"] == "exact":
        want = exact(P0, W, c["launches"])
        if not np.array_equal(got, want):
            bad.append("%d entries differ from the exact result, by up to %g" % (int((got != want).sum()), float(np.abs(got - want).max())))
    else:
        g = gates[key_of(c)]
        mx, rms = norm_err(got, P0, W, c["launches"], U32 if c["dtype"] == "f32" else U64)
        fig = dict(max=mx, rms=rms, plain_max=g["plain_max"], plain_rms=g["plain_rms"])
        if not mx <= g["gate_max"]:
            bad.append("max %.3g u above the gate %.3g (plain: %.3g)" % (mx, g["gate_max"], g["plain_max"]))
        if not rms <= g["gate_rms"]:
            bad.append("RMS %.3g u above the gate %.3g (plain: %.3g)" % (rms, g["gate_rms"], g["plain_rms"]))
    return bad, fig
