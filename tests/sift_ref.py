"""sift_vedal(I) restated statement by statement in numpy: the oracle of the device extractor (3pre_amd/csrc/pre3_sift.h, pre3_sift.hip).

    sift/sift_vedal.m:127-323        -> sift_vedal          sift/gaussianss.m:72-227    -> plan, double_size, gaussianss
    sift/diffss.m:57-66              -> diffss              sift/imsmooth.c:44-80,128-160 -> taps, imsmooth (econvolve: PAD_BY_CONTINUITY is defined)
    sift/siftlocalmax.c:229-249      -> siftlocalmax        sift/siftrefinemx.c:150-303 -> siftrefinemx
    sift/siftormx.c:138-253          -> siftormx            sift/siftdescriptor.c:310-513 -> siftdescriptor

The stages a test pins bit for bit -- the plan, doubleSize, the smoothing, the differences, the extrema, the boundary test, the refinement -- use one
product or one sum per rounding, and take every constant one value at a time from math.exp / math.pow / math.sqrt (numpy's vectorised forms are other
implementations with other last bits).  Orientation and descriptor are vectorised per keypoint: they are compared within a tolerance.

Switches for tests/golden/make_sift_tolerance.py: jitter=rng moves every transcendental result (pow, exp, atan2, sqrt, fmod, sin, cos; double or float
as the call site has it) by a random -2 .. +2 ulp, shuffle=rng sums every histogram in a random sample order.  margins=dict collects the smallest
margin of every discrete decision behind a transcendental."""
import math

import numpy as np

S, OMIN, SMIN, SMAX = 3, -1, -1, 4
NLEV, NDOG = SMAX - SMIN + 1, SMAX - SMIN
SIGMAN, THRESH, R, MAGNIF, NBP, NBO, NBINS = 0.5, 0.04 / 3 / 2, 10.0, 3.0, 4, 8, 36
TWO_PI = 2 * math.pi
F32 = np.float32
SEEDS = {(69, 85): 11, (144, 176): 12, (37, 45): 13}      # the committed test images


def make_image(M, N, seed=None):
    """three octaves of smoothed noise, summed, scaled to 0 .. 255 and rounded: a generic texture"""
    rng = np.random.default_rng(SEEDS[(M, N)] if seed is None else seed)
    out = np.zeros((M, N))
    for sg in (1.5, 3.0, 6.0):
        a = rng.standard_normal((M + 48, N + 48))
        g = np.exp(-0.5 * (np.arange(-24, 25) / sg) ** 2)
        g /= g.sum()
        a = np.apply_along_axis(lambda v: np.convolve(v, g, "same"), 0, a)
        a = np.apply_along_axis(lambda v: np.convolve(v, g, "same"), 1, a)[24:-24, 24:-24]
        out += a / a.std()
    out = (out - out.min()) / (out.max() - out.min()) * 255.0
    return np.asfortranarray(np.floor(out + 0.5))


def fine_texture(M, N, seed=5, sg=1.2):
    """noise smoothed at sigma 1.2 pixels, scaled to 0 .. 255 and rounded: about 0.047 keypoints and 0.037 refined points per pixel -- the densest
    input found, for the overflow tests (512 x 512 passes PRE3_SR_MAX_KEYPOINTS, 1100 x 1100 passes PRE3_SIFT_MAX_CANDIDATES)"""
    a = np.random.default_rng(seed).standard_normal((M + 16, N + 16))
    g = np.exp(-0.5 * (np.arange(-8, 9) / sg) ** 2)
    g /= g.sum()
    for axis in (0, 1):
        a = sum(g[t] * np.roll(a, 8 - t, axis=axis) for t in range(17))
    a = a[8:-8, 8:-8]
    a = (a - a.min()) / (a.max() - a.min()) * 255.0
    return np.asfortranarray(np.floor(a + 0.5))


def taps(s):
    """imsmooth.c:130-142: (sigma, W, [2 W + 1 taps]); sigma <= 0.01: a copy (W = 0, no taps)"""
    if not s > 0.01:
        return (s, 0, [])
    W = int(math.ceil(4 * s))
    g, acc = [], 0.0
    for j in range(2 * W + 1):
        g.append(math.exp(-0.5 * (j - W) * (j - W) / (s * s)))
        acc += g[-1]
    return (s, W, [v / acc for v in g])


def plan(M, N):
    """sift_vedal.m:127-133, gaussianss.m:72-80,133-203: O, the octave sizes, sigma0, 2^(s/S) for s = smin .. smax - 1, and the taps of every level"""
    O = int(math.floor(math.log2(min(M, N)))) - OMIN - 3
    rows, cols, m, n = [], [], 2 * M, 2 * N
    for _ in range(O):
        rows.append(m); cols.append(n)
        m, n = (m + 1) // 2, (n + 1) // 2
    k = math.pow(2.0, 1.0 / S)
    sigma0 = 1.6 * k
    dsigma0 = sigma0 * math.sqrt(1 - 1 / math.pow(k, 2.0))
    first = math.sqrt(math.pow(sigma0 * math.pow(k, SMIN), 2.0) - math.pow(SIGMAN / math.pow(2.0, OMIN), 2.0))
    sbest = min(SMIN + S, SMAX)
    target, prev = sigma0 * math.pow(k, SMIN), sigma0 * math.pow(k, sbest - S)
    later = math.sqrt(math.pow(target, 2.0) - math.pow(prev, 2.0)) if target > prev else 0.0
    rest = [taps(math.pow(k, float(s)) * dsigma0) for s in range(SMIN + 1, SMAX + 1)]
    lev = [[taps(first if o == 0 else later)] + rest for o in range(O)]
    return dict(O=O, rows=rows, cols=cols, sigma0=sigma0, pow2=[math.pow(2.0, (SMIN + i) / S) for i in range(NDOG)], lev=lev, sbest=sbest - SMIN)


def _u8(v):
    return np.minimum(np.floor(v + 0.5), 255.0)


def double_size(I, strict):
    """gaussianss.m:210-224; strict: I is uint8, so every 0.25 I / 0.5 I term is rounded and the sums saturate, left to right"""
    I = np.asarray(I, dtype=np.float64)
    M, N = I.shape
    J = np.zeros((2 * M, 2 * N), order="F")
    J[0::2, 0::2] = I
    t = (lambda a: _u8(a)) if strict else (lambda a: a)
    add = (lambda a, b: np.minimum(a + b, 255.0)) if strict else (lambda a, b: a + b)
    J[1:-1:2, 1:-1:2] = add(add(add(t(0.25 * I[:-1, :-1]), t(0.25 * I[1:, :-1])), t(0.25 * I[:-1, 1:])), t(0.25 * I[1:, 1:]))
    J[1:-1:2, 0::2] = add(t(0.5 * I[:-1, :]), t(0.5 * I[1:, :]))
    J[0::2, 1:-1:2] = add(t(0.5 * I[:, :-1]), t(0.5 * I[:, 1:]))
    return J


def imsmooth(I, lev):
    """imsmooth.c:128-160 with econvolve (:44-80): along the columns, then along the rows; acc = 0.0, taps ascending, the ends continued"""
    s, W, g = lev
    if not s > 0.01:
        return np.array(I, order="F")
    out = I
    for axis in (0, 1):
        n = out.shape[axis]
        acc = np.zeros_like(out)
        for t in range(2 * W + 1):
            idx = np.clip(np.arange(n) - W + t, 0, n - 1)
            p = g[t] * np.take(out, idx, axis=axis)
            acc = acc + p
        out = acc
    return np.asfortranarray(out)


def gaussianss(I, strict, pl):
    """gaussianss.m:93-203 -> [octave (M, N, 6)]"""
    cur = double_size(I, strict)
    out = []
    for o in range(pl["O"]):
        if o > 0:
            cur = np.asfortranarray(out[-1][0::2, 0::2, pl["sbest"]])
        M, N = cur.shape
        assert (M, N) == (pl["rows"][o], pl["cols"][o])
        G = np.zeros((M, N, NLEV), order="F")
        G[:, :, 0] = imsmooth(cur, pl["lev"][o][0])
        for l in range(1, NLEV):
            G[:, :, l] = imsmooth(G[:, :, l - 1], pl["lev"][o][l])
        out.append(G)
    return out


def diffss(gss):
    return [np.asfortranarray(G[:, :, 1:] - G[:, :, :-1]) for G in gss]


def siftlocalmax(F, threshold):
    """siftlocalmax.c:229-249: 0-based column-major linear indices, ascending, of the interior points >= threshold and > all 26 neighbours"""
    M, N, L = F.shape
    v = F[1:-1, 1:-1, 1:-1]
    mask = v >= threshold
    for ds in (-1, 0, 1):
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                if ds or dx or dy:
                    mask &= v > F[1 + dy:M - 1 + dy, 1 + dx:N - 1 + dx, 1 + ds:L - 1 + ds]
    y, x, s = np.nonzero(mask)
    return np.sort((y + 1) + (x + 1) * M + (s + 1) * M * N)


_PIVOT_FLOOR = float(np.float32(1e-10))


def refine_one(D, x, y, s, threshold=THRESH, r=R):
    """siftrefinemx.c:150-303 for one point (s counted from the first DoG level): None or (xn, yn, sn + smin)"""
    M, N, SS = D.shape
    if x < 1 or x > N - 2 or y < 1 or y > M - 2 or s < 1 or s > SS - 2:
        return None
    dx = dy = 0
    b = [0.0, 0.0, 0.0]
    for _ in range(5):
        x += dx; y += dy
        at = lambda ax, ay, as_: float(D[y + ay, x + ax, s + as_])
        Dx = 0.5 * (at(1, 0, 0) - at(-1, 0, 0)); Dy = 0.5 * (at(0, 1, 0) - at(0, -1, 0)); Ds = 0.5 * (at(0, 0, 1) - at(0, 0, -1))
        Dxx = at(1, 0, 0) + at(-1, 0, 0) - 2.0 * at(0, 0, 0)
        Dyy = at(0, 1, 0) + at(0, -1, 0) - 2.0 * at(0, 0, 0)
        Dss = at(0, 0, 1) + at(0, 0, -1) - 2.0 * at(0, 0, 0)
        Dxy = 0.25 * (at(1, 1, 0) + at(-1, -1, 0) - at(-1, 1, 0) - at(1, -1, 0))
        Dxs = 0.25 * (at(1, 0, 1) + at(-1, 0, -1) - at(-1, 0, 1) - at(1, 0, -1))
        Dys = 0.25 * (at(0, 1, 1) + at(0, -1, -1) - at(0, -1, 1) - at(0, 1, -1))
        A = [[Dxx, Dxy, Dxs], [Dxy, Dyy, Dys], [Dxs, Dys, Dss]]      # A[i][j]
        b = [-Dx, -Dy, -Ds]
        for j in range(3):
            maxa, maxabsa, maxi = 0.0, 0.0, -1
            for i in range(j, 3):
                a = A[i][j]
                absa = a if a > 0 else -a
                if absa > maxabsa:
                    maxa, maxabsa, maxi = a, absa, i
            if maxabsa < _PIVOT_FLOOR:
                b = [0.0, 0.0, 0.0]
                break
            i = maxi
            for jj in range(j, 3):
                A[i][jj], A[j][jj] = A[j][jj], A[i][jj]
                A[j][jj] = A[j][jj] / maxa
            b[j], b[i] = b[i], b[j]
            b[j] = b[j] / maxa
            for ii in range(j + 1, 3):
                xx = A[ii][j]
                for jj in range(j, 3):
                    A[ii][jj] = A[ii][jj] - xx * A[j][jj]
                b[ii] = b[ii] - xx * b[j]
        for i in (2, 1):
            xx = b[i]
            for ii in range(i - 1, -1, -1):
                b[ii] = b[ii] - xx * A[ii][i]
        dx = (1 if (b[0] > 0.6 and x < N - 2) else 0) + (-1 if (b[0] < -0.6 and x > 1) else 0)
        dy = (1 if (b[1] > 0.6 and y < M - 2) else 0) + (-1 if (b[1] < -0.6 and y > 1) else 0)
        if dx == 0 and dy == 0:
            break
    val = float(D[y, x, s]) + 0.5 * (Dx * b[0] + Dy * b[1] + Ds * b[2])
    det = Dxx * Dyy - Dxy * Dxy
    with np.errstate(all="ignore"):
        score = float(np.float64((Dxx + Dyy) * (Dxx + Dyy)) / np.float64(det))
    xn, yn, sn = x + b[0], y + b[1], s + b[2]
    if (abs(val) > threshold and score < (r + 1) * (r + 1) / r and score >= 0 and abs(b[0]) < 1.5 and abs(b[1]) < 1.5 and abs(b[2]) < 1.5
            and 0 <= xn <= N - 1 and 0 <= yn <= M - 1 and 0 <= sn <= SS - 1):
        return (xn, yn, sn + SMIN)
    return None


class _Opts:
    def __init__(self, jitter=None, shuffle=None, margins=None):
        self.jitter, self.shuffle, self.margins = jitter, shuffle, margins

    def j(self, v):
        """a transcendental's result moved by -2 .. +2 ulp of its own format"""
        if self.jitter is None:
            return v
        a = np.asarray(v)
        k = self.jitter.integers(-2, 3, a.shape)
        for _ in range(2):
            a = np.where(k > 0, np.nextafter(a, a.dtype.type(np.inf)), np.where(k < 0, np.nextafter(a, a.dtype.type(-np.inf)), a))
            k = k - np.sign(k)
        return a if a.shape else a[()]

    def order(self, n):
        return np.arange(n) if self.shuffle is None else self.shuffle.permutation(n)

    def margin(self, key, v):
        if self.margins is not None and np.size(v):
            self.margins[key] = min(self.margins.get(key, np.inf), float(np.min(v)))


def _frac_margin(q):
    return np.minimum(q - np.floor(q), np.ceil(q) - q) if np.all(np.floor(q) != q) else np.zeros(1)


def orient_one(G, x, y, s, sigma0, op=_Opts(), raw=None):
    """siftormx.c:139-253 for one refined point of the octave G (M, N, 6): the list of its orientations, in bin order (empty: dropped)"""
    M, N, L = G.shape
    xi, yi, si = int(x + 0.5), int(y + 0.5), int(s + 0.5) - SMIN
    sigmaw = 1.5 * sigma0 * float(op.j(np.float64(math.pow(2.0, s / S))))
    W = int(math.floor(3.0 * sigmaw))
    op.margin("orient_W", _frac_margin(np.float64(3.0 * sigmaw)) / (3.0 * sigmaw))
    if xi < 0 or xi > N - 1 or yi < 0 or yi > M - 1 or si < 0 or si > L - 1:
        return []
    xs, ys = np.meshgrid(np.arange(max(-W, 1 - xi), min(W, N - 2 - xi) + 1), np.arange(max(-W, 1 - yi), min(W, M - 2 - yi) + 1), indexing="ij")
    xs, ys = xs.ravel(), ys.ravel()                       # xs outer, ys inner: the reference's order
    P = G[:, :, si]
    Dx = 0.5 * (P[yi + ys, xi + xs + 1] - P[yi + ys, xi + xs - 1]); Dy = 0.5 * (P[yi + ys + 1, xi + xs] - P[yi + ys - 1, xi + xs])
    dx, dy = (xi + xs).astype(np.float64) - x, (yi + ys).astype(np.float64) - y
    r2 = dx * dx + dy * dy
    keep = ~(r2 >= W * W + 0.5)
    Dx, Dy, r2 = Dx[keep], Dy[keep], r2[keep]
    win = op.j(np.exp(-r2 / (2 * sigmaw * sigmaw)))
    mod = op.j(np.sqrt(Dx * Dx + Dy * Dy))
    theta = op.j(np.fmod(op.j(np.arctan2(Dy, Dx)) + TWO_PI, TWO_PI))
    q = NBINS * theta / TWO_PI
    amount = mod * win
    op.margin("orient_bin", _frac_margin(q[amount != 0]) if np.any(amount != 0) else [])
    bins = np.minimum(q.astype(np.int64), NBINS - 1)
    H = np.zeros(NBINS)
    o = op.order(len(bins))
    np.add.at(H, bins[o], amount[o])
    H = [float(v) for v in H]
    if raw is not None:
        raw.extend(H)                                     # the histogram before the smoother, for the tests
    for _ in range(6):                                    # in place: bin 35 reads the NEW bin 0, so the smoother is not circularly symmetric
        prev = H[NBINS - 1]
        for i in range(NBINS):
            nh = (prev + H[i] + H[(i + 1) % NBINS]) / 3.0
            prev = H[i]
            H[i] = nh
    maxh = max(H)
    out = []
    for i in range(NBINS):
        h0, hm, hp = H[i], H[(i - 1) % NBINS], H[(i + 1) % NBINS]
        if maxh > 0:      # the margin of the conjunction: a peak stands by its weakest condition, a non-peak falls by its clearest failure
            conds = [(h0 > 0.8 * maxh, abs(h0 - 0.8 * maxh) / maxh), (h0 > hm, abs(h0 - hm) / maxh), (h0 > hp, abs(h0 - hp) / maxh)]
            op.margin("peak", [min(m for _, m in conds)] if all(c for c, _ in conds) else [max(m for c, m in conds if not c)])
        if h0 > 0.8 * maxh and h0 > hm and h0 > hp:
            di = -0.5 * (hp - hm) / (hp + hm - 2 * h0)
            out.append(TWO_PI * (i + di + 0.5) / NBINS)
    return out


def _fast_mod(th, op):
    th = th.copy()
    for _ in range(4):
        th = np.where(th < 0, (th.astype(np.float64) + TWO_PI).astype(F32), th)
    for _ in range(4):
        th = np.where(th.astype(np.float64) > TWO_PI, (th.astype(np.float64) - TWO_PI).astype(F32), th)
    return th


def _fast_floor(v):
    return (v - np.where(v >= 0, F32(0), F32(1)).astype(F32)).astype(np.int64)      # the cast truncates


def descriptor_one(G, x, y, s, theta0, sigma0, op=_Opts()):
    """siftdescriptor.c:381-513 for one oriented point of the octave G: 128 doubles (zeros when the point is out of bounds)"""
    M, N, L = G.shape
    x, y, s, theta0 = F32(x), F32(y), F32(s), F32(theta0)
    st0, ct0 = F32(op.j(np.sin(theta0))), F32(op.j(np.cos(theta0)))
    xi, yi = int(math.floor(float(x) + 0.5)), int(math.floor(float(y) + 0.5))
    si = int(math.floor(float(s) + 0.5)) - SMIN
    sigma = F32(sigma0) * F32(op.j(np.power(F32(2), s / F32(S))))
    SBP = F32(MAGNIF) * sigma
    Wf = math.sqrt(2.0) * float(SBP) * (NBP + 1) / 2.0 + 0.5
    W = int(math.floor(Wf))
    op.margin("desc_W", _frac_margin(np.float64(Wf)) / Wf)
    d = np.zeros(128, F32)
    if xi < 0 or xi > N - 1 or yi < 0 or yi > M - 1 or si < 0 or si > L - 1:
        return d.astype(np.float64)
    dxi, dyi = np.meshgrid(np.arange(max(-W, 1 - xi), min(W, N - 2 - xi) + 1), np.arange(max(-W, 1 - yi), min(W, M - 2 - yi) + 1), indexing="ij")
    dxi, dyi = dxi.ravel(), dyi.ravel()
    P = G[:, :, si]
    Dx = (0.5 * (P[yi + dyi, xi + dxi + 1] - P[yi + dyi, xi + dxi - 1])).astype(F32)
    Dy = (0.5 * (P[yi + dyi + 1, xi + dxi] - P[yi + dyi - 1, xi + dxi])).astype(F32)
    mod = op.j(np.sqrt(Dx * Dx + Dy * Dy))
    angle = np.where(mod > 0, op.j(np.arctan2(Dy, Dx)), F32(0)).astype(F32)
    theta = _fast_mod(-angle + theta0, op)
    dx, dy = (xi + dxi).astype(F32) - x, (yi + dyi).astype(F32) - y
    nx = (ct0 * dx + st0 * dy) / SBP
    ny = (-st0 * dx + ct0 * dy) / SBP
    nt = ((F32(NBO) * theta).astype(np.float64) / TWO_PI).astype(F32)
    win = op.j(np.exp(((-(nx * nx + ny * ny)).astype(np.float64) / 8.0).astype(F32)))
    binx, biny, bint = _fast_floor((nx.astype(np.float64) - 0.5).astype(F32)), _fast_floor((ny.astype(np.float64) - 0.5).astype(F32)), _fast_floor(nt)
    rbinx = (nx.astype(np.float64) - (binx + 0.5)).astype(F32); rbiny = (ny.astype(np.float64) - (biny + 0.5)).astype(F32)
    rbint = nt - bint.astype(F32)
    idx, wts = [], []
    for dbx in (0, 1):
        for dby in (0, 1):
            for dbt in (0, 1):
                okb = (binx + dbx >= -2) & (binx + dbx < 2) & (biny + dby >= -2) & (biny + dby < 2)
                w = win * mod * np.abs(F32(1 - dbx) - rbinx) * np.abs(F32(1 - dby) - rbiny) * np.abs(F32(1 - dbt) - rbint)
                idx.append(np.where(okb, ((bint + dbt) % NBO) + NBO * ((binx + dbx + 2) + NBP * (biny + dby + 2)), -1))
                wts.append(w.astype(F32))
    idx, wts = np.stack(idx, 1), np.stack(wts, 1)          # sample-major, the eight bins in the reference's order
    o = op.order(idx.shape[0])
    idx, wts = idx[o].ravel(), wts[o].ravel()
    np.add.at(d, idx[idx >= 0], wts[idx >= 0])
    for ps in range(2):
        norm = F32(0)
        for v in d:
            norm = F32(norm + F32(v * v))
        norm = F32(op.j(np.sqrt(norm)))
        d = (d / F32(norm + F32(np.finfo(F32).eps))).astype(F32)
        if ps == 0:
            d = np.where(d.astype(np.float64) > 0.2, F32(0.2), d).astype(F32)
    return d.astype(np.float64)


def sift_vedal(I, strict=True, pl=None, jitter=None, shuffle=None, margins=None, descriptors=True):
    """[frames, descriptors, gss, dogss] = sift_vedal(I) plus what the tests compare: counts (O, 4) = maxima, inside the boundary, refined, oriented;
    refined = [per octave (3, n)]; npeaks = [per octave (n,)]; octave_of (K,)"""
    I = np.asarray(I, dtype=np.float64)
    pl = plan(*I.shape) if pl is None else pl
    op = _Opts(jitter, shuffle, margins)
    gss = gaussianss(I, strict, pl)
    dogss = diffss(gss)
    sigma0 = pl["sigma0"]
    frames, des, counts, refined, npeaks, octave_of = [], [], [], [], [], []
    for o in range(pl["O"]):
        D, G = dogss[o], gss[o]
        M, N, _ = D.shape
        idx = np.concatenate([siftlocalmax(D, 0.8 * THRESH), siftlocalmax(-D, 0.8 * THRESH)])
        yy, xx, ss = idx % M, (idx // M) % N, idx // (M * N)
        ins = []
        for x, y, s in zip(xx, yy, ss):                    # sift_vedal.m:259-265 (s here counts from the first DoG level: pow2[s] = 2^((s + smin) / S))
            rad = MAGNIF * sigma0 * pl["pow2"][s] * NBP / 2
            if x - rad >= 1 and x + rad <= N and y - rad >= 1 and y + rad <= M:
                ins.append((int(x), int(y), int(s)))
        ref = [q for q in (refine_one(D, *p) for p in ins) if q is not None]
        pk = [orient_one(G, q[0], q[1], q[2], sigma0, op) for q in ref]
        sc = 2.0 ** (o + OMIN)
        for q, ths in zip(ref, pk):
            for th in ths:
                frames.append((sc * q[0], sc * q[1], sc * sigma0 * float(op.j(np.float64(math.pow(2.0, q[2] / S)))), th))
                octave_of.append(o)
                if descriptors:
                    des.append(descriptor_one(G, q[0], q[1], q[2], th, sigma0, op))
        counts.append((len(idx), len(ins), len(ref), sum(len(t) for t in pk)))
        refined.append(np.array(ref, dtype=np.float64).reshape(-1, 3).T)
        npeaks.append(np.array([len(t) for t in pk], dtype=np.int64))
    K = len(frames)
    return dict(frames=np.asfortranarray(np.array(frames, dtype=np.float64).reshape(K, 4).T),
                descriptors=np.asfortranarray(np.array(des, dtype=np.float64).reshape(len(des), 128).T), gss=gss, dogss=dogss,
                counts=np.array(counts, dtype=np.int64).reshape(-1, 4), refined=refined, npeaks=npeaks, octave_of=np.array(octave_of, dtype=np.int64), plan=pl)
