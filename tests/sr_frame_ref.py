"""Two statements of the SR4000 frame conditioning that are not the library's, and the synthetic frames both suites share.

(a) the numpy restatement of the kernels' rule: padded arrays and nine shifted products added in the library's tap order (column-major: dj outer, di
    inner), every product and sum rounded on its own; MATLAB's round and uint8; the two gates vectorised.  The GPU suite compares bit for bit with it.
(b) an independent form: the filter is scipy.ndimage.correlate (mode='constant', cval=0 or mode='nearest'), the keypoint loops are line-by-line
    transliterations of inittialize_depth_my_version.m:16,40-45,74-92 (under SIFT_extract_save.m:71-88) and confidence_filtering.m:1-13.
"""
import numpy as np

SATURATED, MIN_RANGE = 65000.0, 0.4


# ---- MATLAB's scalar rules ---------------------------------------------------------------------------------------------------------------------------
def matlab_round(v):
    """to the nearest integer, halves away from zero; exact (no v + 0.5, which rounds 0.49999999999999994 up); NaN stays NaN"""
    v = np.asarray(v, dtype=np.float64)
    t = np.trunc(v)
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(v - t) >= 0.5, t + np.copysign(1.0, v), t)      # (round(-0.4) is -0, as C's and MATLAB's)


def matlab_uint8(g):
    """uint8(g) as doubles 0 .. 255: rounded half away from zero, saturated, NaN -> 0"""
    r = matlab_round(g)
    with np.errstate(invalid="ignore"):
        return np.where(r > 0.0, np.minimum(r, 255.0), 0.0)


def gauss3(sigma):
    """fspecial('gaussian', [3 3], sigma), closed form: w[3 (j + 1) + (i + 1)], the sum taken column-major and sequentially"""
    h = [np.exp(-(i * i + j * j) / (2.0 * sigma * sigma)) for j in (-1, 0, 1) for i in (-1, 0, 1)]
    s = 0.0
    for v in h:
        s = s + v
    return np.array([v / s for v in h])


def maxima(amp, conf):
    """imax: the largest amplitude <= 65000 (0 when there is none; read_image_sr4000.m:12-17); cmax: MATLAB's max(confidence_map(:))"""
    ok = amp[amp <= SATURATED]
    imax = float(ok.max()) if ok.size else 0.0
    if conf is None or np.isnan(conf).all():
        return imax, float("nan")
    return imax, float(np.nanmax(conf))


# ---- (a) the restatement -----------------------------------------------------------------------------------------------------------------------------
def filter9(p, w, mode):
    """acc = w[0] p[0]; acc = acc + w[k] p[k], k = 1 .. 8, taps column-major (k = 3 (dj + 1) + (di + 1)); mode 0: zero padding, 1: replicate"""
    R, Cn = p.shape
    pad = np.pad(p, 1, mode="constant", constant_values=0.0) if mode == 0 else np.pad(p, 1, mode="edge")
    acc = None
    with np.errstate(invalid="ignore"):
        for dj in range(3):
            for di in range(3):
                t = w[3 * dj + di] * pad[di:di + R, dj:dj + Cn]
                acc = t if acc is None else acc + t
    return acc


def normalise(amp, imax):
    """read_image_sr4000.m:12-21 + normalzie_image.m:4: uint8(sqrt(v) / sqrt(imax) * 255)"""
    v = np.where(amp > SATURATED, imax, amp)
    with np.errstate(invalid="ignore", divide="ignore"):
        g = np.sqrt(v) / np.sqrt(np.float64(imax))
        g = g * 255.0
    return matlab_uint8(g)


def condition(fr, mode, w, filt=filter9):
    """dict(x, y, z, img, conf, imax, cmax) of a frame dict(z, x, y, amp, conf)"""
    imax, cmax = maxima(fr["amp"], fr["conf"])
    out = {k: filt(np.asarray(fr[k], dtype=np.float64), w, mode) for k in ("x", "y", "z")}
    out["img"] = matlab_uint8(filt(normalise(fr["amp"], imax), w, mode))
    out.update(conf=fr["conf"], imax=imax, cmax=cmax)
    return out


def keypoints(cond, frm, des, gate):
    """dict(keep_idx, frames, descriptors[, xyz, rho]) of frm (ldf, K), des (ND, K) on a conditioned frame"""
    frm, des = np.asarray(frm, dtype=np.float64), np.asarray(des, dtype=np.float64)
    r = matlab_round(frm[1]).astype(int) - 1
    c = matlab_round(frm[0]).astype(int) - 1
    conf = None if cond["conf"] is None else cond["conf"][r, c]
    with np.errstate(invalid="ignore", divide="ignore"):
        if gate == 1:
            keep = ~(conf < 0.5 * cond["cmax"])
        else:
            xf, yf, zf = cond["x"][r, c], cond["y"][r, c], cond["z"][r, c]
            s = xf * xf + yf * yf
            df = np.sqrt(s + zf * zf)
            keep = ~np.isnan(xf) & ~(df < MIN_RANGE)
            if conf is not None:
                keep &= ~(conf <= 0.5 * cond["cmax"])
    idx = np.flatnonzero(keep).astype(np.int32)
    out = dict(keep_idx=idx, frames=frm[:, idx], descriptors=des[:, idx])
    if gate == 0:
        with np.errstate(invalid="ignore", divide="ignore"):
            out["xyz"], out["rho"] = np.stack([-xf[idx], -yf[idx], zf[idx]]), 1.0 / df[idx]
    return out


# ---- (b) the independent form ------------------------------------------------------------------------------------------------------------------------
def filter_scipy(p, w, mode):
    from scipy import ndimage
    G = np.asarray(w, dtype=np.float64).reshape(3, 3).T                      # G[i + 1, j + 1] = h(i, j)
    if mode == 0:
        return ndimage.correlate(p, G, mode="constant", cval=0.0)
    return ndimage.correlate(p, G, mode="nearest")


def _round1(v):
    """MATLAB's round for one scalar, in integers of halves: floor(|v|) and the fraction compared with 1/2"""
    import math
    a = abs(v)
    n = math.floor(a)
    n = n + 1 if a - n >= 0.5 else n
    return -n if v < 0 else n


def depth_gate_loop(cond, frm, des):
    """SIFT_extract_save.m:71-88 calling inittialize_depth_my_version.m line by line"""
    import math
    x, y, z, confidence_map = cond["x"], cond["y"], cond["z"], cond["conf"]
    idxRemain, xyz_data, rho = [], [], []
    for idxFrame in range(frm.shape[1]):
        uvd = frm[0:2, idxFrame]
        uv = [uvd[1], uvd[0]]                                               # :16
        if confidence_map is not None:
            max_confidence = np.nan if np.isnan(confidence_map).all() else np.nanmax(confidence_map)      # :32
        ROW, COL = _round1(uv[0]) - 1, _round1(uv[1]) - 1
        if not math.isnan(x[ROW, COL]):                                     # :40
            xf, yf, zf = x[ROW, COL], y[ROW, COL], z[ROW, COL]
            df = np.sqrt(xf ** 2 + yf ** 2 + zf ** 2)                       # :45
        else:
            continue                                                        # :51-54
        if df < 0.4 or (confidence_map is not None and confidence_map[ROW, COL] <= (2 / 4) * max_confidence):           # :74
            continue
        idxRemain.append(idxFrame)                                          # SIFT_extract_save.m:82
        xyz_data.append([-xf, -yf, zf])                                     # :85
        rho.append(1 / np.linalg.norm([-xf, -yf, zf]))                      # :87-92
    idx = np.array(idxRemain, dtype=np.int32)
    return dict(keep_idx=idx, frames=frm[:, idx], descriptors=des[:, idx], xyz=np.array(xyz_data).reshape(-1, 3).T, rho=np.array(rho))


def confidence_filtering_loop(cond, frm, des):
    """confidence_filtering.m:1-13 line by line"""
    confidence_map = cond["conf"]
    max_confidence = np.nan if np.isnan(confidence_map).all() else np.nanmax(confidence_map)
    threshold = 0.5
    idx_to_remove = []
    for i in range(frm.shape[1]):
        ROW, COLUMN = _round1(frm[1, i]) - 1, _round1(frm[0, i]) - 1
        if confidence_map[ROW, COLUMN] < threshold * max_confidence:
            idx_to_remove.append(i)
    idx = np.array([i for i in range(frm.shape[1]) if i not in set(idx_to_remove)], dtype=np.int32)
    return dict(keep_idx=idx, frames=frm[:, idx], descriptors=des[:, idx])


# ---- shared synthetic frames -------------------------------------------------------------------------------------------------------------------------
CMAX = 65534.0                     # 0.5 * CMAX = 32767 exactly


def make_frame(rows, cols, seed=0, conf=True):
    """a seeded frame: ranges of 0.5 .. 4 m, a patch of short ranges, amplitudes with a few saturated pixels, integer confidences up to CMAX"""
    rng = np.random.default_rng(1000 * rows + cols + seed)
    fr = dict(z=rng.uniform(0.5, 4.0, (rows, cols)), x=rng.uniform(-1.5, 1.5, (rows, cols)), y=rng.uniform(-1.0, 1.0, (rows, cols)),
              amp=np.floor(rng.uniform(0.0, 30000.0, (rows, cols))))
    if rows >= 16 and cols >= 16:
        fr["z"][4:12, 4:12] = rng.uniform(0.05, 0.2, (8, 8))
        fr["x"][4:12, 4:12] = rng.uniform(-0.05, 0.05, (8, 8))
        fr["y"][4:12, 4:12] = rng.uniform(-0.05, 0.05, (8, 8))
    sat = rng.random((rows, cols)) < 0.03
    fr["amp"][sat] = 65535.0
    fr["amp"].flat[rng.integers(rows * cols)] = 0.0
    if conf:
        fr["conf"] = np.floor(rng.uniform(0.0, CMAX, (rows, cols)))
        fr["conf"].flat[rng.integers(rows * cols)] = CMAX
    else:
        fr["conf"] = None
    return {k: (None if v is None else np.asfortranarray(v)) for k, v in fr.items()}


# special pixels of make_keypoint_frame (0-based row, column), all far from each other and from the short-range patch
PX_CONF_EQ, PX_R04, PX_RBELOW, PX_NANX, PX_NANY, PX_GOOD, PX_BAD = (20, 30), (50, 60), (60, 80), (70, 100), (80, 120), (100, 140), (110, 150)


def _patch_for(target, w, mode):
    """a 3 x 3 patch of values within a few ulp of 0.4 whose filtered centre is exactly `target` (a seeded search over the restatement)"""
    rng = np.random.default_rng(4)
    ulp = np.spacing(np.float64(0.25))
    for _ in range(20000):
        patch = 0.4 + ulp * rng.integers(-6, 7, (3, 3))
        if filter9(np.pad(patch, 1, mode="edge"), w, mode)[2, 2] == target:
            return patch
    raise AssertionError("no patch gives a filtered range of %r: widen the search" % target)


def make_keypoint_frame(w, mode, seed=7):
    """the 144 x 176 frame of the keypoint cases: make_frame plus pixels whose confidence is exactly half the largest, whose filtered range is exactly
    0.4 and the double just below it (x = y = 0 there: df = |z|), a NaN x, a NaN y alone, and a surely kept and a surely dropped pixel"""
    fr = make_frame(144, 176, seed)
    for (r, c) in (PX_CONF_EQ, PX_R04, PX_RBELOW, PX_NANX, PX_NANY, PX_GOOD):
        fr["conf"][r - 2:r + 3, c - 2:c + 3] = CMAX
    fr["conf"][PX_CONF_EQ] = 0.5 * CMAX
    fr["conf"][PX_BAD] = 0.0
    fr["z"][PX_BAD], fr["x"][PX_BAD] = 3.0, 0.0
    for px, target in ((PX_R04, np.float64(0.4)), (PX_RBELOW, np.nextafter(np.float64(0.4), 0.0))):
        r, c = px
        fr["x"][r - 1:r + 2, c - 1:c + 2] = 0.0
        fr["y"][r - 1:r + 2, c - 1:c + 2] = 0.0
        fr["z"][r - 1:r + 2, c - 1:c + 2] = _patch_for(target, w, mode)
    fr["x"][PX_NANX] = np.nan
    fr["y"][PX_NANY] = np.nan
    return fr


def make_keypoints(K, rows=144, cols=176, ldf=4, ND=128, seed=0, specials=True):
    """frm (ldf, K), des (ND, K): seeded positions whose rounded pixel lies inside the image; the first keypoints (and every 97th after them) sit on the
    special pixels, some at exactly x.5 in both coordinates (which round up, away from zero)"""
    rng = np.random.default_rng(77 * K + seed)
    frm = np.zeros((ldf, K), order="F")
    frm[0] = rng.uniform(0.5, cols + 0.49, K)
    frm[1] = rng.uniform(0.5, rows + 0.49, K)
    frm[2:] = rng.uniform(0.5, 8.0, (ldf - 2, K))
    des = np.asfortranarray(np.floor(rng.uniform(0, 256, (ND, K))))
    if specials and rows == 144 and cols == 176:
        sp = []
        for (r, c) in (PX_CONF_EQ, PX_R04, PX_RBELOW, PX_NANX, PX_NANY, PX_GOOD, PX_BAD):
            sp.append((c + 1.0, r + 1.0))                                   # 1-based, exact
            sp.append((c + 0.5, r + 0.5))                                   # x.5 in both coordinates: rounds to (r + 1, c + 1), the same pixel
            sp.append((c + 1.3, r + 0.7))
        for i in list(range(min(K, len(sp)))) + list(range(len(sp), K, 97)):
            frm[0, i], frm[1, i] = sp[i % len(sp)]
    return frm, des
