"""Two statements of the 3 x 3 median and of the bad-pixel compensation in front of the frame's Gaussian that are not the
library's, and the planted frames both suites share.

(a) numpy: np.pad(.., 1, mode='symmetric' | 'constant'), the nine shifted views stacked, np.sort(axis=0)[4]; the NaN rule by np.isnan(..).any(0);
    compensate as np.where(conf < cutoff, med, plane); the conditioned frame of (mode, form) by feeding the compensated planes and image to
    tests/sr_frame_ref.py's filter9 / normalise / maxima.
(b) scipy.ndimage.median_filter(size=3, mode='reflect') for 'symmetric', (size=3, mode='constant', cval=0) for zeros.

A median is a selection: "equal" means equal as values (-0 equals +0) with NaNs in the same places -- same().
"""
import numpy as np

import sr_frame_ref as sr

NONE, BADPIXEL, IMAGE_MEDIAN = 0, 1, 2
SIZES = ((1, 1), (1, 5), (5, 1), (2, 2), (3, 3), (17, 70))          # (17, 70) crosses the tile rows 15 | 16 and the tile columns at 16, 32, 48, 64
CUTOFF = 3000.0


def same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.array_equal(a, b, equal_nan=True))


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------------------------
def medfilt3(a, padding):
    """medfilt2(a, [3 3]) (padding 'zeros') or medfilt2(a, [3 3], 'symmetric'); a NaN in the window makes the pixel NaN"""
    a = np.asarray(a, dtype=np.float64)
    R, Cn = a.shape
    pad = np.pad(a, 1, mode="symmetric") if padding == "symmetric" else np.pad(a, 1, mode="constant", constant_values=0.0)
    st = np.stack([pad[di:di + R, dj:dj + Cn] for dj in range(3) for di in range(3)])
    nan = np.isnan(st).any(0)
    return np.where(nan, np.nan, np.sort(st, axis=0)[4])


def bad_mask(conf, cutoff, shape):
    if conf is None:
        return np.zeros(shape, bool)
    with np.errstate(invalid="ignore"):
        return np.asarray(conf) < cutoff                                    # strictly; NaN compares false


def compensate(plane, conf, cutoff):
    """compensate_badpixel_soonhac.m:6-14 for one plane: the median of the plane AS GIVEN where conf < cutoff"""
    plane = np.asarray(plane, dtype=np.float64)
    return np.where(bad_mask(conf, cutoff, plane.shape), medfilt3(plane, "symmetric"), plane)


def compensate_sequential(plane, conf, cutoff):
    """what the rule is NOT: the bad pixels replaced one after the other (column-major), each median seeing the replacements before it"""
    p = np.array(plane, dtype=np.float64)
    bad = bad_mask(conf, cutoff, p.shape)
    for c in range(p.shape[1]):
        for r in range(p.shape[0]):
            if bad[r, c]:
                p[r, c] = medfilt3(p, "symmetric")[r, c]
    return p


def condition(fr, mode, w, form, cutoff=CUTOFF):
    """sr_frame_ref.condition under a compensation: dict(x, y, z, img, conf, imax, cmax, n_bad)"""
    imax, cmax = sr.maxima(fr["amp"], fr["conf"])
    planes = {k: np.asarray(fr[k], dtype=np.float64) for k in ("x", "y", "z")}
    U = sr.normalise(fr["amp"], imax)
    n_bad = 0
    if form == BADPIXEL:
        planes = {k: compensate(p, fr["conf"], cutoff) for k, p in planes.items()}
        U = compensate(U, fr["conf"], cutoff)
        n_bad = int(bad_mask(fr["conf"], cutoff, U.shape).sum())
    elif form == IMAGE_MEDIAN:
        U = medfilt3(U, "zeros")
    out = {k: sr.filter9(p, w, mode) for k, p in planes.items()}
    out["img"] = sr.matlab_uint8(sr.filter9(U, w, mode))
    out.update(conf=fr["conf"], imax=imax, cmax=cmax, n_bad=n_bad)
    return out


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------------------------
def medfilt3_scipy(a, padding):
    from scipy import ndimage
    a = np.asarray(a, dtype=np.float64)
    if padding == "symmetric":
        return ndimage.median_filter(a, size=3, mode="reflect")
    return ndimage.median_filter(a, size=3, mode="constant", cval=0.0)


# ---- shared planted frames ---------------------------------------------------------------------------------------------------------------------------
def planted_pixels(rows, cols):
    """(bad, block, at_cutoff, nan_conf): the 0-based pixels planted bad -- the four corners, the middle of each edge, rows and columns 15, 16, 17 where
    the frame has them, a 2 x 2 block of adjacent ones -- and one pixel each whose confidence is exactly the cut-off and NaN (neither is bad)"""
    rm, cm = rows // 2, cols // 2
    bad = {(0, 0), (0, cols - 1), (rows - 1, 0), (rows - 1, cols - 1), (0, cm), (rows - 1, cm), (rm, 0), (rm, cols - 1)}
    for k in (15, 16, 17):
        if k < rows:
            bad |= {(k, min(3, cols - 1)), (k, cm)}
        if k < cols:
            bad |= {(min(3, rows - 1), k), (rm, k)}
        if k < rows and k < cols:
            bad.add((k, k))
    block, at_cutoff, nan_conf = [], None, None
    if rows >= 12 and cols >= 60:
        r0, c0 = 5, 40
        block = [(r0, c0), (r0 + 1, c0), (r0, c0 + 1), (r0 + 1, c0 + 1)]
        bad |= set(block)
        at_cutoff, nan_conf = (3, 50), (10, 20)
        bad -= {at_cutoff, nan_conf}
    return sorted(bad), block, at_cutoff, nan_conf


def planted_frame(rows, cols, seed=0, cutoff=CUTOFF):
    """sr_frame_ref.make_frame with every confidence above the cut-off except at planted_pixels: those are flying pixels (confidence below the cut-off,
    range off by metres).  Returns (frame, n_bad)."""
    fr = sr.make_frame(rows, cols, seed)
    fr["conf"] = np.asfortranarray(cutoff + 1.0 + np.floor(fr["conf"] / 2.0))
    bad, block, at_cutoff, nan_conf = planted_pixels(rows, cols)
    rng = np.random.default_rng(31 * rows + cols + seed)
    for (r, c) in bad:
        fr["conf"][r, c] = np.floor(rng.uniform(0.0, cutoff))
        fr["z"][r, c] += rng.uniform(3.0, 6.0)
        fr["x"][r, c] -= rng.uniform(3.0, 6.0)
        fr["y"][r, c] += rng.uniform(3.0, 6.0)
        fr["amp"][r, c] = 0.0
    if bad:
        fr["conf"][bad[0]] = np.nextafter(cutoff, 0.0)                       # the double just below the cut-off: bad
    if at_cutoff is not None:
        fr["conf"][at_cutoff] = cutoff
        fr["conf"][nan_conf] = np.nan
        for px in (at_cutoff, nan_conf):
            fr["z"][px] += 4.0
    return fr, len(bad)
