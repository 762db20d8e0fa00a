"""Host-side mirror of the reference's floor-plane fit (plane_fit_to_data.m) over the C ABI; DESIGN.md section 17.

    plane_fit_to_data.m:13-21,41        -> crop_points (camera coordinates, the box, the column-major point list)
    plane_fitting/ransac.m:142-176      -> draw_plane_hypotheses (the reference's rejection rule, any numpy Generator)
    plane_fitting/ransac.m:142-176      -> plane_fit_seeded (the same rule on the device, from (seed, seq))
    plane_fit_to_data.m:7-149           -> plane_fit (RANSAC over the draws, refit, sign rule, R), EkfFilter.heading_from_scan in ekf.py
    plane_fit_to_data.m:7-149           -> plane_fit_frame, plane_fit_frame_seeded (the same fit on a resident sr4000.SrFrame: the box is gathered
                                           from its filtered planes on the device), EkfFilter.heading_from_frame in ekf.py

All compute runs in libpre3.so on the GPU; this module marshals numpy arrays and draws random numbers.
"""
import ctypes as C

import numpy as np

from ._lib import Pre3Error, check, dptr, f64, i32, lib

DEFAULT_BOX = (80, 144, 50, 120)          # plane_fit_to_data.m:17-18: rows 80..144, columns 50..120, 1-based inclusive
MAX_DRAWS = 1001                          # ransac.m:209: the loop breaks once trialcount exceeds maxTrials = 1000
MAX_DATA_TRIALS = 100                     # ransac.m:122


class PlaneResult(C.Structure):
    _fields_ = [("B", C.c_double * 4), ("R", C.c_double * 9), ("p_orig", C.c_double * 3), ("p_ray", C.c_double * 3), ("N", C.c_double),
                ("sta", C.c_int32), ("n_inliers", C.c_int32), ("n_trials", C.c_int32), ("best", C.c_int32)]


def crop_points(x_sr, y_sr, z_sr, box=None):
    """plane_fit_to_data.m:13, :19-21, :41: (x1, y1, z1, XYZ) -- the box of the range image in camera coordinates (x = -x_sr, y = -y_sr, z = z_sr)
    and its points stacked column-major, XYZ (3, npts)."""
    r0, r1, c0, c1 = DEFAULT_BOX if box is None else [int(v) for v in box]
    x, y, z = -np.asarray(x_sr, dtype=np.float64), -np.asarray(y_sr, dtype=np.float64), np.asarray(z_sr, dtype=np.float64)
    if not (1 <= r0 <= r1 <= x.shape[0] and 1 <= c0 <= c1 <= x.shape[1]):
        raise Pre3Error(-1, "crop_points: box outside the image")
    x1, y1, z1 = x[r0 - 1:r1, c0 - 1:c1], y[r0 - 1:r1, c0 - 1:c1], z[r0 - 1:r1, c0 - 1:c1]
    return x1, y1, z1, np.stack([x1.ravel(order="F"), y1.ravel(order="F"), z1.ravel(order="F")])


def draw_plane_hypotheses(XYZ, n_draw, rng):
    """ransac.m:142-176, n_draw times: three distinct positions (randsample), redrawn while the points are collinear
    (iscolinear.m:62: norm(cross(p2 - p1, p3 - p1)) < eps), at most 100 times -- the last sample is then kept, as the reference keeps it.
    Returns 0-based positions (n_draw, 3), int32."""
    X = np.asarray(XYZ, dtype=np.float64)
    npts = X.shape[1]
    eps = np.finfo(float).eps
    out = np.zeros((int(n_draw), 3), np.int32)
    for k in range(int(n_draw)):
        for _ in range(MAX_DATA_TRIALS):
            ind = rng.choice(npts, 3, replace=False)
            p1, p2, p3 = X[:, ind[0]], X[:, ind[1]], X[:, ind[2]]
            if not np.linalg.norm(np.cross(p2 - p1, p3 - p1)) < eps:
                break
        out[k] = ind
    return out


def _images(x_sr, y_sr, z_sr):
    imgs = [np.asfortranarray(f64(a)) for a in (x_sr, y_sr, z_sr)]
    if imgs[0].ndim != 2 or any(a.shape != imgs[0].shape for a in imgs):
        raise Pre3Error(-1, "plane fit: x_sr, y_sr, z_sr must be equally sized 2-D range images")
    return imgs


def _box(box):
    return None if box is None else i32(np.asarray(box).ravel())


def _result(res):
    return dict(B=np.array(res.B), R=np.array(res.R).reshape(3, 3, order="F"), p_orig=np.array(res.p_orig), p_ray=np.array(res.p_ray), N=res.N,
                sta=int(res.sta), n_inliers=int(res.n_inliers), n_trials=int(res.n_trials), best=int(res.best))


def _check_frame(rc, res):
    """check() that hands the result block of a refused box to the caller: Pre3Error.result (sta = 5) on PRE3_E_NUMERIC"""
    try:
        check(rc)
    except Pre3Error as e:
        if e.code == -5:
            e.result = _result(res)
        raise


def _fit(who, box, draws, n_draw, call, frame=False):
    """The marshalling of the four fit wrappers: the box and its point count, the output arrays, the call and the result dict.  draws: the supplied
    table (n_draw, 3), or None for a seeded form, whose table of n_draw rows comes back in the dict.  call(box, n_draw, draws, counts, inliers, res)
    makes the library call and returns its status."""
    bx = _box(box)
    if bx is not None and bx.shape[0] != 4:
        raise Pre3Error(-1, "%s: box is (row0, row1, col0, col1)" % who)
    r0, r1, c0, c1 = DEFAULT_BOX if bx is None else bx
    npts = max(0, int(r1) - int(r0) + 1) * max(0, int(c1) - int(c0) + 1)
    seeded = draws is None
    if seeded:
        n_draw = int(n_draw)
        draws = np.zeros((min(max(n_draw, 1), MAX_DRAWS), 3), np.int32)
    else:
        n_draw = draws.shape[0]
    counts, inl = np.zeros(max(draws.shape[0], 1), np.int32), np.zeros(max(npts, 1), np.int32)
    res = PlaneResult()
    rc = call(dptr(bx), n_draw, dptr(draws), dptr(counts), dptr(inl), C.byref(res))
    if frame:
        _check_frame(rc, res)
    else:
        check(rc)
    out = _result(res)
    out["counts"], out["inliers"] = counts[:n_draw], inl[:npts].astype(bool)
    if seeded:
        out["draws"] = draws[:n_draw]
    return out


def plane_fit(x_sr, y_sr, z_sr, draws, box=None, t=0.02, device=0):
    """[R, T] = plane_fit_to_data(idx) on the range image (rows, cols) in SR4000 coordinates; draws (n_draw, 3) 0-based positions in the cropped
    point list (draw_plane_hypotheses).  Returns a dict: R (3, 3), B, p_orig, p_ray, N, sta (1 ok, 0 no inlier, 2 the stopping rule wanted more
    draws, 3 axes undefined), n_inliers, n_trials, best, counts (the score of every draw), inliers (the winner's mask over the cropped points)."""
    imgs = _images(x_sr, y_sr, z_sr)
    rows, cols = imgs[0].shape
    return _fit("plane_fit", box, i32(draws).reshape(-1, 3), None, lambda bx, nd, dr, cnt, inl, res: lib.pre3_plane_fit(
        int(device), rows, cols, dptr(imgs[0]), dptr(imgs[1]), dptr(imgs[2]), bx, float(t), nd, dr, cnt, inl, res))


def plane_fit_seeded(x_sr, y_sr, z_sr, seed, seq=0, n_draw=MAX_DRAWS, box=None, t=0.02, device=0):
    """plane_fit with the draws made on the device from (seed, seq) by ransac.m:142-176's rule: only the box crosses PCIe.
    The dict also carries draws (n_draw, 3)."""
    imgs = _images(x_sr, y_sr, z_sr)
    rows, cols = imgs[0].shape
    return _fit("plane_fit_seeded", box, None, n_draw, lambda bx, nd, dr, cnt, inl, res: lib.pre3_plane_fit_seeded(
        int(device), rows, cols, dptr(imgs[0]), dptr(imgs[1]), dptr(imgs[2]), bx, float(t), nd, int(seed), int(seq), dr, cnt, inl, res))


def plane_fit_frame(frame, draws, box=None, t=0.02):
    """plane_fit on the filtered planes a resident sr4000.SrFrame holds: the box is gathered on the device, only the draw table
    crosses PCIe.  The dict is plane_fit's, bit for bit what plane_fit(*frame.planes()[:3], draws, box, t) returns.  A non-finite coordinate inside the
    box raises Pre3Error with code -5 (PRE3_E_NUMERIC); its .result carries sta = 5."""
    return _fit("plane_fit_frame", box, i32(draws).reshape(-1, 3), None, lambda bx, nd, dr, cnt, inl, res: lib.pre3_plane_fit_frame(
        frame._h, bx, float(t), nd, dr, cnt, inl, res), frame=True)


def plane_fit_frame_seeded(frame, seed, seq=0, n_draw=MAX_DRAWS, box=None, t=0.02):
    """plane_fit_seeded on the filtered planes a resident sr4000.SrFrame holds: nothing crosses PCIe on the way in.  The dict also carries draws."""
    return _fit("plane_fit_frame_seeded", box, None, n_draw, lambda bx, nd, dr, cnt, inl, res: lib.pre3_plane_fit_frame_seeded(
        frame._h, bx, float(t), nd, int(seed), int(seq), dr, cnt, inl, res), frame=True)


def plane_bench(x_sr, y_sr, z_sr, draws, box=None, t=0.02, reps=50, device=0):
    """measurement only: average device time (ms) of one fit -- upload of the box from pinned memory and both launches"""
    imgs = _images(x_sr, y_sr, z_sr)
    draws = i32(draws).reshape(-1, 3)
    ms = C.c_double(0)
    check(lib.pre3_plane_bench(int(device), imgs[0].shape[0], imgs[0].shape[1], dptr(imgs[0]), dptr(imgs[1]), dptr(imgs[2]), dptr(_box(box)), float(t),
                               draws.shape[0], dptr(draws), int(reps), C.byref(ms)))
    return ms.value
