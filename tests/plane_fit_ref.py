"""CPU truth of the floor-plane fit (pre3_plane_fit / pre3_heading_from_scan): plane_fit_to_data.m restated in numpy.

scene(seed, outl)                     a seeded SR4000-like range image of a floor under a pitched camera (the test scenes)
crop(x_sr, y_sr, z_sr, box)           plane_fit_to_data.m:13, :17-21, :41
plane_dist(P, X)                      plane_fitting/ransacfitplane.m:90-103 (the three products and sums in the reference's order, no contraction)
replay(counts, npts)                  plane_fitting/ransac.m:127-133, :135-215 on a list of scores
fitplane(X)                           plane_fitting/fitplane.m:47-54 (SVD form, as the reference)
line_plane(B, p)                      plane_fitting/plane_imp_line_par_int_3d.m:56-100 for a ray from the origin
axes(B, p_orig, p_ray)                plane_fit_to_data.m:49-58, :82, :99-125, :138-149 over aux_code/find_angle_bw_2_vecs.m:3-12
plane_fit(...)                        the whole call, vectorised: every draw scored, the rule replayed afterwards (the form the device takes)
plane_fit_loops(...)                  the same as a literal walk through the .m files' loops, one trial at a time (the cross-check of the restatement)
heading_RR(R_plane)                   ekf_heading_update.m:36-40 with the closed-form e2q Jacobian the library evaluates on host and device

Statuses as include/pre3.h: 1 ok, 0 no trial had an inlier, 2 the rule wanted more trials than were supplied, 3 axes undefined.
"""
import numpy as np

EPS = np.finfo(float).eps
DEFAULT_BOX = (80, 144, 50, 120)
ROWS, COLS = 144, 176


def scene(seed, outl, tilt_deg=25.0, roll_deg=4.0, height=1.2, noise=0.004):
    """(x_sr, y_sr, z_sr, normal): pixel (u, v) 0-based, f = 250, cx = 88, cy = 72, ray d = ((u - cx) / f, -(v - cy) / f, 1); the floor
    n . p + height = 0 with n = Rz(roll) (0, cos tilt, -sin tilt); range clipped to [0.3, 7]; Gaussian noise; a fraction outl of the pixels displaced
    by U(-0.5, 0.5)^3; SR4000 coordinates (x_sr = -x, y_sr = -y)."""
    rng = np.random.default_rng(seed)
    f, cx, cy = 250.0, 88.0, 72.0
    v, u = np.mgrid[0:ROWS, 0:COLS].astype(float)
    d = np.stack([(u - cx) / f, -(v - cy) / f, np.ones_like(u)], 0)
    t, r = np.deg2rad(tilt_deg), np.deg2rad(roll_deg)
    Rz = np.array([[np.cos(r), -np.sin(r), 0], [np.sin(r), np.cos(r), 0], [0, 0, 1]])
    nrm = Rz @ np.array([0.0, np.cos(t), -np.sin(t)])
    den = np.einsum("i,ijk->jk", nrm, d)
    s = np.where(den < -1e-3, -height / np.where(den < -1e-3, den, -1.0), 7.0)
    s = np.clip(s, 0.3, 7.0)
    p = d * s
    p += rng.normal(0, noise, p.shape)
    m = rng.random((ROWS, COLS)) < outl
    p[:, m] += rng.uniform(-0.5, 0.5, (3, int(m.sum())))
    return -p[0], -p[1], p[2], nrm


def scene_draws(seed, npts, n_draw=1001):
    rng = np.random.default_rng(100 + seed)
    return np.stack([rng.choice(npts, 3, replace=False) for _ in range(n_draw)]).astype(np.int32)


def crop(x_sr, y_sr, z_sr, box=None):
    r0, r1, c0, c1 = DEFAULT_BOX if box is None else box
    x, y, z = -np.asarray(x_sr, float), -np.asarray(y_sr, float), np.asarray(z_sr, float)
    x1, y1, z1 = x[r0 - 1:r1, c0 - 1:c1], y[r0 - 1:r1, c0 - 1:c1], z[r0 - 1:r1, c0 - 1:c1]
    return x1, y1, z1, np.stack([x1.ravel(order="F"), y1.ravel(order="F"), z1.ravel(order="F")])


def plane_dist(P, X):
    """signed distances of the columns of X (3, npts) from the plane through the columns of P (3, 3); NaN for a collinear or repeated sample"""
    a, b = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    n = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])
    with np.errstate(invalid="ignore", divide="ignore"):
        n = n / np.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])
        d = np.zeros(X.shape[1])
        for i in range(3):
            d = d + (X[i] - P[i, 0]) * n[i]
    return d


def ransac_N(nin, npts, s=3, p=0.99):
    pno = 1 - (nin / npts) ** s
    pno = max(EPS, pno)
    pno = min(1 - EPS, pno)
    return np.log(1 - p) / np.log(pno)


def replay(counts, npts, max_trials=1000):
    """(best, bestscore, n_trials, N, sta) of ransac.m's loop fed with the scores counts[0], counts[1], ... in order"""
    best, bestscore, N, trial, sta = -1, 0, 1.0, 0, 1
    while N > trial:
        if trial >= len(counts):
            sta = 2
            break
        if counts[trial] > bestscore:
            bestscore, best = int(counts[trial]), trial
            N = ransac_N(bestscore, npts)
        trial += 1
        if trial > max_trials:
            break
    if best < 0:
        sta = 0
    return best, bestscore, trial, float(N), sta


def fitplane(X):
    A = np.c_[X.T, np.ones(X.shape[1])]
    if X.shape[1] == 3:
        A = np.r_[A, np.zeros((1, 4))]
    return np.linalg.svd(A)[2][3].copy()


def _acosd(c):
    return np.degrees(np.arccos(np.clip(c, -1.0, 1.0)))


def line_plane(B, p):
    """(intersect, point) of the plane B . (x, y, z, 1) = 0 with the line through the origin along p"""
    norm1, norm2 = np.sqrt(B[0] * B[0] + B[1] * B[1] + B[2] * B[2]), np.sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2])
    denom = B[0] * p[0] + B[1] * p[1] + B[2] * p[2]
    if not abs(denom) >= 0.00001 * norm1 * norm2:
        return False, np.zeros(3)
    return True, (-B[3] / denom) * np.asarray(p, float)


def axes(B, p_orig, p_ray):
    """(B after the sign rule, R (3, 3) with columns x_axis, z_axis, y_axis, sta in {1, 3})"""
    B = np.array(B, float)
    a7 = _acosd(np.dot(B[:3], -p_orig) / np.linalg.norm(B[:3]) / np.linalg.norm(p_orig))
    if a7 < 90:
        B = -B
    z_axis = B[:3] / np.linalg.norm(B[:3])
    ok1, i1 = line_plane(B, p_ray)
    ok2, i2 = line_plane(B, p_orig)
    if not (ok1 and ok2):
        return B, np.zeros((3, 3)), 3
    y_axis = i1 - i2
    ny = np.linalg.norm(y_axis)
    if not (0 < ny < np.inf):
        return B, np.zeros((3, 3)), 3
    y_axis = y_axis / ny
    x_axis = np.cross(y_axis, z_axis)
    x_axis = -x_axis / np.linalg.norm(x_axis)
    return B, np.stack([x_axis, z_axis, y_axis], 1), 1


def _centre(x1):
    io, jo = x1.shape[0] // 2, x1.shape[1] // 2
    assert io - 20 >= 0
    return io, jo


def plane_fit(x_sr, y_sr, z_sr, draws, box=None, t=0.02):
    """dict: counts (every draw), best, n_inliers, n_trials, N, sta, inliers (bool mask), B, R, p_orig, p_ray, margin = the smallest
    | |d| - t | over every point of every trial that happened (how far the integer results are from a rounding decision)"""
    x1, y1, z1, XYZ = crop(x_sr, y_sr, z_sr, box)
    npts = XYZ.shape[1]
    draws = np.asarray(draws).reshape(-1, 3)
    D = [plane_dist(XYZ[:, dr], XYZ) for dr in draws]
    counts = np.array([int((np.abs(d) < t).sum()) for d in D], np.int32)
    best, score, n_trials, N, sta = replay(counts, npts)
    with np.errstate(invalid="ignore"):
        margin = min(float(np.nanmin(np.abs(np.abs(d) - t))) if np.isfinite(d).any() else np.inf for d in D[:n_trials])
    io, jo = _centre(x1)
    p_orig = np.array([x1[io, jo], y1[io, jo], z1[io, jo]])
    p_ray = np.array([x1[io - 20, jo], y1[io - 20, jo], z1[io - 20, jo]])
    out = dict(counts=counts, best=best, n_inliers=score, n_trials=n_trials, N=N, sta=sta, margin=margin, p_orig=p_orig, p_ray=p_ray,
               inliers=np.zeros(npts, bool), B=np.zeros(4), R=np.zeros((3, 3)), npts=npts)
    if best < 0:
        return out
    out["inliers"] = np.abs(D[best]) < t
    B, R, sta_ax = axes(fitplane(XYZ[:, out["inliers"]]), p_orig, p_ray)
    out["B"], out["R"] = B, R
    if sta_ax == 3:
        out["sta"] = 3
    return out


def plane_fit_loops(x_sr, y_sr, z_sr, draws, box=None):
    """plane_fit_to_data.m:13-149 as the .m files run it: ransac.m's while loop with the next row of draws as its sample, planeptdist's loop over the
    three coordinates, find(), fitplane's svd, the two calls of plane_imp_line_par_int_3d, the R of :147-149 entry by entry.  Raises where the
    reference raises (ransac.m:224).  Returns (R, B, inliers (1-based, as find returns them), trialcount, N, bestindex (0-based))."""
    BoxLimX, BoxLimY = ((80, 144), (50, 120)) if box is None else ((box[0], box[1]), (box[2], box[3]))
    x, y, z = -np.asarray(x_sr, float), -np.asarray(y_sr, float), np.asarray(z_sr, float)
    x1 = x[BoxLimX[0] - 1:BoxLimX[1], BoxLimY[0] - 1:BoxLimY[1]]
    y1 = y[BoxLimX[0] - 1:BoxLimX[1], BoxLimY[0] - 1:BoxLimY[1]]
    z1 = z[BoxLimX[0] - 1:BoxLimX[1], BoxLimY[0] - 1:BoxLimY[1]]
    XYZ = np.zeros((3, x1.size))
    k = 0
    for c in range(x1.shape[1]):                      # x1(:)': column after column
        for r in range(x1.shape[0]):
            XYZ[:, k] = (x1[r, c], y1[r, c], z1[r, c])
            k += 1
    t, s, p, maxTrials = 0.02, 3, 0.99, 1000
    npts = XYZ.shape[1]
    bestM, trialcount, bestscore, N, bestinliers, bestindex = None, 0, 0, 1, None, -1
    while N > trialcount:
        ind = draws[trialcount]
        P = XYZ[:, ind]                               # defineplane
        n = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
        with np.errstate(invalid="ignore", divide="ignore"):
            n = n / np.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])
            d = np.zeros(npts)
            for i in range(3):
                for j in range(npts):
                    d[j] = d[j] + (XYZ[i, j] - P[i, 0]) * n[i]
        inliers = [j + 1 for j in range(npts) if abs(d[j]) < t]
        ninliers = len(inliers)
        if ninliers > bestscore:
            bestscore, bestinliers, bestM, bestindex = ninliers, inliers, P, trialcount
            fracinliers = ninliers / npts
            pNoOutliers = 1 - fracinliers ** s
            pNoOutliers = max(EPS, pNoOutliers)
            pNoOutliers = min(1 - EPS, pNoOutliers)
            N = np.log(1 - p) / np.log(pNoOutliers)
        trialcount = trialcount + 1
        if trialcount > maxTrials:
            break
    if bestM is None:
        raise RuntimeError("ransac was unable to find a useful solution")
    Xin = XYZ[:, [j - 1 for j in bestinliers]]
    A = np.c_[Xin.T, np.ones(Xin.shape[1])]
    if Xin.shape[1] == 3:
        A = np.r_[A, np.zeros((1, 4))]
    _, _, vt = np.linalg.svd(A)
    B = vt.T[:, 3].copy()
    ro, co = x1.shape[0] // 2 + 1, x1.shape[1] // 2 + 1                   # floor(size / 2) + 1, 1-based
    p_orig = np.array([x1[ro - 1, co - 1], y1[ro - 1, co - 1], z1[ro - 1, co - 1]])
    v1, v2 = B[:3], -p_orig
    a7 = np.degrees(np.arccos(np.dot(v1, v2) / np.linalg.norm(v1) / np.linalg.norm(v2)))
    if a7 < 90:
        B = -B
    z_axis = B[:3] / np.linalg.norm(B[:3])
    p_ray = np.array([x1[ro - 1 - 20, co - 1], y1[ro - 1 - 20, co - 1], z1[ro - 1 - 20, co - 1]])

    def plane_imp_line_par_int_3d(a, b, c, d, x0, y0, z0, f, g, h):
        tol = 0.00001
        norm1, norm2 = np.sqrt(a * a + b * b + c * c), np.sqrt(f * f + g * g + h * h)
        denom = a * f + b * g + c * h
        if abs(denom) < tol * norm1 * norm2:
            if a * x0 + b * y0 + c * z0 + d == 0.0:
                return 1, np.array([x0, y0, z0])
            return 0, np.zeros(3)
        tt = -(a * x0 + b * y0 + c * z0 + d) / denom
        return 1, np.array([x0 + tt * f, y0 + tt * g, z0 + tt * h])

    _, p_intersect1 = plane_imp_line_par_int_3d(B[0], B[1], B[2], B[3], 0, 0, 0, p_ray[0], p_ray[1], p_ray[2])
    _, p_intersect2 = plane_imp_line_par_int_3d(B[0], B[1], B[2], B[3], 0, 0, 0, p_orig[0], p_orig[1], p_orig[2])
    y_axis = p_intersect1 - p_intersect2
    y_axis = y_axis / np.linalg.norm(y_axis)
    x_axis = np.cross(y_axis, z_axis)
    x_axis = -x_axis / np.linalg.norm(x_axis)
    orig = np.eye(3)
    cam = [x_axis, z_axis, y_axis]                    # x_axis_cam, y_axis_cam = z_axis, z_axis_cam = y_axis
    R = np.array([[cam[j] @ orig[:, i] for j in range(3)] for i in range(3)])
    return R, B, bestinliers, trialcount, float(N), bestindex


def heading_RR(R_plane):
    """RR = J_z J_e2q diag((pi / 180)^2) J_e2q' J_z' at q = R2q(R_plane), e = q2e(q), with e2q's Jacobian written out (e2q.m:22-35)"""
    from test_heading_ref import R2q, heading_rows, q2e
    q = R2q(np.asarray(R_plane, float))
    e = q2e(q)
    sr, sp, sy, cr, cp, cy = np.sin(e[0] / 2), np.sin(e[1] / 2), np.sin(e[2] / 2), np.cos(e[0] / 2), np.cos(e[1] / 2), np.cos(e[2] / 2)
    Qe = 0.5 * np.array([[-cy * cp * sr + sy * sp * cr, -cy * sp * cr + sy * cp * sr, -sy * cp * cr + cy * sp * sr],
                         [cy * cp * cr + sy * sp * sr, -cy * sp * sr - sy * cp * cr, -sy * cp * sr - cy * sp * cr],
                         [-cy * sp * sr + sy * cp * cr, cy * cp * cr - sy * sp * sr, -sy * sp * cr + cy * cp * sr],
                         [-sy * cp * sr - cy * sp * cr, -cy * cp * sr - sy * sp * cr, cy * cp * cr + sy * sp * sr]])
    A = heading_rows(q)[1] @ Qe
    return A @ (np.eye(3) * (np.pi / 180.0) ** 2) @ A.T
