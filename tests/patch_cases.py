"""Seeded scenes for the patch-search tests (tests/test_patch_match_ref.py on the CPU, tests/test_gpu_patch_search.py on the device): a camera, two
images, a map whose landmarks project where the case wants them, a covariance whose S_i are chosen by hand, and the stored patches."""
import numpy as np

import patch_match_ref as ref

FD_FORK = 250.57731 / (4.0 / 176 * 0.001)          # cam.F / cam.dx of initialize_cam.m:76-80


def make_cam(nRows, nCols):
    s = nCols / 176.0
    return dict(f=250.57731 * s, Cx=(90 + 1.69) * s, Cy=(70 + 2.27) * nRows / 144.0, k1=-0.84656, k2=0.53701, nRows=float(nRows), nCols=float(nCols))


def cam_list(cam):
    return [cam[k] for k in ("f", "Cx", "Cy", "k1", "k2", "nRows", "nCols")]


def smooth_image(rng, nRows, nCols, passes=2):
    """seeded, smoothed random bytes with enough contrast for a template standard deviation well above 5 grey levels"""
    a = rng.random((nRows + 8, nCols + 8))
    for _ in range(passes):
        a = (a[:-1, :-1] + a[1:, :-1] + a[:-1, 1:] + a[1:, 1:]) / 4
    a = a[:nRows, :nCols]
    a = (a - a.min()) / (a.max() - a.min())
    return np.ascontiguousarray(np.round(a * 255).astype(np.uint8))


def shift_image(im, sx, sy, rng):
    """B(row, column) = A(row - sy, column - sx); the uncovered border is fresh noise"""
    B = rng.integers(0, 256, im.shape).astype(np.uint8)
    R, Cn = im.shape
    r0, r1, c0, c1 = max(sy, 0), min(R + sy, R), max(sx, 0), min(Cn + sx, Cn)
    B[r0:r1, c0:c1] = im[r0 - sy:r1 - sy, c0 - sx:c1 - sx]
    return B


def landmark_for_pixel(cam, pose, uv, depth, cartesian=False):
    """the landmark (inverse depth, anchored at the camera; or Cartesian) that the camera at `pose` = [r; q] sees at the distorted pixel uv"""
    und = ref.undistort(np.asarray(uv, dtype=np.float64).reshape(2, 1), cam)[:, 0]
    d = np.array([(und[0] - cam["Cx"]) / cam["f"], (und[1] - cam["Cy"]) / cam["f"], 1.0])
    dw = ref.q2r(pose[3:7]) @ d
    if cartesian:
        return pose[0:3] + dw * depth
    dw = dw / np.linalg.norm(dw)
    theta, phi = np.arctan2(dw[0], dw[2]), np.arctan2(-dw[1], np.hypot(dw[0], dw[2]))
    return np.array([pose[0], pose[1], pose[2], theta, phi, 1.0 / (depth * np.linalg.norm(d))])


def cut_patch(im, uv):
    u, v = int(uv[0]), int(uv[1])
    return im[v - 21:v + 20, u - 21:u + 20].copy()


def covariance_for_S(orc, types, off, x, cam, S_target):
    """a covariance P (zero outside the landmarks' own blocks) with H_i P H_i' + I = S_target[i] for every predicted landmark"""
    n = x.shape[0]
    cl = cam_list(cam)
    h, has_h = orc.project(types, off, x, cl)
    Hc, Hl = orc.jacobian(types, off, x, cl, h, has_h)
    P = np.zeros((n, n))
    for i, t in enumerate(types):
        w = 6 if t == 0 else 3
        if not has_h[i]:
            P[off[i]:off[i] + w, off[i]:off[i] + w] = np.eye(w) * 1e-4
            continue
        Hp = np.linalg.pinv(Hl[i][:, :w])
        B = Hp @ (S_target[i] - np.eye(2)) @ Hp.T
        P[off[i]:off[i] + w, off[i]:off[i] + w] = (B + B.T) / 2
    return P, h, has_h


def S_of(sx, sy=None, rho=0.0):
    sy = sx if sy is None else sy
    return np.array([[sx * sx, rho * sx * sy], [rho * sx * sy, sy * sy]])


def build_scene(orc, nRows, nCols, spec, seed, moved=True):
    """spec: a list of dicts -- uv (where the landmark is seen from the initial pose), S (2 x 2 target), depth, and optionally cartesian, behind,
    no_patch, flat_patch, flat_block.  Returns a dict with everything a test needs."""
    rng = np.random.default_rng(seed)
    cam = make_cam(nRows, nCols)
    imA = smooth_image(rng, nRows, nCols)
    pose0 = np.array([0.0, 0, 0, 1, 0, 0, 0])
    pose1 = pose0.copy()
    if moved:
        ang = np.array([0.004, -0.003, 0.01])
        q = np.array([1.0, ang[0] / 2, ang[1] / 2, ang[2] / 2])
        pose1 = np.concatenate([[0.02, -0.015, 0.03], q / np.linalg.norm(q)])
    types = np.array([1 if s.get("cartesian") else 0 for s in spec], np.int32)
    off, n = [], 13
    for t in types:
        off.append(n)
        n += 3 if t else 6
    off = np.array(off, np.int32)
    x = np.zeros(n)
    x[0:7] = pose1
    N = len(spec)
    bank = dict(patch=np.zeros((N, 41, 41), np.uint8), uv_init=np.zeros((N, 2)), r_wc=np.zeros((N, 3)), R_wc=np.zeros((N, 3, 3)), has_patch=np.ones(N, bool))
    for i, s in enumerate(spec):
        y = landmark_for_pixel(cam, pose0, s["uv"], s.get("depth", 8.0), bool(s.get("cartesian")))
        if s.get("behind"):
            y[3] += np.pi
        x[off[i]:off[i] + len(y)] = y
        uv0 = np.asarray(s.get("uv_init", np.round(s["uv"])), dtype=np.float64)
        uv0 = np.array([min(max(uv0[0], 21), nCols - 20), min(max(uv0[1], 21), nRows - 20)])
        bank["uv_init"][i], bank["r_wc"][i], bank["R_wc"][i] = uv0, pose0[0:3] + np.array([0, 0, s.get("init_z", 0.0)]), ref.q2r(pose0[3:7])
        bank["patch"][i] = 100 if s.get("flat_patch") else cut_patch(imA, uv0)
        bank["has_patch"][i] = not s.get("no_patch")
    imB = imA.copy()
    S_target = np.stack([np.asarray(s["S"], dtype=np.float64) for s in spec]) if N else np.zeros((0, 2, 2))
    P, h, has_h = covariance_for_S(orc, types, off, x, cam, S_target) if N else (np.zeros((13, 13)), np.zeros((0, 2)), np.zeros(0, np.int32))
    for i, s in enumerate(spec):
        if s.get("flat_block") and has_h[i]:
            u, v = int(round(h[i][0])), int(round(h[i][1]))
            imB[max(v - 9, 0):v + 8, max(u - 9, 0):u + 8] = 90
    P += np.eye(n) * 1e-9                                     # (positive definite, so that a step can follow)
    S = orc.innovation(types, off, P, *orc.jacobian(types, off, x, cam_list(cam), h, has_h), has_h) if N else np.zeros((0, 2, 2))
    return dict(cam=cam, imA=imA, imB=imB, types=types, off=off, x=x, P=P, h=h, has_h=has_h, S=S, bank=bank, spec=spec, pose0=pose0)


def spec_windows(nRows, nCols):
    """the hand-made landmarks of the 144 x 176 scene (and, scaled down, of the 60 x 80 one): one each per window size and landmark case"""
    big = nCols >= 176
    cx, cy = nCols / 2.0, nRows / 2.0
    ox, oy = round(0.17 * nCols), round(0.14 * nRows)
    sp = [
        dict(uv=(cx + 0.3, cy - 0.2), S=S_of(1.0)),                          # 2 <= K <= 98
        dict(uv=(cx - 20.4, cy + 10.3), S=S_of(2.8, 2.9, 0.2)),              # K in 99 .. 199
        dict(uv=(cx + 22.2, cy - 14.6), S=S_of(3.6, 3.7, -0.3)),             # K >= 200: a lost tail
        dict(uv=(cx - 3.3, cy + 2.4), S=S_of(8.0, 8.2, 0.1)),                # K above one workgroup's lanes
        dict(uv=(9.4, cy + 1.3), S=S_of(4.0)),                               # clipped by the left border
        dict(uv=(nCols - 9.3, cy - 3.1), S=S_of(4.0), cartesian=True),       # ... the right
        dict(uv=(cx + 5.2, 9.2), S=S_of(4.0)),                               # ... the top
        dict(uv=(cx - 7.7, nRows - 9.4), S=S_of(4.0)),                       # ... the bottom
        dict(uv=(cx + 1.4, cy + 0.7), S=S_of(22.0 if big else 9.0)),         # below the LDS staging limit
        dict(uv=(cx - 1.6, cy - 0.4), S=S_of(25.0 if big else 40.0)),        # above it (60 x 80: the whole image fits; see the test)
        dict(uv=(cx + 0.6, cy + 0.2), S=S_of(100.0)),                        # the whole image
        dict(uv=(4.7, cy), S=S_of(1.0)),                                     # the border band: zero patch, K = 1
        dict(uv=(2.5, cy + 4), S=S_of(1.0), cartesian=True),                 # the border band: zero patch, K = 0
        dict(uv=(cx, cy), S=S_of(1.0), behind=True),                         # behind the camera: not predicted
        dict(uv=(cx + ox + 0.2, cy + oy + 0.1), S=S_of(2.0), no_patch=True),      # without a patch
        dict(uv=(cx - ox - 0.3, cy - oy - 0.2), S=S_of(2.0), init_z=3.6),         # the warp leaves the stored patch: the camera pulled back to half the depth
        dict(uv=(cx + ox - 1.6, cy - oy - 2.3), S=S_of(3.0), flat_block=True),    # flat candidates
        dict(uv=(cx - ox + 3.9, cy + oy + 1.7), S=S_of(2.0), flat_patch=True),    # a flat stored patch
    ]
    return sp


def spec_random(rng, nRows, nCols, N, cart_every=4, sig=(1.5, 4.0)):
    sp = []
    for i in range(N):
        uv = (rng.uniform(24, nCols - 24), rng.uniform(24, nRows - 24))
        sx, sy = rng.uniform(*sig, 2)
        sp.append(dict(uv=uv, S=S_of(sx, sy, rng.uniform(-0.5, 0.5)), depth=rng.uniform(4, 12), cartesian=(i % cart_every == cart_every - 1)))
    return sp


def reference(sc, im, thr, strict, fd=FD_FORK, h=None, has_h=None, S=None, x=None, closed=False):
    return ref.search(sc["cam"], fd, im, sc["x"] if x is None else x, sc["types"], sc["off"], sc["h"] if h is None else h,
                      sc["has_h"] if has_h is None else has_h, sc["S"] if S is None else S, sc["bank"], thr, strict, closed=closed)
