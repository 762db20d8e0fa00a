"""A pinhole-consistent frame pair for the pair form of EPnP (pre3_vo_pair_pnp_seeded; tests/test_gpu_vo_pair_pnp.py), in the
format of tests/vo_pair_cases.py.

Range planes are back-projected through the fixture camera: a keypoint at pixel (c, r) -- in the kept uv's 1-based pixel base -- with depth z holds
x = -(c - Cx) z / f, y = -(r - Cy) z / f over its 3 x 3 block, so its range point [-x; -y; z] projects to (c, r).  prev's keypoints sit at integer pixels;
cur's at the exact sub-pixel projections of the same scene points after the planted motion pset1 = rot pset2 + trans, their range points planted over the
block of the pixel the keypoint rounds to.  Both frames measure the range along the pixel's ray with 2 mm of noise (so that a pose from them has an error
a bound can be taken from), and a few of cur's depths at keypoints are corrupted by +0.3 m: outliers for the 3-D / 3-D fit."""
import numpy as np

import pnp_cases as pc
import sr_frame_ref as sr
from vo_pair_cases import unit

ROWS, COLS, K, N_CORRUPT, SEED = 144, 176, 48, 6, 1          # the seed: the first whose projections stay inside the image
RANGE_SIGMA = 0.002


def pinhole_pair(seed=SEED):
    rng = np.random.default_rng(seed)
    cam = pc.fixture_cam()
    f, Cx, Cy = cam[0], cam[1], cam[2]
    rot, trans = pc.rot(rng.normal(0, 0.004, 3)), rng.normal(0, 0.004, 3)
    cells = [(9 * i + 4, 9 * j + 4) for i in range(ROWS // 9) for j in range(COLS // 9)]          # 0-based (row, column), nine pixels apart
    px1 = [cells[i] for i in rng.permutation(len(cells))[:K]]
    z1 = rng.uniform(1.0, 4.0, K)
    c1, r1 = np.array([c + 1.0 for r, c in px1]), np.array([r + 1.0 for r, c in px1])
    P1 = np.stack([(c1 - Cx) * z1 / f, (r1 - Cy) * z1 / f, z1])              # the scene points in prev's frame
    P2 = rot.T @ (P1 - trans[:, None])
    u2, v2 = Cx + f * P2[0] / P2[2], Cy + f * P2[1] / P2[2]
    order = rng.permutation(K)                                                # cur lists its keypoints in another order
    px2 = [(int(np.floor(v2[k] + 0.5)) - 1, int(np.floor(u2[k] + 0.5)) - 1) for k in order]
    assert all(1 <= r < ROWS - 1 and 1 <= c < COLS - 1 for r, c in px2), "a projection leaves the image: another seed"
    assert min(max(abs(a[0] - b[0]), abs(a[1] - b[1])) for i, a in enumerate(px2) for b in px2[:i]) >= 3, "two 3 x 3 blocks of cur overlap: another seed"
    M1 = P1 * (1 + RANGE_SIGMA * rng.normal(size=K) / np.linalg.norm(P1, axis=0))          # what prev measures: along the ray
    M2 = (P2 * (1 + RANGE_SIGMA * rng.normal(size=K) / np.linalg.norm(P2, axis=0)))[:, order]
    corrupt = rng.permutation(K)[:N_CORRUPT]
    M2[2, corrupt] += 0.3
    des2 = unit(rng, K)
    des1 = np.zeros((128, K))
    for j, k in enumerate(order):                                             # cur's keypoint j is prev's keypoint k
        d = des2[:, j] + rng.normal(0.0, 1e-3, 128)
        des1[:, k] = d / np.linalg.norm(d)
    frames = []
    for px, P in ((px1, M1), (px2, M2)):
        fr = dict(z=rng.uniform(0.8, 4.0, (ROWS, COLS)), x=rng.uniform(-1.5, 1.5, (ROWS, COLS)), y=rng.uniform(-1.0, 1.0, (ROWS, COLS)),
                  amp=np.floor(rng.uniform(100.0, 30000.0, (ROWS, COLS))), conf=np.full((ROWS, COLS), sr.CMAX))
        for k, (r, c) in enumerate(px):
            fr["x"][r - 1:r + 2, c - 1:c + 2] = -P[0, k]; fr["y"][r - 1:r + 2, c - 1:c + 2] = -P[1, k]; fr["z"][r - 1:r + 2, c - 1:c + 2] = P[2, k]
        frames.append({k: np.asfortranarray(v) for k, v in fr.items()})
    frm1, frm2 = np.zeros((4, K), order="F"), np.zeros((4, K), order="F")
    frm1[0], frm1[1] = c1, r1
    frm2[0], frm2[1] = u2[order], v2[order]
    for fm in (frm1, frm2):
        fm[2] = rng.uniform(1.0, 3.0, K); fm[3] = rng.uniform(-3.0, 3.0, K)
    return dict(rows=ROWS, cols=COLS, fr1=frames[0], fr2=frames[1], frm1=frm1, des1=np.asfortranarray(des1), frm2=frm2, des2=np.asfortranarray(des2),
                rot=rot, trans=trans, cam=cam, corrupt=np.sort(corrupt), order=order, name="pinhole")


def truth_RT(c):
    """the planted motion as EPnP states it: Xc = R Xw + T with Xw = pset1, Xc = pset2"""
    return c["rot"].T, -c["rot"].T @ c["trans"]
