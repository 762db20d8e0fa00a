"""The two synthetic 144 x 176 frames of the dense ICP's frame suite (tests/test_gpu_icp_frames.py, tests/golden/make_icp_tolerance.py).

prev sees a smooth surface on the pixel lattice; cur sees the same surface from a pose a little off, sampled half a pixel aside so that no point of one
cloud is a point of the other.  A few raw pixels are NaN and a few lie behind the camera: after the 3 x 3 filter their neighbourhoods are non-finite or
have z <= 0, and the compaction drops them.  The clouds are stated here on the CPU from tests/sr_frame_ref.py's conditioning, which the frame suite
holds bit-equal to the device's."""
import numpy as np

import icp_ref as R
import sr_frame_ref as sr

ROWS, COLS, MODE, SIGMA = 144, 176, 1, 1.0
RES = 0.02
NAN_PIXELS = ((10, 20), (70, 90), (130, 160))
BEHIND_PIXELS = ((40, 40), (100, 120))


def _surface(x, y):
    return 2.0 + 0.25 * np.sin(2.1 * x + 0.3) * np.cos(1.7 * y) + 0.15 * x * y + 0.1 * np.cos(3.3 * x - 1.1 * y)


def make_frames(seed=5):
    """dict(fr1, fr2, R_true, T_true, Rinit, Tinit): camera-frame points [-x; -y; z] of fr1 ~ R_true (those of fr2) + T_true"""
    rng = np.random.default_rng(seed)
    r, c = np.meshgrid(np.arange(ROWS), np.arange(COLS), indexing="ij")
    R_true, T_true = R.rotvec(rng.normal(0, 0.03, 3)), rng.normal(0, 0.02, 3)
    frames = []
    for shift, moved in ((0.0, False), (0.5, True)):
        X, Y = (c + shift - COLS / 2) / (COLS / 2), 0.8 * (r + shift - ROWS / 2) / (ROWS / 2)
        P = np.stack([X.ravel(), Y.ravel(), _surface(X, Y).ravel()])
        if moved:
            P = R_true.T @ (P - T_true[:, None])
        fr = dict(x=-P[0].reshape(ROWS, COLS), y=-P[1].reshape(ROWS, COLS), z=P[2].reshape(ROWS, COLS),
                  amp=np.floor(rng.uniform(100.0, 30000.0, (ROWS, COLS))), conf=np.full((ROWS, COLS), sr.CMAX))
        for px in NAN_PIXELS:
            fr["x"][px] = np.nan
        for px in BEHIND_PIXELS:
            fr["z"][px] = -100.0
        frames.append({k: np.asfortranarray(v) for k, v in fr.items()})
    Rinit = R.rotvec(0.01 * R.unit(rng)) @ R_true
    Tinit = T_true + 0.005 * R.unit(rng)
    return dict(fr1=frames[0], fr2=frames[1], R_true=R_true, T_true=T_true, Rinit=Rinit, Tinit=Tinit)


def clouds(x1, y1, z1, x2, y2, z2, stride):
    """the compaction's rule on filtered planes (rows x cols): dict(model (3, n1), source (3, n2), mpix, spix) in column-major pixel order"""
    rows, cols = x1.shape
    out = {}
    for name, (x, y, z), st in (("model", (x1, y1, z1), 1), ("source", (x2, y2, z2), stride)):
        rr, cc = np.arange(0, rows, st), np.arange(0, cols, st)
        pix = (cc[:, None] * rows + rr[None, :]).ravel()                               # column outer, row inner
        a, b, d = x.ravel(order="F")[pix], y.ravel(order="F")[pix], z.ravel(order="F")[pix]
        with np.errstate(invalid="ignore"):
            keep = np.isfinite(a) & np.isfinite(b) & np.isfinite(d) & (d > 0.0)
        out[name] = np.stack([-a[keep], -b[keep], d[keep]])
        out["mpix" if name == "model" else "spix"] = pix[keep].astype(np.int32)
    return out


def restated_clouds(sc, stride):
    w = sr.gauss3(SIGMA)
    c1, c2 = sr.condition(sc["fr1"], MODE, w), sr.condition(sc["fr2"], MODE, w)
    return clouds(c1["x"], c1["y"], c1["z"], c2["x"], c2["y"], c2["z"], stride)
