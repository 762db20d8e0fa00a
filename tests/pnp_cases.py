"""The committed EPnP cases: what tests/golden/make_pnp_tolerance.py measures on, and what tests/test_epnp_ref.py,
tests/test_pnp_host.py and tests/test_gpu_pnp.py run.  Everything is seeded; nothing here needs a device."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SR_CAM = [250.57731, 90.0, 70.0, -0.84656, 0.53701, 144.0, 176.0]          # the SR4000 of the reference's snapshot
SIZES = (6, 7, 63, 64, 65, 255, 256, 257)          # the minimum, the wave's edges, the edges of k_pnp_solve's 256-thread stride
DIM3_GOOD_SEED = 47                                 # see dim3_good(): found by search_dim3_good() on the CPU
RANSAC_SEEDS = {1: 11, 64: 12, 65: 13, 700: 14}     # n_hyp -> the scene's and the table's seed
THR_PX = 2.0


def fixture():
    d = np.load(os.path.join(HERE, "golden", "epnp_input_data_noise.npz"))
    kat = json.load(open(os.path.join(HERE, "golden", "epnp_kat.json")))
    return {k: d[k] for k in d.files}, kat


def fixture_cam():
    return fixture()[1]["cam"]


def rot(rv):
    """Rodrigues"""
    rv = np.asarray(rv, np.float64)
    th = np.linalg.norm(rv)
    if th == 0:
        return np.eye(3)
    k = rv / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def project(cam, Xc):
    return np.column_stack([cam[1] + cam[0] * Xc[:, 0] / Xc[:, 2], cam[2] + cam[0] * Xc[:, 1] / Xc[:, 2]])


def sr_scene(n, seed, cam=None, noise=0.3, fov=(1.0, 0.8)):
    """camera points in x in +-fov[0], y in +-fov[1], z in [1, 4] m; a pose about 0.05 rad / 0.05 m off; `noise` px of Gaussian pixel noise.
    Returns Xw (n, 3), U (n, 2), the clean pixels, R, T with Xc = R Xw + T."""
    cam = fixture_cam() if cam is None else cam
    g = np.random.default_rng(seed)
    Xc = np.column_stack([g.uniform(-fov[0], fov[0], n), g.uniform(-fov[1], fov[1], n), g.uniform(1.0, 4.0, n)])
    R = rot(g.normal(size=3) * 0.05 / np.sqrt(3))
    T = g.normal(size=3) * 0.05 / np.sqrt(3)
    Xw = (Xc - T) @ R                                   # R'(Xc - T), row by row
    U0 = project(cam, Xc)
    return Xw, U0 + noise * g.normal(size=(n, 2)), U0, R, T


def outlier_sta2():
    """the fixture's noisy pixels with the first eight moved by (150, -120): dimension 3 is entered and ends above 20 (sta = 2)"""
    d, kat = fixture()
    U = d["Ximg_pix"].copy()
    U[:8] += [150.0, -120.0]
    return d["Xworld"], U, kat["cam"]


def dim3_good(seed=DIM3_GOOD_SEED):
    """dimension 3 entered and ending below 20: a near-planar scene seen far away with a long lens and strong pixel noise, so that the one- and
    two-vector answers are poor and the three-vector one is not"""
    g = np.random.default_rng(seed)
    cam = fixture_cam()
    n = 30
    Xc = np.column_stack([g.uniform(-2, 2, n), g.uniform(-1.5, 1.5, n), 60.0 + g.uniform(-0.5, 0.5, n)])
    cam = [cam[0] * 20, cam[1], cam[2], 0.0, 0.0, cam[5], cam[6]]
    R = rot(g.normal(size=3) * 0.3)
    T = g.normal(size=3)
    Xw = (Xc - T) @ R
    return Xw, project(cam, Xc) + 3.0 * g.normal(size=(n, 2)), cam


def search_dim3_good(limit=2000):
    """the seeds of dim3_good() on which the restatement enters dimension 3 and answers below 20 with margin"""
    import epnp_ref as ref
    hits = []
    for s in range(limit):
        Xw, U, cam = dim3_good(s)
        r = ref.epnp(Xw, U, cam)
        e = r["err"]
        if r["dim3"] and r["sta"] == 1 and np.nanmin(e) < 15 and min(abs(e[0] - 20), abs(e[1] - 20)) > 2 and abs(e[2] - min(e[0], e[1])) > 1:
            hits.append((s, e.tolist(), r["best"]))
    return hits


def ransac_scene(n_hyp, n=40, outliers=0.25):
    """n correspondences of sr_scene, a quarter of the pixels replaced by uniform ones over the image; the draw table from tests/pnp_draws_ref.py"""
    import pnp_draws_ref as dr
    seed = RANSAC_SEEDS[n_hyp]
    cam = fixture_cam()
    Xw, U, U0, R, T = sr_scene(n, 1000 + seed, cam)
    g = np.random.default_rng(2000 + seed)
    bad = g.permutation(n)[:int(round(outliers * n))]
    U = U.copy()
    U[bad] = np.column_stack([g.uniform(0, cam[6], len(bad)), g.uniform(0, cam[5], len(bad))])
    draws = dr.draw_pnp(seed, 3, n, n_hyp)
    return dict(Xw=Xw, U=U, cam=cam, R=R, T=T, draws=draws, seed=seed, seq=3, bad=np.sort(bad))


def behind():
    """one point behind the camera (z = -2 m), its pixel the projection the pinhole equations give it, 0.3 px noise: the z < 0 rule fires and negates
    the whole Xc, as the reference would"""
    cam = fixture_cam()
    Xw, U, U0, R, T = sr_scene(30, 31, cam)
    g = np.random.default_rng(32)
    Xc = Xw @ R.T + T
    Xc[4, 2] = -2.0
    return (Xc - T) @ R, project(cam, Xc) + 0.3 * g.normal(size=(30, 2)), cam


def tolerance_cases():
    """name -> (Xw, U, cam): the cases the tolerance is measured on"""
    d, kat = fixture()
    out = {"fixture_true": (d["Xworld"], d["Ximg_pix_true"], kat["cam"]), "fixture_noisy": (d["Xworld"], d["Ximg_pix"], kat["cam"]),
           "outlier_sta2": outlier_sta2(), "dim3_good": dim3_good(), "behind": behind()}
    for n in SIZES:
        Xw, U, _, _, _ = sr_scene(n, 100 + n)
        out["sr_%d" % n] = (Xw, U, fixture_cam())
    return out


def pose_error(R, T, R0, T0):
    """(rotation angle between the two in degrees, distance of the two camera centres in metres)"""
    c = (np.trace(R @ R0.T) - 1) / 2
    return float(np.degrees(np.arccos(np.clip(c, -1, 1)))), float(np.linalg.norm(-R.T @ T + R0.T @ T0))
