"""The committed relocalisation cases: what tests/golden/make_reloc_tolerance.py measures on and what tests/test_reloc_host.py
and tests/test_gpu_relocalise.py run.  Everything is seeded; nothing here needs a device.

fixture_scene(seed)    the map is tests/golden/sr4000_step3.npz's x_k_k with its 185 descriptors; the true pose is the fixture's moved by MOVES[seed];
                       the scan holds the visible landmarks' descriptors plus N(0, 0.02) noise, renormalised, at pixels h(true pose) + 0.3 px noise, a
                       quarter of the pixels replaced by uniform ones, 60 distractor descriptors, all of it permuted.
synth_scene(name)      small maps of 3pre_amd/synth.py built so that n_corr is exactly 5, 6, 64 or 65 -- the minimum and the edges of the mask word read
                       with a device count --, one of them mixing inverse-depth and Cartesian landmarks, one with a rho = 0 landmark among the matched.
A scene: dict(name, types, off, x, P, bank (N, 128), scan_desc (K2, 128), scan_pos (K2, 4), cam, seed, seq, n_hyp, thr_px, min_support, truth)."""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import np_twin as tw  # noqa: E402
from util import load_sr4000  # noqa: E402

synth = importlib.import_module("3pre_amd.synth")

MOVES = {1: (0.25, 0.2), 2: (0.4, 0.35), 3: (0.1, 0.1)}          # seed -> (metres, radians) between the fixture's pose and the true one
N_DISTRACTORS = 60
THR_PX, MIN_SUPPORT = 2.0, 12
SYNTH = {"n5": dict(n_corr=5, extra=3, n_hyp=64, seed=41), "n6": dict(n_corr=6, extra=3, n_hyp=1, seed=42),
         "n64_mixed": dict(n_corr=64, extra=4, n_hyp=64, seed=43, mixed=True), "n65_rho0": dict(n_corr=65, extra=4, n_hyp=64, seed=44, rho0=True)}
# (n6: six correspondences give every hypothesis the same six points, so any two tie; one hypothesis has no runner-up)


def unit(v):
    return v / np.linalg.norm(v)


def moved_pose(x7, g, metres, radians):
    ax = unit(g.normal(size=3))
    dq = np.concatenate([[np.cos(radians / 2)], np.sin(radians / 2) * ax])
    q = tw.qProd(x7[3:7], dq)[0]
    return np.concatenate([x7[:3] + metres * unit(g.normal(size=3)), q / np.linalg.norm(q)])


def descriptors(g, n):
    d = np.abs(g.normal(size=(n, 128)))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def build_scan(g, cam, bank, seen, uv, n_distractors, outliers, desc_noise=0.02, px_noise=0.3):
    """the scan of the landmarks `seen` at pixels uv (len(seen), 2): (scan_desc, scan_pos, the scan index of every seen landmark, which of them kept
    their true pixel)"""
    m = len(seen)
    d = bank[seen] + desc_noise * g.normal(size=(m, 128))
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    px = uv + px_noise * g.normal(size=(m, 2))
    bad = g.permutation(m)[:int(round(outliers * m))]
    px[bad] = np.column_stack([g.uniform(0, cam[6], len(bad)), g.uniform(0, cam[5], len(bad))])
    d = np.vstack([d, descriptors(g, n_distractors)])
    px = np.vstack([px, np.column_stack([g.uniform(0, cam[6], n_distractors), g.uniform(0, cam[5], n_distractors)])])
    perm = g.permutation(len(d))
    pos = np.column_stack([px, g.uniform(1.0, 4.0, len(d)), g.uniform(-np.pi, np.pi, len(d))])
    where = np.empty(len(d), int)
    where[perm] = np.arange(len(d))
    good = np.ones(m, bool)
    good[bad] = False
    return np.ascontiguousarray(d[perm]), np.ascontiguousarray(pos[perm]), where[:m], good


def fixture_scene(seed):
    fx = load_sr4000()
    g = np.random.default_rng(7000 + seed)
    x, cam, N = fx["x_k_k"].copy(), fx["cam"], fx["N"]
    types, off = np.zeros(N, np.int32), (13 + 6 * np.arange(N)).astype(np.int32)
    pose = moved_pose(x[:7], g, *MOVES[seed])
    xt = x.copy()
    xt[:7] = pose
    h, has = tw.project(types, off, xt, cam)
    seen = np.nonzero(has)[0]
    bank = np.ascontiguousarray(fx["descriptor"])
    sd, sp, where, good = build_scan(g, cam, bank, seen, h[seen], N_DISTRACTORS, 0.25)
    return dict(name="fixture_%d" % seed, types=types, off=off, x=x, P=fx["p_k_k"], bank=bank, scan_desc=sd, scan_pos=sp, cam=cam, seed=100 + seed, seq=seed,
                n_hyp=200, thr_px=THR_PX, min_support=MIN_SUPPORT, truth=pose, seen=seen, where=where, good=good)


def synth_scene(name):
    spec = SYNTH[name]
    n_corr, N = spec["n_corr"], spec["n_corr"] + spec["extra"] + (1 if spec.get("rho0") else 0)
    g = np.random.default_rng(8000 + spec["seed"])
    x0, P0, _ = synth.make_map(N, seed=spec["seed"])
    cam = synth.CAM
    pose = moved_pose(x0[:7], g, 0.05, 0.05)
    Y = x0[13:].reshape(N, 6)
    uv, vis = synth.pixels(pose, Y, cam)
    assert vis.sum() >= n_corr + (1 if spec.get("rho0") else 0), "not enough of the map is visible from the moved pose"
    seen = np.nonzero(vis)[0][:n_corr + (1 if spec.get("rho0") else 0)]
    types = np.zeros(N, np.int32)
    if spec.get("mixed"):
        types[1::3] = tw.INVDEPTH + 1                                # every third landmark Cartesian
    # the state and covariance re-laid for the types: a Cartesian landmark keeps its point and the first three rows / columns of its block
    keep, xs = list(range(13)), [x0[:13]]
    off = np.zeros(N, np.int32)
    for i in range(N):
        off[i] = len(keep)
        if types[i] == tw.INVDEPTH:
            keep += list(range(13 + 6 * i, 19 + 6 * i))
            xs.append(Y[i])
        else:
            keep += list(range(13 + 6 * i, 16 + 6 * i))
            xs.append(Y[i, :3] + tw.m_dir(Y[i, 3], Y[i, 4]) / Y[i, 5])
    x = np.concatenate(xs)
    P = np.ascontiguousarray(P0[np.ix_(keep, keep)])
    bank = descriptors(g, N)
    outl = 0.0 if n_corr <= 6 else 0.25
    # (six points are EPnP's minimum: with 0.3 px of noise their pose scatters by several pixels, so the two smallest cases carry a tenth of the noise)
    sd, sp, where, good = build_scan(g, cam, bank, seen, uv[seen], 12, outl, px_noise=0.3 if n_corr > 6 else 0.03)
    if spec.get("rho0"):
        assert types[seen[-1]] == tw.INVDEPTH
        x[off[seen[-1]] + 5] = 0.0                                   # matched, but a point at infinity: left out of the correspondences
    return dict(name=name, types=types, off=off, x=x, P=P, bank=bank, scan_desc=sd, scan_pos=sp, cam=cam, seed=spec["seed"], seq=2, n_hyp=spec["n_hyp"],
                thr_px=THR_PX, min_support=6 if n_corr <= 6 else MIN_SUPPORT, truth=pose, seen=seen, where=where, good=good, n_corr=n_corr)


def names():
    return ["fixture_%d" % s for s in MOVES] + list(SYNTH)


_CACHE = {}


def scene(name):
    if name not in _CACHE:
        _CACHE[name] = fixture_scene(int(name.split("_")[1])) if name.startswith("fixture_") else synth_scene(name)
    return _CACHE[name]


def restated(name, **over):
    """reloc_ref.relocalise on a scene (cached for the scene's own parameters)"""
    import reloc_ref as rr
    sc = scene(name)
    key = (name, tuple(sorted(over.items())))
    if key not in _CACHE:
        kw = dict(seed=sc["seed"], seq=sc["seq"], thresh=1.5, n_hyp=sc["n_hyp"], thr_px=sc["thr_px"], undistort=True, min_support=sc["min_support"])
        kw.update(over)
        _CACHE[key] = rr.relocalise(sc["types"], sc["off"], sc["x"], sc["bank"], sc["scan_desc"], sc["scan_pos"], sc["cam"], **kw)
    return _CACHE[key]


def pose_error(pose, truth):
    """(degrees, metres) between two [r; q]"""
    c = abs(float(np.dot(unit(pose[3:7]), unit(truth[3:7]))))
    return float(np.degrees(2 * np.arccos(min(1.0, c)))), float(np.linalg.norm(pose[:3] - truth[:3]))
