"""GPU: the blocks that grow on demand (3pre_amd/csrc/pre3_own.h) through the Python layer.  A context or frame handle is driven
small, large, small, so that its blocks are replaced under it; what the last call returns is compared byte for byte with a fresh context (or handle) that
was given only the last input.  The map-management ring goes five calls round against the oracle.  The last test counts live blocks in a process of its
own (tests/regrow_worker.py): after everything is closed, the four counters are where they were.

The half-failure rule of the lazy groups is proven on the host (tests/test_own_host.py): nothing here makes an allocation fail on the device."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import vo_pair_cases as vp
from test_gpu_icsearch import _scan, _scene
from test_gpu_vo_pair import RES_FIELDS, bits

pytestmark = pytest.mark.gpu
synth = importlib.import_module("3pre_amd.synth")
srm = importlib.import_module("3pre_amd.sr4000")
vo = importlib.import_module("3pre_amd.vo")
HERE = os.path.dirname(os.path.abspath(__file__))


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("fused,rank,route", [("0", "0", 0), ("0", "1", 0), ("1", "1", 2)])
def test_scan_and_staging_ring_regrow(pre3, orc, fused, rank, route, monkeypatch):
    """N = 24, scans of K2 = 40, 300, 40: 300 takes scan_cap from 256 to 512 and the upload blocks from 64 KiB to 320 KiB (300 x 132 doubles), the
    third scan goes into the blocks the second left.  PRE3_IC_RANK=1 with the fused route off: every scan is also packed for the matrix-core matcher,
    whose planes are rebuilt after the growth (at 24 x 300 pairs the search itself stays on the exact kernel); the last row is the default route."""
    monkeypatch.setenv("PRE3_IC_FUSED", fused)
    monkeypatch.setenv("PRE3_IC_RANK", rank)
    N = 24
    rng, seq, bank = _scene(N, 53)
    s = seq["steps"][0]
    types, off, n = orc.landmark_table(np.zeros(N, int))

    def search(f, bank_now, sd, sp):
        f.set_x_p_k_k(seq["x0"], seq["P0"]); f.set_descriptors(bank_now); f.ekf_prediction(s["u"])
        f.load_scan(sd, sp)
        out = f.matching_sift_based(1.5, strict_reference=True)
        assert f.ic_search_route() == route
        return out, f.get_descriptors()

    f = pre3.EkfFilter(seq["cam"], types, dtype="f64", max_hyp=8)
    f.set_x_p_k_k(seq["x0"], seq["P0"]); f.ekf_prediction(s["u"])
    x1, P1 = f.get_x_k_km1(), f.get_p_k_km1()
    h, has_h = orc.project(types, off, x1, seq["cam"])
    scans = []
    for K2 in (40, 300, 40):
        sd, sp = _scan(rng, h, has_h, bank, K2, frac_seen=1.0, px_sigma=3.0)
        scans.append((sd[:, :K2].copy(), sp[:, :K2].copy()))
    for sd, sp in scans:
        out, bank_after = search(f, bank, sd, sp)
    g = pre3.EkfFilter(seq["cam"], types, dtype="f64", max_hyp=8)
    ref, ref_bank = search(g, bank, *scans[2])
    assert ref["match_idx"].shape[1] > 3 and len(ref["meas_idx"]) > 0
    for k in ("match_idx", "accepted", "meas_idx", "z"):
        assert same(out[k], ref[k]), k
    assert same(bank_after, ref_bank)
    orc_ref = orc.ic_search(types, off, x1, P1, seq["cam"], bank, *scans[2], 1.5, True)
    assert np.array_equal(out["match_idx"], orc_ref["match_idx"]) and np.array_equal(out["meas_idx"], orc_ref["meas_idx"])
    f.close(); g.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_marginal_block_regrow(pre3, dtype):
    """N = 12, index sets of k = 3, 40, 3: the index-set block and its pinned image grow with k; each read equals get_p_k_k()[np.ix_]"""
    N = 12
    x, P, _ = synth.make_map(N, seed=9)
    rng = np.random.default_rng(4)
    f = pre3.EkfFilter(synth.CAM.copy(), np.zeros(N, np.int32), dtype=dtype, max_hyp=8)
    f.set_x_p_k_k(x, P)
    xf, Pf = f.get_x_k_k(), f.get_p_k_k()
    sets = [np.array([0, 5, 20]), rng.integers(0, f.n, 40), np.array([84, 3, 13])]
    for idx in sets:
        xm, Pm = f.marginal(idx)
        assert same(xm, xf[idx]) and same(Pm, Pf[np.ix_(idx, idx)])
    g = pre3.EkfFilter(synth.CAM.copy(), np.zeros(N, np.int32), dtype=dtype, max_hyp=8)
    g.set_x_p_k_k(x, P)
    xg, Pg = g.marginal(sets[2])
    assert same(xm, xg) and same(Pm, Pg)
    f.close(); g.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_map_policy_scratch_regrow(pre3, dtype):
    """K = 4, 200, 4 candidates on a map that starts at N = 16: the policy's scratch and its mapped result block grow with K.  The fresh context takes
    the first one's state, map and book as they stand in front of the last call, and the same measurement flags."""
    N, cap, step = 16, 48, 25
    x, P, _ = synth.make_map(N, seed=21)
    cam = synth.CAM.copy()
    rng = np.random.default_rng(8)
    book = np.stack([rng.integers(0, 6, N), rng.integers(0, 4, N), rng.integers(6, step, N), rng.integers(6, step, N)], 1).astype(np.int32)

    def cands(K):
        uv = np.stack([rng.uniform(3, cam[6] - 3, K), rng.uniform(3, cam[5] - 3, K)], 1)
        d = rng.standard_normal((K, 3)); d[:, 2] = np.abs(d[:, 2]) + 0.5
        return uv, d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, 5.0, (K, 1))

    def call(f, uv, xyz):
        m = np.arange(0, f.N, 3)
        f.predict_camera_measurements(0, clear_first=True)
        f.set_measurements(m, np.zeros((len(m), 2)))
        f.set_flags((m % 2 == 0).astype(np.int32), np.zeros(len(m), np.int32))
        out = f.map_management_policy(step, uv, xyz, None, min_features=f.N + 3, linearity_index_threshold=0.1, std_pxl=1.0)
        return out, f.book(), f.lm_type.copy(), f.get_x_k_k(), f.get_p_k_k()

    f = pre3.EkfFilter(cam, np.zeros(N, np.int32), dtype=dtype, max_landmarks=cap)
    f.set_x_p_k_k(x, P); f.set_book(book)
    for K in (4, 200):
        out = call(f, *cands(K))[0]
    assert len(out["accepted"]) > 0 and out["examined"] > 4                  # (the large call walked beyond what the small block held)
    g = pre3.EkfFilter(cam, f.lm_type, dtype=dtype, max_landmarks=cap)
    g.set_x_p_k_k(f.get_x_k_k(), f.get_p_k_k()); g.set_book(f.book())
    uv, xyz = cands(4)
    a, b = call(f, uv, xyz), call(g, uv, xyz)
    for k in a[0]:
        assert same(np.asarray(a[0][k]), np.asarray(b[0][k])), k
    for u, v in zip(a[1:], b[1:]):
        assert same(u, v)
    f.close(); g.close()


def test_sr_frame_blocks_regrow(pre3):
    """a 24 x 32 frame pair; on each handle keypoint sets of K = 8, 300, 8 (the keypoint block and the pinned stage grow: 300 x 132 doubles), then
    the VO pair call between the two (the pair stage's work blocks, allocated on its first use)"""
    c = vp.make_pair(24, 32, 8, 8, 6, seed=17)
    rng = np.random.default_rng(2)
    big = (np.stack([rng.uniform(1, 32, 300), rng.uniform(1, 24, 300), np.full(300, 2.0), np.zeros(300)]), vp.unit(rng, 300))

    def handles(sets):
        out = []
        for w in (1, 2):
            f = srm.SrFrame(24, 32)
            f.load(c["fr%d" % w], 1)
            for frm, des in sets(w):
                k = f.keypoints(frm, des, 1)
            out += [f, k]
        return out

    f1, k1, f2, k2 = handles(lambda w: [(c["frm%d" % w], c["des%d" % w]), big, (c["frm%d" % w], c["des%d" % w])])
    g1, j1, g2, j2 = handles(lambda w: [(c["frm%d" % w], c["des%d" % w])])
    with f1, f2, g1, g2:
        for a, b in ((k1, j1), (k2, j2)):
            assert len(a["keep_idx"]) == 8
            for key in a:
                assert same(a[key], b[key]), key
        out, ref = vo.vo_pair_seeded(f1, f2, 20261018, 3), vo.vo_pair_seeded(g1, g2, 20261018, 3)
        assert out["pnum"] == 6 and out["sta"] == 1
        for key in ("match", "draws", "cnum", "state", "inliers", "pset1", "pset2"):
            assert same(out[key], ref[key]), key
        assert (out["capped"], out["rst"]) == (ref["capped"], ref["rst"])
        for key in RES_FIELDS:
            assert np.array_equal(bits(out[key]), bits(ref[key])), key


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_map_management_ring_goes_round(pre3, orc, dtype):
    """five map-management calls in a row on N = 8: staging slots 2, 3, 2, 3, 2.  One context makes them back to back (nothing in between waits for
    the stream: the ring's own wait is what keeps a block from being overwritten), a second one reads x, P and the types after each call; both hold
    the oracle's exact selection, the second after every call"""
    N = 8
    seq = synth.make_sequence(N, 1, 8, seed=19)
    types, off, n = orc.landmark_table(np.zeros(N, int))
    f = pre3.EkfFilter(seq["cam"], types, dtype=dtype, max_hyp=8)
    f.set_x_p_k_k(seq["x0"], seq["P0"])
    x, P = seq["x0"], (seq["P0"].astype(np.float32).astype(np.float64) if dtype == "f32" else seq["P0"])
    r = pre3.EkfFilter(seq["cam"], types, dtype=dtype, max_hyp=8)
    r.set_x_p_k_k(seq["x0"], seq["P0"])
    want = []
    for d in (3, 0, 4, 1, 0):
        f.map_management(del_idx=[d])
        r.map_management(del_idx=[d])
        x, P, types = orc.map_delete(types, off, x, P, [d])
        types, off, n = orc.landmark_table(types)
        want.append((x, P, types))
        assert r.N == len(types) and np.array_equal(r.lm_type, types) and same(r.get_x_k_k(), x) and same(r.get_p_k_k(), P), len(want)
    r.close()
    assert f.N == 3 and np.array_equal(f.lm_type, types)
    assert same(f.get_x_k_k(), x) and same(f.get_p_k_k(), P)
    g = pre3.EkfFilter(seq["cam"], want[3][2], dtype=dtype, max_hyp=8)
    g.set_x_p_k_k(want[3][0], want[3][1])
    g.map_management(del_idx=[0])
    assert same(f.get_x_k_k(), g.get_x_k_k()) and same(f.get_p_k_k(), g.get_p_k_k())
    f.close(); g.close()


def test_every_block_is_released(pre3):
    """tests/regrow_worker.py: two contexts and a frame handle touch every lazy group, everything is closed -- device blocks, device bytes, pinned
    blocks and pinned bytes are EQUAL to what they were after the warm-up"""
    env = dict(os.environ, PRE3_TEST_HOOKS="1")
    r = subprocess.run([sys.executable, os.path.join(HERE, "regrow_worker.py")], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    line = [ln for ln in r.stdout.decode().split("\n") if ln.startswith("LIVEJSON ")]
    assert len(line) == 1, r.stdout.decode()[-2000:]
    res = json.loads(line[0][9:])
    print(res)
    assert all(p > b for p, b in zip(res["peak"], res["base"])), res          # (the counters do count: two contexts and a handle were live)
    assert res["end"] == res["base"], res
