"""tests/patch_match_ref.py -- the numpy restatement of search_IC_matches.m:45-51's patch branch -- against things known without it (CPU only)."""
import numpy as np
import pytest

import patch_cases as pc
import patch_match_ref as ref


@pytest.fixture(scope="module")
def still(orc):
    """the camera where it was at initialisation; landmarks seen at integer pixels"""
    rng = np.random.default_rng(5)
    sp = [dict(uv=(float(rng.integers(30, 146)), float(rng.integers(30, 114))), S=pc.S_of(2.5), depth=rng.uniform(4, 12), cartesian=(i % 3 == 2)) for i in range(12)]
    return pc.build_scene(orc, 144, 176, sp, seed=21, moved=False)


def test_identity_warp(still):
    """the predicted patch is the centre 13 x 13 of the stored one (the undistort / distort round trip alone: <= 5e-13 grey levels; bound 1e-10)"""
    sc = still
    for fd in (pc.FD_FORK, sc["cam"]["f"]):
        r = pc.reference(sc, sc["imA"], 0.6, 0, fd=fd)
        assert (r["pstatus"] == ref.WARPED).all()
        for i in range(len(sc["types"])):
            want = sc["bank"]["patch"][i][14:27, 14:27].astype(np.float64)
            assert np.abs(r["patches"][i] - want).max() <= 1e-10


def test_planted_shift(still):
    sc = still
    sx, sy = 3, -2
    imB = pc.shift_image(sc["imA"], sx, sy, np.random.default_rng(1))
    r = pc.reference(sc, imB, 0.6, 0)
    assert (r["status"] == ref.MATCHED).all()
    assert np.array_equal(r["z"], sc["bank"]["uv_init"] + [sx, sy])
    assert (r["corr"] > 1 - 1e-12).all()


def _cand_list(K):
    return [(30 + k // 25, 40 + k % 25) for k in range(K)]


@pytest.mark.parametrize("K,plant,found", [(60, 31, True), (98, 50, True), (125, 110, False), (125, 60, True), (250, 230, False), (250, 150, True)])
def test_fork_mode(K, plant, found):
    """corrcoef_partitioned.m behind matching.m:118: K <= 98 returns the candidate BEFORE the best; K = 125 ignores candidates 100 and up, K = 250
    candidates 200 and up (1-based) -- a true maximum planted in the lost tail is not found, while the original line :115 finds it"""
    im = pc.smooth_image(np.random.default_rng(7), 144, 176)
    cands = _cand_list(K)
    j, i = cands[plant]
    pred = im[i - 7:i + 6, j - 7:j + 6].astype(np.float64)
    ok0, z0, mx0, _ = ref.match_one(im, pred, cands, 0.6, 0)
    assert ok0 and z0 == cands[plant] and mx0 > 1 - 1e-12
    ok1, z1, mx1, _ = ref.match_one(im, pred, cands, 0.6, 1)
    if K + 1 < 100:
        assert ok1 and z1 == cands[plant - 1] and mx1 > 1 - 1e-12
    elif found:
        assert ok1 and z1 == cands[plant] and mx1 > 1 - 1e-12
    else:
        assert mx1 < 1 - 1e-6 and z1 != cands[plant]
    assert ref.match_closed(im, pred, cands, 0.6, 1)[:2] == (ok1, z1)


def _one(sc, im, S=None, strict=0, **kw):
    return pc.reference(sc, im, 0.6, strict, S=S, **kw)


def test_no_match_K0_K1(still):
    sc = still
    imB = sc["imA"]
    S0 = np.tile(np.eye(2) * 1e-3, (len(sc["types"]), 1, 1))            # an ellipse that holds no pixel: h is moved off the lattice
    h = sc["h"] + 0.5
    r = pc.reference(sc, imB, 0.6, 0, S=S0, h=h)
    assert (r["ncand"] == 0).all() and (r["status"] == ref.NO_CANDIDATE).all() and np.isnan(r["corr"]).all() and len(r["meas_idx"]) == 0
    S1 = np.tile(np.eye(2) * 0.05, (len(sc["types"]), 1, 1))            # exactly one pixel, the perfect match: the original line finds it, the fork's cannot
    r0, r1 = pc.reference(sc, imB, 0.6, 0, S=S1), pc.reference(sc, imB, 0.6, 1, S=S1)
    assert (r0["ncand"] == 1).all() and (r0["status"] == ref.MATCHED).all()
    assert (r1["ncand"] == 1).all() and (r1["status"] == ref.BELOW).all() and np.isnan(r1["corr"]).all()


def test_no_match_flat_template_and_flat_candidates(orc):
    for shape in ((144, 176), (60, 80)):
        sc = pc.build_scene(orc, shape[0], shape[1], pc.spec_windows(*shape), seed=11)
        r = _one(sc, sc["imB"])
        kinds = [("flat_patch", ref.BELOW), ("no_patch", ref.NO_PATCH), ("behind", ref.NOT_PREDICTED), ("init_z", ref.WARP_OUTSIDE)]
        for key, st in kinds:
            i = [k for k, s in enumerate(sc["spec"]) if s.get(key)][0]
            assert r["status"][i] == st and np.isnan(r["corr"][i])
        i = [k for k, s in enumerate(sc["spec"]) if s.get("flat_block")][0]
        cands, _ = ref.candidates(sc["h"][i], sc["S"][i], *shape)
        flat = [im_flat(sc["imB"], c) for c in cands]
        assert any(flat) and not all(flat)                               # flat candidates are skipped (NaN), the rest are searched
        assert r["status"][i] in (ref.BELOW, ref.MATCHED) and not np.isnan(r["corr"][i])
        zero = [k for k in range(len(sc["spec"])) if r["status"][k] == ref.ZERO_PATCH]
        assert len(zero) == 2 and sorted(r["ncand"][zero].tolist()) == [0, 1] and np.isnan(r["corr"][zero]).all()
        assert np.isnan(r["patches"][[k for k, s in enumerate(sc["spec"]) if s.get("init_z")][0]]).any()      # the NaN sample


def im_flat(im, c):
    j, i = c
    p = im[i - 7:i + 6, j - 7:j + 6]
    return p.min() == p.max()


@pytest.mark.parametrize("shape", [(144, 176), (60, 80)])
@pytest.mark.parametrize("strict", [0, 1])
def test_literal_loop_equals_closed_form(orc, shape, strict):
    """on the scenes of tests/test_gpu_patch_search.py (h and S from the CPU oracle here, from the device there)"""
    scenes = [pc.build_scene(orc, shape[0], shape[1], pc.spec_windows(*shape), seed=11),
              pc.build_scene(orc, shape[0], shape[1], pc.spec_random(np.random.default_rng(3), shape[0], shape[1], 70 if shape[0] == 144 else 20), seed=12)]
    for sc in scenes:
        a = pc.reference(sc, sc["imB"], 0.6, strict)
        b = pc.reference(sc, sc["imB"], 0.6, strict, closed=True)
        assert np.array_equal(a["status"], b["status"]) and np.array_equal(a["ncand"], b["ncand"]) and np.array_equal(a["meas_idx"], b["meas_idx"])
        assert np.array_equal(np.nan_to_num(a["z"], nan=-1), np.nan_to_num(b["z"], nan=-1))
        assert np.array_equal(np.isnan(a["corr"]), np.isnan(b["corr"]))
        ok = ~np.isnan(a["corr"])
        assert np.abs(a["corr"][ok] - b["corr"][ok]).max() <= 1e-12
        assert a["margin_ellipse"].min() >= 1e-6 and a["margin_gap"].min() >= 1e-6
