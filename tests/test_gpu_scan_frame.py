"""GPU: the IC search's scan taken from a resident SR4000 frame (pre3_set_scan_frame).  The oracle is always pre3_set_scan fed
from the host with the arrays handed to (which = 0) or returned by (which = 1) SrFrame.keypoints(); pre3_ic_search behind either must give the same
bits: the match list, the measurement list, z and the refreshed bank."""
import importlib

import numpy as np
import pytest

import sr_frame_ref as sr

pytestmark = pytest.mark.gpu
srm = importlib.import_module("3pre_amd.sr4000")
synth = importlib.import_module("3pre_amd.synth")

ROWS, COLS = 144, 176
K2S = (0, 1, 63, 64, 65, 300)            # empty; one lane; a wave and its edges; more than one workgroup of the copy (64 lanes per descriptor)
LDFS = (2, 4, 5)                         # no third entry (zeros); the reference's; odd (the scalar read path of the copy)


def _context(pre3, orc, sr4000, which):
    """(filter, x, P, bank (128, N), h (N, 2)): the SR4000 fixture's prediction (N = 185, fp64) or a synthetic N = 8 map (fp32); h the predicted pixels,
    NaN where a landmark is not predicted"""
    if which == "fixture_f64":
        d = sr4000
        f = pre3.EkfFilter(d["cam"], np.zeros(d["N"], np.int32), dtype="f64", max_hyp=8, std_z=d["std_z"])
        return f, d["x_k_km1"].copy(), d["p_k_km1"], np.ascontiguousarray(d["descriptor"].T), d["h"]
    x0, P0, _ = synth.make_map(8, None)
    rng = np.random.default_rng(8)
    bank = np.abs(rng.normal(0, 1, (128, 8)))
    bank /= np.linalg.norm(bank, axis=0)
    types, off, n = orc.landmark_table(np.zeros(8, int))
    h, has_h = orc.project(types, off, x0, synth.CAM)
    h = np.array(h, dtype=np.float64)
    h[np.asarray(has_h) == 0] = np.nan
    return pre3.EkfFilter(synth.CAM, np.zeros(8, np.int32), dtype="f32", max_hyp=8), x0, P0, bank, h


def _reset(f, x, P, bank):
    f.set_x_p_k_km1(x, P)
    f.set_descriptors(bank)


def _scan(rng, h, bank, K2, ldf):
    """K2 keypoints: noisy copies of the landmarks' descriptors near their predicted pixels (kept inside the image), then clutter; frames (ldf, K2)"""
    N = bank.shape[1]
    des, frm = np.zeros((128, K2), order="F"), np.zeros((ldf, K2), order="F")
    for k in range(K2):
        if k < N and np.isfinite(h[k]).all():
            des[:, k] = bank[:, k] + rng.normal(0, 0.01, 128)
            uv = h[k] + rng.normal(0, 1.5, 2)
        else:
            d = np.abs(rng.normal(0, 1, 128))
            des[:, k] = d / np.linalg.norm(d)
            uv = np.array([rng.uniform(1, COLS), rng.uniform(1, ROWS)])
        frm[0, k], frm[1, k] = np.clip(uv[0], 1.0, COLS), np.clip(uv[1], 1.0, ROWS)
        frm[2:, k] = rng.uniform(1, 4, ldf - 2)
    perm = rng.permutation(K2)
    return np.asfortranarray(des[:, perm]), np.asfortranarray(frm[:, perm])


def _pos4(frm):
    """SCALE_ORIENT_POS_RAW as pre3_set_scan takes it: entries 0..3 of every frame, zeros beyond ldf"""
    p = np.zeros((4, frm.shape[1]))
    n = min(4, frm.shape[0])
    p[:n] = frm[:n]
    return p


def _search(f):
    out = f.matching_sift_based(1.5, strict_reference=True)
    out["bank"] = f.get_descriptors()
    return out


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


@pytest.fixture(scope="module")
def frame():
    with srm.SrFrame(ROWS, COLS) as fh:
        fh.load(sr.make_frame(ROWS, COLS, seed=21), 0)
        yield fh


@pytest.mark.parametrize("ldf", LDFS)
@pytest.mark.parametrize("K2", K2S)
@pytest.mark.parametrize("ctx", ["fixture_f64", "synth_f32"])
def test_the_search_behind_either_scan_is_the_same(pre3, orc, sr4000, frame, ctx, K2, ldf):
    f, x, P, bank, h = _context(pre3, orc, sr4000, ctx)
    rng = np.random.default_rng(1000 * K2 + ldf)
    des, frm = _scan(rng, h, bank, K2, ldf)
    kept = frame.keypoints(frm, des, srm.GATE_DEPTH)
    # which = 0: the raw set
    _reset(f, x, P, bank)
    f.load_scan(des, _pos4(frm))
    ref = _search(f)
    _reset(f, x, P, bank)
    f.set_scan_frame(frame, 0)
    got = _search(f)
    _same(got, ref)
    if K2 >= 63 and ctx == "fixture_f64":
        assert ref["match_idx"].shape[1] > 10 and len(ref["meas_idx"]) > 5         # the comparison is not of two empty lists
    if K2 == 0:
        assert ref["match_idx"].shape[1] == 0 and len(ref["meas_idx"]) == 0
    # which = 1: the kept set
    _reset(f, x, P, bank)
    f.load_scan(kept["descriptors"], _pos4(kept["frames"]))
    ref1 = _search(f)
    _reset(f, x, P, bank)
    f.set_scan_frame(frame, 1)
    _same(_search(f), ref1)
    f.close()


@pytest.mark.parametrize("rank_env", ["1", "0"])
def test_a_descriptor_outside_the_ranked_routes_bounds(pre3, orc, sr4000, frame, rank_env, monkeypatch):
    """N * K2 >= 65536 with the fused route off: the ranked route applies to an in-bounds scan; one entry of 1e-50 and both forms leave it, with the same
    results -- the handle noted the bounds when the descriptors passed through its staging.  PRE3_IC_RANK=0: the exact kernel on both sides."""
    monkeypatch.setenv("PRE3_IC_FUSED", "0")
    monkeypatch.setenv("PRE3_IC_RANK", rank_env)
    f, x, P, bank, h = _context(pre3, orc, sr4000, "fixture_f64")
    rng = np.random.default_rng(5)
    des, frm = _scan(rng, h, bank, 400, 4)
    for bad in (False, True):
        if bad:
            des = des.copy(order="F"); des[77, 41] = 1e-50
        kept = frame.keypoints(frm, des, srm.GATE_DEPTH)
        for which, (d_host, f_host) in enumerate(((des, frm), (kept["descriptors"], kept["frames"]))):
            _reset(f, x, P, bank)
            f.load_scan(d_host, _pos4(f_host))
            ref = _search(f)
            route_ref = f.ic_search_route()
            _reset(f, x, P, bank)
            f.set_scan_frame(frame, which)
            _same(_search(f), ref)
            # (which = 1 with the offending entry dropped by the gate: the raw set's flag stands in, the exact kernel gives the same bits)
            assert f.ic_search_route() == route_ref or (which == 1 and bad and f.ic_search_route() == 0)
            if which == 0:
                assert route_ref == (1 if rank_env == "1" and not bad else 0)
    f.close()


def test_state_errors_and_the_release_of_the_keypoint_block(pre3, orc, sr4000):
    f, x, P, bank, h = _context(pre3, orc, sr4000, "fixture_f64")
    rng = np.random.default_rng(3)
    des_a, frm_a = _scan(rng, h, bank, 300, 4)
    des_b, frm_b = _scan(rng, h, bank, 300, 4)
    with srm.SrFrame(ROWS, COLS) as fh:
        for which in (0, 1):
            with pytest.raises(pre3.Pre3Error) as e:                               # nothing loaded
                f.set_scan_frame(fh, which)
            assert e.value.code == -4
        fr = sr.make_frame(ROWS, COLS, seed=4)
        fh.load(fr, 0)
        with pytest.raises(pre3.Pre3Error) as e:                                   # no keypoint record yet
            f.set_scan_frame(fh, 0)
        assert e.value.code == -4
        fh.keypoints(frm_a, des_a, srm.GATE_DEPTH)
        for which in (-1, 2):
            with pytest.raises(pre3.Pre3Error) as e:
                f.set_scan_frame(fh, which)
            assert e.value.code == -1
        fh.load(fr, 0)                                                             # a load makes the record stale
        with pytest.raises(pre3.Pre3Error) as e:
            f.set_scan_frame(fh, 0)
        assert e.value.code == -4
        fh.keypoints(frm_a[:, :10], des_a[:5, :10], srm.GATE_DEPTH)                # descriptors of 5 entries
        with pytest.raises(pre3.Pre3Error) as e:
            f.set_scan_frame(fh, 0)
        assert e.value.code == -1
        # a keypoint call on the handle straight after set_scan_frame, then the search: results from the first set
        _reset(f, x, P, bank)
        f.load_scan(des_a, _pos4(frm_a))
        ref = _search(f)
        fh.keypoints(frm_a, des_a, srm.GATE_DEPTH)
        _reset(f, x, P, bank)
        f.set_scan_frame(fh, 0)
        fh.keypoints(frm_b, des_b, srm.GATE_DEPTH)
        _same(_search(f), ref)
        assert ref["match_idx"].shape[1] > 10
    f.close()
