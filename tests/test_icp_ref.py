"""CPU: the numpy restatement of the dense ICP (tests/icp_ref.py) against things that are not it -- scipy's k-d tree for the
nearest neighbour, a hand-made case for the dedupe rule, the p < 3 status, convergence to a planted pose -- and the bookkeeping the GPU suites lean on:
the margins of every scene they use, the committed tolerance table, the new symbols."""
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np
import pytest

import icp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_icp_tolerance as T  # noqa: E402


def test_the_nearest_neighbour_against_a_kd_tree():
    spatial = pytest.importorskip("scipy.spatial")
    rng = np.random.default_rng(3)
    for n1, n2 in ((1, 5), (2, 3), (300, 257), (2049, 130)):
        model, src = R.surface(rng, n1), R.surface(rng, n2) + rng.normal(0, 0.01, (3, n2))
        d, idx, gap = R.nearest(model, src)
        dist, ref = spatial.cKDTree(model.T).query(src.T)
        assert np.array_equal(idx, ref)
        assert np.abs(np.sqrt(d) - dist).max() < 1e-14
        if n1 > 1:
            two = np.sort(((src.T[:, None, :] - model.T[None, :, :]) ** 2).sum(axis=2), axis=1)[:, :2]
            assert np.abs(gap - (two[:, 1] - two[:, 0])).max() < 1e-14 and (gap >= 0).all()
    # a tie goes to the lowest model index
    model = np.array([[0.0, 1.0, 1.0, 0.0], [0.0, 0.0, 0.0, 0.0], [1.0, 1.0, 1.0, 1.0]])
    d, idx, gap = R.nearest(model, np.array([[0.75], [0.0], [1.0]]))
    assert idx[0] == 1 and gap[0] == 0.0


def test_the_dedupe_keeps_the_smallest_distance_and_on_a_tie_the_highest_source():
    # sources 1..5 (1-based) on model points 2, 2, 4, 4, 7 (0-based 1, 1, 3, 3, 6): unequal D on the first pair, equal D on the second, one alone
    idx = np.array([1, 1, 3, 3, 6, 0])
    D = np.array([0.03, 0.01, 0.02, 0.02, 0.005, 0.5])
    corr, rj, cl = R.dedupe(idx, D, res=0.05)                             # the sixth is farther than 2 res: dropped
    assert corr.tolist() == [[2.0, 2.0, 0.01], [4.0, 4.0, 0.02], [7.0, 5.0, 0.005]]
    assert cl == 0.0 and abs(rj - 0.07) < 1e-15                            # the nearest D to 2 res = 0.1 is 0.03
    # MATLAB's current unique would keep the first occurrence -- the largest D: the legacy rule is the one built
    first = R.dedupe(np.array([1, 1]), np.array([0.03, 0.01]), res=0.05)[0]
    assert first.tolist() == [[2.0, 2.0, 0.01]]
    corr, rj, cl = R.dedupe(np.array([5, 5, 5]), np.array([0.03, 0.01, 0.02]), res=0.05)
    assert corr.tolist() == [[6.0, 2.0, 0.01]] and abs(cl - 0.01) < 1e-15
    # D exactly 2 res stays (D > 2 res is the rejection)
    assert len(R.dedupe(np.array([0]), np.array([0.1]), res=0.05)[0]) == 1


def test_fewer_than_three_pairs_is_status_two_with_the_transform_so_far():
    model = np.array([[0.0, 1.0, 0.0, 5.0], [0.0, 0.0, 1.0, 5.0], [1.0, 1.0, 1.0, 9.0]])
    src = model[:, :3] + 0.001
    r = R.icp_with_init(model, np.concatenate([src[:, :2], [[40.0], [40.0], [40.0]]], axis=1), 0.01)
    assert r["sta"] == R.FEW and (r["iters1"], r["iters2"], r["p"]) == (1, 0, 2)
    assert np.array_equal(r["R"], np.eye(3)) and not r["t"].any() and r["error"] == 1000000.0
    assert r["log"].tolist() == [[1.0, 2.0, 0.0]]
    ok = R.icp_with_init(model, src, 0.01)
    assert ok["sta"] == R.OK and ok["p"] == 3 and np.abs(ok["data2"] - model[:, :3]).max() < 1e-12


@pytest.mark.parametrize("n1,k,seed", [(1000, 3, 1), (1000, 3, 2), (4097, 5, 1), (4097, 5, 3)])
def test_a_planted_pose_is_recovered_from_a_start_a_centiradian_and_five_millimetres_off(n1, k, seed):
    s = R.subset_scene(n1, k, seed)
    r = R.icp_with_init(s["data1"], s["data2"], s["res"], s["Rinit"], s["Tinit"])
    a0, t0 = R.pose_error(s["Rinit"], s["Tinit"], s)
    a1, t1 = R.pose_error(r["Rtot"], r["ttot"], s)
    print("n1 k seed", n1, k, seed, "angle %.2e -> %.2e, translation %.2e -> %.2e" % (a0, a1, t0, t1), "iterations", r["iters1"], r["iters2"])
    assert abs(a0 - 0.01) < 1e-9 and abs(t0 - 0.005) < 1e-12 and r["sta"] == R.OK
    assert a1 * 5 <= a0 and t1 * 5 <= t0
    # u = [ttot; R2q(Rtot)] registers the source: data1 ~ Rtot data2 + ttot
    assert np.abs(r["data2"] - R.apply(r["Rtot"], r["ttot"], s["data2"])).max() < 1e-12


def test_the_runs_use_both_phases_and_the_no_change_ending():
    s = R.surface_scene(1000, 777, 4)
    r = R.icp_with_init(s["data1"], s["data2"], s["res"], s["Rinit"], s["Tinit"])
    assert r["iters1"] == 15 and r["iters2"] == 11 and r["sta"] == R.OK and len(r["ps"]) == 26
    assert r["error"] == min(r["log"][-1][2], r["log"][-2][2])


def test_the_tolerance_table_names_every_gpu_scene_and_is_reproduced():
    tab = json.load(open(os.path.join(ROOT, "tests", "golden", "icp_tolerance.json")))
    lim = T.header_limits()
    assert tab["limits"] == lim and tab["factor"] == 100 and tab["floor"] == 1e-12 and tuple(tab["seeds"]) == R.SEEDS
    names = [T.scene_name(*s) for s in T.all_scenes(lim)]
    assert sorted(names + ["frames_stride8"]) == sorted(tab["spread"])
    assert all(0.0 <= v < 1e-12 for v in tab["spread"].values())
    for (n1, n2, seed) in ((3, 3, 1), (257, 64, 2), (1000, 777, 1)):
        assert T.measure_scene(n1, n2, seed) == tab["spread"][T.scene_name(n1, n2, seed)]
    assert T.tolerance(tab, "257x64_s2") == 1e-12


@pytest.mark.parametrize("shape", [(3, 3), (257, 64), (1000, 777)])
def test_the_margins_of_the_small_gpu_scenes(shape):
    """(the larger ones are asserted by the GPU suite itself, on the restatement alone, before it compares anything)"""
    for seed in R.SEEDS:
        s = R.surface_scene(shape[0], shape[1], seed)
        r = R.icp_with_init(s["data1"], s["data2"], s["res"], s["Rinit"], s["Tinit"])
        assert R.margins_ok(r), (shape, seed, r["margins"])


def test_the_new_symbols(pre3):
    txt = open(os.path.join(ROOT, "include", "pre3.h")).read()
    lib = C.CDLL(pre3.LIB_PATH)
    for name in ("pre3_icp", "pre3_icp_limits", "pre3_icp_frames", "pre3_icp_pair_seeded"):
        assert "PRE3_API int %s(" % name in txt and name in pre3._lib.EXPORTS and hasattr(lib, name)
    vo = importlib.import_module("3pre_amd.vo")
    lim = vo.icp_limits()
    assert (lim["src_tile"], lim["chunk"]) == (T.header_limits()["src_tile"], T.header_limits()["chunk"]) and lim["iter_cap"] == R.ITER_CAP == 62
    assert lim["src_tile"] % (64 * lim["pts_per_lane"]) == 0
    assert C.sizeof(vo.IcpResult) == 288 and [f[0] for f in vo.IcpResult._fields_][-7:] == ["sta", "p", "iters1", "iters2", "n_model", "n_source", "pad"]
    for fn in (vo.icp_with_init, vo.icp_frames, vo.icp_pair_seeded, vo.icp_limits):
        assert callable(fn)
