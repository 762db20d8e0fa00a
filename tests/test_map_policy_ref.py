"""CPU truth of pre3_map_policy (tests/map_policy_ref.py): the deletion rule, the counters, the target, quirks Q13 / Q14, the walk, the
reference's own snapshot3 book, and agreement with a literal transliteration of the .m loops."""
import importlib
import os

import numpy as np
import pytest

import map_policy_ref as mp

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _decide(step, book, ic=None, li=None, hi=None, pred=None, h=None, vis=None, cand=(), new_h=None, **kw):
    book = np.asarray(book, int).reshape(-1, 4)
    N = book.shape[0]
    z = np.zeros(N, int)
    return mp.decide(step, book, z if ic is None else ic, z if li is None else li, z if hi is None else hi, z if pred is None else pred,
                     np.zeros((N, 2)) if h is None else np.asarray(h, float), z if vis is None else vis, np.asarray(cand, float).reshape(-1, 2),
                     new_h or (lambda c: None), **kw)


def test_each_deletion_clause_fires_on_its_own():
    step = 30
    book = [[6, 2, 25, 29],      # tm < tp/2 and tp > 5
            [5, 2, 25, 29],      # tp = 5: kept
            [0, 0, 9, 29],       # step - init = 21
            [0, 0, 10, 29],      # step - init = 20: kept
            [0, 0, 25, 9]]       # stale, but N <= 20: kept
    assert list(_decide(step, book)["deleted"]) == [0, 2]
    # the N > 20 gate is on the map BEFORE deletion: 21 landmarks, one of which goes by clause 1, the stale one still goes
    book21 = [[0, 0, 25, 29]] * 19 + [[6, 0, 25, 29], [0, 0, 25, 9]]
    assert list(_decide(step, book21)["deleted"]) == [19, 20]
    assert list(_decide(step, book21[:20])["deleted"]) == [19]
    # an IC landmark of last frame is stamped visible at step - 1 before the rule
    ic = np.zeros(21, int); ic[20] = 1
    out = _decide(step, book21, ic=ic)
    assert list(out["deleted"]) == [19] and out["book"][-1, 3] == step - 1


def test_measured_and_the_counters_count_survivors_only():
    book = [[0, 0, 5, 5], [6, 0, 5, 5], [1, 1, 5, 5]]
    li, hi, pred = np.array([1, 1, 0]), np.array([0, 0, 1]), np.array([1, 1, 0])
    out = _decide(10, book, li=li, hi=hi, pred=pred, min_features=5)
    assert list(out["deleted"]) == [1] and out["measured"] == 2 and out["T"] == 3
    assert out["book"][:2].tolist() == [[1, 1, 5, 5], [1, 2, 5, 5]]


@pytest.mark.parametrize("strict,adds", [(True, 4), (False, 7)])
def test_q13_double_count(strict, adds):
    cand = [(20 + 40 * k, 20) for k in range(12)]
    out = _decide(3, np.zeros((0, 4)), cand=cand, min_features=7, strict=strict)
    assert out["T"] == 7 and len(out["accepted"]) == adds and out["examined"] == adds
    assert out["book"].tolist() == [[0, 0, 2, 2]] * adds


def test_the_target():
    li = np.ones(60, int)
    out = _decide(3, [[0, 0, 2, 2]] * 60, li=li, cand=[(10, 10)], min_features=50)
    assert out["T"] == 0 and len(out["accepted"]) == 0 and out["examined"] == 0
    out = _decide(3, [[0, 0, 2, 2]] * 3, cand=[(10, 10)] * 3, min_features=50, strict=False)
    assert out["measured"] == 0 and out["T"] == 50 and out["examined"] == 3


def test_q14_swapped_box():
    # candidate (u, v) = (100, 40); a landmark at (45, 95): inside only the swapped box (u vs v +- 15, v vs u +- 10)
    swapped = _decide(3, [[0, 0, 2, 2]], h=[(45, 95)], vis=[1], cand=[(100, 40)], min_features=2, strict=True)
    true_box = _decide(3, [[0, 0, 2, 2]], h=[(45, 95)], vis=[1], cand=[(100, 40)], min_features=2, strict=False)
    assert len(swapped["accepted"]) == 0 and len(true_box["accepted"]) == 1
    # a landmark at (110, 45): inside only the true box
    swapped = _decide(3, [[0, 0, 2, 2]], h=[(110, 45)], vis=[1], cand=[(100, 40)], min_features=2, strict=True)
    true_box = _decide(3, [[0, 0, 2, 2]], h=[(110, 45)], vis=[1], cand=[(100, 40)], min_features=2, strict=False)
    assert len(swapped["accepted"]) == 1 and len(true_box["accepted"]) == 0
    # invisible and deleted landmarks block nothing
    assert len(_decide(3, [[0, 0, 2, 2]], h=[(110, 45)], vis=[0], cand=[(100, 40)], min_features=2, strict=False)["accepted"]) == 1
    assert len(_decide(30, [[0, 0, 2, 2]], h=[(110, 45)], vis=[1], cand=[(100, 40)], min_features=2, strict=False)["accepted"]) == 1


def test_a_new_feature_blocks_a_later_candidate():
    cand = [(100, 40), (105, 42), (200, 40)]
    out = _decide(3, np.zeros((0, 4)), cand=cand, new_h=lambda c: tuple(cand[c]), min_features=6, strict=False)
    assert list(out["accepted"]) == [0, 2] and out["examined"] == 3
    out = _decide(3, np.zeros((0, 4)), cand=cand, new_h=lambda c: None, min_features=6, strict=False)
    assert list(out["accepted"]) == [0, 1, 2]


def test_snapshot3_book_from_the_reference_file():
    snapshot = importlib.import_module("3pre_amd.snapshot")
    s = snapshot.load_snapshot(os.path.join(GOLDEN, "snapshot3_sub.mat"))
    fi = s["features_info"]
    book = mp.features_info_book(fi)
    flag = lambda k: np.array([int(np.asarray(a[k]).reshape(-1)[0]) if np.size(a[k]) else 0 for a in fi])
    ic, li, hi = flag("individually_compatible"), flag("low_innovation_inlier"), flag("high_innovation_inlier")
    assert ic.sum() == 4 and (book[:, 2] == 2).all()
    out = _decide(4, book, ic=ic, li=li, hi=hi, pred=np.ones(len(fi), int))
    assert len(out["deleted"]) == 0
    assert (out["book"][ic == 1, 3] == 3).all() and (out["book"][ic == 0, 3] == 2).all()
    assert out["measured"] == int(((li + hi) > 0).sum())


@pytest.mark.parametrize("seed", range(40))
def test_restatement_agrees_with_the_literal_loops(seed):
    rng = np.random.default_rng(seed)
    N, K = int(rng.integers(0, 40)), int(rng.integers(0, 30))
    step = int(rng.integers(2, 40))
    book = np.stack([rng.integers(0, 12, N), rng.integers(0, 8, N), rng.integers(max(0, step - 25), step, N), rng.integers(max(0, step - 25), step, N)], 1) \
        if N else np.zeros((0, 4), int)
    ic, li, hi, pred = (rng.random(N) < 0.3).astype(int), (rng.random(N) < 0.3).astype(int), (rng.random(N) < 0.1).astype(int), (rng.random(N) < 0.6).astype(int)
    h = rng.uniform(0, 200, (N, 2)); vis = (rng.random(N) < 0.7).astype(int)
    cand = rng.uniform(0, 200, (K, 2))
    newh = {c: (tuple(cand[c] + rng.normal(0, 3, 2)) if rng.random() < 0.8 else None) for c in range(K)}
    mf = int(rng.integers(0, 30))
    for strict in (True, False):
        out = _decide(step, book, ic, li, hi, pred, h, vis, cand, newh.get, min_features=mf, strict=strict)
        info = [dict(times_predicted=int(book[i, 0]), times_measured=int(book[i, 1]), init_frame=int(book[i, 2]), last_visible=int(book[i, 3]),
                     individually_compatible=int(ic[i]), low_innovation_inlier=int(li[i]), high_innovation_inlier=int(hi[i]),
                     h=(0, 0) if pred[i] else None, h_kk=tuple(h[i]) if vis[i] else None) for i in range(N)]
        dl, acc, measured, T, res = mp.literal(step, info, [tuple(c) for c in cand], newh.get, min_features=mf, strict=strict)
        assert list(out["deleted"]) == dl and list(out["accepted"]) == acc and (out["measured"], out["T"]) == (measured, T)
        lit_book = np.array([[a["times_predicted"], a["times_measured"], a["init_frame"], a["last_visible"]] for a in res], int).reshape(-1, 4)
        assert np.array_equal(out["book"], lit_book)


def test_policy_on_a_filter_state_converts_and_projects():
    """policy(): a converted landmark is projected as its Cartesian point; the candidates' rho is 1 / norm(xyz)"""
    synth = importlib.import_module("3pre_amd.synth")
    seq = synth.make_sequence(12, 1, 4, seed=5)
    x, P, cam = seq["x0"], seq["P0"], seq["cam"]
    types = np.zeros(12, np.int32)
    book = np.tile([0, 0, 2, 2], (12, 1))
    z = np.zeros(12, int)
    out = mp.policy(3, types, x, P, cam, book, z, z, z, z, [(50.0, 60.0)], [(0.0, 0.0, 2.0)], threshold=1e9, min_features=4)
    assert out["converted"].sum() == 12 and (out["types"] == mp.CARTESIAN).all()
    assert out["rho"][0] == 0.5
    out0 = mp.policy(3, types, x, P, cam, book, z, z, z, z, [(50.0, 60.0)], [(0.0, 0.0, 2.0)], threshold=None, min_features=4)
    assert out0["converted"].sum() == 0
    np.testing.assert_allclose(out["h"][out["has_h"] == 1], out0["h"][out["has_h"] == 1], atol=1e-6)
