"""CPU: the numpy restatement of FAST-9 and of the patch-feature initialisation policy (tests/fast_ref.py) against the fixture
tests/golden/fast_lab_crop.npz -- what the reference's decision tree computes on a crop where it and the published segment test agree (the generator
tests/golden/make_fast_fixtures.py re-derives that where the reference exists; this test reads only the fixture) -- the bit-trick 9-run against a
literal loop, the seeded box centres against numpy's Philox, and the two forms of the "features in the box" test."""
import os

import numpy as np
import pytest

import draws_ref as dr
import fast_ref as fr

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(HERE, "golden", "fast_lab_crop.npz")))


def test_fixture_is_what_the_issue_measured(fx):
    assert fx["image"].shape == (144, 176) and fx["image"].dtype == np.uint8
    assert [len(fx["corners_%d" % t]) for t in (10, 20, 30)] == [297, 72, 25]
    assert fx["exhaustive"].tolist() == [785268, 46658, 747510, 8900]      # tree, segment test, tree only, segment test only, of 3^16 ring states
    assert fx["box_centres"].shape == (3948, 2) and int((fx["box_first"][:, 0] > 0).sum()) == 3422


@pytest.mark.parametrize("t", [10, 20, 30])
def test_corners_equal_the_trees_in_order(fx, t):
    got = fr.fast_corner_detect_9(fx["image"], t)
    assert got.dtype == np.int32 and np.array_equal(got, fx["corners_%d" % t])
    lin = (got[:, 0].astype(np.int64) - 1) * 144 + got[:, 1]
    assert (np.diff(lin) > 0).all()                                         # x outer, y inner: the column-major index ascends


def adjacent_pairs(c):
    s = {tuple(p) for p in c.tolist()}
    return sum(1 for (x, y) in s for dx, dy in ((1, -1), (1, 0), (1, 1), (0, 1)) if (x + dx, y + dy) in s)


def test_suppression_equals_fast_nonmax_and_keeps_both_quirks(fx):
    mx, sc = fr.fast_nonmax(fx["image"], 10, 20)
    assert np.array_equal(mx, fx["maxima_10_20"]) and np.array_equal(sc, fx["maxima_scores_10_20"])
    assert len(mx) == 96 and int((sc == 0).sum()) == 16 and adjacent_pairs(mx) == 7      # score-0 maxima and ties kept on both sides


def test_first_maximum_of_every_box(fx):
    im = fx["image"]
    assert fr.all_centres(144, 176) == [tuple(c) for c in fx["box_centres"].tolist()]
    # every box's detection, from one pass per box (the policy's own path)
    for i in range(0, 3948, 1):
        got = fr.box_first_maximum(im, tuple(fx["box_centres"][i]))
        want = tuple(fx["box_first"][i])
        assert (got if got is not None else (0, 0)) == want, i


def test_bit_trick_run9_on_all_masks():
    m = np.arange(1 << 16, dtype=np.uint32)
    fast = fr.has_run9(m)
    slow = np.array([fr.has_run9_loop(v) for v in range(1 << 16)])
    assert np.array_equal(fast, slow)
    assert int(slow.sum()) == sum(1 for v in range(1 << 16) if fr.has_run9_loop(v)) and slow[0x01FF] and slow[0xFF80 | 0x0001] and not slow[0x00FF] and not slow[0xAAAA]


def test_seeded_centres_are_round_of_uniform_over_numpys_philox():
    for seed, seq, shape in ((3, 0, (144, 176)), (2 ** 63 + 5, 77, (240, 320)), (11, 2 ** 40, (144, 176))):
        got = fr.seeded_centres(seed, seq, *shape)
        for a in range(fr.MAX_ATTEMPTS):
            # numpy advances the counter before its first block: start one below [attempt, 0, seq, 0]; attempt 0 would wrap, so use the restated block
            # there and pin the block itself against numpy at attempt >= 1
            if a >= 1:
                g = np.random.Philox(counter=np.array([a - 1, 0, seq, 0], dtype=np.uint64), key=np.array([seed, fr.STREAM_FAST], dtype=np.uint64))
                w = [int(v) for v in g.random_raw(4)]
                assert w == dr.block([a, 0, seq, 0], [seed, fr.STREAM_FAST])
            else:
                w = dr.block([0, 0, seq, 0], [seed, fr.STREAM_FAST])
            u1, u2 = (w[0] >> 11) * 2.0 ** -53, (w[1] >> 11) * 2.0 ** -53
            rr, cr = (shape[0] - 1) - 42 - 60, (shape[1] - 1) - 42 - 40
            assert tuple(got[a]) == (int(np.floor(u1 * rr + 0.5)) + 51, int(np.floor(u2 * cr + 0.5)) + 41)
        assert (got[:, 0] >= 51).all() and (got[:, 0] <= shape[0] - 1 - 51).all() and (got[:, 1] >= 41).all() and (got[:, 1] <= shape[1] - 1 - 41).all()
    assert fr.STREAM_FAST == 5 and fr.STREAM_FAST not in (dr.STREAM_1P, dr.STREAM_VO, dr.STREAM_PLANE, 4)
    assert not np.array_equal(fr.seeded_centres(3, 0, 144, 176), fr.seeded_centres(3, 1, 144, 176))
    # the fork's constants at 144 x 176 (initialize_a_feature.m:62-68): ranges 41 and 93, offsets 51 and 41
    assert fr.centre_ranges(144, 176) == (41, 51, 93, 41)
    assert fr.box_centre(0.0, 0.0, 144, 176) == (51, 41) and fr.box_centre(1.0 - 2.0 ** -53, 1.0 - 2.0 ** -53, 144, 176) == (92, 134)


def test_both_forms_of_the_box_test_on_a_scene_where_they_differ():
    centre = (60, 100)                                       # row centre 60 +/- 30, column centre 100 +/- 20
    inside_matched = np.array([[100.0, 60.0]])               # u = column 100, v = row 60: in the box
    assert fr.features_in_box(inside_matched, centre, strict_reference=False)
    assert not fr.features_in_box(inside_matched, centre, strict_reference=True)       # as written: u = 100 against 60 +/- 30 fails
    swapped = np.array([[60.0, 100.0]])                      # u = 60, v = 100: outside the box, inside the reference's transposed test
    assert fr.features_in_box(swapped, centre, strict_reference=True) and not fr.features_in_box(swapped, centre, strict_reference=False)
    # strict inequalities: a feature exactly on the edge is outside
    assert not fr.features_in_box(np.array([[120.0, 60.0]]), centre, False) and fr.features_in_box(np.array([[119.999, 60.0]]), centre, False)
    assert not fr.features_in_box(np.array([[100.0, 30.0]]), centre, False) and not fr.features_in_box(np.zeros((0, 2)), centre, True)


def test_policy_walks_the_attempts():
    fxd = dict(np.load(os.path.join(HERE, "golden", "fast_lab_crop.npz")))
    im = fxd["image"]
    planes = dict(x=np.full(im.shape, 1.0), y=np.full(im.shape, 2.0), z=np.full(im.shape, 2.0), conf=None, cmax=0.0)
    full = fxd["box_centres"][fxd["box_first"][:, 0] > 0]
    empty = fxd["box_centres"][fxd["box_first"][:, 0] == 0]
    assert len(empty) == 526
    r = fr.initialize_a_feature(im, planes, np.zeros((0, 2)), np.concatenate([empty[:3], full[:7]]))
    assert r["status"] == fr.INITIALISED and r["attempts"] == 4 and r["rho"] == 1.0 / 3.0 and r["xyz"] == (-1.0, -2.0, 2.0)
    assert fr.initialize_a_feature(im, planes, np.zeros((0, 2)), empty[:10])["status"] == fr.NO_BOX
    planes["x"][:] = np.nan
    r = fr.initialize_a_feature(im, planes, np.zeros((0, 2)), full[:10])
    assert r["status"] == fr.NO_DEPTH_NAN and r["attempts"] == 1
