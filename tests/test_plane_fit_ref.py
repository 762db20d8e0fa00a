"""CPU: the numpy restatement of plane_fit_to_data.m (tests/plane_fit_ref.py; the truth tests/test_gpu_plane_fit.py holds the device to) against a
literal walk through the .m files' loops, and the properties of what it returns.  DESIGN.md section 17."""
import numpy as np
import pytest

import plane_fit_ref as pr
from test_heading_ref import axis_rot
from test_heading_ref import heading_RR as heading_RR_ref

SCENES = [(seed, outl) for seed in range(4) for outl in (0.1, 0.5, 0.7)]


def _scene(seed, outl):
    x, y, z, nrm = pr.scene(seed, outl)
    return x, y, z, nrm, pr.scene_draws(seed, 65 * 71)


@pytest.mark.parametrize("seed,outl", SCENES)
def test_restatement_against_the_loops_of_the_reference(seed, outl):
    x, y, z, nrm, draws = _scene(seed, outl)
    a = pr.plane_fit(x, y, z, draws)
    R, B, inl, trials, N, best = pr.plane_fit_loops(x, y, z, draws)
    assert a["sta"] == 1 and a["npts"] == 4615
    assert (a["best"], a["n_trials"], a["n_inliers"]) == (best, trials, len(inl))
    assert np.array_equal(np.nonzero(a["inliers"])[0] + 1, inl)
    assert a["N"] == N
    assert np.abs(a["B"] - B).max() <= 1e-14 and np.abs(a["R"] - R).max() <= 1e-14
    # the stopping rule's trial counts on these scenes: 4 at 10 % outliers, about 30 at 50 %, 115 .. 173 at 70 %
    lo, hi = {0.1: (4, 4), 0.5: (25, 40), 0.7: (100, 200)}[outl]
    assert lo <= trials <= hi
    assert a["margin"] >= 1e-9                                  # no integer above hinges on a rounding
    # R: orthonormal, a rotation; the normal within a degree of the scene's
    assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-14 and abs(np.linalg.det(R) - 1) <= 1e-14
    ang = np.degrees(np.arccos(min(1.0, abs(a["R"][:, 1] @ nrm))))
    assert ang < 1.0, ang


def test_both_branches_of_the_sign_rule_give_the_same_R():
    seen = set()
    for seed, outl in SCENES:
        x, y, z, _, draws = _scene(seed, outl)
        a = pr.plane_fit(x, y, z, draws)
        _, _, _, XYZ = pr.crop(x, y, z)
        B0 = pr.fitplane(XYZ[:, a["inliers"]])                  # the sign LAPACK left
        seen.add(bool(B0 @ a["B"] < 0))
        for Bs in (B0, -B0):
            B, R, sta = pr.axes(Bs, a["p_orig"], a["p_ray"])
            assert sta == 1 and np.array_equal(B, a["B"]) and np.array_equal(R, a["R"])
        assert a["B"][:3] @ a["p_orig"] > 0                     # the normal points away from the camera: more than 90 degrees from -p_orig
    assert seen == {True, False}                                # both branches occur with LAPACK's own signs


def test_stopping_rule_on_hand_built_scores():
    npts = 1000
    # every point an inlier at the first trial: N = log(0.01) / log(eps) < 1 ends it
    assert pr.replay([1000, 5, 7], npts)[:3] == (0, 1000, 1) and pr.replay([1000], npts)[4] == 1
    # 800 of 1000: N = 6.3 -> 7 trials; a later, larger score inside them takes over and shortens the run
    best, score, trials, N, sta = pr.replay([800] + [10] * 20, npts)
    assert (best, score, trials, sta) == (0, 800, 7, 1) and abs(N - np.log(0.01) / np.log(1 - 0.8 ** 3)) < 1e-12
    assert pr.replay([800, 10, 900] + [10] * 20, npts)[:3] == (2, 900, 4)
    # equal scores do not replace the best (strictly larger, ransac.m:189)
    assert pr.replay([800, 800, 800, 800, 800, 800, 800, 800], npts)[0] == 0
    # never improves after trial 0 and wants thousands of trials: 1001 happen (the break follows the increment)
    best, score, trials, N, sta = pr.replay([3] + [3] * 1000, 4615)
    assert (best, score, trials, sta) == (0, 3, 1001, 1) and N > 1e9
    # ... and with fewer draws than that the status says so
    assert pr.replay([3] * 8, 4615)[2:] == (8, pr.ransac_N(3, 4615), 2)
    # no trial has an inlier: N stays 1, one trial, no solution (ransac.m:224)
    assert pr.replay([0, 0, 50], npts) == (-1, 0, 1, 1.0, 0)
    # zeros in front count as trials once a score has raised N
    assert pr.replay([500, 0, 0] + [0] * 40, npts)[2] == int(np.ceil(np.log(0.01) / np.log(1 - 0.125)))


def test_a_degenerate_draw_scores_zero_and_counts():
    x, y, z, _, draws = _scene(1, 0.5)
    _, _, _, XYZ = pr.crop(x, y, z)
    assert np.isnan(pr.plane_dist(XYZ[:, [5, 5, 9]], XYZ)).all()
    d2 = draws.copy()
    d2[0] = (5, 5, 9)                                           # a repeated point
    d2[1] = (7, 7, 7)
    a, b = pr.plane_fit(x, y, z, draws), pr.plane_fit(x, y, z, d2)
    assert b["counts"][0] == 0 and b["counts"][1] == 0 and np.array_equal(b["counts"][2:], a["counts"][2:])
    # N is still 1 after the first trial, which scored 0: the loop ends there without a solution -- what the reference does, too
    assert (b["sta"], b["n_trials"], b["best"]) == (0, 1, -1)
    with pytest.raises(RuntimeError):
        pr.plane_fit_loops(x, y, z, d2)
    # exactly collinear points (a zero normal) score 0 as well
    X3 = np.array([[0.0, 1.0, 2.0], [0.0, 1.0, 2.0], [1.0, 1.0, 1.0]])
    assert np.isnan(pr.plane_dist(X3, XYZ)).all()


def test_axes_are_undefined_when_a_ray_is_parallel_to_the_plane():
    B = np.array([0.0, 1.0, 0.0, 1.2])                          # the floor y = -1.2
    p_orig = np.array([0.0, -1.2, 3.0])
    assert pr.axes(B, p_orig, np.array([0.1, -1.2, 2.0]))[2] == 1
    assert pr.axes(B, p_orig, np.array([0.1, 0.0, 2.0]))[2] == 3            # the ray through p_ray runs along the floor
    assert pr.axes(B, p_orig, 2.0 * p_orig)[2] == 3                         # both rays meet the plane in the same point: y_axis = 0


def test_second_box_and_few_draws():
    x, y, z, nrm, draws = _scene(2, 0.7)
    a = pr.plane_fit(x, y, z, draws[:8])
    assert a["sta"] == 2 and a["n_trials"] == 8 and a["best"] == int(np.argmax(a["counts"])) and np.abs(a["R"]).max() > 0
    box = (60, 140, 30, 150)
    _, _, _, XYZ = pr.crop(x, y, z, box)
    b = pr.plane_fit(x, y, z, pr.scene_draws(2, XYZ.shape[1]), box)
    R, B, inl, trials, N, best = pr.plane_fit_loops(x, y, z, pr.scene_draws(2, XYZ.shape[1]), box)
    assert b["npts"] == 81 * 121 and (b["best"], b["n_trials"], b["n_inliers"]) == (best, trials, len(inl))
    assert np.abs(b["R"] - R).max() <= 1e-14


def test_heading_RR_closed_form_equals_the_reference_form():
    rng = np.random.default_rng(7)
    for _ in range(30):
        ax = rng.normal(size=3)
        Rp = axis_rot(ax, rng.uniform(-170, 170))
        a, b = pr.heading_RR(Rp), heading_RR_ref(Rp)
        assert np.abs(a - b).max() <= 1e-15 * max(1.0, np.abs(b).max() / 1e-4)
    x, y, z, _, draws = _scene(0, 0.5)
    R = pr.plane_fit(x, y, z, draws)["R"]
    assert np.abs(pr.heading_RR(R.T) - heading_RR_ref(R.T)).max() <= 1e-18
