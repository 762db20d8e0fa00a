"""CPU suite: 3pre_amd/csrc/pre3_reloc.h built for the host (tests/reloc_host_main.cpp) with the address and undefined-behaviour sanitizers and run as a
program -- nothing is loaded into python -- against tests/reloc_ref.py: the rule's branches, the hemisphere flip, where the predicted pose lands, the
committed cases, and the committed tolerance table reproduced."""
import json
import os
import sys

import numpy as np
import pytest

import reloc_cases as rc
import reloc_ref as rr

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_reloc_tolerance as T  # noqa: E402

TAB = json.load(open(os.path.join(HERE, "golden", "reloc_tolerance.json")))
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("reloc_host"))
    exe, sanitized = T.build_host(d, sanitize=True)
    if exe is None:
        pytest.skip("no host C++ compiler")
    assert sanitized, "a host C++ compiler is there but reloc_host_main does not build with -fsanitize=address,undefined: the header is not checked under them"
    return lambda cases: T.run_rule(exe, d, cases)


def a_pose(g, flip=False):
    """x[0:7] and a refit's u = [r*; q*] some decimetres and tenths of a radian away; flip: q* in the other hemisphere than q"""
    x7 = np.concatenate([g.normal(size=3), rc.unit(g.normal(size=4))])
    star = rc.moved_pose(x7, g, 0.3, 0.4)
    if (np.dot(star[3:7], x7[3:7]) > 0) == flip:
        star[3:7] = -star[3:7]
    return x7, star


def test_the_rules_branches(host):
    g = np.random.default_rng(5)
    x7, star = a_pose(g)
    cases = [(x7, star, 1, 12, 12), (x7, star, 1, 11, 12), (x7, star, 0, 40, 12), (x7, star, 2, 40, 12), (x7, star, -1, 40, 12), (x7, star, 1, 6, 6)]
    got = host(cases)
    assert [h["taken"] for h in got] == [1, 0, 0, 0, 0, 1] == [h["takes"] for h in got]
    for c, h in zip(cases, got):
        u, taken = rr.select(*c[:1], c[2], c[3], c[4], c[1])
        assert taken == h["taken"] and np.abs(h["u"] - u).max() <= 8 * EPS
        if not taken:
            assert h["u"].view(np.uint64).tolist() == rr.IDENTITY_U.view(np.uint64).tolist(), "the identity with +0 zeros"
            assert np.abs(h["pose"] - x7).max() <= 4 * EPS


@pytest.mark.parametrize("flip", [False, True])
def test_the_predicted_pose_lands_on_the_refits(host, flip):
    g = np.random.default_rng(11 + flip)
    poses = [a_pose(g, flip) for _ in range(50)]
    got = host([(x7, star, 1, 20, 12) for x7, star in poses])
    for (x7, star), h in zip(poses, got):
        assert h["taken"] == 1 and h["u"][3] >= 0, "dq keeps q in its hemisphere"
        want_q = rc.unit(star[3:7]) * (-1.0 if flip else 1.0)
        assert np.abs(h["pose"][:3] - star[:3]).max() <= 64 * EPS * max(1.0, np.abs(star[:3]).max())
        assert np.abs(h["pose"][3:] - want_q).max() <= 64 * EPS
        assert np.dot(h["pose"][3:], x7[3:7]) > 0
        assert np.abs(rr.predict_pose(x7, h["u"]) - h["pose"]).max() <= 16 * EPS * max(1.0, np.abs(star[:3]).max())


def test_a_state_quaternion_off_the_unit_sphere(host):
    """the state's q is normalised to rounding only: dq = conj(q) (x) q* / |q|^2 divides the norm out"""
    g = np.random.default_rng(21)
    x7, star = a_pose(g)
    x7[3:7] *= 1 + 1e-9
    h = host([(x7, star, 1, 20, 12)])[0]
    assert np.abs(h["pose"][3:] - rc.unit(star[3:7])).max() <= 64 * EPS and np.abs(h["pose"][:3] - star[:3]).max() < 1e-8


@pytest.mark.parametrize("name", rc.names())
def test_every_committed_case_against_the_restatement(host, name):
    sc, r = rc.scene(name), rc.restated(name)
    h = host([(sc["x"][:7], r["pnp_u"], r["sta"], r["n_support"], sc["min_support"])])[0]
    assert h["taken"] == r["taken"] and np.abs(h["u"] - r["u"]).max() <= TAB["tol_u"]
    assert np.abs(h["pose"] - r["pose"]).max() <= TAB["tol_u"]
    if name.startswith("n"):
        assert r["n_corr"] == sc["n_corr"], "the case is built for this count"
    if r["n_corr"] < 6:
        assert (r["winner"], r["sta"], r["taken"]) == (-1, 0, 0)
    else:
        assert r["sta"] == 1 and r["taken"] == 1
        # what the restatement itself is worth on the scene: a few millimetres and tenths of a degree where dozens of inliers average the 0.3 px out
        # (n6 is EPnP's minimum: six points leave the depth loose, centimetres, and the case is there for its count)
        ang, dist = rc.pose_error(r["pose"], sc["truth"])
        print("%s: the restatement is %.3f deg, %.1f mm from the planted pose" % (name, ang, 1e3 * dist))
        if r["n_support"] >= 30:
            assert ang < 0.5 and dist < 0.03, (ang, dist)


def test_the_rho0_and_mixed_cases_are_what_they_say():
    r, sc = rc.restated("n65_rho0"), rc.scene("n65_rho0")
    assert r["n_matches"] == 66 and r["n_corr"] == 65 and (~r["keep"]).sum() == 1
    assert not np.isfinite(rr.landmark_points(sc["types"], sc["off"], sc["x"])[r["pairs"][~r["keep"]][0, 0]]).all()
    m = rc.scene("n64_mixed")
    assert 0 < (m["types"] != 0).sum() < len(m["types"]) and (m["types"][rc.restated("n64_mixed")["pairs"][:, 0]] != 0).any()


def test_the_committed_tolerance_is_reproduced():
    got = T.measure()
    assert got["factor"] == TAB["factor"] == 16 and got["guard_factor"] == TAB["guard_factor"] == 64
    assert list(got["cases"]) == list(TAB["cases"]) == rc.names()
    for k in ("floor_u", "floor_pose", "floor_dist"):
        # (another libm or LAPACK build moves every case by its own last ulps: a small factor, not a percentage)
        assert TAB[k] / 4 <= got[k] <= TAB[k] * 4, k
        assert TAB["tol_" + k[6:]] == 16 * TAB[k]
    assert TAB["guard"] == 64 * TAB["floor_dist"]
    for name, v in got["cases"].items():
        assert v["n_corr"] == TAB["cases"][name]["n_corr"]
        if v["n_hyp"]:
            assert (v["winner"], v["support"], v["taken"]) == tuple(TAB["cases"][name][k] for k in ("winner", "support", "taken"))
            assert v["excluded"] <= 0.05 * v["n_hyp"] and not v["winner_excluded"] and not v["tie"]
