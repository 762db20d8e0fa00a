"""CPU suite: 3pre_amd/csrc/pre3_pnp.h built for the host (tests/pnp_host_main.cpp) with the address and undefined-behaviour sanitizers and run as a
program -- nothing is loaded into python -- against tests/epnp_ref.py on every committed case, and the committed tolerance table reproduced."""
import json
import os
import sys

import numpy as np
import pytest

import epnp_ref as ref
import pnp_cases as pc

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_pnp_tolerance as T  # noqa: E402

TAB = json.load(open(os.path.join(HERE, "golden", "pnp_tolerance.json")))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("pnp_host"))
    exe, sanitized = T.build_host(d, sanitize=True)
    if exe is None:
        pytest.skip("no host C++ compiler")
    if not sanitized:
        print("pnp_host_main: the sanitized link failed; running the plain build")
    return lambda cases: T.run_host(exe, d, cases)


def test_every_committed_case_against_the_restatement(host):
    named = pc.tolerance_cases()
    for (name, (Xw, U, cam)), h in zip(named.items(), host(list(named.values()))):
        r = ref.epnp(Xw, U, cam)
        df = T.diffs(h, r)
        assert df is not None, name
        own = name in T.OWN_FLOOR
        lim = [4 * TAB["cases"][name][k] for k in ("pose", "err", "dist")] if own else [TAB["tol_pose"], TAB["tol_err"], TAB["tol_dist"]]
        assert df[0] <= lim[0] and df[1] <= lim[1] and df[2] <= lim[2], (name, df)
        assert np.abs(h["u"] - ref.pair_u(h["R"], h["T"])).max() < 1e-12
        assert h["sweeps"] <= 10 and np.abs(h["w"] - r["w"]).max() <= 1e-12 * r["w"].max()


def test_the_hypotheses_of_a_ransac_scene(host):
    sc = pc.ransac_scene(65)
    hs = host([(sc["Xw"][d], sc["U"][d], sc["cam"]) for d in sc["draws"]])
    for d, h in zip(sc["draws"], hs):
        df = T.diffs(h, ref.epnp(sc["Xw"][d], sc["U"][d], sc["cam"]))
        assert df is not None and df[0] <= TAB["tol_pose"] and df[1] <= TAB["tol_err"] and df[2] <= TAB["tol_dist"]


def test_a_non_finite_coordinate(host):
    Xw, U, _, _, _ = pc.sr_scene(12, 9)
    bad, badu = Xw.copy(), U.copy()
    bad[3, 2] = np.nan
    badu[11, 1] = -np.inf
    h = host([(bad, U, pc.fixture_cam()), (Xw, badu, pc.fixture_cam()), (Xw, U, pc.fixture_cam())])
    assert h[0]["sta"] == -1 and h[1]["sta"] == -1 and h[2]["sta"] == 1
    assert ref.epnp(bad, U, pc.fixture_cam())["sta"] == -1 and ref.epnp(Xw, badu, pc.fixture_cam())["sta"] == -1


def test_the_committed_tolerance_is_reproduced():
    got = T.measure()
    assert got["factor"] == TAB["factor"] == 16 and got["guard_factor"] == TAB["guard_factor"] == 64
    assert list(got["cases"]) == list(TAB["cases"]) and list(got["hypotheses"]) == list(TAB["hypotheses"])
    for k in ("floor_pose", "floor_err", "floor_dist"):
        # (another libm or LAPACK build moves every case by its own last ulps: a small factor, not a percentage)
        assert TAB[k] / 4 <= got[k] <= TAB[k] * 4, k
        assert TAB["tol_" + k[6:]] == 16 * TAB[k]
    assert TAB["guard"] == 64 * TAB["floor_dist"]
    assert all(v["decide_differently"] == 0 for v in got["hypotheses"].values())
    # the floors the issue's scratch figures lead one to expect: 5e-10 worst over six-point samples, 1e-12 on the whole sets
    assert TAB["floor_pose"] < 5e-9 and max(v["pose"] for k, v in TAB["cases"].items() if k not in T.OWN_FLOOR) < 5e-12
