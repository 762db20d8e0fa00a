"""CPU suite: 3pre_amd/csrc/pre3_pnpref.h and the new part of pre3_reloc.h built for the host (tests/pnp_refine_host_main.cpp) with the address and
undefined-behaviour sanitizers and run as a program -- nothing is loaded into python -- against tests/pnp_refine_ref.py: every branch of the taking rule
and of sta from hand-made inputs, the committed cases, reloc_noise_from_pose bit for bit, and the committed tolerance table reproduced."""
import json
import os
import sys

import numpy as np
import pytest

import epnp_ref as ref
import pnp_cases as pc
import pnp_refine_ref as gn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_pnp_refine_tolerance as T  # noqa: E402

TAB = json.load(open(os.path.join(HERE, "golden", "pnp_refine_tolerance.json")))
CAM = pc.fixture_cam()
RISING_START = np.array([0.78, -0.2, 1.88, -0.04, -0.4, 0.57])          # tests/test_pnp_refine_ref.py


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("pnp_refine_host"))
    exe, sanitized = T.build_host(d, sanitize=True)
    if exe is None:
        pytest.skip("no host C++ compiler")
    if not sanitized:                                   # the plain build would pass without the coverage this file is for
        pytest.skip("the link with -fsanitize=address,undefined failed: no sanitizer runtime for this compiler")
    return lambda cases: T.run_host(exe, d, cases)


@pytest.fixture(scope="module")
def scene():
    Xw, U, _, _, _ = pc.sr_scene(12, 1003)
    e = ref.epnp(Xw, U, CAM)
    return Xw, U, e["R"], e["T"]


def case(Xw, U, R0, T0, n_iter=5, sigma_px=0.0, sta_in=1, x7=T.X7, cam=CAM):
    return dict(Xw=Xw, U=U, cam=cam, R0=R0, T0=T0, n_iter=n_iter, sigma_px=sigma_px, sta_in=sta_in, x7=x7)


def test_every_committed_case_against_the_restatement(host):
    named = T.cases()
    for (name, c), h in zip(named.items(), host(list(named.values()))):
        r, pn = T.restate(c)
        assert h["sta"] == r["sta"] == 1, name
        df = T.diffs(h, r, pn)
        assert all(df[k] <= 4 * TAB["floor_" + k] for k in T.KEYS), (name, df)
        assert np.array_equal(h["cov"], h["cov"].T) and np.array_equal(h["cov6"], h["cov6"].T) and np.array_equal(h["Pn"], h["Pn"].T)
        # reloc_noise_from_pose fuses no product into a sum and the restatement follows its order: equal bits from the host's own cov7
        assert gn.noise_from_pose(c["x7"], h["cov"]).view(np.uint64).tolist() == h["Pn"].view(np.uint64).tolist(), name


def test_every_iteration_count_and_both_noise_sources(host, scene):
    Xw, U, R0, T0 = scene
    cs = [case(Xw, U, R0, T0, k, s) for k in range(11) for s in (0.0, 0.3)]
    for c, h in zip(cs, host(cs)):
        r, pn = T.restate(c)
        assert h["sta"] == r["sta"] == (2 if c["n_iter"] == 0 else 1)
        assert np.isnan(h["cost"][c["n_iter"] + 1:]).all() and np.isfinite(h["cost"][:c["n_iter"] + 1]).all()
        df = T.diffs(h, r, pn)
        assert all(df[k] <= TAB["tol_" + k] for k in T.KEYS), (c["n_iter"], df)
        assert h["sigma2"] == (0.3 * 0.3 if c["sigma_px"] else h["cost"][c["n_iter"]] / (2 * len(Xw) - 6))
    h0 = host([case(Xw, U, R0, T0, 0)])[0]
    assert np.array_equal(h0["R"], R0) and np.array_equal(h0["T"], T0)


def test_every_branch_of_the_taking_rule_and_of_sta(host, scene):
    Xw, U, R0, T0 = scene
    Rr, Tr = gn.perturb(R0, T0, RISING_START)
    nan = Xw.copy()
    nan[3, 1] = np.nan
    nanu = U.copy()
    nanu[0, 0] = np.inf
    behind = Xw.copy()
    behind[2] = R0.T @ (np.array([0.1, 0.1, -1.0]) - T0)            # camera-frame z = -1 at the input pose, and at any pose a few steps away
    same = np.tile(Xw[:1], (12, 1))
    cs = [case(Xw, U, Rr, Tr, 1), case(nan, U, R0, T0), case(Xw, nanu, R0, T0), case(behind, U, R0, T0), case(same, U, R0, T0), case(Xw, U, R0, T0, 0),
          case(Xw, U, R0, T0, sta_in=0), case(Xw, U, R0, T0, sta_in=-1), case(Xw, U, R0, T0, sta_in=2), case(Xw[:5], U[:5], R0, T0), case(same, U, R0, T0, 0)]
    hs = host(cs)
    assert [h["sta"] for h in hs] == [2, -1, -1, -1, -1, 2, 0, 0, 1, 0, -1]
    assert [h["sta"] for h in hs] == [T.restate(c)[0]["sta"] for c in cs]
    rising = hs[0]
    assert rising["cost"][1] > 10 * rising["cost"][0] and np.array_equal(rising["R"], Rr) and np.array_equal(rising["T"], Tr) and np.isfinite(rising["cov"]).all()
    for c, h in zip(cs, hs):
        if h["sta"] in (0, -1):                                    # the input's pose, no covariance
            assert np.array_equal(h["R"], c["R0"]) and np.array_equal(h["T"], c["T0"]) and np.abs(h["u"] - ref.pair_u(c["R0"], c["T0"])).max() < 1e-15
            assert np.isnan(h["cov"]).all() and np.isnan(h["cov6"]).all() and np.isnan(h["sigma2"]) and np.isnan(h["Pn"]).all()
        if h["sta"] == 0:
            assert np.isnan(h["cost"]).all()


def test_the_committed_tolerance_is_reproduced():
    got = T.measure()
    assert got["factor"] == TAB["factor"] == 16 and got["n_iter"] == TAB["n_iter"] and list(got["cases"]) == list(TAB["cases"])
    assert got["left_out"] == TAB["left_out"] == []
    assert sorted(TAB["cases"]) == sorted(["sr_%d" % n for n in T.SR_SIZES] + ["reloc_" + k for k in ("fixture_1", "fixture_2", "fixture_3", "n6", "n64_mixed", "n65_rho0")])
    for k in T.KEYS:
        # (another libm or BLAS build moves every case by its own last ulps: a small factor, not a percentage)
        assert TAB["floor_" + k] / 4 <= got["floor_" + k] <= TAB["floor_" + k] * 4, k
        assert TAB["tol_" + k] == 16 * TAB["floor_" + k]
    assert TAB["floor_pose"] < 1e-13 and TAB["floor_cov7"] < 1e-11
