"""GPU suite: pre3_relocalise_refined_seeded (3pre_amd/csrc/pre3_reloc.hip) on f32 and f64 contexts in its three noise modes -- bit
for bit against the chain joined by hand from the calls it fuses, and against tests/pnp_refine_ref.py to 16 times the floors of
tests/golden/pnp_refine_tolerance.json.

The hand-joined chain: pre3_get_landmarks, pre3_siftmatch_f64 on pre3_get_descriptors and the scan, a gather of the finite matches,
pre3_pnp_ransac_refined_seeded, the two rules on the host, pre3_set_process_noise(Pn) when taken, pre3_predict(u), the previous setting restored.  Of the
two rules, reloc_noise_from_pose is evaluated on the host by tests/pnp_refine_ref.py's noise_from_pose, which tests/test_pnp_refine_host.py holds bit
for bit to the header built for the host (no product is fused into a sum on either side).  reloc_select has no such form -- the device build fuses its
products into sums, the host build does not -- so the bit-for-bit chain predicts with the call's own u, as in tests/test_gpu_relocalise.py, which is held
to the restated reloc_select of the chain's pose to 1e-14; and, so that the state comparison does not rest on that u alone, a second chain predicts with
the HOST's u and must end on the same x_k_km1 and P to what 1e-14 in u and one rounding of P's storage type can move them."""
import importlib
import json
import os

import numpy as np
import pytest

import pnp_cases as pc
import pnp_refine_ref as gn
import reloc_cases as rc
import reloc_ref as rr

pytestmark = pytest.mark.gpu

vo = importlib.import_module("3pre_amd.vo")
TAB = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pnp_refine_tolerance.json")))
PN = np.diag([0.05 ** 2] * 3 + [0.02 ** 2] * 4)
PN[0, 4] = PN[4, 0] = 1e-5                          # not diagonal: a transposed read would show
IDENTITY = np.array([0.0, 0, 0, 1, 0, 0, 0])
MODES = ("caller", "pose", "pose_floor")
KEYS = ("pose", "u", "cost", "cov6", "cov7")


def make_filter(pre3, sc, dtype, own_noise=None):
    f = pre3.EkfFilter(sc["cam"], sc["types"], dtype=dtype, max_hyp=16)
    f.set_x_p_k_k(sc["x"], sc["P"])
    f.set_descriptors(sc["bank"].T)
    f.load_scan(sc["scan_desc"].T, sc["scan_pos"].T)
    if own_noise is not None:
        f.set_process_noise(own_noise)
    return f


def params(sc, **over):
    kw = dict(seed=sc["seed"], seq=sc["seq"], thresh=1.5, n_hyp=sc["n_hyp"], thr_px=sc["thr_px"], undistort=True, min_support=sc["min_support"], n_iter=5,
              sigma_px=0.0, noise="pose", Pn=PN)
    kw.update(over)
    return kw


def base_params(kw):
    return {k: v for k, v in kw.items() if k not in ("n_iter", "sigma_px", "noise")}


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64).tolist()


def pnp_bits(r):
    return u64(np.concatenate([r["R"].ravel(), r["T"], r["u"], r["err"]])) + [r["best"], r["sta"], r["n"], r["n_support"]]


def ref_bits(r):
    return u64(np.concatenate([r["R"].ravel(), r["T"], r["u"], r["cost"], r["cov6"].ravel(), r["cov"].ravel(), [r["sigma2"]]])) + [r["sta"], r["n"], r["n_iter"]]


def same_state(a, b):
    return np.array_equal(a.get_x_k_km1(), b.get_x_k_km1()) and np.array_equal(a.get_p_k_km1(), b.get_p_k_km1())


def hand_joined(pre3, g, sc, kw, got):
    """the chain on filter g; the prediction's increment is the call's own (see the module's text)"""
    xyz = g.landmarks()["xyz"]
    m = pre3.siftmatch(g.get_descriptors(), sc["scan_desc"].T, kw["thresh"]).astype(np.int64) - 1
    pairs = m.T.reshape(-1, 2)
    keep = np.isfinite(xyz[pairs[:, 0]]).all(axis=1) if len(pairs) else np.zeros(0, bool)
    kept = pairs[keep]
    Xw, U = xyz[kept[:, 0]], sc["scan_pos"][kept[:, 1], :2]
    out = dict(pairs=pairs, n_corr=len(kept), pnp=None, taken=0, noise_taken="own", Pn=None, host_u=IDENTITY.copy())
    if len(kept) >= 6:
        r = vo.pnp_ransac_refined_seeded(Xw, U, sc["cam"], kw["n_hyp"], kw["thr_px"], kw["seed"], kw["seq"], undistort=kw["undistort"], n_iter=kw["n_iter"],
                                         sigma_px=kw["sigma_px"])
        out.update(pnp=r, taken=int(r["sta"] == 1 and r["n_support"] >= kw["min_support"]))
        if out["taken"]:
            pose_u = r["ref"]["u"] if r["ref"]["sta"] == 1 else r["u"]
            want_u, _ = rr.select(sc["x"][:7], r["sta"], r["n_support"], kw["min_support"], pose_u)
            assert np.abs(got["u"] - want_u).max() < 1e-14, "the increment is not reloc_select's of the chain's pose"
            out["host_u"] = want_u
            if kw["noise"] == "caller" or r["ref"]["sta"] not in (1, 2):
                out.update(noise_taken="caller", Pn=np.array(kw["Pn"]))
            else:
                pose = gn.noise_from_pose(sc["x"][:7], r["ref"]["cov"])
                out.update(noise_taken=kw["noise"], Pn=pose if kw["noise"] == "pose" else pose + kw["Pn"])
    prev, src = g.process_noise
    if out["taken"]:
        g.set_process_noise(out["Pn"])
    g.ekf_prediction(got["u"])
    g.set_process_noise(prev if src == "caller" else None)
    if out["Pn"] is None:
        out["Pn"] = prev
    return out


def check_chain(pre3, sc, dtype, own_noise=None, **over):
    kw = params(sc, **over)
    f, g = make_filter(pre3, sc, dtype, own_noise), make_filter(pre3, sc, dtype, own_noise)
    got = f.relocalise_refined_seeded(**kw)
    ch = hand_joined(pre3, g, sc, kw, got)
    assert np.array_equal(got["match_idx"].T, ch["pairs"]) and got["n_matches"] == len(ch["pairs"]) and got["n_corr"] == ch["n_corr"]
    assert got["taken"] == ch["taken"] and got["noise_taken"] == ch["noise_taken"]
    if ch["pnp"] is None:
        assert got["winner"] == -1 and got["pnp"]["sta"] == 0 and got["ref"]["sta"] == 0 and np.isnan(got["ref"]["cov"]).all()
    else:
        assert pnp_bits(got["pnp"]) == pnp_bits(ch["pnp"]) and np.array_equal(got["inliers"], ch["pnp"]["inliers"])
        assert ref_bits(got["ref"]) == ref_bits(ch["pnp"]["ref"]), "the refinement differs from pre3_pnp_ransac_refined_seeded's"
    if got["taken"] or own_noise is not None:
        assert u64(got["Pn"]) == u64(ch["Pn"]), "Pn differs from the rule evaluated on the host"
    else:                                               # the constant is rebuilt in the launch (sines and cosines of the device), not read from a block
        assert np.allclose(got["Pn"], ch["Pn"], rtol=1e-12, atol=0)
    if not got["taken"]:
        assert u64(got["u"]) == u64(IDENTITY)
    assert same_state(f, g), "x_k_km1 or P differs from the hand-joined chain's"
    # the chain once more with the increment the host's rule gives: u within 1e-14 moves the pose by a few 1e-14 and an entry of P by that fraction of
    # the largest, and P's storage type rounds once more (2^-24 in f32: four of them allowed; 1e-12 in f64)
    h = make_filter(pre3, sc, dtype, own_noise)
    if ch["taken"]:
        h.set_process_noise(ch["Pn"])
    h.ekf_prediction(ch["host_u"])
    Pf, Ph = f.get_p_k_km1(), h.get_p_k_km1()
    assert np.abs(f.get_x_k_km1() - h.get_x_k_km1()).max() < 1e-13, "x_k_km1 differs from the chain under the host's own increment"
    assert np.abs(Pf - Ph).max() <= (4 * 2.0 ** -24 if dtype == "f32" else 1e-12) * np.abs(Pf).max(), "P differs from the chain under the host's own increment"
    h.close()
    assert f.process_noise[1] == g.process_noise[1] == ("caller" if own_noise is not None else "constant")
    if own_noise is not None:
        assert np.array_equal(f.process_noise[0], own_noise)
    f.close(); g.close()
    return got


@pytest.mark.parametrize("noise", MODES)
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("name", rc.names())
def test_the_call_equals_the_hand_joined_chain(pre3, name, dtype, noise):
    sc = rc.scene(name)
    own = np.diag([1e-4] * 3 + [1e-5] * 4) if dtype == "f32" else None
    got = check_chain(pre3, sc, dtype, own_noise=own, noise=noise)
    print("%s %s %s: support %d, sta %d, taken %d, ref.sta %d, noise %s" % (name, dtype, noise, got["pnp"]["n_support"], got["pnp"]["sta"], got["taken"],
                                                                              got["ref"]["sta"], got["noise_taken"]))
    assert got["taken"] == (0 if name == "n5" else 1) and got["noise_taken"] == ("own" if name == "n5" else noise)
    if name != "n5":
        assert got["ref"]["sta"] == 1


def test_sigma_px_and_no_iteration(pre3):
    sc = rc.scene("fixture_2")
    a = check_chain(pre3, sc, "f64", sigma_px=0.3, noise="pose_floor")
    b = check_chain(pre3, sc, "f64", n_iter=0, noise="pose")
    assert a["ref"]["sigma2"] == 0.3 * 0.3 and b["ref"]["sta"] == 2 and b["noise_taken"] == "pose" and u64(b["ref"]["u"]) == u64(b["pnp"]["u"])


# ---- against the restatement -------------------------------------------------------------------------------------------------------------------------
def rel_cov(got, want):
    d = np.sqrt(np.abs(np.diag(want)))
    return float((np.abs(got - want) / np.outer(d, d)).max())


@pytest.mark.parametrize("name", [n for n in rc.names() if n != "n5"])
def test_against_the_restatement(pre3, name):
    sc, w = rc.scene(name), rc.restated(name)
    f = make_filter(pre3, sc, "f64")
    got = f.relocalise_refined_seeded(**params(sc))
    assert got["winner"] == w["winner"] and np.array_equal(got["inliers"], w["inliers"]), "tests/test_gpu_relocalise.py holds the winner outside the guard"
    inl = np.nonzero(w["inliers"])[0]
    # from the device's own refit: the start is an input of the refinement, and the refit has its own tolerance (tests/test_gpu_relocalise.py)
    want = gn.refine(w["Xw"][inl], w["Uu"][inl], sc["cam"], got["pnp"]["R"], got["pnp"]["T"], 5, 0.0, got["pnp"]["sta"])
    h, fin = got["ref"], np.isfinite(want["cost"])
    df = dict(pose=max(np.abs(h["R"] - want["R"]).max(), np.abs(h["T"] - want["T"]).max()), u=np.abs(h["u"] - want["u"]).max(),
              cost=(np.abs(h["cost"][fin] - want["cost"][fin]) / np.maximum(1.0, want["cost"][fin])).max(), cov6=rel_cov(h["cov6"], want["cov6"]),
              cov7=rel_cov(h["cov"], want["cov"]), pn=rel_cov(got["Pn"], gn.noise_from_pose(sc["x"][:7], want["cov"])))
    print("%s: " % name + "  ".join("%s %.2e (tol %.2e)" % (k, df[k], TAB["tol_" + k]) for k in KEYS + ("pn",)))
    assert h["sta"] == want["sta"] == 1 and all(df[k] <= TAB["tol_" + k] for k in KEYS + ("pn",))
    pose = f.get_x_k_km1()[:7]
    a0, d0 = rc.pose_error(w["pose"], sc["truth"])
    a1, d1 = rc.pose_error(pose, sc["truth"])
    print("   against the planted pose: EPnP %.3f deg %.2f mm, refined %.3f deg %.2f mm" % (a0, 1e3 * d0, a1, 1e3 * d1))
    assert np.abs(pose - rr.predict_pose(sc["x"][:7], got["u"])).max() < 1e-14 and d1 < d0
    assert np.abs(pose[:3] - want["u"][:3]).max() <= 16 * TAB["tol_u"] + 1e-14
    f.close()


# ---- the not-taken paths -------------------------------------------------------------------------------------------------------------------------------
def sta2_scene():
    """tests/pnp_cases.py's outlier_sta2 as map and scan (as tests/test_gpu_relocalise.py builds it): the refit ends with sta = 2"""
    Xw, U, cam = pc.outlier_sta2()
    N = len(Xw)
    g = np.random.default_rng(3)
    bank = rc.descriptors(g, N)
    x = np.concatenate([[0, 0, 0, 1, 0, 0, 0], np.zeros(6), Xw.ravel()]).astype(np.float64)
    A = g.normal(size=(len(x), len(x))) * 1e-3
    pos = np.column_stack([U, np.ones(N), np.zeros(N)])
    return dict(name="sta2", types=np.ones(N, np.int32), off=(13 + 3 * np.arange(N)).astype(np.int32), x=x, P=A @ A.T + 1e-6 * np.eye(len(x)), bank=bank,
                scan_desc=bank.copy(), scan_pos=pos, cam=np.array(cam, np.float64), seed=9, seq=1, n_hyp=16, thr_px=1e7, min_support=12, truth=None)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("which", ["n5", "min_support", "sta2"])
def test_not_taken_is_the_identity_prediction_on_the_contexts_own_noise(pre3, which, dtype):
    own = np.diag([2e-4] * 3 + [3e-5] * 4) if dtype == "f32" else None
    over = {}
    if which == "n5":
        sc = rc.scene("n5")
    elif which == "min_support":
        sc = rc.scene("fixture_2")
        over = dict(min_support=rc.restated("fixture_2")["n_support"] + 1)
    else:
        sc, over = sta2_scene(), dict(undistort=False)
    f, g = make_filter(pre3, sc, dtype, own), make_filter(pre3, sc, dtype, own)
    got = f.relocalise_refined_seeded(**params(sc, noise="pose_floor", **over))
    g.ekf_prediction(IDENTITY)
    assert got["taken"] == 0 and got["noise_taken"] == "own" and u64(got["u"]) == u64(IDENTITY)
    assert (which != "n5" or got["ref"]["sta"] == 0) and (which != "sta2" or got["pnp"]["sta"] == 2) and (which != "min_support" or got["ref"]["sta"] == 1)
    if own is not None:
        assert u64(got["Pn"]) == u64(own)
    else:                                               # the constant is rebuilt in the launch, not read from a block
        assert np.allclose(got["Pn"], g.process_noise[0], rtol=1e-12, atol=0)
    assert same_state(f, g) and f.process_noise[1] == ("caller" if own is not None else "constant")
    f.close(); g.close()


# ---- wait=False, and the unrefined call beside it --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_the_form_that_does_not_wait(pre3, dtype):
    sc = rc.scene("fixture_1")
    f, g = make_filter(pre3, sc, dtype), make_filter(pre3, sc, dtype)
    assert f.relocalise_refined_seeded(wait=False, **params(sc, noise="pose_floor")) is None
    res = g.relocalise_refined_seeded(**params(sc, noise="pose_floor"))
    outs = []
    for h in (f, g):
        ic = h.matching_sift_based(1.5)
        st = h.step_predicted_seeded(seed=5, seq=7, n_draw=16)
        outs.append((ic, st))
    assert res["taken"] == 1 and len(outs[0][0]["meas_idx"]) > 30, "the search finds the map again behind the relocalised prediction"
    assert np.array_equal(outs[0][0]["meas_idx"], outs[1][0]["meas_idx"]) and np.array_equal(outs[0][0]["z"], outs[1][0]["z"]) and outs[0][1] == outs[1][1]
    assert np.array_equal(f.get_x_k_k(), g.get_x_k_k()) and np.array_equal(f.get_p_k_k(), g.get_p_k_k())
    f.close(); g.close()


def test_the_unrefined_call_gives_the_same_bits_before_and_after_a_refined_one(pre3):
    sc = rc.scene("fixture_3")
    f = make_filter(pre3, sc, "f32")
    kw = base_params(params(sc))

    def plain():
        f.set_x_p_k_k(sc["x"], sc["P"])
        r = f.relocalise_seeded(**kw)
        return pnp_bits(r["pnp"]) + u64(r["u"]) + [r["n_matches"], r["n_corr"], r["winner"], r["taken"]] + r["inliers"].tolist(), f.get_x_k_km1(), f.get_p_k_km1()

    before = plain()
    f.set_x_p_k_k(sc["x"], sc["P"])
    assert f.relocalise_refined_seeded(**params(sc, noise="pose_floor"))["taken"] == 1
    after = plain()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2])
    f.close()


def test_refusals_queue_nothing(pre3):
    sc = rc.scene("fixture_1")
    f = make_filter(pre3, sc, "f64")
    x, P = f.get_x_k_k(), f.get_p_k_k()
    for over in (dict(n_iter=-1), dict(n_iter=11), dict(sigma_px=-1.0), dict(sigma_px=np.nan), dict(noise=3), dict(noise=-1), dict(n_hyp=0), dict(min_support=5)):
        with pytest.raises(pre3.Pre3Error) as e:
            f.relocalise_refined_seeded(**params(sc, **over))
        assert e.value.code == -1, over
    assert np.array_equal(f.get_x_k_k(), x) and np.array_equal(f.get_p_k_k(), P)
    f.close()
