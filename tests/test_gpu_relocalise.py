"""GPU suite: pre3_relocalise_seeded (3pre_amd/csrc/pre3_reloc.hip) on f32 and f64 contexts -- bit for bit against the chain joined
by hand from the calls it fuses, and against tests/reloc_ref.py to 16 times what tests/golden/make_reloc_tolerance.py measured between the same headers
run on the host and that restatement; decisions exactly, outside the guard.

The hand-joined chain: pre3_get_landmarks, pre3_siftmatch_f64 on pre3_get_descriptors and the scan, a gather of the finite matches,
pre3_pnp_ransac_seeded, pre3_set_process_noise(Pn_reloc) when taken, pre3_predict(u), the previous noise setting restored.  The step that follows the
call in the wait=False test is pre3_ic_search and pre3_step_predicted_seeded: the seeded step over the measurements the search installs."""
import ctypes as C
import importlib
import json
import os

import numpy as np
import pytest

import epnp_ref as ref
import pnp_cases as pc
import reloc_cases as rc
import reloc_ref as rr

pytestmark = pytest.mark.gpu

vo = importlib.import_module("3pre_amd.vo")
_lib = importlib.import_module("3pre_amd._lib")
TAB = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reloc_tolerance.json")))
PN = np.diag([0.05 ** 2] * 3 + [0.02 ** 2] * 4)
PN[0, 4] = PN[4, 0] = 1e-5                          # not diagonal: a transposed read would show
IDENTITY = np.array([0.0, 0, 0, 1, 0, 0, 0])
E_ARG, E_STATE = -1, -4


def make_filter(pre3, sc, dtype, own_noise=None):
    f = pre3.EkfFilter(sc["cam"], sc["types"], dtype=dtype, max_hyp=16)
    f.set_x_p_k_k(sc["x"], sc["P"])
    f.set_descriptors(sc["bank"].T)
    f.load_scan(sc["scan_desc"].T, sc["scan_pos"].T)
    if own_noise is not None:
        f.set_process_noise(own_noise)
    return f


def params(sc, **over):
    kw = dict(seed=sc["seed"], seq=sc["seq"], thresh=1.5, n_hyp=sc["n_hyp"], thr_px=sc["thr_px"], undistort=True, min_support=sc["min_support"], Pn=PN)
    kw.update(over)
    return kw


def pnp_bits(r):
    return np.concatenate([r["R"].ravel(), r["T"], r["u"], r["err"]]).view(np.uint64).tolist() + [r["best"], r["sta"], r["n"], r["n_support"]]


def hand_joined(pre3, f, sc, kw, u):
    """the chain on filter f, its prediction made with the call's own increment u; returns dict(pairs, n_corr, pnp, inliers, support, taken)"""
    xyz = f.landmarks()["xyz"]
    m = pre3.siftmatch(f.get_descriptors(), sc["scan_desc"].T, kw["thresh"]).astype(np.int64) - 1
    pairs = m.T.reshape(-1, 2)
    keep = np.isfinite(xyz[pairs[:, 0]]).all(axis=1) if len(pairs) else np.zeros(0, bool)
    kept = pairs[keep]
    Xw, U = xyz[kept[:, 0]], sc["scan_pos"][kept[:, 1], :2]
    out = dict(pairs=pairs, n_corr=len(kept), pnp=None, inliers=np.zeros(len(kept), np.int32), taken=0, Xw=Xw, U=U)
    if len(kept) >= 6:
        r = vo.pnp_ransac_seeded(Xw, U, sc["cam"], kw["n_hyp"], kw["thr_px"], kw["seed"], kw["seq"], undistort=kw["undistort"], hyp_results=True)
        out.update(pnp=r, inliers=r["inliers"], support=r["support"])
        out["taken"] = int(r["sta"] == 1 and r["n_support"] >= kw["min_support"])
    prev, src = f.process_noise
    if out["taken"]:
        f.set_process_noise(kw["Pn"])
    f.ekf_prediction(u)
    f.set_process_noise(prev if src == "caller" else None)
    return out


def same_state(a, b):
    return np.array_equal(a.get_x_k_km1(), b.get_x_k_km1()) and np.array_equal(a.get_p_k_km1(), b.get_p_k_km1())


# ---- chain identity ----------------------------------------------------------------------------------------------------------------------------------
def check_chain(pre3, sc, dtype, own_noise=None, **over):
    kw = params(sc, **over)
    f, g = make_filter(pre3, sc, dtype, own_noise), make_filter(pre3, sc, dtype, own_noise)
    got = f.relocalise_seeded(**kw)
    ch = hand_joined(pre3, g, sc, kw, got["u"])
    assert np.array_equal(got["match_idx"].T, ch["pairs"]) and got["n_matches"] == len(ch["pairs"]) and got["n_corr"] == ch["n_corr"]
    assert got["taken"] == ch["taken"]
    if ch["pnp"] is None:
        assert got["winner"] == -1 and got["pnp"]["sta"] == 0 and got["pnp"]["n_support"] == 0 and np.array_equal(got["pnp"]["u"], IDENTITY)
    else:
        assert pnp_bits(got["pnp"]) == pnp_bits(ch["pnp"]), "the refit differs from pre3_pnp_ransac_seeded's"
        assert np.array_equal(got["inliers"], ch["inliers"])
        assert 0 <= got["winner"] < kw["n_hyp"] and ch["support"][got["winner"]] == ch["support"].max() == got["pnp"]["n_support"]
        assert ch["pnp"]["hyp"][got["winner"]]["n_support"] == got["inliers"].sum()
    if not got["taken"]:
        assert got["u"].view(np.uint64).tolist() == IDENTITY.view(np.uint64).tolist()
    assert same_state(f, g), "x_k_km1 or P differs from the hand-joined chain's"
    assert f.process_noise[1] == g.process_noise[1] == ("caller" if own_noise is not None else "constant")
    if own_noise is not None:
        assert np.array_equal(f.process_noise[0], own_noise)
    f.close(); g.close()
    return got


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("name", rc.names())
def test_the_call_equals_the_hand_joined_chain(pre3, name, dtype):
    sc = rc.scene(name)
    got = check_chain(pre3, sc, dtype)
    print("%s %s: %d matches, %d correspondences, winner %d, support %d, sta %d, taken %d" % (name, dtype, got["n_matches"], got["n_corr"], got["winner"],
                                                                                             got["pnp"]["n_support"], got["pnp"]["sta"], got["taken"]))
    assert got["taken"] == (0 if name == "n5" else 1)


@pytest.mark.parametrize("n_hyp", [1, 64, 200])
@pytest.mark.parametrize("undistort", [False, True])
def test_parameter_sweep(pre3, n_hyp, undistort):
    own = np.diag([1e-4] * 3 + [1e-5] * 4)
    got = check_chain(pre3, rc.scene("fixture_3"), "f32", own_noise=own, n_hyp=n_hyp, undistort=undistort)
    assert got["n_corr"] == rc.restated("fixture_3")["n_corr"]


# ---- against the restatement -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rc.names())
def test_against_the_restatement(pre3, name):
    sc, want = rc.scene(name), rc.restated(name)
    f = make_filter(pre3, sc, "f64")
    got = f.relocalise_seeded(**params(sc))
    assert np.array_equal(got["match_idx"].T, want["pairs"]) and (got["n_matches"], got["n_corr"], got["taken"]) == (want["n_matches"], want["n_corr"], want["taken"])
    if want["ransac"] is None:
        assert got["winner"] == -1 and got["pnp"]["sta"] == 0
        f.close()
        return
    skip, tie = ref.guard_excluded(want["ransac"], sc["thr_px"], TAB["guard"] * max(1.0, sc["thr_px"]))
    assert not tie and not skip[want["winner"]], "the committed cases keep their winner outside the guard (make_reloc_tolerance.py asserts it)"
    assert got["winner"] == want["winner"] and np.array_equal(got["inliers"], want["inliers"])
    assert (got["pnp"]["sta"], got["pnp"]["best"], got["pnp"]["n_support"]) == (want["pnp"]["sta"], want["pnp"]["best"], want["n_support"])
    dp = max(np.abs(got["pnp"]["R"] - want["pnp"]["R"]).max(), np.abs(got["pnp"]["T"] - want["pnp"]["T"]).max())
    du = np.abs(got["u"] - want["u"]).max()
    pose = f.get_x_k_km1()[:7]
    ang0, dist0 = rc.pose_error(want["pose"], sc["truth"])
    ang, dist = rc.pose_error(pose, sc["truth"])
    print("%s: pose %.3e (tol %.3e)  u %.3e (tol %.3e); truth: restatement %.4f deg %.2f mm, device %.4f deg %.2f mm" %
          (name, dp, TAB["tol_pose"], du, TAB["tol_u"], ang0, 1e3 * dist0, ang, 1e3 * dist))
    assert dp <= TAB["tol_pose"] and du <= TAB["tol_u"]
    assert np.abs(pose - want["pose"]).max() <= TAB["tol_u"] and np.abs(pose - rr.predict_pose(sc["x"][:7], got["u"])).max() < 1e-14
    # no worse against the planted truth than the restatement, plus the tolerance (radians -> degrees for the angle)
    assert ang <= ang0 + np.degrees(4 * TAB["tol_u"]) and dist <= dist0 + 2 * TAB["tol_u"]
    f.close()


# ---- the not-taken paths -------------------------------------------------------------------------------------------------------------------------------
def sta2_scene():
    """tests/pnp_cases.py's outlier_sta2 as map and scan: its points as Cartesian landmarks, its pixels as the scan's; a threshold that makes every
    correspondence an inlier, so that the refit is the whole-set answer -- dimension 3 entered and ending above 20: sta = 2"""
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
    own = np.diag([2e-4] * 3 + [3e-5] * 4) if dtype == "f32" else None          # a caller's noise on one, the constant on the other
    over = {}
    if which == "n5":
        sc = rc.scene("n5")
    elif which == "min_support":
        sc = rc.scene("fixture_2")
        over = dict(min_support=rc.restated("fixture_2")["n_support"] + 1)
    else:
        sc, over = sta2_scene(), dict(undistort=False)
    f, g = make_filter(pre3, sc, dtype, own), make_filter(pre3, sc, dtype, own)
    got = f.relocalise_seeded(**params(sc, **over))
    g.ekf_prediction(IDENTITY)
    print("%s %s: n_corr %d, sta %d, support %d, winner %d" % (which, dtype, got["n_corr"], got["pnp"]["sta"], got["pnp"]["n_support"], got["winner"]))
    assert got["taken"] == 0 and got["u"].view(np.uint64).tolist() == IDENTITY.view(np.uint64).tolist()
    if which == "n5":
        assert got["n_corr"] == 5 and got["winner"] == -1 and got["pnp"]["sta"] == 0
    elif which == "min_support":
        assert got["pnp"]["sta"] == 1 and got["pnp"]["n_support"] == over["min_support"] - 1
    else:
        assert got["pnp"]["sta"] == 2 and got["n_corr"] == len(sc["types"]) and ref.epnp(*pc.outlier_sta2())["sta"] == 2
    assert same_state(f, g)
    assert f.process_noise[1] == ("caller" if own is not None else "constant")
    if own is not None:
        assert np.array_equal(f.process_noise[0], own)
    f.close(); g.close()


# ---- wait=False ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_the_form_that_does_not_wait(pre3, dtype):
    sc = rc.scene("fixture_1")
    f, g = make_filter(pre3, sc, dtype), make_filter(pre3, sc, dtype)
    assert f.relocalise_seeded(wait=False, **params(sc)) is None
    res = g.relocalise_seeded(**params(sc))
    outs = []
    for h in (f, g):
        ic = h.matching_sift_based(1.5)
        st = h.step_predicted_seeded(seed=5, seq=7, n_draw=16)
        outs.append((ic, st))
    assert res["taken"] == 1 and len(outs[0][0]["meas_idx"]) > 30, "the search finds the map again behind the relocalised prediction"
    assert np.array_equal(outs[0][0]["meas_idx"], outs[1][0]["meas_idx"]) and np.array_equal(outs[0][0]["z"], outs[1][0]["z"]) and outs[0][1] == outs[1][1]
    assert np.array_equal(f.get_x_k_k(), g.get_x_k_k()) and np.array_equal(f.get_p_k_k(), g.get_p_k_k())
    f.close(); g.close()


# ---- what the call leaves alone ----------------------------------------------------------------------------------------------------------------------
def snapshot(f, bank=True, predicted=False):
    """everything a refused call must leave alone; bank=False on a context without descriptors, predicted=True where the buffers hold the prediction"""
    lf = f.landmark_fields()
    x, P = (f.get_x_k_km1(), f.get_p_k_km1()) if predicted else (f.get_x_k_k(), f.get_p_k_k())
    return dict(x=x, P=P, h=lf["h"], has_h=lf["has_h"], Hc=lf["Hc"], Hl=lf["Hl"], S=lf["S"], bank=f.get_descriptors() if bank else None,
                flags=np.concatenate(f.get_flags()), pn=f.process_noise[0], src=f.process_noise[1])


def same_snapshot(a, b, keys=None):
    return all(np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k] for k in (keys or a))


def test_h_flags_and_the_bank_are_untouched(pre3):
    sc = rc.scene("n64_mixed")
    f = make_filter(pre3, sc, "f32")
    # a frame as the filter ran it before it got lost: a prediction, the search, a step -- h, H, S, z and the flags are set
    f.ekf_prediction(IDENTITY)
    ic = f.matching_sift_based(1.5)
    f.step_predicted_seeded(seed=1, seq=1, n_draw=8)
    assert len(ic["match_idx"].T) >= 60 and f.landmark_fields()["has_h"].sum() > 30
    before = snapshot(f)
    got = f.relocalise_seeded(**params(sc))
    after_fields = f.landmark_fields()
    assert got["n_corr"] >= 6
    for k in ("h", "has_h", "Hc", "Hl", "S"):
        assert np.array_equal(before[k], after_fields[k]), k
    assert np.array_equal(before["bank"], f.get_descriptors()) and np.array_equal(before["flags"], np.concatenate(f.get_flags()))
    assert np.array_equal(before["x"], f.get_x_k_k()), "x_k_k stays; the prediction is written to x_k_km1"
    f.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------------
def refused(f, code, bank=True, predicted=False, **kw):
    before = snapshot(f, bank, predicted)
    with pytest.raises(_lib.Pre3Error) as e:
        f.relocalise_seeded(**kw)
    assert e.value.code == code, (e.value.code, str(e.value))
    assert same_snapshot(before, snapshot(f, bank, predicted)), "a refused call changed the context"


def test_refusals_leave_the_context_unchanged(pre3):
    sc = rc.scene("n64_mixed")
    ok = params(sc)
    f = make_filter(pre3, sc, "f32", np.diag([2e-4] * 3 + [3e-5] * 4))
    bad_pn = [PN * np.nan, -PN, PN + np.eye(7, k=1) * 1e-9]
    for over in ([dict(n_hyp=0), dict(n_hyp=701), dict(thr_px=0.0), dict(thr_px=-1.0), dict(thr_px=np.nan), dict(thr_px=np.inf), dict(thresh=0.0),
                  dict(thresh=np.nan), dict(thresh=np.inf), dict(min_support=5)] + [dict(Pn=p) for p in bad_pn]):
        refused(f, E_ARG, **dict(ok, **over))
    # a null Pn_reloc (the wrapper always passes one)
    before = snapshot(f)
    rc_ = _lib.lib.pre3_relocalise_seeded(f._ctx, 1.5, 64, 1, 0, 2.0, 1, 12, None, None, None, None)
    assert rc_ == E_ARG and same_snapshot(before, snapshot(f))
    # the covariance buffer holds the prediction
    f.ekf_prediction(IDENTITY)
    refused(f, E_STATE, predicted=True, **ok)
    f.close()
    # no descriptor bank and no scan; a bank but no scan; a scan but no bank
    g = pre3.EkfFilter(sc["cam"], sc["types"], dtype="f64", max_hyp=16)
    g.set_x_p_k_k(sc["x"], sc["P"])
    refused(g, E_STATE, bank=False, **ok)
    g.set_descriptors(sc["bank"].T)
    refused(g, E_STATE, **ok)
    g.close()
    g = pre3.EkfFilter(sc["cam"], sc["types"], dtype="f64", max_hyp=16)
    g.set_x_p_k_k(sc["x"], sc["P"])
    g.load_scan(sc["scan_desc"].T, sc["scan_pos"].T)
    refused(g, E_STATE, bank=False, **ok)
    g.close()
    # a map below six landmarks
    small = rc.scene("n5")
    keep = 5
    n5 = 13 + 6 * keep
    g = pre3.EkfFilter(small["cam"], small["types"][:keep], dtype="f64", max_hyp=16)
    g.set_x_p_k_k(small["x"][:n5], small["P"][:n5, :n5])
    g.set_descriptors(small["bank"][:keep].T)
    g.load_scan(small["scan_desc"].T, small["scan_pos"].T)
    refused(g, E_ARG, **params(small))
    g.close()


def test_a_map_above_the_limit_is_refused(pre3):
    """N above pre3_reloc_limits: refused on the map's size alone, before anything else is looked at (Cartesian landmarks keep the context small)"""
    lim = np.zeros(2, np.int32)
    _lib.check(_lib.lib.pre3_reloc_limits(_lib.dptr(lim)))
    N = int(lim[0]) + 1
    f = pre3.EkfFilter(rc.scene("n6")["cam"], np.ones(N, np.int32), dtype="f32", max_hyp=4)
    with pytest.raises(_lib.Pre3Error) as e:
        f.relocalise_seeded(seed=1, Pn=PN)
    assert e.value.code == E_ARG and "pre3_reloc_limits" in str(e.value)
    f.close()


def test_no_camera_is_refused(pre3):
    sc = rc.scene("n6")
    lib, ctx = _lib.lib, C.c_void_p()
    N, x, P = len(sc["types"]), _lib.f64(sc["x"]), _lib.f64(sc["P"])
    _lib.check(lib.pre3_create(C.byref(ctx), 0, _lib.F64, N, 16))
    try:
        t = _lib.i32(sc["types"])
        _lib.check(lib.pre3_set_map(ctx, N, _lib.dptr(t)))
        _lib.check(lib.pre3_set_state(ctx, _lib.X_K_K, len(x), _lib.dptr(x), _lib.dptr(P)))
        b, sd, sp = _lib.f64(sc["bank"]), _lib.f64(sc["scan_desc"]), _lib.f64(sc["scan_pos"])
        _lib.check(lib.pre3_set_descriptors(ctx, 0, N, _lib.dptr(b)))
        _lib.check(lib.pre3_set_scan(ctx, len(sd), _lib.dptr(sd), _lib.dptr(sp)))
        pn = _lib.f64(PN)
        assert lib.pre3_relocalise_seeded(ctx, 1.5, 1, 1, 0, 2.0, 1, 6, _lib.dptr(pn), None, None, None) == E_ARG
        assert b"camera" in lib.pre3_last_error()
        x1 = np.zeros(len(x))
        _lib.check(lib.pre3_get_state(ctx, _lib.X_K_K, len(x), _lib.dptr(x1), None))
        assert np.array_equal(x1, x)
    finally:
        lib.pre3_destroy(ctx)


def test_the_limits(pre3):
    out = np.zeros(2, np.int32)
    _lib.check(_lib.lib.pre3_reloc_limits(_lib.dptr(out)))
    assert out[0] >= 2000 and out[1] == 700
