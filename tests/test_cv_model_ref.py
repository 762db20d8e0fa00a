"""CPU: the numpy restatement of the camera-only motion models (tests/cv_model_ref.py) checked against itself -- its F against central differences of
its state functions, the omega = 0 limit against the reference's w_0 = 1e-15, the predicted P's symmetry and definiteness, type 0 against the fork's
odometry model (fv.m:52-53 is that identity), and the step_cv helper against np_twin.step."""
import importlib

import numpy as np
import pytest

import cv_model_ref as cvm
from test_oracle import _mixed_problem

twin = importlib.import_module("oracle.np_twin")
synth = importlib.import_module("3pre_amd.synth")

DT = 0.1                                                              # predict_state_and_covariance.m:35


def _xv(seed=0, omega=(0.31, -0.22, 0.41)):
    rng = np.random.default_rng(seed)
    q = np.array([0.93, 0.21, -0.17, 0.24])
    return np.concatenate([rng.normal(0, 1.0, 3), q / np.linalg.norm(q), [0.4, -0.3, 0.25], omega])


def _central(xv, type, h=1e-6):
    J = np.zeros((13, 13))
    for k in range(13):
        e = np.zeros(13)
        e[k] = h
        J[:, k] = (cvm.fv(xv + e, DT, type) - cvm.fv(xv - e, DT, type)) / (2 * h)
    return J


# Where the reference's F is NOT the Jacobian of its own state function (dfv_by_dxv.m:43-66 against fv.m:64-87): F(4:7,4:7) = dq3_by_dq2(v2q(omega dt)) is
# set for every type from the omega that comes in, also where the state function keeps q; type 1 keeps r + v dt but gets no dt I; type 2 turns q by
# omega but gets no F(4:7,11:13).  These blocks are the reference's and must be exactly what dfv_by_dxv.m leaves there; everything else is a derivative.
_NOT_A_DERIVATIVE = {
    cvm.CV: [],
    cvm.CO: [(slice(0, 3), slice(7, 10)), (slice(3, 7), slice(3, 7))],
    cvm.CP: [(slice(3, 7), slice(10, 13))],
    cvm.CPO: [(slice(3, 7), slice(3, 7))],
}


@pytest.mark.parametrize("type", range(4), ids=cvm.TYPES)
def test_F_against_central_differences(type):
    """step 1e-6: truncation h^2 f'''/6 ~ 1e-12 * (dt^3 ~ 1e-3), rounding eps |f| / h ~ 2.2e-16 * 3 / 1e-6 = 7e-10 at worst; the bound is 2e-9"""
    xv = _xv()
    F = cvm.dfv_by_dxv(xv, DT, type)
    J = _central(xv, type)
    mask = np.ones((13, 13), bool)
    for blk in _NOT_A_DERIVATIVE[type]:
        mask[blk] = False
    err = np.abs(F - J)[mask].max()
    print("type %d: |F - central differences| = %.3g" % (type, err))
    assert err < 2e-9
    qw = cvm.dq3_by_dq2(cvm.v2q(xv[10:13] * DT))
    want = {(0, 7): np.zeros((3, 3)), (3, 3): qw, (3, 10): np.zeros((4, 3))}
    for blk in _NOT_A_DERIVATIVE[type]:
        assert np.array_equal(F[blk], want[(blk[0].start, blk[1].start)])
    if type == cvm.CV:
        assert not _NOT_A_DERIVATIVE[type] and mask.all()


def test_omega_zero_limit_against_the_reference_prior():
    """The limit form at omega = 0 against the reference's formulas at its prior w_0 = 1e-15 [1 1 1] (initialize_x_and_p.m:29-32), entry by entry.  At that
    omega row 1 is -(dt/2)(w_a/|w|) sin(|w| dt/2) = -dt^2/4 w_a = -2.5e-18 where the limit has 0; the other entries are dt/2 = 0.05 and differ by the
    rounding of the reference's own evaluation there (a sum of two terms of size dt/6 and dt/3: a few ulp of 0.05, 6.9e-18 each).  Bound: dt^2/4 |w|_inf
    + 4 ulp(dt/2) = 2.5e-18 + 2.8e-17 -> 3.1e-17, on dqomegadt_by_domega itself and on F and G (dq3_by_dq1 of a unit q: rows of norm 1, factor 2)."""
    w0 = 1e-15 * np.ones(3)
    bound = DT * DT / 4 * 1e-15 + 4 * np.spacing(DT / 2)
    D0 = cvm.dqomegadt_by_domega(np.zeros(3), DT)
    Dw = cvm.dqomegadt_by_domega(w0, DT, limit_at_zero=False)
    assert np.isfinite(D0).all()
    assert np.array_equal(D0[0], np.zeros(3)) and np.array_equal(D0[1:], np.eye(3) * DT / 2)
    err = np.abs(D0 - Dw).max()
    print("|limit - reference at w_0|: %.3g (bound %.3g)" % (err, bound))
    assert err <= bound
    xv0, xvw = _xv(omega=(0, 0, 0)), _xv(omega=tuple(w0))
    for type in range(4):
        F0, Fw = cvm.dfv_by_dxv(xv0, DT, type), cvm.dfv_by_dxv(xvw, DT, type, limit_at_zero=False)
        assert np.isfinite(F0).all() and np.abs(F0 - Fw).max() <= 2 * bound
    G0, Gw = cvm.func_G(xv0, DT), cvm.func_G(xvw, DT, limit_at_zero=False)
    assert np.isfinite(G0).all() and np.abs(G0 - Gw).max() <= 2 * bound
    # without the limit the reference's formulas are 0/0 there: that is the deviation
    with np.errstate(all="ignore"):
        assert not np.isfinite(cvm.dqomegadt_by_domega(np.zeros(3), DT, limit_at_zero=False)).all()


@pytest.mark.parametrize("type", range(4), ids=cvm.TYPES)
@pytest.mark.parametrize("omega", [(0.31, -0.22, 0.41), (0.0, 0.0, 0.0)], ids=["turning", "omega0"])
def test_predicted_P_is_symmetric_and_not_indefinite(type, omega):
    """symmetric to the rounding of F P F' (two 13-term sums of entries bounded by max|P|: 26 * 1.1e-16 -> 1e-14 max|P|); lowest eigenvalue not below
    -1e-12 max|P|; landmarks and their block untouched; q normalised"""
    types, x, P, cam = _mixed_problem(seed=5, N=12)
    x = x.copy()
    x[0:13] = _xv(1, omega)
    xo, Po = cvm.predict(x, P, DT, 0.007, 0.007, type)
    assert np.isfinite(xo).all() and np.isfinite(Po).all()
    scale = np.abs(Po).max()
    assert np.abs(Po - Po.T).max() <= 1e-14 * scale
    assert np.linalg.eigvalsh(0.5 * (Po + Po.T)).min() >= -1e-12 * scale
    assert np.array_equal(xo[13:], x[13:]) and np.array_equal(Po[13:, 13:], P[13:, 13:])
    assert abs(np.linalg.norm(xo[3:7]) - 1) < 1e-15
    # the noise adds what func_Q says it adds
    _, P0 = cvm.predict(x, P, DT, 0.0, 0.0, type)
    Jn = np.eye(13)
    Jn[3:7, 3:7] = twin.normJac(cvm.fv(x[0:13], DT, type)[3:7])
    assert np.abs((Po - P0)[0:13, 0:13] - Jn @ cvm.func_Q(x[0:13], DT, 0.007, 0.007) @ Jn.T).max() <= 1e-14 * scale
    assert np.array_equal(Po[13:, :13], P0[13:, :13])


def test_type0_against_the_forks_odometry_model(orc):
    """fv.m:52-53: vW = q2R(q) dX / dt, wW = q2v(dq) / dt.  With those in the state, type 0's pose is the fork's r + q2R(q) dX, q (x) dq.  The rotation
    vector goes through atan2 / sin / cos and back: some twenty roundings of values below 4 (4.4e-16 each) -> 1e-14."""
    types, x, P, cam = _mixed_problem(seed=6, N=9)
    dX = np.array([0.012, -0.02, 0.031])
    dq = np.array([0.9996, 0.011, -0.017, 0.02])
    dq /= np.linalg.norm(dq)
    nv = np.linalg.norm(dq[1:])
    rotvec = 2 * np.arctan2(nv, dq[0]) * dq[1:] / nv
    x = x.copy()
    q = np.array([0.93, 0.21, -0.17, 0.24])
    x[3:7] = q / np.linalg.norm(q)
    x[7:10] = twin.q2R(x[3:7]) @ dX / DT
    x[10:13] = rotvec / DT
    xr, _ = orc.predict(x, P, np.concatenate([dX, dq]))
    xc, _ = cvm.predict(x, P, DT, 0.007, 0.007, cvm.CV)
    err = np.abs(xc[0:7] - xr[0:7]).max()
    print("pose against the odometry model: %.3g" % err)
    assert err < 1e-14
    assert np.array_equal(xc[7:13], x[7:13]) and np.array_equal(xr[7:13], np.zeros(6))


def test_step_cv_is_the_twins_step_behind_another_prediction():
    """step_cv = cv_model_ref.predict + the stages of np_twin.step (:349-367), the twin's own functions.  Type 3 without noise from a state whose v and
    omega are zero: the prediction is then known by hand (x unchanged, rows / columns 7..12 of P zeroed), and the stages rerun from it one by one must
    give step_cv's flags, x and P exactly."""
    N = 20
    seq = synth.make_sequence(N, 1, 8, seed=31)
    types = np.zeros(N, np.int32)
    off = 13 + 6 * np.arange(N)
    s = seq["steps"][0]
    x, P = seq["x0"].copy(), seq["P0"]
    a = cvm.step_cv(types, off, seq["cam"], x, P, DT, 0.0, 0.0, s["meas_idx"], s["z"], s["hyp"], 1.0, early_exit=False, type=cvm.CPO)
    # what step_cv predicted, by hand: x unchanged (v, omega zeroed: they are zero), P with rows / cols 7..12 zeroed
    F = np.eye(n := x.shape[0])
    F[7:13, 7:13] = 0
    P1 = twin.jnorm_rebuild(F @ P @ F.T, twin.normJac(x[3:7]))
    assert np.array_equal(a["x_km1"], x) and np.abs(a["P_km1"] - P1).max() <= 1e-15 * np.abs(P1).max()
    # the stages behind it are np_twin.step's: rerun them from step_cv's own prediction
    h, has_h = twin.project(types, off, a["x_km1"], seq["cam"])
    Hc, Hl = twin.jacobian(types, off, a["x_km1"], seq["cam"], h, has_h)
    z = np.zeros((N, 2))
    z[s["meas_idx"]] = s["z"]
    r = twin.ransac(types, off, a["x_km1"], a["P_km1"], Hc, Hl, z, h, s["meas_idx"], s["meas_idx"], seq["cam"], s["hyp"], 1.0, False)
    assert np.array_equal(r["support"], a["ransac"]["support"]) and np.array_equal(r["li_mask"], a["li"])
    li = np.zeros(N, np.int32)
    li[s["meas_idx"]] = r["li_mask"]
    x2, P2 = twin.update_landmarks(types, off, np.nonzero(li)[0], a["x_km1"], a["P_km1"], Hc, Hl, z, h)
    h2, has2 = twin.project(types, off, x2, seq["cam"], h, has_h)
    Hc2, Hl2 = twin.jacobian(types, off, x2, seq["cam"], h2, has2)
    ic = np.zeros(N, np.int32)
    ic[s["meas_idx"]] = 1
    hi = twin.rescue(types, off, P2, Hc2, Hl2, h2, z, ic, li)
    x3, P3 = twin.update_landmarks(types, off, np.nonzero(hi)[0], x2, P2, Hc2, Hl2, z, h2)
    assert a["li"].sum() >= 3 and n == 13 + 6 * N
    assert np.array_equal(a["hi"], hi[s["meas_idx"]]) and np.array_equal(a["x_kk"], x3) and np.array_equal(a["P_kk"], P3)
    assert len(a["gate_d2"]) == int((1 - a["li"]).sum())
    assert np.array_equal((a["gate_d2"] < 5.9915).astype(np.int32), a["hi"][a["li"] == 0])


# ---- the device code's model header, compiled for the host, against the restatement
HOST_PROGRAM = r"""
#include <cstdio>
#include "pre3_predictcv.h"
using namespace pre3;
// stdin: records of 13 doubles x | dt | type (as a double);  stdout: per record xo (13) | F (169) | G (78) | whether a row of P changes (13)
int main()
{
    double in[15];
    while (fread(in, 8, 15, stdin) == 15) {
        const int type = (int)in[14];
        CvModel m; double F[169], G[78], changed[13];
        cv_model(in, type, in[13], m);
        for (int i = 0; i < 13; ++i) {
            for (int k = 0; k < 13; ++k) F[i * 13 + k] = cv_F_entry(i, k, type, in[13], m.Rq, m.M);
            for (int c = 0; c < 6; ++c) G[i * 6 + c] = cv_G_entry(i, c, in[13], m.M);
            changed[i] = cv_row_changes(i, type);
        }
        if (fwrite(m.xo, 8, 13, stdout) != 13 || fwrite(F, 8, 169, stdout) != 169 || fwrite(G, 8, 78, stdout) != 78 || fwrite(changed, 8, 13, stdout) != 13) return 3;
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def model_exe(tmp_path_factory):
    import os
    import shutil
    import subprocess
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = tmp_path_factory.mktemp("predictcv_host")
    src, exe = d / "predictcv_host.cpp", d / "predictcv_host"
    src.write_text(HOST_PROGRAM)
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(root, "3pre_amd", "csrc"), str(src), "-o", str(exe)])
    return str(exe)


@pytest.mark.parametrize("omega", [(0.31, -0.22, 0.41), (0.0, 0.0, 0.0), (1e-15, 1e-15, 1e-15), (3.0, -2.0, 4.0)], ids=["turning", "omega0", "w0", "fast"])
def test_the_model_header_against_the_restatement(model_exe, omega):
    """3pre_amd/csrc/pre3_predictcv.h (what lane 0 of every block of k_predict_cv evaluates) on the host: x, F and the G block of every type against
    the restatement, and the rows of P it says change.  Both sides are a few dozen double operations on values below 4 in another order (the header
    takes omega / |omega| once): 1e-15 (4 ulp of 1, 1 ulp of 4)."""
    import subprocess
    xv = _xv(2, omega)
    inp = b"".join(np.concatenate([xv, [DT, t]]).tobytes() for t in range(4))
    out = np.frombuffer(subprocess.run([model_exe], input=inp, stdout=subprocess.PIPE, check=True).stdout, np.float64).reshape(4, 273)
    for t in range(4):
        xo, F, G, changed = out[t, :13], out[t, 13:182].reshape(13, 13), out[t, 182:260].reshape(13, 6), out[t, 260:]
        Fr = cvm.dfv_by_dxv(xv, DT, t)
        assert np.isfinite(out[t]).all()
        assert np.abs(xo - cvm.fv(xv, DT, t)).max() < 1e-15
        assert np.abs(F - Fr).max() < 1e-15
        assert np.abs(G - cvm.func_G(xv, DT)).max() < 1e-15
        assert np.array_equal(F == 0, Fr == 0) and np.array_equal(G == 0, cvm.func_G(xv, DT) == 0)          # the same blocks are zero
        # the rows the launch stores: those whose row of F is not the identity's, and rows 3..6 (Jnorm)
        want = np.any(Fr != np.eye(13), axis=1)
        want[3:7] = True
        assert np.array_equal(changed.astype(bool), want)


def test_the_symbol_is_declared_exported_and_mirrored(pre3):
    import ctypes as C
    import inspect
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "pre3.h")).read()
    assert "pre3_predict_cv" in set(re.findall(r"PRE3_API\s+[\w\s\*]+?\b(pre3_\w+)\s*\(", txt))
    assert hasattr(C.CDLL(pre3.LIB_PATH), "pre3_predict_cv")
    assert "pre3_predict_cv" in pre3._lib.EXPORTS and len(pre3._lib.lib.pre3_predict_cv.argtypes) == 5
    sig = inspect.signature(pre3.EkfFilter.ekf_prediction_cv).parameters
    assert list(sig) == ["self", "dt", "sigma_a", "sigma_alpha", "type"] and sig["type"].default == "constant_velocity"
    assert pre3.EkfFilter.CV_TYPES == cvm.TYPES
    assert "\"predict_cv\"" in open(os.path.join(root, "mex", "ekf_ctx_gateway.c")).read()
    # the argument errors return before a device is touched
    for args in ((None, 0, DT, 0.007, 0.007),):
        assert pre3._lib.lib.pre3_predict_cv(*args) == -1
