"""numpy restatement of the camera-only motion models of predict_state_and_covariance.m -- the ones the fork left in place and switched off -- written
from the formulas, independent of the device code (3pre_amd/csrc/pre3_predictcv.h).  TEST INFRASTRUCTURE ONLY.

Citations: paths relative to the reference's matlab_code/.
  state functions   fv.m:64-87 and the commented original :98-106
  F                 predict_state_and_covariance.m:82, dfv_by_dxv.m:38-116
  Q = G Pn G'       predict_state_and_covariance.m:127, func_Q.m:41-54; Pn: :89-90, :103-104
  assembly          predict_state_and_covariance.m:129-143

One deviation, shared with the device code: at |omega| = 0 exactly dqomegadt_by_domega is 0/0 in the reference (it relies on the prior w_0 = 1e-15,
initialize_x_and_p.m:29-32); here the limit is taken -- row 1 zero, dt/2 on the diagonal of rows 2:4.
"""
import importlib

import numpy as np

twin = importlib.import_module("oracle.np_twin")

TYPES = ("constant_velocity", "constant_orientation", "constant_position", "constant_position_and_orientation")
CV, CO, CP, CPO = range(4)
EPS = np.finfo(float).eps
TINY = np.finfo(float).tiny


def v2q(v):                               # v2q.m:35-41, quaternion.m:37
    theta = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    if theta < EPS:
        return np.array([1.0, 0.0, 0.0, 0.0])
    s = np.sin(theta / 2)
    return np.array([np.cos(theta / 2), s * v[0] / theta, s * v[1] / theta, s * v[2] / theta])


def qprod(q, p):                          # qprod.m:28-33
    a, v = q[0], np.asarray(q[1:4], float)
    x, u = p[0], np.asarray(p[1:4], float)
    return np.concatenate([[a * x - v @ u], a * u + x * v + np.cross(v, u)])


def dq3_by_dq1(q):                        # dq3_by_dq1.m:34-37: d(q (x) p) / dp
    r, x, y, z = q
    return np.array([[r, -x, -y, -z], [x, r, -z, y], [y, z, r, -x], [z, -y, x, r]])


def dq3_by_dq2(p):                        # dq3_by_dq2.m:34-38: d(q (x) p) / dq
    r, x, y, z = p
    return np.array([[r, -x, -y, -z], [x, r, z, -y], [y, -z, r, x], [z, y, -x, r]])


def dqomegadt_by_domega(om, dt, limit_at_zero=True):     # dfv_by_dxv.m:70-116
    om = np.asarray(om, float)
    w2 = om @ om
    if limit_at_zero and w2 < TINY:
        D = np.zeros((4, 3))
        D[1:, :] = np.eye(3) * dt / 2.0
        return D
    w = np.sqrt(w2)
    s, c = np.sin(w * dt / 2.0), np.cos(w * dt / 2.0)
    D = np.zeros((4, 3))
    for a in range(3):
        D[0, a] = (-dt / 2.0) * (om[a] / w) * s
        for b in range(3):
            if a == b:
                D[1 + a, b] = (dt / 2.0) * om[a] * om[a] / (w * w) * c + (1.0 / w) * (1.0 - om[a] * om[a] / (w * w)) * s
            else:
                D[1 + a, b] = (om[a] * om[b] / (w * w)) * ((dt / 2.0) * c - (1.0 / w) * s)
    return D


def fv(xv, dt, type):
    """x[0:13] -> the predicted 13 entries, quaternion not normalised"""
    r, q, v, om = xv[0:3], xv[3:7], xv[7:10], xv[10:13]
    if type == CV:
        return np.concatenate([r + v * dt, qprod(q, v2q(om * dt)), v, om])
    if type == CO:
        return np.concatenate([r + v * dt, q, v, np.zeros(3)])
    if type == CP:
        return np.concatenate([r, qprod(q, v2q(om * dt)), np.zeros(3), om])
    if type == CPO:
        return np.concatenate([r, q, np.zeros(3), np.zeros(3)])
    raise ValueError("type %r" % (type,))


def dfv_by_dxv(xv, dt, type, limit_at_zero=True):        # dfv_by_dxv.m:41-66
    q, om = xv[3:7], xv[10:13]
    F = np.eye(13)
    F[3:7, 3:7] = dq3_by_dq2(v2q(om * dt))
    if type == CV:
        F[0:3, 7:10] = np.eye(3) * dt
        F[3:7, 10:13] = dq3_by_dq1(q) @ dqomegadt_by_domega(om, dt, limit_at_zero)
    if type in (CO, CPO):
        F[3:7, 10:13] = 0
        F[10:13, 10:13] = 0
    if type in (CP, CPO):
        F[0:3, 7:10] = 0
        F[7:10, 7:10] = 0
    return F


def func_G(xv, dt, limit_at_zero=True):                  # func_Q.m:45-50
    G = np.zeros((13, 6))
    G[7:10, 0:3] = np.eye(3)
    G[10:13, 3:6] = np.eye(3)
    G[0:3, 0:3] = np.eye(3) * dt
    G[3:7, 3:6] = dq3_by_dq1(xv[3:7]) @ dqomegadt_by_domega(xv[10:13], dt, limit_at_zero)
    return G


def func_Q(xv, dt, sigma_a, sigma_alpha):                # func_Q.m:54 with the Pn of predict_state_and_covariance.m:89-90,103-104
    Pn = np.diag([(sigma_a * dt) ** 2] * 3 + [(sigma_alpha * dt) ** 2] * 3)
    G = func_G(xv, dt)
    return G @ Pn @ G.T


def predict(X_k, P_k, dt, sigma_a, sigma_alpha, type=CV):
    """(x_k_k, p_k_k) -> (x_k_km1, p_k_km1), predict_state_and_covariance.m:40,79,82,127-143"""
    n = X_k.shape[0]
    X = np.concatenate([fv(X_k[0:13], dt, type), X_k[13:]])
    F = dfv_by_dxv(X_k[0:13], dt, type)
    Q = func_Q(X_k[0:13], dt, sigma_a, sigma_alpha)
    P = np.block([[F @ P_k[0:13, 0:13] @ F.T + Q, F @ P_k[0:13, 13:n]], [P_k[13:n, 0:13] @ F.T, P_k[13:n, 13:n]]])
    P = twin.jnorm_rebuild(P, twin.normJac(X[3:7]))
    X[3:7] = X[3:7] / np.linalg.norm(X[3:7])
    return X, P


def step_cv(types, off, cam, x_kk, P_kk, dt, sigma_a, sigma_alpha, meas_idx, z_meas, hyp, threshold, early_exit=True, chi2=5.9915, type=CV):
    """mono_slam.m:153-187 with the camera-only prediction in front: predict above, then the stages of np_twin.step, the twin's own functions"""
    N = len(types)
    meas_idx = np.asarray(meas_idx, np.int64)
    x1, P1 = predict(x_kk, P_kk, dt, sigma_a, sigma_alpha, type)
    h, has_h = twin.project(types, off, x1, cam)
    Hc, Hl = twin.jacobian(types, off, x1, cam, h, has_h)
    S = twin.innovation(types, off, P1, Hc, Hl, has_h)
    z = np.zeros((N, 2))
    z[meas_idx] = z_meas
    ic = np.zeros(N, np.int32)
    ic[meas_idx] = 1
    li = np.zeros(N, np.int32)
    out = dict(x_km1=x1, P_km1=P1, S=S, h=h, has_h=has_h)
    if len(meas_idx) >= hyp.shape[1] and len(meas_idx) > 0:
        r = twin.ransac(types, off, x1, P1, Hc, Hl, z, h, meas_idx, meas_idx, cam, hyp, threshold, early_exit)
        li[meas_idx] = r["li_mask"]
        out["ransac"] = r
    x2, P2 = twin.update_landmarks(types, off, np.nonzero(li)[0], x1, P1, Hc, Hl, z, h)
    h2, has2 = twin.project(types, off, x2, cam, h, has_h)
    Hc2, Hl2 = twin.jacobian(types, off, x2, cam, h2, has2)
    hi = twin.rescue(types, off, P2, Hc2, Hl2, h2, z, ic, li, chi2)
    x3, P3 = twin.update_landmarks(types, off, np.nonzero(hi)[0], x2, P2, Hc2, Hl2, z, h2)
    # the rescue gate's chi2 values, for the tests that must know how far a decision is from the gate
    d2 = []
    for i in range(N):
        if ic[i] == 1 and li[i] == 0:
            c = twin._sparse_cols(types, off, [i])
            Hi = twin._rows(P2.shape[0], types, off, [i], Hc2, Hl2)[:, c]
            nui = z[i] - h2[i]
            try:
                d2.append(float(nui @ np.linalg.inv(Hi @ P2[np.ix_(c, c)] @ Hi.T) @ nui))
            except np.linalg.LinAlgError:                        # a measured landmark the projection skipped (np_twin.rescue: not an inlier)
                d2.append(np.inf)
    out.update(x_kk=x3, P_kk=P3, li=li[meas_idx], hi=hi[meas_idx], gate_d2=np.array(d2))
    return out
