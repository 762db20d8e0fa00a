"""CPU: numpy truth of @ekf_filter/ekf_heading_update.m:27-52 (pre3_heading_update) and its checks.

heading_rows(q)              aux_code/observe_heading_func.m:19-23, observe_heading_jac.m:31-38
heading_RR(R_plane)          ekf_heading_update.m:37-40 over slamToolbox_11_02_18/FrameTransforms/Rotations/R2q.m:11-55, q2e.m:15-38, e2q.m:14-35
heading_gate(z, h, strict)   ekf_heading_update.m:41-44 over aux_code/find_angle_bw_2_vecs.m:3-12 (True = the update is skipped; quirk Q12)
heading_update(x, P, R_plane, strict) the whole call, composed with oracle/np_twin.update
"""
import numpy as np
import pytest

from oracle import np_twin as tw


def R2q(R):                                    # R2q.m:11-55
    T = np.trace(R) + 1.0
    if T > 0.00000001:
        S = 2 * np.sqrt(T)
        a, b, c, d = 0.25 * S, (R[1, 2] - R[2, 1]) / S, (R[2, 0] - R[0, 2]) / S, (R[0, 1] - R[1, 0]) / S
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        S = 2 * np.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2])
        a, b, c, d = (R[1, 2] - R[2, 1]) / S, 0.25 * S, (R[0, 1] + R[1, 0]) / S, (R[2, 0] + R[0, 2]) / S
    elif R[1, 1] > R[2, 2]:
        S = 2 * np.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2])
        a, b, c, d = (R[2, 0] - R[0, 2]) / S, (R[0, 1] + R[1, 0]) / S, 0.25 * S, (R[1, 2] + R[2, 1]) / S
    else:
        S = 2 * np.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1])
        a, b, c, d = (R[0, 1] - R[1, 0]) / S, (R[2, 0] + R[0, 2]) / S, (R[1, 2] + R[2, 1]) / S, 0.25 * S
    return np.array([a, -b, -c, -d])


def q2e(q):                                    # q2e.m:15-38
    a, b, c, d = q
    y1, x1 = 2 * c * d + 2 * a * b, a * a - b * b - c * c + d * d
    z2 = -2 * b * d + 2 * a * c
    y3, x3 = 2 * b * c + 2 * a * d, a * a + b * b - c * c - d * d
    return np.array([np.arctan2(y1, x1), np.arcsin(z2), np.arctan2(y3, x3)])


def e2q(e):                                    # e2q.m:14-18 (au2q: [cos(a/2); sin(a/2) * axis])
    def au2q(a, u):
        return np.concatenate([[np.cos(a / 2)], np.sin(a / 2) * np.asarray(u, float)])
    qx, qy, qz = au2q(e[0], [1, 0, 0]), au2q(e[1], [0, 1, 0]), au2q(e[2], [0, 0, 1])
    return tw.qProd(tw.qProd(qz, qy)[0], qx)[0], tw.e2q_jac(e)


def heading_rows(q):
    q1, q2, q3, q4 = q
    h = np.array([q1 * q4 * -2.0 + q2 * q3 * 2.0, q1 ** 2 - q2 ** 2 + q3 ** 2 - q4 ** 2, q1 * q2 * 2.0 + q3 * q4 * 2.0])
    H = np.array([[-2 * q4, 2 * q3, 2 * q2, -2 * q1], [2 * q1, -2 * q2, 2 * q3, -2 * q4], [2 * q2, 2 * q1, 2 * q4, 2 * q3]])
    return h, H


def heading_RR(R_plane):
    q = R2q(R_plane)
    _, Je = e2q(q2e(q))
    Jz = heading_rows(q)[1]
    A = Jz @ Je
    return A @ np.diag((np.pi * np.ones(3) / 180) ** 2) @ A.T


def _acosd(c):
    return np.degrees(np.arccos(np.clip(c, -1.0, 1.0)))


def heading_angles(z, h):                      # find_angle_bw_2_vecs.m:3-12
    mz, mh = np.linalg.norm(z), np.linalg.norm(h)
    return np.concatenate([_acosd(z / mz), _acosd(h / mh), [_acosd(np.dot(z, h) / mz / mh)]])


def heading_gate(z, h, strict):
    a = heading_angles(z, h)
    return bool(np.all(a > 4)) if strict else bool(a[6] > 4)


def heading_update(x, P, R_plane, strict=True):
    """(x, P, applied) after ekf_heading_update.m on (x_k_k, p_k_k)"""
    z = R_plane[:, 1].copy()
    h, Hq = heading_rows(x[3:7])
    if heading_gate(z, h, strict):
        return x.copy(), P.copy(), False
    H = np.zeros((3, x.shape[0]))
    H[:, 3:7] = Hq
    xo, Po, _ = tw.update(x, P, H, heading_RR(R_plane), z, h)
    return xo, Po, True


def axis_rot(axis, deg):
    """rotation by deg degrees about axis (Rodrigues)"""
    u = np.asarray(axis, float) / np.linalg.norm(axis)
    t = np.radians(deg)
    K = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def _rand_q(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def test_h_is_the_second_column_of_q2R():
    rng = np.random.default_rng(1)
    for _ in range(50):
        q = _rand_q(rng) * rng.uniform(0.5, 2.0)
        assert np.allclose(heading_rows(q)[0], tw.q2R(q)[:, 1], rtol=0, atol=1e-14 * np.dot(q, q))


def test_H_is_the_jacobian_of_h():
    rng = np.random.default_rng(2)
    for _ in range(20):
        q = rng.normal(size=4)
        Hn = np.zeros((3, 4))
        for k in range(4):
            e = np.zeros(4)
            e[k] = 1e-6
            Hn[:, k] = (heading_rows(q + e)[0] - heading_rows(q - e)[0]) / 2e-6
        assert np.abs(Hn - heading_rows(q)[1]).max() < 1e-8


def test_R2q_inverts_q2R():
    rng = np.random.default_rng(3)
    qs = [_rand_q(rng) for _ in range(200)]
    qs += [np.array([0.0, 1.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.0, 0.0]), np.array([0.0, 0.0, 0.0, 1.0]),
           np.array([1e-6, 0.6, 0.8, 0.0]) / np.linalg.norm([1e-6, 0.6, 0.8, 0.0])]      # every branch of R2q.m:13-52
    for q in qs:
        p = R2q(tw.q2R(q))
        assert min(np.abs(p - q).max(), np.abs(p + q).max()) < 1e-10, (q, p)


def test_q2e_e2q_round_trip_and_the_jacobian():
    rng = np.random.default_rng(4)
    for _ in range(100):
        e = np.array([rng.uniform(-3, 3), rng.uniform(-1.5, 1.5), rng.uniform(-3, 3)])
        q, J = e2q(e)
        assert abs(np.linalg.norm(q) - 1) < 1e-14
        assert np.abs(q2e(q) - e).max() < 1e-9
        Jn = np.zeros((4, 3))
        for k in range(3):
            d = np.zeros(3)
            d[k] = 1e-6
            Jn[:, k] = (e2q(e + d)[0] - e2q(e - d)[0]) / 2e-6
        assert np.abs(Jn - J).max() < 1e-8


def test_RR_is_a_symmetric_psd_observation_covariance_blind_along_z():
    rng = np.random.default_rng(5)
    for _ in range(20):
        Rp = tw.q2R(_rand_q(rng))
        RR = heading_RR(Rp)
        assert np.allclose(RR, RR.T, atol=1e-18)
        w = np.linalg.eigvalsh(RR)
        assert w.min() > -1e-15 and w.max() < 1e-2
        # z = R_plane(:, 2) is a unit vector: its perturbations are orthogonal to it
        assert abs(Rp[:, 1] @ RR @ Rp[:, 1]) < 1e-12 * w.max()


def test_gate_modes_on_hand_built_pairs():
    y = np.array([0.0, 1.0, 0.0])
    # z one degree from the y axis, h 6 degrees from z: the angle between them exceeds 4, but z's own angle to the y axis does not
    z = axis_rot([1, 0, 0], 1.0) @ y
    h = axis_rot([0, 0, 1], 6.0) @ z
    a = heading_angles(z, h)
    assert a[6] > 4 and a[1] < 4
    assert heading_gate(z, h, strict=True) is False        # the reference applies the update (quirk Q12)
    assert heading_gate(z, h, strict=False) is True         # the evident intent skips it
    # both far from every axis and 10 degrees apart: both modes skip
    z2 = np.array([1.0, 1.0, 1.0]) / np.sqrt(3)
    h2 = axis_rot([1, -1, 0], 10.0) @ z2
    assert heading_gate(z2, h2, True) and heading_gate(z2, h2, False)
    # 2 degrees apart: neither mode skips
    h3 = axis_rot([1, -1, 0], 2.0) @ z2
    assert not heading_gate(z2, h3, True) and not heading_gate(z2, h3, False)
    # a cosine just outside [-1, 1] from rounding is clamped
    assert heading_angles(y, y * (1 + 1e-16))[6] == 0.0


@pytest.mark.parametrize("deg", [1.5, 3.0])
def test_heading_update_pulls_the_orientation_towards_the_plane(deg):
    rng = np.random.default_rng(6)
    n = 13 + 6 * 4
    A = rng.normal(size=(n, n)) * 0.01
    P = A @ A.T + 1e-4 * np.eye(n)
    x = np.zeros(n)
    x[3:7] = _rand_q(rng)
    P = tw.jnorm_rebuild(P, tw.normJac(x[3:7]))
    Rp = tw.q2R(x[3:7]) @ axis_rot([1.0, 0.3, -0.2], deg)
    xo, Po, applied = heading_update(x, P, Rp, strict=False)
    assert applied
    assert abs(np.linalg.norm(xo[3:7]) - 1) < 1e-14
    before = heading_angles(Rp[:, 1], heading_rows(x[3:7])[0])[6]
    after = heading_angles(Rp[:, 1], heading_rows(xo[3:7])[0])[6]
    assert after < before
    assert np.array_equal(Po, Po.T) or np.abs(Po - Po.T).max() < 1e-18
