"""The numpy restatement of the ICP's closed-form covariance and of the rule by which the prediction takes u and Pn from a refined pair (DESIGN.md
section 34).  Nothing here is taken from 3pre_amd/csrc/pre3_icpcov.h or pre3_predicticp.h: the pairs are gathered and handed to tests/vo_cov_ref.py's
sums / cov (the implicit-function covariance of a rigid fit, itself checked against finite differences in tests/test_vo_cov_ref.py).

    f_p = data1(:, corr(k, 1)), f_n = data2(:, corr(k, 2)) -- the ORIGINAL source, before Rinit / Tinit --, r = T + R(q) f_n - f_p, X = u = [T; q]
    status 0: fewer than four pairs; 2: a non-finite coordinate in a pair, a Cholesky pivot at or below 7 eps times its diagonal, a non-finite result
"""
import functools

import numpy as np

import icp_ref
import vo_cov_ref

NOISE_CONTEXT, NOISE_PAIR, NOISE_ICP, NOISE_ICP_FLOOR = 0, 1, 2, 3
U_IDENTITY, U_PAIR, U_ICP = 0, 1, 2


def gather(data1, data2, corr):
    """(P1, P2), each (3, p), from 1-based (model, source) rows"""
    c = np.asarray(corr)[:, :2].astype(np.int64) - 1
    return np.asarray(data1, float)[:, c[:, 0]], np.asarray(data2, float)[:, c[:, 1]]


def sums(data1, data2, corr, u, order=None, m=vo_cov_ref.Math()):
    P1, P2 = gather(data1, data2, corr)
    return vo_cov_ref.sums(P1, P2, None, u, order, m)


def cov(data1, data2, corr, u, order=None, solver="chol", m=vo_cov_ref.Math()):
    """(cov (7, 7) or None, status, n) -- pre3_icp_cov's contract"""
    if len(corr) < 4:
        return None, 0, 0
    P1, P2 = gather(data1, data2, corr)
    return vo_cov_ref.cov(P1, P2, None, u, order, solver, m)


# ---- which u and which Pn the prediction takes (pre3_predict_icp_pair_seeded's rule)
def select(sta, pnum, bad, dist_ok, icp_sta, icp_u_finite, icp_error, max_error, noise, cov_pair_status, cov_icp_status):
    """(u_taken, noise_taken, refusal): refusal 0 none, 1 a bad match, 2 no matched point beyond 0.4 m -- as pre3_predict_pair_seeded's"""
    refusal = 0
    if pnum >= 4:
        refusal = 1 if bad != 0 else (2 if dist_ok == 0 else 0)
    pair = vo_cov_ref.pair_takes_u(sta, pnum, bad, dist_ok)
    u_taken = U_PAIR if pair else U_IDENTITY
    if pair and icp_sta == 1 and icp_u_finite and icp_error <= max_error:      # (a NaN error compares false)
        u_taken = U_ICP
    noise_taken = NOISE_CONTEXT
    if noise in (NOISE_ICP, NOISE_ICP_FLOOR) and u_taken == U_ICP and cov_icp_status == 1:
        noise_taken = noise
    elif noise != NOISE_CONTEXT and vo_cov_ref.predict_takes(sta, pnum, bad, dist_ok, cov_pair_status):
        noise_taken = NOISE_PAIR
    return u_taken, noise_taken, refusal


def taken_pn(noise_taken, pn_context, cov_pair, cov_icp):
    """the Pn the prediction uses: mode 3 is one fp64 addition per entry"""
    if noise_taken == NOISE_PAIR:
        return cov_pair
    if noise_taken == NOISE_ICP:
        return cov_icp
    if noise_taken == NOISE_ICP_FLOOR:
        return np.asarray(cov_icp, float) + np.asarray(pn_context, float)
    return pn_context


# ---- the committed cases (tests/golden/icp_cov_tolerance.json is measured on exactly these)
SHAPES = icp_ref.FIXED_SHAPES[1:]                   # (257, 64), (1000, 777), (4097, 1500)
SEED = 1
TRUNCATIONS = (4, 255, 256, 257, 513)               # of the largest scene's list; 256 x limits[1] + 1 is added by the tests from pre3_icp_cov_limits


@functools.lru_cache(maxsize=None)
def scene(n1, n2, seed=SEED):
    """(scene, the restatement's ICP run on it): shared by every test of a session and left unchanged"""
    s = icp_ref.surface_scene(n1, n2, seed)
    return s, icp_ref.icp_with_init(s["data1"], s["data2"], s["res"], s["Rinit"], s["Tinit"])


def case_name(n1, n2, p):
    return "surface_%dx%d_seed%d_p%d" % (n1, n2, SEED, p)


def committed_cases(extra_truncations=()):
    """[(name, data1, data2, corr (p, 2) int, u)]: every shape's full list, then the truncations of the largest scene's"""
    out = []
    for n1, n2 in SHAPES:
        s, r = scene(n1, n2)
        c = r["corr"][:, :2].astype(np.int64)
        out.append((case_name(n1, n2, len(c)), s["data1"], s["data2"], c, r["u"]))
    n1, n2 = SHAPES[-1]
    s, r = scene(n1, n2)
    c = r["corr"][:, :2].astype(np.int64)
    for p in tuple(TRUNCATIONS) + tuple(extra_truncations):
        if p < len(c):
            out.append((case_name(n1, n2, p), s["data1"], s["data2"], c[:p], r["u"]))
    return out
