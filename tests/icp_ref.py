"""The numpy restatement of the dense ICP (TestScripts/icp_with_init.m:34-120), the scenes both suites share, and the margins that
say whether a scene's integer results can be compared at all.

Every sum of squares, every transform of a point and every comparison is written out elementwise, one rounding per operation, in the order the library
documents: d = (dx dx + dy dy) + dz dz, x' = ((r0 x + r1 y) + r2 z) + t.  The svd is numpy's, and the sums of reg() are taken in the order `sums` names
('forward': one after the other; 'reversed'; 'pairwise': numpy's tree) -- tests/golden/make_icp_tolerance.py measures what that choice moves.

The dedupe is the reference's three lines as they stand: -sortrows(-corr, 3), the stable sortrows(corr, 1), and the 2005 code's unique, which returned
the LAST occurrence.  Together: the smallest D per model index, on equal D the highest source index.

One departure (documented in include/pre3.h): an iteration that finds p < 3 pairs ends the run with status 2 and the transform accumulated so far.
"""
import numpy as np

MAX_ITER, NOCHANGE, ITER_CAP = 30, 10, 62
NOT_RUN, OK, FEW = 0, 1, 2


# ---- loop control: 3pre_amd/csrc/pre3_icp.h's icp_advance, restated ------------------------------------------------------------------------------------
class Ctl:
    def __init__(self, res):
        self.phase, self.n, self.c1, self.c2, self.no_change, self.done, self.status = 1, 0, 0, 1, 0, 0, NOT_RUN
        self.it1 = self.it2 = self.total = self.p = 0
        self.e1, self.e2, self.res, self.last_e = 1000001.0, 1000000.0, float(res), 0.0
        self.nochange_margin = np.inf

    def advance(self, p, sum_d):
        """returns True when the iteration's transform is applied"""
        if self.done:
            return False
        self.total += 1
        if self.phase == 1:
            self.it1 += 1
        else:
            self.it2 += 1
        self.p = int(p)
        if p < 3:
            self.done, self.status, self.last_e = 1, FEW, 0.0
            return False
        e = np.float64(sum_d) / (np.float64(p) * np.float64(self.res))                 # :90
        self.last_e = float(e)
        if self.phase == 1:
            self.c1 = self.c2                                                         # :48
            self.c2 = int(p)                                                          # :63
            self.n += 1
            if self.n > MAX_ITER or self.c2 == self.c1:                               # :65-67, :47
                self.phase, self.n, self.no_change, self.e1, self.e2 = 2, 0, 0, 1000001.0, 1000000.0
        else:
            self.e1 = self.e2                                                         # :75
            self.e2 = float(e)
            self.n += 1
            if self.n > MAX_ITER:                                                     # :93-95
                self.done, self.status = 1, OK
            else:
                gap, lim = abs(np.float64(self.e2) - np.float64(self.e1)), np.float64(self.res) / 10000
                self.nochange_margin = min(self.nochange_margin, float(abs(gap - lim)))
                if gap < lim:                                                         # :96-98
                    self.no_change += 1
                if self.no_change >= NOCHANGE:                                        # :74
                    self.done, self.status = 1, OK
        return True

    def state(self):
        return (self.phase, self.n, self.c1, self.c2, self.no_change, self.done, self.status, self.it1, self.it2, self.total, self.p, self.e1, self.e2,
                self.last_e)

    def error(self):
        return min(self.e1, self.e2)                                                  # :100


# ---- the pieces of one iteration -----------------------------------------------------------------------------------------------------------------------
def nearest(model, src, block=128):
    """dsearchn(model', src') without a triangulation: (d, idx, gap) per source point -- the smallest squared distance, the lowest model index that has it,
    and the distance from it to the second smallest (inf for a model of one point)"""
    n2 = src.shape[1]
    d, idx, gap = np.empty(n2), np.empty(n2, np.int64), np.full(n2, np.inf)
    mx, my, mz = model[0][None, :], model[1][None, :], model[2][None, :]
    for j0 in range(0, n2, block):
        s = src[:, j0:j0 + block]
        dx, dy, dz = s[0][:, None] - mx, s[1][:, None] - my, s[2][:, None] - mz
        dd = (dx * dx + dy * dy) + dz * dz
        k = np.argmin(dd, axis=1)                                                     # the first minimum: the lowest index
        d[j0:j0 + block], idx[j0:j0 + block] = dd[np.arange(len(k)), k], k
        if dd.shape[1] > 1:
            dd[np.arange(len(k)), k] = np.inf
            gap[j0:j0 + block] = dd.min(axis=1) - d[j0:j0 + block]
    return d, idx, gap


def dedupe(idx, D, res):
    """:50-56.  corr (p, 3) = [model, source, D] 1-based, ascending in the model index; the margins of the rejection and of the claims"""
    n2 = len(D)
    corr = np.stack([idx + 1.0, np.arange(1, n2 + 1.0), D], axis=1)
    reject_margin = float(np.abs(D - 2 * res).min()) if n2 else np.inf
    corr = corr[~(D > 2 * res)]                                                        # :51
    corr = -(-corr)[np.argsort((-corr)[:, 2], kind="stable")]                          # :53  -sortrows(-corr, 3)
    corr = corr[np.argsort(corr[:, 0], kind="stable")]                                 # :54  sortrows(corr, 1)
    claim_margin = np.inf
    if len(corr) > 1:
        same = corr[1:, 0] == corr[:-1, 0]
        last = np.append(corr[1:, 0] != corr[:-1, 0], True)                            # :55  unique, legacy: the last occurrence
        two_best = same & last[1:]                                                     # the kept row and the one before it share a model index
        if two_best.any():
            claim_margin = float((corr[:-1, 2] - corr[1:, 2])[two_best].min())
        corr = corr[last]
    return corr, reject_margin, claim_margin


def total(v, sums):
    v = np.asarray(v, dtype=np.float64)
    if v.size == 0:
        return np.float64(0.0)
    if sums == "forward":
        return np.cumsum(v)[-1]
    if sums == "reversed":
        return np.cumsum(v[::-1])[-1]
    return np.sum(v)


def apply(R, t, pts):
    """((r0 x + r1 y) + r2 z) + t, elementwise"""
    x, y, z = pts
    return np.stack([((R[i, 0] * x + R[i, 1] * y) + R[i, 2] * z) + t[i] for i in range(3)])


def reg(model, src, corr, sums):
    """:103-120"""
    n = len(corr)
    M, S = model[:, corr[:, 0].astype(int) - 1], src[:, corr[:, 1].astype(int) - 1]
    mm = np.array([total(M[i], sums) / n for i in range(3)])
    ms = np.array([total(S[i], sums) / n for i in range(3)])
    Ss, Ms = S - ms[:, None], M - mm[:, None]
    K = np.array([[total(Ss[i] * Ms[j], sums) for j in range(3)] for i in range(3)]) / n
    U, A, Vh = np.linalg.svd(K)
    V = Vh.T
    R1 = V @ U.T
    if np.linalg.det(R1) < 0:
        B = np.eye(3)
        B[2, 2] = np.linalg.det(V @ U.T)
        R1 = V @ B @ U.T
    t1 = mm - apply(R1, np.zeros(3), ms)
    return R1, t1


def R2q(R):
    """R2q.m with Calculate_V_Omega_RANSAC_dr_ye.m:48's sign"""
    Tq = R[0, 0] + R[1, 1] + R[2, 2] + 1
    if Tq > 0.00000001:
        S = 2 * np.sqrt(Tq)
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


# ---- the run -------------------------------------------------------------------------------------------------------------------------------------------
def icp_with_init(data1, data2, res, Rinit=None, Tinit=None, sums="forward"):
    """dict(R, t, Rtot, ttot, u, corr (p, 3), p, error, data2, sta, iters1, iters2, log (rows [phase, p, e]), ps (p of every iteration),
    margins = dict(reject, nn, claim, nochange))"""
    model = np.ascontiguousarray(data1, dtype=np.float64)
    Rinit = np.eye(3) if Rinit is None else np.asarray(Rinit, dtype=np.float64).reshape(3, 3)
    Tinit = np.zeros(3) if Tinit is None else np.asarray(Tinit, dtype=np.float64).reshape(3)
    src = apply(Rinit, Tinit, np.asarray(data2, dtype=np.float64))                     # :34-35
    R, t = np.eye(3), np.zeros(3)
    c = Ctl(res)
    log, corr = [], np.zeros((0, 3))
    mg = dict(reject=np.inf, nn=np.inf, claim=np.inf)
    while not c.done:
        phase = c.phase
        d, idx, gap = nearest(model, src)
        D = np.sqrt(d)
        corr, rj, cl = dedupe(idx, D, res)
        mg["reject"], mg["nn"], mg["claim"] = min(mg["reject"], rj), min(mg["nn"], float(gap.min())), min(mg["claim"], cl)
        p = len(corr)
        if c.advance(p, total(corr[:, 2], sums) if p >= 3 else 0.0):
            R1, t1 = reg(model, src, corr, sums)
            src = apply(R1, t1, src)                                                   # :59-60
            R, t = R1 @ R, apply(R1, t1, t)                                            # :61-62
        log.append([phase, p, c.last_e])
    mg["nochange"] = c.nochange_margin
    Rtot, ttot = R @ Rinit, apply(R, t, Tinit)
    return dict(R=R, t=t, Rtot=Rtot, ttot=ttot, u=np.concatenate([ttot, R2q(Rtot)]), corr=corr, p=len(corr), error=c.error(), data2=src, sta=c.status,
                iters1=c.it1, iters2=c.it2, log=np.array(log).reshape(-1, 3), ps=[int(r[1]) for r in log], margins=mg)


# ---- scenes --------------------------------------------------------------------------------------------------------------------------------------------
def rotvec(w):
    w = np.asarray(w, dtype=np.float64)
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def surface(rng, n, extent=1.0):
    """n points on a smooth, nowhere symmetric range surface about 2 m away"""
    x, y = rng.uniform(-extent, extent, n), rng.uniform(-0.8 * extent, 0.8 * extent, n)
    z = 2.0 + 0.25 * np.sin(2.1 * x + 0.3) * np.cos(1.7 * y) + 0.15 * x * y + 0.1 * np.cos(3.3 * x - 1.1 * y)
    return np.stack([x, y, z])


def surface_scene(n1, n2, seed):
    """two independent samplings of one surface: the source is the surface seen from a pose a little off, the initial pose 0.01 rad / 5 mm off the truth.
    dict(data1, data2, res, Rinit, Tinit, R_true, T_true): data1 ~ R_true data2 + T_true"""
    rng = np.random.default_rng(1000003 * n1 + 1009 * n2 + seed)
    model, other = surface(rng, n1), surface(rng, n2)
    R_true, T_true = rotvec(rng.normal(0, 0.05, 3)), rng.normal(0, 0.03, 3)
    data2 = R_true.T @ (other - T_true[:, None])
    res = 2.0 * np.sqrt(3.2 / n1)                                                      # about twice the mean spacing of the model
    Rinit = rotvec(0.01 * unit(rng)) @ R_true
    Tinit = T_true + 0.005 * unit(rng)
    return dict(data1=np.asfortranarray(model), data2=np.asfortranarray(data2), res=float(res), Rinit=Rinit, Tinit=Tinit, R_true=R_true, T_true=T_true)


def unit(rng):
    v = rng.normal(0, 1, 3)
    return v / np.linalg.norm(v)


def subset_scene(n1, k, seed, noise=0.001):
    """the source is every k-th model point moved by a known pose, with `noise` m of noise per coordinate"""
    rng = np.random.default_rng(7919 * n1 + 31 * k + seed)
    model = surface(rng, n1)
    R_true, T_true = rotvec(rng.normal(0, 0.05, 3)), rng.normal(0, 0.03, 3)
    pick = model[:, ::k]
    data2 = R_true.T @ (pick + rng.normal(0, noise, pick.shape) - T_true[:, None])
    res = 2.0 * np.sqrt(3.2 / n1)
    Rinit = rotvec(0.01 * unit(rng)) @ R_true
    Tinit = T_true + 0.005 * unit(rng)
    return dict(data1=np.asfortranarray(model), data2=np.asfortranarray(data2), res=float(res), Rinit=Rinit, Tinit=Tinit, R_true=R_true, T_true=T_true)


def pose_error(R, T, s):
    """(angle in rad between R and the truth, |T - truth|)"""
    dR = R @ s["R_true"].T
    return float(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1))), float(np.linalg.norm(T - s["T_true"]))


MARGIN = 1e-9


def margins_ok(r):
    return all(v >= MARGIN for v in r["margins"].values())


# the (n1, n2) shapes of tests/test_gpu_icp.py that do not depend on the library's limits, and the seeds each runs with
FIXED_SHAPES = ((3, 3), (257, 64), (1000, 777), (4097, 1500))
SEEDS = (1, 2, 3)


def limit_shapes(src_tile, chunk):
    """one model chunk - 1, + 0, + 1 and two chunks + 1 against one source tile - 1, + 0, + 1"""
    return tuple((n1, n2) for n1, n2 in ((chunk - 1, src_tile - 1), (chunk, src_tile), (chunk + 1, src_tile + 1), (2 * chunk + 1, src_tile - 1),
                                         (chunk - 1, src_tile + 1), (2 * chunk + 1, src_tile + 1)))
