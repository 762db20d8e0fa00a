"""The factorisation and solve alone (update.m:32-33: S = L L', L W = [B | nu]): plain-numpy restatements, the seeded inputs and the case lists
of tests/test_chol_ref.py (CPU), tests/test_gpu_chol_alone.py (device) and tests/golden/make_chol_tolerance.py (the gate).  Nothing here
touches the library.

    figures        E1 = |L L' - S|_ij / (u (|L||L|')_ij) over the lower triangle, E2 = |L W - [B | nu]|_ij / (u (|L||W|)_ij) over every entry,
                   each as max and RMS, from the JUDGED L and W themselves (backward errors: no cond(S) in them; the Cholesky factor is unique,
                   so the two together are complete).  Where a denominator is zero the numerator must be exactly zero.
    plain          right-looking Cholesky and forward substitution in the dtype, one column at a time, every entry rounded after every
                   product and every subtraction, correctly rounded sqrt and divide: what "f32 accuracy" means
    blocked        64-row panels; the diagonal block by `plain`, its explicit inverse M_J by substitution in the dtype, then L(i,J) = A(i,J) M_J',
                   A(i,k) -= L(i,J) L(k,J)', C_j -= L(j,J) W_J, W_J = M_J C_J with every product rounded ONCE
    emulate_cholp  the persistent form's arithmetic restated (fp32): the same panels, every product as three round-to-nearest-even bf16 planes
                   per operand (k9_ref.split3), six plane products per 16-wide k-step in mma6's order, f32 accumulation; A(i,k) updates
                   accumulate from zero and are subtracted once, a strip's right-hand side C_j is ONE accumulator from start to finish.
                   The tests' own tool and the carrier of the mutants; its diagonal blocks take `plain` (v_rcp / v_rsq are not restated).

Two input classes.  Accuracy: S = D (Q diag(lambda) Q') D with lambda log-spaced over kappa and D a random permutation of logspace(-1, 1, r),
B with columns spread over three decades and two zero columns, nu standard normal.  Exact: L0 unit lower triangular with +-1 subdiagonals inside
each 64 x 64 diagonal block (its inverse has entries in {-1, 0, 1}, every pivot is 1) and integers in -2 .. 2 elsewhere, W0 integers in
-255 .. 255, S = L0 L0', B = L0 W0: every form in either dtype must return L0 and W0 bit for bit.
"""
import functools

import numpy as np

import k9_ref as K9
from k9_ref import U32, U64, round_up, state_size, ld_of, rcap_of, split3, SIX  # noqa: F401

NB = 64
KAPPAS = (10, 1000)
LIMIT = 2 ** 24
DT = {"f32": np.float32, "f64": np.float64}


def u_of(dtype):
    return U32 if dtype == "f32" else U64


# ---- the library's sizes and form selection (pre3_create, launch_chol_solve, cholp_usable), restated
def ldw_of(cap):
    return ld_of(cap) + NB


def cholp_stride(nH, num_cus):
    if 8 * nH + 1 <= num_cus:
        return 8
    for st in (7, 5, 3, 1):
        if st * nH + 1 <= num_cus:
            return st
    return 0


def cholp_takes(nrb, cap, num_cus, predicted_prior=False):
    """does launch_chol_solve hand an fp32 bf16-form context's update of nrb panels to k_cholp (chol_persist on, at most two live contexts)?"""
    return (nrb >= 2 or predicted_prior) and 1 <= nrb <= 16 and nrb <= rcap_of(cap) // NB and cholp_stride(max(nrb - 2, 0), num_cus) >= 1


def early_panel(r):
    """k_chol_step's `early` instantiation: real rows of the last panel, if at least one of its 8-row sub-panels is padding"""
    last = r - (round_up(r, NB) - NB)
    return last if last <= NB - 8 else 0


def trail_plan(nrb, cap, num_cus, split, p):
    """(panels followed by an own k_chol_trail_b3 launch, {paired panel: updates pending}, panels followed by a group sweep) of the per-panel form"""
    nW = ldw_of(cap) // NB

    def n_trail(J):
        nK = nrb - J - 1 if J >= 1 else 0
        return nK * (nK + 1) // 2 + nK * nW

    def own_at(J):
        return split > 0 and n_trail(J) > split * 2 * num_cus
    p = min(4, max(1, p))
    Jt = 0
    if p > 1 and own_at(1):
        Jt = p
        while Jt < nrb and own_at(Jt):
            Jt += p
    own, paired, sweeps = [], {}, []
    for J in range(nrb):
        if 1 <= J <= Jt:
            paired[J] = p if J % p == 0 else J % p
            if J % p == p - 1 and J + 2 <= nrb - 1:
                sweeps.append(J)
        elif own_at(J):
            own.append(J)
    return own, paired, sweeps


# ---- inputs
@functools.lru_cache(maxsize=None)
def accuracy_case(n, r, kappa, dtype):
    """(S, B, nu) holding values of `dtype` in float64 arrays; S symmetric positive definite"""
    t = DT[dtype]
    rng = np.random.default_rng([11, 2, n, r, kappa, 32 if dtype == "f32" else 64])
    Q, _ = np.linalg.qr(rng.standard_normal((r, r)))
    lam = np.logspace(0.0, np.log10(kappa), r)
    D = rng.permutation(np.logspace(-1, 1, r))
    F = np.rint(Q * np.sqrt(lam) * 2.0 ** 14) / 2.0 ** 14          # Q diag(lambda) Q' = F F' with F on a 2^-14 grid below 2^5: the sum is exact in fp64 in
    S = F @ F.T                                                    # any order, so the input does not depend on how a BLAS happens to block it
    S = D[:, None] * S * D[None, :]
    S = S.astype(t).astype(np.float64)
    S = np.tril(S) + np.tril(S, -1).T
    B = rng.standard_normal((r, n)) * np.logspace(-2, 1, n)[None, :]
    B[:, rng.choice(n, 2, replace=False)] = 0.0
    B = B.astype(t).astype(np.float64)
    nu = rng.standard_normal(r).astype(t).astype(np.float64)
    assert np.array_equal(S, S.T) and np.linalg.eigvalsh(S).min() > 0
    for a in (S, B, nu):
        a.setflags(write=False)
    return S, B, nu


@functools.lru_cache(maxsize=None)
def exact_case(n, r):
    """(S, B, nu, L0, W0): integers; W0 is r x (n + 1), its last column goes with nu"""
    rng = np.random.default_rng([11, 1, n, r])
    L0 = np.tril(rng.integers(-2, 3, (r, r)).astype(np.float64), -1)
    for j0 in range(0, r, NB):
        j1 = min(r, j0 + NB)
        blk = np.eye(j1 - j0)
        if j1 - j0 > 1:
            blk[np.arange(1, j1 - j0), np.arange(0, j1 - j0 - 1)] = rng.choice((-1.0, 1.0), j1 - j0 - 1)
        L0[j0:j1, j0:j1] = blk
    W0 = rng.integers(-255, 256, (r, n + 1)).astype(np.float64)
    W0[:, rng.choice(n, 2, replace=False)] = 0.0
    S = L0 @ L0.T
    Bn = L0 @ W0
    b = exact_bounds(L0, W0)
    assert b["sums"] < LIMIT and b["operands"] < 2 ** 16, b
    for a in (S, Bn, L0, W0):
        a.setflags(write=False)
    return S, Bn[:, :n], Bn[:, n], L0, W0


def block_inverse(L0):
    """block diagonal of the inverses of L0's 64 x 64 diagonal blocks"""
    M = np.zeros_like(L0)
    for j0 in range(0, len(L0), NB):
        j1 = min(len(L0), j0 + NB)
        M[j0:j1, j0:j1] = np.linalg.inv(L0[j0:j1, j0:j1])
    return M


def exact_bounds(L0, W0):
    """sums: an upper bound of every partial sum, in any order, of any form (right- or left-looking, through M_J or by substitution);
    operands: the largest magnitude any matrix-core product is handed (two bf16 planes hold an integer below 2^16: no third plane)"""
    a, w = np.abs(L0), np.abs(W0)
    M = block_inverse(L0)
    assert np.array_equal(M, np.rint(M)) and np.abs(M).max() <= 1
    lw, ll = a @ w, a @ a.T
    sums = max(ll.max(), lw.max(), (np.abs(M) @ lw).max(), (np.abs(M) @ ll).max())
    Ld = np.where(block_inverse(np.ones_like(L0) + len(L0) * np.eye(len(L0))) != 0, L0, 0.0)          # L0's diagonal blocks: C_J = L_JJ W_J is a strip's operand
    operands = max(np.abs(L0 @ L0.T).max(), np.abs(L0 @ W0).max(), a.max(), np.abs(M).max(), w.max(), np.abs(Ld @ W0).max())
    return dict(sums=float(sums), operands=float(operands))


# ---- wide products for the fp64 figures: slices of 20 bits (relative to the row's / column's largest entry) whose products sum exactly in
# fp64, the partial results added error-free.  What is left out lies below 2^-120 of rowmax x colmax per term: wide_matmul returns that bound too, and
# figures() refuses a reference that is not at least 2^6 finer than the unit it measures in.
WIDE_SLICES, WIDE_BITS = 7, 20


def _slices(A, axis):
    mx = np.abs(A).max(axis=axis, keepdims=True)
    e = np.ceil(np.log2(np.where(mx > 0, mx, 1.0)))
    rest, out = A.copy(), []
    for s in range(WIDE_SLICES):
        sigma = 0.75 * 2.0 ** (e + 53 - WIDE_BITS * (s + 1))
        hi = (rest + sigma) - sigma
        out.append(hi)
        rest = rest - hi
        if not rest.any():
            break
    return out, rest, mx


def wide_matmul(A, B):
    """A @ B as an unevaluated sum hi + lo of two doubles, and an entrywise bound of what hi + lo leaves out (inner dimension up to 2048)"""
    k = A.shape[1]
    assert k == B.shape[0] <= 2048
    hi, lo = np.zeros((A.shape[0], B.shape[1])), np.zeros((A.shape[0], B.shape[1]))
    (sa, ra, ma), (sb, rb, mb) = _slices(A, 1), _slices(B, 0)
    for i, a in enumerate(sa):
        for j, b in enumerate(sb):
            if i + j <= 5:
                hi, e = K9._two_sum(hi, a @ b)
                lo += e
    left = k * 2.0 ** (-WIDE_BITS * 6) * 1.01 * ma * mb + np.abs(ra) @ np.abs(B) + np.abs(A) @ np.abs(rb) + 2.0 ** -100 * np.abs(hi)
    return hi, lo, left


# ---- the figures
def figures(L, W, S, B, nu, dtype):
    """dict(e1_max, e1_rms, e2_max, e2_rms) of the judged L (r x r; only its lower triangle is read) and W (r x (n + 1)); a list of failures second"""
    u, r = u_of(dtype), len(S)
    L = np.tril(np.asarray(L, np.float64))
    W = np.asarray(W, np.float64)
    Bn = np.concatenate([B, nu[:, None]], axis=1)
    assert L.shape == (r, r) and W.shape == Bn.shape
    bad = []
    if not (np.isfinite(L).all() and np.isfinite(W).all()):
        return dict(e1_max=np.inf, e1_rms=np.inf, e2_max=np.inf, e2_rms=np.inf), ["not finite"]
    if dtype == "f64":
        h1, l1, w1 = wide_matmul(L, L.T)
        n1 = np.abs((h1 - S) + l1)
        h2, l2, w2 = wide_matmul(L, W)
        n2 = np.abs((h2 - Bn) + l2)
        assert (w1 <= 2.0 ** -6 * u * np.abs(L) @ np.abs(L).T).all() and (w2 <= 2.0 ** -6 * u * np.abs(L) @ np.abs(W)).all(), "the wide reference is too coarse here"
    else:
        n1, n2 = np.abs(L @ L.T - S), np.abs(L @ W - Bn)
    out = {}
    for name, num, den, mask in (("e1", n1, np.abs(L) @ np.abs(L).T, np.tril(np.ones((r, r), bool))), ("e2", n2, np.abs(L) @ np.abs(W), np.ones(Bn.shape, bool))):
        zero = mask & (den == 0)
        if (num[zero] != 0).any():
            bad.append("%s: %d entries with a zero denominator and a non-zero residual" % (name, int((num[zero] != 0).sum())))
        e = np.where(den > 0, num / (u * np.where(den > 0, den, 1.0)), 0.0)[mask]
        out[name + "_max"], out[name + "_rms"] = float(e.max()), float(np.sqrt(np.mean(e * e)))
    zc = ~Bn.any(axis=0)
    if W[:, zc].any():
        bad.append("a zero column of B came back non-zero")
    return out, bad


# ---- the restatements
def _round(x, t):
    return np.asarray(x).astype(t)


def plain(S, B, nu, dtype):
    """(L, W) as float64 arrays holding values of the dtype"""
    t = DT[dtype]
    A = _round(S, t).copy()
    W = _round(np.concatenate([B, nu[:, None]], axis=1), t)
    r = len(A)
    L = np.zeros((r, r), t)
    for k in range(r):
        assert A[k, k] > 0, "not positive definite at row %d" % k
        d = np.sqrt(A[k, k])
        col = A[k + 1:, k] / d
        L[k, k], L[k + 1:, k] = d, col
        A[k + 1:, k + 1:] -= np.multiply.outer(col, col)
        W[k] = W[k] / d
        W[k + 1:] -= np.multiply.outer(col, W[k])
    assert L.dtype == t and W.dtype == t and A.dtype == t
    return L.astype(np.float64), W.astype(np.float64)


def _once(A, B, t):
    """A @ B rounded once to the dtype"""
    if t is np.float32:
        return (A.astype(np.float64) @ B.astype(np.float64)).astype(t)
    hi, lo, _ = wide_matmul(A, B)
    return hi + lo


def _mm6(A, B, pairs=SIX, acc=None):
    """acc + A @ B on the bf16 matrix cores' terms: three planes per operand, per 16-wide k-step the six plane products in mma6's order (those in
    `pairs`), each summed exactly and added to the f32 accumulator"""
    m, k = A.shape
    kp = round_up(k, 16)
    Ap, Bp = np.zeros((m, kp), np.float32), np.zeros((kp, B.shape[1]), np.float32)
    Ap[:, :k], Bp[:k] = A, B
    pa, pb = [p.astype(np.float64) for p in split3(Ap)], [p.astype(np.float64) for p in split3(Bp)]
    acc = np.zeros((m, B.shape[1]), np.float32) if acc is None else acc.astype(np.float32)
    for q in range(0, kp, 16):
        for x, y in SIX:
            if (x, y) in pairs:
                acc = (acc.astype(np.float64) + pa[x][:, q:q + 16] @ pb[y][q:q + 16]).astype(np.float32)
    return acc


def _panels(S, B, nu, t, prod_s, prod_w_acc, prod_w, skip_s=None, skip_w=None):
    """the blocked scheme shared by `blocked` and `emulate_cholp`.  prod_s(A, B): a product from zero; prod_w_acc(C, A, B): C - A B accumulated;
    prod_w(A, B): M_J C_J.  skip_s = (i, k, J): tile A(i,k) misses panel J's update; skip_w = (j, J, c0, c1): columns c0:c1 of C_j miss L(j,J) W_J"""
    A = _round(S, t).copy()
    C = _round(np.concatenate([B, nu[:, None]], axis=1), t)
    r = len(A)
    nrb = -(-r // NB)
    L, W = np.zeros((r, r), t), np.zeros(C.shape, t)
    sl = [slice(J * NB, min(r, J * NB + NB)) for J in range(nrb)]
    for J in range(nrb):
        sJ = sl[J]
        m = sJ.stop - sJ.start
        LJ, M = plain(A[sJ, sJ].astype(np.float64), np.eye(m), np.zeros(m), "f32" if t is np.float32 else "f64")
        LJ, M = LJ.astype(t), M[:, :m].astype(t)
        L[sJ, sJ] = LJ
        W[sJ] = prod_w(M, C[sJ])
        for i in range(J + 1, nrb):
            L[sl[i], sJ] = prod_s(A[sl[i], sJ], M.T)
        for i in range(J + 1, nrb):
            for k in range(J + 1, i + 1):
                if skip_s != (i, k, J):
                    A[sl[i], sl[k]] = A[sl[i], sl[k]] - prod_s(L[sl[i], sJ], L[sl[k], sJ].T)
            new = prod_w_acc(C[sl[i]], L[sl[i], sJ], W[sJ])
            if skip_w is not None and skip_w[:2] == (i, J):
                new[:, skip_w[2]:skip_w[3]] = C[sl[i], skip_w[2]:skip_w[3]]
            C[sl[i]] = new
    assert L.dtype == t and W.dtype == t
    return L.astype(np.float64), W.astype(np.float64)


def blocked(S, B, nu, dtype):
    t = DT[dtype]
    return _panels(S, B, nu, t, lambda a, b: _once(a, b, t), lambda c, a, b: c - _once(a, b, t), lambda a, b: _once(a, b, t))


def emulate_cholp(S, B, nu, pairs_w=SIX, skip_s=None, skip_w=None):
    return _panels(S, B, nu, np.float32, _mm6, lambda c, a, b: -_mm6(a, b, pairs_w, -c), lambda a, b: _mm6(a, b, pairs_w), skip_s, skip_w)


NO_02 = tuple(p for p in SIX if p != (0, 2))


def mutants(r, n):
    """{name: keyword arguments of emulate_cholp}: the three mistakes the gate must catch; the block mutants need two panels"""
    out = {"strips drop (0,2)": dict(pairs_w=NO_02)}
    if r > NB:
        last = -(-r // NB) - 1
        out["tile misses a rank-64 update"] = dict(skip_s=(last, last, 0))
        c0 = 32 if n + 1 > 32 else 0                                 # a strip is 32 columns of [B | nu]
        out["strip misses L(J,K) W_K"] = dict(skip_w=(last, 0, c0, min(c0 + 32, n + 1)))
    return out


# ---- the cases
CONTEXTS = ((3, 8), (20, 96), (96, 96), (40, 520))                # (N, cap): n = 31 (rcap 128), 133 and 589 (rcap 256), 253 (ld = 3200, rcap 1152)
ROWS = {
    (3, 8): (1, 7, 8, 9, 56, 57, 63, 64, 65, 120, 121, 127, 128),
    (20, 96): (63, 64, 65, 127, 128, 129, 192),
    (96, 96): (57, 121, 129, 192),
    (40, 520): (9, 65, 192, 768, 832, 1000, 1024, 1025, 1152),
}
BIG = (40, 520)
EXACT_MAX_R = 1088
TRAIL_ROWS = (704, 960, 1024)                                     # 11, 15 and 16 panels
TRAIL_KNOBS = ((1, 2), (4, 2), (4, 0))                            # (PRE3_CHOL_TRAIL_P, PRE3_CHOL_TRAIL_T128) with PRE3_CHOL_TRAIL_SPLIT=1
MODE1_ROWS = (9, 65, 192, 832)
MODE1_CONTEXTS = ((20, 96), (40, 520))


def _case(N, cap, r, cls, kappa, dtype):
    return dict(N=N, cap=cap, n=state_size(N), r=r, cls=cls, kappa=kappa, dtype=dtype)


def cases_for(N, cap, rows, dtype):
    out = []
    for r in rows:
        assert round_up(r, NB) <= rcap_of(cap)
        if r <= EXACT_MAX_R:
            out.append(_case(N, cap, r, "exact", 0, dtype))
        out += [_case(N, cap, r, "acc", k, dtype) for k in KAPPAS]
    return out


def group_cases(group, dtype):
    """'cholp': 2 .. 16 panels; 'cholp1': one panel (predicted_prior); 'step': the launch-per-panel forms, every r; 'trail': the trailing sweeps' rows"""
    out = []
    for N, cap in CONTEXTS:
        rows = ROWS[(N, cap)]
        if group == "cholp":
            rows = [r for r in rows if 2 <= -(-r // NB) <= 16]
        elif group == "cholp1":
            rows = [r for r in rows if r <= NB]
        elif group == "trail":
            rows = TRAIL_ROWS if (N, cap) == BIG else ()
        elif group != "step":
            raise KeyError(group)
        out += cases_for(N, cap, rows, dtype)
    return out


def key_of(c):
    return "n%d_r%d_k%d_%s" % (c["n"], c["r"], c["kappa"], c["dtype"])


def accuracy_keys():
    """every accuracy input a device test uses, once: {key: (n, r, kappa, dtype)}"""
    keys = {}
    for g, dt in (("step", "f32"), ("step", "f64"), ("trail", "f32")):
        for c in group_cases(g, dt):
            if c["cls"] == "acc":
                keys[key_of(c)] = (c["n"], c["r"], c["kappa"], c["dtype"])
    return keys


def inputs(c):
    """(S, B, nu) of a case"""
    return accuracy_case(c["n"], c["r"], c["kappa"], c["dtype"]) if c["cls"] == "acc" else exact_case(c["n"], c["r"])[:3]


FIGS = ("e1_max", "e1_rms", "e2_max", "e2_rms")


def judge(c, L, W, gates):
    """what the device tests assert of one case: L is r x r, W is round_up(r, 64) x (n + 1).  Returns (list of failures, figures)"""
    r, bad, fig = c["r"], [], {}
    if W[r:].any():
        bad.append("%d non-zero entries in the padded rows of W" % int((W[r:] != 0).sum()))
    W = W[:r]
    if not (np.isfinite(L).all() and np.isfinite(W).all()):
        return bad + ["not finite"], fig
    if c["cls"] == "exact":
        _, _, _, L0, W0 = exact_case(c["n"], r)
        if not np.array_equal(np.tril(L), L0):
            bad.append("%d entries of L differ from L0, by up to %g" % (int((np.tril(L) != L0).sum()), float(np.abs(np.tril(L) - L0).max())))
        if not np.array_equal(W, W0):
            bad.append("%d entries of W differ from W0, by up to %g" % (int((W != W0).sum()), float(np.abs(W - W0).max())))
    else:
        S, B, nu = inputs(c)
        fig, bad2 = figures(L, W, S, B, nu, c["dtype"])
        bad += bad2
        g = gates[key_of(c)]
        for f in FIGS:
            if not fig[f] <= g["gate"][f]:
                bad.append("%s %.3g u above the gate %.3g (plain %.3g, blocked %.3g)" % (f, fig[f], g["gate"][f], g["plain"][f], g["blocked"][f]))
    return bad, fig
