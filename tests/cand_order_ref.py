"""The candidates' weighted order restated: the truth of pre3_candidate_order / pre3_map_policy_seeded.

Two independent statements of Weighted_Smpl_wo_replacement.m:
  * keys() / order(): the exponential race the library runs -- key_i = -log1p(-U_i) * exp(q_i), U_i the uniform of word 0 of
    draws_ref.block([i, 0, seq, 0], [seed, 4]), the order the stable argsort of the keys -- in numpy / Python floats;
  * weighted_sample(): the MATLAB file line by line, on a tape of uniforms: mvnpdf weights (:3-4, :24, the density as its definition writes it),
    then K times randsample(p, 1, true, w) as the inverse CDF on the normalised weights (randsample.m: edges = min([0 cumsum(p)], 1), edges(end) = 1,
    histc), the pick's weight zeroed and the rest re-normalised (:28-34).  Its last re-normalisation is 0 / 0: harmless, the loop has ended.
Both sample the Plackett-Luce distribution of the weights; pl_probability() gives an order's exact probability."""
import math

import numpy as np

import draws_ref as dr

STREAM_CAND = 4
BOX = (176, 144)             # BoxLimX(2), BoxLimY(2) of the reference: mean (88, 72), sigma (29, 24)


def matlab_round(v):
    """round(): half away from zero"""
    return math.floor(v + 0.5) if v >= 0 else -math.floor(-v + 0.5)


def box_params(box=BOX):
    W, H = box
    return (float(matlab_round(W / 2)), float(matlab_round(H / 2))), (float(matlab_round(W / 6)), float(matlab_round(H / 6)))


def q_of(uv, box=BOX):
    """0.5 * (((u - mu) / su)^2 + ((v - mv) / sv)^2), every operation rounded on its own"""
    (mu, mv), (su, sv) = box_params(box)
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    du, dv = (uv[:, 0] - mu) / su, (uv[:, 1] - mv) / sv
    return 0.5 * (du * du + dv * dv)


def weights(uv, box=BOX):
    """the normalised weights the race samples with"""
    w = np.exp(-q_of(uv, box))
    return w / w.sum()


def uniform_of(seed, seq, i):
    return dr.uniform(dr.block([i, 0, seq, 0], [seed, STREAM_CAND])[0])


def keys(uv, seed, seq, box=BOX, uniform=None):
    """key_i per candidate; uniform(i) replaces the stream (a stub).  E == 0 (U == 0) gives key 0 whatever exp(q) is: no key is NaN."""
    q = q_of(uv, box)
    out = np.zeros(len(q))
    with np.errstate(over="ignore"):
        for i in range(len(q)):
            U = uniform_of(seed, seq, i) if uniform is None else uniform(i)
            E = -math.log1p(-U)
            out[i] = 0.0 if not E > 0.0 else E * float(np.exp(q[i]))
    return out


def order_of_keys(k):
    """the candidates sorted by (key, index) ascending"""
    k = np.asarray(k)
    assert not np.isnan(k).any()
    return np.lexsort((np.arange(len(k)), k)).astype(np.int32)


def order(uv, seed, seq, box=BOX, uniform=None):
    return order_of_keys(keys(uv, seed, seq, box, uniform))


def min_relative_gap(k):
    """the smallest (k[i+1] - k[i]) / k[i+1] over adjacent sorted keys (inf for fewer than two)"""
    s = np.sort(np.asarray(k, np.float64))
    if len(s) < 2:
        return math.inf
    with np.errstate(invalid="ignore", divide="ignore"):
        g = (s[1:] - s[:-1]) / s[1:]
    return float(np.nanmin(g))


def pl_probability(w, perm):
    """P(order = perm) when each pick is proportional to the remaining weights"""
    w = np.asarray(w, np.float64)
    rest, p = w.sum(), 1.0
    for i in perm:
        p *= w[i] / rest
        rest -= w[i]
    return p


# ---- Weighted_Smpl_wo_replacement.m, line by line -----------------------------------------------------------------------------------------------------
def mvnpdf(x, mean, cov_diag):
    """mvnpdf(x, mean, diag(cov_diag)) for one 2-vector: exp(-0.5 * (x - m) Sigma^-1 (x - m)') / sqrt((2 pi)^2 |Sigma|)"""
    r0, r1 = math.sqrt(cov_diag[0]), math.sqrt(cov_diag[1])          # chol(Sigma) of a diagonal Sigma
    d0, d1 = (x[0] - mean[0]) / r0, (x[1] - mean[1]) / r1
    return math.exp(-0.5 * (d0 * d0 + d1 * d1)) / math.sqrt((2 * math.pi) ** 2 * cov_diag[0] * cov_diag[1])


def randsample_one(w, u):
    """randsample(p, 1, true, w) on the uniform u, 0-based: the bin of u in edges = min([0 cumsum(w / sum(w))], 1), edges(end) = 1"""
    p = w / w.sum()
    edges = np.minimum(np.r_[0.0, np.cumsum(p)], 1.0)
    edges[-1] = 1.0
    return int(np.searchsorted(edges, u, side="right")) - 1          # histc: edges(k) <= u < edges(k+1); empty bins are never hit


def matlab_weights(uv, box=BOX):
    """:3-4, :21-27: the normalised mvnpdf weights"""
    W, H = box
    mean = [matlab_round(W / 2), matlab_round(H / 2)]                                                    # :3
    cov = [matlab_round(W / 6) ** 2, matlab_round(H / 6) ** 2]                                           # :4
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    w = np.array([mvnpdf(uv[i], mean, cov) for i in range(len(uv))])                                     # :23-25
    return w / w.sum()                                                                                   # :27


def weighted_sample(uv, tape, box=BOX):
    """:28-34 on a tape of uniforms (an iterator); returns the 0-based WeightedSample_idx"""
    w = matlab_weights(uv, box)
    out = np.zeros(len(w), np.int32)
    for i in range(len(w)):                                                                              # :30
        out[i] = randsample_one(w, next(tape))                                                           # :31
        w[out[i]] = 0.0                                                                                  # :32
        with np.errstate(invalid="ignore", divide="ignore"):
            w = w / w.sum()                                                                              # :33 (the last one is 0 / 0)
    return out
