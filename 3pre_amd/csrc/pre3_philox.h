// pre3_philox.h -- the counter-based random stream behind the seeded RANSAC entry points and the three draw rules on it.
// Philox4x64-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) with its public constants: one block is a pure
// function of (counter[4], key[2]); no state lives anywhere.  numpy.random.Philox is the same generator (it advances the counter before its first
// block): tests/test_draws_ref.py pins tests/draws_ref.py's restatement against it, tests/test_gpu_draws.py the kernels against the restatement.
//   key     = [seed, stream]               stream 1: 1-point RANSAC, 2: VO 4-point RANSAC, 3: floor-plane RANSAC, 4: the candidates' weighted order,
//                                          5: initialize_a_feature's box centres (counter [attempt, 0, seq, 0]), 6: the EPnP RANSAC's samples
//   counter = [index, attempt, seq, 0]     index: the hypothesis; attempt: the redraw number (0 = first draw); seq: the caller's frame / step number
// A bounded integer in [0, range) is the high 64 bits of word * range: no rejection, so value v is drawn with probability floor- or ceil-(2^64 / range)
// / 2^64 -- a bias of at most range / 2^64 (below 2^-50 for every range of this library).  A uniform double is the word's top 53 bits times 2^-53.
// Everything here is __host__ __device__: the same text runs in the kernels (pre3_draws.hip) and in a host program that checks them.
#pragma once
#include <stdint.h>
#include <math.h>

#if defined(__HIPCC__)
#define PRE3_HD __host__ __device__ inline
#else
#define PRE3_HD inline
#endif

namespace pre3 {

constexpr uint64_t PHILOX_M0 = 0xD2E7470EE14C6C93ull, PHILOX_M1 = 0xCA5A826395121157ull;
constexpr uint64_t PHILOX_W0 = 0x9E3779B97F4A7C15ull, PHILOX_W1 = 0xBB67AE8584CAA73Bull;
enum { DRAW_STREAM_1P = 1, DRAW_STREAM_VO = 2, DRAW_STREAM_PLANE = 3, DRAW_STREAM_CAND = 4,
       DRAW_STREAM_FAST = 5 /* initialize_a_feature.m:64: counter [attempt, 0, seq, 0], words 0 and 1 -> the box centre's two uniforms */,
       DRAW_STREAM_PNP = 6 /* the EPnP RANSAC's six-point samples: counter [hypothesis, block 0 or 1, seq, 0] */ };
constexpr int VO_MAX_REDRAWS = 64;          // per position; ransac_dr_ye.m:28-46 loops for ever
constexpr int PLANE_MAX_ATTEMPTS = 100;     // ransac.m:122 maxDataTrials

PRE3_HD uint64_t mulhi64(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

struct PhiloxBlock { uint64_t w[4]; };

PRE3_HD PhiloxBlock philox_block(uint64_t c0, uint64_t c1, uint64_t c2, uint64_t c3, uint64_t k0, uint64_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) { k0 += PHILOX_W0; k1 += PHILOX_W1; }
        const uint64_t h0 = mulhi64(PHILOX_M0, c0), l0 = PHILOX_M0 * c0, h1 = mulhi64(PHILOX_M1, c2), l1 = PHILOX_M1 * c2;
        c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
    }
    PhiloxBlock b;
    b.w[0] = c0; b.w[1] = c1; b.w[2] = c2; b.w[3] = c3;
    return b;
}

PRE3_HD PhiloxBlock draw_block(uint64_t seed, int stream, uint64_t index, uint64_t attempt, uint64_t seq)
{
    return philox_block(index, attempt, seq, 0, seed, (uint64_t)stream);
}

PRE3_HD int draw_bounded(uint64_t w, int range) { return (int)mulhi64(w, (uint64_t)range); }
PRE3_HD double draw_uniform(uint64_t w) { return (double)(w >> 11) * 1.1102230246251565e-16; }      // 2^-53

// three distinct of m (m >= 3) with randperm(m)(1:3)'s distribution: ranks in [0,m), [0,m-1), [0,m-2), each later one shifted past the earlier picks
// in ascending order (a partial Fisher-Yates on ranks) -- no redraws
PRE3_HD void draw_three_distinct(int m, const PhiloxBlock &b, int32_t out[3])
{
    const int i0 = draw_bounded(b.w[0], m);
    int i1 = draw_bounded(b.w[1], m - 1);
    if (i1 >= i0) ++i1;
    int i2 = draw_bounded(b.w[2], m - 2);
    const int lo = i0 < i1 ? i0 : i1, hi = i0 < i1 ? i1 : i0;
    if (i2 >= lo) ++i2;
    if (i2 >= hi) ++i2;
    out[0] = i0; out[1] = i1; out[2] = i2;
}

// ---- the EPnP RANSAC's table (pre3_pnp.hip): six distinct of n (n >= 6) for hypothesis h -- ranks in [0,n), [0,n-1), ..., [0,n-5),
// each later one shifted past the earlier picks in ascending order: draw_three_distinct's rule continued.  Ranks 0..3 are words 0..3 of
// block(h, 0, seq), ranks 4 and 5 words 0 and 1 of block(h, 1, seq).  No redraws; every index a compile-time one (no per-lane array in memory).
PRE3_HD void draw_rule_pnp(uint64_t seed, uint64_t seq, int n, int h, int32_t out[6])
{
    const PhiloxBlock b0 = draw_block(seed, DRAW_STREAM_PNP, (uint64_t)h, 0, seq), b1 = draw_block(seed, DRAW_STREAM_PNP, (uint64_t)h, 1, seq);
    int32_t sorted[6] = { 0, 0, 0, 0, 0, 0 };
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        int r = draw_bounded(j < 4 ? b0.w[j & 3] : b1.w[j & 3], n - j);
#pragma unroll
        for (int s = 0; s < j; ++s) if (r >= sorted[s]) ++r;
        out[j] = r;
        sorted[j] = r;
#pragma unroll
        for (int s = j; s > 0; --s)
            if (sorted[s - 1] > sorted[s]) { const int32_t t = sorted[s]; sorted[s] = sorted[s - 1]; sorted[s - 1] = t; }
    }
}

// ---- select_random_match.m:40-51: k positions of hypothesis h in the individually compatible list of m (k = 3 when m > 3, else 1; m == 0: zero)
PRE3_HD void draw_rule_1p(uint64_t seed, uint64_t seq, int m, int k, int h, int32_t *out /* [k] */)
{
    if (m <= 0) { for (int s = 0; s < k; ++s) out[s] = 0; return; }
    const PhiloxBlock b = draw_block(seed, DRAW_STREAM_1P, (uint64_t)h, 0, seq);
    if (k == 3) draw_three_distinct(m, b, out);
    else out[0] = draw_bounded(b.w[0], m);
}

// ---- ransac_dr_ye.m:28-48.  round((pnum - 1) * u + 1), MATLAB rounding, then 0-based
PRE3_HD int vo_position(int pnum, uint64_t w)
{
#pragma clang fp contract(off)
    const double u = draw_uniform(w);
    double v = (double)(pnum - 1) * u;
    v = v + 1.0;
    v = v + 0.5;
    return (int)floor(v) - 1;
}

// whether position p (1..3) must be redrawn: it repeats an earlier position or ind_dup<p> fires -- the reference's comparisons as they stand, the
// mixed-row ones of ind_dup3 (match(1,.) against match(2,.)) included.  m1 / m2: the two rows of the match list, element stride `ms`
PRE3_HD bool vo_bad(const double *m1, const double *m2, int ms, const int *r, int p)
{
#define M1(i) m1[(size_t)(i) * ms]
#define M2(i) m2[(size_t)(i) * ms]
    if (p == 1) return r[1] == r[0] || M1(r[0]) == M1(r[1]) || M2(r[0]) == M2(r[1]);
    if (p == 2) return r[2] == r[0] || r[2] == r[1] || M1(r[0]) == M1(r[2]) || M1(r[1]) == M1(r[2]) || M2(r[0]) == M2(r[2]) || M2(r[1]) == M2(r[2]);
    return r[3] == r[0] || r[3] == r[1] || r[3] == r[2] || M1(r[0]) == M1(r[3]) || M1(r[1]) == M2(r[3]) || M1(r[2]) == M1(r[3]) || M2(r[0]) == M1(r[3])
           || M2(r[1]) == M2(r[3]) || M2(r[2]) == M2(r[3]);
#undef M1
#undef M2
}

// The four first draws are words 0..3 of block(h, 0); the redraw of position p at attempt a >= 1 is word p of block(h, a).  A position stops after
// VO_MAX_REDRAWS redraws and keeps its last value.  Returns 1 when a position is still inadmissible then (a capped hypothesis).
PRE3_HD int draw_rule_vo(uint64_t seed, uint64_t seq, int pnum, const double *m1, const double *m2, int ms, int h, int32_t out[4])
{
    int r[4];
    const PhiloxBlock b0 = draw_block(seed, DRAW_STREAM_VO, (uint64_t)h, 0, seq);
    for (int p = 0; p < 4; ++p) r[p] = vo_position(pnum, b0.w[p]);
    int capped = 0;
    for (int p = 1; p < 4; ++p) {
        int a = 0;
        bool bad = vo_bad(m1, m2, ms, r, p);
        while (bad && a < VO_MAX_REDRAWS) {
            ++a;
            const PhiloxBlock b = draw_block(seed, DRAW_STREAM_VO, (uint64_t)h, (uint64_t)a, seq);
            r[p] = vo_position(pnum, p == 1 ? b.w[1] : (p == 2 ? b.w[2] : b.w[3]));
            bad = vo_bad(m1, m2, ms, r, p);
        }
        capped |= bad ? 1 : 0;
    }
    for (int p = 0; p < 4; ++p) out[p] = r[p];
    return capped;
}

// ---- ransac.m:142-176: three distinct of npts per attempt, redrawn while norm(cross(p2 - p1, p3 - p1)) < eps (iscolinear.m:62) on the cropped
// points as k_plane_score sees them, every product and sum rounded on its own; at most PLANE_MAX_ATTEMPTS attempts, the last one kept
PRE3_HD void draw_rule_plane(uint64_t seed, uint64_t seq, int npts, const double *X, const double *Y, const double *Z, int h, int32_t out[3])
{
#pragma clang fp contract(off)
    for (int a = 0; a < PLANE_MAX_ATTEMPTS; ++a) {
        const PhiloxBlock b = draw_block(seed, DRAW_STREAM_PLANE, (uint64_t)h, (uint64_t)a, seq);
        draw_three_distinct(npts, b, out);
        const double px = X[out[0]], py = Y[out[0]], pz = Z[out[0]];
        const double a0 = X[out[1]] - px, a1 = Y[out[1]] - py, a2 = Z[out[1]] - pz, b0 = X[out[2]] - px, b1 = Y[out[2]] - py, b2 = Z[out[2]] - pz;
        const double n0 = a1 * b2 - a2 * b1, n1 = a2 * b0 - a0 * b2, n2 = a0 * b1 - a1 * b0;
        const double nn = sqrt(n0 * n0 + n1 * n1 + n2 * n2);
        if (!(nn < 2.220446049250313e-16)) return;
    }
}

// ---- Weighted_Smpl_wo_replacement.m:3-4,24,28-34: the order of the initialisation candidates.  The reference draws one index at a
// time with probability proportional to the remaining weights w_i = mvnpdf(uv_i, mean, diag(sigma^2)) -- Plackett-Luce sampling, which an exponential
// race samples with no sequential dependence: candidate i gets key_i = E_i / w_i, E_i = -log1p(-U_i) a unit exponential, and the order is the
// candidates sorted by (key, index) ascending.  mean = round([W H] / 2), sigma = round([W H] / 6), MATLAB rounding (half away from zero); the
// normalising constant of the weights drops out, so key_i = E_i * exp(q_i), q_i = ((u - mu) / su)^2 / 2 + ((v - mv) / sv)^2 / 2.
struct CandBox { double mu, mv, su, sv; };

PRE3_HD double round_half_away(double v) { return v < 0.0 ? -floor(-v + 0.5) : floor(v + 0.5); }

// (su or sv == 0 -- a box below 3 pixels -- is refused by the entry points)
PRE3_HD CandBox cand_box(int box_w, int box_h)
{
    CandBox b;
    b.mu = round_half_away((double)box_w / 2.0); b.mv = round_half_away((double)box_h / 2.0);
    b.su = round_half_away((double)box_w / 6.0); b.sv = round_half_away((double)box_h / 6.0);
    return b;
}

// every quotient, product and sum rounded on its own, as numpy rounds them
PRE3_HD double cand_q(double u, double v, const CandBox &b)
{
#pragma clang fp contract(off)
    const double du = (u - b.mu) / b.su, dv = (v - b.mv) / b.sv;
    const double su2 = du * du, sv2 = dv * dv;
    const double s = su2 + sv2;
    return 0.5 * s;
}

// U = uniform(word 0 of block(i, 0, seq; seed, stream 4)).  For finite (u, v) the key is never NaN: q >= 0, so exp(q) is in [1, +inf]; E is in
// [0, 37) and E == 0 (U == 0) gives key 0 whatever exp(q) is -- the one product that could be 0 * inf is not formed.  +inf (a pixel absurdly far from
// the image) and 0 are legal keys: they sort by value, then by index.
PRE3_HD double cand_key(uint64_t seed, uint64_t seq, int i, double u, double v, const CandBox &b)
{
    const double U = draw_uniform(draw_block(seed, DRAW_STREAM_CAND, (uint64_t)i, 0, seq).w[0]);
    const double E = -log1p(-U);
    if (!(E > 0.0)) return 0.0;
    return E * exp(cand_q(u, v, b));
}

}  // namespace pre3
