// pre3_vodev.h -- the device bodies of the VO front end's 4-point RANSAC, shared by the kernels that take pnum and the hypothesis count
// from the host (pre3_vo.hip, pre3_draws.hip) and by the ones that read them from a device header block (pre3_vopair.hip).
//   vodometry_dr_ye.m:162-236  (adaptive count, winner, final fit, error statistics)
//   ransac_dr_ye.m:13-23,28-72 (point gathering from the range images, inlier radius, the draw rule, per-hypothesis support)
//   find_transform_matrix_dr_ye.m:8-41 (centroids, H = sum q2 q1', svd, V U', reflection handling)
//   R2e.m:21-23, R2q.m, Calculate_V_Omega_RANSAC_dr_ye.m:40-50 (Euler angles and the u = [T; q] the predict kernel consumes)
// One text, so one arithmetic: both families of kernels give the same bits on the same inputs.  All fp64, no contraction (the inlier test is a
// discontinuity; keep the operation order of the reference's loops).
#pragma once
#include "pre3_internal.h"
#include "pre3_philox.h"
#include "pre3_svd3.h"

namespace pre3 {

struct VoOut {                 // device-side result block
    double rot[9], trans[3], euler[3], u[7];
    double error_mean, error_std, dist;
    int32_t sta, n_support, n_iterations, best, dist_ok, pad[3];
};
inline void vo_result(const VoOut &o, pre3_vo_result *res)      // the block as the ABI hands it out
{
    memcpy(res->rot, o.rot, sizeof o.rot); memcpy(res->trans, o.trans, sizeof o.trans); memcpy(res->euler, o.euler, sizeof o.euler);
    memcpy(res->u, o.u, sizeof o.u);
    res->error_mean = o.error_mean; res->error_std = o.error_std; res->dist = o.dist;
    res->sta = o.sta; res->n_support = o.n_support; res->n_iterations = o.n_iterations; res->best = o.best;
}

// find_transform_matrix_dr_ye.m:19-44 from the centroids and H
__device__ inline int vo_solve(const double *H, const double *ct1, const double *ct2, double *rot, double *trans)
{
#pragma clang fp contract(off)
    double U[9], sv[3], V[9], Xq[9];
    vo_svd3(H, U, sv, V);
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) Xq[3 * i + j] = V[3 * i] * U[3 * j] + V[3 * i + 1] * U[3 * j + 1] + V[3 * i + 2] * U[3 * j + 2];
    const double mdet = Xq[0] * (Xq[4] * Xq[8] - Xq[5] * Xq[7]) - Xq[1] * (Xq[3] * Xq[8] - Xq[5] * Xq[6]) + Xq[2] * (Xq[3] * Xq[7] - Xq[4] * Xq[6]);
    int state;
    if (round(mdet) == 1) state = 1;
    else if (round(mdet) == -1) {
        int zn = -1, cnt = 0;
        for (int j = 0; j < 3; ++j) if (fabs(sv[j]) < 0.00000000000001) { zn = j; ++cnt; }
        if (cnt == 1) {
            for (int i = 0; i < 3; ++i) V[3 * i + zn] = -V[3 * i + zn];
            for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) Xq[3 * i + j] = V[3 * i] * U[3 * j] + V[3 * i + 1] * U[3 * j + 1] + V[3 * i + 2] * U[3 * j + 2];
            state = 2;
        } else state = -1;
    } else state = 0;
    if (state >= 1) {
        for (int i = 0; i < 9; ++i) rot[i] = Xq[i];
        for (int i = 0; i < 3; ++i) trans[i] = ct1[i] - (rot[3 * i] * ct2[0] + rot[3 * i + 1] * ct2[1] + rot[3 * i + 2] * ct2[2]);
    } else {
        for (int i = 0; i < 9; ++i) rot[i] = H[i];
        trans[0] = trans[1] = trans[2] = 0;
    }
    return state;
}

// ransac_dr_ye.m:13-19 for match position i of one frame: pset(:,i) = [-x(ROW,COL); -y(ROW,COL); z(ROW,COL)]; bad: bit 0 an unknown keypoint, bit 1 a pixel
// outside the image
__device__ __forceinline__ void vo_gather_one(const int i, int rows, int cols, const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ z,
                                              int ldf, const double *__restrict__ frm, int K, const double *__restrict__ sel, int sel_stride,
                                              double *__restrict__ pset, int32_t *__restrict__ bad)
{
    const int k = (int)sel[(size_t)i * sel_stride] - 1;
    if (k < 0 || k >= K) { atomicOr(bad, 1); return; }
    const int COL = (int)round(frm[(size_t)ldf * k]), ROW = (int)round(frm[(size_t)ldf * k + 1]);
    if (ROW < 1 || ROW > rows || COL < 1 || COL > cols) { atomicOr(bad, 2); return; }
    const size_t o = (size_t)(COL - 1) * rows + (ROW - 1);
    pset[3 * i] = -x[o]; pset[3 * i + 1] = -y[o]; pset[3 * i + 2] = z[o];
}

// ransac_dr_ye.m:20-23 -- one wave (lane = threadIdx.x)
__device__ __forceinline__ void vo_dist_wave(int pnum, const double *__restrict__ pset2, VoOut *__restrict__ out)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x;
    double mz = INFINITY;
    for (int k = lane; k < pnum; k += 64) {
        const double a = pset2[3 * k], b = pset2[3 * k + 1], c = pset2[3 * k + 2];
        const double nr = sqrt(c * c + b * b + a * a);
        if (nr > 0.4 && c < mz) mz = c;
    }
    for (int o = 32; o > 0; o >>= 1) { const double v = __shfl_xor(mz, o, 64); mz = v < mz ? v : mz; }
    int first = 0x7fffffff;
    for (int k = lane; k < pnum; k += 64) if (pset2[3 * k + 2] == mz && k < first) first = k;
    for (int o = 32; o > 0; o >>= 1) { const int v = __shfl_xor(first, o, 64); first = v < first ? v : first; }
    if (lane == 0) {
        const bool ok = mz < INFINITY && first < pnum;
        out->dist_ok = ok;
        out->dist = ok ? sqrt(pset2[3 * first] * pset2[3 * first] + pset2[3 * first + 1] * pset2[3 * first + 1] + pset2[3 * first + 2] * pset2[3 * first + 2]) : 0.0;
    }
}

// ransac_dr_ye.m:48-72 for hypothesis hyp -- one wave
__device__ __forceinline__ void vo_score_hyp(const int hyp, int pnum, const double *__restrict__ pset1, const double *__restrict__ pset2,
                                             const int32_t *__restrict__ draws, const VoOut *__restrict__ out, int words,
                                             unsigned long long *__restrict__ masks, int32_t *__restrict__ cnum, int32_t *__restrict__ state)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x;
    double ct1[3] = { 0, 0, 0 }, ct2[3] = { 0, 0, 0 }, H[9], rot[9], tr[3];
    int d[4];
    for (int s = 0; s < 4; ++s) d[s] = draws[4 * hyp + s];
    for (int s = 0; s < 4; ++s) for (int i = 0; i < 3; ++i) { ct1[i] += pset1[3 * d[s] + i]; ct2[i] += pset2[3 * d[s] + i]; }
    for (int i = 0; i < 3; ++i) { ct1[i] /= 4; ct2[i] /= 4; }
    for (int i = 0; i < 9; ++i) H[i] = 0;
    for (int s = 0; s < 4; ++s) {
        double q1[3], q2[3];
        for (int i = 0; i < 3; ++i) { q1[i] = pset1[3 * d[s] + i] - ct1[i]; q2[i] = pset2[3 * d[s] + i] - ct2[i]; }
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) H[3 * i + j] += q2[i] * q1[j];
    }
    const int st = vo_solve(H, ct1, ct2, rot, tr);
    const double thr = 0.001 * out->dist;
    int cnt = 0;
    for (int w = 0; w < words; ++w) {
        const int k = w * 64 + lane;
        int in = 0;
        if (k < pnum) {
            double dd = 0;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                double v = rot[3 * i] * pset2[3 * k] + rot[3 * i + 1] * pset2[3 * k + 1] + rot[3 * i + 2] * pset2[3 * k + 2];
                v = v + tr[i];
                const double e = v - pset1[3 * k + i];
                dd = dd + e * e;
            }
            in = dd < thr;
        }
        const unsigned long long b = __ballot(in);
        if (lane == 0) masks[(size_t)hyp * words + w] = b;
        cnt += __popcll(b);
    }
    if (lane == 0) { cnum[hyp] = cnt; state[hyp] = st; }
}

// vodometry_dr_ye.m:185-236: winner = first maximum, adaptive count, final fit on its inliers, error statistics -- one wave
__device__ __forceinline__ void vo_final_wave(int pnum, int n_hyp, const double *__restrict__ pset1, const double *__restrict__ pset2,
                                              const int32_t *__restrict__ cnum, int words, const unsigned long long *__restrict__ masks,
                                              VoOut *__restrict__ out, int32_t *__restrict__ inl_out)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x;
    int bc = -1, bi = 0x7fffffff;
    for (int i = lane; i < n_hyp; i += 64) { const int c = cnum[i]; if (c > bc) { bc = c; bi = i; } }
    for (int o = 32; o > 0; o >>= 1) {
        const int oc = __shfl_xor(bc, o, 64), oi = __shfl_xor(bi, o, 64);
        if (oc > bc || (oc == bc && oi < bi)) { bc = oc; bi = oi; }
    }
    // nIterations is overwritten at every strict improvement, so its final value belongs to the global maximum (:185-188)
    double nIter = n_hyp;
    if (bc > 0) nIter = 5 * ceil(log(0.01) / log(1 - pow((double)bc / pnum, 4)));
    const int n_it = (int)(nIter < n_hyp ? nIter : n_hyp);
    for (int k = lane; k < pnum; k += 64) inl_out[k] = bc >= 3 ? (int)((masks[(size_t)bi * words + (k >> 6)] >> (k & 63)) & 1ull) : 0;
    if (bc < 3) {                                                                          // :198-205
        if (lane == 0) { out->sta = 4; out->n_support = bc < 0 ? 0 : bc; out->n_iterations = n_it; out->best = bi;
                         for (int i = 0; i < 9; ++i) out->rot[i] = 0; for (int i = 0; i < 3; ++i) { out->trans[i] = 0; out->euler[i] = 0; }
                         out->error_mean = out->error_std = 0; out->u[0] = out->u[1] = out->u[2] = 0; out->u[3] = 1; out->u[4] = out->u[5] = out->u[6] = 0; }
        return;
    }
    const unsigned long long *mk = masks + (size_t)bi * words;
    // centroids, then H = sum q2 q1' over the inliers (lane-strided partial sums, butterfly-reduced)
    double s[6] = { 0, 0, 0, 0, 0, 0 };
    for (int k = lane; k < pnum; k += 64)
        if ((mk[k >> 6] >> (k & 63)) & 1ull) for (int i = 0; i < 3; ++i) { s[i] += pset1[3 * k + i]; s[3 + i] += pset2[3 * k + i]; }
    for (int o = 32; o > 0; o >>= 1) for (int i = 0; i < 6; ++i) s[i] += __shfl_xor(s[i], o, 64);
    double ct1[3], ct2[3], H[9];
    for (int i = 0; i < 3; ++i) { ct1[i] = s[i] / bc; ct2[i] = s[3 + i] / bc; }
    for (int i = 0; i < 9; ++i) H[i] = 0;
    for (int k = lane; k < pnum; k += 64)
        if ((mk[k >> 6] >> (k & 63)) & 1ull) {
            double q1[3], q2[3];
            for (int i = 0; i < 3; ++i) { q1[i] = pset1[3 * k + i] - ct1[i]; q2[i] = pset2[3 * k + i] - ct2[i]; }
            for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) H[3 * i + j] += q2[i] * q1[j];
        }
    for (int o = 32; o > 0; o >>= 1) for (int i = 0; i < 9; ++i) H[i] += __shfl_xor(H[i], o, 64);
    double rot[9], tr[3];
    const int sta = vo_solve(H, ct1, ct2, rot, tr);
    // ErrorRANSAC_Norm, mean and (N-1)-normalised std (:222-225)
    double se = 0;
    for (int k = lane; k < pnum; k += 64)
        if ((mk[k >> 6] >> (k & 63)) & 1ull) {
            double s2 = 0;
            for (int i = 0; i < 3; ++i) {
                const double v = rot[3 * i] * pset2[3 * k] + rot[3 * i + 1] * pset2[3 * k + 1] + rot[3 * i + 2] * pset2[3 * k + 2] + tr[i] - pset1[3 * k + i];
                s2 += v * v;
            }
            se += sqrt(s2);
        }
    for (int o = 32; o > 0; o >>= 1) se += __shfl_xor(se, o, 64);
    const double mean = se / bc;
    double var = 0;
    for (int k = lane; k < pnum; k += 64)
        if ((mk[k >> 6] >> (k & 63)) & 1ull) {
            double s2 = 0;
            for (int i = 0; i < 3; ++i) {
                const double v = rot[3 * i] * pset2[3 * k] + rot[3 * i + 1] * pset2[3 * k + 1] + rot[3 * i + 2] * pset2[3 * k + 2] + tr[i] - pset1[3 * k + i];
                s2 += v * v;
            }
            const double e = sqrt(s2) - mean;
            var += e * e;
        }
    for (int o = 32; o > 0; o >>= 1) var += __shfl_xor(var, o, 64);
    if (lane == 0) {
        for (int i = 0; i < 9; ++i) out->rot[i] = rot[i];
        for (int i = 0; i < 3; ++i) out->trans[i] = tr[i];
        out->error_mean = mean; out->error_std = bc > 1 ? sqrt(var / (bc - 1)) : 0.0;
        out->sta = sta; out->n_support = bc; out->n_iterations = n_it; out->best = bi;
        out->euler[0] = out->euler[1] = out->euler[2] = 0;
        if (sta >= 1) { out->euler[0] = atan2(rot[7], rot[8]); out->euler[1] = asin(-rot[6]); out->euler[2] = atan2(rot[3], rot[0]); }   // R2e.m:21-23
        // Calculate_V_Omega_RANSAC_dr_ye.m:40-50: u = [T; R2q(R)], identity unless sta == 1
        double R[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 }, T3[3] = { 0, 0, 0 };
        if (sta == 1) { for (int i = 0; i < 9; ++i) R[i] = rot[i]; for (int i = 0; i < 3; ++i) T3[i] = tr[i]; }
        const double Tq = R[0] + R[4] + R[8] + 1;
        double a, b, c, d, S;
        if (Tq > 0.00000001) { S = 2 * sqrt(Tq); a = 0.25 * S; b = (R[5] - R[7]) / S; c = (R[6] - R[2]) / S; d = (R[1] - R[3]) / S; }
        else if (R[0] > R[4] && R[0] > R[8]) { S = 2 * sqrt(1.0 + R[0] - R[4] - R[8]); a = (R[5] - R[7]) / S; b = 0.25 * S; c = (R[1] + R[3]) / S; d = (R[6] + R[2]) / S; }
        else if (R[4] > R[8]) { S = 2 * sqrt(1.0 + R[4] - R[0] - R[8]); a = (R[6] - R[2]) / S; b = (R[1] + R[3]) / S; c = 0.25 * S; d = (R[5] + R[7]) / S; }
        else { S = 2 * sqrt(1.0 + R[8] - R[0] - R[4]); a = (R[1] - R[3]) / S; b = (R[6] + R[2]) / S; c = (R[5] + R[7]) / S; d = 0.25 * S; }
        out->u[0] = T3[0]; out->u[1] = T3[1]; out->u[2] = T3[2]; out->u[3] = a; out->u[4] = -b; out->u[5] = -c; out->u[6] = -d;
    }
}

// ransac_dr_ye.m:28-48 for hypothesis h (one lane each; every lane of the wave reaches the ballot).  *capped is zero when the launch starts
__device__ __forceinline__ void vo_draw_lane(const int h, uint64_t seed, uint64_t seq, int n_hyp, int pnum, const double *__restrict__ m1, const double *__restrict__ m2,
                                             int ms, int32_t *__restrict__ draws, int32_t *__restrict__ capped)
{
    int cap = 0;
    if (h < n_hyp) {
        int32_t r[4];
        cap = draw_rule_vo(seed, seq, pnum, m1, m2, ms, h, r);
        *reinterpret_cast<int4 *>(draws + 4 * (size_t)h) = make_int4(r[0], r[1], r[2], r[3]);
    }
    const int n = __popcll(__ballot(cap != 0));         // (every lane of the wave reaches the ballot)
    if (threadIdx.x == 0 && n) atomicAdd(capped, n);
}

}  // namespace pre3
