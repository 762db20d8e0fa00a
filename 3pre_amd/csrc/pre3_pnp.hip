// pre3_pnp.hip -- k_pnp_solve, k_pnp_hyp, k_pnp_select, k_pnp_draw: the camera pose from 3-D / 2-D correspondences by EPnP, and its RANSAC (DESIGN.md
// section 35; the algorithm, its quirks and what is left out: pre3_pnp.h).
//   aux_code/EPnP_matlab/EPnP/efficient_pnp.m:34-175 -- the solver mex_files/RANSAC_CALCULATION/RANSAC_CALC_VER2.m:187-191 leaves commented out
// k_pnp_solve   one workgroup of 256 threads per problem: the whole set, or the refit over an inlier list read on the device.
// k_pnp_hyp     one wave per hypothesis: the same body over its six sampled points, then all n correspondences scored under the answer.
// k_pnp_select  one workgroup: the winner (largest support, smallest inlier distance sum, lowest index) and its inlier list in ascending order.
// k_pnp_draw    one lane per hypothesis: six distinct of n (pre3_philox.h, stream 6).
// k_pnp_pair_prep  one workgroup behind a VO pair's launches (pre3_vo_pair_pnp_seeded): cur's pixels of the matches, the pair's inliers as a list.
// k_pnp_refine  one workgroup of 256 threads: Gauss-Newton on the reprojection error from a result block's pose, and the pose's covariance (pre3_pnpref.h;
//               DESIGN.md section 37).
// One body (pnp_body), templated on the thread count and on whether the points come through an index list.  Every sum over the points: thread t adds
// points t, t + NT, ... in ascending order, the lanes of a wave meet in the xor butterfly, the waves in wave order through LDS -- a tree whose shape
// depends on the count alone.  No floating-point atomics: equal bits from run to run.  The 12 x 12, its eigenvectors and the 6 x 7 system live in
// LDS (an index chosen at run time reaches them); the Jacobi round's six disjoint rotations are 72 + 72 two-entry items dealt over the lanes.  What
// every thread needs of a reduced sum it computes for itself: the scalars of a dimension (scale, sign, svd, pose) are the same in every thread.
// All fp64.  The chain of rotations and the handful of dependent passes make these kernels latency-bound: neither HBM nor the matrix cores limit them.
#include <cmath>
#include <cstring>
#include <vector>

#include "pre3_internal.h"
#include "pre3_geomdev.h"
#include "pre3_philox.h"
#include "pre3_pnp.h"
#include "pre3_pnpref.h"
#include "pre3_vodev.h"
#include "pre3_vopair.h"

namespace pre3 {

namespace {

static_assert(sizeof(pre3_pnp_result) == 22 * 8 + 4 * 4, "pre3_pnp_result is 22 doubles and four words");

// where the correspondences lie: Xw 3 x n_all and U 2 x n_all, column-major; undistort != 0: every pixel through undistort_fm_my_version.m first
struct PnpSrc { const double *Xw, *U; int n_all; CamD cam; int undistort; };
// what k_pnp_select leaves for the refit
struct PnpCtl { int32_t winner, support, pad[2]; };
// how many of the arrays' positions hold a correspondence: the launch's own count (PnpNHost: every caller but one), or a device word an earlier launch
// left, clamped to the launch's count (PnpNDev: pre3_relocalise_seeded, whose count is the matcher's).  Below six under PnpNDev the draw writes zeros,
// no hypothesis is solved and the selection leaves winner = -1, support = 0; nothing indexes beyond the count.
struct PnpNHost {};
struct PnpNDev { const int32_t *n; };
__device__ __forceinline__ int pnp_n(const PnpNHost &, int n) { return n; }
__device__ __forceinline__ int pnp_n(const PnpNDev &c, int n) { const int v = *c.n; return v < n ? (v < 0 ? 0 : v) : n; }
template <typename CN> constexpr bool pnp_n_dev = false;
template <> constexpr bool pnp_n_dev<PnpNDev> = true;
// a problem's answer, the same in every thread
struct PnpAns { double R[9], T[3], err[3]; int32_t best, sta; };

template <int NT> struct PnpLds {
    double A[144], V[144], acc[PNP_MTM], cs[12], X[12], w6[42], red[(NT / 64) * PNP_MTM];
    int32_t ord[3], flag;
};

template <int K, int NT> __device__ __forceinline__ void pnp_reduce(double (&v)[K], double *red)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (int i = 0; i < K; ++i) v[i] += __shfl_xor(v[i], o, 64);
    if constexpr (NT > 64) {
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < K; ++i) red[wv * K + i] = v[i];
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < K; ++i) {
            double s = red[i];
#pragma unroll
            for (int w = 1; w < NT / 64; ++w) s += red[w * K + i];
            v[i] = s;
        }
        __syncthreads();
    }
}

// point k of the problem: a list entry outside the arrays gives NaN coordinates (the answer is then sta = -1; the host checks a caller's table and the
// launches write indices below n_all: a guard, not a path)
template <bool IDX> __device__ __forceinline__ void pnp_point(const PnpSrc &s, const int32_t *idx, int k, double xw[3], double *u, double *v, bool pixel)
{
    int j = k;
    if (IDX) j = idx[k];
    if ((unsigned)j >= (unsigned)s.n_all) { xw[0] = xw[1] = xw[2] = NAN; *u = *v = NAN; return; }
    xw[0] = s.Xw[3 * (size_t)j]; xw[1] = s.Xw[3 * (size_t)j + 1]; xw[2] = s.Xw[3 * (size_t)j + 2];
    if (!pixel) return;
    const double ud = s.U[2 * (size_t)j], vd = s.U[2 * (size_t)j + 1];
    if (s.undistort) d_undistort10(s.cam, ud, vd, u, v);
    else { *u = ud; *v = vd; }
}

// one dimension's answer from its control points C (compute_norm_sign_scaling_factor.m, getrotT, the reprojection error): five passes over the points
template <int NT, bool IDX>
__device__ __forceinline__ void pnp_dim(const PnpSrc &s, const int32_t *idx, int n, const double wcent[3], double C[12], double *red, double R[9], double T[3], double *err)
{
    const int tid = threadIdx.x;
    double xw[3], a[4], xc[3], u, v;
    double s3[3] = { 0, 0, 0 };
#pragma unroll 1
    for (int k = tid; k < n; k += NT) {
        pnp_point<IDX>(s, idx, k, xw, &u, &v, false);
        pnp_alphas(xw[0], xw[1], xw[2], a); pnp_xc(a, C, xc);
        s3[0] += xc[0]; s3[1] += xc[1]; s3[2] += xc[2];
    }
    pnp_reduce<3, NT>(s3, red);
    const double cc_[3] = { s3[0] / n, s3[1] / n, s3[2] / n };
    double s2[2] = { 0, 0 };
#pragma unroll 1
    for (int k = tid; k < n; k += NT) {
        pnp_point<IDX>(s, idx, k, xw, &u, &v, false);
        pnp_alphas(xw[0], xw[1], xw[2], a); pnp_xc(a, C, xc);
        const double dc = pnp_dist3(xc, cc_), dw = pnp_dist3(xw, wcent);
        s2[0] += dc * dc; s2[1] += dc * dw;
    }
    pnp_reduce<2, NT>(s2, red);
    pnp_scale(s2[0], s2[1], C);
    double s4[4] = { 0, 0, 0, 0 };
#pragma unroll 1
    for (int k = tid; k < n; k += NT) {
        pnp_point<IDX>(s, idx, k, xw, &u, &v, false);
        pnp_alphas(xw[0], xw[1], xw[2], a); pnp_xc(a, C, xc);
        s4[0] += xc[0]; s4[1] += xc[1]; s4[2] += xc[2]; s4[3] += xc[2] < 0 ? 1.0 : 0.0;
    }
    pnp_reduce<4, NT>(s4, red);
    const double sg = s4[3] > 0 ? -1.0 : 1.0;                      // any z < 0: the whole Xc is negated
    const double ccent[3] = { sg * s4[0] / n, sg * s4[1] / n, sg * s4[2] / n };
    double M[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
#pragma unroll 1
    for (int k = tid; k < n; k += NT) {
        pnp_point<IDX>(s, idx, k, xw, &u, &v, false);
        pnp_alphas(xw[0], xw[1], xw[2], a); pnp_xc(a, C, xc);
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) M[3 * i + j] += (sg * xc[i] - ccent[i]) * (xw[j] - wcent[j]);
    }
    pnp_reduce<9, NT>(M, red);
    pnp_getrot(M, ccent, wcent, R, T);
    double P[12], e[1] = { 0 };
    pnp_proj_matrix(R, T, s.cam.f, s.cam.Cx, s.cam.Cy, P);
#pragma unroll 1
    for (int k = tid; k < n; k += NT) {
        double zc;
        pnp_point<IDX>(s, idx, k, xw, &u, &v, true);
        e[0] += pnp_reproj(P, xw, u, v, &zc);
    }
    pnp_reduce<1, NT>(e, red);
    *err = e[0] / n;
}

// efficient_pnp.m:34-175 for dimensions 1 to 3 over n points; every thread of the workgroup enters and leaves with the same answer
template <int NT, bool IDX>
__device__ __forceinline__ void pnp_body(const PnpSrc &s, const int32_t *idx, int n, PnpLds<NT> &L, PnpAns &ans)
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 9; ++i) ans.R[i] = i % 4 == 0 ? 1.0 : 0.0;
    ans.T[0] = ans.T[1] = ans.T[2] = 0; ans.err[0] = ans.err[1] = ans.err[2] = NAN; ans.best = 0; ans.sta = PNP_NONFINITE;
    double wcent[3];
    {
        double acc[PNP_MTM], sw[3] = { 0, 0, 0 };
#pragma unroll
        for (int i = 0; i < PNP_MTM; ++i) acc[i] = 0;
#pragma unroll 1
        for (int k = tid; k < n; k += NT) {
            double xw[3], a[4], u, v;
            pnp_point<IDX>(s, idx, k, xw, &u, &v, true);
            pnp_alphas(xw[0], xw[1], xw[2], a);
            pnp_mtm_point(a, s.cam.f, s.cam.Cx - u, s.cam.Cy - v, acc);
            sw[0] += xw[0]; sw[1] += xw[1]; sw[2] += xw[2];
        }
        pnp_reduce<3, NT>(sw, L.red);
        wcent[0] = sw[0] / n; wcent[1] = sw[1] / n; wcent[2] = sw[2] / n;
        // the 78 sums: the butterfly in registers, then entry t's waves joined in wave order by thread t, which leaves the sum in LDS (the full matrix is
        // built from there; 78 sums held by every thread of four waves would not fit the register file)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
#pragma unroll
            for (int i = 0; i < PNP_MTM; ++i) acc[i] += __shfl_xor(acc[i], o, 64);
        if ((tid & 63) == 0) {
#pragma unroll
            for (int i = 0; i < PNP_MTM; ++i) L.red[(tid >> 6) * PNP_MTM + i] = acc[i];
        }
    }
    __syncthreads();
    bool bad = false;
    for (int t = tid; t < PNP_MTM; t += NT) {
        double sum = L.red[t];
        for (int w = 1; w < NT / 64; ++w) sum += L.red[w * PNP_MTM + t];
        L.acc[t] = sum;
        bad = bad || !isfinite(sum);
    }
    if (__syncthreads_or(bad ? 1 : 0)) return;                          // a non-finite coordinate: sta = -1 (the workgroup leaves as one)
    for (int e = tid; e < 144; e += NT) pnp_mtm_entry(L.acc, e, L.A, L.V);
    for (int sweep = 0; ; ++sweep) {
        __syncthreads();
        if (tid == 0) L.flag = pnp_jac_done(L.A) ? 1 : 0;
        __syncthreads();
        if (L.flag != 0 || sweep >= PNP_SWEEPS) break;
        for (int r = 0; r < 11; ++r) {
            if (tid < 6) pnp_jac_angle_item(L.A, r, tid, L.cs);
            __syncthreads();
            for (int it = tid; it < 72; it += NT) pnp_jac_col_item(L.A, L.V, r, it, L.cs);
            __syncthreads();
            for (int it = tid; it < 72; it += NT) pnp_jac_row_item(L.A, r, it, L.cs);
            __syncthreads();
        }
    }
    if (tid == 0) {
        pnp_order3(L.A, L.ord);
        for (int t = 0; t < 3; ++t) pnp_fix_sign(L.V, L.ord[t]);
    }
    bool fin = true;
    int nd = 2;
    double best_err = 0;
    for (int d = 0; d < 3; ++d) {
        if (d == 2) {
            if (!(fin && pnp_enters_dim3(ans.err[0], ans.err[1]))) break;
            nd = 3;
        }
        __syncthreads();
        if (tid == 0) {
            if (d == 0) for (int i = 0; i < 12; ++i) L.X[i] = L.V[12 * i + L.ord[0]];
            else if (d == 1) pnp_dim2(L.V, L.ord, L.X);
            else pnp_dim3(L.V, L.ord, L.w6, L.X);
        }
        __syncthreads();
        double C[12], R[9], T[3], err;
#pragma unroll
        for (int i = 0; i < 12; ++i) C[i] = L.X[i];
        pnp_dim<NT, IDX>(s, idx, n, wcent, C, L.red, R, T, &err);
        if (d == 0) ans.err[0] = err; else if (d == 1) ans.err[1] = err; else ans.err[2] = err;
        fin = fin && pnp_finite(R, 9) && pnp_finite(T, 3) && isfinite(err);
        if (d == 0 || err < best_err) {                                 // the first index on ties, as pnp_answer
            best_err = err;
#pragma unroll
            for (int i = 0; i < 9; ++i) ans.R[i] = R[i];
            ans.T[0] = T[0]; ans.T[1] = T[1]; ans.T[2] = T[2];
        }
    }
    pnp_answer(ans.err, nd, fin, &ans.best, &ans.sta);
}

__device__ __forceinline__ void pnp_store(const PnpAns &a, int n, int n_support, pre3_pnp_result *res)
{
    const bool ok = a.sta == PNP_OK || a.sta == PNP_BEST_OF_THREE;      // otherwise no pose: the identity, whatever a candidate left behind
    for (int i = 0; i < 9; ++i) res->R[i] = ok ? a.R[i] : (i % 4 == 0 ? 1.0 : 0.0);
    for (int i = 0; i < 3; ++i) { res->T[i] = ok ? a.T[i] : 0.0; res->err[i] = a.err[i]; }
    if (ok) pnp_pair_u(a.R, a.T, res->u); else pnp_identity_u(res->u);
    res->best = a.best; res->sta = a.sta; res->n = n; res->n_support = n_support;
}

// idx == nullptr: the n_host points of the arrays.  Otherwise the list idx[0 .. n), n = ctl->support read on the device (ctl == nullptr: n_host); below six
// nothing is solved (sta = 0, the identity u)
template <bool IDX>
__global__ __launch_bounds__(PNP_THREADS) void k_pnp_solve(PnpSrc s, const int32_t *__restrict__ idx, const PnpCtl *__restrict__ ctl, int n_host,
                                                           pre3_pnp_result *__restrict__ res)
{
    __shared__ PnpLds<PNP_THREADS> L;
    int n = n_host;
    if (ctl != nullptr) n = ctl->support;
    if (n > s.n_all) n = s.n_all;
    PnpAns ans;
    if (n < PNP_MIN_N) {                                                // (one word for every thread)
        if (threadIdx.x == 0) {
            for (int i = 0; i < 9; ++i) ans.R[i] = i % 4 == 0 ? 1.0 : 0.0;
            ans.T[0] = ans.T[1] = ans.T[2] = 0; ans.err[0] = ans.err[1] = ans.err[2] = NAN; ans.best = 0; ans.sta = PNP_NOT_COMPUTED;
            pnp_store(ans, n < 0 ? 0 : n, n < 0 ? 0 : n, res);
        }
        return;
    }
    pnp_body<PNP_THREADS, IDX>(s, idx, n, L, ans);
    if (threadIdx.x == 0) pnp_store(ans, n, n, res);
}

// hypothesis h = blockIdx.x over draws[6 h .. 6 h + 5], then every correspondence scored under its answer; masks: `words` 64-bit words a hypothesis
template <typename CN>
__global__ __launch_bounds__(64) void k_pnp_hyp(PnpSrc s_in, const int32_t *__restrict__ draws, double thr_px, int words, unsigned long long *__restrict__ masks,
                                                int32_t *__restrict__ support, int32_t *__restrict__ state, double *__restrict__ dsum,
                                                pre3_pnp_result *__restrict__ hyp_res, CN cn)
{
    __shared__ PnpLds<64> L;
    const int h = blockIdx.x, lane = threadIdx.x;
    PnpSrc s = s_in;
    PnpAns ans;
    if constexpr (pnp_n_dev<CN>) {
        s.n_all = pnp_n(cn, s.n_all);
        if (s.n_all < PNP_MIN_N) {                                      // (one word for every lane) nothing to sample: empty masks, support 0, state 0
            for (int w = lane; w < words; w += 64) masks[(size_t)h * words + w] = 0ull;
            if (lane == 0) {
                for (int i = 0; i < 9; ++i) ans.R[i] = i % 4 == 0 ? 1.0 : 0.0;
                ans.T[0] = ans.T[1] = ans.T[2] = 0; ans.err[0] = ans.err[1] = ans.err[2] = NAN; ans.best = 0; ans.sta = PNP_NOT_COMPUTED;
                support[h] = 0; state[h] = PNP_NOT_COMPUTED; dsum[h] = 0.0;
                pnp_store(ans, 0, 0, hyp_res + h);
            }
            return;
        }
    }
    pnp_body<64, true>(s, draws + 6 * (size_t)h, 6, L, ans);
    const bool ok = ans.sta == PNP_OK || ans.sta == PNP_BEST_OF_THREE;
    double P[12];
    pnp_proj_matrix(ans.R, ans.T, s.cam.f, s.cam.Cx, s.cam.Cy, P);
    int cnt = 0;
    double ds[1] = { 0 };
    for (int w = 0; w < words; ++w) {
        const int k = w * 64 + lane;
        bool in = false;
        double dist = 0;
        if (ok && k < s.n_all) {
            double xw[3], u, v, zc;
            pnp_point<false>(s, nullptr, k, xw, &u, &v, true);
            dist = pnp_reproj(P, xw, u, v, &zc);
            in = pnp_inlier(dist, zc, thr_px);
        }
        const unsigned long long b = __ballot(in);
        if (lane == 0) masks[(size_t)h * words + w] = b;
        cnt += __popcll(b);
        ds[0] += in ? dist : 0.0;
    }
    pnp_reduce<1, 64>(ds, nullptr);
    if (lane == 0) {
        support[h] = cnt; state[h] = ok ? ans.sta : PNP_NONFINITE; dsum[h] = ds[0];
        pnp_store(ans, 6, cnt, hyp_res + h);
    }
}

constexpr int SEL_T = 256;
template <typename CN>
__global__ __launch_bounds__(SEL_T) void k_pnp_select(int n_hyp, int n_in, int words, const int32_t *__restrict__ support, const double *__restrict__ dsum,
                                                      const unsigned long long *__restrict__ masks, PnpCtl *__restrict__ ctl, int32_t *__restrict__ inl_idx,
                                                      int32_t *__restrict__ inl_flag, CN cn)
{
    __shared__ int s_s[SEL_T / 64], s_i[SEL_T / 64], s_cnt[SEL_T], s_win;
    __shared__ double s_d[SEL_T / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n = pnp_n(cn, n_in);
    if constexpr (pnp_n_dev<CN>) {
        if (n < PNP_MIN_N) {                                            // (one word for every thread) no hypothesis ran
            if (tid < n) inl_flag[tid] = 0;
            if (tid == 0) { ctl->winner = -1; ctl->support = 0; }
            return;
        }
    }
    int bs = -1, bi = 0x7fffffff;
    double bd = 0;
    for (int h = tid; h < n_hyp; h += SEL_T) {
        const int sh = support[h];
        const double dh = dsum[h];
        if (bs < 0 || pnp_better(sh, dh, h, bs, bd, bi)) { bs = sh; bd = dh; bi = h; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const int os = __shfl_xor(bs, o, 64), oi = __shfl_xor(bi, o, 64);
        const double od = __shfl_xor(bd, o, 64);
        if (os >= 0 && (bs < 0 || pnp_better(os, od, oi, bs, bd, bi))) { bs = os; bd = od; bi = oi; }
    }
    if (lane == 0) { s_s[wv] = bs; s_d[wv] = bd; s_i[wv] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < SEL_T / 64; ++w)
            if (s_s[w] >= 0 && (bs < 0 || pnp_better(s_s[w], s_d[w], s_i[w], bs, bd, bi))) { bs = s_s[w]; bd = s_d[w]; bi = s_i[w]; }
        s_win = bi;
    }
    __syncthreads();
    const int win = s_win;                                              // (n_hyp >= 1: a hypothesis was seen)
    const unsigned long long *mk = masks + (size_t)win * words;
    const int wpt = (words + SEL_T - 1) / SEL_T, w0 = tid * wpt, w1 = min(words, w0 + wpt);
    int c = 0;
    for (int w = w0; w < w1; ++w) c += __popcll(mk[w]);
    s_cnt[tid] = c;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int t = 0; t < SEL_T; ++t) { const int v = s_cnt[t]; s_cnt[t] = run; run += v; }
        ctl->winner = win; ctl->support = run;
    }
    __syncthreads();
    int o = s_cnt[tid];
    for (int w = w0; w < w1; ++w) {
        const unsigned long long b = mk[w];
        for (int j = 0; j < 64; ++j) {
            const int k = w * 64 + j;
            if (k >= n) break;
            const int in = (int)((b >> j) & 1ull);
            inl_flag[k] = in;
            if (in) { if (o < n) inl_idx[o] = k; ++o; }
        }
    }
}

template <typename CN>
__global__ __launch_bounds__(64) void k_pnp_draw(uint64_t seed, uint64_t seq, int n_hyp, int n_in, int32_t *__restrict__ draws, CN cn)
{
    const int h = blockIdx.x * 64 + threadIdx.x;
    if (h >= n_hyp) return;
    const int n = pnp_n(cn, n_in);
    int32_t r[6];
    if constexpr (pnp_n_dev<CN>) {
        if (n < PNP_MIN_N) {
#pragma unroll
            for (int j = 0; j < 6; ++j) draws[6 * (size_t)h + j] = 0;
            return;
        }
    }
    draw_rule_pnp(seed, seq, n, h, r);
#pragma unroll
    for (int j = 0; j < 6; ++j) draws[6 * (size_t)h + j] = r[j];
}

// behind a VO pair's launches: cur's pixels of the matches and the pair's inliers as an ascending list; ctl->support = 0 unless the pair is taken
constexpr int PREP_T = 256;
__global__ __launch_bounds__(PREP_T) void k_pnp_pair_prep(const VoPairHeader *__restrict__ hdr, const VoOut *__restrict__ out, int n1, const double *__restrict__ match,
                                                          const double *__restrict__ frm2, int ldf2, int K2, const int32_t *__restrict__ inl,
                                                          double *__restrict__ pix2, PnpCtl *__restrict__ ctl, int32_t *__restrict__ list)
{
    __shared__ int s_cnt[PREP_T];
    const int tid = threadIdx.x;
    int pnum = hdr->pnum;
    if (pnum > n1) pnum = n1;                                           // (the arrays hold n1 positions whatever the header says)
    const bool gathered = pnum >= 4 && hdr->bad == 0;
    const bool taken = gathered && out->dist_ok != 0 && out->sta == 1;  // (the same words for every thread)
    if (gathered)
        for (int i = tid; i < pnum; i += PREP_T) {
            const int k = (int)match[2 * (size_t)i + 1] - 1;
            const bool in = k >= 0 && k < K2;                           // (k_vp_gather has flagged anything else: a guard)
            pix2[2 * (size_t)i] = in ? frm2[(size_t)ldf2 * k] : NAN; pix2[2 * (size_t)i + 1] = in ? frm2[(size_t)ldf2 * k + 1] : NAN;
        }
    if (!taken) { if (tid == 0) { ctl->winner = -1; ctl->support = 0; } return; }
    const int per = (pnum + PREP_T - 1) / PREP_T, i0 = min(pnum, tid * per), i1 = min(pnum, i0 + per);
    int c = 0;
    for (int i = i0; i < i1; ++i) c += inl[i] != 0 ? 1 : 0;
    s_cnt[tid] = c;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int t = 0; t < PREP_T; ++t) { const int v = s_cnt[t]; s_cnt[t] = run; run += v; }
        ctl->winner = out->best; ctl->support = run;
    }
    __syncthreads();
    int o = s_cnt[tid];
    for (int i = i0; i < i1; ++i) if (inl[i] != 0) list[o++] = i;       // o <= i < n1
}

// ---- the refinement (pre3_pnpref.h) ------------------------------------------------------------------------------------------
// One pass over the points at the pose (R, T): the 28 sums in every thread, and whether every depth is positive.  The pixels are undistorted again in
// every pass (sixteen points a thread at the relocaliser's 4096): no scratch array.
template <bool IDX>
__device__ __forceinline__ bool pnpref_pass(const PnpSrc &s, const int32_t *idx, int n, const double R[9], const double T[3], double *red, double (&acc)[PNPREF_SUMS])
{
    bool front = true;
#pragma unroll
    for (int i = 0; i < PNPREF_SUMS; ++i) acc[i] = 0;
#pragma unroll 1
    for (int k = threadIdx.x; k < n; k += PNP_THREADS) {
        double xw[3], u, v;
        pnp_point<IDX>(s, idx, k, xw, &u, &v, true);
        const double z = pnpref_point(R, T, s.cam.f, s.cam.Cx, s.cam.Cy, xw, u, v, acc);
        front = front && z > 0;
    }
    pnp_reduce<PNPREF_SUMS, PNP_THREADS>(acc, red);
    return __syncthreads_and(front ? 1 : 0) != 0;
}

// The starting pose comes from a result block in device memory (the refit's, or the one pre3_pnp_refine uploads); idx, ctl and n_host as k_pnp_solve.
// Every thread holds the same sums behind pnp_reduce, so every thread solves and updates for itself (as pnp_dim's scalars) and every branch on them is
// taken by the workgroup as one.  Exactly n_iter steps.  Thread 0 writes the result; cost[k] goes out as the loop finds it (an index chosen at run time
// would put a local array into scratch).
template <bool IDX>
__global__ __launch_bounds__(PNP_THREADS) void k_pnp_refine(PnpSrc s, const int32_t *__restrict__ idx, const PnpCtl *__restrict__ ctl, int n_host,
                                                            const pre3_pnp_result *__restrict__ start, int n_iter, double sigma_px,
                                                            pre3_pnp_refine_result *__restrict__ out)
{
    __shared__ double red[(PNP_THREADS / 64) * PNPREF_SUMS];
    const int tid = threadIdx.x;
    int n = n_host;
    if (ctl != nullptr) n = ctl->support;
    if (n > s.n_all) n = s.n_all;
    if (n < 0) n = 0;
    const int sta_in = start->sta;
    double R0[9], T0[3], R[9], T[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = R0[i] = start->R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) T[i] = T0[i] = start->T[i];
    if (tid == 0) {
        for (int i = 0; i <= PNPREF_MAX_ITER; ++i) out->cost[i] = NAN;
        for (int i = 0; i < 36; ++i) out->cov6[i] = NAN;
        for (int i = 0; i < 49; ++i) out->cov[i] = NAN;
        for (int i = 0; i < 9; ++i) out->R[i] = R0[i];
        for (int i = 0; i < 3; ++i) out->T[i] = T0[i];
        for (int i = 0; i < 7; ++i) out->u[i] = start->u[i];
        out->sigma2 = NAN; out->sta = PNPREF_NOT_COMPUTED; out->n = n; out->n_iter = n_iter; out->pad = 0;
    }
    if (!(sta_in == PNP_OK || sta_in == PNP_BEST_OF_THREE) || n < PNP_MIN_N) return;        // (the same words for every thread)
    double acc[PNPREF_SUMS], cost_first = 0;
    bool fin = true;
#pragma unroll 1
    for (int k = 0; k < n_iter; ++k) {
        (void)pnpref_pass<IDX>(s, idx, n, R, T, red, acc);
        if (k == 0) cost_first = acc[27];
        if (tid == 0) out->cost[k] = acc[27];
        fin = fin && pnp_finite(acc, PNPREF_SUMS);
        fin = pnpref_step(acc, R, T) && fin;
        fin = fin && pnp_finite(R, 9) && pnp_finite(T, 3);
    }
    bool front = pnpref_pass<IDX>(s, idx, n, R, T, red, acc);
    if (n_iter == 0) cost_first = acc[27];
    if (tid == 0) out->cost[n_iter] = acc[27];
    fin = fin && pnp_finite(acc, PNPREF_SUMS);
    const bool taken = pnpref_takes(n_iter, fin, front, cost_first, acc[27]);
    if (!taken && n_iter >= 1) {                                        // the input pose is kept: the covariance is evaluated there
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = R0[i];
        T[0] = T0[0]; T[1] = T0[1]; T[2] = T0[2];
        front = pnpref_pass<IDX>(s, idx, n, R, T, red, acc);
    }
    if (tid != 0) return;
    double u[7], cov6[36], cov7[49];
    const double s2 = pnpref_sigma2(sigma_px, acc[27], n);
    pnp_pair_u(R, T, u);
    bool ok = front && pnp_finite(acc, PNPREF_SUMS) && isfinite(s2) && pnp_finite(u, 7);
    ok = ok && pnpref_cov6(acc, s2, cov6);
    ok = ok && pnpref_cov7(R, u, cov6, cov7);
    if (!ok) {                                                          // no covariance: the input's pose
        pnp_pair_u(R0, T0, u);
        for (int i = 0; i < 7; ++i) out->u[i] = u[i];
        out->sta = PNPREF_NO_COV;
        return;
    }
    for (int i = 0; i < 9; ++i) out->R[i] = R[i];
    for (int i = 0; i < 3; ++i) out->T[i] = T[i];
    for (int i = 0; i < 7; ++i) out->u[i] = u[i];
    for (int i = 0; i < 36; ++i) out->cov6[i] = cov6[i];
    for (int i = 0; i < 49; ++i) out->cov[i] = cov7[i];
    out->sigma2 = s2; out->sta = taken ? PNPREF_TAKEN : PNPREF_KEPT;
}

// ---- the host side ---------------------------------------------------------------------------------------------------------------------------------
int pnp_check(const char *who, const pre3_cam *cam, int n, const double *Xw, const double *U, const void *res)
{
    PRE3_CHECK(cam != nullptr && Xw != nullptr && U != nullptr && res != nullptr, PRE3_E_ARG, "%s: a null camera, point array, pixel array or result", who);
    PRE3_CHECK(cam->f > 0, PRE3_E_ARG, "%s: the focal length must be positive", who);
    PRE3_CHECK(n >= PNP_MIN_N && n <= PNP_MAX_N, PRE3_E_ARG, "%s: %d correspondences, %d .. %d are solved", who, n, PNP_MIN_N, PNP_MAX_N);
    return PRE3_OK;
}

PnpSrc pnp_src(const pre3_cam *cam, int undistort, int n, const double *Xw_dev, const double *U_dev)
{
    PnpSrc s;
    s.Xw = Xw_dev; s.U = U_dev; s.n_all = n; s.undistort = undistort ? 1 : 0;
    s.cam = CamD{ cam->f, cam->Cx, cam->Cy, cam->k1, cam->k2, cam->nRows, cam->nCols };
    return s;
}

// the RANSAC's block: [Xw | U | masks | out], out = [draws | support | state | dsum | ctl | list | flags | res | ref | hypothesis results] comes back in one
// copy; ref, the refinement's result, is there in the refined form alone
struct PnpRansac {
    Scratch blk; PnpSrc src; int n, n_hyp, words; double thr;
    size_t o_mask, o_out, o_draws, o_sup, o_sta, o_dsum, o_ctl, o_idx, o_flag, o_res, o_ref, o_hyp, total;
    char *d;
    template <typename T> T *at(size_t o) const { return (T *)(d + o); }
};

int pnp_ransac_fill(PnpRansac *r, const pre3_cam *cam, int undistort, int n, const double *Xw, const double *U, int n_hyp, const int32_t *draws, double thr,
                    bool refined = false)
{
    r->n = n; r->n_hyp = n_hyp; r->words = ceil_div(n, 64); r->thr = thr;
    const size_t o_xw = 0, o_u = o_xw + up16(sizeof(double) * 3 * (size_t)n), o_mask = o_u + up16(sizeof(double) * 2 * (size_t)n);
    r->o_mask = o_mask;
    r->o_out = o_mask + up16(sizeof(unsigned long long) * (size_t)n_hyp * r->words);
    r->o_draws = r->o_out; r->o_sup = r->o_draws + up16(sizeof(int32_t) * 6 * (size_t)n_hyp); r->o_sta = r->o_sup + up16(sizeof(int32_t) * (size_t)n_hyp);
    r->o_dsum = r->o_sta + up16(sizeof(int32_t) * (size_t)n_hyp); r->o_ctl = r->o_dsum + up16(sizeof(double) * (size_t)n_hyp);
    r->o_idx = r->o_ctl + up16(sizeof(PnpCtl)); r->o_flag = r->o_idx + up16(sizeof(int32_t) * (size_t)n); r->o_res = r->o_flag + up16(sizeof(int32_t) * (size_t)n);
    r->o_ref = r->o_res + up16(sizeof(pre3_pnp_result)); r->o_hyp = r->o_ref + (refined ? up16(sizeof(pre3_pnp_refine_result)) : 0); r->total = r->o_hyp + up16(sizeof(pre3_pnp_result) * (size_t)n_hyp);
    PRE3_TRY(r->blk.alloc(r->total));
    r->d = r->blk.as<char>();
    PRE3_HIP(hipMemcpy(r->d + o_xw, Xw, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice));
    PRE3_HIP(hipMemcpy(r->d + o_u, U, sizeof(double) * 2 * (size_t)n, hipMemcpyHostToDevice));
    if (draws != nullptr) PRE3_HIP(hipMemcpy(r->d + r->o_draws, draws, sizeof(int32_t) * 6 * (size_t)n_hyp, hipMemcpyHostToDevice));
    r->src = pnp_src(cam, undistort, n, (const double *)(r->d + o_xw), (const double *)(r->d + o_u));
    return PRE3_OK;
}

// [k_pnp_draw,] k_pnp_hyp, k_pnp_select, k_pnp_solve over the winner's list: on st, no wait
int pnp_ransac_launch(const PnpRansac &r, bool draw, uint64_t seed, uint64_t seq, hipStream_t st)
{
    unsigned long long *masks = r.at<unsigned long long>(r.o_mask);
    if (draw) hipLaunchKernelGGL(k_pnp_draw<PnpNHost>, dim3(ceil_div(r.n_hyp, 64)), dim3(64), 0, st, seed, seq, r.n_hyp, r.n, r.at<int32_t>(r.o_draws), PnpNHost{});
    hipLaunchKernelGGL(k_pnp_hyp<PnpNHost>, dim3(r.n_hyp), dim3(64), 0, st, r.src, (const int32_t *)r.at<int32_t>(r.o_draws), r.thr, r.words, masks, r.at<int32_t>(r.o_sup),
                       r.at<int32_t>(r.o_sta), r.at<double>(r.o_dsum), r.at<pre3_pnp_result>(r.o_hyp), PnpNHost{});
    hipLaunchKernelGGL(k_pnp_select<PnpNHost>, dim3(1), dim3(SEL_T), 0, st, r.n_hyp, r.n, r.words, (const int32_t *)r.at<int32_t>(r.o_sup), (const double *)r.at<double>(r.o_dsum),
                       (const unsigned long long *)masks, r.at<PnpCtl>(r.o_ctl), r.at<int32_t>(r.o_idx), r.at<int32_t>(r.o_flag), PnpNHost{});
    hipLaunchKernelGGL(k_pnp_solve<true>, dim3(1), dim3(PNP_THREADS), 0, st, r.src, (const int32_t *)r.at<int32_t>(r.o_idx), (const PnpCtl *)r.at<PnpCtl>(r.o_ctl), 0,
                       r.at<pre3_pnp_result>(r.o_res));
    PRE3_HIP(hipGetLastError());
    return PRE3_OK;
}

int pnp_ransac_args(const char *who, const pre3_cam *cam, int n, const double *Xw, const double *U, int n_hyp, double thr_px, const void *res)
{
    PRE3_TRY(pnp_check(who, cam, n, Xw, U, res));
    PRE3_CHECK(n_hyp >= 1 && n_hyp <= PNP_MAX_HYP, PRE3_E_ARG, "%s: %d hypotheses, 1 .. %d are evaluated", who, n_hyp, PNP_MAX_HYP);
    PRE3_CHECK(std::isfinite(thr_px) && thr_px > 0, PRE3_E_ARG, "%s: thr_px must be positive and finite", who);
    return PRE3_OK;
}

// k_pnp_refine over the winner's list, from the refit's result block: behind pnp_ransac_launch on st, no wait
int pnp_refine_launch(const PnpRansac &r, int n_iter, double sigma_px, hipStream_t st)
{
    hipLaunchKernelGGL(k_pnp_refine<true>, dim3(1), dim3(PNP_THREADS), 0, st, r.src, (const int32_t *)r.at<int32_t>(r.o_idx), (const PnpCtl *)r.at<PnpCtl>(r.o_ctl), 0,
                       (const pre3_pnp_result *)r.at<pre3_pnp_result>(r.o_res), n_iter, sigma_px, r.at<pre3_pnp_refine_result>(r.o_ref));
    PRE3_HIP(hipGetLastError());
    return PRE3_OK;
}

int pnp_refine_args(const char *who, int n_iter, double sigma_px)
{
    PRE3_CHECK(n_iter >= 0 && n_iter <= PNPREF_MAX_ITER, PRE3_E_ARG, "%s: %d iterations, 0 .. %d are run", who, n_iter, PNPREF_MAX_ITER);
    PRE3_CHECK(std::isfinite(sigma_px) && sigma_px >= 0, PRE3_E_ARG, "%s: sigma_px must be finite and not negative", who);
    return PRE3_OK;
}

// ref != nullptr: the refined form (n_iter, sigma_px), one more launch in front of the one wait
int pnp_ransac_run(const char *who, int device, const pre3_cam *cam, int undistort, int n, const double *Xw, const double *U, int n_hyp, const int32_t *draws,
                   bool seeded, uint64_t seed, uint64_t seq, double thr_px, int32_t *draws_out, int32_t *support_out, int32_t *state_out, int32_t *inlier_out,
                   pre3_pnp_result *hyp_res_out, pre3_pnp_result *res, int n_iter = 0, double sigma_px = 0, pre3_pnp_refine_result *ref = nullptr)
{
    PRE3_TRY(select_device(who, device));
    PnpRansac r;
    PRE3_TRY(pnp_ransac_fill(&r, cam, undistort, n, Xw, U, n_hyp, seeded ? nullptr : draws, thr_px, ref != nullptr));
    PRE3_TRY(pnp_ransac_launch(r, seeded, seed, seq, 0));
    if (ref != nullptr) PRE3_TRY(pnp_refine_launch(r, n_iter, sigma_px, 0));
    const size_t bytes = (hyp_res_out != nullptr ? r.total : r.o_hyp) - r.o_out;
    std::vector<char> out(bytes);
    PRE3_HIP(hipMemcpy(out.data(), r.d + r.o_out, bytes, hipMemcpyDeviceToHost));              // the one wait
    const char *o = out.data() - r.o_out;
    if (draws_out) memcpy(draws_out, o + r.o_draws, sizeof(int32_t) * 6 * (size_t)n_hyp);
    if (support_out) memcpy(support_out, o + r.o_sup, sizeof(int32_t) * (size_t)n_hyp);
    if (state_out) memcpy(state_out, o + r.o_sta, sizeof(int32_t) * (size_t)n_hyp);
    if (inlier_out) memcpy(inlier_out, o + r.o_flag, sizeof(int32_t) * (size_t)n);
    if (hyp_res_out) memcpy(hyp_res_out, o + r.o_hyp, sizeof(pre3_pnp_result) * (size_t)n_hyp);
    memcpy(res, o + r.o_res, sizeof *res);
    if (ref) memcpy(ref, o + r.o_ref, sizeof *ref);
    return PRE3_OK;
}

}  // namespace

// k_pnp_refine behind launch_pnp_ransac_dev on st, no wait: over the same list and count, from the refit's result block
int launch_pnp_refine_dev(const PnpRansacDev &r, const pre3_cam *cam, int undistort, int n_iter, double sigma_px, pre3_pnp_refine_result *ref, hipStream_t st)
{
    const PnpSrc s = pnp_src(cam, undistort, r.n_cap, r.Xw, r.U);
    hipLaunchKernelGGL(k_pnp_refine<true>, dim3(1), dim3(PNP_THREADS), 0, st, s, (const int32_t *)r.idx, (const PnpCtl *)r.ctl, 0, (const pre3_pnp_result *)r.res, n_iter,
                       sigma_px, ref);
    PRE3_HIP(hipGetLastError());
    return PRE3_OK;
}

int launch_pnp_pair(const VoPairHeader *hdr, const VoOut *out, int n1, const double *pset1, const double *match, const double *frm2, int ldf2, int K2,
                    const int32_t *inl, const pre3_cam *cam, int undistort, double *pix2, int32_t *list, pre3_pnp_result *res, hipStream_t st)
{
    PnpCtl *ctl = (PnpCtl *)list;
    int32_t *idx = list + sizeof(PnpCtl) / sizeof(int32_t);
    const PnpSrc s = pnp_src(cam, undistort, n1, pset1, pix2);
    hipLaunchKernelGGL(k_pnp_pair_prep, dim3(1), dim3(PREP_T), 0, st, hdr, out, n1, match, frm2, ldf2, K2, inl, pix2, ctl, idx);
    hipLaunchKernelGGL(k_pnp_solve<true>, dim3(1), dim3(PNP_THREADS), 0, st, s, (const int32_t *)idx, (const PnpCtl *)ctl, 0, res);
    PRE3_HIP(hipGetLastError());
    return PRE3_OK;
}

// pnp_ransac_launch's four launches with the count read on the device (pre3_pnp.h: PnpRansacDev): grid, masks and words sized by r.n_cap
int launch_pnp_ransac_dev(const PnpRansacDev &r, const pre3_cam *cam, int undistort, uint64_t seed, uint64_t seq, hipStream_t st)
{
    static_assert(sizeof(PnpCtl) == sizeof(int32_t) * PNP_CTL_WORDS, "PnpRansacDev::ctl is a PnpCtl");
    const PnpSrc s = pnp_src(cam, undistort, r.n_cap, r.Xw, r.U);
    const PnpNDev cn{ r.n_dev };
    const int words = ceil_div(r.n_cap, 64);
    PnpCtl *ctl = (PnpCtl *)r.ctl;
    hipLaunchKernelGGL(k_pnp_draw<PnpNDev>, dim3(ceil_div(r.n_hyp, 64)), dim3(64), 0, st, seed, seq, r.n_hyp, r.n_cap, r.draws, cn);
    hipLaunchKernelGGL(k_pnp_hyp<PnpNDev>, dim3(r.n_hyp), dim3(64), 0, st, s, (const int32_t *)r.draws, r.thr_px, words, r.masks, r.support, r.state, r.dsum, r.hyp, cn);
    hipLaunchKernelGGL(k_pnp_select<PnpNDev>, dim3(1), dim3(SEL_T), 0, st, r.n_hyp, r.n_cap, words, (const int32_t *)r.support, (const double *)r.dsum,
                       (const unsigned long long *)r.masks, ctl, r.idx, r.flag, cn);
    hipLaunchKernelGGL(k_pnp_solve<true>, dim3(1), dim3(PNP_THREADS), 0, st, s, (const int32_t *)r.idx, (const PnpCtl *)ctl, 0, r.res);
    PRE3_HIP(hipGetLastError());
    return PRE3_OK;
}

}  // namespace pre3

using namespace pre3;

extern "C" {

int pre3_pnp_limits(int32_t out[2])
{
    PRE3_CHECK(out != nullptr, PRE3_E_ARG, "pre3_pnp_limits: null output");
    out[0] = PNP_MAX_N; out[1] = PNP_MAX_HYP;
    return PRE3_OK;
}

int pre3_epnp(int device, const pre3_cam *cam, int undistort, int n, const double *Xw, const double *U, pre3_pnp_result *res)
{
    const char *who = "pre3_epnp";
    PRE3_TRY(pnp_check(who, cam, n, Xw, U, res));
    PRE3_TRY(select_device(who, device));
    const size_t o_u = up16(sizeof(double) * 3 * (size_t)n), o_res = o_u + up16(sizeof(double) * 2 * (size_t)n);
    Scratch blk;
    PRE3_TRY(blk.alloc(o_res + sizeof(pre3_pnp_result)));
    char *d = blk.as<char>();
    PRE3_HIP(hipMemcpy(d, Xw, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice));
    PRE3_HIP(hipMemcpy(d + o_u, U, sizeof(double) * 2 * (size_t)n, hipMemcpyHostToDevice));
    const PnpSrc s = pnp_src(cam, undistort, n, (const double *)d, (const double *)(d + o_u));
    hipLaunchKernelGGL(k_pnp_solve<false>, dim3(1), dim3(PNP_THREADS), 0, 0, s, (const int32_t *)nullptr, (const PnpCtl *)nullptr, n, (pre3_pnp_result *)(d + o_res));
    PRE3_HIP(hipGetLastError());
    PRE3_HIP(hipMemcpy(res, d + o_res, sizeof *res, hipMemcpyDeviceToHost));
    return PRE3_OK;
}

int pre3_pnp_ransac(int device, const pre3_cam *cam, int undistort, int n, const double *Xw, const double *U, int n_hyp, const int32_t *draws, double thr_px,
                    int32_t *support_out, int32_t *state_out, int32_t *inlier_out, pre3_pnp_result *hyp_res_out, pre3_pnp_result *res)
{
    const char *who = "pre3_pnp_ransac";
    PRE3_TRY(pnp_ransac_args(who, cam, n, Xw, U, n_hyp, thr_px, res));
    PRE3_CHECK(draws != nullptr, PRE3_E_ARG, "%s: null draw table", who);
    for (int h = 0; h < n_hyp; ++h)
        for (int a = 0; a < 6; ++a) {
            const int32_t v = draws[6 * (size_t)h + a];
            PRE3_CHECK(v >= 0 && v < n, PRE3_E_ARG, "%s: hypothesis %d draws index %d of %d correspondences", who, h, (int)v, n);
            for (int b = 0; b < a; ++b) PRE3_CHECK(draws[6 * (size_t)h + b] != v, PRE3_E_ARG, "%s: hypothesis %d draws index %d twice", who, h, (int)v);
        }
    return pnp_ransac_run(who, device, cam, undistort, n, Xw, U, n_hyp, draws, false, 0, 0, thr_px, nullptr, support_out, state_out, inlier_out, hyp_res_out, res);
}

int pre3_pnp_ransac_seeded(int device, const pre3_cam *cam, int undistort, int n, const double *Xw, const double *U, int n_hyp, uint64_t seed, uint64_t seq,
                           double thr_px, int32_t *draws_out, int32_t *support_out, int32_t *state_out, int32_t *inlier_out, pre3_pnp_result *hyp_res_out,
                           pre3_pnp_result *res)
{
    const char *who = "pre3_pnp_ransac_seeded";
    PRE3_TRY(pnp_ransac_args(who, cam, n, Xw, U, n_hyp, thr_px, res));
    return pnp_ransac_run(who, device, cam, undistort, n, Xw, U, n_hyp, nullptr, true, seed, seq, thr_px, draws_out, support_out, state_out, inlier_out, hyp_res_out, res);
}

int pre3_pnp_refine(int device, const pre3_cam *cam, int undistort, int n, const double *Xw, const double *U, const double *R0, const double *T0, int n_iter,
                    double sigma_px, pre3_pnp_refine_result *res)
{
    const char *who = "pre3_pnp_refine";
    PRE3_TRY(pnp_check(who, cam, n, Xw, U, res));
    PRE3_CHECK(R0 != nullptr && T0 != nullptr, PRE3_E_ARG, "%s: a null starting pose", who);
    PRE3_TRY(pnp_refine_args(who, n_iter, sigma_px));
    PRE3_TRY(select_device(who, device));
    const size_t o_u = up16(sizeof(double) * 3 * (size_t)n), o_start = o_u + up16(sizeof(double) * 2 * (size_t)n), o_res = o_start + up16(sizeof(pre3_pnp_result));
    Scratch blk;
    PRE3_TRY(blk.alloc(o_res + sizeof(pre3_pnp_refine_result)));
    char *d = blk.as<char>();
    pre3_pnp_result start;
    memset(&start, 0, sizeof start);
    memcpy(start.R, R0, sizeof start.R); memcpy(start.T, T0, sizeof start.T);
    pnp_pair_u(start.R, start.T, start.u);                              // (the kernel forms u of the pose it ends on itself: these seven are never returned)
    start.err[0] = start.err[1] = start.err[2] = NAN; start.sta = PNP_OK; start.n = n; start.n_support = n;
    PRE3_HIP(hipMemcpy(d, Xw, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice));
    PRE3_HIP(hipMemcpy(d + o_u, U, sizeof(double) * 2 * (size_t)n, hipMemcpyHostToDevice));
    PRE3_HIP(hipMemcpy(d + o_start, &start, sizeof start, hipMemcpyHostToDevice));
    const PnpSrc s = pnp_src(cam, undistort, n, (const double *)d, (const double *)(d + o_u));
    hipLaunchKernelGGL(k_pnp_refine<false>, dim3(1), dim3(PNP_THREADS), 0, 0, s, (const int32_t *)nullptr, (const PnpCtl *)nullptr, n,
                       (const pre3_pnp_result *)(d + o_start), n_iter, sigma_px, (pre3_pnp_refine_result *)(d + o_res));
    PRE3_HIP(hipGetLastError());
    PRE3_HIP(hipMemcpy(res, d + o_res, sizeof *res, hipMemcpyDeviceToHost));
    return PRE3_OK;
}

int pre3_pnp_ransac_refined_seeded(int device, const pre3_cam *cam, int undistort, int n, const double *Xw, const double *U, int n_hyp, uint64_t seed, uint64_t seq,
                                   double thr_px, int32_t *draws_out, int32_t *support_out, int32_t *state_out, int32_t *inlier_out, pre3_pnp_result *hyp_res_out,
                                   pre3_pnp_result *res, int n_iter, double sigma_px, pre3_pnp_refine_result *ref)
{
    const char *who = "pre3_pnp_ransac_refined_seeded";
    PRE3_TRY(pnp_ransac_args(who, cam, n, Xw, U, n_hyp, thr_px, res));
    PRE3_CHECK(ref != nullptr, PRE3_E_ARG, "%s: a null refinement result", who);
    PRE3_TRY(pnp_refine_args(who, n_iter, sigma_px));
    return pnp_ransac_run(who, device, cam, undistort, n, Xw, U, n_hyp, nullptr, true, seed, seq, thr_px, draws_out, support_out, state_out, inlier_out, hyp_res_out, res,
                          n_iter, sigma_px, ref);
}

int pre3_pnp_bench(int device, const pre3_cam *cam, int undistort, int n, const double *Xw, const double *U, int n_hyp, uint64_t seed, uint64_t seq, double thr_px,
                   int reps, double *ms_per_ransac_out)
{
    const char *who = "pre3_pnp_bench";
    PRE3_CHECK(reps >= 1 && ms_per_ransac_out != nullptr, PRE3_E_ARG, "%s: reps < 1 or a null output", who);
    PRE3_TRY(pnp_ransac_args(who, cam, n, Xw, U, n_hyp, thr_px, ms_per_ransac_out));
    PRE3_TRY(select_device(who, device));
    PnpRansac r;
    PRE3_TRY(pnp_ransac_fill(&r, cam, undistort, n, Xw, U, n_hyp, nullptr, thr_px));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    PRE3_HIP(hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); set_error("pre3_pnp_bench: hipEventCreate failed"); return PRE3_E_HIP; }
    float ms = 0;
    int rc = PRE3_OK;
    for (int k = 0; k < 3 && rc == PRE3_OK; ++k) rc = pnp_ransac_launch(r, true, seed, seq, 0);        // warm-up
    if (rc == PRE3_OK && hipEventRecord(e0, 0) != hipSuccess) rc = PRE3_E_HIP;
    for (int k = 0; k < reps && rc == PRE3_OK; ++k) rc = pnp_ransac_launch(r, true, seed, seq, 0);
    if (rc != PRE3_OK || hipEventRecord(e1, 0) != hipSuccess || hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess ||
        hipGetLastError() != hipSuccess) { set_error("pre3_pnp_bench: launch or event timing failed"); rc = PRE3_E_HIP; }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    PRE3_HIP(hipDeviceSynchronize());
    if (rc == PRE3_OK) *ms_per_ransac_out = ms / reps;
    return rc;
}

}  // extern "C"
