// pre3_draws.hip -- the three RANSAC draw tables and the candidates' weighted order on the device, from the counter-based stream of pre3_philox.h
// (DESIGN.md sections 18 and 19).
//   select_random_match.m:40-51   k_draw_1p     (three distinct positions in the individually compatible list, or one)
//   ransac_dr_ye.m:28-48          k_draw_vo     (four positions redrawn while they repeat or share a keypoint; capped)
//   ransac.m:142-176              k_draw_plane  (three distinct points redrawn while collinear, at most 100 attempts)
//   Weighted_Smpl_wo_replacement.m  k_cand_keys, k_cand_rank  (the exponential-race keys, then their counting rank: section 19)
// The tables: one lane per hypothesis, no LDS, nothing between workgroups.  Each kernel writes straight into the table the scoring kernel behind it on the same
// stream reads; a table crosses PCIe only when the caller asks for it back.  The rules themselves are pre3_philox.h's __host__ __device__ functions.
#include "pre3_internal.h"
#include "pre3_philox.h"
#include "pre3_vodev.h"

namespace pre3 {

namespace {

constexpr int DB = 64;          // lanes per workgroup: one wave

__global__ __launch_bounds__(DB) void k_draw_1p(uint64_t seed, uint64_t seq, int n_draw, int m, int k, int32_t *__restrict__ hyp)
{
    const int h = blockIdx.x * DB + threadIdx.x;
    if (h >= n_draw) return;
    int32_t r[3] = { 0, 0, 0 };
    draw_rule_1p(seed, seq, m, k == 3 ? 3 : 1, h, r);
    if (k == 3) { hyp[3 * (size_t)h] = r[0]; hyp[3 * (size_t)h + 1] = r[1]; hyp[3 * (size_t)h + 2] = r[2]; }
    else hyp[h] = r[0];
}

__global__ __launch_bounds__(DB) void k_draw_vo(uint64_t seed, uint64_t seq, int n_hyp, int pnum, const double *__restrict__ m1, const double *__restrict__ m2,
                                                int ms, int32_t *__restrict__ draws, int32_t *__restrict__ capped)
{
    vo_draw_lane(blockIdx.x * DB + threadIdx.x, seed, seq, n_hyp, pnum, m1, m2, ms, draws, capped);
}

__global__ __launch_bounds__(DB) void k_draw_plane(uint64_t seed, uint64_t seq, int n_draw, int npts, const double *__restrict__ pts, int32_t *__restrict__ draws,
                                                   const int32_t *__restrict__ flag /* null, or the crop's word: non-zero = a non-finite point, no draw is made */)
{
    const int h = blockIdx.x * DB + threadIdx.x;
    if (flag != nullptr && *flag != 0) return;              // (the redraw rule compares norms of the points: a NaN never satisfies it)
    if (h >= n_draw) return;
    int32_t r[3];
    draw_rule_plane(seed, seq, npts, pts, pts + npts, pts + 2 * (size_t)npts, h, r);
    draws[3 * (size_t)h] = r[0]; draws[3 * (size_t)h + 1] = r[1]; draws[3 * (size_t)h + 2] = r[2];
}

// ---- the candidates' weighted order.  raw: [K][2] pixels (| rho[K] behind them in the context form), in the caller's order
// k_real != nullptr (both kernels): K is the layout count -- the grid and the offset of rho behind the pixels -- and min(*k_real, K) candidates exist;
// work items at or beyond that count leave at once, every loop stays bounded by K.
__global__ __launch_bounds__(DB) void k_cand_keys(uint64_t seed, uint64_t seq, int K, CandBox box, const double *__restrict__ raw, double *__restrict__ keys,
                                                  const int32_t *__restrict__ k_real)
{
    const int i = blockIdx.x * DB + threadIdx.x;
    if (k_real != nullptr) K = max(0, min(*k_real, K));
    if (i >= K) return;
    keys[i] = cand_key(seed, seq, i, raw[2 * (size_t)i], raw[2 * (size_t)i + 1], box);
}

// rank_i = #{ j : (key_j, j) < (key_i, i) }, order[rank_i] = i.  A workgroup owns CR_I consecutive i (lane l of every wave holds i0 + l) and streams
// all K keys through LDS in tiles of CR_TJ; its four waves take a quarter of each tile, every lane of a wave reading the same LDS word (a broadcast:
// no bank conflict), and their partial counts meet in LDS.  No NaN reaches the comparison (cand_key), so (key, index) is a strict total order, the
// ranks are a permutation of 0 .. K-1 and every output slot has one writer: no atomics, no waiting between workgroups, bit-equal on every run.
// Whatever the keys hold, rank_i < K: no store leaves the arrays.  cand_out != nullptr (the context form): candidate i's pixel and rho go to
// position rank_i of the [K][2] | rho[K] block k_policy_prefilter and k_policy_walk read.
constexpr int CR_I = 64, CR_WAVES = 4, CR_TJ = 1024;
__global__ __launch_bounds__(CR_I * CR_WAVES) void k_cand_rank(int K, const double *__restrict__ keys, const double *__restrict__ raw, int32_t *__restrict__ order,
                                                                 double *__restrict__ cand_out, const int32_t *__restrict__ k_real, int32_t *__restrict__ order2)
{
    __shared__ double s_key[CR_TJ];
    __shared__ int s_cnt[CR_WAVES][CR_I];
    const int lane = threadIdx.x & (CR_I - 1), wv = threadIdx.x / CR_I;
    const int i = blockIdx.x * CR_I + lane;
    const int Klay = K;                                                  // where rho starts in raw and cand_out
    if (k_real != nullptr) K = max(0, min(*k_real, K));
    if ((int)blockIdx.x * CR_I >= K) return;                             // (the whole workgroup: nothing of it is ranked)
    const double ki = i < K ? keys[i] : 0.0;
    int cnt = 0;
    for (int j0 = 0; j0 < K; j0 += CR_TJ) {
        const int nj = min(CR_TJ, K - j0);
        __syncthreads();
        for (int t = threadIdx.x; t < nj; t += CR_I * CR_WAVES) s_key[t] = keys[j0 + t];
        __syncthreads();
        const int t1 = min(nj, (wv + 1) * (CR_TJ / CR_WAVES));
        for (int t = wv * (CR_TJ / CR_WAVES); t < t1; ++t) {
            const double kj = s_key[t];
            cnt += (kj < ki || (kj == ki && j0 + t < i)) ? 1 : 0;
        }
    }
    s_cnt[wv][lane] = cnt;
    __syncthreads();
    if (wv != 0 || i >= K) return;
    const int r = s_cnt[0][lane] + s_cnt[1][lane] + s_cnt[2][lane] + s_cnt[3][lane];
    order[r] = i;
    if (order2 != nullptr) order2[r] = i;
    if (cand_out != nullptr) {
        cand_out[2 * (size_t)r] = raw[2 * (size_t)i]; cand_out[2 * (size_t)r + 1] = raw[2 * (size_t)i + 1];
        cand_out[2 * (size_t)Klay + r] = raw[2 * (size_t)Klay + i];
    }
}

}  // namespace

// raw_dev: [K][2] pixels in the caller's order (cand_out_dev != nullptr: rho[K] behind them); keys_dev[K], order_dev[K] (device addresses; order_dev
// may be mapped host memory).  K >= 1, box checked by the caller.
int launch_cand_order(unsigned long long seed, unsigned long long seq, int K, int box_w, int box_h, const double *raw_dev, double *keys_dev, int32_t *order_dev,
                      double *cand_out_dev, hipStream_t st, const int32_t *k_real_dev, int32_t *order2_dev)
{
    hipLaunchKernelGGL(k_cand_keys, dim3(ceil_div(K, DB)), dim3(DB), 0, st, (uint64_t)seed, (uint64_t)seq, K, cand_box(box_w, box_h), raw_dev, keys_dev, k_real_dev);
    hipLaunchKernelGGL(k_cand_rank, dim3(ceil_div(K, CR_I)), dim3(CR_I * CR_WAVES), 0, st, K, keys_dev, raw_dev, order_dev, cand_out_dev, k_real_dev, order2_dev);
    PRE3_HIP(hipGetLastError());
    return PRE3_OK;
}

int launch_draw_1p(unsigned long long seed, unsigned long long seq, int n_draw, int m, int k, int32_t *hyp_dev, hipStream_t st)
{
    hipLaunchKernelGGL(k_draw_1p, dim3(ceil_div(n_draw, DB)), dim3(DB), 0, st, (uint64_t)seed, (uint64_t)seq, n_draw, m, k, hyp_dev);
    PRE3_HIP(hipGetLastError());
    return PRE3_OK;
}

// match rows m1 / m2 (element stride ms) and the tables in device memory; *capped_dev must be zero when the launch starts
int launch_draw_vo(unsigned long long seed, unsigned long long seq, int n_hyp, int pnum, const double *m1_dev, const double *m2_dev, int ms, int32_t *draws_dev,
                   int32_t *capped_dev, hipStream_t st)
{
    hipLaunchKernelGGL(k_draw_vo, dim3(ceil_div(n_hyp, DB)), dim3(DB), 0, st, (uint64_t)seed, (uint64_t)seq, n_hyp, pnum, m1_dev, m2_dev, ms, draws_dev, capped_dev);
    PRE3_HIP(hipGetLastError());
    return PRE3_OK;
}

// pts: [X | Y | Z] of npts cropped points, as k_plane_score reads them
int launch_draw_plane(unsigned long long seed, unsigned long long seq, int n_draw, int npts, const double *pts_dev, int32_t *draws_dev, hipStream_t st,
                      const int32_t *flag_dev)
{
    hipLaunchKernelGGL(k_draw_plane, dim3(ceil_div(n_draw, DB)), dim3(DB), 0, st, (uint64_t)seed, (uint64_t)seq, n_draw, npts, pts_dev, draws_dev, flag_dev);
    PRE3_HIP(hipGetLastError());
    return PRE3_OK;
}

}  // namespace pre3
