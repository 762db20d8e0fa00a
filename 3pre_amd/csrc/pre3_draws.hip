// pre3_draws.hip -- the three RANSAC draw tables on the device, from the counter-based stream of pre3_philox.h.
//   select_random_match.m:40-51   k_draw_1p     (three distinct positions in the individually compatible list, or one)
//   ransac_dr_ye.m:28-48          k_draw_vo     (four positions redrawn while they repeat or share a keypoint; capped)
//   ransac.m:142-176              k_draw_plane  (three distinct points redrawn while collinear, at most 100 attempts)
// One lane per hypothesis, no LDS, nothing between workgroups.  Each kernel writes straight into the table the scoring kernel behind it on the same
// stream reads; a table crosses PCIe only when the caller asks for it back.  The rules themselves are pre3_philox.h's __host__ __device__ functions.
#include "pre3_internal.h"
#include "pre3_philox.h"

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
    const int h = blockIdx.x * DB + threadIdx.x;
    int cap = 0;
    if (h < n_hyp) {
        int32_t r[4];
        cap = draw_rule_vo(seed, seq, pnum, m1, m2, ms, h, r);
        *reinterpret_cast<int4 *>(draws + 4 * (size_t)h) = make_int4(r[0], r[1], r[2], r[3]);
    }
    const int n = __popcll(__ballot(cap != 0));         // (every lane of the wave reaches the ballot)
    if (threadIdx.x == 0 && n) atomicAdd(capped, n);
}

__global__ __launch_bounds__(DB) void k_draw_plane(uint64_t seed, uint64_t seq, int n_draw, int npts, const double *__restrict__ pts, int32_t *__restrict__ draws)
{
    const int h = blockIdx.x * DB + threadIdx.x;
    if (h >= n_draw) return;
    int32_t r[3];
    draw_rule_plane(seed, seq, npts, pts, pts + npts, pts + 2 * (size_t)npts, h, r);
    draws[3 * (size_t)h] = r[0]; draws[3 * (size_t)h + 1] = r[1]; draws[3 * (size_t)h + 2] = r[2];
}

}  // namespace

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
int launch_draw_plane(unsigned long long seed, unsigned long long seq, int n_draw, int npts, const double *pts_dev, int32_t *draws_dev, hipStream_t st)
{
    hipLaunchKernelGGL(k_draw_plane, dim3(ceil_div(n_draw, DB)), dim3(DB), 0, st, (uint64_t)seed, (uint64_t)seq, n_draw, npts, pts_dev, draws_dev);
    PRE3_HIP(hipGetLastError());
    return PRE3_OK;
}

}  // namespace pre3
