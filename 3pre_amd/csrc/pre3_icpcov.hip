// pre3_icpcov.hip -- k_icp_cov_part, k_icp_cov_fin: the closed-form covariance of the dense ICP's increment u = [T; q] over its final correspondences,
// two launches behind k_icp_final (the formula and its convention: pre3_icpcov.h, pre3_vocov.h).
//   aux_code/d2E_*_4cov.m, dE_*_4cov.m, Calc_derivatives_for_covariance.m, aux_code/cov_pose_shift_calc.m:24-40 over TestScripts/icp_with_init.m:76-89's pairs
// k_icp_cov_part  256 threads, workgroup w owns pairs [256 w, 256 w + 256), thread t pair 256 w + t: the pair's H_i and B_i Sigma_i B_i' (vc_add_point into
//                 zeroed sums: one pair per thread, so no accumulator outlives the pair), the lanes joined by k_vo_cov's xor butterfly, the four waves in
//                 wave order through LDS; one partial (28 + 28 doubles, count, non-finite flag) per workgroup.  The grid is sized by the layout's cap; p is
//                 read from the device, and a workgroup at or beyond ceil(p / 256) returns at once.
// k_icp_cov_fin   one workgroup: thread t sums partials t, t + 256, ... in ascending order, the same butterfly and wave-order join, then k_vo_cov's tail:
//                 every lane factors H, seven lanes solve one right-hand side each, 49 lanes symmetrise and store a VoCov block.
// The tree's shape depends on p alone, so the stateless form and the form that rides behind a run give equal bits on equal inputs.  All fp64, contraction
// off, no floating-point atomics; the hand-off between the two launches is the launch boundary.
#include <cmath>
#include <cstring>
#include <vector>

#include "pre3_internal.h"
#include "pre3_geomdev.h"
#include "pre3_icp.h"
#include "pre3_icpcov.h"

namespace pre3 {

namespace {

constexpr int IC_NW = IC_PAIRS / 64;
static_assert(IC_PAIRS == IC_FIN_THREADS, "both kernels join four waves");

// the run's state: the words earlier launches left on the device (the same for every thread), or the host's
__device__ __forceinline__ void ic_state(const IcCovArgs &a, int *sta, int *p)
{
    *sta = 1; *p = a.p;
    if (a.ctl != nullptr) { *sta = a.ctl->status; *p = a.ctl->p; }
}

// the lanes of every wave joined by the xor butterfly (every lane ends with the wave's sum), then lane 0 of every wave leaves it in LDS
__device__ __forceinline__ void ic_wave_join(double (&H)[28], double (&M)[28], int &n, int &nonfinite, double (*s_red)[56], int (*s_cnt)[2], int lane, int wv)
{
#pragma clang fp contract(off)
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int i = 0; i < 28; ++i) { H[i] += __shfl_xor(H[i], o, 64); M[i] += __shfl_xor(M[i], o, 64); }
        n += __shfl_xor(n, o, 64); nonfinite |= __shfl_xor(nonfinite, o, 64);
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 28; ++i) { s_red[wv][i] = H[i]; s_red[wv][28 + i] = M[i]; }
        s_cnt[wv][0] = n; s_cnt[wv][1] = nonfinite;
    }
    __syncthreads();
}

__global__ __launch_bounds__(IC_PAIRS) void k_icp_cov_part(IcCovArgs a, IcPart *__restrict__ part)
{
#pragma clang fp contract(off)
    int sta, p;
    ic_state(a, &sta, &p);
    if (!ic_computes(sta, p, a.cap) || (int)blockIdx.x >= ic_parts(p)) return;
    __shared__ double s_red[IC_NW][56];
    __shared__ int s_cnt[IC_NW][2];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    double X[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) X[i] = a.u_dev != nullptr ? a.u_dev[i] : a.u.v[i];
    double H[28], M[28];
#pragma unroll
    for (int i = 0; i < 28; ++i) { H[i] = 0; M[i] = 0; }
    int n = 0, nonfinite = 0;
    const int k = blockIdx.x * IC_PAIRS + tid;
    if (k < p) {
        n = 1;
        const int im = a.corr_m[k], is = a.corr_s[k];
        // (the ICP's launches write indices below n1, n2 and pixels of the frame, and the host checks a caller's list: a guard, not a path)
        bool in = (unsigned)im < (unsigned)a.cap1 && (unsigned)is < (unsigned)a.cap2;
        int js = is;
        if (in && a.spix != nullptr) { js = a.spix[is]; in = (unsigned)js < (unsigned)a.npix; }
        if (!in) nonfinite = 1;
        else {
            const double fp[3] = { a.mx[im], a.my[im], a.mz[im] };
            const double sx = a.sx[js], sy = a.sy[js], sz = a.sz[js];
            const double fn[3] = { a.spix != nullptr ? -sx : sx, a.spix != nullptr ? -sy : sy, sz };      // ransac_dr_ye.m:17-18: the frames forms' camera frame
            if (!vc_add_point(fp, fn, X, H, M)) nonfinite = 1;
        }
    }
    ic_wave_join(H, M, n, nonfinite, s_red, s_cnt, lane, wv);
    IcPart &o = part[blockIdx.x];
    if (tid < 56) {                                                               // the four waves in wave order
        double s = s_red[0][tid];
#pragma unroll
        for (int w = 1; w < IC_NW; ++w) s += s_red[w][tid];
        if (tid < 28) o.H[tid] = s; else o.M[tid - 28] = s;
    }
    if (tid == 64) {
        int c = 0, f = 0;
#pragma unroll
        for (int w = 0; w < IC_NW; ++w) { c += s_cnt[w][0]; f |= s_cnt[w][1]; }
        o.n = c; o.nonfinite = f;
    }
}

__global__ __launch_bounds__(IC_FIN_THREADS) void k_icp_cov_fin(IcCovArgs a, const IcPart *__restrict__ part, VoCov *__restrict__ cov)
{
#pragma clang fp contract(off)
    __shared__ double s_red[IC_NW][56];
    __shared__ int s_cnt[IC_NW][2];
    __shared__ double sA[49], sB[49];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int sta, p;
    ic_state(a, &sta, &p);
    if (!ic_computes(sta, p, a.cap)) {                                            // (the same words for every thread: the workgroup leaves as one)
        if (tid == 0) { cov->status = VC_NOT_COMPUTED; cov->n_inliers = 0; }
        return;
    }
    const int nparts = ic_parts(p);
    double H[28], M[28];
#pragma unroll
    for (int i = 0; i < 28; ++i) { H[i] = 0; M[i] = 0; }
    int n = 0, nonfinite = 0;
    for (int q = tid; q < nparts; q += IC_FIN_THREADS) {
        const IcPart &pt = part[q];
#pragma unroll
        for (int i = 0; i < 28; ++i) { H[i] += pt.H[i]; M[i] += pt.M[i]; }
        n += pt.n; nonfinite |= pt.nonfinite;
    }
    ic_wave_join(H, M, n, nonfinite, s_red, s_cnt, lane, wv);
#pragma unroll
    for (int i = 0; i < 28; ++i) {
        double h = s_red[0][i], m = s_red[0][28 + i];
#pragma unroll
        for (int w = 1; w < IC_NW; ++w) { h += s_red[w][i]; m += s_red[w][28 + i]; }
        H[i] = h; M[i] = m;
    }
    n = 0; nonfinite = 0;
#pragma unroll
    for (int w = 0; w < IC_NW; ++w) { n += s_cnt[w][0]; nonfinite |= s_cnt[w][1]; }
    // k_vo_cov's tail (pre3_vocov.hip), with the thread index for its lane: the threads beyond 49 factor H like the rest and store nothing
    double L[28];
    const bool ok = vc_chol7(H, L) && nonfinite == 0;
    if (tid == 0) {
#pragma unroll
        for (int r = 0; r < 7; ++r)
#pragma unroll
            for (int c = 0; c <= r; ++c) { sA[7 * r + c] = M[vc_ix(r, c)]; sA[7 * c + r] = M[vc_ix(r, c)]; }
    }
    __syncthreads();
    double x[7];
    if (tid < 7) {                                                                // column `tid` of H^-1 M
#pragma unroll
        for (int i = 0; i < 7; ++i) x[i] = sA[7 * i + tid];
        vc_solve7(L, x);
#pragma unroll
        for (int i = 0; i < 7; ++i) sB[7 * i + tid] = x[i];
    }
    __syncthreads();
    if (tid < 7) {                                                                // row `tid` of (H^-1 M) H^-1
#pragma unroll
        for (int j = 0; j < 7; ++j) x[j] = sB[7 * tid + j];
        vc_solve7(L, x);
#pragma unroll
        for (int j = 0; j < 7; ++j) sA[7 * tid + j] = x[j];                       // (sA was last read in front of the barrier above)
    }
    __syncthreads();
    double v = 0;
    if (tid < 49) { const int i = tid / 7, j = tid % 7; v = (sA[7 * i + j] + sA[7 * j + i]) / 2; }
    const bool fin = __ballot(tid < 49 && !isfinite(v)) == 0ull;                  // (tid < 49 lies in the first wave, which alone stores)
    if (ok && fin && tid < 49) cov->cov[tid] = v;
    if (tid == 0) { cov->status = ok && fin ? VC_VALID : VC_UNUSABLE; cov->n_inliers = n; }
}

}  // namespace

int launch_icp_cov(const IcCovArgs &a, IcPart *part, VoCov *cov, hipStream_t st)
{
    hipLaunchKernelGGL(k_icp_cov_part, dim3(ic_parts(a.cap)), dim3(IC_PAIRS), 0, st, a, part);
    hipLaunchKernelGGL(k_icp_cov_fin, dim3(1), dim3(IC_FIN_THREADS), 0, st, a, (const IcPart *)part, cov);
    PRE3_HIP(hipGetLastError());
    return PRE3_OK;
}

}  // namespace pre3

using namespace pre3;

namespace {

// what both stateless entries refuse before a device is touched
int ic_check_args(const char *who, const double *data1, int n1, const double *data2, int n2, const int32_t *corr, int p, const double *u)
{
    PRE3_CHECK(data1 != nullptr && data2 != nullptr && n1 >= 1 && n2 >= 1 && u != nullptr && p >= 0 && (p == 0 || corr != nullptr), PRE3_E_ARG,
               "%s: a null cloud or u, an empty cloud, a negative p, or a null list", who);
    PRE3_CHECK(p <= IC_MAX_P, PRE3_E_ARG, "%s: %d pairs, at most %d", who, p, IC_MAX_P);
    for (int k = 0; k < p; ++k)
        PRE3_CHECK(corr[2 * (size_t)k] >= 1 && corr[2 * (size_t)k] <= n1 && corr[2 * (size_t)k + 1] >= 1 && corr[2 * (size_t)k + 1] <= n2, PRE3_E_ARG,
                   "%s: pair %d is (%d, %d), the clouds hold %d and %d points", who, k + 1, (int)corr[2 * (size_t)k], (int)corr[2 * (size_t)k + 1], n1, n2);
    return PRE3_OK;
}

// the stateless forms' block: [model x y z | source x y z | corr_m | corr_s | VoCov | partials], filled from a host image of its front
struct IcStateless { Scratch blk; IcCovArgs a; IcPart *part; VoCov *cov; };
int ic_stateless_fill(IcStateless *s, const double *data1, int n1, const double *data2, int n2, const int32_t *corr, int p, const double *u)
{
    const size_t o_m = 0, o_s = o_m + up16(sizeof(double) * 3 * (size_t)n1), o_cm = o_s + up16(sizeof(double) * 3 * (size_t)n2);
    const size_t o_cs = o_cm + up16(sizeof(int32_t) * (size_t)p), o_cov = o_cs + up16(sizeof(int32_t) * (size_t)p), o_part = o_cov + up16(sizeof(VoCov));
    const size_t total = o_part + ic_part_bytes(p);
    std::vector<char> img(o_cov);
    double *hm = (double *)(img.data() + o_m), *hs = (double *)(img.data() + o_s);
    int32_t *hcm = (int32_t *)(img.data() + o_cm), *hcs = (int32_t *)(img.data() + o_cs);
    for (int i = 0; i < n1; ++i) { hm[i] = data1[3 * (size_t)i]; hm[n1 + i] = data1[3 * (size_t)i + 1]; hm[2 * (size_t)n1 + i] = data1[3 * (size_t)i + 2]; }
    for (int j = 0; j < n2; ++j) { hs[j] = data2[3 * (size_t)j]; hs[n2 + j] = data2[3 * (size_t)j + 1]; hs[2 * (size_t)n2 + j] = data2[3 * (size_t)j + 2]; }
    for (int k = 0; k < p; ++k) { hcm[k] = corr[2 * (size_t)k] - 1; hcs[k] = corr[2 * (size_t)k + 1] - 1; }
    PRE3_TRY(s->blk.alloc(total));
    char *d = s->blk.as<char>();
    PRE3_HIP(hipMemcpy(d, img.data(), o_cov, hipMemcpyHostToDevice));
    PRE3_HIP(hipMemset(d + o_cov, 0, sizeof(VoCov)));
    IcCovArgs &a = s->a;
    a = IcCovArgs{};
    a.ctl = nullptr; a.u_dev = nullptr; a.p = p; a.cap = p; a.cap1 = n1; a.cap2 = n2; a.npix = 0;
    for (int i = 0; i < 7; ++i) a.u.v[i] = u[i];
    a.corr_m = (const int32_t *)(d + o_cm); a.corr_s = (const int32_t *)(d + o_cs);
    a.mx = (const double *)(d + o_m); a.my = a.mx + n1; a.mz = a.my + n1;
    a.sx = (const double *)(d + o_s); a.sy = a.sx + n2; a.sz = a.sy + n2;
    a.spix = nullptr;
    s->part = (IcPart *)(d + o_part); s->cov = (VoCov *)(d + o_cov);
    return PRE3_OK;
}

}  // namespace

extern "C" {

int pre3_icp_cov_limits(int32_t out[2])
{
    PRE3_CHECK(out != nullptr, PRE3_E_ARG, "pre3_icp_cov_limits: null output");
    out[0] = IC_PAIRS; out[1] = IC_FIN_PER_THREAD;
    return PRE3_OK;
}

int pre3_icp_cov(int device, const double *data1, int n1, const double *data2, int n2, const int32_t *corr, int p, const double u[7], double *cov_out,
                 int32_t *status_out, int32_t *n_out)
{
    const char *who = "pre3_icp_cov";
    PRE3_CHECK(status_out != nullptr, PRE3_E_ARG, "%s: null status_out", who);
    PRE3_TRY(ic_check_args(who, data1, n1, data2, n2, corr, p, u));
    PRE3_TRY(select_device(who, device));
    *status_out = VC_NOT_COMPUTED;
    if (n_out) *n_out = 0;
    if (p < 4) return PRE3_OK;                          // seven unknowns: as pre3_vo_cov, nothing to propagate
    IcStateless s;
    PRE3_TRY(ic_stateless_fill(&s, data1, n1, data2, n2, corr, p, u));
    PRE3_TRY(launch_icp_cov(s.a, s.part, s.cov, 0));
    VoCov o;
    PRE3_HIP(hipMemcpy(&o, s.cov, sizeof o, hipMemcpyDeviceToHost));
    *status_out = o.status;
    if (n_out) *n_out = o.n_inliers;
    if (o.status == VC_VALID && cov_out) memcpy(cov_out, o.cov, sizeof o.cov);
    return PRE3_OK;
}

int pre3_icp_cov_bench(int device, const double *data1, int n1, const double *data2, int n2, const int32_t *corr, int p, const double u[7], int reps,
                       double *ms_per_pair_of_launches_out)
{
    const char *who = "pre3_icp_cov_bench";
    PRE3_CHECK(reps >= 1 && ms_per_pair_of_launches_out != nullptr && p >= 4, PRE3_E_ARG, "%s: reps < 1, fewer than four pairs, or a null output", who);
    PRE3_TRY(ic_check_args(who, data1, n1, data2, n2, corr, p, u));
    PRE3_TRY(select_device(who, device));
    IcStateless s;
    PRE3_TRY(ic_stateless_fill(&s, data1, n1, data2, n2, corr, p, u));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    PRE3_HIP(hipEventCreate(&e0)); PRE3_HIP(hipEventCreate(&e1));
    float ms = 0;
    int rc = PRE3_OK;
    for (int r = 0; r < 3 && rc == PRE3_OK; ++r) rc = launch_icp_cov(s.a, s.part, s.cov, 0);        // warm-up
    if (rc == PRE3_OK && hipEventRecord(e0, 0) != hipSuccess) rc = PRE3_E_HIP;
    for (int r = 0; r < reps && rc == PRE3_OK; ++r) rc = launch_icp_cov(s.a, s.part, s.cov, 0);
    if (rc != PRE3_OK || hipEventRecord(e1, 0) != hipSuccess || hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess ||
        hipGetLastError() != hipSuccess) { set_error("pre3_icp_cov_bench: launch or event timing failed"); rc = PRE3_E_HIP; }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    PRE3_HIP(hipDeviceSynchronize());
    *ms_per_pair_of_launches_out = ms / reps;
    return rc;
}

}  // extern "C"
