// pre3_vocov.hip -- k_vo_cov: the covariance of a VO pair's increment u = [T; q] from its inliers, one launch behind k_vo_final.
//   aux_code/calc_cov_RANSAC_dr_ye.m:17-30, aux_code/cov_pose_shift_calc.m:4-40 -- the Pn predict_state_and_covariance.m:115 leaves commented out
// One wave.  The inliers are lane-strided in increasing index; every lane adds its points' H_i and B_i Sigma_i B_i' into 28 + 28 fp64 sums (the packed
// lower triangles of H and M, pre3_vocov.h), and the lanes are joined by the xor butterfly vo_final_wave uses: a fixed order, no float atomics, every
// lane ends with the same bits.  Each lane then factors H for itself (uniform control flow, no broadcast); lanes 0..6 solve one right-hand side each
// -- a column of H^-1 M, then a row of (H^-1 M) H^-1 -- through LDS, and 49 lanes symmetrise and store.  Results are bit-equal from run to run.
// What bounds one wave: a pair has at most n1 <= PRE3_SR_MAX_KEYPOINTS (8192) matches, a lane visits ceil(pnum / 64) <= 128 of them, and a point
// costs ~1.5 kflop and four sin / cos / atan2 pairs; the reference's scenes give 20 - 300 matches, where the launch floor dominates.
#include "pre3_internal.h"
#include "pre3_geomdev.h"
#include "pre3_vodev.h"
#include "pre3_vopair.h"
#include "pre3_vocov.h"

namespace pre3 {

// where pnum, the solution state and u come from: the header and result block a pair's launches left on the device (hdr != null), or the host (sta = 1)
struct VcSrc { const VoPairHeader *hdr; const VoOut *out; int pnum, cap; U7 u; };

// inl: one int32 per match position, as k_vo_final leaves them (null: every point is an inlier).  pset1, pset2, inl hold at least s.cap positions.
__global__ __launch_bounds__(64) void k_vo_cov(VcSrc s, const double *__restrict__ pset1, const double *__restrict__ pset2,
                                               const int32_t *__restrict__ inl, VoCov *__restrict__ cov)
{
#pragma clang fp contract(off)
    __shared__ double sA[49], sB[49];
    const int lane = threadIdx.x;
    int pnum = s.pnum, sta = 1, bad = 0, dist_ok = 1;
    double X[7];
    if (s.hdr != nullptr) {
        pnum = s.hdr->pnum; bad = s.hdr->bad; sta = s.out->sta; dist_ok = s.out->dist_ok;
#pragma unroll
        for (int i = 0; i < 7; ++i) X[i] = s.out->u[i];
    } else {
#pragma unroll
        for (int i = 0; i < 7; ++i) X[i] = s.u.v[i];
    }
    if (!vc_pair_computes(sta, pnum, bad, dist_ok) || pnum > s.cap) {            // (the same words for every lane: the wave leaves as one)
        if (lane == 0) { cov->status = VC_NOT_COMPUTED; cov->n_inliers = 0; }
        return;
    }
    double H[28], M[28];
#pragma unroll
    for (int i = 0; i < 28; ++i) { H[i] = 0; M[i] = 0; }
    int n = 0, nonfinite = 0;
    for (int k = lane; k < pnum; k += 64)
        if (inl == nullptr || inl[k] != 0) {
            ++n;
            if (!vc_add_point(pset1 + 3 * (size_t)k, pset2 + 3 * (size_t)k, X, H, M)) nonfinite = 1;
        }
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int i = 0; i < 28; ++i) { H[i] += __shfl_xor(H[i], o, 64); M[i] += __shfl_xor(M[i], o, 64); }
        n += __shfl_xor(n, o, 64); nonfinite |= __shfl_xor(nonfinite, o, 64);
    }
    double L[28];
    const bool ok = vc_chol7(H, L) && nonfinite == 0;
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 7; ++a)
#pragma unroll
            for (int b = 0; b <= a; ++b) { sA[7 * a + b] = M[vc_ix(a, b)]; sA[7 * b + a] = M[vc_ix(a, b)]; }
    }
    __syncthreads();
    double x[7];
    if (lane < 7) {                                                               // column `lane` of H^-1 M
#pragma unroll
        for (int i = 0; i < 7; ++i) x[i] = sA[7 * i + lane];
        vc_solve7(L, x);
#pragma unroll
        for (int i = 0; i < 7; ++i) sB[7 * i + lane] = x[i];
    }
    __syncthreads();
    if (lane < 7) {                                                               // row `lane` of (H^-1 M) H^-1
#pragma unroll
        for (int j = 0; j < 7; ++j) x[j] = sB[7 * lane + j];
        vc_solve7(L, x);
#pragma unroll
        for (int j = 0; j < 7; ++j) sA[7 * lane + j] = x[j];                      // (sA was last read in front of the barrier above)
    }
    __syncthreads();
    double v = 0;
    if (lane < 49) { const int i = lane / 7, j = lane % 7; v = (sA[7 * i + j] + sA[7 * j + i]) / 2; }
    const bool fin = __ballot(lane < 49 && !isfinite(v)) == 0ull;
    if (ok && fin && lane < 49) cov->cov[lane] = v;
    if (lane == 0) { cov->status = ok && fin ? VC_VALID : VC_UNUSABLE; cov->n_inliers = n; }
}

int launch_vo_cov_pair(const VoPairHeader *hdr, const VoOut *out, int cap, const double *pset1, const double *pset2, const int32_t *inl, VoCov *cov, hipStream_t st)
{
    const VcSrc s{ hdr, out, 0, cap, U7{} };
    hipLaunchKernelGGL(k_vo_cov, dim3(1), dim3(64), 0, st, s, pset1, pset2, inl, cov);
    PRE3_HIP(hipGetLastError());
    return PRE3_OK;
}

}  // namespace pre3

using namespace pre3;

extern "C" {

int pre3_vo_cov(int device, int pnum, const double *pset1, const double *pset2, const int32_t *inlier, const double u[7], double *cov_out,
                int32_t *status_out, int32_t *n_inliers_out)
{
    PRE3_TRY(select_device("pre3_vo_cov", device));
    PRE3_CHECK(pnum >= 0 && u != nullptr && status_out != nullptr && (pnum == 0 || (pset1 != nullptr && pset2 != nullptr)), PRE3_E_ARG,
               "pre3_vo_cov: a negative pnum, or a null point set, u or status_out");
    *status_out = VC_NOT_COMPUTED;
    if (n_inliers_out) *n_inliers_out = 0;
    if (pnum < 4) return PRE3_OK;                       // ransac_dr_ye.m:5-11: no fit, so nothing to propagate
    const size_t pb = sizeof(double) * 3 * (size_t)pnum;
    Scratch p1, p2, in, cv;
    PRE3_TRY(p1.alloc(pb)); PRE3_TRY(p2.alloc(pb)); PRE3_TRY(cv.alloc(sizeof(VoCov)));
    PRE3_HIP(hipMemcpy(p1.p, pset1, pb, hipMemcpyHostToDevice));
    PRE3_HIP(hipMemcpy(p2.p, pset2, pb, hipMemcpyHostToDevice));
    if (inlier) { PRE3_TRY(in.alloc(sizeof(int32_t) * (size_t)pnum)); PRE3_HIP(hipMemcpy(in.p, inlier, sizeof(int32_t) * (size_t)pnum, hipMemcpyHostToDevice)); }
    PRE3_HIP(hipMemset(cv.p, 0, sizeof(VoCov)));
    VcSrc s{ nullptr, nullptr, pnum, pnum, U7{} };
    for (int i = 0; i < 7; ++i) s.u.v[i] = u[i];
    hipLaunchKernelGGL(k_vo_cov, dim3(1), dim3(64), 0, 0, s, p1.as<double>(), p2.as<double>(), inlier ? in.as<int32_t>() : (const int32_t *)nullptr, cv.as<VoCov>());
    PRE3_HIP(hipGetLastError());
    VoCov o;
    PRE3_HIP(hipMemcpy(&o, cv.p, sizeof o, hipMemcpyDeviceToHost));
    *status_out = o.status;
    if (n_inliers_out) *n_inliers_out = o.n_inliers;
    if (o.status == VC_VALID && cov_out) memcpy(cov_out, o.cov, sizeof o.cov);
    return PRE3_OK;
}

}  // extern "C"
