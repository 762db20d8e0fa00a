// pre3_vo.hip -- SURVEY 8(f)-4: the visual-odometry front end's 4-point 3D-3D RANSAC on the device.
//   vodometry_dr_ye.m:162-236  (adaptive count, winner, final fit, error statistics)
//   ransac_dr_ye.m:13-23,48-72 (point gathering from the range images, inlier radius, per-hypothesis support)
//   find_transform_matrix_dr_ye.m:8-41 (centroids, H = sum q2 q1', svd, V U', reflection handling)
//   R2e.m:21-23, R2q.m, Calculate_V_Omega_RANSAC_dr_ye.m:40-50 (Euler angles and the u = [T; q] the predict kernel consumes)
// One workgroup (one wave) per hypothesis: every lane solves the same 3x3 SVD (uniform control flow, no broadcast),
// then the lanes stride over the matched points; ballots give the inlier bit mask and the support.  All fp64, no
// contraction (the inlier test is a discontinuity; keep the operation order of the reference's loops).
#include <algorithm>
#include <vector>

#include "pre3_internal.h"
#include "pre3_vodev.h"

namespace pre3 {

// ransac_dr_ye.m:13-19 for one frame
__global__ void k_vo_gather(int rows, int cols, const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ z,
                            int ldf, const double *__restrict__ frm, int K, int pnum, const double *__restrict__ sel, int sel_stride,
                            double *__restrict__ pset, int32_t *__restrict__ bad)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= pnum) return;
    vo_gather_one(i, rows, cols, x, y, z, ldf, frm, K, sel, sel_stride, pset, bad);
}

// ransac_dr_ye.m:20-23 -- one wave
__global__ void k_vo_dist(int pnum, const double *__restrict__ pset2, VoOut *__restrict__ out)
{
    vo_dist_wave(pnum, pset2, out);
}

// ransac_dr_ye.m:48-72 for hypothesis blockIdx.x
__global__ __launch_bounds__(64) void k_vo_score(int pnum, const double *__restrict__ pset1, const double *__restrict__ pset2,
                                                 const int32_t *__restrict__ draws, const VoOut *__restrict__ out, int words,
                                                 unsigned long long *__restrict__ masks, int32_t *__restrict__ cnum, int32_t *__restrict__ state)
{
    vo_score_hyp(blockIdx.x, pnum, pset1, pset2, draws, out, words, masks, cnum, state);
}

// vodometry_dr_ye.m:185-236 -- one wave
__global__ void k_vo_final(int pnum, int n_hyp, const double *__restrict__ pset1, const double *__restrict__ pset2,
                           const int32_t *__restrict__ cnum, int words, const unsigned long long *__restrict__ masks,
                           VoOut *__restrict__ out, int32_t *__restrict__ inl_out)
{
    vo_final_wave(pnum, n_hyp, pset1, pset2, cnum, words, masks, out, inl_out);
}


// the seeded forms: the draws come from k_draw_vo, which reads the match list (2 x pnum doubles, column-major) on the device
struct VoSeed { unsigned long long seed, seq; const double *match_dev; int32_t *draws_out, *capped_out; };

static int vo_run(int pnum, const double *d_p1, const double *d_p2, int n_hyp, const int32_t *draws, int32_t *cnum_out, int32_t *state_out,
                  int32_t *inlier_out, pre3_vo_result *res, int reps, double *ms_out, const VoSeed *sd = nullptr)
{
    const int words = ceil_div(pnum, 64);
    Scratch dd, dm, dc, ds, dout, dinl, dcap;
    PRE3_TRY(dd.alloc(sizeof(int32_t) * 4 * (size_t)n_hyp)); PRE3_TRY(dm.alloc(sizeof(unsigned long long) * (size_t)n_hyp * words));
    PRE3_TRY(dc.alloc(sizeof(int32_t) * n_hyp)); PRE3_TRY(ds.alloc(sizeof(int32_t) * n_hyp)); PRE3_TRY(dout.alloc(sizeof(VoOut)));
    PRE3_TRY(dinl.alloc(sizeof(int32_t) * pnum));
    if (sd) {
        PRE3_TRY(dcap.alloc(sizeof(int32_t)));
        PRE3_HIP(hipMemsetAsync(dcap.p, 0, sizeof(int32_t), 0));
        PRE3_TRY(launch_draw_vo(sd->seed, sd->seq, n_hyp, pnum, sd->match_dev, sd->match_dev + 1, 2, dd.as<int32_t>(), dcap.as<int32_t>(), 0));
    } else
    PRE3_HIP(hipMemcpy(dd.p, draws, sizeof(int32_t) * 4 * (size_t)n_hyp, hipMemcpyHostToDevice));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (ms_out) { PRE3_HIP(hipEventCreate(&e0)); PRE3_HIP(hipEventCreate(&e1)); PRE3_HIP(hipEventRecord(e0, 0)); }
    for (int r = 0; r < reps; ++r) {
        hipLaunchKernelGGL(k_vo_dist, dim3(1), dim3(64), 0, 0, pnum, d_p2, dout.as<VoOut>());
        hipLaunchKernelGGL(k_vo_score, dim3(n_hyp), dim3(64), 0, 0, pnum, d_p1, d_p2, dd.as<int32_t>(), dout.as<VoOut>(), words,
                           dm.as<unsigned long long>(), dc.as<int32_t>(), ds.as<int32_t>());
        hipLaunchKernelGGL(k_vo_final, dim3(1), dim3(64), 0, 0, pnum, n_hyp, d_p1, d_p2, dc.as<int32_t>(), words, dm.as<unsigned long long>(),
                           dout.as<VoOut>(), dinl.as<int32_t>());
    }
    int rc = PRE3_OK;
    if (hipGetLastError() != hipSuccess) { set_error("vo: kernel launch failed"); rc = PRE3_E_HIP; }
    if (ms_out && rc == PRE3_OK) {
        float ms = 0;
        if (hipEventRecord(e1, 0) != hipSuccess || hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) { set_error("vo: event timing failed"); rc = PRE3_E_HIP; }
        *ms_out = ms / reps;
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    PRE3_TRY(rc);
    PRE3_HIP(hipDeviceSynchronize());
    VoOut o;
    PRE3_HIP(hipMemcpy(&o, dout.p, sizeof o, hipMemcpyDeviceToHost));
    if (sd && sd->draws_out) PRE3_HIP(hipMemcpy(sd->draws_out, dd.p, sizeof(int32_t) * 4 * (size_t)n_hyp, hipMemcpyDeviceToHost));
    if (sd && sd->capped_out) PRE3_HIP(hipMemcpy(sd->capped_out, dcap.p, sizeof(int32_t), hipMemcpyDeviceToHost));
    PRE3_CHECK(o.dist_ok, PRE3_E_NUMERIC, "vo: no matched point is farther than 0.4 m from the camera (ransac_dr_ye.m:21 has no minimum there)");
    if (cnum_out) PRE3_HIP(hipMemcpy(cnum_out, dc.p, sizeof(int32_t) * n_hyp, hipMemcpyDeviceToHost));
    if (state_out) PRE3_HIP(hipMemcpy(state_out, ds.p, sizeof(int32_t) * n_hyp, hipMemcpyDeviceToHost));
    if (inlier_out) PRE3_HIP(hipMemcpy(inlier_out, dinl.p, sizeof(int32_t) * pnum, hipMemcpyDeviceToHost));
    if (res) vo_result(o, res);
    return PRE3_OK;
}

static int vo_check(int device, int pnum, int n_hyp, const int32_t *draws, bool seeded = false)
{
    PRE3_TRY(select_device("vo", device));
    PRE3_CHECK(pnum >= 4, PRE3_E_ARG, "vo: number of points is smaller than 4: insufficient for ransac");      // ransac_dr_ye.m:5-11
    PRE3_CHECK(n_hyp >= 1 && (draws || seeded), PRE3_E_ARG, "vo: no hypotheses");
    for (int i = 0; !seeded && i < 4 * n_hyp; ++i) PRE3_CHECK(draws[i] >= 0 && draws[i] < pnum, PRE3_E_ARG, "vo: draws[%d]=%d is not a match position (pnum=%d)", i, draws[i], pnum);
    return PRE3_OK;
}

}  // namespace pre3

using namespace pre3;

extern "C" {

int pre3_vo_ransac(int device, int pnum, const double *pset1, const double *pset2, int n_hyp, const int32_t *draws, int32_t *cnum_out,
                   int32_t *state_out, int32_t *inlier_out, pre3_vo_result *res)
{
    PRE3_TRY(vo_check(device, pnum, n_hyp, draws));
    PRE3_CHECK(pset1 && pset2, PRE3_E_ARG, "pre3_vo_ransac: null point set");
    Scratch p1, p2;
    PRE3_TRY(p1.alloc(sizeof(double) * 3 * pnum)); PRE3_TRY(p2.alloc(sizeof(double) * 3 * pnum));
    PRE3_HIP(hipMemcpy(p1.p, pset1, sizeof(double) * 3 * pnum, hipMemcpyHostToDevice));
    PRE3_HIP(hipMemcpy(p2.p, pset2, sizeof(double) * 3 * pnum, hipMemcpyHostToDevice));
    return vo_run(pnum, p1.as<double>(), p2.as<double>(), n_hyp, draws, cnum_out, state_out, inlier_out, res, 1, nullptr);
}

int pre3_vo_ransac_seeded(int device, int pnum, const double *pset1, const double *pset2, const double *match, int n_hyp, uint64_t seed, uint64_t seq,
                          int32_t *draws_out, int32_t *capped_out, int32_t *cnum_out, int32_t *state_out, int32_t *inlier_out, pre3_vo_result *res)
{
    PRE3_TRY(vo_check(device, pnum, n_hyp, nullptr, true));
    PRE3_CHECK(pset1 && pset2 && match, PRE3_E_ARG, "pre3_vo_ransac_seeded: null point set or match list");
    Scratch p1, p2, mt;
    PRE3_TRY(p1.alloc(sizeof(double) * 3 * pnum)); PRE3_TRY(p2.alloc(sizeof(double) * 3 * pnum)); PRE3_TRY(mt.alloc(sizeof(double) * 2 * pnum));
    PRE3_HIP(hipMemcpy(p1.p, pset1, sizeof(double) * 3 * pnum, hipMemcpyHostToDevice));
    PRE3_HIP(hipMemcpy(p2.p, pset2, sizeof(double) * 3 * pnum, hipMemcpyHostToDevice));
    PRE3_HIP(hipMemcpy(mt.p, match, sizeof(double) * 2 * pnum, hipMemcpyHostToDevice));
    const VoSeed sd{ seed, seq, mt.as<double>(), draws_out, capped_out };
    return vo_run(pnum, p1.as<double>(), p2.as<double>(), n_hyp, nullptr, cnum_out, state_out, inlier_out, res, 1, nullptr, &sd);
}

static int vo_frames(int device, int rows, int cols, const double *x1, const double *y1, const double *z1, const double *x2,
                     const double *y2, const double *z2, int ldf, int K1, const double *frm1, int K2, const double *frm2, int pnum,
                     const double *match, int n_hyp, const int32_t *draws, double *pset1_out, double *pset2_out, int32_t *cnum_out,
                     int32_t *state_out, int32_t *inlier_out, pre3_vo_result *res, VoSeed *sd)
{
    PRE3_TRY(vo_check(device, pnum, n_hyp, draws, sd != nullptr));
    PRE3_CHECK(rows > 0 && cols > 0 && x1 && y1 && z1 && x2 && y2 && z2 && frm1 && frm2 && match && ldf >= 2 && K1 > 0 && K2 > 0, PRE3_E_ARG,
               "pre3_vo_ransac_frames: bad arguments");
    const size_t img = sizeof(double) * (size_t)rows * cols;
    Scratch im, f1, f2, mt, p1, p2, bad;
    PRE3_TRY(im.alloc(6 * img)); PRE3_TRY(f1.alloc(sizeof(double) * (size_t)ldf * K1)); PRE3_TRY(f2.alloc(sizeof(double) * (size_t)ldf * K2));
    PRE3_TRY(mt.alloc(sizeof(double) * 2 * pnum)); PRE3_TRY(p1.alloc(sizeof(double) * 3 * pnum)); PRE3_TRY(p2.alloc(sizeof(double) * 3 * pnum));
    PRE3_TRY(bad.alloc(sizeof(int32_t)));
    const double *src[6] = { x1, y1, z1, x2, y2, z2 };
    for (int i = 0; i < 6; ++i) PRE3_HIP(hipMemcpy((char *)im.p + i * img, src[i], img, hipMemcpyHostToDevice));
    PRE3_HIP(hipMemcpy(f1.p, frm1, sizeof(double) * (size_t)ldf * K1, hipMemcpyHostToDevice));
    PRE3_HIP(hipMemcpy(f2.p, frm2, sizeof(double) * (size_t)ldf * K2, hipMemcpyHostToDevice));
    PRE3_HIP(hipMemcpy(mt.p, match, sizeof(double) * 2 * pnum, hipMemcpyHostToDevice));
    PRE3_HIP(hipMemset(bad.p, 0, sizeof(int32_t)));
    const double *I = im.as<double>();
    const size_t n = (size_t)rows * cols;
    hipLaunchKernelGGL(k_vo_gather, dim3(ceil_div(pnum, 64)), dim3(64), 0, 0, rows, cols, I, I + n, I + 2 * n, ldf, f1.as<double>(), K1, pnum,
                       mt.as<double>(), 2, p1.as<double>(), bad.as<int32_t>());
    hipLaunchKernelGGL(k_vo_gather, dim3(ceil_div(pnum, 64)), dim3(64), 0, 0, rows, cols, I + 3 * n, I + 4 * n, I + 5 * n, ldf, f2.as<double>(), K2, pnum,
                       mt.as<double>() + 1, 2, p2.as<double>(), bad.as<int32_t>());
    PRE3_HIP(hipGetLastError());
    int32_t b = 0;
    PRE3_HIP(hipMemcpy(&b, bad.p, sizeof b, hipMemcpyDeviceToHost));
    PRE3_CHECK(b == 0, PRE3_E_ARG, "pre3_vo_ransac_frames: %s", (b & 1) ? "a match refers to a keypoint that does not exist" : "a keypoint rounds to a pixel outside the range image");
    if (pset1_out) PRE3_HIP(hipMemcpy(pset1_out, p1.p, sizeof(double) * 3 * pnum, hipMemcpyDeviceToHost));
    if (pset2_out) PRE3_HIP(hipMemcpy(pset2_out, p2.p, sizeof(double) * 3 * pnum, hipMemcpyDeviceToHost));
    if (sd) sd->match_dev = mt.as<double>();
    return vo_run(pnum, p1.as<double>(), p2.as<double>(), n_hyp, draws, cnum_out, state_out, inlier_out, res, 1, nullptr, sd);
}

int pre3_vo_ransac_frames(int device, int rows, int cols, const double *x1, const double *y1, const double *z1, const double *x2,
                          const double *y2, const double *z2, int ldf, int K1, const double *frm1, int K2, const double *frm2, int pnum,
                          const double *match, int n_hyp, const int32_t *draws, double *pset1_out, double *pset2_out, int32_t *cnum_out,
                          int32_t *state_out, int32_t *inlier_out, pre3_vo_result *res)
{
    return vo_frames(device, rows, cols, x1, y1, z1, x2, y2, z2, ldf, K1, frm1, K2, frm2, pnum, match, n_hyp, draws, pset1_out, pset2_out, cnum_out,
                     state_out, inlier_out, res, nullptr);
}

int pre3_vo_ransac_frames_seeded(int device, int rows, int cols, const double *x1, const double *y1, const double *z1, const double *x2,
                                 const double *y2, const double *z2, int ldf, int K1, const double *frm1, int K2, const double *frm2, int pnum,
                                 const double *match, int n_hyp, uint64_t seed, uint64_t seq, int32_t *draws_out, int32_t *capped_out,
                                 double *pset1_out, double *pset2_out, int32_t *cnum_out, int32_t *state_out, int32_t *inlier_out, pre3_vo_result *res)
{
    VoSeed sd{ seed, seq, nullptr, draws_out, capped_out };
    return vo_frames(device, rows, cols, x1, y1, z1, x2, y2, z2, ldf, K1, frm1, K2, frm2, pnum, match, n_hyp, nullptr, pset1_out, pset2_out, cnum_out,
                     state_out, inlier_out, res, &sd);
}

// measurement only: kernels of one RANSAC (dist + score + final) on resident inputs, averaged over reps
int pre3_vo_bench(int device, int pnum, const double *pset1, const double *pset2, int n_hyp, const int32_t *draws, int reps, double *ms_per_call)
{
    PRE3_TRY(vo_check(device, pnum, n_hyp, draws));
    PRE3_CHECK(pset1 && pset2 && reps >= 1 && ms_per_call, PRE3_E_ARG, "pre3_vo_bench: bad arguments");
    Scratch p1, p2;
    PRE3_TRY(p1.alloc(sizeof(double) * 3 * pnum)); PRE3_TRY(p2.alloc(sizeof(double) * 3 * pnum));
    PRE3_HIP(hipMemcpy(p1.p, pset1, sizeof(double) * 3 * pnum, hipMemcpyHostToDevice));
    PRE3_HIP(hipMemcpy(p2.p, pset2, sizeof(double) * 3 * pnum, hipMemcpyHostToDevice));
    PRE3_TRY(vo_run(pnum, p1.as<double>(), p2.as<double>(), n_hyp, draws, nullptr, nullptr, nullptr, nullptr, 3, nullptr));   // warm-up
    return vo_run(pnum, p1.as<double>(), p2.as<double>(), n_hyp, draws, nullptr, nullptr, nullptr, nullptr, reps, ms_per_call);
}

}  // extern "C"
