// pre3_plane.hip -- the floor-plane fit that produces R_plane for the heading update (pre3_plane_fit, pre3_heading_from_scan).
//   plane_fit_to_data.m:13-21,41-58,82,94-125,138-149   (camera coordinates, crop, sign rule, the two rays, the axes, R)
//   plane_fitting/ransacfitplane.m:90-105               (a trial's plane is its three points; the distance accumulated coordinate by coordinate)
//   plane_fitting/ransac.m:127-133,135-215              (p = 0.99, N, the stopping rule, at most 1001 trials)
//   plane_fitting/fitplane.m:47-54                      (least squares on the winner's inliers: the last right singular vector of [XYZ' 1])
//   plane_fitting/plane_imp_line_par_int_3d.m:56-100    (ray / plane intersection with its parallel test)
//   aux_code/find_angle_bw_2_vecs.m:12                  (the angle of the sign rule)
// Two launches behind the upload of the cropped points -- or, from a resident SR4000 frame (pre3_plane_fit_frame, pre3_heading_from_frame; DESIGN.md
// section 23), behind k_plane_crop, which gathers the box from the handle's filtered planes into the same point block:
//   k_plane_crop   one lane per point of the box, adjacent lanes adjacent rows of a column (the planes are column-major): X = -x, Y = -y, Z = z into
//                  [X | Y | Z] (plane_pack's layout, pre3_planecrop.h's arithmetic); a wave that met a non-finite value ORs 1 into the flag word.  The
//                  launches behind it read that word first and leave at once when it is set (k_plane_fit reports sta = 5).
//   k_plane_score  one workgroup per PG hypotheses.  Every lane builds the PG planes from their draws (uniform), then the lanes stride over the points:
//                  a point is loaded once and tested against the PG planes; ballot + popcount per wave, the four waves summed through LDS.  Every draw
//                  supplied is scored; no atomics, no workgroup waits for another.
//   k_plane_fit    one workgroup.  The stopping rule replayed on the scores: after T trials ransac.m's N is a function of the largest of the first T scores
//                  alone, so the trial count is the smallest T with N(T) <= T (or T = 1001) -- a prefix maximum and a minimum, no sequential loop.  Then
//                  the winner's mask, the ten sums of [XYZ' 1]'[XYZ' 1] over it (per-lane partial sums in point order, xor butterfly, the waves in order:
//                  the same bits on every run), its smallest eigenvector by cyclic Jacobi in lane 0, the sign rule, the rays, R; in the context form also
//                  z = R_plane(:, 2) and RR (ekf_heading_update.m:29, :36-40) for the heading rows queued behind it (pre3_rows.hip).
// All fp64.  The inlier test is a discontinuity: plane_of / plane_dist are compiled without contraction and shared by both kernels, so the mask of the
// fit launch is the mask the score counted.
#include <cmath>
#include <mutex>

#include "pre3_internal.h"
#include "pre3_geomdev.h"
#include "pre3_planecrop.h"

namespace pre3 {

namespace {

constexpr int PG = 4;           // hypotheses per workgroup of the score launch
constexpr int PB = 256;         // threads per workgroup of both launches
constexpr int PW = PB / 64;
static_assert(PB * 4 >= PRE3_PLANE_MAX_DRAWS, "k_plane_fit replays four trials per thread");

struct PlaneOut {               // device-side result block (pre3_plane_result's content)
    double B[4], R[9], p_orig[3], p_ray[3], N;
    int32_t sta, n_inliers, n_trials, best;
};

struct Plane3 { double p[3], n[3]; };

// ransacfitplane.m:92-93 from the three points of a draw; collinear or repeated points give n = NaN (0 / 0), which scores 0
__device__ inline Plane3 plane_of(const double *X, const double *Y, const double *Z, const int32_t *d)
{
#pragma clang fp contract(off)
    Plane3 pl;
    const int i1 = d[0], i2 = d[1], i3 = d[2];
    pl.p[0] = X[i1]; pl.p[1] = Y[i1]; pl.p[2] = Z[i1];
    const double a[3] = { X[i2] - pl.p[0], Y[i2] - pl.p[1], Z[i2] - pl.p[2] }, b[3] = { X[i3] - pl.p[0], Y[i3] - pl.p[1], Z[i3] - pl.p[2] };
    const double n0 = a[1] * b[2] - a[2] * b[1], n1 = a[2] * b[0] - a[0] * b[2], n2 = a[0] * b[1] - a[1] * b[0];
    const double nn = sqrt(n0 * n0 + n1 * n1 + n2 * n2);
    pl.n[0] = n0 / nn; pl.n[1] = n1 / nn; pl.n[2] = n2 / nn;
    return pl;
}

// ransacfitplane.m:101-103: d = d + (X(i,:) - P(i,1)) * n(i), i = 1, 2, 3 -- three products, two sums, each rounded on its own
__device__ inline double plane_dist(const Plane3 &pl, double x, double y, double z)
{
#pragma clang fp contract(off)
    double d = (x - pl.p[0]) * pl.n[0];
    d = d + (y - pl.p[1]) * pl.n[1];
    d = d + (z - pl.p[2]) * pl.n[2];
    return d;
}

// ransac.m:196-200 at a best score of c > 0 inliers out of npts (s = 3, p = 0.99)
__device__ inline double ransac_N(int c, int npts)
{
    const double eps = 2.220446049250313e-16, frac = (double)c / (double)npts;
    double pno = 1.0 - pow(frac, 3.0);
    pno = fmax(eps, pno);
    pno = fmin(1.0 - eps, pno);
    return log(1.0 - 0.99) / log(pno);
}

// the box of a resident frame into the fit's point block; flag (zero at launch) |= 1 when a point of the box is not finite.  Reads stay inside the
// planes (the host has checked the box against the frame), writes inside [0, 3 npts).
__global__ __launch_bounds__(PB) void k_plane_crop(PlaneCrop b, const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ z,
                                                   double *__restrict__ pts, int32_t *__restrict__ flag)
{
    const int k = blockIdx.x * PB + threadIdx.x;
    const bool bad = k < b.nr * b.nc && plane_crop_point(b, k, x, y, z, pts);
    if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(flag, 1);      // (one word, one value: the result does not depend on the order)
}

__global__ __launch_bounds__(PB) void k_plane_score(int npts, const double *__restrict__ pts, int n_draw, const int32_t *__restrict__ draws, double t,
                                                    int32_t *__restrict__ counts, const int32_t *__restrict__ flag /* null, or the crop's word */)
{
    __shared__ int32_t s_cnt[PW][PG];
    if (flag != nullptr && *flag != 0) return;              // (uniform: a non-finite point in the box, nothing is scored)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h0 = blockIdx.x * PG;
    const double *X = pts, *Y = pts + npts, *Z = pts + 2 * (size_t)npts;
    Plane3 pl[PG];
#pragma unroll
    for (int g = 0; g < PG; ++g) pl[g] = plane_of(X, Y, Z, draws + 3 * (size_t)min(h0 + g, n_draw - 1));      // (the last group repeats the last draw)
    int cnt[PG];
#pragma unroll
    for (int g = 0; g < PG; ++g) cnt[g] = 0;
    for (int base = 0; base < npts; base += PB) {           // (the same trip count in every lane: the ballots are whole waves)
        const int k = base + tid;
        const bool ok = k < npts;
        const double x = ok ? X[k] : 0.0, y = ok ? Y[k] : 0.0, z = ok ? Z[k] : 0.0;
#pragma unroll
        for (int g = 0; g < PG; ++g) cnt[g] += __popcll(__ballot(ok && fabs(plane_dist(pl[g], x, y, z)) < t));      // ransacfitplane.m:105
    }
    if (lane == 0) {
#pragma unroll
        for (int g = 0; g < PG; ++g) s_cnt[wave][g] = cnt[g];
    }
    __syncthreads();
    if (tid < PG && h0 + tid < n_draw) {
        int s = 0;
        for (int w = 0; w < PW; ++w) s += s_cnt[w][tid];
        counts[h0 + tid] = s;
    }
}

__device__ inline int block_min(int v, int *s_w /* [PW] */)
{
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    __syncthreads();                                        // (s_w may still be read from the previous use)
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    int r = s_w[0];
    for (int w = 1; w < PW; ++w) r = min(r, s_w[w]);
    return r;
}

// the smallest eigenvector of the symmetric 4 x 4 M by cyclic Jacobi (one lane); relative stopping rule |m_pq| <= eps sqrt(m_pp m_qq)
__device__ void plane_eig4(const double *m10 /* xx xy xz x yy yz y zz z 1 */, double B[4])
{
    double A[4][4], V[4][4];
    A[0][0] = m10[0]; A[0][1] = m10[1]; A[0][2] = m10[2]; A[0][3] = m10[3];
    A[1][1] = m10[4]; A[1][2] = m10[5]; A[1][3] = m10[6];
    A[2][2] = m10[7]; A[2][3] = m10[8]; A[3][3] = m10[9];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) { if (j < i) A[i][j] = A[j][i]; V[i][j] = i == j ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 60; ++sweep) {
        int rotated = 0;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                const double apq = A[p][q], app = A[p][p], aqq = A[q][q];
                if (apq == 0.0 || fabs(apq) <= 2.220446049250313e-16 * sqrt(fabs(app * aqq))) continue;
                rotated = 1;
                const double theta = (aqq - app) / (2.0 * apq);
                const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
#pragma unroll
                for (int k = 0; k < 4; ++k) {               // A <- A J, V <- V J
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq;
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {               // A <- J' A
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk;
                }
                A[p][q] = 0.0; A[q][p] = 0.0;
            }
        }
        if (!rotated) break;
    }
    int kmin = 0;
    double lmin = A[0][0];
#pragma unroll
    for (int k = 1; k < 4; ++k) if (A[k][k] < lmin) { lmin = A[k][k]; kmin = k; }
#pragma unroll
    for (int i = 0; i < 4; ++i) B[i] = kmin == 0 ? V[i][0] : (kmin == 1 ? V[i][1] : (kmin == 2 ? V[i][2] : V[i][3]));
}

// plane_imp_line_par_int_3d.m:56-100 for the line through the origin along (f, g, h); false: parallel (the reference returns p = 0 then)
__device__ inline bool plane_ray(const double *B, const double *dir, double *p)
{
    const double norm1 = sqrt(B[0] * B[0] + B[1] * B[1] + B[2] * B[2]), norm2 = sqrt(dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2]);
    const double denom = B[0] * dir[0] + B[1] * dir[1] + B[2] * dir[2];
    if (!(fabs(denom) >= 0.00001 * norm1 * norm2)) return false;
    const double tt = -B[3] / denom;
    for (int i = 0; i < 3; ++i) p[i] = tt * dir[i];
    return true;
}

__global__ __launch_bounds__(PB) void k_plane_fit(int npts, const double *__restrict__ pts, int n_draw, const int32_t *__restrict__ draws,
                                                  const int32_t *__restrict__ counts, double t, int po, int pr, int transpose,
                                                  PlaneOut *__restrict__ out, int32_t *__restrict__ inl_out, HeadingSrc *__restrict__ src,
                                                  const int32_t *__restrict__ flag /* null, or the crop's word */)
{
    __shared__ int s_w[PW], s_M;
    __shared__ double s_m[PW][10];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // ---- a non-finite point in the box of a resident frame (uniform): neither the draws nor the scores were written, and a NaN in the ten sums would
    // never meet the Jacobi sweep's relative stopping rule.  sta = 5, an empty result, and the heading rows skip on that status.
    if (flag != nullptr && *flag != 0) {
        if (inl_out != nullptr) for (int k = tid; k < npts; k += PB) inl_out[k] = 0;
        if (tid != 0) return;
        PlaneOut o;
        for (int i = 0; i < 4; ++i) o.B[i] = 0.0;
        for (int i = 0; i < 9; ++i) o.R[i] = 0.0;
        for (int i = 0; i < 3; ++i) { o.p_orig[i] = 0.0; o.p_ray[i] = 0.0; }
        o.N = 0.0; o.sta = 5; o.n_inliers = 0; o.n_trials = 0; o.best = -1;
        *out = o;
        if (src != nullptr) {
            HeadingSrc hs;
            hs.sta = 5; hs.pad_ = 0;
            for (int i = 0; i < 3; ++i) hs.z[i] = 0.0;
            for (int i = 0; i < 9; ++i) hs.RR[i] = 0.0;
            *src = hs;
        }
        return;
    }
    const double *X = pts, *Y = pts + npts, *Z = pts + 2 * (size_t)npts;
    // ---- ransac.m:135-215 replayed: thread tid owns trials 4 tid .. 4 tid + 3
    int v[4], run[4], m = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { const int i = 4 * tid + j; v[j] = i < n_draw ? counts[i] : 0; m = max(m, v[j]); }
    int s = m;                                              // inclusive prefix maximum over the threads
    for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(s, o, 64); if (lane >= o) s = max(s, u); }
    if (lane == 63) s_w[wave] = s;
    __syncthreads();
    int excl = __shfl_up(s, 1, 64);
    if (lane == 0) excl = 0;
    for (int w = 0; w < wave; ++w) excl = max(excl, s_w[w]);
    int myT = 0x7fffffff;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        excl = max(excl, v[j]); run[j] = excl;              // the best score after T = 4 tid + j + 1 trials
        const int T = 4 * tid + j + 1;
        if (T <= n_draw && myT == 0x7fffffff) {
            const double N = run[j] > 0 ? ransac_N(run[j], npts) : 1.0;
            if (!(N > (double)T) || T > 1000) myT = T;      // ransac.m:135 at the top of the next pass, :209 after the increment
        }
    }
    const int Tend = block_min(myT, s_w);
    const int n_trials = Tend == 0x7fffffff ? n_draw : Tend;
#pragma unroll
    for (int j = 0; j < 4; ++j) if (4 * tid + j + 1 == n_trials) s_M = run[j];
    __syncthreads();
    const int M = s_M;
    int mine = 0x7fffffff;                                  // the first trial that reached M: the last strict improvement
#pragma unroll
    for (int j = 3; j >= 0; --j) if (4 * tid + j < n_trials && v[j] == M) mine = 4 * tid + j;
    const int first = block_min(mine, s_w);
    const int best = M > 0 ? first : -1;
    int sta = M > 0 ? (Tend == 0x7fffffff ? 2 : 1) : 0;     // ransac.m:224 (no trial had an inlier); 2: the rule wanted more trials than were supplied
    // ---- the winner's mask and the ten sums of [XYZ' 1]' [XYZ' 1] over it (fitplane.m:47)
    double acc[10];
#pragma unroll
    for (int e = 0; e < 10; ++e) acc[e] = 0.0;
    if (best >= 0) {
        const Plane3 pl = plane_of(X, Y, Z, draws + 3 * (size_t)best);
        for (int k = tid; k < npts; k += PB) {
            const double x = X[k], y = Y[k], z = Z[k];
            const bool in = fabs(plane_dist(pl, x, y, z)) < t;
            if (inl_out != nullptr) inl_out[k] = in ? 1 : 0;
            if (in) {
                acc[0] += x * x; acc[1] += x * y; acc[2] += x * z; acc[3] += x;
                acc[4] += y * y; acc[5] += y * z; acc[6] += y;
                acc[7] += z * z; acc[8] += z; acc[9] += 1.0;
            }
        }
    } else if (inl_out != nullptr) {
        for (int k = tid; k < npts; k += PB) inl_out[k] = 0;
    }
#pragma unroll
    for (int e = 0; e < 10; ++e) {
        double a = acc[e];
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
        if (lane == 0) s_m[wave][e] = a;
    }
    __syncthreads();
    if (tid != 0) return;
    PlaneOut o;
    for (int i = 0; i < 4; ++i) o.B[i] = 0.0;
    for (int i = 0; i < 9; ++i) o.R[i] = 0.0;
    o.p_orig[0] = X[po]; o.p_orig[1] = Y[po]; o.p_orig[2] = Z[po];          // plane_fit_to_data.m:46-48
    o.p_ray[0] = X[pr]; o.p_ray[1] = Y[pr]; o.p_ray[2] = Z[pr];             // :94-96
    o.N = M > 0 ? ransac_N(M, npts) : 1.0;
    o.n_inliers = M; o.n_trials = n_trials; o.best = best;
    if (best >= 0) {
        double m10[10], B[4];
        for (int e = 0; e < 10; ++e) { double a = s_m[0][e]; for (int w = 1; w < PW; ++w) a += s_m[w][e]; m10[e] = a; }
        plane_eig4(m10, B);
        // plane_fit_to_data.m:49-58: B = -B when the angle between B(1:3) and -p_orig is below 90 degrees
        const double nb = sqrt(B[0] * B[0] + B[1] * B[1] + B[2] * B[2]);
        const double np_ = sqrt(o.p_orig[0] * o.p_orig[0] + o.p_orig[1] * o.p_orig[1] + o.p_orig[2] * o.p_orig[2]);
        const double cs = -(B[0] * o.p_orig[0] + B[1] * o.p_orig[1] + B[2] * o.p_orig[2]) / nb / np_;
        const double a7 = acos(fmin(fmax(cs, -1.0), 1.0)) * (180.0 / 3.14159265358979323846);
        if (a7 < 90.0) for (int i = 0; i < 4; ++i) B[i] = -B[i];
        for (int i = 0; i < 4; ++i) o.B[i] = B[i];
        const double zax[3] = { B[0] / nb, B[1] / nb, B[2] / nb };         // :82
        double i1[3], i2[3];
        bool ok = plane_ray(B, o.p_ray, i1) && plane_ray(B, o.p_orig, i2);  // :99-100, :116-117
        double yax[3] = { 0, 0, 0 }, xax[3] = { 0, 0, 0 };
        if (ok) {
            for (int i = 0; i < 3; ++i) yax[i] = i1[i] - i2[i];             // :120
            const double ny = sqrt(yax[0] * yax[0] + yax[1] * yax[1] + yax[2] * yax[2]);
            ok = ny > 0.0 && ny < INFINITY;
            if (ok) {
                for (int i = 0; i < 3; ++i) yax[i] /= ny;                   // :123
                const double cx[3] = { yax[1] * zax[2] - yax[2] * zax[1], yax[2] * zax[0] - yax[0] * zax[2], yax[0] * zax[1] - yax[1] * zax[0] };
                const double nx = sqrt(cx[0] * cx[0] + cx[1] * cx[1] + cx[2] * cx[2]);
                ok = nx > 0.0 && nx < INFINITY;
                if (ok) for (int i = 0; i < 3; ++i) xax[i] = -cx[i] / nx;   // :124-125
            }
        }
        if (ok) for (int i = 0; i < 3; ++i) { o.R[i] = xax[i]; o.R[3 + i] = zax[i]; o.R[6 + i] = yax[i]; }      // :138-149, columns x_axis, z_axis, y_axis
        else sta = 3;
    }
    o.sta = sta;
    *out = o;
    if (src != nullptr) {
        HeadingSrc hs;
        hs.sta = sta; hs.pad_ = 0;
        for (int i = 0; i < 3; ++i) hs.z[i] = 0.0;
        for (int i = 0; i < 9; ++i) hs.RR[i] = 0.0;
        if (sta == 1) {
            double Rp[9];                                                   // R_plane column-major: R' (mono_slam.m:192) or R
            for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) Rp[j * 3 + i] = transpose ? o.R[i * 3 + j] : o.R[j * 3 + i];
            for (int i = 0; i < 3; ++i) hs.z[i] = Rp[3 + i];               // ekf_heading_update.m:29
            heading_RR(Rp, hs.RR);
        }
        *src = hs;
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------------------
struct PlaneJob {
    int r0, c0, nr, nc, npts, po, pr, n_draw;
    size_t off_draws, bytes_in, off_counts, off_out, off_inl, off_flag, bytes_total;      // off_flag: the crop's word (a resident frame)
    size_t bytes_up;            // what crosses PCIe from host planes: bytes_in, or the points alone when the draws are made on the device (the seeded forms)
};
struct PlaneSeed { unsigned long long seed, seq; };      // k_draw_plane writes the draws region behind the upload

// where the points come from: three host planes (rows x cols, column-major) for `device`, or a resident SR4000 frame, whose
// view plane_check fills
struct PlaneSource {
    bool resident;
    int device, rows, cols;
    const double *x, *y, *z;
    pre3_sr_frame *frame;
    SrFrameView v;
    hipStream_t stream() const { return resident ? v.stream : nullptr; }      // of the stateless fit: the handle's, or the null stream
    const SrFrameView *crop() const { return resident ? &v : nullptr; }
};
static PlaneSource host_planes(int device, int rows, int cols, const double *x_sr, const double *y_sr, const double *z_sr)
{
    PlaneSource s{};
    s.device = device; s.rows = rows; s.cols = cols; s.x = x_sr; s.y = y_sr; s.z = z_sr;
    return s;
}
static PlaneSource resident_frame(pre3_sr_frame *f)
{
    PlaneSource s{};
    s.resident = true; s.frame = f;
    return s;
}

// every host check that needs no coordinate, and the layout of the work block
static int plane_job(const char *who, int rows, int cols, const int32_t *box, double t, int n_draw, const int32_t *draws, PlaneJob *job, bool seeded)
{
    PRE3_CHECK(draws || seeded, PRE3_E_ARG, "%s: null argument", who);
    PRE3_CHECK(rows >= 1 && cols >= 1, PRE3_E_ARG, "%s: a %d x %d image", who, rows, cols);
    const int32_t dflt[4] = { 80, 144, 50, 120 };           // plane_fit_to_data.m:17-18
    const int32_t *b = box ? box : dflt;
    PRE3_CHECK(b[0] >= 1 && b[0] <= b[1] && b[1] <= rows && b[2] >= 1 && b[2] <= b[3] && b[3] <= cols, PRE3_E_ARG,
               "%s: box rows %d..%d, columns %d..%d outside the %d x %d image", who, b[0], b[1], b[2], b[3], rows, cols);
    PlaneJob j{};
    j.r0 = b[0] - 1; j.c0 = b[2] - 1; j.nr = b[1] - b[0] + 1; j.nc = b[3] - b[2] + 1;
    PRE3_CHECK((long long)j.nr * j.nc >= 3, PRE3_E_ARG, "%s: too few points to fit plane", who);      // ransacfitplane.m:63-65
    j.npts = j.nr * j.nc;
    const int io = j.nr / 2, jo = j.nc / 2;                 // floor(size / 2) + 1, 0-based
    PRE3_CHECK(io - 20 >= 0, PRE3_E_ARG, "%s: p_ray lies 20 rows above the centre of the box, outside a box of %d rows", who, j.nr);
    j.po = jo * j.nr + io; j.pr = j.po - 20;
    PRE3_CHECK(n_draw >= 1 && n_draw <= PRE3_PLANE_MAX_DRAWS, PRE3_E_ARG, "%s: n_draw=%d outside [1, %d]", who, n_draw, PRE3_PLANE_MAX_DRAWS);
    PRE3_CHECK(t > 0.0 && std::isfinite(t), PRE3_E_ARG, "%s: t must be positive", who);
    for (int i = 0; !seeded && i < 3 * n_draw; ++i)
        PRE3_CHECK(draws[i] >= 0 && draws[i] < j.npts, PRE3_E_ARG, "%s: draws[%d]=%d is not a point of the box (npts=%d)", who, i, draws[i], j.npts);
    j.n_draw = n_draw;
    j.off_draws = up16(sizeof(double) * 3 * (size_t)j.npts);      // (16-byte aligned: a table for a resident frame is pulled there on its own)
    j.bytes_in = up16(j.off_draws + sizeof(int32_t) * 3 * (size_t)n_draw);
    j.off_counts = j.bytes_in;
    j.off_out = up16(j.off_counts + sizeof(int32_t) * (size_t)n_draw);
    j.off_inl = up16(j.off_out + sizeof(PlaneOut));
    j.off_flag = up16(j.off_inl + sizeof(int32_t) * (size_t)j.npts);
    j.bytes_total = j.off_flag + 16;
    j.bytes_up = seeded ? j.off_draws : j.bytes_in;
    *job = j;
    return PRE3_OK;
}

// every host check on the source and the job, before anything is launched: a resident frame gives its view (the device tests its coordinates, sta = 5);
// host planes are tested here, coordinate by coordinate
static int plane_check(const char *who, PlaneSource *s, const int32_t *box, double t, int n_draw, const int32_t *draws, PlaneJob *job, bool seeded = false)
{
    PRE3_CHECK(s->resident ? s->frame != nullptr : s->x && s->y && s->z && (draws || seeded), PRE3_E_ARG, "%s: null argument", who);
    if (s->resident) {
        PRE3_TRY(sr_frame_view(s->frame, &s->v));
        s->device = s->v.device; s->rows = s->v.rows; s->cols = s->v.cols;
    }
    PlaneJob j;
    PRE3_TRY(plane_job(who, s->rows, s->cols, box, t, n_draw, draws, &j, seeded));
    for (int c = 0; !s->resident && c < j.nc; ++c) {
        const size_t o = (size_t)(j.c0 + c) * s->rows + j.r0;
        for (int r = 0; r < j.nr; ++r)
            PRE3_CHECK(std::isfinite(s->x[o + r]) && std::isfinite(s->y[o + r]) && std::isfinite(s->z[o + r]), PRE3_E_ARG,
                       "%s: a coordinate at row %d, column %d is not finite", who, j.r0 + r + 1, j.c0 + c + 1);
    }
    *job = j;
    return PRE3_OK;
}

// plane_fit_to_data.m:13, :19-21, :41: the box in camera coordinates, column-major, as [X | Y | Z | draws] -- the only bytes that cross PCIe
static void plane_pack(const PlaneJob &j, const PlaneSource &s, const int32_t *draws, void *stage)
{
    double *X = (double *)stage, *Y = X + j.npts, *Z = Y + j.npts;
    for (int c = 0; c < j.nc; ++c) {
        const size_t o = (size_t)(j.c0 + c) * s.rows + j.r0, d = (size_t)c * j.nr;
        for (int r = 0; r < j.nr; ++r) { X[d + r] = -s.x[o + r]; Y[d + r] = -s.y[o + r]; Z[d + r] = s.z[o + r]; }
    }
    const size_t end_pts = sizeof(double) * 3 * (size_t)j.npts;
    if (j.off_draws > end_pts) memset((char *)stage + end_pts, 0, j.off_draws - end_pts);
    if (draws) memcpy((char *)stage + j.off_draws, draws, sizeof(int32_t) * 3 * (size_t)j.n_draw);
}

// what a call stages and sends up, and where it lands in the work block: plane_pack's image of host planes (stage bytes_in, send bytes_up); for a
// resident frame a supplied table alone, padded to where the scores begin -- nothing when the draws are seeded
struct PlaneUpload { size_t off, stage_bytes, bytes; };
static PlaneUpload plane_upload(const PlaneJob &j, const PlaneSource &s, const int32_t *draws)
{
    if (!s.resident) return { 0, j.bytes_in, j.bytes_up };
    const size_t b = draws ? j.bytes_in - j.off_draws : 0;
    return { j.off_draws, b, b };
}
static void plane_stage_fill(const PlaneJob &j, const PlaneSource &s, const int32_t *draws, const PlaneUpload &up, void *stage)
{
    if (!s.resident) { plane_pack(j, s, draws, stage); return; }
    memset(stage, 0, up.stage_bytes);
    memcpy(stage, draws, sizeof(int32_t) * 3 * (size_t)j.n_draw);
}

// crop != nullptr (a resident frame): the point block comes from the view's planes by k_plane_crop, queued here in front of the draws; the flag word at
// j.off_flag is zeroed on `st` first and every launch behind the crop reads it
static int plane_launch(const PlaneJob &j, char *buf, double t, int transpose, bool want_inl, HeadingSrc *src, hipStream_t st, const PlaneSeed *sd = nullptr,
                        const SrFrameView *crop = nullptr)
{
    const double *pts = (const double *)buf;
    const int32_t *draws = (const int32_t *)(buf + j.off_draws);
    int32_t *flag = crop ? (int32_t *)(buf + j.off_flag) : nullptr;
    if (crop) {
        PRE3_HIP(hipMemsetAsync(flag, 0, 16, st));
        const PlaneCrop b{ crop->rows, j.r0, j.c0, j.nr, j.nc };
        hipLaunchKernelGGL(k_plane_crop, dim3(ceil_div(j.npts, PB)), dim3(PB), 0, st, b, crop->x, crop->y, crop->z, (double *)buf, flag);
        PRE3_HIP(hipGetLastError());
    }
    if (sd) PRE3_TRY(launch_draw_plane(sd->seed, sd->seq, j.n_draw, j.npts, pts, (int32_t *)(buf + j.off_draws), st, flag));
    int32_t *counts = (int32_t *)(buf + j.off_counts);
    hipLaunchKernelGGL(k_plane_score, dim3(ceil_div(j.n_draw, PG)), dim3(PB), 0, st, j.npts, pts, j.n_draw, draws, t, counts, (const int32_t *)flag);
    PRE3_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_plane_fit, dim3(1), dim3(PB), 0, st, j.npts, pts, j.n_draw, draws, (const int32_t *)counts, t, j.po, j.pr, transpose,
                       (PlaneOut *)(buf + j.off_out), want_inl ? (int32_t *)(buf + j.off_inl) : (int32_t *)nullptr, src, (const int32_t *)flag);
    PRE3_HIP(hipGetLastError());
    return PRE3_OK;
}

static void plane_result(const PlaneOut &o, pre3_plane_result *res)
{
    memcpy(res->B, o.B, sizeof o.B); memcpy(res->R, o.R, sizeof o.R);
    memcpy(res->p_orig, o.p_orig, sizeof o.p_orig); memcpy(res->p_ray, o.p_ray, sizeof o.p_ray);
    res->N = o.N; res->sta = o.sta; res->n_inliers = o.n_inliers; res->n_trials = o.n_trials; res->best = o.best;
}

// the scores, the winner's mask and the table from the work block of a fit that has finished (any may be null)
static int plane_read_back(const PlaneJob &j, const char *buf, int32_t *count_out, int32_t *inlier_out, int32_t *draws_out)
{
    if (count_out) PRE3_HIP(hipMemcpy(count_out, buf + j.off_counts, sizeof(int32_t) * (size_t)j.n_draw, hipMemcpyDeviceToHost));
    if (inlier_out) PRE3_HIP(hipMemcpy(inlier_out, buf + j.off_inl, sizeof(int32_t) * (size_t)j.npts, hipMemcpyDeviceToHost));
    if (draws_out) PRE3_HIP(hipMemcpy(draws_out, buf + j.off_draws, sizeof(int32_t) * 3 * (size_t)j.n_draw, hipMemcpyDeviceToHost));
    return PRE3_OK;
}

// pinned staging of the stateless entry point: one block per process, grown on demand, held for the length of a call
static PinBlock g_stage; static std::mutex g_stage_mu;      // (whoever touches g_stage holds g_stage_mu)

struct StreamIdle {             // a work block fed from a handle's stream goes back to its pool only once that stream is idle, on every way out
    hipStream_t st;
    ~StreamIdle() { if (st) (void)hipStreamSynchronize(st); }
};

// the context's work block [points | draws | scores | result | mask | flag], grown on demand, and the block the heading rows read: both zeroed on the
// context's stream, which does not synchronise with the null stream
static int plane_reserve(pre3_ctx *c, const char *who, size_t bytes)
{
    DevBlock &buf = c->mem.plane_buf;
    if (buf.p && buf.bytes < bytes) PRE3_TRY(stream_drain(c, who));
    PRE3_TRY(buf.reserve(bytes, bytes + bytes / 4, Zero::on_stream(c->stream)));
    if (c->plane_src == nullptr) PRE3_TRY(c->mem.fixed.dev(&c->plane_src, sizeof(HeadingSrc), Zero::on_stream(c->stream)));
    return PRE3_OK;
}

}  // namespace

}  // namespace pre3

using namespace pre3;

extern "C" {

// the stateless fit, from host planes on the null stream or from a resident frame on the handle's (DESIGN.md sections 17 and 23).  A frame's box with
// a non-finite coordinate: sta = 5, PRE3_E_NUMERIC with res filled and every other output zeroed (neither the table nor the scores were written).
static int plane_fit_impl(const char *who, PlaneSource s, const int32_t *box, double t, int n_draw, const int32_t *draws, int32_t *count_out,
                          int32_t *inlier_out, pre3_plane_result *res, const PlaneSeed *sd, int32_t *draws_out)
{
    PlaneJob j;
    PRE3_CHECK(res != nullptr, PRE3_E_ARG, "%s: null argument", who);
    PRE3_TRY(plane_check(who, &s, box, t, n_draw, draws, &j, sd != nullptr));
    PRE3_TRY(select_device(who, s.device));
    Scratch d;
    PRE3_TRY(d.alloc(j.bytes_total));
    const hipStream_t st = s.stream();
    StreamIdle idle{ st };
    const PlaneUpload up = plane_upload(j, s, draws);
    PlaneOut o;
    {
        std::lock_guard<std::mutex> lk(g_stage_mu);
        if (up.bytes) {
            PRE3_TRY(g_stage.reserve(up.stage_bytes, (up.stage_bytes + 65535) & ~(size_t)65535, PIN_DEFAULT));
            plane_stage_fill(j, s, draws, up, g_stage.p);
            PRE3_HIP(hipMemcpyAsync(d.as<char>() + up.off, g_stage.p, up.bytes, hipMemcpyHostToDevice, st));
        }
        PRE3_TRY(plane_launch(j, d.as<char>(), t, 0, inlier_out != nullptr, nullptr, st, sd, s.crop()));
        // (either way the stream is idle afterwards: the staging block is free again)
        if (st == nullptr) PRE3_HIP(hipMemcpy(&o, d.as<char>() + j.off_out, sizeof o, hipMemcpyDeviceToHost));
        else {
            PRE3_HIP(hipMemcpyAsync(&o, d.as<char>() + j.off_out, sizeof o, hipMemcpyDeviceToHost, st));
            PRE3_HIP(hipStreamSynchronize(st));
        }
    }
    plane_result(o, res);
    if (o.sta == 5) {
        if (count_out) memset(count_out, 0, sizeof(int32_t) * (size_t)n_draw);
        if (inlier_out) memset(inlier_out, 0, sizeof(int32_t) * (size_t)j.npts);
        if (draws_out) memset(draws_out, 0, sizeof(int32_t) * 3 * (size_t)n_draw);
        set_error("%s: a coordinate inside the box of the resident frame is not finite (sta = 5)", who);
        return PRE3_E_NUMERIC;
    }
    return plane_read_back(j, d.as<char>(), count_out, inlier_out, draws_out);
}

int pre3_plane_fit(int device, int rows, int cols, const double *x_sr, const double *y_sr, const double *z_sr, const int32_t *box, double t,
                   int n_draw, const int32_t *draws, int32_t *count_out, int32_t *inlier_out, pre3_plane_result *res)
{
    return plane_fit_impl("pre3_plane_fit", host_planes(device, rows, cols, x_sr, y_sr, z_sr), box, t, n_draw, draws, count_out, inlier_out, res, nullptr, nullptr);
}

int pre3_plane_fit_seeded(int device, int rows, int cols, const double *x_sr, const double *y_sr, const double *z_sr, const int32_t *box, double t,
                          int n_draw, uint64_t seed, uint64_t seq, int32_t *draws_out, int32_t *count_out, int32_t *inlier_out, pre3_plane_result *res)
{
    const PlaneSeed sd{ seed, seq };
    return plane_fit_impl("pre3_plane_fit_seeded", host_planes(device, rows, cols, x_sr, y_sr, z_sr), box, t, n_draw, nullptr, count_out, inlier_out, res, &sd,
                          draws_out);
}

int pre3_plane_fit_frame(pre3_sr_frame *f, const int32_t *box, double t, int n_draw, const int32_t *draws, int32_t *count_out, int32_t *inlier_out,
                         pre3_plane_result *res)
{
    return plane_fit_impl("pre3_plane_fit_frame", resident_frame(f), box, t, n_draw, draws, count_out, inlier_out, res, nullptr, nullptr);
}

int pre3_plane_fit_frame_seeded(pre3_sr_frame *f, const int32_t *box, double t, int n_draw, uint64_t seed, uint64_t seq, int32_t *draws_out,
                                int32_t *count_out, int32_t *inlier_out, pre3_plane_result *res)
{
    const PlaneSeed sd{ seed, seq };
    return plane_fit_impl("pre3_plane_fit_frame_seeded", resident_frame(f), box, t, n_draw, nullptr, count_out, inlier_out, res, &sd, draws_out);
}

// measurement only: device time of one fit (upload + score + fit launches) between two events, averaged over reps warmed calls
int pre3_plane_bench(int device, int rows, int cols, const double *x_sr, const double *y_sr, const double *z_sr, const int32_t *box, double t,
                     int n_draw, const int32_t *draws, int reps, double *ms_per_call)
{
    const char *who = "pre3_plane_bench";
    PlaneJob j;
    PlaneSource s = host_planes(device, rows, cols, x_sr, y_sr, z_sr);
    PRE3_CHECK(reps >= 1 && ms_per_call != nullptr, PRE3_E_ARG, "%s: bad arguments", who);
    PRE3_TRY(plane_check(who, &s, box, t, n_draw, draws, &j));
    PRE3_TRY(select_device(who, device));
    Scratch d;
    PRE3_TRY(d.alloc(j.bytes_total));
    PinBlock stb;
    PRE3_TRY(stb.reserve(j.bytes_in, j.bytes_in, PIN_DEFAULT));
    void *const st = stb.p;
    plane_pack(j, s, draws, st);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = PRE3_OK;
    float ms = 0;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) { set_error("%s: event creation failed", who); rc = PRE3_E_HIP; }
    for (int r = -3; r < reps && rc == PRE3_OK; ++r) {       // three warm-up calls
        if (r == 0 && hipEventRecord(e0, 0) != hipSuccess) { set_error("%s: event record failed", who); rc = PRE3_E_HIP; break; }
        if (hipMemcpyAsync(d.p, st, j.bytes_in, hipMemcpyHostToDevice, 0) != hipSuccess) { set_error("%s: upload failed", who); rc = PRE3_E_HIP; break; }
        rc = plane_launch(j, d.as<char>(), t, 0, false, nullptr, 0);
    }
    if (rc == PRE3_OK && (hipEventRecord(e1, 0) != hipSuccess || hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess)) {
        set_error("%s: event timing failed", who); rc = PRE3_E_HIP;
    }
    (void)hipDeviceSynchronize();
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    PRE3_TRY(rc);
    *ms_per_call = ms / reps;
    return PRE3_OK;
}

// the wait of the context forms, as pre3_heading_update with applied_out: the gate word, the result block and the error words behind one wait.
// sta == 5 (a resident frame: a non-finite point in the box) is PRE3_E_NUMERIC with res filled, applied = 0 and a table of zeros.
static int heading_wait(pre3_ctx *c, const char *who, const PlaneJob &j, int32_t *applied_out, pre3_plane_result *res_out, int32_t *draws_out)
{
    int32_t applied = 0;
    PlaneOut o;
    PRE3_HIP(hipMemcpyAsync(c->pinned_stats, c->stats, sizeof(int32_t) * 16, hipMemcpyDeviceToHost, c->stream));
    PRE3_TRY(rows_applied(c, &applied));
    PRE3_HIP(hipMemcpyAsync(&o, c->mem.plane_buf.as<char>() + j.off_out, sizeof o, hipMemcpyDeviceToHost, c->stream));
    if (draws_out) PRE3_HIP(hipMemcpyAsync(draws_out, c->mem.plane_buf.as<char>() + j.off_draws, sizeof(int32_t) * 3 * (size_t)j.n_draw, hipMemcpyDeviceToHost, c->stream));
    PRE3_TRY(stream_drain(c, who));
    if (res_out) plane_result(o, res_out);
    if (o.sta == 5 && draws_out) memset(draws_out, 0, sizeof(int32_t) * 3 * (size_t)j.n_draw);      // (no draw was made: the region holds an earlier call's)
    int rc = stats_words(c);
    if (applied_out) *applied_out = rc == PRE3_OK ? applied : 0;
    if (rc != PRE3_OK) {
        (void)hipMemsetAsync(c->stats + 6, 0, sizeof(int32_t) * 2, c->stream);
        c->mail_host[6] = 0; c->mail_host[7] = 0;
        PRE3_TRY(stream_drain(c, who));
    }
    if (rc == PRE3_OK && o.sta == 5) { set_error("%s: a coordinate inside the box of the resident frame is not finite (sta = 5); x and P are untouched", who); rc = PRE3_E_NUMERIC; }
    return rc;
}

// the fit in front of the heading rows, on the context's stream (DESIGN.md sections 17 and 23).  A resident frame is lent to that stream for the crop
// and reclaimed behind the fit's launches, so that a load that follows cannot overwrite planes that are still being read.
static int heading_impl(const char *who, pre3_ctx *c, PlaneSource s, const int32_t *box, double t, int n_draw, const int32_t *draws, int transpose,
                        int strict_reference, int32_t *applied_out, pre3_plane_result *res_out, const PlaneSeed *sd, int32_t *draws_out)
{
    PlaneJob j;
    PRE3_CHECK(c != nullptr, PRE3_E_ARG, "%s: null context", who);
    PRE3_CHECK(!s.resident || s.frame != nullptr, PRE3_E_ARG, "%s: null handle", who);
    PRE3_TRY(plane_check(who, &s, box, t, n_draw, draws, &j, sd != nullptr));
    PRE3_CHECK(!s.resident || s.device == c->device, PRE3_E_ARG, "%s: the frame is on device %d, the context on device %d", who, s.device, c->device);
    PRE3_CHECK(c->x_valid[PRE3_X_K_K] && c->p_which == PRE3_X_K_K, PRE3_E_STATE,
               "%s: acts on (x_k_k, p_k_k); the covariance buffer holds the prediction (update first)", who);
    EntryScope scope(c); PRE3_TRY(scope.rc);
    PRE3_TRY(plane_reserve(c, who, j.bytes_total));
    const PlaneUpload up = plane_upload(j, s, draws);
    if (up.bytes) {
        void *st = nullptr, *st_dev = nullptr; int slot = 0;
        PRE3_TRY(stage_acquire(c, up.stage_bytes, &st, &st_dev, &slot));
        plane_stage_fill(j, s, draws, up, st);
        PRE3_TRY(launch_pull(c, st, c->mem.plane_buf.as<char>() + up.off, up.bytes, slot));
        PRE3_TRY(stage_release(c, slot));
    }
    if (s.resident) PRE3_TRY(sr_frame_lend(s.frame, c->stream));
    PRE3_TRY(plane_launch(j, c->mem.plane_buf.as<char>(), t, transpose ? 1 : 0, false, c->plane_src, c->stream, sd, s.crop()));
    if (s.resident) PRE3_TRY(sr_frame_reclaim(s.frame, c->stream));
    RowsHeading hd{};
    hd.on = 1; hd.strict = strict_reference ? 1 : 0; hd.src = c->plane_src;
    c->rows_form = 1;
    PRE3_TRY(launch_rows_update(c, nullptr, &hd));
    c->hp_all_valid = false;
    if (applied_out == nullptr && res_out == nullptr && draws_out == nullptr) return PRE3_OK;
    return heading_wait(c, who, j, applied_out, res_out, draws_out);
}

int pre3_heading_from_scan(pre3_ctx *c, int rows, int cols, const double *x_sr, const double *y_sr, const double *z_sr, const int32_t *box, double t,
                           int n_draw, const int32_t *draws, int transpose, int strict_reference, int32_t *applied_out, pre3_plane_result *res_out)
{
    return heading_impl("pre3_heading_from_scan", c, host_planes(0, rows, cols, x_sr, y_sr, z_sr), box, t, n_draw, draws, transpose, strict_reference,
                        applied_out, res_out, nullptr, nullptr);
}

int pre3_heading_from_scan_seeded(pre3_ctx *c, int rows, int cols, const double *x_sr, const double *y_sr, const double *z_sr, const int32_t *box, double t,
                                  int n_draw, uint64_t seed, uint64_t seq, int transpose, int strict_reference, int32_t *draws_out, int32_t *applied_out,
                                  pre3_plane_result *res_out)
{
    const PlaneSeed sd{ seed, seq };
    return heading_impl("pre3_heading_from_scan", c, host_planes(0, rows, cols, x_sr, y_sr, z_sr), box, t, n_draw, nullptr, transpose, strict_reference,
                        applied_out, res_out, &sd, draws_out);
}

int pre3_heading_from_frame(pre3_ctx *c, pre3_sr_frame *f, const int32_t *box, double t, int n_draw, const int32_t *draws, int transpose,
                            int strict_reference, int32_t *applied_out, pre3_plane_result *res_out)
{
    return heading_impl("pre3_heading_from_frame", c, resident_frame(f), box, t, n_draw, draws, transpose, strict_reference, applied_out, res_out, nullptr,
                        nullptr);
}

int pre3_heading_from_frame_seeded(pre3_ctx *c, pre3_sr_frame *f, const int32_t *box, double t, int n_draw, uint64_t seed, uint64_t seq, int transpose,
                                   int strict_reference, int32_t *draws_out, int32_t *applied_out, pre3_plane_result *res_out)
{
    const PlaneSeed sd{ seed, seq };
    return heading_impl("pre3_heading_from_frame", c, resident_frame(f), box, t, n_draw, nullptr, transpose, strict_reference, applied_out, res_out, &sd,
                        draws_out);
}

}  // extern "C"
