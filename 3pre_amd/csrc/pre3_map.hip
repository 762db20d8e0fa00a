// pre3_map.hip -- SURVEY 8(f)-1: map management on the device (map_management.m:27-79), so that P never leaves HBM.
//
// All three operations of the reference are congruences  P <- A P A' (+ D)  with a very sparse A:
//   delete_a_feature.m:47-51                       A = row selection
//   add_a_feature_covariance_inverse_depth.m:83-90  A = [I ; dy_dxv], D = dy_dhd Padd dy_dhd' on the new 6x6 block
//   inversedepth_2_cartesian.m:58-72                A = blkdiag(I, J(3x6), I)
// A is built row by row on the device (k_map_fill: <= 6 non-zeros per row) from a host-made row descriptor list, then
// applied in ONE pass into a second ld x ld buffer that becomes P (k_map_one: out[a][b] = sum_t val[b][t] * T[a][col[b][t]] with
// T[a][c] = sum_t val[a][t] * P[col[a][t]][c] formed on the fly and rounded as a stored T would be; almost every entry is a plain copy
// P[src(a)][src(b)] -- 36 MB read + 36 MB written at N = 500 instead of the two gather passes T = A P, P = T A' of rounds 1-3, which moved
// twice that at half the rate: 53 -> ~17 us per call).  Rows that are plain copies (coefficient 1) reproduce their source bit for bit.
#include <algorithm>
#include <cmath>

#include "pre3_internal.h"
#include "pre3_geomdev.h"
#include "pre3_philox.h"
#include "pre3_vopair.h"
#include "pre3_patch.h"

namespace pre3 {

struct CamM { double f, Cx, Cy, k1, k2; };
constexpr int MAPW = 8;          // ELL width of A
constexpr int FEATW = 64;        // doubles per new feature: y[6], dth_dq[4], dph_dq[4], Nn[36]
constexpr int CONVW = 24;        // doubles per landmark for the conversion: p[3], J[18]

__device__ inline void m_q2r(const double *q, double *R)
{
    double r = q[0], x = q[1], y = q[2], z = q[3];
    R[0] = r * r + x * x - y * y - z * z; R[1] = 2 * (x * y - r * z);           R[2] = 2 * (z * x + r * y);
    R[3] = 2 * (x * y + r * z);           R[4] = r * r - x * x + y * y - z * z; R[5] = 2 * (y * z - r * x);
    R[6] = 2 * (z * x - r * y);           R[7] = 2 * (y * z + r * x);           R[8] = r * r - x * x - y * y + z * z;
}

// hinv_my_version.m:26-53 and the Jacobians of add_a_feature_covariance_inverse_depth.m:29-82, one lane per new feature
__global__ void k_map_new_features(int n_new, const double *__restrict__ uvd, const double *__restrict__ rho0, double std_pxl,
                                   const double *__restrict__ x, CamM cam, double *__restrict__ feat)
{
    // No fma contraction here: where a Jacobian entry cancels exactly (q_wc = (1, 0, 0, 0): d(theta, phi)/dq0 = 0) what is left of it is the rounding
    // residue of the products, and a contracted sum leaves another residue than the reference's plain products and sums -- one ulp of the cancelled
    // terms, which the congruence then multiplies with P[3][c] (tests/test_gpu_map_blocks.py: 218 units of the entry's rounding bound at N = 340).
    // Product by product, in the order of add_a_feature_covariance_inverse_depth.m:54-60, the residue is the reference's.  (One lane per new feature.)
#pragma clang fp contract(off)
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n_new) return;
    const double ud = uvd[2 * f], vd = uvd[2 * f + 1];
    // undistort_fm_my_version.m:27-48
    double xd = (ud - cam.Cx) / cam.f, yd = (vd - cam.Cy) / cam.f;
    double rd = sqrt(xd * xd + yd * yd);
    double ru = rd / (1 + cam.k1 * rd * rd + cam.k2 * rd * rd * rd * rd);
    for (int k = 0; k < 10; ++k) {
        double f1 = ru + cam.k1 * ru * ru * ru + cam.k2 * ru * ru * ru * ru * ru - rd;
        double f1p = 1 + 3 * cam.k1 * ru * ru + 5 * cam.k2 * ru * ru * ru * ru;
        ru = ru - f1 / f1p;
    }
    const double Dd = 1 + cam.k1 * ru * ru + cam.k2 * ru * ru * ru * ru;
    const double uu = cam.f * xd / Dd + cam.Cx, vu = cam.f * yd / Dd + cam.Cy;
    double R[9];
    m_q2r(x + 3, R);
    const double hc[3] = { -(cam.Cx - uu) / cam.f, -(cam.Cy - vu) / cam.f, 1.0 };
    double nw[3];
    for (int i = 0; i < 3; ++i) nw[i] = R[i * 3] * hc[0] + R[i * 3 + 1] * hc[1] + R[i * 3 + 2] * hc[2];
    double *o = feat + (size_t)f * FEATW;
    o[0] = x[0]; o[1] = x[1]; o[2] = x[2];
    o[3] = atan2(nw[0], nw[2]); o[4] = atan2(-nw[1], sqrt(nw[0] * nw[0] + nw[2] * nw[2])); o[5] = rho0[f];
    const double Xw = nw[0], Yw = nw[1], Zw = nw[2];
    const double dth[3] = { Zw / (Xw * Xw + Zw * Zw), 0, -Xw / (Xw * Xw + Zw * Zw) };
    const double s2 = Xw * Xw + Yw * Yw + Zw * Zw, sxz = sqrt(Xw * Xw + Zw * Zw);
    const double dph[3] = { (Xw * Yw) / (s2 * sxz), -sxz / s2, (Zw * Yw) / (s2 * sxz) };
    // dRq_times_a_by_dq(q_wc, XYZ_c)  (dRq_times_a_by_dq.m:29-101)
    const double q0 = x[3], qx = x[4], qy = x[5], qz = x[6], a0 = hc[0], a1 = hc[1], a2 = hc[2];
    double dq[12];
    dq[0] = 2 * q0 * a0 - 2 * qz * a1 + 2 * qy * a2;  dq[4] = 2 * qz * a0 + 2 * q0 * a1 - 2 * qx * a2;  dq[8]  = -2 * qy * a0 + 2 * qx * a1 + 2 * q0 * a2;
    dq[1] = 2 * qx * a0 + 2 * qy * a1 + 2 * qz * a2;  dq[5] = 2 * qy * a0 - 2 * qx * a1 - 2 * q0 * a2;  dq[9]  = 2 * qz * a0 + 2 * q0 * a1 - 2 * qx * a2;
    dq[2] = -2 * qy * a0 + 2 * qx * a1 + 2 * q0 * a2; dq[6] = 2 * qx * a0 + 2 * qy * a1 + 2 * qz * a2;  dq[10] = -2 * q0 * a0 + 2 * qz * a1 - 2 * qy * a2;
    dq[3] = -2 * qz * a0 - 2 * q0 * a1 + 2 * qx * a2; dq[7] = 2 * q0 * a0 - 2 * qz * a1 + 2 * qy * a2;  dq[11] = 2 * qx * a0 + 2 * qy * a1 + 2 * qz * a2;
    for (int c = 0; c < 4; ++c) {
        o[6 + c] = dth[0] * dq[c] + dth[1] * dq[4 + c] + dth[2] * dq[8 + c];
        o[10 + c] = dph[0] * dq[c] + dph[1] * dq[4 + c] + dph[2] * dq[8 + c];
    }
    // dy_dhd = [dyprima_dgw * R_wc * dgc_dhu * dhu_dhd , 0 ; 0 0 1],  dhu_dhd = inv(jacob_distor(uvd))
    const double xx = ud - cam.Cx, yy = vd - cam.Cy, f2 = cam.f * cam.f;
    const double r2 = (xx * xx + yy * yy) / f2, r4 = r2 * r2, g = cam.k1 + 2 * cam.k2 * r2, D0 = 1 + cam.k1 * r2 + cam.k2 * r4;
    const double Jd[4] = { D0 + xx * g * (2 * xx / f2), xx * g * (2 * yy / f2), yy * g * (2 * xx / f2), D0 + yy * g * (2 * yy / f2) };
    const double det = Jd[0] * Jd[3] - Jd[1] * Jd[2];
    const double Ji[4] = { Jd[3] / det, -Jd[1] / det, -Jd[2] / det, Jd[0] / det };
    double A[6][3];                         // dy_dhd
    for (int r_ = 0; r_ < 6; ++r_) for (int c = 0; c < 3; ++c) A[r_][c] = 0;
    for (int r_ = 3; r_ < 5; ++r_) {
        const double *dg = r_ == 3 ? dth : dph;
        double t1[3];                       // row * R_wc
        for (int c = 0; c < 3; ++c) t1[c] = dg[0] * R[c] + dg[1] * R[3 + c] + dg[2] * R[6 + c];
        const double t2[2] = { t1[0] / cam.f, t1[1] / cam.f };          // * dgc_dhu
        A[r_][0] = t2[0] * Ji[0] + t2[1] * Ji[2];
        A[r_][1] = t2[0] * Ji[1] + t2[1] * Ji[3];
    }
    A[5][2] = 1;
    const double std_rho = rho0[f] * rho0[f] * 0.01;                    // add_features_inverse_depth.m:41
    const double pd[3] = { std_pxl * std_pxl, std_pxl * std_pxl, std_rho * std_rho };
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) {
            double s = 0;
            for (int t = 0; t < 3; ++t) s += (A[i][t] * pd[t]) * A[j][t];
            o[14 + i * 6 + j] = s;
        }
}

// inversedepth_2_cartesian.m:38-57: linearity index per inverse-depth landmark, plus the point p and the 3x6 Jacobian
template <typename T>
__global__ void k_map_convert_flags(int N, const int32_t *__restrict__ lm_type, const int32_t *__restrict__ lm_off,
                                    const double *__restrict__ x, const T *__restrict__ P, int ld, double threshold,
                                    int32_t *__restrict__ flags, double *__restrict__ conv)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    int flag = 0;
    if (lm_type[i] == PRE3_INVDEPTH) {
        const int o = lm_off[i];
        double p[3], lin, J[18];
        id_to_cartesian(x, o, (double)P[(size_t)(o + 5) * ld + o + 5], p, &lin, J);      // (pre3_geomdev.h: shared with the landmark reader)
        flag = lin < threshold ? 1 : 0;
        double *cv = conv + (size_t)i * CONVW;
        for (int r_ = 0; r_ < 3; ++r_) {
            cv[r_] = p[r_];
            for (int c = 0; c < 6; ++c) cv[3 + r_ * 6 + c] = J[r_ * 6 + c];
        }
    }
    flags[i] = flag;
}

// Row a of A and entry a of the new state from its descriptor (kind, p0, p1):
//   0: copy of old row p0;  1: row p1 (0..5) of new feature p0;  2: row p1 (0..2) of the conversion of landmark p0 (old offset in desc[3a+... see host)
template <typename T>
__global__ void k_map_fill(int n_new, const int32_t *__restrict__ desc, const double *__restrict__ x_old, const double *__restrict__ feat,
                           const double *__restrict__ conv, const int32_t *__restrict__ lm_off_old, int32_t *__restrict__ col,
                           T *__restrict__ val, double *__restrict__ x_new, int32_t *__restrict__ src0)
{
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n_new) return;
    const int kind = desc[3 * a], p0 = desc[3 * a + 1], p1 = desc[3 * a + 2];
    src0[a] = kind == 0 ? p0 : -1;                  // k_map_one: the old row / column a plain copy comes from
    int32_t *cc = col + a * MAPW;
    T *vv = val + a * MAPW;
    for (int t = 0; t < MAPW; ++t) { cc[t] = 0; vv[t] = (T)0; }
    if (kind == 0) {
        cc[0] = p0; vv[0] = (T)1; x_new[a] = x_old[p0];
    } else if (kind == 1) {
        const double *o = feat + (size_t)p0 * FEATW;
        x_new[a] = o[p1];
        if (p1 < 3) { cc[0] = p1; vv[0] = (T)1; }
        else if (p1 < 5) { for (int c = 0; c < 4; ++c) { cc[c] = 3 + c; vv[c] = (T)o[(p1 == 3 ? 6 : 10) + c]; } }
    } else {
        const double *cv = conv + (size_t)p0 * CONVW;
        const int o = lm_off_old[p0];
        x_new[a] = cv[p1];
        for (int c = 0; c < 6; ++c) { cc[c] = o + c; vv[c] = (T)cv[3 + p1 * 6 + c]; }
    }
}

// T = A P : dst[a][j] = sum_t val[a][t] * P[col[a][t]][j]   (a < n_new; zero rows beyond)
template <typename T>
__global__ __launch_bounds__(256) void k_map_rows(int n_new, const int32_t *__restrict__ desc, const int32_t *__restrict__ col,
                                                  const T *__restrict__ val, const T *__restrict__ P, int ld, T *__restrict__ dst)
{
    const int a = blockIdx.y;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ld) return;
    T s = (T)0;
    if (a < n_new) {
        if (desc[3 * a] == 0) s = P[(size_t)col[a * MAPW] * ld + j];          // plain copy row (almost all of them): one load
        else {
#pragma unroll
            for (int t = 0; t < MAPW; ++t) s += val[a * MAPW + t] * P[(size_t)col[a * MAPW + t] * ld + j];
        }
    }
    dst[(size_t)a * ld + j] = s;
}

// P = T A' : dst[a][b] = sum_t val[b][t] * Tm[a][col[b][t]]   (a, b < n_new; zero elsewhere)
template <typename T>
__global__ __launch_bounds__(256) void k_map_cols(int n_new, const int32_t *__restrict__ desc, const int32_t *__restrict__ col,
                                                  const T *__restrict__ val, const T *__restrict__ Tm, int ld, T *__restrict__ dst)
{
    const int a = blockIdx.y;
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= ld) return;
    T s = (T)0;
    if (a < n_new && b < n_new) {
        if (desc[3 * b] == 0) s = Tm[(size_t)a * ld + col[b * MAPW]];
        else {
#pragma unroll
            for (int t = 0; t < MAPW; ++t) s += val[b * MAPW + t] * Tm[(size_t)a * ld + col[b * MAPW + t]];
        }
    }
    dst[(size_t)a * ld + b] = s;
}

// Everything that follows the congruence as riders of the congruence's launch (k_map_one; round 4: it was one copy, two uploads, three fills and the bank gather with two
// stream synchronisations): the new state, the new landmark table, the per-landmark fields cleared (update_features_info.m:30-44), the
// inbox cleared, and the descriptor bank re-laid-out (src[i] = old index of new landmark i, -1: a new landmark, zero descriptor).
// A booked context (pre3_set_book) also re-lays out its book the same way (a new landmark: {0, 0, s, s}) and clears the rescue's visibility record.
struct MapFinish {
    int n_new; const double *x_alt; double *x_kk; int N; const int32_t *types_src, *off_src; int32_t *lm_type, *lm_off; int capN;
    int32_t *has_h, *has_S, *inbox; int inbox_words; const int32_t *src; const double *bank; double *bank_out;
    const int32_t *book; int32_t *book_out; int32_t *book_vis; int book_s;
};
__device__ __forceinline__ void map_finish_block(const MapFinish &f, int t, int nt)
{
    for (int i = t; i < f.n_new; i += nt) f.x_kk[i] = f.x_alt[i];
    for (int i = t; i < f.N; i += nt) { f.lm_type[i] = f.types_src[i]; f.lm_off[i] = f.off_src[i]; }
    for (int i = t; i < f.capN; i += nt) { f.has_h[i] = 0; f.has_S[i] = 0; }
    for (int i = t; i < f.inbox_words; i += nt) f.inbox[i] = 0;
    if (f.bank != nullptr)
        for (int i = t; i < f.N * 128; i += nt) { const int sidx = f.src[i >> 7]; f.bank_out[i] = sidx >= 0 ? f.bank[(size_t)sidx * 128 + (i & 127)] : 0.0; }
    if (f.book_out != nullptr) {
        for (int i = t; i < f.N * 4; i += nt) { const int sidx = f.src[i >> 2]; f.book_out[i] = sidx >= 0 ? f.book[sidx * 4 + (i & 3)] : ((i & 3) < 2 ? 0 : f.book_s); }
        for (int i = t; i < f.capN; i += nt) f.book_vis[i] = 0;
    }
}
__global__ __launch_bounds__(256) void k_map_finish(MapFinish f) { map_finish_block(f, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x); }

// out = A P A' (+ D) in one pass: out[a][b] = sum_t val[b][t] * T[a][col[b][t]],  T[a][c] = sum_t val[a][t] * P[col[a][t]][c] -- the sums of
// k_map_rows / k_map_cols term for term, T rounded to the storage type as the stored intermediate was.  A workgroup writes 8 rows x 1024
// columns; where row and columns are plain copies (src0 >= 0: everything but the few new / converted rows) an entry is one load.
// feat != nullptr: the new features' 6x6 noise blocks (add_a_feature_covariance_inverse_depth.m:88-90, k_map_add_noise) are added here.
template <typename T>
__device__ __forceinline__ T map_tm(const int32_t *__restrict__ col, const T *__restrict__ val, const T *__restrict__ P, int ld, int a, int ka, int c)
{
    if (ka == 0) return P[(size_t)col[a * MAPW] * ld + c];
    T s = (T)0;
#pragma unroll
    for (int t = 0; t < MAPW; ++t) s = ell_fma(val[a * MAPW + t], P[(size_t)col[a * MAPW + t] * ld + c], s);
    return s;
}
// an entry whose row AND column are computed (the new features' own blocks, a converted landmark's block: a few dozen entries per call)
template <typename T>
__device__ __attribute__((noinline)) T map_entry(int a, int b, const int32_t *__restrict__ desc, const int32_t *__restrict__ col, const T *__restrict__ val,
                                                 const T *__restrict__ P, int ld, const double *__restrict__ feat)
{
    const int ka = desc[3 * a];
    T tm[MAPW];                                     // (all 64 loads in flight: the few lanes that come here are the longest chain of the launch)
#pragma unroll
    for (int t = 0; t < MAPW; ++t) tm[t] = map_tm(col, val, P, ld, a, ka, col[b * MAPW + t]);
    T s = (T)0;
#pragma unroll
    for (int t = 0; t < MAPW; ++t) s = ell_fma(val[b * MAPW + t], tm[t], s);
    if (feat != nullptr && ka == 1 && desc[3 * b] == 1 && desc[3 * a + 1] == desc[3 * b + 1])
        s = (T)((double)s + feat[(size_t)desc[3 * a + 1] * FEATW + 14 + desc[3 * a + 2] * 6 + desc[3 * b + 2]]);
    return s;
}
template <typename T>
__global__ __launch_bounds__(256) void k_map_one(int n_new, const int32_t *__restrict__ desc, const int32_t *__restrict__ col, const T *__restrict__ val,
                                                 const int32_t *__restrict__ src0, const T *__restrict__ P, int ld, T *__restrict__ dst,
                                                 const double *__restrict__ feat, int ny, MapFinish fin)
{
    constexpr int RB = 8, CB = 4;                                                     // a workgroup writes RB rows x CB * 256 columns
    // the block rows behind the congruence's own: what follows it (new state, landmark table, cleared fields, inbox, descriptor bank) -- it
    // needs nothing of this launch, so it rides here instead of going out as k_map_finish
    if ((int)blockIdx.y >= ny) { map_finish_block(fin, (((int)blockIdx.y - ny) * gridDim.x + blockIdx.x) * 256 + threadIdx.x, ((int)gridDim.y - ny) * gridDim.x * 256); return; }
    // (ld is a multiple of 128: all RB rows exist.)  Last rows first: the computed rows of an add sit at the end of the state and take a dozen
    // microseconds of dependent loads -- dispatched first they hide behind the copies, dispatched last they were the tail of the launch
    const int a0 = (ny - 1 - (int)blockIdx.y) * RB;
    int sa[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) sa[r] = a0 + r < n_new ? src0[a0 + r] : -2;
    bool rows_plain = true;
#pragma unroll
    for (int r = 0; r < RB; ++r) rows_plain = rows_plain && sa[r] != -1;
    if (rows_plain) {
        // Round 5 -- the common case (workgroup-uniform: no computed row among the RB) at HBM rate: a lane takes FOUR consecutive destination
        // columns.  Behind a deleted landmark their sources are four consecutive columns too, shifted by a multiple of 3 entries: element-aligned
        // only, which a 16-byte global load takes (the hardware needs dword alignment; tools/probe_unaligned.hip), so a run moves as 16-byte loads
        // and aligned 16-byte stores instead of the dword accesses of round 4 (2.9 TB/s).  A lane whose four columns are not such a run (the edge
        // of a deletion, a computed column of a new / converted landmark, the end of the state) takes them one by one, as before.
        typedef T tv4_t __attribute__((ext_vector_type(4), aligned(sizeof(T))));
        typedef T tv4a_t __attribute__((ext_vector_type(4)));
        const int c4 = blockIdx.x * CB * 256 + threadIdx.x * 4;
        if (c4 >= ld) return;
        int sb4[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) sb4[j] = c4 + j < n_new ? src0[c4 + j] : -2;     // -1: a computed column, -2: beyond the new state (zero)
        const bool run = sb4[0] >= 0 && sb4[1] == sb4[0] + 1 && sb4[2] == sb4[0] + 2 && sb4[3] == sb4[0] + 3;
        tv4a_t o[RB];
        if (run) {
            tv4_t t[RB];
#pragma unroll
            for (int r = 0; r < RB; ++r) t[r] = *reinterpret_cast<const tv4_t *>(P + (size_t)(sa[r] >= 0 ? sa[r] : 0) * ld + sb4[0]);
#pragma unroll
            for (int r = 0; r < RB; ++r) o[r] = sa[r] >= 0 ? tv4a_t{ t[r].x, t[r].y, t[r].z, t[r].w } : tv4a_t{ (T)0, (T)0, (T)0, (T)0 };
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (sb4[j] != -1) {
#pragma unroll
                    for (int r = 0; r < RB; ++r) {
                        const T v = P[(size_t)(sa[r] >= 0 ? sa[r] : 0) * ld + (sb4[j] >= 0 ? sb4[j] : 0)];
                        o[r][j] = (sa[r] >= 0 && sb4[j] >= 0) ? v : (T)0;
                    }
                } else {
                    // a computed column (a new feature's, a converted landmark's: a handful of lanes per call): its <= 8 terms for all RB rows at once
                    T vv[MAPW]; int cc[MAPW];
#pragma unroll
                    for (int t = 0; t < MAPW; ++t) { vv[t] = val[(c4 + j) * MAPW + t]; cc[t] = col[(c4 + j) * MAPW + t]; }
#pragma unroll
                    for (int r = 0; r < RB; ++r) {
                        T e = (T)0;
#pragma unroll
                        for (int t = 0; t < MAPW; ++t) e = ell_fma(vv[t], P[(size_t)(sa[r] >= 0 ? sa[r] : 0) * ld + cc[t]], e);
                        o[r][j] = sa[r] >= 0 ? e : (T)0;
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < RB; ++r) *reinterpret_cast<tv4a_t *>(dst + (size_t)(a0 + r) * ld + c4) = o[r];
        return;
    }
    int cb[CB], sb[CB];                                                               // lane-consecutive columns: every access of a wave is one contiguous run
#pragma unroll
    for (int k = 0; k < CB; ++k) {
        cb[k] = (blockIdx.x * CB + k) * 256 + threadIdx.x;
        sb[k] = cb[k] < n_new ? src0[cb[k]] : -2;                                    // -1: a computed column, -2: beyond the new state (zero)
    }
#pragma unroll 1
    for (int r = 0; r < RB; ++r) {
        const int a = a0 + r;
        const int ka = sa[r] == -1 ? desc[3 * a] : 0;
#pragma unroll
        for (int k = 0; k < CB; ++k) {
            if (cb[k] >= ld) continue;
            T e = (T)0;
            if (sa[r] != -2 && sb[k] != -2) {
                if (sb[k] >= 0) e = map_tm(col, val, P, ld, a, ka, sb[k]);           // (a copied row: one load; a computed row: its <= 8 terms, unrolled)
                else if (sa[r] >= 0) {                                               // a computed column of a copied row
#pragma unroll
                    for (int t = 0; t < MAPW; ++t) e = ell_fma(val[cb[k] * MAPW + t], P[(size_t)sa[r] * ld + col[cb[k] * MAPW + t]], e);
                } else e = map_entry(a, cb[k], desc, col, val, P, ld, feat);
            }
            dst[(size_t)a * ld + cb[k]] = e;
        }
    }
}

template <typename T>
__global__ void k_map_add_noise(int n_feat, int first_off, const double *__restrict__ feat, T *__restrict__ P, int ld)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_feat * 36) return;
    const int f = t / 36, i = (t % 36) / 6, j = t % 6;
    const size_t o = (size_t)(first_off + 6 * f + i) * ld + first_off + 6 * f + j;
    P[o] = (T)((double)P[o] + feat[(size_t)f * FEATW + 14 + i * 6 + j]);
}

#define DISPATCH_T(c, expr_f64, expr_f32) do { if ((c)->dtype == PRE3_F64) { expr_f64; } else { expr_f32; } } while (0)

static int ensure_map_buffers(pre3_ctx *c)
{
    if (c->map_ready) return PRE3_OK;
    Group g(c->mem.fixed, c->map_ready);      // complete, or gone with its pointers null: a call after a failed one starts over
    auto bytes = [&](auto **p, size_t b) { return g.dev(p, b ? b : 16, Zero::none()); };      // (none is zeroed: P_alt at N = 2000 is 580 MB)
    PRE3_TRY(bytes(&c->P_alt, (size_t)c->ld * c->ld * c->esz)); PRE3_TRY(bytes(&c->x_alt, sizeof(double) * c->capn));
    PRE3_TRY(bytes(&c->map_col, sizeof(int32_t) * (size_t)c->capn * MAPW)); PRE3_TRY(bytes(&c->map_val, c->esz * (size_t)c->capn * MAPW));
    PRE3_TRY(bytes(&c->map_desc, sizeof(int32_t) * (3 * (size_t)c->capn + 3 * (size_t)c->capN + 16) + sizeof(double) * 3 * (size_t)c->capN + 16));
    PRE3_TRY(bytes(&c->map_feat, sizeof(double) * (size_t)c->capN * (FEATW > CONVW ? FEATW : CONVW)));
    PRE3_TRY(bytes(&c->map_flags, sizeof(int32_t) * c->capN)); PRE3_TRY(bytes(&c->map_src0, sizeof(int32_t) * (size_t)c->ld));
    PRE3_TRY(bytes(&c->map_conv, sizeof(double) * (size_t)c->capN * CONVW));
    g.commit();
    return PRE3_OK;
}
// the map ring's one capacity ([desc | types | off | src | uvd, rho]: ONE upload per call).  Its two blocks are used alternately: a block is written
// again only after the call before last has been consumed, so a call does not end in a stream synchronisation
static size_t map_stage_bytes(const pre3_ctx *c)
{
    return (sizeof(int32_t) * (3 * (size_t)c->capn + 3 * (size_t)c->capN + 16) + sizeof(double) * 3 * (size_t)c->capN + 15) & ~(size_t)15;
}

// apply the state map described by desc (3 ints per new row), then install the new landmark table.  uvd_rho: 3 n_feat doubles ([u v] per new
// feature, then rho0 per feature) for pre3_map_add_inverse_depth, staged with everything else.
static int apply_map(pre3_ctx *c, const std::vector<int32_t> &desc, int n_new, const std::vector<int32_t> &new_types,
                     int n_feat, int first_new_off, const std::vector<int32_t> &lm_src, const double *uvd = nullptr, const double *rho0 = nullptr,
                     double std_pxl = 0.0)
{
    PRE3_CHECK(n_new <= c->capn && (int)new_types.size() <= c->capN, PRE3_E_ARG, "map management: the new map (N=%zu, n=%d) exceeds the context capacity (N=%d, n=%d)",
               new_types.size(), n_new, c->capN, c->capn);
    const int N = (int)new_types.size();
    std::vector<int32_t> off(N ? N : 1);
    int n = 13;
    for (int i = 0; i < N; ++i) { off[i] = n; n += new_types[i] == PRE3_INVDEPTH ? 6 : 3; }
    PRE3_CHECK(n == n_new, PRE3_E_STATE, "map management: internal size mismatch (%d vs %d)", n, n_new);
    // ---- stage: [desc 3 n_new | types N | off N | src N | pad to 8 bytes | uvd 2 n_feat, rho n_feat]
    StageRing &ring = c->mem.map_ring;
    void *st_v = nullptr; int k = 0;
    PRE3_TRY(ring.acquire(map_stage_bytes(c), map_stage_bytes(c), &st_v, &k));
    int32_t *st = static_cast<int32_t *>(st_v);
    const size_t o_types = desc.size(), o_off = o_types + (size_t)N, o_src = o_off + (size_t)N, o_end = (o_src + (size_t)N + 1) & ~(size_t)1;
    memcpy(st, desc.data(), sizeof(int32_t) * desc.size());
    if (N) { memcpy(st + o_types, new_types.data(), sizeof(int32_t) * N); memcpy(st + o_off, off.data(), sizeof(int32_t) * N); memcpy(st + o_src, lm_src.data(), sizeof(int32_t) * N); }
    size_t bytes = sizeof(int32_t) * o_end;
    if (n_feat > 0) {
        double *sd = reinterpret_cast<double *>(st + o_end);
        memcpy(sd, uvd, sizeof(double) * 2 * n_feat); memcpy(sd + 2 * n_feat, rho0, sizeof(double) * n_feat);
        bytes += sizeof(double) * 3 * (size_t)n_feat;
    }
    PRE3_CHECK(bytes <= ring.cap, PRE3_E_ARG, "map management: staging block too small");
    PRE3_TRY(launch_pull(c, st, c->map_desc, bytes, ring.base + k));        // (read over PCIe by the device: no DMA-engine copy; announces itself: no event)
    ring.release(k);
    const int32_t *d_types = c->map_desc + o_types, *d_off = c->map_desc + o_off, *d_src = c->map_desc + o_src;
    if (n_feat > 0) {
        const double *d_uvd = reinterpret_cast<const double *>(c->map_desc + o_end);
        CamM cam{ c->cam.f, c->cam.Cx, c->cam.Cy, c->cam.k1, c->cam.k2 };
        hipLaunchKernelGGL(k_map_new_features, dim3(ceil_div(n_feat, 64)), dim3(64), 0, c->stream, n_feat, d_uvd, d_uvd + 2 * n_feat, std_pxl, c->x_kk, cam, c->map_feat);
    }
    const double *feat = c->map_feat, *conv = c->map_conv;
    DISPATCH_T(c,
        hipLaunchKernelGGL(k_map_fill<double>, dim3(ceil_div(n_new, 256)), dim3(256), 0, c->stream, n_new, c->map_desc, c->x_kk, feat, conv, c->lm.off, c->map_col, (double *)c->map_val, c->x_alt, c->map_src0),
        hipLaunchKernelGGL(k_map_fill<float>, dim3(ceil_div(n_new, 256)), dim3(256), 0, c->stream, n_new, c->map_desc, c->x_kk, feat, conv, c->lm.off, c->map_col, (float *)c->map_val, c->x_alt, c->map_src0));
    // new state, landmark table, cleared per-landmark fields and inbox, re-laid-out descriptor bank: riders of the congruence's launch (or one launch behind the two-pass form); no synchronisation
    const bool with_bank = c->bank != nullptr && c->bank_alt != nullptr && N > 0;
    const bool with_book = c->booked;
    const int fin_work = std::max(std::max(std::max(n_new, (int)(c->inbox_bytes / 4)), with_bank ? N * 128 : 0), with_book ? std::max(4 * N, c->capN) : 0);
    const MapFinish fin{ n_new, c->x_alt, c->x_kk, N, d_types, d_off, c->lm.type, c->lm.off, c->capN, c->lm.has_h, c->lm.has_S, (int32_t *)c->inbox_dev, (int)(c->inbox_bytes / 4),
                         d_src, with_bank ? c->bank : nullptr, c->bank_alt,
                         c->req.book_from ? c->req.book_from : c->book, with_book ? c->book_alt : nullptr, c->book_vis, c->book_s };
    if (knob::map_one_pass()) {
        // one pass into the second buffer, which becomes P
        const int gx = ceil_div(c->ld, 1024), ny = c->ld / 8, fin_rows = std::min(64, ceil_div(ceil_div(fin_work, 256), gx));
        dim3 g1(gx, ny + fin_rows), b(256);
        const double *noise = n_feat > 0 ? feat : nullptr;
        DISPATCH_T(c,
            hipLaunchKernelGGL(k_map_one<double>, g1, b, 0, c->stream, n_new, c->map_desc, c->map_col, (const double *)c->map_val, c->map_src0, (const double *)c->P, c->ld, (double *)c->P_alt, noise, ny, fin),
            hipLaunchKernelGGL(k_map_one<float>, g1, b, 0, c->stream, n_new, c->map_desc, c->map_col, (const float *)c->map_val, c->map_src0, (const float *)c->P, c->ld, (float *)c->P_alt, noise, ny, fin));
        std::swap(c->P, c->P_alt);
    } else {
        dim3 g(ceil_div(c->ld, 256), c->ld), b(256);
        DISPATCH_T(c,
            hipLaunchKernelGGL(k_map_rows<double>, g, b, 0, c->stream, n_new, c->map_desc, c->map_col, (const double *)c->map_val, (const double *)c->P, c->ld, (double *)c->P_alt),
            hipLaunchKernelGGL(k_map_rows<float>, g, b, 0, c->stream, n_new, c->map_desc, c->map_col, (const float *)c->map_val, (const float *)c->P, c->ld, (float *)c->P_alt));
        DISPATCH_T(c,
            hipLaunchKernelGGL(k_map_cols<double>, g, b, 0, c->stream, n_new, c->map_desc, c->map_col, (const double *)c->map_val, (const double *)c->P_alt, c->ld, (double *)c->P),
            hipLaunchKernelGGL(k_map_cols<float>, g, b, 0, c->stream, n_new, c->map_desc, c->map_col, (const float *)c->map_val, (const float *)c->P_alt, c->ld, (float *)c->P));
        if (n_feat > 0) {
            DISPATCH_T(c,
                hipLaunchKernelGGL(k_map_add_noise<double>, dim3(ceil_div(n_feat * 36, 256)), dim3(256), 0, c->stream, n_feat, first_new_off, feat, (double *)c->P, c->ld),
                hipLaunchKernelGGL(k_map_add_noise<float>, dim3(ceil_div(n_feat * 36, 256)), dim3(256), 0, c->stream, n_feat, first_new_off, feat, (float *)c->P, c->ld));
        }
        hipLaunchKernelGGL(k_map_finish, dim3(std::min(1024, ceil_div(fin_work, 256))), dim3(256), 0, c->stream, fin);
    }
    PRE3_HIP(hipGetLastError());
    if (with_bank) std::swap(c->bank, c->bank_alt);
    if (with_book) std::swap(c->book, c->book_alt);
    PRE3_TRY(patch_follow_map(c, N, d_src));       // the patch bank, when there is one: a launch of its own behind the congruence (pre3_patch.hip)
    c->N = N; c->n = n; c->lm_type_host = new_types;
    c->m = 0; c->meas_host.clear(); c->measurements_set = false; c->projected = false; c->innovated = false; c->hp_all_valid = false;
    c->li_from_host = c->hi_from_host = -1; c->li_kernel = c->hi_kernel = false;
    c->x_valid[PRE3_X_K_KM1] = false;
    return PRE3_OK;
}

static int map_precheck(pre3_ctx *c, const char *who)
{
    PRE3_CHECK(c != nullptr, PRE3_E_ARG, "null context");
    PRE3_HIP(hipSetDevice(c->device));
    PRE3_CHECK(c->x_valid[PRE3_X_K_K] && c->p_which == PRE3_X_K_K, PRE3_E_STATE, "%s: needs (x_k_k, p_k_k) on the device (map management runs between steps)", who);
    // (a rows/cols 3..6 pass -- and the HI down-date behind it -- that a marginal reader left pending for the next step goes out first: the map is re-laid out)
    if (c->carry.jn_pending) PRE3_TRY(flush_unless_kept(c));
    return ensure_map_buffers(c);
}

// ---- marginal readers (pre3_get_landmarks / pre3_get_marginal): plots_complete.m:161-237 and inversedepth_2_cartesian.m:36-62 read a few blocks of
// P, not all of it.  Plain gathers plus a small reduction, no waits between workgroups; the results go to a device block and leave in ONE copy.
// PRE3_OPT_PEND_HI: while a HI down-date is pending P stands for P - W~'W~ (PendW); the reading launch subtracts the landmark's / the tile's share of
// W~'W~ itself (in double, as the S_i riders do), and leaves the pending rows pending.
constexpr int LMR_W = 49;        // doubles per landmark: xyz 3 | cov_xyz 9 | cov_native 36 | linearity 1
constexpr int LMR_PER_WG = 4;    // landmarks per 256-thread workgroup: one wave64 each
constexpr int PEND_CHUNK = 128;  // pending rows staged in LDS at a time (k_hi_fused leaves at most 2 x 64)
constexpr int MS_T = 16;         // output tile edge of the index-set reader

template <typename T>
__global__ __launch_bounds__(256) void k_read_landmarks(int first, int count, const int32_t *__restrict__ lm_type, const int32_t *__restrict__ lm_off,
                                                        const double *__restrict__ x, const T *__restrict__ P, int ld,
                                                        const float *__restrict__ pend_W, int pend_ldw, int pend_rows, double *__restrict__ out)
{
    __shared__ float sW[LMR_PER_WG][PEND_CHUNK][6];
    __shared__ double sB[LMR_PER_WG][36];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q = blockIdx.x * LMR_PER_WG + wv;
    const bool valid = q < count;
    const int i = first + (valid ? q : 0);
    const int d = lm_type[i] == PRE3_INVDEPTH ? 6 : 3, o = lm_off[i];
    // lanes 0..35: entry (a, b) of the landmark's own block -- six rows of six contiguous entries (3 x 3 for a Cartesian landmark)
    const int a = lane / 6, b = lane % 6;
    const bool mine = valid && lane < 36 && a < d && b < d;
    const double pv = mine ? (double)P[(size_t)(o + a) * ld + o + b] : 0.0;
    double s = 0.0;
    for (int r0 = 0; r0 < pend_rows; r0 += PEND_CHUNK) {          // (pend_rows is the same for the whole workgroup)
        const int nr = min(PEND_CHUNK, pend_rows - r0);
        __syncthreads();
        for (int t = lane; t < nr * 6; t += 64) {
            const int r = t / 6, cc = t % 6;
            sW[wv][r][cc] = valid && cc < d ? pend_W[(size_t)(r0 + r) * pend_ldw + o + cc] : 0.f;
        }
        __syncthreads();
        if (mine)
            for (int r = 0; r < nr; ++r) s += (double)sW[wv][r][a] * (double)sW[wv][r][b];
    }
    const double v = mine ? pv - s : 0.0;
    if (lane < 36) sB[wv][lane] = v;
    __syncthreads();
    if (!valid) return;
    double *res = out + (size_t)q * LMR_W;
    if (lane < 36) res[12 + lane] = v;
    if (lane != 0) return;
    const double *B = sB[wv];
    if (d == 6) {
        double p[3], lin, J[18], Tm[18];
        id_to_cartesian(x, o, B[35], p, &lin, J);
        for (int r = 0; r < 3; ++r)                                // J * P_ii * J' (inversedepth_2_cartesian.m:58-69 on the landmark's block)
            for (int c = 0; c < 6; ++c) {
                double t = 0.0;
                for (int e = 0; e < 6; ++e) t += J[r * 6 + e] * B[e * 6 + c];
                Tm[r * 6 + c] = t;
            }
        for (int r = 0; r < 3; ++r)
            for (int c = r; c < 3; ++c) {
                double t = 0.0;
                for (int e = 0; e < 6; ++e) t += Tm[r * 6 + e] * J[c * 6 + e];
                res[3 + r * 3 + c] = t; res[3 + c * 3 + r] = t;
            }
        for (int r = 0; r < 3; ++r) res[r] = p[r];
        res[48] = lin;
    } else {
        for (int r = 0; r < 3; ++r) {
            res[r] = x[o + r];
            for (int c = 0; c < 3; ++c) res[3 + r * 3 + c] = B[r * 6 + c];
        }
        res[48] = -1.0;
    }
}

// entry (s, t) of P - W~'W~ straight from global memory (the few entries a pending rows/cols 3..6 pass needs)
template <typename T>
__device__ double pend_entry(const T *__restrict__ P, int ld, const float *__restrict__ W, int ldw, int rows, int s, int t)
{
    double acc = 0.0;
    for (int r = 0; r < rows; ++r) acc += (double)W[(size_t)r * ldw + s] * (double)W[(size_t)r * ldw + t];
    return (double)P[(size_t)s * ld + t] - acc;
}

// entry (a, b) of P after a pending rows/cols 3..6 <- Jn pass (update.m:42-46), value for value as k_jnorm_P stores it (pre3_geom.hip: jn_row,
// the 4 x 4 corner through its double-precision intermediate, the result rounded to T)
template <typename T>
__device__ double jn_entry(const T *__restrict__ P, int ld, const float *__restrict__ W, int ldw, int rows, const double *__restrict__ jn, int a, int b)
{
    const bool ja = a >= 3 && a < 7, jb = b >= 3 && b < 7;
    if (ja && jb) {
        double T1[4];
        for (int t = 0; t < 4; ++t) {
            const double w[4] = { pend_entry(P, ld, W, ldw, rows, 3, 3 + t), pend_entry(P, ld, W, ldw, rows, 4, 3 + t),
                                  pend_entry(P, ld, W, ldw, rows, 5, 3 + t), pend_entry(P, ld, W, ldw, rows, 6, 3 + t) };
            T1[t] = jn_row(jn, a - 3, w);
        }
        return (double)(T)jn_row(jn, b - 3, T1);
    }
    const int r = ja ? a - 3 : b - 3, col = ja ? b : a;
    const double v[4] = { pend_entry(P, ld, W, ldw, rows, 3, col), pend_entry(P, ld, W, ldw, rows, 4, col),
                          pend_entry(P, ld, W, ldw, rows, 5, col), pend_entry(P, ld, W, ldw, rows, 6, col) };
    return (double)(T)jn_row(jn, r, v);
}

// P[idx, idx] (k x k, row-major) and x[idx]: one 16 x 16 output tile per workgroup; the tile's rows and columns of W~ are staged in LDS
template <typename T>
__global__ __launch_bounds__(256) void k_read_marginal(int k, const int32_t *__restrict__ idx, const double *__restrict__ x, const T *__restrict__ P, int ld,
                                                       const float *__restrict__ pend_W, int pend_ldw, int pend_rows, const double *__restrict__ jn,
                                                       double *__restrict__ x_out, double *__restrict__ P_out)
{
    __shared__ float sR[PEND_CHUNK][MS_T], sC[PEND_CHUNK][MS_T + 1];
    const int ty = threadIdx.x / MS_T, tx = threadIdx.x % MS_T;
    const int i0 = blockIdx.y * MS_T, j0 = blockIdx.x * MS_T, i = i0 + ty, j = j0 + tx;
    const int a = idx[i < k ? i : k - 1], b = idx[j < k ? j : k - 1];
    double s = 0.0;
    for (int r0 = 0; r0 < pend_rows; r0 += PEND_CHUNK) {
        const int nr = min(PEND_CHUNK, pend_rows - r0);
        __syncthreads();
        for (int t = threadIdx.x; t < nr * MS_T; t += blockDim.x) {
            const int r = t / MS_T, cc = t % MS_T;
            const float *wr = pend_W + (size_t)(r0 + r) * pend_ldw;
            sR[r][cc] = i0 + cc < k ? wr[idx[i0 + cc]] : 0.f;
            sC[r][cc] = j0 + cc < k ? wr[idx[j0 + cc]] : 0.f;
        }
        __syncthreads();
        for (int r = 0; r < nr; ++r) s += (double)sR[r][ty] * (double)sC[r][tx];
    }
    if (i >= k || j >= k) return;
    if (blockIdx.y == 0 && ty == 0) x_out[j] = x[b];
    const bool jn_ab = jn != nullptr && ((a >= 3 && a < 7) || (b >= 3 && b < 7));
    P_out[(size_t)i * k + j] = jn_ab ? jn_entry(P, ld, pend_W, pend_ldw, pend_rows, jn, a, b) : (double)P[(size_t)a * ld + b] - s;
}

int read_landmarks(pre3_ctx *c, int which, int first, int count, double *xyz, double *cov_xyz, double *cov_native, double *linearity)
{
    if (count <= 0 || (!xyz && !cov_xyz && !cov_native && !linearity)) return PRE3_OK;
    if (!c->lmr_ready) {
        const size_t bytes = sizeof(double) * LMR_W * (size_t)std::max(c->capN, 1);
        Group g(c->mem.fixed, c->lmr_ready);
        PRE3_TRY(g.dev(&c->lmr_dev, bytes, Zero::none())); PRE3_TRY(g.pin(&c->lmr_host, bytes, PIN_DEFAULT));
        g.commit();
    }
    const PendW pw = pend_args(c);
    const double *x = which == PRE3_X_K_K ? c->x_kk : c->x_km1;
    const dim3 g(ceil_div(count, LMR_PER_WG)), blk(256);
    DISPATCH_T(c,
        hipLaunchKernelGGL(k_read_landmarks<double>, g, blk, 0, c->stream, first, count, c->lm.type, c->lm.off, x, (const double *)c->P, c->ld, pw.W, pw.ldw, pw.rows, c->lmr_dev),
        hipLaunchKernelGGL(k_read_landmarks<float>, g, blk, 0, c->stream, first, count, c->lm.type, c->lm.off, x, (const float *)c->P, c->ld, pw.W, pw.ldw, pw.rows, c->lmr_dev));
    PRE3_HIP(hipGetLastError());
    PRE3_HIP(hipMemcpyAsync(c->lmr_host, c->lmr_dev, sizeof(double) * LMR_W * (size_t)count, hipMemcpyDeviceToHost, c->stream));
    PRE3_TRY(stream_drain(c, __func__));
    for (int q = 0; q < count; ++q) {
        const double *r = c->lmr_host + (size_t)q * LMR_W;
        if (xyz) memcpy(xyz + 3 * (size_t)q, r, sizeof(double) * 3);
        if (cov_xyz) memcpy(cov_xyz + 9 * (size_t)q, r + 3, sizeof(double) * 9);
        if (cov_native) memcpy(cov_native + 36 * (size_t)q, r + 12, sizeof(double) * 36);
        if (linearity) linearity[q] = r[48];
    }
    return PRE3_OK;
}

int read_marginal(pre3_ctx *c, int which, int k, const int32_t *idx, const double *jn, double *x_out, double *P_out)
{
    if (k <= 0 || (!x_out && !P_out)) return PRE3_OK;
    const size_t o_x = ((size_t)k * sizeof(int32_t) + 15) & ~(size_t)15, o_P = o_x + sizeof(double) * (size_t)k;
    const size_t bytes = o_P + sizeof(double) * (size_t)k * (size_t)k;
    // (both grow with k; the call before this one has drained the stream)
    PRE3_TRY(c->mem.mset_dev.reserve(bytes, bytes, Zero::none())); PRE3_TRY(c->mem.mset_host.reserve(bytes, bytes, PIN_DEFAULT));
    unsigned char *hb = c->mem.mset_host.as<unsigned char>(), *db = c->mem.mset_dev.as<unsigned char>();
    memcpy(hb, idx, sizeof(int32_t) * (size_t)k);
    PRE3_HIP(hipMemcpyAsync(db, hb, sizeof(int32_t) * (size_t)k, hipMemcpyHostToDevice, c->stream));
    const PendW pw = pend_args(c);
    const double *x = which == PRE3_X_K_K ? c->x_kk : c->x_km1;
    const dim3 g(ceil_div(k, MS_T), ceil_div(k, MS_T)), blk(MS_T * MS_T);
    const int32_t *d_idx = reinterpret_cast<const int32_t *>(db);
    double *d_x = reinterpret_cast<double *>(db + o_x), *d_P = reinterpret_cast<double *>(db + o_P);
    DISPATCH_T(c,
        hipLaunchKernelGGL(k_read_marginal<double>, g, blk, 0, c->stream, k, d_idx, x, (const double *)c->P, c->ld, pw.W, pw.ldw, pw.rows, jn, d_x, d_P),
        hipLaunchKernelGGL(k_read_marginal<float>, g, blk, 0, c->stream, k, d_idx, x, (const float *)c->P, c->ld, pw.W, pw.ldw, pw.rows, jn, d_x, d_P));
    PRE3_HIP(hipGetLastError());
    const size_t back = P_out ? bytes - o_x : o_P - o_x;          // x and P are contiguous: one copy
    PRE3_HIP(hipMemcpyAsync(hb + o_x, db + o_x, back, hipMemcpyDeviceToHost, c->stream));
    PRE3_TRY(stream_drain(c, __func__));
    if (x_out) memcpy(x_out, hb + o_x, sizeof(double) * (size_t)k);
    if (P_out) memcpy(P_out, hb + o_P, sizeof(double) * (size_t)k * (size_t)k);
    return PRE3_OK;
}


// ---- map policy (pre3_map_policy): delete_features.m:31-49, update_features_info.m:30-44 and the walk of
// initialize_features.m:110-142 -> initialize_a_feature_sift_3.m:72-138 on the device.  Three launches, none waits on another workgroup:
//   k_policy_lm        one lane per landmark: IC stamp, deletion rule, counters, projection of every survivor at x_k_k (a converted landmark as the
//                      Cartesian point the conversion writes)
//   k_policy_prefilter one workgroup per candidate: the box test against every visible survivor (exact: an addition does not move the map)
//   k_policy_walk      ONE wave: compaction, measured, the target, then the candidates in the caller's order, each unblocked one tested only
//                      against the features accepted before it (ballot), the accepted ones projected at x_k_k; results into mapped host memory
constexpr int POL_HDR = 8;           // result block: measured, T, examined, N after, n_del, n_acc, n_surv, pad | del[capN] | acc[K] | conv[capN]
constexpr double POL_SEMI_U = 15.0, POL_SEMI_V = 10.0;     // initialize_a_feature_sift_3.m:58-60: [60,40]/2/2

struct PolicyArgs {
    int N, K, step, min_features, strict, capN;
    const int32_t *type, *off, *ic, *li, *hi, *has_h, *vis, *conv_flags;
    const double *conv, *x; CamD cam;
    const int32_t *book;                // [N][4] as it stands
    int32_t *book_new;                  // [N][4] the survivors' updated counters (scratch: apply_map re-lays them out; the book itself is untouched until then)
    int32_t *del, *mh, *pvis; double *puv;          // per landmark
    const double *cand;                 // [K][2] distorted pixels, then rho[K]
    int32_t *blocked;                   // [K]
    int32_t *res;                       // the result block (device address of mapped pinned memory)
    // pre3_map_policy_frames_seeded; all null in the other entry points.  k_real: K above is the LAYOUT count (grids, the offset
    // of rho in cand, the place of conv behind acc in res) and min(*k_real, K) candidates exist.  The walk then leaves each accepted candidate's
    // (u, v, rho) in acc_uvr (mapped host memory, 3 doubles each) and the row of prev's keypoint block it came from in acc_row.
    const int32_t *k_real;
    double *acc_uvr; int32_t *acc_row;
    const int32_t *order; const double *match;      // drawn position -> candidate; candidate -> 1-based kept position (2 doubles per candidate)
};

__device__ __forceinline__ int pol_count(const PolicyArgs &a) { return a.k_real != nullptr ? max(0, min(*a.k_real, a.K)) : a.K; }

__device__ __forceinline__ bool pol_in_box(double pu, double pv, double cu, double cv, int strict)
{
    // initialize_a_feature_sift_3.m:80-98: search_region_center = (UV(c,2), UV(c,1)) is compared with uv_pred(1,:) +- 15 and uv_pred(2,:) +- 10
    // (quirk Q14: u against the candidate's v); strict = 0 compares u with u and v with v
    const double bu = strict ? cv : cu, bv = strict ? cu : cv;
    return pu > bu - POL_SEMI_U && pu < bu + POL_SEMI_U && pv > bv - POL_SEMI_V && pv < bv + POL_SEMI_V;
}

__global__ __launch_bounds__(64) void k_policy_lm(PolicyArgs a)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.N) return;
    const int32_t *b = a.book + 4 * i;
    int32_t *nb = a.book_new + 4 * i;
    const int tp = b[0], tm = b[1], init = b[2];
    const int lv = a.ic[i] ? a.step - 1 : b[3];                      // matching_sift_based.m:133: last frame's IC matches were visible at step - 1
    // delete_features.m:31-49, on the counters as they stand; the N > 20 gate on the map before deletion
    const bool del = ((double)tm < 0.5 * (double)tp && tp > 5) || (a.step - init > 20) || (a.N > 20 && a.step - lv > 20);
    a.del[i] = del ? 1 : 0;
    if (del) { a.mh[i] = 0; a.pvis[i] = 0; return; }
    // update_features_info.m:30-44: times_predicted += ~isempty(h) (the IC search's projection, or the rescue's: has_h || the recorded visibility)
    const int pred = (a.has_h[i] || (a.vis != nullptr && a.vis[i])) ? 1 : 0, meas = (a.li[i] || a.hi[i]) ? 1 : 0;
    nb[0] = tp + pred; nb[1] = tm + meas; nb[2] = init; nb[3] = lv;
    a.mh[i] = meas;
    // predict_camera_measurements at x_k_k (initialize_a_feature_sift_3.m:72-76), on the map as inversedepth_2_cartesian leaves it
    const bool cv = a.conv_flags[i] != 0;
    const double *y = cv ? a.conv + (size_t)i * CONVW : a.x + a.off[i];
    double zi[2] = { 0, 0 }, hc[14], hl[12];
    bool fresh = false;
    (void)project_core(cv ? PRE3_CARTESIAN : a.type[i], a.x, y, a.cam, 0, nullptr, zi, fresh, hc, hl);
    a.pvis[i] = fresh ? 1 : 0;
    a.puv[2 * i] = zi[0]; a.puv[2 * i + 1] = zi[1];
}

__global__ __launch_bounds__(256) void k_policy_prefilter(PolicyArgs a)
{
    const int c = blockIdx.x;
    if (c >= pol_count(a)) return;                                          // (the whole workgroup)
    const double cu = a.cand[2 * c], cv = a.cand[2 * c + 1];
    int hit = 0;
    for (int j = threadIdx.x; j < a.N; j += blockDim.x)
        hit |= (a.pvis[j] && pol_in_box(a.puv[2 * j], a.puv[2 * j + 1], cu, cv, a.strict)) ? 1 : 0;
    hit = __syncthreads_or(hit);
    if (threadIdx.x == 0) a.blocked[c] = hit;
}

// hinv_my_version.m:26-53 (the geometry of k_map_new_features) and its projection at x_k_k: the h the reference's next attempt sees for it
__device__ __noinline__ bool pol_new_feature_h(double ud, double vd, double rho, const double *x, const CamD &cam, double zi[2])
{
    double xd = (ud - cam.Cx) / cam.f, yd = (vd - cam.Cy) / cam.f;
    double rd = sqrt(xd * xd + yd * yd);
    double ru = rd / (1 + cam.k1 * rd * rd + cam.k2 * rd * rd * rd * rd);
    for (int k = 0; k < 10; ++k) {
        double f1 = ru + cam.k1 * ru * ru * ru + cam.k2 * ru * ru * ru * ru * ru - rd;
        double f1p = 1 + 3 * cam.k1 * ru * ru + 5 * cam.k2 * ru * ru * ru * ru;
        ru = ru - f1 / f1p;
    }
    const double Dd = 1 + cam.k1 * ru * ru + cam.k2 * ru * ru * ru * ru;
    const double uu = cam.f * xd / Dd + cam.Cx, vu = cam.f * yd / Dd + cam.Cy;
    double R[9];
    m_q2r(x + 3, R);
    const double hcv[3] = { -(cam.Cx - uu) / cam.f, -(cam.Cy - vu) / cam.f, 1.0 };
    double nw[3];
    for (int i = 0; i < 3; ++i) nw[i] = R[i * 3] * hcv[0] + R[i * 3 + 1] * hcv[1] + R[i * 3 + 2] * hcv[2];
    const double y[6] = { x[0], x[1], x[2], atan2(nw[0], nw[2]), atan2(-nw[1], sqrt(nw[0] * nw[0] + nw[2] * nw[2])), rho };
    double hc[14], hl[12];
    bool fresh = false;
    (void)project_core(PRE3_INVDEPTH, x, y, cam, 0, nullptr, zi, fresh, hc, hl);
    return fresh;
}

constexpr int POL_MAX_FEATURES = 1024;     // min_features cap: the accepted features' h live in LDS
__global__ __launch_bounds__(64) void k_policy_walk(PolicyArgs a)
{
    __shared__ double s_hu[POL_MAX_FEATURES], s_hv[POL_MAX_FEATURES];
    __shared__ int s_newvis;
    const int lane = threadIdx.x;
    int32_t *r_del = a.res + POL_HDR, *r_acc = r_del + a.capN, *r_conv = r_acc + a.K;
    // survivors in order, measured (map_management.m:37-40: LI || HI of last frame, survivors only), conversion flags of the survivors
    int n_del = 0, measured = 0;
    for (int base = 0; base < a.N; base += 64) {
        const int i = base + lane;
        const int d = i < a.N ? a.del[i] : 0;
        const unsigned long long bm = __ballot(d);
        if (d) r_del[n_del + __popcll(bm & ((1ull << lane) - 1ull))] = i;
        n_del += __popcll(bm);
        measured += __popcll(__ballot(i < a.N && !d && a.mh[i]));
        if (i < a.N) r_conv[i] = d ? 0 : a.conv_flags[i];
    }
    const int n_surv = a.N - n_del;
    // map_management.m:58-66; quirk Q13 (initialize_features.m:127-129 + :138-140 count one SIFT feature twice): ceil(T / 2) additions
    const int T = measured == 0 ? a.min_features : max(0, a.min_features - measured);
    const int goal = min(a.strict ? (T + 1) / 2 : T, a.capN - n_surv);      // (additions stop at the capacity: stats[3] shows it)
    int n_acc = 0, nh = 0, examined = 0;
    const int K = pol_count(a);                                             // (a.K stays the layout: r_conv above, rho below)
    for (int c0 = 0; c0 < K && n_acc < goal; c0 += 64) {
        const int cl = c0 + lane;
        const int blk = cl < K ? a.blocked[cl] : 1;
        const double u = cl < K ? a.cand[2 * cl] : 0.0, v = cl < K ? a.cand[2 * cl + 1] : 0.0;
        for (int k = 0; k < 64 && c0 + k < K && n_acc < goal; ++k) {
            examined = c0 + k + 1;
            if (__shfl(blk, k)) continue;                                   // a survivor of the map is in its box
            const double cu = __shfl(u, k), cv = __shfl(v, k);
            int hit = 0;
            for (int j = lane; j < nh; j += 64) hit |= pol_in_box(s_hu[j], s_hv[j], cu, cv, a.strict) ? 1 : 0;
            if (__any(hit)) continue;                                       // ... or a feature this walk has added
            if (lane == 0) {
                r_acc[n_acc] = c0 + k;
                double zi[2];
                const double rho = a.cand[2 * a.K + c0 + k];
                if (a.acc_uvr != nullptr) {                                 // n_acc < goal <= POL_MAX_FEATURES
                    a.acc_uvr[3 * n_acc] = cu; a.acc_uvr[3 * n_acc + 1] = cv; a.acc_uvr[3 * n_acc + 2] = rho;
                    a.acc_row[n_acc] = (int)a.match[2 * (size_t)a.order[c0 + k]] - 1;
                }
                const bool vis = pol_new_feature_h(cu, cv, rho, a.x, a.cam, zi);
                if (vis) { s_hu[nh] = zi[0]; s_hv[nh] = zi[1]; }
                s_newvis = vis ? 1 : 0;
            }
            __syncthreads();
            nh += s_newvis; ++n_acc;
            __syncthreads();
        }
    }
    if (lane == 0) {
        a.res[0] = measured; a.res[1] = T; a.res[2] = examined; a.res[3] = n_surv + n_acc;
        a.res[4] = n_del; a.res[5] = n_acc; a.res[6] = n_surv; a.res[7] = 0;
    }
}

// the rescue's visibility record: has_h (the IC search's projection at x_k_km1) || visible at the post-LI x_k_k (rescue_hi_inliers.m:32 projects
// every landmark there and keeps stale h for the ones it cannot see, quirk Q7)
__global__ __launch_bounds__(64) void k_book_vis(int N, const int32_t *__restrict__ type, const int32_t *__restrict__ off, const double *__restrict__ x,
                                                 CamD cam, const int32_t *__restrict__ has_h, int32_t *__restrict__ vis)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    double zi[2] = { 0, 0 }, hc[14], hl[12];
    bool fresh = false;
    (void)project_core(type[i], x, x + off[i], cam, 0, nullptr, zi, fresh, hc, hl);
    vis[i] = (has_h[i] || fresh) ? 1 : 0;
}

// initialize_features.m:95-99 on the device (pre3_map_policy_frames_seeded): candidate c is prev's kept keypoint match[0][c] - 1.  One lane per
// c < pnum writes the [Kcap][2] | rho[Kcap] block k_cand_keys / k_cand_rank read and raises the header flags the host looks at behind the call's one
// wait: a pixel that is not finite, a rho that is not finite and positive (gate 0 keeps a keypoint whose y or z is NaN), a descriptor entry outside
// the bounds of pre3_set_descriptors' check (finite, |x| <= 2^60, no non-zero |x| < 2^-40), a match naming a keypoint that does not exist (clamped).
// Each lane stores its bits to its own word flags[c] -- one writer per slot, no atomics; the words come back behind match in the same transfer and the
// host ORs them.
__global__ __launch_bounds__(64) void k_fc_gather(int Kcap, int n1, int ldf, const double *__restrict__ frm, const double *__restrict__ rho,
                                                  const double *__restrict__ des, const double *__restrict__ match, const VoPairHeader *__restrict__ hdr,
                                                  double *__restrict__ raw, int32_t *__restrict__ flags)
{
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= min(hdr->pnum, Kcap)) return;
    int k1 = (int)match[2 * (size_t)c] - 1, bad = 0;
    if (k1 < 0 || k1 >= n1) { bad |= FC_BAD_INDEX; k1 = min(max(k1, 0), n1 - 1); }
    const double u = frm[(size_t)k1 * ldf], v = frm[(size_t)k1 * ldf + 1], r = rho[k1];
    if (!(isfinite(u) && isfinite(v))) bad |= FC_BAD_PIXEL;
    if (!(isfinite(r) && r > 0.0)) bad |= FC_BAD_RHO;
    const double *d = des + (size_t)k1 * DESC_DIM;
    int db = 0;
    for (int q = 0; q < DESC_DIM; ++q) {
        const double ax = fabs(d[q]);
        db |= (int)!(ax <= 0x1p60) | ((int)(ax != 0.0) & (int)(ax < 0x1p-40));
    }
    if (db) bad |= FC_BAD_DESC;
    raw[2 * (size_t)c] = u; raw[2 * (size_t)c + 1] = v; raw[2 * (size_t)Kcap + c] = r;
    flags[c] = bad;
}

static CamD cam_d(const pre3_ctx *c) { return CamD{ c->cam.f, c->cam.Cx, c->cam.Cy, c->cam.k1, c->cam.k2, c->cam.nRows, c->cam.nCols }; }

int launch_book_vis(pre3_ctx *c)
{
    hipLaunchKernelGGL(k_book_vis, dim3(ceil_div(c->N, 64)), dim3(64), 0, c->stream, c->N, c->lm.type, c->lm.off, c->x_kk, cam_d(c), c->lm.has_h, c->book_vis);
    PRE3_HIP(hipGetLastError());
    return PRE3_OK;
}

static int ensure_book(pre3_ctx *c)
{
    if (c->book_ready) return PRE3_OK;
    const size_t b4 = sizeof(int32_t) * 4 * (size_t)c->capN, b1 = sizeof(int32_t) * (size_t)c->capN;
    Group g(c->mem.fixed, c->book_ready);
    PRE3_TRY(g.dev(&c->book, b4, Zero::none())); PRE3_TRY(g.dev(&c->book_alt, b4, Zero::none())); PRE3_TRY(g.dev(&c->book_vis, b1, Zero::none()));
    g.commit();
    return PRE3_OK;
}

// a context's first booking starts from zero counters and an empty visibility record
static int start_book(pre3_ctx *c)
{
    PRE3_TRY(ensure_book(c));
    if (!c->booked) {
        PRE3_HIP(hipMemsetAsync(c->book, 0, sizeof(int32_t) * 4 * (size_t)c->capN, c->stream));
        PRE3_HIP(hipMemsetAsync(c->book_vis, 0, sizeof(int32_t) * (size_t)c->capN, c->stream));
        c->booked = true;
    }
    return PRE3_OK;
}

}  // namespace pre3

using namespace pre3;

// The composition of pre3_map_management with the conversion flags already known (flags[i]: the conversion of old landmark i, its points and
// Jacobians in c->map_conv): pre3_map_management after k_map_convert_flags, pre3_map_policy with the flags its own launches produced.
// always: apply the (identity) map even when nothing changes -- the policy's book and cleared fields go through it.
static int map_compose(pre3_ctx *c, int n_del, const int32_t *del_idx, std::vector<int32_t> &flags, int32_t *converted_out,
                       int n_new, const double *uvd, double std_pxl, const double *initial_rho, bool always)
{
    const int N = c->N;
    std::vector<int32_t> desc, types, src;
    desc.reserve(3 * (size_t)(c->n + 6 * n_new)); types.reserve(N + n_new); src.reserve(N + n_new);
    for (int i = 0; i < 13; ++i) { desc.push_back(0); desc.push_back(i); desc.push_back(0); }
    int d = 0, off = 13, n_out = 13;
    bool any = always || n_del > 0 || n_new > 0;
    for (int i = 0; i < N; ++i) {
        const int dim = c->lm_type_host[i] == PRE3_INVDEPTH ? 6 : 3;
        if (d < n_del && del_idx[d] == i) { ++d; off += dim; flags[i] = 0; continue; }
        if (flags[i]) {
            for (int q = 0; q < 3; ++q) { desc.push_back(2); desc.push_back(i); desc.push_back(q); }
            types.push_back(PRE3_CARTESIAN); n_out += 3; any = true;
        } else {
            for (int q = 0; q < dim; ++q) { desc.push_back(0); desc.push_back(off + q); desc.push_back(0); }
            types.push_back(c->lm_type_host[i]); n_out += dim;
        }
        src.push_back(i);
        off += dim;
    }
    if (converted_out) for (int i = 0; i < N; ++i) converted_out[i] = flags[i];
    if (!any) return PRE3_OK;
    const int first_new_off = n_out;
    for (int f = 0; f < n_new; ++f) {
        for (int q = 0; q < 6; ++q) { desc.push_back(1); desc.push_back(f); desc.push_back(q); }
        types.push_back(PRE3_INVDEPTH); src.push_back(-1); n_out += 6;
    }
    return apply_map(c, desc, n_out, types, n_new, first_new_off, src, uvd, initial_rho, std_pxl);
}



extern "C" {

int pre3_get_map(pre3_ctx *c, int32_t *lm_type_out)
{
    if (!c) return PRE3_E_ARG;
    if (lm_type_out) for (int i = 0; i < c->N; ++i) lm_type_out[i] = c->lm_type_host[i];
    return c->N;
}

int pre3_map_delete(pre3_ctx *c, int n_del, const int32_t *del_idx)
{
    PRE3_TRY(map_precheck(c, "pre3_map_delete"));
    PRE3_CHECK(n_del >= 0 && (n_del == 0 || del_idx), PRE3_E_ARG, "pre3_map_delete: bad arguments");
    for (int d = 0; d < n_del; ++d)
        PRE3_CHECK(del_idx[d] >= 0 && del_idx[d] < c->N && (d == 0 || del_idx[d] > del_idx[d - 1]), PRE3_E_ARG, "pre3_map_delete: indices must be ascending and in range");
    if (n_del == 0) return PRE3_OK;
    std::vector<int32_t> desc, types, src;
    for (int i = 0; i < 13; ++i) { desc.push_back(0); desc.push_back(i); desc.push_back(0); }
    int d = 0, off = 13;
    for (int i = 0; i < c->N; ++i) {
        const int dim = c->lm_type_host[i] == PRE3_INVDEPTH ? 6 : 3;
        if (d < n_del && del_idx[d] == i) { ++d; off += dim; continue; }
        for (int q = 0; q < dim; ++q) { desc.push_back(0); desc.push_back(off + q); desc.push_back(0); }
        types.push_back(c->lm_type_host[i]); src.push_back(i);
        off += dim;
    }
    return apply_map(c, desc, (int)desc.size() / 3, types, 0, 0, src);
}

int pre3_map_add_inverse_depth(pre3_ctx *c, int n_new, const double *uvd, double std_pxl, const double *initial_rho)
{
    PRE3_TRY(map_precheck(c, "pre3_map_add_inverse_depth"));
    PRE3_CHECK(c->have_cam, PRE3_E_STATE, "pre3_map_add_inverse_depth: camera not set");
    PRE3_CHECK(n_new >= 0 && (n_new == 0 || (uvd && initial_rho)), PRE3_E_ARG, "pre3_map_add_inverse_depth: bad arguments");
    if (n_new == 0) return PRE3_OK;
    PRE3_CHECK(c->N + n_new <= c->capN, PRE3_E_ARG, "pre3_map_add_inverse_depth: %d + %d landmarks exceed the capacity %d", c->N, n_new, c->capN);
    PRE3_CHECK((size_t)n_new * FEATW <= (size_t)c->capN * FEATW, PRE3_E_ARG, "pre3_map_add_inverse_depth: too many new features in one call");
    std::vector<int32_t> desc, types(c->lm_type_host), src;
    for (int i = 0; i < c->N; ++i) src.push_back(i);
    for (int i = 0; i < c->n; ++i) { desc.push_back(0); desc.push_back(i); desc.push_back(0); }
    for (int f = 0; f < n_new; ++f) {
        for (int q = 0; q < 6; ++q) { desc.push_back(1); desc.push_back(f); desc.push_back(q); }
        types.push_back(PRE3_INVDEPTH); src.push_back(-1);
    }
    return apply_map(c, desc, c->n + 6 * n_new, types, n_new, c->n, src, uvd, initial_rho, std_pxl);
}

int pre3_map_inversedepth_2_cartesian(pre3_ctx *c, double thr, int32_t *converted_out)
{
    PRE3_TRY(map_precheck(c, "pre3_map_inversedepth_2_cartesian"));
    const int N = c->N;
    if (N == 0) return PRE3_OK;
    DISPATCH_T(c,
        hipLaunchKernelGGL(k_map_convert_flags<double>, dim3(ceil_div(N, 64)), dim3(64), 0, c->stream, N, c->lm.type, c->lm.off, c->x_kk, (const double *)c->P, c->ld, thr, c->map_flags, c->map_conv),
        hipLaunchKernelGGL(k_map_convert_flags<float>, dim3(ceil_div(N, 64)), dim3(64), 0, c->stream, N, c->lm.type, c->lm.off, c->x_kk, (const float *)c->P, c->ld, thr, c->map_flags, c->map_conv));
    PRE3_HIP(hipGetLastError());
    std::vector<int32_t> flags(N);
    PRE3_TRY(stream_drain(c, __func__));
    PRE3_HIP(hipMemcpy(flags.data(), c->map_flags, sizeof(int32_t) * N, hipMemcpyDeviceToHost));
    if (converted_out) for (int i = 0; i < N; ++i) converted_out[i] = flags[i];
    bool any = false;
    for (int i = 0; i < N; ++i) any |= flags[i] != 0;
    if (!any) return PRE3_OK;
    std::vector<int32_t> desc, types, src;
    for (int i = 0; i < N; ++i) src.push_back(i);
    for (int i = 0; i < 13; ++i) { desc.push_back(0); desc.push_back(i); desc.push_back(0); }
    int off = 13;
    for (int i = 0; i < N; ++i) {
        const int dim = c->lm_type_host[i] == PRE3_INVDEPTH ? 6 : 3;
        if (flags[i]) {
            for (int q = 0; q < 3; ++q) { desc.push_back(2); desc.push_back(i); desc.push_back(q); }
            types.push_back(PRE3_CARTESIAN);
        } else {
            for (int q = 0; q < dim; ++q) { desc.push_back(0); desc.push_back(off + q); desc.push_back(0); }
            types.push_back(c->lm_type_host[i]);
        }
        off += dim;
    }
    return apply_map(c, desc, (int)desc.size() / 3, types, 0, 0, src);
}

// map_management.m:27-79 as ONE call and ONE congruence: delete_features (:33), inversedepth_2_cartesian (:48, convert_threshold < 0: skipped),
// initialize_features' add (:58-66).  All three only select / recombine rows of the OLD state (the new features' Jacobians read the camera
// block, which neither a deletion nor a conversion touches), so their row maps compose into one descriptor list and P makes one pass
// through k_map_one instead of up to three.  converted_out (may be null): per OLD landmark, 1 = converted (a deleted landmark reads 0).
int pre3_map_management(pre3_ctx *c, int n_del, const int32_t *del_idx, double convert_threshold, int32_t *converted_out,
                        int n_new, const double *uvd, double std_pxl, const double *initial_rho)
{
    PRE3_TRY(map_precheck(c, "pre3_map_management"));
    PRE3_CHECK(n_del >= 0 && (n_del == 0 || del_idx), PRE3_E_ARG, "pre3_map_management: bad deletion list");
    for (int d = 0; d < n_del; ++d)
        PRE3_CHECK(del_idx[d] >= 0 && del_idx[d] < c->N && (d == 0 || del_idx[d] > del_idx[d - 1]), PRE3_E_ARG, "pre3_map_management: deletion indices must be ascending and in range");
    PRE3_CHECK(n_new >= 0 && (n_new == 0 || (uvd && initial_rho)), PRE3_E_ARG, "pre3_map_management: bad new-feature arguments");
    PRE3_CHECK(n_new == 0 || c->have_cam, PRE3_E_STATE, "pre3_map_management: camera not set");
    PRE3_CHECK(c->N - n_del + n_new <= c->capN, PRE3_E_ARG, "pre3_map_management: %d - %d + %d landmarks exceed the capacity %d", c->N, n_del, n_new, c->capN);
    const int N = c->N;
    std::vector<int32_t> flags(N ? N : 1, 0);
    if (convert_threshold >= 0 && N > 0) {
        DISPATCH_T(c,
            hipLaunchKernelGGL(k_map_convert_flags<double>, dim3(ceil_div(N, 64)), dim3(64), 0, c->stream, N, c->lm.type, c->lm.off, c->x_kk, (const double *)c->P, c->ld, convert_threshold, c->map_flags, c->map_conv),
            hipLaunchKernelGGL(k_map_convert_flags<float>, dim3(ceil_div(N, 64)), dim3(64), 0, c->stream, N, c->lm.type, c->lm.off, c->x_kk, (const float *)c->P, c->ld, convert_threshold, c->map_flags, c->map_conv));
        PRE3_HIP(hipGetLastError());
        PRE3_TRY(stream_drain(c, __func__));
        PRE3_HIP(hipMemcpy(flags.data(), c->map_flags, sizeof(int32_t) * N, hipMemcpyDeviceToHost));
    }
    return map_compose(c, n_del, del_idx, flags, converted_out, n_new, uvd, std_pxl, initial_rho, false);
}
int pre3_set_book(pre3_ctx *c, int first, int count, const int32_t *book)
{
    PRE3_CHECK(c != nullptr, PRE3_E_ARG, "null context");
    PRE3_CHECK(first >= 0 && count >= 0 && (long long)first + count <= c->N && (count == 0 || book != nullptr), PRE3_E_ARG,
               "pre3_set_book: landmarks %d .. %d outside the map (N=%d)", first, first + count - 1, c->N);
    EntryScope scope(c); PRE3_TRY(scope.rc);
    PRE3_TRY(start_book(c));
    if (count > 0) PRE3_HIP(hipMemcpyAsync(c->book + 4 * (size_t)first, book, sizeof(int32_t) * 4 * (size_t)count, hipMemcpyHostToDevice, c->stream));
    return stream_drain(c, __func__);
}

int pre3_get_book(pre3_ctx *c, int first, int count, int32_t *book_out)
{
    PRE3_CHECK(c != nullptr, PRE3_E_ARG, "null context");
    PRE3_CHECK(c->booked, PRE3_E_STATE, "pre3_get_book: the context has no book (pre3_set_book)");
    PRE3_CHECK(first >= 0 && count >= 0 && (long long)first + count <= c->N && (count == 0 || book_out != nullptr), PRE3_E_ARG,
               "pre3_get_book: landmarks %d .. %d outside the map (N=%d)", first, first + count - 1, c->N);
    EntryScope scope(c); PRE3_TRY(scope.rc);
    if (count > 0) PRE3_HIP(hipMemcpyAsync(book_out, c->book + 4 * (size_t)first, sizeof(int32_t) * 4 * (size_t)count, hipMemcpyDeviceToHost, c->stream));
    return stream_drain(c, __func__);
}

// map_management.m:27-79 with its policy: the decisions on the device (k_policy_lm, k_policy_prefilter, k_policy_walk), ONE host wait for the
// result block, then the composition of pre3_map_management with those lists (one pass over P), the candidates' descriptors and the book rows.
// sd == nullptr: pre3_map_policy, the candidates walked in the caller's order.  sd != nullptr: pre3_map_policy_seeded -- the
// candidates go up in the caller's order, k_cand_keys and k_cand_rank in front of k_policy_prefilter re-lay them in the drawn order, the order comes
// back in the result block and maps the accepted positions to the caller's indices.
struct CandSeed { uint64_t seed, seq; int box_w, box_h; };
// fc != nullptr: pre3_map_policy_frames_seeded -- the candidates are built on the device from two resident frames (k_vp_match,
// k_vp_pairs, k_fc_gather on cur's stream); K is then the cap n1 every buffer, grid and the result block are laid out by, the real count pnum stays in
// the device header and reaches the host with the one wait.  The views have been checked by the caller.
struct FrameCand { pre3_sr_frame *prev, *cur; double thresh; SrFrameView v1, v2; SrKeypointView k1, k2; int32_t *K_out; double *match_out; };

static int cand_box_check(const char *who, int box_w, int box_h)
{
    PRE3_CHECK(box_w > 0 && box_h > 0, PRE3_E_ARG, "%s: box sizes %d x %d must be positive", who, box_w, box_h);
    const CandBox b = cand_box(box_w, box_h);
    PRE3_CHECK(b.su > 0.0 && b.sv > 0.0, PRE3_E_ARG, "%s: box %d x %d gives a zero sigma (round(size / 6))", who, box_w, box_h);
    return PRE3_OK;
}

static int map_policy_impl(const char *who, pre3_ctx *c, int step, int min_features, double convert_threshold, double std_pxl, int strict_reference, int K,
                           const double *cand_uv, const double *cand_xyz, const double *cand_desc, const CandSeed *sd, int32_t *order_out,
                           int32_t *del_out, int32_t *n_del_out, int32_t *accepted_out, int32_t *n_acc_out, int32_t *converted_out, int32_t stats[4],
                           const FrameCand *fc = nullptr)
{
    // ---- every argument and state check before anything is launched: an error leaves the context as it was
    PRE3_CHECK(c != nullptr, PRE3_E_ARG, "null context");
    PRE3_CHECK(K >= 0 && K <= PRE3_POLICY_MAX_CANDIDATES && (K == 0 || fc != nullptr || (cand_uv && cand_xyz)), PRE3_E_ARG,
               "%s: K=%d candidates (at most %d, uv and xyz required)", who, K, PRE3_POLICY_MAX_CANDIDATES);
    PRE3_CHECK(min_features >= 0 && min_features <= POL_MAX_FEATURES, PRE3_E_ARG, "%s: min_features=%d outside 0 .. %d", who, min_features, POL_MAX_FEATURES);
    PRE3_CHECK(std::isfinite(std_pxl) && std::isfinite(convert_threshold), PRE3_E_ARG, "%s: std_pxl and the threshold must be finite", who);
    if (sd) PRE3_TRY(cand_box_check(who, sd->box_w, sd->box_h));
    std::vector<double> rho(fc ? 0 : K);
    for (int k = 0; k < K && !fc; ++k) {
        const double x = cand_xyz[3 * k], y = cand_xyz[3 * k + 1], z = cand_xyz[3 * k + 2];
        rho[k] = 1.0 / sqrt(x * x + y * y + z * z);                 // initialize_a_feature_sift_3.m:116-117
        PRE3_CHECK(std::isfinite(cand_uv[2 * k]) && std::isfinite(cand_uv[2 * k + 1]), PRE3_E_ARG, "%s: candidate %d has a non-finite pixel", who, k);
        PRE3_CHECK(std::isfinite(rho[k]) && rho[k] > 0, PRE3_E_ARG, "%s: candidate %d has a zero or non-finite XYZ", who, k);
    }
    PRE3_CHECK(c->have_cam, PRE3_E_STATE, "%s: camera not set", who);
    PRE3_CHECK(c->x_valid[PRE3_X_K_K] && c->p_which == PRE3_X_K_K, PRE3_E_STATE, "%s: needs (x_k_k, p_k_k) on the device (map management runs between steps)", who);
    PRE3_CHECK(c->booked || c->N == 0, PRE3_E_STATE, "%s: the context has no book (pre3_set_book)", who);
    // ---- a deferred HI update completed, pending work flushed (map_precheck); the book
    EntryScope scope(c); PRE3_TRY(scope.rc);
    PRE3_TRY(map_precheck(c, who));
    PRE3_TRY(start_book(c));
    const int N = c->N;
    // ---- buffers: device scratch [cand 3K | puv 2capN | (seeded: raw 3K | keys K) | del, mh, pvis capN | blocked K], the mapped result block
    // [hdr | del capN | acc K | conv capN | (seeded: order K) | cand 3K]
    const size_t cap = (size_t)std::max(c->capN, 1), Kc = (size_t)std::max(K, 1), Ks = sd ? Kc : 0;
    // (frames: order2 K | acc_row behind blocked on the device; the accepted candidates' (u, v, rho) behind cand in the result block)
    const bool fcq = fc != nullptr && K > 0;                       // K == 0 (no kept keypoint on either side): nothing to match, the plain K = 0 call
    const size_t dev_bytes = sizeof(double) * (3 * Kc + 2 * cap + 4 * Ks) + sizeof(int32_t) * (7 * cap + Kc + (fcq ? Kc + POL_MAX_FEATURES : 0));
    const size_t o_order = POL_HDR + 2 * (size_t)c->capN + (size_t)K;
    const size_t res_words = ((POL_HDR + 2 * cap + Kc + Ks) + 1) & ~(size_t)1;
    const size_t host_bytes = sizeof(int32_t) * res_words + sizeof(double) * 3 * (Kc + (fcq ? POL_MAX_FEATURES : 0));
    // (frames) cur's work block [header | match 2K | flags K | the matcher's partials]; header, match and flags come back in one transfer
    const size_t fo_match = sizeof(VoPairHeader), fo_flags = fo_match + sizeof(double) * 2 * Kc, fo_part = (fo_flags + sizeof(int32_t) * Kc + 15) & ~(size_t)15;
    char *f_dev = nullptr, *f_pin = nullptr;
    if (fcq) PRE3_TRY(sr_frame_pair_work(fc->cur, fo_part + vp_match_part_bytes(K, fc->k2.n_kept), fo_part, (void **)&f_dev, (void **)&f_pin));
    PRE3_TRY(c->mem.pol_dev.reserve(dev_bytes, dev_bytes, Zero::none()));
    bool new_host = false;
    const int rc_host = c->mem.pol_host.reserve(host_bytes, host_bytes, PIN_MAPPED, &new_host);
    if (rc_host != PRE3_OK || new_host) {               // (the typed pointers follow the block, a failed one too)
        c->pol_host = c->mem.pol_host.as<int32_t>(); c->pol_host_dev = nullptr;
        PRE3_TRY(rc_host);
        if (hipHostGetDevicePointer((void **)&c->pol_host_dev, c->pol_host, 0) != hipSuccess) {
            c->mem.pol_host.release(); c->pol_host = c->pol_host_dev = nullptr;
            set_error("%s: the result block has no device address", who); return PRE3_E_HIP;
        }
    }
    double *h_cand = reinterpret_cast<double *>(c->pol_host + res_words);
    for (int k = 0; k < K && !fc; ++k) { h_cand[2 * k] = cand_uv[2 * k]; h_cand[2 * k + 1] = cand_uv[2 * k + 1]; h_cand[2 * K + k] = rho[k]; }
    double *d_cand = c->mem.pol_dev.as<double>(), *d_puv = d_cand + 3 * Kc, *d_raw = d_puv + 2 * cap, *d_keys = d_raw + 3 * Ks;
    int32_t *d_del = reinterpret_cast<int32_t *>(d_keys + Ks), *d_mh = d_del + cap, *d_pvis = d_mh + cap, *d_nbook = d_pvis + cap, *d_blocked = d_nbook + 4 * cap;
    int32_t *d_order2 = fcq ? d_blocked + Kc : nullptr, *d_acc_row = fcq ? d_order2 + Kc : nullptr;
    const int32_t *d_kreal = nullptr;
    if (fcq) {
        // ---- prev lent to cur's stream: the match list and its count (pre3_vo_pair_seeded's launches), the gather; header, match and flags towards the
        // host; then cur lent to the context's stream, which waits for all of it
        hipStream_t fs = fc->v2.stream;
        VoPairHeader *hdr = reinterpret_cast<VoPairHeader *>(f_dev);
        double *d_match = reinterpret_cast<double *>(f_dev + fo_match);
        int32_t *d_flags = reinterpret_cast<int32_t *>(f_dev + fo_flags);
        PRE3_TRY(sr_frame_lend(fc->prev, fs));
        PRE3_HIP(hipMemsetAsync(f_dev, 0, fo_part, fs));
        PRE3_TRY(launch_vp_match(K, fc->k2.n_kept, fc->k1.des, fc->k2.des, fc->thresh, f_dev + fo_part, d_match, hdr, fs));
        hipLaunchKernelGGL(k_fc_gather, dim3(ceil_div(K, 64)), dim3(64), 0, fs, K, K, fc->k1.ldf, fc->k1.frm, fc->k1.rho, fc->k1.des, (const double *)d_match,
                           (const VoPairHeader *)hdr, d_raw, d_flags);
        PRE3_HIP(hipGetLastError());
        PRE3_HIP(hipMemcpyAsync(f_pin, f_dev, fo_part, hipMemcpyDeviceToHost, fs));
        PRE3_TRY(sr_frame_lend(fc->cur, c->stream));
        d_kreal = &hdr->pnum;
    } else if (K > 0) PRE3_HIP(hipMemcpyAsync(sd ? d_raw : d_cand, h_cand, sizeof(double) * 3 * K, hipMemcpyHostToDevice, c->stream));
    // ---- seeded: the keys and their rank re-lay the block in the drawn order (d_raw -> d_cand); the order goes into the result block
    if (sd && K > 0) PRE3_TRY(launch_cand_order(sd->seed, sd->seq, K, sd->box_w, sd->box_h, d_raw, d_keys, c->pol_host_dev + o_order, d_cand, c->stream, d_kreal, d_order2));
    // ---- inversedepth_2_cartesian's flags and points (the same launch pre3_map_management makes: the same linearity numbers)
    if (convert_threshold >= 0 && N > 0) {
        DISPATCH_T(c,
            hipLaunchKernelGGL(k_map_convert_flags<double>, dim3(ceil_div(N, 64)), dim3(64), 0, c->stream, N, c->lm.type, c->lm.off, c->x_kk, (const double *)c->P, c->ld, convert_threshold, c->map_flags, c->map_conv),
            hipLaunchKernelGGL(k_map_convert_flags<float>, dim3(ceil_div(N, 64)), dim3(64), 0, c->stream, N, c->lm.type, c->lm.off, c->x_kk, (const float *)c->P, c->ld, convert_threshold, c->map_flags, c->map_conv));
    } else if (N > 0) PRE3_HIP(hipMemsetAsync(c->map_flags, 0, sizeof(int32_t) * N, c->stream));
    const PolicyArgs pa{ N, K, step, min_features, strict_reference ? 1 : 0, c->capN, c->lm.type, c->lm.off, c->lm.ic, c->lm.li, c->lm.hi, c->lm.has_h, c->book_vis,
                         c->map_flags, c->map_conv, c->x_kk, cam_d(c), c->book, d_nbook, d_del, d_mh, d_pvis, d_puv, d_cand, d_blocked, c->pol_host_dev,
                         d_kreal, fcq ? reinterpret_cast<double *>(c->pol_host_dev + res_words) + 3 * Kc : nullptr, d_acc_row, d_order2,
                         fcq ? reinterpret_cast<const double *>(f_dev + fo_match) : nullptr };
    if (N > 0) hipLaunchKernelGGL(k_policy_lm, dim3(ceil_div(N, 64)), dim3(64), 0, c->stream, pa);
    if (K > 0) {
        if (N > 0) hipLaunchKernelGGL(k_policy_prefilter, dim3(K), dim3(256), 0, c->stream, pa);
        else PRE3_HIP(hipMemsetAsync(d_blocked, 0, sizeof(int32_t) * K, c->stream));
    }
    hipLaunchKernelGGL(k_policy_walk, dim3(1), dim3(64), 0, c->stream, pa);
    PRE3_HIP(hipGetLastError());
    PRE3_TRY(stream_drain(c, who));                                 // the one host wait
    const int32_t *res = c->pol_host, *r_del = res + POL_HDR, *r_acc = r_del + c->capN, *r_conv = r_acc + K;
    const int n_del = res[4], n_acc = res[5], n_surv = res[6];
    // (frames) the real count and the gather's flags arrived with the same wait; K stays the layout of the result block
    int Kr = K, fc_bad = 0;
    if (fcq) {
        const VoPairHeader h = *reinterpret_cast<const VoPairHeader *>(f_pin);
        PRE3_CHECK(h.pnum >= 0 && h.pnum <= K, PRE3_E_HIP, "%s: the device reports %d matches of %d keypoints", who, h.pnum, K);
        Kr = h.pnum;
        const int32_t *fl = reinterpret_cast<const int32_t *>(f_pin + fo_flags);
        for (int k = 0; k < Kr; ++k) fc_bad |= fl[k];
        PRE3_CHECK(!(fc_bad & FC_BAD_INDEX), PRE3_E_HIP, "%s: a match refers to a keypoint that does not exist", who);
        // (the counters reach the book only with the re-layout below: context, book, map and both handles are as they were)
        PRE3_CHECK(!(fc_bad & FC_BAD_PIXEL), PRE3_E_NUMERIC, "%s: a matched keypoint of prev has a non-finite pixel", who);
        PRE3_CHECK(!(fc_bad & FC_BAD_RHO), PRE3_E_NUMERIC, "%s: a matched keypoint of prev has a rho that is not finite and positive (a NaN y or z passes the depth gate)", who);
        PRE3_CHECK(n_acc <= POL_MAX_FEATURES, PRE3_E_HIP, "%s: inconsistent result block", who);
    }
    PRE3_CHECK(n_del >= 0 && n_del <= N && n_acc >= 0 && n_acc <= Kr && n_surv == N - n_del && n_surv + n_acc <= c->capN, PRE3_E_HIP, "%s: inconsistent result block", who);
    std::vector<int32_t> dl(r_del, r_del + n_del), acc(r_acc, r_acc + n_acc), flags(N ? N : 1, 0);
    for (int i = 0; i < N; ++i) flags[i] = r_conv[i];
    int32_t st[4] = { res[0], res[1], res[2], res[3] };
    if (sd) {                                                       // drawn positions -> the caller's candidate indices (stats[2] stays a count of positions)
        const int32_t *r_order = res + o_order;
        for (int a = 0; a < n_acc; ++a) {
            PRE3_CHECK(acc[a] >= 0 && acc[a] < Kr && r_order[acc[a]] >= 0 && r_order[acc[a]] < Kr, PRE3_E_HIP, "%s: inconsistent result block", who);
            acc[a] = r_order[acc[a]];
        }
        if (order_out) for (int k = 0; k < Kr; ++k) order_out[k] = r_order[k];
    }
    std::vector<double> uvd(2 * (size_t)n_acc), rho_acc(n_acc);
    if (fcq) {                                                      // the walk left them in the result block: the host never had the candidates
        const double *uvr = reinterpret_cast<const double *>(c->pol_host + res_words) + 3 * Kc;
        for (int a = 0; a < n_acc; ++a) { uvd[2 * a] = uvr[3 * a]; uvd[2 * a + 1] = uvr[3 * a + 1]; rho_acc[a] = uvr[3 * a + 2]; }
    } else
        for (int a = 0; a < n_acc; ++a) { uvd[2 * a] = cand_uv[2 * acc[a]]; uvd[2 * a + 1] = cand_uv[2 * acc[a] + 1]; rho_acc[a] = rho[acc[a]]; }
    // ---- the state: pre3_map_management's composition with these lists; the book rides along (new landmarks: {0, 0, step - 1, step - 1},
    // initialize_features.m:120 passes step - 1 to add_feature_to_info_vector_my_version_sift.m:42-60)
    // (the counters reach the book only through this re-layout: a failure before it leaves the book as it was)
    const int book_s_before = c->book_s;
    c->book_s = step - 1; c->req.book_from = d_nbook;
    const int rc_map = map_compose(c, n_del, dl.data(), flags, converted_out, n_acc, uvd.data(), std_pxl, rho_acc.data(), true);
    if (rc_map != PRE3_OK) { c->book_s = book_s_before; return rc_map; }
    if (cand_desc != nullptr && n_acc > 0) {                        // initialize_a_feature_sift_3.m:132: the candidate's own descriptor
        std::vector<double> dsc(128 * (size_t)n_acc);
        for (int a = 0; a < n_acc; ++a) memcpy(dsc.data() + 128 * (size_t)a, cand_desc + 128 * (size_t)acc[a], sizeof(double) * 128);
        PRE3_TRY(set_descriptors_impl(c, n_surv, n_acc, dsc.data()));
    }
    if (fcq) {
        // initialize_a_feature_sift_3.m:132 from prev's keypoint block, on the context's stream; then both handles are reclaimed from it, so that a
        // later load or keypoint call cannot overwrite blocks that are still being read
        if (n_acc > 0) PRE3_TRY(set_descriptors_rows_dev(c, n_surv, n_acc, fc->k1.des, d_acc_row, K, !(fc_bad & FC_BAD_DESC)));
        PRE3_TRY(sr_frame_reclaim(fc->prev, c->stream));
        PRE3_TRY(sr_frame_reclaim(fc->cur, c->stream));
        if (fc->match_out) memcpy(fc->match_out, f_pin + fo_match, sizeof(double) * 2 * (size_t)Kr);
    }
    if (fc && fc->K_out) *fc->K_out = Kr;
    if (del_out) for (int d = 0; d < n_del; ++d) del_out[d] = dl[d];
    if (n_del_out) *n_del_out = n_del;
    if (accepted_out) for (int a = 0; a < n_acc; ++a) accepted_out[a] = acc[a];
    if (n_acc_out) *n_acc_out = n_acc;
    if (stats) for (int q = 0; q < 4; ++q) stats[q] = st[q];
    return PRE3_OK;
}

int pre3_map_policy(pre3_ctx *c, int step, int min_features, double convert_threshold, double std_pxl, int strict_reference, int K,
                    const double *cand_uv, const double *cand_xyz, const double *cand_desc, int32_t *del_out, int32_t *n_del_out,
                    int32_t *accepted_out, int32_t *n_acc_out, int32_t *converted_out, int32_t stats[4])
{
    return map_policy_impl("pre3_map_policy", c, step, min_features, convert_threshold, std_pxl, strict_reference, K, cand_uv, cand_xyz, cand_desc, nullptr, nullptr,
                           del_out, n_del_out, accepted_out, n_acc_out, converted_out, stats);
}

int pre3_map_policy_seeded(pre3_ctx *c, int step, int min_features, double convert_threshold, double std_pxl, int strict_reference, int K,
                           const double *cand_uv, const double *cand_xyz, const double *cand_desc, int box_w, int box_h, uint64_t seed, uint64_t seq,
                           int32_t *order_out, int32_t *del_out, int32_t *n_del_out, int32_t *accepted_out, int32_t *n_acc_out, int32_t *converted_out,
                           int32_t stats[4])
{
    const CandSeed sd{ seed, seq, box_w, box_h };
    return map_policy_impl("pre3_map_policy_seeded", c, step, min_features, convert_threshold, std_pxl, strict_reference, K, cand_uv, cand_xyz, cand_desc, &sd,
                           order_out, del_out, n_del_out, accepted_out, n_acc_out, converted_out, stats);
}

// map_management.m:27-79 with initialize_features.m:95-99 in front of it, from two resident frames
int pre3_map_policy_frames_seeded(pre3_ctx *c, pre3_sr_frame *prev, pre3_sr_frame *cur, double thresh, int step, int min_features, double convert_threshold,
                                  double std_pxl, int strict_reference, int box_w, int box_h, uint64_t seed, uint64_t seq, int32_t *K_out, double *match_out,
                                  int32_t *order_out, int32_t *del_out, int32_t *n_del_out, int32_t *accepted_out, int32_t *n_acc_out, int32_t *converted_out,
                                  int32_t stats[4])
{
    const char *who = "pre3_map_policy_frames_seeded";
    PRE3_CHECK(c != nullptr, PRE3_E_ARG, "null context");
    FrameCand fc{};
    fc.prev = prev; fc.cur = cur; fc.thresh = thresh; fc.K_out = K_out; fc.match_out = match_out;
    PRE3_TRY(sr_frame_pair_views(who, prev, cur, thresh, &fc.v1, &fc.v2, &fc.k1, &fc.k2));
    PRE3_CHECK(fc.v1.device == c->device, PRE3_E_ARG, "%s: the frames are on device %d, the context on device %d", who, fc.v1.device, c->device);
    PRE3_CHECK(fc.k1.gate == 0, PRE3_E_ARG, "%s: prev's keypoints went through gate %d; the candidates' rho comes from gate 0 (the depth gate)", who, fc.k1.gate);
    const int K = fc.k2.n_kept > 0 ? fc.k1.n_kept : 0;             // the cap: pnum <= n1; siftmatch against an empty set matches nothing
    const CandSeed sd{ seed, seq, box_w, box_h };
    return map_policy_impl(who, c, step, min_features, convert_threshold, std_pxl, strict_reference, K, nullptr, nullptr, nullptr, &sd, order_out, del_out,
                           n_del_out, accepted_out, n_acc_out, converted_out, stats, &fc);
}

// Weighted_Smpl_wo_replacement.m on its own: the keys and the order of K candidates, stateless, on the pooled device scratch
int pre3_candidate_order(int device, int K, const double *cand_uv, int box_w, int box_h, uint64_t seed, uint64_t seq, int32_t *order_out, double *keys_out)
{
    const char *who = "pre3_candidate_order";
    PRE3_CHECK(K >= 0 && K <= PRE3_POLICY_MAX_CANDIDATES, PRE3_E_ARG, "%s: K=%d candidates (at most %d)", who, K, PRE3_POLICY_MAX_CANDIDATES);
    PRE3_TRY(cand_box_check(who, box_w, box_h));
    if (K == 0) return PRE3_OK;
    PRE3_CHECK(cand_uv != nullptr && order_out != nullptr, PRE3_E_ARG, "%s: null argument", who);
    for (int k = 0; k < 2 * K; ++k) PRE3_CHECK(std::isfinite(cand_uv[k]), PRE3_E_ARG, "%s: candidate %d has a non-finite pixel", who, k / 2);
    PRE3_TRY(select_device(who, device));
    Scratch d;
    PRE3_TRY(d.alloc(sizeof(double) * 3 * (size_t)K + sizeof(int32_t) * (size_t)K));      // [uv 2K | keys K | order K]
    double *d_uv = d.as<double>(), *d_keys = d_uv + 2 * (size_t)K;
    int32_t *d_order = reinterpret_cast<int32_t *>(d_keys + K);
    PRE3_HIP(hipMemcpy(d_uv, cand_uv, sizeof(double) * 2 * (size_t)K, hipMemcpyHostToDevice));
    PRE3_TRY(launch_cand_order(seed, seq, K, box_w, box_h, d_uv, d_keys, d_order, nullptr, 0));
    PRE3_HIP(hipMemcpy(order_out, d_order, sizeof(int32_t) * (size_t)K, hipMemcpyDeviceToHost));                  // (synchronises)
    if (keys_out) PRE3_HIP(hipMemcpy(keys_out, d_keys, sizeof(double) * (size_t)K, hipMemcpyDeviceToHost));
    return PRE3_OK;
}

}  // extern "C"
