// pre3_pnp.h -- the camera pose from n >= 6 correspondences of 3-D points and pixels by EPnP (Moreno-Noguer, Lepetit, Fua: "Accurate Non-Iterative
// O(n) Solution to the PnP Problem", ICCV 2007) as the reference's aux_code/EPnP_matlab/EPnP/efficient_pnp.m:34-175 computes it for kernel dimensions
// 1, 2 and 3 -- the solver mex_files/RANSAC_CALCULATION/RANSAC_CALC_VER2.m:187-191 leaves commented out (pre3_pnp.hip).
//   define_control_points.m, compute_alphas.m      Cw = [e1; e2; e3; 0] (not centred on the data), so Alph = [x, y, z, 1 - x - y - z]
//   compute_M_ver2.m:32-52, kernel_noise.m:19-22   M'M summed point by point (its 78 unique entries), eig(M'M) by a cyclic Jacobi
//   compute_norm_sign_scaling_factor.m:26-61       sc = 1 / (inv(dc'dc) dc'dw); the whole Xc negated if any z < 0
//   efficient_pnp.m:179-205 (getrotT)              R = U V' of svd(sum c_i' w_i), R = -R (the whole matrix) if det(R) < 0, T = ccent' - R wcent'
//   efficient_pnp.m:210-226                        the mean pixel distance, no test on depth
//   compute_constraint_distance_2param_6eq_3unk.m, _3param_6eq_6unk.m, define_distances_btw_control_points.m     the betas of dimensions 2 and 3
// Dimension 4 (:129-169) is not built: its result depends on the basis null() happens to return.  Where the reference would enter it (min(err) > 20
// after dimension 3) the answer is the best of the three with sta = PNP_BEST_OF_THREE.
// Everything here is __host__ __device__ and free of HIP headers: the kernels and a host program (tests/pnp_host_main.cpp) run the same text.  The
// matrices an index chosen at run time reaches (the 12 x 12, its eigenvectors, the 6 x 7 system) are addressed through pointers: LDS in the kernels.
#pragma once
#include <stdint.h>
#include <math.h>

#include "pre3_svd3.h"

#if defined(__HIPCC__)
#define PRE3_PNP_HD __host__ __device__ inline
#else
#define PRE3_PNP_HD inline
#endif

namespace pre3 {

constexpr int PNP_MIN_N = 6;                        // 12 unknowns, two equations a point
constexpr int PNP_MAX_N = 262144;                   // two 144 x 176 frames give at most 25344
constexpr int PNP_MAX_HYP = 700;
constexpr int PNP_THREADS = 256;                    // k_pnp_solve's one workgroup; k_pnp_hyp runs one wave
constexpr int PNP_SWEEPS = 30;
constexpr int PNP_MTM = 78;                         // unique entries of the symmetric 12 x 12
constexpr double PNP_ERR_THRESHOLD = 20.0;          // efficient_pnp.m:37 THRESHOLD_REPROJECTION_ERROR: pixels, whatever its comment says
constexpr double PNP_EPS = 2.220446049250313e-16;   // 2^-52
enum { PNP_NOT_COMPUTED = 0, PNP_OK = 1, PNP_BEST_OF_THREE = 2, PNP_NONFINITE = -1 };

// ---- M'M ------------------------------------------------------------------------------------------------------------------------------------------
PRE3_PNP_HD void pnp_alphas(double x, double y, double z, double a[4]) { a[0] = x; a[1] = y; a[2] = z; a[3] = 1.0 - x - y - z; }

// entry (r, c), r <= c, of the upper triangle, row by row
PRE3_PNP_HD constexpr int pnp_ix(int r, int c) { return r * 12 - r * (r - 1) / 2 + (c - r); }

// acc += the point's two rows of M times themselves: row 1 = [a_j f, 0, a_j du], row 2 = [0, a_j f, a_j dv] for j = 1..4 with du = u0 - u, dv = v0 - v
// (compute_M_ver2.m:42-43).  The entries both rows leave zero are never touched.
PRE3_PNP_HD void pnp_mtm_point(const double a[4], double f, double du, double dv, double acc[PNP_MTM])
{
    double r1[12], r2[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) { r1[3 * j] = a[j] * f; r1[3 * j + 1] = 0.0; r1[3 * j + 2] = a[j] * du; r2[3 * j] = 0.0; r2[3 * j + 1] = a[j] * f; r2[3 * j + 2] = a[j] * dv; }
#pragma unroll
    for (int r = 0; r < 12; ++r)
#pragma unroll
        for (int c = r; c < 12; ++c) {
            const int i = r % 3, l = c % 3;
            if ((i == 0 && l == 1) || (i == 1 && l == 0)) continue;
            if (i == 2 && l == 2) acc[pnp_ix(r, c)] += r1[r] * r1[c] + r2[r] * r2[c];
            else if (i == 0 || l == 0) acc[pnp_ix(r, c)] += r1[r] * r1[c];
            else acc[pnp_ix(r, c)] += r2[r] * r2[c];
        }
}

// the summed triangle as the full matrix A (row-major 12 x 12), and V = I
PRE3_PNP_HD void pnp_mtm_entry(const double *s, int e /* 0..143 */, double *A, double *V)
{
    const int r = e / 12, c = e % 12;
    A[e] = r <= c ? s[pnp_ix(r, c)] : s[pnp_ix(c, r)];
    V[e] = r == c ? 1.0 : 0.0;
}

// ---- the cyclic Jacobi eigensolver of a symmetric 12 x 12: A = V diag(w) V' ---------------------------------------------------------------------
// A sweep is eleven rounds of six disjoint pairs (the round-robin schedule: every pair once a sweep, in a fixed order).  The six rotations of a round
// touch disjoint rows and columns: their angles come from A as the round finds it, then every column pair of A and V turns, then every row pair of A.
// The work of a round is 72 + 72 items of two entries each, which the kernels deal over the lanes; the host walks the same items in order.
PRE3_PNP_HD void pnp_jac_pair(int round, int k, int *p, int *q)
{
    const int a = k == 0 ? 11 : (round + k) % 11, b = k == 0 ? round : (round - k + 11) % 11;
    *p = a < b ? a : b; *q = a < b ? b : a;
}

PRE3_PNP_HD void pnp_jac_angle(double app, double aqq, double apq, double *c, double *s)
{
    if (apq == 0.0) { *c = 1.0; *s = 0.0; return; }
    const double zeta = (aqq - app) / (2.0 * apq);
    const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    *c = 1.0 / sqrt(1.0 + t * t);
    *s = *c * t;
}

// cs[2 k], cs[2 k + 1]: the rotation of pair k of this round
PRE3_PNP_HD void pnp_jac_angle_item(const double *A, int round, int k, double *cs)
{
    int p, q;
    pnp_jac_pair(round, k, &p, &q);
    pnp_jac_angle(A[13 * p], A[13 * q], A[12 * p + q], &cs[2 * k], &cs[2 * k + 1]);
}

// item = 12 k + i: row i of the column pair k, in A and in V
PRE3_PNP_HD void pnp_jac_col_item(double *A, double *V, int round, int item, const double *cs)
{
    const int k = item / 12, i = item % 12;
    int p, q;
    pnp_jac_pair(round, k, &p, &q);
    const double c = cs[2 * k], s = cs[2 * k + 1];
    const double ap = A[12 * i + p], aq = A[12 * i + q], vp = V[12 * i + p], vq = V[12 * i + q];
    A[12 * i + p] = c * ap - s * aq; A[12 * i + q] = s * ap + c * aq;
    V[12 * i + p] = c * vp - s * vq; V[12 * i + q] = s * vp + c * vq;
}

// item = 12 k + j: column j of the row pair k; the entry the rotation annihilates is set to zero
PRE3_PNP_HD void pnp_jac_row_item(double *A, int round, int item, const double *cs)
{
    const int k = item / 12, j = item % 12;
    int p, q;
    pnp_jac_pair(round, k, &p, &q);
    const double c = cs[2 * k], s = cs[2 * k + 1];
    const double ap = A[12 * p + j], aq = A[12 * q + j];
    double np_ = c * ap - s * aq, nq = s * ap + c * aq;
    if (s != 0.0) { if (j == q) np_ = 0.0; if (j == p) nq = 0.0; }
    A[12 * p + j] = np_; A[12 * q + j] = nq;
}

// the off-diagonal Frobenius norm at or below 2^-52 times the diagonal's (a NaN never satisfies it: the sweep count bounds the loop)
PRE3_PNP_HD bool pnp_jac_done(const double *A)
{
    double off = 0.0, dia = 0.0;
    for (int i = 0; i < 12; ++i)
        for (int j = 0; j < 12; ++j) { const double v = A[12 * i + j] * A[12 * i + j]; if (i == j) dia += v; else off += v; }
    return sqrt(off) <= PNP_EPS * sqrt(dia);
}

// the columns of the three smallest eigenvalues, ascending, the lower column first on ties
PRE3_PNP_HD void pnp_order3(const double *A, int32_t ord[3])
{
    for (int t = 0; t < 3; ++t) {
        int best = -1;
        for (int i = 0; i < 12; ++i) {
            bool taken = false;
            for (int s = 0; s < t; ++s) taken = taken || ord[s] == i;
            if (taken) continue;
            if (best < 0 || A[13 * i] < A[13 * best]) best = i;
        }
        ord[t] = best;
    }
}

// eig leaves the sign of a vector open, and where the z < 0 rule meets an Xc of mixed signs (a poor six-point sample) the reference's answer depends
// on it: negating such an Xc leaves it mixed.  So the sign is fixed first: the entry of largest magnitude (the lowest index on ties) is made positive.
PRE3_PNP_HD void pnp_fix_sign(double *V, int col)
{
    int big = 0;
    for (int i = 1; i < 12; ++i) if (fabs(V[12 * i + col]) > fabs(V[12 * big + col])) big = i;
    if (V[12 * big + col] < 0) for (int i = 0; i < 12; ++i) V[12 * i + col] = -V[12 * i + col];
}

// ---- the betas of dimensions 2 and 3 --------------------------------------------------------------------------------------------------------------
PRE3_PNP_HD double pnp_sign(double v) { return v > 0 ? 1.0 : (v < 0 ? -1.0 : 0.0); }

// d = K(3 i : 3 i + 2) - K(3 j : 3 j + 2) for the control-point pair e in the order 12 13 14 23 24 34; K is column `col` of V
PRE3_PNP_HD void pnp_diff(const double *V, int col, int e, double d[3])
{
    const int i = e < 3 ? 0 : (e < 5 ? 1 : 2), j = e < 3 ? e + 1 : (e < 5 ? e - 1 : 3);
    for (int t = 0; t < 3; ++t) d[t] = V[12 * (3 * i + t) + col] - V[12 * (3 * j + t) + col];
}
PRE3_PNP_HD double pnp_dot3(const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
PRE3_PNP_HD double pnp_dsq(int e) { return e == 2 || e >= 4 ? 1.0 : 2.0; }          // define_distances_btw_control_points.m: [2 2 1 2 1 1]'

// efficient_pnp.m:73-82: X2 = beta1 Km1 + beta2 Km2 with Km1 = Km(:, end-1), Km2 = Km(:, end), betas_ = inv(D'D) D' dsq
PRE3_PNP_HD void pnp_dim2(const double *V, const int32_t ord[3], double X[12])
{
    const int c1 = ord[1], c2 = ord[0];
    double N[6] = { 0, 0, 0, 0, 0, 0 } /* 00 01 02 11 12 22 */, r[3] = { 0, 0, 0 };
    for (int e = 0; e < 6; ++e) {
        double d1[3], d2[3];
        pnp_diff(V, c1, e, d1); pnp_diff(V, c2, e, d2);
        const double row[3] = { pnp_dot3(d1, d1), 2 * pnp_dot3(d1, d2), pnp_dot3(d2, d2) };
        N[0] += row[0] * row[0]; N[1] += row[0] * row[1]; N[2] += row[0] * row[2]; N[3] += row[1] * row[1]; N[4] += row[1] * row[2]; N[5] += row[2] * row[2];
        const double w = pnp_dsq(e);
        r[0] += row[0] * w; r[1] += row[1] * w; r[2] += row[2] * w;
    }
    // inv(D'D) by its adjugate
    const double c00 = N[3] * N[5] - N[4] * N[4], c01 = N[2] * N[4] - N[1] * N[5], c02 = N[1] * N[4] - N[2] * N[3];
    const double c11 = N[0] * N[5] - N[2] * N[2], c12 = N[1] * N[2] - N[0] * N[4], c22 = N[0] * N[3] - N[1] * N[1];
    const double det = N[0] * c00 + N[1] * c01 + N[2] * c02;
    const double b0 = (c00 * r[0] + c01 * r[1] + c02 * r[2]) / det, b1 = (c01 * r[0] + c11 * r[1] + c12 * r[2]) / det, b2 = (c02 * r[0] + c12 * r[1] + c22 * r[2]) / det;
    const double beta1 = sqrt(fabs(b0)), beta2 = sqrt(fabs(b2)) * pnp_sign(b1) * pnp_sign(b0);
    for (int i = 0; i < 12; ++i) X[i] = beta1 * V[12 * i + c1] + beta2 * V[12 * i + c2];
}

// efficient_pnp.m:100-112: X3 = beta1 Km1 + beta2 Km2 + beta3 Km3 with Km1 = Km(:, end-2), ..., betas_ = inv(D) dsq solved by elimination with row
// pivoting in w[6][7]
PRE3_PNP_HD void pnp_dim3(const double *V, const int32_t ord[3], double *w, double X[12])
{
    const int c1 = ord[2], c2 = ord[1], c3 = ord[0];
    for (int e = 0; e < 6; ++e) {
        double d1[3], d2[3], d3[3];
        pnp_diff(V, c1, e, d1); pnp_diff(V, c2, e, d2); pnp_diff(V, c3, e, d3);
        w[7 * e] = pnp_dot3(d1, d1); w[7 * e + 1] = 2 * pnp_dot3(d1, d2); w[7 * e + 2] = 2 * pnp_dot3(d1, d3);
        w[7 * e + 3] = pnp_dot3(d2, d2); w[7 * e + 4] = 2 * pnp_dot3(d2, d3); w[7 * e + 5] = pnp_dot3(d3, d3); w[7 * e + 6] = pnp_dsq(e);
    }
    for (int k = 0; k < 6; ++k) {
        int piv = k;
        for (int i = k + 1; i < 6; ++i) if (fabs(w[7 * i + k]) > fabs(w[7 * piv + k])) piv = i;
        if (piv != k) for (int j = 0; j < 7; ++j) { const double t = w[7 * k + j]; w[7 * k + j] = w[7 * piv + j]; w[7 * piv + j] = t; }
        for (int i = k + 1; i < 6; ++i) {
            const double m = w[7 * i + k] / w[7 * k + k];
            for (int j = k; j < 7; ++j) w[7 * i + j] -= m * w[7 * k + j];
        }
    }
    for (int k = 5; k >= 0; --k) {
        double s = w[7 * k + 6];
        for (int j = k + 1; j < 6; ++j) s -= w[7 * k + j] * w[7 * j + 6];
        w[7 * k + 6] = s / w[7 * k + k];
    }
    const double b0 = w[6], b1 = w[13], b2 = w[20], b3 = w[27], b5 = w[41];
    const double beta1 = sqrt(fabs(b0)), beta2 = sqrt(fabs(b3)) * pnp_sign(b1) * pnp_sign(b0), beta3 = sqrt(fabs(b5)) * pnp_sign(b2) * pnp_sign(b0);
    for (int i = 0; i < 12; ++i) X[i] = beta1 * V[12 * i + c1] + beta2 * V[12 * i + c2] + beta3 * V[12 * i + c3];
}

// ---- the passes over the points: what one point adds ----------------------------------------------------------------------------------------------
// Alph(i, :) * C for the control points C (4 x 3, row-major)
PRE3_PNP_HD void pnp_xc(const double a[4], const double C[12], double xc[3])
{
#pragma unroll
    for (int t = 0; t < 3; ++t) xc[t] = a[0] * C[t] + a[1] * C[3 + t] + a[2] * C[6 + t] + a[3] * C[9 + t];
}
PRE3_PNP_HD double pnp_dist3(const double p[3], const double c[3])
{
    const double a = p[0] - c[0], b = p[1] - c[1], d = p[2] - c[2];
    return sqrt(a * a + b * b + d * d);
}
// sc = 1 / (inv(dc'dc) dc'dw), Cc = Cc_ / sc (compute_norm_sign_scaling_factor.m:47-50)
PRE3_PNP_HD void pnp_scale(double cc, double cw, double C[12])
{
    const double sc = 1.0 / ((1.0 / cc) * cw);
#pragma unroll
    for (int i = 0; i < 12; ++i) C[i] = C[i] / sc;
}

// getrotT from M = sum (c_i - ccent)' (w_i - wcent) (row-major) and the two centroids
PRE3_PNP_HD void pnp_getrot(const double M[9], const double ccent[3], const double wcent[3], double R[9], double T[3])
{
    double U[9], sv[3], V[9];
    vo_svd3(M, U, sv, V);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) R[3 * i + j] = U[3 * i] * V[3 * j] + U[3 * i + 1] * V[3 * j + 1] + U[3 * i + 2] * V[3 * j + 2];
    const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
    if (det < 0) {
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = -R[i];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) T[i] = ccent[i] - (R[3 * i] * wcent[0] + R[3 * i + 1] * wcent[1] + R[3 * i + 2] * wcent[2]);
}

// P = A [R, T] with A = [f 0 Cx; 0 f Cy; 0 0 1] (row-major 3 x 4), and the pixel distance of one point under it (efficient_pnp.m:215-225); *zc: the
// camera-frame depth the division uses
PRE3_PNP_HD void pnp_proj_matrix(const double R[9], const double T[3], double f, double Cx, double Cy, double P[12])
{
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const double r0 = c < 3 ? R[c] : T[0], r1 = c < 3 ? R[3 + c] : T[1], r2 = c < 3 ? R[6 + c] : T[2];
        P[c] = f * r0 + Cx * r2; P[4 + c] = f * r1 + Cy * r2; P[8 + c] = r2;
    }
}
PRE3_PNP_HD double pnp_reproj(const double P[12], const double xw[3], double u, double v, double *zc)
{
    const double a = P[0] * xw[0] + P[1] * xw[1] + P[2] * xw[2] + P[3], b = P[4] * xw[0] + P[5] * xw[1] + P[6] * xw[2] + P[7];
    const double c = P[8] * xw[0] + P[9] * xw[1] + P[10] * xw[2] + P[11];
    const double du = u - a / c, dv = v - b / c;
    *zc = c;
    return sqrt(du * du + dv * dv);
}

// ---- the answer -----------------------------------------------------------------------------------------------------------------------------------
PRE3_PNP_HD bool pnp_finite(const double *v, int n)
{
    bool ok = true;
    for (int i = 0; i < n; ++i) ok = ok && isfinite(v[i]);
    return ok;
}
// dimension 3 is entered when the first two are finite and both above the threshold (efficient_pnp.m:98)
PRE3_PNP_HD bool pnp_enters_dim3(double e0, double e1) { return isfinite(e0) && isfinite(e1) && (e0 < e1 ? e0 : e1) > PNP_ERR_THRESHOLD; }
// [min_err, best] = min(err), the first index on ties; sta as the header documents it.  nd: dimensions computed (2 or 3); finite: every err, R and T of them is
PRE3_PNP_HD void pnp_answer(const double err[3], int nd, bool finite, int32_t *best, int32_t *sta)
{
    *best = 0;
    if (!finite) { *sta = PNP_NONFINITE; return; }
    double e = err[0];                                  // (no index chosen at run time: err stays in registers)
    if (err[1] < e) { e = err[1]; *best = 1; }
    if (nd == 3 && err[2] < e) { e = err[2]; *best = 2; }
    *sta = nd == 3 && e > PNP_ERR_THRESHOLD ? PNP_BEST_OF_THREE : PNP_OK;
}

// u = [-R'T; R2q(R')]: Xc = R Xw + T read as pset1 ~ rot pset2 + trans with pset1 = Xw, pset2 = Xc -- the VO pair's convention
// (Calculate_V_Omega_RANSAC_dr_ye.m:40-50 over R2q.m, as pre3_vodev.h's final fit writes it), what pre3_predict takes
PRE3_PNP_HD void pnp_pair_u(const double Rm[9], const double T[3], double u[7])
{
    double R[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) R[3 * i + j] = Rm[3 * j + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) u[i] = -(R[3 * i] * T[0] + R[3 * i + 1] * T[1] + R[3 * i + 2] * T[2]);
    const double Tq = R[0] + R[4] + R[8] + 1;
    double a, b, c, d, S;
    if (Tq > 0.00000001) { S = 2 * sqrt(Tq); a = 0.25 * S; b = (R[5] - R[7]) / S; c = (R[6] - R[2]) / S; d = (R[1] - R[3]) / S; }
    else if (R[0] > R[4] && R[0] > R[8]) { S = 2 * sqrt(1.0 + R[0] - R[4] - R[8]); a = (R[5] - R[7]) / S; b = 0.25 * S; c = (R[1] + R[3]) / S; d = (R[6] + R[2]) / S; }
    else if (R[4] > R[8]) { S = 2 * sqrt(1.0 + R[4] - R[0] - R[8]); a = (R[6] - R[2]) / S; b = (R[1] + R[3]) / S; c = 0.25 * S; d = (R[5] + R[7]) / S; }
    else { S = 2 * sqrt(1.0 + R[8] - R[0] - R[4]); a = (R[1] - R[3]) / S; b = (R[6] + R[2]) / S; c = (R[5] + R[7]) / S; d = 0.25 * S; }
    u[3] = a; u[4] = -b; u[5] = -c; u[6] = -d;
}
PRE3_PNP_HD void pnp_identity_u(double u[7]) { u[0] = u[1] = u[2] = 0; u[3] = 1; u[4] = u[5] = u[6] = 0; }

// the RANSAC's inlier rule and the winner's order: the larger support, then the smaller sum of inlier distances, then the lower index
PRE3_PNP_HD bool pnp_inlier(double dist, double zc, double thr_px) { return dist < thr_px && zc > 0; }
PRE3_PNP_HD bool pnp_better(int sa, double da, int ia, int sb, double db, int ib) { return sa > sb || (sa == sb && (da < db || (da == db && ia < ib))); }

}  // namespace pre3

#if defined(__HIPCC__)
#include "pre3_internal.h"
#include "pre3_geomdev.h"
namespace pre3 {
struct VoOut; struct VoPairHeader;
// RANSAC_CALC_VER2.m:191 in place, behind a VO pair's launches on st, no wait (pre3_vo_pair_pnp_seeded): k_pnp_pair_prep gathers cur's pixel of every
// match -- entries 0 and 1 of cur's kept keypoint frame at match(2, i) -- into pix2[2 x n1] and the pair's inlier flags into an ascending list, then
// k_pnp_solve over that list with pset1 as the points.  The pair not taken (pnum < 4, a refused pair, sta != 1) or fewer than six inliers: sta = 0.
// list holds n1 + 4 words (the count in front).
int launch_pnp_pair(const VoPairHeader *hdr, const VoOut *out, int n1, const double *pset1, const double *match, const double *frm2, int ldf2, int K2,
                    const int32_t *inl, const pre3_cam *cam, int undistort, double *pix2, int32_t *list, pre3_pnp_result *res, hipStream_t st);
// pre3_pnp_ransac_seeded's four launches on st, no wait, over resident correspondences whose count an earlier launch on st left in *n_dev
// (pre3_relocalise_seeded): Xw[3 x n_cap], U[2 x n_cap], of which the first min(*n_dev, n_cap) are read.  The grid, masks
// (n_hyp x ceil(n_cap / 64) words) and every array are sized by n_cap; the draws are draw_rule_pnp(seed, seq, *n_dev, h).  *n_dev < 6: the draw writes
// zeros, no hypothesis is solved, ctl = { winner -1, support 0 } and res->sta = 0.  ctl: PNP_CTL_WORDS words, the winner and its support first.
constexpr int PNP_CTL_WORDS = 4;
struct PnpRansacDev {
    const double *Xw, *U; int n_cap; const int32_t *n_dev; int n_hyp; double thr_px;
    unsigned long long *masks; int32_t *draws, *support, *state; double *dsum; int32_t *ctl, *idx, *flag; pre3_pnp_result *res, *hyp;
};
int launch_pnp_ransac_dev(const PnpRansacDev &r, const pre3_cam *cam, int undistort, uint64_t seed, uint64_t seq, hipStream_t st);
// k_pnp_refine (pre3_pnpref.h) behind those launches on st, no wait: Gauss-Newton over the winner's list from the refit's result block
int launch_pnp_refine_dev(const PnpRansacDev &r, const pre3_cam *cam, int undistort, int n_iter, double sigma_px, pre3_pnp_refine_result *ref, hipStream_t st);
}  // namespace pre3
#endif
