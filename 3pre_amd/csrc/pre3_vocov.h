// pre3_vocov.h -- the covariance of a VO pair's increment u = [T; q], propagated from the SR4000's per-point range and angle noise through the rigid fit
// (DESIGN.md section 27): aux_code/calc_cov_RANSAC_dr_ye.m:17-30 over aux_code/cov_pose_shift_calc.m:4-40, the line predict_state_and_covariance.m:115
// leaves commented out.  With vo_final_wave's convention (pre3_vodev.h) f_p = pset1(:,i), f_n = pset2(:,i), r_i = T + R(q) f_n - f_p, R(q) = d_q2R_sola's
// homogeneous quadratic form (not normalised), X = [T; q], E = sum_i 1/2 |r_i|^2 over the winner's inliers:
//   A_i = d(R f_n)/dq (3 x 4),  J_i = [I3 A_i],  H_i = J_i'J_i + [0 0; 0 S_i],  S_i(k, l) = r_i' (d2R/dq_k dq_l) f_n
//   B_i = [-J_i' , J_i'R + [0; rows r_i' dR/dq_k]]  (7 x 6),  Sigma_i = blkdiag(C(f_p), C(f_n)),  C(p): cov_pose_shift_calc.m:24-40
//   H = sum H_i,  M = sum B_i Sigma_i B_i',  cov = H^-1 M H^-1 (H by a 7 x 7 Cholesky), symmetrised as (C + C')/2
// Deviation from the reference, on purpose: cov_pose_shift_calc.m:14,19 takes pinv of each point's own H_i; that matrix has rank 3 at zero residual, so
// pinv's rank decision hangs on measurement noise.  The summed form is the implicit-function covariance of the fit find_transform_matrix_dr_ye solves.
// __host__ __device__, so that a host program can evaluate the per-point terms, the factorisation and the status rule (tests/vo_cov_host_main.cpp);
// k_vo_cov (pre3_vocov.hip) accumulates and solves with these functions, k_predict (pre3_geom.hip) applies the status rule.  All fp64, no contraction.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PRE3_VC_HD __host__ __device__ inline
#else
#define PRE3_VC_HD inline
#endif
#if defined(__clang__)
#define PRE3_VC_NOCONTRACT _Pragma("clang fp contract(off)")
#else
#define PRE3_VC_NOCONTRACT
#endif

namespace pre3 {

// what k_vo_cov leaves behind k_vo_final's result block: 400 bytes
struct VoCov { double cov[49]; int32_t status, n_inliers; };

constexpr int VC_NOT_COMPUTED = 0;      // pnum < 4, sta != 1, or a pair predict_u_select (pre3_predictu.h) refuses: cov is not written
constexpr int VC_VALID = 1;
constexpr int VC_UNUSABLE = 2;          // a non-finite inlier coordinate, a Cholesky pivot <= 7 eps (its original diagonal entry), a non-finite result: cov is not written

// the pair's increment is the one the prediction takes (predict_u_select's `take`, restated without its outputs): only then is a covariance computed
PRE3_VC_HD bool vc_pair_computes(int sta, int pnum, int bad, int dist_ok) { return pnum >= 4 && bad == 0 && dist_ok != 0 && sta == 1; }
// the prediction takes the pair's covariance as Pn; otherwise the context's own noise (caller-set, or the constant) stands behind it
PRE3_VC_HD bool vc_predict_takes(int sta, int pnum, int bad, int dist_ok, int status) { return vc_pair_computes(sta, pnum, bad, dist_ok) && status == VC_VALID; }

// packed lower triangle of a symmetric 7 x 7: (i, j), j <= i
PRE3_VC_HD constexpr int vc_ix(int i, int j) { return i * (i + 1) / 2 + j; }

PRE3_VC_HD void vc_q2R(const double *q, double *R)      // d_q2R_sola (pre3_geomdev.h), term for term
{
    PRE3_VC_NOCONTRACT
    const double a = q[0], b = q[1], c = q[2], d = q[3];
    const double aa = a * a, ab = 2 * a * b, ac = 2 * a * c, ad = 2 * a * d;
    const double bb = b * b, bc = 2 * b * c, bd = 2 * b * d, cc = c * c, cd = 2 * c * d, dd = d * d;
    R[0] = aa + bb - cc - dd; R[1] = bc - ad;           R[2] = bd + ac;
    R[3] = bc + ad;           R[4] = aa - bb + cc - dd; R[5] = cd - ab;
    R[6] = bd - ac;           R[7] = cd + ab;           R[8] = aa - bb - cc + dd;
}

// A[i * 4 + k] = ((dR/dq_k)(q) f)_i.  dR/dq_k is linear in q, so the same text at q = e_l gives the constant second derivative (d2R/dq_k dq_l) f.
PRE3_VC_HD void vc_dRf(const double *q, const double *f, double *A)
{
    PRE3_VC_NOCONTRACT
    const double a = q[0], b = q[1], c = q[2], d = q[3], x = f[0], y = f[1], z = f[2];
    const double p0 = a * x - d * y + c * z, p1 = d * x + a * y - b * z, p2 = b * y - c * x + a * z, p3 = b * x + c * y + d * z;
    A[0] = 2 * p0; A[1] = 2 * p3;  A[2] = 2 * p2;   A[3] = -2 * p1;
    A[4] = 2 * p1; A[5] = -2 * p2; A[6] = 2 * p3;   A[7] = 2 * p0;
    A[8] = 2 * p2; A[9] = 2 * p1;  A[10] = -2 * p0; A[11] = 2 * p3;
}
// G[k * 3 + j] = (r' (dR/dq_k)(q))_j
PRE3_VC_HD void vc_rdR(const double *q, const double *r, double *G)
{
    PRE3_VC_NOCONTRACT
    const double a = q[0], b = q[1], c = q[2], d = q[3], x = r[0], y = r[1], z = r[2];
    const double s0 = a * x + d * y - c * z, s1 = a * y - d * x + b * z, s2 = c * x - b * y + a * z, s3 = b * x + c * y + d * z;
    G[0] = 2 * s0;  G[1] = 2 * s1;   G[2] = 2 * s2;
    G[3] = 2 * s3;  G[4] = 2 * s2;   G[5] = -2 * s1;
    G[6] = -2 * s2; G[7] = 2 * s3;   G[8] = 2 * s0;
    G[9] = 2 * s1;  G[10] = -2 * s0; G[11] = 2 * s3;
}

// the polynomial per-point terms: Hi[28] (packed lower triangle), Bi[7 * 6] row-major = [d2E/dX dfp , d2E/dX dfn], r[3]
PRE3_VC_HD void vc_point_terms(const double *fp, const double *fn, const double *X, double *Hi, double *Bi, double *r)
{
    PRE3_VC_NOCONTRACT
    const double *q = X + 3;
    double R[9], A[12], G[12], J[21], S[16];
    vc_q2R(q, R);
    for (int i = 0; i < 3; ++i) r[i] = R[3 * i] * fn[0] + R[3 * i + 1] * fn[1] + R[3 * i + 2] * fn[2] + X[i] - fp[i];      // vo_final_wave's residual
    vc_dRf(q, fn, A);
    vc_rdR(q, r, G);
    for (int i = 0; i < 3; ++i) {
        for (int k = 0; k < 3; ++k) J[7 * i + k] = i == k ? 1.0 : 0.0;
        for (int k = 0; k < 4; ++k) J[7 * i + 3 + k] = A[4 * i + k];
    }
    for (int l = 0; l < 4; ++l) {
        const double e[4] = { l == 0 ? 1.0 : 0.0, l == 1 ? 1.0 : 0.0, l == 2 ? 1.0 : 0.0, l == 3 ? 1.0 : 0.0 };
        double D[12];
        vc_dRf(e, fn, D);
        for (int k = 0; k < 4; ++k) S[4 * k + l] = r[0] * D[k] + r[1] * D[4 + k] + r[2] * D[8 + k];
    }
    for (int a = 0; a < 7; ++a)
        for (int b = 0; b <= a; ++b) {
            double s = J[a] * J[b] + J[7 + a] * J[7 + b] + J[14 + a] * J[14 + b];
            if (b >= 3) s = s + S[4 * (a - 3) + (b - 3)];
            Hi[vc_ix(a, b)] = s;
        }
    for (int a = 0; a < 7; ++a)
        for (int s = 0; s < 3; ++s) {
            Bi[6 * a + s] = -J[7 * s + a];
            double v = J[a] * R[s] + J[7 + a] * R[3 + s] + J[14 + a] * R[6 + s];
            if (a >= 3) v = v + G[3 * (a - 3) + s];
            Bi[6 * a + 3 + s] = v;
        }
}

// cov_pose_shift_calc.m:24-40: C = J_s diag(sigma_r^2, sigma_a^2, sigma_a^2) J_s', J_s's columns d/dr, d/daz, d/del at cart2sph(p); C[9] row-major
PRE3_VC_HD void vc_point_cov(const double *p, double *C)
{
    PRE3_VC_NOCONTRACT
    const double PI = 3.141592653589793238462643383279502884;
    const double sr = 0.01 / 2, sa = 0.24 * PI / 180 / 4;
    const double vr = sr * sr, va = sa * sa;
    const double hxy = hypot(p[0], p[1]);
    const double az = atan2(p[1], p[0]), el = atan2(p[2], hxy), rr = hypot(hxy, p[2]);
    const double ca = cos(az), sn = sin(az), ce = cos(el), se = sin(el);
    const double jr[3] = { ce * ca, ce * sn, se };
    const double ja[3] = { -rr * ce * sn, rr * ce * ca, 0.0 };
    const double je[3] = { -rr * se * ca, -rr * se * sn, rr * ce };
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C[3 * i + j] = vr * jr[i] * jr[j] + va * ja[i] * ja[j] + va * je[i] * je[j];
}

// H += H_i, M += B_i blkdiag(Cp, Cn) B_i' (packed lower triangles)
PRE3_VC_HD void vc_accumulate(const double *Hi, const double *Bi, const double *Cp, const double *Cn, double *H, double *M)
{
    PRE3_VC_NOCONTRACT
    double W[42];
    for (int a = 0; a < 7; ++a)
        for (int s = 0; s < 3; ++s) {
            W[6 * a + s] = Bi[6 * a] * Cp[s] + Bi[6 * a + 1] * Cp[3 + s] + Bi[6 * a + 2] * Cp[6 + s];
            W[6 * a + 3 + s] = Bi[6 * a + 3] * Cn[s] + Bi[6 * a + 4] * Cn[3 + s] + Bi[6 * a + 5] * Cn[6 + s];
        }
    for (int a = 0; a < 7; ++a)
        for (int b = 0; b <= a; ++b) {
            double s = 0;
            for (int t = 0; t < 6; ++t) s = s + W[6 * a + t] * Bi[6 * b + t];
            M[vc_ix(a, b)] = M[vc_ix(a, b)] + s;
            H[vc_ix(a, b)] = H[vc_ix(a, b)] + Hi[vc_ix(a, b)];
        }
}
PRE3_VC_HD bool vc_finite3(const double *p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }
// one inlier into the sums; false (nothing added) for a non-finite coordinate
PRE3_VC_HD bool vc_add_point(const double *fp, const double *fn, const double *X, double *H, double *M)
{
    if (!vc_finite3(fp) || !vc_finite3(fn)) return false;
    double Hi[28], Bi[42], r[3], Cp[9], Cn[9];
    vc_point_terms(fp, fn, X, Hi, Bi, r);
    vc_point_cov(fp, Cp);
    vc_point_cov(fn, Cn);
    vc_accumulate(Hi, Bi, Cp, Cn, H, M);
    return true;
}

// H = L L' (packed lower triangles); false when a pivot is not above 7 eps times its original diagonal entry (a NaN pivot included).  The loop runs to
// the end either way, so that every lane of a wave takes the same path; L is then not to be used.
PRE3_VC_HD bool vc_chol7(const double *H, double *L)
{
    PRE3_VC_NOCONTRACT
    const double tol = 7 * 2.220446049250313e-16;
    bool ok = true;
    for (int j = 0; j < 7; ++j) {
        double d = H[vc_ix(j, j)];
        for (int k = 0; k < j; ++k) d = d - L[vc_ix(j, k)] * L[vc_ix(j, k)];
        if (!(d > tol * H[vc_ix(j, j)])) ok = false;
        const double l = sqrt(d);
        L[vc_ix(j, j)] = l;
        for (int i = j + 1; i < 7; ++i) {
            double s = H[vc_ix(i, j)];
            for (int k = 0; k < j; ++k) s = s - L[vc_ix(i, k)] * L[vc_ix(j, k)];
            L[vc_ix(i, j)] = s / l;
        }
    }
    return ok;
}
// x <- (L L')^-1 x
PRE3_VC_HD void vc_solve7(const double *L, double *x)
{
    PRE3_VC_NOCONTRACT
    for (int i = 0; i < 7; ++i) {
        double s = x[i];
        for (int k = 0; k < i; ++k) s = s - L[vc_ix(i, k)] * x[k];
        x[i] = s / L[vc_ix(i, i)];
    }
    for (int i = 6; i >= 0; --i) {
        double s = x[i];
        for (int k = i + 1; k < 7; ++k) s = s - L[vc_ix(k, i)] * x[k];
        x[i] = s / L[vc_ix(i, i)];
    }
}
// column j of H^-1 M, then row i of (H^-1 M) H^-1: the two solves k_vo_cov deals over seven lanes
PRE3_VC_HD void vc_column_of_M(const double *M, int j, double *x) { for (int i = 0; i < 7; ++i) x[i] = i >= j ? M[vc_ix(i, j)] : M[vc_ix(j, i)]; }

// the whole finish on one thread (the host's form; k_vo_cov runs the same operations, one right-hand side per lane): status, and cov on VC_VALID only
PRE3_VC_HD int vc_finish(const double *H, const double *M, bool points_finite, double *cov)
{
    double L[28], Xm[49], C[49];
    if (!points_finite || !vc_chol7(H, L)) return VC_UNUSABLE;
    for (int j = 0; j < 7; ++j) {
        double x[7];
        vc_column_of_M(M, j, x);
        vc_solve7(L, x);
        for (int i = 0; i < 7; ++i) Xm[7 * i + j] = x[i];
    }
    for (int i = 0; i < 7; ++i) {
        double x[7];
        for (int j = 0; j < 7; ++j) x[j] = Xm[7 * i + j];
        vc_solve7(L, x);
        for (int j = 0; j < 7; ++j) C[7 * i + j] = x[j];
    }
    bool fin = true;
    for (int i = 0; i < 7; ++i)
        for (int j = 0; j < 7; ++j) { const double v = (C[7 * i + j] + C[7 * j + i]) / 2; Xm[7 * i + j] = v; fin = fin && isfinite(v); }
    if (!fin) return VC_UNUSABLE;
    for (int i = 0; i < 49; ++i) cov[i] = Xm[i];
    return VC_VALID;
}

}  // namespace pre3
