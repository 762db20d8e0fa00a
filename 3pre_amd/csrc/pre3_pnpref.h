// pre3_pnpref.h -- the EPnP pose refined by Gauss-Newton on the reprojection error it is scored by, and the covariance of the pose that comes with it
// (k_pnp_refine, pre3_pnp.hip).  The project's own follow-up of sections 35 and 36.  The reference puts a Gauss-Newton stage behind
// the same solver (aux_code/EPnP_matlab/EPnP/efficient_pnp_gauss.m:191-225, kept "if Gauss Newton improves results"), but that one runs over the betas
// against the control-point distances (gauss_newton.m): another quantity, and no covariance.  Only its taking rule (:221) is followed here.
//   pose (R, T), Xc = R Xw + T (EPnP's);  perturbation d = (tau, omega) on the camera side: R <- E R, T <- E T + tau, E = exp([omega]x) (pnpref_exp)
//   r_i = [u - (Cx + f x/z); v - (Cy + f y/z)],  J_i = D [I3, -[Xc]x],  D = f [1/z 0 -x/z^2; 0 1/z -y/z^2]        (pixels undistorted when asked to)
//   28 sums over the points: the upper triangle of J'J (21, row by row), J'r (6), r'r
//   step: (J'J) d = J'r by a 6 x 6 Cholesky; a pivot at or below 7 eps times its own original diagonal entry (a NaN included) makes it unusable
//   exactly n_iter steps, no early exit; cost[k] = r'r before step k, cost[n_iter] after the last
//   taken  iff  n_iter >= 1, every intermediate finite, every z > 0 at the refined pose, cost[n_iter] < cost[0]; otherwise the input pose is kept
//   cov6 = s^2 (J'J)^-1 at the pose the call ends on, by the Cholesky inverse, (C + C')/2;  s^2 = sigma_px^2, or cost / (2 n - 6) when sigma_px == 0
//   u = pnp_pair_u(R, T) = [r*; q*];  cov7 = Jm cov6 Jm', (C + C')/2, with dr* = -R' tau, dq* = -1/2 L(q*)[:, 1:4] omega: rank 6, null vector [0; q*]
// THE COVARIANCE TREATS THE MAP POINTS AS EXACT.  It carries the pixel noise alone: neither the landmarks' own uncertainty nor their correlation with
// the pose enters.  Like section 34's it is therefore optimistic, and on a real map PRE3_RELOC_NOISE_POSE_FLOOR is the form to use.
// sta: 0 not computed (the pose fed in has sta outside {1, 2}, or n < 6); 1 refined pose taken, covariance valid; 2 input pose kept, covariance valid;
// -1 no covariance (a pivot refused, a non-finite coordinate or result, or a depth <= 0 at the pose the call ends on).  With -1 or 0: R, T, u are the
// input's and the covariances and sigma2 hold NaN.
// __host__ __device__ and free of HIP headers: k_pnp_refine and tests/pnp_refine_host_main.cpp run the same text.
#pragma once
#include <stdint.h>
#include <math.h>

#include "pre3_pnp.h"

namespace pre3 {

constexpr int PNPREF_MAX_ITER = 10;
constexpr int PNPREF_SUMS = 28;                     // 21 of J'J, 6 of J'r, r'r
constexpr double PNPREF_SMALL_ANGLE2 = 1e-8;        // theta^2 below this: the series to theta^4 (the next terms are below 1e-19 of the value)
enum { PNPREF_NOT_COMPUTED = 0, PNPREF_TAKEN = 1, PNPREF_KEPT = 2, PNPREF_NO_COV = -1 };

// entry (r, c), r <= c, of the 6 x 6 upper triangle, row by row
PRE3_PNP_HD constexpr int pnpref_ix(int r, int c) { return r * 6 - r * (r - 1) / 2 + (c - r); }

// E = exp([w]x) by Rodrigues, row-major: I + a K + b K^2 with a = sin t / t, b = (1 - cos t) / t^2
PRE3_PNP_HD void pnpref_exp(const double w[3], double E[9])
{
    const double xx = w[0] * w[0], yy = w[1] * w[1], zz = w[2] * w[2], t2 = xx + yy + zz;
    double a, b;
    if (t2 < PNPREF_SMALL_ANGLE2) { a = 1.0 - t2 / 6.0 + t2 * t2 / 120.0; b = 0.5 - t2 / 24.0 + t2 * t2 / 720.0; }
    else { const double t = sqrt(t2); a = sin(t) / t; b = (1.0 - cos(t)) / t2; }
    const double xy = w[0] * w[1], xz = w[0] * w[2], yz = w[1] * w[2];
    E[0] = 1.0 - b * (yy + zz); E[1] = -a * w[2] + b * xy;  E[2] = a * w[1] + b * xz;
    E[3] = a * w[2] + b * xy;   E[4] = 1.0 - b * (xx + zz); E[5] = -a * w[0] + b * yz;
    E[6] = -a * w[1] + b * xz;  E[7] = a * w[0] + b * yz;   E[8] = 1.0 - b * (xx + yy);
}

// R <- E R, T <- E T + tau for d = (tau, omega)
PRE3_PNP_HD void pnpref_update(const double d[6], double R[9], double T[3])
{
    double E[9], Rn[9], Tn[3];
    pnpref_exp(d + 3, E);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) Rn[3 * i + j] = E[3 * i] * R[j] + E[3 * i + 1] * R[3 + j] + E[3 * i + 2] * R[6 + j];
        Tn[i] = E[3 * i] * T[0] + E[3 * i + 1] * T[1] + E[3 * i + 2] * T[2] + d[i];
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = Rn[i];
    T[0] = Tn[0]; T[1] = Tn[1]; T[2] = Tn[2];
}

// what one point adds to the 28 sums at the pose (R, T); returns its camera-frame depth
PRE3_PNP_HD double pnpref_point(const double R[9], const double T[3], double f, double Cx, double Cy, const double xw[3], double u, double v, double acc[PNPREF_SUMS])
{
    const double x = R[0] * xw[0] + R[1] * xw[1] + R[2] * xw[2] + T[0], y = R[3] * xw[0] + R[4] * xw[1] + R[5] * xw[2] + T[1];
    const double z = R[6] * xw[0] + R[7] * xw[1] + R[8] * xw[2] + T[2];
    const double iz = 1.0 / z, xz = x * iz, yz = y * iz, fz = f * iz;
    const double ju[6] = { fz, 0.0, -fz * xz, -f * xz * yz, f * (1.0 + xz * xz), -f * yz };
    const double jv[6] = { 0.0, fz, -fz * yz, -f * (1.0 + yz * yz), f * xz * yz, f * xz };
    const double ru = u - (Cx + f * xz), rv = v - (Cy + f * yz);
#pragma unroll
    for (int r = 0; r < 6; ++r) {
#pragma unroll
        for (int c = r; c < 6; ++c) acc[pnpref_ix(r, c)] += ju[r] * ju[c] + jv[r] * jv[c];
        acc[21 + r] += ju[r] * ru + jv[r] * rv;
    }
    acc[27] += ru * ru + rv * rv;
    return z;
}

// H = L L' from the summed upper triangle (L: the lower triangle, row-major 6 x 6, the upper left alone); false when a pivot is not above 7 eps times its
// own original diagonal entry.  The loop runs to the end either way: every thread takes the same path; L is then not to be used.
PRE3_PNP_HD bool pnpref_chol6(const double *s, double L[36])
{
    const double tol = 7 * PNP_EPS;
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double d = s[pnpref_ix(j, j)];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= L[6 * j + k] * L[6 * j + k];
        if (!(d > tol * s[pnpref_ix(j, j)])) ok = false;
        const double l = sqrt(d);
        L[6 * j + j] = l;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double t = s[pnpref_ix(j, i)];
#pragma unroll
            for (int k = 0; k < j; ++k) t -= L[6 * i + k] * L[6 * j + k];
            L[6 * i + j] = t / l;
        }
    }
    return ok;
}
// x <- (L L')^-1 x
PRE3_PNP_HD void pnpref_solve6(const double L[36], double x[6])
{
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double t = x[i];
#pragma unroll
        for (int k = 0; k < i; ++k) t -= L[6 * i + k] * x[k];
        x[i] = t / L[6 * i + i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double t = x[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) t -= L[6 * k + i] * x[k];
        x[i] = t / L[6 * i + i];
    }
}

// one step from the 28 sums: false (and the pose left alone) when a pivot is refused
PRE3_PNP_HD bool pnpref_step(const double acc[PNPREF_SUMS], double R[9], double T[3])
{
    double L[36], d[6];
    const bool ok = pnpref_chol6(acc, L);
#pragma unroll
    for (int i = 0; i < 6; ++i) d[i] = acc[21 + i];
    pnpref_solve6(L, d);
    if (ok) pnpref_update(d, R, T);
    return ok;
}

// the one decision, after efficient_pnp_gauss.m:221
PRE3_PNP_HD bool pnpref_takes(int n_iter, bool finite, bool in_front, double cost_first, double cost_last)
{
    return n_iter >= 1 && finite && in_front && cost_last < cost_first;
}

// cov6 = s2 (J'J)^-1 from the sums at the final pose, symmetrised; false: a pivot refused or a non-finite entry
PRE3_PNP_HD bool pnpref_cov6(const double acc[PNPREF_SUMS], double s2, double cov6[36])
{
    double L[36], C[36];
    if (!pnpref_chol6(acc, L)) return false;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double e[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) e[i] = i == j ? 1.0 : 0.0;
        pnpref_solve6(L, e);
#pragma unroll
        for (int i = 0; i < 6; ++i) C[6 * i + j] = s2 * e[i];
    }
    bool fin = true;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) { const double v = (C[6 * i + j] + C[6 * j + i]) / 2; cov6[6 * i + j] = v; fin = fin && isfinite(v); }
    return fin;
}

// Jm (7 x 6, row-major): d pnp_pair_u(E R, E T + tau) / d (tau, omega) at 0 -- rows 0..2 are [-R', 0], rows 3..6 are [0, -1/2 L(q*)[:, 1:4]] with L the
// left-multiplication matrix of qProd (tests/test_pnp_refine_ref.py holds the restated Jm to finite differences of pair_u itself)
PRE3_PNP_HD void pnpref_jm(const double R[9], const double u[7], double Jm[42])
{
#pragma unroll
    for (int i = 0; i < 42; ++i) Jm[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Jm[6 * i + j] = -R[3 * j + i];
    const double a = u[3], b = u[4], c = u[5], d = u[6];
    const double Lq[12] = { -b, -c, -d,  a, -d, c,  d, a, -b,  -c, b, a };
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Jm[6 * (3 + i) + 3 + j] = -0.5 * Lq[3 * i + j];
}

// cov7 = Jm cov6 Jm', symmetrised exactly; false on a non-finite entry
PRE3_PNP_HD bool pnpref_cov7(const double R[9], const double u[7], const double cov6[36], double cov7[49])
{
    double Jm[42], W[42], C[49];
    pnpref_jm(R, u, Jm);
    for (int i = 0; i < 7; ++i)
        for (int j = 0; j < 6; ++j) { double s = 0; for (int t = 0; t < 6; ++t) s += Jm[6 * i + t] * cov6[6 * t + j]; W[6 * i + j] = s; }
    for (int i = 0; i < 7; ++i)
        for (int j = 0; j < 7; ++j) { double s = 0; for (int t = 0; t < 6; ++t) s += W[6 * i + t] * Jm[6 * j + t]; C[7 * i + j] = s; }
    bool fin = true;
    for (int i = 0; i < 7; ++i)
        for (int j = 0; j < 7; ++j) { const double v = (C[7 * i + j] + C[7 * j + i]) / 2; cov7[7 * i + j] = v; fin = fin && isfinite(v); }
    return fin;
}

// s^2: the caller's pixel noise, or the a-posteriori variance of 2 n residuals on 6 parameters (n >= 6: the divisor is at least 6)
PRE3_PNP_HD double pnpref_sigma2(double sigma_px, double cost_end, int n) { return sigma_px > 0 ? sigma_px * sigma_px : cost_end / (2.0 * n - 6.0); }

}  // namespace pre3
