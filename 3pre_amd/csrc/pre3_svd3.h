// pre3_svd3.h -- the 3 x 3 singular value decomposition of the VO front end's rigid fits (pre3_vodev.h: find_transform_matrix_dr_ye.m) and of EPnP's
// exterior orientation (pre3_pnp.h: efficient_pnp.m:179-205).  __host__ __device__ and free of HIP headers, so that a host program can run the very
// text the kernels run (tests/pnp_host_main.cpp).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define PRE3_SVD_HD __host__ __device__ inline
#else
#define PRE3_SVD_HD inline
#endif

namespace pre3 {

// svd of a 3x3 by one-sided Jacobi; returns U, sv, V with H = U diag(sv) V'
PRE3_SVD_HD void vo_svd3(const double *H, double *U, double *sv, double *V)
{
#pragma clang fp contract(off)
    double A[9];
    for (int i = 0; i < 9; ++i) { A[i] = H[i]; V[i] = (i % 4 == 0) ? 1.0 : 0.0; U[i] = 0.0; }
    for (int sweep = 0; sweep < 60; ++sweep) {
        int rotated = 0;
#pragma unroll
        for (int pq = 0; pq < 3; ++pq) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
            double alpha = 0, beta = 0, gamma = 0;
#pragma unroll
            for (int i = 0; i < 3; ++i) { alpha += A[3 * i + p] * A[3 * i + p]; beta += A[3 * i + q] * A[3 * i + q]; gamma += A[3 * i + p] * A[3 * i + q]; }
            if (gamma == 0.0 || fabs(gamma) <= 2.2e-16 * sqrt(alpha * beta)) continue;
            rotated = 1;
            const double zeta = (beta - alpha) / (2.0 * gamma);
            const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
            const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double ap = A[3 * i + p], aq = A[3 * i + q];
                A[3 * i + p] = c * ap - s * aq; A[3 * i + q] = s * ap + c * aq;
                const double vp = V[3 * i + p], vq = V[3 * i + q];
                V[3 * i + p] = c * vp - s * vq; V[3 * i + q] = s * vp + c * vq;
            }
        }
        if (!rotated) break;
    }
    int ok[3];
    double big = 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) { sv[j] = sqrt(A[j] * A[j] + A[3 + j] * A[3 + j] + A[6 + j] * A[6 + j]); big = sv[j] > big ? sv[j] : big; }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        ok[j] = sv[j] > 1e-300 && sv[j] > 1e-18 * big;
        if (ok[j]) for (int i = 0; i < 3; ++i) U[3 * i + j] = A[3 * i + j] / sv[j];
    }
    const int nok = ok[0] + ok[1] + ok[2];
    if (nok == 2) {                       // orthonormal completion for a zero singular value
        const int j = !ok[0] ? 0 : (!ok[1] ? 1 : 2), a = (j + 1) % 3, b = (j + 2) % 3;
        const double ua[3] = { U[a], U[3 + a], U[6 + a] }, ub[3] = { U[b], U[3 + b], U[6 + b] };
        const double w[3] = { ua[1] * ub[2] - ua[2] * ub[1], ua[2] * ub[0] - ua[0] * ub[2], ua[0] * ub[1] - ua[1] * ub[0] };
        for (int i = 0; i < 3; ++i) U[3 * i + j] = w[i];
    } else if (nok < 2) {
        for (int i = 0; i < 9; ++i) U[i] = (i % 4 == 0) ? 1.0 : 0.0;
        if (nok == 1) {
            const int j = ok[0] ? 0 : (ok[1] ? 1 : 2), a = (j + 1) % 3, b = (j + 2) % 3;
            const double u[3] = { A[j] / sv[j], A[3 + j] / sv[j], A[6 + j] / sv[j] };
            const int m = fabs(u[0]) < fabs(u[1]) ? (fabs(u[0]) < fabs(u[2]) ? 0 : 2) : (fabs(u[1]) < fabs(u[2]) ? 1 : 2);
            double e[3] = { 0, 0, 0 }; e[m] = 1;
            double w[3] = { u[1] * e[2] - u[2] * e[1], u[2] * e[0] - u[0] * e[2], u[0] * e[1] - u[1] * e[0] };
            const double nw = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
            for (int i = 0; i < 3; ++i) w[i] /= nw;
            const double x[3] = { u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0] };
            for (int i = 0; i < 3; ++i) { U[3 * i + j] = u[i]; U[3 * i + a] = w[i]; U[3 * i + b] = x[i]; }
        }
    }
}

}  // namespace pre3
