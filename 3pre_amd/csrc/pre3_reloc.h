// pre3_reloc.h -- the rule by which pre3_relocalise_seeded's prediction takes the pose EPnP found.  The project's own: the
// reference has no relocalisation.  Lane 0 of every block of k_predict (US = PredictUReloc, NS = PnReloc; pre3_geom.hip) evaluates reloc_select from
// the refit's result block and x_k_k[0:7]; tests/reloc_host_main.cpp runs the same text on the host.  __host__ __device__, free of HIP headers.
//   taken  iff  sta == 1 and n_support >= min_support
//   r* = -R'T, q* = R2q(R'): pnp.u, the convention h is built on -- h = distort(C + f (R_wc'(X - r))_xy / z) with R_wc = R(q*)
//   dX = R(q)'(r* - r), dq = conj(q) (x) q* / |q|^2, negated when its scalar part is negative: q (x) dq then stays in the hemisphere of q, the one
//   the cross-covariances of P were built in.  predict_pose (pre3_geomdev.h) of (x, u) lands on (r*, +-q* / |q*|).
//   not taken: u = [0 0 0 1 0 0 0] with +0 zeros, and the prediction keeps the context's own process noise
#pragma once
#include <stdint.h>
#include <math.h>

#if defined(__HIPCC__)
#define PRE3_RELOC_HD __host__ __device__ inline
#else
#define PRE3_RELOC_HD inline
#endif

namespace pre3 {

constexpr int RELOC_MAX_N = 4096;                   // landmarks a call matches (the masks hold RELOC_MAX_N / 64 words a hypothesis)
constexpr int RELOC_MIN_SUPPORT = 6;                // EPnP's minimum: a refit over fewer inliers does not exist

PRE3_RELOC_HD bool reloc_takes(int32_t sta, int32_t n_support, int32_t min_support) { return sta == 1 && n_support >= min_support; }

// q2R as the prediction rotates its increment, row-major.  A second copy of pre3_geomdev.h's d_q2R_sola, kept so that this header stays free of HIP: the
// two texts must stay equal, or predict_pose no longer lands on (r*, q*).  tests/reloc_host_main.cpp checks the landing with THIS copy; the device's
// predict_pose is held to it by tests/test_gpu_relocalise.py (x_k_km1 against the restatement's predict_pose of the device's own u, 1e-14).
PRE3_RELOC_HD void reloc_q2R(const double q[4], double R[9])
{
    const double a = q[0], b = q[1], c = q[2], d = q[3];
    const double aa = a * a, ab = 2 * a * b, ac = 2 * a * c, ad = 2 * a * d;
    const double bb = b * b, bc = 2 * b * c, bd = 2 * b * d, cc = c * c, cd = 2 * c * d, dd = d * d;
    R[0] = aa + bb - cc - dd; R[1] = bc - ad;           R[2] = bd + ac;
    R[3] = bc + ad;           R[4] = aa - bb + cc - dd; R[5] = cd - ab;
    R[6] = bd - ac;           R[7] = cd + ab;           R[8] = aa - bb - cc + dd;
}

// x: x_k_k[0:7] = [r; q]; pnp_u: the refit's u = [r*; q*].  Writes the increment and returns 1 when the pose is taken, else the identity and 0.
PRE3_RELOC_HD int reloc_select(const double x[7], int32_t sta, int32_t n_support, int32_t min_support, const double pnp_u[7], double u[7])
{
    if (!reloc_takes(sta, n_support, min_support)) {
        u[0] = 0.0; u[1] = 0.0; u[2] = 0.0; u[3] = 1.0; u[4] = 0.0; u[5] = 0.0; u[6] = 0.0;
        return 0;
    }
    double R[9];
    reloc_q2R(x + 3, R);
    const double d0 = pnp_u[0] - x[0], d1 = pnp_u[1] - x[1], d2 = pnp_u[2] - x[2];
    u[0] = R[0] * d0 + R[3] * d1 + R[6] * d2;           // R(q)'(r* - r)
    u[1] = R[1] * d0 + R[4] * d1 + R[7] * d2;
    u[2] = R[2] * d0 + R[5] * d1 + R[8] * d2;
    const double a = x[3], b = -x[4], c = -x[5], d = -x[6];            // conj(q)
    const double w = pnp_u[3], xx = pnp_u[4], y = pnp_u[5], z = pnp_u[6];
    const double n2 = x[3] * x[3] + x[4] * x[4] + x[5] * x[5] + x[6] * x[6];
    double q0 = (a * w - b * xx - c * y - d * z) / n2;                 // qProd.m:16-33
    double q1 = (a * xx + b * w + c * z - d * y) / n2;
    double q2 = (a * y - b * z + c * w + d * xx) / n2;
    double q3 = (a * z + b * y - c * xx + d * w) / n2;
    if (q0 < 0) { q0 = -q0; q1 = -q1; q2 = -q2; q3 = -q3; }
    u[3] = q0; u[4] = q1; u[5] = q2; u[6] = q3;
    return 1;
}

// ---- the refined form's process noise (pre3_relocalise_refined_seeded) ------------------------------------------------------
// The covariance of the pose's u = [r*; q*] (cov7, pre3_pnpref.h) carried through reloc_select to the covariance of the increment the prediction takes:
//   Pn = Jd cov7 Jd',  Jd = blkdiag(R(q)', L(conj q) / |q|^2) at x_k_k's q,  (M + M') / 2
// The hemisphere flip negates Jd's lower block and leaves Pn alone.  The work is cut into items of one entry each, which k_predict deals over 49 lanes of
// block 0 with barriers between the stages and the host walks in order; no product is fused into a sum, so both give the same bits.
#if defined(__clang__)
#define PRE3_RELOC_NOCONTRACT _Pragma("clang fp contract(off)")
#else
#define PRE3_RELOC_NOCONTRACT
#endif
enum { RELOC_NOISE_CALLER = 0, RELOC_NOISE_POSE = 1, RELOC_NOISE_POSE_FLOOR = 2, RELOC_NOISE_OWN = -1 };       // OWN: the context's own noise (the pose not taken)

PRE3_RELOC_HD void reloc_noise_jd(const double x[7], double Jd[49])
{
    PRE3_RELOC_NOCONTRACT
    double R[9];
    {                                                                  // reloc_q2R's expressions, restated under this function's no-contraction rule
        const double qa = x[3], qb = x[4], qc = x[5], qd = x[6];
        const double aa = qa * qa, ab = 2 * qa * qb, ac = 2 * qa * qc, ad = 2 * qa * qd;
        const double bb = qb * qb, bc = 2 * qb * qc, bd = 2 * qb * qd, cc = qc * qc, cd = 2 * qc * qd, dd = qd * qd;
        R[0] = aa + bb - cc - dd; R[1] = bc - ad;           R[2] = bd + ac;
        R[3] = bc + ad;           R[4] = aa - bb + cc - dd; R[5] = cd - ab;
        R[6] = bd - ac;           R[7] = cd + ab;           R[8] = aa - bb - cc + dd;
    }
    for (int i = 0; i < 49; ++i) Jd[i] = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) Jd[7 * i + k] = R[3 * k + i];
    const double a = x[3], b = -x[4], c = -x[5], d = -x[6];            // conj(q)
    const double n2 = x[3] * x[3] + x[4] * x[4] + x[5] * x[5] + x[6] * x[6];
    const double Lq[16] = { a, -b, -c, -d,  b, a, -d, c,  c, d, a, -b,  d, -c, b, a };
    for (int i = 0; i < 4; ++i)
        for (int k = 0; k < 4; ++k) Jd[7 * (3 + i) + 3 + k] = Lq[4 * i + k] / n2;
}
// entry t = 7 i + k of Jd C, of (Jd C) Jd', and of the symmetrised result
PRE3_RELOC_HD double reloc_noise_left(const double *Jd, const double *C, int t)
{
    PRE3_RELOC_NOCONTRACT
    const int i = t / 7, k = t % 7;
    double s = 0.0;
    for (int q = 0; q < 7; ++q) s = s + Jd[7 * i + q] * C[7 * q + k];
    return s;
}
PRE3_RELOC_HD double reloc_noise_right(const double *T1, const double *Jd, int t)
{
    PRE3_RELOC_NOCONTRACT
    const int i = t / 7, k = t % 7;
    double s = 0.0;
    for (int q = 0; q < 7; ++q) s = s + T1[7 * i + q] * Jd[7 * k + q];
    return s;
}
PRE3_RELOC_HD double reloc_noise_sym(const double *M, int t) { PRE3_RELOC_NOCONTRACT return (M[t] + M[7 * (t % 7) + t / 7]) / 2; }
// PRE3_RELOC_NOISE_POSE_FLOOR: the caller's block added entry by entry, one fp64 addition each
PRE3_RELOC_HD double reloc_noise_floor(double pose, double caller) { PRE3_RELOC_NOCONTRACT return pose + caller; }

PRE3_RELOC_HD void reloc_noise_from_pose(const double x[7], const double cov7[49], double Pn[49])
{
    double Jd[49], T1[49], M[49];
    reloc_noise_jd(x, Jd);
    for (int t = 0; t < 49; ++t) T1[t] = reloc_noise_left(Jd, cov7, t);
    for (int t = 0; t < 49; ++t) M[t] = reloc_noise_right(T1, Jd, t);
    for (int t = 0; t < 49; ++t) Pn[t] = reloc_noise_sym(M, t);
}

// which noise the refined form's prediction uses: the pose's covariance needs the pose taken and a refinement that left one (ref_sta 1 or 2)
PRE3_RELOC_HD int reloc_noise_rule(bool taken, int32_t noise, int32_t ref_sta)
{
    if (!taken) return RELOC_NOISE_OWN;
    if (noise == RELOC_NOISE_CALLER || !(ref_sta == 1 || ref_sta == 2)) return RELOC_NOISE_CALLER;
    return noise == RELOC_NOISE_POSE ? RELOC_NOISE_POSE : RELOC_NOISE_POSE_FLOOR;
}

}  // namespace pre3
