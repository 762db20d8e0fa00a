// pre3_predictcv.h -- the camera-only motion models of predict_state_and_covariance.m that the fork switched off: the state
// functions fv.m:64-87 and the commented original :98-106, F = dfv_by_dxv (:82, dfv_by_dxv.m:38-116) and the G of Q = func_Q (:127, func_Q.m:41-54),
// restated from the formulas.  pre3_predict_cv's one launch (k_predict_cv, pre3_geom.hip) evaluates cv_model once per block, in one lane.  __host__ __device__, so
// that a host program can check it.  All of it fp64.
//
// Types 0..3: constant_velocity, constant_orientation, constant_position, constant_position_and_orientation.  Not built:
// constant_position_and_orientation_location_noise, whose G goes through dq_by_deuler(tr2rpy(q2tr(q))) (func_Q.m:29-37).
//
// One deviation: dqomegadt_by_domega (dfv_by_dxv.m:70-116) is 0/0 at |omega| = 0, and the reference relies on the prior w_0 = 1e-15
// (initialize_x_and_p.m:29-32) never to get there.  Here |omega|^2 below the smallest normal double takes the limit instead: row 1 zero, dt/2 on the
// diagonal of rows 2:4.  The fork's own prediction writes exact zeros into x[7:13], so the case is the usual one behind pre3_predict or a step.
#pragma once
#include <math.h>
#include <float.h>

#if defined(__HIPCC__)
#define PRE3_CV_HD __host__ __device__ inline
#else
#define PRE3_CV_HD inline
#endif

namespace pre3 {

constexpr int CV_CONSTANT_VELOCITY = 0, CV_CONSTANT_ORIENTATION = 1, CV_CONSTANT_POSITION = 2, CV_CONSTANT_POSITION_AND_ORIENTATION = 3;
constexpr int CV_N_TYPES = 4;

// what pre3_predict_cv hands its launch
struct CvArgs { int type; double dt, var_a, var_alpha; };      // var_a = (sigma_a dt)^2, var_alpha = (sigma_alpha dt)^2: Pn's diagonal (:89-90)

// What lane 0 of every block works out, once: the predicted 13 entries with the quaternion NOT yet normalised (predict_state_and_covariance.m:137 takes
// normJac there), Rq = dq3_by_dq2(v2q(omega dt)) = F(4:7,4:7) of every type (dfv_by_dxv.m:43-44, dq3_by_dq2.m:34-38; 4 x 4 row-major) and
// M = dq3_by_dq1(q) dqomegadt_by_domega(omega, dt) (4 x 3): G(4:7,4:6) of every type (func_Q.m:50) and F(4:7,11:13) of type 0 (dfv_by_dxv.m:48).
// F and G themselves are read off these pieces entry by entry (cv_F_entry, cv_G_entry).
struct CvModel { double xo[13], Rq[16], M[12]; };

PRE3_CV_HD bool cv_moves(int type) { return type == CV_CONSTANT_VELOCITY || type == CV_CONSTANT_ORIENTATION; }      // r + v dt, v kept   (fv.m:66-69, :99-105)
PRE3_CV_HD bool cv_turns(int type) { return type == CV_CONSTANT_VELOCITY || type == CV_CONSTANT_POSITION; }         // q (x) v2q(omega dt), omega kept   (fv.m:74-77)

// One serial pass, written for the single lane that runs it: one square root, two divisions, one sine and one cosine.  With n = omega / |omega|,
// theta = |omega| dt, s = sin(theta / 2), c = cos(theta / 2):
//   v2q(omega dt) = [c, s n], the identity below eps (v2q.m:35-41, quaternion.m:37)
//   dqomegadt_by_domega (dfv_by_dxv.m:70-116): row 1 = -(dt/2) n_a s; rows 2:4 = (dt/2) n_a n_a c + (1/|omega|)(1 - n_a n_a) s on the diagonal,
//   n_a n_b ((dt/2) c - (1/|omega|) s) off it -- the reference's expressions with omega_a / |omega| taken once
PRE3_CV_HD void cv_model(const double *x, int type, double dt, CvModel &m)
{
    const double *r = x, *q = x + 3, *v = x + 7, *om = x + 10;
    const bool moves = cv_moves(type), turns = cv_turns(type);
    const double om2 = om[0] * om[0] + om[1] * om[1] + om[2] * om[2];
    double qw[4] = { 1, 0, 0, 0 }, D[12];
    if (om2 < DBL_MIN) {                                            // the limit (see above); v2q is the identity there
        for (int i = 0; i < 12; ++i) D[i] = 0;
        D[3] = D[7] = D[11] = dt / 2.0;
    } else {
        const double w = sqrt(om2), iw = 1.0 / w, theta = w * dt;
        const double n[3] = { om[0] * iw, om[1] * iw, om[2] * iw };
        const double s = sin(theta / 2.0), c = cos(theta / 2.0);
        if (!(theta < DBL_EPSILON)) { qw[0] = c; qw[1] = s * n[0]; qw[2] = s * n[1]; qw[3] = s * n[2]; }
        const double hc = (dt / 2.0) * c, is = iw * s;
        for (int a = 0; a < 3; ++a) {
            D[a] = (-dt / 2.0) * n[a] * s;                                                                          // dq0_by_domegaA, :100
            for (int b = 0; b < 3; ++b)
                D[3 * (1 + a) + b] = a == b ? n[a] * n[a] * hc + (1.0 - n[a] * n[a]) * is                           // dqA_by_domegaA, :104-107
                                            : n[a] * n[b] * (hc - is);                                              // dqA_by_domegaB, :113-115
        }
    }
    for (int i = 0; i < 3; ++i) {
        m.xo[i] = moves ? r[i] + v[i] * dt : r[i];
        m.xo[7 + i] = moves ? v[i] : 0.0;
        m.xo[10 + i] = turns ? om[i] : 0.0;
    }
    const double a = q[0], b = q[1], c = q[2], d = q[3];
    if (turns) {                                                    // qprod.m:28-33
        const double w = qw[0], xx = qw[1], y = qw[2], z = qw[3];
        m.xo[3] = a * w - b * xx - c * y - d * z;
        m.xo[4] = a * xx + w * b + (c * z - d * y);
        m.xo[5] = a * y + w * c + (d * xx - b * z);
        m.xo[6] = a * z + w * d + (b * y - c * xx);
    } else {
        for (int i = 0; i < 4; ++i) m.xo[3 + i] = q[i];
    }
    const double L[16] = { a, -b, -c, -d,  b, a, -d, c,  c, d, a, -b,  d, -c, b, a };           // dq3_by_dq1(q), dq3_by_dq1.m:34-37
    for (int i = 0; i < 4; ++i)
        for (int k = 0; k < 3; ++k) m.M[i * 3 + k] = L[i * 4] * D[k] + L[i * 4 + 1] * D[3 + k] + L[i * 4 + 2] * D[6 + k] + L[i * 4 + 3] * D[9 + k];
    const double Rq[16] = { qw[0], -qw[1], -qw[2], -qw[3],  qw[1], qw[0], qw[3], -qw[2],  qw[2], -qw[3], qw[0], qw[1],  qw[3], qw[2], -qw[1], qw[0] };
    for (int i = 0; i < 16; ++i) m.Rq[i] = Rq[i];
}

// F(i, k), 0-based (dfv_by_dxv.m:41-66): the identity, F(4:7,4:7) = Rq for every type; type 0 alone gets dt I at (1:3,8:10) and M at (4:7,11:13); types 1
// and 3 zero (11:13,11:13), types 2 and 3 zero (8:10,8:10) -- the blocks :51-66 zeroes, and no others
PRE3_CV_HD double cv_F_entry(int i, int k, int type, double dt, const double *Rq, const double *M)
{
    if (i < 3) return k == i ? 1.0 : (k == 7 + i && type == CV_CONSTANT_VELOCITY) ? dt : 0.0;
    if (i < 7) return (k >= 3 && k < 7) ? Rq[(i - 3) * 4 + k - 3] : (k >= 10 && type == CV_CONSTANT_VELOCITY) ? M[(i - 3) * 3 + k - 10] : 0.0;
    if (k != i) return 0.0;
    if (i < 10) return (type == CV_CONSTANT_POSITION || type == CV_CONSTANT_POSITION_AND_ORIENTATION) ? 0.0 : 1.0;
    return (type == CV_CONSTANT_ORIENTATION || type == CV_CONSTANT_POSITION_AND_ORIENTATION) ? 0.0 : 1.0;
}
// whether the prediction changes row i of P: F's row is not the identity's (dt > 0), or Jnorm touches it (rows 3..6)
PRE3_CV_HD bool cv_row_changes(int i, int type)
{
    if (i < 3) return type == CV_CONSTANT_VELOCITY;
    if (i < 7) return true;
    if (i < 10) return type == CV_CONSTANT_POSITION || type == CV_CONSTANT_POSITION_AND_ORIENTATION;
    return type == CV_CONSTANT_ORIENTATION || type == CV_CONSTANT_POSITION_AND_ORIENTATION;
}
// G(i, c), 13 x 6 (func_Q.m:45-50), the same for the four types
PRE3_CV_HD double cv_G_entry(int i, int c, double dt, const double *M)
{
    if (i < 3) return c == i ? dt : 0.0;
    if (i < 7) return c >= 3 ? M[(i - 3) * 3 + c - 3] : 0.0;
    return c == i - 7 ? 1.0 : 0.0;                                  // G(8:10,1:3) = I, G(11:13,4:6) = I
}

}  // namespace pre3
