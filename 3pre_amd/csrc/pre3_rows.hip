// pre3_rows.hip -- update.m:27-56 with at most 16 rows on the resident current estimate (pre3_update_rows, pre3_heading_update).
//
// For r <= 16 rows the update is bound by the sweep of P; the rest is a few rows of P and a 16 x 16 factorisation.  Two launches:
//   A  k_rows_hp     HP = H * P (r x ncols, fp64) in column strips, from the <= 16 r rows of P that H touches.  In the heading form
//                    (@ekf_filter/ekf_heading_update.m:29-44) every workgroup first builds h and H from the resident quaternion x_k_k(4:7) and
//                    evaluates the angle gate; workgroup 0 publishes rows, nu, R, the gate word and the prior quaternion to RowsBlock.
//   B  k_rows_sweep  a persistent grid over the upper-triangle 64 x 64 tiles of P.  Every workgroup first recomputes the same small-rank algebra in
//                    fp64 from the same inputs -- S = HP[:, cols(H)] H' + R, L = chol(S), L^-1, y = L^-1 nu, the updated quaternion, its norm and
//                    Jnorm -- so that every decision (gate, S not positive definite, the quaternion) is the same in all of them and no workgroup
//                    ever waits for another.  Then, per tile: W_I = L^-1 HP[:, I], W_J = L^-1 HP[:, J], D = P_IJ - W_I' W_J (update.m:37), the
//                    rows / columns 3..6 of D through Jnorm where the tile holds them (update.m:42-46), the tile and its mirror image written
//                    from the same values (exactly symmetric, update.m:38), x(J) += W_J' y (update.m:36), x(4:7) normalised (update.m:48).
// P is read once (its upper triangle) and written once.  S, L, y and W are fp64 on both dtypes: the heading update's S is nearly singular by
// construction (lambda_min scales with the square of the angle between z and h), which fp32 would not resolve.
#include "pre3_internal.h"

namespace pre3 {

namespace {

constexpr int RT = 64;          // sweep tile
constexpr int RB = 256;         // threads per workgroup of both launches

__device__ inline double rows_acosd(double c) { return acos(fmin(fmax(c, -1.0), 1.0)) * (180.0 / 3.14159265358979323846); }

// aux_code/observe_heading_func.m:19-23 and observe_heading_jac.m:31-38 at q = x(4:7)
__device__ inline void heading_rows(const double *q, double *h, double *H /* 3 x 4 row-major */)
{
    const double q1 = q[0], q2 = q[1], q3 = q[2], q4 = q[3];
    h[0] = q1 * q4 * -2.0 + q2 * q3 * 2.0;
    h[1] = q1 * q1 - q2 * q2 + q3 * q3 - q4 * q4;
    h[2] = q1 * q2 * 2.0 + q3 * q4 * 2.0;
    H[0] = -2.0 * q4; H[1] = 2.0 * q3;  H[2] = 2.0 * q2;  H[3] = -2.0 * q1;
    H[4] = 2.0 * q1;  H[5] = -2.0 * q2; H[6] = 2.0 * q3;  H[7] = -2.0 * q4;
    H[8] = 2.0 * q2;  H[9] = 2.0 * q1;  H[10] = 2.0 * q4; H[11] = 2.0 * q3;
}

// ekf_heading_update.m:41-44 over aux_code/find_angle_bw_2_vecs.m:3-12: true = skip the update.  MATLAB's `if a > 4` on the 7-vector is true only when
// every angle exceeds 4 degrees (strict = 1, quirk Q12); strict = 0: the angle between z and h alone.  Cosines clamped to [-1, 1].
__device__ inline bool heading_gate_skips(const double *z, const double *h, int strict)
{
    const double mz = sqrt(z[0] * z[0] + z[1] * z[1] + z[2] * z[2]), mh = sqrt(h[0] * h[0] + h[1] * h[1] + h[2] * h[2]);
    const double a7 = rows_acosd((z[0] * h[0] + z[1] * h[1] + z[2] * h[2]) / mz / mh);
    if (!strict) return a7 > 4.0;
    bool all = a7 > 4.0;
    for (int k = 0; k < 3; ++k) all = all && rows_acosd(z[k] / mz) > 4.0 && rows_acosd(h[k] / mh) > 4.0;
    return all;
}

// Launch A.  grid (ceil(ncols / 256), r): row a of HP for 256 columns per workgroup.
template <typename T>
__global__ __launch_bounds__(RB) void k_rows_hp(const T *__restrict__ P, int ld, int ncols, const double *__restrict__ x, RowsBlock *__restrict__ blk,
                                                double *__restrict__ HP, RowsHeading hd)
{
    __shared__ int32_t s_col[RMAX];
    __shared__ double s_val[RMAX];
    const int a = blockIdx.y, tid = threadIdx.x;
    if (hd.on) {
        double q[4] = { x[3], x[4], x[5], x[6] }, h[3], H[12];
        heading_rows(q, h, H);
        // the by-value z / RR (pre3_heading_update), or what the plane fit queued ahead of this launch left on the device (pre3_heading_from_scan):
        // a fit that is not sta == 1 skips like the gate
        double z[3] = { hd.z[0], hd.z[1], hd.z[2] };
        bool skip;
        if (hd.src != nullptr) {
            for (int k = 0; k < 3; ++k) z[k] = hd.src->z[k];
            skip = hd.src->sta != 1 || heading_gate_skips(z, h, hd.strict);
        } else skip = heading_gate_skips(z, h, hd.strict);
        if (blockIdx.x == 0 && a == 0 && tid == 0) {
            blk->r = 3; blk->applied = skip ? 0 : 1;
            for (int k = 0; k < 4; ++k) blk->q[k] = q[k];
            for (int i = 0; i < 3; ++i) {
                for (int t = 0; t < RMAX; ++t) { blk->col[i * RMAX + t] = t < 4 ? 3 + t : 0; blk->val[i * RMAX + t] = t < 4 ? H[i * 4 + t] : 0.0; }
                blk->nu[i] = z[i] - h[i];
                for (int j = 0; j < 3; ++j) blk->R[i * 3 + j] = hd.src != nullptr ? hd.src->RR[i * 3 + j] : hd.RR[i * 3 + j];
            }
        }
        if (skip) return;                                   // (the same decision in every workgroup)
        if (tid < RMAX) { s_col[tid] = tid < 4 ? 3 + tid : 0; s_val[tid] = tid < 4 ? H[a * 4 + tid] : 0.0; }
    } else {
        if (blockIdx.x == 0 && a == 0 && tid == 0) { blk->applied = 1; for (int k = 0; k < 4; ++k) blk->q[k] = x[3 + k]; }
        if (tid < RMAX) { s_col[tid] = blk->col[a * RMAX + tid]; s_val[tid] = blk->val[a * RMAX + tid]; }
    }
    __syncthreads();
    const int j = blockIdx.x * RB + tid;
    if (j >= ncols) return;
    double s = 0.0;
#pragma unroll
    for (int t = 0; t < RMAX; ++t) s = __builtin_fma(s_val[t], (double)P[(size_t)s_col[t] * ld + j], s);
    HP[(size_t)a * ld + j] = s;
}

struct SweepShared {
    double S[RMAX][RMAX + 1];       // S, then L in its lower triangle
    double Li[RMAX][RMAX + 1];      // L^-1
    double y[RMAX];                 // L^-1 nu
    double qn[4];                   // x(4:7) after update.m:36, then normalised (update.m:48)
    double Jn[16];
    int bad;
    double WI[RMAX][RT], WJ[RMAX][RT];
    double F[RT][RT + 1];
};

// Launch B.  A persistent grid; tile t of the upper triangle (row-major over I <= J of nT x nT).
template <typename T>
__global__ __launch_bounds__(RB) void k_rows_sweep(T *__restrict__ P, int ld, int n, int nT, int r, double *__restrict__ x,
                                                   const RowsBlock *__restrict__ blk, const double *__restrict__ HP, int32_t *__restrict__ stats)
{
    __shared__ SweepShared sh;
    const int tid = threadIdx.x;
    if (blk->applied == 0) return;                          // ekf_heading_update.m:42-44 (the gate word of launch A)
    // ---- the small-rank algebra, the same in every workgroup (update.m:32-33, 36, 42, 48)
    if (tid < r * r) {
        const int a = tid / r, b = tid % r;
        double s = blk->R[a * r + b];
        double g = 0.0;
#pragma unroll
        for (int t = 0; t < RMAX; ++t) g = __builtin_fma(blk->val[b * RMAX + t], HP[(size_t)a * ld + blk->col[b * RMAX + t]], g);
        sh.S[a][b] = g + s;
    }
    if (tid == 0) sh.bad = 0;
    __syncthreads();
    for (int k = 0; k < r; ++k) {
        if (tid == 0) {
            const double d = sh.S[k][k];
            if (!(d > 0.0)) sh.bad = 1;
            sh.S[k][k] = sqrt(fmax(d, 0.0));
        }
        __syncthreads();
        if (sh.bad) break;                                  // (uniform: read after the barrier)
        if (tid > k && tid < r) sh.S[tid][k] /= sh.S[k][k];
        __syncthreads();
        for (int e = tid; e < r * r; e += RB) {
            const int i = e / r, j = e % r;
            if (i > k && j > k && j <= i) sh.S[i][j] = __builtin_fma(-sh.S[i][k], sh.S[j][k], sh.S[i][j]);
        }
        __syncthreads();
    }
    if (sh.bad) {                                           // x and P stay as they are; the error word as the other updates set it
        if (blockIdx.x == 0 && tid == 0) atomicExch(stats + 6, 1);
        return;
    }
    if (tid < r) {                                          // column tid of L^-1
        for (int i = 0; i < r; ++i) {
            double v = i == tid ? 1.0 : 0.0;
            for (int k = tid; k < i; ++k) v = __builtin_fma(-sh.S[i][k], sh.Li[k][tid], v);
            sh.Li[i][tid] = i < tid ? 0.0 : v / sh.S[i][i];
        }
    }
    __syncthreads();
    if (tid < r) {
        double v = 0.0;
        for (int b = 0; b <= tid; ++b) v = __builtin_fma(sh.Li[tid][b], blk->nu[b], v);
        sh.y[tid] = v;
    }
    __syncthreads();
    if (tid < 4) {                                          // x(4:7) + W(:, 4:7)' y
        double acc = 0.0;
        for (int a = 0; a < r; ++a) {
            double w = 0.0;
            for (int b = 0; b <= a; ++b) w = __builtin_fma(sh.Li[a][b], HP[(size_t)b * ld + 3 + tid], w);
            acc = __builtin_fma(w, sh.y[a], acc);
        }
        sh.qn[tid] = blk->q[tid] + acc;
    }
    __syncthreads();
    if (tid == 0) {
        double q[4] = { sh.qn[0], sh.qn[1], sh.qn[2], sh.qn[3] }, J[16];
        d_normjac(q, J);
        for (int k = 0; k < 16; ++k) sh.Jn[k] = J[k];
        const double nq = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        for (int k = 0; k < 4; ++k) sh.qn[k] = q[k] / nq;
    }
    __syncthreads();
    // ---- the tiles
    const int ntiles = nT * (nT + 1) / 2;
    const int jj = tid & (RT - 1), ig = tid / RT;           // element (ig + 4 k, jj) of a tile
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        int I = 0, rem = t;
        while (rem >= nT - I) { rem -= nT - I; ++I; }
        const int J = I + rem, I0 = I * RT, J0 = J * RT;
        T pv[RT / 4];
#pragma unroll
        for (int k = 0; k < RT / 4; ++k) pv[k] = P[(size_t)(I0 + ig + 4 * k) * ld + J0 + jj];       // (in flight while W is formed)
        if (tid < 2 * RT) {                                 // W_I (tid < 64) or W_J: L^-1 HP[:, col]
            const int side = tid / RT, c = (side ? J0 : I0) + jj;
            double hp[RMAX];
#pragma unroll
            for (int b = 0; b < RMAX; ++b) hp[b] = b < r ? HP[(size_t)b * ld + c] : 0.0;
#pragma unroll
            for (int a = 0; a < RMAX; ++a) {
                double w = 0.0;
#pragma unroll
                for (int b = 0; b <= a; ++b) w = __builtin_fma(sh.Li[a][b], hp[b], w);      // (Li is zero above the diagonal; hp beyond r is zero)
                if (a < r) { if (side) sh.WJ[a][jj] = w; else sh.WI[a][jj] = w; }
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < RT / 4; ++k) {
            const int ii = ig + 4 * k;
            double d = (double)pv[k];
            for (int a = 0; a < r; ++a) d = __builtin_fma(-sh.WI[a][ii], sh.WJ[a][jj], d);
            sh.F[ii][jj] = d;
        }
        __syncthreads();
        if (I == J) {                                       // (update.m:38: the upper triangle is the tile)
            for (int e = tid; e < RT * RT; e += RB) { const int i = e / RT, j = e % RT; if (i > j) sh.F[i][j] = sh.F[j][i]; }
            __syncthreads();
        }
        if (I == 0) {                                       // update.m:44-46: rows 4:7 through Jnorm ...
            const int rr = tid / RT;
            double v = 0.0;
            for (int k = 0; k < 4; ++k) v = __builtin_fma(sh.Jn[rr * 4 + k], sh.F[3 + k][jj], v);
            __syncthreads();
            sh.F[3 + rr][jj] = v;
            __syncthreads();
            if (J == 0) {                                   // ... and columns 4:7 (Jnorm P Jnorm' on the quaternion block)
                double w = 0.0;
                for (int k = 0; k < 4; ++k) w = __builtin_fma(sh.F[jj][3 + k], sh.Jn[rr * 4 + k], w);
                __syncthreads();
                sh.F[jj][3 + rr] = w;
                __syncthreads();
                for (int e = tid; e < RT * RT; e += RB) { const int i = e / RT, j = e % RT; if (i > j) sh.F[i][j] = sh.F[j][i]; }
                __syncthreads();
            }
        }
#pragma unroll
        for (int k = 0; k < RT / 4; ++k) P[(size_t)(I0 + ig + 4 * k) * ld + J0 + jj] = (T)sh.F[ig + 4 * k][jj];
        if (I != J) {                                       // the mirror image, from the same values
#pragma unroll
            for (int k = 0; k < RT / 4; ++k) P[(size_t)(J0 + ig + 4 * k) * ld + I0 + jj] = (T)sh.F[jj][ig + 4 * k];
        }
        if (I == 0 && tid < RT) {                           // update.m:36 on this tile's columns, update.m:48
            const int j = J0 + tid;
            if (j >= 3 && j < 7) x[j] = sh.qn[j - 3];
            else if (j < n) {
                double v = 0.0;
                for (int a = 0; a < r; ++a) v = __builtin_fma(sh.WJ[a][tid], sh.y[a], v);
                x[j] = x[j] + v;
            }
        }
        __syncthreads();
    }
}

}  // namespace

int launch_rows_update(pre3_ctx *c, const RowsBlock *rows, const RowsHeading *hd)
{
    if (!c->rows_ready) {
        Group g(c->mem.fixed, c->rows_ready);
        PRE3_TRY(g.dev(&c->rows_blk, sizeof(RowsBlock), Zero::none())); PRE3_TRY(g.dev(&c->rows_hp, sizeof(double) * RMAX * (size_t)c->ld, Zero::none()));
        g.commit();
    }
    const int r = rows ? rows->r : 3;
    PRE3_CHECK(r >= 1 && r <= RMAX, PRE3_E_ARG, "launch_rows_update: %d rows", r);
    if (rows) PRE3_HIP(hipMemcpyAsync(c->rows_blk, rows, sizeof(RowsBlock), hipMemcpyHostToDevice, c->stream));
    RowsHeading h{};
    if (hd) h = *hd;
    const int nT = ceil_div(c->n, RT), ncols = nT * RT;      // (nT * 64 <= ld: ld is a multiple of 128)
    const int ntiles = nT * (nT + 1) / 2;
    const int grid = std::min(ntiles, 2 * c->num_cus);
    if (c->dtype == PRE3_F64) {
        hipLaunchKernelGGL(k_rows_hp<double>, dim3(ceil_div(ncols, RB), r), dim3(RB), 0, c->stream, (const double *)c->P, c->ld, ncols, c->x_kk, c->rows_blk, c->rows_hp, h);
        PRE3_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_rows_sweep<double>, dim3(grid), dim3(RB), 0, c->stream, (double *)c->P, c->ld, c->n, nT, r, c->x_kk, c->rows_blk, c->rows_hp, c->stats);
    } else {
        hipLaunchKernelGGL(k_rows_hp<float>, dim3(ceil_div(ncols, RB), r), dim3(RB), 0, c->stream, (const float *)c->P, c->ld, ncols, c->x_kk, c->rows_blk, c->rows_hp, h);
        PRE3_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_rows_sweep<float>, dim3(grid), dim3(RB), 0, c->stream, (float *)c->P, c->ld, c->n, nT, r, c->x_kk, c->rows_blk, c->rows_hp, c->stats);
    }
    PRE3_HIP(hipGetLastError());
    return PRE3_OK;
}

int rows_applied(pre3_ctx *c, int32_t *applied_host)
{
    PRE3_CHECK(c->rows_ready, PRE3_E_STATE, "no small-rank update has run");
    PRE3_HIP(hipMemcpyAsync(applied_host, &c->rows_blk->applied, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    return PRE3_OK;
}

}  // namespace pre3
