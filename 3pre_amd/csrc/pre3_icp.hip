// pre3_icp.hip -- dense ICP between two point clouds on the device: Mian's icp_with_init.m, the refinement of the VO pair's pose the reference's author
// tried and left commented out (RANSAC_CALC_VER_test.m:77-78) because MATLAB could not afford it per frame.
//   TestScripts/icp_with_init.m:34-35    data2 <- Rinit data2 + Tinit
//   :49-51, :76-78                       dsearchn without its triangulation (the exact nearest model point), D > 2 res dropped
//   :53-56, :80-83                       one pair per model index: the smallest D, on equal D the highest source index (the 2005 code's unique: last occurrence)
//   :58-62, :85-89, :103-120             reg: means, K = Sshifted Mshifted' / n, R1 = V U', the det < 0 repair, t1; data2, R, t updated every iteration
//   :47-48, :63-75, :90-100              loop control (pre3_icp.h)
//   ransac_dr_ye.m:17-18                 the camera frame of the *_frames forms: [-x; -y; z]
// All fp64, contraction off.  Per iteration five launches on one stream, every hand-off a launch boundary, no workgroup waits on another:
//   k_icp_nn      2-D grid, source tile x model chunk: the chunk staged in LDS as x / y / z, every lane ICP_PTS source points in registers, all lanes read the
//                 same model point (an LDS broadcast); partial (d, index) per (chunk, source), ties to the lower index by scan order
//   k_icp_claim1  the chunks merged in ascending order (strict <), D = sqrt(d), D > 2 res dropped; a 64-bit atomic minimum of D's bits per model index
//   k_icp_claim2  the sources that hold that minimum claim the model index by an atomic maximum of the source index
//   k_icp_reg     ONE workgroup: the claims compacted ascending in the model index (ballot prefix), sums by a tree of fixed shape, then one thread: svd,
//                 R1, t1, R, t, the loop-control rule and the log
//   k_icp_apply   data2 <- R1 data2 + t1, for the iteration whose number the state block names
// The host queues all 62 iterations at once; a launch that finds `done` returns at its first instruction.  One host wait.
// Every slot has one writer or an integer atomic: results are bit-equal from run to run.
#include <cmath>
#include <mutex>

#include "pre3_internal.h"
#include "pre3_vodev.h"
#include "pre3_icp.h"
#include "pre3_icpcov.h"
#include "pre3_srframe.h"

namespace pre3 {

namespace {

constexpr int REG_NTH = 1024, REG_NW = REG_NTH / 64;

// the device block of a run; the front of it (IcpHead) comes back to the host
struct IcpHead {
    IcpCtl ctl;
    double R[9], t[3];              // accumulated (row-major)
    double R1[9], t1[3];            // the last iteration's
    double Rinit[9], Tinit[3];
    double Rtot[9], ttot[3], u[7], error;
    double log[3 * ICP_ITER_CAP];
};

struct IcpWork {
    IcpHead *h;
    int cap1, cap2;                                 // layout counts (>= the real n1, n2 of the state block)
    double *mx, *my, *mz, *sx, *sy, *sz;
    double *pd; int32_t *pi;                        // [chunks][cap2]
    double *bD; int32_t *bi;                        // [cap2]
    unsigned long long *minD; int32_t *owner;       // [cap1]
    int32_t *corr_m, *corr_s; double *corr_d;       // [cap1]
    int32_t *mpix, *spix;                           // frames: the pixel of every kept point
};

__device__ __forceinline__ bool finite3(double a, double b, double c) { return isfinite(a) && isfinite(b) && isfinite(c); }

// a VO pair's result block as the seed: sta != 1 leaves the run where the host's image put it (ICP_NOT_RUN) and ends it
__global__ void k_icp_seed(IcpHead *h, const VoOut *__restrict__ vo)
{
    if (threadIdx.x != 0) return;
    if (vo->sta != 1) { h->ctl.done = 1; h->ctl.status = ICP_NOT_RUN; return; }
    for (int i = 0; i < 9; ++i) h->Rinit[i] = vo->rot[i];
    for (int i = 0; i < 3; ++i) h->Tinit[i] = vo->trans[i];
}

// head_image's fields (the host's image of a run that starts at n1 = n2 = 0 with the identity seed) written into a head the stream has zeroed
__global__ void k_icp_head(IcpHead *h, double res)
{
    if (threadIdx.x != 0) return;
    icp_ctl_start(&h->ctl, 0, 0, res);
    for (int i = 0; i < 9; ++i) { h->R[i] = (i % 4 == 0) ? 1.0 : 0.0; h->Rinit[i] = h->R[i]; }
}

// the two clouds from two resident frames: blockIdx.x == 0 every pixel of prev, 1 cur's pixels at rows and columns 0, stride, ...; a pixel with a
// non-finite coordinate or z <= 0 is dropped, the order kept (ballot prefix, as k_vp_pairs)
__global__ __launch_bounds__(REG_NTH) void k_icp_pack(IcpWork w, int rows, int cols, int stride, const double *__restrict__ x1, const double *__restrict__ y1,
                                                      const double *__restrict__ z1, const double *__restrict__ x2, const double *__restrict__ y2,
                                                      const double *__restrict__ z2)
{
    if (w.h->ctl.done) return;
    __shared__ int s_cnt[REG_NW];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const bool model = blockIdx.x == 0;
    const int st = model ? 1 : stride;
    const int nr = (rows + st - 1) / st, nc = (cols + st - 1) / st, ncand = nr * nc;
    const double *x = model ? x1 : x2, *y = model ? y1 : y2, *z = model ? z1 : z2;
    double *ox = model ? w.mx : w.sx, *oy = model ? w.my : w.sy, *oz = model ? w.mz : w.sz;
    int32_t *opix = model ? w.mpix : w.spix;
    const int cap = model ? w.cap1 : w.cap2;
    int base = 0;
    for (int q0 = 0; q0 < ncand; q0 += REG_NTH) {
        const int q = q0 + tid;
        int ok = 0, pix = 0;
        double a = 0, b = 0, c = 0;
        if (q < ncand) {
            pix = (q / nr) * st * rows + (q % nr) * st;
            a = x[pix]; b = y[pix]; c = z[pix];
            ok = finite3(a, b, c) && c > 0.0;
        }
        const unsigned long long bal = __ballot(ok);
        if (lane == 0) s_cnt[wv] = __popcll(bal);
        __syncthreads();
        int off = 0, tot = 0;
#pragma unroll
        for (int k = 0; k < REG_NW; ++k) { const int cw = s_cnt[k]; if (k < wv) off += cw; tot += cw; }
        if (ok) {
            const int o = base + off + __popcll(bal & ((1ull << lane) - 1ull));
            if (o < cap) { ox[o] = -a; oy[o] = -b; oz[o] = c; opix[o] = pix; }
        }
        base += tot;
        __syncthreads();
    }
    if (tid == 0) { if (model) w.h->ctl.n1 = base; else w.h->ctl.n2 = base; }
}

// :34-35, the finiteness check of both clouds, the claim tables cleared, fewer than three points on either side
__global__ __launch_bounds__(256) void k_icp_init(IcpWork w)
{
#pragma clang fp contract(off)
    IcpCtl &c = w.h->ctl;
    if (c.done) return;
    const int n1 = c.n1, n2 = c.n2;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (n1 < 3 || n2 < 3) {                             // every thread sees the same counts: nothing is seeded, whatever order the workgroups run in
        if (i == 0) { atomicOr(&c.done, 1); atomicMax(&c.status, ICP_FEW); }
        return;
    }
    int bad = 0;
    if (i < n1 && i < w.cap1) {
        bad |= !finite3(w.mx[i], w.my[i], w.mz[i]);
        w.minD[i] = ~0ull; w.owner[i] = -1;
    }
    if (i < n2 && i < w.cap2) {
        const double a = w.sx[i], b = w.sy[i], d = w.sz[i];
        bad |= !finite3(a, b, d);
        const double *R = w.h->Rinit, *T = w.h->Tinit;
        w.sx[i] = ((R[0] * a + R[1] * b) + R[2] * d) + T[0];
        w.sy[i] = ((R[3] * a + R[4] * b) + R[5] * d) + T[1];
        w.sz[i] = ((R[6] * a + R[7] * b) + R[8] * d) + T[2];
    }
    if (bad) { atomicOr(&c.done, 1); atomicMax(&c.status, ICP_NONFINITE); }
}

// :49, :76 -- the exact nearest model point of every source point inside one model chunk
__global__ __launch_bounds__(ICP_NN_THREADS) void k_icp_nn(IcpWork w)
{
#pragma clang fp contract(off)
    const IcpCtl &c = w.h->ctl;
    if (c.done) return;
    const int n1 = min(c.n1, w.cap1), n2 = min(c.n2, w.cap2);
    const int m0 = blockIdx.y * ICP_CHUNK, s0 = blockIdx.x * ICP_SRC_TILE;
    if (m0 >= n1 || s0 >= n2) return;
    __shared__ double lx[ICP_CHUNK], ly[ICP_CHUNK], lz[ICP_CHUNK];
    const int tid = threadIdx.x;
    const int mc = min(ICP_CHUNK, n1 - m0);
    for (int m = tid; m < mc; m += ICP_NN_THREADS) { lx[m] = w.mx[m0 + m]; ly[m] = w.my[m0 + m]; lz[m] = w.mz[m0 + m]; }
    double px[ICP_PTS], py[ICP_PTS], pz[ICP_PTS], best[ICP_PTS];
    int bm[ICP_PTS];
#pragma unroll
    for (int k = 0; k < ICP_PTS; ++k) {
        const int j = s0 + tid + k * ICP_NN_THREADS;
        const bool in = j < n2;
        px[k] = in ? w.sx[j] : 0.0; py[k] = in ? w.sy[j] : 0.0; pz[k] = in ? w.sz[j] : 0.0;
        best[k] = INFINITY; bm[k] = 0;
    }
    __syncthreads();
#pragma unroll 4
    for (int m = 0; m < mc; ++m) {
        const double x = lx[m], y = ly[m], z = lz[m];
#pragma unroll
        for (int k = 0; k < ICP_PTS; ++k) {
            const double dx = px[k] - x, dy = py[k] - y, dz = pz[k] - z;
            const double d = (dx * dx + dy * dy) + dz * dz;
            if (d < best[k]) { best[k] = d; bm[k] = m; }            // strict: a tie keeps the lower model index
        }
    }
#pragma unroll
    for (int k = 0; k < ICP_PTS; ++k) {
        const int j = s0 + tid + k * ICP_NN_THREADS;
        if (j < n2) { const size_t o = (size_t)blockIdx.y * w.cap2 + j; w.pd[o] = best[k]; w.pi[o] = m0 + bm[k]; }
    }
}

__device__ __forceinline__ bool icp_kept(double D, double res) { return !(D > 2.0 * res); }      // :51

__global__ __launch_bounds__(256) void k_icp_claim1(IcpWork w)
{
#pragma clang fp contract(off)
    const IcpCtl &c = w.h->ctl;
    if (c.done) return;
    const int n1 = min(c.n1, w.cap1), n2 = min(c.n2, w.cap2);
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n2) return;
    const int nch = (n1 + ICP_CHUNK - 1) / ICP_CHUNK;
    double d = INFINITY; int idx = 0;
    for (int k = 0; k < nch; ++k) {
        const size_t o = (size_t)k * w.cap2 + j;
        const double dk = w.pd[o];
        if (dk < d) { d = dk; idx = w.pi[o]; }
    }
    const double D = sqrt(d);
    w.bD[j] = D; w.bi[j] = idx;
    if (icp_kept(D, c.res) && idx >= 0 && idx < n1) atomicMin(&w.minD[idx], (unsigned long long)__double_as_longlong(D));      // D >= 0: its bits order as an integer
}

__global__ __launch_bounds__(256) void k_icp_claim2(IcpWork w)
{
    const IcpCtl &c = w.h->ctl;
    if (c.done) return;
    const int n1 = min(c.n1, w.cap1), n2 = min(c.n2, w.cap2);
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n2) return;
    const double D = w.bD[j];
    const int idx = w.bi[j];
    if (icp_kept(D, c.res) && idx >= 0 && idx < n1 && w.minD[idx] == (unsigned long long)__double_as_longlong(D)) atomicMax(&w.owner[idx], j);
}

// a sum over the workgroup by a tree of fixed shape: the wave's butterfly, then the sixteen waves' sums in order.  Every thread returns the total.
template <int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV], double (*s_red)[REG_NW], int lane, int wv)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (int i = 0; i < NV; ++i) v[i] += __shfl_xor(v[i], o, 64);
    __syncthreads();                                    // (s_red's readers of the previous sum are through)
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < NV; ++i) s_red[i][wv] = v[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        double a = s_red[i][0];
#pragma unroll
        for (int k = 1; k < REG_NW; ++k) a += s_red[i][k];
        v[i] = a;
    }
}

// R2q.m with Calculate_V_Omega_RANSAC_dr_ye.m:48's sign, as vo_final_wave forms u
__device__ inline void icp_r2q(const double *R, double *q)
{
#pragma clang fp contract(off)
    const double Tq = R[0] + R[4] + R[8] + 1;
    double a, b, c, d, S;
    if (Tq > 0.00000001) { S = 2 * sqrt(Tq); a = 0.25 * S; b = (R[5] - R[7]) / S; c = (R[6] - R[2]) / S; d = (R[1] - R[3]) / S; }
    else if (R[0] > R[4] && R[0] > R[8]) { S = 2 * sqrt(1.0 + R[0] - R[4] - R[8]); a = (R[5] - R[7]) / S; b = 0.25 * S; c = (R[1] + R[3]) / S; d = (R[6] + R[2]) / S; }
    else if (R[4] > R[8]) { S = 2 * sqrt(1.0 + R[4] - R[0] - R[8]); a = (R[6] - R[2]) / S; b = (R[1] + R[3]) / S; c = 0.25 * S; d = (R[5] + R[7]) / S; }
    else { S = 2 * sqrt(1.0 + R[8] - R[0] - R[4]); a = (R[1] - R[3]) / S; b = (R[6] + R[2]) / S; c = (R[5] + R[7]) / S; d = 0.25 * S; }
    q[0] = a; q[1] = -b; q[2] = -c; q[3] = -d;
}

__device__ inline double det3(const double *X)
{
#pragma clang fp contract(off)
    return X[0] * (X[4] * X[8] - X[5] * X[7]) - X[1] * (X[3] * X[8] - X[5] * X[6]) + X[2] * (X[3] * X[7] - X[4] * X[6]);
}

// :103-120 from the means and K (row-major, K = Sshifted Mshifted' / n), then :61-62 and the loop-control rule -- one thread
__device__ __noinline__ void icp_solve_update(IcpHead *h, const double *K, const double *mm, const double *ms, int p, double sum_d)
{
#pragma clang fp contract(off)
    double U[9], sv[3], V[9], R1[9], t1[3];
    vo_svd3(K, U, sv, V);
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) R1[3 * i + j] = (V[3 * i] * U[3 * j] + V[3 * i + 1] * U[3 * j + 1]) + V[3 * i + 2] * U[3 * j + 2];
    const double dt = det3(R1);
    if (dt < 0) {               // :115-119: B(3,3) = det(V U') on the column of the smallest singular value (svd's third)
        const int js = (sv[0] <= sv[1] && sv[0] <= sv[2]) ? 0 : (sv[1] <= sv[2] ? 1 : 2);
        for (int i = 0; i < 3; ++i) V[3 * i + js] = V[3 * i + js] * dt;
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) R1[3 * i + j] = (V[3 * i] * U[3 * j] + V[3 * i + 1] * U[3 * j + 1]) + V[3 * i + 2] * U[3 * j + 2];
    }
    for (int i = 0; i < 3; ++i) t1[i] = mm[i] - ((R1[3 * i] * ms[0] + R1[3 * i + 1] * ms[1]) + R1[3 * i + 2] * ms[2]);
    double Rn[9], tn[3];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) Rn[3 * i + j] = (R1[3 * i] * h->R[j] + R1[3 * i + 1] * h->R[3 + j]) + R1[3 * i + 2] * h->R[6 + j];
        tn[i] = ((R1[3 * i] * h->t[0] + R1[3 * i + 1] * h->t[1]) + R1[3 * i + 2] * h->t[2]) + t1[i];
    }
    for (int i = 0; i < 9; ++i) { h->R[i] = Rn[i]; h->R1[i] = R1[i]; }
    for (int i = 0; i < 3; ++i) { h->t[i] = tn[i]; h->t1[i] = t1[i]; }
    const int row = h->ctl.total, phase = h->ctl.phase;
    icp_advance(&h->ctl, p, sum_d);
    if (row < ICP_ITER_CAP) { h->log[3 * row] = phase; h->log[3 * row + 1] = p; h->log[3 * row + 2] = h->ctl.last_e; }
}

__global__ __launch_bounds__(REG_NTH) void k_icp_reg(IcpWork w)
{
#pragma clang fp contract(off)
    IcpHead *h = w.h;
    if (h->ctl.done) return;
    __shared__ int s_cnt[REG_NW];
    __shared__ double s_red[9][REG_NW];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n1 = min(h->ctl.n1, w.cap1);
    // :53-56 -- the claimed model indices, ascending
    int base = 0;
    for (int q0 = 0; q0 < n1; q0 += REG_NTH) {
        const int i = q0 + tid;
        int own = -1;
        if (i < n1) { own = w.owner[i]; w.owner[i] = -1; w.minD[i] = ~0ull; }        // (cleared for the next iteration)
        const int ok = own >= 0;
        const unsigned long long bal = __ballot(ok);
        if (lane == 0) s_cnt[wv] = __popcll(bal);
        __syncthreads();
        int off = 0, tot = 0;
#pragma unroll
        for (int k = 0; k < REG_NW; ++k) { const int cw = s_cnt[k]; if (k < wv) off += cw; tot += cw; }
        if (ok) {
            const int o = base + off + __popcll(bal & ((1ull << lane) - 1ull));      // o <= i < cap1
            w.corr_m[o] = i; w.corr_s[o] = own; w.corr_d[o] = w.bD[own];
        }
        base += tot;
        __syncthreads();
    }
    const int p = base;
    if (p < 3) {
        if (tid == 0) {
            const int row = h->ctl.total, phase = h->ctl.phase;
            icp_advance(&h->ctl, p, 0.0);
            if (row < ICP_ITER_CAP) { h->log[3 * row] = phase; h->log[3 * row + 1] = p; h->log[3 * row + 2] = 0.0; }
        }
        return;
    }
    __syncthreads();                                    // this workgroup's own writes of corr_* are read below by other threads
    // :104-108 -- the means, and sum(D)
    double s[7] = { 0, 0, 0, 0, 0, 0, 0 };
    for (int k = tid; k < p; k += REG_NTH) {
        const int im = w.corr_m[k], is = w.corr_s[k];
        s[0] += w.mx[im]; s[1] += w.my[im]; s[2] += w.mz[im];
        s[3] += w.sx[is]; s[4] += w.sy[is]; s[5] += w.sz[is];
        s[6] += w.corr_d[k];
    }
    block_sum<7>(s, s_red, lane, wv);
    double mm[3], ms[3];
    for (int i = 0; i < 3; ++i) { mm[i] = s[i] / p; ms[i] = s[3 + i] / p; }
    // :109-112 -- K = Sshifted Mshifted' / n
    double K[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
    for (int k = tid; k < p; k += REG_NTH) {
        const int im = w.corr_m[k], is = w.corr_s[k];
        const double M[3] = { w.mx[im] - mm[0], w.my[im] - mm[1], w.mz[im] - mm[2] };
        const double S[3] = { w.sx[is] - ms[0], w.sy[is] - ms[1], w.sz[is] - ms[2] };
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) K[3 * i + j] += S[i] * M[j];
    }
    block_sum<9>(K, s_red, lane, wv);
    if (tid == 0) {
        for (int i = 0; i < 9; ++i) K[i] = K[i] / p;
        icp_solve_update(h, K, mm, ms, p, s[6]);
    }
}

// :59-60, :86-87 for iteration `seq` (1-based): only when that iteration produced a transform
__global__ __launch_bounds__(256) void k_icp_apply(IcpWork w, int seq)
{
#pragma clang fp contract(off)
    const IcpHead *h = w.h;
    if (h->ctl.apply_seq != seq) return;
    const int n2 = min(h->ctl.n2, w.cap2);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n2) return;
    const double *R = h->R1, *T = h->t1;
    const double a = w.sx[i], b = w.sy[i], d = w.sz[i];
    w.sx[i] = ((R[0] * a + R[1] * b) + R[2] * d) + T[0];
    w.sy[i] = ((R[3] * a + R[4] * b) + R[5] * d) + T[1];
    w.sz[i] = ((R[6] * a + R[7] * b) + R[8] * d) + T[2];
}

// Rtot = R Rinit, ttot = R Tinit + t, u = [ttot; R2q(Rtot)], error (:100)
__global__ void k_icp_final(IcpHead *h)
{
#pragma clang fp contract(off)
    if (threadIdx.x != 0 || h->ctl.status == ICP_NOT_RUN || h->ctl.status == ICP_NONFINITE) return;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) h->Rtot[3 * i + j] = (h->R[3 * i] * h->Rinit[j] + h->R[3 * i + 1] * h->Rinit[3 + j]) + h->R[3 * i + 2] * h->Rinit[6 + j];
        h->ttot[i] = ((h->R[3 * i] * h->Tinit[0] + h->R[3 * i + 1] * h->Tinit[1]) + h->R[3 * i + 2] * h->Tinit[2]) + h->t[i];
    }
    for (int i = 0; i < 3; ++i) h->u[i] = h->ttot[i];
    icp_r2q(h->Rtot, h->u + 3);
    h->error = icp_error(&h->ctl);
}

// ---- host side
std::mutex g_pin_mu;
PinBlock g_pin;                                         // the library's pinned block of ICP results, grown on demand, held by one run at a time

int pin_reserve(IcpJob *job, size_t bytes)
{
    job->pin_lock = std::unique_lock<std::mutex>(g_pin_mu);
    PRE3_TRY(g_pin.reserve(bytes, (bytes + bytes / 4 + 65535) & ~(size_t)65535, PIN_PORTABLE));      // (one block for every device's runs)
    job->pin = g_pin.as<char>();
    return PRE3_OK;
}

// the device block laid out for cap1 model and cap2 source points; what travels back sits in front: [head | corr_m | corr_s | corr_d | sx sy sz | mpix | spix]
int icp_layout(IcpJob *job, int cap1, int cap2, IcpWork *w, size_t *o_model)
{
    const int nch = ceil_div(cap1, ICP_CHUNK);
    size_t o = up16(sizeof(IcpHead));
    job->cap1 = cap1; job->cap2 = cap2;
    job->o_corr_m = o; o += up16(sizeof(int32_t) * (size_t)cap1);
    job->o_corr_s = o; o += up16(sizeof(int32_t) * (size_t)cap1);
    job->o_corr_d = o; o += up16(sizeof(double) * (size_t)cap1);
    job->o_src = o; o += up16(sizeof(double) * 3 * (size_t)cap2);
    job->o_mpix = o; o += up16(sizeof(int32_t) * (size_t)cap1);
    job->o_spix = o; o += up16(sizeof(int32_t) * (size_t)cap2);
    job->pin_bytes = o;
    *o_model = o; o += up16(sizeof(double) * 3 * (size_t)cap1);
    const size_t o_pd = o; o += up16(sizeof(double) * (size_t)nch * cap2);
    const size_t o_pi = o; o += up16(sizeof(int32_t) * (size_t)nch * cap2);
    const size_t o_bD = o; o += up16(sizeof(double) * (size_t)cap2);
    const size_t o_bi = o; o += up16(sizeof(int32_t) * (size_t)cap2);
    const size_t o_min = o; o += up16(sizeof(unsigned long long) * (size_t)cap1);
    const size_t o_own = o; o += up16(sizeof(int32_t) * (size_t)cap1);
    if (job->with_cov) { job->o_cov = o; o += up16(sizeof(VoCov)); job->o_part = o; o += up16(ic_part_bytes(cap1 < cap2 ? cap1 : cap2)); }
    if (job->block != nullptr) { job->o_taken = o; o += 16; }
    if (job->block != nullptr) PRE3_TRY(job->block(job->owner, o, &job->d));
    else { PRE3_TRY(job->dev.alloc(o)); job->d = job->dev.as<char>(); }
    char *d = job->d;
    w->h = (IcpHead *)d; w->cap1 = cap1; w->cap2 = cap2;
    w->corr_m = (int32_t *)(d + job->o_corr_m); w->corr_s = (int32_t *)(d + job->o_corr_s); w->corr_d = (double *)(d + job->o_corr_d);
    w->sx = (double *)(d + job->o_src); w->sy = w->sx + cap2; w->sz = w->sy + cap2;
    w->mpix = (int32_t *)(d + job->o_mpix); w->spix = (int32_t *)(d + job->o_spix);
    w->mx = (double *)(d + *o_model); w->my = w->mx + cap1; w->mz = w->my + cap1;
    w->pd = (double *)(d + o_pd); w->pi = (int32_t *)(d + o_pi); w->bD = (double *)(d + o_bD); w->bi = (int32_t *)(d + o_bi);
    w->minD = (unsigned long long *)(d + o_min); w->owner = (int32_t *)(d + o_own);
    return PRE3_OK;
}

void head_image(IcpHead *h, int n1, int n2, double res, const double *Rinit, const double *Tinit)
{
    memset(h, 0, sizeof *h);
    icp_ctl_start(&h->ctl, n1, n2, res);
    for (int i = 0; i < 9; ++i) { h->R[i] = (i % 4 == 0) ? 1.0 : 0.0; h->Rinit[i] = Rinit ? Rinit[i] : h->R[i]; }
    for (int i = 0; i < 3; ++i) h->Tinit[i] = Tinit ? Tinit[i] : 0.0;
}

// k_icp_init, the 62 iterations, k_icp_final and the transfer of the front of the block -- all on st, no wait
int icp_queue_run(IcpJob *job, const IcpWork &w, const IcpOutputs &want, hipStream_t st)
{
    const int cap1 = w.cap1, cap2 = w.cap2;
    const int g2 = ceil_div(cap2, 256), gi = ceil_div(cap1 > cap2 ? cap1 : cap2, 256);
    const dim3 gnn(ceil_div(cap2, ICP_SRC_TILE), ceil_div(cap1, ICP_CHUNK));
    hipLaunchKernelGGL(k_icp_init, dim3(gi), dim3(256), 0, st, w);
    for (int it = 1; it <= ICP_ITER_CAP; ++it) {
        hipLaunchKernelGGL(k_icp_nn, gnn, dim3(ICP_NN_THREADS), 0, st, w);
        hipLaunchKernelGGL(k_icp_claim1, dim3(g2), dim3(256), 0, st, w);
        hipLaunchKernelGGL(k_icp_claim2, dim3(g2), dim3(256), 0, st, w);
        hipLaunchKernelGGL(k_icp_reg, dim3(1), dim3(REG_NTH), 0, st, w);
        hipLaunchKernelGGL(k_icp_apply, dim3(g2), dim3(256), 0, st, w, it);
    }
    hipLaunchKernelGGL(k_icp_final, dim3(1), dim3(64), 0, st, w.h);
    PRE3_HIP(hipGetLastError());
    char *d = job->d;
    if (job->with_cov) {            // the covariance of u over the final pairs: the state block, u, the pairs and both clouds are read where they lie
        IcCovArgs a{};
        a.ctl = &w.h->ctl; a.u_dev = w.h->u; a.cap = cap1 < cap2 ? cap1 : cap2; a.cap1 = cap1; a.cap2 = cap2; a.npix = job->cov_npix;
        a.corr_m = w.corr_m; a.corr_s = w.corr_s; a.mx = w.mx; a.my = w.my; a.mz = w.mz;
        a.sx = job->cov_x; a.sy = job->cov_y; a.sz = job->cov_z; a.spix = w.spix;
        PRE3_TRY(launch_icp_cov(a, (IcPart *)(d + job->o_part), (VoCov *)(d + job->o_cov), st));
    }
    size_t need = up16(sizeof(IcpHead));            // the prefix of the block the caller's outputs reach into
    if (want.corr || want.corr_pix) need = job->o_src;
    if (want.data2) need = job->o_mpix;
    if (want.corr_pix) need = job->pin_bytes;
    if (job->pin_back) {
        PRE3_HIP(hipMemcpyAsync(job->pin, d, need, hipMemcpyDeviceToHost, st));
        if (job->with_cov) PRE3_HIP(hipMemcpyAsync(job->pin + job->o_pin_cov, d + job->o_cov, sizeof(VoCov), hipMemcpyDeviceToHost, st));
    }
    job->st = st; job->queued = true;
    return PRE3_OK;
}

}  // namespace

int icp_check_args(const char *who, int stride, double res)
{
    PRE3_CHECK(stride >= 1, PRE3_E_ARG, "%s: stride must be at least 1", who);
    PRE3_CHECK(std::isfinite(res) && res > 0.0, PRE3_E_ARG, "%s: res must be positive and finite", who);
    return PRE3_OK;
}

int icp_job_queue_frames(IcpJob *job, const SrFrameView &v1, const SrFrameView &v2, int stride, double res, const double *Rinit, const double *Tinit,
                         const VoOut *vo_dev, const IcpOutputs &want, hipStream_t st)
{
    const int cap1 = v1.rows * v1.cols, cap2 = ceil_div(v2.rows, stride) * ceil_div(v2.cols, stride);
    IcpWork w{};
    size_t o_model = 0;
    PRE3_TRY(icp_layout(job, cap1, cap2, &w, &o_model));
    job->o_pin_cov = job->pin_bytes;
    job->o_pin_taken = job->o_pin_cov + (job->with_cov ? up16(sizeof(VoCov)) : 0);
    if (job->pin_back) PRE3_TRY(pin_reserve(job, job->o_pin_taken + (job->block != nullptr ? 16 : 0)));
    job->frames = true;
    job->cov_x = v2.x; job->cov_y = v2.y; job->cov_z = v2.z; job->cov_npix = v2.rows * v2.cols;
    if (job->block != nullptr) {        // head_image's bytes without the pinned block: nothing the host holds has to outlive the call
        PRE3_CHECK(Rinit == nullptr && Tinit == nullptr, PRE3_E_STATE, "icp_job_queue_frames: a run in an owner's block is seeded on the device");
        PRE3_HIP(hipMemsetAsync(w.h, 0, sizeof(IcpHead), st));
        hipLaunchKernelGGL(k_icp_head, dim3(1), dim3(64), 0, st, w.h, res);
    } else {
        head_image((IcpHead *)job->pin, 0, 0, res, Rinit, Tinit);
        PRE3_HIP(hipMemcpyAsync(w.h, job->pin, sizeof(IcpHead), hipMemcpyHostToDevice, st));
    }
    if (vo_dev) hipLaunchKernelGGL(k_icp_seed, dim3(1), dim3(64), 0, st, w.h, vo_dev);
    hipLaunchKernelGGL(k_icp_pack, dim3(2), dim3(REG_NTH), 0, st, w, v1.rows, v1.cols, stride, v1.x, v1.y, v1.z, v2.x, v2.y, v2.z);
    return icp_queue_run(job, w, want, st);
}

void icp_job_dev_view(const IcpJob *job, IcpDevView *v)
{
    const IcpHead *h = (const IcpHead *)job->d;
    v->ctl = &h->ctl; v->u = h->u; v->error = &h->error;
    v->cov = job->with_cov ? (const VoCov *)(job->d + job->o_cov) : nullptr;
    v->taken = job->block != nullptr ? (int32_t *)(job->d + job->o_taken) : nullptr;
}

// after the wait: the front of the block, checked, into the caller's arrays
int icp_job_collect(IcpJob *job, const char *who, const IcpOutputs &o)
{
    job->waited = true;
    if (o.cov_status) *o.cov_status = VC_NOT_COMPUTED;
    const IcpHead *h = (const IcpHead *)job->pin;
    const IcpCtl &c = h->ctl;
    if (c.status == ICP_NOT_RUN && c.done) { if (o.res) o.res->sta = ICP_NOT_RUN; return PRE3_OK; }
    PRE3_CHECK(c.status != ICP_NONFINITE, PRE3_E_NUMERIC, "%s: a coordinate of the model or of the source is not finite", who);
    PRE3_CHECK(c.done && (c.status == ICP_OK || c.status == ICP_FEW) && c.n1 >= 0 && c.n1 <= job->cap1 && c.n2 >= 0 && c.n2 <= job->cap2 && c.p >= 0 &&
               c.p <= c.n1 && c.p <= c.n2 && c.total <= ICP_ITER_CAP, PRE3_E_HIP, "%s: the device reports status %d after %d iterations (%d model, %d source points, p = %d)",
               who, c.status, c.total, c.n1, c.n2, c.p);
    const int p = c.total > 0 ? c.p : 0, n2 = c.n2, cap2 = job->cap2;
    if (o.res) {
        pre3_icp_result *r = o.res;
        memcpy(r->R, h->R, sizeof r->R); memcpy(r->t, h->t, sizeof r->t);
        memcpy(r->Rtot, h->Rtot, sizeof r->Rtot); memcpy(r->ttot, h->ttot, sizeof r->ttot); memcpy(r->u, h->u, sizeof r->u);
        r->error = h->error; r->sta = c.status; r->p = p; r->iters1 = c.it1; r->iters2 = c.it2; r->n_model = c.n1; r->n_source = c.n2; r->pad = 0;
    }
    const int32_t *cm = (const int32_t *)(job->pin + job->o_corr_m), *cs = (const int32_t *)(job->pin + job->o_corr_s);
    if (o.corr) {
        const double *cd = (const double *)(job->pin + job->o_corr_d);
        for (int k = 0; k < p; ++k) { o.corr[3 * k] = cm[k] + 1; o.corr[3 * k + 1] = cs[k] + 1; o.corr[3 * k + 2] = cd[k]; }
    }
    if (o.corr_pix && job->frames) {
        const int32_t *mp = (const int32_t *)(job->pin + job->o_mpix), *sp = (const int32_t *)(job->pin + job->o_spix);
        for (int k = 0; k < p; ++k) { o.corr_pix[2 * k] = mp[cm[k]]; o.corr_pix[2 * k + 1] = sp[cs[k]]; }
    }
    if (o.data2) {
        const double *s = (const double *)(job->pin + job->o_src);
        for (int j = 0; j < n2; ++j) { o.data2[3 * j] = s[j]; o.data2[3 * j + 1] = s[cap2 + j]; o.data2[3 * j + 2] = s[2 * (size_t)cap2 + j]; }
    }
    if (o.log) memcpy(o.log, h->log, sizeof h->log);
    if (job->with_cov) {
        const VoCov *cv = (const VoCov *)(job->pin + job->o_pin_cov);
        PRE3_CHECK(cv->status >= VC_NOT_COMPUTED && cv->status <= VC_UNUSABLE, PRE3_E_HIP, "%s: the device reports covariance status %d", who, cv->status);
        if (o.cov_status) *o.cov_status = cv->status;
        if (o.cov && cv->status == VC_VALID) memcpy(o.cov, cv->cov, sizeof cv->cov);
    }
    return PRE3_OK;
}

}  // namespace pre3

using namespace pre3;

extern "C" {

int pre3_icp_limits(int32_t out[4])
{
    PRE3_CHECK(out != nullptr, PRE3_E_ARG, "pre3_icp_limits: null output");
    out[0] = ICP_SRC_TILE; out[1] = ICP_CHUNK; out[2] = ICP_PTS; out[3] = ICP_ITER_CAP;
    return PRE3_OK;
}

int pre3_icp(int device, const double *data1, int n1, const double *data2, int n2, double res, const double Rinit[9], const double Tinit[3],
             pre3_icp_result *out, double *corr_out, double *data2_out, double *log_out)
{
    PRE3_CHECK(data1 != nullptr && data2 != nullptr && n1 >= 3 && n2 >= 3, PRE3_E_ARG, "pre3_icp: each cloud needs at least three points (n1 = %d, n2 = %d)", n1, n2);
    PRE3_TRY(icp_check_args("pre3_icp", 1, res));
    PRE3_TRY(select_device("pre3_icp", device));
    IcpJob job;
    IcpWork w{};
    size_t o_model = 0;
    PRE3_TRY(icp_layout(&job, n1, n2, &w, &o_model));
    // the pinned block carries the upload too: [head | ... | source SoA at o_src] and the model SoA behind the part that comes back
    const size_t up_bytes = job.pin_bytes + up16(sizeof(double) * 3 * (size_t)n1);
    PRE3_TRY(pin_reserve(&job, up_bytes));
    head_image((IcpHead *)job.pin, n1, n2, res, Rinit, Tinit);
    double *ps = (double *)(job.pin + job.o_src), *pm = (double *)(job.pin + job.pin_bytes);
    for (int j = 0; j < n2; ++j) { ps[j] = data2[3 * (size_t)j]; ps[n2 + j] = data2[3 * (size_t)j + 1]; ps[2 * (size_t)n2 + j] = data2[3 * (size_t)j + 2]; }
    for (int i = 0; i < n1; ++i) { pm[i] = data1[3 * (size_t)i]; pm[n1 + i] = data1[3 * (size_t)i + 1]; pm[2 * (size_t)n1 + i] = data1[3 * (size_t)i + 2]; }
    const hipStream_t st = 0;
    char *d = job.dev.as<char>();
    PRE3_HIP(hipMemcpyAsync(d, job.pin, sizeof(IcpHead), hipMemcpyHostToDevice, st));
    PRE3_HIP(hipMemcpyAsync(d + job.o_src, ps, sizeof(double) * 3 * (size_t)n2, hipMemcpyHostToDevice, st));
    PRE3_HIP(hipMemcpyAsync(d + o_model, pm, sizeof(double) * 3 * (size_t)n1, hipMemcpyHostToDevice, st));
    const IcpOutputs o{ out, corr_out, nullptr, data2_out, log_out };
    PRE3_TRY(icp_queue_run(&job, w, o, st));
    PRE3_HIP(hipStreamSynchronize(st));
    return icp_job_collect(&job, "pre3_icp", o);
}

int pre3_icp_nn_bench(int device, const double *data1, int n1, const double *data2, int n2, int reps, double *ms_per_launch_out)
{
    PRE3_CHECK(data1 != nullptr && data2 != nullptr && n1 >= 3 && n2 >= 3 && reps >= 1 && ms_per_launch_out != nullptr, PRE3_E_ARG, "pre3_icp_nn_bench: bad arguments");
    PRE3_TRY(select_device("pre3_icp_nn_bench", device));
    IcpJob job;
    IcpWork w{};
    size_t o_model = 0;
    PRE3_TRY(icp_layout(&job, n1, n2, &w, &o_model));
    PRE3_TRY(pin_reserve(&job, job.pin_bytes + up16(sizeof(double) * 3 * (size_t)n1)));
    head_image((IcpHead *)job.pin, n1, n2, 1.0, nullptr, nullptr);
    double *ps = (double *)(job.pin + job.o_src), *pm = (double *)(job.pin + job.pin_bytes);
    for (int j = 0; j < n2; ++j) { ps[j] = data2[3 * (size_t)j]; ps[n2 + j] = data2[3 * (size_t)j + 1]; ps[2 * (size_t)n2 + j] = data2[3 * (size_t)j + 2]; }
    for (int i = 0; i < n1; ++i) { pm[i] = data1[3 * (size_t)i]; pm[n1 + i] = data1[3 * (size_t)i + 1]; pm[2 * (size_t)n1 + i] = data1[3 * (size_t)i + 2]; }
    char *d = job.dev.as<char>();
    PRE3_HIP(hipMemcpy(d, job.pin, sizeof(IcpHead), hipMemcpyHostToDevice));
    PRE3_HIP(hipMemcpy(d + job.o_src, ps, sizeof(double) * 3 * (size_t)n2, hipMemcpyHostToDevice));
    PRE3_HIP(hipMemcpy(d + o_model, pm, sizeof(double) * 3 * (size_t)n1, hipMemcpyHostToDevice));
    const dim3 gnn(ceil_div(n2, ICP_SRC_TILE), ceil_div(n1, ICP_CHUNK));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    PRE3_HIP(hipEventCreate(&e0)); PRE3_HIP(hipEventCreate(&e1));
    float ms = 0;
    int rc = PRE3_OK;
    for (int r = 0; r < 3; ++r) hipLaunchKernelGGL(k_icp_nn, gnn, dim3(ICP_NN_THREADS), 0, 0, w);        // warm-up
    if (hipEventRecord(e0, 0) != hipSuccess) rc = PRE3_E_HIP;
    for (int r = 0; r < reps; ++r) hipLaunchKernelGGL(k_icp_nn, gnn, dim3(ICP_NN_THREADS), 0, 0, w);
    if (rc != PRE3_OK || hipEventRecord(e1, 0) != hipSuccess || hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess ||
        hipGetLastError() != hipSuccess) { set_error("pre3_icp_nn_bench: launch or event timing failed"); rc = PRE3_E_HIP; }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    PRE3_HIP(hipDeviceSynchronize());
    *ms_per_launch_out = ms / reps;
    return rc;
}

int pre3_icp_frames(pre3_sr_frame *prev, pre3_sr_frame *cur, int stride, double res, const double Rinit[9], const double Tinit[3], pre3_icp_result *out,
                    double *corr_out, int32_t *corr_pix_out, double *data2_out, double *log_out)
{
    const char *who = "pre3_icp_frames";
    PRE3_CHECK(prev != nullptr && cur != nullptr, PRE3_E_ARG, "%s: null handle", who);
    PRE3_CHECK(prev != cur, PRE3_E_ARG, "%s: prev and cur are the same handle", who);
    PRE3_TRY(icp_check_args(who, stride, res));
    SrFrameView v1, v2;
    PRE3_TRY(sr_frame_view(prev, &v1)); PRE3_TRY(sr_frame_view(cur, &v2));
    PRE3_CHECK(v1.device == v2.device && v1.rows == v2.rows && v1.cols == v2.cols, PRE3_E_ARG,
               "%s: the frames differ (device %d, %d x %d against device %d, %d x %d)", who, v1.device, v1.rows, v1.cols, v2.device, v2.rows, v2.cols);
    PRE3_TRY(select_device(who, v2.device));
    IcpJob job;
    const IcpOutputs o{ out, corr_out, corr_pix_out, data2_out, log_out };
    const hipStream_t st = v2.stream;
    PRE3_TRY(sr_frame_lend(prev, st));
    PRE3_TRY(icp_job_queue_frames(&job, v1, v2, stride, res, Rinit, Tinit, nullptr, o, st));
    PRE3_TRY(sr_frame_reclaim(prev, st));
    PRE3_HIP(hipStreamSynchronize(st));
    return icp_job_collect(&job, who, o);
}

}  // extern "C"
