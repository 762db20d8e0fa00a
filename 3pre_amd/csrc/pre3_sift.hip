// pre3_sift.hip -- sift_vedal(I) on a resident frame's image: the raw SIFT set made in the handle's keypoint block (pre3_sr_frame_sift; DESIGN.md
// section 25).
//   sift/sift_vedal.m:127-323     sift/gaussianss.m:133-227     sift/diffss.m:57-66     sift/imsmooth.c:44-80,128-160     sift/siftlocalmax.c:229-249
//   sift/siftrefinemx.c:150-303   sift/siftormx.c:138-253       sift/siftdescriptor.c:310-513
// All on the handle's stream, the arithmetic pre3_sift.h's:
//   k_sift_double   doubleSize of the image (uint8-class or double interpolation), one thread per output pixel
//   k_sift_smooth   one pass of the separable fp64 Gaussian (first along the columns, then along the rows), one thread per output pixel, the taps from the
//                   host-built plan; k_sift_halve takes every second row and column; k_sift_dog the five differences of an octave
//   k_sift_detect   ONE workgroup walks every octave's DoG in column-major linear-index order, +D then -D, 1024 points at a time: extremum test,
//                   boundary test and refinement are three predicates of one point, counted by ballot, and the accepted points are written in
//                   order (a ballot prefix per wave, the waves' sums through LDS)
//   k_sift_orient   one wave per refined point: every lane owns a private 36-bin histogram in LDS for the window columns it walks, the bins are summed
//                   over the lanes in lane order, lane 0 smooths and takes the peaks
//   k_sift_scan     one workgroup: the prefix sum of the peak counts, the oriented list in order, K
//   k_sift_desc     one wave per oriented point: lane-private 128-bin float histograms in LDS, summed in lane order, normalised by lane 0; writes the
//                   1-based frame and the descriptor into the keypoint block, the 0-based frame beside it, and or-reduces the descriptor bounds test
// No float atomics, every slot one writer (the only atomics are integer adds and an integer or): results are bit-equal from run to run.  Grids are
// sized by capacity; every stage reads its count from the word the previous one wrote; the host waits once.
#include <cmath>

#include "pre3_internal.h"
#include "pre3_sift.h"
#include "pre3_srframe.h"

namespace pre3 {

namespace {

constexpr int CAND_CAP = PRE3_SIFT_MAX_CANDIDATES, KP_CAP = PRE3_SR_MAX_KEYPOINTS;
constexpr int DB = 1024;                                     // threads of the two single-workgroup kernels
constexpr int W_NCAND = 4 * SIFT_MAX_OCTAVES, W_K = W_NCAND + 1, W_BAD = W_NCAND + 2, N_WORDS = W_NCAND + 4;

struct SiftOctaves { int O; int M[SIFT_MAX_OCTAVES], N[SIFT_MAX_OCTAVES]; double *gss[SIFT_MAX_OCTAVES], *dog[SIFT_MAX_OCTAVES]; };
struct SiftConsts { double sigma0, pow2[SIFT_NDOG], thresh, r; };

}  // namespace

struct SiftWork {
    SiftPlan plan;
    SiftOctaves oc;
    DevBlock dev_blk; PinBlock pin_blk;                      // the owners of dev and pin
    char *dev = nullptr;
    SiftLevelPlan *d_lev = nullptr;                          // [2][SIFT_NLEV]
    double *d_img = nullptr, *d_tmp0 = nullptr, *d_tmp1 = nullptr;
    double *d_cand = nullptr, *d_pth = nullptr, *d_okp = nullptr, *d_frm0 = nullptr;      // [CAND_CAP][4], [CAND_CAP][18], [KP_CAP][5], [KP_CAP][4]
    int32_t *d_npk = nullptr, *d_words = nullptr;
    char *pin = nullptr;                                     // words | frames + descriptors at capacity | 0-based frames
    bool has_result = false;
    int n_cand = -1;                                         // refined points of the last call; -1: none, or it overflowed
};

void sift_work_free(SiftWork *w)
{
    delete w;
}

namespace {

__global__ __launch_bounds__(256) void k_sift_double(const double *__restrict__ I, int M, int N, int strict, double *__restrict__ J)
{
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x, n = (size_t)4 * M * N;
    if (g >= n) return;
    const int r = (int)(g % (size_t)(2 * M)), c = (int)(g / (size_t)(2 * M));
    J[g] = sift_double_size(I, M, N, r, c, strict != 0);
}

// dir 0: along the columns (the samples of a column are contiguous), dir 1: along the rows
__global__ __launch_bounds__(256) void k_sift_smooth(const double *__restrict__ src, double *__restrict__ dst, int M, int N,
                                                     const SiftLevelPlan *__restrict__ lev, int dir)
{
    __shared__ double s_t[SIFT_MAX_TAPS];
    const int W = lev->W;
    if (threadIdx.x < SIFT_MAX_TAPS) s_t[threadIdx.x] = lev->taps[threadIdx.x];
    __syncthreads();
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= (size_t)M * N) return;
    const int r = (int)(g % (size_t)M), c = (int)(g / (size_t)M);
    dst[g] = dir == 0 ? sift_tap_sum(s_t, W, src + (size_t)c * M, 1, M, r) : sift_tap_sum(s_t, W, src + r, (size_t)M, N, c);
}

__global__ __launch_bounds__(256) void k_sift_halve(const double *__restrict__ src, int Ms, double *__restrict__ dst, int Md, int Nd)
{
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= (size_t)Md * Nd) return;
    const int r = (int)(g % (size_t)Md), c = (int)(g / (size_t)Md);
    dst[g] = src[(size_t)(2 * r) + (size_t)(2 * c) * Ms];
}

__global__ __launch_bounds__(256) void k_sift_dog(const double *__restrict__ gss, size_t n /* npix * SIFT_NDOG */, size_t npix, double *__restrict__ dog)
{
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= n) return;
    dog[g] = gss[g + npix] - gss[g];
}

__global__ __launch_bounds__(DB) void k_sift_detect(SiftOctaves oc, SiftConsts cs, double *__restrict__ cand, int32_t *__restrict__ words)
{
    __shared__ int s_cnt[3][DB / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    const double thr08 = 0.8 * cs.thresh;
    int n_ref = 0;
    for (int o = 0; o < oc.O; ++o) {
        const int M = oc.M[o], N = oc.N[o];
        const double *D = oc.dog[o];
        const long long npix = (long long)M * N, total = npix * (SIFT_NDOG - 2);
        int n_max = 0, n_in = 0, n_ref_o = 0;
        for (int pass = 0; pass < 2; ++pass) {
            const double sign = pass ? -1.0 : 1.0;
            for (long long base = 0; base < total; base += DB) {
                const long long e = base + tid;
                bool is_max = false, inside = false, ok = false;
                double out[3] = {0.0, 0.0, 0.0};
                if (e < total) {
                    const int s = 1 + (int)(e / npix);
                    const long long rem = e % npix;
                    const int x = (int)(rem / M), y = (int)(rem % M);
                    if (x >= 1 && x <= N - 2 && y >= 1 && y <= M - 2) {
                        is_max = sift_is_max(D, M, N, y, x, s, sign, thr08);
                        if (is_max) inside = sift_inside((double)x, (double)y, cs.pow2[s], cs.sigma0, M, N);
                        if (inside) ok = sift_refine(D, M, N, x, y, s, cs.thresh, cs.r, out);
                    }
                }
                const unsigned long long bm = __ballot(is_max), bi = __ballot(inside), bo = __ballot(ok);
                if (lane == 0) { s_cnt[0][wave] = __popcll(bm); s_cnt[1][wave] = __popcll(bi); s_cnt[2][wave] = __popcll(bo); }
                __syncthreads();
                int off = 0, tot = 0, tm = 0, ti = 0;
                for (int w = 0; w < DB / 64; ++w) {
                    const int c = s_cnt[2][w];
                    if (w < wave) off += c;
                    tot += c; tm += s_cnt[0][w]; ti += s_cnt[1][w];
                }
                if (ok) {
                    const int slot = n_ref + off + __popcll(bo & below);
                    if (slot < CAND_CAP) {
                        double *q = cand + 4 * (size_t)slot;
                        q[0] = out[0]; q[1] = out[1]; q[2] = out[2]; q[3] = (double)o;
                    }
                }
                n_ref += tot; n_ref_o += tot; n_max += tm; n_in += ti;
                __syncthreads();
            }
        }
        if (tid == 0) { words[4 * o] = n_max; words[4 * o + 1] = n_in; words[4 * o + 2] = n_ref_o; }
    }
    if (tid == 0) words[W_NCAND] = n_ref;
}

__global__ __launch_bounds__(64) void k_sift_orient(SiftOctaves oc, double sigma0, const double *__restrict__ cand, const int32_t *__restrict__ words,
                                                    int32_t *__restrict__ npk, double *__restrict__ pth)
{
    __shared__ double s_h[64][SIFT_NBINS + 1];
    __shared__ double s_H[SIFT_NBINS];
    const int c = blockIdx.x, lane = threadIdx.x;
    const int n = min(words[W_NCAND], CAND_CAP);
    if (c >= n) return;
    const double *q = cand + 4 * (size_t)c;
    const int o = (int)q[3], M = oc.M[o], N = oc.N[o];
    const SiftOrientSetup a = sift_orient_setup(q[0], q[1], q[2], sigma0, M, N);
    if (!a.ok) { if (lane == 0) npk[c] = 0; return; }        // siftormx.c:154-162 drops the point
    for (int b = 0; b < SIFT_NBINS; ++b) s_h[lane][b] = 0.0;
    const double *L = oc.gss[o] + (size_t)a.si * M * N;
    const int x0 = max(-a.W, 1 - a.xi), x1 = min(a.W, N - 2 - a.xi), y0 = max(-a.W, 1 - a.yi), y1 = min(a.W, M - 2 - a.yi);
    for (int xs = x0 + lane; xs <= x1; xs += 64)
        for (int ys = y0; ys <= y1; ++ys) {
            int bin;
            double amt;
            if (sift_orient_sample(L, M, a, xs, ys, &bin, &amt)) s_h[lane][bin] += amt;
        }
    __syncthreads();
    if (lane < SIFT_NBINS) {
        double h = 0.0;
        for (int l = 0; l < 64; ++l) h += s_h[l][lane];
        s_H[lane] = h;
    }
    __syncthreads();
    if (lane == 0) {
        double H[SIFT_NBINS], th[SIFT_MAX_PEAKS];
        for (int b = 0; b < SIFT_NBINS; ++b) H[b] = s_H[b];
        const int k = sift_orient_peaks(H, th);
        npk[c] = k;
        for (int j = 0; j < k; ++j) pth[(size_t)c * SIFT_MAX_PEAKS + j] = th[j];
    }
}

__global__ __launch_bounds__(DB) void k_sift_scan(const double *__restrict__ cand, const int32_t *__restrict__ npk, const double *__restrict__ pth,
                                                  int32_t *__restrict__ words, double *__restrict__ okp)
{
    __shared__ int s_w[DB / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = min(words[W_NCAND], CAND_CAP);
    int base = 0;
    for (int b = 0; b < n; b += DB) {
        const int c = b + tid;
        const int k = c < n ? npk[c] : 0;
        int v = k;
        for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(v, d, 64); if (lane >= d) v += t; }
        if (lane == 63) s_w[wave] = v;
        __syncthreads();
        int off = 0, tot = 0;
        for (int w = 0; w < DB / 64; ++w) { if (w < wave) off += s_w[w]; tot += s_w[w]; }
        if (k > 0) {
            const double *q = cand + 4 * (size_t)c;
            const int first = base + off + v - k;
            for (int j = 0; j < k; ++j) {
                const int slot = first + j;
                if (slot < KP_CAP) {
                    double *p = okp + 5 * (size_t)slot;
                    p[0] = q[0]; p[1] = q[1]; p[2] = q[2]; p[3] = pth[(size_t)c * SIFT_MAX_PEAKS + j]; p[4] = q[3];
                }
            }
            atomicAdd(&words[4 * (int)q[3] + 3], k);         // the octave's oriented count: an integer sum, the same in any order
        }
        base += tot;
        __syncthreads();
    }
    if (tid == 0) words[W_K] = base;
}

__global__ __launch_bounds__(64) void k_sift_desc(SiftOctaves oc, double sigma0, const double *__restrict__ okp, int32_t *__restrict__ words,
                                                  double *__restrict__ kp /* [K][4] frames, [K][128] descriptors behind them */,
                                                  double *__restrict__ frm0)
{
    __shared__ float s_d[128 * 64];                          // [bin][lane]
    __shared__ float s_out[128];
    const int k = blockIdx.x, lane = threadIdx.x;
    const int K = words[W_K];
    if (K > KP_CAP || k >= K) return;                        // an overflowing set is dropped whole
    const double *p = okp + 5 * (size_t)k;
    const int o = (int)p[4], M = oc.M[o], N = oc.N[o];
    const SiftDescSetup a = sift_desc_setup(p[0], p[1], p[2], p[3], sigma0, M, N);
    for (int b = 0; b < 128; ++b) s_d[b * 64 + lane] = 0.0f;
    if (a.ok) {                                              // siftdescriptor.c:417-424: a point out of bounds keeps its all-zero column
        const double *L = oc.gss[o] + (size_t)a.si * M * N + a.yi + (size_t)a.xi * M;
        const int x0 = max(-a.W, 1 - a.xi), x1 = min(a.W, N - 2 - a.xi), y0 = max(-a.W, 1 - a.yi), y1 = min(a.W, M - 2 - a.yi);
        for (int dxi = x0 + lane; dxi <= x1; dxi += 64)
            for (int dyi = y0; dyi <= y1; ++dyi) {
                float mod, angle, w[8];
                int bins[8];
                sift_gradient(L + (ptrdiff_t)dxi * M + dyi, M, &mod, &angle);
                const int nb = sift_desc_sample(a, mod, angle, dxi, dyi, bins, w);
                for (int j = 0; j < nb; ++j) s_d[bins[j] * 64 + lane] += w[j];
            }
    }
    __syncthreads();
    for (int b = lane; b < 128; b += 64) {
        float h = 0.0f;
        for (int l = 0; l < 64; ++l) h += s_d[b * 64 + l];
        s_out[b] = h;
    }
    __syncthreads();
    if (lane == 0) {
        float d[128];
        for (int b = 0; b < 128; ++b) d[b] = s_out[b];
        if (a.ok) sift_desc_finish(d);
        for (int b = 0; b < 128; ++b) s_out[b] = d[b];
        double f[4];
        sift_frame(o, sigma0, p[0], p[1], p[2], p[3], f);
        double *f0 = frm0 + 4 * (size_t)k, *f1 = kp + 4 * (size_t)k;
        f0[0] = f[0]; f0[1] = f[1]; f0[2] = f[2]; f0[3] = f[3];
        f1[0] = f[0] + 1.0; f1[1] = f[1] + 1.0; f1[2] = f[2]; f1[3] = f[3];      // SIFT_extract_save.m:55-56
    }
    __syncthreads();
    double *des = kp + 4 * (size_t)K + 128 * (size_t)k;
    bool bad = false;
    for (int b = lane; b < 128; b += 64) { const double v = (double)s_out[b]; des[b] = v; bad |= sift_desc_out_of_bounds(v); }
    if (__ballot(bad) != 0ull && lane == 0) atomicOr(&words[W_BAD], 1);
}

int sift_work_get(pre3_sr_frame *f, const SiftPlan &plan)
{
    if (f->sift != nullptr) return PRE3_OK;
    SiftWork *w = new SiftWork;
    w->plan = plan;
    const size_t npix = (size_t)f->rows * f->cols, n0 = 4 * npix;
    size_t off = 0;
    auto take = [&off](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_lev = take(sizeof(SiftLevelPlan) * 2 * SIFT_NLEV), o_img = take(8 * npix), o_t0 = take(8 * n0), o_t1 = take(8 * n0);
    size_t o_gss[SIFT_MAX_OCTAVES], o_dog[SIFT_MAX_OCTAVES];
    for (int o = 0; o < plan.O; ++o) {
        const size_t n = (size_t)plan.rows[o] * plan.cols[o];
        o_gss[o] = take(8 * n * SIFT_NLEV); o_dog[o] = take(8 * n * SIFT_NDOG);
    }
    const size_t o_cand = take(8 * 4 * (size_t)CAND_CAP), o_pth = take(8 * (size_t)SIFT_MAX_PEAKS * CAND_CAP), o_npk = take(4 * (size_t)CAND_CAP);
    const size_t o_okp = take(8 * 5 * (size_t)KP_CAP), o_frm0 = take(8 * 4 * (size_t)KP_CAP), o_words = take(4 * N_WORDS);
    const size_t pin_bytes = 1024 + 8 * (size_t)(4 + 128) * KP_CAP + 8 * 4 * (size_t)KP_CAP;
    int rc = w->dev_blk.reserve(off, off, Zero::on_stream(f->stream));
    if (rc == PRE3_OK) rc = w->pin_blk.reserve(pin_bytes, pin_bytes, PIN_DEFAULT);
    if (rc != PRE3_OK) { delete w; return rc; }
    w->dev = w->dev_blk.as<char>(); w->pin = w->pin_blk.as<char>();
    f->sift = w;
    w->d_lev = (SiftLevelPlan *)(w->dev + o_lev); w->d_img = (double *)(w->dev + o_img);
    w->d_tmp0 = (double *)(w->dev + o_t0); w->d_tmp1 = (double *)(w->dev + o_t1);
    w->oc.O = plan.O;
    for (int o = 0; o < SIFT_MAX_OCTAVES; ++o) {
        w->oc.M[o] = o < plan.O ? plan.rows[o] : 0; w->oc.N[o] = o < plan.O ? plan.cols[o] : 0;
        w->oc.gss[o] = o < plan.O ? (double *)(w->dev + o_gss[o]) : nullptr; w->oc.dog[o] = o < plan.O ? (double *)(w->dev + o_dog[o]) : nullptr;
    }
    w->d_cand = (double *)(w->dev + o_cand); w->d_pth = (double *)(w->dev + o_pth); w->d_npk = (int32_t *)(w->dev + o_npk);
    w->d_okp = (double *)(w->dev + o_okp); w->d_frm0 = (double *)(w->dev + o_frm0); w->d_words = (int32_t *)(w->dev + o_words);
    memcpy(w->pin, &plan.lev[0][0], sizeof(SiftLevelPlan) * 2 * SIFT_NLEV);
    PRE3_HIP(hipMemcpyAsync(w->d_lev, w->pin, sizeof(SiftLevelPlan) * 2 * SIFT_NLEV, hipMemcpyHostToDevice, f->stream));
    PRE3_HIP(hipStreamSynchronize(f->stream));               // the pinned block is reused by the call that follows
    return PRE3_OK;
}

inline unsigned blocks256(size_t n) { return (unsigned)((n + 255) / 256); }

// imsmooth.c:128-160 from src into dst (both M x N); tmp holds the column pass
int launch_smooth(pre3_sr_frame *f, const SiftWork *w, const SiftLevelPlan *host, const SiftLevelPlan *dev, const double *src, double *dst, double *tmp,
                  int M, int N)
{
    const size_t n = (size_t)M * N;
    if (!(host->sigma > 0.01)) {
        if (src != dst) PRE3_HIP(hipMemcpyAsync(dst, src, 8 * n, hipMemcpyDeviceToDevice, f->stream));
        return PRE3_OK;
    }
    hipLaunchKernelGGL(k_sift_smooth, dim3(blocks256(n)), dim3(256), 0, f->stream, src, tmp, M, N, dev, 0);
    hipLaunchKernelGGL(k_sift_smooth, dim3(blocks256(n)), dim3(256), 0, f->stream, (const double *)tmp, dst, M, N, dev, 1);
    PRE3_HIP(hipGetLastError());
    return PRE3_OK;
}

int sift_impl(pre3_sr_frame *f, const double *image, int strict, int one_based, int32_t *K_out, double *frm_out, double *des_out, int32_t *counts_out,
              bool *touched)
{
    PRE3_CHECK(f != nullptr && K_out != nullptr, PRE3_E_ARG, "pre3_sr_frame_sift: null argument");
    SiftPlan plan;
    PRE3_CHECK((f->rows < f->cols ? f->rows : f->cols) >= 8 && sift_plan(f->rows, f->cols, &plan), PRE3_E_ARG,
               "pre3_sr_frame_sift: a %d x %d image has no octave (sift_vedal.m:132 needs min(rows, cols) >= 8)", f->rows, f->cols);
    const size_t npix = (size_t)f->rows * f->cols;
    if (image != nullptr)
        for (size_t i = 0; i < npix; ++i) {
            const double v = image[i];
            PRE3_CHECK(std::isfinite(v), PRE3_E_ARG, "pre3_sr_frame_sift: the image is not finite at row %d, column %d", (int)(i % f->rows) + 1,
                       (int)(i / f->rows) + 1);
            PRE3_CHECK(!strict || (v >= 0.0 && v <= 255.0 && v == floor(v)), PRE3_E_ARG,
                       "pre3_sr_frame_sift: strict_reference takes a uint8 image; %g at row %d, column %d", v, (int)(i % f->rows) + 1, (int)(i / f->rows) + 1);
        }
    else
        PRE3_CHECK(f->loaded, PRE3_E_STATE, "pre3_sr_frame_sift: no frame has been loaded and no image was given");
    PRE3_TRY(select_device("pre3_sr_frame_sift", f->device));
    *K_out = 0;
    PRE3_HIP(hipStreamSynchronize(f->stream));               // the staging block and the keypoint block are free again
    PRE3_TRY(sift_work_get(f, plan));
    SiftWork *w = f->sift;
    PRE3_TRY(sr_frame_kp_reserve(f, kp_layout(KP_CAP, 4, DESC_DIM).total));
    if (image != nullptr) PRE3_TRY(sr_grow_stage(f, 8 * npix));
    *touched = true;
    f->kp_valid = 1; f->kp_K = 0; f->kp_ldf = 4; f->kp_ND = DESC_DIM; f->kp_gate = 0; f->kp_n = 0;      // a valid empty record until the count is in
    f->kp_K_in = 0; f->kp_o_des_in = 0; f->kp_raw_ok = true;
    w->has_result = false; w->n_cand = -1;
    const double *img = f->filt + 3 * npix;
    if (image != nullptr) {
        memcpy(f->stage, image, 8 * npix);
        PRE3_HIP(hipMemcpyAsync(w->d_img, f->stage, 8 * npix, hipMemcpyHostToDevice, f->stream));
        img = w->d_img;
    }
    PRE3_HIP(hipMemsetAsync(w->d_words, 0, 4 * N_WORDS, f->stream));
    const SiftOctaves &oc = w->oc;
    // gaussianss.m:93-96,133-203
    hipLaunchKernelGGL(k_sift_double, dim3(blocks256(4 * npix)), dim3(256), 0, f->stream, img, f->rows, f->cols, strict, w->d_tmp0);
    PRE3_HIP(hipGetLastError());
    for (int o = 0; o < oc.O; ++o) {
        const int M = oc.M[o], N = oc.N[o], pl = o == 0 ? 0 : 1;
        const size_t n = (size_t)M * N;
        if (o > 0) {
            hipLaunchKernelGGL(k_sift_halve, dim3(blocks256(n)), dim3(256), 0, f->stream,
                               (const double *)(oc.gss[o - 1] + (size_t)SIFT_SBEST_LEVEL * oc.M[o - 1] * oc.N[o - 1]), oc.M[o - 1], w->d_tmp0, M, N);
            PRE3_HIP(hipGetLastError());
        }
        PRE3_TRY(launch_smooth(f, w, &w->plan.lev[pl][0], w->d_lev + pl * SIFT_NLEV, w->d_tmp0, oc.gss[o], w->d_tmp1, M, N));
        for (int l = 1; l < SIFT_NLEV; ++l)
            PRE3_TRY(launch_smooth(f, w, &w->plan.lev[pl][l], w->d_lev + pl * SIFT_NLEV + l, oc.gss[o] + (size_t)(l - 1) * n, oc.gss[o] + (size_t)l * n,
                                   w->d_tmp1, M, N));
        hipLaunchKernelGGL(k_sift_dog, dim3(blocks256(n * SIFT_NDOG)), dim3(256), 0, f->stream, (const double *)oc.gss[o], n * SIFT_NDOG, n, oc.dog[o]);
        PRE3_HIP(hipGetLastError());
    }
    SiftConsts cs;
    cs.sigma0 = plan.sigma0; cs.thresh = SIFT_THRESH; cs.r = SIFT_R;
    for (int i = 0; i < SIFT_NDOG; ++i) cs.pow2[i] = plan.pow2[i];
    hipLaunchKernelGGL(k_sift_detect, dim3(1), dim3(DB), 0, f->stream, oc, cs, w->d_cand, w->d_words);
    PRE3_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_sift_orient, dim3(CAND_CAP), dim3(64), 0, f->stream, oc, plan.sigma0, (const double *)w->d_cand, (const int32_t *)w->d_words,
                       w->d_npk, w->d_pth);
    PRE3_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_sift_scan, dim3(1), dim3(DB), 0, f->stream, (const double *)w->d_cand, (const int32_t *)w->d_npk, (const double *)w->d_pth,
                       w->d_words, w->d_okp);
    PRE3_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_sift_desc, dim3(KP_CAP), dim3(64), 0, f->stream, oc, plan.sigma0, (const double *)w->d_okp, w->d_words, (double *)f->kp, w->d_frm0);
    PRE3_HIP(hipGetLastError());
    // the one transfer back: the words, and at capacity whatever the caller asked for (K is not known yet)
    int32_t *words = (int32_t *)w->pin;
    double *p_kp = (double *)(w->pin + 1024), *p_f0 = p_kp + (size_t)(4 + 128) * KP_CAP;
    PRE3_HIP(hipMemcpyAsync(words, w->d_words, 4 * N_WORDS, hipMemcpyDeviceToHost, f->stream));
    if (des_out != nullptr) PRE3_HIP(hipMemcpyAsync(p_kp, f->kp, 8 * (size_t)(4 + 128) * KP_CAP, hipMemcpyDeviceToHost, f->stream));
    else if (frm_out != nullptr && one_based) PRE3_HIP(hipMemcpyAsync(p_kp, f->kp, 8 * (size_t)4 * KP_CAP, hipMemcpyDeviceToHost, f->stream));
    if (frm_out != nullptr && !one_based) PRE3_HIP(hipMemcpyAsync(p_f0, w->d_frm0, 8 * (size_t)4 * KP_CAP, hipMemcpyDeviceToHost, f->stream));
    PRE3_HIP(hipStreamSynchronize(f->stream));
    if (counts_out != nullptr) memcpy(counts_out, words, sizeof(int32_t) * 4 * oc.O);
    w->has_result = true;
    const int n_cand = words[W_NCAND], K = words[W_K];
    PRE3_CHECK(n_cand >= 0 && K >= 0, PRE3_E_HIP, "pre3_sr_frame_sift: the device reports %d refined and %d oriented keypoints", n_cand, K);
    PRE3_CHECK(n_cand <= CAND_CAP, PRE3_E_NOMEM, "pre3_sr_frame_sift: %d refined keypoints, the capacity is %d", n_cand, CAND_CAP);
    PRE3_CHECK(K <= KP_CAP, PRE3_E_NOMEM, "pre3_sr_frame_sift: %d keypoints, the capacity is %d", K, KP_CAP);
    w->n_cand = n_cand;
    *K_out = K;
    f->kp_K = K; f->kp_K_in = K; f->kp_o_des_in = sizeof(double) * 4 * (size_t)K; f->kp_raw_ok = words[W_BAD] == 0;
    if (frm_out != nullptr) memcpy(frm_out, one_based ? p_kp : p_f0, 8 * (size_t)4 * K);
    if (des_out != nullptr) memcpy(des_out, p_kp + 4 * (size_t)K, 8 * (size_t)128 * K);
    return PRE3_OK;
}

}  // namespace

}  // namespace pre3

using namespace pre3;

extern "C" {

int pre3_sift_plan_get(int rows, int cols, int32_t *O_out, int32_t *oct_rows, int32_t *oct_cols, double *sigma0_out, double *pow2_out, double *sigma_out,
                       int32_t *W_out, double *taps_out)
{
    SiftPlan plan;
    PRE3_CHECK(O_out != nullptr, PRE3_E_ARG, "pre3_sift_plan_get: null argument");
    PRE3_CHECK(rows >= 8 && cols >= 8 && (long long)rows * cols <= (1ll << 26) && sift_plan(rows, cols, &plan), PRE3_E_ARG,
               "pre3_sift_plan_get: a %d x %d image has no octave (sift_vedal.m:132 needs min(rows, cols) >= 8)", rows, cols);
    *O_out = plan.O;
    if (sigma0_out) *sigma0_out = plan.sigma0;
    if (pow2_out) for (int i = 0; i < SIFT_NDOG; ++i) pow2_out[i] = plan.pow2[i];
    for (int o = 0; o < plan.O; ++o) {
        if (oct_rows) oct_rows[o] = plan.rows[o];
        if (oct_cols) oct_cols[o] = plan.cols[o];
        for (int l = 0; l < SIFT_NLEV; ++l) {
            const SiftLevelPlan &p = plan.lev[o == 0 ? 0 : 1][l];
            const size_t i = (size_t)o * SIFT_NLEV + l;
            if (sigma_out) sigma_out[i] = p.sigma;
            if (W_out) W_out[i] = p.W;
            if (taps_out) memcpy(taps_out + i * PRE3_SIFT_MAX_TAPS, p.taps, sizeof(double) * PRE3_SIFT_MAX_TAPS);
        }
    }
    return PRE3_OK;
}

int pre3_sr_frame_sift(pre3_sr_frame *f, const double *image, int strict_reference, int one_based, int32_t *K_out, double *frm_out, double *des_out,
                       int32_t *counts_out)
{
    bool touched = false;
    const int rc = sift_impl(f, image, strict_reference != 0, one_based != 0, K_out, frm_out, des_out, counts_out, &touched);
    if (rc != PRE3_OK && touched) { f->kp_K = 0; f->kp_n = 0; f->kp_K_in = 0; }      // a call that failed behind its checks leaves a valid empty record
    return rc;
}

int pre3_sr_frame_sift_level(pre3_sr_frame *f, int octave, int level, int dog, double *out)
{
    PRE3_CHECK(f != nullptr && out != nullptr, PRE3_E_ARG, "pre3_sr_frame_sift_level: null argument");
    PRE3_CHECK(f->sift != nullptr && f->sift->has_result, PRE3_E_STATE, "pre3_sr_frame_sift_level: the handle holds no scale space (no pre3_sr_frame_sift yet)");
    const SiftWork *w = f->sift;
    PRE3_CHECK(octave >= 0 && octave < w->oc.O && level >= 0 && level < (dog ? SIFT_NDOG : SIFT_NLEV), PRE3_E_ARG,
               "pre3_sr_frame_sift_level: octave %d, level %d outside %d octaves of %d levels", octave, level, w->oc.O, dog ? SIFT_NDOG : SIFT_NLEV);
    PRE3_TRY(select_device("pre3_sr_frame_sift_level", f->device));
    const size_t n = (size_t)w->oc.M[octave] * w->oc.N[octave];
    PRE3_HIP(hipMemcpyAsync(out, (dog ? w->oc.dog[octave] : w->oc.gss[octave]) + (size_t)level * n, 8 * n, hipMemcpyDeviceToHost, f->stream));
    PRE3_HIP(hipStreamSynchronize(f->stream));
    return PRE3_OK;
}

int pre3_sr_frame_sift_refined(pre3_sr_frame *f, int32_t *n_out, double *out)
{
    PRE3_CHECK(f != nullptr && n_out != nullptr, PRE3_E_ARG, "pre3_sr_frame_sift_refined: null argument");
    PRE3_CHECK(f->sift != nullptr && f->sift->has_result && f->sift->n_cand >= 0, PRE3_E_STATE,
               "pre3_sr_frame_sift_refined: the handle holds no refined list (no pre3_sr_frame_sift yet, or it overflowed)");
    const SiftWork *w = f->sift;
    *n_out = w->n_cand;
    if (out == nullptr || w->n_cand == 0) return PRE3_OK;
    PRE3_TRY(select_device("pre3_sr_frame_sift_refined", f->device));
    PRE3_HIP(hipMemcpyAsync(out, w->d_cand, 8 * 4 * (size_t)w->n_cand, hipMemcpyDeviceToHost, f->stream));
    PRE3_HIP(hipStreamSynchronize(f->stream));
    return PRE3_OK;
}

}  // extern "C"
