// pre3_sr.hip -- one resident, conditioned SR4000 frame per .dat scan and the keypoint stage on it (pre3_sr_frame_*).
//   read_xyz_sr4000.m:8-21, read_image_sr4000.m:10-24, normalzie_image.m:4             (mode 0: sigma = 2, zero padding)
//   code_from_dr_ye/read_sr4000_data_dr_ye.m:8,11-21,42,70,88-90                       (mode 1: sigma = 1, replicated border)
//   SIFT_extract_save.m:71-88 over inittialize_depth_my_version.m:16,40-45,74-92       (gate 0: the depth gate, XYZ_DATA, rho)
//   code_from_dr_ye/confidence_filtering.m:1-13                                        (gate 1)
//   aux_code/compensate_badpixel_soonhac.m:5-14, code_from_dr_ye/read_image_sr4000_dr_ye.m:21-24   (the compensation in front of the Gaussian, section 32)
// Three launches, all fp64, on the handle's own stream:
//   k_sr_maxima     one workgroup: imax (the largest unsaturated amplitude), cmax (max(confidence_map(:)), NaNs skipped) and, under form 1, the number
//                   of pixels with conf < cutoff -- xor butterfly per wave, the waves combined through LDS.
//   k_sr_condition  16 x 16 tiles with a one-pixel halo in LDS: the filtered x, y, z and the filtered uint8 image.  Halo pixels recompute the
//                   normalisation from the raw amplitude; the image exists only filtered.  The compensated instantiations stage a two-pixel halo and
//                   fill the same tiles with the compensated values first.
//   k_sr_keypoints  a workgroup owns 256 consecutive keypoints; its base offset is the predicate of every earlier keypoint re-evaluated by itself
//                   (ballot + popcount), ranks inside it are a ballot prefix per wave plus the wave sums through LDS; then one wave per kept keypoint
//                   copies its frame entries and descriptor to slot `rank`.
// No workgroup waits on another, there are no atomics, every output slot has one writer: results are bit-equal from run to run.  The arithmetic is
// pre3_sr.h's, compiled without contraction.
#include <cmath>

#include "pre3_internal.h"
#include "pre3_sr.h"
#include "pre3_srframe.h"

namespace pre3 {

namespace {

constexpr int ST = 16;              // tile edge of k_sr_condition
constexpr int SH = ST + 2;          // ... with its halo
constexpr int SW = ST + 4;          // ... with the two-pixel halo of the compensated forms: a Gaussian tap one pixel outside the tile needs the 3 x 3 around it
constexpr int MF = 256;             // threads of k_sr_medfilt3
constexpr int MB = 1024;            // threads of k_sr_maxima's one workgroup
constexpr int KB = 256;             // keypoints (and threads) per workgroup of k_sr_keypoints
constexpr int KW = KB / 64;
static_assert(PRE3_SR_MAX_KEYPOINTS % KB == 0 && PRE3_SR_MAX_KEYPOINTS / KB == 32, "32 predicate batches per workgroup at the cap");

struct SrWeights { double w[9]; };

__global__ __launch_bounds__(MB) void k_sr_maxima(int npix, const double *__restrict__ amp, const double *__restrict__ conf /* null: none */,
                                                  int count_bad, double cutoff, double *__restrict__ out /* imax, cmax, n_bad */)
{
    __shared__ double s_a[MB / 64], s_c[MB / 64];
    __shared__ int s_n[MB / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double a = 0.0, c = NAN;
    int n = 0;                                               // pixels with conf < cutoff (form 1 only): at most npix <= 2^26
    for (int i = tid; i < npix; i += MB) {
        const double v = amp[i];
        if (v <= SR_SATURATED && v > a) a = v;               // read_image_sr4000.m:12-17: saturated pixels count as 0
        if (conf != nullptr) { const double cv = conf[i]; c = sr_nanmax(c, cv); n += (count_bad != 0 && sr_is_bad(true, cv, cutoff)) ? 1 : 0; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double a2 = __shfl_xor(a, o, 64), c2 = __shfl_xor(c, o, 64);
        a = a2 > a ? a2 : a;
        c = sr_nanmax(c, c2);
        n += __shfl_xor(n, o, 64);
    }
    if (lane == 0) { s_a[wave] = a; s_c[wave] = c; s_n[wave] = n; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < MB / 64; ++w) { a = s_a[w] > a ? s_a[w] : a; c = sr_nanmax(c, s_c[w]); n += s_n[w]; }
        out[0] = a; out[1] = c; out[2] = (double)n;
    }
}

// the 3 x 3 median around (lr, lc) of a staged SW x SW tile [lc * SW + lr]; 1 <= lr, lc <= SW - 2
__device__ inline double tile_median9(const double *s, int lr, int lc)
{
    double p[9];
#pragma unroll
    for (int dj = 0; dj < 3; ++dj)
#pragma unroll
        for (int di = 0; di < 3; ++di) p[3 * dj + di] = s[(lc + dj - 1) * SW + lr + di - 1];
    return sr_median9(p);
}

// COMP: the compensation in front of the Gaussian.  SR_COMP_NONE is the launch as it was before there was one.
//   SR_COMP_BADPIXEL      x, y, z, U and the confidence staged with a TWO-pixel halo (SW x SW), every pixel outside the image read at the clamped
//                         coordinates -- one step out, that is medfilt2's 'symmetric' mirror; two steps out, the value is never read.  Then the
//                         SH x SH tile the nine-tap sums read: at a pixel inside the image bad ? median9 of the staged window : the staged pixel;
//                         outside it 0.0 (mode 0) or the same expression at the clamped coordinates (mode 1).
//   SR_COMP_IMAGE_MEDIAN  only U is staged SW x SW, with 0.0 outside the image (medfilt2's default padding); its SH x SH tile is the median at every
//                         pixel, outside the image as above; x, y, z go straight into their SH x SH tiles as in SR_COMP_NONE.
// Index arithmetic: SH-tile (lr, lc) is the pixel (r0 + lr - 1, c0 + lc - 1); clamped into the image it lies in [r0 - 1, r0 + ST] x [c0 - 1, c0 + ST]
// still (the tile holds at least one image row and column), i.e. at SW-tile (cr - r0 + 2, cc - c0 + 2) in [1, SW - 2]: its window stays in [0, SW - 1].
template <int COMP>
__global__ __launch_bounds__(ST * ST) void k_sr_condition(int rows, int cols, int mode, SrWeights W, const double *__restrict__ raw,
                                                          const double *__restrict__ maxima, double *__restrict__ filt, int has_conf, double cutoff)
{
    __shared__ double s_p[4][SH * SH];                       // x, y, z, uint8 image; [lc * SH + lr]
    const size_t npix = (size_t)rows * cols;
    const double *Z = raw, *X = raw + npix, *Y = raw + 2 * npix, *A = raw + 3 * npix;
    const int tid = threadIdx.x, r0 = blockIdx.x * ST, c0 = blockIdx.y * ST;
    const double imax = maxima[0];
    if constexpr (COMP == SR_COMP_NONE) {
        for (int i = tid; i < SH * SH; i += ST * ST) {
            const int lr = i % SH, lc = i / SH;
            int gr = r0 + lr - 1, gc = c0 + lc - 1;
            const bool inside = gr >= 0 && gr < rows && gc >= 0 && gc < cols;
            double x = 0.0, y = 0.0, z = 0.0, u = 0.0;           // mode 0: imfilter(.., 'same') pads with zeros (the uint8 image too)
            if (inside || mode == 1) {                           // mode 1: 'replicate' reads the nearest edge pixel
                gr = min(max(gr, 0), rows - 1); gc = min(max(gc, 0), cols - 1);
                const size_t g = (size_t)gc * rows + gr;
                x = X[g]; y = Y[g]; z = Z[g]; u = sr_norm_pixel(A[g], imax);
            }
            s_p[0][i] = x; s_p[1][i] = y; s_p[2][i] = z; s_p[3][i] = u;
        }
    } else {
        constexpr int NW = COMP == SR_COMP_BADPIXEL ? 5 : 1;     // staged with the two-pixel halo: x, y, z, U, confidence -- or U alone
        __shared__ double s_w[NW][SW * SW];                      // [lc * SW + lr]
        const double *Cf = raw + 4 * npix;
        for (int i = tid; i < SW * SW; i += ST * ST) {
            const int lr = i % SW, lc = i / SW;
            int gr = r0 + lr - 2, gc = c0 + lc - 2;
            const bool inside = gr >= 0 && gr < rows && gc >= 0 && gc < cols;
            gr = min(max(gr, 0), rows - 1); gc = min(max(gc, 0), cols - 1);
            const size_t g = (size_t)gc * rows + gr;
            if constexpr (COMP == SR_COMP_BADPIXEL) {
                s_w[0][i] = X[g]; s_w[1][i] = Y[g]; s_w[2][i] = Z[g]; s_w[3][i] = sr_norm_pixel(A[g], imax);
                s_w[4][i] = has_conf ? Cf[g] : 0.0;
            } else {
                s_w[0][i] = inside ? sr_norm_pixel(A[g], imax) : 0.0;
            }
        }
        __syncthreads();
        for (int i = tid; i < SH * SH; i += ST * ST) {
            const int lr = i % SH, lc = i / SH;
            const int gr = r0 + lr - 1, gc = c0 + lc - 1;
            const bool inside = gr >= 0 && gr < rows && gc >= 0 && gc < cols;
            double x = 0.0, y = 0.0, z = 0.0, u = 0.0;           // mode 0: a tap outside the image is a literal 0.0, compensation or not
            if (inside || mode == 1) {                           // mode 1: the compensated edge pixel
                const int cr = min(max(gr, 0), rows - 1), cc = min(max(gc, 0), cols - 1);
                const int wr = cr - r0 + 2, wc = cc - c0 + 2, j = wc * SW + wr;
                if constexpr (COMP == SR_COMP_BADPIXEL) {
                    const bool bad = sr_is_bad(has_conf != 0, s_w[4][j], cutoff);
                    x = bad ? tile_median9(s_w[0], wr, wc) : s_w[0][j];
                    y = bad ? tile_median9(s_w[1], wr, wc) : s_w[1][j];
                    z = bad ? tile_median9(s_w[2], wr, wc) : s_w[2][j];
                    u = bad ? tile_median9(s_w[3], wr, wc) : s_w[3][j];
                } else {
                    const size_t g = (size_t)cc * rows + cr;
                    x = X[g]; y = Y[g]; z = Z[g]; u = tile_median9(s_w[0], wr, wc);
                }
            }
            s_p[0][i] = x; s_p[1][i] = y; s_p[2][i] = z; s_p[3][i] = u;
        }
    }
    __syncthreads();
    const int tr = tid % ST, tc = tid / ST, r = r0 + tr, c = c0 + tc;
    if (r >= rows || c >= cols) return;
    const size_t g = (size_t)c * rows + r;
#pragma unroll
    for (int pl = 0; pl < 4; ++pl) {
        double p[9];
#pragma unroll
        for (int dj = 0; dj < 3; ++dj)
#pragma unroll
            for (int di = 0; di < 3; ++di) p[3 * dj + di] = s_p[pl][(tc + dj) * SH + tr + di];
        const double v = sr_tap9(W.w, p);
        filt[pl * npix + g] = pl == 3 ? matlab_uint8(v) : v;  // imfilter on a uint8 image returns uint8
    }
}

struct KpArgs {
    int K, ldf, ND, gate, rows, cols, has_conf;
    const double *frm, *des;                                 // [K][ldf], [K][ND]
    const double *xf, *yf, *zf, *conf, *maxima;
    int32_t *n_kept, *keep_idx;
    double *frm_out, *des_out, *xyz_out, *rho_out;
};

// n doubles by one wave; 16-byte accesses when both ends are 16-byte aligned and n is even
__device__ inline void wave_copy(double *__restrict__ dst, const double *__restrict__ src, int n, int lane)
{
    if ((((uintptr_t)dst | (uintptr_t)src) & 15) == 0 && (n & 1) == 0) {
        const double2 *s2 = (const double2 *)src;
        double2 *d2 = (double2 *)dst;
        for (int i = lane; i < n / 2; i += 64) d2[i] = s2[i];
    } else {
        for (int i = lane; i < n; i += 64) dst[i] = src[i];
    }
}

// the pixel of keypoint k (0-based, column-major offset).  The host has checked that it lies inside the image; the clamp changes no valid position and
// keeps the gather inside the planes whatever the block holds
__device__ inline size_t kp_pixel(const KpArgs &a, int k)
{
    const double u = a.frm[(size_t)k * a.ldf], v = a.frm[(size_t)k * a.ldf + 1];      // row 1: the pixel column, row 2: the pixel row, both 1-based
    const int r = min(max((int)matlab_round(v) - 1, 0), a.rows - 1), c = min(max((int)matlab_round(u) - 1, 0), a.cols - 1);
    return (size_t)c * a.rows + r;
}

__device__ inline bool kp_keep(const KpArgs &a, int k, double cmax)
{
    const size_t g = kp_pixel(a, k);
    if (a.gate == 1) return sr_gate_confidence(a.conf[g], cmax);
    const double xf = a.xf[g];
    return sr_gate_depth(xf, sr_range(xf, a.yf[g], a.zf[g]), a.has_conf != 0, a.has_conf ? a.conf[g] : 0.0, cmax);
}

__global__ __launch_bounds__(KB) void k_sr_keypoints(KpArgs a)
{
    __shared__ int s_base[KW], s_cnt[KW], s_k[KB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double cmax = a.maxima[1];
    // the base offset: how many of the keypoints in front of this workgroup's are kept
    int before = 0;
    for (int b = 0; b < (int)blockIdx.x; ++b) before += __popcll(__ballot(kp_keep(a, b * KB + tid, cmax)));      // (earlier batches are full)
    const int k = blockIdx.x * KB + tid;
    const bool keep = k < a.K && kp_keep(a, k, cmax);
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) { s_base[wave] = before; s_cnt[wave] = __popcll(bal); }
    __syncthreads();
    int base = 0, off = 0, n_local = 0;
    for (int w = 0; w < KW; ++w) { base += s_base[w]; if (w < wave) off += s_cnt[w]; n_local += s_cnt[w]; }
    if (keep) s_k[off + __popcll(bal & ((1ull << lane) - 1ull))] = k;
    __syncthreads();
    if (blockIdx.x == gridDim.x - 1 && tid == 0) *a.n_kept = base + n_local;
    // one wave per kept keypoint, in the caller's order
    for (int j = wave; j < n_local; j += KW) {
        const int kk = s_k[j], slot = base + j;
        wave_copy(a.frm_out + (size_t)slot * a.ldf, a.frm + (size_t)kk * a.ldf, a.ldf, lane);
        if (a.ND > 0) wave_copy(a.des_out + (size_t)slot * a.ND, a.des + (size_t)kk * a.ND, a.ND, lane);
        if (lane == 0) a.keep_idx[slot] = kk;
        if (a.gate == 0 && lane < 4) {
            const size_t g = kp_pixel(a, kk);
            const double xf = a.xf[g], yf = a.yf[g], zf = a.zf[g];
            if (lane < 3) a.xyz_out[3 * (size_t)slot + lane] = lane == 0 ? -xf : (lane == 1 ? -yf : zf);      // inittialize_depth_my_version.m:85
            else a.rho_out[slot] = 1.0 / sr_range(xf, yf, zf);                                                  // :87-92 (norm restated as df)
        }
    }
}

// medfilt2(A, [3 3]) on a whole plane, one pixel per thread straight from global memory (pre3_sr_medfilt3): the window and the network are pre3_sr.h's
__global__ __launch_bounds__(MF) void k_sr_medfilt3(int rows, int cols, int padding, const double *__restrict__ A, double *__restrict__ out)
{
    const size_t g = (size_t)blockIdx.x * MF + threadIdx.x;
    if (g >= (size_t)rows * cols) return;
    out[g] = sr_medfilt_pixel(A, rows, cols, (int)(g % rows), (int)(g / rows), padding);
}

// Device memory of the handle is zeroed ON THE HANDLE'S STREAM: the stream does not synchronise with the null stream (hipStreamNonBlocking), so a
// hipMemset there -- asynchronous to the host -- could land behind the first transfer queued into the block.
static Zero sr_zero(pre3_sr_frame *f) { return Zero::on_stream(f->stream); }

}  // namespace

int sr_grow_stage(pre3_sr_frame *f, size_t bytes)
{
    const int rc = f->mem.stage.reserve(bytes, (bytes + 65535) & ~(size_t)65535, PIN_DEFAULT);
    f->stage = f->mem.stage.p;
    return rc;
}

KpLayout kp_layout(int K, int ldf, int ND)
{
    KpLayout l;
    l.b_frm = up16(sizeof(double) * (size_t)K * ldf); l.b_des = up16(sizeof(double) * (size_t)K * ND);
    l.o_frm_out = l.b_frm + l.b_des; l.o_des_out = l.o_frm_out + l.b_frm; l.o_xyz = l.o_des_out + l.b_des;
    l.o_rho = l.o_xyz + up16(sizeof(double) * 3 * (size_t)K); l.o_idx = l.o_rho + up16(sizeof(double) * (size_t)K);
    l.o_n = l.o_idx + up16(sizeof(int32_t) * (size_t)K); l.total = l.o_n + 16;
    return l;
}

int sr_frame_kp_reserve(pre3_sr_frame *f, size_t total)
{
    const int rc = f->mem.kp.reserve(total, total + total / 4, sr_zero(f));
    f->kp = f->mem.kp.p;
    return rc;
}

// the device half of a load, behind whatever put the planes into `raw` (the staged transfer of pre3_sr_frame_load, the text parse of
// pre3_sr_frame_load_text): the maxima launch and the conditioning launch on the handle's stream, then the handle holds the frame
int sr_condition_run(pre3_sr_frame *f, int mode, bool has_conf)
{
    const size_t npix = (size_t)f->rows * f->cols;
    const int form = f->comp_form;                            // the setting as it stands when the load is queued (pre3_sr_frame_set_compensation)
    const double cutoff = f->comp_cutoff;
    hipLaunchKernelGGL(k_sr_maxima, dim3(1), dim3(MB), 0, f->stream, (int)npix, (const double *)(f->raw + 3 * npix),
                       has_conf ? (const double *)(f->raw + 4 * npix) : (const double *)nullptr, form == SR_COMP_BADPIXEL ? 1 : 0, cutoff, f->maxima);
    PRE3_HIP(hipGetLastError());
    SrWeights W;
    sr_gauss3(mode == 0 ? 2.0 : 1.0, W.w);
    const dim3 grid(ceil_div(f->rows, ST), ceil_div(f->cols, ST));
    auto *kern = form == SR_COMP_BADPIXEL ? k_sr_condition<SR_COMP_BADPIXEL>
                                          : (form == SR_COMP_IMAGE_MEDIAN ? k_sr_condition<SR_COMP_IMAGE_MEDIAN> : k_sr_condition<SR_COMP_NONE>);
    hipLaunchKernelGGL(kern, grid, dim3(ST * ST), 0, f->stream, f->rows, f->cols, mode, W, (const double *)f->raw, (const double *)f->maxima, f->filt,
                       has_conf ? 1 : 0, cutoff);
    PRE3_HIP(hipGetLastError());
    f->mode = mode; f->has_conf = has_conf ? 1 : 0; f->loaded = 1; f->frame_form = form;
    return PRE3_OK;
}

// the text stage's blocks (pre3_dattext.hip), allocated on its first use: the work block behind the text, grown on demand, and the spare plane block
// the parse writes -- it and `raw` swap once a text is accepted.  The caller has waited for the stream.
int sr_frame_text_work(pre3_sr_frame *f, size_t work_bytes, size_t spare_bytes)
{
    const int rc = f->mem.text_dev.reserve(work_bytes, work_bytes + work_bytes / 4, sr_zero(f));
    f->text_dev = f->mem.text_dev.p;
    PRE3_TRY(rc);
    if (f->spare == nullptr) PRE3_TRY(f->mem.fixed.dev(&f->spare, spare_bytes, sr_zero(f)));
    return PRE3_OK;
}

int select_device(const char *who, int device)
{
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) { set_error("%s: no HIP device available (libpre3 has no CPU fallback)", who); return PRE3_E_NODEVICE; }
    if (hipSetDevice(device) != hipSuccess) { set_error("%s: no HIP device %d", who, device); return PRE3_E_NODEVICE; }
    return PRE3_OK;
}

int sr_frame_view(pre3_sr_frame *f, SrFrameView *v)
{
    PRE3_CHECK(f != nullptr && v != nullptr, PRE3_E_ARG, "sr_frame_view: null argument");
    PRE3_CHECK(f->loaded, PRE3_E_STATE, "sr_frame_view: no frame has been loaded");
    const size_t npix = (size_t)f->rows * f->cols;
    v->device = f->device; v->rows = f->rows; v->cols = f->cols; v->mode = f->mode; v->has_conf = f->has_conf;
    v->x = f->filt; v->y = f->filt + npix; v->z = f->filt + 2 * npix; v->img = f->filt + 3 * npix;
    v->conf = f->has_conf ? f->raw + 4 * npix : nullptr;
    v->maxima = f->maxima; v->stream = f->stream; v->comp_form = f->frame_form;
    return PRE3_OK;
}

int sr_frame_keypoint_view(pre3_sr_frame *f, SrKeypointView *v)
{
    PRE3_CHECK(f != nullptr && v != nullptr, PRE3_E_ARG, "sr_frame_keypoint_view: null argument");
    PRE3_CHECK(f->loaded && f->kp_valid, PRE3_E_STATE, "the frame holds no keypoint result (none yet, or a frame was loaded after it)");
    v->K = f->kp_K; v->ldf = f->kp_ldf; v->ND = f->kp_ND; v->gate = f->kp_gate; v->n_kept = f->kp_n;
    v->frm = f->kp_n > 0 ? (const double *)((const char *)f->kp + f->kp_o_frm) : nullptr;
    v->des = f->kp_n > 0 ? (const double *)((const char *)f->kp + f->kp_o_des) : nullptr;
    const bool depth = f->kp_n > 0 && f->kp_gate == 0;
    v->xyz = depth ? (const double *)((const char *)f->kp + f->kp_o_xyz) : nullptr;
    v->rho = depth ? (const double *)((const char *)f->kp + f->kp_o_rho) : nullptr;
    v->keep_idx = f->kp_n > 0 ? (const int32_t *)((const char *)f->kp + f->kp_o_idx) : nullptr;
    v->K_in = f->kp_K_in;
    v->frm_in = f->kp_K_in > 0 ? (const double *)f->kp : nullptr;
    v->des_in = f->kp_K_in > 0 ? (const double *)((const char *)f->kp + f->kp_o_des_in) : nullptr;
    v->raw_in_bounds = f->kp_raw_ok;
    return PRE3_OK;
}

// dev_bytes of device memory and pin_bytes of pinned host memory owned by the handle, grown on demand; a new device block is zeroed on the handle's stream
// (sr_zero's rule).  The caller has made sure that nothing queued still uses the old blocks.
int sr_frame_pair_work(pre3_sr_frame *f, size_t dev_bytes, size_t pin_bytes, void **dev, void **pin)
{
    PRE3_CHECK(f != nullptr, PRE3_E_ARG, "sr_frame_pair_work: null handle");
    PRE3_TRY(f->mem.pair_dev.reserve(dev_bytes, dev_bytes + dev_bytes / 4, sr_zero(f)));
    PRE3_TRY(f->mem.pair_pin.reserve(pin_bytes, (pin_bytes + pin_bytes / 4 + 65535) & ~(size_t)65535, PIN_DEFAULT));
    *dev = f->mem.pair_dev.p; *pin = f->mem.pair_pin.p;
    return PRE3_OK;
}

// the same rule for the ICP run of pre3_predict_icp_pair_seeded: owned by the handle, so that it outlives the prediction's read in the no-wait form
int sr_frame_icp_work(pre3_sr_frame *f, size_t dev_bytes, void **dev)
{
    PRE3_CHECK(f != nullptr, PRE3_E_ARG, "sr_frame_icp_work: null handle");
    PRE3_TRY(f->mem.icp_dev.reserve(dev_bytes, dev_bytes + dev_bytes / 4, sr_zero(f)));
    *dev = f->mem.icp_dev.p;
    return PRE3_OK;
}

int sr_frame_lend(pre3_sr_frame *f, hipStream_t consumer)
{
    PRE3_CHECK(f != nullptr, PRE3_E_ARG, "sr_frame_lend: null handle");
    PRE3_HIP(hipEventRecord(f->pair_ev, f->stream));
    PRE3_HIP(hipStreamWaitEvent(consumer, f->pair_ev, 0));
    return PRE3_OK;
}

int sr_frame_reclaim(pre3_sr_frame *f, hipStream_t consumer)
{
    PRE3_CHECK(f != nullptr, PRE3_E_ARG, "sr_frame_reclaim: null handle");
    PRE3_HIP(hipEventRecord(f->pair_ev, consumer));
    PRE3_HIP(hipStreamWaitEvent(f->stream, f->pair_ev, 0));
    return PRE3_OK;
}

int sr_frame_pair_views(const char *who, pre3_sr_frame *prev, pre3_sr_frame *cur, double thresh, SrFrameView *v1, SrFrameView *v2, SrKeypointView *k1,
                        SrKeypointView *k2)
{
    PRE3_CHECK(prev != nullptr && cur != nullptr, PRE3_E_ARG, "%s: null handle", who);
    PRE3_CHECK(prev != cur, PRE3_E_ARG, "%s: prev and cur are the same handle", who);
    PRE3_CHECK(std::isfinite(thresh) && thresh > 0.0, PRE3_E_ARG, "%s: thresh must be positive and finite", who);
    PRE3_TRY(sr_frame_view(prev, v1)); PRE3_TRY(sr_frame_view(cur, v2));
    PRE3_CHECK(v1->device == v2->device && v1->rows == v2->rows && v1->cols == v2->cols, PRE3_E_ARG,
               "%s: the frames differ (device %d, %d x %d against device %d, %d x %d)", who, v1->device, v1->rows, v1->cols, v2->device, v2->rows, v2->cols);
    PRE3_TRY(sr_frame_keypoint_view(prev, k1)); PRE3_TRY(sr_frame_keypoint_view(cur, k2));
    PRE3_CHECK(k1->ND == DESC_DIM && k2->ND == DESC_DIM, PRE3_E_ARG, "%s: descriptors of %d and %d entries (the matcher's tile is written for %d)", who,
               k1->ND, k2->ND, DESC_DIM);
    return PRE3_OK;
}

}  // namespace pre3

using namespace pre3;

extern "C" {

int pre3_sr_gauss3(double sigma, double w[9])
{
    PRE3_CHECK(w != nullptr && sigma > 0.0 && std::isfinite(sigma), PRE3_E_ARG, "pre3_sr_gauss3: sigma must be positive and finite, w non-null");
    sr_gauss3(sigma, w);
    return PRE3_OK;
}

int pre3_sr_frame_destroy(pre3_sr_frame *f)
{
    if (f == nullptr) return PRE3_OK;
    (void)hipSetDevice(f->device);
    if (f->stream) { (void)hipStreamSynchronize(f->stream); (void)hipStreamDestroy(f->stream); }
    f->mem = {};
    if (f->pair_ev) (void)hipEventDestroy(f->pair_ev);
    if (f->sift) sift_work_free(f->sift);
    delete f;
    return PRE3_OK;
}

static int sr_create_buffers(pre3_sr_frame *f)
{
    const size_t npix = (size_t)f->rows * f->cols;
    PRE3_HIP(hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking));
    PRE3_HIP(hipEventCreateWithFlags(&f->pair_ev, hipEventDisableTiming));
    PRE3_TRY(f->mem.fixed.dev(&f->raw, sizeof(double) * 5 * npix, sr_zero(f)));
    PRE3_TRY(f->mem.fixed.dev(&f->filt, sizeof(double) * 4 * npix, sr_zero(f)));
    PRE3_TRY(f->mem.fixed.dev(&f->maxima, sizeof(double) * 4, sr_zero(f)));     // imax, cmax, n_bad (and a spare)
    PRE3_TRY(f->mem.fixed.pin(&f->pinned_n, 64, PIN_DEFAULT));
    return sr_grow_stage(f, sizeof(double) * 5 * npix);
}

int pre3_sr_frame_create(pre3_sr_frame **out, int device, int rows, int cols)
{
    PRE3_CHECK(out != nullptr, PRE3_E_ARG, "pre3_sr_frame_create: null argument");
    *out = nullptr;
    PRE3_CHECK(rows >= 1 && cols >= 1 && (long long)rows * cols <= (1ll << 26), PRE3_E_ARG, "pre3_sr_frame_create: a %d x %d frame", rows, cols);
    PRE3_TRY(select_device("pre3_sr_frame_create", device));
    pre3_sr_frame *f = new pre3_sr_frame;
    f->device = device; f->rows = rows; f->cols = cols;
    const int rc = sr_create_buffers(f);
    if (rc != PRE3_OK) { (void)pre3_sr_frame_destroy(f); return rc; }
    *out = f;
    return PRE3_OK;
}

int pre3_sr_frame_load(pre3_sr_frame *f, int mode, const double *z, const double *x, const double *y, const double *amp, const double *conf)
{
    PRE3_CHECK(f != nullptr && z != nullptr && x != nullptr && y != nullptr && amp != nullptr, PRE3_E_ARG, "pre3_sr_frame_load: null argument");
    PRE3_CHECK(mode == 0 || mode == 1, PRE3_E_ARG, "pre3_sr_frame_load: mode %d is neither 0 (read_xyz_sr4000) nor 1 (read_sr4000_data_dr_ye)", mode);
    const size_t npix = (size_t)f->rows * f->cols;
    for (size_t i = 0; i < npix; ++i)                         // MATLAB's sqrt of a negative amplitude goes complex
        PRE3_CHECK(std::isfinite(amp[i]) && amp[i] >= 0.0, PRE3_E_ARG, "pre3_sr_frame_load: the amplitude at row %d, column %d is negative or not finite",
                   (int)(i % f->rows) + 1, (int)(i / f->rows) + 1);
    PRE3_TRY(select_device("pre3_sr_frame_load", f->device));
    PRE3_HIP(hipStreamSynchronize(f->stream));                // the staging block may still be the source of the previous load's transfer
    double *st = (double *)f->stage;
    memcpy(st, z, sizeof(double) * npix); memcpy(st + npix, x, sizeof(double) * npix); memcpy(st + 2 * npix, y, sizeof(double) * npix);
    memcpy(st + 3 * npix, amp, sizeof(double) * npix);
    if (conf != nullptr) memcpy(st + 4 * npix, conf, sizeof(double) * npix);
    f->loaded = 0; f->kp_valid = 0;                           // the keypoint record belongs to the frame that is being replaced
    PRE3_HIP(hipMemcpyAsync(f->raw, st, sizeof(double) * (conf != nullptr ? 5 : 4) * npix, hipMemcpyHostToDevice, f->stream));
    return sr_condition_run(f, mode, conf != nullptr);
}

int pre3_sr_frame_get(pre3_sr_frame *f, double *x, double *y, double *z, double *img, double *conf, double *imax, double *cmax)
{
    PRE3_CHECK(f != nullptr, PRE3_E_ARG, "pre3_sr_frame_get: null handle");
    PRE3_CHECK(f->loaded, PRE3_E_STATE, "pre3_sr_frame_get: no frame has been loaded");
    PRE3_CHECK(conf == nullptr || f->has_conf, PRE3_E_ARG, "pre3_sr_frame_get: the frame was loaded without a confidence map");
    PRE3_TRY(select_device("pre3_sr_frame_get", f->device));
    const size_t npix = (size_t)f->rows * f->cols, nb = sizeof(double) * npix;
    double mx[2];
    if (x) PRE3_HIP(hipMemcpyAsync(x, f->filt, nb, hipMemcpyDeviceToHost, f->stream));
    if (y) PRE3_HIP(hipMemcpyAsync(y, f->filt + npix, nb, hipMemcpyDeviceToHost, f->stream));
    if (z) PRE3_HIP(hipMemcpyAsync(z, f->filt + 2 * npix, nb, hipMemcpyDeviceToHost, f->stream));
    if (img) PRE3_HIP(hipMemcpyAsync(img, f->filt + 3 * npix, nb, hipMemcpyDeviceToHost, f->stream));
    if (conf) PRE3_HIP(hipMemcpyAsync(conf, f->raw + 4 * npix, nb, hipMemcpyDeviceToHost, f->stream));
    if (imax || cmax) PRE3_HIP(hipMemcpyAsync(mx, f->maxima, sizeof mx, hipMemcpyDeviceToHost, f->stream));
    PRE3_HIP(hipStreamSynchronize(f->stream));
    if (imax) *imax = mx[0];
    if (cmax) *cmax = mx[1];
    return PRE3_OK;
}

int pre3_sr_frame_set_compensation(pre3_sr_frame *f, int form, double cutoff)
{
    PRE3_CHECK(f != nullptr, PRE3_E_ARG, "pre3_sr_frame_set_compensation: null handle");
    PRE3_CHECK(form >= SR_COMP_NONE && form <= SR_COMP_IMAGE_MEDIAN, PRE3_E_ARG,
               "pre3_sr_frame_set_compensation: form %d is neither 0 (none), 1 (bad pixels) nor 2 (the image's median)", form);
    PRE3_CHECK(form != SR_COMP_BADPIXEL || std::isfinite(cutoff), PRE3_E_ARG, "pre3_sr_frame_set_compensation: the cut-off of form 1 must be finite");
    f->comp_form = form; f->comp_cutoff = cutoff;
    return PRE3_OK;
}

int pre3_sr_frame_get_compensation(pre3_sr_frame *f, int32_t *form, double *cutoff)
{
    PRE3_CHECK(f != nullptr, PRE3_E_ARG, "pre3_sr_frame_get_compensation: null handle");
    if (form) *form = f->comp_form;
    if (cutoff) *cutoff = f->comp_cutoff;
    return PRE3_OK;
}

int pre3_sr_frame_bad_pixels(pre3_sr_frame *f, int32_t *form_of_frame, int32_t *n_bad)
{
    PRE3_CHECK(f != nullptr, PRE3_E_ARG, "pre3_sr_frame_bad_pixels: null handle");
    PRE3_CHECK(f->loaded, PRE3_E_STATE, "pre3_sr_frame_bad_pixels: no frame has been loaded");
    PRE3_TRY(select_device("pre3_sr_frame_bad_pixels", f->device));
    double n = 0.0;
    PRE3_HIP(hipMemcpyAsync(&n, f->maxima + 2, sizeof n, hipMemcpyDeviceToHost, f->stream));
    PRE3_HIP(hipStreamSynchronize(f->stream));
    if (form_of_frame) *form_of_frame = f->frame_form;
    if (n_bad) *n_bad = (int32_t)n;
    return PRE3_OK;
}

int pre3_sr_medfilt3(int device, int rows, int cols, const double *A, int padding, double *out)
{
    const char *who = "pre3_sr_medfilt3";
    PRE3_CHECK(A != nullptr && out != nullptr, PRE3_E_ARG, "%s: null argument", who);
    PRE3_CHECK(padding == SR_PAD_ZEROS || padding == SR_PAD_SYMMETRIC, PRE3_E_ARG, "%s: padding %d is neither 0 (zeros) nor 1 (symmetric)", who, padding);
    PRE3_CHECK(rows >= 1 && cols >= 1 && (long long)rows * cols <= PRE3_SR_MEDFILT_MAX_PIXELS, PRE3_E_ARG, "%s: a %d x %d plane", who, rows, cols);
    PRE3_TRY(select_device(who, device));
    const size_t npix = (size_t)rows * cols, nb = sizeof(double) * npix;
    Scratch d;
    PRE3_TRY(d.alloc(2 * nb));
    double *dA = d.as<double>(), *dO = dA + npix;
    PRE3_HIP(hipMemcpy(dA, A, nb, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_sr_medfilt3, dim3((unsigned)((npix + MF - 1) / MF)), dim3(MF), 0, nullptr, rows, cols, padding, (const double *)dA, dO);
    PRE3_HIP(hipGetLastError());
    PRE3_HIP(hipStreamSynchronize(nullptr));
    PRE3_HIP(hipMemcpy(out, dO, nb, hipMemcpyDeviceToHost));
    return PRE3_OK;
}

// the gate launch over the raw set in the keypoint block (kp_K_in frames of kp_ldf entries at offset 0, descriptors of kp_ND at kp_o_des_in), the
// count read back, then the outputs the caller asked for
static int sr_gate_run(pre3_sr_frame *f, const char *who, int gate, int32_t *n_kept, int32_t *keep_idx, double *frm_out, double *des_out, double *xyz_out,
                       double *rho_out)
{
    const int K = f->kp_K_in, ldf = f->kp_ldf, ND = f->kp_ND;
    const KpLayout l = kp_layout(K, ldf, ND);
    char *d = (char *)f->kp;
    const size_t npix = (size_t)f->rows * f->cols;
    KpArgs a;
    a.K = K; a.ldf = ldf; a.ND = ND; a.gate = gate; a.rows = f->rows; a.cols = f->cols; a.has_conf = f->has_conf;
    a.frm = (const double *)d; a.des = (const double *)(d + l.b_frm);
    a.xf = f->filt; a.yf = f->filt + npix; a.zf = f->filt + 2 * npix; a.conf = f->raw + 4 * npix; a.maxima = f->maxima;
    a.n_kept = (int32_t *)(d + l.o_n); a.keep_idx = (int32_t *)(d + l.o_idx);
    a.frm_out = (double *)(d + l.o_frm_out); a.des_out = (double *)(d + l.o_des_out); a.xyz_out = (double *)(d + l.o_xyz); a.rho_out = (double *)(d + l.o_rho);
    hipLaunchKernelGGL(k_sr_keypoints, dim3(ceil_div(K, KB)), dim3(KB), 0, f->stream, a);
    PRE3_HIP(hipGetLastError());
    PRE3_HIP(hipMemcpyAsync(f->pinned_n, a.n_kept, sizeof(int32_t), hipMemcpyDeviceToHost, f->stream));
    PRE3_HIP(hipStreamSynchronize(f->stream));
    const int n = *f->pinned_n;
    PRE3_CHECK(n >= 0 && n <= K, PRE3_E_HIP, "%s: the device kept %d of %d keypoints", who, n, K);
    *n_kept = n;
    f->kp_n = n; f->kp_o_frm = l.o_frm_out; f->kp_o_des = l.o_des_out; f->kp_o_xyz = l.o_xyz; f->kp_o_rho = l.o_rho; f->kp_o_idx = l.o_idx;
    if (n == 0) return PRE3_OK;
    if (keep_idx) PRE3_HIP(hipMemcpyAsync(keep_idx, a.keep_idx, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, f->stream));
    if (frm_out) PRE3_HIP(hipMemcpyAsync(frm_out, a.frm_out, sizeof(double) * (size_t)n * ldf, hipMemcpyDeviceToHost, f->stream));
    if (des_out && ND > 0) PRE3_HIP(hipMemcpyAsync(des_out, a.des_out, sizeof(double) * (size_t)n * ND, hipMemcpyDeviceToHost, f->stream));
    if (xyz_out && gate == 0) PRE3_HIP(hipMemcpyAsync(xyz_out, a.xyz_out, sizeof(double) * 3 * (size_t)n, hipMemcpyDeviceToHost, f->stream));
    if (rho_out && gate == 0) PRE3_HIP(hipMemcpyAsync(rho_out, a.rho_out, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, f->stream));
    PRE3_HIP(hipStreamSynchronize(f->stream));
    return PRE3_OK;
}

// touched: set once the call is past its checks -- from there on the keypoint block no longer holds the previous result
static int sr_keypoints_impl(pre3_sr_frame *f, int gate, int ldf, int K, const double *frm, int ND, const double *des, int32_t *n_kept, int32_t *keep_idx,
                             double *frm_out, double *des_out, double *xyz_out, double *rho_out, bool *touched)
{
    PRE3_CHECK(f != nullptr && n_kept != nullptr, PRE3_E_ARG, "pre3_sr_frame_keypoints: null argument");
    PRE3_CHECK(gate == 0 || gate == 1, PRE3_E_ARG, "pre3_sr_frame_keypoints: gate %d is neither 0 (depth) nor 1 (confidence)", gate);
    PRE3_CHECK(K >= 0 && K <= PRE3_SR_MAX_KEYPOINTS, PRE3_E_ARG, "pre3_sr_frame_keypoints: K=%d outside [0, %d]", K, PRE3_SR_MAX_KEYPOINTS);
    PRE3_CHECK(ldf >= 2 && ldf <= 4096, PRE3_E_ARG, "pre3_sr_frame_keypoints: ldf=%d (a frame holds at least the pixel column and row)", ldf);
    PRE3_CHECK(ND >= 0 && ND <= 4096, PRE3_E_ARG, "pre3_sr_frame_keypoints: ND=%d", ND);
    PRE3_CHECK(K == 0 || (frm != nullptr && (ND == 0 || des != nullptr)), PRE3_E_ARG, "pre3_sr_frame_keypoints: null frames or descriptors");
    PRE3_CHECK(f->loaded, PRE3_E_STATE, "pre3_sr_frame_keypoints: no frame has been loaded");
    PRE3_CHECK(gate == 0 || f->has_conf, PRE3_E_ARG, "pre3_sr_frame_keypoints: gate 1 needs the confidence map (the frame was loaded without one)");
    for (int k = 0; k < K; ++k) {                             // MATLAB would raise an index error
        const double u = frm[(size_t)k * ldf], v = frm[(size_t)k * ldf + 1];
        PRE3_CHECK(std::isfinite(u) && std::isfinite(v), PRE3_E_ARG, "pre3_sr_frame_keypoints: the position of keypoint %d is not finite", k);
        const double r = matlab_round(v), c = matlab_round(u);
        PRE3_CHECK(r >= 1.0 && r <= (double)f->rows && c >= 1.0 && c <= (double)f->cols, PRE3_E_ARG,
                   "pre3_sr_frame_keypoints: keypoint %d rounds to row %.0f, column %.0f outside the %d x %d frame", k, r, c, f->rows, f->cols);
    }
    PRE3_TRY(select_device("pre3_sr_frame_keypoints", f->device));
    *n_kept = 0;
    *touched = true;
    f->kp_valid = 1; f->kp_K = K; f->kp_ldf = ldf; f->kp_ND = ND; f->kp_gate = gate; f->kp_n = 0;      // a valid empty record until the count is in
    f->kp_K_in = 0; f->kp_o_des_in = 0; f->kp_raw_ok = true;
    if (K == 0) return PRE3_OK;
    // [frm | des] up; [frm_out | des_out | xyz | rho | keep_idx | n_kept] behind them
    const KpLayout l = kp_layout(K, ldf, ND);
    PRE3_HIP(hipStreamSynchronize(f->stream));                // the staging block and the keypoint block are free again
    PRE3_TRY(sr_frame_kp_reserve(f, l.total));
    PRE3_TRY(sr_grow_stage(f, l.b_frm + l.b_des));
    memcpy(f->stage, frm, sizeof(double) * (size_t)K * ldf);
    // (the same copy, with the bounds of the ranked IC route noted on the way: pre3_set_scan_frame takes the raw set from this block)
    if (ND > 0) f->kp_raw_ok = desc_copy_checked((double *)((char *)f->stage + l.b_frm), des, (size_t)K * ND);
    f->kp_o_des_in = l.b_frm;
    PRE3_HIP(hipMemcpyAsync(f->kp, f->stage, l.b_frm + l.b_des, hipMemcpyHostToDevice, f->stream));
    f->kp_K_in = K;
    return sr_gate_run(f, "pre3_sr_frame_keypoints", gate, n_kept, keep_idx, frm_out, des_out, xyz_out, rho_out);
}

int pre3_sr_frame_keypoints(pre3_sr_frame *f, int gate, int ldf, int K, const double *frm, int ND, const double *des, int32_t *n_kept, int32_t *keep_idx,
                            double *frm_out, double *des_out, double *xyz_out, double *rho_out)
{
    bool touched = false;
    const int rc = sr_keypoints_impl(f, gate, ldf, K, frm, ND, des, n_kept, keep_idx, frm_out, des_out, xyz_out, rho_out, &touched);
    if (rc != PRE3_OK && touched) { f->kp_n = 0; f->kp_K_in = 0; }      // a call that failed behind its checks leaves a valid empty record
    return rc;
}

// pre3_sr_frame_keypoints' gate over the raw set that is already in the block (a pre3_sr_frame_sift's, or an earlier upload's): nothing is sent
int pre3_sr_frame_gate(pre3_sr_frame *f, int gate, int32_t *n_kept, int32_t *keep_idx, double *frm_out, double *des_out, double *xyz_out, double *rho_out)
{
    PRE3_CHECK(f != nullptr && n_kept != nullptr, PRE3_E_ARG, "pre3_sr_frame_gate: null argument");
    PRE3_CHECK(gate == 0 || gate == 1, PRE3_E_ARG, "pre3_sr_frame_gate: gate %d is neither 0 (depth) nor 1 (confidence)", gate);
    PRE3_CHECK(f->loaded && f->kp_valid, PRE3_E_STATE, "pre3_sr_frame_gate: the frame holds no keypoint set (none yet, or a frame was loaded after it)");
    PRE3_CHECK(gate == 0 || f->has_conf, PRE3_E_ARG, "pre3_sr_frame_gate: gate 1 needs the confidence map (the frame was loaded without one)");
    PRE3_CHECK(f->kp_ldf == 4 && f->kp_ND == DESC_DIM, PRE3_E_ARG, "pre3_sr_frame_gate: the set in the block has ldf = %d, ND = %d; the outputs are sized for 4 and %d",
               f->kp_ldf, f->kp_ND, DESC_DIM);
    PRE3_TRY(select_device("pre3_sr_frame_gate", f->device));
    *n_kept = 0;
    f->kp_gate = gate; f->kp_n = 0;
    if (f->kp_K_in == 0) return PRE3_OK;
    const int rc = sr_gate_run(f, "pre3_sr_frame_gate", gate, n_kept, keep_idx, frm_out, des_out, xyz_out, rho_out);
    if (rc != PRE3_OK) f->kp_n = 0;                           // (the raw set stays: it was not this call's)
    return rc;
}

}  // extern "C"
