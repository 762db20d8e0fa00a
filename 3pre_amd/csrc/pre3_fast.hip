// pre3_fast.hip -- FAST-9 corners on the resident byte image.
//   detection    the segment test of the FAST papers (Rosten and Drummond, ICCV 2005 / ECCV 2006): 9 contiguous pixels of the 16-pixel ring all
//                > centre + t or all < centre - t, strict as fast_corner_detect_9.m:61-63.  The reference's fast_corner_detect_9.m is a learned
//                decision tree that is NOT this test (785 268 of the 3^16 ring states are corners to the tree, 46 658 to the segment test); it is
//                program text of the reference and is not reproduced.  The two agree on the fixture tests/golden/fast_lab_crop.npz at thresholds 10,
//                20 and 30; a tree-exact mode does not exist.
//   score        fast_nonmax.m:70-75 with its own barrier, at detected corners only
//   suppression  fast_nonmax.m:87-92: kept when >= all eight neighbours' scores (ties on both sides, a score-0 corner among score-0 neighbours)
//   order        fast_corner_detect_9.m:59-60: x outer, y inner = the ascending column-major index
// The rectangle is taken as an image of its own (imTemp2 of initialize_a_feature.m:93-94): candidates are its pixels 4 .. size - 3, the ring never
// leaves it.  Two launches: k_fast_strip (a workgroup owns FAST_STRIP whole columns plus a halo of 4: bytes in LDS, 16-bit bright / dark masks, the
// 9-run by rotate-and-AND, scores in LDS, the verdict per pixel into a map, the strip's count) and k_fast_emit (a strip's run of the output starts
// at the sum of the earlier strips' counts).  No atomics on memory, one writer per slot: the lists are the same from run to run.
//   k_fast_box   initialize_a_feature.m:55-194 as ONE workgroup: per attempt the box centre (a caller's table, or stream 5 of pre3_philox.h), the
//                61 x 41 box (2501 pixels) through the same verdict function, the first maximum as a min-reduction over the linear index, the
//                "features in the box" test over the landmarks with an h, gate 0 of pre3_sr_frame_keypoints (pre3_sr.h) at the chosen pixel
//   k_fast_gate  initialize_n_features_FAST.m:118-127: gate 0 at every listed maximum
#include <cmath>
#include <new>
#include <vector>
#include "pre3_fast.h"
#include "pre3_patch.h"
#include "pre3_philox.h"
#include "pre3_sr.h"

namespace pre3 {

static_assert(FAST_MAX_DIM == PATCH_MAX_DIM, "the strip tile is sized for the resident image's bound");

// fast_nonmax.m:44-59: ring pixel k is (dx, dy); consecutive k are neighbours on the circle
__device__ constexpr int FAST_DX[16] = { 0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1 };
__device__ constexpr int FAST_DY[16] = { 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3 };

__device__ __forceinline__ unsigned rotl16(unsigned m, int k) { return ((m << k) | (m >> (16 - k))) & 0xffffu; }
// 9 circularly contiguous set bits of a 16-bit mask: runs of 2, 4, 8, then 9
__device__ __forceinline__ bool run9(unsigned m)
{
    const unsigned r2 = m & rotl16(m, 1), r4 = r2 & rotl16(r2, 2), r8 = r4 & rotl16(r4, 4);
    return (r8 & rotl16(m, 8)) != 0;
}
// the verdict at p (column stride ld bytes): 0, or 0x8000 | score
__device__ __forceinline__ unsigned fast_pixel(const uint8_t *p, int ld, int thr, int bar)
{
    const int ctr = *p, cb = ctr + thr, c_b = ctr - thr, sb = ctr + bar, s_b = ctr - bar;
    unsigned bright = 0, dark = 0; int pos = 0, neg = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int q = p[FAST_DX[j] * ld + FAST_DY[j]];
        bright |= (unsigned)(q > cb) << j; dark |= (unsigned)(q < c_b) << j;
        pos += max(q - sb, 0); neg += max(s_b - q, 0);
    }
    return (run9(bright) || run9(dark)) ? (0x8000u | (unsigned)max(pos, neg)) : 0u;      // a score is at most 16 * 255
}

struct FastArgs { const uint8_t *img; int ld, r0, c0, rows, cols, thr, bar, nonmax; uint16_t *map; int32_t *blk; };

__global__ __launch_bounds__(256) void k_fast_strip(FastArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t tile[(FAST_STRIP + 2 * FAST_HALO) * FAST_MAX_DIM];      // [tile column][row]
    __shared__ uint16_t sc[(FAST_STRIP + 2) * FAST_MAX_DIM];                                                // columns cs - 1 .. cs + FAST_STRIP
    __shared__ int s_cnt;
    const int t = threadIdx.x, rows = a.rows, cols = a.cols;
    const int cs = blockIdx.x * FAST_STRIP, tc0 = cs - FAST_HALO;           // first own column, the rectangle's column of tile column 0
    const int lo = max(tc0, 0), hi = min(cs + FAST_STRIP + FAST_HALO, cols);
    if (t == 0) s_cnt = 0;
    for (int k = t; k < (hi - lo) * rows; k += 256) {
        const int c = lo + k / rows, r = k - (c - lo) * rows;
        tile[(c - tc0) * rows + r] = a.img[(size_t)(a.c0 + c) * a.ld + (a.r0 + r)];
    }
    __syncthreads();
    // the verdicts of the own columns and one more on either side; a candidate's ring lies in columns c - 3 .. c + 3, inside [lo, hi)
    for (int k = t; k < (FAST_STRIP + 2) * rows; k += 256) {
        const int sc_c = k / rows, r = k - sc_c * rows, c = cs - 1 + sc_c;
        unsigned v = 0;
        if (c >= 3 && c < cols - 3 && r >= 3 && r < rows - 3) v = fast_pixel(tile + (c - tc0) * rows + r, rows, a.thr, a.bar);
        sc[k] = (uint16_t)v;
    }
    __syncthreads();
    int n = 0;
    for (int k = t; k < FAST_STRIP * rows; k += 256) {
        const int oc = k / rows, r = k - oc * rows, c = cs + oc;
        if (c >= cols) break;
        const uint16_t *s = sc + (oc + 1) * rows + r;
        unsigned v = *s;
        if (v != 0 && a.nonmax) {                               // a corner has 3 <= r < rows - 3: its neighbours' rows exist
            const unsigned me = v & 0x7fffu;
            bool keep = true;
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx)
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy)
                    if (dx != 0 || dy != 0) keep = keep && me >= (s[dx * rows + dy] & 0x7fffu);
            if (!keep) v = 0;
        }
        a.map[(size_t)c * rows + r] = (uint16_t)v;
        n += v != 0;
    }
    if (n) atomicAdd(&s_cnt, n);
    __syncthreads();
    if (t == 0) a.blk[4 + blockIdx.x] = s_cnt;
}

// a strip's listed pixels in ascending column-major order, behind those of the strips in front of it
__global__ __launch_bounds__(256) void k_fast_emit(int rows, int cols, const uint16_t *__restrict__ map, int32_t *blk)
{
    __shared__ int cnts[256];
    const int t = threadIdx.x, cs = blockIdx.x * FAST_STRIP, own = min(FAST_STRIP, cols - cs), tot = own * rows;
    const int per = (tot + 255) / 256, lo = min(t * per, tot), hi = min(lo + per, tot);
    const uint16_t *m = map + (size_t)cs * rows;
    int n = 0;
    for (int i = lo; i < hi; ++i) n += m[i] != 0;
    cnts[t] = n;
    __syncthreads();
    if (t == 0) {
        int s = 0;
        for (int b = 0; b < (int)blockIdx.x; ++b) s += blk[4 + b];
        for (int k = 0; k < 256; ++k) { const int v = cnts[k]; cnts[k] = s; s += v; }
        if (blockIdx.x == gridDim.x - 1) blk[0] = s;            // the whole count, capped or not
    }
    __syncthreads();
    int o = cnts[t];
    int32_t *uv = blk + FAST_O_UV, *score = blk + FAST_O_SCORE;
    for (int i = lo; i < hi; ++i) {
        const unsigned v = m[i];
        if (v == 0) continue;
        if (o < PRE3_FAST_MAX_CORNERS) {
            const int oc = i / rows;
            uv[2 * o] = cs + oc + 1; uv[2 * o + 1] = i - oc * rows + 1; score[o] = (int32_t)(v & 0x7fffu);
        }
        ++o;
    }
}


// ---------------------------------------------------------------------------------------------------------------------------------------------
// the depth gate and the two initialisation kernels
// ---------------------------------------------------------------------------------------------------------------------------------------------
struct FastPlanes { const double *x, *y, *z, *conf, *maxima; int has_conf, ld; };
// gate 0 of pre3_sr_frame_keypoints at the 1-based pixel (u, v) (inittialize_depth_my_version.m:40-45, :74-92): the verdict, rho = 1 / df, [-x, -y, z]
__device__ inline int fast_gate0(const FastPlanes &pl, int u, int v, double *rho, double *xyz)
{
    const size_t g = (size_t)(u - 1) * pl.ld + (v - 1);
    const double xf = pl.x[g], yf = pl.y[g], zf = pl.z[g];
    const double df = sr_range(xf, yf, zf), cmax = pl.maxima[1], conf = pl.has_conf ? pl.conf[g] : 0.0;
    if (!sr_gate_depth(xf, df, pl.has_conf != 0, conf, cmax)) {
        *rho = 0.0; xyz[0] = xyz[1] = xyz[2] = 0.0;
        return xf != xf ? PRE3_FAST_NO_DEPTH_NAN : (df < SR_MIN_RANGE ? PRE3_FAST_NO_DEPTH_NEAR : PRE3_FAST_NO_DEPTH_CONF);      // the order of :40, :74
    }
    *rho = 1.0 / df; xyz[0] = -xf; xyz[1] = -yf; xyz[2] = zf;
    return PRE3_FAST_INITIALISED;
}

struct BoxArgs {
    const uint8_t *img; int nRows, nCols, thr, bar, strict, attempts, seeded; uint64_t seed, seq; int32_t centres[2 * PRE3_FAST_MAX_ATTEMPTS];
    int N; const double *h; const int32_t *has_h; FastPlanes pl; double *res;
};
__global__ __launch_bounds__(256) void k_fast_box(BoxArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t tile[FAST_BOX_PIX];       // [column][row] of the box
    __shared__ uint16_t sc[FAST_BOX_PIX];
    __shared__ int s_first;
    const int t = threadIdx.x;
    constexpr int R = FAST_BOX_ROWS, C = FAST_BOX_COLS, SR = R / 2, SC = C / 2;
    int status = PRE3_FAST_NO_BOX, used = 0;
    for (int at = 0; at < a.attempts; ++at) {
        // ---- the box centre (initialize_a_feature.m:64-68, BoxLimX = [1 nCols], BoxLimY = [1 nRows]): (row, column), 1-based
        int cr, cc;
        if (a.seeded) {
            const PhiloxBlock b = draw_block(a.seed, DRAW_STREAM_FAST, (uint64_t)at, 0, a.seq);
            cr = (int)matlab_round(draw_uniform(b.w[0]) * (double)((a.nRows - 1) - 2 * FAST_BAND - 2 * SR)) + FAST_BAND + SR;
            cc = (int)matlab_round(draw_uniform(b.w[1]) * (double)((a.nCols - 1) - 2 * FAST_BAND - 2 * SC)) + FAST_BAND + SC;
        } else { cr = a.centres[2 * at]; cc = a.centres[2 * at + 1]; }
        used = at + 1;
        if (t == 0) { a.res[8 + 2 * at] = cr; a.res[9 + 2 * at] = cc; s_first = FAST_BOX_PIX; }
        // ---- are there other features in the box (:164-174)?  strict: u against the ROW centre +/- 30, v against the COLUMN centre +/- 20, as written.
        // Asked first: an occupied box fails the attempt whatever its corners are (:176), so its detection is not run
        int inside = 0;
        for (int i = t; i < a.N; i += 256) {
            if (!a.has_h[i]) continue;
            const double hu = a.h[2 * i], hv = a.h[2 * i + 1];
            const double p = a.strict ? hu : hv, q = a.strict ? hv : hu;
            inside |= (p > (double)(cr - SR)) && (p < (double)(cr + SR)) && (q > (double)(cc - SC)) && (q < (double)(cc + SC));
        }
        if (__syncthreads_or(inside)) continue;                                // (uniform)
        const int r0 = cr - SR - 1, c0 = cc - SC - 1;                          // 0-based origin of imTemp2 (:93-94); inside the image: checked by the host
        for (int k = t; k < FAST_BOX_PIX; k += 256) { const int c = k / R, r = k - c * R; tile[k] = a.img[(size_t)(c0 + c) * a.nRows + (r0 + r)]; }
        __syncthreads();
        for (int k = t; k < FAST_BOX_PIX; k += 256) {
            const int c = k / R, r = k - c * R;
            sc[k] = (c >= 3 && c < C - 3 && r >= 3 && r < R - 3) ? (uint16_t)fast_pixel(tile + k, R, a.thr, a.bar) : (uint16_t)0;
        }
        __syncthreads();
        // ---- the first maximum in scan order (:104-106, :179): ascending k is x outer, y inner
        int mine = FAST_BOX_PIX;
        for (int k = t; k < FAST_BOX_PIX && mine == FAST_BOX_PIX; k += 256) {
            const unsigned v = sc[k];
            if (v == 0) continue;
            const unsigned me = v & 0x7fffu;
            bool keep = true;
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx)
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy)
                    if (dx != 0 || dy != 0) keep = keep && me >= (sc[k + dx * R + dy] & 0x7fffu);
            if (keep) mine = k;
        }
        if (mine < FAST_BOX_PIX) atomicMin(&s_first, mine);
        __syncthreads();
        const int first = s_first;
        __syncthreads();                                                       // s_first and the tiles are rewritten by the next attempt
        if (first < FAST_BOX_PIX) {
            // ---- :152-157, :179: the corner in image coordinates; :188: its depth, or the call ends without a feature (:191-194)
            if (t == 0) {
                const int c = first / R, r = first - c * R, u = c0 + c + 1, v = r0 + r + 1;
                double rho, xyz[3];
                const int st = fast_gate0(a.pl, u, v, &rho, xyz);
                a.res[0] = st; a.res[2] = u; a.res[3] = v; a.res[4] = rho; a.res[5] = xyz[0]; a.res[6] = xyz[1]; a.res[7] = xyz[2];
            }
            status = -1;
            break;
        }
    }
    if (t == 0) {
        if (status == PRE3_FAST_NO_BOX) { a.res[0] = PRE3_FAST_NO_BOX; for (int k = 2; k < 8; ++k) a.res[k] = 0.0; }
        a.res[1] = used;
        for (int k = used; k < PRE3_FAST_MAX_ATTEMPTS; ++k) { a.res[8 + 2 * k] = 0.0; a.res[9 + 2 * k] = 0.0; }
    }
}

// gate 0 at every listed maximum of the rectangle whose origin is (band, band): verdict and rho per maximum, uv shifted into image coordinates
__global__ __launch_bounds__(256) void k_fast_gate(int band, FastPlanes pl, int32_t *blk, double *rho)
{
    const int k = blockIdx.x * 256 + threadIdx.x, K = min(blk[0], PRE3_FAST_MAX_CORNERS);
    if (k >= K) return;
    int32_t *uv = blk + FAST_O_UV;
    const int u = uv[2 * k] + band, v = uv[2 * k + 1] + band;
    double xyz[3];
    blk[FAST_O_VERDICT + k] = fast_gate0(pl, u, v, &rho[k], xyz);
    uv[2 * k] = u; uv[2 * k + 1] = v;
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------------------------
void free_fast(pre3_ctx *c)
{
    FastState *f = c->fast;
    if (!f) return;
    for (hipEvent_t e : f->ev) if (e) (void)hipEventDestroy(e);
    delete f;
    c->fast = nullptr;
}

static int32_t *blk_ints(double *blk) { return reinterpret_cast<int32_t *>(blk + FAST_BLK_DOUBLES); }

static int ensure_fast(pre3_ctx *c, const char *who, size_t px)
{
    if (!c->fast) {
        FastState *f = new (std::nothrow) FastState;
        PRE3_CHECK(f != nullptr, PRE3_E_NOMEM, "%s: out of host memory", who);
        // the state is the group: the context takes it complete, or it goes with what it allocated
        int rc = f->mem.fixed.dev(&f->blk, FAST_BLK_BYTES, Zero::none());
        if (rc == PRE3_OK) rc = f->mem.fixed.pin(&f->blk_host, FAST_BLK_BYTES, PIN_DEFAULT);
        if (rc != PRE3_OK) { delete f; return rc; }
        c->fast = f;
    }
    FastState *f = c->fast;
    if (f->map_px < px) {
        PRE3_TRY(stream_drain(c, who));
        f->map = nullptr; f->map_px = 0;
        PRE3_TRY(f->mem.map.reserve(sizeof(uint16_t) * px, sizeof(uint16_t) * px, Zero::none()));
        f->map = f->mem.map.as<uint16_t>(); f->map_px = px;
    }
    return PRE3_OK;
}

static int timing_begin(pre3_ctx *c)
{
    FastState *f = c->fast;
    f->ev_valid = false;
    if (!c->kt.enabled) return PRE3_OK;
    for (hipEvent_t &e : f->ev) if (!e) PRE3_HIP(hipEventCreate(&e));
    PRE3_HIP(hipEventRecord(f->ev[0], c->stream));
    return PRE3_OK;
}
static int timing_end(pre3_ctx *c)
{
    FastState *f = c->fast;
    if (!c->kt.enabled) return PRE3_OK;
    PRE3_HIP(hipEventRecord(f->ev[1], c->stream));
    f->ev_valid = true;
    return PRE3_OK;
}

// the two detector launches over a rectangle of the resident image; the list stays in the block
static int launch_detect(pre3_ctx *c, int r0, int c0, int rows, int cols, int threshold, int barrier, int nonmax)
{
    PatchState *p = c->patch;
    FastState *f = c->fast;
    const int strips = ceil_div(cols, FAST_STRIP);               // <= FAST_MAX_STRIPS: cols <= PATCH_MAX_DIM
    const FastArgs fa{ p->img, p->rows, r0, c0, rows, cols, threshold, barrier, nonmax ? 1 : 0, f->map, blk_ints(f->blk) };
    hipLaunchKernelGGL(k_fast_strip, dim3(strips), dim3(256), 0, c->stream, fa);
    PRE3_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_fast_emit, dim3(strips), dim3(256), 0, c->stream, rows, cols, (const uint16_t *)f->map, blk_ints(f->blk));
    PRE3_HIP(hipGetLastError());
    return PRE3_OK;
}

int fast_detect(pre3_ctx *c, int r0, int c0, int rows, int cols, int threshold, int barrier, int nonmax, int32_t *K_out, int32_t *uv_out, int32_t *score_out)
{
    const char *who = "pre3_fast_detect";
    PRE3_CHECK(K_out != nullptr && uv_out != nullptr, PRE3_E_ARG, "%s: null K_out or uv_out", who);
    *K_out = 0;
    PRE3_CHECK(threshold >= 0 && barrier >= 0, PRE3_E_ARG, "%s: threshold %d, barrier %d (neither may be negative)", who, threshold, barrier);
    PRE3_CHECK(rows >= FAST_MIN_DIM && cols >= FAST_MIN_DIM, PRE3_E_ARG, "%s: a %d x %d rectangle has no candidate pixel (at least %d x %d)", who, rows, cols, FAST_MIN_DIM, FAST_MIN_DIM);
    PatchState *p = c->patch;
    PRE3_CHECK(p != nullptr && p->img_set, PRE3_E_STATE, "%s: call pre3_set_image first", who);
    PRE3_CHECK(r0 >= 0 && c0 >= 0 && rows <= p->rows - r0 && cols <= p->cols - c0, PRE3_E_ARG, "%s: rows [%d, %d) x columns [%d, %d) leave the %d x %d image", who, r0, r0 + rows,
               c0, c0 + cols, p->rows, p->cols);
    PRE3_TRY(ensure_fast(c, who, (size_t)p->rows * p->cols));
    FastState *f = c->fast;
    PRE3_TRY(timing_begin(c));
    PRE3_TRY(launch_detect(c, r0, c0, rows, cols, threshold, barrier, nonmax));
    PRE3_TRY(timing_end(c));
    PRE3_HIP(hipMemcpyAsync(blk_ints(f->blk_host), blk_ints(f->blk), sizeof(int32_t) * FAST_O_VERDICT, hipMemcpyDeviceToHost, c->stream));
    PRE3_TRY(stream_drain(c, who));                              // the call's one host wait
    const int32_t *hb = blk_ints(f->blk_host);
    const int K = hb[0];
    PRE3_CHECK(K >= 0 && (size_t)K <= (size_t)rows * cols, PRE3_E_STATE, "%s: inconsistent count %d", who, K);
    PRE3_CHECK(K <= PRE3_FAST_MAX_CORNERS, PRE3_E_NOMEM, "%s: %d corners, the list holds %d (raise the threshold or take a smaller rectangle)", who, K, PRE3_FAST_MAX_CORNERS);
    *K_out = K;
    for (int i = 0; i < 2 * K; ++i) uv_out[i] = hb[FAST_O_UV + i];
    if (score_out) for (int i = 0; i < K; ++i) score_out[i] = hb[FAST_O_SCORE + i];
    return PRE3_OK;
}

// what the two initialisation calls share: the context between steps, the image, a frame of its shape on the context's device
static int init_checks(pre3_ctx *c, const char *who, pre3_sr_frame *fr, double std_pxl, int *threshold, int *barrier, int def_threshold, SrFrameView *v)
{
    PRE3_CHECK(fr != nullptr, PRE3_E_ARG, "%s: null frame", who);
    PRE3_CHECK(std::isfinite(std_pxl) && std_pxl > 0, PRE3_E_ARG, "%s: std_pxl must be finite and positive", who);
    if (*threshold == -1) *threshold = def_threshold;            // initialize_a_feature.m:103 / initialize_n_features_FAST.m:70
    if (*barrier == -1) *barrier = 20;                           // :105 / :82
    PRE3_CHECK(*threshold >= 0 && *barrier >= 0, PRE3_E_ARG, "%s: threshold %d, barrier %d (-1: the reference's; otherwise not negative)", who, *threshold, *barrier);
    PatchState *p = c->patch;
    PRE3_CHECK(c->have_cam, PRE3_E_STATE, "%s: camera not set", who);
    PRE3_CHECK(p != nullptr && p->img_set, PRE3_E_STATE, "%s: call pre3_set_image first", who);
    PRE3_CHECK(c->x_valid[PRE3_X_K_K] && c->p_which == PRE3_X_K_K, PRE3_E_STATE, "%s: needs (x_k_k, p_k_k) on the device (features are initialised between steps)", who);
    PRE3_TRY(sr_frame_view(fr, v));
    PRE3_CHECK(v->device == c->device, PRE3_E_ARG, "%s: the frame is on device %d, the context on device %d", who, v->device, c->device);
    PRE3_CHECK(v->rows == p->rows && v->cols == p->cols, PRE3_E_ARG, "%s: the frame is %d x %d, the resident image %d x %d", who, v->rows, v->cols, p->rows, p->cols);
    return PRE3_OK;
}

int fast_init_feature(pre3_ctx *c, pre3_sr_frame *fr, double std_pxl, int strict_reference, int threshold, int barrier, const int32_t *centres, int attempts,
                      uint64_t seed, uint64_t seq, pre3_fast_init_result *out)
{
    const char *who = centres ? "pre3_init_feature_fast" : "pre3_init_feature_fast_seeded";
    PRE3_CHECK(out != nullptr, PRE3_E_ARG, "%s: null result", who);
    SrFrameView v;
    PRE3_TRY(init_checks(c, who, fr, std_pxl, &threshold, &barrier, 10, &v));
    PatchState *p = c->patch;
    // initialize_a_feature.m:65-68 with BoxLimX = [1 nCols], BoxLimY = [1 nRows]: the centres that can be drawn
    const int r_lo = FAST_BAND + FAST_BOX_ROWS / 2, r_hi = (p->rows - 1) - FAST_BAND - FAST_BOX_ROWS / 2, c_lo = FAST_BAND + FAST_BOX_COLS / 2, c_hi = (p->cols - 1) - FAST_BAND - FAST_BOX_COLS / 2;
    PRE3_CHECK(r_hi >= r_lo && c_hi >= c_lo, PRE3_E_ARG, "%s: a %d x %d image has no room for a box centre (at least %d x %d)", who, p->rows, p->cols, 2 * r_lo + 1, 2 * c_lo + 1);
    PRE3_CHECK(attempts >= 1 && attempts <= PRE3_FAST_MAX_ATTEMPTS, PRE3_E_ARG, "%s: %d attempts outside 1 .. %d", who, attempts, PRE3_FAST_MAX_ATTEMPTS);
    BoxArgs ba{};
    for (int a = 0; a < attempts && centres; ++a) {
        PRE3_CHECK(centres[2 * a] >= r_lo && centres[2 * a] <= r_hi && centres[2 * a + 1] >= c_lo && centres[2 * a + 1] <= c_hi, PRE3_E_ARG,
                   "%s: centre %d (row %d, column %d) outside rows %d .. %d, columns %d .. %d", who, a, centres[2 * a], centres[2 * a + 1], r_lo, r_hi, c_lo, c_hi);
        ba.centres[2 * a] = centres[2 * a]; ba.centres[2 * a + 1] = centres[2 * a + 1];
    }
    PRE3_CHECK(c->N + 1 <= c->capN, PRE3_E_NOMEM, "%s: the context holds %d landmarks of %d: no room for a new one", who, c->N, c->capN);
    PRE3_TRY(ensure_fast(c, who, (size_t)p->rows * p->cols));
    FastState *f = c->fast;
    // predict_camera_measurements at x_k_k (:48): the existing projection launch
    if (c->N > 0) PRE3_TRY(launch_project(c, PRE3_X_K_K, 1));
    c->projected = false; c->innovated = false;                  // :211-213: the h are cleared again
    ba.img = p->img; ba.nRows = p->rows; ba.nCols = p->cols; ba.thr = threshold; ba.bar = barrier; ba.strict = strict_reference ? 1 : 0; ba.attempts = attempts;
    ba.seeded = centres ? 0 : 1; ba.seed = seed; ba.seq = seq; ba.N = c->N; ba.h = c->lm.h; ba.has_h = c->lm.has_h;
    ba.pl = FastPlanes{ v.x, v.y, v.z, v.conf, v.maxima, v.has_conf, v.rows }; ba.res = f->blk;
    PRE3_TRY(sr_frame_lend(fr, c->stream));
    PRE3_TRY(timing_begin(c));
    hipLaunchKernelGGL(k_fast_box, dim3(1), dim3(256), 0, c->stream, ba);
    PRE3_HIP(hipGetLastError());
    PRE3_TRY(timing_end(c));
    PRE3_TRY(sr_frame_reclaim(fr, c->stream));
    PRE3_HIP(hipMemcpyAsync(f->blk_host, f->blk, sizeof(double) * FAST_RES, hipMemcpyDeviceToHost, c->stream));
    PRE3_TRY(stream_drain(c, who));                              // the call's one host wait
    const double *r = f->blk_host;
    *out = pre3_fast_init_result{};
    out->status = (int32_t)r[0]; out->attempts = (int32_t)r[1]; out->landmark = -1;
    PRE3_CHECK(out->status >= PRE3_FAST_INITIALISED && out->status <= PRE3_FAST_NO_DEPTH_CONF && out->attempts >= 1 && out->attempts <= attempts, PRE3_E_HIP, "%s: inconsistent result block", who);
    for (int k = 0; k < 2 * PRE3_FAST_MAX_ATTEMPTS; ++k) out->centres[k] = (int32_t)r[8 + k];
    if (out->status == PRE3_FAST_NO_BOX) return PRE3_OK;
    out->uv[0] = (int32_t)r[2]; out->uv[1] = (int32_t)r[3]; out->rho = r[4];
    for (int k = 0; k < 3; ++k) out->xyz[k] = r[5 + k];
    if (out->status != PRE3_FAST_INITIALISED) return PRE3_OK;
    // (a NaN y or z passes the depth gate, as in the reference: such a rho cannot enter the map)
    PRE3_CHECK(std::isfinite(out->rho) && out->rho > 0, PRE3_E_NUMERIC, "%s: the corner at (%d, %d) has a rho that is not finite and positive (a NaN y or z passes the depth gate)", who,
               out->uv[0], out->uv[1]);
    // :195-203: add_features_inverse_depth and add_feature_to_info_vector_my_version, queued behind the wait -- the existing calls, as a caller makes them
    const double uvd[2] = { (double)out->uv[0], (double)out->uv[1] };
    PRE3_TRY(pre3_map_add_inverse_depth(c, 1, uvd, std_pxl, &out->rho));
    out->landmark = c->N - 1;
    return patch_cut(c, out->landmark, 1, out->uv);
}

int fast_init_all(pre3_ctx *c, pre3_sr_frame *fr, double std_pxl, int threshold, int barrier, int32_t *K_out, int32_t *n_added_out, int32_t *uv_out,
                  double *rho_out, int32_t *verdict_out)
{
    const char *who = "pre3_init_features_fast_all";
    PRE3_CHECK(K_out != nullptr && n_added_out != nullptr, PRE3_E_ARG, "%s: null K_out or n_added_out", who);
    *K_out = 0; *n_added_out = 0;
    SrFrameView v;
    PRE3_TRY(init_checks(c, who, fr, std_pxl, &threshold, &barrier, 5, &v));
    PatchState *p = c->patch;
    // initialize_n_features_FAST.m:62-64: the image inside the 20-pixel band
    const int rows = p->rows - 2 * FAST_ALL_BAND, cols = p->cols - 2 * FAST_ALL_BAND;
    PRE3_CHECK(rows >= FAST_MIN_DIM && cols >= FAST_MIN_DIM, PRE3_E_ARG, "%s: a %d x %d image has no candidate pixel inside the %d-pixel band", who, p->rows, p->cols, FAST_ALL_BAND);
    PRE3_TRY(ensure_fast(c, who, (size_t)p->rows * p->cols));
    FastState *f = c->fast;
    PRE3_TRY(timing_begin(c));
    PRE3_TRY(launch_detect(c, FAST_ALL_BAND, FAST_ALL_BAND, rows, cols, threshold, barrier, 1));
    PRE3_TRY(sr_frame_lend(fr, c->stream));
    hipLaunchKernelGGL(k_fast_gate, dim3(PRE3_FAST_MAX_CORNERS / 256), dim3(256), 0, c->stream, FAST_ALL_BAND, FastPlanes{ v.x, v.y, v.z, v.conf, v.maxima, v.has_conf, v.rows },
                       blk_ints(f->blk), f->blk + FAST_RES);
    PRE3_HIP(hipGetLastError());
    PRE3_TRY(timing_end(c));
    PRE3_TRY(sr_frame_reclaim(fr, c->stream));
    PRE3_HIP(hipMemcpyAsync(f->blk_host, f->blk, sizeof(double) * FAST_BLK_DOUBLES + sizeof(int32_t) * FAST_O_CENTRES, hipMemcpyDeviceToHost, c->stream));
    PRE3_TRY(stream_drain(c, who));                              // the call's one host wait
    const int32_t *hb = blk_ints(f->blk_host);
    const double *h_rho = f->blk_host + FAST_RES;
    const int K = hb[0];
    PRE3_CHECK(K >= 0 && (size_t)K <= (size_t)rows * cols, PRE3_E_STATE, "%s: inconsistent count %d", who, K);
    PRE3_CHECK(K <= PRE3_FAST_MAX_CORNERS, PRE3_E_NOMEM, "%s: %d maxima, the list holds %d", who, K, PRE3_FAST_MAX_CORNERS);
    // the survivors in scan order (:118-127); every check before the map is touched
    std::vector<double> uvd, rho;
    std::vector<int32_t> uvi;
    for (int k = 0; k < K; ++k) {
        if (hb[FAST_O_VERDICT + k] != PRE3_FAST_INITIALISED) continue;
        PRE3_CHECK(std::isfinite(h_rho[k]) && h_rho[k] > 0, PRE3_E_NUMERIC, "%s: the maximum at (%d, %d) has a rho that is not finite and positive (a NaN y or z passes the depth gate)", who,
                   hb[FAST_O_UV + 2 * k], hb[FAST_O_UV + 2 * k + 1]);
        uvd.push_back(hb[FAST_O_UV + 2 * k]); uvd.push_back(hb[FAST_O_UV + 2 * k + 1]); rho.push_back(h_rho[k]);
        uvi.push_back(hb[FAST_O_UV + 2 * k]); uvi.push_back(hb[FAST_O_UV + 2 * k + 1]);
    }
    const int n_add = (int)rho.size();
    PRE3_CHECK(c->N + n_add <= c->capN, PRE3_E_NOMEM, "%s: %d maxima pass the depth gate, the context has room for %d (%d landmarks of %d)", who, n_add, c->capN - c->N, c->N, c->capN);
    *K_out = K;
    if (uv_out) for (int i = 0; i < 2 * K; ++i) uv_out[i] = hb[FAST_O_UV + i];
    if (rho_out) for (int i = 0; i < K; ++i) rho_out[i] = h_rho[i];
    if (verdict_out) for (int i = 0; i < K; ++i) verdict_out[i] = hb[FAST_O_VERDICT + i];
    if (n_add == 0) return PRE3_OK;
    const int first = c->N;
    PRE3_TRY(pre3_map_add_inverse_depth(c, n_add, uvd.data(), std_pxl, rho.data()));
    *n_added_out = n_add;
    return patch_cut(c, first, n_add, uvi.data());
}

int fast_timing(pre3_ctx *c, double *detect_ms)
{
    FastState *f = c->fast;
    PRE3_CHECK(f != nullptr && f->ev_valid, PRE3_E_STATE, "pre3_fast_timing: no call of pre3_fast_detect / pre3_init_feature_fast / pre3_init_features_fast_all has run under pre3_kernel_timing");
    PRE3_TRY(stream_drain(c, "pre3_fast_timing"));
    float ms = 0;
    PRE3_HIP(hipEventElapsedTime(&ms, f->ev[0], f->ev[1]));
    if (detect_ms) *detect_ms = ms;
    return PRE3_OK;
}

}  // namespace pre3
