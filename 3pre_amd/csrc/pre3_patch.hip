// pre3_patch.hip -- search_IC_matches.m:45-51, the patch branch: predict_features_appearance.m:34-53 + pred_patch_fc.m:27-85 (k_patch_warp),
// mex_files/CorePar_Ver1/matching.m:39-146 over corrcoef_partitioned.m:3-21 (k_patch_search), the compaction of the accepted landmarks, and the
// bank of stored patches (add_feature_to_info_vector_my_version.m:33-41: k_patch_cut) that follows the map.  fp64 throughout; DESIGN.md section 29.
#include <algorithm>
#include <cmath>
#include <new>
#include <vector>
#include "pre3_patch.h"
#include "pre3_geomdev.h"

namespace pre3 {

// ---------------------------------------------------------------------------------------------------------------------------------------------
// device helpers
// ---------------------------------------------------------------------------------------------------------------------------------------------

// (d_undistort10, undistort_fm_my_version.m's ten Newton steps: pre3_geomdev.h, shared with pre3_pnp.hip)
// distort_fm_my_version.m:52-61
__device__ inline void d_distort(const CamD &cam, double u, double v, double *ud, double *vd)
{
    const double xu = (u - cam.Cx) / cam.f, yu = (v - cam.Cy) / cam.f;
    const double ru = sqrt(xu * xu + yu * yu);
    const double r2 = ru * ru;
    const double D = 1 + cam.k1 * r2 + cam.k2 * (r2 * r2);
    *ud = xu * D * cam.f + cam.Cx;
    *vd = yu * D * cam.f + cam.Cy;
}
// row-major 3 x 3 helpers
__device__ inline void d_inv3(const double *A, double *B)
{
    const double c00 = A[4] * A[8] - A[5] * A[7], c01 = A[5] * A[6] - A[3] * A[8], c02 = A[3] * A[7] - A[4] * A[6];
    const double det = A[0] * c00 + A[1] * c01 + A[2] * c02, id = 1.0 / det;
    B[0] = c00 * id; B[1] = (A[2] * A[7] - A[1] * A[8]) * id; B[2] = (A[1] * A[5] - A[2] * A[4]) * id;
    B[3] = c01 * id; B[4] = (A[0] * A[8] - A[2] * A[6]) * id; B[5] = (A[2] * A[3] - A[0] * A[5]) * id;
    B[6] = c02 * id; B[7] = (A[1] * A[6] - A[0] * A[7]) * id; B[8] = (A[0] * A[4] - A[1] * A[3]) * id;
}
__device__ inline void d_mul3(const double *A, const double *B, double *C)
{
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) C[r * 3 + c] = A[r * 3] * B[c] + A[r * 3 + 1] * B[3 + c] + A[r * 3 + 2] * B[6 + c];
}
__device__ inline void d_mv3(const double *A, const double *x, double *y)
{
    for (int r = 0; r < 3; ++r) y[r] = A[r * 3] * x[0] + A[r * 3 + 1] * x[1] + A[r * 3 + 2] * x[2];
}
__device__ inline double d_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// ---------------------------------------------------------------------------------------------------------------------------------------------
// k_patch_warp: one workgroup per landmark, one lane per sample of the 13 x 13 patch; lane 0 builds the homography once
// ---------------------------------------------------------------------------------------------------------------------------------------------
struct WarpArgs {
    int N; const double *x; const int32_t *type, *off; const double *h; const int32_t *has_h; const double *meta; const uint8_t *pb;
    CamD cam; double fd; double *warp; int32_t *wstatus;
};
__global__ __launch_bounds__(192) void k_patch_warp(WarpArgs a)
{
    __shared__ double sH[9], sC[4];
    __shared__ int sSt;
    const int b = blockIdx.x, t = threadIdx.x;
    const double *mt = a.meta + (size_t)b * PATCH_META;
    if (t == 0) {
        int st = PRE3_PATCH_WARPED;
        const double h0 = a.h[2 * b], h1 = a.h[2 * b + 1];
        if (!a.has_h[b]) st = PRE3_PATCH_NOT_PREDICTED;
        else if (mt[14] == 0.0) st = PRE3_PATCH_NO_PATCH;
        else if (!(h0 > PATCH_HALF && h0 < a.cam.nCols - PATCH_HALF && h1 > PATCH_HALF && h1 < a.cam.nRows - PATCH_HALF)) st = PRE3_PATCH_ZERO;      // pred_patch_fc.m:33-34, :84
        if (st == PRE3_PATCH_WARPED) {
            const CamD &cam = a.cam;
            const double u0 = mt[0], v0 = mt[1];
            double R1[9], R1i[9], R2[9], Rk[9], tk[3], w[3];
            for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) R1[r * 3 + c] = mt[5 + c * 3 + r];
            d_q2r(a.x + 3, R2);
            // H_Wk_p_f = [R1, R1 r1; 0 1], H_Wk = [R2, R2 r2; 0 1] (:40, :43); H_kpf_k = inv(H_Wk_p_f) H_Wk = [R1^-1 R2, R1^-1 R2 r2 - r1] (:46)
            d_inv3(R1, R1i);
            d_mul3(R1i, R2, Rk);
            d_mv3(Rk, a.x, w);
            for (int r = 0; r < 3; ++r) tk[r] = w[r] - mt[2 + r];
            // the normals (:52-60)
            double n1[3] = { u0 - cam.Cx, v0 - cam.Cy, -a.fd }, n2p[3] = { h0 - cam.Cx, h1 - cam.Cy, -a.fd }, n2[3], n[3];
            d_mv3(Rk, n2p, n2);
            for (int r = 0; r < 3; ++r) n2[r] += tk[r];
            const double l1 = sqrt(n1[0] * n1[0] + n1[1] * n1[1] + n1[2] * n1[2]), l2 = sqrt(n2[0] * n2[0] + n2[1] * n2[1] + n2[2] * n2[2]);
            for (int r = 0; r < 3; ++r) n[r] = n1[r] / l1 + n2[r] / l2;
            const double ln = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
            for (int r = 0; r < 3; ++r) n[r] /= ln;
            // XYZ_w (predict_features_appearance.m:36-44), XYZ_kpf = inv(H_Wk_p_f) [XYZ_w; 1], d = -n' XYZ_kpf (:62-64)
            const double *y = a.x + a.off[b];
            double X[3] = { y[0], y[1], y[2] };
            if (a.type[b] == PRE3_INVDEPTH) {
                double sth, cth, sph, cph;
                sincos(y[3], &sth, &cth); sincos(y[4], &sph, &cph);
                X[0] = y[0] + (1 / y[5]) * (cph * sth); X[1] = y[1] + (1 / y[5]) * (-sph); X[2] = y[2] + (1 / y[5]) * (cph * cth);
            }
            double Xk[3];
            d_mv3(R1i, X, Xk);
            for (int r = 0; r < 3; ++r) Xk[r] -= mt[2 + r];
            const double d = -(n[0] * Xk[0] + n[1] * Xk[1] + n[2] * Xk[2]);
            // K (R - t n' / d) inv(K) (rotate_with_dist_fc_c1c2.m:41) and its inverse (rotate_with_dist_fc_c2c1.m:48)
            double M[9], KM[9], Hf[9], Hi[9];
            for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) M[r * 3 + c] = Rk[r * 3 + c] - tk[r] * n[c] / d;
            const double K[9] = { cam.f, 0, cam.Cx, 0, cam.f, cam.Cy, 0, 0, 1 }, Ki[9] = { 1 / cam.f, 0, -cam.Cx / cam.f, 0, 1 / cam.f, -cam.Cy / cam.f, 0, 0, 1 };
            d_mul3(K, M, KM);
            d_mul3(KM, Ki, Hf);
            d_inv3(Hf, Hi);
            // the patch centre in the current image (pred_patch_fc.m:66)
            double uu, vu, p[3], q[3];
            d_undistort10(cam, u0, v0, &uu, &vu);
            p[0] = uu; p[1] = vu; p[2] = 1;
            d_mv3(Hi, p, q);
            d_distort(cam, q[0] / q[2], q[1] / q[2], &sC[0], &sC[1]);
            sC[2] = u0; sC[3] = v0;
            for (int k = 0; k < 9; ++k) sH[k] = Hf[k];
        }
        sSt = st;
    }
    __syncthreads();
    const int st = sSt;
    double *out = a.warp + (size_t)b * PATCH_PIX;
    if (st != PRE3_PATCH_WARPED) {
        if (t < PATCH_PIX) out[t] = 0.0;
        if (t == 0) a.wstatus[b] = st;
        return;
    }
    double val = 0.0;
    if (t < PATCH_PIX) {
        // meshgrid (:68): sample t = col * 13 + row sits at (uc - 6 + col, vc - 6 + row); back into the initial image (:74), shifted into the stored
        // patch (:75-76) and read with interp2, linear, NaN outside [1, 41] (:81)
        const int col = t / PATCH_W, row = t - col * PATCH_W;
        double uu, vu, p[3], q[3], ud, vd;
        d_undistort10(a.cam, sC[0] - PATCH_HALF + col, sC[1] - PATCH_HALF + row, &uu, &vu);
        p[0] = uu; p[1] = vu; p[2] = 1;
        d_mv3(sH, p, q);
        d_distort(a.cam, q[0] / q[2], q[1] / q[2], &ud, &vd);
        const double xs = ud - (sC[2] - PATCH_INIT_HALF - 1), ys = vd - (sC[3] - PATCH_INIT_HALF - 1);
        if (!(xs >= 1.0 && xs <= (double)PATCH_INIT_W && ys >= 1.0 && ys <= (double)PATCH_INIT_W)) val = d_nan();
        else {
            const int x0 = min((int)floor(xs), PATCH_INIT_W - 1), y0 = min((int)floor(ys), PATCH_INIT_W - 1);
            const double fx = xs - x0, fy = ys - y0;
            const uint8_t *pp = a.pb + (size_t)b * PATCH_BYTES + (size_t)(x0 - 1) * PATCH_INIT_W + (y0 - 1);      // patch(v, u), column-major
            const double v00 = pp[0], v01 = pp[1], v10 = pp[PATCH_INIT_W], v11 = pp[PATCH_INIT_W + 1];
            const double top = v00 + fx * (v10 - v00), bot = v01 + fx * (v11 - v01);       // (a flat patch interpolates to itself exactly)
            val = top + fy * (bot - top);
        }
        out[t] = val;
    }
    const int any_nan = __syncthreads_or(val != val);
    if (t == 0) a.wstatus[b] = any_nan ? PRE3_PATCH_OUTSIDE : PRE3_PATCH_WARPED;
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// k_patch_search: one workgroup per landmark.  Window columns -> per-column candidate runs -> prefix sum (a candidate's ordinal in the scan order
// of matching.m:74-77) -> lanes take candidates -> arg-max, the lowest ordinal winning ties.
// ---------------------------------------------------------------------------------------------------------------------------------------------
constexpr int PS_THREADS = 256;
struct SearchArgs {
    int N; const uint8_t *img; int nRows, nCols; const double *h, *S; const double *warp; const int32_t *wstatus; double thr; int mode;
    double *z; double *corr; int32_t *ncand, *status;
};
// Pearson's r of the centred template ac (norm na) and the 13 x 13 bytes at p (leading dimension ld); NaN for a flat image patch, exactly
__device__ __forceinline__ double ncc_at(const double *ac, double na, const uint8_t *p, int ld)
{
    int sb = 0; unsigned sb2 = 0; double dot = 0.0;
    for (int dc = 0; dc < PATCH_W; ++dc) {
        const uint8_t *col = p + dc * ld;
#pragma unroll
        for (int dr = 0; dr < PATCH_W; ++dr) {
            const int v = col[dr];
            sb += v; sb2 += (unsigned)(v * v);
            dot = fma(ac[dc * PATCH_W + dr], (double)v, dot);
        }
    }
    const long long var169 = (long long)PATCH_PIX * (long long)sb2 - (long long)sb * (long long)sb;      // 169 sum(b^2) - sum(b)^2: exact
    if (var169 == 0 || !(na > 0.0)) return d_nan();
    const double r = dot / (na * sqrt((double)var169 / (double)PATCH_PIX));
    return r != r ? r : fmin(fmax(r, -1.0), 1.0);       // corrcoef clamps to [-1, 1]
}
__global__ __launch_bounds__(PS_THREADS) void k_patch_search(SearchArgs a)
{
    __shared__ double ac[PATCH_PIX];
    __shared__ double s_na;
    __shared__ int32_t pre[PATCH_MAX_DIM + 1];
    __shared__ int16_t ia[PATCH_MAX_DIM], cnt[PATCH_MAX_DIM];
    __shared__ int box[4];                      // min column, max column (window-relative), min row, max row of the candidates
    __shared__ double rv[PS_THREADS]; __shared__ int32_t ri[PS_THREADS];
    __shared__ __attribute__((aligned(16))) uint8_t stage[PATCH_STAGE_BYTES];
    const int b = blockIdx.x, t = threadIdx.x;
    const int st = a.wstatus[b];
    if (st == PRE3_PATCH_NOT_PREDICTED || st == PRE3_PATCH_NO_PATCH) {
        if (t == 0) { a.status[b] = st; a.corr[b] = d_nan(); a.ncand[b] = 0; }
        return;
    }
    // ---- the window (matching.m:61-62, :74-77) clipped to the band of :81-82
    const double h0 = a.h[2 * b], h1 = a.h[2 * b + 1];
    const double S11 = a.S[4 * b], S12 = a.S[4 * b + 1], S21 = a.S[4 * b + 2], S22 = a.S[4 * b + 3];
    const double det = S11 * S22 - S12 * S21;
    const double i11 = S22 / det, i12 = -S12 / det, i21 = -S21 / det, i22 = S11 / det;
    int j0 = 1, j1 = 0, i0 = 1, i1 = 0;
    if (isfinite(h0) && isfinite(h1) && isfinite(S11) && isfinite(S22) && S11 >= 0.0 && S22 >= 0.0 && fabs(h0) < 1e8 && fabs(h1) < 1e8) {
        const double hx = fmin(ceil(5 * sqrt(S11)), 1e8), hy = fmin(ceil(5 * sqrt(S22)), 1e8);
        const double cx = round(h0), cy = round(h1);
        j0 = (int)fmax(cx - hx, (double)(PATCH_HALF + 1)); j1 = (int)fmin(cx + hx, (double)(a.nCols - PATCH_HALF - 1));
        i0 = (int)fmax(cy - hy, (double)(PATCH_HALF + 1)); i1 = (int)fmin(cy + hy, (double)(a.nRows - PATCH_HALF - 1));
    }
    const int W = (j1 >= j0 && i1 >= i0) ? j1 - j0 + 1 : 0;      // <= nCols <= PATCH_MAX_DIM
    if (t == 0) { box[0] = W; box[1] = -1; box[2] = 1 << 30; box[3] = -1; }
    __syncthreads();
    for (int c = t; c < W; c += PS_THREADS) {
        const double dx = (double)(j0 + c) - h0;
        int first = 0, n = 0, last = 0;
        for (int i = i0; i <= i1; ++i) {
            const double dy = (double)i - h1;
            const double q = dx * (i11 * dx + i12 * dy) + dy * (i21 * dx + i22 * dy);        // nu' inv(S) nu (:79-80)
            if (q < 5.9915) { if (n == 0) first = i; last = i; ++n; }
        }
        // (a column's candidates are one run: the ellipse is convex)
        ia[c] = (int16_t)first; cnt[c] = (int16_t)(n > 0 ? last - first + 1 : 0);
        if (n > 0) { atomicMin(&box[0], c); atomicMax(&box[1], c); atomicMin(&box[2], first); atomicMax(&box[3], last); }
    }
    __syncthreads();
    if (t == 0) { int s = 0; for (int c = 0; c < W; ++c) { pre[c] = s; s += cnt[c]; } pre[W] = s; }
    // ---- the template, centred once
    const bool have_tmpl = st == PRE3_PATCH_WARPED;
    if (have_tmpl && t < PATCH_PIX) ac[t] = a.warp[(size_t)b * PATCH_PIX + t];
    __syncthreads();
    const int K = pre[W];
    if (have_tmpl && t == 0) {
        double s = 0.0;
        for (int k = 0; k < PATCH_PIX; ++k) s += ac[k];
        s_na = s / PATCH_PIX;
    }
    __syncthreads();
    if (have_tmpl && t < PATCH_PIX) ac[t] -= s_na;
    __syncthreads();
    if (have_tmpl && t == 0) {
        double s = 0.0;
        for (int k = 0; k < PATCH_PIX; ++k) s = fma(ac[k], ac[k], s);
        s_na = sqrt(s);
    }
    // ---- which ordinals the maximum is taken over, and which candidate z is (matching.m:115 / :118 over corrcoef_partitioned.m:3-21)
    int lo = 0, hi = K, zoff = 0;
    if (a.mode != 0) {
        const int n = K + 1;
        if (n < 100) { lo = 1; zoff = -1; }
        else hi = 100 * (n / 100) - 1;
    }
    double best = 0.0; int besti = -1;
    if (have_tmpl && K > 0) {
        // ---- the candidates' bounding box plus the 6-pixel halo, as bytes in LDS when it fits
        const int bc0 = j0 + box[0] - PATCH_HALF, br0 = box[2] - PATCH_HALF;                    // 1-based, inside the image (the band)
        const int SW = box[1] - box[0] + 1 + 2 * PATCH_HALF, SH = box[3] - box[2] + 1 + 2 * PATCH_HALF;
        const bool staged = (long long)SW * SH <= PATCH_STAGE_BYTES;
        if (staged)
            for (int k = t; k < SW * SH; k += PS_THREADS) { const int c = k / SH, r = k - c * SH; stage[k] = a.img[(size_t)(bc0 - 1 + c) * a.nRows + (br0 - 1 + r)]; }
        __syncthreads();
        const double na = s_na;
        for (int k = lo + t; k < hi; k += PS_THREADS) {
            int cl = 0, ch = W - 1;                          // the column with pre[c] <= k < pre[c + 1]
            while (cl < ch) { const int mid = (cl + ch + 1) >> 1; if (pre[mid] <= k) cl = mid; else ch = mid - 1; }
            const int j = j0 + cl, i = ia[cl] + (k - pre[cl]);
            const double r = staged ? ncc_at(ac, na, stage + (size_t)(j - PATCH_HALF - bc0) * SH + (i - PATCH_HALF - br0), SH)
                                    : ncc_at(ac, na, a.img + (size_t)(j - PATCH_HALF - 1) * a.nRows + (i - PATCH_HALF - 1), a.nRows);
            if (r == r && (besti < 0 || r > best)) { best = r; besti = k; }     // max ignores NaN; ordinals ascend, so the first maximum stays
        }
    }
    rv[t] = best; ri[t] = besti;
    __syncthreads();
    for (int s = PS_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) {
            const int o = ri[t + s];
            if (o >= 0 && (ri[t] < 0 || rv[t + s] > rv[t] || (rv[t + s] == rv[t] && o < ri[t]))) { rv[t] = rv[t + s]; ri[t] = o; }
        }
        __syncthreads();
    }
    if (t == 0) {
        int status = st;                                             // a zero patch / a NaN sample: every correlation is NaN
        double corr = d_nan();
        if (have_tmpl) {
            status = K == 0 ? PRE3_PATCH_NO_CANDIDATE : PRE3_PATCH_BELOW;
            if (ri[0] >= 0) {
                corr = rv[0];
                if (corr > a.thr) {
                    status = PRE3_PATCH_MATCHED;
                    const int k = ri[0] + zoff;
                    int cl = 0, ch = W - 1;
                    while (cl < ch) { const int mid = (cl + ch + 1) >> 1; if (pre[mid] <= k) cl = mid; else ch = mid - 1; }
                    a.z[2 * b] = (double)(j0 + cl); a.z[2 * b + 1] = (double)(ia[cl] + (k - pre[cl]));
                }
            }
        }
        a.status[b] = status; a.corr[b] = corr; a.ncand[b] = K;
    }
}

// the accepted landmarks in ascending order: hdr[0] = m, meas[m], zc[2 m] -- one workgroup, a chunk of landmarks per lane
__global__ __launch_bounds__(256) void k_patch_compact(int N, const int32_t *__restrict__ status, const double *__restrict__ z, int32_t *hdr, int32_t *meas, double *zc)
{
    __shared__ int cnts[256];
    const int t = threadIdx.x, per = (N + 255) / 256, lo = min(t * per, N), hi = min(lo + per, N);
    int n = 0;
    for (int i = lo; i < hi; ++i) n += status[i] == PRE3_PATCH_MATCHED;
    cnts[t] = n;
    __syncthreads();
    if (t == 0) { int s = 0; for (int k = 0; k < 256; ++k) { const int v = cnts[k]; cnts[k] = s; s += v; } hdr[0] = s; hdr[1] = 0; }
    __syncthreads();
    int o = cnts[t];
    for (int i = lo; i < hi; ++i)
        if (status[i] == PRE3_PATCH_MATCHED) { meas[o] = i; zc[2 * o] = z[2 * i]; zc[2 * o + 1] = z[2 * i + 1]; ++o; }
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// the bank
// ---------------------------------------------------------------------------------------------------------------------------------------------
// a staged upload [meta 14 doubles per landmark | patches 1681 bytes per landmark] into the bank at `first`
__global__ __launch_bounds__(256) void k_patch_set(int count, const unsigned char *__restrict__ up, uint8_t *__restrict__ pb, double *__restrict__ meta)
{
    const int b = blockIdx.x, t = threadIdx.x;
    const double *m = (const double *)up + (size_t)b * 14;
    const uint8_t *p = up + sizeof(double) * 14 * (size_t)count + (size_t)b * PATCH_BYTES;
    for (int k = t; k < PATCH_BYTES; k += 256) pb[(size_t)b * PATCH_BYTES + k] = p[k];
    if (t < 14) meta[(size_t)b * PATCH_META + t] = m[t];
    if (t == 14) meta[(size_t)b * PATCH_META + 14] = 1.0;
    if (t == 15) meta[(size_t)b * PATCH_META + 15] = 0.0;
}
// add_feature_to_info_vector_my_version.m:33-41: 41 x 41 around the integer pixel uv out of the resident image, r_wc and q2r(q) of x_k_k
__global__ __launch_bounds__(256) void k_patch_cut(const int32_t *__restrict__ uv, const uint8_t *__restrict__ img, int nRows, const double *__restrict__ x,
                                                   uint8_t *__restrict__ pb, double *__restrict__ meta)
{
    const int b = blockIdx.x, t = threadIdx.x;
    const int u = uv[2 * b], v = uv[2 * b + 1];
    for (int k = t; k < PATCH_BYTES; k += 256) {
        const int c = k / PATCH_INIT_W, r = k - c * PATCH_INIT_W;
        pb[(size_t)b * PATCH_BYTES + k] = img[(size_t)(u - PATCH_INIT_HALF - 1 + c) * nRows + (v - PATCH_INIT_HALF - 1 + r)];
    }
    if (t == 0) {
        double R[9], *m = meta + (size_t)b * PATCH_META;
        d_q2r(x + 3, R);
        m[0] = u; m[1] = v; m[2] = x[0]; m[3] = x[1]; m[4] = x[2];
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) m[5 + c * 3 + r] = R[r * 3 + c];
        m[14] = 1.0; m[15] = 0.0;
    }
}
// the bank re-laid out by the map's source list: src[i] = old index of new landmark i, -1: a new landmark without a patch
__global__ __launch_bounds__(256) void k_patch_follow(const int32_t *__restrict__ src, const uint8_t *__restrict__ pb, const double *__restrict__ meta,
                                                      uint8_t *__restrict__ pb_out, double *__restrict__ meta_out)
{
    const int b = blockIdx.x, t = threadIdx.x, s = src[b];
    if (s < 0) { if (t < PATCH_META) meta_out[(size_t)b * PATCH_META + t] = 0.0; return; }
    for (int k = t; k < PATCH_BYTES; k += 256) pb_out[(size_t)b * PATCH_BYTES + k] = pb[(size_t)s * PATCH_BYTES + k];
    if (t < PATCH_META) meta_out[(size_t)b * PATCH_META + t] = meta[(size_t)s * PATCH_META + t];
}
// the image plane of a resident SR4000 frame (doubles holding 0 .. 255) as bytes
__global__ __launch_bounds__(256) void k_patch_image_frame(int n, const double *__restrict__ src, uint8_t *__restrict__ dst)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { const double v = src[i]; dst[i] = (uint8_t)(v >= 255.0 ? 255 : (v > 0.0 ? (int)(v + 0.5) : 0)); }
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------------------------
static size_t blk_doubles(int capN) { return 3 * (size_t)capN; }                        // corr[capN] | zc[2 capN]
static size_t blk_size(int capN) { return sizeof(double) * blk_doubles(capN) + sizeof(int32_t) * (4 + 3 * (size_t)capN); }      // | hdr[4] | meas | status | ncand

static int ensure_patch(pre3_ctx *c)
{
    if (c->patch) return PRE3_OK;
    PatchState *p = new (std::nothrow) PatchState;
    PRE3_CHECK(p != nullptr, PRE3_E_NOMEM, "patch search: out of host memory");
    const size_t N = (size_t)(c->capN > 0 ? c->capN : 1);
    p->up_bytes = up16(N * (PATCH_BYTES + 14 * sizeof(double))) + 16;
    p->blk_bytes = up16(blk_size((int)N));
    // the state is the group: the context takes it complete, or it goes with everything it allocated
    BlockList &m = p->mem.fixed;
    const Zero z = Zero::sync(), nz = Zero::none();
    int rc = PRE3_OK;
    auto A = [&](int r) { if (rc == PRE3_OK) rc = r; };
    A(m.dev(&p->pb, N * PATCH_BYTES, z)); A(m.dev(&p->pb_alt, N * PATCH_BYTES, z));
    A(m.dev(&p->meta, sizeof(double) * N * PATCH_META, z)); A(m.dev(&p->meta_alt, sizeof(double) * N * PATCH_META, z));
    A(m.dev(&p->up, p->up_bytes, nz)); A(m.dev(&p->warp, sizeof(double) * N * PATCH_PIX, nz));
    A(m.dev(&p->wstatus, sizeof(int32_t) * N, nz)); A(m.dev(&p->blk, p->blk_bytes, nz));
    A(m.pin(&p->blk_host, p->blk_bytes, PIN_DEFAULT));
    if (rc == PRE3_OK && hipDeviceSynchronize() != hipSuccess) { set_error("patch search: device allocation failed"); rc = PRE3_E_NOMEM; }
    if (rc != PRE3_OK) { delete p; return rc; }
    c->patch = p;
    return PRE3_OK;
}

void free_patch(pre3_ctx *c)
{
    PatchState *p = c->patch;
    if (!p) return;
    for (hipEvent_t e : p->ev) if (e) (void)hipEventDestroy(e);
    delete p;
    c->patch = nullptr;
}

void patch_drop_bank(pre3_ctx *c)
{
    PatchState *p = c->patch;
    if (!p || !p->bank_set) return;
    (void)hipMemsetAsync(p->meta, 0, sizeof(double) * (size_t)c->capN * PATCH_META, c->stream);
    p->bank_set = false;
}

// the image buffer for the camera's shape (PRE3_E_ARG when the shape is not the camera's)
static int image_reserve(pre3_ctx *c, const char *who, int nRows, int nCols)
{
    PRE3_CHECK(c->have_cam, PRE3_E_STATE, "%s: camera not set", who);
    PRE3_CHECK(nRows == (int)c->cam.nRows && nCols == (int)c->cam.nCols, PRE3_E_ARG, "%s: a %d x %d image, the camera's is %d x %d", who, nRows, nCols, (int)c->cam.nRows, (int)c->cam.nCols);
    PRE3_CHECK(nRows >= 2 * PATCH_HALF + 3 && nCols >= 2 * PATCH_HALF + 3 && nRows <= PATCH_MAX_DIM && nCols <= PATCH_MAX_DIM, PRE3_E_ARG,
               "%s: a %d x %d image (the search takes %d .. %d rows and columns)", who, nRows, nCols, 2 * PATCH_HALF + 3, PATCH_MAX_DIM);
    PRE3_TRY(ensure_patch(c));
    PatchState *p = c->patch;
    if (p->rows != nRows || p->cols != nCols || p->img == nullptr) {
        PRE3_TRY(stream_drain(c, who));
        p->mem.img.release();                 // (replaced for every new shape, a smaller one too)
        p->img = nullptr; p->img_set = false; p->rows = p->cols = 0;
        const size_t bytes = up16((size_t)nRows * nCols);
        PRE3_TRY(p->mem.img.reserve(bytes, bytes, Zero::none()));
        p->img = p->mem.img.as<uint8_t>(); p->rows = nRows; p->cols = nCols;
    }
    return PRE3_OK;
}

int patch_set_image(pre3_ctx *c, int nRows, int nCols, const uint8_t *im)
{
    PRE3_CHECK(im != nullptr, PRE3_E_ARG, "pre3_set_image: null image");
    PRE3_TRY(image_reserve(c, "pre3_set_image", nRows, nCols));
    PatchState *p = c->patch;
    const size_t bytes = (size_t)nRows * nCols;
    void *st = nullptr, *st_dev = nullptr; int slot = 0;
    PRE3_TRY(stage_acquire(c, up16(bytes), &st, &st_dev, &slot));
    memcpy(st, im, bytes);
    PRE3_TRY(launch_pull(c, st, p->img, bytes, slot));
    PRE3_TRY(stage_release(c, slot));
    p->img_set = true;
    return PRE3_OK;
}

int patch_get_image(pre3_ctx *c, int nRows, int nCols, uint8_t *im)
{
    PatchState *p = c->patch;
    PRE3_CHECK(p != nullptr && p->img_set, PRE3_E_STATE, "pre3_get_image: no image has been set");
    PRE3_CHECK(im != nullptr && nRows == p->rows && nCols == p->cols, PRE3_E_ARG, "pre3_get_image: the resident image is %d x %d", p->rows, p->cols);
    PRE3_TRY(stream_drain(c, "pre3_get_image"));
    PRE3_HIP(hipMemcpy(im, p->img, (size_t)nRows * nCols, hipMemcpyDeviceToHost));
    return PRE3_OK;
}

int patch_set_image_frame(pre3_ctx *c, pre3_sr_frame *f)
{
    const char *who = "pre3_set_image_frame";
    PRE3_CHECK(f != nullptr, PRE3_E_ARG, "%s: null handle", who);
    SrFrameView v;
    PRE3_TRY(sr_frame_view(f, &v));
    PRE3_CHECK(v.device == c->device, PRE3_E_ARG, "%s: the frame is on device %d, the context on device %d", who, v.device, c->device);
    PRE3_TRY(image_reserve(c, who, v.rows, v.cols));
    PatchState *p = c->patch;
    const int n = v.rows * v.cols;
    PRE3_TRY(sr_frame_lend(f, c->stream));
    hipLaunchKernelGGL(k_patch_image_frame, dim3(ceil_div(n, 256)), dim3(256), 0, c->stream, n, v.img, p->img);
    PRE3_HIP(hipGetLastError());
    PRE3_TRY(sr_frame_reclaim(f, c->stream));
    p->img_set = true;
    return PRE3_OK;
}

int patch_set_patches(pre3_ctx *c, int first, int count, const uint8_t *patch, const double *uv, const double *r_wc, const double *R_wc)
{
    PRE3_CHECK(first >= 0 && count >= 0 && first + count <= c->N, PRE3_E_ARG, "pre3_set_patches: range [%d, %d) outside the map (N=%d)", first, first + count, c->N);
    PRE3_CHECK(count == 0 || (patch && uv && r_wc && R_wc), PRE3_E_ARG, "pre3_set_patches: null pointer");
    for (int i = 0; i < count; ++i) {
        bool fin = std::isfinite(uv[2 * i]) && std::isfinite(uv[2 * i + 1]);
        for (int k = 0; k < 3; ++k) fin = fin && std::isfinite(r_wc[3 * i + k]);
        for (int k = 0; k < 9; ++k) fin = fin && std::isfinite(R_wc[9 * i + k]);
        PRE3_CHECK(fin, PRE3_E_ARG, "pre3_set_patches: landmark %d has a non-finite uv, r_wc or R_wc", first + i);
    }
    PRE3_TRY(ensure_patch(c));
    PatchState *p = c->patch;
    if (count) {
        const size_t mbytes = sizeof(double) * 14 * (size_t)count, bytes = mbytes + (size_t)count * PATCH_BYTES;
        void *st = nullptr, *st_dev = nullptr; int slot = 0;
        PRE3_TRY(stage_acquire(c, up16(bytes), &st, &st_dev, &slot));
        double *m = static_cast<double *>(st);
        for (int i = 0; i < count; ++i) {
            m[14 * i] = uv[2 * i]; m[14 * i + 1] = uv[2 * i + 1];
            for (int k = 0; k < 3; ++k) m[14 * i + 2 + k] = r_wc[3 * i + k];
            for (int k = 0; k < 9; ++k) m[14 * i + 5 + k] = R_wc[9 * i + k];
        }
        memcpy(static_cast<unsigned char *>(st) + mbytes, patch, (size_t)count * PATCH_BYTES);
        PRE3_TRY(launch_pull(c, st, p->up, bytes, slot));
        PRE3_TRY(stage_release(c, slot));
        hipLaunchKernelGGL(k_patch_set, dim3(count), dim3(256), 0, c->stream, count, p->up, p->pb + (size_t)first * PATCH_BYTES, p->meta + (size_t)first * PATCH_META);
        PRE3_HIP(hipGetLastError());
    }
    p->bank_set = true;
    return PRE3_OK;
}

int patch_get_patches(pre3_ctx *c, int first, int count, uint8_t *patch, double *uv, double *r_wc, double *R_wc, int32_t *has)
{
    PatchState *p = c->patch;
    PRE3_CHECK(first >= 0 && count >= 0 && first + count <= c->N, PRE3_E_ARG, "pre3_get_patches: range [%d, %d) outside the map (N=%d)", first, first + count, c->N);
    PRE3_CHECK(p != nullptr && p->bank_set, PRE3_E_STATE, "pre3_get_patches: no patch has been set");
    PRE3_TRY(stream_drain(c, "pre3_get_patches"));
    if (count == 0) return PRE3_OK;
    if (patch) PRE3_HIP(hipMemcpy(patch, p->pb + (size_t)first * PATCH_BYTES, (size_t)count * PATCH_BYTES, hipMemcpyDeviceToHost));
    std::vector<double> m((size_t)count * PATCH_META);
    PRE3_HIP(hipMemcpy(m.data(), p->meta + (size_t)first * PATCH_META, sizeof(double) * m.size(), hipMemcpyDeviceToHost));
    for (int i = 0; i < count; ++i) {
        const double *mi = m.data() + (size_t)i * PATCH_META;
        if (uv) { uv[2 * i] = mi[0]; uv[2 * i + 1] = mi[1]; }
        if (r_wc) for (int k = 0; k < 3; ++k) r_wc[3 * i + k] = mi[2 + k];
        if (R_wc) for (int k = 0; k < 9; ++k) R_wc[9 * i + k] = mi[5 + k];
        if (has) has[i] = mi[14] != 0.0;
        if (patch && mi[14] == 0.0) memset(patch + (size_t)i * PATCH_BYTES, 0, PATCH_BYTES);      // (a landmark without a patch reads zeros)
    }
    return PRE3_OK;
}

int patch_cut(pre3_ctx *c, int first, int count, const int32_t *uv)
{
    PatchState *p = c->patch;
    PRE3_CHECK(first >= 0 && count >= 0 && first + count <= c->N, PRE3_E_ARG, "pre3_patch_cut: range [%d, %d) outside the map (N=%d)", first, first + count, c->N);
    PRE3_CHECK(count == 0 || uv != nullptr, PRE3_E_ARG, "pre3_patch_cut: null pointer");
    PRE3_CHECK(p != nullptr && p->img_set, PRE3_E_STATE, "pre3_patch_cut: no image has been set");
    PRE3_CHECK(c->x_valid[PRE3_X_K_K], PRE3_E_STATE, "pre3_patch_cut: x_k_k is not on the device");
    for (int i = 0; i < count; ++i)
        PRE3_CHECK(uv[2 * i] - PATCH_INIT_HALF >= 1 && uv[2 * i] + PATCH_INIT_HALF <= p->cols && uv[2 * i + 1] - PATCH_INIT_HALF >= 1 && uv[2 * i + 1] + PATCH_INIT_HALF <= p->rows,
                   PRE3_E_ARG, "pre3_patch_cut: the 41 x 41 patch around (%d, %d) leaves the %d x %d image", uv[2 * i], uv[2 * i + 1], p->rows, p->cols);
    if (count) {
        const size_t bytes = sizeof(int32_t) * 2 * (size_t)count;
        void *st = nullptr, *st_dev = nullptr; int slot = 0;
        PRE3_TRY(stage_acquire(c, up16(bytes), &st, &st_dev, &slot));
        memcpy(st, uv, bytes);
        PRE3_TRY(launch_pull(c, st, p->up, bytes, slot));
        PRE3_TRY(stage_release(c, slot));
        hipLaunchKernelGGL(k_patch_cut, dim3(count), dim3(256), 0, c->stream, (const int32_t *)p->up, p->img, p->rows, c->x_kk,
                           p->pb + (size_t)first * PATCH_BYTES, p->meta + (size_t)first * PATCH_META);
        PRE3_HIP(hipGetLastError());
    }
    p->bank_set = true;
    return PRE3_OK;
}

int patch_follow_map(pre3_ctx *c, int N_new, const int32_t *d_src)
{
    PatchState *p = c->patch;
    if (!p || !p->bank_set || N_new <= 0) return PRE3_OK;
    hipLaunchKernelGGL(k_patch_follow, dim3(N_new), dim3(256), 0, c->stream, d_src, p->pb, p->meta, p->pb_alt, p->meta_alt);
    PRE3_HIP(hipGetLastError());
    std::swap(p->pb, p->pb_alt); std::swap(p->meta, p->meta_alt);
    return PRE3_OK;
}

static int timing_events(pre3_ctx *c)
{
    PatchState *p = c->patch;
    if (!c->kt.enabled) { p->ev_valid = false; return PRE3_OK; }
    for (hipEvent_t &e : p->ev) if (!e) PRE3_HIP(hipEventCreate(&e));
    return PRE3_OK;
}

static int launch_warp(pre3_ctx *c, double fd)
{
    PatchState *p = c->patch;
    const CamD cam{ c->cam.f, c->cam.Cx, c->cam.Cy, c->cam.k1, c->cam.k2, c->cam.nRows, c->cam.nCols };
    const WarpArgs wa{ c->N, c->x_km1, c->lm.type, c->lm.off, c->lm.h, c->lm.has_h, p->meta, p->pb, cam, fd, p->warp, p->wstatus };
    hipLaunchKernelGGL(k_patch_warp, dim3(c->N), dim3(192), 0, c->stream, wa);
    PRE3_HIP(hipGetLastError());
    return PRE3_OK;
}

int patch_predict(pre3_ctx *c, double focal_over_d, double *patch_out, int32_t *status_out)
{
    const char *who = "pre3_predict_patches";
    PRE3_CHECK(std::isfinite(focal_over_d) && focal_over_d > 0, PRE3_E_ARG, "%s: focal_over_d must be finite and positive", who);
    PRE3_CHECK(status_out != nullptr, PRE3_E_ARG, "%s: null status_out", who);
    PRE3_CHECK(c->have_cam, PRE3_E_STATE, "%s: camera not set", who);
    PRE3_CHECK(c->x_valid[PRE3_X_K_KM1] && (c->projected || c->N == 0), PRE3_E_STATE, "%s: needs a projection at x_k_km1 (pre3_project)", who);
    if (c->N == 0) return PRE3_OK;
    PRE3_TRY(ensure_patch(c));
    PatchState *p = c->patch;
    PRE3_TRY(launch_warp(c, focal_over_d));
    PRE3_TRY(stream_drain(c, who));
    PRE3_HIP(hipMemcpy(status_out, p->wstatus, sizeof(int32_t) * c->N, hipMemcpyDeviceToHost));
    if (patch_out) PRE3_HIP(hipMemcpy(patch_out, p->warp, sizeof(double) * (size_t)c->N * PATCH_PIX, hipMemcpyDeviceToHost));
    return PRE3_OK;
}

int patch_search(pre3_ctx *c, double focal_over_d, double corr_threshold, int strict_reference, int32_t *m_out, int32_t *meas_idx_out, double *z_out,
                 double *corr_out, int32_t *ncand_out, int32_t *status_out)
{
    const char *who = "pre3_patch_search";
    PatchState *p = c->patch;
    PRE3_CHECK(m_out != nullptr, PRE3_E_ARG, "%s: null m_out", who);
    PRE3_CHECK(std::isfinite(focal_over_d) && focal_over_d > 0, PRE3_E_ARG, "%s: focal_over_d must be finite and positive", who);
    PRE3_CHECK(!std::isnan(corr_threshold), PRE3_E_ARG, "%s: the correlation threshold is NaN", who);
    PRE3_CHECK(c->x_valid[PRE3_X_K_KM1] && c->p_which == PRE3_X_K_KM1, PRE3_E_STATE, "%s: needs the predicted estimate (call a prediction first)", who);
    PRE3_CHECK(p != nullptr && p->img_set, PRE3_E_STATE, "%s: call pre3_set_image first", who);
    const int N = c->N;
    if (N == 0) {
        *m_out = 0;
        c->projected = true; c->innovated = true;
        return install_measurements(c, 0, nullptr, nullptr, nullptr, 0);
    }
    PRE3_CHECK(c->have_cam, PRE3_E_STATE, "%s: camera not set", who);
    PRE3_CHECK(p->rows == (int)c->cam.nRows && p->cols == (int)c->cam.nCols, PRE3_E_STATE, "%s: the resident image is %d x %d, the camera's %d x %d", who, p->rows, p->cols,
               (int)c->cam.nRows, (int)c->cam.nCols);
    // search_IC_matches.m:31-44: h, H, S at the prediction -- pre3_ic_search's launch, as it calls it
    PRE3_TRY(launch_project_innovation(c, PRE3_X_K_KM1, 1, 0, 0.0, true, true, nullptr));
    c->projected = true; c->innovated = true;
    PRE3_TRY(timing_events(c));
    const bool timed = c->kt.enabled;
    const int capN = c->capN;
    double *b_corr = static_cast<double *>(p->blk), *b_zc = b_corr + capN;
    int32_t *b_hdr = reinterpret_cast<int32_t *>(b_corr + blk_doubles(capN)), *b_meas = b_hdr + 4, *b_status = b_meas + capN, *b_ncand = b_status + capN;
    if (timed) PRE3_HIP(hipEventRecord(p->ev[0], c->stream));
    PRE3_TRY(launch_warp(c, focal_over_d));
    if (timed) { PRE3_HIP(hipEventRecord(p->ev[1], c->stream)); PRE3_HIP(hipEventRecord(p->ev[2], c->stream)); }
    const SearchArgs sa{ N, p->img, p->rows, p->cols, c->lm.h, c->lm.S, p->warp, p->wstatus, corr_threshold, strict_reference ? 1 : 0, c->lm.z, b_corr, b_ncand, b_status };
    hipLaunchKernelGGL(k_patch_search, dim3(N), dim3(PS_THREADS), 0, c->stream, sa);
    PRE3_HIP(hipGetLastError());
    if (timed) { PRE3_HIP(hipEventRecord(p->ev[3], c->stream)); p->ev_valid = true; }
    hipLaunchKernelGGL(k_patch_compact, dim3(1), dim3(256), 0, c->stream, N, b_status, c->lm.z, b_hdr, b_meas, b_zc);
    PRE3_HIP(hipGetLastError());
    PRE3_HIP(hipMemcpyAsync(p->blk_host, p->blk, blk_size(capN), hipMemcpyDeviceToHost, c->stream));
    PRE3_TRY(stream_drain(c, who));                        // the call's one host wait
    const double *h_corr = static_cast<const double *>(p->blk_host), *h_zc = h_corr + capN;
    const int32_t *h_hdr = reinterpret_cast<const int32_t *>(h_corr + blk_doubles(capN)), *h_meas = h_hdr + 4, *h_status = h_meas + capN, *h_ncand = h_status + capN;
    const int m = h_hdr[0];
    PRE3_CHECK(m >= 0 && m <= N, PRE3_E_STATE, "%s: inconsistent count (%d accepted of %d)", who, m, N);
    std::vector<int32_t> meas(h_meas, h_meas + m);
    *m_out = m;
    if (meas_idx_out) for (int j = 0; j < m; ++j) meas_idx_out[j] = meas[j];
    if (z_out) for (int j = 0; j < 2 * m; ++j) z_out[j] = h_zc[j];
    if (corr_out) for (int i = 0; i < N; ++i) corr_out[i] = h_corr[i];
    if (ncand_out) for (int i = 0; i < N; ++i) ncand_out[i] = h_ncand[i];
    if (status_out) for (int i = 0; i < N; ++i) status_out[i] = h_status[i];
    // z of the accepted is on the device where the kernel left it: the path pre3_ic_search ends in
    return install_measurements(c, m, meas.data(), nullptr, nullptr, 0);
}

int patch_timing(pre3_ctx *c, double *warp_ms, double *search_ms)
{
    PatchState *p = c->patch;
    PRE3_CHECK(p != nullptr && p->ev_valid, PRE3_E_STATE, "pre3_patch_timing: no pre3_patch_search has run under pre3_kernel_timing");
    PRE3_TRY(stream_drain(c, "pre3_patch_timing"));
    float a = 0, b = 0;
    PRE3_HIP(hipEventElapsedTime(&a, p->ev[0], p->ev[1]));
    PRE3_HIP(hipEventElapsedTime(&b, p->ev[2], p->ev[3]));
    if (warp_ms) *warp_ms = a;
    if (search_ms) *search_ms = b;
    return PRE3_OK;
}

}  // namespace pre3
