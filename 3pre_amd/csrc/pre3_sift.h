// pre3_sift.h -- the arithmetic of the SIFT extractor (pre3_sift.hip), as functions that compile for the device and for the
// host: the scale-space plan, doubleSize in both forms, the tap sum of imsmooth, the DoG extremum test, the boundary test, one keypoint's
// refinement, the frame scaling, and the per-sample arithmetic of the orientation histogram and of the descriptor.
//   sift/sift_vedal.m:127-139,205,238-298      sift/gaussianss.m:72-80,129-227      sift/diffss.m:57-66      sift/imsmooth.c:44-80,128-160
//   sift/siftlocalmax.c:229-249                sift/siftrefinemx.c:150-303          sift/siftormx.c:138-253  sift/siftdescriptor.c:110-141,310-513
// Every statement a test pins bit for bit is compiled without contraction: one product or one sum per rounding, as numpy rounds them
// (tests/sift_ref.py).  tests/test_sift_ref.py builds this header with the host compiler and compares it with that restatement.
// Planes are column-major, M rows by N columns: pixel (row y, column x) at y + x * M; a level of an octave is one such plane.
#pragma once
#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "pre3_sr.h"

namespace pre3 {

constexpr int SIFT_S = 3, SIFT_OMIN = -1, SIFT_SMIN = -1, SIFT_SMAX = SIFT_S + 1;      // sift_vedal.m:130-131,205
constexpr int SIFT_NLEV = SIFT_SMAX - SIFT_SMIN + 1;                                    // 6 Gaussian levels per octave
constexpr int SIFT_NDOG = SIFT_NLEV - 1;                                                // 5 DoG levels
constexpr int SIFT_MAX_OCTAVES = 24;
constexpr int SIFT_MAX_TAPS = 32;                                                       // 2 W + 1 <= 27 with the defaults
constexpr double SIFT_SIGMAN = 0.5, SIFT_THRESH = 0.04 / 3 / 2, SIFT_R = 10.0, SIFT_MAGNIF = 3.0;      // sift_vedal.m:134-139
constexpr int SIFT_NBP = 4, SIFT_NBO = 8, SIFT_NBINS = 36, SIFT_MAX_PEAKS = SIFT_NBINS / 2;
constexpr double SIFT_2PI = 2 * 3.14159265358979323846;                                 // 2*M_PI

struct SiftLevelPlan { double sigma; int W; double taps[SIFT_MAX_TAPS]; };              // sigma <= 0.01: the level is a copy (imsmooth.c:128,159)
struct SiftPlan {
    int O, rows[SIFT_MAX_OCTAVES], cols[SIFT_MAX_OCTAVES];
    double sigma0, pow2[SIFT_NDOG];                                                     // pow2[s - smin] = 2^(s / S), s = smin .. smax - 1
    SiftLevelPlan lev[2][SIFT_NLEV];                                                    // [0]: the first octave, [1]: every later one
};

// imsmooth.c:130-142: W = ceil(4 s), g(j) = exp(-0.5 (j - W)^2 / s^2) over their running sum
inline void sift_taps(double s, SiftLevelPlan *p)
{
    p->sigma = s; p->W = 0;
    for (int j = 0; j < SIFT_MAX_TAPS; ++j) p->taps[j] = 0.0;
    if (!(s > 0.01)) return;
    const int W = (int)ceil(4 * s);
    p->W = W;
    double acc = 0.0;
    for (int j = 0; j < 2 * W + 1; ++j) { p->taps[j] = exp(-0.5 * (j - W) * (j - W) / (s * s)); acc += p->taps[j]; }
    for (int j = 0; j < 2 * W + 1; ++j) p->taps[j] /= acc;
}

// sift_vedal.m:127-133 and gaussianss.m:72-80,133-203 for an M x N image: false when O < 1
inline bool sift_plan(int M, int N, SiftPlan *p)
{
    const int mn = M < N ? M : N;
    int lg = 0;
    while ((2 << lg) <= mn) ++lg;                                                       // floor(log2(min(M, N)))
    p->O = lg - SIFT_OMIN - 3;
    if (mn < 1 || p->O < 1 || p->O > SIFT_MAX_OCTAVES) return false;
    int m = 2 * M, n = 2 * N;
    for (int o = 0; o < p->O; ++o) { p->rows[o] = m; p->cols[o] = n; m = (m + 1) / 2; n = (n + 1) / 2; }      // halveSize: I(1:2:end, 1:2:end)
    const double k = pow(2.0, 1.0 / SIFT_S);
    p->sigma0 = 1.6 * k;                                                                // sift_vedal.m:133 (2^(1/S) once more: the same bits)
    const double dsigma0 = p->sigma0 * sqrt(1 - 1 / pow(k, 2.0));
    for (int i = 0; i < SIFT_NDOG; ++i) p->pow2[i] = pow(2.0, (double)(SIFT_SMIN + i) / SIFT_S);
    const double a = p->sigma0 * pow(k, (double)SIFT_SMIN), b = SIFT_SIGMAN / pow(2.0, (double)SIFT_OMIN);
    sift_taps(sqrt(pow(a, 2.0) - pow(b, 2.0)), &p->lev[0][0]);                          // gaussianss.m:134-135
    // :183-190: sbest = min(smin + S, smax), target_sigma = sigma0 k^smin, prev_sigma = sigma0 k^(sbest - S): smoothed only when target > prev
    const int sbest = SIFT_SMIN + SIFT_S < SIFT_SMAX ? SIFT_SMIN + SIFT_S : SIFT_SMAX;
    const double target = p->sigma0 * pow(k, (double)SIFT_SMIN), prev = p->sigma0 * pow(k, (double)(sbest - SIFT_S));
    sift_taps(target > prev ? sqrt(pow(target, 2.0) - pow(prev, 2.0)) : 0.0, &p->lev[1][0]);
    for (int s = SIFT_SMIN + 1; s <= SIFT_SMAX; ++s) {                                  // :149, :198
        sift_taps(pow(k, (double)s) * dsigma0, &p->lev[0][s - SIFT_SMIN]);
        p->lev[1][s - SIFT_SMIN] = p->lev[0][s - SIFT_SMIN];
    }
    return true;
}
constexpr int SIFT_SBEST_LEVEL = (SIFT_SMIN + SIFT_S < SIFT_SMAX ? SIFT_SMIN + SIFT_S : SIFT_SMAX) - SIFT_SMIN;

// gaussianss.m:210-224 for the pixel (r, c) of J = doubleSize(I), I being M x N.  strict: the interpolated entries in uint8 class -- every term
// rounded by itself, the sums saturated left to right; else in double.  The last row and the last column stay zero (the 2:2:end-1 ranges).
PRE3_HD double sift_u8_add(double a, double b) { const double s = a + b; return s > 255.0 ? 255.0 : s; }
PRE3_HD double sift_double_size(const double *I, int M, int N, int r, int c, bool strict)
{
#pragma clang fp contract(off)
    const int i = r >> 1, j = c >> 1;
    if (((r | c) & 1) == 0) return I[i + (size_t)j * M];
    if (((r & 1) && i >= M - 1) || ((c & 1) && j >= N - 1)) return 0.0;
    if ((r & 1) && (c & 1)) {
        const double a = 0.25 * I[i + (size_t)j * M], b = 0.25 * I[i + 1 + (size_t)j * M], d = 0.25 * I[i + (size_t)(j + 1) * M],
                     e = 0.25 * I[i + 1 + (size_t)(j + 1) * M];
        if (strict) return sift_u8_add(sift_u8_add(sift_u8_add(matlab_uint8(a), matlab_uint8(b)), matlab_uint8(d)), matlab_uint8(e));
        double s = a + b;
        s = s + d;
        return s + e;
    }
    const double a = 0.5 * I[i + (size_t)j * M], b = 0.5 * ((r & 1) ? I[i + 1 + (size_t)j * M] : I[i + (size_t)(j + 1) * M]);
    if (strict) return sift_u8_add(matlab_uint8(a), matlab_uint8(b));
    return a + b;
}

// imsmooth.c:44-80 (econvolve: PAD_BY_CONTINUITY is defined at :16) for one output sample: 2 W + 1 taps from acc = 0.0 in ascending order, one
// product and one sum per rounding; a tap outside the line reads the nearest end.  src points at the line's first sample, `stride` apart, n long.
PRE3_HD double sift_tap_sum(const double *taps, int W, const double *src, size_t stride, int n, int i)
{
#pragma clang fp contract(off)
    double acc = 0.0;
    for (int t = 0; t < 2 * W + 1; ++t) {
        int k = i - W + t;
        k = k < 0 ? 0 : (k > n - 1 ? n - 1 : k);
        const double p = taps[t] * src[(size_t)k * stride];
        acc = acc + p;
    }
    return acc;
}

// siftlocalmax.c:229-249 on sign * D at the interior point (y, x, s) of the M x N x SIFT_NDOG array D: v >= threshold and v > every one of the 26
// neighbours
PRE3_HD bool sift_is_max(const double *D, int M, int N, int y, int x, int s, double sign, double threshold)
{
    const size_t xo = (size_t)M, so = (size_t)M * N;
    const double *pt = D + y + x * xo + s * so;
    const double v = sign * *pt;
    if (!(v >= threshold)) return false;
    for (int ds = -1; ds <= 1; ++ds)
        for (int dx = -1; dx <= 1; ++dx)
            for (int dy = -1; dy <= 1; ++dy) {
                if (ds == 0 && dx == 0 && dy == 0) continue;
                if (!(v > sign * pt[(ptrdiff_t)dy + (ptrdiff_t)dx * (ptrdiff_t)xo + (ptrdiff_t)ds * (ptrdiff_t)so])) return false;
            }
    return true;
}

// sift_vedal.m:259-264: x, y 0-based, p2 = 2^(s / S) from the plan
PRE3_HD bool sift_inside(double x, double y, double p2, double sigma0, int M, int N)
{
#pragma clang fp contract(off)
    double rad = SIFT_MAGNIF * sigma0;
    rad = rad * p2;
    rad = rad * SIFT_NBP;
    rad = rad / 2;
    return x - rad >= 1 && x + rad <= (double)N && y - rad >= 1 && y + rad <= (double)M;
}

// siftrefinemx.c:150-303 for one point: x, y, s are the integer coordinates of an extremum, s counted from the first DoG level.  true: accepted,
// out = (xn, yn, sn + smin)
PRE3_HD bool sift_refine(const double *D, int M, int N, int x, int y, int s, double threshold, double r, double out[3])
{
#pragma clang fp contract(off)
    const int S = SIFT_NDOG;
    if (x < 1 || x > N - 2 || y < 1 || y > M - 2 || s < 1 || s > S - 2) return false;
    const ptrdiff_t xo = M, so = (ptrdiff_t)M * N;
    const double *pt = D + y + x * xo + s * so;
#define PRE3_AT(dx, dy, ds) (pt[(dx) * xo + (dy) + (ds) * so])
    double Dx = 0, Dy = 0, Ds = 0, Dxx = 0, Dyy = 0, Dss = 0, Dxy = 0, Dxs = 0, Dys = 0;
    double b[3] = {0, 0, 0};
    int dx = 0, dy = 0;
    for (int iter = 0; iter < 5; ++iter) {
        double A[9];
#define PRE3_A(i, j) (A[(i) + (j) * 3])
        x += dx; y += dy;
        pt = D + y + x * xo + s * so;
        Dx = 0.5 * (PRE3_AT(+1, 0, 0) - PRE3_AT(-1, 0, 0));
        Dy = 0.5 * (PRE3_AT(0, +1, 0) - PRE3_AT(0, -1, 0));
        Ds = 0.5 * (PRE3_AT(0, 0, +1) - PRE3_AT(0, 0, -1));
        Dxx = (PRE3_AT(+1, 0, 0) + PRE3_AT(-1, 0, 0) - 2.0 * PRE3_AT(0, 0, 0));
        Dyy = (PRE3_AT(0, +1, 0) + PRE3_AT(0, -1, 0) - 2.0 * PRE3_AT(0, 0, 0));
        Dss = (PRE3_AT(0, 0, +1) + PRE3_AT(0, 0, -1) - 2.0 * PRE3_AT(0, 0, 0));
        Dxy = 0.25 * (PRE3_AT(+1, +1, 0) + PRE3_AT(-1, -1, 0) - PRE3_AT(-1, +1, 0) - PRE3_AT(+1, -1, 0));
        Dxs = 0.25 * (PRE3_AT(+1, 0, +1) + PRE3_AT(-1, 0, -1) - PRE3_AT(-1, 0, +1) - PRE3_AT(+1, 0, -1));
        Dys = 0.25 * (PRE3_AT(0, +1, +1) + PRE3_AT(0, -1, -1) - PRE3_AT(0, -1, +1) - PRE3_AT(0, +1, -1));
        PRE3_A(0, 0) = Dxx; PRE3_A(1, 1) = Dyy; PRE3_A(2, 2) = Dss;
        PRE3_A(0, 1) = PRE3_A(1, 0) = Dxy;
        PRE3_A(0, 2) = PRE3_A(2, 0) = Dxs;
        PRE3_A(1, 2) = PRE3_A(2, 1) = Dys;
        b[0] = -Dx; b[1] = -Dy; b[2] = -Ds;
        for (int j = 0; j < 3; ++j) {                       // Gauss elimination, :214-257
            double maxa = 0, maxabsa = 0, tmp;
            int maxi = -1;
            for (int i = j; i < 3; ++i) {
                const double a = PRE3_A(i, j), absa = a > 0 ? a : -a;      // the abs macro of :66
                if (absa > maxabsa) { maxa = a; maxabsa = absa; maxi = i; }
            }
            if (maxabsa < (double)1e-10f) { b[0] = 0; b[1] = 0; b[2] = 0; break; }      // :232: a float literal compared in double
            const int i = maxi;
            for (int jj = j; jj < 3; ++jj) {
                tmp = PRE3_A(i, jj); PRE3_A(i, jj) = PRE3_A(j, jj); PRE3_A(j, jj) = tmp;
                PRE3_A(j, jj) = PRE3_A(j, jj) / maxa;
            }
            tmp = b[j]; b[j] = b[i]; b[i] = tmp;
            b[j] = b[j] / maxa;
            for (int ii = j + 1; ii < 3; ++ii) {
                const double xx = PRE3_A(ii, j);
                for (int jj = j; jj < 3; ++jj) { const double t = xx * PRE3_A(j, jj); PRE3_A(ii, jj) = PRE3_A(ii, jj) - t; }
                const double t = xx * b[j];
                b[ii] = b[ii] - t;
            }
        }
        for (int i = 2; i > 0; --i) {                       // backward substitution, :260-265
            const double xx = b[i];
            for (int ii = i - 1; ii >= 0; --ii) { const double t = xx * PRE3_A(ii, i); b[ii] = b[ii] - t; }
        }
        dx = ((b[0] > 0.6 && x < N - 2) ? 1 : 0) + ((b[0] < -0.6 && x > 1) ? -1 : 0);
        dy = ((b[1] > 0.6 && y < M - 2) ? 1 : 0) + ((b[1] < -0.6 && y > 1) ? -1 : 0);
        if (dx == 0 && dy == 0) break;
    }
    double t0 = Dx * b[0], t1 = Dy * b[1], t2 = Ds * b[2];
    t0 = t0 + t1;
    t0 = t0 + t2;
    t0 = 0.5 * t0;
    const double val = PRE3_AT(0, 0, 0) + t0;
    const double tr = Dxx + Dyy, tr2 = tr * tr, d0 = Dxx * Dyy, d1 = Dxy * Dxy, det = d0 - d1;
    const double score = tr2 / det;
    const double r1 = r + 1, lim = r1 * r1 / r;
    const double xn = x + b[0], yn = y + b[1], sn = s + b[2];
#undef PRE3_A
#undef PRE3_AT
    if (fabs(val) > threshold && score < lim && score >= 0 && fabs(b[0]) < 1.5 && fabs(b[1]) < 1.5 && fabs(b[2]) < 1.5 && xn >= 0 && xn <= N - 1 &&
        yn >= 0 && yn <= M - 1 && sn >= 0 && sn <= S - 1) {
        out[0] = xn; out[1] = yn; out[2] = sn + SIFT_SMIN;
        return true;
    }
    return false;
}

// ---- orientation (siftormx.c:138-253), double throughout ----
struct SiftOrientSetup { double x, y, sigmaw; int xi, yi, si, W; bool ok; };

// :139-162 for one refined point of an M x N octave
PRE3_HD SiftOrientSetup sift_orient_setup(double x, double y, double s, double sigma0, int M, int N)
{
#pragma clang fp contract(off)
    SiftOrientSetup a;
    a.x = x; a.y = y;
    a.xi = (int)(x + 0.5); a.yi = (int)(y + 0.5); a.si = (int)(s + 0.5) - SIFT_SMIN;
    double sw = 1.5 * sigma0;
    a.sigmaw = sw * pow(2.0, s / SIFT_S);
    a.W = (int)floor(3.0 * a.sigmaw);
    a.ok = !(a.xi < 0 || a.xi > N - 1 || a.yi < 0 || a.yi > M - 1 || a.si < 0 || a.si > SIFT_NLEV - 1);
    return a;
}

// :177-189 for the sample at offset (xs, ys) on the level plane L: false when it lies outside the window; else the bin and the amount added to it.
// (The reference indexes H_pt[36] when 36 theta / 2 pi rounds up to 36; that sample goes to bin 35 here.)
PRE3_HD bool sift_orient_sample(const double *L, int M, const SiftOrientSetup &a, int xs, int ys, int *bin, double *amount)
{
#pragma clang fp contract(off)
    const double *pt = L + a.yi + (ptrdiff_t)a.xi * M;
    const ptrdiff_t o = (ptrdiff_t)xs * M + ys;
    const double Dx = 0.5 * (pt[o + M] - pt[o - M]), Dy = 0.5 * (pt[o + 1] - pt[o - 1]);
    const double dx = (double)(a.xi + xs) - a.x, dy = (double)(a.yi + ys) - a.y;
    const double dx2 = dx * dx, dy2 = dy * dy, r2 = dx2 + dy2;
    if (r2 >= a.W * a.W + 0.5) return false;
    double den = 2 * a.sigmaw;
    den = den * a.sigmaw;
    const double win = exp(-r2 / den);
    const double gx = Dx * Dx, gy = Dy * Dy;
    const double mod = sqrt(gx + gy);
    const double theta = fmod(atan2(Dy, Dx) + SIFT_2PI, SIFT_2PI);
    double q = SIFT_NBINS * theta;
    q = q / SIFT_2PI;
    int bi = (int)q;
    *bin = bi > SIFT_NBINS - 1 ? SIFT_NBINS - 1 : (bi < 0 ? 0 : bi);
    *amount = mod * win;
    return true;
}

// :195-253: six passes of the circular 3-tap smoother (the non-LOWE_BUG form), then every peak above 0.8 max with its parabolic offset, in bin
// order.  Returns the number of peaks (<= SIFT_MAX_PEAKS)
PRE3_HD int sift_orient_peaks(double H[SIFT_NBINS], double th[SIFT_MAX_PEAKS])
{
#pragma clang fp contract(off)
    for (int iter = 0; iter < 6; ++iter) {
        double prev = H[SIFT_NBINS - 1];
        for (int i = 0; i < SIFT_NBINS; ++i) {
            double nh = prev + H[i];
            nh = nh + H[(i + 1) % SIFT_NBINS];
            nh = nh / 3.0;
            prev = H[i];
            H[i] = nh;
        }
    }
    double maxh = H[0];
    for (int i = 1; i < SIFT_NBINS; ++i) maxh = maxh > H[i] ? maxh : H[i];
    int n = 0;
    for (int i = 0; i < SIFT_NBINS; ++i) {
        const double h0 = H[i], hm = H[(i - 1 + SIFT_NBINS) % SIFT_NBINS], hp = H[(i + 1 + SIFT_NBINS) % SIFT_NBINS];
        if (h0 > 0.8 * maxh && h0 > hm && h0 > hp) {
            double num = -0.5 * (hp - hm), den = hp + hm;
            den = den - 2 * h0;
            const double di = num / den;
            double t = i + di;
            t = t + 0.5;
            t = SIFT_2PI * t;
            if (n < SIFT_MAX_PEAKS) th[n++] = t / SIFT_NBINS;
        }
    }
    return n;
}

// sift_vedal.m:296-298: the frame of a point of octave o (0-based: 2^(o + omin)), x and y 0-based
PRE3_HD void sift_frame(int o, double sigma0, double x, double y, double s, double theta, double frm[4])
{
#pragma clang fp contract(off)
    const double sc = ldexp(1.0, o + SIFT_OMIN);
    frm[0] = sc * x; frm[1] = sc * y;
    double sg = sc * sigma0;
    frm[2] = sg * pow(2.0, s / SIFT_S);
    frm[3] = theta;
}

// ---- descriptor (siftdescriptor.c:381-513), float throughout ----
PRE3_HD float sift_fast_mod(float th)                       // :110-115
{
    while (th < 0) th = (float)((double)th + SIFT_2PI);
    while ((double)th > SIFT_2PI) th = (float)((double)th - SIFT_2PI);
    return th;
}
PRE3_HD int sift_fast_floor(float x) { return (int)(x - (float)((x >= 0) ? 0 : 1)); }      // :120-123

struct SiftDescSetup { float x, y, theta0, st0, ct0, SBP; int xi, yi, si, W; bool ok; };

// :396-424 for one oriented point of an M x N octave
PRE3_HD SiftDescSetup sift_desc_setup(double px, double py, double ps, double pth, double sigma0d, int M, int N)
{
#pragma clang fp contract(off)
    SiftDescSetup a;
    a.x = (float)px; a.y = (float)py;
    const float s = (float)ps;
    a.theta0 = (float)pth;
    a.st0 = sinf(a.theta0); a.ct0 = cosf(a.theta0);
    a.xi = (int)floor((double)a.x + 0.5); a.yi = (int)floor((double)a.y + 0.5); a.si = (int)floor((double)s + 0.5) - SIFT_SMIN;
    const float sigma = (float)sigma0d * powf(2.0f, s / (float)SIFT_S);
    a.SBP = (float)SIFT_MAGNIF * sigma;
    a.W = (int)floor(sqrt(2.0) * (double)a.SBP * (SIFT_NBP + 1) / 2.0 + 0.5);
    a.ok = !(a.xi < 0 || a.xi > N - 1 || a.yi < 0 || a.yi > M - 1 || a.si < 0 || a.si > SIFT_NLEV - 1);
    return a;
}

// :314-315, :346-352 for the pixel at `pt` of a level plane: the float gradient modulus and angle
PRE3_HD void sift_gradient(const double *pt, int M, float *mod, float *angle)
{
#pragma clang fp contract(off)
    const float Dx = (float)(0.5 * (pt[M] - pt[-M])), Dy = (float)(0.5 * (pt[1] - pt[-1]));
    const float a = Dx * Dx, b = Dy * Dy;
    *mod = sqrtf(a + b);
    *angle = *mod > 0 ? atan2f(Dy, Dx) : 0.0f;
}

// :442-496 for the sample at offset (dxi, dyi): up to eight (bin, weight) pairs, bin = t + NBO * (x + NBP * y) of Lowe's layout.  Returns their number
PRE3_HD int sift_desc_sample(const SiftDescSetup &a, float mod, float angle, int dxi, int dyi, int bins[8], float weights[8])
{
#pragma clang fp contract(off)
    const float theta = sift_fast_mod(-angle + a.theta0);
    const float dx = (float)(a.xi + dxi) - a.x, dy = (float)(a.yi + dyi) - a.y;
    float p0 = a.ct0 * dx, p1 = a.st0 * dy;
    const float nx = (p0 + p1) / a.SBP;
    p0 = -a.st0 * dx; p1 = a.ct0 * dy;
    const float ny = (p0 + p1) / a.SBP;
    const float nt = (float)((double)((float)SIFT_NBO * theta) / SIFT_2PI);
    const float wsigma = SIFT_NBP / 2;
    const float nx2 = nx * nx, ny2 = ny * ny;
    const float win = expf((float)((double)(-(nx2 + ny2)) / (2.0 * wsigma * wsigma)));
    const int binx = sift_fast_floor((float)((double)nx - 0.5)), biny = sift_fast_floor((float)((double)ny - 0.5)), bint = sift_fast_floor(nt);
    const float rbinx = (float)((double)nx - (binx + 0.5)), rbiny = (float)((double)ny - (biny + 0.5)), rbint = nt - (float)bint;
    int n = 0;
    for (int dbx = 0; dbx < 2; ++dbx)
        for (int dby = 0; dby < 2; ++dby)
            for (int dbt = 0; dbt < 2; ++dbt)
                if (binx + dbx >= -(SIFT_NBP / 2) && binx + dbx < (SIFT_NBP / 2) && biny + dby >= -(SIFT_NBP / 2) && biny + dby < (SIFT_NBP / 2)) {
                    float w = win * mod;
                    w = w * fabsf((float)(1 - dbx) - rbinx);
                    w = w * fabsf((float)(1 - dby) - rbiny);
                    w = w * fabsf((float)(1 - dbt) - rbint);
                    bins[n] = (((bint + dbt) % SIFT_NBO) + SIFT_NBO) % SIFT_NBO + SIFT_NBO * ((binx + dbx + SIFT_NBP / 2) + SIFT_NBP * (biny + dby + SIFT_NBP / 2));
                    weights[n] = w;
                    ++n;
                }
    return n;
}

// :128-141, :501-512: normalise with + FLT_EPSILON, clip at 0.2, normalise again; in place, by one thread
PRE3_HD void sift_desc_finish(float d[128])
{
#pragma clang fp contract(off)
    for (int pass = 0; pass < 2; ++pass) {
        float norm = 0.0f;
        for (int i = 0; i < 128; ++i) { const float t = d[i] * d[i]; norm = norm + t; }
        norm = sqrtf(norm);
        const float den = norm + FLT_EPSILON;
        for (int i = 0; i < 128; ++i) d[i] = d[i] / den;
        if (pass == 0)
            for (int i = 0; i < 128; ++i) if ((double)d[i] > 0.2) d[i] = (float)0.2;
    }
}

// the test copy_desc_checked makes on the host (pre3_api.hip): true when v is outside the ranked IC route's bounds
PRE3_HD bool sift_desc_out_of_bounds(double v)
{
    const double a = fabs(v);
    return !(a <= 1152921504606846976.0) || (a != 0.0 && a < 9.094947017729282e-13);      // 2^60, 2^-40
}

}  // namespace pre3
