// pre3_sr.h -- the arithmetic of the SR4000 frame conditioning (pre3_sr.hip), as functions that compile for the device and for
// the host: MATLAB's round and uint8, the 3 x 3 Gaussian of fspecial, the nine-tap sum of imfilter, the amplitude normalisation, the two keypoint gates.
//   read_xyz_sr4000.m:8-21, read_image_sr4000.m:3,10-24, normalzie_image.m:4           (sigma = 2, zero padding)
//   code_from_dr_ye/read_sr4000_data_dr_ye.m:8,11-21,42,70,88-90                       (sigma = 1, replicated border)
//   inittialize_depth_my_version.m:16,40-45,74-92, code_from_dr_ye/confidence_filtering.m:6-8
//   aux_code/compensate_badpixel_soonhac.m:5-14, code_from_dr_ye/read_image_sr4000_dr_ye.m:21-24   (the 3 x 3 median in front of the Gaussian; section 32)
// Every statement a test pins bit for bit is compiled without contraction: one product or one sum per rounding, as numpy rounds them
// (tests/sr_frame_ref.py).  tests/test_sr_frame_ref.py builds this header with the host compiler and compares it with that restatement.
#pragma once
#include <stdint.h>
#include <math.h>

#ifndef PRE3_HD
#if defined(__HIPCC__)
#define PRE3_HD __host__ __device__ inline
#else
#define PRE3_HD inline
#endif
#endif

namespace pre3 {

constexpr double SR_SATURATED = 65000.0;    // read_image_sr4000.m:12: amplitudes above it are replaced by the frame's largest unsaturated one
constexpr double SR_MIN_RANGE = 0.4;        // inittialize_depth_my_version.m:74
constexpr double SR_CONF_FRACTION = 0.5;    // :74 (2/4), confidence_filtering.m:3

// MATLAB's round: to the nearest integer, halves away from zero (C's round; exact, also at 0.49999999999999994); NaN stays NaN
PRE3_HD double matlab_round(double v) { return round(v); }

// MATLAB's uint8(g) as a double in 0 .. 255: rounded half away from zero, saturated, NaN -> 0 (never -0)
PRE3_HD double matlab_uint8(double g)
{
    const double r = round(g);
    if (!(r > 0.0)) return 0.0;
    return r > 255.0 ? 255.0 : r;
}

// fspecial('gaussian', [3 3], sigma): h(i, j) = exp(-(i^2 + j^2) / (2 sigma^2)), i, j in {-1, 0, 1}, over the sum of the nine values taken
// column-major, one after the other.  w[3 (j + 1) + (i + 1)].  (No entry falls under eps * max: that branch of fspecial never fires.)
inline void sr_gauss3(double sigma, double w[9])
{
    const double d = 2.0 * sigma * sigma;
    double s = 0.0;
    for (int j = -1; j <= 1; ++j)
        for (int i = -1; i <= 1; ++i) { const double h = exp(-(double)(i * i + j * j) / d); w[3 * (j + 1) + (i + 1)] = h; s = s + h; }
    for (int k = 0; k < 9; ++k) w[k] = w[k] / s;
}

// imfilter's sum over the 3 x 3 neighbourhood p (column-major: dj = -1, 0, 1 outer, di = -1, 0, 1 inner): every tap is added, the padding included,
// so a NaN anywhere in the neighbourhood makes the pixel NaN and signed zeros come out as numpy's
PRE3_HD double sr_tap9(const double w[9], const double p[9])
{
#pragma clang fp contract(off)
    double acc = w[0] * p[0];
    for (int k = 1; k < 9; ++k) { const double t = w[k] * p[k]; acc = acc + t; }
    return acc;
}

// read_image_sr4000.m:12-21 + normalzie_image.m:4 for one pixel: uint8(sqrt(v) / sqrt(imax) * 255), v = imax where the amplitude is saturated.
// imax == 0 (every pixel saturated, or a black frame): 0 / 0 = NaN -> 0
PRE3_HD double sr_norm_pixel(double amp, double imax)
{
#pragma clang fp contract(off)
    const double v = amp > SR_SATURATED ? imax : amp;
    double g = sqrt(v) / sqrt(imax);
    g = g * 255.0;
    return matlab_uint8(g);
}

// inittialize_depth_my_version.m:45: df = sqrt(xf^2 + yf^2 + zf^2), summed left to right
PRE3_HD double sr_range(double xf, double yf, double zf)
{
#pragma clang fp contract(off)
    const double a = xf * xf, b = yf * yf, c = zf * zf;
    double s = a + b;
    s = s + c;
    return sqrt(s);
}

// gate 0 (inittialize_depth_my_version.m:40, :74): kept unless x is NaN, the range is below 0.4 m, or -- with a confidence map -- the pixel's
// confidence is <= half the frame's largest.  Comparisons with NaN are false: a NaN y or z survives with NaN coordinates, as in the reference.
PRE3_HD bool sr_gate_depth(double xf, double df, bool has_conf, double conf, double cmax)
{
#pragma clang fp contract(off)
    if (xf != xf) return false;
    if (df < SR_MIN_RANGE) return false;
    if (has_conf) { const double thr = SR_CONF_FRACTION * cmax; if (conf <= thr) return false; }
    return true;
}

// gate 1 (confidence_filtering.m:8): dropped when the confidence is < half the largest (strictly: a pixel exactly at the threshold is kept)
PRE3_HD bool sr_gate_confidence(double conf, double cmax)
{
#pragma clang fp contract(off)
    const double thr = SR_CONF_FRACTION * cmax;
    return !(conf < thr);
}

// MATLAB's max over a set with NaNs: NaNs are skipped, the result is NaN only when every entry is NaN
PRE3_HD double sr_nanmax(double a, double b) { return a != a ? b : (b != b ? a : (b > a ? b : a)); }

// ---- the bad-pixel compensation: aux_code/compensate_badpixel_soonhac.m:5-14, code_from_dr_ye/read_image_sr4000_dr_ye.m:21-24
constexpr int SR_COMP_NONE = 0, SR_COMP_BADPIXEL = 1, SR_COMP_IMAGE_MEDIAN = 2;      // PRE3_SR_COMP_*
constexpr int SR_PAD_ZEROS = 0, SR_PAD_SYMMETRIC = 1;                                // medfilt2's default, and its 'symmetric'

// one compare-exchange: afterwards a <= b.  Two selects on one comparison, no branch
PRE3_HD void sr_cswap(double &a, double &b)
{
    const bool s = b < a;
    const double lo = s ? b : a, hi = s ? a : b;
    a = lo; b = hi;
}

// medfilt2(.., [3 3]) for one pixel: the fifth smallest of the nine window values.  A fixed network of 19 compare-exchanges (Paeth's median of nine:
// three sorted columns, the largest of the lows, the median of the middles, the smallest of the highs, and the median of those three); the same 19
// whatever the data.  Our rule for NaN (medfilt2 documents none; MATLAB's median returns NaN): a NaN anywhere in the window makes the result NaN.
// The result is a value: where the window holds -0 and +0 and the median is zero, its sign is not specified.
PRE3_HD double sr_median9(const double p[9])
{
    double a = p[0], b = p[1], c = p[2], d = p[3], e = p[4], f = p[5], g = p[6], h = p[7], i = p[8];
    bool nan = false;
    for (int k = 0; k < 9; ++k) nan = nan | (p[k] != p[k]);
    sr_cswap(b, c); sr_cswap(e, f); sr_cswap(h, i);
    sr_cswap(a, b); sr_cswap(d, e); sr_cswap(g, h);
    sr_cswap(b, c); sr_cswap(e, f); sr_cswap(h, i);
    sr_cswap(a, d); sr_cswap(f, i); sr_cswap(e, h);
    sr_cswap(d, g); sr_cswap(b, e); sr_cswap(c, f);
    sr_cswap(e, h); sr_cswap(e, c); sr_cswap(g, e);
    sr_cswap(e, c);
    return nan ? (double)NAN : e;
}

// the window's index rule one step outside 0 .. n - 1, 'symmetric': -1 reads 0 and n reads n - 1 (a 1-row or 1-column image mirrors onto itself).
// The window is 3 wide, so no index lies further out; one step out, MATLAB's mirror and a clamp are the same pixel.
PRE3_HD int sr_sym_index(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// the 3 x 3 window of the column-major plane P around (r, c), taps column-major (dj outer, di inner): SR_PAD_SYMMETRIC mirrors at the edge,
// SR_PAD_ZEROS reads 0.0 outside
PRE3_HD void sr_window9(const double *P, int rows, int cols, int r, int c, int padding, double p[9])
{
    for (int dj = -1; dj <= 1; ++dj)
        for (int di = -1; di <= 1; ++di) {
            const int gr = r + di, gc = c + dj;
            const bool inside = gr >= 0 && gr < rows && gc >= 0 && gc < cols;
            double v = 0.0;
            if (inside || padding == SR_PAD_SYMMETRIC) v = P[(size_t)sr_sym_index(gc, cols) * rows + sr_sym_index(gr, rows)];
            p[3 * (dj + 1) + (di + 1)] = v;
        }
}

PRE3_HD double sr_medfilt_pixel(const double *P, int rows, int cols, int r, int c, int padding)
{
    double p[9];
    sr_window9(P, rows, cols, r, c, padding, p);
    return sr_median9(p);
}

// compensate_badpixel_soonhac.m:6: c < confidence_cut_off, strictly; a NaN confidence compares false and is not bad; a frame without a confidence map
// has no bad pixel (the reference's call sits inside `if size(sr_data, 1) >= 720`)
PRE3_HD bool sr_is_bad(bool has_conf, double conf, double cutoff) { return has_conf && conf < cutoff; }

// the value the mode's Gaussian reads at the pixel (r, c) INSIDE the image, for the plane P (x, y, z as loaded, or the normalised uint8 image U):
//   SR_COMP_BADPIXEL      bad(r, c) ? the symmetric median of P around it : P(r, c)      -- every median on the plane as loaded
//   SR_COMP_IMAGE_MEDIAN  the zero-padded median of P around it, at every pixel            -- the caller passes U only; x, y, z stay as loaded
PRE3_HD double sr_comp_pixel(const double *P, const double *conf /* null: none */, int rows, int cols, int r, int c, int form, double cutoff)
{
    const size_t g = (size_t)c * rows + r;
    if (form == SR_COMP_IMAGE_MEDIAN) return sr_medfilt_pixel(P, rows, cols, r, c, SR_PAD_ZEROS);
    if (form == SR_COMP_BADPIXEL && sr_is_bad(conf != nullptr, conf != nullptr ? conf[g] : 0.0, cutoff)) return sr_medfilt_pixel(P, rows, cols, r, c, SR_PAD_SYMMETRIC);
    return P[g];
}

}  // namespace pre3
