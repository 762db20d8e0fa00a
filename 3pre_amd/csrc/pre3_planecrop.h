// pre3_planecrop.h -- the index arithmetic of the crop that feeds the floor-plane fit from a resident frame (k_plane_crop in pre3_plane.hip; DESIGN.md
// section 23), as functions that compile for the device and for the host.
//   plane_fit_to_data.m:13, :19-21, :41      (camera coordinates x = -x_sr, y = -y_sr, z = z_sr; the box; the column-major point list)
// tests/test_frame_consumers_ref.py builds this header with the host compiler and compares it with a numpy restatement of plane_pack.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <math.h>

#ifndef PRE3_HD
#if defined(__HIPCC__)
#define PRE3_HD __host__ __device__ inline
#else
#define PRE3_HD inline
#endif
#endif

namespace pre3 {

struct PlaneCrop { int rows, r0, c0, nr, nc; };      // the planes' row count (they are column-major); the box's first row and column, 0-based; its size

// point k of the box, 0 <= k < nr * nc, counted column-major inside the box: its offset in a plane.  Adjacent k are adjacent rows of one column, so
// adjacent lanes read adjacent doubles.
PRE3_HD size_t plane_crop_src(const PlaneCrop &b, int k)
{
    const int c = k / b.nr, r = k - c * b.nr;
    return (size_t)(b.c0 + c) * (size_t)b.rows + (size_t)(b.r0 + r);
}

// finite: neither NaN nor an infinity (a comparison, so that host and device agree whatever their isfinite is)
PRE3_HD bool plane_crop_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

// point k into the fit's point block [X | Y | Z] of npts = nr * nc entries each (plane_pack's layout): X = -x, Y = -y, Z = z.
// Returns true when any of the three values is not finite.
PRE3_HD bool plane_crop_point(const PlaneCrop &b, int k, const double *x, const double *y, const double *z, double *pts)
{
    const size_t npts = (size_t)b.nr * (size_t)b.nc, g = plane_crop_src(b, k);
    const double xv = x[g], yv = y[g], zv = z[g];
    pts[k] = -xv; pts[npts + k] = -yv; pts[2 * npts + k] = zv;
    return !(plane_crop_finite(xv) && plane_crop_finite(yv) && plane_crop_finite(zv));
}

}  // namespace pre3
