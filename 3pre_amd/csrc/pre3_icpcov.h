// pre3_icpcov.h -- the closed-form covariance of the dense ICP's refined increment u = [T; q] over its final correspondences (pre3_icpcov.hip; DESIGN.md
// section 34): pre3_vocov.h's implicit-function covariance H^-1 M H^-1 of a rigid fit over point pairs (aux_code/d2E_*_4cov.m, dE_*_4cov.m,
// Calc_derivatives_for_covariance.m over aux_code/cov_pose_shift_calc.m:24-40), applied to the pairs TestScripts/icp_with_init.m:76-89 ends with.
// f_p is the model point, f_n the ORIGINAL source point (before Rinit / Tinit and before any registration step): r = T + R(q) f_n - f_p, as
// data1 ~ Rtot data2 + ttot.  The estimate propagates the sensor's range and angle noise only; it says nothing about the error two independent samplings
// of one surface leave (DESIGN.md section 34 has the figures), so it is optimistic as a process noise -- see PRE3_NOISE_ICP_FLOOR (pre3_predicticp.h).
// The constants and the status rule are __host__ __device__, so that a host program can restate the tree of partial sums (tests/icp_cov_host_main.cpp).
#pragma once
#include <stdint.h>

#include "pre3_vocov.h"

namespace pre3 {

constexpr int IC_PAIRS = 256;                       // pairs per workgroup of k_icp_cov_part, one per thread
constexpr int IC_FIN_THREADS = 256;                 // k_icp_cov_fin's one workgroup
constexpr int IC_FIN_PER_THREAD = 4;                // partials a thread of the finisher sums at the largest supported p
constexpr int IC_MAX_P = IC_PAIRS * IC_FIN_THREADS * IC_FIN_PER_THREAD;      // 262144 pairs (two 144 x 176 frames give at most 25344)

// what one workgroup of k_icp_cov_part leaves: the packed lower triangles of its pairs' H and M, their count, and whether one had a non-finite coordinate
struct IcPart { double H[28], M[28]; int32_t n, nonfinite; };

PRE3_VC_HD constexpr int ic_parts(int p) { return (p + IC_PAIRS - 1) / IC_PAIRS; }
// a covariance is computed: the run ended by the reference's rule (ICP_OK), with at least four pairs, and the list fits the layout it was sized for
PRE3_VC_HD bool ic_computes(int icp_sta, int p, int cap) { return icp_sta == 1 && p >= 4 && p <= cap; }

}  // namespace pre3

#if defined(__HIPCC__)
#include "pre3_internal.h"
#include "pre3_geomdev.h"
#include "pre3_icp.h"
namespace pre3 {
// where the two launches read their operands.  The run's state and u: the state block and the u k_icp_final left on the device (ctl != nullptr), or
// the host's (sta = 1, p, u by value).  The pairs: 0-based (model, source) indices.  The model: three planes of cap1 points.  The source: three planes
// indexed by the pair's source index (spix == nullptr), or -- the frames forms -- a frame's filtered planes read at spix[source index] as [-x; -y; z].
struct IcCovArgs {
    const IcpCtl *ctl; const double *u_dev; int p; U7 u;
    int cap;                                        // pairs the layout holds: corr_m, corr_s and the partials are sized for it
    int cap1, cap2, npix;                           // points of the model planes, entries of spix (or of the source planes), pixels of a frame plane
    const int32_t *corr_m, *corr_s;
    const double *mx, *my, *mz, *sx, *sy, *sz;
    const int32_t *spix;
};
inline size_t ic_part_bytes(int cap) { return sizeof(IcPart) * (size_t)ic_parts(cap); }
// k_icp_cov_part over ceil(cap / 256) workgroups, then k_icp_cov_fin; both on st, no wait.  part holds ic_parts(cap) entries.
int launch_icp_cov(const IcCovArgs &a, IcPart *part, VoCov *cov, hipStream_t st);
}  // namespace pre3
#endif
