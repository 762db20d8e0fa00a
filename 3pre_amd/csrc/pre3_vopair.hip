// pre3_vopair.hip -- the VO front end between the keypoint sets two resident SR4000 frames hold, in one call (pre3_vo_pair_seeded).
//   vodometry_dr_ye.m:139-236  (siftmatch on the filtered keypoint sets, pnum < 4, rst, the RANSAC and its statistics)
//   sift/siftmatch.c:97-122    (every pair's bins in order, first index on ties, the ratio test in float)
//   ransac_dr_ye.m:13-72, find_transform_matrix_dr_ye.m:8-41, Calculate_V_Omega_RANSAC_dr_ye.m:41-50 (pre3_vodev.h)
// Eight launches on cur's stream, every hand-off a launch boundary; no workgroup waits on another.  The host knows n1 and n2 (the kept keypoints of the
// two frames) and sizes buffers and grids by the caps pnum <= n1 and rst <= 700; the real pnum and rst are written by k_vp_pairs into a device header
// (VoPairHeader) that every launch behind it reads: work items beyond them leave at once.
//   k_vp_match   ic_match_tile (pre3_geomdev.h): 32 x 32 pairs per workgroup, prev's kept descriptors the queries, cur's the scan; partial
//                (best, second, first index) per (column tile, query)
//   k_vp_pairs   ONE workgroup: the column tiles merged in scan order (merge3), siftmatch.c:122 in float, the accepted pairs compacted in increasing k1 by
//                ballot prefix into match (2 x pnum doubles, 1-based); then pnum and rst into the header
//   k_vp_gather  vo_gather_one for both frames (blockIdx.y), the bad flags into the header
//   k_vp_dist, k_vp_draw, k_vp_score, k_vp_final    the bodies of k_vo_dist, k_draw_vo, k_vo_score, k_vo_final with pnum / rst from the header
// Every output slot has one writer (the capped count is an integer sum): results are bit-equal from run to run, and bit-equal to
// pre3_vo_ransac_frames_seeded fed the same match list with n_hyp = rst.
// pre3_predict_pair_seeded queues the same eight launches through the same host path (vp_queue) and puts the prediction behind
// them on the context's stream: k_predict reads u from the VoOut block k_vp_final wrote, so the increment never reaches the host.
// pre3_vo_pair_pnp_seeded queues two more launches behind the eight (launch_pnp_pair, pre3_pnp.hip): the EPnP refit over the pair's
// inliers, prev's range points against cur's pixels; its pixels and result ride in the same transfer.
#include <cmath>

#include "pre3_internal.h"
#include "pre3_geomdev.h"
#include "pre3_vodev.h"
#include "pre3_vopair.h"
#include "pre3_predictu.h"
#include "pre3_vocov.h"
#include "pre3_icp.h"
#include "pre3_predicticp.h"
#include "pre3_pnp.h"

namespace pre3 {

namespace {

constexpr int VP_NTH = 1024;                  // threads of k_vp_pairs' one workgroup
constexpr int VP_NW = VP_NTH / 64;

__global__ __launch_bounds__(256) void k_vp_match(IcMatchRide r)
{
    __shared__ double Qs[ICS_T][ICS_LD], Bs[ICS_T][ICS_LD];
    ic_match_tile(r, blockIdx.x, Qs, Bs);
}

__global__ __launch_bounds__(VP_NTH) void k_vp_pairs(int n1, int ntn, float thresh, const double *__restrict__ pb, const double *__restrict__ ps,
                                                     const int32_t *__restrict__ pa, double *__restrict__ match, VoPairHeader *__restrict__ hdr)
{
    __shared__ int s_cnt[VP_NW];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int base = 0;
    for (int q0 = 0; q0 < n1; q0 += VP_NTH) {
        const int k1 = q0 + tid;
        int ok = 0, k2 = -1;
        if (k1 < n1) {
            double best = acc_max<double>(), second = acc_max<double>();
            for (int t = 0; t < ntn; ++t) {                                // scan order: ties keep the first index (siftmatch.c:110)
                const size_t o = (size_t)t * n1 + k1;
                merge3(best, second, k2, pb[o], ps[o], pa[o]);
            }
            ok = k2 >= 0 && thresh * (float)best <= (float)second;        // siftmatch.c:122; one scan keypoint: second stays at the accumulator's maximum
        }
        const unsigned long long b = __ballot(ok);
        if (lane == 0) s_cnt[wv] = __popcll(b);
        __syncthreads();
        int off = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < VP_NW; ++w) { const int cw = s_cnt[w]; if (w < wv) off += cw; tot += cw; }
        if (ok) {
            const int c = base + off + __popcll(b & ((1ull << lane) - 1ull));      // c <= k1 < n1: inside match
            match[2 * (size_t)c] = (double)(k1 + 1); match[2 * (size_t)c + 1] = (double)(k2 + 1);
        }
        base += tot;
        __syncthreads();                                                    // (s_cnt is rewritten by the next pass)
    }
    if (tid == 0) { hdr->pnum = base; hdr->rst = vo_rst(base); hdr->bad = 0; hdr->capped = 0; }
}

struct VpFrame { const double *x, *y, *z, *frm; int ldf, K; };

__global__ __launch_bounds__(64) void k_vp_gather(int rows, int cols, VpFrame f1, VpFrame f2, const double *__restrict__ match, double *__restrict__ pset1,
                                                  double *__restrict__ pset2, VoPairHeader *__restrict__ hdr)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= hdr->pnum) return;
    const VpFrame &f = blockIdx.y == 0 ? f1 : f2;
    vo_gather_one(i, rows, cols, f.x, f.y, f.z, f.ldf, f.frm, f.K, match + blockIdx.y, 2, blockIdx.y == 0 ? pset1 : pset2, &hdr->bad);
}

__global__ __launch_bounds__(64) void k_vp_dist(const VoPairHeader *__restrict__ hdr, const double *__restrict__ pset2, VoOut *__restrict__ out)
{
    const int pnum = hdr->pnum;
    if (pnum < 4 || hdr->bad != 0) return;
    vo_dist_wave(pnum, pset2, out);
}

__global__ __launch_bounds__(64) void k_vp_draw(uint64_t seed, uint64_t seq, VoPairHeader *__restrict__ hdr, const double *__restrict__ match,
                                                int32_t *__restrict__ draws)
{
    if (hdr->bad != 0) return;
    vo_draw_lane(blockIdx.x * 64 + threadIdx.x, seed, seq, hdr->rst, hdr->pnum, match, match + 1, 2, draws, &hdr->capped);
}

__global__ __launch_bounds__(64) void k_vp_score(const VoPairHeader *__restrict__ hdr, const double *__restrict__ pset1, const double *__restrict__ pset2,
                                                 const int32_t *__restrict__ draws, const VoOut *__restrict__ out, unsigned long long *__restrict__ masks,
                                                 int32_t *__restrict__ cnum, int32_t *__restrict__ state)
{
    const int pnum = hdr->pnum;
    if ((int)blockIdx.x >= hdr->rst || hdr->bad != 0) return;
    vo_score_hyp(blockIdx.x, pnum, pset1, pset2, draws, out, (pnum + 63) / 64, masks, cnum, state);
}

__global__ __launch_bounds__(64) void k_vp_final(const VoPairHeader *__restrict__ hdr, const double *__restrict__ pset1, const double *__restrict__ pset2,
                                                 const int32_t *__restrict__ cnum, const unsigned long long *__restrict__ masks, VoOut *__restrict__ out,
                                                 int32_t *__restrict__ inl_out)
{
    const int pnum = hdr->pnum;
    if (pnum < 4 || hdr->bad != 0) return;
    vo_final_wave(pnum, hdr->rst, pset1, pset2, cnum, (pnum + 63) / 64, masks, out, inl_out);
}

// vodometry_dr_ye.m:152-160: fewer than four matches
void vo_no_solution(pre3_vo_result *res)
{
    if (res == nullptr) return;
    memset(res, 0, sizeof *res);
    res->sta = 4; res->u[3] = 1.0;
}

}  // namespace

static size_t vp_part_each(int n1, int n2) { return up16(sizeof(double) * (size_t)ceil_div(n2, ICS_T) * n1); }
size_t vp_match_part_bytes(int n1, int n2) { return 3 * vp_part_each(n1, n2); }      // pb | ps | pa (pa needs half of its share)

int launch_vp_match(int n1, int n2, const double *des1, const double *des2, double thresh, void *part, double *match, void *hdr_dev, hipStream_t st)
{
    const int ntn = ceil_div(n2, ICS_T);
    char *p = (char *)part;
    IcMatchRide r{};
    r.ntn = ntn; r.N = n1; r.K2 = n2; r.n_blocks = ntn * ceil_div(n1, ICS_T);
    r.bank = des1; r.scan = des2; r.has_h = nullptr;
    r.pb = (double *)p; r.ps = (double *)(p + vp_part_each(n1, n2)); r.pa = (int32_t *)(p + 2 * vp_part_each(n1, n2));
    hipLaunchKernelGGL(k_vp_match, dim3(r.n_blocks), dim3(256), 0, st, r);
    hipLaunchKernelGGL(k_vp_pairs, dim3(1), dim3(VP_NTH), 0, st, n1, ntn, (float)thresh, (const double *)r.pb, (const double *)r.ps, (const int32_t *)r.pa, match,
                       (VoPairHeader *)hdr_dev);
    PRE3_HIP(hipGetLastError());
    return PRE3_OK;
}

}  // namespace pre3

using namespace pre3;

// ---- one host path for the pair (pre3_vo_pair_seeded, pre3_predict_pair_seeded): the views, the layout of cur's work block, the launches, and the checks
// of what comes back.  [header | VoOut | match | pset1 | pset2 | draws | cnum | state | inliers] come back in one transfer; the partials and masks stay
namespace {
struct VpPair {
    SrFrameView v1, v2; SrKeypointView k1, k2;
    size_t o_out, o_match, o_p1, o_p2, o_draws, o_cnum, o_state, o_inl, o_end;
    bool with_cov = false; size_t o_cov = 0;        // the *_cov_* entry points: a VoCov block behind the result block, k_vo_cov behind k_vp_final
    // pre3_vo_pair_pnp_seeded: cur's pixels of the matches and the EPnP result behind the inlier flags, inside the transfer
    const pre3_cam *pnp_cam = nullptr; int pnp_undistort = 0; size_t o_pix = 0, o_pnp = 0;
    char *d = nullptr, *pin = nullptr;              // cur's device work block and its pinned image
};
bool vp_empty(const VpPair &p) { return p.k1.n_kept == 0 || p.k2.n_kept == 0; }

// offsets, work blocks, prev lent to cur's stream, the memset of header and result block, the eight launches -- everything on cur's stream, no wait
int vp_queue(pre3_sr_frame *prev, pre3_sr_frame *cur, double thresh, uint64_t seed, uint64_t seq, VpPair *q)
{
    const SrFrameView &v1 = q->v1, &v2 = q->v2;
    const SrKeypointView &k1 = q->k1, &k2 = q->k2;
    const int n1 = k1.n_kept, n2 = k2.n_kept;
    const int wcap = ceil_div(n1, 64);
    const size_t o_out = sizeof(VoPairHeader), o_cov = up16(o_out + sizeof(VoOut)), o_match = q->with_cov ? up16(o_cov + sizeof(VoCov)) : o_cov;
    const size_t o_p1 = o_match + up16(sizeof(double) * 2 * (size_t)n1);
    const size_t o_p2 = o_p1 + up16(sizeof(double) * 3 * (size_t)n1), o_draws = o_p2 + up16(sizeof(double) * 3 * (size_t)n1);
    const size_t o_cnum = o_draws + up16(sizeof(int32_t) * 4 * VO_RST_CAP), o_state = o_cnum + up16(sizeof(int32_t) * VO_RST_CAP);
    const bool pnp = q->pnp_cam != nullptr;
    const size_t o_inl = o_state + up16(sizeof(int32_t) * VO_RST_CAP), o_pix = o_inl + up16(sizeof(int32_t) * (size_t)n1);
    const size_t o_pnp = pnp ? o_pix + up16(sizeof(double) * 2 * (size_t)n1) : o_pix, o_end = pnp ? o_pnp + up16(sizeof(pre3_pnp_result)) : o_pix;
    const size_t o_part = o_end, o_masks = o_part + vp_match_part_bytes(n1, n2), o_list = up16(o_masks + sizeof(unsigned long long) * (size_t)VO_RST_CAP * wcap);
    const size_t total = pnp ? o_list + sizeof(int32_t) * ((size_t)n1 + 4) : o_masks + sizeof(unsigned long long) * (size_t)VO_RST_CAP * wcap;
    q->o_out = o_out; q->o_match = o_match; q->o_p1 = o_p1; q->o_p2 = o_p2; q->o_draws = o_draws; q->o_cnum = o_cnum; q->o_state = o_state;
    q->o_inl = o_inl; q->o_end = o_end; q->o_cov = o_cov; q->o_pix = o_pix; q->o_pnp = o_pnp;
    char *d = nullptr;
    PRE3_TRY(sr_frame_pair_work(cur, total, o_end, (void **)&d, (void **)&q->pin));
    q->d = d;
    hipStream_t st = v2.stream;
    PRE3_TRY(sr_frame_lend(prev, st));
    PRE3_HIP(hipMemsetAsync(d, 0, o_match, st));                          // the header (*capped starts at zero) and the result block

    VoPairHeader *hdr = (VoPairHeader *)d;
    VoOut *out = (VoOut *)(d + o_out);
    double *match = (double *)(d + o_match), *p1 = (double *)(d + o_p1), *p2 = (double *)(d + o_p2);
    int32_t *draws = (int32_t *)(d + o_draws), *cnum = (int32_t *)(d + o_cnum), *state = (int32_t *)(d + o_state), *inl = (int32_t *)(d + o_inl);
    unsigned long long *masks = (unsigned long long *)(d + o_masks);
    PRE3_TRY(launch_vp_match(n1, n2, k1.des, k2.des, thresh, d + o_part, match, hdr, st));
    const VpFrame f1{ v1.x, v1.y, v1.z, k1.frm, k1.ldf, n1 }, f2{ v2.x, v2.y, v2.z, k2.frm, k2.ldf, n2 };
    hipLaunchKernelGGL(k_vp_gather, dim3(ceil_div(n1, 64), 2), dim3(64), 0, st, v2.rows, v2.cols, f1, f2, (const double *)match, p1, p2, hdr);
    hipLaunchKernelGGL(k_vp_dist, dim3(1), dim3(64), 0, st, (const VoPairHeader *)hdr, (const double *)p2, out);
    hipLaunchKernelGGL(k_vp_draw, dim3(ceil_div(VO_RST_CAP, 64)), dim3(64), 0, st, seed, seq, hdr, (const double *)match, draws);
    hipLaunchKernelGGL(k_vp_score, dim3(VO_RST_CAP), dim3(64), 0, st, (const VoPairHeader *)hdr, (const double *)p1, (const double *)p2, (const int32_t *)draws,
                       (const VoOut *)out, masks, cnum, state);
    hipLaunchKernelGGL(k_vp_final, dim3(1), dim3(64), 0, st, (const VoPairHeader *)hdr, (const double *)p1, (const double *)p2, (const int32_t *)cnum,
                       (const unsigned long long *)masks, out, inl);
    PRE3_HIP(hipGetLastError());
    // (the memset above left status = 0 in the block; pset1, pset2 and inl hold n1 positions, which bounds the launch whatever the header says)
    if (q->with_cov) PRE3_TRY(launch_vo_cov_pair(hdr, out, n1, p1, p2, inl, (VoCov *)(d + o_cov), st));
    if (pnp) PRE3_TRY(launch_pnp_pair(hdr, out, n1, p1, match, k2.frm, k2.ldf, n2, inl, q->pnp_cam, q->pnp_undistort, (double *)(d + o_pix), (int32_t *)(d + o_list),
                                      (pre3_pnp_result *)(d + o_pnp), st));
    return PRE3_OK;
}

// what the transfer brought: the header (checked against the sizing rule) and the result block; then the two pairs that are refused (pnum >= 4)
int vp_header(const VpPair &p, VoPairHeader *h, VoOut *o)
{
    *h = *(const VoPairHeader *)p.pin;
    *o = *(const VoOut *)(p.pin + p.o_out);
    PRE3_CHECK(h->pnum >= 0 && h->pnum <= p.k1.n_kept && h->rst == vo_rst(h->pnum), PRE3_E_HIP, "pre3_vo_pair_seeded: the device reports %d matches of %d keypoints and %d hypotheses",
               h->pnum, p.k1.n_kept, h->rst);
    return PRE3_OK;
}
int vp_refuse_bad(const VoPairHeader &h)
{
    PRE3_CHECK(h.bad == 0, PRE3_E_HIP, "pre3_vo_pair_seeded: %s", (h.bad & 1) ? "a match refers to a keypoint that does not exist" : "a kept keypoint rounds to a pixel outside the range image");
    return PRE3_OK;
}
int vp_refuse_near(const VoOut &o)
{
    PRE3_CHECK(o.dist_ok, PRE3_E_NUMERIC, "vo: no matched point is farther than 0.4 m from the camera (ransac_dr_ye.m:21 has no minimum there)");
    return PRE3_OK;
}

// the pair's covariance block as the ABI hands it out: cov on status 1 only
void vp_cov_out(const VpPair &p, double *cov_out, int32_t *cov_status_out)
{
    const VoCov *cv = (const VoCov *)(p.pin + p.o_cov);
    if (cov_status_out) *cov_status_out = cv->status;
    if (cov_out && cv->status == VC_VALID) memcpy(cov_out, cv->cov, sizeof cv->cov);
}

// the dense ICP queued behind the pair's launches (pre3_icp_pair_seeded)
// the EPnP refit queued behind the pair's launches (pre3_vo_pair_pnp_seeded)
struct PnpAttach { const pre3_cam *cam; int undistort; double *pix2_out; pre3_pnp_result *res; };
void pnp_not_computed(pre3_pnp_result *r)
{
    memset(r, 0, sizeof *r);
    r->R[0] = r->R[4] = r->R[8] = 1.0; r->u[3] = 1.0; r->err[0] = r->err[1] = r->err[2] = NAN; r->sta = 0;
}
struct IcpAttach { int stride; double res; IcpOutputs out; bool with_cov = false; };      // with_cov: pre3_icp_pair_cov_seeded
void icp_not_run(const IcpAttach *icp)
{
    if (icp && icp->out.res) icp->out.res->sta = ICP_NOT_RUN;
    if (icp && icp->out.cov_status) *icp->out.cov_status = VC_NOT_COMPUTED;
}

// pre3_vo_pair_seeded, and -- with_cov -- pre3_vo_pair_cov_seeded: the same launches, transfer and checks, k_vo_cov and its block besides;
// icp != nullptr: pre3_icp_frames' launches behind them on the same stream, seeded from the pair's result block
int vo_pair_impl(const char *who, bool with_cov, pre3_sr_frame *prev, pre3_sr_frame *cur, double thresh, uint64_t seed, uint64_t seq, int32_t *pnum_out, double *match_out,
                 double *pset1_out, double *pset2_out, int32_t *draws_out, int32_t *capped_out, int32_t *cnum_out, int32_t *state_out,
                 int32_t *inlier_out, pre3_vo_result *res, double *cov_out, int32_t *cov_status_out, const IcpAttach *icp = nullptr, const PnpAttach *pnp = nullptr)
{
    VpPair p;
    p.with_cov = with_cov;
    if (pnp) {
        PRE3_CHECK(pnp->cam != nullptr && pnp->res != nullptr, PRE3_E_ARG, "%s: a null camera or EPnP result", who);
        PRE3_CHECK(pnp->cam->f > 0, PRE3_E_ARG, "%s: the focal length must be positive", who);
        p.pnp_cam = pnp->cam; p.pnp_undistort = pnp->undistort;
    }
    PRE3_TRY(sr_frame_pair_views(who, prev, cur, thresh, &p.v1, &p.v2, &p.k1, &p.k2));
    if (icp) PRE3_TRY(icp_check_args(who, icp->stride, icp->res));
    PRE3_TRY(select_device(who, p.v2.device));
    if (pnum_out) *pnum_out = 0;
    if (cov_status_out) *cov_status_out = VC_NOT_COMPUTED;
    if (icp && icp->out.cov_status) *icp->out.cov_status = VC_NOT_COMPUTED;
    if (pnp) pnp_not_computed(pnp->res);                                   // what every early way out leaves: sta = 0, the identity increment
    if (vp_empty(p)) { vo_no_solution(res); icp_not_run(icp); return PRE3_OK; }      // siftmatch of an empty set: no match, nothing to queue
    PRE3_TRY(vp_queue(prev, cur, thresh, seed, seq, &p));
    IcpJob job;
    job.with_cov = icp != nullptr && icp->with_cov;
    if (icp) PRE3_TRY(icp_job_queue_frames(&job, p.v1, p.v2, icp->stride, icp->res, nullptr, nullptr, (const VoOut *)(p.d + p.o_out), icp->out, p.v2.stream));
    size_t need = p.o_match;                    // the prefix of the block the caller's outputs reach into
    if (match_out) need = p.o_p1;
    if (pset1_out) need = p.o_p2;
    if (pset2_out) need = p.o_draws;
    if (draws_out) need = p.o_cnum;
    if (cnum_out) need = p.o_state;
    if (state_out) need = p.o_inl;
    if (inlier_out) need = p.o_pix;
    if (pnp) need = p.o_end;
    const hipStream_t st = p.v2.stream;
    char *pin = p.pin;
    PRE3_HIP(hipMemcpyAsync(pin, p.d, need, hipMemcpyDeviceToHost, st));
    PRE3_TRY(sr_frame_reclaim(prev, st));                                 // a later load into prev stays behind these reads
    PRE3_HIP(hipStreamSynchronize(st));

    VoPairHeader h; VoOut o;
    PRE3_TRY(vp_header(p, &h, &o));
    const int pnum = h.pnum, rst = h.rst;
    if (pnum_out) *pnum_out = pnum;
    if (match_out) memcpy(match_out, pin + p.o_match, sizeof(double) * 2 * (size_t)pnum);
    if (pnum < 4) { vo_no_solution(res); icp_not_run(icp); return PRE3_OK; }
    PRE3_TRY(vp_refuse_bad(h));
    if (with_cov) vp_cov_out(p, cov_out, cov_status_out);
    if (pset1_out) memcpy(pset1_out, pin + p.o_p1, sizeof(double) * 3 * (size_t)pnum);
    if (pset2_out) memcpy(pset2_out, pin + p.o_p2, sizeof(double) * 3 * (size_t)pnum);
    if (draws_out) memcpy(draws_out, pin + p.o_draws, sizeof(int32_t) * 4 * (size_t)rst);
    if (capped_out) *capped_out = h.capped;
    PRE3_TRY(vp_refuse_near(o));
    if (cnum_out) memcpy(cnum_out, pin + p.o_cnum, sizeof(int32_t) * (size_t)rst);
    if (state_out) memcpy(state_out, pin + p.o_state, sizeof(int32_t) * (size_t)rst);
    if (inlier_out) memcpy(inlier_out, pin + p.o_inl, sizeof(int32_t) * (size_t)pnum);
    if (res) vo_result(o, res);
    if (pnp) {
        if (pnp->pix2_out) memcpy(pnp->pix2_out, pin + p.o_pix, sizeof(double) * 2 * (size_t)pnum);
        memcpy(pnp->res, pin + p.o_pnp, sizeof *pnp->res);
        pnp->res->n_support = o.n_support;
    }
    if (icp) PRE3_TRY(icp_job_collect(&job, who, icp->out));
    return PRE3_OK;
}

// fv.m:47 + Calculate_V_Omega_RANSAC_dr_ye.m:41-50 + predict_state_and_covariance.m:27-143: the pair's launches on cur's stream,
// then k_predict on the context's stream with the increment chosen on the device from the pair's result block; u never reaches the host.
// with_cov (pre3_predict_pair_cov_seeded): k_vo_cov behind k_vp_final, and its block is this one prediction's Pn under the status rule
int predict_pair_impl(const char *who, bool with_cov, pre3_ctx *c, pre3_sr_frame *prev, pre3_sr_frame *cur, double thresh, uint64_t seed, uint64_t seq, int32_t *pnum_out,
                      pre3_vo_result *res_out, double *cov_out, int32_t *cov_status_out)
{
    static const double u_identity[7] = { 0, 0, 0, 1, 0, 0, 0 };
    VpPair p;
    p.with_cov = with_cov;
    PRE3_CHECK(c != nullptr, PRE3_E_ARG, "%s: null context", who);
    PRE3_TRY(sr_frame_pair_views(who, prev, cur, thresh, &p.v1, &p.v2, &p.k1, &p.k2));
    PRE3_CHECK(p.v2.device == c->device, PRE3_E_ARG, "%s: the frames are on device %d, the context on device %d", who, p.v2.device, c->device);
    PRE3_CHECK(c->x_valid[PRE3_X_K_K] && c->p_which == PRE3_X_K_K, PRE3_E_STATE, "%s: needs (x_k_k, p_k_k) on the device", who);
    EntryScope scope(c); PRE3_TRY(scope.rc);            // as pre3_predict's
    const bool wait = pnum_out != nullptr || res_out != nullptr || cov_out != nullptr || cov_status_out != nullptr;
    if (pnum_out) *pnum_out = 0;
    if (cov_status_out) *cov_status_out = VC_NOT_COMPUTED;
    if (vp_empty(p)) {                                  // no pair launches: the ordinary prediction with the identity increment
        PRE3_TRY(launch_predict_impl(c, u_identity));
        c->x_valid[PRE3_X_K_KM1] = true; c->p_which = PRE3_X_K_KM1; c->hp_all_valid = false;
        vo_no_solution(res_out);
        return PRE3_OK;
    }
    PRE3_TRY(vp_queue(prev, cur, thresh, seed, seq, &p));
    const hipStream_t st = p.v2.stream;
    PRE3_TRY(sr_frame_reclaim(prev, st));               // prev is read by the pair's launches only
    PRE3_TRY(sr_frame_lend(cur, c->stream));            // the prediction reads cur's work block behind k_vp_final
    const PredictUDev ud{ (const VoOut *)(p.d + p.o_out), (const VoPairHeader *)p.d, c->stats + 6 };
    const PnPair pp{ (const VoCov *)(p.d + p.o_cov), ud.out, ud.hdr, nullptr };
    PRE3_TRY(launch_predict_impl(c, nullptr, false, 0, 0, &ud, with_cov ? &pp : nullptr));
    c->x_valid[PRE3_X_K_KM1] = true; c->p_which = PRE3_X_K_KM1; c->hp_all_valid = false;
    // the next pair call's memset of this work block, a load or a keypoint call on cur stay behind the read of u
    if (wait) PRE3_HIP(hipMemcpyAsync(c->pinned_stats, c->stats, sizeof(int32_t) * 16, hipMemcpyDeviceToHost, c->stream));
    PRE3_TRY(sr_frame_reclaim(cur, c->stream));
    if (!wait) return PRE3_OK;

    // one wait, on cur's stream, which now stands behind the prediction as well: header and result block in one transfer
    PRE3_HIP(hipMemcpyAsync(p.pin, p.d, p.o_match, hipMemcpyDeviceToHost, st));
    PRE3_TRY(stream_drain_on(st, c->comm, who));
    if (pu_word_refusal(c->pinned_stats[6]) != PU_OK) (void)hipMemsetAsync(c->stats + 6, 0, sizeof(int32_t), c->stream);      // reported by this call's return code
    VoPairHeader h; VoOut o;
    PRE3_TRY(vp_header(p, &h, &o));
    if (pnum_out) *pnum_out = h.pnum;
    if (h.pnum < 4) { vo_no_solution(res_out); return PRE3_OK; }
    PRE3_TRY(vp_refuse_bad(h));
    PRE3_TRY(vp_refuse_near(o));
    if (with_cov) vp_cov_out(p, cov_out, cov_status_out);
    if (res_out) vo_result(o, res_out);
    return PRE3_OK;
}

// the ICP run's device block from cur's handle (pre3_own.h: one owner, which outlives the prediction's read when no host waits)
int icp_block_of_frame(void *owner, size_t bytes, char **out) { return sr_frame_icp_work((pre3_sr_frame *)owner, bytes, (void **)out); }

// predict_pair_impl with the dense ICP and both covariances between the pair and the prediction (pre3_predict_icp_pair_seeded):
// pre3_icp_pair_cov_seeded's launches on cur's stream, then k_predict on the context's with u and Pn taken on the device under predict_icp_select
int predict_icp_pair_impl(const char *who, pre3_ctx *c, pre3_sr_frame *prev, pre3_sr_frame *cur, double thresh, uint64_t seed, uint64_t seq, int stride, double res,
                          double max_error, int noise, int32_t *pnum_out, pre3_vo_result *res_out, pre3_icp_result *icp_out, double *cov_out,
                          int32_t *cov_status_out, int32_t *taken_out)
{
    static const double u_identity[7] = { 0, 0, 0, 1, 0, 0, 0 };
    VpPair p;
    p.with_cov = true;
    PRE3_CHECK(c != nullptr, PRE3_E_ARG, "%s: null context", who);
    PRE3_TRY(sr_frame_pair_views(who, prev, cur, thresh, &p.v1, &p.v2, &p.k1, &p.k2));
    PRE3_TRY(icp_check_args(who, stride, res));
    PRE3_CHECK(pi_max_error_ok(max_error), PRE3_E_ARG, "%s: max_error must be positive (+inf: no gate)", who);
    PRE3_CHECK(noise >= PRE3_NOISE_CONTEXT && noise <= PRE3_NOISE_ICP_FLOOR, PRE3_E_ARG, "%s: noise is %d, not one of PRE3_NOISE_*", who, noise);
    PRE3_CHECK(p.v2.device == c->device, PRE3_E_ARG, "%s: the frames are on device %d, the context on device %d", who, p.v2.device, c->device);
    PRE3_CHECK(c->x_valid[PRE3_X_K_K] && c->p_which == PRE3_X_K_K, PRE3_E_STATE, "%s: needs (x_k_k, p_k_k) on the device", who);
    EntryScope scope(c); PRE3_TRY(scope.rc);            // as pre3_predict's
    const bool wait = pnum_out != nullptr || res_out != nullptr || icp_out != nullptr || cov_out != nullptr || cov_status_out != nullptr || taken_out != nullptr;
    if (pnum_out) *pnum_out = 0;
    if (cov_status_out) cov_status_out[0] = cov_status_out[1] = VC_NOT_COMPUTED;
    if (taken_out) { taken_out[0] = PI_U_IDENTITY; taken_out[1] = PI_NOISE_CONTEXT; }
    if (vp_empty(p)) {                                  // no pair launches, no ICP: the ordinary prediction with the identity increment
        PRE3_TRY(launch_predict_impl(c, u_identity));
        c->x_valid[PRE3_X_K_KM1] = true; c->p_which = PRE3_X_K_KM1; c->hp_all_valid = false;
        vo_no_solution(res_out);
        if (icp_out) icp_out->sta = ICP_NOT_RUN;
        return PRE3_OK;
    }
    PRE3_TRY(vp_queue(prev, cur, thresh, seed, seq, &p));
    const hipStream_t st = p.v2.stream;
    IcpJob job;
    job.with_cov = true; job.block = icp_block_of_frame; job.owner = cur; job.pin_back = wait;
    const IcpOutputs io{ icp_out, nullptr, nullptr, nullptr, nullptr, cov_out ? cov_out + 49 : nullptr, cov_status_out ? cov_status_out + 1 : nullptr };
    PRE3_TRY(icp_job_queue_frames(&job, p.v1, p.v2, stride, res, nullptr, nullptr, (const VoOut *)(p.d + p.o_out), io, st));
    PRE3_TRY(sr_frame_reclaim(prev, st));               // prev is read by the pair's and the ICP's launches only
    PRE3_TRY(sr_frame_lend(cur, c->stream));            // the prediction reads cur's work blocks behind the ICP's last launch
    IcpDevView iv;
    icp_job_dev_view(&job, &iv);
    const PredictUIcp ui{ PredictIcpSrc{ (const VoOut *)(p.d + p.o_out), (const VoPairHeader *)p.d, (const VoCov *)(p.d + p.o_cov), iv.ctl, iv.u, iv.error, iv.cov,
                                         max_error, noise }, c->stats + 6, iv.taken };
    PRE3_TRY(launch_predict_icp(c, ui));
    c->x_valid[PRE3_X_K_KM1] = true; c->p_which = PRE3_X_K_KM1; c->hp_all_valid = false;
    if (wait) PRE3_HIP(hipMemcpyAsync(c->pinned_stats, c->stats, sizeof(int32_t) * 16, hipMemcpyDeviceToHost, c->stream));
    PRE3_TRY(sr_frame_reclaim(cur, c->stream));         // the next call's launches into these blocks, a load or a keypoint call on cur stay behind the reads
    if (!wait) return PRE3_OK;

    // one wait, on cur's stream, which now stands behind the prediction as well
    PRE3_HIP(hipMemcpyAsync(p.pin, p.d, p.o_match, hipMemcpyDeviceToHost, st));
    PRE3_HIP(hipMemcpyAsync(job.pin + job.o_pin_taken, iv.taken, sizeof(int32_t) * 2, hipMemcpyDeviceToHost, st));
    PRE3_TRY(stream_drain_on(st, c->comm, who));
    job.waited = true;
    if (pu_word_refusal(c->pinned_stats[6]) != PU_OK) (void)hipMemsetAsync(c->stats + 6, 0, sizeof(int32_t), c->stream);      // reported by this call's return code
    VoPairHeader h; VoOut o;
    PRE3_TRY(vp_header(p, &h, &o));
    if (pnum_out) *pnum_out = h.pnum;
    if (h.pnum < 4) { vo_no_solution(res_out); if (icp_out) icp_out->sta = ICP_NOT_RUN; return PRE3_OK; }
    PRE3_TRY(vp_refuse_bad(h));
    PRE3_TRY(vp_refuse_near(o));
    vp_cov_out(p, cov_out, cov_status_out);
    if (res_out) vo_result(o, res_out);
    PRE3_TRY(icp_job_collect(&job, who, io));
    const int32_t *tk = (const int32_t *)(job.pin + job.o_pin_taken);
    if (taken_out) { taken_out[0] = tk[0]; taken_out[1] = tk[1]; }
    return PRE3_OK;
}
}  // namespace

extern "C" {

int pre3_vo_pair_seeded(pre3_sr_frame *prev, pre3_sr_frame *cur, double thresh, uint64_t seed, uint64_t seq, int32_t *pnum_out, double *match_out,
                        double *pset1_out, double *pset2_out, int32_t *draws_out, int32_t *capped_out, int32_t *cnum_out, int32_t *state_out,
                        int32_t *inlier_out, pre3_vo_result *res)
{
    return vo_pair_impl("pre3_vo_pair_seeded", false, prev, cur, thresh, seed, seq, pnum_out, match_out, pset1_out, pset2_out, draws_out, capped_out, cnum_out, state_out,
                        inlier_out, res, nullptr, nullptr);
}

// RANSAC_CALC_VER2.m:191 in place: pre3_vo_pair_seeded's launches, then the EPnP refit over the pair's inliers -- prev's range
// points against cur's PIXELS -- on the same stream; still one host wait
int pre3_vo_pair_pnp_seeded(pre3_sr_frame *prev, pre3_sr_frame *cur, double thresh, uint64_t seed, uint64_t seq, const pre3_cam *cam, int undistort,
                            int32_t *pnum_out, double *match_out, double *pset1_out, double *pset2_out, int32_t *draws_out, int32_t *capped_out,
                            int32_t *cnum_out, int32_t *state_out, int32_t *inlier_out, pre3_vo_result *res, double *pix2_out, pre3_pnp_result *pnp)
{
    const PnpAttach a{ cam, undistort, pix2_out, pnp };
    PRE3_CHECK(pnp != nullptr, PRE3_E_ARG, "pre3_vo_pair_pnp_seeded: null EPnP result");
    return vo_pair_impl("pre3_vo_pair_pnp_seeded", false, prev, cur, thresh, seed, seq, pnum_out, match_out, pset1_out, pset2_out, draws_out, capped_out, cnum_out,
                        state_out, inlier_out, res, nullptr, nullptr, nullptr, &a);
}

// calc_cov_RANSAC_dr_ye.m:17-30 behind vodometry_dr_ye.m: pre3_vo_pair_seeded with k_vo_cov behind k_vp_final, still one host wait
int pre3_vo_pair_cov_seeded(pre3_sr_frame *prev, pre3_sr_frame *cur, double thresh, uint64_t seed, uint64_t seq, int32_t *pnum_out, double *match_out,
                            double *pset1_out, double *pset2_out, int32_t *draws_out, int32_t *capped_out, int32_t *cnum_out, int32_t *state_out,
                            int32_t *inlier_out, pre3_vo_result *res, double *cov_out, int32_t *cov_status_out)
{
    return vo_pair_impl("pre3_vo_pair_cov_seeded", true, prev, cur, thresh, seed, seq, pnum_out, match_out, pset1_out, pset2_out, draws_out, capped_out, cnum_out, state_out,
                        inlier_out, res, cov_out, cov_status_out);
}

// icp_with_init.m behind vodometry_dr_ye.m:139-236: pre3_vo_pair_seeded's launches, then the ICP's on the same stream, one host wait
int pre3_icp_pair_seeded(pre3_sr_frame *prev, pre3_sr_frame *cur, double thresh, uint64_t seed, uint64_t seq, int stride, double res, int32_t *pnum_out,
                         double *match_out, double *pset1_out, double *pset2_out, int32_t *draws_out, int32_t *capped_out, int32_t *cnum_out,
                         int32_t *state_out, int32_t *inlier_out, pre3_vo_result *vo_res, pre3_icp_result *icp, double *corr_out, int32_t *corr_pix_out,
                         double *data2_out, double *log_out)
{
    const IcpAttach at{ stride, res, IcpOutputs{ icp, corr_out, corr_pix_out, data2_out, log_out } };
    return vo_pair_impl("pre3_icp_pair_seeded", false, prev, cur, thresh, seed, seq, pnum_out, match_out, pset1_out, pset2_out, draws_out, capped_out, cnum_out, state_out,
                        inlier_out, vo_res, nullptr, nullptr, &at);
}

// both covariances behind pre3_icp_pair_seeded: k_vo_cov behind the pair's final fit, k_icp_cov_part / k_icp_cov_fin behind k_icp_final
int pre3_icp_pair_cov_seeded(pre3_sr_frame *prev, pre3_sr_frame *cur, double thresh, uint64_t seed, uint64_t seq, int stride, double res, int32_t *pnum_out,
                             double *match_out, double *pset1_out, double *pset2_out, int32_t *draws_out, int32_t *capped_out, int32_t *cnum_out,
                             int32_t *state_out, int32_t *inlier_out, pre3_vo_result *vo_res, pre3_icp_result *icp, double *corr_out, int32_t *corr_pix_out,
                             double *data2_out, double *log_out, double *cov_pair_out, int32_t *cov_pair_status_out, double *cov_icp_out,
                             int32_t *cov_icp_status_out)
{
    const IcpAttach at{ stride, res, IcpOutputs{ icp, corr_out, corr_pix_out, data2_out, log_out, cov_icp_out, cov_icp_status_out }, true };
    return vo_pair_impl("pre3_icp_pair_cov_seeded", true, prev, cur, thresh, seed, seq, pnum_out, match_out, pset1_out, pset2_out, draws_out, capped_out, cnum_out,
                        state_out, inlier_out, vo_res, cov_pair_out, cov_pair_status_out, &at);
}

// the prediction fed from the ICP-refined pair, u and Pn chosen on the device
int pre3_predict_icp_pair_seeded(pre3_ctx *c, pre3_sr_frame *prev, pre3_sr_frame *cur, double thresh, uint64_t seed, uint64_t seq, int stride, double res,
                                 double max_error, int noise, int32_t *pnum_out, pre3_vo_result *vo_res_out, pre3_icp_result *icp_out, double *cov_out,
                                 int32_t *cov_status_out, int32_t *taken_out)
{
    return predict_icp_pair_impl("pre3_predict_icp_pair_seeded", c, prev, cur, thresh, seed, seq, stride, res, max_error, noise, pnum_out, vo_res_out, icp_out,
                                 cov_out, cov_status_out, taken_out);
}

int pre3_predict_pair_seeded(pre3_ctx *c, pre3_sr_frame *prev, pre3_sr_frame *cur, double thresh, uint64_t seed, uint64_t seq, int32_t *pnum_out,
                             pre3_vo_result *res_out)
{
    return predict_pair_impl("pre3_predict_pair_seeded", false, c, prev, cur, thresh, seed, seq, pnum_out, res_out, nullptr, nullptr);
}

// predict_state_and_covariance.m:115: pre3_predict_pair_seeded with the pair's own covariance as this one prediction's Pn
int pre3_predict_pair_cov_seeded(pre3_ctx *c, pre3_sr_frame *prev, pre3_sr_frame *cur, double thresh, uint64_t seed, uint64_t seq, int32_t *pnum_out,
                                 pre3_vo_result *res_out, double *cov_out, int32_t *cov_status_out)
{
    return predict_pair_impl("pre3_predict_pair_cov_seeded", true, c, prev, cur, thresh, seed, seq, pnum_out, res_out, cov_out, cov_status_out);
}

}  // extern "C"
