// pre3_reloc.hip -- pre3_relocalise_seeded: the prediction of a frame on which the caller has judged the filter lost, as an EPnP pose of the whole map
// against the scan.  The project's own follow-up of sections 9 and 35: the reference has no relocalisation.
// On the context's stream, no host wait between the stages:
//   k_reloc_match   siftmatch(bank(128 x N), Descriptor_RAW(128 x K2)) exactly: the IC search's 32 x 32 tile (ic_match_tile, pre3_geomdev.h) with the
//                   identity as the stack -- every landmark is a query, no window gate; partials per (column tile, landmark)
//   k_reloc_corr    ONE workgroup: the column tiles merged in scan order, Lowe's test in float, the pairs compacted in ascending k1 (ballots and a
//                   prefix over the waves); per match the landmark's point at x_k_k -- id_point, the landmark reader's own function -- and the
//                   scan's pixel, the matches with a finite point compacted once more into Xw / U; the two counts left in device words
//   k_pnp_draw, k_pnp_hyp, k_pnp_select, k_pnp_solve (pre3_pnp.hip) with the count read on the device
//   k_predict       US = PredictUReloc, NS = PnReloc (pre3_geom.hip): u and Pn under reloc_select (pre3_reloc.h)
// pre3_relocalise_refined_seeded queues the same with k_pnp_refine (pre3_pnp.hip) between the refit and the prediction, whose tags
// are then PredictURelocRef / PnRelocRef: the refinement's u and, by the caller's mode, its covariance as the prediction's noise.
// k_reloc_corr is bound by its dependent loads (partials -> scan position; type -> offset -> state) and the sincos of an inverse-depth point, not by
// HBM or the vector pipes: a few hundred landmarks, one pass of 512.
#include <cmath>
#include <cstring>

#include "pre3_internal.h"
#include "pre3_geomdev.h"
#include "pre3_pnp.h"
#include "pre3_reloc.h"

namespace pre3 {

namespace {

static_assert(sizeof(pre3_reloc_result) == sizeof(pre3_pnp_result) + 7 * 8 + 4 * 4, "pre3_reloc_result is the refit, seven doubles and four words");

constexpr int RC_T = 512, RC_NW = RC_T / 64;

// what goes back to the host sits in front of the block's second half, in this order: header, ctl, res, pairs, flags
struct RelocHdr { int32_t n_matches, n_corr, taken, pad; double u[7], pad2; };
struct Pn49 { double v[49]; };
// the refined form's own block at the end of the work block: what k_pnp_refine and its prediction leave, back in a second transfer in front of the one wait
struct RelocRefBlk { pre3_pnp_refine_result ref; double Pn[49]; int32_t noise_taken, pad; };
static_assert(sizeof(pre3_reloc_refined_result) == sizeof(pre3_reloc_result) + sizeof(RelocRefBlk), "pre3_reloc_refined_result is the base and the refined form's block");

struct RelocLayout {
    size_t o_xw, o_u, o_mask, o_hdr, o_ctl, o_res, o_pairs, o_flag, o_back_end, o_pn, o_draws, o_sup, o_sta, o_dsum, o_idx, o_hyp, o_ref, total;
    explicit RelocLayout(int cap)
    {
        const size_t n = (size_t)cap, H = PNP_MAX_HYP;
        o_xw = 0; o_u = o_xw + up16(sizeof(double) * 3 * n); o_mask = o_u + up16(sizeof(double) * 2 * n);
        o_hdr = o_mask + up16(sizeof(unsigned long long) * H * (size_t)ceil_div(cap, 64));
        o_ctl = o_hdr + up16(sizeof(RelocHdr)); o_res = o_ctl + up16(sizeof(int32_t) * PNP_CTL_WORDS); o_pairs = o_res + up16(sizeof(pre3_pnp_result));
        o_flag = o_pairs + up16(sizeof(int32_t) * 2 * n); o_back_end = o_flag + up16(sizeof(int32_t) * n);
        o_pn = o_back_end; o_draws = o_pn + up16(sizeof(double) * 49); o_sup = o_draws + up16(sizeof(int32_t) * 6 * H); o_sta = o_sup + up16(sizeof(int32_t) * H);
        o_dsum = o_sta + up16(sizeof(int32_t) * H); o_idx = o_dsum + up16(sizeof(double) * H); o_hyp = o_idx + up16(sizeof(int32_t) * n);
        o_ref = o_hyp + up16(sizeof(pre3_pnp_result) * H);
        total = o_ref + up16(sizeof(RelocRefBlk));
    }
};

__global__ __launch_bounds__(256) void k_reloc_match(IcMatchRide r)
{
    __shared__ double Qs[ICS_T][ICS_LD], Bs[ICS_T][ICS_LD];
    ic_match_tile(r, blockIdx.x, Qs, Bs);
}

struct RelocCorr {
    int N, ntn, K2; float thresh;
    const double *pb, *ps; const int32_t *pa;       // the matcher's partials [column tile][landmark]
    const double *pos;                              // the scan's SCALE_ORIENT_POS_RAW [K2][4]: entries 0 and 1 are what pre3_ic_search installs as z
    const int32_t *lm_type, *lm_off; const double *x;
    double *Xw, *U; int32_t *pairs, *flag; RelocHdr *hdr;
    Pn49 pn; double *pn_out;                        // the call's wide noise travels as a launch argument (as k_set_pn's) into the block k_predict reads
};

__global__ __launch_bounds__(RC_T) void k_reloc_corr(RelocCorr a)
{
    __shared__ int s_m[RC_NW], s_f[RC_NW];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid < 49) a.pn_out[tid] = a.pn.v[tid];
    int n_match = 0, n_corr = 0;
    for (int q0 = 0; q0 < a.N; q0 += RC_T) {
        const int k1 = q0 + tid;
        int ok = 0, k2 = -1, fin = 0;
        double p[3] = { 0, 0, 0 };
        if (k1 < a.N) {
            a.flag[k1] = 0;                                                 // (k_pnp_select writes the first n_corr)
            double best = acc_max<double>(), second = acc_max<double>();
            for (int t = 0; t < a.ntn; ++t) {                              // scan order: ties keep the first index (siftmatch.c:110)
                const size_t o = (size_t)t * a.N + k1;
                merge3(best, second, k2, a.pb[o], a.ps[o], a.pa[o]);
            }
            ok = k2 >= 0 && k2 < a.K2 && a.thresh * (float)best <= (float)second;       // siftmatch.c:122 (k2 < K2: a guard, the tiles write no other)
            if (ok) {
                const int o = a.lm_off[k1];
                if (a.lm_type[k1] == PRE3_INVDEPTH) {
                    id_point(a.x, o, p);                                    // the point of pre3_get_landmarks (id_to_cartesian's first statement)
                } else {
                    p[0] = a.x[o]; p[1] = a.x[o + 1]; p[2] = a.x[o + 2];
                }
                fin = isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]);   // rho = 0 gives a point at infinity: left out, order kept
            }
        }
        const unsigned long long bm = __ballot(ok), bf = __ballot(fin);
        if (lane == 0) { s_m[wv] = __popcll(bm); s_f[wv] = __popcll(bf); }
        __syncthreads();
        int om = 0, tm = 0, of = 0, tf = 0;
#pragma unroll
        for (int w = 0; w < RC_NW; ++w) { const int cm = s_m[w], cf = s_f[w]; if (w < wv) { om += cm; of += cf; } tm += cm; tf += cf; }
        const unsigned long long below = (1ull << lane) - 1ull;
        if (ok) {
            const int c = n_match + om + __popcll(bm & below);              // c <= k1 < N: inside pairs
            a.pairs[2 * (size_t)c] = k1; a.pairs[2 * (size_t)c + 1] = k2;
        }
        if (fin) {
            const int f = n_corr + of + __popcll(bf & below);               // f <= c
            a.Xw[3 * (size_t)f] = p[0]; a.Xw[3 * (size_t)f + 1] = p[1]; a.Xw[3 * (size_t)f + 2] = p[2];
            a.U[2 * (size_t)f] = a.pos[4 * (size_t)k2]; a.U[2 * (size_t)f + 1] = a.pos[4 * (size_t)k2 + 1];
        }
        n_match += tm; n_corr += tf;
        __syncthreads();                                                    // (s_m / s_f are rewritten by the next pass)
    }
    if (tid == 0) { a.hdr->n_matches = n_match; a.hdr->n_corr = n_corr; a.hdr->taken = 0; a.hdr->pad = 0; }
}

}  // namespace

int reloc_alloc(pre3_ctx *c)
{
    const int cap = c->capN < RELOC_MAX_N ? c->capN : RELOC_MAX_N;
    const RelocLayout L(cap);
    PRE3_TRY(c->mem.fixed.dev(&c->reloc_dev, L.total, Zero::sync()));
    PRE3_TRY(c->mem.fixed.pin(&c->reloc_host, up16(L.o_back_end - L.o_hdr) + sizeof(RelocRefBlk), PIN_DEFAULT));
    c->reloc_cap = cap;
    return PRE3_OK;
}

namespace {

// the refined form's arguments; null: pre3_relocalise_seeded as it stands
struct RelocRefine { int n_iter; double sigma_px; int noise; };

int relocalise_run(const char *who, pre3_ctx *c, double thresh, int n_hyp, uint64_t seed, uint64_t seq, double thr_px, int undistort, int min_support,
                   const RelocRefine *rf, const double *Pn_reloc, pre3_reloc_result *res_out, RelocRefBlk *ref_out, int32_t *pairs_out, int32_t *inlier_out)
{
    PRE3_CHECK(c != nullptr, PRE3_E_ARG, "%s: null context", who);
    // every refusal comes before the scope: a refused call queues nothing and leaves deferred and pending work where it was
    PRE3_CHECK(c->N >= PNP_MIN_N, PRE3_E_ARG, "%s: a map of %d landmarks, EPnP needs %d", who, c->N, PNP_MIN_N);
    PRE3_CHECK(c->N <= c->reloc_cap, PRE3_E_ARG, "%s: a map of %d landmarks, at most %d are matched (pre3_reloc_limits)", who, c->N, c->reloc_cap);
    PRE3_CHECK(c->bank_set && c->bank != nullptr, PRE3_E_STATE, "%s: call pre3_set_descriptors first", who);
    PRE3_CHECK(c->scan_K2 > 0 && c->scan_desc != nullptr && c->scan_pos != nullptr, PRE3_E_STATE, "%s: call pre3_set_scan first (a scan of at least one keypoint)", who);
    PRE3_CHECK(c->x_valid[PRE3_X_K_K] && c->p_which == PRE3_X_K_K, PRE3_E_STATE, "%s: needs (x_k_k, p_k_k) on the device", who);
    PRE3_CHECK(n_hyp >= 1 && n_hyp <= PNP_MAX_HYP, PRE3_E_ARG, "%s: %d hypotheses, 1 .. %d are evaluated", who, n_hyp, PNP_MAX_HYP);
    PRE3_CHECK(std::isfinite(thr_px) && thr_px > 0, PRE3_E_ARG, "%s: thr_px must be positive and finite", who);
    PRE3_CHECK(std::isfinite(thresh) && thresh > 0, PRE3_E_ARG, "%s: thresh must be positive and finite", who);
    PRE3_CHECK(min_support >= RELOC_MIN_SUPPORT, PRE3_E_ARG, "%s: min_support is %d, a pose needs at least %d inliers", who, min_support, RELOC_MIN_SUPPORT);
    if (rf != nullptr) {
        PRE3_CHECK(rf->n_iter >= 0 && rf->n_iter <= PRE3_PNP_REFINE_MAX_ITER, PRE3_E_ARG, "%s: %d iterations, 0 .. %d are run", who, rf->n_iter, PRE3_PNP_REFINE_MAX_ITER);
        PRE3_CHECK(std::isfinite(rf->sigma_px) && rf->sigma_px >= 0, PRE3_E_ARG, "%s: sigma_px must be finite and not negative", who);
        PRE3_CHECK(rf->noise >= PRE3_RELOC_NOISE_CALLER && rf->noise <= PRE3_RELOC_NOISE_POSE_FLOOR, PRE3_E_ARG, "%s: noise mode %d, 0 .. 2 exist", who, rf->noise);
    }
    PRE3_CHECK(Pn_reloc != nullptr, PRE3_E_ARG, "%s: null Pn_reloc", who);
    PRE3_TRY(process_noise_check(who, Pn_reloc));
    PRE3_CHECK(c->have_cam && c->cam.f > 0, PRE3_E_ARG, "%s: camera not set", who);
    const int N = c->N, K2 = c->scan_K2, ntn = ceil_div(K2, ICS_T);
    PRE3_CHECK((size_t)ntn * N <= c->ic_pcap, PRE3_E_STATE, "%s: the matcher's partial arrays hold %zu entries, %zu are needed", who, c->ic_pcap, (size_t)ntn * N);

    EntryScope scope(c); PRE3_TRY(scope.rc);            // as pre3_predict's: a deferred HI update is completed, pending passes go out in front
    const RelocLayout L(c->reloc_cap);
    char *d = c->reloc_dev;
    RelocHdr *hdr = (RelocHdr *)(d + L.o_hdr);
    pre3_pnp_result *res = (pre3_pnp_result *)(d + L.o_res);

    IcMatchRide m{};
    m.ntn = ntn; m.N = N; m.K2 = K2; m.n_blocks = ntn * ceil_div(N, ICS_T);
    m.bank = c->bank; m.scan = c->scan_desc; m.has_h = nullptr; m.pb = c->ic_pb; m.ps = c->ic_ps; m.pa = c->ic_pa;
    hipLaunchKernelGGL(k_reloc_match, dim3(m.n_blocks), dim3(256), 0, c->stream, m);

    RelocCorr a{};
    a.N = N; a.ntn = ntn; a.K2 = K2; a.thresh = (float)thresh;
    a.pb = c->ic_pb; a.ps = c->ic_ps; a.pa = c->ic_pa; a.pos = c->scan_pos;
    a.lm_type = c->lm.type; a.lm_off = c->lm.off; a.x = c->x_kk;
    a.Xw = (double *)(d + L.o_xw); a.U = (double *)(d + L.o_u); a.pairs = (int32_t *)(d + L.o_pairs); a.flag = (int32_t *)(d + L.o_flag); a.hdr = hdr;
    for (int i = 0; i < 49; ++i) a.pn.v[i] = Pn_reloc[i];
    a.pn_out = (double *)(d + L.o_pn);
    hipLaunchKernelGGL(k_reloc_corr, dim3(1), dim3(RC_T), 0, c->stream, a);
    PRE3_HIP(hipGetLastError());

    PnpRansacDev r{};
    r.Xw = a.Xw; r.U = a.U; r.n_cap = N; r.n_dev = &hdr->n_corr; r.n_hyp = n_hyp; r.thr_px = thr_px;
    r.masks = (unsigned long long *)(d + L.o_mask); r.draws = (int32_t *)(d + L.o_draws); r.support = (int32_t *)(d + L.o_sup); r.state = (int32_t *)(d + L.o_sta);
    r.dsum = (double *)(d + L.o_dsum); r.ctl = (int32_t *)(d + L.o_ctl); r.idx = (int32_t *)(d + L.o_idx); r.flag = a.flag; r.res = res;
    r.hyp = (pre3_pnp_result *)(d + L.o_hyp);
    PRE3_TRY(launch_pnp_ransac_dev(r, &c->cam, undistort, seed, seq, c->stream));

    const PredictUReloc ur{ res, c->x_kk, min_support, hdr->u, &hdr->taken };
    RelocRefBlk *rb = (RelocRefBlk *)(d + L.o_ref);
    if (rf != nullptr) {
        PRE3_TRY(launch_pnp_refine_dev(r, &c->cam, undistort, rf->n_iter, rf->sigma_px, &rb->ref, c->stream));
        PRE3_TRY(launch_predict_reloc_refined(c, ur, a.pn_out, &rb->ref, rf->noise, rb->Pn, &rb->noise_taken));
    } else {
        PRE3_TRY(launch_predict_reloc(c, ur, a.pn_out));
    }
    c->x_valid[PRE3_X_K_KM1] = true; c->p_which = PRE3_X_K_KM1; c->hp_all_valid = false;
    if (res_out == nullptr && ref_out == nullptr && pairs_out == nullptr && inlier_out == nullptr) return PRE3_OK;       // nothing is synchronised

    // the one wait: header, ctl and refit, and the two lists when they are asked for, in one transfer (the refined form's block in a second one)
    const size_t back = (pairs_out != nullptr || inlier_out != nullptr ? L.o_flag + sizeof(int32_t) * (size_t)N : L.o_pairs) - L.o_hdr;
    PRE3_HIP(hipMemcpyAsync(c->reloc_host, d + L.o_hdr, back, hipMemcpyDeviceToHost, c->stream));
    char *ref_host = c->reloc_host + up16(L.o_back_end - L.o_hdr);
    if (rf != nullptr) PRE3_HIP(hipMemcpyAsync(ref_host, rb, sizeof(RelocRefBlk), hipMemcpyDeviceToHost, c->stream));
    PRE3_TRY(stream_drain(c, who));
    auto at = [&](size_t o) { return (const char *)c->reloc_host + (o - L.o_hdr); };
    RelocHdr hh;
    memcpy(&hh, at(L.o_hdr), sizeof hh);
    PRE3_CHECK(hh.n_matches >= 0 && hh.n_matches <= N && hh.n_corr >= 0 && hh.n_corr <= hh.n_matches, PRE3_E_STATE, "%s: inconsistent counts (%d matches, %d correspondences)",
               who, hh.n_matches, hh.n_corr);
    if (res_out) {
        int32_t ctl[PNP_CTL_WORDS];
        memcpy(ctl, at(L.o_ctl), sizeof ctl);
        memcpy(&res_out->pnp, at(L.o_res), sizeof res_out->pnp);
        memcpy(res_out->u, hh.u, sizeof res_out->u);
        res_out->n_matches = hh.n_matches; res_out->n_corr = hh.n_corr; res_out->winner = ctl[0]; res_out->taken = hh.taken;
    }
    if (ref_out && rf != nullptr) memcpy(ref_out, ref_host, sizeof *ref_out);
    if (pairs_out) memcpy(pairs_out, at(L.o_pairs), sizeof(int32_t) * 2 * (size_t)hh.n_matches);
    if (inlier_out) memcpy(inlier_out, at(L.o_flag), sizeof(int32_t) * (size_t)hh.n_corr);
    return PRE3_OK;
}

}  // namespace

}  // namespace pre3

using namespace pre3;

extern "C" {

int pre3_reloc_limits(int32_t out[2])
{
    PRE3_CHECK(out != nullptr, PRE3_E_ARG, "pre3_reloc_limits: null output");
    out[0] = RELOC_MAX_N; out[1] = PNP_MAX_HYP;
    return PRE3_OK;
}

int pre3_relocalise_seeded(pre3_ctx *c, double thresh, int n_hyp, uint64_t seed, uint64_t seq, double thr_px, int undistort, int min_support,
                           const double *Pn_reloc, pre3_reloc_result *res_out, int32_t *pairs_out, int32_t *inlier_out)
{
    return relocalise_run("pre3_relocalise_seeded", c, thresh, n_hyp, seed, seq, thr_px, undistort, min_support, nullptr, Pn_reloc, res_out, nullptr, pairs_out, inlier_out);
}

int pre3_relocalise_refined_seeded(pre3_ctx *c, double thresh, int n_hyp, uint64_t seed, uint64_t seq, double thr_px, int undistort, int min_support, int n_iter,
                                   double sigma_px, int noise, const double *Pn_reloc, pre3_reloc_refined_result *res_out, int32_t *pairs_out, int32_t *inlier_out)
{
    const RelocRefine rf{ n_iter, sigma_px, noise };
    // (the refined result is the base and, behind it, the block the launches leave: relocalise_run's static_assert)
    return relocalise_run("pre3_relocalise_refined_seeded", c, thresh, n_hyp, seed, seq, thr_px, undistort, min_support, &rf, Pn_reloc,
                          res_out != nullptr ? &res_out->base : nullptr, res_out != nullptr ? (RelocRefBlk *)&res_out->ref : nullptr, pairs_out, inlier_out);
}

}  // extern "C"
