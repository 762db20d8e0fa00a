// pre3_step.hip -- the stage order of one filter step (mono_slam.m:153-187): the RANSAC round, the LI / HI updates, the rescue stage, the
// small-rank updates on the resident estimate, and pre3_step / pre3_step_all / pre3_step_predicted that chain them.  No compute happens on the host.
#include <time.h>
#include <algorithm>
#include <cmath>

#include "pre3_internal.h"
#include "pre3_geomdev.h"
#include "pre3_cholp.h"
#include "pre3_philox.h"

using namespace pre3;

extern "C" {

// ---- RANSAC ---------------------------------------------------------------------------------------
// zero_words > 0 (the sliced forms): that many words of c->support (supports, masks [, the missing-slice word]) are cleared on the way
// table_on_device (the seeded forms): c->hyp has been written by a draw kernel queued on the context's stream -- there is no host table to check or pull
static int ransac_prepare(pre3_ctx *c, int n_draw, int k, const int32_t *hyp, int lo = 0, int hi = -1, bool slice_form = false, size_t zero_words = 0,
                          bool table_on_device = false)
{
    PRE3_CHECK(c->measurements_set && c->projected, PRE3_E_STATE, "ransac: needs pre3_project and measurements");
    PRE3_CHECK(c->p_which == PRE3_X_K_KM1, PRE3_E_STATE, "ransac: needs the predicted estimate (call pre3_predict or set x_k_km1)");
    PRE3_CHECK(n_draw >= 1 && n_draw <= c->caph, PRE3_E_ARG, "ransac: n_draw=%d exceeds capacity %d", n_draw, c->caph);
    PRE3_CHECK(k >= 1 && k <= MAXK, PRE3_E_ARG, "ransac: k=%d unsupported (1..%d)", k, MAXK);
    PRE3_CHECK(hyp != nullptr || table_on_device, PRE3_E_ARG, "ransac: null hypothesis table");
    PRE3_CHECK(c->m >= k, PRE3_E_ARG, "ransac: %d measurements but k=%d", c->m, k);
    for (int i = 0; !table_on_device && i < n_draw * k; ++i) PRE3_CHECK(hyp[i] >= 0 && hyp[i] < c->m, PRE3_E_ARG, "ransac: hyp[%d]=%d not a position in the IC list (m=%d)", i, hyp[i], c->m);
    if (hi < 0) hi = n_draw;
    const bool sliced = lo > 0 || hi < n_draw || slice_form;
    const bool need_pull = !table_on_device && hyp != (const int32_t *)(c->inbox_host + c->off_hyp);       // not already shipped with the measurements
    if (need_pull) {
        if (c->inbox_pending) { PRE3_TRY(wait_mail(c, 10, c->seq_inbox)); c->inbox_pending = false; }
        memcpy(c->inbox_host + c->off_hyp, hyp, sizeof(int32_t) * n_draw * k);
    }
    if (sliced) {
        // one launch: the clear, the pull and the marks of the measurements this slice's hypotheses draw (k_slice_prepare)
        ++c->need_tag;
        PRE3_TRY(launch_slice_prepare(c, (const unsigned char *)c->inbox_host_dev + c->off_hyp, need_pull ? (sizeof(int32_t) * n_draw * k + 15) / 16 : 0,
                                      need_pull ? ++c->seq_inbox : c->seq_inbox, (int)zero_words, k, lo, hi, c->need_tag));
        if (need_pull) c->inbox_pending = true;
    } else {
        if (zero_words) PRE3_HIP(hipMemsetAsync(c->support, 0, sizeof(int32_t) * zero_words, c->stream));
        // (need_pull: the caller's table crosses PCIe as a rider of the H*P launch below -- its first reader is the scorer behind that launch)
    }
    c->masks = reinterpret_cast<uint32_t *>(c->support + round_up(n_draw, 4));
    c->scored_n_draw = n_draw; c->scored_k = k;         // the mask offset depends on n_draw: select / export / import must use the same
    int r = 2 * c->m, r_pad = round_up(r, NB);
    const bool inline_g = knob::inline_g() != 0;
    if (sliced) {
        // a rank's slice of a sharded round: H*P and H*P*H' only for the measurements its hypotheses draw (the scorer of hypothesis h
        // reads the 2k rows of its own landmarks and the entries of G among them, nothing else) -- the part of the round that
        // shrinks with the number of ranks.  The LI update must not gather from these partial products: hp_all_valid stays false.
        PRE3_TRY(launch_ell_HP_build(c, c->HP, c->need, c->need_tag));
        if (!inline_g) PRE3_TRY(launch_ell_G_hyp(c, k, lo, hi, r_pad));
        c->g_valid = !inline_g;
        c->hp_all_valid = false;
        return PRE3_OK;
    }
    if (need_pull) {
        const size_t n16 = (sizeof(int32_t) * n_draw * k + 15) / 16;
        const InboxRide ib{ (const int4 *)((const unsigned char *)c->inbox_host_dev + c->off_hyp), (int4 *)c->hyp, (int)n16, c->mail_dev, ++c->seq_inbox, 10, nullptr, 0 };
        c->inbox_pending = true;
        PRE3_TRY(launch_ell_HP_build(c, c->HP, nullptr, 0, &ib));
    } else
    PRE3_TRY(launch_ell_HP_build(c, c->HP));
    // H*P*H' of all measured rows is no longer built (6.6 us of launch in front of the scoring, PRE3_INLINE_G=0 brings it back): the scorer
    // computes the (2k)^2 entries among its hypothesis' rows and the LI gather the entries of S it needs, both with k_ell_G's sum
    if (!inline_g) PRE3_TRY(launch_ell_G(c, r, c->HP, c->G, r_pad, 0, nullptr, true));      // lower triangle: the scorer and the LI gather read (max, min)
    c->g_valid = !inline_g;
    c->hp_all_valid = true;
    return PRE3_OK;
}

int pre3_ransac_score(pre3_ctx *c, int n_draw, int k, const int32_t *hyp, double threshold, int hyp_begin, int hyp_end,
                      void **support_dev, void **mask_dev, int *mask_words)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    PRE3_CHECK(hyp_begin >= 0 && hyp_begin <= hyp_end && hyp_end <= n_draw, PRE3_E_ARG, "ransac: bad hypothesis range [%d,%d) of %d", hyp_begin, hyp_end, n_draw);
    int words = ceil_div(c->m, 32);
    PRE3_CHECK(n_draw >= 1 && n_draw <= c->caph, PRE3_E_ARG, "ransac: n_draw=%d exceeds capacity %d", n_draw, c->caph);
    PRE3_TRY(ransac_prepare(c, n_draw, k, hyp, hyp_begin, hyp_end, false, (size_t)round_up(n_draw, 4) + (size_t)n_draw * words));   // (supports + masks cleared on the way)
    PRE3_TRY(launch_ransac_score_impl(c, k, threshold, hyp_begin, hyp_end, round_up(2 * c->m, NB), c->support, c->masks, words));
    if (support_dev) *support_dev = c->support;
    if (mask_dev) *mask_dev = c->masks;
    if (mask_words) *mask_words = words;
    PRE3_TRY(stream_drain(c, __func__));     // the caller's collective runs on another stream
    return PRE3_OK;
}

// after the selection stage has been enqueued
static int ransac_results(pre3_ctx *c, int n_draw, int32_t *support, int32_t *li_mask, int32_t stats[4])
{
    c->li_from_host = -1; c->li_kernel = true;
    if (support || li_mask) {
        // (behind a collective the synchronisation comes second: the selection's mailbox word first, under the communicator's deadline)
        if (c->shard_round) PRE3_TRY(wait_mail(c, 8, c->seq_select));
        PRE3_TRY(stream_drain(c, __func__));
        if (support) PRE3_HIP(hipMemcpy(support, c->support, sizeof(int32_t) * n_draw, hipMemcpyDeviceToHost));
        if (li_mask && c->m) PRE3_HIP(hipMemcpy(li_mask, c->li_meas, sizeof(int32_t) * c->m, hipMemcpyDeviceToHost));
    }
    if (stats) {
        PRE3_TRY(wait_mail(c, 8, c->seq_select));
        PRE3_CHECK(!c->shard_round || c->mail_host[11] == 0, PRE3_E_COMM, "sharded RANSAC: a rank failed before the collective of this round (its slice is missing from the sums)");
        for (int i = 0; i < 4; ++i) stats[i] = c->mail_host[i];
    }
    return PRE3_OK;
}

int pre3_ransac_select(pre3_ctx *c, int n_draw, int k, int early_exit, int32_t *support, int32_t *li_mask, int32_t stats[4])
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    PRE3_CHECK(n_draw >= 1 && n_draw <= c->caph, PRE3_E_ARG, "ransac: n_draw out of range");
    PRE3_CHECK(n_draw == c->scored_n_draw && k == c->scored_k, PRE3_E_STATE, "pre3_ransac_select: n_draw=%d, k=%d differs from the scored round (n_draw=%d, k=%d): the mask buffer is laid out for that round", n_draw, k, c->scored_n_draw, c->scored_k);
    int words = ceil_div(c->m, 32);
    PRE3_TRY(launch_ransac_select_impl(c, n_draw, k, early_exit, c->support, c->masks, words));
    return ransac_results(c, n_draw, support, li_mask, stats);
}

int pre3_ransac_export(pre3_ctx *c, int n_draw, void *support_dst_dev, void *mask_dst_dev)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    PRE3_CHECK(n_draw >= 1 && n_draw <= c->caph, PRE3_E_ARG, "ransac: n_draw out of range");
    PRE3_CHECK(n_draw == c->scored_n_draw, PRE3_E_STATE, "pre3_ransac_export: n_draw=%d differs from the scored round (n_draw=%d): the mask buffer is laid out for that round", n_draw, c->scored_n_draw);
    int words = ceil_div(c->m, 32);
    if (support_dst_dev) PRE3_HIP(hipMemcpyAsync(support_dst_dev, c->support, sizeof(int32_t) * n_draw, hipMemcpyDeviceToDevice, c->stream));
    if (mask_dst_dev) PRE3_HIP(hipMemcpyAsync(mask_dst_dev, c->masks, sizeof(uint32_t) * (size_t)n_draw * words, hipMemcpyDeviceToDevice, c->stream));
    PRE3_TRY(stream_drain(c, __func__));
    return PRE3_OK;
}

int pre3_ransac_import(pre3_ctx *c, int n_draw, const void *support_src_dev, const void *mask_src_dev)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    PRE3_CHECK(n_draw >= 1 && n_draw <= c->caph, PRE3_E_ARG, "ransac: n_draw out of range");
    PRE3_CHECK(n_draw == c->scored_n_draw, PRE3_E_STATE, "pre3_ransac_import: n_draw=%d differs from the scored round (n_draw=%d): the mask buffer is laid out for that round", n_draw, c->scored_n_draw);
    int words = ceil_div(c->m, 32);
    if (support_src_dev) PRE3_HIP(hipMemcpyAsync(c->support, support_src_dev, sizeof(int32_t) * n_draw, hipMemcpyDeviceToDevice, c->stream));
    if (mask_src_dev) PRE3_HIP(hipMemcpyAsync(c->masks, mask_src_dev, sizeof(uint32_t) * (size_t)n_draw * words, hipMemcpyDeviceToDevice, c->stream));
    PRE3_TRY(stream_drain(c, __func__));
    return PRE3_OK;
}

// One sharded RANSAC round with everything on the context's stream: [H*P | H*P*H' of this rank's measurements] -> scoring of hypotheses
// [lo, hi) -> ncclAllReduce(sum) of [supports | masks], in place (the slices are disjoint and the buffer is cleared first: the integer sum
// is the union) -> selection.  The host waits once, on the selection's mailbox word.
int pre3_ransac_sharded(pre3_ctx *c, int n_draw, int k, const int32_t *hyp, double threshold, int early_exit, int32_t *support, int32_t *li_mask,
                        int32_t stats[4])
{
    // What may differ between the ranks must not decide whether a rank enters the collective: only the arguments every rank passes alike (the
    // communicator, n_draw) return early.  Everything rank-local -- the deferred work of the previous step (EntryScope), the measurements, the
    // table, a failed launch -- is folded into rc_local: the rank then still enters ncclAllReduce, with its slice zero and the missing-slice
    // word set, and every rank fails the round with PRE3_E_COMM instead of waiting for a partner that has returned.
    PRE3_CHECK(c != nullptr, PRE3_E_ARG, "null context");
    PRE3_HIP(hipSetDevice(c->device));
    PRE3_CHECK(c->comm != nullptr, PRE3_E_STATE, "pre3_ransac_sharded: no communicator (pre3_comm_init / pre3_set_comm)");
    PRE3_CHECK(n_draw >= 1 && n_draw <= c->caph, PRE3_E_ARG, "ransac: n_draw=%d exceeds capacity %d", n_draw, c->caph);
    EntryScope scope(c);
    int rc_local = scope.rc;
    int rank = 0, world = 1;
    comm_rank_world(c->comm, &rank, &world);
    const int base = n_draw / world, rem = n_draw % world;
    const int lo = rank * base + std::min(rank, rem), hi = lo + base + (rank < rem ? 1 : 0);
    const int words = ceil_div(c->m, 32);
    // the element count of the all-reduce comes from the contexts' capacities, which the ranks share (replicas), not from this rank's
    // measurement count: supports | masks laid out for the capacity's mask words | the missing-slice word
    const size_t count = (size_t)round_up(n_draw, 4) + (size_t)n_draw * c->mask_words_cap;
    if (rc_local == PRE3_OK) rc_local = ransac_prepare(c, n_draw, k, hyp, lo, hi, true, count + 1);
    if (rc_local != PRE3_OK) (void)hipMemsetAsync(c->support, 0, sizeof(int32_t) * (count + 1), c->stream);      // (a failure in front of the prepare launch: the buffer must still be clear)
    if (rc_local == PRE3_OK && hi > lo) rc_local = launch_ransac_score_impl(c, k, threshold, lo, hi, round_up(2 * c->m, NB), c->support, c->masks, words);
    if (rc_local != PRE3_OK) {
        (void)hipMemsetAsync(c->support, 0, sizeof(int32_t) * count, c->stream);                      // whatever part of the slice got written does not count
        (void)hipMemsetAsync(c->support + count, 1, sizeof(int32_t), c->stream);                       // (0x01010101: non-zero is all that matters)
    }
    const int rc_coll = comm_all_reduce_i32(c->comm, c->support, count + 1, c->stream);
    if (rc_local != PRE3_OK) return rc_local;
    PRE3_TRY(rc_coll);
    PRE3_TRY(launch_ransac_select_impl(c, n_draw, k, early_exit, c->support, c->masks, words, (int)count));
    c->shard_round = true;
    return ransac_results(c, n_draw, support, li_mask, stats);
}

static int ransac_impl(pre3_ctx *c, int n_draw, int k, const int32_t *hyp, double threshold, int early_exit, int32_t *support, int32_t *li_mask, int32_t stats[4],
                       bool table_on_device = false)
{
    c->shard_round = false; c->carry.select_pending = false;
    PRE3_TRY(ransac_prepare(c, n_draw, k, hyp, 0, -1, false, 0, table_on_device));
    int words = ceil_div(c->m, 32);
    // Scoring, then the selection stage (the reference's loop replayed on the supports) as a launch of its own, never in the scoring launch's
    // last workgroup: every workgroup would pay a device-scope release (an L2 write-back) and a ticket before it may finish, and the last one
    // would start the selection behind an L2 invalidate (measured: DESIGN.md section 4a).
    PRE3_TRY(launch_ransac_score_impl(c, k, threshold, 0, n_draw, round_up(2 * c->m, NB), c->support, c->masks, words));
    // pre3_step: the selection rides in the LI gather's launch (k_select_gather), which pre3_update_li sends next
    if (c->req.defer_select && !support && !li_mask && !stats && select_gather_usable(c)) {
        c->carry.select_pending = true; c->carry.sel_n_draw = n_draw; c->carry.sel_k = k; c->carry.sel_early_exit = early_exit;
        c->li_from_host = -1; c->li_kernel = true;
        return PRE3_OK;
    }
    PRE3_TRY(launch_ransac_select_impl(c, n_draw, k, early_exit, c->support, c->masks, words));
    return ransac_results(c, n_draw, support, li_mask, stats);
}
int pre3_ransac(pre3_ctx *c, int n_draw, int k, const int32_t *hyp, double threshold, int early_exit, int32_t *support, int32_t *li_mask,
                int32_t stats[4])
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    return ransac_impl(c, n_draw, k, hyp, threshold, early_exit, support, li_mask, stats);
}

// ---- the seeded forms: the table is drawn on the device, on the context's stream, in front of the launches that read it
struct DrawSeed { unsigned long long seed, seq; };
static inline int seeded_k(int m) { return m > 3 ? 3 : 1; }          // select_random_match.m:47-51
// the table back to the caller, on request only (synchronises)
static int seeded_table_out(pre3_ctx *c, int n_draw, int k, int32_t *hyp_out, int32_t *k_out)
{
    if (k_out) *k_out = k;
    if (hyp_out == nullptr) return PRE3_OK;
    PRE3_HIP(hipMemcpyAsync(hyp_out, c->hyp, sizeof(int32_t) * (size_t)n_draw * k, hipMemcpyDeviceToHost, c->stream));
    return stream_drain(c, __func__);
}

int pre3_ransac_seeded(pre3_ctx *c, uint64_t seed, uint64_t seq, int n_draw, double threshold, int early_exit, int32_t *hyp_out, int32_t *k_out,
                       int32_t *support, int32_t *li_mask, int32_t stats[4])
{
    PRE3_CHECK(c != nullptr, PRE3_E_ARG, "null context");
    PRE3_CHECK(n_draw >= 1 && n_draw <= c->caph, PRE3_E_ARG, "ransac: n_draw=%d outside [1, %d]", n_draw, c->caph);
    EntryScope scope(c); PRE3_TRY(scope.rc);
    PRE3_CHECK(c->measurements_set && c->projected, PRE3_E_STATE, "ransac: needs pre3_project and measurements");
    PRE3_CHECK(c->p_which == PRE3_X_K_KM1, PRE3_E_STATE, "ransac: needs the predicted estimate (call pre3_predict or set x_k_km1)");
    const int k = seeded_k(c->m);
    PRE3_TRY(launch_draw_1p(seed, seq, n_draw, c->m, k, c->hyp, c->stream));
    if (c->m == 0) {
        // nothing to score (pre3_step skips the stage likewise): the one-column table of zeros is all there is
        if (support) for (int i = 0; i < n_draw; ++i) support[i] = -1;
        if (stats) { stats[0] = -1; stats[1] = stats[2] = stats[3] = 0; }
        return seeded_table_out(c, n_draw, k, hyp_out, k_out);
    }
    PRE3_TRY(ransac_impl(c, n_draw, k, nullptr, threshold, early_exit, support, li_mask, stats, true));
    return seeded_table_out(c, n_draw, k, hyp_out, k_out);
}

// ---- updates --------------------------------------------------------------------------------------
static int update_selected(pre3_ctx *c, int which_prior, int nsel, const int32_t *sel_dev, bool gathered = false, bool first_done = false)
{
    PRE3_CHECK(c->p_which == which_prior, PRE3_E_STATE, "update: the covariance buffer does not hold the required prior");
    int r = 2 * nsel;
    // rows of the predicted-state update that RANSAC already multiplied out: gather instead of recomputing
    const bool reuse = r > 0 && which_prior == PRE3_X_K_KM1 && c->hp_all_valid && sel_dev != nullptr;
    bool hp_built = false;
    if (reuse) { if (!gathered) PRE3_TRY(launch_gather_li(c, nsel, nsel, sel_dev, round_up(2 * c->m, NB))); }
    else if (r > 0) {
        // rows built on the fly inside the H*P launch (one launch instead of k_build_rows + k_ell_HP; PRE3_FUSE_ROWS=0: the two)
        if (knob::fuse_rows() && round_up(r, NB) <= c->rcap) { PRE3_TRY(launch_ell_HP_build_sel(c, nsel, sel_dev, c->W)); hp_built = true; }
        else PRE3_TRY(launch_build_rows_impl(c, nsel, sel_dev, round_up(r, NB)));
    }
    PRE3_TRY(run_update(c, which_prior, r, false, nullptr, reuse, first_done && reuse, hp_built));
    c->hp_all_valid = false;                 // P changed
    c->x_valid[PRE3_X_K_K] = true; c->p_which = PRE3_X_K_K;
    return PRE3_OK;
}

static int update_li_impl(pre3_ctx *c)
{
    PRE3_CHECK(c->measurements_set && c->projected, PRE3_E_STATE, "pre3_update_li: needs projection and measurements");
    int n_li = 0;       // no RANSAC / flags for this measurement set: no low-innovation inliers, update is the identity
    bool gathered = false, first_done = false;
    if (c->li_from_host >= 0) n_li = c->li_from_host;
    else if (c->li_kernel) {
        const Carried sel = c->carry;
        const bool fused_sel = sel.select_pending && c->p_which == PRE3_X_K_KM1 && c->hp_all_valid && c->m > 0;
        if (sel.select_pending && !fused_sel) PRE3_TRY(launch_ransac_select_impl(c, sel.sel_n_draw, sel.sel_k, sel.sel_early_exit, c->support, c->masks, ceil_div(c->m, 32)));
        c->carry.select_pending = false;
        // the gather of the LI rows does not need the count on the host: issue it first, with the grid sized for all
        // measurements, so that the GPU has work while the host polls the mailbox and launches the factorisation
        if (c->p_which == PRE3_X_K_KM1 && c->hp_all_valid && c->m > 0) {
            if (fused_sel) PRE3_TRY(launch_select_gather(c, sel.sel_n_draw, sel.sel_k, sel.sel_early_exit, ceil_div(c->m, 32)));
            else PRE3_TRY(launch_gather_li(c, -1, c->m, c->sel_rows, round_up(2 * c->m, NB)));
            gathered = true;
            // ... and so does the first panel of the factorisation (row count read on the device, grid sized for all measurements)
            if (knob::chol_spec0() && round_up(2 * c->m, NB) <= c->rcap) {
                // fp32: the whole factorisation + solve is ONE launch that reads the row count on the device (pre3_cholp.hip)
                if (cholp_usable(c, round_up(2 * c->m, NB) / NB)) {
                    // pre3_step: the rescue stage and the HI update ride in the same launch (mono_slam.m:184-187 as panel nrb of this factorisation)
                    CholpTailReq tail{ c->req.tail_chi2, c->seq_collect + 1 };
                    PRE3_TRY(launch_cholp(c, -1, round_up(2 * c->m, NB) / NB, -1, PRE3_X_K_KM1, c->req.tail_want ? &tail : nullptr));
                    if (c->out.tail_launched) ++c->seq_collect;
                }
                else PRE3_TRY(launch_chol_first_spec(c, c->m));
                first_done = true;
            }
        }
        PRE3_TRY(wait_mail(c, 8, c->seq_select)); n_li = c->mail_host[4];
        PRE3_CHECK(!c->shard_round || c->mail_host[11] == 0, PRE3_E_COMM, "sharded RANSAC: a rank failed before the collective of the round this update follows");
    }
    // (a launch that found no rows on the device returned at once: the tail has not run either)
    c->carry.tail_done = first_done && c->out.cholp_done && c->out.tail_launched && n_li > 0;
    const int rc = update_selected(c, PRE3_X_K_KM1, n_li, c->sel_rows, gathered, first_done);
    if (rc != PRE3_OK) c->carry.tail_done = false;      // (nothing that is carried comes out of an update that failed)
    return rc;
}
int pre3_update_li(pre3_ctx *c)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    return update_li_impl(c);
}

static int rescue_impl(pre3_ctx *c, double chi2, int32_t *hi_mask)
{
    if (c->N) {
        if (c->out.rescue_projected) PRE3_TRY(launch_innovation(c, 1, chi2));      // h / H at x_k_k came with the K9 launch
        else PRE3_TRY(launch_project_innovation(c, PRE3_X_K_K, 0, 1, chi2));
    }
    c->hi_from_host = -1; c->hi_kernel = true;
    if (hi_mask) {
        PRE3_TRY(stream_drain(c, __func__));
        if (c->m) PRE3_HIP(hipMemcpy(hi_mask, c->hi_meas, sizeof(int32_t) * c->m, hipMemcpyDeviceToHost));
    }
    return PRE3_OK;
}

// record: a booked context records what rescue_hi_inliers.m:32 projects (pre3_map_policy's times_predicted), at the x_k_k this projection uses
// (pre3_step records it itself, in front of whichever rescue form it takes)
static int rescue_checked(pre3_ctx *c, double chi2, int32_t *hi_mask, bool record)
{
    PRE3_CHECK(c->p_which == PRE3_X_K_K && c->x_valid[PRE3_X_K_K], PRE3_E_STATE, "pre3_rescue: needs (x_k_k, p_k_k), i.e. after the LI update");
    if (record && c->booked && c->m > 0 && c->N > 0) PRE3_TRY(launch_book_vis(c));
    return rescue_impl(c, chi2, hi_mask);
}
int pre3_rescue(pre3_ctx *c, double chi2, int32_t *hi_mask)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    return rescue_checked(c, chi2, hi_mask, true);
}

}  // extern "C"
int pre3::update_hi_impl(pre3_ctx *c)
{
    int n_hi = 0;
    const bool tail_done = c->carry.tail_done, was_fused = c->carry.hi_fused, pend_launched = c->carry.hi_pend_launched;
    c->carry.tail_done = false; c->carry.hi_fused = false; c->carry.hi_pend_launched = false;      // (taken: before anything can return)
    if (c->hi_from_host >= 0) n_hi = c->hi_from_host;
    else if (c->hi_kernel) {
        PRE3_TRY(wait_mail(c, 9, c->seq_collect)); n_hi = c->mail_host[5];
        // the collection stage also brings the device's error words: what went wrong in this step's launches fails THIS call -- once: the words
        // are cleared with the report, so that a context that installs a fresh state (pre3_set_state) works again
        const int e_wait = c->mail_host[7], e_npd = c->mail_host[6];
        if (e_wait != 0 || e_npd != 0) {
            c->mail_host[6] = 0; c->mail_host[7] = 0;
            (void)hipMemsetAsync(c->stats + 6, 0, sizeof(int32_t) * 2, c->stream);
        }
        PRE3_CHECK(e_wait == 0, PRE3_E_HIP, "a device-side wait on another workgroup gave up (counter never arrived): results are invalid");
        PRE3_CHECK(e_npd == 0, PRE3_E_NUMERIC, "%s", numeric_word_message(e_npd));
    }
    if (tail_done) {
        // The persistent launch of the LI update has run the rescue stage and (up to 32 landmarks) the HI update as well (pre3_cholp.hip, CpTail):
        // P holds P - W'W - W~'W~ and update.m:42-46 of BOTH updates is one pending rows / columns 3..6 pass (params[16..] = params[96..] = J2 J1,
        // or J1 alone when nothing was updated).  More than 32: that pass now (J1), then the general path.
        c->hp_all_valid = false;
        if (c->hi_from_host < 0 && n_hi <= 32) {
            if (c->req.leave_jn_to_predict) c->carry.jn_pending = true;
            else PRE3_TRY(launch_jnorm(c, 0));
            return PRE3_OK;
        }
        PRE3_TRY(launch_jnorm(c, 0));
        return update_selected(c, PRE3_X_K_K, n_hi, c->sel_rows);
    }
    if (was_fused) {
        // pre3_step sent the collection and the update out as one device-driven pair of launches (k_hi_fused + its down-date): up to 64
        // landmarks (two panels) are done, only the Jnorm pass of update.m:42-46 is left; more than that take the general path now
        if (c->hi_from_host < 0 && n_hi <= hi_fused_max(c)) {
            if (n_hi > 0) {
                c->hp_all_valid = false;
                // PRE3_OPT_PEND_HI: k_hi_fused's down-date was not launched -- from here on P stands for P - W~'W~ (2 n_hi rows) until somebody takes it
                if (pend_launched) {
                    c->carry.pend_rows = 2 * n_hi;
                    // (two panels of pending rows cost the next H*P launch ~19 us more, one panel ~5: sending the two-panel ones out at once -- PRE3_PEND_MAX_ROWS=64 --
                    //  measured 5922 against 5954 steps/s: the launch they then need costs as much)
                    if (c->carry.pend_rows > knob::pend_max_rows()) PRE3_TRY(pend_flush(c));
                }
                if (c->req.leave_jn_to_predict) c->carry.jn_pending = true;
                else PRE3_TRY(launch_jnorm(c, 0));              // (flushes the pending rows first: the pass reads P)
            }
            return PRE3_OK;
        }
        // (more than k_hi_fused takes: it has written nothing -- no W~, no x-update --, the general path follows)
    }
    return update_selected(c, PRE3_X_K_K, n_hi, c->sel_rows);
}
extern "C" {

int pre3_update_hi(pre3_ctx *c)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    return update_hi_impl(c);
}

int pre3_update_all(pre3_ctx *c)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    PRE3_CHECK(c->measurements_set && c->projected, PRE3_E_STATE, "pre3_update_all: needs projection and measurements");
    return update_selected(c, PRE3_X_K_KM1, c->m, nullptr);
}

// ---- update.m on the resident current estimate (pre3_rows.hip) -------------------------------------------------------------
// The host checks of both calls, before anything is launched
static int rows_precheck(pre3_ctx *c, const char *who)
{
    PRE3_CHECK(c != nullptr, PRE3_E_ARG, "null context");
    PRE3_CHECK(c->x_valid[PRE3_X_K_K] && c->p_which == PRE3_X_K_K, PRE3_E_STATE,
               "%s: acts on (x_k_k, p_k_k); the covariance buffer holds the prediction (update first)", who);
    return PRE3_OK;
}

int pre3_update_rows(pre3_ctx *c, int r, int width, const int32_t *nnz, const int32_t *col, const double *val, const double *R, const double *z,
                     const double *h)
{
    PRE3_CHECK(c != nullptr, PRE3_E_ARG, "null context");
    PRE3_CHECK(r >= 0, PRE3_E_ARG, "pre3_update_rows: r=%d", r);
    PRE3_CHECK(round_up(r, NB) <= c->rcap, PRE3_E_ARG, "pre3_update_rows: %d rows exceed the context's capacity %d", r, c->rcap);
    PRE3_CHECK(r == 0 || (nnz && col && val && z && h && width >= 1), PRE3_E_ARG, "pre3_update_rows: null row data");
    for (int a = 0; a < r; ++a) {
        PRE3_CHECK(nnz[a] >= 0 && nnz[a] <= width && nnz[a] <= ELLW, PRE3_E_ARG, "pre3_update_rows: row %d has %d non-zeros (max %d)", a, nnz[a], ELLW);
        for (int t = 0; t < nnz[a]; ++t)
            PRE3_CHECK(col[(size_t)a * width + t] >= 0 && col[(size_t)a * width + t] < c->n, PRE3_E_ARG,
                       "pre3_update_rows: column index %d out of range (n=%d) in row %d", col[(size_t)a * width + t], c->n, a);
    }
    PRE3_TRY(rows_precheck(c, "pre3_update_rows"));
    EntryScope scope(c); PRE3_TRY(scope.rc);
    if (r == 0) return PRE3_OK;                 // update.m:50-55
    if (r <= RMAX) {
        // the single-sweep form (pre3_rows.hip)
        RowsBlock b{};
        b.r = r; b.applied = 1;
        for (int a = 0; a < r; ++a) {
            for (int t = 0; t < nnz[a]; ++t) { b.col[a * RMAX + t] = col[(size_t)a * width + t]; b.val[a * RMAX + t] = val[(size_t)a * width + t]; }
            b.nu[a] = z[a] - h[a];
            for (int e = 0; e < r; ++e) b.R[a * r + e] = R ? R[(size_t)a * r + e] : (a == e ? 1.0 : 0.0);
        }
        c->rows_form = 1;
        PRE3_TRY(launch_rows_update(c, &b, nullptr));
        c->hp_all_valid = false;
        return PRE3_OK;
    }
    // above RMAX rows: the rows as pre3_update_ell installs them, then the existing route (run_update) in place on x_k_k / p_k_k
    const int r_pad = round_up(r, NB);
    std::vector<int32_t> hc((size_t)r_pad * ELLW, 0);
    std::vector<double> hv((size_t)r_pad * ELLW, 0.0), nu(r_pad, 0.0);
    for (int a = 0; a < r; ++a) {
        for (int t = 0; t < nnz[a]; ++t) { hc[(size_t)a * ELLW + t] = col[(size_t)a * width + t]; hv[(size_t)a * ELLW + t] = val[(size_t)a * width + t]; }
        nu[a] = z[a] - h[a];
    }
    PRE3_HIP(hipMemcpyAsync(c->row_col, hc.data(), sizeof(int32_t) * hc.size(), hipMemcpyHostToDevice, c->stream));
    std::vector<float> hf, rf;
    if (c->dtype == PRE3_F64) PRE3_HIP(hipMemcpyAsync(c->row_val, hv.data(), sizeof(double) * hv.size(), hipMemcpyHostToDevice, c->stream));
    else { hf.assign(hv.begin(), hv.end()); PRE3_HIP(hipMemcpyAsync(c->row_val, hf.data(), sizeof(float) * hf.size(), hipMemcpyHostToDevice, c->stream)); }
    PRE3_HIP(hipMemcpyAsync(c->row_nu, nu.data(), sizeof(double) * r_pad, hipMemcpyHostToDevice, c->stream));
    if (R) {
        if (c->Rdense == nullptr) PRE3_TRY(dmalloc_bytes(c, &c->Rdense, (size_t)c->rcap * c->rcap * c->esz));
        if (c->dtype == PRE3_F64) PRE3_HIP(hipMemcpyAsync(c->Rdense, R, sizeof(double) * r * r, hipMemcpyHostToDevice, c->stream));
        else { rf.assign(R, R + (size_t)r * r); PRE3_HIP(hipMemcpyAsync(c->Rdense, rf.data(), sizeof(float) * rf.size(), hipMemcpyHostToDevice, c->stream)); }
    }
    c->rows_form = 0;
    PRE3_TRY(run_update(c, PRE3_X_K_K, r, R != nullptr, nullptr));
    c->hp_all_valid = false;
    c->x_valid[PRE3_X_K_K] = true; c->p_which = PRE3_X_K_K;
    // (the host vectors may go: a copy from pageable memory has consumed its source when hipMemcpyAsync returns)
    return PRE3_OK;
}

int pre3_heading_update(pre3_ctx *c, const double R_plane[9], int strict_reference, int32_t *applied_out)
{
    PRE3_CHECK(c != nullptr && R_plane != nullptr, PRE3_E_ARG, "pre3_heading_update: null argument");
    for (int k = 0; k < 9; ++k) PRE3_CHECK(std::isfinite(R_plane[k]), PRE3_E_ARG, "pre3_heading_update: R_plane is not finite");
    PRE3_TRY(rows_precheck(c, "pre3_heading_update"));
    EntryScope scope(c); PRE3_TRY(scope.rc);
    RowsHeading hd{};
    hd.on = 1; hd.strict = strict_reference ? 1 : 0;
    for (int k = 0; k < 3; ++k) hd.z[k] = R_plane[3 + k];          // ekf_heading_update.m:29, z = R_plane(:, 2)
    heading_RR(R_plane, hd.RR);
    c->rows_form = 1;
    PRE3_TRY(launch_rows_update(c, nullptr, &hd));
    c->hp_all_valid = false;
    if (applied_out) {
        int32_t applied = 0;
        PRE3_HIP(hipMemcpyAsync(c->pinned_stats, c->stats, sizeof(int32_t) * 16, hipMemcpyDeviceToHost, c->stream));
        PRE3_TRY(rows_applied(c, &applied));
        PRE3_TRY(stream_drain(c, __func__));
        const int rc = stats_words(c);
        *applied_out = rc == PRE3_OK ? applied : 0;
        if (rc != PRE3_OK) {
            // reported once, as the step's collection reports them: the words are cleared with the report
            (void)hipMemsetAsync(c->stats + 6, 0, sizeof(int32_t) * 2, c->stream);
            c->mail_host[6] = 0; c->mail_host[7] = 0;
            PRE3_TRY(stream_drain(c, __func__));
        }
        return rc;
    }
    return PRE3_OK;
}

// mono_slam.m:178-187 behind the prediction and the IC search: RANSAC, LI update, rescue, HI update, every launch sized on the device.
// hyp: the draw table -- the inbox's own copy when it was shipped with the measurements (pre3_step), the caller's otherwise.
static int step_back(pre3_ctx *c, int m, int n_draw, int k, const int32_t *hyp, double threshold, int early_exit, double chi2, int32_t stats[8],
                     bool table_on_device = false)
{
    int32_t st[8] = { -1, 0, 0, 0, 0, 0, 0, 0 };
    bool ran = false;
    if (m >= k && m > 0) {
        // mono_slam.m:178; the statistics are read after pre3_update_li's poll of the same mailbox
        c->req.defer_select = true;                                 // the selection stage rides in the LI gather's launch (update_li_impl below)
        const int rc_r = ransac_impl(c, n_draw, k, hyp, threshold, early_exit, nullptr, nullptr, nullptr, table_on_device);
        if (c->req.ride_innovation && !c->out.innovation_rode) {    // the H*P launch did not go out (error before it): S_i on its own, flags cleared
            c->req.ride_innovation = false;
            PRE3_TRY(launch_innovation(c, 0, 0.0, true));
        }
        PRE3_TRY(rc_r);
        ran = true;
    }
    const int ride_rescue = knob::ride_rescue();
    c->req.ride_rescue_projection = ride_rescue != 0;               // the rescue's projection rides in the LI update's K9 launch
    {
        // ... or, with the whole rescue stage and the HI update, in the persistent launch itself (not on a booked context: the rescue's visibility
        // record needs the point between the LI update and the rescue, which that form does not have -- the step takes the default form)
        c->req.tail_want = c->step_tail && !c->booked && hi_fused_usable(c); c->req.tail_chi2 = chi2;
        // ... or projection AND chi2 gate in the Jnorm pass's launch, when the persistent launch's consumers leave rows 3..6 of P behind (GateRide)
        c->req.want_gate_ride = ride_rescue != 0 && !c->req.tail_want && hi_fused_usable(c); c->req.rescue_chi2 = chi2;
        PRE3_TRY(update_li_impl(c));                                // mono_slam.m:181
        // (asked of the LI update's launches only: the HI update's K9 launch carries no riders)
        c->req.tail_want = false; c->req.want_gate_ride = false; c->req.ride_rescue_projection = false;
    }
    if (ran) for (int i = 0; i < 4; ++i) st[i] = c->mail_host[i];
    // a booked context: visibility at the post-LI x_k_k, where rescue_hi_inliers.m:32 projects -- one small launch in stream order between the LI
    // update and the rescue / HI update (also under PRE3_OPT_DEFER_HI / PEND_HI, which only move the HI update later); only when the reference's
    // rescue runs ('1PRE' with at least one IC measurement, mono_slam.m:165)
    if (c->booked && m > 0 && c->N > 0 && !c->carry.tail_done) PRE3_TRY(launch_book_vis(c));
    if (c->carry.tail_done) {
        // mono_slam.m:184 + :187 went out with the LI update's launch: the count arrives with mailbox word 9 (update_hi_impl)
        c->hi_from_host = -1; c->hi_kernel = true; c->carry.hi_fused = false;
    } else if (hi_fused_usable(c)) {
        // mono_slam.m:184 + :187 without the host in between: the chi2 gate, then the collection and the HI update of up to 32 landmarks as ONE
        // launch that reads the count on the device, and its down-date behind it (pre3_update.hip, k_hi_fused)
        PRE3_CHECK(c->p_which == PRE3_X_K_K && c->x_valid[PRE3_X_K_K], PRE3_E_STATE, "pre3_step: the LI update did not leave (x_k_k, p_k_k)");
        if (c->out.rescue_gated) { /* the gate rode with the Jnorm pass */ }
        else if (c->out.rescue_projected) PRE3_TRY(launch_innovation(c, 1, chi2, false, false));
        else PRE3_TRY(launch_project_innovation(c, PRE3_X_K_K, 0, 1, chi2, false));
        c->hi_from_host = -1; c->hi_kernel = true;
        PRE3_TRY(launch_hi_fused(c, ++c->seq_collect));
        c->carry.hi_fused = true;
    } else
    PRE3_TRY(rescue_checked(c, chi2, nullptr, false));             // mono_slam.m:184
    if (c->defer_hi) c->carry.hi_pending = true;                    // mono_slam.m:187, completed at the next call on this context
    else PRE3_TRY(update_hi_impl(c));                               // mono_slam.m:187
    st[4] = c->li_from_host >= 0 ? c->li_from_host : (c->li_kernel ? c->mail_host[4] : 0);
    st[5] = c->defer_hi ? c->carry.last_n_hi : (c->hi_from_host >= 0 ? c->hi_from_host : (c->hi_kernel ? c->mail_host[5] : 0));
    st[7] = c->defer_hi ? 1 : 0;          // 1: st[5] is the HI count of the PREVIOUS step (this step's is still on the device)
    if (stats) for (int i = 0; i < 8; ++i) stats[i] = st[i];
    return PRE3_OK;
}

// ds != null: the seeded form -- no table in the inbox; k_draw_1p writes c->hyp behind the prediction's launch (whose inbox pull covers that region)
static int step_front(pre3_ctx *c, const double u[7], int m, const int32_t *meas_idx, const double *z, int n_draw, int k, const int32_t *hyp,
                      double threshold, int early_exit, double chi2, int32_t stats[8], const DrawSeed *ds)
{
    // Entry::step: the previous step's deferred HI update is completed here; its rows/cols 3..6 <- Jn pass (update.m:42-46) is left to the prediction's
    // launch below (one launch less per step; PRE3_FUSE_JN=0: as its own launch).  Any return before that launch flushes it.
    // (a pass a marginal reader has left pending since -- it completed the update -- rides the same way)
    // PRE3_OPT_PEND_HI (pend_keep): this call's own launches take a pending HI down-date along (prediction, H*P + S_i, the LI update's consumers); whatever
    // of it cannot -- and every launch made from in here that reads P some other way -- flushes it first (pend_flush in the launchers)
    EntryScope scope(c, Entry::step, c && c->pend_opt && c->dtype == PRE3_F32 && m >= k && m > 0 && c->N > 0); PRE3_TRY(scope.rc);
    const bool trace = knob::step_trace();
    static double acc[8], t_prev_end = 0; static int nacc = 0;
    auto now = [] { timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec * 1e6 + t.tv_nsec * 1e-3; };
    double t0 = trace ? now() : 0, t1 = 0, t5 = 0;
    PRE3_CHECK(u != nullptr, PRE3_E_ARG, "pre3_step: null u");
    PRE3_CHECK(c->have_cam, PRE3_E_STATE, "pre3_step: camera not set");
    PRE3_CHECK(c->x_valid[PRE3_X_K_K] && c->p_which == PRE3_X_K_K, PRE3_E_STATE, "pre3_step: needs (x_k_k, p_k_k) on the device");
    PRE3_CHECK(m == 0 || (meas_idx && z), PRE3_E_ARG, "pre3_step: null measurement pointers");
    PRE3_CHECK(n_draw >= 1 && n_draw <= c->caph && k >= 1 && k <= MAXK && (hyp || ds), PRE3_E_ARG, "pre3_step: bad hypothesis table");
    // matching_sift_based.m:131-134 outcome (+ the draws) into the pinned inbox; it crosses PCIe in one extra block of the prediction's
    // launch (nothing in that launch reads it), so the copy costs neither a launch nor stream time.  Flags cleared by k_innovation.
    size_t inbox_bytes = 0;
    PRE3_TRY(install_measurements(c, m, meas_idx, z, ds ? nullptr : hyp, ds ? 0 : n_draw * k, c->N > 0, false, &inbox_bytes));
    // mono_slam.m:153 + search_IC_matches.m:31-32: prediction, with the projection of every landmark at x_k_km1 riding in the
    // same launch; then search_IC_matches.m:33-44 (S_i), which also clears the previous frame's inlier flags
    {
        const int ride_proj = knob::ride_proj();
        const int rc_p = launch_predict_impl(c, u, ride_proj != 0, (inbox_bytes + 15) / 16, ++c->seq_inbox);
        c->inbox_pending = rc_p == PRE3_OK;
        if (rc_p != PRE3_OK) { c->measurements_set = false; return rc_p; }
        if (!ride_proj && c->N) PRE3_TRY(launch_project(c, PRE3_X_K_KM1, 1));
    }
    c->x_valid[PRE3_X_K_KM1] = true; c->p_which = PRE3_X_K_KM1; c->hp_all_valid = false;
    c->projected = true;
    // S_i (which also clears last frame's inlier flags) rides in the H*P launch of the RANSAC stage when there is one
    c->req.ride_innovation = knob::ride_innov() && c->N > 0 && m >= k && m > 0;
    if (c->N && !c->req.ride_innovation) PRE3_TRY(launch_innovation(c, 0, 0.0, true));
    c->innovated = true;
    if (trace) t1 = now();
    if (ds) PRE3_TRY(launch_draw_1p(ds->seed, ds->seq, n_draw, m, k, c->hyp, c->stream));
    const int rc_back = step_back(c, m, n_draw, k, ds ? nullptr : (const int32_t *)(c->inbox_host + c->off_hyp), threshold, early_exit, chi2, stats, ds != nullptr);
    if (trace) {
        t5 = now();
        acc[0] += t1 - t0; acc[1] += t5 - t1;
        if (t_prev_end > 0) acc[5] += t0 - t_prev_end;
        t_prev_end = t5;
        if (++nacc == 100) {
            fprintf(stderr, "[pre3 step trace, us] predict+project+innov launches %.1f | ransac .. HI update (polls + launches) %.1f | caller between steps %.1f\n",
                    acc[0] / nacc, acc[1] / nacc, acc[5] / nacc);
            nacc = 0; for (double &a2 : acc) a2 = 0;
        }
    }
    return rc_back;
}

int pre3_step(pre3_ctx *c, const double u[7], int m, const int32_t *meas_idx, const double *z, int n_draw, int k, const int32_t *hyp,
              double threshold, int early_exit, double chi2, int32_t stats[8])
{
    return step_front(c, u, m, meas_idx, z, n_draw, k, hyp, threshold, early_exit, chi2, stats, nullptr);
}

int pre3_step_seeded(pre3_ctx *c, const double u[7], int m, const int32_t *meas_idx, const double *z, uint64_t seed, uint64_t seq, int n_draw,
                     double threshold, int early_exit, double chi2, int32_t *hyp_out, int32_t *k_out, int32_t stats[8])
{
    PRE3_CHECK(c != nullptr, PRE3_E_ARG, "null context");
    PRE3_CHECK(n_draw >= 1 && n_draw <= c->caph, PRE3_E_ARG, "pre3_step_seeded: n_draw=%d outside [1, %d]", n_draw, c->caph);
    PRE3_CHECK(u != nullptr && m >= 0 && (m == 0 || (meas_idx && z)), PRE3_E_ARG, "pre3_step_seeded: null argument");
    const DrawSeed ds{ seed, seq };
    const int k = seeded_k(m);
    PRE3_TRY(step_front(c, u, m, meas_idx, z, n_draw, k, nullptr, threshold, early_exit, chi2, stats, &ds));
    return seeded_table_out(c, n_draw, k, hyp_out, k_out);
}

/* mono_slam.m:153-162 + :199 -- the 'PURE_EKF' branch (config_file.m:21): prediction, projection + Jacobians + S_i of every landmark, then ONE
 * update with every individually compatible measurement (ekf_update_all.m:46-62), as one call: the projection and the inbox ride in the
 * prediction's launch, S_i and the flag clearing in the H*P launch -- four launches fewer than the call-by-call sequence
 * (pre3_predict, pre3_project, pre3_innovation, pre3_set_measurements, pre3_update_all), the same arithmetic. */
int pre3_step_all(pre3_ctx *c, const double u[7], int m, const int32_t *meas_idx, const double *z)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    PRE3_CHECK(u != nullptr, PRE3_E_ARG, "pre3_step_all: null u");
    PRE3_CHECK(c->have_cam, PRE3_E_STATE, "pre3_step_all: camera not set");
    PRE3_CHECK(c->x_valid[PRE3_X_K_K] && c->p_which == PRE3_X_K_K, PRE3_E_STATE, "pre3_step_all: needs (x_k_k, p_k_k) on the device");
    PRE3_CHECK(m == 0 || (meas_idx && z), PRE3_E_ARG, "pre3_step_all: null measurement pointers");
    size_t inbox_bytes = 0;
    PRE3_TRY(install_measurements(c, m, meas_idx, z, nullptr, 0, c->N > 0 && m > 0, false, &inbox_bytes));
    {
        const int rc_p = launch_predict_impl(c, u, true, (inbox_bytes + 15) / 16, ++c->seq_inbox);
        c->inbox_pending = rc_p == PRE3_OK;
        if (rc_p != PRE3_OK) { c->measurements_set = false; return rc_p; }
    }
    c->x_valid[PRE3_X_K_KM1] = true; c->p_which = PRE3_X_K_KM1; c->hp_all_valid = false;
    c->projected = true;
    c->req.ride_innovation = c->N > 0 && m > 0;      // S_i (and the clearing of last frame's flags) in the update's H*P launch
    if (c->N && !c->req.ride_innovation) PRE3_TRY(launch_innovation(c, 0, 0.0, true));
    c->innovated = true;
    PRE3_TRY(update_selected(c, PRE3_X_K_KM1, c->m, nullptr));
    if (c->req.ride_innovation && !c->out.innovation_rode) PRE3_TRY(launch_innovation(c, 0, 0.0, true));      // (the H*P launch did not go out: S_i on its own)
    return PRE3_OK;
}

/* The same behind a prediction and an IC search the caller has already run (mono_slam.m:153 ekf_prediction, :159 search_IC_matches +
 * matching_sift_based, e.g. pre3_predict + pre3_ic_search): the installed measurements are used. */
int pre3_step_predicted(pre3_ctx *c, int n_draw, int k, const int32_t *hyp, double threshold, int early_exit, double chi2, int32_t stats[8])
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    PRE3_CHECK(c->x_valid[PRE3_X_K_KM1] && c->p_which == PRE3_X_K_KM1, PRE3_E_STATE, "pre3_step_predicted: needs the predicted estimate (pre3_predict)");
    PRE3_CHECK(c->measurements_set && c->projected && c->innovated, PRE3_E_STATE, "pre3_step_predicted: needs projection, S_i and measurements (pre3_ic_search, or pre3_project + pre3_innovation + pre3_set_measurements)");
    PRE3_CHECK(n_draw >= 1 && n_draw <= c->caph && k >= 1 && k <= MAXK && hyp, PRE3_E_ARG, "pre3_step_predicted: bad hypothesis table");
    return step_back(c, c->m, n_draw, k, hyp, threshold, early_exit, chi2, stats);
}

int pre3_step_predicted_seeded(pre3_ctx *c, uint64_t seed, uint64_t seq, int n_draw, double threshold, int early_exit, double chi2, int32_t *hyp_out,
                               int32_t *k_out, int32_t stats[8])
{
    PRE3_CHECK(c != nullptr, PRE3_E_ARG, "null context");
    PRE3_CHECK(n_draw >= 1 && n_draw <= c->caph, PRE3_E_ARG, "pre3_step_predicted_seeded: n_draw=%d outside [1, %d]", n_draw, c->caph);
    EntryScope scope(c); PRE3_TRY(scope.rc);
    PRE3_CHECK(c->x_valid[PRE3_X_K_KM1] && c->p_which == PRE3_X_K_KM1, PRE3_E_STATE, "pre3_step_predicted_seeded: needs the predicted estimate (pre3_predict)");
    PRE3_CHECK(c->measurements_set && c->projected && c->innovated, PRE3_E_STATE, "pre3_step_predicted_seeded: needs projection, S_i and measurements (pre3_ic_search, or pre3_project + pre3_innovation + pre3_set_measurements)");
    const int k = seeded_k(c->m);
    PRE3_TRY(launch_draw_1p(seed, seq, n_draw, c->m, k, c->hyp, c->stream));
    PRE3_TRY(step_back(c, c->m, n_draw, k, nullptr, threshold, early_exit, chi2, stats, true));
    return seeded_table_out(c, n_draw, k, hyp_out, k_out);
}

}  // extern "C"
