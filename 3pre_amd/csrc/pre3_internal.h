// pre3_internal.h -- shared host-side declarations of libpre3.so (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/pre3.h"
#include "pre3_knobs.h"
#include "pre3_own.h"

namespace pre3 {

void set_error(const char *fmt, ...);

#define PRE3_HIP(call)                                                                         \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess) {                                                                \
            pre3::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return PRE3_E_HIP;                                                                 \
        }                                                                                      \
    } while (0)

#define PRE3_CHECK(cond, status, ...)                                                          \
    do {                                                                                       \
        if (!(cond)) { pre3::set_error(__VA_ARGS__); return (status); }                        \
    } while (0)

#define PRE3_TRY(expr)                                                                         \
    do { int rc_ = (expr); if (rc_ != PRE3_OK) return rc_; } while (0)

static inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
static inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }      // offsets inside a work block: 16-byte aligned

constexpr int TILE = 128;       // K9 output tile; P's leading dimension is a multiple of this
constexpr int NB = 64;          // Cholesky / triangular-solve panel width
constexpr int ELLW = 16;        // ELL width of measurement rows (7 pose + 6 landmark = 13 used)
constexpr int MAXK = 4;         // landmarks per RANSAC hypothesis (reference uses 3 or 1)

// one term of an ELL row product (k_ell_G and everything that restates its sums entry by entry: the scorer, the LI gather): an explicit fma,
// so that every kernel holding that sum rounds it the same way
#ifdef __HIPCC__
__device__ __forceinline__ float ell_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double ell_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
#endif

// flags of the per-landmark table
struct LmBuffers {
    int32_t *type = nullptr, *off = nullptr;          // [N]
    double *h = nullptr;                              // [2N]
    int32_t *has_h = nullptr;                         // [N]
    double *Hc = nullptr, *Hl = nullptr;              // [14N], [12N]
    double *S = nullptr;                              // [4N]
    int32_t *has_S = nullptr;                         // [N]
    double *z = nullptr;                              // [2N]
    int32_t *ic = nullptr, *li = nullptr, *hi = nullptr;   // [N]
};

// the small-rank update of pre3_update_rows / pre3_heading_update (pre3_rows.hip): r <= RMAX rows in ELL form (RMAX entries per row), all fp64
constexpr int RMAX = 16;
struct RowsBlock {
    int32_t r, applied, pad_[2];    // applied: 0 = the heading gate returned (ekf_heading_update.m:42-44); written by the rows launch
    int32_t col[RMAX * RMAX];
    double val[RMAX * RMAX];
    double nu[RMAX];                // z - h
    double R[RMAX * RMAX];          // r x r, leading dimension r
    double q[4];                    // x_k_k(4:7) before the update (the sweep writes x)
};
// what the plane fit's launch leaves for the heading update queued behind it (pre3_heading_from_scan, pre3_plane.hip): sta != 1 -> the gate word is cleared
struct HeadingSrc { double z[3]; double RR[9]; int32_t sta, pad_; };
struct RowsHeading { int on, strict; double z[3]; double RR[9]; const HeadingSrc *src; };    // ekf_heading_update.m:29, :37-40 (RR row-major); src != null: z, RR from the device block

struct KernelTiming {
    bool enabled = false;
    int every = 1, seen = 0;        // bracket one K9 launch out of `every` (an event pair costs ~11 us of stream time)
    std::vector<hipEvent_t> ev;     // pairs
    int used = 0;
    double flops = 0, bytes = 0;
    // launches of the persistent factorisation that carry the down-date (pre3_cholp.hip) are bracketed instead of the K9 launch they replace:
    // `flops` keeps the SYRK count of those updates, `fact_flops` the factorisation + solve the same launch executes (r^3/3 + n r^2)
    int fused = 0; double fact_flops = 0; bool pending = false;     // pending: a bracketed launch whose row count the host does not know yet
};

}  // namespace pre3

// ---- hand-offs between the host stages of one API call.  W: who writes, R: who reads.
// What the current entry point asks the launchers below it to carry.  Written by extern "C" entry points, step_back and EntryScope; read-only for launchers.
struct StepRequest {
    bool leave_jn_to_predict = false;      // W EntryScope (step, readers) while it completes a deferred HI update | R update_hi_impl, run_update, flush_unless_kept
    bool pend_keep = false;                // W EntryScope (step): this call's launches take a pending HI down-date along | R flush_unless_kept
    bool defer_select = false;             // W step_back: the selection stage rides in the LI gather's launch | R ransac_impl
    bool ride_innovation = false;          // W pre3_step, pre3_step_all: S_i goes out with the next H*P build launch | R launch_ell_HP_build(_sel)
    bool ride_rescue_projection = false;   // W step_back: the LI update's K9 launch also projects at x_k_k | R launch_downdate
    bool want_gate_ride = false; double rescue_chi2 = 0.0;   // W step_back: projection AND chi2 gate in the Jnorm pass's launch (GateRide) | R launch_cholp, launch_jnorm
    bool tail_want = false; double tail_chi2 = 0.0;          // W step_back: the LI update's persistent launch carries the tail (CpTail) | R update_li_impl
    const int32_t *book_from = nullptr;    // W pre3_map_policy: the updated counters the map re-layout reads instead of book | R apply_map
};
// What the launchers of the current call report back.  Written by launchers only; everybody else reads it or resets it whole.
struct LaunchOutcome {
    bool innovation_rode = false;          // W launch_ell_HP_build(_sel): S_i went out with this launch | R the same (once per call), step_back, pre3_step_all
    bool rescue_projected = false;         // W launch_downdate, launch_jnorm: h / H at the current x_k_k are on the device | R the same (once per call), rescue_impl, step_back
    bool proj_with_jnorm = false;          // W launch_downdate: no K9 launch was left, the projection rides in the next k_jnorm_P | R launch_jnorm (clears), run_update
    bool rescue_gated = false;             // W launch_jnorm: the chi2 gate rode with the Jnorm pass | R step_back
    bool cholp_done = false;               // W launch_cholp: the speculative launch has factored and solved | R update_li_impl, launch_chol_solve (clears)
    bool tail_launched = false;            // W launch_cholp: that launch carried the tail | R update_li_impl
    bool x_done = false;                   // W launch_cholp: its strips have computed x_k_k | R launch_downdate (clears)
    bool jn_q_valid = false;               // W launch_cholp: its consumers left the un-normalised rows 3..6 of P in jn_q | R launch_jnorm (clears)
    bool proj_in_cholp = false;            // W launch_cholp: its strips projected every landmark at x_k_k | R launch_jnorm (clears)
    int dd_done = 0;                       // W launch_cholp: groups its consumers have down-dated | R launch_downdate (clears)
    int split_rows = 0;                    // W launch_cholp, launch_chol_solve: rows of W whose bf16 planes exist | R launch_downdate (clears)
};
// Work one API call leaves for the next.  drop_carried() is the only reset (pre3_set_state).
struct Carried {
    bool hi_pending = false;               // W step_back (PRE3_OPT_DEFER_HI) | R EntryScope: completed by whatever call comes next
    int last_n_hi = 0;                     // W EntryScope: the HI count of the deferred update it completed | R step_back (stats[5] under PRE3_OPT_DEFER_HI)
    bool jn_pending = false;               // W update_hi_impl, run_update: a rows/cols 3..6 <- Jn pass waits for the next k_predict | R launch_predict_impl (takes it), EntryScope, readers
    int pend_rows = 0;                     // W update_hi_impl (PRE3_OPT_PEND_HI): P stands for P - W~'W~ | R pend_args, pend_flush, launch_cholp (take them)
    bool hi_pend_launched = false;         // W launch_hi_fused: W~ went to the pending buffers, no down-date launched | R update_hi_impl
    bool hi_fused = false;                 // W step_back: collection + HI update went out as k_hi_fused | R update_hi_impl
    bool tail_done = false;                // W update_li_impl: the tail ran inside the LI update's launch | R run_update, step_back, update_hi_impl
    bool select_pending = false; int sel_n_draw = 0, sel_k = 0, sel_early_exit = 0;   // W ransac_impl: the selection is still to be launched | R update_li_impl; install_measurements drops it
};

namespace pre3 { struct PatchState; struct FastState; }
// Every device and pinned block of a context (pre3_own.h).  `fixed`: what lives as long as the context and never grows -- the
// typed pointers of pre3_ctx point into it.  The rest grows on demand.  pre3_destroy releases all of it by assigning an empty one.
struct CtxMemory {
    pre3::BlockList fixed;
    pre3::StageRing up_ring, map_ring;                          // pinned staging of uploads (mailbox words 16, 17) and of map management (18, 19)
    pre3::DevBlock scan_desc, scan_pos, ic_pb, ic_ps, ic_pa;    // scan_reserve
    pre3::DevBlock mset_dev; pre3::PinBlock mset_host;          // read_marginal: the index-set block and its pinned image, grown with k
    pre3::DevBlock plane_buf;                                   // pre3_heading_from_scan's work block
    pre3::DevBlock pol_dev; pre3::PinBlock pol_host;            // the map policy's scratch and its mapped result block
};
struct pre3_ctx {
    int device = 0, dtype = PRE3_F32;
    size_t esz = 4;
    hipStream_t stream = nullptr;
    int capN = 0, capn = 0, capm = 0, caph = 0;
    int N = 0, n = 0;
    int ld = 0;                 // leading dimension of P (multiple of TILE), rows/cols >= n are zero
    int ldw = 0;                // leading dimension of the row workspace W/HP: ld + NB (column `ld` carries nu)
    int rcap = 0;               // max update rows (2*capm rounded to NB)
    pre3_cam cam{};
    bool have_cam = false;
    // device state
    double *x_kk = nullptr, *x_km1 = nullptr;     // [capn]
    void *P = nullptr;                            // [ld*ld] T
    void *tiles = nullptr;                        // int2[n_tiles]: (I,J) of every 64x64 upper-triangle tile, XCD-aware order
    int n_tiles = 0;
    void *tiles_flat = nullptr;                   // int2[n_tiles]: the 8 lists interleaved (block b -> list b % 8) for the one-tile kernel
    unsigned int *tile_ctr = nullptr;             // device ticket counter of the persistent K9 grid
    int *tile_cnt = nullptr; int tiles_stride = 0;  // per-list lengths [8] and list stride
    bool tile_ctr_clean = false;                  // the 8 counters are zero (k_update_x resets them ahead of K9)
    int num_cus = 256;
    void *Wp = nullptr;                           // fp32 path: bf16 planes of W in stage-image order (k_split_w), ld x rcap x 6 B
    bool k9_b3 = false;                           // fp32: K9 as three-way bf16 split on the bf16 matrix cores (PRE3_K9_B3=0 turns it off)
    void *Sp = nullptr;                           // fp32 path: bf16 planes of the factorisation's S blocks (pending updates), rcap/64 x rcap/64 x 24 KB
    void *tiles128 = nullptr; int n_tiles128 = 0; // int2[n_tiles128]: 128x128 upper-triangle tiles of k_downdate_b3, XCD-interleaved
    unsigned int *chol_arrive = nullptr; unsigned int chol_target = 0;   // [0] panel arrivals, [1],[2] unused, [3],[4] rider producers
    unsigned int ride_target[2] = { 0, 0 };
    void *comm = nullptr; bool comm_owned = false;                 // RCCL communicator (pre3_comm.hip): pre3_comm_init / pre3_set_comm
    StepRequest req; LaunchOutcome out; Carried carry;             // the hand-offs of a call: see the three structs above
    bool defer_hi = false;                                         // PRE3_OPT_DEFER_HI (pre3_set_option)
    int p_which = -1;                             // which estimate P currently holds (-1: none)
    bool x_valid[2] = {false, false};
    pre3::LmBuffers lm;
    // measurements (host mirrors kept: m and the index list are host-known)
    int m = 0;
    std::vector<int32_t> meas_host;
    int32_t *meas = nullptr;                      // [capm] landmark index per measurement
    // measurement-row workspace
    int32_t *row_col = nullptr;                   // [rcap*ELLW]
    void *row_val = nullptr;                      // [rcap*ELLW] T
    double *row_nu = nullptr;                     // [rcap]  z-h per row
    void *HP = nullptr;                           // [rcap*ldw] T   H*P for all measured rows (RANSAC)
    void *G = nullptr;                            // [rcap*rcap] T  H*P*H' (no +R)
    void *W = nullptr;                            // [rcap*ldw] T   update workspace: HP rows -> W = L^-1 HP
    void *Smat = nullptr;                         // [rcap*rcap] T  S -> L
    void *Rdense = nullptr;                       // [rcap*rcap] T  optional dense R (stateless update)
    int32_t *sel_rows = nullptr;                  // [rcap] compacted row list (indices into the measured rows)
    // RANSAC
    int32_t *hyp = nullptr;                       // [caph*MAXK]
    int32_t *support = nullptr;                   // [caph]
    uint32_t *masks = nullptr;                    // [caph*mask_words_cap]
    int mask_words_cap = 0;
    int scored_n_draw = 0, scored_k = 0;          // the round pre3_ransac_score / pre3_ransac laid the support + mask buffer out for
    int32_t *stats = nullptr;                     // [16] device: best, iters, n_hyp, max_support, n_li, n_hi, status
    int32_t *li_meas = nullptr, *hi_meas = nullptr;   // [capm] flags in measurement order
    double *pred_params = nullptr;                // [192] predict: Qq1(16) Jn(16) Q(49->7x7) etc.; [128 .. 176] the process noise block
    bool pn_set = false; double pn_host[49] = {};  // pre3_set_process_noise: the caller's Pn is in force (pre3_set_state does not reset it); its host copy
    int32_t *pinned_stats = nullptr;              // host pinned [16]
    // mailbox: pinned, host-coherent; the selection and HI-collection stages store their counts here and bump a
    // sequence word, so the host learns r for the next launches by polling instead of a copy + stream sync
    int32_t *mail_host = nullptr, *mail_dev = nullptr;
    int32_t seq_select = 0, seq_collect = 0;
    bool g_valid = false;                         // c->G holds H*P*H' of all measured rows (PRE3_INLINE_G=0); otherwise the scorer and the LI gather compute their entries
    int li_from_host = -1, hi_from_host = -1;     // row counts forced through pre3_set_flags (-1: use the kernels' counts)
    bool li_kernel = false, hi_kernel = false;    // a select / collect kernel has run for the current measurement set
    // per-step inbox: [meas | ic | hyp | z] contiguous on the device, mirrored in pinned host memory -> ONE H2D copy
    void *inbox_dev = nullptr; unsigned char *inbox_host = nullptr; void *inbox_host_dev = nullptr;   // pinned + device-mapped: the device address of inbox_host
    size_t inbox_bytes = 0, off_meas = 0, off_ic = 0, off_hyp = 0, off_z = 0, off_flags = 0, flags_bytes = 0;
    int32_t seq_inbox = 0;                        // sequence number of the last inbox pull (published by the kernel in mailbox word 10)
    bool inbox_pending = false;                   // a pull out of the pinned inbox may still be in flight (install_measurements waits before it overwrites)
    // map management (allocated on first use)
    void *P_alt = nullptr; double *x_alt = nullptr; int32_t *map_col = nullptr; void *map_val = nullptr; int32_t *map_desc = nullptr; int32_t *map_src0 = nullptr; double *map_conv = nullptr;
    double *map_feat = nullptr; int32_t *map_flags = nullptr;
    bool map_ready = false;                       // ensure_map_buffers' group is complete
    std::vector<int32_t> lm_type_host;
    // IC search (matching_sift_based.m): landmark descriptor bank [capN][128], the current scan's SIFT set, match scratch
    double *bank = nullptr, *bank_alt = nullptr; bool bank_set = false; bool ic_ready = false;      // ic_ready: ensure_ic_buffers' group is complete
    double *scan_desc = nullptr, *scan_pos = nullptr; int scan_K2 = 0, scan_cap = 0;
    // pinned staging of host arrays on their way to the device (the per-frame scan, descriptors of new landmarks): mem.up_ring's two blocks, used
    // alternately; the caller's data is copied (and bounds-checked) into a block, the device pulls it over PCIe on the context's stream --
    // no synchronisation, no read-back (pre3_api.hip: stage_acquire / stage_release)
    int32_t stage_seq[4] = { 0, 0, 0, 0 };          // sequence number of the last pull of staging block k (0, 1: uploads; 2, 3: map management)
    void *ic_result_host = nullptr, *ic_result_host_dev = nullptr; int32_t seq_ic = 0;    // the IC search's result block in mapped pinned memory: written by the device, announced through mailbox word 12
    int32_t *ic_pred = nullptr, *ic_counts = nullptr, *ic_arg = nullptr, *ic_pairs = nullptr, *ic_newk2 = nullptr; double *ic_best = nullptr, *ic_second = nullptr;
    int32_t *bank_src = nullptr;
    int ic_route = 0;                             // the last pre3_ic_search's matcher: 0 exact tiled kernel, 1 ranked (matrix cores), 2 fused small-problem route
    bool ic_last_ranked = false;                  // the last pre3_ic_search matched on the matrix cores (PRE3_OPT_IC_RANKED)
    void *ic_rank = nullptr; bool bank_ok = false;   // the scan packed for the matrix-core matcher (pre3_match.hip: IcRank); every bank descriptor inside its bounds
    size_t ic_pcap = 0;                           // elements in each of ic_pb / ic_ps / ic_pa
    double *ic_pb = nullptr, *ic_ps = nullptr; int32_t *ic_pa = nullptr;     // per (column tile, landmark) partials of the tiled matcher [scan_cap/64][capN]
    // timing
    hipEvent_t t0 = nullptr, t1 = nullptr;
    pre3::KernelTiming kt;
    bool measurements_set = false, projected = false, innovated = false;
    int32_t *need = nullptr; int need_tag = 0;    // [capm] sharded RANSAC: need[s] == need_tag where this rank's hypothesis slice draws measurement s
    // persistent factorisation (pre3_cholp.hip)
    unsigned int *cholp_flags = nullptr; void *cholp_tp = nullptr; unsigned int cholp_epoch = 0; bool chol_persist = true;
    bool cholp_counted = false;                   // this context is in pre3_cholp.hip's per-device count
    // down-date consumers inside the persistent factorisation (pre3_cholp.hip): group records, all tiles in group order, first tile per group
    int32_t *dd_groups = nullptr; int dd_n_groups = 0; void *dd_tiles = nullptr; std::vector<int> dd_tile_off;
    bool k9_overlap = true;                       // PRE3_OPT_K9_OVERLAP
    bool shard_round = false;                     // the last RANSAC round was pre3_ransac_sharded (its selection publishes the missing-slice word in mail[11])
    float *jn_q = nullptr;                        // un-normalised rows 3..6 of P, left by the persistent launch's consumers for the gate that rides with the Jnorm pass (GateRide)
    bool hp_all_valid = false;                    // HP / G hold H*P, H*P*H' of ALL measured rows at the current prior (ransac_prepare)
    // the rescue stage + HI update inside the persistent launch (pre3_cholp.hip, CpTail): per landmark the planes of y = H J W' and the row H J;
    // crit's published list
    void *tail_yp = nullptr; float *tail_hb = nullptr; int32_t *tail_hib = nullptr; float *tail_wt = nullptr;
    // PRE3_OPT_PEND_HI (PendW, pre3_geomdev.h): k_hi_fused's W~ goes to its own buffers and the down-date is not launched; carry.pend_rows > 0 from the moment the host
    // has the HI count (pre3_update_hi) until k_cholp's consumers have taken the panels (launch_cholp) or pend_flush() has run k_downdate_b3 on them
    bool pend_opt = false;
    unsigned long long *hf_sx = nullptr;          // k_hi_fused, two panels: S as [128][128] (sequence number, value) pairs, dealt over the workgroups (hf_S_dealt)
    float *W_pend = nullptr; void *Wp_pend = nullptr; unsigned *hf_xy = nullptr;      // hf_xy: [0] k_hi_fused's "L^-1 nu is out" word, [64 .. 191] L^-1 nu (hf_x_update)
    bool step_tail = false;                       // PRE3_OPT_STEP_TAIL (default: the environment's PRE3_TAIL, else off)
    // marginal readers (pre3_get_landmarks / pre3_get_marginal, pre3_map.hip), allocated on first use: device results and their pinned host image;
    // the landmark block is sized by the map capacity, the index-set block grows with k
    double *lmr_dev = nullptr, *lmr_host = nullptr; bool lmr_ready = false;
    // pre3_relocalise_seeded (pre3_reloc.hip), allocated by pre3_create: the work block [Xw | U | masks | what goes back | the RANSAC's tables] for
    // min(capN, RELOC_MAX_N) landmarks and the pinned image of the part that goes back
    char *reloc_dev = nullptr, *reloc_host = nullptr; int reloc_cap = 0;
    // pre3_update_rows / pre3_heading_update (pre3_rows.hip), allocated on first use: the rows block and H*P (RMAX x ld, fp64)
    pre3::RowsBlock *rows_blk = nullptr; double *rows_hp = nullptr; bool rows_ready = false;
    int rows_form = 0;                            // PRE3_OPT_ROWS_FORM: 1 the single-sweep form, 0 run_update
    // pre3_heading_from_scan (pre3_plane.hip), allocated on first use: [points | draws | scores | result] and the block the heading rows read
    pre3::HeadingSrc *plane_src = nullptr;
    // features_info bookkeeping and the map policy (pre3_set_book / pre3_map_policy, pre3_map.hip).  A booked context carries
    // [capN][4] int32 (times_predicted, times_measured, init_frame, last_visible) through every map call; book_vis[i] = has_h || visible at x_k_k
    // after the LI update, recorded where the reference's rescue projects (pre3_step / pre3_step_predicted / pre3_rescue), cleared by every map call
    bool booked = false; int book_s = 0;          // book_s: init_frame / last_visible of landmarks a map call adds (the last policy call's step - 1)
    int32_t *book = nullptr, *book_alt = nullptr, *book_vis = nullptr; bool book_ready = false;
    int32_t *pol_host = nullptr, *pol_host_dev = nullptr;                  // the policy's result block (mem.pol_host) and its device address
    // the patch branch of the IC search (pre3_patch.hip), allocated on first use: the resident image, the patch bank, the warped patches
    pre3::PatchState *patch = nullptr;
    // FAST-9 corners on the resident image (pre3_fast.hip), allocated on first use: the verdict map and the result block
    pre3::FastState *fast = nullptr;
    CtxMemory mem;
};

namespace pre3 {

// normJac.m:27-38
__device__ inline void d_normjac(const double *q, double *J)
{
    double r = q[0], x = q[1], y = q[2], z = q[3];
    double s = pow(r * r + x * x + y * y + z * z, -1.5);
    J[0] = s * (x * x + y * y + z * z); J[1] = s * (-r * x); J[2] = s * (-r * y); J[3] = s * (-r * z);
    J[4] = s * (-x * r); J[5] = s * (r * r + y * y + z * z); J[6] = s * (-x * y); J[7] = s * (-x * z);
    J[8] = s * (-y * r); J[9] = s * (-y * x); J[10] = s * (r * r + x * x + z * z); J[11] = s * (-y * z);
    J[12] = s * (-z * r); J[13] = s * (-z * x); J[14] = s * (-z * y); J[15] = s * (r * r + x * x + y * y);
}

// ---- the way into and out of every stateful entry point (pre3_api.hip).  In: the context is checked, a deferred HI update completed and pending work
// flushed -- `ordinary`: all of it; `step`: the rows/cols 3..6 pass is left to the prediction's launch and (pend_keep) a pending HI down-date to this call's
// own launches; `reader`: nothing is flushed.  Out: a rows/cols 3..6 pass nobody took goes out as its own launch (a reader that settled leaves it to the next
// step), then req and out are reset.  Nested calls go through the *_impl functions, never through an exported wrapper.
enum class Entry { ordinary, step, reader };
struct EntryScope {
    pre3_ctx *c; Entry kind; int rc;
    explicit EntryScope(pre3_ctx *c, Entry kind = Entry::ordinary, bool pend_keep = false);
    ~EntryScope();
    EntryScope(const EntryScope &) = delete;
};
int flush_unless_kept(pre3_ctx *c);      /* a pending rows/cols 3..6 pass, then a pending HI down-date, out unless this call keeps them */
void drop_carried(pre3_ctx *c);          /* the deferred work of a state that is being replaced is dropped, not run */
template <typename T> int dmalloc_bytes(pre3_ctx *c, T **p, size_t bytes) { return c->mem.fixed.dev(p, bytes ? bytes : 16, Zero::sync()); }      /* a zeroed block on the context's fixed list (at least 16 bytes) */
int wait_mail(pre3_ctx *c, int slot, int32_t seq);      /* poll the pinned mailbox until the kernel launched with `seq` has published in word `slot` */
int stats_words(pre3_ctx *c);            /* the device's error words, once a copy of them into pinned_stats has completed */
const char *numeric_word_message(int32_t word);      /* what a non-zero numeric error word (stats[6]) says: the factorisation's, or a refused VO pair's (pre3_predictu.h) */
int fetch_stats(pre3_ctx *c);
// Fill the pinned inbox and ship it: [meas | ic | (hyp) | z].  pull == false: the caller's next launch carries the pull of *nbytes_out bytes (pre3_step: k_predict)
int install_measurements(pre3_ctx *c, int m, const int32_t *meas_idx, const double *z /* 2m, null: z already on device */, const int32_t *hyp, int n_hyp_ints,
                         bool flags_clear = false, bool pull = true, size_t *nbytes_out = nullptr);
int set_descriptors_impl(pre3_ctx *c, int first, int count, const double *desc);
int update_hi_impl(pre3_ctx *c);         /* pre3_step.hip: pre3_update_hi without the way in (EntryScope completes a deferred HI update with it) */

// ---- pooled device scratch of the stateless entry points (pre3_match.hip)
int scratch_acquire(size_t bytes, void **p_out, int *slot_out);
void scratch_release(int slot, void *p);
void release_scratch();
struct Scratch {                // one block of it, held for a scope: no hipMalloc / hipFree per call once warm
    void *p = nullptr;
    int slot = -1;
    Scratch() = default;
    Scratch(const Scratch &) = delete;
    Scratch &operator=(const Scratch &) = delete;
    ~Scratch() { scratch_release(slot, p); }
    int alloc(size_t bytes) { return scratch_acquire(bytes, &p, &slot); }
    template <typename T> T *as() const { return (T *)p; }
};
// the device of a stateless entry point selected, or PRE3_E_NODEVICE with `who` in the message: none at all, or no such index (pre3_sr.hip)
int select_device(const char *who, int device);
// ---- matchers (pre3_match.hip)
int match_partial(int device, int cls, int ND, int K1, const void *L1, int K2, const void *L2, int k2_offset, double *best, double *second, int32_t *arg);
int knn_run(int device, int D, int N, const double *data, int M, const double *query, int k, double *ids, double *dist);
void *match_bench_create(int cls, int ND, int K1, const void *L1, int K2, const void *L2);
int match_bench_info(void *h, int32_t info[3]);
int match_bench_run(void *h, int reps, double *ms_per);
int match_bench_fetch(void *h, double *best, double *second, int32_t *arg);
void match_bench_destroy(void *h);
void *match_shard_create(int device, int cls, int ND, int K1, const void *L1, int K2, const void *L2, int k2_offset);
int match_shard_run(void *h, void **partial_dev, int *n_doubles);
int match_shard_merge(void *h, int G, const void *gathered_dev, double thresh, double *pairs_out, double *score_out, int *M_out);
void match_shard_destroy(void *h);
int match_shard_set_comm(void *h, void *comm);
int match_shard_match(void *h, double thresh, double *pairs_out, double *score_out, int *M_out);
int match_shard_test_stall(void *h, int release);

// ---- RCCL communicator (pre3_comm.hip): collectives on the caller's stream
int comm_all_reduce_i32(void *comm, void *buf, size_t count, hipStream_t st);                       /* in place, sum */
int comm_all_gather_f64(void *comm, const void *src, void *dst, size_t count_per_rank, hipStream_t st);
int comm_timeout_ms(void *comm);                                                                   /* deadline of a host wait behind a collective */
int comm_give_up(void *comm, const char *what);                                                     /* deadline passed: abort, mark broken, PRE3_E_COMM */
int comm_poll_error(void *comm);
int comm_abort_ms(void *comm);                                                                       /* bound of a join of the abort thread (>= 10 s) */
bool comm_broken(void *comm);                                                                       /* the communicator has been aborted (deadline or asynchronous error) */
bool comm_abort_wait(void *comm, int ms);                                                           /* an abort started by comm_give_up has returned (joined) within ms; true also when none is running */
/* Wait until everything queued on a stream has finished.  Without a communicator: hipStreamSynchronize.  With one (a collective may be queued on the
   stream, and a peer may never enter it): hipStreamQuery polls with the communicator's wall-clock deadline; on expiry the communicator is aborted and the
   call returns PRE3_E_COMM -- no host wait of the library ends in an unbounded synchronisation behind a collective. */
int stream_drain_on(hipStream_t st, void *comm, const char *what);
int stream_drain(pre3_ctx *c, const char *what);                                                                    /* PRE3_E_COMM once the communicator has failed (and is aborted) */
void comm_rank_world(void *comm, int *rank, int *world);
int comm_device(void *comm);

// ---- IC search (pre3_match.hip)
int launch_ic_search(pre3_ctx *c, double thresh, int strict);
bool ic_search_fused_applies(const pre3_ctx *c);      /* N * K2 <= 2^20 pairs, N <= 4096, K2 <= 2048: the two-launch route */
int launch_ic_search_fused(pre3_ctx *c, double thresh, int strict, int32_t seq, int slot, bool matched);      /* matched: the matcher rode in the projection's launch */
int launch_bank_gather(pre3_ctx *c, int N_new, const int32_t *src_host);
int ic_rank_set_scan(pre3_ctx *c, bool in_bounds);
int launch_pull(pre3_ctx *c, const void *pinned_host, void *dst_dev, size_t bytes, int done_slot = -1);      // done_slot >= 0: the pull announces itself in mailbox word 16 + slot (stage_wait)
int stage_wait(pre3_ctx *c, int k);      // pinned host block -> device, by a kernel (pre3_api.hip)
void ic_rank_free(pre3_ctx *c);
constexpr int DESC_DIM = 128;

// ---- geometry / RANSAC kernels (pre3_geom.hip)
int launch_project(pre3_ctx *c, int which, int clear_first);
int launch_innovation(pre3_ctx *c, int mode /*0: S=HPH'+I for predicted; 1: rescue gate + HI list*/, double chi2, bool clear_flags = false, bool collect = true /* mode 1: the HI list follows (k_collect_hi) */);
struct IcMatchRide;
int launch_project_innovation(pre3_ctx *c, int which, int clear_first, int mode, double chi2, bool collect = true, bool clear_ic = false, const IcMatchRide *ride = nullptr);
int launch_update_x(pre3_ctx *c, int which_prior, int r);
int launch_jnorm(pre3_ctx *c, int which);
struct PredictUDev; struct PnPair; struct PredictUIcp;
int launch_predict_impl(pre3_ctx *c, const double u[7], bool with_projection = false, size_t inbox_n16 = 0, int32_t inbox_seq = 0,
                        const PredictUDev *u_dev = nullptr /* the increment from a VO pair's device result block (pre3_geomdev.h); u unused */,
                        const PnPair *pn_pair = nullptr /* with u_dev: the pair's covariance as Pn under the status rule (pre3_vocov.h); its `behind` is filled here */);
// the prediction behind a VO pair and the dense ICP that refined it: u and Pn under predict_icp_select (pre3_predicticp.h)
int launch_predict_icp(pre3_ctx *c, const PredictUIcp &u_icp);
// the prediction behind an EPnP RANSAC of the map against the scan: u and Pn under reloc_select (pre3_reloc.h)
struct PredictUReloc;
int launch_predict_reloc(pre3_ctx *c, const PredictUReloc &u_reloc, const double *pn_reloc_dev);
// the same behind k_pnp_refine (pre3_relocalise_refined_seeded): noise is PRE3_RELOC_NOISE_*, pn_out[49] / noise_out[0] what was used
int launch_predict_reloc_refined(pre3_ctx *c, const PredictUReloc &u_reloc, const double *pn_reloc_dev, const pre3_pnp_refine_result *ref, int noise, double *pn_out,
                                 int32_t *noise_out);
// pre3_relocalise_seeded's device block and the pinned image of what it returns, sized by the map capacity (pre3_reloc.hip; pre3_create)
int reloc_alloc(pre3_ctx *c);
// the camera-only prediction (pre3_predict_cv; pre3_predictcv.h): one launch, no riders, pred_params untouched
int launch_predict_cv(pre3_ctx *c, int type, double dt, double sigma_a, double sigma_alpha);
constexpr int PRED_PN_OFF = 128;         /* pred_params[128 .. 176]: the context's process noise block (pre3_set_process_noise) */
int launch_set_pn(pre3_ctx *c, const double *Pn);
int process_noise_check(const char *who, const double *Pn);      /* finite, no negative diagonal entry, exactly symmetric: else PRE3_E_ARG */
int launch_get_pn_const(pre3_ctx *c, double *dst_dev);      /* d_process_noise's 49 doubles into device memory, on the context's stream */
struct VoOut; struct VoPairHeader; struct VoCov;
int launch_vo_cov_pair(const VoPairHeader *hdr, const VoOut *out, int cap, const double *pset1, const double *pset2, const int32_t *inl, VoCov *cov, hipStream_t st);
// (either direction: 16-byte words between device memory and a mapped pinned block, then `seq` into mailbox word `slot`)
int launch_inbox_pull(pre3_ctx *c, const void *src_host_mapped, void *dst_dev, size_t n16, int32_t seq, int slot = 10, int32_t *clear = nullptr, int n_clear = 0);
int launch_slice_prepare(pre3_ctx *c, const void *src_host_mapped, size_t n16, int32_t seq, int n_zero, int k, int lo, int hi, int tag);
int launch_window_gate(pre3_ctx *c, int M, const int32_t *pred_idx_dev, const int32_t *k1_dev, const double *zc_dev, int strict, int32_t *accept_dev);
int launch_build_rows_impl(pre3_ctx *c, int nsel, const int32_t *sel_dev, int r_pad);
int launch_ransac_score_impl(pre3_ctx *c, int k, double threshold, int hyp_begin, int hyp_end, int ldg, int32_t *support_dev, uint32_t *mask_dev, int mask_words);
int launch_ransac_select_impl(pre3_ctx *c, int n_draw, int k, int early_exit, int32_t *support_dev, const uint32_t *mask_dev, int mask_words, int err_idx = -1);

// ---- marginal readers (pre3_map.hip): gathers of x and P at `which`, a pending HI down-date (PendW) and a pending rows/cols 3..6 pass (jn: Jn on the
// device, null: none) applied by the reading launch itself; results into the caller's host arrays (any may be null).  Arguments checked by the caller.
int read_landmarks(pre3_ctx *c, int which, int first, int count, double *xyz, double *cov_xyz, double *cov_native, double *linearity);
int read_marginal(pre3_ctx *c, int which, int k, const int32_t *idx, const double *jn, double *x_out, double *P_out);

// ---- small-rank update on the resident x_k_k / p_k_k (pre3_rows.hip): rows from the host block, or (rows == null) the heading rows built on the device
// from x_k_k(4:7) behind the gate of hd.  Two launches, P swept once.  rows_applied: the gate word into host memory, on the stream (caller drains).
int launch_rows_update(pre3_ctx *c, const RowsBlock *rows, const RowsHeading *hd);
int rows_applied(pre3_ctx *c, int32_t *applied_host);

int stage_acquire(pre3_ctx *c, size_t bytes, void **host, void **dev, int *slot);      /* pre3_api.hip: a pinned staging block of the context ... */
int stage_release(pre3_ctx *c, int slot);                                              /* ... handed to the pull queued with launch_pull(.., slot) */

// ---- seeded draw tables (pre3_draws.hip, pre3_philox.h): one lane per hypothesis, written where the scoring launch behind them reads
int launch_draw_1p(unsigned long long seed, unsigned long long seq, int n_draw, int m, int k, int32_t *hyp_dev, hipStream_t st);
int launch_draw_vo(unsigned long long seed, unsigned long long seq, int n_hyp, int pnum, const double *m1_dev, const double *m2_dev, int ms, int32_t *draws_dev,
                   int32_t *capped_dev /* zero at launch */, hipStream_t st);
// flag_dev != nullptr: the word k_plane_crop ORs into; non-zero when the launch runs: it leaves at once, the table is not written
int launch_draw_plane(unsigned long long seed, unsigned long long seq, int n_draw, int npts, const double *pts_dev, int32_t *draws_dev, hipStream_t st,
                      const int32_t *flag_dev = nullptr);
// the candidates' weighted order: keys, then their counting rank; cand_out_dev != nullptr: the [K][2] | rho[K] block re-laid in drawn order
// k_real_dev != nullptr: K is the layout count (grids, the offset of rho behind the pixels) and *k_real_dev <= K, on the device, the number of candidates
// there are -- work items at or beyond it leave at once; order2_dev != nullptr: a second copy of the order (device memory, for the launches behind)
int launch_cand_order(unsigned long long seed, unsigned long long seq, int K, int box_w, int box_h, const double *raw_dev, double *keys_dev, int32_t *order_dev,
                      double *cand_out_dev, hipStream_t st, const int32_t *k_real_dev = nullptr, int32_t *order2_dev = nullptr);

// ---- the resident SR4000 frame (pre3_sr.hip): the handle's device pointers and stream for other translation units -- a plane fit
// that crops from the resident frame, a VO gather from two resident frames, the candidate build.  Planes are rows x cols, column-major; conf is null when
// the frame was loaded without a confidence map; maxima = { imax, cmax }.  Work queued on `stream` is ordered behind the frame's conditioning launches.
struct SrFrameView {
    int device, rows, cols, mode, has_conf;
    const double *x, *y, *z, *img, *conf, *maxima;
    hipStream_t stream;
    int comp_form;                  // the compensation the frame was conditioned with (0 none, 1 bad pixels, 2 the image's median): x .. img hold its result
};
int sr_frame_view(pre3_sr_frame *f, SrFrameView *v);      /* PRE3_E_STATE before the first load */
// the handle's last keypoint result (pre3_sr_frame_keypoints), which stays in its keypoint block: the kept frames [n_kept][ldf] and descriptors
// [n_kept][ND] in the caller's order.  A load makes it stale; a keypoint call with K == 0, or one that fails behind its argument checks, leaves a valid
// empty one (n_kept == 0, frm == des == nullptr).  PRE3_E_STATE when there is none or it is stale.
// xyz [n_kept][3] = [-x, -y, z], rho [n_kept] (gate 0 only: null otherwise) and keep_idx [n_kept] sit in the same block.
// frm_in [K_in][ldf] / des_in [K_in][ND]: the RAW set handed to that call, at the front of the same block (K_in == K, or 0 with null pointers for an
// empty record); raw_in_bounds: every raw descriptor entry passed copy_desc_checked's test on its way through the handle's staging
// (pre3_set_scan_frame hands it to ic_rank_set_scan).
struct SrKeypointView { int K, ldf, ND, gate, n_kept; const double *frm, *des; const double *xyz, *rho; const int32_t *keep_idx;
                        int K_in; const double *frm_in, *des_in; bool raw_in_bounds; };
int sr_frame_keypoint_view(pre3_sr_frame *f, SrKeypointView *v);
int sr_frame_pair_work(pre3_sr_frame *f, size_t dev_bytes, size_t pin_bytes, void **dev, void **pin);      /* pre3_vopair.hip's work blocks */
int sr_frame_icp_work(pre3_sr_frame *f, size_t dev_bytes, void **dev);      /* the device block of an ICP run a prediction reads without a host wait */
// the hand-off between the handle's stream and a consumer's, on the handle's own event.  lend: `consumer` waits for everything
// queued on the handle's stream so far (a load, the conditioning launches).  reclaim: the handle's stream waits for everything queued on `consumer` so
// far, so that a load or a keypoint call that follows cannot overwrite blocks the consumer's launches still read.
int sr_frame_lend(pre3_sr_frame *f, hipStream_t consumer);
int sr_frame_reclaim(pre3_sr_frame *f, hipStream_t consumer);
// every check the calls on a (prev, cur) pair of resident frames share, `who` in every message: two distinct handles, thresh, both views on one
// device with one size, both keypoint results with DESC_DIM entries per descriptor
int sr_frame_pair_views(const char *who, pre3_sr_frame *prev, pre3_sr_frame *cur, double thresh, SrFrameView *v1, SrFrameView *v2, SrKeypointView *k1,
                        SrKeypointView *k2);
// ---- the match stage of the pair call on its own (pre3_vopair.hip: k_vp_match, k_vp_pairs), for pre3_map_policy_frames_seeded.  des1 [n1][128] the
// queries, des2 [n2][128] the scan (n1, n2 >= 1); part: vp_match_part_bytes(n1, n2) of device scratch; match 2 x n1 doubles; hdr_dev a VoPairHeader
// (pnum, rst written; bad and capped cleared).  Everything on `st`.
size_t vp_match_part_bytes(int n1, int n2);
int launch_vp_match(int n1, int n2, const double *des1, const double *des2, double thresh, void *part, double *match, void *hdr_dev, hipStream_t st);
// the accepted candidates' descriptors from a keypoint block into the bank (pre3_api.hip): landmark first + a takes row rows_dev[a] of des_dev [..][128]
int set_descriptors_rows_dev(pre3_ctx *c, int first, int count, const double *des_dev, const int32_t *rows_dev, int n_rows, bool in_bounds);
// copy_desc_checked for other translation units (pre3_api.hip): count doubles src -> dst; true when every value is finite with |x| <= 2^60 and no
// non-zero |x| < 2^-40 (the ranked IC route's bounds)
bool desc_copy_checked(double *dst, const double *src, size_t count);

// ---- map policy (pre3_map.hip): the rescue-visibility rider of a booked context (one small launch at the post-LI x_k_k), buffers
int launch_book_vis(pre3_ctx *c);

int run_hypothesis_support(int n, const double *xi, const pre3_cam &cam, int n_id, const int32_t *i1, const int32_t *i2, const int32_t *i3,
                           const double *z_id, int n_euc, const int32_t *i4, const double *z_euc, double threshold, int32_t *out_host /* [1 + n_id + n_euc] */);

// ---- dense update kernels (pre3_update.hip)
// rows: ELL rows [r] in c->row_col/row_val with nu in c->row_nu; computes W = H*P (+ nu column),
// S = H*P*H' + R, Cholesky, W = L^-1 [HP | nu], x += W' y, P -= W'W, Jnorm + normalise.
int run_update(pre3_ctx *c, int which_prior, int r, bool dense_R, void *Kt_out_dev /*nullable, r_pad x ldw T*/, bool prebuilt = false, bool first_done = false,
               bool hp_built = false /* rows and W = H*P are in place (launch_ell_HP_build_sel), S is not */);
int launch_ell_HP_build_sel(pre3_ctx *c, int nsel, const int32_t *sel_dev /* nullable: the first nsel measurements */, void *dst);
int launch_chol_first_spec(pre3_ctx *c, int nsel_max);
int chol_solve_for_test(pre3_ctx *c, int r_pad, bool predicted_prior, int r);      /* pre3_test_factor_solve's way to the (static) launch_chol_solve: S and [B | nu] are in place */
struct InboxRide;
int launch_ell_HP_build(pre3_ctx *c, void *dst, const int32_t *need = nullptr, int need_tag = 0 /* sharded RANSAC: only the measurements with need[s] == need_tag */,
                        const InboxRide *ib = nullptr /* a pull from the pinned inbox that rides in the launch */);
int launch_ell_G_hyp(pre3_ctx *c, int k, int lo, int hi, int ldg);                 /* H*P*H' entries among each hypothesis' own rows, hypotheses [lo, hi) */
int launch_gather_li(pre3_ctx *c, int nsel /* < 0: count read on the device */, int nsel_max, const int32_t *sel_dev, int ldg);
int launch_select_gather(pre3_ctx *c, int n_draw, int k, int early_exit, int mask_words);     // selection + LI gather in one launch (pre3_geom.hip)
bool select_gather_usable(const pre3_ctx *c);
int launch_ell_HP(pre3_ctx *c, int r, void *dst /*r_pad x ldw*/, bool with_nu);
int launch_ell_G(pre3_ctx *c, int r, const void *HPsrc, void *dst, int ldg, int add_identity, const void *Rdense, bool lower_only = false);
int launch_downdate(pre3_ctx *c, int r, const void *W, int which_prior = -1 /* >= 0: also x <- x_prior + W'y (update.m:36) */,
                    int planes_rows = 0 /* pre3_bench_downdate: rows of W whose bf16 planes an earlier launch of the same W has produced */);
int launch_fill_w(pre3_ctx *c, int r_pad);
bool hi_fused_usable(const pre3_ctx *c);
int hi_fused_max(const pre3_ctx *c);                  /* landmarks k_hi_fused updates with on its own (64: two panels; 32) */
int launch_hi_fused(pre3_ctx *c, int32_t seq);        /* the HI collection + update of up to 32 landmarks without the host (k_hi_fused + its down-date) */

}  // namespace pre3
