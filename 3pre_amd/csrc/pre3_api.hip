// pre3_api.hip -- the C ABI of include/pre3.h: context management, the way into and out of every stateful call (EntryScope), host<->device
// marshalling, the stateless drop-ins, matcher forwards and timers.  The stage order of a filter step is in pre3_step.hip.
#include <time.h>
#include <algorithm>
#include <atomic>
#include <immintrin.h>
#include <cmath>
#include <cstdarg>
#include <new>

#include <chrono>
#include "pre3_internal.h"
#include "pre3_test_hooks.h"
#include "pre3_geomdev.h"
#include "pre3_predictu.h"
#include "pre3_predictcv.h"
#include <mutex>
#include "pre3_cholp.h"
#include "pre3_patch.h"
#include "pre3_fast.h"

namespace pre3 {

static thread_local char g_err[512] = "";
void set_error(const char *fmt, ...)
{
    va_list ap; va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

// ---- the seam of pre3_own.h over HIP: the only allocations of the library besides the ScratchPool's (pre3_match.hip).  g_live: device blocks, device
// bytes, pinned blocks, pinned bytes that are live (pre3_test_live_blocks)
static std::atomic<int64_t> g_live[4];
static void live_count(int kind, int sign, size_t bytes)
{
    g_live[2 * kind].fetch_add(sign, std::memory_order_relaxed);
    g_live[2 * kind + 1].fetch_add(sign * (int64_t)bytes, std::memory_order_relaxed);
}
int own_dev_alloc(void **p, size_t bytes)
{
    if (hipMalloc(p, bytes) != hipSuccess) { *p = nullptr; set_error("hipMalloc of %zu bytes failed", bytes); return PRE3_E_NOMEM; }
    live_count(0, +1, bytes);
    return PRE3_OK;
}
void own_dev_free(void *p, size_t bytes) { (void)hipFree(p); live_count(0, -1, bytes); }
static_assert(PIN_DEFAULT == hipHostMallocDefault && PIN_PORTABLE == hipHostMallocPortable && PIN_MAPPED == hipHostMallocMapped, "pre3_own.h's flags are HIP's");
int own_pin_alloc(void **p, size_t bytes, unsigned flags)
{
    if (hipHostMalloc(p, bytes, flags) != hipSuccess) { *p = nullptr; set_error("hipHostMalloc of %zu bytes failed", bytes); return PRE3_E_NOMEM; }
    live_count(1, +1, bytes);
    return PRE3_OK;
}
void own_pin_free(void *p, size_t bytes) { (void)hipHostFree(p); live_count(1, -1, bytes); }
int own_dev_zero(void *p, size_t bytes, void *stream)
{
    const hipError_t e = stream ? hipMemsetAsync(p, 0, bytes, (hipStream_t)stream) : hipMemset(p, 0, bytes);
    if (e != hipSuccess) { set_error("hipMemset failed: %s", hipGetErrorString(e)); return PRE3_E_HIP; }
    return PRE3_OK;
}

// a block on the context's fixed list with defined contents: a recycled allocation must not leak a previous context's data into fields the reference
// leaves empty (a measured landmark that is not predicted has h = [] there; its h/H were whatever the allocator returned here)
template <typename T> static int dmalloc(pre3_ctx *c, T **p, size_t count) { return c->mem.fixed.dev(p, sizeof(T) * (count ? count : 1), Zero::sync()); }

static int complete_deferred_hi(pre3_ctx *c)
{
    if (c->carry.hi_pending) {           // PRE3_OPT_DEFER_HI: the previous step's HI update is completed by whatever call comes next
        c->carry.hi_pending = false;
        PRE3_TRY(update_hi_impl(c));
        c->carry.last_n_hi = c->hi_from_host >= 0 ? c->hi_from_host : (c->hi_kernel ? c->mail_host[5] : 0);
    }
    return PRE3_OK;
}
// PRE3_OPT_PEND_HI: only pre3_step carries a pending HI down-date into its launches (req.pend_keep); for everybody else P is P before the call goes on.
// The marginal readers (pre3_get_landmarks / pre3_get_marginal) complete a deferred HI update as pre3_step would and leave its rows/cols 3..6 pass
// pending for the next prediction's launch, as pre3_step would: whoever else comes next runs that pass first (k_jnorm_P, behind the flush it makes).
int flush_unless_kept(pre3_ctx *c)
{
    if (c->carry.jn_pending && !c->req.leave_jn_to_predict) { c->carry.jn_pending = false; PRE3_TRY(launch_jnorm(c, 0)); }
    if (c->carry.pend_rows > 0 && !c->req.pend_keep) PRE3_TRY(pend_flush(c));
    return PRE3_OK;
}
void drop_carried(pre3_ctx *c) { c->carry = {}; }
static int enter_ctx(pre3_ctx *c, Entry kind, bool pend_keep)
{
    PRE3_CHECK(c != nullptr, PRE3_E_ARG, "null context");
    PRE3_HIP(hipSetDevice(c->device));
    // step: the completed update's rows/cols 3..6 pass (or one a reader has left pending since) is left to the prediction's launch (PRE3_FUSE_JN=0: its own launch)
    c->req.leave_jn_to_predict = kind != Entry::ordinary && knob::fuse_jn() && (c->carry.hi_pending || (kind == Entry::step && c->carry.jn_pending));
    c->req.pend_keep = pend_keep;
    int rc = complete_deferred_hi(c);
    if (rc == PRE3_OK && kind != Entry::reader) rc = flush_unless_kept(c);
    c->req.leave_jn_to_predict = false;
    return rc;
}
EntryScope::EntryScope(pre3_ctx *c_, Entry kind_, bool pend_keep) : c(c_), kind(kind_), rc(enter_ctx(c_, kind_, pend_keep)) {}
EntryScope::~EntryScope()
{
    if (c == nullptr) return;
    if (c->carry.jn_pending && !(kind == Entry::reader && rc == PRE3_OK)) { c->carry.jn_pending = false; (void)launch_jnorm(c, 0); }
    c->req = {}; c->out = {};
}

// Poll the pinned mailbox until the kernel that was launched with sequence number `seq` has published.
// slot 8: k_ransac_select, slot 9: k_collect_hi.  Falls back to a stream sync if the word does not arrive.
static double now_ms() { timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec * 1e3 + t.tv_nsec * 1e-6; }
// see pre3_internal.h
int stream_drain_on(hipStream_t st, void *comm, const char *what)
{
    if (comm == nullptr) { PRE3_HIP(hipStreamSynchronize(st)); return PRE3_OK; }
    const bool was_broken = comm_broken(comm);
    const double t0 = now_ms();
    for (long spin = 0; ; ++spin) {
        const hipError_t e = hipStreamQuery(st);
        if (e == hipSuccess) return PRE3_OK;
        if (e != hipErrorNotReady) PRE3_HIP(e);
        if ((spin & 15) == 15) {
            if (!was_broken) PRE3_TRY(comm_poll_error(comm));
            if (now_ms() - t0 > comm_timeout_ms(comm)) {
                if (!was_broken) return comm_give_up(comm, what);
                set_error("%s: the stream has not drained %d ms after its communicator was aborted", what, comm_timeout_ms(comm));
                return PRE3_E_COMM;
            }
            timespec ts = { 0, 20000 };
            nanosleep(&ts, nullptr);
        }
    }
}
int stream_drain(pre3_ctx *c, const char *what) { return stream_drain_on(c->stream, c->comm, what); }
int wait_mail(pre3_ctx *c, int slot, int32_t seq)
{
    volatile int32_t *w = c->mail_host + slot;
    // With a communicator on the context the awaited kernel may sit behind a collective: a peer that stalls (or never entered) must not hang this
    // host for ever -- the wait has a wall-clock deadline (pre3_comm_set_timeout), and never ends in a bare hipStreamSynchronize.
    const bool coll = c->comm != nullptr;
    const double t0 = coll ? now_ms() : 0;
    double t_q = 0;
    for (long spin = 0; coll || spin < 2000000000L; ++spin) {
        if (__atomic_load_n(w, __ATOMIC_ACQUIRE) == seq) return PRE3_OK;
        if ((spin & 1023) == 1023) {
            // Is the stream idle although the word has not come (the producing kernel was never launched)?  hipStreamQuery is not free of side effects:
            // to learn the state of the last launch the runtime appends a marker (a barrier packet with a completion signal) behind it, and the next
            // launch then starts ~6 us after its predecessor has ended -- the two "holes" of the step (behind k_cholp and behind the HI down-date: the
            // two places where the host polls a count) were these markers, not store drains.  So: only after 2 ms without the word.
            const double t = now_ms();
            if (t_q == 0) { t_q = t; continue; }
            if (t - t_q < 2.0) continue;
            if (hipStreamQuery(c->stream) == hipSuccess) break;
            if (coll && (spin & 0x3ffff) == 0x3ffff) {
                PRE3_TRY(comm_poll_error(c->comm));     // a collective in front of the awaited kernel whose peer died
                if (now_ms() - t0 > comm_timeout_ms(c->comm)) return comm_give_up(c->comm, "a collective in front of the awaited kernel");
            }
        }
    }
    PRE3_TRY(stream_drain(c, __func__));
    PRE3_CHECK(__atomic_load_n(w, __ATOMIC_ACQUIRE) == seq, PRE3_E_STATE, "mailbox: the producing kernel has not been launched");
    return PRE3_OK;
}

const char *numeric_word_message(int32_t word)
{
    switch (pu_word_refusal(word)) {
    case PU_REFUSED_NEAR: return "pre3_predict_pair_seeded: the pair was refused -- no matched point is farther than 0.4 m from the camera; the prediction was made with the identity increment";
    case PU_REFUSED_BAD: return "pre3_predict_pair_seeded: the pair was refused -- a match names a keypoint that does not exist, or a kept keypoint rounds to a pixel outside the range image; the prediction was made with the identity increment";
    default: return "innovation covariance S is not positive definite";
    }
}
int stats_words(pre3_ctx *c)
{
    PRE3_CHECK(c->pinned_stats[7] == 0, PRE3_E_HIP, "a device-side wait on another workgroup gave up (counter never arrived): results are invalid");
    const int32_t w = c->pinned_stats[6];
    if (pu_word_refusal(w) != PU_OK) {
        // a refused pair belongs to one call, not to the state (x and P hold a valid prediction): reported once, the word cleared with the report
        (void)hipMemsetAsync(c->stats + 6, 0, sizeof(int32_t), c->stream);
        if (c->mail_host) c->mail_host[6] = 0;
    }
    PRE3_CHECK(w == 0, PRE3_E_NUMERIC, "%s", numeric_word_message(w));
    return PRE3_OK;
}
int fetch_stats(pre3_ctx *c)
{
    PRE3_HIP(hipMemcpyAsync(c->pinned_stats, c->stats, sizeof(int32_t) * 16, hipMemcpyDeviceToHost, c->stream));
    PRE3_TRY(stream_drain(c, __func__));
    return stats_words(c);
}

// the staged scan [descriptors | positions] out of pinned host memory into the two device arrays (n16_pos == 0: one array)
// done.ctr != nullptr: the last workgroup to finish publishes done.seq in the pinned mailbox word done.mail -- the host may then overwrite the staging
// block (stage_wait).  An event recorded behind the launch would tell the same, but its record puts a barrier packet with a completion signal into the
// stream, and the NEXT launch then starts ~6 us after this one has ended (measured in the frame leg: three such holes per frame).
struct StageDone { unsigned int *ctr; int32_t *mail; int32_t seq; };
__global__ __launch_bounds__(256) void k_scan_pull(const int4 *__restrict__ src, int n16_desc, int4 *__restrict__ desc, int n16_pos, int4 *__restrict__ pos, StageDone done)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n16_desc) desc[i] = src[i];
    else if (i < n16_desc + n16_pos) pos[i - n16_desc] = src[i];
    if (done.ctr != nullptr) {
        __syncthreads();                                 // (this workgroup's reads of the block have returned: their values are on their way out)
        if (threadIdx.x == 0 && atomicAdd(done.ctr, 1u) == gridDim.x - 1) {
            atomicExch(done.ctr, 0u);
            __threadfence_system();
            __hip_atomic_store(done.mail, done.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}
// the accepted candidates' descriptors from a resident frame's keypoint block into the bank (pre3_map_policy_frames_seeded):
// one wave per new landmark, 16 bytes per lane; rows[a] is clamped to the block, so no read leaves it whatever the walk wrote
__global__ __launch_bounds__(64) void k_fc_desc(int n_rows, const int32_t *__restrict__ rows, const double *__restrict__ des, double *__restrict__ bank_dst)
{
    const int row = min(max(rows[blockIdx.x], 0), n_rows - 1);
    const double2 *s2 = (const double2 *)(des + (size_t)row * DESC_DIM);
    double2 *d2 = (double2 *)(bank_dst + (size_t)blockIdx.x * DESC_DIM);
    d2[threadIdx.x] = s2[threadIdx.x];
}
// the IC search's scan out of a resident frame's keypoint block (pre3_set_scan_frame): [K2][128] descriptors into scan_desc, 16
// bytes per lane, and entries 0..3 of every keypoint's frame [K2][ldf] into scan_pos[K2][4] (entries at or beyond ldf: zero), one lane per keypoint --
// 16-byte reads where ldf is even, 16-byte writes always.  des, frm (when ldf is even), scan_desc and scan_pos are 16-byte aligned (checked on the host).
__global__ __launch_bounds__(256) void k_scan_frame(int K2, int ldf, const double *__restrict__ frm, const double *__restrict__ des,
                                                    double *__restrict__ scan_desc, double *__restrict__ scan_pos)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, n16 = K2 * (DESC_DIM / 2);
    if (i < n16) { reinterpret_cast<double2 *>(scan_desc)[i] = reinterpret_cast<const double2 *>(des)[i]; return; }
    const int k = i - n16;
    if (k >= K2) return;
    const double *fk = frm + (size_t)k * ldf;
    double2 a, b = make_double2(0.0, 0.0);
    if ((ldf & 1) == 0) {
        a = reinterpret_cast<const double2 *>(fk)[0];
        if (ldf >= 4) b = reinterpret_cast<const double2 *>(fk)[1];
    } else {
        a = make_double2(fk[0], fk[1]);
        b = make_double2(fk[2], ldf > 3 ? fk[3] : 0.0);      // (ldf is odd and >= 2: entry 2 exists)
    }
    reinterpret_cast<double2 *>(scan_pos)[2 * (size_t)k] = a;
    reinterpret_cast<double2 *>(scan_pos)[2 * (size_t)k + 1] = b;
}
// the staging block `k` (0, 1: uploads; 2, 3: map management) has been pulled: one read of host memory (after 2 ms: a stream synchronisation)
int stage_wait(pre3_ctx *c, int k)
{
    volatile int32_t *w = c->mail_host + 16 + k;
    const int32_t seq = c->stage_seq[k];
    if (seq == 0) return PRE3_OK;
    double t0 = 0;
    for (long spin = 0; ; ++spin) {
        if (__atomic_load_n(w, __ATOMIC_ACQUIRE) == seq) return PRE3_OK;
        if ((spin & 1023) == 1023) {
            const double t = now_ms();
            if (t0 == 0) t0 = t;
            else if (t - t0 > 2.0) break;
        }
    }
    PRE3_TRY(stream_drain(c, __func__));
    if (__atomic_load_n(w, __ATOMIC_ACQUIRE) != seq) {
        c->stage_seq[k] = 0;                         // (the stream is idle: the block is free whatever became of that launch; the next pull starts a fresh count)
        (void)hipMemsetAsync(c->chol_arrive + 8 + k, 0, sizeof(unsigned int), c->stream);
        set_error("staging block %d: its pull has not run", k);
        return PRE3_E_STATE;
    }
    return PRE3_OK;
}
static int ring_wait(void *ctx, int slot) { return stage_wait(static_cast<pre3_ctx *>(ctx), slot); }
static StageDone stage_done(pre3_ctx *c, int k) { return StageDone{ c->chol_arrive + 8 + k, c->mail_dev + 16 + k, ++c->stage_seq[k] }; }

// bytes of a pinned (device-mapped) host block -> device memory, read over PCIe by the device itself on the context's stream: no DMA engine,
// whose copies start with ~10 us of latency each (and, once in a few hundred calls, with tens of milliseconds inside the runtime)
int launch_pull(pre3_ctx *c, const void *pinned_host, void *dst_dev, size_t bytes, int done_slot)
{
    void *src_dev = nullptr;
    PRE3_HIP(hipHostGetDevicePointer(&src_dev, const_cast<void *>(pinned_host), 0));
    const int n16 = (int)((bytes + 15) / 16);
    if (n16 == 0) return PRE3_OK;
    hipLaunchKernelGGL(k_scan_pull, dim3(ceil_div(n16, 256)), dim3(256), 0, c->stream, (const int4 *)src_dev, n16, (int4 *)dst_dev, 0, (int4 *)nullptr,
                       done_slot >= 0 ? stage_done(c, done_slot) : StageDone{ nullptr, nullptr, 0 });
    PRE3_HIP(hipGetLastError());
    return PRE3_OK;
}

// see pre3_internal.h: ONE pull of [meas | ic | (hyp) | z]; hyp (n_hyp_ints ints) optional
int install_measurements(pre3_ctx *c, int m, const int32_t *meas_idx, const double *z, const int32_t *hyp, int n_hyp_ints, bool flags_clear, bool pull, size_t *nbytes_out)
{
    PRE3_CHECK(m >= 0 && m <= c->capm, PRE3_E_ARG, "measurements: m=%d exceeds capacity %d", m, c->capm);
    for (int j = 0; j < m; ++j) {
        PRE3_CHECK(meas_idx[j] >= 0 && meas_idx[j] < c->N, PRE3_E_ARG, "measurements: landmark index %d out of range", meas_idx[j]);
        PRE3_CHECK(j == 0 || meas_idx[j] > meas_idx[j - 1], PRE3_E_ARG, "measurements: landmark indices must be strictly ascending");
    }
    // the previous pull out of the pinned inbox must have completed before the host overwrites it (it has, a whole step ago: the pull
    // kernel publishes its sequence number in mailbox word 10, so this is one read of host memory -- no event, whose record would put
    // a barrier packet into the stream -- and, unlike a stream sync, it does not wait for the kernels queued since)
    if (c->inbox_pending) { PRE3_TRY(wait_mail(c, 10, c->seq_inbox)); c->inbox_pending = false; }
    c->m = m; c->meas_host.assign(meas_idx, meas_idx + m);
    c->carry.select_pending = false;
    int32_t *hm = (int32_t *)(c->inbox_host + c->off_meas), *hic = (int32_t *)(c->inbox_host + c->off_ic);
    double *hz = (double *)(c->inbox_host + c->off_z);
    memset(hic, 0, sizeof(int32_t) * c->N);
    for (int j = 0; j < m; ++j) { hm[j] = meas_idx[j]; hic[meas_idx[j]] = 1; }
    if (z) {
        memset(hz, 0, sizeof(double) * 2 * c->N);
        for (int j = 0; j < m; ++j) { hz[2 * meas_idx[j]] = z[2 * j]; hz[2 * meas_idx[j] + 1] = z[2 * j + 1]; }
    }
    if (hyp) memcpy(c->inbox_host + c->off_hyp, hyp, sizeof(int32_t) * n_hyp_ints);
    // The inbox crosses PCIe by a KERNEL that reads the pinned, device-mapped host buffer (14 KB at N=500): a hipMemcpyAsync between
    // kernels is a blit with barrier packets on both sides and opened two ~10 us holes in the stream around a 3 us copy.
    const size_t nbytes = z ? c->off_z + sizeof(double) * 2 * c->N : c->off_hyp + (hyp ? sizeof(int32_t) * n_hyp_ints : 0);
    // (the inlier flags behind the inbox are cleared by the pull's own workgroup: a hipMemsetAsync is a fill kernel between barrier packets)
    int32_t *const flags = (int32_t *)((unsigned char *)c->inbox_dev + c->off_flags);
    if (pull) { PRE3_TRY(launch_inbox_pull(c, c->inbox_host_dev, c->inbox_dev, (nbytes + 15) / 16, ++c->seq_inbox, 10, flags_clear ? nullptr : flags, flags_clear ? 0 : (int)(c->flags_bytes / 4))); c->inbox_pending = true; }
    if (nbytes_out) *nbytes_out = nbytes;
    if (!flags_clear && !pull) PRE3_HIP(hipMemsetAsync(flags, 0, c->flags_bytes, c->stream));
    c->li_from_host = c->hi_from_host = -1; c->li_kernel = c->hi_kernel = false;
    c->hp_all_valid = false;
    c->measurements_set = true;
    return PRE3_OK;
}

}  // namespace pre3

using namespace pre3;

extern "C" {

const char *pre3_last_error(void) { return pre3::g_err; }
const char *pre3_version(void) { return "pre3-mi355x 0.1 (gfx950)"; }

int pre3_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// The tail of the persistent launch (rescue stage + HI update inside k_cholp, CpTail; off by default): per landmark y = H J W' as bf16 planes (+ one zero
// slot), the row H J, crit's list, and W once more column-major.  Allocated on demand (pre3_set_option(PRE3_OPT_STEP_TAIL, 1) or PRE3_TAIL=1 at creation).
// PRE3_OPT_PEND_HI's buffers: W~ of up to two panels (f32 rows) and its planes in Wp's layout (same nst_total, so that the consumers' offsets hold for both)
static int pend_alloc(pre3_ctx *c)
{
    if (c->W_pend && c->Wp_pend && c->hf_xy) return PRE3_OK;
    PRE3_CHECK(c->dtype == PRE3_F32 && c->Wp != nullptr && c->rcap >= 2 * NB, PRE3_E_STATE, "PRE3_OPT_PEND_HI: fp32 contexts with the persistent factorisation only");
    int rc = PRE3_OK;
    auto A = [&](int r) { if (rc == PRE3_OK) rc = r; };
    if (!c->W_pend) A(dmalloc_bytes(c, &c->W_pend, (size_t)2 * NB * c->ldw * sizeof(float)));
    if (!c->Wp_pend) A(dmalloc_bytes(c, &c->Wp_pend, (size_t)ceil_div(c->ldw, 128) * (c->rcap / 16) * (3 * 4 * 64) * 16));
    if (!c->hf_xy) A(dmalloc_bytes(c, &c->hf_xy, sizeof(unsigned) * 256));
    return rc;
}

static int tail_alloc(pre3_ctx *c)
{
    if (c->tail_yp && c->tail_hb && c->tail_hib && c->tail_wt) return PRE3_OK;
    PRE3_CHECK(c->dtype == PRE3_F32 && c->Wp != nullptr, PRE3_E_STATE, "PRE3_OPT_STEP_TAIL: fp32 contexts with the persistent factorisation only");
    int rc = PRE3_OK;
    auto A = [&](int r) { if (rc == PRE3_OK) rc = r; };
    if (!c->tail_yp) A(dmalloc_bytes(c, &c->tail_yp, (size_t)(c->capN + 1) * 2 * 3 * c->rcap * 2));
    if (!c->tail_hb) A(dmalloc_bytes(c, &c->tail_hb, (size_t)c->capN * 2 * 16 * sizeof(float)));
    if (!c->tail_hib) A(dmalloc_bytes(c, &c->tail_hib, sizeof(int32_t) * (64 + 64 * 16)));
    if (!c->tail_wt) A(dmalloc_bytes(c, &c->tail_wt, (size_t)c->ldw * c->rcap * sizeof(float)));
    return rc;
}

int pre3_create(pre3_ctx **out, int device, int dtype, int max_landmarks, int max_hyp)
{
    PRE3_CHECK(out != nullptr, PRE3_E_ARG, "pre3_create: null output pointer");
    *out = nullptr;
    PRE3_CHECK(dtype == PRE3_F64 || dtype == PRE3_F32, PRE3_E_ARG, "pre3_create: dtype must be PRE3_F64 or PRE3_F32");
    PRE3_CHECK(max_landmarks >= 1 && max_hyp >= 1, PRE3_E_ARG, "pre3_create: capacities must be >= 1");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device available (libpre3 has no CPU fallback)"); return PRE3_E_NODEVICE; }
    PRE3_CHECK(device >= 0 && device < ndev, PRE3_E_NODEVICE, "pre3_create: device %d out of range (have %d)", device, ndev);
    PRE3_HIP(hipSetDevice(device));
    pre3_ctx *c = new (std::nothrow) pre3_ctx();
    PRE3_CHECK(c != nullptr, PRE3_E_NOMEM, "out of host memory");
    c->device = device; c->dtype = dtype; c->esz = dtype == PRE3_F64 ? 8 : 4;
    c->capN = max_landmarks; c->capn = 13 + 6 * max_landmarks; c->capm = max_landmarks; c->caph = max_hyp;
    c->ld = round_up(c->capn, TILE); c->ldw = c->ld + NB;
    c->step_tail = knob::tail() != 0;               // PRE3_OPT_STEP_TAIL
    c->rcap = round_up(2 * c->capm, NB) + NB;       // (+ one panel: the rescued landmarks' rows follow the LI update's inside the persistent launch, pre3_cholp.hip)
    c->mask_words_cap = ceil_div(c->capm, 32);
    int rc = PRE3_OK;
    auto A = [&](int r) { if (rc == PRE3_OK) rc = r; };
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { set_error("hipStreamCreate failed"); delete c; return PRE3_E_HIP; }
    for (StageRing *r : { &c->mem.up_ring, &c->mem.map_ring }) { r->flags = PIN_MAPPED; r->wait = ring_wait; r->wait_ctx = c; }
    c->mem.map_ring.base = 2;
    A(dmalloc(c, &c->x_kk, c->capn)); A(dmalloc(c, &c->x_km1, c->capn));
    A(dmalloc_bytes(c, &c->P, (size_t)c->ld * c->ld * c->esz));
    A(dmalloc(c, &c->lm.type, c->capN)); A(dmalloc(c, &c->lm.off, c->capN));
    A(dmalloc(c, &c->lm.h, 2 * (size_t)c->capN)); A(dmalloc(c, &c->lm.has_h, c->capN));
    A(dmalloc(c, &c->lm.Hc, 14 * (size_t)c->capN)); A(dmalloc(c, &c->lm.Hl, 12 * (size_t)c->capN));
    A(dmalloc(c, &c->lm.S, 4 * (size_t)c->capN)); A(dmalloc(c, &c->lm.has_S, c->capN));
    {
        // inbox: [meas | ic | hyp | z] is what the one H2D copy of a step ships (kept under 16 KB at N=500: larger copies
        // leave the runtime's shader path for the SDMA path, +20 us); the inlier flags [li | hi | li_meas | hi_meas] follow
        // in the same allocation and are cleared on the device (k_project_innovation in a step, a memset otherwise)
        c->off_meas = 0;
        c->off_ic = c->off_meas + sizeof(int32_t) * c->capm;
        c->off_hyp = (c->off_ic + sizeof(int32_t) * c->capN + 15) / 16 * 16;
        c->off_z = (c->off_hyp + sizeof(int32_t) * (size_t)c->caph * MAXK + 15) / 16 * 16;
        c->off_flags = c->off_z + sizeof(double) * 2 * c->capN;
        const size_t off_li = c->off_flags, off_hi = off_li + sizeof(int32_t) * c->capN;
        const size_t off_lim = off_hi + sizeof(int32_t) * c->capN, off_him = off_lim + sizeof(int32_t) * c->capm;
        c->flags_bytes = sizeof(int32_t) * (2 * (size_t)c->capN + 2 * (size_t)c->capm);
        c->inbox_bytes = c->off_flags + c->flags_bytes;
        A(dmalloc_bytes(c, &c->inbox_dev, c->inbox_bytes));
        if (rc == PRE3_OK) A(c->mem.fixed.pin(&c->inbox_host, c->inbox_bytes, PIN_MAPPED));
        if (rc == PRE3_OK && hipHostGetDevicePointer((void **)&c->inbox_host_dev, c->inbox_host, 0) != hipSuccess) { set_error("hipHostGetDevicePointer failed"); rc = PRE3_E_HIP; }
        if (rc == PRE3_OK) {
            memset(c->inbox_host, 0, c->inbox_bytes);
            unsigned char *d = (unsigned char *)c->inbox_dev;
            c->meas = (int32_t *)(d + c->off_meas); c->lm.ic = (int32_t *)(d + c->off_ic);
            c->lm.li = (int32_t *)(d + off_li); c->lm.hi = (int32_t *)(d + off_hi); c->li_meas = (int32_t *)(d + off_lim); c->hi_meas = (int32_t *)(d + off_him);
            c->hyp = (int32_t *)(d + c->off_hyp); c->lm.z = (double *)(d + c->off_z);
        }
    }
    A(dmalloc(c, &c->row_col, (size_t)c->rcap * ELLW)); A(dmalloc_bytes(c, &c->row_val, (size_t)c->rcap * ELLW * c->esz));
    A(dmalloc(c, &c->row_nu, c->rcap));
    A(dmalloc_bytes(c, &c->HP, (size_t)c->rcap * c->ldw * c->esz));
    A(dmalloc_bytes(c, &c->W, (size_t)c->rcap * c->ldw * c->esz));
    A(dmalloc_bytes(c, &c->G, (size_t)c->rcap * c->rcap * c->esz));
    A(dmalloc_bytes(c, &c->Smat, (size_t)c->rcap * c->rcap * c->esz));
    A(dmalloc(c, &c->sel_rows, c->rcap)); A(dmalloc(c, &c->need, c->capm));
    if (rc == PRE3_OK) (void)hipMemset(c->need, 0, sizeof(int32_t) * c->capm);
    // supports and inlier masks in ONE allocation, the masks right behind the n_draw supports of the current round (ransac_prepare sets
    // c->masks): a sharded round all-reduces both with a single collective over one contiguous range
    A(dmalloc(c, &c->support, (size_t)c->caph + 4 + (size_t)c->caph * c->mask_words_cap));
    if (rc == PRE3_OK) c->masks = reinterpret_cast<uint32_t *>(c->support + c->caph + 4);
    A(dmalloc(c, &c->stats, 16));
    A(dmalloc(c, &c->pred_params, 192));
    A(reloc_alloc(c));
    {
        // K9 tile schedule: upper-triangle 64x64 tiles in 4x4 super-tile order, so that the tiles in flight at
        // any moment (tickets are handed out in this order) share W panels in L2 / Infinity Cache.
        const int nt = c->ld / 64, ns = ceil_div(nt, 4);
        std::vector<std::vector<int2>> lists(8);
        int sidx = 0;
        for (int SI = 0; SI < ns; ++SI)
            for (int SJ = SI; SJ < ns; ++SJ) {
                // whole super-tiles go to the currently shortest list (balanced to within one super-tile)
                int best = 0;
                for (int x = 1; x < 8; ++x) if (lists[x].size() < lists[best].size()) best = x;
                (void)sidx;
                for (int i = SI * 4; i < std::min(nt, SI * 4 + 4); ++i)
                    for (int j = SJ * 4; j < std::min(nt, SJ * 4 + 4); ++j)
                        if (j >= i) lists[best].push_back(make_int2(i, j));
            }
        for (;;) {       // even the lists out to within one tile (moves come from the tail: the last, partial super-tiles)
            int lo = 0, hi = 0;
            for (int x = 1; x < 8; ++x) { if (lists[x].size() < lists[lo].size()) lo = x; if (lists[x].size() > lists[hi].size()) hi = x; }
            if (lists[hi].size() <= lists[lo].size() + 1) break;
            lists[lo].push_back(lists[hi].back());
            lists[hi].pop_back();
        }
        size_t mx = 1;
        int cnts[8];
        for (int x = 0; x < 8; ++x) { mx = std::max(mx, lists[x].size()); cnts[x] = (int)lists[x].size(); }
        std::vector<int2> flat(mx * 8, make_int2(0, 0));
        int total = 0;
        for (int x = 0; x < 8; ++x) { for (size_t k2 = 0; k2 < lists[x].size(); ++k2) flat[x * mx + k2] = lists[x][k2]; total += cnts[x]; }
        c->tiles_stride = (int)mx;
        c->n_tiles = total;
        {
            std::vector<int2> inter;                  // interleave: block b takes the next tile of list b % 8
            size_t pos[8] = { 0 };
            while ((int)inter.size() < total)
                for (int x = 0; x < 8 && (int)inter.size() < total; ++x)
                    if (pos[x] < lists[x].size()) inter.push_back(lists[x][pos[x]++]);
            A(dmalloc_bytes(c, &c->tiles_flat, sizeof(int2) * (inter.size() ? inter.size() : 1)));
            if (rc == PRE3_OK && hipMemcpy(c->tiles_flat, inter.data(), sizeof(int2) * inter.size(), hipMemcpyHostToDevice) != hipSuccess) { set_error("tile table upload failed"); rc = PRE3_E_HIP; }
        }
        A(dmalloc(c, &c->tile_ctr, 8)); A(dmalloc(c, &c->tile_cnt, 8)); A(dmalloc(c, &c->chol_arrive, 16));      // ([8..11]: arrival counters of the staging pulls)
        if (rc == PRE3_OK) (void)hipMemset(c->chol_arrive, 0, sizeof(unsigned int) * 16);
        if (rc == PRE3_OK) { (void)hipMemset(c->tile_ctr, 0, sizeof(unsigned int) * 8); (void)hipMemcpy(c->tile_cnt, cnts, sizeof(cnts), hipMemcpyHostToDevice); }
        { hipDeviceProp_t pr; if (hipGetDeviceProperties(&pr, device) == hipSuccess && pr.multiProcessorCount > 0) c->num_cus = pr.multiProcessorCount; }
        A(dmalloc_bytes(c, &c->tiles, sizeof(int2) * flat.size()));
        if (rc == PRE3_OK && hipMemcpy(c->tiles, flat.data(), sizeof(int2) * flat.size(), hipMemcpyHostToDevice) != hipSuccess) { set_error("tile table upload failed"); rc = PRE3_E_HIP; }
    }
    if (dtype == PRE3_F32) {
        c->k9_b3 = knob::k9_b3() != 0;
        // k_downdate_b3: bf16 planes of W and the 128x128 tile list (4x4 super-tiles dealt to 8 lists, lists interleaved: block b runs
        // on XCD b % 8, so a super-tile's 8 column blocks of planes stay in one L2)
        A(dmalloc_bytes(c, &c->Wp, (size_t)(c->ld + 128) * c->rcap * 6));       // + one column block for the nu strip's planes
        A(dmalloc_bytes(c, &c->Sp, (size_t)(c->rcap / NB) * (c->rcap / NB) * 1536 * 16));
        // persistent factorisation (pre3_cholp.hip): flag words (zero: every launch brings its own epoch), one plane block per row for the hand-over to crit
        A(dmalloc_bytes(c, &c->cholp_flags, cholp_flag_bytes(c->ldw / 32)));
        {   // the down-date consumers' schedule (pre3_cholp.hip)
            std::vector<int32_t> rec; std::vector<int2> t64;
            dd_build_groups(c->ld / 64, rec, t64, c->dd_tile_off);
            c->dd_n_groups = (int)c->dd_tile_off.size() - 1;
            A(dmalloc_bytes(c, &c->dd_groups, sizeof(int32_t) * rec.size()));
            A(dmalloc_bytes(c, &c->dd_tiles, sizeof(int2) * t64.size()));
            if (rc == PRE3_OK && (hipMemcpy(c->dd_groups, rec.data(), sizeof(int32_t) * rec.size(), hipMemcpyHostToDevice) != hipSuccess ||
                                  hipMemcpy(c->dd_tiles, t64.data(), sizeof(int2) * t64.size(), hipMemcpyHostToDevice) != hipSuccess)) { set_error("consumer table upload failed"); rc = PRE3_E_HIP; }
        }
        A(dmalloc_bytes(c, &c->cholp_tp, (size_t)(c->rcap / NB) * 1536 * 16));
        A(dmalloc_bytes(c, &c->jn_q, sizeof(float) * 4 * (size_t)c->ld));
        A(dmalloc_bytes(c, &c->hf_sx, sizeof(unsigned long long) * (2 * NB) * (2 * NB)));      // rows 3..6 of P before the Jnorm pass (GateRide, pre3_geom.hip)
        // (the buffers of the in-launch tail, PRE3_OPT_STEP_TAIL, are allocated when the option is switched on: tail_alloc -- at N = 2000 they are
        //  ~300 MB that the default path never touches)
        if (c->step_tail) A(tail_alloc(c));
        if (knob::pend_hi() != 0 && c->rcap >= 2 * NB && c->rcap / NB <= CP_MAX_NRB + 1) { A(pend_alloc(c)); c->pend_opt = rc == PRE3_OK; }      // PRE3_OPT_PEND_HI
        if (rc == PRE3_OK) { cholp_context_count(c->device, +1); c->cholp_counted = true; }
        const int nt = c->ld / 128, ns = ceil_div(nt, 4);
        std::vector<std::vector<int2>> lists(8);
        for (int SI = 0; SI < ns; ++SI)
            for (int SJ = SI; SJ < ns; ++SJ) {
                int best = 0;
                for (int x = 1; x < 8; ++x) if (lists[x].size() < lists[best].size()) best = x;
                for (int i = SI * 4; i < std::min(nt, SI * 4 + 4); ++i)
                    for (int j = SJ * 4; j < std::min(nt, SJ * 4 + 4); ++j)
                        if (j >= i) lists[best].push_back(make_int2(i, j));
            }
        for (;;) {
            int lo = 0, hi = 0;
            for (int x = 1; x < 8; ++x) { if (lists[x].size() < lists[lo].size()) lo = x; if (lists[x].size() > lists[hi].size()) hi = x; }
            if (lists[hi].size() <= lists[lo].size() + 1) break;
            lists[lo].push_back(lists[hi].back());
            lists[hi].pop_back();
        }
        // whole rounds of large tiles; the left-over tiles (diagonal ones first: a quarter of each is below the diagonal) as 64x64
        std::vector<int2> inter;
        const int total = nt * (nt + 1) / 2;
        size_t pos[8] = { 0 };
        while ((int)inter.size() < total)
            for (int x = 0; x < 8 && (int)inter.size() < total; ++x)
                if (pos[x] < lists[x].size()) inter.push_back(lists[x][pos[x]++]);
        const int n_big = total <= c->num_cus ? total : total / c->num_cus * c->num_cus;
        int n_small_src = total - n_big;
        std::vector<int2> big, small;
        for (int pass = 0; pass < 2; ++pass)                         // pass 0: pick diagonal tiles for splitting, from the back of the order
            for (int k2 = (int)inter.size() - 1; k2 >= 0 && n_small_src > 0; --k2) {
                int2 &t = inter[k2];
                if (t.x < 0 || (pass == 0 && t.x != t.y)) continue;
                for (int a2 = 0; a2 < 2; ++a2)
                    for (int b2 = 0; b2 < 2; ++b2)
                        if (t.x != t.y || b2 >= a2) small.push_back(make_int2(2 * t.x + a2, 2 * t.y + b2));
                t.x = -1; --n_small_src;
            }
        for (const int2 &t : inter) if (t.x >= 0) big.push_back(make_int2((2 * t.x) | (1 << 16), 2 * t.y));
        inter = big;
        inter.insert(inter.end(), small.begin(), small.end());
        c->n_tiles128 = (int)inter.size();
        A(dmalloc_bytes(c, &c->tiles128, sizeof(int2) * inter.size()));
        if (rc == PRE3_OK && hipMemcpy(c->tiles128, inter.data(), sizeof(int2) * inter.size(), hipMemcpyHostToDevice) != hipSuccess) { set_error("tile table upload failed"); rc = PRE3_E_HIP; }
    }
    if (rc == PRE3_OK) A(c->mem.fixed.pin(&c->pinned_stats, sizeof(int32_t) * 16, PIN_DEFAULT));
    if (rc == PRE3_OK) A(c->mem.fixed.pin(&c->mail_host, sizeof(int32_t) * 32, PIN_MAPPED));
    if (rc == PRE3_OK) {
        memset(c->mail_host, 0, sizeof(int32_t) * 32);      // (words 16..19: the staging blocks' "pulled" sequence numbers, stage_wait)
        if (hipHostGetDevicePointer((void **)&c->mail_dev, c->mail_host, 0) != hipSuccess) { set_error("hipHostGetDevicePointer failed"); rc = PRE3_E_HIP; }
    }
    if (rc == PRE3_OK && (hipEventCreate(&c->t0) != hipSuccess || hipEventCreate(&c->t1) != hipSuccess)) { set_error("hipEventCreate failed"); rc = PRE3_E_HIP; }
    if (rc != PRE3_OK) { pre3_destroy(c); return rc; }
    (void)hipMemsetAsync(c->stats, 0, sizeof(int32_t) * 16, c->stream);
    (void)hipMemsetAsync(c->P, 0, (size_t)c->ld * c->ld * c->esz, c->stream);
    (void)stream_drain(c, __func__);
    *out = c;
    return PRE3_OK;
}

int pre3_destroy(pre3_ctx *c)
{
    if (!c) return PRE3_OK;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)stream_drain(c, __func__);
    // an abort started by a deadline may still be inside RCCL, and the collective it unblocks may still touch this context's buffers: joined (within the
    // deadline) and the stream drained again before anything is freed
    if (c->comm && !comm_abort_wait(c->comm, comm_abort_ms(c->comm))) set_error("pre3_destroy: the communicator's abort has not returned: buffers are freed under it");
    else if (c->comm && comm_broken(c->comm) && c->stream) (void)stream_drain(c, __func__);
    if (c->cholp_counted) { cholp_context_count(c->device, -1); c->cholp_counted = false; }
    ic_rank_free(c);
    if (c->comm && c->comm_owned) (void)pre3_comm_destroy((pre3_comm *)c->comm);
    c->comm = nullptr;
    c->mem = CtxMemory();                 // every device and pinned block of the context (the typed pointers dangle from here on)
    free_patch(c);
    free_fast(c);
    for (hipEvent_t e : c->kt.ev) (void)hipEventDestroy(e);
    if (c->t0) (void)hipEventDestroy(c->t0);
    if (c->t1) (void)hipEventDestroy(c->t1);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return PRE3_OK;
}

int pre3_set_option(pre3_ctx *c, int option, int value)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    switch (option) {
    case PRE3_OPT_DEFER_HI: c->defer_hi = value != 0; return PRE3_OK;
    case PRE3_OPT_K9_BF16X3: c->k9_b3 = value != 0 && c->dtype == PRE3_F32 && c->Wp != nullptr; return PRE3_OK;
    case PRE3_OPT_CHOL_PERSIST: c->chol_persist = value != 0; return PRE3_OK;
    case PRE3_OPT_K9_OVERLAP: c->k9_overlap = value != 0; return PRE3_OK;
    case PRE3_OPT_STEP_TAIL:
        // (fp64 contexts have no persistent launch: the option is accepted and stays without effect, pre3_get_option reports 0)
        if (value != 0 && c->dtype == PRE3_F32 && c->Wp != nullptr) { const int rc = tail_alloc(c); if (rc != PRE3_OK) { c->step_tail = false; return rc; } }
        c->step_tail = value != 0;
        return PRE3_OK;
    case PRE3_OPT_PEND_HI:
        // (contexts that cannot take the persistent launch at their capacity -- fp64, more than 16 panels of rows -- accept the option and stay without it: the
        //  pending rows would only ever be flushed, and their planes mirror Wp's size)
        if (value != 0 && c->dtype == PRE3_F32 && c->Wp != nullptr && c->rcap / NB <= CP_MAX_NRB + 1) { const int rc = pend_alloc(c); if (rc != PRE3_OK) { c->pend_opt = false; return rc; } }
        c->pend_opt = value != 0 && c->W_pend != nullptr;
        return PRE3_OK;
    default: set_error("pre3_set_option: unknown option %d", option); return PRE3_E_ARG;
    }
}

int pre3_get_option(pre3_ctx *c, int option, int *value_out)
{
    PRE3_CHECK(c != nullptr && value_out != nullptr, PRE3_E_ARG, "pre3_get_option: null argument");
    switch (option) {
    case PRE3_OPT_DEFER_HI: *value_out = c->defer_hi ? 1 : 0; return PRE3_OK;
    case PRE3_OPT_K9_BF16X3: *value_out = c->k9_b3 ? 1 : 0; return PRE3_OK;
    case PRE3_OPT_CHOL_PERSIST: *value_out = cholp_usable(c, 1) ? 1 : 0; return PRE3_OK;
    case PRE3_OPT_IC_RANKED: *value_out = c->ic_last_ranked ? 1 : 0; return PRE3_OK;
    case PRE3_OPT_IC_ROUTE: *value_out = c->ic_route; return PRE3_OK;
    case PRE3_OPT_K9_OVERLAP: *value_out = c->k9_overlap ? 1 : 0; return PRE3_OK;
    case PRE3_OPT_STEP_TAIL: *value_out = (c->step_tail && c->tail_yp != nullptr) ? 1 : 0; return PRE3_OK;
    case PRE3_OPT_PEND_HI: *value_out = c->pend_opt ? 1 : 0; return PRE3_OK;
    case PRE3_OPT_ROWS_FORM: *value_out = c->rows_form; return PRE3_OK;
    default: set_error("pre3_get_option: unknown option %d", option); return PRE3_E_ARG;
    }
}

int pre3_sync(pre3_ctx *c)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    PRE3_TRY(stream_drain(c, __func__));
    return PRE3_OK;
}

int pre3_set_cam(pre3_ctx *c, const pre3_cam *cam)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    PRE3_CHECK(cam != nullptr && cam->f > 0, PRE3_E_ARG, "pre3_set_cam: invalid camera");
    c->cam = *cam; c->have_cam = true;
    return PRE3_OK;
}

int pre3_set_map(pre3_ctx *c, int N, const int32_t *lm_type)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    PRE3_CHECK(N >= 0 && N <= c->capN, PRE3_E_ARG, "pre3_set_map: N=%d exceeds capacity %d", N, c->capN);
    PRE3_CHECK(N == 0 || lm_type != nullptr, PRE3_E_ARG, "pre3_set_map: null type list");
    std::vector<int32_t> off(N ? N : 1);
    int n = 13;
    for (int i = 0; i < N; ++i) {
        PRE3_CHECK(lm_type[i] == PRE3_INVDEPTH || lm_type[i] == PRE3_CARTESIAN, PRE3_E_ARG, "pre3_set_map: landmark %d has unknown type %d", i, lm_type[i]);
        off[i] = n; n += lm_type[i] == PRE3_INVDEPTH ? 6 : 3;
    }
    PRE3_CHECK(n <= c->capn, PRE3_E_ARG, "pre3_set_map: state size %d exceeds capacity %d", n, c->capn);
    PRE3_TRY(stream_drain(c, __func__));
    if (N) {
        PRE3_HIP(hipMemcpy(c->lm.type, lm_type, sizeof(int32_t) * N, hipMemcpyHostToDevice));
        PRE3_HIP(hipMemcpy(c->lm.off, off.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice));
    }
    c->N = N; c->n = n;
    c->lm_type_host.assign(lm_type, lm_type + N);
    // the P buffer keeps its capacity-sized leading dimension; entries beyond n stay zero
    PRE3_HIP(hipMemset(c->lm.has_h, 0, sizeof(int32_t) * c->capN)); PRE3_HIP(hipMemset(c->lm.has_S, 0, sizeof(int32_t) * c->capN));
    // update_features_info.m:30-44 empties h, H, S, z: a landmark that is measured but never predicted must read zeros, not a previous map's values
    PRE3_HIP(hipMemset(c->lm.h, 0, sizeof(double) * 2 * c->capN)); PRE3_HIP(hipMemset(c->lm.Hc, 0, sizeof(double) * 14 * c->capN));
    PRE3_HIP(hipMemset(c->lm.Hl, 0, sizeof(double) * 12 * c->capN)); PRE3_HIP(hipMemset(c->lm.S, 0, sizeof(double) * 4 * c->capN));
    PRE3_HIP(hipMemset(c->inbox_dev, 0, c->inbox_bytes)); PRE3_HIP(hipMemset(c->lm.li, 0, sizeof(int32_t) * c->capN));
    PRE3_HIP(hipMemset(c->lm.hi, 0, sizeof(int32_t) * c->capN));
    c->m = 0; c->meas_host.clear(); c->measurements_set = false; c->projected = false; c->innovated = false;
    c->x_valid[0] = c->x_valid[1] = false; c->p_which = -1;
    c->booked = false; c->book_s = 0;             // a new map has no book until pre3_set_book (or an empty map's first pre3_map_policy)
    patch_drop_bank(c);                           // ... and no patches (pre3_patch.hip; nothing is queued when there is no bank)
    return PRE3_OK;
}

int pre3_state_size(pre3_ctx *c) { return c ? c->n : PRE3_E_ARG; }

int pre3_set_state(pre3_ctx *c, int which, int n, const double *x, const double *P)
{
    // a fresh state also clears what an earlier state left in the device's error words (a factorisation that was not positive definite, a
    // wait that gave up): the deferred work of the old state is dropped with them
    EntryScope scope(c);
    if (c == nullptr || (scope.rc != PRE3_OK && scope.rc != PRE3_E_NUMERIC && scope.rc != PRE3_E_HIP)) return scope.rc;
    PRE3_HIP(hipSetDevice(c->device));
    (void)stream_drain(c, __func__);
    (void)hipMemsetAsync(c->stats + 6, 0, sizeof(int32_t) * 2, c->stream);
    if (c->mail_host) { c->mail_host[6] = 0; c->mail_host[7] = 0; }
    drop_carried(c);
    PRE3_CHECK(which == PRE3_X_K_K || which == PRE3_X_K_KM1, PRE3_E_ARG, "pre3_set_state: bad selector");
    PRE3_CHECK(n == c->n, PRE3_E_ARG, "pre3_set_state: n=%d but the map defines n=%d", n, c->n);
    PRE3_CHECK(x && P, PRE3_E_ARG, "pre3_set_state: null pointer");
    PRE3_TRY(stream_drain(c, __func__));
    PRE3_HIP(hipMemcpy(which == PRE3_X_K_K ? c->x_kk : c->x_km1, x, sizeof(double) * n, hipMemcpyHostToDevice));
    const int ld = c->ld;
    PRE3_HIP(hipMemset(c->P, 0, (size_t)ld * ld * c->esz));
    if (c->dtype == PRE3_F64) {
        PRE3_HIP(hipMemcpy2D(c->P, (size_t)ld * 8, P, (size_t)n * 8, (size_t)n * 8, n, hipMemcpyHostToDevice));
    } else {
        std::vector<float> tmp((size_t)n * n);
        for (size_t i = 0; i < (size_t)n * n; ++i) tmp[i] = (float)P[i];
        PRE3_HIP(hipMemcpy2D(c->P, (size_t)ld * 4, tmp.data(), (size_t)n * 4, (size_t)n * 4, n, hipMemcpyHostToDevice));
    }
    c->x_valid[which] = true; c->p_which = which; c->hp_all_valid = false;
    return PRE3_OK;
}

int pre3_get_state(pre3_ctx *c, int which, int n, double *x, double *P)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    PRE3_CHECK(which == PRE3_X_K_K || which == PRE3_X_K_KM1, PRE3_E_ARG, "pre3_get_state: bad selector");
    PRE3_CHECK(n == c->n, PRE3_E_ARG, "pre3_get_state: n=%d but the map defines n=%d", n, c->n);
    PRE3_CHECK(c->x_valid[which], PRE3_E_STATE, "pre3_get_state: that estimate has not been computed");
    PRE3_TRY(fetch_stats(c));
    if (x) PRE3_HIP(hipMemcpy(x, which == PRE3_X_K_K ? c->x_kk : c->x_km1, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (P) {
        PRE3_CHECK(c->p_which == which, PRE3_E_STATE, "pre3_get_state: the covariance buffer currently holds the other estimate (it is updated in place)");
        const int ld = c->ld;
        if (c->dtype == PRE3_F64) {
            PRE3_HIP(hipMemcpy2D(P, (size_t)n * 8, c->P, (size_t)ld * 8, (size_t)n * 8, n, hipMemcpyDeviceToHost));
        } else {
            std::vector<float> tmp((size_t)n * n);
            PRE3_HIP(hipMemcpy2D(tmp.data(), (size_t)n * 4, c->P, (size_t)ld * 4, (size_t)n * 4, n, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < (size_t)n * n; ++i) P[i] = (double)tmp[i];
        }
    }
    return PRE3_OK;
}

// The checks every marginal reader makes on the host before anything is launched
static int reader_precheck(pre3_ctx *c, int which, const char *who)
{
    PRE3_CHECK(c != nullptr, PRE3_E_ARG, "null context");
    PRE3_CHECK(which == PRE3_X_K_K || which == PRE3_X_K_KM1, PRE3_E_ARG, "%s: bad selector", who);
    PRE3_CHECK(c->x_valid[which], PRE3_E_STATE, "%s: that estimate has not been computed", who);
    PRE3_CHECK(c->p_which == which, PRE3_E_STATE, "%s: the covariance buffer currently holds the other estimate (it is updated in place)", who);
    return PRE3_OK;
}
// Entry::reader has completed a deferred HI update as pre3_step would complete it (its rows/cols 3..6 pass left to the next prediction's launch) and
// flushed nothing that is pending: the filter's next step runs exactly as it would have without the read.  Returns the pending pass's Jn on the device, or null.
static int reader_settle(pre3_ctx *c, const double **jn)
{
    // fetch_stats with the reader's own synchronisation: the error words leave in front of the gather, and are checked once the stream has drained
    PRE3_HIP(hipMemcpyAsync(c->pinned_stats, c->stats, sizeof(int32_t) * 16, hipMemcpyDeviceToHost, c->stream));
    *jn = c->carry.jn_pending ? c->pred_params + 16 : nullptr;     // (k_jnorm_P's Jn: params[16..31])
    return PRE3_OK;
}
static int reader_finish(pre3_ctx *c, int rc)
{
    PRE3_TRY(rc);
    PRE3_TRY(stream_drain(c, __func__));
    return stats_words(c);
}

int pre3_get_landmarks(pre3_ctx *c, int which, int first, int count, double *xyz, double *cov_xyz, double *cov_native, double *linearity)
{
    PRE3_TRY(reader_precheck(c, which, "pre3_get_landmarks"));
    PRE3_CHECK(first >= 0 && count >= 0 && (long long)first + count <= c->N, PRE3_E_ARG, "pre3_get_landmarks: landmarks %d .. %d outside the map (N=%d)", first, first + count - 1, c->N);
    EntryScope scope(c, Entry::reader); PRE3_TRY(scope.rc);
    const double *jn = nullptr;
    PRE3_TRY(reader_settle(c, &jn));
    return reader_finish(c, c->N == 0 ? PRE3_OK : read_landmarks(c, which, first, count, xyz, cov_xyz, cov_native, linearity));
}

int pre3_get_marginal(pre3_ctx *c, int which, int k, const int32_t *idx, double *x_out, double *P_out)
{
    PRE3_TRY(reader_precheck(c, which, "pre3_get_marginal"));
    PRE3_CHECK(k >= 0 && (k == 0 || idx != nullptr), PRE3_E_ARG, "pre3_get_marginal: bad index set");
    PRE3_CHECK(ceil_div(k, 16) <= 65535, PRE3_E_ARG, "pre3_get_marginal: k=%d indices exceed the launch grid", k);
    for (int t = 0; t < k; ++t)
        PRE3_CHECK(idx[t] >= 0 && idx[t] < c->n, PRE3_E_ARG, "pre3_get_marginal: index %d outside the state (n=%d)", idx[t], c->n);
    EntryScope scope(c, Entry::reader); PRE3_TRY(scope.rc);
    const double *jn = nullptr;
    PRE3_TRY(reader_settle(c, &jn));
    return reader_finish(c, read_marginal(c, which, k, idx, jn, x_out, P_out));
}

int pre3_predict(pre3_ctx *c, const double u[7])
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    PRE3_CHECK(u != nullptr, PRE3_E_ARG, "pre3_predict: null u");
    PRE3_CHECK(c->x_valid[PRE3_X_K_K] && c->p_which == PRE3_X_K_K, PRE3_E_STATE, "pre3_predict: needs (x_k_k, p_k_k) on the device");
    PRE3_TRY(launch_predict_impl(c, u));
    c->x_valid[PRE3_X_K_KM1] = true; c->p_which = PRE3_X_K_KM1; c->hp_all_valid = false;
    return PRE3_OK;
}

// The camera-only prediction (include/pre3.h).  The argument and state checks come before the scope: a refused call queues nothing and
// leaves deferred and pending work where it was.  A pending update.m:42-46 pass belongs IN FRONT of this prediction: it goes out as its own launch here --
// left to the scope's destructor it would run behind k_predict_cv, on the predicted covariance.
int pre3_predict_cv(pre3_ctx *c, int type, double dt, double sigma_a, double sigma_alpha)
{
    PRE3_CHECK(c != nullptr, PRE3_E_ARG, "null context");
    PRE3_CHECK(type >= 0 && type < CV_N_TYPES, PRE3_E_ARG, "pre3_predict_cv: type %d outside 0..3", type);
    PRE3_CHECK(std::isfinite(dt) && dt > 0, PRE3_E_ARG, "pre3_predict_cv: dt must be finite and positive");
    PRE3_CHECK(std::isfinite(sigma_a) && sigma_a >= 0 && std::isfinite(sigma_alpha) && sigma_alpha >= 0, PRE3_E_ARG, "pre3_predict_cv: the sigmas must be finite and not negative");
    PRE3_CHECK(c->x_valid[PRE3_X_K_K] && c->p_which == PRE3_X_K_K, PRE3_E_STATE, "pre3_predict_cv: needs (x_k_k, p_k_k) on the device");
    EntryScope scope(c); PRE3_TRY(scope.rc);
    if (c->carry.jn_pending) { c->carry.jn_pending = false; PRE3_TRY(launch_jnorm(c, 0)); }
    PRE3_TRY(launch_predict_cv(c, type, dt, sigma_a, sigma_alpha));
    c->x_valid[PRE3_X_K_KM1] = true; c->p_which = PRE3_X_K_KM1; c->hp_all_valid = false;
    return PRE3_OK;
}

// predict_state_and_covariance.m:98-102,115: the Pn every prediction of this context takes.  A setting, not a step: deferred and
// pending work is left where it is (no EntryScope), and the block changes in stream order behind the predictions already queued.
int pre3_set_process_noise(pre3_ctx *c, const double *Pn)
{
    PRE3_CHECK(c != nullptr, PRE3_E_ARG, "pre3_set_process_noise: null context");
    if (Pn == nullptr) { c->pn_set = false; return PRE3_OK; }
    PRE3_TRY(process_noise_check("pre3_set_process_noise", Pn));
    PRE3_HIP(hipSetDevice(c->device));
    PRE3_TRY(launch_set_pn(c, Pn));
    memcpy(c->pn_host, Pn, sizeof c->pn_host);
    c->pn_set = true;
    return PRE3_OK;
}

int pre3_get_process_noise(pre3_ctx *c, double *Pn_out, int *source_out)
{
    PRE3_CHECK(c != nullptr && (Pn_out != nullptr || source_out != nullptr), PRE3_E_ARG, "pre3_get_process_noise: null argument");
    if (source_out) *source_out = c->pn_set ? 1 : 0;
    if (Pn_out == nullptr) return PRE3_OK;
    if (c->pn_set) { memcpy(Pn_out, c->pn_host, sizeof c->pn_host); return PRE3_OK; }
    // the constant as the prediction's launch builds it: written into the (unused while nothing is set) block on the context's stream and read back
    PRE3_HIP(hipSetDevice(c->device));
    PRE3_TRY(launch_get_pn_const(c, c->pred_params + PRED_PN_OFF));
    PRE3_HIP(hipMemcpyAsync(Pn_out, c->pred_params + PRED_PN_OFF, sizeof(double) * 49, hipMemcpyDeviceToHost, c->stream));
    PRE3_TRY(stream_drain(c, "pre3_get_process_noise"));
    return PRE3_OK;
}

int pre3_project(pre3_ctx *c, int which, int clear_first)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    PRE3_CHECK(which == PRE3_X_K_K || which == PRE3_X_K_KM1, PRE3_E_ARG, "pre3_project: bad selector");
    PRE3_CHECK(c->have_cam, PRE3_E_STATE, "pre3_project: camera not set");
    PRE3_CHECK(c->x_valid[which], PRE3_E_STATE, "pre3_project: that estimate is not on the device");
    if (c->N == 0) return PRE3_OK;
    PRE3_TRY(launch_project(c, which, clear_first));
    c->projected = true;
    return PRE3_OK;
}

int pre3_innovation(pre3_ctx *c)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    PRE3_CHECK(c->projected, PRE3_E_STATE, "pre3_innovation: call pre3_project first");
    if (c->N == 0) return PRE3_OK;
    PRE3_TRY(launch_innovation(c, 0, 0.0));
    c->innovated = true;
    return PRE3_OK;
}

int pre3_get_landmark_fields(pre3_ctx *c, double *h, int32_t *has_h, double *Hc, double *Hl, double *S)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    PRE3_TRY(stream_drain(c, __func__));
    int N = c->N;
    if (N == 0) return PRE3_OK;
    if (h) PRE3_HIP(hipMemcpy(h, c->lm.h, sizeof(double) * 2 * N, hipMemcpyDeviceToHost));
    if (has_h) PRE3_HIP(hipMemcpy(has_h, c->lm.has_h, sizeof(int32_t) * N, hipMemcpyDeviceToHost));
    if (Hc) PRE3_HIP(hipMemcpy(Hc, c->lm.Hc, sizeof(double) * 14 * N, hipMemcpyDeviceToHost));
    if (Hl) PRE3_HIP(hipMemcpy(Hl, c->lm.Hl, sizeof(double) * 12 * N, hipMemcpyDeviceToHost));
    if (S) PRE3_HIP(hipMemcpy(S, c->lm.S, sizeof(double) * 4 * N, hipMemcpyDeviceToHost));
    return PRE3_OK;
}

int pre3_set_measurements(pre3_ctx *c, int m, const int32_t *meas_idx, const double *z)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    PRE3_CHECK(m == 0 || (meas_idx && z), PRE3_E_ARG, "pre3_set_measurements: null pointer");
    return install_measurements(c, m, meas_idx, z, nullptr, 0);
}

int pre3_window_gate(pre3_ctx *c, int M, const int32_t *k1, const double *zc, int strict_reference, int32_t *accept_out)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    PRE3_CHECK(c->projected, PRE3_E_STATE, "pre3_window_gate: call pre3_project / pre3_innovation first");
    PRE3_CHECK(M >= 0 && (M == 0 || (k1 && zc)), PRE3_E_ARG, "pre3_window_gate: bad arguments");
    int N = c->N;
    std::vector<int32_t> has_h(N ? N : 1), pred;
    PRE3_TRY(stream_drain(c, __func__));
    if (N) PRE3_HIP(hipMemcpy(has_h.data(), c->lm.has_h, sizeof(int32_t) * N, hipMemcpyDeviceToHost));
    for (int i = 0; i < N; ++i) if (has_h[i]) pred.push_back(i);
    PRE3_CHECK(M <= (int)pred.size(), PRE3_E_ARG, "pre3_window_gate: %d candidates but only %zu predicted landmarks", M, pred.size());
    for (int q = 0; q < M; ++q) PRE3_CHECK(k1[q] >= 0 && k1[q] < (int)pred.size(), PRE3_E_ARG, "pre3_window_gate: k1[%d]=%d out of range", q, k1[q]);
    std::vector<int32_t> acc(M ? M : 1, 0);
    if (M) {
        // temporaries, released on every exit path
        BlockList tmp;
        int32_t *d_pred = nullptr, *d_k1 = nullptr, *d_acc = nullptr; double *d_zc = nullptr;
        PRE3_TRY(tmp.dev(&d_pred, sizeof(int32_t) * pred.size(), Zero::sync()));
        PRE3_TRY(tmp.dev(&d_k1, sizeof(int32_t) * M, Zero::sync()));
        PRE3_TRY(tmp.dev(&d_acc, sizeof(int32_t) * M, Zero::sync()));
        PRE3_TRY(tmp.dev(&d_zc, sizeof(double) * 2 * (size_t)M, Zero::sync()));
        PRE3_HIP(hipMemcpy(d_pred, pred.data(), sizeof(int32_t) * pred.size(), hipMemcpyHostToDevice));
        PRE3_HIP(hipMemcpy(d_k1, k1, sizeof(int32_t) * M, hipMemcpyHostToDevice));
        PRE3_HIP(hipMemcpy(d_zc, zc, sizeof(double) * 2 * M, hipMemcpyHostToDevice));
        PRE3_HIP(hipMemsetAsync(c->lm.ic, 0, sizeof(int32_t) * N, c->stream));
        PRE3_TRY(launch_window_gate(c, M, d_pred, d_k1, d_zc, strict_reference, d_acc));
        PRE3_TRY(stream_drain(c, __func__));
        PRE3_HIP(hipMemcpy(acc.data(), d_acc, sizeof(int32_t) * M, hipMemcpyDeviceToHost));
    }
    // accepted candidates become the measurement list (ascending landmark order; one match per landmark)
    std::vector<int32_t> flag(N ? N : 1, 0);
    for (int q = 0; q < M; ++q) if (acc[q]) flag[pred[k1[q]]] = 1;
    std::vector<int32_t> meas;
    for (int i = 0; i < N; ++i) if (flag[i]) meas.push_back(i);
    if (accept_out) for (int q = 0; q < M; ++q) accept_out[q] = acc[q];
    // z was written on the device by the gate kernel; keep it (z == nullptr)
    return install_measurements(c, (int)meas.size(), meas.data(), nullptr, nullptr, 0);
}

// ---- IC search on the device ---------------------------------------------------------
static int ensure_ic_buffers(pre3_ctx *c)
{
    if (c->ic_ready) return PRE3_OK;
    const size_t N = (size_t)c->capN;
    Group g(c->mem.fixed, c->ic_ready);       // complete, or gone with its pointers null: a call after a failed one starts over
    auto D = [&](auto **p, size_t count) { return g.dev(p, sizeof(**p) * count, Zero::sync()); };      // (dmalloc's zeroing)
    PRE3_TRY(D(&c->bank, N * DESC_DIM)); PRE3_TRY(D(&c->bank_alt, N * DESC_DIM));
    // result block, fetched with ONE copy: [counts(4) | meas(capN) | pairs(3 capN) | z(2 capN doubles)]
    PRE3_TRY(D(&c->ic_pred, N)); PRE3_TRY(D(&c->ic_counts, 4 + 4 * N + 4 * N + 4)); PRE3_TRY(D(&c->ic_arg, N));
    c->ic_pairs = c->ic_counts + 4 + N; g.alias(&c->ic_pairs);
    PRE3_HIP(hipMemset(c->ic_counts, 0, sizeof(int32_t) * (4 + 8 * N)));
    PRE3_TRY(D(&c->ic_newk2, N)); PRE3_TRY(D(&c->ic_best, N)); PRE3_TRY(D(&c->ic_second, N)); PRE3_TRY(D(&c->bank_src, N));
    PRE3_HIP(hipMemset(c->bank, 0, sizeof(double) * N * DESC_DIM));
    const size_t blk_bytes = (sizeof(int32_t) * (4 + 4 * N) + sizeof(double) * 2 * N + 15) & ~(size_t)15;
    PRE3_TRY(g.pin(&c->ic_result_host, blk_bytes, PIN_MAPPED));
    g.alias(&c->ic_result_host_dev);
    PRE3_HIP(hipHostGetDevicePointer(&c->ic_result_host_dev, c->ic_result_host, 0));
    g.commit();
    return PRE3_OK;
}

// k_rank_pack's test of its input, on the host: every value finite with |x| <= 2^60 and no non-zero |x| < 2^-40 (an or-reduction of two
// compares per value), made on the way into the staging block: one pass over the caller's array instead of a copy and a second read
// (AVX2 where the host has it: 36 us for copy + check of 600 keypoints -> see DESIGN.md section 11)
__attribute__((target("avx2"))) static bool copy_desc_checked_avx2(double *__restrict__ dst, const double *__restrict__ src, size_t count)
{
    const __m256d absmask = _mm256_castsi256_pd(_mm256_set1_epi64x(0x7fffffffffffffffLL)), hi = _mm256_set1_pd(0x1p60), lo = _mm256_set1_pd(0x1p-40), zero = _mm256_setzero_pd();
    __m256d bad = zero;
    size_t i = 0;
    for (; i + 8 <= count; i += 8) {
        const __m256d v0 = _mm256_loadu_pd(src + i), v1 = _mm256_loadu_pd(src + i + 4);
        _mm256_storeu_pd(dst + i, v0); _mm256_storeu_pd(dst + i + 4, v1);
        const __m256d a0 = _mm256_and_pd(v0, absmask), a1 = _mm256_and_pd(v1, absmask);
        // !(ax <= 2^60) (true for NaN too)  |  (ax != 0 && ax < 2^-40)
        bad = _mm256_or_pd(bad, _mm256_cmp_pd(a0, hi, _CMP_NLE_UQ)); bad = _mm256_or_pd(bad, _mm256_cmp_pd(a1, hi, _CMP_NLE_UQ));
        bad = _mm256_or_pd(bad, _mm256_and_pd(_mm256_cmp_pd(a0, zero, _CMP_NEQ_OQ), _mm256_cmp_pd(a0, lo, _CMP_LT_OQ)));
        bad = _mm256_or_pd(bad, _mm256_and_pd(_mm256_cmp_pd(a1, zero, _CMP_NEQ_OQ), _mm256_cmp_pd(a1, lo, _CMP_LT_OQ)));
    }
    int b = _mm256_movemask_pd(bad);
    for (; i < count; ++i) {
        const double v = src[i], ax = fabs(v);
        dst[i] = v;
        b |= (int)!(ax <= 0x1p60);
        b |= (int)(ax != 0.0) & (int)(ax < 0x1p-40);
    }
    return b == 0;
}
static bool copy_desc_checked(double *__restrict__ dst, const double *__restrict__ src, size_t count)
{
    static const bool avx2 = __builtin_cpu_supports("avx2");
    if (avx2) return copy_desc_checked_avx2(dst, src, count);
    int bad = 0;
    for (size_t i = 0; i < count; ++i) {
        const double v = src[i], ax = fabs(v);
        dst[i] = v;
        bad |= (int)!(ax <= 0x1p60);
        bad |= (int)(ax != 0.0) & (int)(ax < 0x1p-40);
    }
    return bad == 0;
}

}  // extern "C"
// a process noise's three checks (pre3_set_process_noise, pre3_relocalise_seeded): finite, no negative diagonal entry, exactly symmetric
int pre3::process_noise_check(const char *who, const double *Pn)
{
    for (int i = 0; i < 49; ++i) PRE3_CHECK(std::isfinite(Pn[i]), PRE3_E_ARG, "%s: Pn[%d] is not finite", who, i);
    for (int i = 0; i < 7; ++i) {
        PRE3_CHECK(Pn[8 * i] >= 0, PRE3_E_ARG, "%s: the diagonal entry %d is negative", who, i);
        for (int j = 0; j < i; ++j) PRE3_CHECK(Pn[7 * i + j] == Pn[7 * j + i], PRE3_E_ARG, "%s: Pn(%d,%d) != Pn(%d,%d)", who, i, j, j, i);
    }
    return PRE3_OK;
}
bool pre3::desc_copy_checked(double *dst, const double *src, size_t count) { return copy_desc_checked(dst, src, count); }
// A pinned block of the context for `bytes` of host data on their way to the device: two blocks, used alternately, grown on demand; a block is
// written again only after the pull of its previous contents has run (its sequence number in the mailbox: stage_wait).  The caller fills *host, enqueues the pull from *dev on the
// context's stream and calls stage_release.
int pre3::stage_acquire(pre3_ctx *c, size_t bytes, void **host, void **dev, int *slot)
{
    PRE3_TRY(c->mem.up_ring.acquire(bytes, (bytes + 65535) & ~(size_t)65535, host, slot));
    PRE3_HIP(hipHostGetDevicePointer(dev, *host, 0));
    return PRE3_OK;
}
int pre3::stage_release(pre3_ctx *c, int slot)        // (the pull launched with stage_done(c, slot) announces itself)
{
    c->mem.up_ring.release(slot);
    return PRE3_OK;
}

int pre3::set_descriptors_impl(pre3_ctx *c, int first, int count, const double *desc)
{
    PRE3_CHECK(first >= 0 && count >= 0 && first + count <= c->N && (count == 0 || desc), PRE3_E_ARG, "pre3_set_descriptors: range [%d, %d) outside the map (N=%d)", first, first + count, c->N);
    PRE3_TRY(ensure_ic_buffers(c));
    bool ok = true;
    if (count) {
        // staged and pulled on the context's stream like the scan (pre3_set_scan): map management calls this once per frame for the new
        // landmark -- it used to cost a stream synchronisation, a blocking copy and a device-side bounds check with a read-back
        const size_t nd = (size_t)count * DESC_DIM;
        void *st = nullptr, *st_dev = nullptr; int slot = 0;
        PRE3_TRY(stage_acquire(c, sizeof(double) * nd, &st, &st_dev, &slot));
        ok = copy_desc_checked(static_cast<double *>(st), desc, nd);
        hipLaunchKernelGGL(k_scan_pull, dim3(ceil_div((int)(nd / 2), 256)), dim3(256), 0, c->stream, (const int4 *)st_dev, (int)(nd / 2),
                           (int4 *)(c->bank + (size_t)first * DESC_DIM), 0, (int4 *)nullptr, stage_done(c, slot));
        PRE3_HIP(hipGetLastError());
        PRE3_TRY(stage_release(c, slot));
    }
    c->bank_set = true;
    if (!ok) c->bank_ok = false;            // (sticky until the whole bank is rewritten: a bad descriptor may stay in the map)
    else if (first == 0 && count >= c->N) c->bank_ok = true;
    return PRE3_OK;
}
// set_descriptors_impl with the source on the device: nothing is staged; in_bounds is the caller's knowledge of copy_desc_checked's test
int pre3::set_descriptors_rows_dev(pre3_ctx *c, int first, int count, const double *des_dev, const int32_t *rows_dev, int n_rows, bool in_bounds)
{
    PRE3_CHECK(first >= 0 && count >= 0 && first + count <= c->N && (count == 0 || (des_dev && rows_dev && n_rows > 0)), PRE3_E_ARG,
               "descriptors from a keypoint block: range [%d, %d) outside the map (N=%d)", first, first + count, c->N);
    PRE3_CHECK(((uintptr_t)des_dev & 15) == 0, PRE3_E_ARG, "descriptors from a keypoint block: the block is not 16-byte aligned");
    PRE3_TRY(ensure_ic_buffers(c));
    if (count) {
        hipLaunchKernelGGL(k_fc_desc, dim3(count), dim3(DESC_DIM / 2), 0, c->stream, n_rows, rows_dev, des_dev, c->bank + (size_t)first * DESC_DIM);
        PRE3_HIP(hipGetLastError());
    }
    c->bank_set = true;
    if (!in_bounds) c->bank_ok = false;
    else if (first == 0 && count >= c->N) c->bank_ok = true;
    return PRE3_OK;
}
extern "C" {

int pre3_set_descriptors(pre3_ctx *c, int first, int count, const double *desc)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    return set_descriptors_impl(c, first, count, desc);
}

int pre3_get_descriptors(pre3_ctx *c, int first, int count, double *desc)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    PRE3_CHECK(first >= 0 && count >= 0 && first + count <= c->N && (count == 0 || desc), PRE3_E_ARG, "pre3_get_descriptors: range outside the map");
    PRE3_CHECK(c->bank_set, PRE3_E_STATE, "pre3_get_descriptors: no descriptors have been set");
    PRE3_TRY(stream_drain(c, __func__));
    if (count) PRE3_HIP(hipMemcpy(desc, c->bank + (size_t)first * DESC_DIM, sizeof(double) * (size_t)count * DESC_DIM, hipMemcpyDeviceToHost));
    return PRE3_OK;
}

// room for a scan of K2 keypoints and the IC search's partial arrays; *grew (may be null): the buffers were replaced
static int scan_reserve(pre3_ctx *c, int K2, bool *grew)
{
    if (grew) *grew = false;
    if (K2 > c->scan_cap) {
        PRE3_TRY(stream_drain(c, __func__));             // (the buffers being replaced may still be read by queued kernels)
        CtxMemory &m = c->mem;
        for (DevBlock *b : { &m.scan_desc, &m.scan_pos, &m.ic_pb, &m.ic_ps, &m.ic_pa }) b->release();      // all five first: the peak does not rise
        c->scan_desc = c->scan_pos = nullptr; c->ic_pb = c->ic_ps = nullptr; c->ic_pa = nullptr; c->scan_cap = 0; c->ic_pcap = 0;
        const int cap = round_up(K2, 256);
        // [scan_cap/64][capN] for the 64-wide tiles; the fused route: [capN][64 column tiles of 32]; pre3_relocalise_seeded: [scan_cap/32][capN], whatever K2
        const size_t np = std::max((size_t)(cap / ICS_T) * c->capN, (size_t)64 * c->capN);
        const size_t b_desc = sizeof(double) * cap * DESC_DIM, b_pos = sizeof(double) * cap * 4, b_d = sizeof(double) * np, b_i = sizeof(int32_t) * np;
        PRE3_TRY(m.scan_desc.reserve(b_desc, b_desc, Zero::sync())); PRE3_TRY(m.scan_pos.reserve(b_pos, b_pos, Zero::sync()));
        PRE3_TRY(m.ic_pb.reserve(b_d, b_d, Zero::sync())); PRE3_TRY(m.ic_ps.reserve(b_d, b_d, Zero::sync())); PRE3_TRY(m.ic_pa.reserve(b_i, b_i, Zero::sync()));
        c->scan_desc = m.scan_desc.as<double>(); c->scan_pos = m.scan_pos.as<double>();
        c->ic_pb = m.ic_pb.as<double>(); c->ic_ps = m.ic_ps.as<double>(); c->ic_pa = m.ic_pa.as<int32_t>();
        c->ic_pcap = np; c->scan_cap = cap;
        if (grew) *grew = true;
    }
    return PRE3_OK;
}

int pre3_set_scan(pre3_ctx *c, int K2, const double *descriptor_raw, const double *scale_orient_pos_raw)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    PRE3_CHECK(K2 >= 0 && (K2 == 0 || (descriptor_raw && scale_orient_pos_raw)), PRE3_E_ARG, "pre3_set_scan: bad arguments");
    bool grew = false;
    PRE3_TRY(scan_reserve(c, K2, &grew));
    // (as pre3_set_scan_frame: the new buffers are zeroed on the null stream, which the context's stream does not wait for -- the pull below writes the
    //  scan, and pre3_relocalise_seeded's matcher the partial arrays, right behind this call)
    if (grew) PRE3_HIP(hipStreamSynchronize(0));
    bool in_bounds = true;
    if (K2) {
        // The frame's scan crosses PCIe from a pinned block of the context's own, enqueued on its stream: the call neither waits for the queued
        // work nor ends in a read-back.  The bounds the ranked route needs of the descriptors (k_rank_pack's test: finite, |x| <= 2^60, no
        // non-zero |x| < 2^-40) are checked here, on the way into that block.
        const int trace = knob::scan_trace();
        const auto t0 = std::chrono::steady_clock::now();
        void *st_v = nullptr, *st_dev = nullptr; int k = 0;
        PRE3_TRY(stage_acquire(c, sizeof(double) * (size_t)K2 * (DESC_DIM + 4), &st_v, &st_dev, &k));
        const auto t1 = std::chrono::steady_clock::now();
        double *st = static_cast<double *>(st_v);
        const size_t nd = (size_t)K2 * DESC_DIM;
        in_bounds = copy_desc_checked(st, descriptor_raw, nd);
        const auto t2 = std::chrono::steady_clock::now();
        memcpy(st + nd, scale_orient_pos_raw, sizeof(double) * (size_t)K2 * 4);
        const auto t3 = std::chrono::steady_clock::now();
        // the device reads the block over PCIe itself (16 bytes per lane, every request in flight at once: ~20 us for 600 keypoints) instead of
        // two DMA-engine copies with their start-up latencies
        const int n16_desc = (int)(nd / 2), n16_pos = K2 * 2;
        hipLaunchKernelGGL(k_scan_pull, dim3(ceil_div(n16_desc + n16_pos, 256)), dim3(256), 0, c->stream, (const int4 *)st_dev, n16_desc, (int4 *)c->scan_desc, n16_pos, (int4 *)c->scan_pos, stage_done(c, k));
        PRE3_HIP(hipGetLastError());
        PRE3_TRY(stage_release(c, k));
        if (trace) { const auto t4 = std::chrono::steady_clock::now(); auto us = [](auto a, auto b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
            fprintf(stderr, "[pre3 set_scan, us] event wait %.1f | descriptors copied + checked %.1f | positions %.1f | enqueue %.1f\n", us(t0, t1), us(t1, t2), us(t2, t3), us(t3, t4)); }
    }
    c->scan_K2 = K2;
    return ic_rank_set_scan(c, in_bounds);
}

// matching_sift_based.m:104,129-135 with the scan taken from a resident frame's keypoint block
int pre3_set_scan_frame(pre3_ctx *c, pre3_sr_frame *f, int which)
{
    const char *who = "pre3_set_scan_frame";
    PRE3_CHECK(c != nullptr, PRE3_E_ARG, "%s: null context", who);
    PRE3_CHECK(f != nullptr, PRE3_E_ARG, "%s: null handle", who);
    PRE3_CHECK(which == 0 || which == 1, PRE3_E_ARG, "%s: which=%d is neither 0 (the raw set) nor 1 (the kept set)", who, which);
    SrFrameView v;
    SrKeypointView kv;
    PRE3_TRY(sr_frame_view(f, &v));
    PRE3_CHECK(v.device == c->device, PRE3_E_ARG, "%s: the frame is on device %d, the context on device %d", who, v.device, c->device);
    PRE3_TRY(sr_frame_keypoint_view(f, &kv));
    PRE3_CHECK(kv.ND == DESC_DIM, PRE3_E_ARG, "%s: descriptors of %d entries (the IC search matches %d)", who, kv.ND, DESC_DIM);
    PRE3_CHECK(kv.ldf >= 2, PRE3_E_ARG, "%s: ldf=%d (a frame holds at least the pixel column and row)", who, kv.ldf);
    const int K2 = which == 0 ? kv.K_in : kv.n_kept;
    const double *frm = which == 0 ? kv.frm_in : kv.frm, *des = which == 0 ? kv.des_in : kv.des;
    PRE3_CHECK(K2 == 0 || (frm != nullptr && des != nullptr && ((uintptr_t)des & 15) == 0 && ((uintptr_t)frm & 15) == 0), PRE3_E_HIP,
               "%s: the keypoint block is not laid out as expected", who);
    EntryScope scope(c); PRE3_TRY(scope.rc);
    bool grew = false;
    PRE3_TRY(scan_reserve(c, K2, &grew));
    if (grew) PRE3_HIP(hipStreamSynchronize(0));         // (the new buffers are zeroed on the null stream, which the context's stream does not wait for)
    if (K2) {
        // the frame is lent to the context's stream (the keypoint stage has been waited for already) and reclaimed behind the copy, so that a load or a
        // keypoint call that follows cannot overwrite the block under it
        PRE3_TRY(sr_frame_lend(f, c->stream));
        hipLaunchKernelGGL(k_scan_frame, dim3(ceil_div(K2 * (DESC_DIM / 2) + K2, 256)), dim3(256), 0, c->stream, K2, kv.ldf, frm, des, c->scan_desc, c->scan_pos);
        PRE3_HIP(hipGetLastError());
        PRE3_TRY(sr_frame_reclaim(f, c->stream));
    }
    c->scan_K2 = K2;
    return ic_rank_set_scan(c, kv.raw_in_bounds);        // (which = 1: the kept set is a subset of the raw one)
}

int pre3_ic_search(pre3_ctx *c, double thresh, int strict_reference, int32_t *n_matches_out, int32_t *m_out, int32_t *meas_idx_out,
                   double *z_out, int32_t *pairs_out)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    PRE3_CHECK(c->bank_set, PRE3_E_STATE, "pre3_ic_search: call pre3_set_descriptors first");
    PRE3_CHECK(c->scan_K2 >= 0 && (c->scan_K2 == 0 || c->scan_desc), PRE3_E_STATE, "pre3_ic_search: call pre3_set_scan first");
    PRE3_CHECK(c->x_valid[PRE3_X_K_KM1] && c->p_which == PRE3_X_K_KM1, PRE3_E_STATE, "pre3_ic_search: needs the predicted estimate (call pre3_predict first)");
    PRE3_CHECK(m_out != nullptr, PRE3_E_ARG, "pre3_ic_search: null m_out");
    const int N = c->N;
    if (N == 0) {
        // matching_sift_based.m:115 `if isempty(des1) return`: a SLAM run starts with an empty map -- nothing to match, no measurements
        if (n_matches_out) *n_matches_out = 0;
        *m_out = 0;
        c->projected = true; c->innovated = true;
        return install_measurements(c, 0, nullptr, nullptr, nullptr, 0);
    }
    // search_IC_matches.m:31-44: h, H and S for every landmark at the prediction
    PRE3_CHECK(c->have_cam, PRE3_E_STATE, "pre3_ic_search: camera not set");
    const bool fused = ic_search_fused_applies(c);
    const IcMatchRide ride = fused ? ic_match_ride(c) : IcMatchRide{};          // the fused route's matcher tiles ride in the projection's launch
    if (N) PRE3_TRY(launch_project_innovation(c, PRE3_X_K_KM1, 1, 0, 0.0, true, true, ride.n_blocks ? &ride : nullptr));      // (also clears individually_compatible of every landmark)
    c->projected = true; c->innovated = true;
    // the result block [counts | meas | pairs | z] is written into mapped pinned memory by the device itself and announced through the mailbox:
    // no DMA-engine copy, no stream synchronisation (the host polls one word)
    const size_t capN = (size_t)c->capN, blk_bytes = sizeof(int32_t) * (4 + 4 * capN) + sizeof(double) * 2 * capN;
    if (fused) {
        // the reference's real sizes: exact matcher + (stack, merge, gate, refresh, result block) as two launches (pre3_match.hip)
        c->ic_last_ranked = false;
        PRE3_TRY(launch_ic_search_fused(c, thresh, strict_reference, ++c->seq_ic, 12, ride.n_blocks > 0));
    } else {
        PRE3_TRY(launch_ic_search(c, thresh, strict_reference));
        PRE3_TRY(launch_inbox_pull(c, c->ic_counts, c->ic_result_host_dev, (blk_bytes + 15) / 16, ++c->seq_ic, 12));
    }
    PRE3_TRY(wait_mail(c, 12, c->seq_ic));
    const int32_t *blk_p = static_cast<const int32_t *>(c->ic_result_host);
    std::vector<int32_t> blk(blk_p, blk_p + (4 + 4 * capN + 4 * capN));
    const int32_t *counts = blk.data();
    const int n_match = c->scan_K2 > 0 ? counts[1] : 0, m = c->scan_K2 > 0 ? counts[2] : 0;
    PRE3_CHECK(m >= 0 && m <= N && n_match >= 0 && n_match <= N, PRE3_E_STATE, "pre3_ic_search: inconsistent counts (%d matches, %d accepted)", n_match, m);
    std::vector<int32_t> meas(blk.begin() + 4, blk.begin() + 4 + m);
    if (n_matches_out) *n_matches_out = n_match;
    if (pairs_out) for (int i = 0; i < 3 * n_match; ++i) pairs_out[i] = blk[4 + capN + i];
    *m_out = m;
    if (meas_idx_out) for (int j = 0; j < m; ++j) meas_idx_out[j] = meas[j];
    if (z_out) { const double *zz = (const double *)(blk.data() + 4 + 4 * capN); for (int j = 0; j < 2 * m; ++j) z_out[j] = zz[j]; }
    return install_measurements(c, (int)meas.size(), meas.data(), nullptr, nullptr, 0);
}

// ---- the patch branch of the IC search (search_IC_matches.m:45-51; pre3_patch.hip) ---------------
int pre3_set_image(pre3_ctx *c, int nRows, int nCols, const uint8_t *im)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    return patch_set_image(c, nRows, nCols, im);
}
int pre3_get_image(pre3_ctx *c, int nRows, int nCols, uint8_t *im)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    return patch_get_image(c, nRows, nCols, im);
}
int pre3_set_image_frame(pre3_ctx *c, pre3_sr_frame *f)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    return patch_set_image_frame(c, f);
}
int pre3_set_patches(pre3_ctx *c, int first, int count, const uint8_t *patch, const double *uv_init, const double *r_wc, const double *R_wc)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    return patch_set_patches(c, first, count, patch, uv_init, r_wc, R_wc);
}
int pre3_get_patches(pre3_ctx *c, int first, int count, uint8_t *patch, double *uv_init, double *r_wc, double *R_wc, int32_t *has_patch)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    return patch_get_patches(c, first, count, patch, uv_init, r_wc, R_wc, has_patch);
}
int pre3_patch_cut(pre3_ctx *c, int first, int count, const int32_t *uv)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    return patch_cut(c, first, count, uv);
}
int pre3_predict_patches(pre3_ctx *c, double focal_over_d, double *patch_out, int32_t *status_out)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    return patch_predict(c, focal_over_d, patch_out, status_out);
}
int pre3_patch_search(pre3_ctx *c, double focal_over_d, double corr_threshold, int strict_reference, int32_t *m_out, int32_t *meas_idx_out,
                      double *z_out, double *corr_out, int32_t *ncand_out, int32_t *status_out)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    return patch_search(c, focal_over_d, corr_threshold, strict_reference, m_out, meas_idx_out, z_out, corr_out, ncand_out, status_out);
}
int pre3_patch_timing(pre3_ctx *c, double *warp_ms_out, double *search_ms_out)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    return patch_timing(c, warp_ms_out, search_ms_out);
}

// ---- FAST-9 corners on the resident image (fast_corner_detect_9.m, fast_nonmax.m; pre3_fast.hip) ---------------
int pre3_fast_detect(pre3_ctx *c, int r0, int c0, int rows, int cols, int threshold, int barrier, int nonmax, int32_t *K_out, int32_t *uv_out, int32_t *score_out)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    return fast_detect(c, r0, c0, rows, cols, threshold, barrier, nonmax, K_out, uv_out, score_out);
}
int pre3_init_feature_fast(pre3_ctx *c, pre3_sr_frame *frame, double std_pxl, int strict_reference, int threshold, int barrier, const int32_t *centres, int attempts,
                           pre3_fast_init_result *out)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    PRE3_CHECK(centres != nullptr, PRE3_E_ARG, "pre3_init_feature_fast: null centres");
    return fast_init_feature(c, frame, std_pxl, strict_reference, threshold, barrier, centres, attempts, 0, 0, out);
}
int pre3_init_feature_fast_seeded(pre3_ctx *c, pre3_sr_frame *frame, double std_pxl, int strict_reference, int threshold, int barrier, uint64_t seed, uint64_t seq,
                                  pre3_fast_init_result *out)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    return fast_init_feature(c, frame, std_pxl, strict_reference, threshold, barrier, nullptr, PRE3_FAST_MAX_ATTEMPTS, seed, seq, out);
}
int pre3_init_features_fast_all(pre3_ctx *c, pre3_sr_frame *frame, double std_pxl, int threshold, int barrier, int32_t *K_out, int32_t *n_added_out, int32_t *uv_out,
                                double *rho_out, int32_t *verdict_out)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    return fast_init_all(c, frame, std_pxl, threshold, barrier, K_out, n_added_out, uv_out, rho_out, verdict_out);
}
int pre3_fast_timing(pre3_ctx *c, double *detect_ms_out)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    return fast_timing(c, detect_ms_out);
}

// ---- RCCL communicator on the context (pre3_comm.hip) ------------------------------------------------
static int set_comm_impl(pre3_ctx *c, pre3_comm *comm)
{
    PRE3_CHECK(comm == nullptr || comm_device(comm) == c->device, PRE3_E_ARG, "pre3_set_comm: the communicator lives on device %d, the context on %d", comm ? comm_device(comm) : -1, c->device);
    if (c->comm && c->comm != (void *)comm) {
        // nothing queued on the stream may still use the handle being replaced (the caller may destroy it next); after a deadline: its abort has come back
        PRE3_TRY(stream_drain(c, __func__));
        PRE3_CHECK(comm_abort_wait(c->comm, comm_abort_ms(c->comm)), PRE3_E_COMM, "pre3_set_comm: the abort of the previous communicator has not returned yet");
        if (c->comm_owned) (void)pre3_comm_destroy((pre3_comm *)c->comm);
    }
    c->comm = comm; c->comm_owned = false;
    return PRE3_OK;
}
int pre3_set_comm(pre3_ctx *c, pre3_comm *comm)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    return set_comm_impl(c, comm);
}

int pre3_comm_init(pre3_ctx *c, const void *id, int rank, int world)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    pre3_comm *cm = nullptr;
    PRE3_TRY(pre3_comm_create(&cm, c->device, id, rank, world));
    const int rc = set_comm_impl(c, cm);
    if (rc != PRE3_OK) { (void)pre3_comm_destroy(cm); return rc; }
    c->comm_owned = true;
    return PRE3_OK;
}

// ---- test hook (pre3_test_hooks.h; inert without PRE3_TEST_HOOKS=1): a kernel that keeps the stream busy until the host releases it (or ~20 s have passed)
__global__ void k_test_stall(volatile int32_t *flag)
{
    for (long spin = 0; spin < 6000000L; ++spin) {          // (~20 s: the kernel lets go by itself)
        if (__hip_atomic_load(const_cast<int32_t *>(flag), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0) return;
        __builtin_amdgcn_s_sleep(100);
    }
}
int pre3_test_stall(pre3_ctx *c, int release)
{
    PRE3_CHECK(knob::test_hooks(), PRE3_E_STATE, "pre3_test_stall: test hooks are off (PRE3_TEST_HOOKS=1 enables them)");
    PRE3_CHECK(c != nullptr, PRE3_E_ARG, "null context");
    PRE3_HIP(hipSetDevice(c->device));
    if (release) { __atomic_store_n(c->mail_host + 15, 1, __ATOMIC_RELEASE); return PRE3_OK; }
    __atomic_store_n(c->mail_host + 15, 0, __ATOMIC_RELEASE);
    hipLaunchKernelGGL(k_test_stall, dim3(1), dim3(1), 0, c->stream, (volatile int32_t *)(c->mail_dev + 15));
    PRE3_HIP(hipGetLastError());
    return PRE3_OK;
}

int pre3_get_flags(pre3_ctx *c, int32_t *li, int32_t *hi)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    PRE3_TRY(stream_drain(c, __func__));
    if (c->m == 0) return PRE3_OK;
    if (li) PRE3_HIP(hipMemcpy(li, c->li_meas, sizeof(int32_t) * c->m, hipMemcpyDeviceToHost));
    if (hi) PRE3_HIP(hipMemcpy(hi, c->hi_meas, sizeof(int32_t) * c->m, hipMemcpyDeviceToHost));
    return PRE3_OK;
}

int pre3_set_flags(pre3_ctx *c, const int32_t *li, const int32_t *hi)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    PRE3_CHECK(c->measurements_set, PRE3_E_STATE, "pre3_set_flags: no measurements");
    PRE3_TRY(stream_drain(c, __func__));
    int m = c->m, N = c->N;
    for (int pass = 0; pass < 2; ++pass) {
        const int32_t *src = pass == 0 ? li : hi;
        if (!src) continue;
        std::vector<int32_t> lmflag(N ? N : 1, 0), sel;
        for (int j = 0; j < m; ++j) { lmflag[c->meas_host[j]] = src[j] ? 1 : 0; if (src[j]) sel.push_back(j); }
        PRE3_HIP(hipMemcpy(pass == 0 ? c->lm.li : c->lm.hi, lmflag.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice));
        if (m) PRE3_HIP(hipMemcpy(pass == 0 ? c->li_meas : c->hi_meas, src, sizeof(int32_t) * m, hipMemcpyHostToDevice));
        if (!sel.empty()) PRE3_HIP(hipMemcpy(c->sel_rows, sel.data(), sizeof(int32_t) * sel.size(), hipMemcpyHostToDevice));
        int32_t cnt = (int32_t)sel.size();
        PRE3_HIP(hipMemcpy(c->stats + (pass == 0 ? 4 : 5), &cnt, sizeof(int32_t), hipMemcpyHostToDevice));
        if (pass == 0) c->li_from_host = cnt; else c->hi_from_host = cnt;
    }
    return PRE3_OK;
}

// ---- stateless update.m drop-in ---------------------------------------------------------------------
int pre3_update_ell(int device, int dtype, int n, int r, const double *x, const double *P, int width, const int32_t *nnz, const int32_t *col,
                    const double *val, const double *R, const double *z, const double *h, double *x_out, double *P_out, double *K_out)
{
    PRE3_CHECK(n >= 13 && r >= 0 && x && P && x_out && P_out, PRE3_E_ARG, "pre3_update_ell: bad arguments");
    PRE3_CHECK(r == 0 || (nnz && col && val && z && h && width >= 1), PRE3_E_ARG, "pre3_update_ell: null row data");
    if (r == 0) {            // update.m:50-55
        if (x_out != x) memcpy(x_out, x, sizeof(double) * n);
        if (P_out != P) memcpy(P_out, P, sizeof(double) * (size_t)n * n);
        return select_device("pre3_update_ell", device);
    }
    for (int a = 0; a < r; ++a) {
        PRE3_CHECK(nnz[a] >= 0 && nnz[a] <= width && nnz[a] <= ELLW, PRE3_E_ARG, "pre3_update_ell: row %d has %d non-zeros (max %d)", a, nnz[a], ELLW);
        for (int t = 0; t < nnz[a]; ++t) PRE3_CHECK(col[a * width + t] >= 0 && col[a * width + t] < n, PRE3_E_ARG, "pre3_update_ell: column index out of range in row %d", a);
    }
    // a throw-away context sized for this call: capacity in "landmarks" such that 13+6*cap >= n and 2*cap >= r
    int capL = std::max((n - 13 + 5) / 6, (r + 1) / 2);
    if (capL < 1) capL = 1;
    pre3_ctx *c = nullptr;
    PRE3_TRY(pre3_create(&c, device, dtype, capL, 1));
    int rc = PRE3_OK;
    do {
        c->n = n; c->N = 0;
        c->x_valid[PRE3_X_K_KM1] = true;
        if ((rc = pre3_set_state(c, PRE3_X_K_KM1, n, x, P)) != PRE3_OK) break;
        int r_pad = round_up(r, NB);
        std::vector<int32_t> hc((size_t)r_pad * ELLW, 0);
        std::vector<double> hv((size_t)r_pad * ELLW, 0.0), nu(r_pad, 0.0);
        for (int a = 0; a < r; ++a) {
            for (int t = 0; t < nnz[a]; ++t) { hc[(size_t)a * ELLW + t] = col[a * width + t]; hv[(size_t)a * ELLW + t] = val[a * width + t]; }
            nu[a] = z[a] - h[a];
        }
        if (hipMemcpy(c->row_col, hc.data(), sizeof(int32_t) * hc.size(), hipMemcpyHostToDevice) != hipSuccess) { rc = PRE3_E_HIP; set_error("copy failed"); break; }
        if (dtype == PRE3_F64) {
            if (hipMemcpy(c->row_val, hv.data(), sizeof(double) * hv.size(), hipMemcpyHostToDevice) != hipSuccess) { rc = PRE3_E_HIP; break; }
        } else {
            std::vector<float> hf(hv.begin(), hv.end());
            if (hipMemcpy(c->row_val, hf.data(), sizeof(float) * hf.size(), hipMemcpyHostToDevice) != hipSuccess) { rc = PRE3_E_HIP; break; }
        }
        if (hipMemcpy(c->row_nu, nu.data(), sizeof(double) * r_pad, hipMemcpyHostToDevice) != hipSuccess) { rc = PRE3_E_HIP; break; }
        if (R) {
            if ((rc = dmalloc_bytes(c, &c->Rdense, (size_t)r * r * c->esz)) != PRE3_OK) break;
            if (dtype == PRE3_F64) { if (hipMemcpy(c->Rdense, R, sizeof(double) * r * r, hipMemcpyHostToDevice) != hipSuccess) { rc = PRE3_E_HIP; break; } }
            else { std::vector<float> rf(R, R + (size_t)r * r); if (hipMemcpy(c->Rdense, rf.data(), sizeof(float) * rf.size(), hipMemcpyHostToDevice) != hipSuccess) { rc = PRE3_E_HIP; break; } }
        }
        void *Kt = nullptr;
        if (K_out) { if ((rc = dmalloc_bytes(c, &Kt, (size_t)r_pad * c->ldw * c->esz)) != PRE3_OK) break; }
        rc = run_update(c, PRE3_X_K_KM1, r, R != nullptr, Kt);
        if (rc == PRE3_OK) { c->x_valid[PRE3_X_K_K] = true; c->p_which = PRE3_X_K_K; rc = pre3_get_state(c, PRE3_X_K_K, n, x_out, P_out); }
        if (rc == PRE3_OK && K_out) {
            // Kt (r x ldw, T) -> K_out (n x r column-major) : K(i,a) = Kt[a][i]
            if (dtype == PRE3_F64) {
                if (hipMemcpy2D(K_out, sizeof(double) * n, Kt, sizeof(double) * c->ldw, sizeof(double) * n, r, hipMemcpyDeviceToHost) != hipSuccess) rc = PRE3_E_HIP;
            } else {
                std::vector<float> kf((size_t)r * n);
                if (hipMemcpy2D(kf.data(), sizeof(float) * n, Kt, sizeof(float) * c->ldw, sizeof(float) * n, r, hipMemcpyDeviceToHost) != hipSuccess) rc = PRE3_E_HIP;
                else for (size_t i = 0; i < kf.size(); ++i) K_out[i] = kf[i];
            }
        }
    } while (0);
    pre3_destroy(c);
    return rc;
}

// ---- matcher ------------------------------------------------------------------------------------------
// Stateless drop-in for compute_hypothesis_support_fast.m:27 (caller: ransac_hypotheses.m:72).
int pre3_hypothesis_support(int device, int n, const double *xi, const pre3_cam *cam, const double *state_vector_pattern,
                            int n_id, const double *z_id, int n_euc, const double *z_euc, double threshold,
                            int32_t *support_out, int32_t *positions_li_inliers_id, int32_t *positions_li_inliers_euc)
{
    PRE3_CHECK(n >= 13 && xi && cam && state_vector_pattern && support_out, PRE3_E_ARG, "pre3_hypothesis_support: bad arguments");
    PRE3_CHECK(n_id >= 0 && n_euc >= 0 && (n_id == 0 || z_id) && (n_euc == 0 || z_euc), PRE3_E_ARG, "pre3_hypothesis_support: bad measurement arrays");
    PRE3_TRY(select_device("pre3_hypothesis_support", device));
    // xi(logical(state_vector_pattern(:,c))): the selected entries in state order, column c of the n x 4 column-major pattern
    std::vector<int32_t> idx[4];
    for (int c = 0; c < 4; ++c)
        for (int i = 0; i < n; ++i) if (state_vector_pattern[(size_t)c * n + i] != 0.0) idx[c].push_back(i);
    // reshape(ri,3,n_id) etc. (:40-43, :84) fail in MATLAB on a count mismatch; so does this
    PRE3_CHECK((int)idx[0].size() == 3 * n_id && (int)idx[1].size() == 2 * n_id && (int)idx[2].size() == n_id, PRE3_E_ARG,
               "pre3_hypothesis_support: pattern selects %zu/%zu/%zu entries for %d inverse-depth measurements (needs 3/2/1 each)",
               idx[0].size(), idx[1].size(), idx[2].size(), n_id);
    PRE3_CHECK((int)idx[3].size() == 3 * n_euc, PRE3_E_ARG, "pre3_hypothesis_support: pattern selects %zu entries for %d cartesian measurements", idx[3].size(), n_euc);
    if (n_id + n_euc == 0) { *support_out = 0; return PRE3_OK; }                       // :29, both branches empty
    std::vector<int32_t> out(1 + (size_t)n_id + n_euc);
    PRE3_TRY(run_hypothesis_support(n, xi, *cam, n_id, idx[0].data(), idx[1].data(), idx[2].data(), z_id, n_euc, idx[3].data(), z_euc, threshold, out.data()));
    *support_out = out[0];
    if (positions_li_inliers_id) for (int j = 0; j < n_id; ++j) positions_li_inliers_id[j] = out[1 + j];
    if (positions_li_inliers_euc) for (int j = 0; j < n_euc; ++j) positions_li_inliers_euc[j] = out[1 + n_id + j];
    return PRE3_OK;
}

// Stateless drop-in for `[X_km1_k, P_km1_k] = predict_state_and_covariance(X_k, P_k, type, SD_A, SD_alpha)`
// (predict_state_and_covariance.m:27, caller @ekf_filter/ekf_prediction.m:29) with the odometry increment made explicit.
struct DenseCtx { pre3_ctx *c = nullptr; int device = 0, dtype = 0, capL = 0; };
static DenseCtx g_dense[4];
static std::mutex g_dense_mu;

int pre3_predict_dense(int device, int dtype, int n, const double *x, const double *P, const double u[7], double *x_out, double *P_out)
{
    PRE3_CHECK(n >= 13 && (n - 13) % 3 == 0 && x && P && u && x_out && P_out, PRE3_E_ARG, "pre3_predict_dense: bad arguments (n = 13 + 6 N_id + 3 N_euc)");
    int capL = std::max((n - 13 + 5) / 6, 1);
    // ekf_prediction.m reaches this entry every frame: the context (P at capacity, the update's work buffers, pinned inbox / mailbox -- more
    // than a GB allocated and cleared at n = 12013) is kept between calls, one per (device, dtype), grown when a larger state arrives and
    // released by pre3_release_scratch().  Calls are serialised on it.
    std::lock_guard<std::mutex> lk(g_dense_mu);
    DenseCtx *slot = nullptr;
    for (DenseCtx &d : g_dense) if (d.c && d.device == device && d.dtype == dtype) slot = &d;
    if (slot && slot->capL < capL) { pre3_destroy(slot->c); slot->c = nullptr; slot = nullptr; }
    if (!slot) {
        for (DenseCtx &d : g_dense) if (!d.c) { slot = &d; break; }
        if (!slot) { slot = &g_dense[0]; pre3_destroy(slot->c); slot->c = nullptr; }
        const int cap = capL + capL / 8;                                     // a little headroom: the map grows by a few landmarks per frame
        PRE3_TRY(pre3_create(&slot->c, device, dtype, cap, 1));
        slot->device = device; slot->dtype = dtype; slot->capL = cap;
        // (this context never factorises: it must not count against the two persistent-factorisation contexts a device serves, pre3_cholp.hip)
        slot->c->chol_persist = false;
        if (slot->c->cholp_counted) { cholp_context_count(device, -1); slot->c->cholp_counted = false; }
    }
    pre3_ctx *c = slot->c;
    int rc = PRE3_OK;
    do {
        c->n = n; c->N = 0;                       // the prediction touches the 13 camera entries and rows/columns 1:13 only: no landmark table needed
        if ((rc = pre3_set_state(c, PRE3_X_K_K, n, x, P)) != PRE3_OK) break;
        if ((rc = pre3_predict(c, u)) != PRE3_OK) break;
        rc = pre3_get_state(c, PRE3_X_K_KM1, n, x_out, P_out);
    } while (0);
    if (rc != PRE3_OK) { pre3_destroy(slot->c); slot->c = nullptr; }         // never reuse a context that failed half-way
    return rc;
}

int pre3_release_scratch(void)
{
    release_scratch();
    std::lock_guard<std::mutex> lk(g_dense_mu);
    for (DenseCtx &d : g_dense) if (d.c) { pre3_destroy(d.c); d.c = nullptr; }
    return PRE3_OK;
}

int pre3_siftmatch_merge(int cls, int G, int K1, const double *best, const double *second, const int32_t *arg, double thresh_d,
                         double *pairs_out, double *score_out, int *M_out)
{
    PRE3_CHECK(G >= 1 && K1 >= 0 && M_out, PRE3_E_ARG, "pre3_siftmatch_merge: bad arguments");
    PRE3_CHECK(K1 == 0 || (best && second && arg && pairs_out), PRE3_E_ARG, "pre3_siftmatch_merge: null pointer");
    const float thresh = (float)thresh_d;      // the gateway passes its double into a float parameter (siftmatch.c:208-216)
    int M = 0;
    for (int k1 = 0; k1 < K1; ++k1) {
        double B = 0, S2 = 0; int K = -1;
        for (int g = 0; g < G; ++g) {
            double ob = best[(size_t)g * K1 + k1], os = second[(size_t)g * K1 + k1]; int ok = arg[(size_t)g * K1 + k1];
            if (ok < 0) continue;
            if (K < 0) { B = ob; S2 = os; K = ok; continue; }
            if (ob < B || (ob == B && ok < K)) { S2 = os < B ? os : B; B = ob; K = ok; }
            else { S2 = ob < S2 ? ob : S2; }
        }
        if (K < 0) continue;
        // Lowe's ratio test in float (siftmatch.c:122); integer classes convert int -> float
        float fb, fs;
        if (cls == 1) { fb = (float)B; fs = (float)S2; }
        else if (cls >= 2) { fb = (float)(int)B; fs = (float)(int)S2; }
        else { fb = (float)B; fs = (float)S2; }
        if (thresh * fb <= fs) {
            pairs_out[2 * M] = k1 + 1; pairs_out[2 * M + 1] = K + 1;
            if (score_out) score_out[M] = B;
            ++M;
        }
    }
    *M_out = M;
    return PRE3_OK;
}

int pre3_siftmatch_partial(int device, int cls, int ND, int K1, const void *L1, int K2_local, const void *L2_local, int k2_offset,
                           double *best, double *second, int32_t *arg)
{
    return match_partial(device, cls, ND, K1, L1, K2_local, L2_local, k2_offset, best, second, arg);
}

static int siftmatch_any(int device, int cls, int ND, int K1, const void *L1, int K2, const void *L2, double thresh, double *pairs_out,
                         double *score_out, int *M_out)
{
    PRE3_CHECK(M_out != nullptr, PRE3_E_ARG, "siftmatch: null M_out");
    *M_out = 0;
    PRE3_CHECK(ND > 0 && K1 >= 0 && K2 >= 0, PRE3_E_ARG, "siftmatch: bad sizes");
    PRE3_TRY(select_device("siftmatch", device));
    if (K1 == 0) return PRE3_OK;
    std::vector<double> b(K1), s(K1); std::vector<int32_t> a(K1);
    PRE3_TRY(match_partial(device, cls, ND, K1, L1, K2, L2, 0, b.data(), s.data(), a.data()));
    return pre3_siftmatch_merge(cls, 1, K1, b.data(), s.data(), a.data(), thresh, pairs_out, score_out, M_out);
}

int pre3_siftmatch_f64(int device, int ND, int K1, const double *L1, int K2, const double *L2, double thresh, double *pairs_out, double *score_out, int *M_out)
{ return siftmatch_any(device, 0, ND, K1, L1, K2, L2, thresh, pairs_out, score_out, M_out); }
int pre3_siftmatch_f32(int device, int ND, int K1, const float *L1, int K2, const float *L2, double thresh, double *pairs_out, double *score_out, int *M_out)
{ return siftmatch_any(device, 1, ND, K1, L1, K2, L2, thresh, pairs_out, score_out, M_out); }
int pre3_siftmatch_u8(int device, int ND, int K1, const uint8_t *L1, int K2, const uint8_t *L2, double thresh, double *pairs_out, double *score_out, int *M_out)
{ return siftmatch_any(device, 2, ND, K1, L1, K2, L2, thresh, pairs_out, score_out, M_out); }
int pre3_siftmatch_i8(int device, int ND, int K1, const int8_t *L1, int K2, const int8_t *L2, double thresh, double *pairs_out, double *score_out, int *M_out)
{ return siftmatch_any(device, 3, ND, K1, L1, K2, L2, thresh, pairs_out, score_out, M_out); }

int pre3_knn_f64(int device, int D, int N, const double *data, int M, const double *query, int k, double *ids_out, double *dist_out)
{
    PRE3_CHECK(data && (M == 0 || (query && ids_out && dist_out)), PRE3_E_ARG, "pre3_knn_f64: null pointer");
    return knn_run(device, D, N, data, M, query, k, ids_out, dist_out);
}

// ---- measurement hooks ---------------------------------------------------------------------------------
int pre3_timer_start(pre3_ctx *c)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    PRE3_HIP(hipEventRecord(c->t0, c->stream));
    return PRE3_OK;
}

int pre3_timer_stop(pre3_ctx *c, double *ms_out)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    PRE3_HIP(hipEventRecord(c->t1, c->stream));
    PRE3_HIP(hipEventSynchronize(c->t1));
    float ms = 0;
    PRE3_HIP(hipEventElapsedTime(&ms, c->t0, c->t1));
    if (ms_out) *ms_out = ms;
    return PRE3_OK;
}

int pre3_kernel_timing(pre3_ctx *c, int enable)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    c->kt.enabled = enable != 0; c->kt.every = enable > 1 ? enable : 1; c->kt.seen = 0; c->kt.used = 0; c->kt.flops = 0; c->kt.bytes = 0;
    c->kt.fused = 0; c->kt.fact_flops = 0; c->kt.pending = false;
    return PRE3_OK;
}

int pre3_kernel_timing_read(pre3_ctx *c, int *launches_out, double *total_ms_out, double *flops_out, double *bytes_out)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    PRE3_TRY(stream_drain(c, __func__));
    double tot = 0;
    for (int i = 0; i + 1 < c->kt.used; i += 2) { float ms = 0; PRE3_HIP(hipEventElapsedTime(&ms, c->kt.ev[i], c->kt.ev[i + 1])); tot += ms; }
    if (launches_out) *launches_out = c->kt.used / 2;
    if (total_ms_out) *total_ms_out = tot;
    if (flops_out) *flops_out = c->kt.flops;
    if (bytes_out) *bytes_out = c->kt.bytes;
    c->kt.used = 0; c->kt.flops = 0; c->kt.bytes = 0;
    return PRE3_OK;
}

int pre3_kernel_timing_info(pre3_ctx *c, int *fused_launches_out, double *fact_flops_out)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    if (fused_launches_out) *fused_launches_out = c->kt.fused;
    if (fact_flops_out) *fact_flops_out = c->kt.fact_flops;
    c->kt.fused = 0; c->kt.fact_flops = 0;
    return PRE3_OK;
}

int pre3_bench_downdate(pre3_ctx *c, int r, int reps, double *ms_per_launch_out)
{
    EntryScope scope(c); PRE3_TRY(scope.rc);
    PRE3_CHECK(r >= 1 && round_up(r, NB) <= c->rcap && reps >= 1, PRE3_E_ARG, "pre3_bench_downdate: bad r/reps");
    PRE3_CHECK(c->n > 0, PRE3_E_STATE, "pre3_bench_downdate: no map/state set");
    int r_pad = round_up(r, NB);
    PRE3_TRY(launch_fill_w(c, r_pad));
    bool was = c->kt.enabled; c->kt.enabled = false;
    PRE3_TRY(launch_downdate(c, r, c->W));                         // (splits W into its bf16 planes on the way)
    PRE3_HIP(hipEventRecord(c->t0, c->stream));
    for (int i = 0; i < reps; ++i) PRE3_TRY(launch_downdate(c, r, c->W, -1, r_pad));      // the planes are there: time the down-date alone, as it runs behind a factorisation
    PRE3_HIP(hipEventRecord(c->t1, c->stream));
    PRE3_HIP(hipEventSynchronize(c->t1));
    float ms = 0; PRE3_HIP(hipEventElapsedTime(&ms, c->t0, c->t1));
    if (ms_per_launch_out) *ms_per_launch_out = ms / reps;
    c->kt.enabled = was;
    return PRE3_OK;
}

// ---- test hook (pre3_test_hooks.h; inert without PRE3_TEST_HOOKS=1): what the seam of pre3_own.h has allocated and not freed
int pre3_test_live_blocks(int64_t out[4])
{
    PRE3_CHECK(knob::test_hooks(), PRE3_E_STATE, "pre3_test_live_blocks: test hooks are off (PRE3_TEST_HOOKS=1 enables them)");
    PRE3_CHECK(out != nullptr, PRE3_E_ARG, "pre3_test_live_blocks: null pointer");
    for (int k = 0; k < 4; ++k) out[k] = g_live[k].load(std::memory_order_relaxed);
    return PRE3_OK;
}

// ---- test hook (pre3_test_hooks.h; inert without PRE3_TEST_HOOKS=1): P <- P - launches * W'W for the caller's W (r x n, row-major, host), through
// launch_downdate alone -- no rows, no factorisation, no x-update rider.  The second and later launches find the bf16 planes split, as in pre3_bench_downdate.
int pre3_test_downdate(pre3_ctx *c, int r, const double *W, int launches)
{
    PRE3_CHECK(knob::test_hooks(), PRE3_E_STATE, "pre3_test_downdate: test hooks are off (PRE3_TEST_HOOKS=1 enables them)");
    PRE3_CHECK(c != nullptr && W != nullptr, PRE3_E_ARG, "pre3_test_downdate: null pointer");
    PRE3_CHECK(r >= 1 && round_up(r, NB) <= c->rcap && launches >= 1, PRE3_E_ARG, "pre3_test_downdate: bad r/launches");
    PRE3_CHECK(c->n > 0, PRE3_E_STATE, "pre3_test_downdate: no map/state set");
    for (size_t i = 0; i < (size_t)r * c->n; ++i) PRE3_CHECK(c->dtype == PRE3_F64 ? std::isfinite(W[i]) : std::isfinite((float)W[i]), PRE3_E_ARG, "pre3_test_downdate: W has a non-finite entry");
    EntryScope scope(c); PRE3_TRY(scope.rc);
    const int r_pad = round_up(r, NB), n = c->n, ldw = c->ldw;
    // rows 0 .. r-1 in the context's dtype at row stride ldw; columns n .. ldw-1 and rows r .. r_pad-1 are the zeros launch_downdate relies on
    std::vector<unsigned char> img((size_t)r_pad * ldw * c->esz, 0);
    for (int i = 0; i < r; ++i)
        for (int j = 0; j < n; ++j) {
            if (c->dtype == PRE3_F64) reinterpret_cast<double *>(img.data())[(size_t)i * ldw + j] = W[(size_t)i * n + j];
            else reinterpret_cast<float *>(img.data())[(size_t)i * ldw + j] = (float)W[(size_t)i * n + j];
        }
    PRE3_TRY(stream_drain(c, __func__));
    PRE3_HIP(hipMemcpy(c->W, img.data(), img.size(), hipMemcpyHostToDevice));
    c->hp_all_valid = false; c->g_valid = false;                   // (H*P of the measured rows belongs to the P before this call)
    bool was = c->kt.enabled; c->kt.enabled = false;
    int rc = launch_downdate(c, r, c->W);
    for (int i = 1; i < launches && rc == PRE3_OK; ++i) rc = launch_downdate(c, r, c->W, -1, r_pad);
    c->kt.enabled = was;
    PRE3_TRY(rc);
    return stream_drain(c, __func__);
}

// ---- test hook (pre3_test_hooks.h; inert without PRE3_TEST_HOOKS=1): S = L L', L W = [B | nu] for the caller's S (r x r), B (r x n) and nu (r), through
// launch_chol_solve alone (mode 0: P is not touched) or followed by launch_downdate on the planes the factorisation wrote, as in run_update (mode 1).
// L_out (r x r, the lower triangle; zeros above) and W_out (round_up(r, 64) x (n + 1), the nu column last) may each be null.
int pre3_test_factor_solve(pre3_ctx *c, int r, const double *S, const double *B, const double *nu, int mode, int predicted_prior, double *L_out, double *W_out)
{
    PRE3_CHECK(knob::test_hooks(), PRE3_E_STATE, "pre3_test_factor_solve: test hooks are off (PRE3_TEST_HOOKS=1 enables them)");
    PRE3_CHECK(c != nullptr && S != nullptr && B != nullptr && nu != nullptr, PRE3_E_ARG, "pre3_test_factor_solve: null pointer");
    PRE3_CHECK(r >= 1 && round_up(r, NB) <= c->rcap && (mode == 0 || mode == 1), PRE3_E_ARG, "pre3_test_factor_solve: bad r/mode");
    PRE3_CHECK(c->n > 0, PRE3_E_STATE, "pre3_test_factor_solve: no map/state set");
    const bool f64 = c->dtype == PRE3_F64;
    auto finite = [&](const double *a, size_t cnt) { for (size_t i = 0; i < cnt; ++i) if (!(f64 ? std::isfinite(a[i]) : std::isfinite((float)a[i]))) return false; return true; };
    PRE3_CHECK(finite(S, (size_t)r * r) && finite(B, (size_t)r * c->n) && finite(nu, (size_t)r), PRE3_E_ARG, "pre3_test_factor_solve: S, B or nu has a non-finite entry");
    EntryScope scope(c); PRE3_TRY(scope.rc);
    const int r_pad = round_up(r, NB), n = c->n, ldw = c->ldw;
    // S at stride r_pad, both triangles, with k_ell_G's padding (identity on the padded diagonal); [B | nu] at stride ldw, nu in column ld, zeros elsewhere
    std::vector<unsigned char> simg((size_t)r_pad * r_pad * c->esz, 0), wimg((size_t)r_pad * ldw * c->esz, 0);
    auto put = [&](std::vector<unsigned char> &img, size_t at, double v) { if (f64) reinterpret_cast<double *>(img.data())[at] = v; else reinterpret_cast<float *>(img.data())[at] = (float)v; };
    auto get = [&](const std::vector<unsigned char> &img, size_t at) { return f64 ? reinterpret_cast<const double *>(img.data())[at] : (double)reinterpret_cast<const float *>(img.data())[at]; };
    for (int i = 0; i < r_pad; ++i) {
        if (i >= r) { put(simg, (size_t)i * r_pad + i, 1.0); continue; }
        for (int j = 0; j < r; ++j) put(simg, (size_t)i * r_pad + j, S[(size_t)i * r + j]);
        for (int j = 0; j < n; ++j) put(wimg, (size_t)i * ldw + j, B[(size_t)i * n + j]);
        put(wimg, (size_t)i * ldw + c->ld, nu[i]);
    }
    PRE3_TRY(stream_drain(c, __func__));
    PRE3_HIP(hipMemcpy(c->Smat, simg.data(), simg.size(), hipMemcpyHostToDevice));
    PRE3_HIP(hipMemcpy(c->W, wimg.data(), wimg.size(), hipMemcpyHostToDevice));
    c->hp_all_valid = false; c->g_valid = false;                   // (H*P and H*P*H' of the measured rows are not what W and Smat hold now)
    const bool kt_was = c->kt.enabled, ov_was = c->k9_overlap;
    c->kt.enabled = false;
    if (mode == 0) c->k9_overlap = false;                          // no down-date consumers in the persistent launch: P stays as it is
    int rc = chol_solve_for_test(c, r_pad, predicted_prior != 0, r);
    c->k9_overlap = ov_was;
    if (rc == PRE3_OK && mode == 1) rc = launch_downdate(c, r, c->W, -1);
    c->kt.enabled = kt_was;
    PRE3_TRY(rc);
    PRE3_TRY(fetch_stats(c));                                      // drains; PRE3_E_NUMERIC if a pivot was not positive
    if (L_out != nullptr) {
        PRE3_HIP(hipMemcpy(simg.data(), c->Smat, simg.size(), hipMemcpyDeviceToHost));
        for (int i = 0; i < r; ++i)
            for (int j = 0; j < r; ++j) L_out[(size_t)i * r + j] = j <= i ? get(simg, (size_t)i * r_pad + j) : 0.0;
    }
    if (W_out != nullptr) {
        PRE3_HIP(hipMemcpy(wimg.data(), c->W, wimg.size(), hipMemcpyDeviceToHost));
        for (int i = 0; i < r_pad; ++i) {
            for (int j = 0; j < n; ++j) W_out[(size_t)i * (n + 1) + j] = get(wimg, (size_t)i * ldw + j);
            W_out[(size_t)i * (n + 1) + n] = get(wimg, (size_t)i * ldw + c->ld);
        }
    }
    return PRE3_OK;
}

// ---- device-resident database shard of the sharded matcher (uint8 class; DESIGN.md "multi-GPU", C2)
int pre3_match_shard_create_cls(pre3_match_shard **out, int device, int cls, int ND, int K1, const void *L1, int K2_local, const void *L2_local, int k2_offset)
{
    PRE3_CHECK(out != nullptr, PRE3_E_ARG, "pre3_match_shard_create: null output");
    PRE3_TRY(select_device("pre3_match_shard_create", device));
    void *h = match_shard_create(device, cls, ND, K1, L1, K2_local, L2_local, k2_offset);
    if (!h) return PRE3_E_ARG;
    *out = (pre3_match_shard *)h;
    return PRE3_OK;
}
int pre3_match_shard_create(pre3_match_shard **out, int device, int ND, int K1, const uint8_t *L1, int K2_local, const uint8_t *L2_local, int k2_offset)
{
    return pre3_match_shard_create_cls(out, device, 2, ND, K1, L1, K2_local, L2_local, k2_offset);
}
int pre3_match_shard_run(pre3_match_shard *s, void **partial_dev, int *n_doubles) { return s ? match_shard_run(s, partial_dev, n_doubles) : PRE3_E_ARG; }
int pre3_match_shard_merge(pre3_match_shard *s, int G, const void *gathered_dev, double thresh, double *pairs_out, double *score_out, int *M_out)
{
    return s ? match_shard_merge(s, G, gathered_dev, thresh, pairs_out, score_out, M_out) : PRE3_E_ARG;
}
int pre3_match_shard_set_comm(pre3_match_shard *s, pre3_comm *comm) { return s ? match_shard_set_comm(s, comm) : PRE3_E_ARG; }
int pre3_match_shard_match(pre3_match_shard *s, double thresh, double *pairs_out, double *score_out, int *M_out)
{
    return s ? match_shard_match(s, thresh, pairs_out, score_out, M_out) : PRE3_E_ARG;
}
int pre3_match_shard_destroy(pre3_match_shard *s) { if (s) match_shard_destroy(s); return PRE3_OK; }
int pre3_match_shard_test_stall(pre3_match_shard *s, int release)
{
    PRE3_CHECK(knob::test_hooks(), PRE3_E_STATE, "pre3_match_shard_test_stall: test hooks are off (PRE3_TEST_HOOKS=1 enables them)");
    return s ? match_shard_test_stall(s, release) : PRE3_E_ARG;
}

// matcher roofline/bench probe (inputs resident in HBM); not part of the reference-shaped API
PRE3_API void *pre3_match_bench_create(int device, int ND, int K1, const uint8_t *L1, int K2, const uint8_t *L2)
{
    if (select_device("pre3_match_bench_create", device) != PRE3_OK) return nullptr;
    return match_bench_create(2, ND, K1, L1, K2, L2);
}
// the same probe for any class (0 double, 1 float, 2 uint8); pre3_match_bench_info: [route (0 exact kernels, 1 int8 MFMA, 2 bf16 rank +
// exact re-evaluation), queries scanned in full, candidates re-evaluated] of the last run
PRE3_API void *pre3_match_bench_create_cls(int device, int cls, int ND, int K1, const void *L1, int K2, const void *L2)
{
    if (select_device("pre3_match_bench_create_cls", device) != PRE3_OK) return nullptr;
    return match_bench_create(cls, ND, K1, L1, K2, L2);
}
PRE3_API int pre3_match_bench_info(void *h, int32_t info[3]) { return h ? match_bench_info(h, info) : PRE3_E_ARG; }
PRE3_API int pre3_match_bench_run(void *h, int reps, double *ms_per) { return h ? match_bench_run(h, reps, ms_per) : PRE3_E_ARG; }
PRE3_API int pre3_match_bench_fetch(void *h, double *best, double *second, int32_t *arg) { return h ? match_bench_fetch(h, best, second, arg) : PRE3_E_ARG; }
PRE3_API void pre3_match_bench_destroy(void *h) { if (h) match_bench_destroy(h); }

}  // extern "C"
