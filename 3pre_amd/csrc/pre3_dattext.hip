// pre3_dattext.hip -- SR4000 .dat text parsed on the device (pre3_sr_text_parse, pre3_sr_frame_load_text).
//   read_xyz_sr4000.m:2-3        load(sprintf('%s/d1_%04d.dat', ...)): the text of one frame
//   read_xyz_sr4000.m:25-42      4 x 144, 5 x 144 or 5 x 144 + 1 rows: without a confidence map, with one, with the timestamp row
// Three launches on one stream; the rules are pre3_dattext.h's:
//   k_dat_count     a workgroup per 4096-byte chunk, a 16-byte load per lane: each lane's summary (token starts, first-of-line starts, what the
//                   stretch in front has to decide), folded in byte order through LDS into one record per chunk.
//   k_dat_offsets   every workgroup derives its own position from the records of the chunks in front of it (sums, and for a chunk whose leading
//                   token waits for a decision a look back to the nearest record that has a \n or a token), scans its lanes' summaries in LDS,
//                   and each lane walks its 16 bytes again: tok_off[t] = byte offset | DAT_FIRST.  Totals and the first line's length go to the
//                   status block.
//   k_dat_parse     a lane per token: the rectangularity rule on (t, DAT_FIRST), the conversion, the store, the flags.
// No workgroup waits on another; the only atomics are integer ones into the status block (or, min, add), so results are bit-equal from run to run.
#include <algorithm>
#include <mutex>
#include <utility>

#include "pre3_internal.h"
#include "pre3_dattext.h"
#include "pre3_srframe.h"

namespace pre3 {

namespace {

constexpr int DL = DAT_CHUNK / 16;          // lanes per workgroup of the two byte passes
constexpr int PB = 256;                     // tokens per workgroup of k_dat_parse
static_assert(DL == 256, "a chunk is 256 lanes of 16 bytes");

// the lane's 16 bytes (zero beyond the text) and the byte in front of them
__device__ inline void lane_bytes(const char *__restrict__ text, size_t nbytes, size_t base, unsigned char b[16], unsigned char *prev)
{
    if (base + 16 <= nbytes) {
        const uint4 v = *reinterpret_cast<const uint4 *>(text + base);      // text and base are 16-byte aligned
        const uint32_t w[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
        for (int i = 0; i < 16; ++i) b[i] = (unsigned char)(w[i >> 2] >> (8 * (i & 3)));
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) b[i] = base + i < nbytes ? (unsigned char)text[base + i] : 0;
    }
    *prev = base > 0 && base <= nbytes ? (unsigned char)text[base - 1] : 0;
}

__device__ inline DatSum lane_sum(const unsigned char b[16], unsigned char prev, size_t base, size_t nbytes)
{
    DatSum s = dat_sum_zero();
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        if (base + i >= nbytes) break;
        dat_sum_byte(s, dat_is_start(i ? b[i - 1] : prev, base + i > 0, b[i]), dat_is_nl(b[i]));
    }
    return s;
}

__global__ __launch_bounds__(DL) void k_dat_count(const char *__restrict__ text, size_t nbytes, DatSum *__restrict__ recs, DatStatus *__restrict__ st)
{
    __shared__ DatSum s_s[DL];
    const int tid = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * DAT_CHUNK + 16 * (size_t)tid;
    unsigned char b[16], prev;
    lane_bytes(text, nbytes, base, b, &prev);
    s_s[tid] = lane_sum(b, prev, base, nbytes);
    __syncthreads();
    for (int d = 1; d < DL; d *= 2) {                        // a tree whose order is the byte order
        if (tid % (2 * d) == 0) s_s[tid] = dat_sum_fold(s_s[tid], s_s[tid + d]);
        __syncthreads();
    }
    if (tid == 0) {
        recs[blockIdx.x] = s_s[0];
        if (blockIdx.x == 0) {
            st->bad_key = ~0ull; st->ragged_key = ~0ull; st->timestamp = -1.0;
            st->n_tokens = 0; st->n_lines = 0; st->cols = 0; st->flags = 0; st->n_undecided = 0; st->pad_ = 0;
        }
    }
}

// whether the line that runs into chunk j already has a token: the nearest record in front that has a \n or a token decides
__device__ inline bool tail_into(const DatSum *__restrict__ recs, int j)
{
    for (int k = j - 1; k >= 0; --k) {
        if (recs[k].nl) return recs[k].tail != 0;
        if (recs[k].ntok > 0) return true;
    }
    return false;
}

__global__ __launch_bounds__(DL) void k_dat_offsets(const char *__restrict__ text, size_t nbytes, const DatSum *__restrict__ recs, uint32_t *__restrict__ tok_off,
                                                    long long cap, DatStatus *__restrict__ st)
{
    __shared__ DatSum s_s[DL];
    __shared__ int s_tok, s_line, s_tail;
    const int tid = threadIdx.x, chunk = blockIdx.x;
    if (tid == 0) { s_tok = 0; s_line = 0; s_tail = tail_into(recs, chunk) ? 1 : 0; }
    __syncthreads();
    int ntok = 0, nline = 0;
    for (int j = tid; j < chunk; j += DL) {
        const DatSum r = recs[j];
        ntok += r.ntok;
        nline += r.nfirst + ((r.lead && !tail_into(recs, j)) ? 1 : 0);
    }
    if (ntok) atomicAdd(&s_tok, ntok);                      // integer sums: the order does not show
    if (nline) atomicAdd(&s_line, nline);
    const size_t base = (size_t)chunk * DAT_CHUNK + 16 * (size_t)tid;
    unsigned char b[16], prev;
    lane_bytes(text, nbytes, base, b, &prev);
    DatSum mine = lane_sum(b, prev, base, nbytes);
    s_s[tid] = mine;
    __syncthreads();
    for (int d = 1; d < DL; d *= 2) {                        // inclusive scan, in byte order
        DatSum v = mine;
        if (tid >= d) v = dat_sum_fold(s_s[tid - d], mine);
        __syncthreads();
        s_s[tid] = mine = v;
        __syncthreads();
    }
    DatPos p;
    p.tok = s_tok; p.line = s_line; p.tail = (uint32_t)s_tail;
    if (tid > 0) p = dat_pos_advance(p, s_s[tid - 1]);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        if (base + i >= nbytes) break;
        if (dat_is_nl(b[i])) p.tail = 0;
        if (dat_is_start(i ? b[i - 1] : prev, base + i > 0, b[i])) {
            const bool first = !p.tail;
            if (p.tok < cap) tok_off[p.tok] = (uint32_t)(base + i) | (first ? DAT_FIRST : 0u);
            if (first && p.line == 1) st->cols = (int32_t)p.tok;      // one lane of the grid
            p.line += first ? 1 : 0; p.tail = 1; ++p.tok;
        }
    }
    if (chunk == (int)gridDim.x - 1 && tid == DL - 1) { st->n_tokens = (int32_t)p.tok; st->n_lines = (int32_t)p.line; }
}

__global__ __launch_bounds__(PB) void k_dat_parse(const char *__restrict__ text, size_t nbytes, const uint32_t *__restrict__ tok_off, long long cap,
                                                  const uint64_t *__restrict__ table, double *__restrict__ out, int plane_rows, int frame_cols,
                                                  DatStatus *st)
{
    const long long t = (long long)blockIdx.x * PB + threadIdx.x;
    const int n = st->n_tokens, lines = st->n_lines;
    if (n > cap || t >= n) return;
    const int cols = dat_cols(n, lines, st->cols);
    const uint32_t word = tok_off[t], off = word & ~DAT_FIRST;
    const unsigned long long key = ((unsigned long long)t << 32) | off;
    if (((word & DAT_FIRST) != 0) != (t % cols == 0)) atomicMin(&st->ragged_key, key);
    double v = 0.0;
    const int rc = dat_convert(text + off, nbytes - off, table, &v, nullptr);
    if (rc == DAT_BAD) { atomicOr(&st->flags, (int)DAT_F_BAD); atomicMin(&st->bad_key, key); return; }
    if (rc == DAT_UNDECIDED) { atomicAdd(&st->n_undecided, 1); return; }
    if ((long long)lines * cols != n) return;
    if (plane_rows > 0 && !dat_frame_shape(lines, cols, plane_rows, frame_cols)) return;
    const long long R = t / cols, j = t % cols, idx = dat_store_index(R, j, lines, cols, plane_rows);      // idx < n <= cap
    if (idx < 0) { if (j == 0) st->timestamp = v; return; }
    out[idx] = v;
    if (plane_rows > 0 && R / plane_rows == 3 && !(v >= 0.0 && v <= 1.7976931348623157e308)) atomicOr(&st->flags, (int)DAT_F_AMP);
}

// the power-of-five table: computed once on the host, uploaded once per device
std::mutex g_table_mu;
std::vector<uint64_t> g_table_host;
DevBlock g_table_dev[64];

int table_on_device(int device, const uint64_t **out)
{
    std::lock_guard<std::mutex> lk(g_table_mu);
    PRE3_CHECK(device >= 0 && device < 64, PRE3_E_ARG, "the .dat text parse keeps a table for devices 0 .. 63, not %d", device);
    DevBlock &t = g_table_dev[device];
    if (t.p == nullptr) {
        if (g_table_host.empty()) { g_table_host.resize(2 * (size_t)DAT_TABLE_ROWS); dat_build_table(g_table_host.data()); }
        const size_t bytes = sizeof(uint64_t) * g_table_host.size();
        PRE3_TRY(t.reserve(bytes, bytes, Zero::none()));
        if (hipMemcpy(t.p, g_table_host.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) { t.release(); set_error("the .dat text parse: table upload failed"); return PRE3_E_HIP; }
    }
    *out = t.as<uint64_t>();
    return PRE3_OK;
}

// the work block behind the text: [text | records | tok_off | status]
struct DatLayout { size_t o_recs, o_off, o_status, total; int nchunks; };

DatLayout dat_layout(size_t nbytes, size_t cap_tokens)
{
    DatLayout l;
    l.nchunks = (int)((nbytes + DAT_CHUNK - 1) / DAT_CHUNK);
    l.o_recs = up16(nbytes + 16);
    l.o_off = l.o_recs + up16(sizeof(DatSum) * (size_t)l.nchunks);
    l.o_status = l.o_off + up16(sizeof(uint32_t) * (cap_tokens + 1));
    l.total = l.o_status + up16(sizeof(DatStatus));
    return l;
}

// the three launches over the text at the front of `work`; status goes to status_host (pinned or not) behind them.  Nothing waits.
int dat_launch(char *work, const DatLayout &l, size_t nbytes, long long cap_tokens, const uint64_t *table, double *out, int plane_rows, int frame_cols,
               DatStatus *status_host, hipStream_t st)
{
    DatSum *recs = (DatSum *)(work + l.o_recs);
    uint32_t *tok_off = (uint32_t *)(work + l.o_off);
    DatStatus *status = (DatStatus *)(work + l.o_status);
    hipLaunchKernelGGL(k_dat_count, dim3(l.nchunks), dim3(DL), 0, st, (const char *)work, nbytes, recs, status);
    PRE3_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_dat_offsets, dim3(l.nchunks), dim3(DL), 0, st, (const char *)work, nbytes, (const DatSum *)recs, tok_off, cap_tokens, status);
    PRE3_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_dat_parse, dim3((unsigned)((cap_tokens + PB - 1) / PB)), dim3(PB), 0, st, (const char *)work, nbytes, (const uint32_t *)tok_off, cap_tokens,
                       table, out, plane_rows, frame_cols, status);
    PRE3_HIP(hipGetLastError());
    PRE3_HIP(hipMemcpyAsync(status_host, status, sizeof(DatStatus), hipMemcpyDeviceToHost, st));
    return PRE3_OK;
}

void info_out(const DatInfo &d, pre3_sr_text_info *o)
{
    o->status = d.status; o->rows = d.rows; o->cols = d.cols; o->has_conf = d.has_conf; o->has_timestamp = d.has_timestamp; o->n_tokens = d.n_tokens;
    o->n_undecided = d.n_undecided; o->bad_row = d.bad_row; o->bad_col = d.bad_col; o->bad_offset = d.bad_offset; o->timestamp = d.timestamp;
}

void info_empty(pre3_sr_text_info *o)
{
    DatStatus s;
    memset(&s, 0, sizeof s);
    s.bad_key = s.ragged_key = ~0ull;
    DatInfo d;
    dat_finish(s, 0, 0, 0, 0, &d);
    info_out(d, o);
}

const char *const STATUS_TEXT[7] = { "ok", "bad token", "ragged rows", "wrong shape for this handle", "undecided token", "negative or non-finite amplitude",
                                     "empty text" };

int refuse(const char *who, const pre3_sr_text_info &o)
{
    if (o.status == DAT_ST_BAD || o.status == DAT_ST_RAGGED)
        set_error("%s: %s at row %d, column %d (byte %lld)", who, STATUS_TEXT[o.status], o.bad_row + 1, o.bad_col + 1, (long long)o.bad_offset);
    else if (o.status == DAT_ST_SHAPE)
        set_error("%s: %s (%d rows of %d tokens, %d tokens)", who, STATUS_TEXT[o.status], o.rows, o.cols, o.n_tokens);
    else if (o.status == DAT_ST_UNDECIDED)
        set_error("%s: %s (%d of them: the conversion could not be decided exactly)", who, STATUS_TEXT[o.status], o.n_undecided);
    else
        set_error("%s: %s", who, STATUS_TEXT[o.status]);
    return PRE3_E_ARG;
}

}  // namespace

}  // namespace pre3

using namespace pre3;

extern "C" {

int pre3_sr_text_limits(int32_t *chunk_bytes, int64_t *max_bytes)
{
    if (chunk_bytes) *chunk_bytes = DAT_CHUNK;
    if (max_bytes) *max_bytes = DAT_MAX_BYTES;
    return PRE3_OK;
}

int pre3_sr_text_parse(int device, const char *text, size_t nbytes, double *out, size_t cap, pre3_sr_text_info *info)
{
    const char *who = "pre3_sr_text_parse";
    PRE3_CHECK(info != nullptr && (text != nullptr || nbytes == 0) && (out != nullptr || cap == 0), PRE3_E_ARG, "%s: null argument", who);
    PRE3_CHECK((int64_t)nbytes <= DAT_MAX_BYTES, PRE3_E_ARG, "%s: %zu bytes of text, above the %lld the offsets are laid out for", who, nbytes, (long long)DAT_MAX_BYTES);
    if (nbytes == 0) { info_empty(info); return refuse(who, *info); }
    PRE3_TRY(select_device(who, device));
    const uint64_t *table = nullptr;
    PRE3_TRY(table_on_device(device, &table));
    const size_t room = std::min(cap, (nbytes + 1) / 2);    // a token and its separator take two bytes
    const DatLayout l = dat_layout(nbytes, room);
    const size_t o_out = l.total;
    Scratch d;
    PRE3_TRY(d.alloc(o_out + sizeof(double) * (room + 1)));
    char *work = d.as<char>();
    PRE3_HIP(hipMemcpy(work, text, nbytes, hipMemcpyHostToDevice));
    DatStatus s;
    PRE3_TRY(dat_launch(work, l, nbytes, (long long)room, table, (double *)(work + o_out), 0, 0, &s, nullptr));
    PRE3_HIP(hipStreamSynchronize(nullptr));
    DatInfo di;
    dat_finish(s, (int64_t)nbytes, (int64_t)(nbytes + 1) / 2, 0, 0, &di);       // every text fits its own bound: the room is the caller's matter
    info_out(di, info);
    if (di.status != DAT_ST_OK) return refuse(who, *info);
    PRE3_CHECK((size_t)di.n_tokens <= cap, PRE3_E_NOMEM, "%s: %d rows of %d tokens, room for %zu doubles", who, di.rows, di.cols, cap);
    PRE3_HIP(hipMemcpy(out, work + o_out, sizeof(double) * (size_t)di.n_tokens, hipMemcpyDeviceToHost));
    return PRE3_OK;
}

int pre3_sr_frame_load_text(pre3_sr_frame *f, int mode, const char *text, size_t nbytes, pre3_sr_text_info *info)
{
    const char *who = "pre3_sr_frame_load_text";
    PRE3_CHECK(f != nullptr && info != nullptr && (text != nullptr || nbytes == 0), PRE3_E_ARG, "%s: null argument", who);
    PRE3_CHECK(mode == 0 || mode == 1, PRE3_E_ARG, "%s: mode %d is neither 0 (read_xyz_sr4000) nor 1 (read_sr4000_data_dr_ye)", who, mode);
    PRE3_CHECK((int64_t)nbytes <= DAT_MAX_BYTES, PRE3_E_ARG, "%s: %zu bytes of text, above the %lld the offsets are laid out for", who, nbytes, (long long)DAT_MAX_BYTES);
    if (nbytes == 0) { info_empty(info); return refuse(who, *info); }
    PRE3_TRY(select_device(who, f->device));
    const uint64_t *table = nullptr;
    PRE3_TRY(table_on_device(f->device, &table));
    const size_t npix = (size_t)f->rows * f->cols, cap = (5 * (size_t)f->rows + 1) * f->cols;
    const DatLayout l = dat_layout(nbytes, cap);
    PRE3_HIP(hipStreamSynchronize(f->stream));                // the staging block may still be the source of the previous load's transfer
    PRE3_TRY(sr_grow_stage(f, up16(nbytes) + sizeof(DatStatus)));
    PRE3_TRY(sr_frame_text_work(f, l.total, sizeof(double) * 5 * npix));
    memcpy(f->stage, text, nbytes);
    DatStatus *pinned = (DatStatus *)((char *)f->stage + up16(nbytes));
    PRE3_HIP(hipMemcpyAsync(f->text_dev, f->stage, nbytes, hipMemcpyHostToDevice, f->stream));
    PRE3_TRY(dat_launch((char *)f->text_dev, l, nbytes, (long long)cap, table, f->spare, f->rows, f->cols, pinned, f->stream));
    PRE3_HIP(hipStreamSynchronize(f->stream));                // the one wait: has_conf, the timestamp, and whether the file is taken at all
    DatInfo di;
    dat_finish(*pinned, (int64_t)nbytes, (int64_t)cap, f->rows, f->cols, &di);
    info_out(di, info);
    if (di.status != DAT_ST_OK) return refuse(who, *info);   // the frame, `loaded` and the keypoint record are as they were
    std::swap(f->raw, f->spare);
    f->loaded = 0; f->kp_valid = 0;                           // the keypoint record belongs to the frame that is being replaced
    PRE3_TRY(sr_condition_run(f, mode, di.has_conf != 0));
    return PRE3_OK;
}

}  // extern "C"
