// The rules of 3pre_amd/csrc/pre3_dattext.h built for the host (tests/test_dattext_ref.py): the three launches of pre3_dattext.hip restated as loops
// over their workgroups and lanes, with the header's own summaries, fold, conversion, status rules and table.
//   dattext_host parse LANES PLANE_ROWS FRAME_COLS < text > result      LANES: 16-byte lanes per chunk (the kernels use 256)
//   dattext_host table > 651 x (high, low) uint64
// result: int32 status, rows, cols, has_conf, has_timestamp, n_tokens, n_undecided, bad_row, bad_col; int64 bad_offset; double timestamp;
//         int32 n_exact (tokens the exact comparison decided); int32 n_out; n_out doubles
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pre3_dattext.h"

using namespace pre3;

static DatSum lane_sum(const std::vector<char> &text, size_t base)
{
    DatSum s = dat_sum_zero();
    for (size_t i = base; i < base + 16 && i < text.size(); ++i) {
        const unsigned char c = (unsigned char)text[i];
        dat_sum_byte(s, dat_is_start(i ? (unsigned char)text[i - 1] : 0, i > 0, c), dat_is_nl(c));
    }
    return s;
}

static bool tail_in(const std::vector<DatSum> &recs, long j)
{
    for (long k = j - 1; k >= 0; --k) {
        if (recs[k].nl) return recs[k].tail != 0;
        if (recs[k].ntok > 0) return true;
    }
    return false;
}

int main(int argc, char **argv)
{
    std::vector<uint64_t> T(2 * DAT_TABLE_ROWS);
    dat_build_table(T.data());
    if (argc >= 2 && !strcmp(argv[1], "table")) { fwrite(T.data(), 8, T.size(), stdout); return 0; }
    if (argc < 5 || strcmp(argv[1], "parse")) return 2;
    const int lanes = atoi(argv[2]), plane_rows = atoi(argv[3]), frame_cols = atoi(argv[4]);
    std::vector<char> text;
    char buf[65536];
    for (size_t n; (n = fread(buf, 1, sizeof buf, stdin)) > 0;) text.insert(text.end(), buf, buf + n);
    const size_t nbytes = text.size(), chunk = 16 * (size_t)lanes, nchunks = (nbytes + chunk - 1) / chunk;
    const int64_t cap = plane_rows > 0 ? (int64_t)(5 * plane_rows + 1) * frame_cols : (int64_t)(nbytes + 1) / 2;
    DatStatus st;
    memset(&st, 0, sizeof st);
    st.bad_key = st.ragged_key = ~0ull;
    // k_dat_count: a summary per lane, folded in a tree whose order is the byte order
    std::vector<DatSum> recs(nchunks);
    for (size_t c = 0; c < nchunks; ++c) {
        std::vector<DatSum> s(lanes);
        for (int l = 0; l < lanes; ++l) s[l] = lane_sum(text, c * chunk + 16 * (size_t)l);
        for (int d = 1; d < lanes; d *= 2)
            for (int l = 0; l + d < lanes; l += 2 * d) s[l] = dat_sum_fold(s[l], s[l + d]);
        recs[c] = s[0];
    }
    // k_dat_offsets
    std::vector<uint32_t> tok_off((size_t)cap + 1, 0);
    for (size_t c = 0; c < nchunks; ++c) {
        DatPos pos = { 0, 0, 0 };
        for (size_t j = 0; j < c; ++j) { pos.tok += recs[j].ntok; pos.line += recs[j].nfirst + ((recs[j].lead && !tail_in(recs, (long)j)) ? 1 : 0); }
        pos.tail = tail_in(recs, (long)c) ? 1u : 0u;
        std::vector<DatSum> s(lanes);
        for (int l = 0; l < lanes; ++l) s[l] = lane_sum(text, c * chunk + 16 * (size_t)l);
        for (int d = 1; d < lanes; d *= 2) {                 // the inclusive scan of the kernel, step by step
            std::vector<DatSum> v(s);
            for (int l = d; l < lanes; ++l) v[l] = dat_sum_fold(s[l - d], s[l]);
            s = v;
        }
        for (int l = 0; l < lanes; ++l) {
            DatPos p = l ? dat_pos_advance(pos, s[l - 1]) : pos;
            const size_t base = c * chunk + 16 * (size_t)l;
            for (size_t i = base; i < base + 16 && i < nbytes; ++i) {
                const unsigned char ch = (unsigned char)text[i];
                if (dat_is_nl(ch)) p.tail = 0;
                if (dat_is_start(i ? (unsigned char)text[i - 1] : 0, i > 0, ch)) {
                    const bool first = !p.tail;
                    if (p.tok < cap) tok_off[p.tok] = (uint32_t)i | (first ? DAT_FIRST : 0u);
                    if (first && p.line == 1) st.cols = (int32_t)p.tok;
                    p.line += first ? 1 : 0; p.tail = 1; ++p.tok;
                }
            }
            if (c == nchunks - 1 && l == lanes - 1) { st.n_tokens = (int32_t)p.tok; st.n_lines = (int32_t)p.line; }
        }
    }
    // k_dat_parse
    std::vector<double> out((size_t)cap + 1, 0.0);
    int n_exact = 0;
    const int n = st.n_tokens, lines = st.n_lines, cols = dat_cols(n, lines, st.cols);
    for (int64_t t = 0; n <= cap && t < n; ++t) {
        const uint32_t word = tok_off[t], off = word & ~DAT_FIRST;
        if (((word & DAT_FIRST) != 0) != (t % cols == 0)) { const unsigned long long key = ((unsigned long long)t << 32) | off; if (key < st.ragged_key) st.ragged_key = key; }
        double v = 0.0;
        const int rc = dat_convert(text.data() + off, nbytes - off, T.data(), &v, nullptr);
        if (rc == DAT_BAD) { st.flags |= DAT_F_BAD; const unsigned long long key = ((unsigned long long)t << 32) | off; if (key < st.bad_key) st.bad_key = key; continue; }
        if (rc == DAT_UNDECIDED) { ++st.n_undecided; continue; }
        if (rc & DAT_EXACT) ++n_exact;
        if ((int64_t)lines * cols != n) continue;
        if (plane_rows > 0 && !dat_frame_shape(lines, cols, plane_rows, frame_cols)) continue;
        const int64_t R = t / cols, j = t % cols, idx = dat_store_index(R, j, lines, cols, plane_rows);
        if (idx < 0) { if (j == 0) st.timestamp = v; continue; }
        out[idx] = v;
        if (plane_rows > 0 && R / plane_rows == 3 && !(v >= 0.0 && v <= 1.7976931348623157e308)) st.flags |= DAT_F_AMP;
    }
    DatInfo info;
    dat_finish(st, (int64_t)nbytes, cap, plane_rows, frame_cols, &info);
    const int32_t head[9] = { info.status, info.rows, info.cols, info.has_conf, info.has_timestamp, info.n_tokens, info.n_undecided, info.bad_row, info.bad_col };
    int32_t n_out = info.status == DAT_ST_OK ? (plane_rows > 0 ? (info.has_conf ? 5 : 4) * plane_rows * frame_cols : info.n_tokens) : 0;
    fwrite(head, 4, 9, stdout); fwrite(&info.bad_offset, 8, 1, stdout); fwrite(&info.timestamp, 8, 1, stdout);
    fwrite(&n_exact, 4, 1, stdout); fwrite(&n_out, 4, 1, stdout); fwrite(out.data(), 8, (size_t)n_out, stdout);
    return 0;
}
