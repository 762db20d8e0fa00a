// pre3_dattext.h -- the rules behind the device parse of SR4000 .dat text (pre3_dattext.hip): byte classes, the per-chunk
// summary and its fold, the token grammar, and the decimal-to-double conversion.  read_xyz_sr4000.m:2-3 reads these files with MATLAB's load;
// numpy.loadtxt accepts the same text.
//   separators     space, tab, \r; a row ends at \n or at the end of the text; a line without a token is skipped
//   token          [+-]?digits[.digits*]?([eE][+-]?digits)?  |  [+-]?.digits([eE][+-]?digits)?  |  [+-]?inf  |  [+-]?nan   (any letter case)
//   everything else is a bad token: d/D exponents, % and # comments, commas, a NUL byte, a lone sign or dot
// Conversion: the result equals Python's float(token) bit for bit -- correctly rounded, ties to even.  Up to 19 significant digits go into a uint64 w,
// digits dropped beyond them move the decimal exponent q, and the Eisel-Lemire product (Lemire, "Number parsing at a gigabyte per second", SPE 2021)
// turns (w, q) into a double with a 128-bit truncated power of five from a table of q in [-342, 308] that the library computes itself
// (dat_build_table: exact big integers, host only).  A token whose dropped digits are not all zero lies strictly between w and w + 1: both are
// converted, and when the two doubles differ the token is compared exactly, as big integers, with the midpoint of the two (its first 768 significant
// digits -- no midpoint of two doubles has more --; a longer one is again an interval, and undecided should the interval straddle the midpoint).  A token that stays undecided -- that, or the
// algorithm's own "cannot decide" branch -- is reported, never stored as a guess.
// Everything here is __host__ __device__ except the table builder: the same text runs in the kernels and in tests/dattext_host_main.cpp.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "pre3_philox.h"        // PRE3_HD, mulhi64

namespace pre3 {

constexpr int DAT_Q_MIN = -342, DAT_Q_MAX = 308, DAT_TABLE_ROWS = DAT_Q_MAX - DAT_Q_MIN + 1;      // 651 rows of (high word, low word)
constexpr int DAT_W_DIGITS = 19;            // significant digits that fit a uint64
constexpr int DAT_EXACT_DIGITS = 768;       // ... that the exact comparison takes
constexpr int DAT_BIG_WORDS = 96;           // 3072 bits: 2^54 * 5^1110 aligned with a 768-digit integer, with room (dat_exact_cmp)
enum { DAT_OK = 0, DAT_BAD = 1, DAT_UNDECIDED = 2, DAT_EXACT = 4 /* informational: the exact comparison decided it */ };
enum { DAT_ST_OK = 0, DAT_ST_BAD = 1, DAT_ST_RAGGED = 2, DAT_ST_SHAPE = 3, DAT_ST_UNDECIDED = 4, DAT_ST_AMPLITUDE = 5, DAT_ST_EMPTY = 6 };

PRE3_HD bool dat_is_sep(unsigned char c) { return c == ' ' || c == '\t' || c == '\r'; }
PRE3_HD bool dat_is_nl(unsigned char c) { return c == '\n'; }
PRE3_HD bool dat_is_gap(unsigned char c) { return dat_is_sep(c) || dat_is_nl(c); }
// byte i starts a token: it is no gap byte and its predecessor is one (or there is none)
PRE3_HD bool dat_is_start(unsigned char prev, bool has_prev, unsigned char c) { return !dat_is_gap(c) && (!has_prev || dat_is_gap(prev)); }

// ---- what a stretch of bytes says about tokens and lines, and the fold of two adjacent stretches (associative, not commutative).
// ntok: token starts.  nfirst: first-of-line starts that the stretch decides alone (a \n of its own in front of them).  lead: a token start in front
// of the stretch's first \n -- first of its line when no token precedes it on that line, which the stretch in front decides.  nl: a \n was seen.
// tail: a token start behind the last \n (without a \n: any token start).
struct DatSum { int32_t ntok, nfirst; uint32_t lead, nl, tail; };

PRE3_HD DatSum dat_sum_zero() { DatSum s; s.ntok = 0; s.nfirst = 0; s.lead = 0; s.nl = 0; s.tail = 0; return s; }

PRE3_HD void dat_sum_byte(DatSum &s, bool start, bool nl)
{
    if (nl) { s.nl = 1; s.tail = 0; }
    if (start) {
        ++s.ntok;
        if (!s.tail) { if (s.nl) ++s.nfirst; else s.lead = 1; }
        s.tail = 1;
    }
}

PRE3_HD DatSum dat_sum_fold(const DatSum &a, const DatSum &b)
{
    DatSum s;
    s.ntok = a.ntok + b.ntok;
    s.nfirst = a.nfirst + b.nfirst + ((b.lead && a.nl && !a.tail) ? 1 : 0);
    s.lead = (a.lead || (!a.nl && !a.tail && b.lead)) ? 1u : 0u;
    s.nl = a.nl | b.nl;
    s.tail = b.nl ? b.tail : (a.tail | b.tail);
    return s;
}

// the running position in front of a stretch: tokens and non-empty lines so far, and whether the current line already has a token
struct DatPos { int64_t tok, line; uint32_t tail; };

PRE3_HD DatPos dat_pos_advance(const DatPos &p, const DatSum &s)
{
    DatPos r;
    r.tok = p.tok + s.ntok;
    r.line = p.line + s.nfirst + ((s.lead && !p.tail) ? 1 : 0);
    r.tail = s.nl ? s.tail : (p.tail | s.tail);
    return r;
}

// ---- fixed-size unsigned big integers, little-endian 32-bit words (the exact comparison and the table builder)
struct DatBig { uint32_t w[DAT_BIG_WORDS]; int n; };       // n: words in use (the value 0 has n == 0)

PRE3_HD void dat_big_set(DatBig &a, uint64_t v)
{
    a.n = 0;
    if (v) { a.w[a.n++] = (uint32_t)v; if (v >> 32) a.w[a.n++] = (uint32_t)(v >> 32); }
}
// a = a * m + add; false when it would not fit
PRE3_HD bool dat_big_muladd(DatBig &a, uint32_t m, uint32_t add)
{
    uint64_t c = add;
    for (int i = 0; i < a.n; ++i) { c += (uint64_t)a.w[i] * m; a.w[i] = (uint32_t)c; c >>= 32; }
    if (c) { if (a.n >= DAT_BIG_WORDS) return false; a.w[a.n++] = (uint32_t)c; }
    return true;
}
PRE3_HD bool dat_big_mul_pow5(DatBig &a, int e)
{
    for (; e >= 13; e -= 13) if (!dat_big_muladd(a, 1220703125u, 0)) return false;      // 5^13 < 2^32
    uint32_t m = 1;
    for (; e > 0; --e) m *= 5;
    return dat_big_muladd(a, m, 0);
}
PRE3_HD bool dat_big_shl(DatBig &a, int bits)
{
    if (a.n == 0 || bits == 0) return true;
    const int ws = bits >> 5, bs = bits & 31;
    if (a.n + ws + 1 > DAT_BIG_WORDS) return false;
    a.w[a.n] = 0;
    for (int i = a.n; i >= 0; --i) {
        const uint32_t hi = i < a.n ? a.w[i] : 0u, lo = i > 0 ? a.w[i - 1] : 0u;
        a.w[i + ws] = bs ? ((hi << bs) | (lo >> (32 - bs))) : hi;
    }
    for (int i = 0; i < ws; ++i) a.w[i] = 0;
    a.n += ws + 1;
    while (a.n > 0 && a.w[a.n - 1] == 0) --a.n;
    return true;
}
PRE3_HD int dat_big_cmp(const DatBig &a, const DatBig &b)
{
    if (a.n != b.n) return a.n < b.n ? -1 : 1;
    for (int i = a.n - 1; i >= 0; --i)
        if (a.w[i] != b.w[i]) return a.w[i] < b.w[i] ? -1 : 1;
    return 0;
}

// sign of D * 10^k - M * 2^e for D, M > 0; 2 when a product does not fit (never for D <= 10^768, k in [-1200, 330], M < 2^55, e in [-1080, 980], D * 10^k within a factor 2 of M * 2^e)
PRE3_HD int dat_exact_cmp(DatBig &D, int k, uint64_t M, int e)
{
    DatBig B;
    dat_big_set(B, M);
    int sd = 0, sb = e;                                     // D * 5^.. * 2^sd  against  B * 5^.. * 2^sb
    if (k >= 0) { if (!dat_big_mul_pow5(D, k)) return 2; sd = k; }
    else { if (!dat_big_mul_pow5(B, -k)) return 2; sb = e - k; }
    const int lo = sd < sb ? sd : sb;
    if (!dat_big_shl(D, sd - lo) || !dat_big_shl(B, sb - lo)) return 2;
    return dat_big_cmp(D, B);
}

// ---- Eisel-Lemire: w != 0, q in [DAT_Q_MIN, DAT_Q_MAX], T the table.  The double's bits without its sign; DAT_UNDECIDED for the branch the algorithm
// cannot decide (the low word all ones with q outside [-27, 55]).
PRE3_HD int dat_lemire(uint64_t w, int q, const uint64_t *T, uint64_t *bits)
{
    const int lz = __builtin_clzll(w);
    w <<= lz;
    const uint64_t t_hi = T[2 * (q - DAT_Q_MIN)], t_lo = T[2 * (q - DAT_Q_MIN) + 1];
    uint64_t upper = mulhi64(w, t_hi), lower = w * t_hi;
    if ((upper & 0x1FFull) == 0x1FFull) {
        const uint64_t second_hi = mulhi64(w, t_lo);
        lower += second_hi;
        if (second_hi > lower) ++upper;
    }
    if (lower == ~0ull && (q < -27 || q > 55)) return DAT_UNDECIDED;
    const int upperbit = (int)(upper >> 63);
    const int shift = upperbit + 9;                         // 64 - 52 - 3
    uint64_t mant = upper >> shift;
    int power2 = (int)(((int64_t)(152170 + 65536) * q) >> 16) + 63 + upperbit - lz + 1023;
    if (power2 <= 0) {                                      // subnormal (or it rounds up to the smallest normal)
        if (-power2 + 1 >= 64) { *bits = 0; return DAT_OK; }
        mant >>= -power2 + 1;
        mant += mant & 1;
        mant >>= 1;
        *bits = mant;                                       // mant == 2^52: exponent field 1, fraction 0 -- the same bits
        return DAT_OK;
    }
    if (lower <= 1 && q >= -4 && q <= 23 && (mant & 3) == 1 && (mant << shift) == upper) mant &= ~1ull;      // an exact tie: to even
    mant += mant & 1;
    mant >>= 1;
    if (mant >= (2ull << 52)) { mant = 1ull << 52; ++power2; }
    mant &= ~(1ull << 52);
    if (power2 >= 0x7FF) { *bits = 0x7FFull << 52; return DAT_OK; }
    *bits = mant | ((uint64_t)power2 << 52);
    return DAT_OK;
}

PRE3_HD int dat_scaled(uint64_t w, int64_t q, const uint64_t *T, uint64_t *bits)
{
    if (w == 0 || q < DAT_Q_MIN) { *bits = 0; return DAT_OK; }                 // w < 2^64: below half the smallest subnormal
    if (q > DAT_Q_MAX) { *bits = 0x7FFull << 52; return DAT_OK; }
    return dat_lemire(w, (int)q, T, bits);
}

PRE3_HD double dat_from_bits(uint64_t b)
{
    double d;
    __builtin_memcpy(&d, &b, sizeof d);
    return d;
}

PRE3_HD unsigned char dat_lower(unsigned char c) { return (c >= 'A' && c <= 'Z') ? (unsigned char)(c + 32) : c; }

// the first DAT_EXACT_DIGITS significant digits of p[from, to) (digits and at most one point) as an integer, plus one on request; *more: a non-zero
// digit behind them.  Returns how many it took.
PRE3_HD int dat_digits_big(const char *p, size_t from, size_t to, bool plus_one, DatBig &D, bool *more)
{
    int taken = 0;
    D.n = 0; *more = false;
    for (size_t j = from; j < to; ++j) {
        if (p[j] == '.') continue;
        const unsigned d = (unsigned)(p[j] - '0');
        if (taken < DAT_EXACT_DIGITS) { (void)dat_big_muladd(D, 10, d); if (D.n) ++taken; }
        else *more |= d != 0;
    }
    if (plus_one) (void)dat_big_muladd(D, 1, 1);
    return taken;
}

// The token at p (p[0] is no gap byte; avail >= 1 bytes are readable): its length up to the next gap byte or the end, and its value.
// Returns DAT_OK (| DAT_EXACT), DAT_BAD or DAT_UNDECIDED; *out is written for DAT_OK only.
PRE3_HD int dat_convert(const char *p, size_t avail, const uint64_t *T, double *out, size_t *len_out)
{
    size_t len = 0;
    while (len < avail && !dat_is_gap((unsigned char)p[len])) ++len;
    if (len_out) *len_out = len;
    size_t i = 0;
    uint64_t sign = 0;
    if (p[0] == '+' || p[0] == '-') { sign = p[0] == '-' ? 1ull << 63 : 0; i = 1; }
    if (len - i == 3) {
        const unsigned char a = dat_lower((unsigned char)p[i]), b = dat_lower((unsigned char)p[i + 1]), c = dat_lower((unsigned char)p[i + 2]);
        if (a == 'i' && b == 'n' && c == 'f') { *out = dat_from_bits(sign | (0x7FFull << 52)); return DAT_OK; }
        if (a == 'n' && b == 'a' && c == 'n') { *out = dat_from_bits(sign | (0x7FF8ull << 48)); return DAT_OK; }
    }
    uint64_t w = 0;
    int nd = 0;
    int64_t q = 0;
    bool any = false, dropped = false;
    const size_t digits_at = i;
    for (; i < len && p[i] >= '0' && p[i] <= '9'; ++i) {
        const unsigned d = (unsigned)(p[i] - '0');
        any = true;
        if (nd < DAT_W_DIGITS) { w = w * 10 + d; if (w) ++nd; }
        else { ++q; dropped |= d != 0; }
    }
    if (i < len && p[i] == '.') {
        for (++i; i < len && p[i] >= '0' && p[i] <= '9'; ++i) {
            const unsigned d = (unsigned)(p[i] - '0');
            any = true;
            if (nd < DAT_W_DIGITS) { w = w * 10 + d; if (w) ++nd; --q; }
            else dropped |= d != 0;
        }
    }
    if (!any) return DAT_BAD;
    const size_t digits_end = i;
    if (i < len && (p[i] == 'e' || p[i] == 'E')) {
        ++i;
        bool eneg = false;
        if (i < len && (p[i] == '+' || p[i] == '-')) { eneg = p[i] == '-'; ++i; }
        if (!(i < len && p[i] >= '0' && p[i] <= '9')) return DAT_BAD;
        int64_t e = 0;
        for (; i < len && p[i] >= '0' && p[i] <= '9'; ++i)
            if (e < (1ll << 40)) e = e * 10 + (p[i] - '0');
        q += eneg ? -e : e;
    }
    if (i != len) return DAT_BAD;
    uint64_t b0 = 0, b1 = 0;
    int rc = dat_scaled(w, q, T, &b0);
    if (rc != DAT_OK) return rc;
    if (!dropped) { *out = dat_from_bits(sign | b0); return DAT_OK; }
    rc = dat_scaled(w + 1, q, T, &b1);                     // w + 1 <= 10^19 < 2^64
    if (rc != DAT_OK) return rc;
    if (b0 == b1) { *out = dat_from_bits(sign | b0); return DAT_OK; }
    // b0 and b1 are neighbours (the interval is far narrower than their gap), b0 finite: the token against their midpoint (2 m + 1) * 2^(e - 1)
    if (b1 != b0 + 1) return DAT_UNDECIDED;
    const int ef = (int)(b0 >> 52);
    const uint64_t m = ef ? ((b0 & ((1ull << 52) - 1)) | (1ull << 52)) : b0;
    const int e2 = (ef ? ef : 1) - 1075;
    DatBig D;
    bool more = false;
    const int taken = dat_digits_big(p, digits_at, digits_end, false, D, &more);
    const int64_t k = q + DAT_W_DIGITS - taken;             // w holds 19 significant digits at exponent q; D holds `taken` of them
    if (k < -1200 || k > 330) return DAT_UNDECIDED;
    int c = dat_exact_cmp(D, (int)k, 2 * m + 1, e2 - 1);
    if (c == 2) return DAT_UNDECIDED;
    if (more) {                                             // strictly between D and D + 1
        if (c < 0) {
            (void)dat_digits_big(p, digits_at, digits_end, true, D, &more);
            const int c1 = dat_exact_cmp(D, (int)k, 2 * m + 1, e2 - 1);
            if (c1 == 2 || c1 > 0) return DAT_UNDECIDED;   // c1 == 0: still below the midpoint, strictly
        } else c = 1;                                       // at or above D >= the midpoint, and strictly above D
    }
    const uint64_t r = c < 0 ? b0 : (c > 0 ? b1 : ((b0 & 1) ? b1 : b0));
    *out = dat_from_bits(sign | r);
    return DAT_OK | DAT_EXACT;
}

// ---- what the three launches leave for the host, and what the host makes of it.
// tok_off[t]: the byte offset of token t, DAT_FIRST set on the first token of a line.  The text is rectangular exactly when token t carries DAT_FIRST
// for t % cols == 0 and for no other t, and n_tokens % cols == 0 -- cols being the token count of the first non-empty line.
constexpr uint32_t DAT_FIRST = 0x80000000u;
constexpr int DAT_CHUNK = 4096;                             // bytes per workgroup of k_dat_count / k_dat_offsets: 256 lanes x 16 bytes
constexpr int64_t DAT_MAX_BYTES = 1ll << 25;                // offsets share a word with DAT_FIRST; 8192 chunk records at most
enum { DAT_F_BAD = 1, DAT_F_AMP = 4 };
struct DatStatus {
    unsigned long long bad_key, ragged_key;                 // (token << 32 | byte offset) of the first bad token / the first token that breaks the rule above
    double timestamp;                                       // token (5 rows, 0) of a frame
    int32_t n_tokens, n_lines, cols, flags, n_undecided, pad_;      // cols: the ordinal of the second line's first token (0: there is one line)
};
struct DatInfo { int32_t status, rows, cols, has_conf, has_timestamp, n_tokens, n_undecided, bad_row, bad_col; int64_t bad_offset; double timestamp; };

PRE3_HD int dat_cols(int n_tokens, int n_lines, int cols_word) { return n_lines <= 1 ? n_tokens : cols_word; }
// a frame of plane_rows x frame_cols: 4, 5 or 5 + 1/plane_rows blocks of rows (read_xyz_sr4000.m:25-42)
PRE3_HD bool dat_frame_shape(int n_lines, int cols, int plane_rows, int frame_cols)
{
    return cols == frame_cols && (n_lines == 4 * plane_rows || n_lines == 5 * plane_rows || n_lines == 5 * plane_rows + 1);
}

// The status rules, in this order: empty text, more tokens than the caller holds room for (shape), ragged rows, a bad token, an undecided token,
// a frame of another shape (plane_rows > 0), an amplitude that is negative or not finite.
inline void dat_finish(const DatStatus &s, int64_t nbytes, int64_t cap_tokens, int plane_rows, int frame_cols, DatInfo *o)
{
    const int cols = dat_cols(s.n_tokens, s.n_lines, s.cols);
    o->status = DAT_ST_OK; o->rows = s.n_lines; o->cols = cols; o->has_conf = 0; o->has_timestamp = 0; o->n_tokens = s.n_tokens;
    o->n_undecided = s.n_undecided; o->bad_row = -1; o->bad_col = -1; o->bad_offset = -1; o->timestamp = -1.0;
    if (s.n_tokens == 0) { o->status = DAT_ST_EMPTY; return; }
    if (s.n_tokens > cap_tokens) { o->status = DAT_ST_SHAPE; return; }
    const bool broke = s.ragged_key != ~0ull;
    if (broke || s.n_tokens % cols != 0) {
        const int64_t m = broke ? (int64_t)(s.ragged_key >> 32) : s.n_tokens;      // a short line shows at the next line's first token, a long one at its first extra token
        o->status = DAT_ST_RAGGED;
        o->bad_row = (int32_t)((m - 1) / cols); o->bad_col = (int32_t)(m - (int64_t)o->bad_row * cols);
        o->bad_offset = broke ? (int64_t)(s.ragged_key & 0xFFFFFFFFull) : nbytes;
        return;
    }
    if (s.flags & DAT_F_BAD) {
        const int64_t t = (int64_t)(s.bad_key >> 32);
        o->status = DAT_ST_BAD; o->bad_row = (int32_t)(t / cols); o->bad_col = (int32_t)(t % cols); o->bad_offset = (int64_t)(s.bad_key & 0xFFFFFFFFull);
        return;
    }
    if (s.n_undecided > 0) { o->status = DAT_ST_UNDECIDED; return; }
    if (plane_rows > 0) {
        if (!dat_frame_shape(s.n_lines, cols, plane_rows, frame_cols)) { o->status = DAT_ST_SHAPE; return; }
        o->has_conf = s.n_lines >= 5 * plane_rows ? 1 : 0;
        o->has_timestamp = s.n_lines == 5 * plane_rows + 1 ? 1 : 0;
        if (o->has_timestamp) o->timestamp = s.timestamp;
        if (s.flags & DAT_F_AMP) o->status = DAT_ST_AMPLITUDE;
    }
}

// where token t = (R, j) of a text of n_lines x cols goes: a matrix, column-major (plane_rows == 0), or the five planes of a frame in file order
// z, x, y, amplitude, confidence, each plane_rows x cols column-major; -1: the timestamp row
PRE3_HD int64_t dat_store_index(int64_t R, int64_t j, int n_lines, int cols, int plane_rows)
{
    if (plane_rows == 0) return R + j * n_lines;
    if (R >= 5 * (int64_t)plane_rows) return -1;
    return (R / plane_rows) * plane_rows * cols + R % plane_rows + j * plane_rows;
}

// ---- the table, host only: row q - DAT_Q_MIN = (high word, low word) of
//   q >= 0: 5^q scaled into [2^127, 2^128), truncated
//   q <  0: floor(2^b / 5^-q) + 1, b = z + 127 for q >= -27 and b = 2 z + 128 (the result halved until it is below 2^128) otherwise, z the smallest
//           integer with 2^z >= 5^-q
struct DatWide { uint32_t w[64]; };                         // 2048 bits

inline int dat_wide_bitlen(const DatWide &a)
{
    for (int i = 63; i >= 0; --i)
        if (a.w[i]) { int b = 32; while (!(a.w[i] >> (b - 1))) --b; return 32 * i + b; }
    return 0;
}
inline int dat_wide_bit(const DatWide &a, int i) { return i < 0 ? 0 : (int)((a.w[i >> 5] >> (i & 31)) & 1u); }
// the top 128 bits of a (bit length L): a >> (L - 128), or a << (128 - L)
inline void dat_wide_top128(const DatWide &a, uint64_t *hi, uint64_t *lo)
{
    const int L = dat_wide_bitlen(a);
    uint64_t h = 0, l = 0;
    for (int k = 0; k < 64; ++k) { h = (h << 1) | (uint64_t)dat_wide_bit(a, L - 1 - k); l = (l << 1) | (uint64_t)dat_wide_bit(a, L - 65 - k); }
    *hi = h; *lo = l;
}
inline void dat_wide_mul5(DatWide &a)
{
    uint64_t c = 0;
    for (int i = 0; i < 64; ++i) { c += (uint64_t)a.w[i] * 5u; a.w[i] = (uint32_t)c; c >>= 32; }
}

inline void dat_build_table(uint64_t *T /* [DAT_TABLE_ROWS][2] */)
{
    DatWide p;
    for (int i = 0; i < 64; ++i) p.w[i] = 0;
    p.w[0] = 1;
    for (int q = 0; q <= DAT_Q_MAX; ++q) {
        dat_wide_top128(p, &T[2 * (q - DAT_Q_MIN)], &T[2 * (q - DAT_Q_MIN) + 1]);
        dat_wide_mul5(p);
    }
    for (int i = 0; i < 64; ++i) p.w[i] = 0;
    p.w[0] = 1;
    for (int q = -1; q >= DAT_Q_MIN; --q) {
        dat_wide_mul5(p);                                   // 5^-q, no power of two: z is its bit length
        const int z = dat_wide_bitlen(p), b = q >= -27 ? z + 127 : 2 * z + 128, pw = (z + 31) / 32 + 1;
        DatWide r, c;
        for (int i = 0; i < 64; ++i) { r.w[i] = 0; c.w[i] = 0; }
        r.w[0] = 1;                                         // the dividend 2^b, one doubling per quotient bit
        for (int s = b - 1; s >= 0; --s) {
            uint32_t carry = 0;
            for (int i = 0; i < pw; ++i) { const uint32_t v = r.w[i]; r.w[i] = (v << 1) | carry; carry = v >> 31; }
            bool ge = true;
            for (int i = pw - 1; i >= 0; --i)
                if (r.w[i] != p.w[i]) { ge = r.w[i] > p.w[i]; break; }
            if (ge) {
                uint64_t bw = 0;
                for (int i = 0; i < pw; ++i) { const uint64_t d = (uint64_t)r.w[i] - p.w[i] - bw; r.w[i] = (uint32_t)d; bw = (d >> 32) & 1u; }
                c.w[s >> 5] |= 1u << (s & 31);
            }
        }
        for (int i = 0; i < 64; ++i) { if (++c.w[i] != 0) break; }      // + 1
        dat_wide_top128(c, &T[2 * (q - DAT_Q_MIN)], &T[2 * (q - DAT_Q_MIN) + 1]);
    }
}

}  // namespace pre3
