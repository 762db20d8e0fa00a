// pre3_fast.h -- FAST-9 corners on the resident byte image (pre3_fast.hip): the published segment test in place of
// mex_files/Fast_Cr_Ver1/fast_corner_detect_9.m:59-3284 (a learned decision tree that is NOT the segment test: section 30 has the counts),
// the score and suppression of fast-matlab-src/fast_nonmax.m:61-100.  Integer arithmetic on bytes: every result is exact.
#pragma once
#include "pre3_internal.h"

namespace pre3 {

constexpr int FAST_STRIP = 8;                    // columns a workgroup of k_fast_strip owns
constexpr int FAST_HALO = 4;                     // ... plus this many on either side: 3 for the ring of a neighbour whose score the suppression reads
constexpr int FAST_MAX_DIM = 1024;               // rows of the rectangle (the resident image's bound, PATCH_MAX_DIM): the strip's LDS tile is sized for it
constexpr int FAST_MAX_STRIPS = FAST_MAX_DIM / FAST_STRIP;
constexpr int FAST_MIN_DIM = 7;                  // one candidate pixel: fast_corner_detect_9.m:59-60 scans 4 .. size - 3

constexpr int FAST_BOX_ROWS = 61, FAST_BOX_COLS = 41, FAST_BOX_PIX = FAST_BOX_ROWS * FAST_BOX_COLS;      // initialize_a_feature.m:35-36: semi-sizes 30 (rows), 20 (columns)
constexpr int FAST_BAND = 21;                    // :33 excluded_band = half_patch_size_when_initialized + 1
constexpr int FAST_ALL_BAND = 20;                // initialize_n_features_FAST.m:62-63
constexpr int FAST_RES = 32;                     // doubles of pre3_init_feature_fast's result block: status, attempts, u, v, rho, xyz(3), centres tried (2 x 10)

// allocated with the first call of this file; a context without one issues no launch of pre3_fast.hip
// One block, and its pinned image: [res FAST_RES doubles | rho PRE3_FAST_MAX_CORNERS doubles | hdr 4 | strip counts FAST_MAX_STRIPS |
// uv 2 x PRE3_FAST_MAX_CORNERS | score PRE3_FAST_MAX_CORNERS | verdict PRE3_FAST_MAX_CORNERS | centres 2 x 10] (the last six int32)
struct FastState {
    uint16_t *map = nullptr; size_t map_px = 0;  // per pixel of the rectangle, column-major: bit 15 = listed, bits 0..14 = score
    double *blk = nullptr, *blk_host = nullptr;
    hipEvent_t ev[2] = { nullptr, nullptr }; bool ev_valid = false;    // pre3_kernel_timing: the bracket of the last call's launches
    struct { BlockList fixed; DevBlock map; } mem;   // the owners: blk and blk_host sit on `fixed`, the map grows with the rectangle
};
constexpr size_t FAST_BLK_DOUBLES = FAST_RES + (size_t)PRE3_FAST_MAX_CORNERS;
constexpr size_t FAST_O_STRIPS = 4, FAST_O_UV = FAST_O_STRIPS + FAST_MAX_STRIPS, FAST_O_SCORE = FAST_O_UV + 2 * (size_t)PRE3_FAST_MAX_CORNERS,
                 FAST_O_VERDICT = FAST_O_SCORE + PRE3_FAST_MAX_CORNERS, FAST_O_CENTRES = FAST_O_VERDICT + PRE3_FAST_MAX_CORNERS,
                 FAST_BLK_INTS = FAST_O_CENTRES + 2 * PRE3_FAST_MAX_ATTEMPTS;
constexpr size_t FAST_BLK_BYTES = sizeof(double) * FAST_BLK_DOUBLES + sizeof(int32_t) * FAST_BLK_INTS;

int fast_detect(pre3_ctx *c, int r0, int c0, int rows, int cols, int threshold, int barrier, int nonmax, int32_t *K_out, int32_t *uv_out, int32_t *score_out);
// initialize_a_feature.m:27-215; centres == nullptr: drawn from (seed, seq)
int fast_init_feature(pre3_ctx *c, pre3_sr_frame *f, double std_pxl, int strict_reference, int threshold, int barrier, const int32_t *centres, int attempts,
                      uint64_t seed, uint64_t seq, pre3_fast_init_result *out);
// initialize_n_features_FAST.m:55-145
int fast_init_all(pre3_ctx *c, pre3_sr_frame *f, double std_pxl, int threshold, int barrier, int32_t *K_out, int32_t *n_added_out, int32_t *uv_out,
                  double *rho_out, int32_t *verdict_out);
int fast_timing(pre3_ctx *c, double *detect_ms);
void free_fast(pre3_ctx *c);

}  // namespace pre3
