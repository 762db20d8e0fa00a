// pre3_vopair.h -- the sizing rule of the VO front end between two resident frames (pre3_vopair.hip) and the device header block the
// launches of one pair call read it from.  __host__ __device__, so that a host program can check the rule (tests/test_vo_pair_ref.py).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PRE3_VP_HD __host__ __device__ inline
#else
#define PRE3_VP_HD inline
#endif

namespace pre3 {

constexpr int VO_RST_CAP = 700;

// vodometry_dr_ye.m:171: rst = min(700, nchoosek(pnum, 4)), in integers.  nchoosek(12, 4) = 495 and nchoosek(13, 4) = 715: only pnum 4 .. 12 fall below the
// cap, so the product is formed for those alone (each quotient below is exact: k consecutive integers hold a multiple of k!).
PRE3_VP_HD int vo_rst(int pnum)
{
    if (pnum < 4) return 0;
    if (pnum >= 13) return VO_RST_CAP;
    const uint64_t p = (uint64_t)pnum;
    const uint64_t c = p * (p - 1) / 2 * (p - 2) / 3 * (p - 3) / 4;
    return c < (uint64_t)VO_RST_CAP ? (int)c : VO_RST_CAP;
}

// what the pairs launch leaves for the launches behind it and for the host: 64 bytes
struct VoPairHeader {
    int32_t pnum;       // size(match, 2)
    int32_t rst;        // vo_rst(pnum)
    int32_t bad;        // k_vo_gather's flags: bit 0 a match names a keypoint that does not exist, bit 1 a keypoint rounds to a pixel outside the image
    int32_t capped;     // hypotheses with a position that hit the redraw cap
    int32_t cand_bad;   // k_fc_gather's flags (pre3_map.hip); the pair call leaves it at zero
    int32_t pad[11];
};
// k_fc_gather's flags
constexpr int FC_BAD_PIXEL = 1, FC_BAD_RHO = 2, FC_BAD_DESC = 4, FC_BAD_INDEX = 8;

}  // namespace pre3
