// pre3_predictu.h -- which increment the prediction takes from the device result block of a VO pair (pre3_predict_pair_seeded):
// fv.m:47 over Calculate_V_Omega_RANSAC_dr_ye.m:41-50 -- u = [T; R2q(R)] of the pair when its solution state is 1, the identity motion otherwise -- and
// the two pairs pre3_vo_pair_seeded refuses after its wait.  __host__ __device__, so that a host program can check the rule
// (tests/test_predict_pair_ref.py); k_predict's device form (pre3_geom.hip) evaluates it once per block.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PRE3_PU_HD __host__ __device__ inline
#else
#define PRE3_PU_HD inline
#endif

namespace pre3 {

// refusal codes, in the order pre3_vo_pair_seeded makes its checks
constexpr int PU_OK = 0;
constexpr int PU_REFUSED_BAD = 1;       // VoPairHeader.bad != 0 with pnum >= 4: pre3_vo_pair_seeded's PRE3_E_HIP
constexpr int PU_REFUSED_NEAR = 2;      // no matched point beyond 0.4 m (dist_ok == 0 with pnum >= 4): its PRE3_E_NUMERIC
// the values block 0 of the prediction leaves in the context's numeric error word (stats[6]; 1 is the factorisation's "S is not positive definite")
constexpr int32_t PU_WORD_BASE = 1;
PRE3_PU_HD int32_t pu_error_word(int refusal) { return PU_WORD_BASE + (int32_t)refusal; }
PRE3_PU_HD int pu_word_refusal(int32_t word) { return word > PU_WORD_BASE && word <= PU_WORD_BASE + PU_REFUSED_NEAR ? (int)(word - PU_WORD_BASE) : PU_OK; }

// u_out = u_in when the pair ended in sta == 1, else [0 0 0 1 0 0 0].  With pnum < 4 no launch behind the match wrote the result block (sta, dist_ok and
// u_in are the zeros of the call's memset): that is a result, not a refusal, and u_in is not read.  u_in is read in the one case that takes it.
PRE3_PU_HD int predict_u_select(int sta, int pnum, int bad, int dist_ok, const double *u_in, double *u_out)
{
    int refusal = PU_OK;
    bool take = false;
    if (pnum >= 4) {
        if (bad != 0) refusal = PU_REFUSED_BAD;
        else if (dist_ok == 0) refusal = PU_REFUSED_NEAR;
        else take = sta == 1;
    }
    if (take) { for (int i = 0; i < 7; ++i) u_out[i] = u_in[i]; }
    else { for (int i = 0; i < 7; ++i) u_out[i] = i == 3 ? 1.0 : 0.0; }
    return refusal;
}

}  // namespace pre3
