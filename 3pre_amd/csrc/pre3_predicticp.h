// pre3_predicticp.h -- which increment u and which process noise Pn the prediction takes when a dense ICP has refined the VO pair's pose on the device
// (DESIGN.md section 34): predict_u_select (pre3_predictu.h) decides whether the pair is taken at all, then ICP's u replaces the pair's when the run
// ended by the reference's rule (TestScripts/icp_with_init.m:74, :93-95), every entry of it is finite and its error (:100) passes the caller's gate;
// Pn follows the `noise` argument (PRE3_NOISE_*, include/pre3.h) with section 27's rule and the context's own noise behind it.
// Mode PRE3_NOISE_ICP is the published closed-form estimator (pre3_icpcov.h) and is optimistic: it propagates the sensor's noise only, while two
// independent samplings of a surface end centimetres from the true pose.  Mode PRE3_NOISE_ICP_FLOOR adds the context's Pn to it, entry by entry, so
// that the caller's pre3_set_process_noise acts as a floor.
// __host__ __device__, so that a host program can check the rule over its whole grid (tests/icp_cov_host_main.cpp, tests/test_icp_cov_ref.py).
#pragma once
#include <math.h>
#include <stdint.h>

#include "pre3_predictu.h"
#include "pre3_vocov.h"

namespace pre3 {

constexpr int PI_U_IDENTITY = 0, PI_U_PAIR = 1, PI_U_ICP = 2;                 // taken_out[0]
constexpr int PI_NOISE_CONTEXT = 0, PI_NOISE_PAIR = 1, PI_NOISE_ICP = 2, PI_NOISE_ICP_FLOOR = 3;      // `noise`, and taken_out[1] (= PRE3_NOISE_*)
constexpr int PI_ICP_OK = 1;                                                  // ICP_OK of pre3_icp.h

PRE3_PU_HD bool pi_max_error_ok(double max_error) { return max_error > 0.0; }          // +inf: no gate; NaN and <= 0 are refused by the host

// ICP's u stands for the pair's: only ever asked for a pair predict_u_select takes
PRE3_PU_HD bool pi_icp_u_usable(int icp_sta, const double *u_icp, double icp_error, double max_error)
{
    if (icp_sta != PI_ICP_OK) return false;
    for (int i = 0; i < 7; ++i) if (!isfinite(u_icp[i])) return false;
    return icp_error <= max_error;
}

// returns predict_u_select's refusal; u_out[7], *u_taken (PI_U_*), *noise_taken (PI_NOISE_*).  u_icp is read only when icp_sta == 1.
PRE3_PU_HD int predict_icp_select(int sta, int pnum, int bad, int dist_ok, const double *u_pair, int icp_sta, const double *u_icp, double icp_error, double max_error,
                                  int noise, int cov_pair_status, int cov_icp_status, double *u_out, int *u_taken, int *noise_taken)
{
    const int refusal = predict_u_select(sta, pnum, bad, dist_ok, u_pair, u_out);
    const bool pair = vc_pair_computes(sta, pnum, bad, dist_ok);               // predict_u_select's `take`
    int ut = pair ? PI_U_PAIR : PI_U_IDENTITY;
    if (pair && pi_icp_u_usable(icp_sta, u_icp, icp_error, max_error)) {
        ut = PI_U_ICP;
        for (int i = 0; i < 7; ++i) u_out[i] = u_icp[i];
    }
    int nt = PI_NOISE_CONTEXT;
    if (noise != PI_NOISE_CONTEXT) {
        if ((noise == PI_NOISE_ICP || noise == PI_NOISE_ICP_FLOOR) && ut == PI_U_ICP && cov_icp_status == VC_VALID) nt = noise;
        else if (vc_predict_takes(sta, pnum, bad, dist_ok, cov_pair_status)) nt = PI_NOISE_PAIR;
    }
    *u_taken = ut; *noise_taken = nt;
    return refusal;
}

}  // namespace pre3
