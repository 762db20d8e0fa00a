/* vo_gateway.c -- MEX binding of pre3_vo_ransac_frames: replaces the hypothesis loop of vodometry_dr_ye.m:171-236
 * (ransac_dr_ye.m + find_transform_matrix_dr_ye.m) with one device call.
 *
 *   [rot, trans, sta, op_match, stat] = pre3_vo(frm1, frm2, match, x1, y1, z1, x2, y2, z2, draws)
 *
 *   frm1, frm2 : 4 x K SIFT frames (rows 1:2 = column,row, 1-based)       match : 2 x pnum (siftmatch output)
 *   x*, y*, z* : rows x cols range images                                  draws : 4 x rst positions (1-based), drawn with
 *                                                                                  ransac_dr_ye.m:28-46's rule by the caller
 *   stat = [nIterationRansac nSupport ErrorMean ErrorStd phi theta psi u(1:7)]
 *
 *   [rot, trans, sta, op_match, stat, draws, capped] = pre3_vo(frm1, frm2, match, x1, y1, z1, x2, y2, z2, seed, seq [, rst])
 *
 *   the seeded form (pre3_vo_ransac_frames_seeded): the draws are made on the device from (seed, seq) by ransac_dr_ye.m:28-48's rule; seed and seq are
 *   scalar doubles (whole numbers up to 2^53), rst defaults to min(700, nchoosek(pnum, 4)) (vodometry_dr_ye.m:171).  draws comes back 4 x rst, 1-based;
 *   capped = hypotheses a position of which hit the 64-redraw cap (the reference would not have returned).
 * NOT compiled in the build container (no MATLAB / mex.h there); build: mex -output pre3_vo mex/vo_gateway.c -Iinclude -L3pre_amd/lib -lpre3
 */
#include <string.h>
#include "mex.h"
#include "pre3.h"

void mexFunction(int nout, mxArray *out[], int nin, const mxArray *in[])
{
    pre3_vo_result r;
    int pnum, n_hyp, i, rc, k, seeded;
    int32_t *draws, *inl, capped = 0;
    double *m;
    if (nin < 10 || nin > 12) mexErrMsgTxt("pre3_vo: ten input arguments required (eleven or twelve for the seeded form)");
    seeded = nin > 10;
    pnum = (int)mxGetN(in[2]);
    if (seeded) {
        double c = 1.0;                     /* min(700, nchoosek(pnum, 4)), vodometry_dr_ye.m:171 */
        for (i = 0; i < 4 && c <= 700.0 * 24.0; ++i) c *= (double)(pnum - i);
        n_hyp = nin > 11 ? (int)mxGetScalar(in[11]) : (pnum < 4 ? 0 : (c / 24.0 < 700.0 ? (int)(c / 24.0 + 0.5) : 700));
    } else {
        n_hyp = (int)mxGetN(in[9]);
        if (mxGetM(in[9]) != 4) mexErrMsgTxt("pre3_vo: draws must be 4 x rst");
    }
    draws = (int32_t *)mxMalloc(sizeof(int32_t) * 4 * (n_hyp > 0 ? n_hyp : 1));
    inl = (int32_t *)mxCalloc(pnum ? pnum : 1, sizeof(int32_t));
    if (seeded)
        rc = pre3_vo_ransac_frames_seeded(0, (int)mxGetM(in[3]), (int)mxGetN(in[3]), mxGetPr(in[3]), mxGetPr(in[4]), mxGetPr(in[5]), mxGetPr(in[6]),
                                          mxGetPr(in[7]), mxGetPr(in[8]), (int)mxGetM(in[0]), (int)mxGetN(in[0]), mxGetPr(in[0]), (int)mxGetN(in[1]),
                                          mxGetPr(in[1]), pnum, mxGetPr(in[2]), n_hyp, (uint64_t)mxGetScalar(in[9]), (uint64_t)mxGetScalar(in[10]),
                                          draws, &capped, NULL, NULL, NULL, NULL, inl, &r);
    else {
        for (i = 0; i < 4 * n_hyp; ++i) draws[i] = (int32_t)mxGetPr(in[9])[i] - 1;
        rc = pre3_vo_ransac_frames(0, (int)mxGetM(in[3]), (int)mxGetN(in[3]), mxGetPr(in[3]), mxGetPr(in[4]), mxGetPr(in[5]), mxGetPr(in[6]),
                                   mxGetPr(in[7]), mxGetPr(in[8]), (int)mxGetM(in[0]), (int)mxGetN(in[0]), mxGetPr(in[0]), (int)mxGetN(in[1]),
                                   mxGetPr(in[1]), pnum, mxGetPr(in[2]), n_hyp, draws, NULL, NULL, NULL, NULL, inl, &r);
    }
    if (rc != PRE3_OK) { mxFree(draws); mxFree(inl); mexErrMsgTxt(pre3_last_error()); }
    if (nout > 5) {
        out[5] = mxCreateDoubleMatrix(4, n_hyp, mxREAL);
        for (i = 0; i < 4 * n_hyp; ++i) mxGetPr(out[5])[i] = draws[i] + 1;
    }
    if (nout > 6) out[6] = mxCreateDoubleScalar((double)capped);
    mxFree(draws);
    out[0] = mxCreateDoubleMatrix(3, 3, mxREAL);
    for (i = 0; i < 3; ++i) for (k = 0; k < 3; ++k) mxGetPr(out[0])[i + 3 * k] = r.rot[3 * i + k];      /* row-major -> column-major */
    if (nout > 1) { out[1] = mxCreateDoubleMatrix(3, 1, mxREAL); memcpy(mxGetPr(out[1]), r.trans, sizeof r.trans); }
    if (nout > 2) out[2] = mxCreateDoubleScalar(r.sta);
    if (nout > 3) {
        out[3] = mxCreateDoubleMatrix(2, r.sta == 4 ? 0 : r.n_support, mxREAL);
        m = mxGetPr(out[3]);
        if (r.sta != 4) for (i = 0, k = 0; i < pnum; ++i) if (inl[i]) { m[2 * k] = mxGetPr(in[2])[2 * i]; m[2 * k + 1] = mxGetPr(in[2])[2 * i + 1]; ++k; }
    }
    if (nout > 4) {
        out[4] = mxCreateDoubleMatrix(1, 14, mxREAL);
        m = mxGetPr(out[4]);
        m[0] = r.n_iterations; m[1] = r.n_support; m[2] = r.error_mean; m[3] = r.error_std;
        memcpy(m + 4, r.euler, sizeof r.euler); memcpy(m + 7, r.u, sizeof r.u);
    }
    mxFree(inl);
}
