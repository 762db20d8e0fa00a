/*
 * ekf_ctx_gateway.c -- MEX gateway `pre3_mex(command, ...)` exposing the device-resident filter context, for
 * users who want P to stay in HBM across calls instead of crossing PCIe at every `update`
 * (the stateless update gateway moves 2 n^2 doubles per call).  The @ekf_filter methods become one-liners:
 *
 *   ekf_prediction.m:29             pre3_mex('predict', u)                      % u = [dX; dq] from fv.m:47
 *   search_IC_matches.m:31-44       pre3_mex('project', 1, 1); pre3_mex('innovation'); f = pre3_mex('fields')
 *   matching_sift_based.m:119-134   acc = pre3_mex('window_gate', k1-1, zc, 1)
 *   ransac_hypotheses.m:40-80       [li, stats] = pre3_mex('ransac', hyp-1, threshold, 1)
 *   ekf_update_li_inliers.m:57      pre3_mex('update_li')
 *   rescue_hi_inliers.m:32-47       hi = pre3_mex('rescue', 5.9915)
 *   ekf_update_hi_inliers.m:57      pre3_mex('update_hi')
 *   get_x_k_k.m / get_p_k_k.m       [x, P] = pre3_mex('get_state', 0)
 *   plots_complete.m:161-237        [xv, Pv] = pre3_mex('marginal', 0:6); s = pre3_mex('landmarks')     % without fetching P
 *   update(x_k_k, p_k_k, H, R, z, h) pre3_mex('update', H, R, z, h)             % in place on the resident estimate; R = [] for eye
 *   ekf_heading_update.m:27-52      applied = pre3_mex('heading', R_plane, 1)
 *   mono_slam.m:189-193             applied = pre3_mex('plane_heading', x_sr, y_sr, z_sr, draws, 1)   % plane_fit_to_data + ekf_heading_update on the device
 *   map_management.m:27-79          [del, acc] = pre3_mex('map_policy', step, UV, XYZ, DESC, 50, 0.1, std_z, 1)   % policy on the device; pre3_mex('set_book', B) first
 *   Weighted_Smpl_wo_replacement.m  [del, acc, cv, st, order] = pre3_mex('map_policy_seeded', step, UV, XYZ, DESC, 50, 0.1, std_z, 1, [176 144], seed, step)   % ... and its draw
 *   read_xyz_sr4000.m, read_image_sr4000.m, read_sr4000_data_dr_ye.m   [x, y, z, img, imax, cmax] = pre3_mex('sr_frame', mode, z, x, y, amp, conf)   % conf = [] for none; the frame stays resident
 *   read_xyz_sr4000.m:2-3,25-42 (load of d1_%04d.dat)                  info = pre3_mex('sr_frame_text', mode, fileread(name))                               % the text parsed on the device; the frame stays resident
 *   SIFT_extract_save.m:71-88, confidence_filtering.m                  [frm, des, idx, xyz, rho] = pre3_mex('sr_keypoints', gate, frames, descriptors)    % on the resident frame; no filter context needed
 *   sift_vedal.m:127-323, SIFT_extract_save.m:44-88                    [frames, descriptors, counts] = pre3_mex('sr_sift'); [frm, des, idx, xyz, rho] = pre3_mex('sr_gate', gate)   % the SIFT set made on the device
 *   vodometry_dr_ye.m:139-236, Calculate_V_Omega_RANSAC_dr_ye.m:41-50  pre3_mex('sr_keep'); ... next frame's 'sr_frame' + 'sr_keypoints' (gate 1) ...; [T, q, R, sta, match, stat] = pre3_mex('vo_pair', seed, seq)
 *   initialize_features.m:95-99 + map_management.m:27-79               pre3_mex('sr_keep'); ... next frame's 'sr_frame' + 'sr_keypoints' (gate 0 on both) ...; [del, acc, cv, st, order, match] = pre3_mex('map_policy_frames', step, 50, 0.1, std_z, 1, [176 144], seed, step)
 *   plane_fit_to_data.m:7-149 on the resident frame                     [R, sta, B, n_inliers] = pre3_mex('plane_frame', seed, seq)                          % the box is gathered on the device
 *   mono_slam.m:189-193 on the resident frame                           applied = pre3_mex('heading_frame', seed, step)                                  % fit + ekf_heading_update, nothing read back
 *   matching_sift_based.m:104,129-135 on the resident frame             pre3_mex('set_scan_frame')                                                       % the scan 'sr_keypoints' was handed, copied on the device
 *   fv.m:47 + ekf_prediction.m:29 on two resident frames                pre3_mex('predict_pair', seed, seq)                                              % 'vo_pair' + 'predict' in one call, u stays on the device
 *   predict_state_and_covariance.m:82,89-90,127 (fv.m:64-106, dfv_by_dxv.m, func_Q.m)   pre3_mex('predict_cv', dt, sigma_a, sigma_alpha [, type])                  % the camera-only models: no u; type 0..3 or its name
 *   predict_state_and_covariance.m:98-102 (Pn)                          [Pn, source] = pre3_mex('process_noise' [, Pn])                                  % the Pn of every prediction; [] -> the constant
 *   aux_code/calc_cov_RANSAC_dr_ye.m:17-30                              [cov, status, n] = pre3_mex('vo_cov', op_pset1, op_pset2, rot, trans [, inliers])  % cached RANSAC_RESULT contents
 *   predict_state_and_covariance.m:115 on two resident frames           [T, q, sta, pnum, cov, cst] = pre3_mex('predict_pair_cov', seed, seq)            % 'predict_pair' with the pair's covariance as Pn
 *   TestScripts/icp_with_init.m on two resident frames                  [R, t, corr, err, data2, sta] = pre3_mex('icp', res, Rinit, Tinit [, stride])      % the dense refinement of a pose; 'sr_keep' as for 'vo_pair'
 *   TestScripts/ICP_RANSAC*.m ("visually bootstrapped ICP")             [T, q, R, sta, icp_sta, err] = pre3_mex('icp_pair', seed, seq, res [, stride, thresh])   % 'vo_pair' with the ICP behind it, one wait
 *
 * The context lives in a static guarded by mexAtExit + mexLock (the convention of the reference's Coder MEX,
 * corrcoef_partitioned_mex.c:25-57).  NOT compiled in the build container (no MATLAB / mex.h there).
 */
#include <math.h>
#include <string.h>
#include "mex.h"
#include "pre3.h"

static pre3_ctx *g_ctx = NULL;
static pre3_sr_frame *g_sr = NULL;          /* the resident SR4000 frame of 'sr_frame' / 'sr_keypoints' */
static pre3_sr_frame *g_sr_prev = NULL;     /* the frame 'sr_keep' put aside: prev of 'vo_pair' */
static int g_sr_rows = 0, g_sr_cols = 0;
static int g_sr_comp_form = PRE3_SR_COMP_NONE;   /* 'sr_compensation': the setting of every frame loaded from now on, whichever handle takes it */
static double g_sr_comp_cutoff = 1.0;
static int g_cam_rows = 0, g_cam_cols = 0;  /* the camera's shape, which is the resident image's ('fast_detect' without a box) */
static void at_exit(void) { if (g_ctx) { pre3_destroy(g_ctx); g_ctx = NULL; } }
static void sr_at_exit(void) { if (g_sr) { pre3_sr_frame_destroy(g_sr); g_sr = NULL; } if (g_sr_prev) { pre3_sr_frame_destroy(g_sr_prev); g_sr_prev = NULL; } at_exit(); }
static void check(int rc) { if (rc != PRE3_OK) mexErrMsgTxt(pre3_last_error()); }

void mexFunction(int nout, mxArray *out[], int nin, const mxArray *in[])
{
    char cmd[32];
    if (nin < 1 || mxGetString(in[0], cmd, sizeof cmd)) mexErrMsgTxt("pre3_mex: first argument must be a command string");
    if (!strcmp(cmd, "create")) {            /* pre3_mex('create', cam_struct, types(0/1), 'f32'|'f64', max_hyp) */
        pre3_cam cam; int N = (int)mxGetNumberOfElements(in[2]), i; int32_t *t; char dt[8];
        const char *fn[7] = { "f", "Cx", "Cy", "k1", "k2", "nRows", "nCols" }; double *cf = &cam.f;
        for (i = 0; i < 7; ++i) { mxArray *v = mxGetField(in[1], 0, fn[i]); if (!v) mexErrMsgTxt("pre3_mex: cam field missing"); cf[i] = mxGetScalar(v); }
        mxGetString(in[3], dt, sizeof dt);
        at_exit();
        check(pre3_create(&g_ctx, 0, !strcmp(dt, "f64") ? PRE3_F64 : PRE3_F32, N, (int)mxGetScalar(in[4])));
        mexAtExit(sr_at_exit); if (!mexIsLocked()) mexLock();
        t = (int32_t *)mxMalloc(sizeof(int32_t) * (N ? N : 1));
        for (i = 0; i < N; ++i) t[i] = (int32_t)mxGetPr(in[2])[i];
        check(pre3_set_cam(g_ctx, &cam)); check(pre3_set_map(g_ctx, N, t)); mxFree(t);
        g_cam_rows = (int)cam.nRows; g_cam_cols = (int)cam.nCols;
        return;
    }
    if (!strcmp(cmd, "sr_frame")) {          /* [x, y, z, img, imax, cmax] = pre3_mex('sr_frame', mode (0: read_xyz_sr4000 / read_image_sr4000, 1: read_sr4000_data_dr_ye),
                                                 z, x, y, amp, conf ([]: none)): the planes of a .dat frame conditioned on the device; img is double 0..255 */
        int rows, cols, i; double imax = 0, cmax = 0;
        if (nin != 7) mexErrMsgTxt("pre3_mex('sr_frame', mode, z, x, y, amp, conf): six arguments");
        rows = (int)mxGetM(in[2]); cols = (int)mxGetN(in[2]);
        for (i = 3; i < 7; ++i)
            if (!(i == 6 && mxIsEmpty(in[6])) && ((int)mxGetM(in[i]) != rows || (int)mxGetN(in[i]) != cols)) mexErrMsgTxt("pre3_mex('sr_frame'): the planes must have the same size");
        if (g_sr && (rows != g_sr_rows || cols != g_sr_cols)) {
            pre3_sr_frame_destroy(g_sr); g_sr = NULL;
            if (g_sr_prev) { pre3_sr_frame_destroy(g_sr_prev); g_sr_prev = NULL; }
        }
        if (!g_sr) { check(pre3_sr_frame_create(&g_sr, 0, rows, cols)); g_sr_rows = rows; g_sr_cols = cols; mexAtExit(sr_at_exit); if (!mexIsLocked()) mexLock(); }
        check(pre3_sr_frame_set_compensation(g_sr, g_sr_comp_form, g_sr_comp_cutoff));
        check(pre3_sr_frame_load(g_sr, (int)mxGetScalar(in[1]), mxGetPr(in[2]), mxGetPr(in[3]), mxGetPr(in[4]), mxGetPr(in[5]), mxIsEmpty(in[6]) ? NULL : mxGetPr(in[6])));
        for (i = 0; i < 4; ++i) out[i] = mxCreateDoubleMatrix(rows, cols, mxREAL);
        check(pre3_sr_frame_get(g_sr, mxGetPr(out[0]), mxGetPr(out[1]), mxGetPr(out[2]), mxGetPr(out[3]), NULL, &imax, &cmax));
        out[4] = mxCreateDoubleScalar(imax); out[5] = mxCreateDoubleScalar(cmax);
        (void)nout;
        return;
    }
    if (!strcmp(cmd, "sr_frame_text")) {     /* info = pre3_mex('sr_frame_text', mode, text (char or uint8) [, rows = 144, cols = 176]): the text of a .dat frame parsed and
                                                 conditioned on the device (pre3_sr_frame_load_text); the frame stays resident as after 'sr_frame'.  info: the fields of
                                                 pre3_sr_text_info; a refused text (info.status ~= 0) leaves the resident frame as it was and is no MATLAB error */
        const char *fn[11] = { "status", "rows", "cols", "has_conf", "has_timestamp", "n_tokens", "n_undecided", "bad_row", "bad_col", "bad_offset", "timestamp" };
        pre3_sr_text_info ti; int rows, cols, rc, is_char; size_t n, i; char *buf = NULL; const char *text; double v[11];
        if (nin != 3 && nin != 5) mexErrMsgTxt("pre3_mex('sr_frame_text', mode, text [, rows, cols]): two or four arguments");
        is_char = mxIsChar(in[2]) ? 1 : 0;
        if (!is_char && mxGetClassID(in[2]) != mxUINT8_CLASS) mexErrMsgTxt("pre3_mex('sr_frame_text'): text must be a char or a uint8 array");
        rows = nin == 5 ? (int)mxGetScalar(in[3]) : 144; cols = nin == 5 ? (int)mxGetScalar(in[4]) : 176;
        if (g_sr && (rows != g_sr_rows || cols != g_sr_cols)) {
            pre3_sr_frame_destroy(g_sr); g_sr = NULL;
            if (g_sr_prev) { pre3_sr_frame_destroy(g_sr_prev); g_sr_prev = NULL; }
        }
        if (!g_sr) { check(pre3_sr_frame_create(&g_sr, 0, rows, cols)); g_sr_rows = rows; g_sr_cols = cols; mexAtExit(sr_at_exit); if (!mexIsLocked()) mexLock(); }
        check(pre3_sr_frame_set_compensation(g_sr, g_sr_comp_form, g_sr_comp_cutoff));
        n = mxGetNumberOfElements(in[2]);
        if (is_char) {                       /* MATLAB's char is 16 bits wide */
            const unsigned short *c = (const unsigned short *)mxGetData(in[2]);
            buf = (char *)mxMalloc(n ? n : 1);
            for (i = 0; i < n; ++i) buf[i] = c[i] < 256 ? (char)c[i] : '?';
            text = buf;
        } else text = (const char *)mxGetData(in[2]);
        memset(&ti, 0, sizeof ti);
        rc = pre3_sr_frame_load_text(g_sr, (int)mxGetScalar(in[1]), text, n, &ti);
        if (buf) mxFree(buf);
        if (rc != PRE3_OK && ti.status == 0) check(rc);
        v[0] = ti.status; v[1] = ti.rows; v[2] = ti.cols; v[3] = ti.has_conf; v[4] = ti.has_timestamp; v[5] = ti.n_tokens; v[6] = ti.n_undecided;
        v[7] = ti.bad_row; v[8] = ti.bad_col; v[9] = (double)ti.bad_offset; v[10] = ti.timestamp;
        out[0] = mxCreateStructMatrix(1, 1, 11, fn);
        for (i = 0; i < 11; ++i) mxSetField(out[0], 0, fn[i], mxCreateDoubleScalar(v[i]));
        (void)nout;
        return;
    }
    if (!strcmp(cmd, "sr_compensation")) {   /* [form, cutoff] = pre3_mex('sr_compensation', h, form, cutoff): the compensation in front of the Gaussian for every 'sr_frame' /
                                                 'sr_frame_text' from now on (pre3_sr_frame_set_compensation) -- form 0: none, 1: aux_code/compensate_badpixel_soonhac.m:5-14 (x, y, z
                                                 and the image replaced by their 3 x 3 symmetric median where conf < cutoff), 2: read_image_sr4000_dr_ye.m:21-24 (medfilt2 of the uint8
                                                 image).  h = 0: the setting is the gateway's, because 'sr_keep' swaps the two handles; the resident frames stay as they are.
                                                 With h alone: returns the setting */
        if (nin != 2 && nin != 4) mexErrMsgTxt("pre3_mex('sr_compensation', h [, form, cutoff]): one or three arguments");
        if ((int)mxGetScalar(in[1]) != 0) mexErrMsgTxt("pre3_mex('sr_compensation'): h must be 0 (the setting belongs to the gateway, not to one of its two frames)");
        if (nin == 4) {
            const int form = (int)mxGetScalar(in[2]); const double cutoff = mxGetScalar(in[3]);
            if (form < PRE3_SR_COMP_NONE || form > PRE3_SR_COMP_IMAGE_MEDIAN || (double)form != mxGetScalar(in[2])) mexErrMsgTxt("pre3_mex('sr_compensation'): form must be 0, 1 or 2");
            if (form == PRE3_SR_COMP_BADPIXEL && !(cutoff - cutoff == 0.0)) mexErrMsgTxt("pre3_mex('sr_compensation'): the cut-off of form 1 must be finite");
            if (g_sr) check(pre3_sr_frame_set_compensation(g_sr, form, cutoff));
            if (g_sr_prev) check(pre3_sr_frame_set_compensation(g_sr_prev, form, cutoff));
            g_sr_comp_form = form; g_sr_comp_cutoff = cutoff;
        }
        out[0] = mxCreateDoubleScalar((double)g_sr_comp_form);
        if (nout > 1) out[1] = mxCreateDoubleScalar(g_sr_comp_cutoff);
        return;
    }
    if (!strcmp(cmd, "sr_bad_pixels")) {     /* [n_bad, form_of_frame] = pre3_mex('sr_bad_pixels', h): how many pixels of the frame were compensated and the form it was conditioned
                                                 with (pre3_sr_frame_bad_pixels).  h = 0: the resident frame, 1: the frame 'sr_keep' put aside */
        int32_t form = 0, n_bad = 0; int h;
        if (nin != 2) mexErrMsgTxt("pre3_mex('sr_bad_pixels', h): one argument");
        h = (int)mxGetScalar(in[1]);
        if (h != 0 && h != 1) mexErrMsgTxt("pre3_mex('sr_bad_pixels'): h must be 0 (the resident frame) or 1 (the frame 'sr_keep' put aside)");
        if (!(h ? g_sr_prev : g_sr)) mexErrMsgTxt("pre3_mex('sr_bad_pixels'): there is no such frame yet");
        check(pre3_sr_frame_bad_pixels(h ? g_sr_prev : g_sr, &form, &n_bad));
        out[0] = mxCreateDoubleScalar((double)n_bad);
        if (nout > 1) out[1] = mxCreateDoubleScalar((double)form);
        return;
    }
    if (!strcmp(cmd, "medfilt3")) {          /* B = pre3_mex('medfilt3', A, padding): medfilt2(A, [3 3]) (padding 0, zeros: MATLAB's default) or medfilt2(A, [3 3], 'symmetric')
                                                 (padding 1) of a double matrix on the device (pre3_sr_medfilt3); a NaN in a window makes that pixel NaN */
        if (nin != 3) mexErrMsgTxt("pre3_mex('medfilt3', A, padding): two arguments");
        if (!mxIsDouble(in[1]) || mxIsComplex(in[1]) || mxGetNumberOfDimensions(in[1]) != 2 || mxIsEmpty(in[1])) mexErrMsgTxt("pre3_mex('medfilt3'): A must be a real, non-empty double matrix");
        out[0] = mxCreateDoubleMatrix(mxGetM(in[1]), mxGetN(in[1]), mxREAL);
        check(pre3_sr_medfilt3(0, (int)mxGetM(in[1]), (int)mxGetN(in[1]), mxGetPr(in[1]), (int)mxGetScalar(in[2]), mxGetPr(out[0])));
        (void)nout;
        return;
    }
    if (!strcmp(cmd, "sr_keypoints")) {      /* [frm, des, idx (1-based), xyz, rho] = pre3_mex('sr_keypoints', gate (0: SIFT_extract_save.m:71-88 over inittialize_depth_my_version.m,
                                                 1: confidence_filtering.m), frames (ldf x K, rows 1:2 = pixel column, row, 1-based), descriptors (ND x K or [])) */
        int ldf, K, ND, gate, i; int32_t n = 0, *idx; double *f2, *d2, *xyz, *rho;
        if (nin != 4) mexErrMsgTxt("pre3_mex('sr_keypoints', gate, frames, descriptors): three arguments");
        if (!g_sr) mexErrMsgTxt("pre3_mex('sr_keypoints'): call pre3_mex('sr_frame', ...) first");
        gate = (int)mxGetScalar(in[1]); ldf = (int)mxGetM(in[2]); K = (int)mxGetN(in[2]); ND = mxIsEmpty(in[3]) ? 0 : (int)mxGetM(in[3]);
        if (ND > 0 && (int)mxGetN(in[3]) != K) mexErrMsgTxt("pre3_mex('sr_keypoints'): descriptors must be ND x K");
        idx = (int32_t *)mxMalloc(sizeof(int32_t) * (K ? K : 1));
        f2 = (double *)mxMalloc(sizeof(double) * (size_t)(K ? K : 1) * (ldf ? ldf : 1)); d2 = (double *)mxMalloc(sizeof(double) * (size_t)(K ? K : 1) * (ND ? ND : 1));
        xyz = (double *)mxMalloc(sizeof(double) * 3 * (K ? K : 1)); rho = (double *)mxMalloc(sizeof(double) * (K ? K : 1));
        check(pre3_sr_frame_keypoints(g_sr, gate, ldf, K, mxGetPr(in[2]), ND, ND ? mxGetPr(in[3]) : NULL, &n, idx, f2, d2, xyz, rho));
        out[0] = mxCreateDoubleMatrix(ldf, n, mxREAL); memcpy(mxGetPr(out[0]), f2, sizeof(double) * (size_t)n * ldf);
        out[1] = mxCreateDoubleMatrix(ND, n, mxREAL); memcpy(mxGetPr(out[1]), d2, sizeof(double) * (size_t)n * ND);
        out[2] = mxCreateDoubleMatrix(1, n, mxREAL); for (i = 0; i < n; ++i) mxGetPr(out[2])[i] = idx[i] + 1;
        out[3] = mxCreateDoubleMatrix(3, gate == 0 ? n : 0, mxREAL); out[4] = mxCreateDoubleMatrix(1, gate == 0 ? n : 0, mxREAL);
        if (gate == 0) { memcpy(mxGetPr(out[3]), xyz, sizeof(double) * 3 * (size_t)n); memcpy(mxGetPr(out[4]), rho, sizeof(double) * (size_t)n); }
        mxFree(idx); mxFree(f2); mxFree(d2); mxFree(xyz); mxFree(rho);
        (void)nout;
        return;
    }
    if (!strcmp(cmd, "sr_sift")) {           /* [frames, descriptors, counts] = pre3_mex('sr_sift' [, strict_reference = 1 [, one_based = 1]]): sift_vedal.m:127-323 on the
                                                 resident frame's own image, made on the device; the set stays in the handle as the raw set (1-based, SIFT_extract_save.m:55-56).
                                                 frames 4 x K (one_based = 0: sift_vedal's own 0-based x, y), descriptors 128 x K, counts 4 x O (maxima, inside the boundary,
                                                 refined, oriented per octave) */
        int32_t K = 0, counts[4 * 32], O = 0; int i; double *f2, *d2;
        if (nin > 3) mexErrMsgTxt("pre3_mex('sr_sift' [, strict_reference [, one_based]]): at most two arguments");
        if (!g_sr) mexErrMsgTxt("pre3_mex('sr_sift'): call pre3_mex('sr_frame', ...) first");
        f2 = (double *)mxMalloc(sizeof(double) * 4 * PRE3_SR_MAX_KEYPOINTS); d2 = (double *)mxMalloc(sizeof(double) * 128 * (size_t)PRE3_SR_MAX_KEYPOINTS);
        check(pre3_sift_plan_get(g_sr_rows, g_sr_cols, &O, NULL, NULL, NULL, NULL, NULL, NULL, NULL));
        check(pre3_sr_frame_sift(g_sr, NULL, nin > 1 ? (int)mxGetScalar(in[1]) : 1, nin > 2 ? (int)mxGetScalar(in[2]) : 1, &K, f2, d2, counts));
        out[0] = mxCreateDoubleMatrix(4, K, mxREAL); memcpy(mxGetPr(out[0]), f2, sizeof(double) * 4 * (size_t)K);
        out[1] = mxCreateDoubleMatrix(128, K, mxREAL); memcpy(mxGetPr(out[1]), d2, sizeof(double) * 128 * (size_t)K);
        out[2] = mxCreateDoubleMatrix(4, O, mxREAL); for (i = 0; i < 4 * O; ++i) mxGetPr(out[2])[i] = counts[i];
        mxFree(f2); mxFree(d2);
        (void)nout;
        return;
    }
    if (!strcmp(cmd, "sr_gate")) {           /* [frm, des, idx (1-based), xyz, rho] = pre3_mex('sr_gate', gate): 'sr_keypoints'' gate over the raw set already in the handle
                                                 ('sr_sift''s, or a 'sr_keypoints' upload of 4 x K frames and 128 x K descriptors: the library refuses any other shape), nothing uploaded */
        int gate, i; int32_t n = 0, *idx; double *f2, *d2, *xyz, *rho; const size_t cap = PRE3_SR_MAX_KEYPOINTS;
        if (nin != 2) mexErrMsgTxt("pre3_mex('sr_gate', gate): one argument");
        if (!g_sr) mexErrMsgTxt("pre3_mex('sr_gate'): call pre3_mex('sr_frame', ...) and pre3_mex('sr_sift') first");
        gate = (int)mxGetScalar(in[1]);
        idx = (int32_t *)mxMalloc(sizeof(int32_t) * cap); f2 = (double *)mxMalloc(sizeof(double) * 4 * cap); d2 = (double *)mxMalloc(sizeof(double) * 128 * cap);
        xyz = (double *)mxMalloc(sizeof(double) * 3 * cap); rho = (double *)mxMalloc(sizeof(double) * cap);
        check(pre3_sr_frame_gate(g_sr, gate, &n, idx, f2, d2, xyz, rho));
        out[0] = mxCreateDoubleMatrix(4, n, mxREAL); memcpy(mxGetPr(out[0]), f2, sizeof(double) * 4 * (size_t)n);
        out[1] = mxCreateDoubleMatrix(128, n, mxREAL); memcpy(mxGetPr(out[1]), d2, sizeof(double) * 128 * (size_t)n);
        out[2] = mxCreateDoubleMatrix(1, n, mxREAL); for (i = 0; i < n; ++i) mxGetPr(out[2])[i] = idx[i] + 1;
        out[3] = mxCreateDoubleMatrix(3, gate == 0 ? n : 0, mxREAL); out[4] = mxCreateDoubleMatrix(1, gate == 0 ? n : 0, mxREAL);
        if (gate == 0) { memcpy(mxGetPr(out[3]), xyz, sizeof(double) * 3 * (size_t)n); memcpy(mxGetPr(out[4]), rho, sizeof(double) * (size_t)n); }
        mxFree(idx); mxFree(f2); mxFree(d2); mxFree(xyz); mxFree(rho);
        (void)nout;
        return;
    }
    if (!strcmp(cmd, "sr_keep")) {           /* pre3_mex('sr_keep'): the resident frame, with its last 'sr_keypoints' result, becomes the previous frame of 'vo_pair';
                                                 the next 'sr_frame' loads into the other handle */
        pre3_sr_frame *t = g_sr_prev;
        if (!g_sr) mexErrMsgTxt("pre3_mex('sr_keep'): call pre3_mex('sr_frame', ...) first");
        g_sr_prev = g_sr; g_sr = t;
        (void)nout;
        return;
    }
    if (!strcmp(cmd, "vo_pair")) {           /* [T, q, R, sta, match, stat] = pre3_mex('vo_pair', seed, seq [, thresh = 1.5]): vodometry_dr_ye.m:139-236 between the frame
                                                 'sr_keep' put aside and the resident one, each with its 'sr_keypoints' (gate 1) result; seed, seq: whole numbers up to 2^53.
                                                 T 3 x 1, q = R2q(R) 4 x 1 and R 3 x 3 are the identity motion unless sta == 1 (Calculate_V_Omega_RANSAC_dr_ye.m:41-50);
                                                 match 2 x pnum (1-based positions in the kept sets); stat = [nIterationRansac nSupport ErrorMean ErrorStd phi theta psi pnum capped] */
        pre3_vo_result r; int32_t pnum = 0, capped = 0; int i, k; mwSize n1; double *mt, *m;
        if (nin < 3 || nin > 4) mexErrMsgTxt("pre3_mex('vo_pair', seed, seq [, thresh]): two or three arguments");
        if (!g_sr || !g_sr_prev) mexErrMsgTxt("pre3_mex('vo_pair'): needs two frames -- 'sr_frame' + 'sr_keypoints', 'sr_keep', then 'sr_frame' + 'sr_keypoints' again");
        n1 = (mwSize)PRE3_SR_MAX_KEYPOINTS;
        mt = (double *)mxMalloc(sizeof(double) * 2 * n1);
        check(pre3_vo_pair_seeded(g_sr_prev, g_sr, nin > 3 ? mxGetScalar(in[3]) : 1.5, (uint64_t)mxGetScalar(in[1]), (uint64_t)mxGetScalar(in[2]), &pnum, mt,
                                  NULL, NULL, NULL, &capped, NULL, NULL, NULL, &r));
        out[0] = mxCreateDoubleMatrix(3, 1, mxREAL); memcpy(mxGetPr(out[0]), r.u, sizeof(double) * 3);
        if (nout > 1) { out[1] = mxCreateDoubleMatrix(4, 1, mxREAL); memcpy(mxGetPr(out[1]), r.u + 3, sizeof(double) * 4); }
        if (nout > 2) {
            out[2] = mxCreateDoubleMatrix(3, 3, mxREAL);
            for (i = 0; i < 3; ++i) for (k = 0; k < 3; ++k) mxGetPr(out[2])[i + 3 * k] = r.sta == 1 ? r.rot[3 * i + k] : (i == k ? 1.0 : 0.0);      /* row-major -> column-major */
        }
        if (nout > 3) out[3] = mxCreateDoubleScalar(r.sta);
        if (nout > 4) { out[4] = mxCreateDoubleMatrix(2, pnum, mxREAL); memcpy(mxGetPr(out[4]), mt, sizeof(double) * 2 * (size_t)pnum); }
        if (nout > 5) {
            out[5] = mxCreateDoubleMatrix(1, 9, mxREAL); m = mxGetPr(out[5]);
            m[0] = r.n_iterations; m[1] = r.n_support; m[2] = r.error_mean; m[3] = r.error_std; memcpy(m + 4, r.euler, sizeof r.euler); m[7] = pnum; m[8] = capped;
        }
        mxFree(mt);
        return;
    }
    if (!strcmp(cmd, "icp") || !strcmp(cmd, "icp_pair")) {
        /* [R, t, corr, err, data2, sta] = pre3_mex('icp', res, Rinit, Tinit [, stride = 1]): icp_with_init.m:34-120 between the frame 'sr_keep' put aside (the model: every
           pixel as [-x; -y; z]) and the resident one (the source: rows and columns 1, 1 + stride, ...), seeded with Rinit 3 x 3, Tinit 3 x 1.  R, t the accumulated
           registration of the seeded source, corr p x 3 = [model source D] (1-based positions in the kept pixel lists), data2 3 x n2 registered, sta 1 / 2.
           [T, q, R, sta, icp_sta, err] = pre3_mex('icp_pair', seed, seq, res [, stride = 1, thresh = 1.5]): 'vo_pair' with that ICP queued behind it on the device, seeded
           with the pair's own R, T; T, q, R are the refined total when icp_sta >= 1, else the pair's as 'vo_pair' returns them (icp_sta = 0: the pair's sta ~= 1). */
        const int pair = !strcmp(cmd, "icp_pair");
        pre3_icp_result ir; pre3_vo_result vr; int32_t pnum = 0; int i, k, stride; mwSize ncand; double Ri[9], *corr, *d2;
        if (!g_sr || !g_sr_prev) mexErrMsgTxt("pre3_mex('icp' / 'icp_pair'): needs two frames -- 'sr_frame', 'sr_keep', then 'sr_frame' again");
        if (pair ? (nin < 4 || nin > 6) : (nin < 4 || nin > 5)) mexErrMsgTxt("pre3_mex('icp', res, Rinit, Tinit [, stride]) or pre3_mex('icp_pair', seed, seq, res [, stride, thresh])");
        stride = nin > 4 ? (int)mxGetScalar(in[4]) : 1;
        if (stride < 1) mexErrMsgTxt("pre3_mex('icp' / 'icp_pair'): stride must be at least 1");
        ncand = (mwSize)((g_sr_rows + stride - 1) / stride) * (mwSize)((g_sr_cols + stride - 1) / stride);
        memset(&ir, 0, sizeof ir);
        if (pair) {
            check(pre3_icp_pair_seeded(g_sr_prev, g_sr, nin > 5 ? mxGetScalar(in[5]) : 1.5, (uint64_t)mxGetScalar(in[1]), (uint64_t)mxGetScalar(in[2]), stride, mxGetScalar(in[3]),
                                       &pnum, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, &vr, &ir, NULL, NULL, NULL, NULL));
            {
                const int refined = ir.sta >= 1;
                const double *u = refined ? ir.u : vr.u, *rot = refined ? ir.Rtot : vr.rot;
                out[0] = mxCreateDoubleMatrix(3, 1, mxREAL); memcpy(mxGetPr(out[0]), u, sizeof(double) * 3);
                if (nout > 1) { out[1] = mxCreateDoubleMatrix(4, 1, mxREAL); memcpy(mxGetPr(out[1]), u + 3, sizeof(double) * 4); }
                if (nout > 2) {
                    out[2] = mxCreateDoubleMatrix(3, 3, mxREAL);
                    for (i = 0; i < 3; ++i) for (k = 0; k < 3; ++k) mxGetPr(out[2])[i + 3 * k] = (refined || vr.sta == 1) ? rot[3 * i + k] : (i == k ? 1.0 : 0.0);
                }
                if (nout > 3) out[3] = mxCreateDoubleScalar(vr.sta);
                if (nout > 4) out[4] = mxCreateDoubleScalar(ir.sta);
                if (nout > 5) out[5] = mxCreateDoubleScalar(refined ? ir.error : 0.0);
            }
            return;
        }
        if (mxGetNumberOfElements(in[2]) != 9 || mxGetNumberOfElements(in[3]) != 3) mexErrMsgTxt("pre3_mex('icp'): Rinit is 3 x 3, Tinit 3 x 1");
        for (i = 0; i < 3; ++i) for (k = 0; k < 3; ++k) Ri[3 * i + k] = mxGetPr(in[2])[i + 3 * k];      /* column-major -> row-major */
        corr = (double *)mxMalloc(sizeof(double) * 3 * ncand); d2 = (double *)mxMalloc(sizeof(double) * 3 * ncand);
        check(pre3_icp_frames(g_sr_prev, g_sr, stride, mxGetScalar(in[1]), Ri, mxGetPr(in[3]), &ir, corr, NULL, d2, NULL));
        out[0] = mxCreateDoubleMatrix(3, 3, mxREAL);
        for (i = 0; i < 3; ++i) for (k = 0; k < 3; ++k) mxGetPr(out[0])[i + 3 * k] = ir.R[3 * i + k];
        if (nout > 1) { out[1] = mxCreateDoubleMatrix(3, 1, mxREAL); memcpy(mxGetPr(out[1]), ir.t, sizeof ir.t); }
        if (nout > 2) {
            out[2] = mxCreateDoubleMatrix(ir.p, 3, mxREAL);
            for (i = 0; i < ir.p; ++i) for (k = 0; k < 3; ++k) mxGetPr(out[2])[i + (size_t)ir.p * k] = corr[3 * i + k];
        }
        if (nout > 3) out[3] = mxCreateDoubleScalar(ir.error);
        if (nout > 4) { out[4] = mxCreateDoubleMatrix(3, ir.n_source, mxREAL); memcpy(mxGetPr(out[4]), d2, sizeof(double) * 3 * (size_t)ir.n_source); }
        if (nout > 5) out[5] = mxCreateDoubleScalar(ir.sta);
        mxFree(corr); mxFree(d2);
        return;
    }
    if (!strcmp(cmd, "plane_frame")) {       /* [R, sta, B, n_inliers] = pre3_mex('plane_frame', seed, seq [, n_draw = 1001, box = [80 144 50 120], t = 0.02]): plane_fit_to_data.m:7-149 on
                                                 the resident frame's filtered x, y, z (load it with mode 0: read_xyz_sr4000) -- the box is gathered on the device, ransac.m:142-176's draws
                                                 come from (seed, seq), nothing is read back to be sent again (pre3_plane_fit_frame_seeded).  R 3 x 3 as plane_fit_to_data returns it.
                                                 A non-finite coordinate inside the box is an error (sta = 5). */
        pre3_plane_result r; int32_t bx[4]; int i;
        if (nin < 3 || nin > 6) mexErrMsgTxt("pre3_mex('plane_frame', seed, seq [, n_draw, box, t]): two to five arguments");
        if (!g_sr) mexErrMsgTxt("pre3_mex('plane_frame'): call pre3_mex('sr_frame', ...) first");
        if (nin > 4 && mxGetNumberOfElements(in[4]) != 4) mexErrMsgTxt("pre3_mex('plane_frame'): box is [row0 row1 col0 col1]");
        for (i = 0; nin > 4 && i < 4; ++i) bx[i] = (int32_t)mxGetPr(in[4])[i];
        check(pre3_plane_fit_frame_seeded(g_sr, nin > 4 ? bx : NULL, nin > 5 ? mxGetScalar(in[5]) : 0.02, nin > 3 ? (int)mxGetScalar(in[3]) : PRE3_PLANE_MAX_DRAWS,
                                          (uint64_t)mxGetScalar(in[1]), (uint64_t)mxGetScalar(in[2]), NULL, NULL, NULL, &r));
        out[0] = mxCreateDoubleMatrix(3, 3, mxREAL); memcpy(mxGetPr(out[0]), r.R, sizeof r.R);
        if (nout > 1) out[1] = mxCreateDoubleScalar(r.sta);
        if (nout > 2) { out[2] = mxCreateDoubleMatrix(4, 1, mxREAL); memcpy(mxGetPr(out[2]), r.B, sizeof r.B); }
        if (nout > 3) out[3] = mxCreateDoubleScalar(r.n_inliers);
        return;
    }
    if (!g_ctx) mexErrMsgTxt("pre3_mex: call pre3_mex('create', ...) first");
    if (!strcmp(cmd, "set_state")) check(pre3_set_state(g_ctx, (int)mxGetScalar(in[1]), (int)mxGetNumberOfElements(in[2]), mxGetPr(in[2]), mxGetPr(in[3])));
    else if (!strcmp(cmd, "get_state")) {
        int n = pre3_state_size(g_ctx);
        out[0] = mxCreateDoubleMatrix(n, 1, mxREAL);
        if (nout > 1) out[1] = mxCreateDoubleMatrix(n, n, mxREAL);
        check(pre3_get_state(g_ctx, (int)mxGetScalar(in[1]), n, mxGetPr(out[0]), nout > 1 ? mxGetPr(out[1]) : NULL));
    }
    else if (!strcmp(cmd, "predict")) check(pre3_predict(g_ctx, mxGetPr(in[1])));
    else if (!strcmp(cmd, "predict_cv")) {        /* pre3_mex('predict_cv', dt, sigma_a, sigma_alpha [, type = 'constant_velocity']): the prediction with the camera-only models the fork
                                                     switched off (pre3_predict_cv): fv.m:64-87 / :98-106, dfv_by_dxv.m:38-116, func_Q.m:41-54.  type: 0..3 or 'constant_velocity',
                                                     'constant_orientation', 'constant_position', 'constant_position_and_orientation' */
        static const char *names[4] = { "constant_velocity", "constant_orientation", "constant_position", "constant_position_and_orientation" };
        int type = PRE3_CV_CONSTANT_VELOCITY;
        if (nin < 4 || nin > 5) mexErrMsgTxt("pre3_mex('predict_cv', dt, sigma_a, sigma_alpha [, type]): three or four arguments");
        if (nin > 4 && mxIsChar(in[4])) {
            char name[64]; int t;
            if (mxGetString(in[4], name, sizeof name)) mexErrMsgTxt("pre3_mex('predict_cv'): type name too long");
            for (t = 0, type = -1; t < 4; ++t) if (!strcmp(name, names[t])) type = t;
            if (type < 0) mexErrMsgTxt("pre3_mex('predict_cv'): unknown type (constant_position_and_orientation_location_noise is not built)");
        } else if (nin > 4) type = (int)mxGetScalar(in[4]);
        check(pre3_predict_cv(g_ctx, type, mxGetScalar(in[1]), mxGetScalar(in[2]), mxGetScalar(in[3])));
    }
    else if (!strcmp(cmd, "project")) check(pre3_project(g_ctx, (int)mxGetScalar(in[1]), (int)mxGetScalar(in[2])));
    else if (!strcmp(cmd, "innovation")) check(pre3_innovation(g_ctx));
    else if (!strcmp(cmd, "update_li")) check(pre3_update_li(g_ctx));
    else if (!strcmp(cmd, "update_hi")) check(pre3_update_hi(g_ctx));
    else if (!strcmp(cmd, "update_all")) check(pre3_update_all(g_ctx));
    else if (!strcmp(cmd, "fields")) {            /* f = pre3_mex('fields'): struct with h (2xN), has_h (1xN), S (2x2xN), Hc (7x2xN), Hl (6x2xN) */
        const char *fn[5] = { "h", "has_h", "S", "Hc", "Hl" };
        int N = (pre3_state_size(g_ctx) - 13) / 3 + 1, i;   /* upper bound on N; exact N is the length of has_h returned */
        mwSize d3[3];
        mxArray *h, *hh, *S, *Hc, *Hl; int32_t *tmp;
        /* the landmark count is what pre3_set_map received; callers pass it as the 2nd argument */
        if (nin > 1) N = (int)mxGetScalar(in[1]);
        h = mxCreateDoubleMatrix(2, N, mxREAL); hh = mxCreateDoubleMatrix(1, N, mxREAL);
        d3[0] = 2; d3[1] = 2; d3[2] = N; S = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL);
        d3[0] = 7; Hc = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL);      /* row-major 2x7 == column-major 7x2 */
        d3[0] = 6; Hl = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL);
        tmp = (int32_t *)mxMalloc(sizeof(int32_t) * (N ? N : 1));
        check(pre3_get_landmark_fields(g_ctx, mxGetPr(h), tmp, mxGetPr(Hc), mxGetPr(Hl), mxGetPr(S)));
        for (i = 0; i < N; ++i) mxGetPr(hh)[i] = tmp[i];
        mxFree(tmp);
        out[0] = mxCreateStructMatrix(1, 1, 5, fn);
        mxSetField(out[0], 0, "h", h); mxSetField(out[0], 0, "has_h", hh); mxSetField(out[0], 0, "S", S);
        mxSetField(out[0], 0, "Hc", Hc); mxSetField(out[0], 0, "Hl", Hl);
    }
    else if (!strcmp(cmd, "window_gate")) {       /* acc = pre3_mex('window_gate', k1 (0-based), zc (2xM), strict) */
        int M = (int)mxGetNumberOfElements(in[1]), i; int32_t *k1 = (int32_t *)mxMalloc(sizeof(int32_t) * (M ? M : 1)), *acc = (int32_t *)mxMalloc(sizeof(int32_t) * (M ? M : 1));
        int rc;
        for (i = 0; i < M; ++i) k1[i] = (int32_t)mxGetPr(in[1])[i];
        rc = pre3_window_gate(g_ctx, M, k1, mxGetPr(in[2]), (int)mxGetScalar(in[3]), acc);
        out[0] = mxCreateDoubleMatrix(1, M, mxREAL);
        for (i = 0; i < M; ++i) mxGetPr(out[0])[i] = acc[i];
        mxFree(k1); mxFree(acc); check(rc);
    }
    else if (!strcmp(cmd, "set_measurements")) {  /* pre3_mex('set_measurements', idx (0-based, ascending), z (2xm)) */
        int m = (int)mxGetNumberOfElements(in[1]), i, rc; int32_t *idx = (int32_t *)mxMalloc(sizeof(int32_t) * (m ? m : 1));
        for (i = 0; i < m; ++i) idx[i] = (int32_t)mxGetPr(in[1])[i];
        rc = pre3_set_measurements(g_ctx, m, idx, mxGetPr(in[2])); mxFree(idx); check(rc);
    }
    else if (!strcmp(cmd, "ransac")) {            /* [li_mask, stats] = pre3_mex('ransac', hyp (n_draw x k, 0-based positions), thr, early_exit) */
        int n_draw = (int)mxGetM(in[1]), k = (int)mxGetN(in[1]), i, j, rc, m;
        int32_t *hyp = (int32_t *)mxMalloc(sizeof(int32_t) * n_draw * k), st[4], *li;
        for (i = 0; i < n_draw; ++i) for (j = 0; j < k; ++j) hyp[i * k + j] = (int32_t)mxGetPr(in[1])[(size_t)j * n_draw + i];
        m = nin > 4 ? (int)mxGetScalar(in[4]) : 4096;               /* number of measurements (size of li_mask) */
        li = (int32_t *)mxCalloc(m, sizeof(int32_t));
        rc = pre3_ransac(g_ctx, n_draw, k, hyp, mxGetScalar(in[2]), (int)mxGetScalar(in[3]), NULL, li, st);
        out[0] = mxCreateDoubleMatrix(1, m, mxREAL);
        for (i = 0; i < m; ++i) mxGetPr(out[0])[i] = li[i];
        if (nout > 1) { out[1] = mxCreateDoubleMatrix(1, 4, mxREAL); for (i = 0; i < 4; ++i) mxGetPr(out[1])[i] = st[i]; }
        mxFree(hyp); mxFree(li); check(rc);
    }
    else if (!strcmp(cmd, "step_predicted")) {    /* stats = pre3_mex('step_predicted', hyp (n_draw x k, 0-based positions), thr, early_exit, chi2): mono_slam.m:178-187 in one call,
                                                     behind pre3_mex('predict', u) and pre3_mex('ic_search', ...) (or 'set_measurements'); stats = [best iters n_hyp max_support n_li n_hi] */
        int n_draw = (int)mxGetM(in[1]), k = (int)mxGetN(in[1]), i, j, rc;
        int32_t *hyp = (int32_t *)mxMalloc(sizeof(int32_t) * n_draw * k), st[8];
        for (i = 0; i < n_draw; ++i) for (j = 0; j < k; ++j) hyp[i * k + j] = (int32_t)mxGetPr(in[1])[(size_t)j * n_draw + i];
        rc = pre3_step_predicted(g_ctx, n_draw, k, hyp, mxGetScalar(in[2]), (int)mxGetScalar(in[3]), nin > 4 ? mxGetScalar(in[4]) : 5.9915, st);
        out[0] = mxCreateDoubleMatrix(1, 6, mxREAL);
        for (i = 0; i < 6; ++i) mxGetPr(out[0])[i] = st[i];
        mxFree(hyp); check(rc);
    }
    else if (!strcmp(cmd, "ransac_seeded")) {     /* [li_mask, stats, hyp] = pre3_mex('ransac_seeded', seed, seq, n_draw, thr, early_exit [, m]): 'ransac' with the table drawn
                                                     on the device from (seed, seq) (pre3_ransac_seeded; select_random_match.m:40-51); hyp n_draw x k, 0-based.  seed and
                                                     seq are doubles: whole numbers up to 2^53 */
        int n_draw = (int)mxGetScalar(in[3]), i, j, rc, m;
        int32_t st[4], *li, *hyp, k = 0;
        if (nin < 6) mexErrMsgTxt("pre3_mex('ransac_seeded', seed, seq, n_draw, thr, early_exit [, m])");
        m = nin > 6 ? (int)mxGetScalar(in[6]) : 4096;
        li = (int32_t *)mxCalloc(m, sizeof(int32_t));
        hyp = (int32_t *)mxCalloc(3 * (size_t)(n_draw > 0 ? n_draw : 1), sizeof(int32_t));
        rc = pre3_ransac_seeded(g_ctx, (uint64_t)mxGetScalar(in[1]), (uint64_t)mxGetScalar(in[2]), n_draw, mxGetScalar(in[4]), (int)mxGetScalar(in[5]),
                                nout > 2 ? hyp : NULL, &k, NULL, li, st);
        out[0] = mxCreateDoubleMatrix(1, m, mxREAL);
        for (i = 0; i < m; ++i) mxGetPr(out[0])[i] = li[i];
        if (nout > 1) { out[1] = mxCreateDoubleMatrix(1, 4, mxREAL); for (i = 0; i < 4; ++i) mxGetPr(out[1])[i] = st[i]; }
        if (nout > 2 && rc == PRE3_OK) {
            out[2] = mxCreateDoubleMatrix(n_draw, k, mxREAL);
            for (i = 0; i < n_draw; ++i) for (j = 0; j < k; ++j) mxGetPr(out[2])[(size_t)j * n_draw + i] = hyp[i * k + j];
        }
        mxFree(hyp); mxFree(li); check(rc);
    }
    else if (!strcmp(cmd, "step_predicted_seeded")) {   /* stats = pre3_mex('step_predicted_seeded', seed, seq, n_draw, thr, early_exit [, chi2]): 'step_predicted' with the table
                                                           drawn on the device (pre3_step_predicted_seeded) */
        int32_t st[8];
        int i, rc;
        if (nin < 6) mexErrMsgTxt("pre3_mex('step_predicted_seeded', seed, seq, n_draw, thr, early_exit [, chi2])");
        rc = pre3_step_predicted_seeded(g_ctx, (uint64_t)mxGetScalar(in[1]), (uint64_t)mxGetScalar(in[2]), (int)mxGetScalar(in[3]), mxGetScalar(in[4]),
                                        (int)mxGetScalar(in[5]), nin > 6 ? mxGetScalar(in[6]) : 5.9915, NULL, NULL, st);
        check(rc);
        out[0] = mxCreateDoubleMatrix(1, 6, mxREAL);
        for (i = 0; i < 6; ++i) mxGetPr(out[0])[i] = st[i];
    }
    else if (!strcmp(cmd, "rescue")) {            /* hi_mask = pre3_mex('rescue', chi2, m) */
        int m = nin > 2 ? (int)mxGetScalar(in[2]) : 4096, i, rc; int32_t *hi = (int32_t *)mxCalloc(m, sizeof(int32_t));
        rc = pre3_rescue(g_ctx, mxGetScalar(in[1]), hi);
        out[0] = mxCreateDoubleMatrix(1, m, mxREAL);
        for (i = 0; i < m; ++i) mxGetPr(out[0])[i] = hi[i];
        mxFree(hi); check(rc);
    }
    else if (!strcmp(cmd, "landmarks")) {         /* s = pre3_mex('landmarks' [, which, first, count]): struct with xyz (3xN), P_xyz (3x3xN), P_native (6x6xN), linearity (1xN)
                                                     plots_complete.m:208-237 / inversedepth_2_cartesian.m:36-62 without get_p_k_k (pre3_get_landmarks) */
        const char *fn[4] = { "xyz", "P_xyz", "P_native", "linearity" };
        int which = nin > 1 ? (int)mxGetScalar(in[1]) : PRE3_X_K_K, first = nin > 2 ? (int)mxGetScalar(in[2]) : 0, count;
        mwSize d3[3];
        mxArray *xyz, *Pxyz, *Pnat, *lin;
        count = nin > 3 ? (int)mxGetScalar(in[3]) : pre3_get_map(g_ctx, NULL) - first;
        if (count < 0) count = 0;
        xyz = mxCreateDoubleMatrix(3, count, mxREAL); lin = mxCreateDoubleMatrix(1, count, mxREAL);
        d3[0] = 3; d3[1] = 3; d3[2] = count; Pxyz = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL);      /* symmetric: row-major == column-major */
        d3[0] = 6; d3[1] = 6; Pnat = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL);
        check(pre3_get_landmarks(g_ctx, which, first, count, mxGetPr(xyz), mxGetPr(Pxyz), mxGetPr(Pnat), mxGetPr(lin)));
        out[0] = mxCreateStructMatrix(1, 1, 4, fn);
        mxSetField(out[0], 0, "xyz", xyz); mxSetField(out[0], 0, "P_xyz", Pxyz); mxSetField(out[0], 0, "P_native", Pnat); mxSetField(out[0], 0, "linearity", lin);
    }
    else if (!strcmp(cmd, "marginal")) {          /* [x, P] = pre3_mex('marginal', idx (0-based, any order, repeats allowed) [, which]): x(idx+1), P(idx+1, idx+1) (pre3_get_marginal) */
        int k = (int)mxGetNumberOfElements(in[1]), i, j, rc, which = nin > 2 ? (int)mxGetScalar(in[2]) : PRE3_X_K_K;
        int32_t *d = (int32_t *)mxMalloc(sizeof(int32_t) * (k ? k : 1));
        double *Prm = (double *)mxMalloc(sizeof(double) * (k ? (size_t)k * k : 1));
        for (i = 0; i < k; ++i) d[i] = (int32_t)mxGetPr(in[1])[i];
        out[0] = mxCreateDoubleMatrix(k, 1, mxREAL);
        rc = pre3_get_marginal(g_ctx, which, k, d, mxGetPr(out[0]), Prm);
        mxFree(d);
        if (rc != PRE3_OK) { mxFree(Prm); check(rc); }
        if (nout > 1) {
            out[1] = mxCreateDoubleMatrix(k, k, mxREAL);
            for (i = 0; i < k; ++i) for (j = 0; j < k; ++j) mxGetPr(out[1])[(size_t)j * k + i] = Prm[(size_t)i * k + j];      /* row-major -> column-major */
        }
        mxFree(Prm);
    }
    else if (!strcmp(cmd, "update")) {            /* pre3_mex('update', H (full or sparse, r x n, <= 16 non-zeros per row), R (r x r, [] = eye), z, h): update.m:27-56 IN PLACE
                                                     on (x_k_k, p_k_k) (pre3_update_rows) */
        int r = (int)mxGetNumberOfElements(in[3]), n = pre3_state_size(g_ctx), a, i, j, rc;
        int32_t *nnz, *col;
        double *val, *Rrow = NULL;
        if (nin != 5) mexErrMsgTxt("pre3_mex('update', H, R, z, h): four arguments");
        if ((int)mxGetNumberOfElements(in[4]) != r) mexErrMsgTxt("pre3_mex('update'): z and h differ in length");
        if (r > 0 && ((int)mxGetM(in[1]) != r || (int)mxGetN(in[1]) != n)) mexErrMsgTxt("pre3_mex('update'): H must be length(z) x n");
        nnz = (int32_t *)mxCalloc(r ? r : 1, sizeof(int32_t));
        col = (int32_t *)mxCalloc((size_t)(r ? r : 1) * 16, sizeof(int32_t));
        val = (double *)mxCalloc((size_t)(r ? r : 1) * 16, sizeof(double));
        if (r > 0 && mxIsSparse(in[1])) {             /* CSC -> rows */
            const mwIndex *ir = mxGetIr(in[1]), *jc = mxGetJc(in[1]);
            const double *pr = mxGetPr(in[1]);
            mwIndex k;
            for (j = 0; j < n; ++j)
                for (k = jc[j]; k < jc[j + 1]; ++k) {
                    a = (int)ir[k];
                    if (pr[k] == 0.0) continue;
                    if (nnz[a] >= 16) mexErrMsgTxt("pre3_mex('update'): a row of H has more than 16 non-zeros");
                    col[a * 16 + nnz[a]] = j; val[a * 16 + nnz[a]] = pr[k]; ++nnz[a];
                }
        } else if (r > 0) {
            const double *H = mxGetPr(in[1]);
            for (j = 0; j < n; ++j)
                for (a = 0; a < r; ++a) {
                    double v = H[(size_t)j * r + a];
                    if (v == 0.0) continue;
                    if (nnz[a] >= 16) mexErrMsgTxt("pre3_mex('update'): a row of H has more than 16 non-zeros");
                    col[a * 16 + nnz[a]] = j; val[a * 16 + nnz[a]] = v; ++nnz[a];
                }
        }
        if (!mxIsEmpty(in[2])) {                      /* column-major -> row-major */
            const double *Rm = mxGetPr(in[2]);
            if ((int)mxGetM(in[2]) != r || (int)mxGetN(in[2]) != r) mexErrMsgTxt("pre3_mex('update'): R must be length(z) x length(z)");
            Rrow = (double *)mxMalloc(sizeof(double) * (size_t)(r ? r * r : 1));
            for (i = 0; i < r; ++i) for (j = 0; j < r; ++j) Rrow[(size_t)i * r + j] = Rm[(size_t)j * r + i];
        }
        rc = pre3_update_rows(g_ctx, r, 16, nnz, col, val, Rrow, mxGetPr(in[3]), mxGetPr(in[4]));
        mxFree(nnz); mxFree(col); mxFree(val); if (Rrow) mxFree(Rrow);
        check(rc);
    }
    else if (!strcmp(cmd, "heading")) {           /* applied = pre3_mex('heading', R_plane (3x3), strict): ekf_heading_update.m:27-52 on the resident estimate
                                                     (pre3_heading_update; strict = 1: the reference's gate, quirk Q12) */
        int32_t applied = 0;
        if (mxGetNumberOfElements(in[1]) != 9) mexErrMsgTxt("pre3_mex('heading'): R_plane must be 3 x 3");
        check(pre3_heading_update(g_ctx, mxGetPr(in[1]), nin > 2 ? (int)mxGetScalar(in[2]) : 1, &applied));
        out[0] = mxCreateDoubleScalar((double)applied);
    }
    else if (!strcmp(cmd, "plane_heading")) {     /* applied = pre3_mex('plane_heading', x_sr, y_sr, z_sr, draws (n_draw x 3, 0-based positions in the cropped
                                                     point list), strict): mono_slam.m:189-193 -- plane_fit_to_data.m on the range image, then
                                                     ekf_heading_update(filter, R_plane') -- fit, gate and update on the device (pre3_heading_from_scan) */
        int32_t applied = 0;
        int rows = (int)mxGetM(in[1]), cols = (int)mxGetN(in[1]), nd = (int)mxGetM(in[4]), i, j, rc;
        int32_t *d;
        if (nin < 5) mexErrMsgTxt("pre3_mex('plane_heading', x_sr, y_sr, z_sr, draws [, strict])");
        if ((int)mxGetM(in[2]) != rows || (int)mxGetN(in[2]) != cols || (int)mxGetM(in[3]) != rows || (int)mxGetN(in[3]) != cols)
            mexErrMsgTxt("pre3_mex('plane_heading'): x_sr, y_sr, z_sr must have the same size");
        if (mxGetN(in[4]) != 3) mexErrMsgTxt("pre3_mex('plane_heading'): draws must be n_draw x 3");
        d = (int32_t *)mxMalloc(sizeof(int32_t) * 3 * (nd ? nd : 1));
        for (i = 0; i < nd; ++i) for (j = 0; j < 3; ++j) d[3 * i + j] = (int32_t)mxGetPr(in[4])[(size_t)j * nd + i];
        rc = pre3_heading_from_scan(g_ctx, rows, cols, mxGetPr(in[1]), mxGetPr(in[2]), mxGetPr(in[3]), NULL, 0.02, nd, d, 1,
                                    nin > 5 ? (int)mxGetScalar(in[5]) : 1, &applied, NULL);
        mxFree(d);
        check(rc);
        out[0] = mxCreateDoubleScalar((double)applied);
    }
    else if (!strcmp(cmd, "plane_heading_seeded")) {   /* applied = pre3_mex('plane_heading_seeded', x_sr, y_sr, z_sr, seed, seq [, n_draw, strict]): 'plane_heading' with
                                                          ransac.m:142-176's draws made on the device from (seed, seq) (pre3_heading_from_scan_seeded); n_draw: 1001 */
        int32_t applied = 0;
        int rows = (int)mxGetM(in[1]), cols = (int)mxGetN(in[1]);
        if (nin < 6) mexErrMsgTxt("pre3_mex('plane_heading_seeded', x_sr, y_sr, z_sr, seed, seq [, n_draw, strict])");
        if ((int)mxGetM(in[2]) != rows || (int)mxGetN(in[2]) != cols || (int)mxGetM(in[3]) != rows || (int)mxGetN(in[3]) != cols)
            mexErrMsgTxt("pre3_mex('plane_heading_seeded'): x_sr, y_sr, z_sr must have the same size");
        check(pre3_heading_from_scan_seeded(g_ctx, rows, cols, mxGetPr(in[1]), mxGetPr(in[2]), mxGetPr(in[3]), NULL, 0.02,
                                            nin > 6 ? (int)mxGetScalar(in[6]) : PRE3_PLANE_MAX_DRAWS, (uint64_t)mxGetScalar(in[4]), (uint64_t)mxGetScalar(in[5]), 1,
                                            nin > 7 ? (int)mxGetScalar(in[7]) : 1, NULL, &applied, NULL));
        out[0] = mxCreateDoubleScalar((double)applied);
    }
    else if (!strcmp(cmd, "heading_frame")) {     /* applied = pre3_mex('heading_frame', seed, seq [, n_draw = 1001, strict = 1]): mono_slam.m:189-193 on the resident frame -- the box
                                                     gathered from its filtered planes, fit, gate and update on the device (pre3_heading_from_frame_seeded); a non-finite coordinate
                                                     inside the box is an error and leaves x and P untouched */
        int32_t applied = 0;
        if (nin < 3 || nin > 5) mexErrMsgTxt("pre3_mex('heading_frame', seed, seq [, n_draw, strict]): two to four arguments");
        if (!g_sr) mexErrMsgTxt("pre3_mex('heading_frame'): call pre3_mex('sr_frame', ...) first");
        check(pre3_heading_from_frame_seeded(g_ctx, g_sr, NULL, 0.02, nin > 3 ? (int)mxGetScalar(in[3]) : PRE3_PLANE_MAX_DRAWS, (uint64_t)mxGetScalar(in[1]),
                                             (uint64_t)mxGetScalar(in[2]), 1, nin > 4 ? (int)mxGetScalar(in[4]) : 1, NULL, &applied, NULL));
        out[0] = mxCreateDoubleScalar((double)applied);
    }
    else if (!strcmp(cmd, "predict_pair")) {      /* [T, q, sta, pnum] = pre3_mex('predict_pair', seed, seq [, thresh = 1.5]): fv.m:47 + ekf_prediction.m:29 -- 'vo_pair' between the
                                                     frame 'sr_keep' put aside and the resident one, then 'predict' with that pair's u = [T; q] (the identity motion unless
                                                     sta == 1) read on the device (pre3_predict_pair_seeded).  Without output arguments nothing is waited for: a pair 'vo_pair'
                                                     would refuse is then predicted with the identity motion and reported by the next call that reads the device's error words */
        pre3_vo_result r; int32_t pnum = 0;
        if (nin < 3 || nin > 4) mexErrMsgTxt("pre3_mex('predict_pair', seed, seq [, thresh]): two or three arguments");
        if (!g_sr || !g_sr_prev) mexErrMsgTxt("pre3_mex('predict_pair'): needs two frames -- 'sr_frame' + 'sr_keypoints', 'sr_keep', then 'sr_frame' + 'sr_keypoints' again");
        check(pre3_predict_pair_seeded(g_ctx, g_sr_prev, g_sr, nin > 3 ? mxGetScalar(in[3]) : 1.5, (uint64_t)mxGetScalar(in[1]), (uint64_t)mxGetScalar(in[2]),
                                       nout > 0 ? &pnum : NULL, nout > 0 ? &r : NULL));
        if (nout > 0) { out[0] = mxCreateDoubleMatrix(3, 1, mxREAL); memcpy(mxGetPr(out[0]), r.u, sizeof(double) * 3); }
        if (nout > 1) { out[1] = mxCreateDoubleMatrix(4, 1, mxREAL); memcpy(mxGetPr(out[1]), r.u + 3, sizeof(double) * 4); }
        if (nout > 2) out[2] = mxCreateDoubleScalar(r.sta);
        if (nout > 3) out[3] = mxCreateDoubleScalar(pnum);
    }
    else if (!strcmp(cmd, "process_noise")) {     /* [Pn, source] = pre3_mex('process_noise' [, Pn]): predict_state_and_covariance.m:98-102 -- with a 7 x 7 Pn every prediction from now
                                                     on takes it (finite, symmetric, no negative diagonal entry); with [] the reference's constant is back; without it nothing is
                                                     set.  Pn out: the noise in force; source 0 the constant, 1 the caller's (pre3_set_process_noise / pre3_get_process_noise) */
        int src = 0;
        if (nin > 2) mexErrMsgTxt("pre3_mex('process_noise' [, Pn]): at most one argument");
        if (nin > 1) {
            if (!mxIsEmpty(in[1]) && (!mxIsDouble(in[1]) || mxIsComplex(in[1]) || mxGetM(in[1]) != 7 || mxGetN(in[1]) != 7)) mexErrMsgTxt("pre3_mex('process_noise', Pn): Pn is a real 7 x 7 double matrix, or []");
            check(pre3_set_process_noise(g_ctx, mxIsEmpty(in[1]) ? NULL : mxGetPr(in[1])));      /* (symmetric: row-major == column-major) */
        }
        if (nout > 0 || nin == 1) {
            out[0] = mxCreateDoubleMatrix(7, 7, mxREAL);
            check(pre3_get_process_noise(g_ctx, mxGetPr(out[0]), &src));
            if (nout > 1) out[1] = mxCreateDoubleScalar(src);
        }
    }
    else if (!strcmp(cmd, "vo_cov")) {            /* [cov, status, n] = pre3_mex('vo_cov', op_pset1, op_pset2, rot, trans [, inliers]): calc_cov_RANSAC_dr_ye.m:17-30 on the cached
                                                     contents of a RANSAC_RESULT_%d_%d.mat -- op_pset1, op_pset2 3 x pnum, rot 3 x 3 with op_pset1 ~ rot * op_pset2 + trans.  cov 7 x 7
                                                     over [T; q] (zeros unless status == 1); status 0 fewer than four points, 1 valid, 2 unusable (pre3_vo_cov, on device 0) */
        double u[7], R[9], Tq, S, a, b, c, d, *rp; int32_t status = 0, n = 0, *inl = NULL; int i, k, rc; mwSize pnum;
        if (nin < 5 || nin > 6) mexErrMsgTxt("pre3_mex('vo_cov', op_pset1, op_pset2, rot, trans [, inliers]): four or five arguments");
        pnum = mxGetN(in[1]);
        if (!mxIsDouble(in[1]) || !mxIsDouble(in[2]) || !mxIsDouble(in[3]) || !mxIsDouble(in[4]) || mxGetM(in[1]) != 3 || mxGetM(in[2]) != 3 || mxGetN(in[2]) != pnum
            || mxGetNumberOfElements(in[3]) != 9 || mxGetNumberOfElements(in[4]) != 3 || (nin > 5 && mxGetNumberOfElements(in[5]) != pnum))
            mexErrMsgTxt("pre3_mex('vo_cov'): op_pset1, op_pset2 are 3 x pnum, rot 3 x 3, trans 3 x 1, inliers pnum x 1 (all double)");
        rp = mxGetPr(in[3]);
        for (i = 0; i < 3; ++i) for (k = 0; k < 3; ++k) R[3 * i + k] = rp[i + 3 * k];      /* column-major -> row-major */
        Tq = R[0] + R[4] + R[8] + 1;                                                       /* R2q.m, the sign of Calculate_V_Omega_RANSAC_dr_ye.m:48 */
        if (Tq > 0.00000001) { S = 2 * sqrt(Tq); a = 0.25 * S; b = (R[5] - R[7]) / S; c = (R[6] - R[2]) / S; d = (R[1] - R[3]) / S; }
        else if (R[0] > R[4] && R[0] > R[8]) { S = 2 * sqrt(1.0 + R[0] - R[4] - R[8]); a = (R[5] - R[7]) / S; b = 0.25 * S; c = (R[1] + R[3]) / S; d = (R[6] + R[2]) / S; }
        else if (R[4] > R[8]) { S = 2 * sqrt(1.0 + R[4] - R[0] - R[8]); a = (R[6] - R[2]) / S; b = (R[1] + R[3]) / S; c = 0.25 * S; d = (R[5] + R[7]) / S; }
        else { S = 2 * sqrt(1.0 + R[8] - R[0] - R[4]); a = (R[1] - R[3]) / S; b = (R[6] + R[2]) / S; c = (R[5] + R[7]) / S; d = 0.25 * S; }
        memcpy(u, mxGetPr(in[4]), sizeof(double) * 3); u[3] = a; u[4] = -b; u[5] = -c; u[6] = -d;
        if (nin > 5) { inl = (int32_t *)mxMalloc(sizeof(int32_t) * (pnum ? pnum : 1)); for (i = 0; i < (int)pnum; ++i) inl[i] = mxGetPr(in[5])[i] != 0; }
        out[0] = mxCreateDoubleMatrix(7, 7, mxREAL);
        rc = pre3_vo_cov(0, (int)pnum, mxGetPr(in[1]), mxGetPr(in[2]), inl, u, mxGetPr(out[0]), &status, &n);
        if (inl) mxFree(inl);
        check(rc);
        if (nout > 1) out[1] = mxCreateDoubleScalar(status);
        if (nout > 2) out[2] = mxCreateDoubleScalar(n);
    }
    else if (!strcmp(cmd, "predict_pair_cov")) {  /* [T, q, sta, pnum, cov, cov_status] = pre3_mex('predict_pair_cov', seed, seq [, thresh = 1.5]): 'predict_pair' with the pair's own
                                                     covariance, computed on the device from its inliers, as this one prediction's Pn (predict_state_and_covariance.m:115) when
                                                     cov_status == 1 and sta == 1 -- else the noise 'process_noise' reports.  cov 7 x 7 (zeros unless cov_status == 1).  Without
                                                     output arguments nothing is waited for (pre3_predict_pair_cov_seeded) */
        pre3_vo_result r; int32_t pnum = 0, cst = 0; double cov[49]; int i;
        if (nin < 3 || nin > 4) mexErrMsgTxt("pre3_mex('predict_pair_cov', seed, seq [, thresh]): two or three arguments");
        if (!g_sr || !g_sr_prev) mexErrMsgTxt("pre3_mex('predict_pair_cov'): needs two frames -- 'sr_frame' + 'sr_keypoints', 'sr_keep', then 'sr_frame' + 'sr_keypoints' again");
        for (i = 0; i < 49; ++i) cov[i] = 0;
        check(pre3_predict_pair_cov_seeded(g_ctx, g_sr_prev, g_sr, nin > 3 ? mxGetScalar(in[3]) : 1.5, (uint64_t)mxGetScalar(in[1]), (uint64_t)mxGetScalar(in[2]),
                                           nout > 0 ? &pnum : NULL, nout > 0 ? &r : NULL, nout > 4 ? cov : NULL, nout > 4 ? &cst : NULL));
        if (nout > 0) { out[0] = mxCreateDoubleMatrix(3, 1, mxREAL); memcpy(mxGetPr(out[0]), r.u, sizeof(double) * 3); }
        if (nout > 1) { out[1] = mxCreateDoubleMatrix(4, 1, mxREAL); memcpy(mxGetPr(out[1]), r.u + 3, sizeof(double) * 4); }
        if (nout > 2) out[2] = mxCreateDoubleScalar(r.sta);
        if (nout > 3) out[3] = mxCreateDoubleScalar(pnum);
        if (nout > 4) { out[4] = mxCreateDoubleMatrix(7, 7, mxREAL); memcpy(mxGetPr(out[4]), cov, sizeof cov); }
        if (nout > 5) out[5] = mxCreateDoubleScalar(cst);
    }
    else if (!strcmp(cmd, "icp_cov")) {           /* [cov, status, n] = pre3_mex('icp_cov', data1, data2, corr, T, q): the closed-form covariance of the ICP's [T; q] over its final
                                                     pairs -- data1 3 x n1 the model, data2 3 x n2 the source AS icp_with_init TOOK IT (before Rinit, Tinit), corr p x 2 or p x 3 as
                                                     icp_with_init returns it (1-based model, source), T 3 x 1 and q 4 x 1 of the run's u (data1 ~ R(q) data2 + T).  cov 7 x 7
                                                     (zeros unless status == 1); status 0 fewer than four pairs, 1 valid, 2 unusable (pre3_icp_cov, on device 0).  Sensor noise
                                                     only: optimistic as a process noise */
        double u[7]; int32_t status = 0, n = 0, *cr; int i, rc; mwSize p, n1, n2;
        if (nin != 6) mexErrMsgTxt("pre3_mex('icp_cov', data1, data2, corr, T, q): five arguments");
        n1 = mxGetN(in[1]); n2 = mxGetN(in[2]); p = mxGetM(in[3]);
        if (!mxIsDouble(in[1]) || !mxIsDouble(in[2]) || !mxIsDouble(in[3]) || !mxIsDouble(in[4]) || !mxIsDouble(in[5]) || mxGetM(in[1]) != 3 || mxGetM(in[2]) != 3
            || (p > 0 && mxGetN(in[3]) != 2 && mxGetN(in[3]) != 3) || mxGetNumberOfElements(in[4]) != 3 || mxGetNumberOfElements(in[5]) != 4)
            mexErrMsgTxt("pre3_mex('icp_cov'): data1 3 x n1, data2 3 x n2, corr p x 2 or p x 3, T 3 x 1, q 4 x 1 (all double)");
        memcpy(u, mxGetPr(in[4]), sizeof(double) * 3); memcpy(u + 3, mxGetPr(in[5]), sizeof(double) * 4);
        cr = (int32_t *)mxMalloc(sizeof(int32_t) * 2 * (p ? p : 1));
        for (i = 0; i < (int)p; ++i) { cr[2 * i] = (int32_t)mxGetPr(in[3])[i]; cr[2 * i + 1] = (int32_t)mxGetPr(in[3])[i + p]; }      /* column-major p x k -> rows */
        out[0] = mxCreateDoubleMatrix(7, 7, mxREAL);
        rc = pre3_icp_cov(0, mxGetPr(in[1]), (int)n1, mxGetPr(in[2]), (int)n2, cr, (int)p, u, mxGetPr(out[0]), &status, &n);
        mxFree(cr);
        check(rc);
        if (nout > 1) out[1] = mxCreateDoubleScalar(status);
        if (nout > 2) out[2] = mxCreateDoubleScalar(n);
    }
    else if (!strcmp(cmd, "epnp") || !strcmp(cmd, "pnp_ransac")) {
        /* [R, T, Xc, best_solution, sta, err, u] = pre3_mex('epnp', Xw, U, cam_struct [, undistort = 0]): aux_code/EPnP_matlab/EPnP/efficient_pnp.m for kernel
           dimensions 1 to 3, in its order of outputs -- Xw 3 x n points, U 2 x n pixels (one correspondence a column), Xc = R Xw + T (3 x n), best_solution
           1-based; sta 1 ok, 2 the best of three where the reference would go on to dimension 4 (not built), -1 a non-finite intermediate; u 7 x 1 the pose in
           the VO pair's convention.  undistort = 1: every pixel through undistort_fm_my_version.m first (pre3_epnp, on device 0).
           [R, T, inliers, support, sta, err, u] = pre3_mex('pnp_ransac', Xw, U, cam_struct, n_hyp, thr_px, seed, seq [, undistort = 0]): up to 700 six-point
           hypotheses drawn on the device, all scored (reprojection distance < thr_px, depth > 0), the refit over the winner's inliers (n x 1 flags);
           sta 0: fewer than six inliers (pre3_pnp_ransac_seeded) */
        pre3_cam cam; pre3_pnp_result r; int i, k, ransac = !strcmp(cmd, "pnp_ransac"), und; mwSize n; int32_t *inl = NULL;
        const char *fn[7] = { "f", "Cx", "Cy", "k1", "k2", "nRows", "nCols" }; double *cf = &cam.f;
        if (ransac ? (nin < 8 || nin > 9) : (nin < 4 || nin > 5))
            mexErrMsgTxt("pre3_mex('epnp', Xw, U, cam [, undistort]) or pre3_mex('pnp_ransac', Xw, U, cam, n_hyp, thr_px, seed, seq [, undistort])");
        n = mxGetN(in[1]);
        if (!mxIsDouble(in[1]) || !mxIsDouble(in[2]) || mxGetM(in[1]) != 3 || mxGetM(in[2]) != 2 || mxGetN(in[2]) != n || !mxIsStruct(in[3]))
            mexErrMsgTxt("pre3_mex('epnp' / 'pnp_ransac'): Xw 3 x n, U 2 x n (double), cam a struct");
        for (i = 0; i < 7; ++i) { mxArray *v = mxGetField(in[3], 0, fn[i]); if (!v) mexErrMsgTxt("pre3_mex: cam field missing"); cf[i] = mxGetScalar(v); }
        memset(&r, 0, sizeof r);
        if (ransac) {
            und = nin > 8 ? (int)mxGetScalar(in[8]) : 0;
            inl = (int32_t *)mxCalloc(n ? n : 1, sizeof(int32_t));
            check(pre3_pnp_ransac_seeded(0, &cam, und, (int)n, mxGetPr(in[1]), mxGetPr(in[2]), (int)mxGetScalar(in[4]), (uint64_t)mxGetScalar(in[6]),
                                         (uint64_t)mxGetScalar(in[7]), mxGetScalar(in[5]), NULL, NULL, NULL, inl, NULL, &r));
        } else {
            und = nin > 4 ? (int)mxGetScalar(in[4]) : 0;
            check(pre3_epnp(0, &cam, und, (int)n, mxGetPr(in[1]), mxGetPr(in[2]), &r));
        }
        out[0] = mxCreateDoubleMatrix(3, 3, mxREAL);
        for (i = 0; i < 3; ++i) for (k = 0; k < 3; ++k) mxGetPr(out[0])[i + 3 * k] = r.R[3 * i + k];      /* row-major -> column-major */
        if (nout > 1) { out[1] = mxCreateDoubleMatrix(3, 1, mxREAL); memcpy(mxGetPr(out[1]), r.T, sizeof r.T); }
        if (nout > 2) {
            if (ransac) { out[2] = mxCreateDoubleMatrix(n, 1, mxREAL); for (i = 0; i < (int)n; ++i) mxGetPr(out[2])[i] = inl[i]; }
            else {
                const double *xw = mxGetPr(in[1]); double *xc;
                out[2] = mxCreateDoubleMatrix(3, n, mxREAL); xc = mxGetPr(out[2]);
                for (i = 0; i < (int)n; ++i) for (k = 0; k < 3; ++k) xc[3 * i + k] = r.R[3 * k] * xw[3 * i] + r.R[3 * k + 1] * xw[3 * i + 1] + r.R[3 * k + 2] * xw[3 * i + 2] + r.T[k];
            }
        }
        if (inl) mxFree(inl);
        if (nout > 3) out[3] = mxCreateDoubleScalar(ransac ? r.n_support : r.best + 1);
        if (nout > 4) out[4] = mxCreateDoubleScalar(r.sta);
        if (nout > 5) { out[5] = mxCreateDoubleMatrix(3, 1, mxREAL); memcpy(mxGetPr(out[5]), r.err, sizeof r.err); }
        if (nout > 6) { out[6] = mxCreateDoubleMatrix(7, 1, mxREAL); memcpy(mxGetPr(out[6]), r.u, sizeof r.u); }
    }
    else if (!strcmp(cmd, "vo_pair_pnp")) {       /* [T, q, sta, pnp_sta, R, Tc, err, pnum, T3, q3] = pre3_mex('vo_pair_pnp', seed, seq, cam_struct [, undistort = 1, thresh = 1.5]):
                                                     RANSAC_CALC_VER2.m:191 in place between the kept frame and the current one -- the VO pair's launches, then
                                                     efficient_pnp over the pair's inliers, prev's range points against cur's PIXELS.  T, q: the EPnP pose in the pair's
                                                     convention (the identity unless pnp_sta is 1 or 2); sta the pair's; R, Tc with Xc = R Xw + Tc; T3, q3 the pair's
                                                     own 3-D / 3-D increment (pre3_vo_pair_pnp_seeded) */
        pre3_cam cam; pre3_pnp_result r; pre3_vo_result v; int32_t pnum = 0; int i, k;
        const char *fn[7] = { "f", "Cx", "Cy", "k1", "k2", "nRows", "nCols" }; double *cf = &cam.f;
        if (nin < 4 || nin > 6 || !mxIsStruct(in[3])) mexErrMsgTxt("pre3_mex('vo_pair_pnp', seed, seq, cam [, undistort, thresh]): three to five arguments, cam a struct");
        if (!g_sr || !g_sr_prev) mexErrMsgTxt("pre3_mex('vo_pair_pnp'): needs two frames -- 'sr_frame' + 'sr_keypoints', 'sr_keep', then 'sr_frame' + 'sr_keypoints' again");
        for (i = 0; i < 7; ++i) { mxArray *f = mxGetField(in[3], 0, fn[i]); if (!f) mexErrMsgTxt("pre3_mex: cam field missing"); cf[i] = mxGetScalar(f); }
        memset(&r, 0, sizeof r); memset(&v, 0, sizeof v);
        check(pre3_vo_pair_pnp_seeded(g_sr_prev, g_sr, nin > 5 ? mxGetScalar(in[5]) : 1.5, (uint64_t)mxGetScalar(in[1]), (uint64_t)mxGetScalar(in[2]), &cam,
                                      nin > 4 ? (int)mxGetScalar(in[4]) : 1, &pnum, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, &v, NULL, &r));
        out[0] = mxCreateDoubleMatrix(3, 1, mxREAL); memcpy(mxGetPr(out[0]), r.u, sizeof(double) * 3);
        if (nout > 1) { out[1] = mxCreateDoubleMatrix(4, 1, mxREAL); memcpy(mxGetPr(out[1]), r.u + 3, sizeof(double) * 4); }
        if (nout > 2) out[2] = mxCreateDoubleScalar(v.sta);
        if (nout > 3) out[3] = mxCreateDoubleScalar(r.sta);
        if (nout > 4) { out[4] = mxCreateDoubleMatrix(3, 3, mxREAL); for (i = 0; i < 3; ++i) for (k = 0; k < 3; ++k) mxGetPr(out[4])[i + 3 * k] = r.R[3 * i + k]; }
        if (nout > 5) { out[5] = mxCreateDoubleMatrix(3, 1, mxREAL); memcpy(mxGetPr(out[5]), r.T, sizeof r.T); }
        if (nout > 6) { out[6] = mxCreateDoubleMatrix(3, 1, mxREAL); memcpy(mxGetPr(out[6]), r.err, sizeof r.err); }
        if (nout > 7) out[7] = mxCreateDoubleScalar(pnum);
        if (nout > 8) { out[8] = mxCreateDoubleMatrix(3, 1, mxREAL); memcpy(mxGetPr(out[8]), v.u, sizeof(double) * 3); }
        if (nout > 9) { out[9] = mxCreateDoubleMatrix(4, 1, mxREAL); memcpy(mxGetPr(out[9]), v.u + 3, sizeof(double) * 4); }
    }
    else if (!strcmp(cmd, "predict_icp_pair")) {  /* [T, q, sta, icp_sta, taken, cov_pair, cov_icp, cov_status] = pre3_mex('predict_icp_pair', seed, seq, res [, stride = 1, max_error = inf,
                                                     noise = 0, thresh = 1.5]): 'predict_pair' with the dense ICP of 'icp_pair' between the pair and the prediction -- the ICP's [T; q]
                                                     when the pair's is taken, icp_sta == 1, it is finite and its error <= max_error; noise 0 the context's own, 1 the pair's covariance,
                                                     2 the ICP's closed-form covariance, 3 that plus the context's own (PRE3_NOISE_*).  T, q: the increment taken (taken(1): 0 identity,
                                                     1 the pair's, 2 the ICP's; taken(2): the noise taken).  Without output arguments nothing is waited for (pre3_predict_icp_pair_seeded) */
        pre3_vo_result r; pre3_icp_result ir; int32_t pnum = 0, cst[2] = { 0, 0 }, tk[2] = { 0, 0 }; double cov[98]; const double *u; int i;
        static const double u_id[7] = { 0, 0, 0, 1, 0, 0, 0 };
        if (nin < 4 || nin > 8) mexErrMsgTxt("pre3_mex('predict_icp_pair', seed, seq, res [, stride, max_error, noise, thresh]): three to seven arguments");
        if (!g_sr || !g_sr_prev) mexErrMsgTxt("pre3_mex('predict_icp_pair'): needs two frames -- 'sr_frame' + 'sr_keypoints', 'sr_keep', then 'sr_frame' + 'sr_keypoints' again");
        for (i = 0; i < 98; ++i) cov[i] = 0;
        memset(&ir, 0, sizeof ir); memset(&r, 0, sizeof r);
        check(pre3_predict_icp_pair_seeded(g_ctx, g_sr_prev, g_sr, nin > 7 ? mxGetScalar(in[7]) : 1.5, (uint64_t)mxGetScalar(in[1]), (uint64_t)mxGetScalar(in[2]),
                                           nin > 4 ? (int)mxGetScalar(in[4]) : 1, mxGetScalar(in[3]), nin > 5 ? mxGetScalar(in[5]) : mxGetInf(),
                                           nin > 6 ? (int)mxGetScalar(in[6]) : PRE3_NOISE_CONTEXT, nout > 0 ? &pnum : NULL, nout > 0 ? &r : NULL, nout > 0 ? &ir : NULL,
                                           nout > 0 ? cov : NULL, nout > 0 ? cst : NULL, nout > 0 ? tk : NULL));
        u = tk[0] == 2 ? ir.u : tk[0] == 1 ? r.u : u_id;
        if (nout > 0) { out[0] = mxCreateDoubleMatrix(3, 1, mxREAL); memcpy(mxGetPr(out[0]), u, sizeof(double) * 3); }
        if (nout > 1) { out[1] = mxCreateDoubleMatrix(4, 1, mxREAL); memcpy(mxGetPr(out[1]), u + 3, sizeof(double) * 4); }
        if (nout > 2) out[2] = mxCreateDoubleScalar(r.sta);
        if (nout > 3) out[3] = mxCreateDoubleScalar(ir.sta);
        if (nout > 4) { out[4] = mxCreateDoubleMatrix(1, 2, mxREAL); mxGetPr(out[4])[0] = tk[0]; mxGetPr(out[4])[1] = tk[1]; }
        if (nout > 5) { out[5] = mxCreateDoubleMatrix(7, 7, mxREAL); memcpy(mxGetPr(out[5]), cov, sizeof(double) * 49); }
        if (nout > 6) { out[6] = mxCreateDoubleMatrix(7, 7, mxREAL); memcpy(mxGetPr(out[6]), cov + 49, sizeof(double) * 49); }
        if (nout > 7) { out[7] = mxCreateDoubleMatrix(1, 2, mxREAL); mxGetPr(out[7])[0] = cst[0]; mxGetPr(out[7])[1] = cst[1]; }
    }
    else if (!strcmp(cmd, "map_delete")) {        /* pre3_mex('map_delete', idx (0-based, ascending))   delete_features.m:54-74 */
        int k = (int)mxGetNumberOfElements(in[1]), i, rc; int32_t *d = (int32_t *)mxMalloc(sizeof(int32_t) * (k ? k : 1));
        for (i = 0; i < k; ++i) d[i] = (int32_t)mxGetPr(in[1])[i];
        rc = pre3_map_delete(g_ctx, k, d); mxFree(d); check(rc);
    }
    else if (!strcmp(cmd, "map_add")) {           /* pre3_mex('map_add', uvd (2xk), std_pxl, initial_rho (1xk))   add_features_inverse_depth.m:27-47 */
        check(pre3_map_add_inverse_depth(g_ctx, (int)mxGetN(in[1]), mxGetPr(in[1]), mxGetScalar(in[2]), mxGetPr(in[3])));
    }
    else if (!strcmp(cmd, "map_convert")) {       /* converted = pre3_mex('map_convert', 0.1)   inversedepth_2_cartesian.m:27-76 */
        int N = pre3_get_map(g_ctx, NULL), i, rc; int32_t *f = (int32_t *)mxCalloc(N ? N : 1, sizeof(int32_t));
        rc = pre3_map_inversedepth_2_cartesian(g_ctx, mxGetScalar(in[1]), f);
        out[0] = mxCreateDoubleMatrix(1, N, mxREAL);
        for (i = 0; i < N; ++i) mxGetPr(out[0])[i] = f[i];
        mxFree(f); check(rc);
    }
    else if (!strcmp(cmd, "map_management")) {    /* converted = pre3_mex('map_management', del_idx (0-based, ascending), linearity_thr (< 0: no conversion), uvd (2xk), std_pxl, initial_rho (1xk))
                                                     map_management.m:27-79 as one call: delete_features, inversedepth_2_cartesian, the new features -- one pass over P */
        int k = (int)mxGetNumberOfElements(in[1]), N = pre3_get_map(g_ctx, NULL), i, rc;
        int32_t *d = (int32_t *)mxMalloc(sizeof(int32_t) * (k ? k : 1)), *f = (int32_t *)mxCalloc(N ? N : 1, sizeof(int32_t));
        for (i = 0; i < k; ++i) d[i] = (int32_t)mxGetPr(in[1])[i];
        rc = pre3_map_management(g_ctx, k, d, mxGetScalar(in[2]), f, (int)mxGetN(in[3]), mxGetPr(in[3]), mxGetScalar(in[4]), mxGetPr(in[5]));
        out[0] = mxCreateDoubleMatrix(1, N, mxREAL);
        for (i = 0; i < N; ++i) mxGetPr(out[0])[i] = f[i];
        mxFree(d); mxFree(f); check(rc);
    }
    else if (!strcmp(cmd, "set_book")) {          /* pre3_mex('set_book', [tp; tm; init_frame; last_visible] (4xN) [, first (0-based)])   features_info's counters */
        int k, i, rc; int32_t *b;
        if (nin < 2) mexErrMsgTxt("pre3_mex('set_book', B [, first]): the book is missing");
        k = (int)mxGetN(in[1]); b = (int32_t *)mxMalloc(sizeof(int32_t) * 4 * (k ? k : 1));
        if (k > 0 && mxGetM(in[1]) != 4) mexErrMsgTxt("pre3_mex('set_book'): the book is 4 x N");
        for (i = 0; i < 4 * k; ++i) b[i] = (int32_t)mxGetPr(in[1])[i];
        rc = pre3_set_book(g_ctx, nin > 2 ? (int)mxGetScalar(in[2]) : 0, k, b); mxFree(b); check(rc);
    }
    else if (!strcmp(cmd, "book")) {              /* b = pre3_mex('book'): 4 x N [times_predicted; times_measured; init_frame; last_visible] */
        int N = pre3_get_map(g_ctx, NULL), i, rc; int32_t *b = (int32_t *)mxCalloc(4 * (N ? N : 1), sizeof(int32_t));
        rc = pre3_get_book(g_ctx, 0, N, b);
        if (rc == PRE3_OK) { out[0] = mxCreateDoubleMatrix(4, N, mxREAL); for (i = 0; i < 4 * N; ++i) mxGetPr(out[0])[i] = b[i]; }
        mxFree(b); check(rc);
    }
    else if (!strcmp(cmd, "map_policy")) {        /* [deleted, accepted, converted, stats] = pre3_mex('map_policy', step, UV (2xK), XYZ (3xK), DESC (128xK or []),
                                                     min_features, linearity_thr (< 0: none), std_pxl, strict): map_management.m:27-79 with its policy; UV is
                                                     UV_GoodFeaturesToInitialize(idx, 1:2)' (2xK, in Weighted_Smpl_wo_replacement's order); 1-based outputs */
        int K, N, i, rc; int32_t nd = 0, na = 0, st[4] = { 0, 0, 0, 0 }, *dl, *acc, *cv;
        if (nin != 9) mexErrMsgTxt("pre3_mex('map_policy', step, UV, XYZ, DESC, min_features, thr, std_pxl, strict): eight arguments");
        K = (int)mxGetN(in[2]); N = pre3_get_map(g_ctx, NULL);
        if ((K > 0 && mxGetM(in[2]) != 2) || (int)mxGetN(in[3]) != K || (K > 0 && mxGetM(in[3]) != 3)) mexErrMsgTxt("pre3_mex('map_policy'): UV is 2xK, XYZ 3xK");
        if (!mxIsEmpty(in[4]) && ((int)mxGetN(in[4]) != K || mxGetM(in[4]) != 128)) mexErrMsgTxt("pre3_mex('map_policy'): DESC is 128xK or []");
        dl = (int32_t *)mxCalloc(N ? N : 1, sizeof(int32_t)); acc = (int32_t *)mxCalloc(K ? K : 1, sizeof(int32_t)); cv = (int32_t *)mxCalloc(N ? N : 1, sizeof(int32_t));
        rc = pre3_map_policy(g_ctx, (int)mxGetScalar(in[1]), (int)mxGetScalar(in[5]), mxGetScalar(in[6]), mxGetScalar(in[7]), (int)mxGetScalar(in[8]), K,
                             mxGetPr(in[2]), mxGetPr(in[3]), mxIsEmpty(in[4]) ? NULL : mxGetPr(in[4]), dl, &nd, acc, &na, cv, st);
        if (rc == PRE3_OK) {
            out[0] = mxCreateDoubleMatrix(1, nd, mxREAL); for (i = 0; i < nd; ++i) mxGetPr(out[0])[i] = dl[i] + 1;
            if (nout > 1) { out[1] = mxCreateDoubleMatrix(1, na, mxREAL); for (i = 0; i < na; ++i) mxGetPr(out[1])[i] = acc[i] + 1; }
            if (nout > 2) { out[2] = mxCreateDoubleMatrix(1, N, mxREAL); for (i = 0; i < N; ++i) mxGetPr(out[2])[i] = cv[i]; }
            if (nout > 3) { out[3] = mxCreateDoubleMatrix(1, 4, mxREAL); for (i = 0; i < 4; ++i) mxGetPr(out[3])[i] = st[i]; }
        }
        mxFree(dl); mxFree(acc); mxFree(cv); check(rc);
    }
    else if (!strcmp(cmd, "map_policy_seeded")) { /* [deleted, accepted, converted, stats, order] = pre3_mex('map_policy_seeded', step, UV (2xK), XYZ (3xK), DESC (128xK or []),
                                                     min_features, linearity_thr (< 0: none), std_pxl, strict, [BoxLimX(2) BoxLimY(2)], seed, seq): 'map_policy' with
                                                     Weighted_Smpl_wo_replacement.m drawn on the device; UV is UV_GoodFeaturesToInitialize(:, 1:2)' as it stands;
                                                     accepted and order index its columns, 1-based (seed, seq: integers below 2^53) */
        int K, N, i, rc; int32_t nd = 0, na = 0, st[4] = { 0, 0, 0, 0 }, *dl, *acc, *cv, *ord;
        if (nin != 12) mexErrMsgTxt("pre3_mex('map_policy_seeded', step, UV, XYZ, DESC, min_features, thr, std_pxl, strict, box, seed, seq): eleven arguments");
        K = (int)mxGetN(in[2]); N = pre3_get_map(g_ctx, NULL);
        if ((K > 0 && mxGetM(in[2]) != 2) || (int)mxGetN(in[3]) != K || (K > 0 && mxGetM(in[3]) != 3)) mexErrMsgTxt("pre3_mex('map_policy_seeded'): UV is 2xK, XYZ 3xK");
        if (!mxIsEmpty(in[4]) && ((int)mxGetN(in[4]) != K || mxGetM(in[4]) != 128)) mexErrMsgTxt("pre3_mex('map_policy_seeded'): DESC is 128xK or []");
        if (mxGetNumberOfElements(in[9]) != 2) mexErrMsgTxt("pre3_mex('map_policy_seeded'): box is [BoxLimX(2) BoxLimY(2)]");
        dl = (int32_t *)mxCalloc(N ? N : 1, sizeof(int32_t)); acc = (int32_t *)mxCalloc(K ? K : 1, sizeof(int32_t)); cv = (int32_t *)mxCalloc(N ? N : 1, sizeof(int32_t));
        ord = (int32_t *)mxCalloc(K ? K : 1, sizeof(int32_t));
        rc = pre3_map_policy_seeded(g_ctx, (int)mxGetScalar(in[1]), (int)mxGetScalar(in[5]), mxGetScalar(in[6]), mxGetScalar(in[7]), (int)mxGetScalar(in[8]), K,
                                    mxGetPr(in[2]), mxGetPr(in[3]), mxIsEmpty(in[4]) ? NULL : mxGetPr(in[4]), (int)mxGetPr(in[9])[0], (int)mxGetPr(in[9])[1],
                                    (uint64_t)mxGetScalar(in[10]), (uint64_t)mxGetScalar(in[11]), ord, dl, &nd, acc, &na, cv, st);
        if (rc == PRE3_OK) {
            out[0] = mxCreateDoubleMatrix(1, nd, mxREAL); for (i = 0; i < nd; ++i) mxGetPr(out[0])[i] = dl[i] + 1;
            if (nout > 1) { out[1] = mxCreateDoubleMatrix(1, na, mxREAL); for (i = 0; i < na; ++i) mxGetPr(out[1])[i] = acc[i] + 1; }
            if (nout > 2) { out[2] = mxCreateDoubleMatrix(1, N, mxREAL); for (i = 0; i < N; ++i) mxGetPr(out[2])[i] = cv[i]; }
            if (nout > 3) { out[3] = mxCreateDoubleMatrix(1, 4, mxREAL); for (i = 0; i < 4; ++i) mxGetPr(out[3])[i] = st[i]; }
            if (nout > 4) { out[4] = mxCreateDoubleMatrix(1, K, mxREAL); for (i = 0; i < K; ++i) mxGetPr(out[4])[i] = ord[i] + 1; }
        }
        mxFree(dl); mxFree(acc); mxFree(cv); mxFree(ord); check(rc);
    }
    else if (!strcmp(cmd, "map_policy_frames")) { /* [deleted, accepted, converted, stats, order, match] = pre3_mex('map_policy_frames', step, min_features, linearity_thr (< 0: none),
                                                     std_pxl, strict, [BoxLimX(2) BoxLimY(2)], seed, seq [, thresh = 1.5]): 'map_policy_seeded' with the candidates of
                                                     initialize_features.m:95-99 built on the device from the frame 'sr_keep' put aside (its 'sr_keypoints' result through gate 0) and
                                                     the resident one; accepted and order index the columns of match, 1-based; match holds 1-based positions in the kept sets */
        int N, K1, i, rc; int32_t K = 0, nd = 0, na = 0, st[4] = { 0, 0, 0, 0 }, *dl, *acc, *cv, *ord; double *mt;
        if (nin < 9 || nin > 10) mexErrMsgTxt("pre3_mex('map_policy_frames', step, min_features, thr, std_pxl, strict, box, seed, seq [, thresh]): eight or nine arguments");
        if (!g_sr || !g_sr_prev) mexErrMsgTxt("pre3_mex('map_policy_frames'): needs two frames -- 'sr_frame' + 'sr_keypoints', 'sr_keep', then 'sr_frame' + 'sr_keypoints' again");
        if (mxGetNumberOfElements(in[6]) != 2) mexErrMsgTxt("pre3_mex('map_policy_frames'): box is [BoxLimX(2) BoxLimY(2)]");
        N = pre3_get_map(g_ctx, NULL); K1 = PRE3_SR_MAX_KEYPOINTS;
        dl = (int32_t *)mxCalloc(N ? N : 1, sizeof(int32_t)); acc = (int32_t *)mxCalloc(K1, sizeof(int32_t)); cv = (int32_t *)mxCalloc(N ? N : 1, sizeof(int32_t));
        ord = (int32_t *)mxCalloc(K1, sizeof(int32_t)); mt = (double *)mxCalloc(2 * (size_t)K1, sizeof(double));
        rc = pre3_map_policy_frames_seeded(g_ctx, g_sr_prev, g_sr, nin > 9 ? mxGetScalar(in[9]) : 1.5, (int)mxGetScalar(in[1]), (int)mxGetScalar(in[2]), mxGetScalar(in[3]),
                                           mxGetScalar(in[4]), (int)mxGetScalar(in[5]), (int)mxGetPr(in[6])[0], (int)mxGetPr(in[6])[1], (uint64_t)mxGetScalar(in[7]),
                                           (uint64_t)mxGetScalar(in[8]), &K, mt, ord, dl, &nd, acc, &na, cv, st);
        if (rc == PRE3_OK) {
            out[0] = mxCreateDoubleMatrix(1, nd, mxREAL); for (i = 0; i < nd; ++i) mxGetPr(out[0])[i] = dl[i] + 1;
            if (nout > 1) { out[1] = mxCreateDoubleMatrix(1, na, mxREAL); for (i = 0; i < na; ++i) mxGetPr(out[1])[i] = acc[i] + 1; }
            if (nout > 2) { out[2] = mxCreateDoubleMatrix(1, N, mxREAL); for (i = 0; i < N; ++i) mxGetPr(out[2])[i] = cv[i]; }
            if (nout > 3) { out[3] = mxCreateDoubleMatrix(1, 4, mxREAL); for (i = 0; i < 4; ++i) mxGetPr(out[3])[i] = st[i]; }
            if (nout > 4) { out[4] = mxCreateDoubleMatrix(1, K, mxREAL); for (i = 0; i < K; ++i) mxGetPr(out[4])[i] = ord[i] + 1; }
            if (nout > 5) { out[5] = mxCreateDoubleMatrix(2, K, mxREAL); memcpy(mxGetPr(out[5]), mt, sizeof(double) * 2 * (size_t)K); }
        }
        mxFree(dl); mxFree(acc); mxFree(cv); mxFree(ord); mxFree(mt); check(rc);
    }
    else if (!strcmp(cmd, "set_descriptors")) {   /* pre3_mex('set_descriptors', [features_info.Descriptor] (128xN), first (0-based)) */
        check(pre3_set_descriptors(g_ctx, nin > 2 ? (int)mxGetScalar(in[2]) : 0, (int)mxGetN(in[1]), mxGetPr(in[1])));
    }
    else if (!strcmp(cmd, "set_scan")) {          /* pre3_mex('set_scan', SCAN_SIFT.Descriptor_RAW, SCAN_SIFT.SCALE_ORIENT_POS_RAW) */
        check(pre3_set_scan(g_ctx, (int)mxGetN(in[1]), mxGetPr(in[1]), mxGetPr(in[2])));
    }
    else if (!strcmp(cmd, "set_scan_frame")) {    /* pre3_mex('set_scan_frame' [, which = 0]): 'set_scan' with the arrays taken from the resident frame's keypoint block on the device --
                                                     which = 0: the set handed to the last 'sr_keypoints' (Descriptor_RAW / SCALE_ORIENT_POS_RAW), 1: the set it kept */
        if (nin > 2) mexErrMsgTxt("pre3_mex('set_scan_frame' [, which]): at most one argument");
        if (!g_sr) mexErrMsgTxt("pre3_mex('set_scan_frame'): call pre3_mex('sr_frame', ...) and pre3_mex('sr_keypoints', ...) first");
        check(pre3_set_scan_frame(g_ctx, g_sr, nin > 1 ? (int)mxGetScalar(in[1]) : 0));
    }
    else if (!strcmp(cmd, "relocalise")) {        /* [T, q, taken, sta, n_support, match_idx, inliers, R, Tc] = pre3_mex('relocalise', seed, seq, Pn [, n_hyp = 200, thr_px = 2,
                                                     min_support = 12, undistort = 1, thresh = 1.5]): the library's own, the reference has none -- IN PLACE OF 'predict' on a frame
                                                     on which the caller has judged the filter lost: siftmatch of the whole map against the scan with no gate, the EPnP RANSAC of
                                                     'pnp_ransac' over the matched landmarks' 3-D points and the scan's pixels, then the prediction onto that pose under the wide
                                                     7 x 7 noise Pn; 'ic_search' and 'step_predicted' follow as usual.  T, q: the increment applied (the identity unless taken);
                                                     sta, n_support: the refit's; match_idx 2 x M, 1-based; inliers: 0/1 over the correspondences; R, Tc with Xc = R Xw + Tc.
                                                     Without output arguments nothing is waited for (pre3_relocalise_seeded) */
        pre3_reloc_result r; int N = pre3_get_map(g_ctx, NULL), i, k, rc;
        int32_t *pairs, *inl;
        if (nin < 4 || nin > 9) mexErrMsgTxt("pre3_mex('relocalise', seed, seq, Pn [, n_hyp, thr_px, min_support, undistort, thresh]): three to eight arguments");
        if (!mxIsDouble(in[3]) || mxIsComplex(in[3]) || mxGetM(in[3]) != 7 || mxGetN(in[3]) != 7) mexErrMsgTxt("pre3_mex('relocalise', seed, seq, Pn): Pn is a real 7 x 7 double matrix");
        memset(&r, 0, sizeof r);
        pairs = (int32_t *)mxCalloc(2 * (N ? N : 1), sizeof(int32_t)); inl = (int32_t *)mxCalloc(N ? N : 1, sizeof(int32_t));
        rc = pre3_relocalise_seeded(g_ctx, nin > 8 ? mxGetScalar(in[8]) : 1.5, nin > 4 ? (int)mxGetScalar(in[4]) : 200, (uint64_t)mxGetScalar(in[1]), (uint64_t)mxGetScalar(in[2]),
                                    nin > 5 ? mxGetScalar(in[5]) : 2.0, nin > 7 ? (int)mxGetScalar(in[7]) : 1, nin > 6 ? (int)mxGetScalar(in[6]) : 12,
                                    mxGetPr(in[3]) /* (symmetric: row-major == column-major) */, nout > 0 ? &r : NULL, nout > 5 ? pairs : NULL, nout > 6 ? inl : NULL);
        if (rc == PRE3_OK) {
            if (nout > 0) { out[0] = mxCreateDoubleMatrix(3, 1, mxREAL); memcpy(mxGetPr(out[0]), r.u, sizeof(double) * 3); }
            if (nout > 1) { out[1] = mxCreateDoubleMatrix(4, 1, mxREAL); memcpy(mxGetPr(out[1]), r.u + 3, sizeof(double) * 4); }
            if (nout > 2) out[2] = mxCreateDoubleScalar(r.taken);
            if (nout > 3) out[3] = mxCreateDoubleScalar(r.pnp.sta);
            if (nout > 4) out[4] = mxCreateDoubleScalar(r.pnp.n_support);
            if (nout > 5) { out[5] = mxCreateDoubleMatrix(2, r.n_matches, mxREAL); for (i = 0; i < 2 * r.n_matches; ++i) mxGetPr(out[5])[i] = pairs[i] + 1; }
            if (nout > 6) { out[6] = mxCreateDoubleMatrix(1, r.n_corr, mxREAL); for (i = 0; i < r.n_corr; ++i) mxGetPr(out[6])[i] = inl[i]; }
            if (nout > 7) { out[7] = mxCreateDoubleMatrix(3, 3, mxREAL); for (i = 0; i < 3; ++i) for (k = 0; k < 3; ++k) mxGetPr(out[7])[i + 3 * k] = r.pnp.R[3 * i + k]; }
            if (nout > 8) { out[8] = mxCreateDoubleMatrix(3, 1, mxREAL); memcpy(mxGetPr(out[8]), r.pnp.T, sizeof(double) * 3); }
        }
        mxFree(pairs); mxFree(inl); check(rc);
    }
    else if (!strcmp(cmd, "ic_search")) {         /* [meas_idx, z, match_idx] = pre3_mex('ic_search', 1.5, strict)   matching_sift_based.m:104-149 */
        int N = pre3_get_map(g_ctx, NULL), i, rc; int32_t nm = 0, m = 0;
        int32_t *meas = (int32_t *)mxCalloc(N ? N : 1, sizeof(int32_t)), *pairs = (int32_t *)mxCalloc(3 * (N ? N : 1), sizeof(int32_t));
        double *z = (double *)mxCalloc(2 * (N ? N : 1), sizeof(double));
        rc = pre3_ic_search(g_ctx, mxGetScalar(in[1]), nin > 2 ? (int)mxGetScalar(in[2]) : 1, &nm, &m, meas, z, pairs);
        if (rc == PRE3_OK) {
            out[0] = mxCreateDoubleMatrix(1, m, mxREAL);
            for (i = 0; i < m; ++i) mxGetPr(out[0])[i] = meas[i] + 1;                       /* 1-based landmark numbers */
            if (nout > 1) { out[1] = mxCreateDoubleMatrix(2, m, mxREAL); memcpy(mxGetPr(out[1]), z, sizeof(double) * 2 * m); }
            if (nout > 2) { out[2] = mxCreateDoubleMatrix(2, nm, mxREAL);
                for (i = 0; i < nm; ++i) { mxGetPr(out[2])[2 * i] = pairs[3 * i] + 1; mxGetPr(out[2])[2 * i + 1] = pairs[3 * i + 1] + 1; } }
        }
        mxFree(meas); mxFree(pairs); mxFree(z); check(rc);
    }
    else if (!strcmp(cmd, "set_image")) {         /* pre3_mex('set_image', im (uint8, nRows x nCols)): the frame search_IC_matches.m:48-51's patch branch reads; with no argument: the
                                                     resident SR4000 frame's filtered image, converted on the device */
        if (nin == 1) {
            if (!g_sr) mexErrMsgTxt("pre3_mex('set_image'): without an image, call pre3_mex('sr_frame', ...) first");
            check(pre3_set_image_frame(g_ctx, g_sr));
        } else {
            if (mxGetClassID(in[1]) != mxUINT8_CLASS) mexErrMsgTxt("pre3_mex('set_image', im): im must be uint8");
            check(pre3_set_image(g_ctx, (int)mxGetM(in[1]), (int)mxGetN(in[1]), (const uint8_t *)mxGetData(in[1])));
        }
    }
    else if (!strcmp(cmd, "set_patches")) {       /* pre3_mex('set_patches', patches (uint8, 41 x 41 x k: [features_info.patch_when_initialized]), uv (2 x k), r_wc (3 x k),
                                                     R_wc (3 x 3 x k) [, first (0-based)]) */
        int k = (int)mxGetN(in[2]);
        if (nin < 5 || mxGetClassID(in[1]) != mxUINT8_CLASS || (int)mxGetNumberOfElements(in[1]) != 1681 * k || (int)mxGetNumberOfElements(in[3]) != 3 * k ||
            (int)mxGetNumberOfElements(in[4]) != 9 * k || (int)mxGetM(in[2]) != 2)
            mexErrMsgTxt("pre3_mex('set_patches', patches, uv, r_wc, R_wc [, first]): uint8 41 x 41 x k, 2 x k, 3 x k, 3 x 3 x k");
        check(pre3_set_patches(g_ctx, nin > 5 ? (int)mxGetScalar(in[5]) : 0, k, (const uint8_t *)mxGetData(in[1]), mxGetPr(in[2]), mxGetPr(in[3]), mxGetPr(in[4])));
    }
    else if (!strcmp(cmd, "patch_cut")) {         /* pre3_mex('patch_cut', uv (2 x k integer pixels, 1-based) [, first (0-based)]): add_feature_to_info_vector_my_version.m:33-41 */
        int k = (int)mxGetN(in[1]), i, rc;
        int32_t *uv = (int32_t *)mxCalloc(2 * (k ? k : 1), sizeof(int32_t));
        if ((int)mxGetM(in[1]) != 2) mexErrMsgTxt("pre3_mex('patch_cut', uv [, first]): uv is 2 x k");
        for (i = 0; i < 2 * k; ++i) uv[i] = (int32_t)mxGetPr(in[1])[i];
        rc = pre3_patch_cut(g_ctx, nin > 2 ? (int)mxGetScalar(in[2]) : 0, k, uv);
        mxFree(uv); check(rc);
    }
    else if (!strcmp(cmd, "patch_search")) {      /* [meas_idx, z, corr, ncand, status] = pre3_mex('patch_search', focal_over_d (cam.F / cam.dx) [, corr_threshold = 0.60 [, strict = 1]]):
                                                     search_IC_matches.m:31-51 on the patch branch (predict_features_appearance.m + matching.m) */
        int N = pre3_get_map(g_ctx, NULL), i, rc; int32_t m = 0;
        int32_t *meas = (int32_t *)mxCalloc(N ? N : 1, sizeof(int32_t)), *nc = (int32_t *)mxCalloc(N ? N : 1, sizeof(int32_t)), *st = (int32_t *)mxCalloc(N ? N : 1, sizeof(int32_t));
        double *z = (double *)mxCalloc(2 * (N ? N : 1), sizeof(double)), *corr = (double *)mxCalloc(N ? N : 1, sizeof(double));
        rc = pre3_patch_search(g_ctx, mxGetScalar(in[1]), nin > 2 ? mxGetScalar(in[2]) : 0.60, nin > 3 ? (int)mxGetScalar(in[3]) : 1, &m, meas, z, corr, nc, st);
        if (rc == PRE3_OK) {
            out[0] = mxCreateDoubleMatrix(1, m, mxREAL);
            for (i = 0; i < m; ++i) mxGetPr(out[0])[i] = meas[i] + 1;                       /* 1-based landmark numbers */
            if (nout > 1) { out[1] = mxCreateDoubleMatrix(2, m, mxREAL); memcpy(mxGetPr(out[1]), z, sizeof(double) * 2 * m); }
            if (nout > 2) { out[2] = mxCreateDoubleMatrix(1, N, mxREAL); memcpy(mxGetPr(out[2]), corr, sizeof(double) * N); }
            if (nout > 3) { out[3] = mxCreateDoubleMatrix(1, N, mxREAL); for (i = 0; i < N; ++i) mxGetPr(out[3])[i] = nc[i]; }
            if (nout > 4) { out[4] = mxCreateDoubleMatrix(1, N, mxREAL); for (i = 0; i < N; ++i) mxGetPr(out[4])[i] = st[i]; }
        }
        mxFree(meas); mxFree(nc); mxFree(st); mxFree(z); mxFree(corr); check(rc);
    }
    else if (!strcmp(cmd, "fast_detect")) {       /* [corners, scores] = pre3_mex('fast_detect', threshold [, barrier = 20 [, nonmax = 0 [, box = [r0 c0 rows cols] (0-based)]]]):
                                                     fast_corner_detect_9.m (nonmax = 0) / fast_nonmax.m (nonmax = 1) on the resident image or a rectangle of it; corners
                                                     K x 2 [x y], 1-based, relative to the rectangle.  The published segment test, not the reference's tree */
        int32_t K = 0, *uv = (int32_t *)mxCalloc(2 * PRE3_FAST_MAX_CORNERS, sizeof(int32_t)), *sc = (int32_t *)mxCalloc(PRE3_FAST_MAX_CORNERS, sizeof(int32_t));
        int box[4] = { 0, 0, 0, 0 }, i, rc;
        if (nin < 2) mexErrMsgTxt("pre3_mex('fast_detect', threshold [, barrier, nonmax, box])");
        if (nin > 4) { if (mxGetNumberOfElements(in[4]) != 4) mexErrMsgTxt("pre3_mex('fast_detect', ...): box is [r0 c0 rows cols]"); for (i = 0; i < 4; ++i) box[i] = (int)mxGetPr(in[4])[i]; }
        else { box[2] = g_cam_rows; box[3] = g_cam_cols; }
        rc = pre3_fast_detect(g_ctx, box[0], box[1], box[2], box[3], (int)mxGetScalar(in[1]), nin > 2 ? (int)mxGetScalar(in[2]) : 20, nin > 3 ? (int)mxGetScalar(in[3]) : 0, &K, uv, sc);
        if (rc == PRE3_OK) {
            out[0] = mxCreateDoubleMatrix(K, 2, mxREAL);
            for (i = 0; i < K; ++i) { mxGetPr(out[0])[i] = uv[2 * i]; mxGetPr(out[0])[K + i] = uv[2 * i + 1]; }
            if (nout > 1) { out[1] = mxCreateDoubleMatrix(K, 1, mxREAL); for (i = 0; i < K; ++i) mxGetPr(out[1])[i] = sc[i]; }
        }
        mxFree(uv); mxFree(sc); check(rc);
    }
    else if (!strcmp(cmd, "init_feature_fast")) { /* [uv, status, rho, xyz, centres] = pre3_mex('init_feature_fast', std_pxl, centres (2 x attempts: [row; column]) | [seed seq]
                                                     [, strict = 1 [, threshold = 10 [, barrier = 20]]]): initialize_a_feature.m:27-215 on the FAST branch with the
                                                     resident frame's depth; a 2 x 1 second argument is one centre, a 1 x 2 one is [seed seq].  uv is [] unless status is 0 */
        pre3_fast_init_result r; int i, rc, strict = nin > 3 ? (int)mxGetScalar(in[3]) : 1, thr = nin > 4 ? (int)mxGetScalar(in[4]) : -1, bar = nin > 5 ? (int)mxGetScalar(in[5]) : -1;
        if (nin < 3) mexErrMsgTxt("pre3_mex('init_feature_fast', std_pxl, centres | [seed seq] [, strict, threshold, barrier])");
        if (!g_sr) mexErrMsgTxt("pre3_mex('init_feature_fast'): call pre3_mex('sr_frame', ...) first");
        if (mxGetM(in[2]) == 1 && mxGetN(in[2]) == 2)
            rc = pre3_init_feature_fast_seeded(g_ctx, g_sr, mxGetScalar(in[1]), strict, thr, bar, (uint64_t)mxGetPr(in[2])[0], (uint64_t)mxGetPr(in[2])[1], &r);
        else {
            int32_t ce[2 * PRE3_FAST_MAX_ATTEMPTS]; int na = (int)mxGetN(in[2]);
            if (mxGetM(in[2]) != 2 || na < 1 || na > PRE3_FAST_MAX_ATTEMPTS) mexErrMsgTxt("pre3_mex('init_feature_fast', ...): centres is 2 x (1 .. 10)");
            for (i = 0; i < 2 * na; ++i) ce[i] = (int32_t)mxGetPr(in[2])[i];
            rc = pre3_init_feature_fast(g_ctx, g_sr, mxGetScalar(in[1]), strict, thr, bar, ce, na, &r);
        }
        check(rc);
        out[0] = mxCreateDoubleMatrix(r.status == PRE3_FAST_INITIALISED ? 2 : 0, r.status == PRE3_FAST_INITIALISED ? 1 : 0, mxREAL);
        if (r.status == PRE3_FAST_INITIALISED) { mxGetPr(out[0])[0] = r.uv[0]; mxGetPr(out[0])[1] = r.uv[1]; }
        if (nout > 1) out[1] = mxCreateDoubleScalar(r.status);
        if (nout > 2) out[2] = mxCreateDoubleScalar(r.rho);
        if (nout > 3) { out[3] = mxCreateDoubleMatrix(3, 1, mxREAL); memcpy(mxGetPr(out[3]), r.xyz, sizeof(double) * 3); }
        if (nout > 4) { out[4] = mxCreateDoubleMatrix(2, r.attempts, mxREAL); for (i = 0; i < 2 * r.attempts; ++i) mxGetPr(out[4])[i] = r.centres[i]; }
    }
    else if (!strcmp(cmd, "init_features_fast_all")) {   /* [uv, rho, verdict, n_added] = pre3_mex('init_features_fast_all', std_pxl [, threshold = 5 [, barrier = 20]]):
                                                            initialize_n_features_FAST.m:55-145 -- uv 2 x K of every maximum, verdict 0 = added */
        int32_t K = 0, n = 0, *uv = (int32_t *)mxCalloc(2 * PRE3_FAST_MAX_CORNERS, sizeof(int32_t)), *ver = (int32_t *)mxCalloc(PRE3_FAST_MAX_CORNERS, sizeof(int32_t));
        double *rho = (double *)mxCalloc(PRE3_FAST_MAX_CORNERS, sizeof(double));
        int i, rc;
        if (nin < 2) mexErrMsgTxt("pre3_mex('init_features_fast_all', std_pxl [, threshold, barrier])");
        if (!g_sr) mexErrMsgTxt("pre3_mex('init_features_fast_all'): call pre3_mex('sr_frame', ...) first");
        rc = pre3_init_features_fast_all(g_ctx, g_sr, mxGetScalar(in[1]), nin > 2 ? (int)mxGetScalar(in[2]) : -1, nin > 3 ? (int)mxGetScalar(in[3]) : -1, &K, &n, uv, rho, ver);
        if (rc == PRE3_OK) {
            out[0] = mxCreateDoubleMatrix(2, K, mxREAL);
            for (i = 0; i < 2 * K; ++i) mxGetPr(out[0])[i] = uv[i];
            if (nout > 1) { out[1] = mxCreateDoubleMatrix(1, K, mxREAL); memcpy(mxGetPr(out[1]), rho, sizeof(double) * K); }
            if (nout > 2) { out[2] = mxCreateDoubleMatrix(1, K, mxREAL); for (i = 0; i < K; ++i) mxGetPr(out[2])[i] = ver[i]; }
            if (nout > 3) out[3] = mxCreateDoubleScalar(n);
        }
        mxFree(uv); mxFree(ver); mxFree(rho); check(rc);
    }
    else if (!strcmp(cmd, "set_option")) {        /* pre3_mex('set_option', option, value): PRE3_OPT_DEFER_HI = 1, PRE3_OPT_K9_BF16X3 = 2, PRE3_OPT_CHOL_PERSIST = 3, PRE3_OPT_K9_OVERLAP = 5 (include/pre3.h) */
        check(pre3_set_option(g_ctx, (int)mxGetScalar(in[1]), (int)mxGetScalar(in[2])));
    }
    else if (!strcmp(cmd, "destroy")) { at_exit(); if (mexIsLocked()) mexUnlock(); }
    else mexErrMsgTxt("pre3_mex: unknown command");
}
