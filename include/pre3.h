/*
 * pre3.h -- C ABI of libpre3.so: the MI355X (gfx950) implementation of the per-step hot path of
 * the MATLAB 1-point-RANSAC EKF-SLAM reference ahtamjidi/3PRE.
 *
 * The reference's only native plug-in boundary is the MATLAB MEX interface
 * (matlab_code/sift/siftmatch.c:139-141 `mexFunction`; Coder variant
 * matlab_code/mex_files/CorePar_Ver1/codegen/mex/corrcoef_partitioned/corrcoef_partitioned_mex.c:50-57).
 * A MEX file named like an .m function shadows it, so each entry point below states the .m (or .c)
 * function it replaces; mex/ holds the gateways and INTEGRATION.md the binding recipe.
 *
 * Conventions
 *   - plain C, no C++/torch types; every function returns 0 on success or a negative pre3_status;
 *     pre3_last_error() gives the message of the calling thread's last failure.  Nothing exits or throws.
 *   - host arrays are caller-owned `double`, MATLAB (column-major) order unless stated; the covariance is
 *     symmetric so its orientation does not matter.  Indices crossing the ABI are 0-based int32
 *     (the MEX gateways convert from MATLAB's 1-based doubles).
 *   - a pre3_ctx owns device-resident filter state (x, P, landmark table, per-landmark h/H/S/z/flags) on
 *     ONE GPU and one HIP stream; calls on one ctx must be serialised by the caller (MATLAB's
 *     interpreter thread does); different contexts are independent.
 *   - dtype selects the storage/compute type of the dense covariance path (P, H*P, S, Cholesky, the
 *     MFMA down-date): PRE3_F64 or PRE3_F32.  The state vector, camera geometry, Jacobians, innovations
 *     and gates are always evaluated in fp64.
 *   - there is no CPU fallback: without a HIP device every call fails with PRE3_E_NODEVICE.
 */
#ifndef PRE3_H
#define PRE3_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PRE3_API __attribute__((visibility("default")))

typedef struct pre3_ctx pre3_ctx;

typedef enum {
    PRE3_OK = 0,
    PRE3_E_ARG = -1,        /* bad argument / shape mismatch (the MEX gateways map this to mexErrMsgTxt) */
    PRE3_E_NODEVICE = -2,   /* no HIP device / HIP runtime failure at init */
    PRE3_E_HIP = -3,        /* a HIP call or kernel failed */
    PRE3_E_STATE = -4,      /* call order violated (e.g. update before predict/project) */
    PRE3_E_NUMERIC = -5,    /* S not positive definite */
    PRE3_E_NOMEM = -6,
    PRE3_E_COMM = -7        /* RCCL: library not found, communicator creation failed, or a collective reported an error */
} pre3_status;

enum { PRE3_F64 = 0, PRE3_F32 = 1 };
enum { PRE3_INVDEPTH = 0, PRE3_CARTESIAN = 1 };   /* features_info(i).type */
enum { PRE3_X_K_K = 0, PRE3_X_K_KM1 = 1 };        /* which estimate (ekf_filter.m:63-87 fields) */

/* cam struct fields used by the path (initialize_cam.m:69-78) */
typedef struct { double f, Cx, Cy, k1, k2, nRows, nCols; } pre3_cam;

PRE3_API const char *pre3_last_error(void);
PRE3_API int pre3_device_count(void);
PRE3_API const char *pre3_version(void);

/* ---- context ----------------------------------------------------------------------------------- */

/* device = HIP ordinal; max_landmarks / max_hyp size the device buffers once (no allocation afterwards). */
PRE3_API int pre3_create(pre3_ctx **out, int device, int dtype, int max_landmarks, int max_hyp);
PRE3_API int pre3_destroy(pre3_ctx *ctx);
PRE3_API int pre3_sync(pre3_ctx *ctx);                       /* wait for the ctx stream */
PRE3_API int pre3_set_cam(pre3_ctx *ctx, const pre3_cam *cam);

/* Landmark table = [features_info.type] in state order (add_feature_to_info_vector_my_version_sift.m:37-60).
 * Resets all per-landmark fields (h, H, S, z, flags), as update_features_info.m:30-44 does each step. */
PRE3_API int pre3_set_map(pre3_ctx *ctx, int N, const int32_t *lm_type);
PRE3_API int pre3_state_size(pre3_ctx *ctx);                 /* n = 13 + 6*N_id + 3*N_euc */

/* x(n), P(n x n) -> device as x_k_k / p_k_k (set_x_k_k.m / set_p_k_k.m), or as x_k_km1 / p_k_km1. */
PRE3_API int pre3_set_state(pre3_ctx *ctx, int which, int n, const double *x, const double *P);
PRE3_API int pre3_get_state(pre3_ctx *ctx, int which, int n, double *x, double *P);   /* P may be NULL */

/* ---- marginals without fetching P -------------------------------------------
 * Both readers follow pre3_get_state's rules: which = PRE3_X_K_K or PRE3_X_K_KM1; the other estimate in the covariance buffer is PRE3_E_STATE;
 * the device's error words are read (as pre3_get_state does); a deferred HI update (PRE3_OPT_DEFER_HI) is completed first -- the landmarks
 * include it, and x_k_k is final only after it.  A range or index outside the map is PRE3_E_ARG, checked on the host before anything is
 * launched.  N = 0: pre3_get_landmarks returns PRE3_OK and writes nothing; pre3_get_marginal still reads the pose (n = 13), as
 * pre3_get_state does.  Synchronous; one gather launch and one device-to-host copy.
 * Unlike every other entry point they do NOT complete a pending HI down-date (PRE3_OPT_PEND_HI) or its pending rows / columns 3..6 pass:
 * the values returned are those of P - W~'W~ (and of that pass), computed by the reading launch itself, and the filter's next step runs
 * exactly as it would have without the read. */

/* plots_complete.m:208-237, inversedepth2cartesian.m, inversedepth_2_cartesian.m:36-62: the map as a set of 3-D points with
 * their uncertainty, for landmarks first .. first+count-1 at the chosen estimate.  Any output may be NULL.
 *   xyz[3*count]         inverse depth: y(1:3) + m(theta,phi)/rho; Cartesian: the state's 3 entries
 *   cov_xyz[9*count]     3x3, J * P_ii * J' with J = [I3, dm_dtheta/rho, dm_dphi/rho, -m/rho^2] (inversedepth_2_cartesian.m:58-62); Cartesian: P_ii
 *   cov_native[36*count] the landmark's own block of P, 6x6; Cartesian: 3x3 in the top-left corner, the rest 0
 *   linearity[count]     inversedepth_2_cartesian.m:36-49's index (camera position x(1:3) of the same estimate); -1 for Cartesian
 * Matrices row-major (all are symmetric).  Synchronous.  Does NOT apply a pending HI down-date to P: the blocks are those of
 * P - W~'W~, computed by the reading launch itself. */
PRE3_API int pre3_get_landmarks(pre3_ctx *ctx, int which, int first, int count,
                                double *xyz, double *cov_xyz, double *cov_native, double *linearity);

/* The state entries x[idx] and the marginal covariance P[idx, idx] (k x k, row-major) for any index set: the pose is
 * idx = 0..6, a landmark's block is its offset .. offset+5, and pose-landmark cross terms are any mix of the two.
 * Indices need not be sorted and may repeat.  x_out / P_out may be NULL.  Same pending rule as above.  Meant for small sets
 * (16 x 16 output tiles); any k works, the staging buffer grows with it (8 k^2 bytes). */
PRE3_API int pre3_get_marginal(pre3_ctx *ctx, int which, int k, const int32_t *idx, double *x_out, double *P_out);

/* ---- a2: predict_state_and_covariance.m:27-143 (called by @ekf_filter/ekf_prediction.m:29) ------ */
/* u = [dX(3); dq(4)], the visual-odometry increment the reference reads through fv.m:47.
 * (x_k_k, p_k_k) -> (x_k_km1, p_k_km1); the covariance is transformed IN PLACE (only rows/cols 4:7
 * and the 7x7 pose block change), so p_k_k is no longer available afterwards. */
PRE3_API int pre3_predict(pre3_ctx *ctx, const double u[7]);

/* The camera-only prediction the fork left in place and switched off: (x_k_k, p_k_k) -> (x_k_km1, p_k_km1) without a u, from
 * the v and omega the state carries.  State functions fv.m:64-87 and the commented original :98-106; F = dfv_by_dxv (predict_state_and_covariance.m:82,
 * dfv_by_dxv.m:38-116); Q = func_Q = G Pn G' (:127, func_Q.m:41-54) with Pn = diag((sigma_a dt)^2 [1 1 1], (sigma_alpha dt)^2 [1 1 1]) (:89-90,
 * :103-104); the covariance assembly and the quaternion's normalisation are :129-143 as they stand.  dt is the reference's delta_t (:35: 0.1).
 *   type 0 constant_velocity                    x = [r + v dt; q (x) v2q(omega dt); v; omega]
 *   type 1 constant_orientation                 x = [r + v dt; q; v; 0]
 *   type 2 constant_position                    x = [r; q (x) v2q(omega dt); 0; omega]
 *   type 3 constant_position_and_orientation    x = [r; q; 0; 0]
 * F and G are the reference's for each type: the blocks dfv_by_dxv.m:51-66 zeroes, and no others -- F(4:7,4:7) = dq3_by_dq2(v2q(omega dt)) in all four.
 * Not built: constant_position_and_orientation_location_noise (its G goes through dq_by_deuler(tr2rpy(q2tr(q))), func_Q.m:29-37).
 * One deviation: at |omega| = 0 the reference's dqomegadt_by_domega is 0/0 (it relies on the prior w_0 = 1e-15, initialize_x_and_p.m:29-32); here the
 * limit is taken -- row 1 zero, dt/2 on the diagonal of rows 2:4.  pre3_predict and the steps leave exactly that omega behind.
 * The covariance is transformed IN PLACE (rows/cols 1:13 change), one launch.  PRE3_E_ARG, with nothing queued and the context as it was, for a type
 * outside 0..3, a dt that is not finite and positive, a sigma that is negative or not finite; PRE3_E_STATE as pre3_predict. */
#define PRE3_CV_CONSTANT_VELOCITY 0
#define PRE3_CV_CONSTANT_ORIENTATION 1
#define PRE3_CV_CONSTANT_POSITION 2
#define PRE3_CV_CONSTANT_POSITION_AND_ORIENTATION 3
PRE3_API int pre3_predict_cv(pre3_ctx *ctx, int type, double dt, double sigma_a, double sigma_alpha);

/* Stateless drop-in for `[X_km1_k, P_km1_k] = predict_state_and_covariance(X_k, P_k, type, SD_A_component_filter,
 * SD_alpha_component_filter)` (predict_state_and_covariance.m:27, caller @ekf_filter/ekf_prediction.m:29): host in, host out.
 * `type` is 'constant_velocity' in every call of the reference and the two standard deviations are unused by this fork (:98-102 hard-
 * code Pn); the increment u = [dX; dq] the .m file reads from disk through fv.m:47 is an explicit argument (the MEX gateway resolves it,
 * INTEGRATION.md).  n = 13 + 6 N_id + 3 N_euc; P, P_out: n x n.
 * The device context behind this entry (P at capacity and the work buffers) is kept between calls, one per (device, dtype), grown when a larger
 * state arrives; calls are serialised on it; pre3_release_scratch() frees it. */
PRE3_API int pre3_predict_dense(int device, int dtype, int n, const double *x, const double *P, const double u[7], double *x_out, double *P_out);

/* ---- a3/a4: predict_camera_measurements.m:27-68 + calculate_derivatives.m:27-60 ------------------ */
/* Projects every landmark at the chosen estimate and linearises it (compact H_i = 2x7 pose block +
 * 2x6 landmark block; columns 8:13 of the reference's H are zero).  clear_first=1 empties h/H first
 * (the state search_IC_matches.m:31 sees after update_features_info.m:40); clear_first=0 keeps the
 * previous h of landmarks that are not predicted now (rescue_hi_inliers.m:32-33, quirk Q7). */
PRE3_API int pre3_project(pre3_ctx *ctx, int which, int clear_first);

/* ---- a5: search_IC_matches.m:33-44: S_i = H_i P H_i' + R_i (R_i = eye(2)) for predicted landmarks */
PRE3_API int pre3_innovation(pre3_ctx *ctx);

/* read back per-landmark fields (any pointer may be NULL): h[2N], has_h[N], Hc[14N] (2x7 row-major),
 * Hl[12N] (2x6 row-major), S[4N] */
PRE3_API int pre3_get_landmark_fields(pre3_ctx *ctx, double *h, int32_t *has_h, double *Hc, double *Hl, double *S);

/* matching_sift_based.m:119-134 window gate.  Candidate c pairs the k1[c]-th PREDICTED landmark (the
 * L1 column siftmatch matched) with pixel zc[2c..2c+1]; accepted candidates become individually
 * compatible and get z.  strict_reference=1 reproduces quirk Q5 (S of the c-th predicted landmark).
 * accept_out[M] may be NULL. */
PRE3_API int pre3_window_gate(pre3_ctx *ctx, int M, const int32_t *k1, const double *zc, int strict_reference,
                              int32_t *accept_out);

/* Direct form: landmarks meas_idx[m] (ascending) are individually compatible with pixels z[2m]
 * (what matching_sift_based.m:131-134 leaves in features_info). */
PRE3_API int pre3_set_measurements(pre3_ctx *ctx, int m, const int32_t *meas_idx, const double *z);

/* ---- a6-a8: ransac_hypotheses.m:27-85 ----------------------------------------------------------- */
/* hyp[n_draw*k]: per hypothesis k positions in the individually-compatible list (what
 * select_random_match.m:40-51 draws with randperm; MATLAB's legacy RNG stream is not reproducible,
 * so the draws are an input).  early_exit=1 replays the reference's adaptive termination (quirk Q1)
 * over the supports; 0 uses all n_draw.  [hyp_begin, hyp_end) restricts the hypotheses THIS context
 * scores (multi-GPU sharding, see pre3_ransac_score / pre3_ransac_select).
 * Outputs (may be NULL): support[n_draw] (int32; -1 for hypotheses after the exit point),
 * li_mask[m] (int32 0/1 in measurement order), stats[4] = {best, iterations, n_hyp, max_support}. */
PRE3_API int pre3_ransac(pre3_ctx *ctx, int n_draw, int k, const int32_t *hyp, double threshold, int early_exit,
                         int32_t *support, int32_t *li_mask, int32_t stats[4]);

/* Stateless drop-in for `[hypothesis_support, positions_li_inliers_id, positions_li_inliers_euc] =
 * compute_hypothesis_support_fast(xi, cam, state_vector_pattern, z_id, z_euc, threshold)` (compute_hypothesis_support_fast.m:27,
 * called from ransac_hypotheses.m:72): host in, host out.  xi: hypothesis state (n); state_vector_pattern: n x 4 column-major
 * 0/1 doubles exactly as generate_state_vector_pattern.m:29-53 builds it (columns: inverse-depth position / angles / rho, cartesian
 * xyz -- xi(logical(pattern(:,c))) is taken in state order); z_id: 2 x n_id, z_euc: 2 x n_euc column-major.  Inverse-depth rule
 * residual < min(residual) + threshold (:70), cartesian rule residual < threshold (:109); the quaternion is used un-normalised (:46).
 * positions_*: int32 0/1 per measurement (may be NULL).  A pattern whose counts do not match n_id / n_euc is PRE3_E_ARG
 * (MATLAB's reshape at :40 fails there too). */
PRE3_API int pre3_hypothesis_support(int device, int n, const double *xi, const pre3_cam *cam, const double *state_vector_pattern,
                                     int n_id, const double *z_id, int n_euc, const double *z_euc, double threshold,
                                     int32_t *support_out, int32_t *positions_li_inliers_id, int32_t *positions_li_inliers_euc);

/* Sharded form: score hypotheses [hyp_begin,hyp_end) only, leaving their supports (int32, others 0)
 * and inlier bitmasks in device buffers; *support_dev / *mask_dev receive DEVICE pointers to
 * int32[n_draw] and uint32[n_draw * mask_words] so the caller can all-reduce them (RCCL) in place;
 * pre3_ransac_select then replays the termination rule on the (reduced) buffers. */
PRE3_API int pre3_ransac_score(pre3_ctx *ctx, int n_draw, int k, const int32_t *hyp, double threshold,
                               int hyp_begin, int hyp_end, void **support_dev, void **mask_dev, int *mask_words);
PRE3_API int pre3_ransac_select(pre3_ctx *ctx, int n_draw, int k, int early_exit,
                                int32_t *support, int32_t *li_mask, int32_t stats[4]);
/* Copy the context's support / mask buffers to (export) or from (import) caller-owned DEVICE buffers of
 * int32[n_draw] and uint32[n_draw*mask_words] -- e.g. torch tensors handed to an RCCL all-reduce.  Either
 * pointer may be NULL.  Synchronous on return. */
PRE3_API int pre3_ransac_export(pre3_ctx *ctx, int n_draw, void *support_dst_dev, void *mask_dst_dev);
PRE3_API int pre3_ransac_import(pre3_ctx *ctx, int n_draw, const void *support_src_dev, const void *mask_src_dev);

/* ---- a9: update.m:27-56 via the @ekf_filter wrappers --------------------------------------------- */
/* ekf_update_li_inliers.m:45-58: prior (x_k_km1,p_k_km1), rows = low-innovation inliers */
PRE3_API int pre3_update_li(pre3_ctx *ctx);
/* rescue_hi_inliers.m:29-47: re-project + re-linearise at x_k_k, chi-square gate (no +R, quirk Q6).
 * hi_mask[m] (may be NULL) in measurement order. */
PRE3_API int pre3_rescue(pre3_ctx *ctx, double chi2, int32_t *hi_mask);
/* ekf_update_hi_inliers.m:45-58: prior (x_k_k,p_k_k), rows = high-innovation inliers */
PRE3_API int pre3_update_hi(pre3_ctx *ctx);
/* ekf_update_all.m:46-62 ('PURE_EKF'): prior km1, rows = all individually compatible landmarks */
PRE3_API int pre3_update_all(pre3_ctx *ctx);
/* read/force the per-measurement flags: li/hi[m] int32 in measurement order (NULL = leave) */
PRE3_API int pre3_get_flags(pre3_ctx *ctx, int32_t *li, int32_t *hi);
PRE3_API int pre3_set_flags(pre3_ctx *ctx, const int32_t *li, const int32_t *hi);

/* One whole filter step of mono_slam.m:153-187 ('1PRE'): predict, project+linearise, S_i,
 * [measurements given], RANSAC, LI update, rescue, HI update -- enqueued back to back on the ctx
 * stream.  stats[8] = {best, iterations, n_hyp, max_support, n_li, n_hi, 0, 0} (may be NULL). */
PRE3_API int pre3_step(pre3_ctx *ctx, const double u[7], int m, const int32_t *meas_idx, const double *z,
                       int n_draw, int k, const int32_t *hyp, double threshold, int early_exit, double chi2,
                       int32_t stats[8]);

/* mono_slam.m:178-187 -- RANSAC, LI update, rescue, HI update -- behind a prediction and an IC search the caller has already run on the
 * context (pre3_predict, then pre3_ic_search or pre3_project + pre3_innovation + pre3_set_measurements): the measurements are the installed
 * ones, the launches are pre3_step's (the persistent factorisation with the down-date inside, the device-driven HI update), none of them
 * sized by a host poll.  stats as pre3_step.  This is what a frame loop that matches on the device calls instead of pre3_step. */
/* mono_slam.m:153-162 + :199, the 'PURE_EKF' branch (config_file.m:21, EST_METHOD): prediction, projection / Jacobians / S_i of every landmark
 * and ONE update with all individually compatible measurements (@ekf_filter/ekf_update_all.m:46-62) as one call -- the same arithmetic as
 * pre3_predict + pre3_project + pre3_innovation + pre3_set_measurements + pre3_update_all, four launches fewer.  meas_idx strictly ascending. */
PRE3_API int pre3_step_all(pre3_ctx *ctx, const double u[7], int m, const int32_t *meas_idx, const double *z /* [2 m] */);
PRE3_API int pre3_step_predicted(pre3_ctx *ctx, int n_draw, int k, const int32_t *hyp, double threshold, int early_exit, double chi2,
                                 int32_t stats[8]);

/* ---- update.m:27-56 on the resident current estimate ----------------------------------------------------------------------
 * Both calls act IN PLACE on (x_k_k, p_k_k), which the covariance buffer must hold (after pre3_predict and before an update it holds the prediction:
 * PRE3_E_STATE).  Arguments are checked on the host before anything is launched (PRE3_E_ARG); the deferred HI update and a pending HI down-date
 * (PRE3_OPT_DEFER_HI / PRE3_OPT_PEND_HI) are completed first, as every entry point but the marginal readers does.  Nothing else of the context changes
 * (flags, per-landmark fields, map, descriptors, options); the next pre3_step predicts from the updated estimate.  S not positive definite: x and P are
 * left untouched and the device's error word is set -- the next call that reads the error words (pre3_get_state, the marginal readers, the next step's
 * collection) returns PRE3_E_NUMERIC.  Asynchronous unless stated.  Up to 16 rows: two launches, P swept once (PRE3_OPT_ROWS_FORM = 1). */
/* update.m:27-56 on the resident current estimate (x_k_k, p_k_k), in place: r rows in pre3_update_ell's ELL form
 * (row a: nnz[a] <= width <= 16 entries col[a*width+t], val[...]), R r x r dense (row-major) or NULL for eye(r), z[r], h[r].
 * r == 0 changes nothing (update.m:50-55).  r above the context's row capacity, a row with more than 16 non-zeros, a column outside [0, n): PRE3_E_ARG.
 * More than 16 rows take the general update route (PRE3_OPT_ROWS_FORM = 0). */
PRE3_API int pre3_update_rows(pre3_ctx *ctx, int r, int width, const int32_t *nnz, const int32_t *col, const double *val,
                              const double *R, const double *z, const double *h);
/* @ekf_filter/ekf_heading_update.m:27-52: z = R_plane(:,2); h, H from the resident quaternion x_k_k(4:7); RR from R_plane; the angle gate.
 * R_plane 3 x 3 column-major (as MATLAB passes it).  applied_out (may be NULL; non-NULL synchronises): 1 = updated, 0 = the gate returned.
 * The gate is evaluated on the device.  strict_reference = 1 reproduces the reference's gate (quirk Q12: `if a > 4` on find_angle_bw_2_vecs' seven
 * angles returns only when ALL of them exceed 4 degrees); 0 returns when the angle between z and h exceeds 4 degrees.  With applied_out the call
 * reads the device's error words itself: an S that was not positive definite (this call's or an earlier one's) is reported here (PRE3_E_NUMERIC,
 * *applied_out = 0) -- once: the words are cleared with the report, as the step's HI collection clears them. */
PRE3_API int pre3_heading_update(pre3_ctx *ctx, const double R_plane[9], int strict_reference, int32_t *applied_out);

/* ---- the floor-plane fit that produces R_plane (plane_fit_to_data.m) --------------------------------------------------------
 * plane_fit_to_data.m:13-149 over ransacfitplane.m:51-116, ransac.m:113-225, fitplane.m:31-54, plane_imp_line_par_int_3d.m:56-100: the SR4000 range
 * image in camera coordinates (x = -x_sr, y = -y_sr, z = z_sr), cropped to a box and stacked column-major; a 3-point RANSAC with inlier distance t,
 * p = 0.99 and at most 1001 trials; a least-squares plane on the winner's inliers; the sign rule; R from the plane's normal and the intersections of
 * the plane with the rays through the box's centre point and the point 20 rows above it.  MATLAB's random stream cannot be reproduced: the draws are an
 * input (the caller applies ransac.m:142-176's rejection rule, 3pre_amd/plane.py: draw_plane_hypotheses).  A collinear or repeated draw is not an
 * error: it scores 0 and counts as a trial (ransac.m:170-184 once the redraws are used up). */
#define PRE3_PLANE_MAX_DRAWS 1001
typedef struct pre3_plane_result {
    double B[4];            /* the plane B(1) x + B(2) y + B(3) z + B(4) = 0, unit 4-vector, after the sign rule of plane_fit_to_data.m:56-58 */
    double R[9];            /* column-major, as plane_fit_to_data returns it: columns x_axis, z_axis (the normal), y_axis; zeros unless sta is 1 or 2 */
    double p_orig[3], p_ray[3];
    double N;               /* ransac.m's N when the loop ended */
    int32_t sta;            /* 1 ok; 0 no trial had an inlier (ransac.m:224; B = 0); 2 the rule wanted more trials than n_draw (the result is that of
                               the n_draw trials); 3 the axes are undefined (a ray parallel to the plane, or a zero y_axis; B is valid);
                               5 (the *_frame forms only) a coordinate inside the box of the resident frame is not finite: nothing was drawn, scored
                               or fitted -- B = R = p_orig = p_ray = N = 0, n_inliers = n_trials = 0, best = -1 */
    int32_t n_inliers, n_trials, best;   /* best 0-based: the first trial with the largest score; -1 when sta == 0 */
} pre3_plane_result;
/* x_sr, y_sr, z_sr: rows x cols column-major, SR4000 coordinates.  box = {row0, row1, col0, col1}, 1-based inclusive (NULL: {80, 144, 50, 120},
 * plane_fit_to_data.m:17-18).  draws[n_draw][3]: 0-based positions in the cropped, column-major point list.  count_out[n_draw] (the scores of ALL
 * draws, also those behind the stopping rule), inlier_out[npts] (the winner's mask): optional.  Only the box crosses PCIe.
 * PRE3_E_ARG before anything is launched: a null pointer, a box outside the image or with fewer than 3 points, a box of fewer than 40 rows (p_ray's row
 * lies outside it), a draw outside [0, npts), n_draw outside [1, PRE3_PLANE_MAX_DRAWS], t <= 0, a non-finite coordinate inside the box. */
PRE3_API int pre3_plane_fit(int device, int rows, int cols, const double *x_sr, const double *y_sr, const double *z_sr,
                            const int32_t *box, double t, int n_draw, const int32_t *draws,
                            int32_t *count_out, int32_t *inlier_out, pre3_plane_result *res);
/* The same fit on the context's stream, then ekf_heading_update.m:27-52 with R_plane = R' (transpose = 1, what mono_slam.m:192 passes) or R (0), in
 * stream order: z, RR and the fit's status stay on the device and the heading rows read them there, nothing is read back in between.  sta != 1: no
 * update (applied = 0), x and P untouched.  State, gate (strict_reference) and error words as pre3_heading_update.  applied_out / res_out may be
 * NULL; with both NULL the call does not synchronise. */
PRE3_API int pre3_heading_from_scan(pre3_ctx *ctx, int rows, int cols, const double *x_sr, const double *y_sr, const double *z_sr,
                                    const int32_t *box, double t, int n_draw, const int32_t *draws, int transpose,
                                    int strict_reference, int32_t *applied_out, pre3_plane_result *res_out);
/* measurement only: average device time of one fit (upload of the box from pinned memory + both launches) over reps calls */
PRE3_API int pre3_plane_bench(int device, int rows, int cols, const double *x_sr, const double *y_sr, const double *z_sr,
                              const int32_t *box, double t, int n_draw, const int32_t *draws, int reps, double *ms_per_call);

/* Stateless drop-in for `[x,P,K] = update(x,P,H,R,z,h)` (update.m:27): host in, host out.
 * H is r x n given by rows in ELL form: row a has nnz[a] <= width entries (col[a*width+t], val[...]);
 * R is r x r dense or NULL for eye(r) (every caller in the reference passes eye).  K_out (n x r,
 * column-major) may be NULL.  r == 0 returns the inputs (update.m:50-55). */
PRE3_API int pre3_update_ell(int device, int dtype, int n, int r, const double *x, const double *P, int width,
                             const int32_t *nnz, const int32_t *col, const double *val, const double *R,
                             const double *z, const double *h, double *x_out, double *P_out, double *K_out);

/* Options.  PRE3_OPT_DEFER_HI = 1: pre3_step returns as soon as the rescue stage is enqueued; the HI count is polled and the HI
 * update (ekf_update_hi_inliers.m) launched by the NEXT call on the context (any entry point: step, get_state, sync ...), so the
 * caller's own time between two steps overlaps the device's rescue stage.  Results are identical; stats[5] of pre3_step then
 * reports the previous step's HI count and stats[7] = 1 says so.  Default 0: pre3_step completes the HI update itself. */
#define PRE3_OPT_DEFER_HI 1
/* PRE3_OPT_K9_BF16X3 (fp32 contexts; default 1, or the environment's PRE3_K9_B3): the covariance down-date of update.m:38-46,
 * P <- P - W'W, multiplies on the bf16 matrix cores: every f32 entry of W is split exactly into three bf16 values and six of
 * the nine partial products are accumulated in f32 (the dropped ones are below f32 rounding), 16/6 of the f32 matrix rate at
 * f32 accuracy.  0: plain f32 MFMA (bitwise an fmaf chain).  No effect on fp64 contexts. */
#define PRE3_OPT_K9_BF16X3 2
/* PRE3_OPT_CHOL_PERSIST (fp32 contexts with PRE3_OPT_K9_BF16X3; default 1, or the environment's PRE3_CHOL_FORM): update.m:32-33 -- the
 * factorisation of S and W = L^-1 [HP | nu] -- as ONE persistent launch (pre3_cholp.hip) for updates of up to 13 x 64 rows;
 * 0: one launch per 64-column panel (the form every fp64 context and every larger update uses).  get: whether the form is in effect. */
#define PRE3_OPT_CHOL_PERSIST 3
/* PRE3_OPT_IC_RANKED (read only): 1 if the last pre3_ic_search ran matching_sift_based.m:118's siftmatch on the matrix cores (bf16 distance
 * GEMM ranks + exact re-evaluation; N * K2 >= 65536 and every descriptor inside the route's bounds), 0 if it took the exact VALU kernel.
 * The environment's PRE3_IC_RANK=0 forces the latter.  Results are bit-identical either way. */
#define PRE3_OPT_IC_RANKED 4
/* PRE3_OPT_K9_OVERLAP (fp32 contexts with PRE3_OPT_CHOL_PERSIST; default 1, or the environment's PRE3_K9_OVERLAP): update.m:37's
 * P - K*S*K' = P - sum_J W_J'W_J is accumulated panel by panel INSIDE the persistent factorisation's launch, by workgroups on the CUs that
 * launch leaves idle (as many tile groups as there are CUs left; the rest, if any, in the launch that follows).  0: the down-date only
 * starts when the factorisation has finished.  Results are bit-identical either way. */
#define PRE3_OPT_K9_OVERLAP 5
/* PRE3_OPT_STEP_TAIL (fp32 contexts with PRE3_OPT_K9_OVERLAP; default 0, or the environment's PRE3_TAIL): inside pre3_step / pre3_step_predicted
 * the rescue stage (rescue_hi_inliers.m:29-47) and the HI update of up to 32 rescued landmarks (ekf_update_hi_inliers.m:45-58, update.m:27-48) run
 * INSIDE the LI update's persistent launch: the rescued landmarks' rows are one more panel of the same block factorisation, P is read and written
 * once per step (P - W'W - W~'W~), and update.m:42-46 of both updates is one rows / columns 3..6 pass with the product of the two normalisation
 * Jacobians, carried by the next prediction's launch.  Same inlier sets; x / P agree with the call-by-call sequence to fp32 rounding (the
 * intermediate P_LI is never rounded to fp32).  0 (default): the rescue stage and the HI update as launches of their own -- on MI355X the
 * in-launch form's hand-offs between workgroups cost what the second sweep of P saves (DESIGN.md section 5d has the measured timeline).
 * pre3_get_option returns the setting; whether a step used it also depends on the launch carrying every tile of P (one live fp32 context). */
#define PRE3_OPT_STEP_TAIL 6
/* PRE3_OPT_IC_ROUTE (read only): how the last pre3_ic_search matched -- 2: the fused small-problem route (N * K2 <= 2^20 pairs, N <= 4096, K2 <= 2048:
 * the sizes of the reference's own runs): siftmatch.c:97-116 exactly on 32 x 32 pair tiles over every landmark of the map, then ONE workgroup that
 * stacks the predicted landmarks, merges the tiles, applies Lowe's test and the window gate, refreshes the accepted landmarks' descriptors and
 * writes the result block into host memory -- two launches; 1: the ranked route of PRE3_OPT_IC_RANKED; 0: the exact 64 x 64 tiled kernel.
 * The environment's PRE3_IC_FUSED=0 disables route 2.  Results are bit-identical on all three. */
#define PRE3_OPT_IC_ROUTE 7
/* PRE3_OPT_PEND_HI (fp32 contexts with PRE3_OPT_K9_OVERLAP; default: the environment's PRE3_PEND_HI, else 0): inside pre3_step the covariance down-date of
 * the HI update (update.m:37-38 as ekf_update_hi_inliers.m:58 calls it) is not launched behind the update; P - W~'W~ stays PENDING across the step
 * boundary: the next pre3_step's prediction transforms W~ with P, its H*P / S_i launch subtracts (H W~')W~, and the consumers of its LI update's
 * persistent launch take W~ as the panels in front of panel 0 -- P is read and written ONCE per step instead of twice.  Every other call on the
 * context (and every path of pre3_step that cannot take the pending rows) first runs the down-date as the launch it would have been.  The same
 * arithmetic except that P between the two updates is never rounded to fp32: results agree with the default form to fp32 rounding, not to the bit. */
#define PRE3_OPT_PEND_HI 8
/* PRE3_OPT_ROWS_FORM (read only): the form the last pre3_update_rows / pre3_heading_update took -- 1: the single-sweep small-rank form (r <= 16 rows,
 * two launches, P read and written once); 0: the general update route (H*P, S, panel factorisation, down-date, Jnorm pass).
 * Chosen from r alone. */
#define PRE3_OPT_ROWS_FORM 9
PRE3_API int pre3_set_option(pre3_ctx *ctx, int option, int value);
PRE3_API int pre3_get_option(pre3_ctx *ctx, int option, int *value_out);

/* ---- map management on the device (map_management.m:27-79) ----------------------------- */
/* These act on (x_k_k, p_k_k) between steps, as map_management.m:140 does, and keep P resident: P <- A P A' (+D) with
 * a sparse A (selection rows / the 6x13 and 3x6 Jacobians of the reference), evaluated by two gather passes through a
 * second ld x ld buffer (allocated on first use).  Per-landmark fields (h, H, S, z, flags) are cleared afterwards,
 * as update_features_info.m:30-44 does.  These calls take the POLICY (which landmarks to delete, which pixels to initialise)
 * from the caller, as delete_features.m:31-52 / initialize_features.m decide it; pre3_map_policy below decides it on the device. */
/* delete_features.m:54-74 -> delete_a_feature.m:47-51: remove landmarks del_idx[n_del] (ascending, 0-based). */
PRE3_API int pre3_map_delete(pre3_ctx *ctx, int n_del, const int32_t *del_idx);
/* add_features_inverse_depth.m:27-47 (hinv_my_version.m:26-53 + add_a_feature_covariance_inverse_depth.m:27-90):
 * append n_new inverse-depth landmarks observed at distorted pixels uvd[2*n_new] with initial inverse depths
 * initial_rho[n_new]; std_rho = initial_rho^2 * 0.01 as the reference hard-codes (:41). */
PRE3_API int pre3_map_add_inverse_depth(pre3_ctx *ctx, int n_new, const double *uvd, double std_pxl, const double *initial_rho);
/* inversedepth_2_cartesian.m:27-76: convert every inverse-depth landmark whose linearity index is below the threshold
 * (0.1 in the reference) to a Cartesian point; converted_out[N] (may be NULL) receives the flags. */
PRE3_API int pre3_map_inversedepth_2_cartesian(pre3_ctx *ctx, double linearity_threshold, int32_t *converted_out);
/* map_management.m:27-79 as one call: delete_features (:33), inversedepth_2_cartesian (:48; convert_threshold < 0: skipped) and the
 * addition of initialize_features (:58-66), in that order, with ONE pass over the covariance (their row maps compose: each only selects or
 * recombines rows of the old state).  converted_out (may be null): per landmark of the map BEFORE the call, 1 = converted.
 * The result is what the three calls in sequence give (bit for bit when nothing is converted; to rounding in the entries that pair
 * a converted landmark with a new one). */
PRE3_API int pre3_map_management(pre3_ctx *ctx, int n_del, const int32_t *del_idx, double convert_threshold, int32_t *converted_out,
                                 int n_new, const double *uvd, double std_pxl, const double *initial_rho);
/* current landmark table: returns N, writes lm_type_out[N] if not NULL */
PRE3_API int pre3_get_map(pre3_ctx *ctx, int32_t *lm_type_out);

/* ---- the policy half of map_management.m:27-79 on the device ----------------------------------------- */
/* The features_info bookkeeping: 4 int32 per landmark, {times_predicted, times_measured, init_frame, last_visible}, for landmarks
 * first .. first+count-1.  A context has a book once pre3_set_book has been called (rows never set read 0), or when its map is empty at
 * the first pre3_map_policy; pre3_set_map drops it.  On a booked context every map call (pre3_map_delete, _add_inverse_depth,
 * _inversedepth_2_cartesian, pre3_map_management, pre3_map_policy) carries the book with the landmarks; landmarks they add get
 * {0, 0, s, s}, s = the last pre3_map_policy's step - 1 (0 before any).  A booked context's pre3_step / pre3_step_predicted / pre3_rescue
 * also record, per landmark, visibility at the x_k_k the rescue projects at (after the LI update, before the HI update) -- only in frames
 * where rescue_hi_inliers.m runs (at least one measurement; pre3_step_all records nothing) -- as one small launch between the two
 * updates; PRE3_OPT_STEP_TAIL has no such point, so a booked context's step takes the default form.  Every map call clears the record. */
PRE3_API int pre3_set_book(pre3_ctx *ctx, int first, int count, const int32_t *book);
PRE3_API int pre3_get_book(pre3_ctx *ctx, int first, int count, int32_t *book_out);     /* PRE3_E_STATE without a book */
#define PRE3_POLICY_MAX_CANDIDATES 8192
/* map_management.m:27-79 as ONE call, policy included (frame `step`, the loop variable of mono_slam.m:113):
 *  1. last_visible = step - 1 for last frame's IC landmarks (matching_sift_based.m:133); delete_features.m:31-49 on the counters as they
 *     stand (tm < 0.5 tp && tp > 5; step - init_frame > 20; N > 20 && step - last_visible > 20, N before deletion);
 *  2. measured = surviving landmarks with LI || HI (:37-40); 3. survivors: tp += (h predicted), tm += (LI || HI) (update_features_info.m);
 *  4. inversedepth_2_cartesian (convert_threshold < 0: skipped);
 *  5. T = measured == 0 ? min_features : max(0, min_features - measured); the K candidates (distorted pixels cand_uv[2K], camera-frame
 *     points cand_xyz[3K], descriptors cand_desc[128K] or NULL) are walked in the given order (the caller's Weighted_Smpl_wo_replacement
 *     draw): a candidate is rejected when any landmark visible at x_k_k -- the map after step 4 and the features accepted before it --
 *     lies strictly inside its box (semisizes 15 x 10 px), otherwise added with initial_rho = 1 / norm(xyz) and std_pxl; the walk ends when
 *     T is met or the candidates run out.  strict_reference = 1 reproduces quirk Q13 (ceil(T/2) additions) and Q14 (the box centre is
 *     (v, u)).  Additions also stop at the capacity.
 * Outputs (any may be NULL): del_out[N] ascending 0-based (*n_del_out of them), accepted_out[K] candidate indices in order (*n_acc_out;
 * they become landmarks N - n_del .. in that order), converted_out[N] per landmark before the call (a deleted one reads 0),
 * stats = {measured, T, candidates examined, N after}.  No book: PRE3_E_STATE.  Non-finite uv, a zero or non-finite xyz norm, K above
 * PRE3_POLICY_MAX_CANDIDATES or min_features above 1024: PRE3_E_ARG, before anything is launched (the context is unchanged).  The counters
 * reach the book only with the map's re-layout: a call that fails before it leaves the book as it was.
 * A deferred HI update is completed first and pending work flushed; x and P are what pre3_map_management gives with the same lists. */
PRE3_API int pre3_map_policy(pre3_ctx *ctx, int step, int min_features, double convert_threshold, double std_pxl, int strict_reference,
                             int K, const double *cand_uv, const double *cand_xyz, const double *cand_desc,
                             int32_t *del_out, int32_t *n_del_out, int32_t *accepted_out, int32_t *n_acc_out, int32_t *converted_out,
                             int32_t stats[4]);

/* ---- the IC-search stage on the device (search_IC_matches.m:31-44 + matching_sift_based.m:104-149) ---- */
/* features_info(i).Descriptor (128 x 1 double each, add_feature_to_info_vector_my_version_sift.m): desc is 128 x count
 * column-major for landmarks first .. first+count-1.  The bank follows the map through pre3_map_* (deleted landmarks
 * drop out, new ones start at zero until set).  Asynchronous: the array is copied into pinned memory of the context's
 * before the call returns (the caller may reuse it at once) and reaches the device on the context's stream. */
PRE3_API int pre3_set_descriptors(pre3_ctx *ctx, int first, int count, const double *desc);
PRE3_API int pre3_get_descriptors(pre3_ctx *ctx, int first, int count, double *desc);
/* the frame's SIFT set as stored in SIFT_result%04d.mat (SIFT_extract_save.m:68-69): SCAN_SIFT.Descriptor_RAW (128 x K2)
 * and SCAN_SIFT.SCALE_ORIENT_POS_RAW (4 x K2; rows 1:2 = pixel u,v), both column-major doubles.  Asynchronous like
 * pre3_set_descriptors: copied (and checked against the matrix-core matcher's bounds) on the host, pulled over PCIe and
 * packed on the context's stream; the call neither waits for queued work nor ends in a read-back. */
PRE3_API int pre3_set_scan(pre3_ctx *ctx, int K2, const double *descriptor_raw, const double *scale_orient_pos_raw);
/* One call = search_IC_matches.m:31-44 (h, H, S at the prediction) + matching_sift_based.m:104-149: stack the descriptors
 * of the predicted landmarks, siftmatch(des1', Descriptor_RAW) (double class, thresh 1.5 in the reference), window
 * gate (strict_reference = 1 reproduces quirk Q5), z / individually_compatible / descriptor refresh for the accepted.
 * Outputs: *n_matches = size(match_idx, 2); *m = number of accepted (= measurements installed, ascending landmark order);
 * meas_idx_out[m], z_out[2m] (optional); pairs_out[3*n_matches] (optional) = (k1, k2, accepted) per match, 0-based. */
PRE3_API int pre3_ic_search(pre3_ctx *ctx, double thresh, int strict_reference, int32_t *n_matches_out, int32_t *m_out,
                            int32_t *meas_idx_out, double *z_out, int32_t *pairs_out);

/* ---- the patch branch of the IC search: warped patches and NCC in the S-ellipse (search_IC_matches.m:45-51) -------------------
 * FEATURE_EXTRACTOR == 'FAST': predict_features_appearance.m:34-53 + pred_patch_fc.m:27-85 warp every predicted landmark's stored 41 x 41 patch
 * (add_feature_to_info_vector_my_version.m:29-41: half_patch_size_when_initialized = 20) to the predicted view as a 13 x 13 patch
 * (half_patch_size_when_matching = 6), and mex_files/CorePar_Ver1/matching.m:39-146 takes the best Pearson correlation (corrcoef) of that patch with
 * im(i-6:i+6, j-6:j+6) over the integer pixels (j, i) inside the 95 % ellipse of S_i (chi_095_2 = 5.9915, :36, :80).  Pixels are the reference's
 * 1-based coordinates; the image and the patches are column-major bytes, as MATLAB stores uint8.  All patch arithmetic is fp64 in both context dtypes.
 *   warp   pred_patch_fc.m:33-34: h outside the open band (6, nCols - 6) x (6, nRows - 6) gives the zero patch (:84), whose correlation with anything is
 *          NaN.  :40, :43: H_Wk_p_f = [R 0; 0 1] [I r; 0 1] = [R, R r] (the uncommented lines), H_kpf_k = inv(H_Wk_p_f) H_Wk (:46).  :52-53: the normals
 *          carry f/d = cam.F / cam.dx, which pre3_cam does not hold: it is the argument focal_over_d (the fork: 250.57731 / (4/176 * 0.001); Civera's
 *          f / dx in pixels works as well).  :66: the patch centre is rotate_with_dist_fc_c2c1.m:41-50 of uv_when_initialized; :68-74: the 13 x 13 integer
 *          grid around that sub-pixel centre goes back through rotate_with_dist_fc_c1c2.m:40-43 -- both over undistort_fm_my_version.m:56-81 (ten Newton
 *          steps, :64-67) and distort_fm_my_version.m:52-61 --, is shifted by uv_when_initialized - 20 - 1 (:75-76) and read with interp2 (:81), linear;
 *          a sample outside [1, 41] in either coordinate is NaN, and one NaN makes every correlation of the landmark NaN.
 *   search matching.m:61-62: the box ceil(5 sqrt(S(1,1))) x ceil(5 sqrt(S(2,2))) around round(h) (only a bound: sqrt(5.9915) < 5 and S >= R = I);
 *          :74-82: candidates in the order j (column, outer), i (row, inner), kept when nu' inv(S) nu < 5.9915 and j > 6 && j < nCols - 6 && i > 6 &&
 *          i < nRows - 6; a flat image patch gives NaN, which max ignores; :121: accepted when maximum_correlation > corr_threshold (0.60 in the fork,
 *          :31; 0.80 in the original, :29); ties go to the first maximum in candidate order.
 *          strict_reference = 0: the original line :115 -- the maximum over all K candidates, z that candidate.
 *          strict_reference = 1: what the fork runs, :118's correlation_matrix(2:end, 1) over corrcoef_partitioned.m:3-21.  With n = K + 1 < 100 the
 *          first candidate is dropped from the maximum and z is the candidate BEFORE the best one in scan order (K <= 1: no match); with n >= 100 the
 *          maximum is over candidates 1 .. 100 floor(n / 100) - 1 only and z is the best of those (the tail is lost).
 *          last_visible (:124) and the MaxInnov print are not part of this. */
#define PRE3_PATCH_NOT_PREDICTED 0     /* isempty(h): not searched */
#define PRE3_PATCH_NO_PATCH 1          /* the landmark has no stored patch (none set or cut since it was added): not searched */
#define PRE3_PATCH_ZERO 2              /* h in the border band: the zero patch, every correlation NaN */
#define PRE3_PATCH_OUTSIDE 3           /* the warp left the stored patch: a NaN sample, every correlation NaN */
#define PRE3_PATCH_NO_CANDIDATE 4      /* K == 0 */
#define PRE3_PATCH_BELOW 5             /* searched; the maximum is not above the threshold (or NaN) */
#define PRE3_PATCH_MATCHED 6
#define PRE3_PATCH_WARPED 7            /* pre3_predict_patches only: the predicted patch is valid */
/* The frame the search reads, nRows x nCols column-major bytes, resident until the next one.  The shape must be the camera's (PRE3_E_ARG; rows and
 * columns 15 .. 1024).  Asynchronous like pre3_set_scan: copied into pinned memory of the context's and pulled on its stream. */
PRE3_API int pre3_set_image(pre3_ctx *ctx, int nRows, int nCols, const uint8_t *im);
PRE3_API int pre3_get_image(pre3_ctx *ctx, int nRows, int nCols, uint8_t *im_out);                  /* synchronises; PRE3_E_STATE without an image */
/* (pre3_set_image_frame, below with pre3_set_scan_frame, takes the image from a resident SR4000 frame) */
/* The per-landmark bank for landmarks first .. first+count-1: patch_when_initialized (1681 bytes each, 41 x 41 column-major), uv_when_initialized (2),
 * r_wc_when_initialized (3), R_wc_when_initialized (9, column-major).  The bank follows the map through every pre3_map_* call and the policy calls,
 * like the descriptor bank: deleted landmarks drop out, survivors keep their patch under their new index, a new landmark has no patch until one is
 * set or cut and is not searched until then; pre3_set_map drops the bank.  The re-layout is one launch of its own behind the map call's, queued only
 * when a bank exists.  Asynchronous.  pre3_get_patches: any output may be NULL; has_patch_out[count] 0 / 1; a landmark without one reads zeros. */
PRE3_API int pre3_set_patches(pre3_ctx *ctx, int first, int count, const uint8_t *patch, const double *uv_init, const double *r_wc, const double *R_wc);
PRE3_API int pre3_get_patches(pre3_ctx *ctx, int first, int count, uint8_t *patch_out, double *uv_init_out, double *r_wc_out, double *R_wc_out,
                              int32_t *has_patch_out);
/* add_feature_to_info_vector_my_version.m:33-41 on the device: 41 x 41 around the integer pixels uv[2 count] (u = column, v = row, 1-based) out of the
 * resident image, r_wc and q2r(q) from the resident x_k_k.  A patch that leaves the image: PRE3_E_ARG before anything is queued.  Asynchronous. */
PRE3_API int pre3_patch_cut(pre3_ctx *ctx, int first, int count, const int32_t *uv);
/* predict_features_appearance.m alone, behind a projection at x_k_km1 (pre3_project): patch_out[169 N] (may be NULL; per landmark 13 x 13
 * column-major; zeros unless the status is PRE3_PATCH_WARPED or PRE3_PATCH_OUTSIDE, whose samples outside the stored patch are NaN),
 * status_out[N] (PRE3_PATCH_NOT_PREDICTED, _NO_PATCH, _ZERO, _OUTSIDE or _WARPED).  Synchronises. */
PRE3_API int pre3_predict_patches(pre3_ctx *ctx, double focal_over_d, double *patch_out, int32_t *status_out);
/* One call = search_IC_matches.m:31-51 on the patch branch: h, H, S at the prediction (pre3_ic_search's launch), k_patch_warp, k_patch_search, the
 * compaction of the accepted into ascending landmark order; one host wait at the end; z / individually_compatible are installed where pre3_ic_search
 * leaves them, so pre3_step_predicted[_seeded] and pre3_update_all follow.  Needs the predicted estimate in the covariance buffer, a camera and an
 * image (PRE3_E_STATE).  N == 0: m = 0.  Outputs: *m_out, meas_idx_out[m], z_out[2 m], and per landmark corr_out[N] (maximum_correlation as the mode
 * computes it; NaN where there is none), ncand_out[N] (K; 0 for a landmark that is not searched), status_out[N] (PRE3_PATCH_*); all but m_out optional. */
PRE3_API int pre3_patch_search(pre3_ctx *ctx, double focal_over_d, double corr_threshold, int strict_reference, int32_t *m_out,
                               int32_t *meas_idx_out, double *z_out, double *corr_out, int32_t *ncand_out, int32_t *status_out);
/* measurement only: with pre3_kernel_timing on, the last pre3_patch_search bracketed k_patch_warp and k_patch_search with events; their times */
PRE3_API int pre3_patch_timing(pre3_ctx *ctx, double *warp_ms_out, double *search_ms_out);

/* ---- FAST-9 corners on the resident image (pre3_fast.hip) --------------------------------------------------------
 * mex_files/Fast_Cr_Ver1/fast_corner_detect_9.m:53-3286 as initialize_a_feature.m:102 and initialize_n_features_FAST.m:69 call it, and
 * fast-matlab-src/fast_nonmax.m:38-100 (:104, :81).  The device computes the PUBLISHED segment test (9 contiguous ring pixels all > centre + threshold
 * or all < centre - threshold, strict as :61-63); the reference's file is a learned decision tree that answers differently on most ring states and
 * on few pixels of a real image (DESIGN.md section 30 has the counts; the fixture tests/golden/fast_lab_crop.npz pins an image where they agree).
 * There is no tree-exact mode. */
#define PRE3_FAST_MAX_CORNERS 8192
/* The rectangle rows [r0, r0 + rows) x columns [c0, c0 + cols) (0-based) of the resident image, taken as an image of its own the way imTemp2 is
 * (initialize_a_feature.m:93-94): candidates are its pixels 4 .. size - 3 (1-based, fast_corner_detect_9.m:59-60) and the ring never leaves it.
 * nonmax = 0: fast_corner_detect_9's list; nonmax = 1: fast_nonmax's (score = max of the two sums over the ring beyond centre +/- barrier, :70-75;
 * kept when >= all eight neighbours' scores, :87-92: ties are kept on both sides and so is a score-0 corner among score-0 neighbours).
 * K_out, uv_out[2 K] (column, row; 1-based, relative to the rectangle as the .m returns them; x outer, y inner as :59-60), score_out[K] (may be NULL;
 * the score at `barrier`, also with nonmax = 0).  uv_out and score_out hold PRE3_FAST_MAX_CORNERS entries unless K is known.  Waits once.
 * PRE3_E_STATE without an image.  PRE3_E_ARG before anything is queued: a rectangle that leaves the image, rows or cols < 7, a negative threshold
 * or barrier.  More than PRE3_FAST_MAX_CORNERS corners: PRE3_E_NOMEM after the wait with *K_out = 0; the context stays usable. */
PRE3_API int pre3_fast_detect(pre3_ctx *ctx, int r0, int c0, int rows, int cols, int threshold, int barrier, int nonmax,
                              int32_t *K_out, int32_t *uv_out, int32_t *score_out);
/* measurement only: with pre3_kernel_timing on, the last call of pre3_fast_detect or of the three pre3_init_feature*_fast* calls below bracketed its launches of pre3_fast.hip with events; their time */
PRE3_API int pre3_fast_timing(pre3_ctx *ctx, double *detect_ms_out);

/* ---- the VO front end's 4-point 3D-3D RANSAC (code_from_dr_ye/) ------------------------------------ */
typedef struct pre3_vo_result {
    double rot[9];          /* final rotation, row-major (find_transform_matrix_dr_ye.m on the winner's inliers, vodometry_dr_ye.m:221) */
    double trans[3];
    double euler[3];        /* R2e(rot): phi, theta, psi (vodometry_dr_ye.m:245-248); zeros when sta < 1 */
    double u[7];            /* Calculate_V_Omega_RANSAC_dr_ye.m:40-50: [T; R2q(R)] -- what pre3_predict takes; identity unless sta == 1 */
    double error_mean, error_std;   /* RANSAC_STAT.ErrorMean / ErrorStd (vodometry_dr_ye.m:222-225) */
    double dist;            /* inlier radius scale of ransac_dr_ye.m:20-23 (threshold = 0.001*dist on squared distances) */
    int32_t sta;            /* state of the final fit: 1 ok, 2 co-planar, -1 / 0 failed; 4 = no consensus (op_num < 3, :198-205) */
    int32_t n_support;      /* op_num */
    int32_t n_iterations;   /* RANSAC_STAT.nIterationRansac = min(rst, nIterations) (:226) */
    int32_t best;           /* rs_ind (0-based): the first hypothesis with the largest consensus */
} pre3_vo_result;
/* vodometry_dr_ye.m:162-236 over ransac_dr_ye.m:48-72.  pset1/pset2: 3 x pnum column-major matched 3-D points (frame 1 / 2).
 * draws[n_hyp][4]: 0-based positions in the match list -- the caller draws them with the reference's own rejection rule
 * (ransac_dr_ye.m:28-46; MATLAB's rand stream is not reproducible) and passes rst = min(700, nchoosek(pnum,4)) of them:
 * the reference evaluates all rst (its for-range is fixed at loop entry).  cnum_out[n_hyp], state_out[n_hyp],
 * inlier_out[pnum] optional. */
PRE3_API int pre3_vo_ransac(int device, int pnum, const double *pset1, const double *pset2, int n_hyp, const int32_t *draws,
                            int32_t *cnum_out, int32_t *state_out, int32_t *inlier_out, pre3_vo_result *res);
/* The same with ransac_dr_ye's own inputs: range images x,y,z (rows x cols column-major) of both frames, SIFT frames
 * frm1 (ldf x K1), frm2 (ldf x K2) (rows 1:2 = pixel column,row; 1-based), match (2 x pnum doubles, 1-based, as
 * siftmatch returns).  The point sets of ransac_dr_ye.m:13-19 are gathered on the device (and returned if asked). */
PRE3_API int pre3_vo_ransac_frames(int device, int rows, int cols, const double *x1, const double *y1, const double *z1,
                                   const double *x2, const double *y2, const double *z2, int ldf, int K1, const double *frm1,
                                   int K2, const double *frm2, int pnum, const double *match, int n_hyp, const int32_t *draws,
                                   double *pset1_out, double *pset2_out, int32_t *cnum_out, int32_t *state_out,
                                   int32_t *inlier_out, pre3_vo_result *res);
/* measurement only: average device time of one RANSAC (inputs resident) */
PRE3_API int pre3_vo_bench(int device, int pnum, const double *pset1, const double *pset2, int n_hyp, const int32_t *draws, int reps,
                           double *ms_per_call);

/* ---- seeded RANSAC: the three hypothesis tables drawn on the device ----------------------------------------------------------
 * Every RANSAC entry point above takes its random draws as an input.  The _seeded forms below take (seed, seq) instead and draw the table on the
 * device, on the stream of the work it feeds, from a counter-based stream: Philox4x64-10 with key = [seed, stream] (stream 1: 1-point RANSAC, 2: VO,
 * 3: floor plane) and counter = [hypothesis, attempt, seq, 0] -- a table is a pure function of (seed, seq) and the inputs its rejection rule reads,
 * identical on every caller, rank and run; seq is the caller's frame or step number.  A bounded integer in [0, range) is the high 64 bits of
 * word * range (no rejection; bias at most range / 2^64); a uniform double is (word >> 11) * 2^-53.  "Three distinct of m" are three ranks in
 * [0,m), [0,m-1), [0,m-2), each later one shifted past the earlier picks: randperm(m)(1:3)'s distribution without redraws.
 * Results are bit-identical to the unseeded entry point fed with the same table; the table comes back only on request (the *_out pointers, which
 * synchronise).  Argument errors are PRE3_E_ARG before anything is launched, the context unchanged. */

/* select_random_match.m:40-51: k = 3 positions per hypothesis when more than 3 measurements are individually compatible, else k = 1; no measurement:
 * a one-column table of zeros.  n_draw in [1, max_hyp].  hyp_out[n_draw * 3] (the first n_draw * k entries are written, k per hypothesis) and k_out
 * may be NULL.  pre3_ransac_seeded with no measurement scores nothing (stats = {-1, 0, 0, 0}, support = -1), as pre3_step skips the stage. */
PRE3_API int pre3_ransac_seeded(pre3_ctx *ctx, uint64_t seed, uint64_t seq, int n_draw, double threshold, int early_exit,
                                int32_t *hyp_out, int32_t *k_out, int32_t *support, int32_t *li_mask, int32_t stats[4]);
/* pre3_step / pre3_step_predicted with the draw kernel queued in front of the scoring launch: no host wait is added, the inbox carries no table;
 * PRE3_OPT_DEFER_HI, PRE3_OPT_PEND_HI and a booked context work as with a supplied table. */
PRE3_API int pre3_step_seeded(pre3_ctx *ctx, const double u[7], int m, const int32_t *meas_idx, const double *z, uint64_t seed, uint64_t seq,
                              int n_draw, double threshold, int early_exit, double chi2, int32_t *hyp_out, int32_t *k_out, int32_t stats[8]);
PRE3_API int pre3_step_predicted_seeded(pre3_ctx *ctx, uint64_t seed, uint64_t seq, int n_draw, double threshold, int early_exit, double chi2,
                                        int32_t *hyp_out, int32_t *k_out, int32_t stats[8]);
/* ransac_dr_ye.m:28-48: a position is round((pnum - 1) * u + 1); the four first draws are words 0..3 of block(h, attempt 0); position p (2nd, 3rd,
 * 4th) is redrawn -- word p of block(h, a), a = 1, 2, .. -- while it repeats an earlier position or shares a keypoint with one (ind_dup1/2/3 as the
 * reference writes them).  match: 2 x pnum doubles, column-major (keypoint numbers of frame 1 / 2), read on the device.  The reference loops for ever
 * when no admissible position exists; here a position stops after 64 redraws and keeps its last value: *capped_out = hypotheses with such a position.
 * n_hyp is the caller's rst.  draws_out[n_hyp * 4], capped_out: may be NULL.  pnum < 4: PRE3_E_ARG. */
PRE3_API int pre3_vo_ransac_seeded(int device, int pnum, const double *pset1, const double *pset2, const double *match, int n_hyp,
                                   uint64_t seed, uint64_t seq, int32_t *draws_out, int32_t *capped_out,
                                   int32_t *cnum_out, int32_t *state_out, int32_t *inlier_out, pre3_vo_result *res);
PRE3_API int pre3_vo_ransac_frames_seeded(int device, int rows, int cols, const double *x1, const double *y1, const double *z1,
                                          const double *x2, const double *y2, const double *z2, int ldf, int K1, const double *frm1,
                                          int K2, const double *frm2, int pnum, const double *match, int n_hyp, uint64_t seed, uint64_t seq,
                                          int32_t *draws_out, int32_t *capped_out, double *pset1_out, double *pset2_out, int32_t *cnum_out,
                                          int32_t *state_out, int32_t *inlier_out, pre3_vo_result *res);
/* ransac.m:142-176: per attempt three distinct of npts (block(h, attempt)); redrawn while norm(cross(p2 - p1, p3 - p1)) < eps on the cropped points,
 * at most 100 attempts, the last one kept.  n_draw in [1, PRE3_PLANE_MAX_DRAWS]; draws_out[n_draw * 3] may be NULL.  Only the points cross PCIe.
 * pre3_heading_from_scan_seeded with draws_out, applied_out and res_out all NULL does not synchronise. */
PRE3_API int pre3_plane_fit_seeded(int device, int rows, int cols, const double *x_sr, const double *y_sr, const double *z_sr,
                                   const int32_t *box, double t, int n_draw, uint64_t seed, uint64_t seq, int32_t *draws_out,
                                   int32_t *count_out, int32_t *inlier_out, pre3_plane_result *res);
PRE3_API int pre3_heading_from_scan_seeded(pre3_ctx *ctx, int rows, int cols, const double *x_sr, const double *y_sr, const double *z_sr,
                                           const int32_t *box, double t, int n_draw, uint64_t seed, uint64_t seq, int transpose,
                                           int strict_reference, int32_t *draws_out, int32_t *applied_out, pre3_plane_result *res_out);

/* ---- seeded map policy: the candidates' weighted order drawn on the device ---------------------------------------------------
 * Weighted_Smpl_wo_replacement.m, the draw initialize_a_feature_sift_3.m:42-46 makes once per frame: the order in which map_management.m walks its
 * initialisation candidates.  The reference draws one index at a time with probability proportional to the remaining weights
 * w_i = mvnpdf(uv_i, mean, diag(sigma^2)), mean = round([box_w box_h] / 2), sigma = round([box_w box_h] / 6) (MATLAB rounding; the reference's box is
 * 176 x 144: mean (88, 72), sigma (29, 24)).  That distribution (Plackett-Luce) is sampled here as an exponential race:
 *   key_i = -log1p(-U_i) * exp(q_i),  q_i = (((u_i - mu) / su)^2 + ((v_i - mv) / sv)^2) / 2,
 *   U_i = the uniform double of word 0 of the Philox block with key = [seed, stream 4] and counter = [i, 0, seq, 0],
 * and the order is the candidates sorted by (key, index) ascending -- a pure function of (seed, seq, box, uv), bit-equal on every run.  A key of 0
 * (U = 0) or +inf (a pixel absurdly far from the image) is legal and sorts by its value, then by index; no key is NaN.
 *
 * pre3_candidate_order: stateless, on the library's per-device scratch.  cand_uv[2K] distorted pixels; order_out[K]: order_out[p] = the candidate at
 * drawn position p (0-based); keys_out[K] (may be NULL): key_i per candidate.  K == 0 is PRE3_OK and writes nothing.  K outside
 * 0 .. PRE3_POLICY_MAX_CANDIDATES, a non-positive box size, a sigma that rounds to 0 (a size below 3), a null or non-finite uv: PRE3_E_ARG before
 * anything is launched. */
PRE3_API int pre3_candidate_order(int device, int K, const double *cand_uv, int box_w, int box_h, uint64_t seed, uint64_t seq,
                                  int32_t *order_out, double *keys_out);
/* pre3_map_policy with step 5's order drawn on the device: the candidates are given in ANY order (uploaded as they are), two launches in front of the
 * walk's on the context's stream re-lay them in the drawn order, and the call's one host wait stays the only one.  Every check, state requirement
 * and output of pre3_map_policy is kept, plus the box checks above.  accepted_out holds the CALLER's candidate indices, in the order of acceptance
 * (the descriptors are taken from cand_desc by them); order_out[K] (may be NULL) is the drawn order; stats[2] ("examined") counts drawn positions.
 * Results are bit-identical to pre3_map_policy fed with the candidate arrays permuted by order_out.  Argument errors are PRE3_E_ARG before anything
 * is launched: the context and the book are unchanged. */
PRE3_API int pre3_map_policy_seeded(pre3_ctx *ctx, int step, int min_features, double convert_threshold, double std_pxl, int strict_reference,
                                    int K, const double *cand_uv, const double *cand_xyz, const double *cand_desc, int box_w, int box_h,
                                    uint64_t seed, uint64_t seq, int32_t *order_out, int32_t *del_out, int32_t *n_del_out,
                                    int32_t *accepted_out, int32_t *n_acc_out, int32_t *converted_out, int32_t stats[4]);

/* ---- the SR4000 frame conditioned on the device: filter, image, keypoint depth gate -------------------------------------------
 * One handle holds one resident frame: the raw planes of a d1_%04d.dat scan, their 3 x 3 Gaussian-filtered x, y, z, the filtered uint8 amplitude image
 * (stored as doubles holding 0 .. 255) and the two scalars imax (the largest amplitude <= 65000; 0 when every pixel is saturated) and cmax
 * (max(confidence_map(:)): NaNs skipped, NaN only when every entry is NaN).  Planes are rows x cols, column-major, as pre3_plane_fit takes them; a .dat
 * frame is 144 x 176, any size >= 1 x 1 is accepted.  The handle owns its stream, its device buffers and its pinned staging; it touches no pre3_ctx and
 * no pooled scratch.  Calls on one handle must be serialised by the caller.  Results are bit-equal from run to run.
 *   mode 0: read_xyz_sr4000.m:8-21 with read_image_sr4000.m:3,10-24 -- fspecial('gaussian', [3 3], 2), imfilter(.., 'same') (a tap outside the image
 *           reads 0);
 *   mode 1: code_from_dr_ye/read_sr4000_data_dr_ye.m:8,11-21,42,70,88-90 -- sigma = 1, imfilter(.., 'replicate') (the nearest edge pixel).
 * A pixel is acc = w[0] p[0]; acc = acc + w[k] p[k], k = 1 .. 8, taps column-major, every product and sum rounded on its own; a NaN in the neighbourhood
 * makes the pixel NaN.  The image: per tap uint8(sqrt(v) / sqrt(imax) * 255), v = imax where the amplitude is above 65000 (normalzie_image.m:4), the tap
 * sum rounded and saturated again (imfilter on uint8).  uint8 is MATLAB's: half away from zero, saturated to [0, 255], NaN -> 0.
 * Deviation: read_sr4000_data_dr_ye.m:34-59 leaves the image un-normalised when the frame has no confidence rows; here conf == NULL changes nothing in
 * the image pipeline -- only gate 0 skips its confidence term and gate 1 is refused. */
#define PRE3_SR_MAX_KEYPOINTS 8192
typedef struct pre3_sr_frame pre3_sr_frame;
/* fspecial('gaussian', [3 3], sigma) (read_xyz_sr4000.m:8, read_sr4000_data_dr_ye.m:8): w[3 (j + 1) + (i + 1)] = exp(-(i^2 + j^2) / (2 sigma^2)) over
 * the sum of the nine values taken column-major -- the bits the conditioning launch uses.  Host only: needs no device. */
PRE3_API int pre3_sr_gauss3(double sigma, double w[9]);
PRE3_API int pre3_sr_frame_create(pre3_sr_frame **out, int device, int rows, int cols);
PRE3_API int pre3_sr_frame_destroy(pre3_sr_frame *f);
/* read_xyz_sr4000.m:10-21 / read_image_sr4000.m:10-24 / read_sr4000_data_dr_ye.m:11-21,27-29,88-90 on the five planes of a frame (conf may be NULL): one
 * staged transfer, then the maxima launch and the conditioning launch queued on the handle's stream; returns without waiting.  PRE3_E_ARG before
 * anything is launched, the previous frame left intact: a null plane, a mode other than 0 or 1, a negative or non-finite amplitude (MATLAB's sqrt
 * would go complex). */
PRE3_API int pre3_sr_frame_load(pre3_sr_frame *f, int mode, const double *z, const double *x, const double *y,
                                const double *amp, const double *conf /* may be NULL */);
/* the filtered x, y, z, the image, the confidence map as loaded, imax, cmax: any may be NULL; synchronises.  PRE3_E_STATE before the first load;
 * conf != NULL on a frame loaded without one: PRE3_E_ARG. */
PRE3_API int pre3_sr_frame_get(pre3_sr_frame *f, double *x, double *y, double *z, double *img, double *conf,
                               double *imax, double *cmax);
/* ---- Low-confidence pixels compensated by a 3 x 3 median in front of the Gaussian -------------------------------------------
 * A setting on the handle, not a mode: it applies to every pre3_sr_frame_load / pre3_sr_frame_load_text queued after it and does not recondition the
 * frame that is resident.  Conditioning stays at two launches.  P a plane as loaded, U the normalised uint8 image, bad = conf < cutoff (strictly; a NaN
 * confidence is not bad; on a frame loaded without a confidence map nothing is bad):
 *   form 0  PRE3_SR_COMP_NONE          nothing: the default, bit for bit the library without this section.
 *   form 1  PRE3_SR_COMP_BADPIXEL      aux_code/compensate_badpixel_soonhac.m:5-14 as code_from_dr_ye/read_sr4000_data_dr_ye.m:44 (commented out
 *           there, between the uint8 normalisation :42 and the Gaussian :70,88-90) and read_xyz_sr4000_dr_ye.m:36-39 (cut-off 1) call it: for x, y, z
 *           and U alike comp = bad ? medfilt2(P, [3 3], 'symmetric') : P, every median taken on the plane as loaded; the mode's Gaussian reads comp.
 *   form 2  PRE3_SR_COMP_IMAGE_MEDIAN  code_from_dr_ye/read_image_sr4000_dr_ye.m:21-24: U' = medfilt2(U, [3 3]) (zero padding) at every pixel, the
 *           Gaussian reads U'; x, y, z are untouched.  With mode 0 this is that file exactly.
 * A Gaussian tap outside the image reads 0.0 in mode 0 and the compensated edge pixel in mode 1.  The median is the fifth smallest of the nine window
 * values; a NaN in the window makes it NaN (our rule: medfilt2 documents none).  raw planes, the confidence map, imax, cmax, both keypoint gates'
 * confidence term and pre3_sr_frame_get's conf are the same in every form.
 * Deviations: form 1 with mode 0 is our composition of the step with read_xyz_sr4000.m's filter (the reference pairs it with sigma = 1 only);
 * read_xyz_sr4000_dr_ye.m's own pairing (sigma = 1 with zero padding) is neither mode and is not reachable. */
#define PRE3_SR_COMP_NONE 0
#define PRE3_SR_COMP_BADPIXEL 1
#define PRE3_SR_COMP_IMAGE_MEDIAN 2
#define PRE3_SR_MEDFILT_MAX_PIXELS (1 << 26)   /* rows * cols of pre3_sr_medfilt3, the cap of pre3_sr_frame_create */
/* the setting for the loads that follow.  PRE3_E_ARG, the setting unchanged: a null handle, a form outside 0 .. 2, a non-finite cutoff with form 1.
 * Host only: launches nothing, waits for nothing. */
PRE3_API int pre3_sr_frame_set_compensation(pre3_sr_frame *f, int form, double cutoff);
PRE3_API int pre3_sr_frame_get_compensation(pre3_sr_frame *f, int32_t *form, double *cutoff);
/* the form the RESIDENT frame was conditioned with and the number of pixels compensate_badpixel_soonhac.m:6 replaced in it: n_bad is 0 under forms 0
 * and 2 and on a frame without a confidence map.  Synchronises.  PRE3_E_STATE before the first load; a refused pre3_sr_frame_load_text leaves both as
 * they were, with the previous frame. */
PRE3_API int pre3_sr_frame_bad_pixels(pre3_sr_frame *f, int32_t *form_of_frame, int32_t *n_bad);
/* medfilt2(A, [3 3]) (padding 0: zeros, MATLAB's default) or medfilt2(A, [3 3], 'symmetric') (padding 1) of a rows x cols column-major plane of
 * doubles -- they may hold uint8 values: the median is a selection.  Stateless, on the library's per-device scratch; synchronises.  Any size from
 * 1 x 1 to PRE3_SR_MEDFILT_MAX_PIXELS pixels.  PRE3_E_ARG: a null pointer, a padding other than 0 or 1, a non-positive size or one above the cap. */
PRE3_API int pre3_sr_medfilt3(int device, int rows, int cols, const double *A, int padding, double *out);
/* ---- The .dat text of a frame parsed on the device (read_xyz_sr4000.m:2-3,25-42: load() of d1_%04d.dat).
 * Grammar -- what MATLAB's load and numpy.loadtxt both accept for these files, nothing more: space, tab and \r separate; a row ends at \n or at the
 * end of the text; a line without a token is skipped; a token is [+-]?digits[.digits*]?([eE][+-]?digits)?, [+-]?.digits with the same exponent,
 * [+-]?inf or [+-]?nan in any letter case.  Anything else -- d/D exponents, % or # comments, commas, a NUL byte, a lone sign or dot -- is a bad token.
 * Every double equals strtod's / Python float()'s bit for bit (correctly rounded, ties to even, signed zeros); a token the conversion cannot decide
 * exactly is never stored as a guess: it fails the call.
 * status: 0 ok, 1 bad token, 2 ragged rows, 3 wrong shape for this handle (or more tokens than the handle holds), 4 undecided token, 5 negative or
 * non-finite amplitude, 6 empty text; checked in the order 6, 2, 1, 4, 3, 5.  Any non-zero status returns PRE3_E_ARG with info filled.  rows, cols:
 * the non-empty lines and the token count of the first.  bad_row, bad_col (0-based), bad_offset (bytes): the bad token; for ragged rows the first row
 * whose token count differs, min(its count, cols), and the offset of its first extra token or of the next row's first token (nbytes when none). */
typedef struct { int32_t status, rows, cols, has_conf, has_timestamp, n_tokens, n_undecided, bad_row, bad_col;
                 int64_t bad_offset; double timestamp; } pre3_sr_text_info;
/* the chunk of the byte passes and the longest text the calls below take.  Host only: needs no device. */
PRE3_API int pre3_sr_text_limits(int32_t *chunk_bytes, int64_t *max_bytes);
/* MATLAB's load for any rectangular ASCII matrix: out[rows x cols], column-major, cap doubles of room.  Stateless, on the library's per-device
 * scratch; synchronises.  out is written on success only.  More than cap tokens: PRE3_E_NOMEM with info->rows, cols, n_tokens filled. */
PRE3_API int pre3_sr_text_parse(int device, const char *text, size_t nbytes, double *out /* column-major */, size_t cap,
                                pre3_sr_text_info *info);
/* pre3_sr_frame_load from the file's bytes: exactly 4 rows, 5 rows or 5 rows + 1 lines of cols tokens (read_xyz_sr4000.m:25-42: z, x, y, amplitude,
 * then the confidence map, then the timestamp in the last line's first entry).  One copy of the bytes through the handle's pinned staging, the three
 * parse launches into a spare plane block, ONE wait on the pinned status (has_conf, the timestamp, and whether the file is taken at all), then -- on
 * success only -- the spare block becomes the frame and the maxima and conditioning launches of pre3_sr_frame_load are queued; returns without a
 * second wait.  On any failure the previous frame, its keypoint record and the handle's state are untouched. */
PRE3_API int pre3_sr_frame_load_text(pre3_sr_frame *f, int mode, const char *text, size_t nbytes, pre3_sr_text_info *info);
/* The keypoint stage on the resident frame.  frm[K][ldf]: one SIFT frame per keypoint (a column of SCALE_ORIENT_POS_RAW), entry 0 the pixel column,
 * entry 1 the pixel row, both 1-based; the pixel is (round(row), round(column)), MATLAB rounding.  des[K][ND]: its descriptor (ND = 128 in the
 * reference; ND == 0: none).
 *   gate 0: SIFT_extract_save.m:71-88 over inittialize_depth_my_version.m:16,40-45,74-92 -- on the FILTERED planes: dropped when x is NaN, when
 *           df = sqrt(x^2 + y^2 + z^2) < 0.4, or (with a confidence map) when conf <= 0.5 cmax; kept keypoints give xyz_out = [-x; -y; z] and
 *           rho_out = 1 / df (the reference's norm([-x -y z]) restated as df).  A NaN y or z alone survives with NaN coordinates, as in the reference.
 *   gate 1: code_from_dr_ye/confidence_filtering.m:1-13 -- dropped when conf < 0.5 cmax (strictly); needs the confidence map; xyz_out and rho_out
 *           are not written.
 * The kept keypoints keep the caller's order: keep_idx[n_kept] (0-based), frm_out[n_kept][ldf], des_out[n_kept][ND], xyz_out 3 x n_kept column-major
 * (XYZ_DATA's layout), rho_out[n_kept]; each output except n_kept may be NULL.  Synchronises.  K == 0 launches nothing.  PRE3_E_ARG before anything is
 * launched: a null handle, n_kept, frm or des; a gate other than 0 or 1; gate 1 without a confidence map; K outside 0 .. PRE3_SR_MAX_KEYPOINTS;
 * ldf < 2 or ND < 0 (or either above 4096); a non-finite position, or one whose rounded pixel lies outside the image (MATLAB would raise an index
 * error).  PRE3_E_STATE before the first load. */
PRE3_API int pre3_sr_frame_keypoints(pre3_sr_frame *f, int gate, int ldf, int K, const double *frm, int ND, const double *des,
                                     int32_t *n_kept, int32_t *keep_idx, double *frm_out, double *des_out,
                                     double *xyz_out /* 3 x n_kept, gate 0 */, double *rho_out);

/* ---- the SIFT extractor on a resident frame -----------------------------------------------------------------------------------
 * [frames, descriptors, gss, dogss] = sift_vedal(I) (sift/sift_vedal.m:127-323) with its defaults -- S = 3, omin = -1, O = floor(log2(min(M, N))) + 1 - 3,
 * sigma0 = 1.6 2^(1/3), sigman = 0.5, thresh = 0.04 / 3 / 2, r = 10, NBP = 4, NBO = 8, magnif = 3, boundary points discarded -- on the handle's stream.
 * It replaces the reference's native per-frame code: imsmooth.c:44-80,128-160 (the fp64 separable Gaussian; PAD_BY_CONTINUITY is defined, so a tap
 * outside the image reads the nearest edge pixel), gaussianss.m:133-227 (the level chain, doubleSize, halveSize), diffss.m:57-66,
 * siftlocalmax.c:229-249, sift_vedal.m:259-265 (the boundary discard), siftrefinemx.c:150-303, siftormx.c:138-253, siftdescriptor.c:310-513.
 * Bit-exact against tests/sift_ref.py: every level of gss and dogss, the counts, the refined points and their order.  Equal: the number and order of
 * the orientations.  Toleranced (they pass through pow, exp, atan2, sqrt, fmod, sin, cos of the device's library and a summation order of their own):
 * sigma, theta and the descriptor entries.  Results are bit-equal from run to run. */
#define PRE3_SIFT_MAX_TAPS 32
#define PRE3_SIFT_LEVELS 6                                  /* Gaussian levels per octave (smin = -1 .. smax = 4); one DoG level fewer */
#define PRE3_SIFT_MAX_CANDIDATES (4 * PRE3_SR_MAX_KEYPOINTS)   /* refined keypoints (before the orientations multiply them), all octaves together */
/* The scale-space plan of a rows x cols image, made with the host's exp / pow / sqrt: the bits the launches use (gaussianss.m:72-80,129-203,
 * imsmooth.c:130-142).  O_out: the number of octaves; oct_rows / oct_cols [O]: their sizes (the first is 2 rows x 2 cols); sigma0_out;
 * pow2_out[5] = 2^(s / S), s = -1 .. 3 (the boundary test's); for octave o and level l at [o * PRE3_SIFT_LEVELS + l]: sigma_out (the smoothing that
 * makes the level from the one before it; <= 0.01: a copy), W_out = ceil(4 sigma), taps_out[.. * PRE3_SIFT_MAX_TAPS] the 2 W + 1 taps (zeros behind
 * them).  Every output except O_out may be NULL.  Host only: needs no device.  min(rows, cols) < 8: PRE3_E_ARG. */
PRE3_API int pre3_sift_plan_get(int rows, int cols, int32_t *O_out, int32_t *oct_rows, int32_t *oct_cols, double *sigma0_out, double *pow2_out,
                                double *sigma_out, int32_t *W_out, double *taps_out);
/* sift_vedal on `image` (rows x cols doubles, column-major) or, with image == NULL, on the handle's own filtered image.  strict_reference = 1: the image
 * is uint8 and doubleSize (gaussianss.m:210-224) interpolates in uint8 class -- every 0.25 I / 0.5 I term rounded half away from zero, the sums
 * saturated at 255 left to right; 0: in double.  The set is left in the handle's keypoint block as the RAW set, as after the transfer of a
 * pre3_sr_frame_keypoints with ldf = 4, ND = 128: frames [K][4] = (x + 1, y + 1, sigma, theta), 1-based as SIFT_extract_save.m:55-56 leaves them,
 * descriptors [K][128] behind them.  No gate has run: pre3_sr_frame_gate is next.  K_out; frm_out 4 x K (one_based = 0: sift_vedal's own 0-based x, y;
 * the block is unaffected); des_out 128 x K; counts_out[4 * O]: per octave the maxima of +D and -D, those inside the boundary, the refined, the oriented.
 * Outputs other than K_out may be NULL; they must hold PRE3_SR_MAX_KEYPOINTS columns unless K is known.  Waits once, at the end.
 * The descriptor bounds of the ranked IC route (finite, |x| <= 2^60, no non-zero |x| < 2^-40) are or-reduced on the device and come back with the counts.
 * PRE3_E_ARG before anything is queued, the previous record intact: a null handle or K_out; min(rows, cols) < 8; a non-finite image entry; with
 * strict_reference an entry that is not an integer in 0 .. 255.  PRE3_E_STATE likewise: image == NULL before the first load.  PRE3_E_NOMEM after the
 * wait, leaving a valid empty record: more than PRE3_SIFT_MAX_CANDIDATES refined keypoints or more than PRE3_SR_MAX_KEYPOINTS keypoints. */
PRE3_API int pre3_sr_frame_sift(pre3_sr_frame *f, const double *image /* NULL: the handle's own filtered image */, int strict_reference, int one_based,
                                int32_t *K_out, double *frm_out /* 4 x K */, double *des_out /* 128 x K */, int32_t *counts_out /* 4 per octave */);
/* pre3_sr_frame_keypoints' gate launch (SIFT_extract_save.m:71-88, confidence_filtering.m:1-13) over the raw set ALREADY in the block -- a
 * pre3_sr_frame_sift's, or an earlier pre3_sr_frame_keypoints' with ldf = 4 and ND = 128 -- with no upload; a position is clamped into the image.
 * Same outputs and the same record as pre3_sr_frame_keypoints fed with that set: frm_out[n_kept][4], des_out[n_kept][128].  PRE3_E_STATE: no frame
 * loaded, or no raw set for the frame the handle holds.  PRE3_E_ARG: the set in the block has another ldf or ND (the outputs are sized for 4 and 128). */
PRE3_API int pre3_sr_frame_gate(pre3_sr_frame *f, int gate, int32_t *n_kept, int32_t *keep_idx, double *frm_out, double *des_out,
                                double *xyz_out /* 3 x n_kept, gate 0 */, double *rho_out);
/* a level of gss (dog = 0: level 0 .. 5) or dogss (dog = 1: 0 .. 4) of octave `octave` of the last pre3_sr_frame_sift -- sift_vedal's third and fourth
 * outputs -- into out[oct_rows x oct_cols], column-major.  Synchronises.  PRE3_E_STATE before the first pre3_sr_frame_sift. */
PRE3_API int pre3_sr_frame_sift_level(pre3_sr_frame *f, int octave, int level, int dog, double *out);
/* the refined points of the last pre3_sr_frame_sift (siftrefinemx's output, before the orientations), all octaves in order: n_out, and out[n][4] =
 * (x, y, s, octave) with x, y, s in the octave's own coordinates, 0-based, and octave counted from 0.  out may be NULL (the count alone), else it holds
 * PRE3_SIFT_MAX_CANDIDATES rows unless n is known.  Synchronises.  PRE3_E_STATE before the first pre3_sr_frame_sift, or after one that overflowed. */
PRE3_API int pre3_sr_frame_sift_refined(pre3_sr_frame *f, int32_t *n_out, double *out);

/* ---- the VO front end between two resident SR4000 frames, in one call ---------------------------------------------------------
 * vodometry_dr_ye.m:139-236 + Calculate_V_Omega_RANSAC_dr_ye.m:41-50 between the keypoint sets held by two resident frames: prev and cur each hold the
 * result of their last pre3_sr_frame_keypoints (gate 1 in the reference: confidence_filtering.m on both frames).  siftmatch(des1, des2, thresh)
 * (sift/siftmatch.c:97-122: every pair's bins in order, the first index on ties, the ratio test in float) with prev's kept descriptors as the queries;
 * pnum = size(match, 2); rst = min(700, nchoosek(pnum, 4)) (:171); ransac_dr_ye.m:13-72 with the draws of pre3_vo_ransac_frames_seeded's rule from
 * (seed, seq); the winner, the final fit and its statistics (:185-236); u = [T; R2q(R)].  Everything runs on the device on cur's stream, pnum and rst never
 * leave it, and the call ends in ONE host wait.  Seeded only: the caller does not know pnum before the call, so it cannot supply a draw table.
 * Results are bit-equal from run to run, and bit-equal to pre3_siftmatch_f64 on the kept descriptors followed by pre3_vo_ransac_frames_seeded on the
 * filtered planes, the kept frames and that match list with n_hyp = rst and the same (seed, seq).
 * Outputs (each may be NULL; arrays sized by the caller for the worst case, n1 = prev's kept keypoints and 700 hypotheses): *pnum_out;
 * match_out 2 x pnum doubles, column-major, 1-based positions in the KEPT sets (what pre3_sr_frame_keypoints returned, not the caller's indices);
 * pset1_out / pset2_out 3 x pnum; draws_out[rst * 4]; *capped_out; cnum_out[rst], state_out[rst], inlier_out[pnum]; res.
 * pnum < 4 is a result (:152-160): PRE3_OK with sta = 4, n_support = n_iterations = 0, u = [0 0 0 1 0 0 0], every other field of res zero; only pnum_out
 * and match_out are written besides.  op_num < 3: sta = 4 as in pre3_vo_ransac.  No matched point beyond 0.4 m: PRE3_E_NUMERIC.
 * PRE3_E_ARG before anything is queued, both handles unchanged: a null handle, prev == cur, handles of different devices or frame sizes, descriptors of
 * other than 128 entries on either side, a thresh that is not positive and finite.  PRE3_E_STATE likewise: a handle without a loaded frame, or without a
 * keypoint result for the frame it holds (none yet, or a pre3_sr_frame_load after it).  Calls that share a handle must be serialised by the caller. */
PRE3_API int pre3_vo_pair_seeded(pre3_sr_frame *prev, pre3_sr_frame *cur, double thresh /* siftmatch's, 1.5 in the reference */,
                                 uint64_t seed, uint64_t seq,
                                 int32_t *pnum_out, double *match_out /* 2 x pnum, 1-based, kept positions */,
                                 double *pset1_out, double *pset2_out, int32_t *draws_out, int32_t *capped_out,
                                 int32_t *cnum_out, int32_t *state_out, int32_t *inlier_out, pre3_vo_result *res);

/* ---- map management's candidate build and policy from two resident frames, in one call ---------------------------------------
 * map_management.m:27-79 for frame `step` with initialize_features.m:95-99 in front of it: matches = siftmatch(DataPre.Descriptor,
 * DataCurrent.Descriptor) between the keypoint sets two resident frames hold (pre3_vo_pair_seeded's matcher: prev's kept descriptors the queries), and
 * candidate c (0-based column of match) is prev's kept keypoint match[0][c] - 1: uv = entries 0 and 1 of its kept frame, rho = the keypoint stage's rho,
 * descriptor = its kept descriptor.  prev's last pre3_sr_frame_keypoints must have been gate 0 (it supplies rho); cur's may be either gate; ND == 128 on
 * both.  From there on the call is pre3_map_policy_seeded with K = pnum = size(match, 2): the order rule from (seed, seq, box), the state checks, the
 * flush of deferred work, outputs and stats are that call's.  pnum never reaches the host before the walk: buffers, grids and the result block are laid
 * out by the cap n1 = prev's kept count (<= PRE3_POLICY_MAX_CANDIDATES), the real count stays in a device header, and the call ends in ONE host wait.
 * The accepted candidates' descriptors go from prev's keypoint block into the context's bank on the device.
 * Outputs (each may be NULL; arrays sized by the caller for n1 candidates): *K_out = pnum; match_out 2 x pnum doubles, column-major, 1-based positions
 * in the KEPT sets; order_out[pnum]; accepted_out holds candidate indices c (map them through match_out and prev's keep_idx); the rest as
 * pre3_map_policy_seeded.  pnum == 0 (n1 == 0 or n2 == 0 included) is a result: the deletion, counters and conversion still happen.
 * Bit-identical to pre3_siftmatch_f64 on the kept descriptors, the gather of prev's kept frames / xyz / descriptors by match[0], and
 * pre3_map_policy_seeded on those arrays.
 * A matched keypoint with a non-finite pixel, or a rho that is not finite and positive (gate 0 lets a NaN y or z through): PRE3_E_NUMERIC after the
 * wait and before the map is touched -- context, book, map and both handles as they were.  PRE3_E_ARG / PRE3_E_STATE before anything is queued, with
 * the context, the book and both handles unchanged: everything pre3_map_policy_seeded and pre3_vo_pair_seeded refuse, prev's record not gate 0, a
 * handle on another device than the context.  Calls that share a handle or the context must be serialised by the caller. */
PRE3_API int pre3_map_policy_frames_seeded(pre3_ctx *ctx, pre3_sr_frame *prev, pre3_sr_frame *cur, double thresh, int step, int min_features,
                                           double convert_threshold, double std_pxl, int strict_reference, int box_w, int box_h, uint64_t seed,
                                           uint64_t seq, int32_t *K_out, double *match_out /* 2 x K, 1-based kept positions */, int32_t *order_out,
                                           int32_t *del_out, int32_t *n_del_out, int32_t *accepted_out, int32_t *n_acc_out, int32_t *converted_out,
                                           int32_t stats[4]);

/* ---- the plane fit, the heading update and the IC search's scan fed from a resident frame --------------------------------------
 * plane_fit_to_data.m:13-149 over ransacfitplane.m:51-116, ransac.m:113-225, fitplane.m:31-54, plane_imp_line_par_int_3d.m:56-100, as pre3_plane_fit,
 * on the FILTERED x, y, z a handle holds (what read_xyz_sr4000 returns when the frame was loaded in mode 0, plane_fit_to_data.m:13's input; mode 1 is
 * taken as it is): the box is gathered from the resident planes on the device into the fit's point block (x = -x_sr, y = -y_sr, z = z_sr, column-major
 * inside the box), and the draw, score and fit launches of pre3_plane_fit[_seeded] run behind that gather.  Nothing of the frame is read back or sent
 * again: a supplied table is the only thing that crosses PCIe, the seeded form sends nothing.  box, t, n_draw, draws, (seed, seq) and every output as
 * pre3_plane_fit / pre3_plane_fit_seeded.  Bit-identical -- every integer and every double of res, count_out, inlier_out, draws_out -- to that call fed
 * with the planes pre3_sr_frame_get returns.  Runs on the handle's stream and the library's per-device scratch; synchronises.
 * A non-finite coordinate inside the box (the filter turns a NaN into a 3 x 3 patch of NaNs) cannot be seen by the host any more: the gather raises a
 * device flag, the launches behind it leave at once, and the call returns PRE3_E_NUMERIC with res filled (sta = 5) and the optional outputs zeroed --
 * a status where pre3_plane_fit has an argument error.
 * PRE3_E_ARG before anything is queued: a null handle or res, and everything pre3_plane_fit refuses except the non-finite coordinate (a box outside
 * the frame or with fewer than 3 points, a box of fewer than 40 rows, n_draw outside [1, PRE3_PLANE_MAX_DRAWS], t <= 0, a null table or a draw
 * outside [0, npts)).  PRE3_E_STATE: a handle without a loaded frame. */
PRE3_API int pre3_plane_fit_frame(pre3_sr_frame *f, const int32_t *box, double t, int n_draw, const int32_t *draws,
                                  int32_t *count_out, int32_t *inlier_out, pre3_plane_result *res);
PRE3_API int pre3_plane_fit_frame_seeded(pre3_sr_frame *f, const int32_t *box, double t, int n_draw, uint64_t seed, uint64_t seq,
                                         int32_t *draws_out, int32_t *count_out, int32_t *inlier_out, pre3_plane_result *res);
/* mono_slam.m:189-193 (and initialize_x_and_p.m:36-37's fit) from a resident frame: pre3_heading_from_scan[_seeded] with the box gathered from the
 * handle's filtered planes.  The context's stream waits for an event on the handle's, the gather, the draws, the score, the fit and the heading rows
 * are queued on the context's stream, and the handle's stream then waits for an event behind them: a pre3_sr_frame_load that follows cannot overwrite
 * planes the gather still reads.  State, gate (strict_reference), transpose, outputs and error words as pre3_heading_from_scan; x, P, applied and res
 * are bit-identical to that call fed with the planes pre3_sr_frame_get returns.  With applied_out, res_out and draws_out all NULL the call does not
 * synchronise.  A non-finite coordinate inside the box: the update is skipped on the device (x and P untouched); a call that waits returns
 * PRE3_E_NUMERIC with res filled (sta = 5), applied = 0 and a table of zeros.  PRE3_E_ARG before anything is queued, context and handle unchanged:
 * a null context or handle, a handle on another device than the context, and the argument errors above.  PRE3_E_STATE: a handle without a loaded
 * frame; a context whose covariance buffer does not hold (x_k_k, p_k_k).  Calls that share the handle or the context must be serialised by the caller. */
PRE3_API int pre3_heading_from_frame(pre3_ctx *ctx, pre3_sr_frame *f, const int32_t *box, double t, int n_draw, const int32_t *draws,
                                     int transpose, int strict_reference, int32_t *applied_out, pre3_plane_result *res_out);
PRE3_API int pre3_heading_from_frame_seeded(pre3_ctx *ctx, pre3_sr_frame *f, const int32_t *box, double t, int n_draw, uint64_t seed, uint64_t seq,
                                            int transpose, int strict_reference, int32_t *draws_out, int32_t *applied_out,
                                            pre3_plane_result *res_out);
/* matching_sift_based.m:104,129-135: pre3_set_scan with Descriptor_RAW / SCALE_ORIENT_POS_RAW taken from the handle's keypoint block instead of the
 * host.  which = 0: the raw set handed to the handle's last pre3_sr_frame_keypoints (des[K][128], entries 0..3 of frm[K][ldf]; entries at or beyond
 * ldf are zero -- only the pixel column and row are read); which = 1: the kept set that call left.  One copy launch on the context's stream behind an
 * event on the handle's, released by an event the handle's stream waits for; nothing crosses PCIe, the call does not synchronise.  The bounds the
 * ranked route needs of the descriptors were noted when the raw set passed through the handle's staging (the kept set inherits them).  Afterwards the
 * context is as after pre3_set_scan with the same arrays.  K == 0 is legal.  PRE3_E_ARG: a null context or handle, which outside {0, 1}, descriptors
 * of other than 128 entries, a handle on another device than the context.  PRE3_E_STATE: a handle without a loaded frame, or without a keypoint
 * result for the frame it holds (none yet, or a pre3_sr_frame_load after it). */
PRE3_API int pre3_set_scan_frame(pre3_ctx *ctx, pre3_sr_frame *f, int which);
/* pre3_set_image with the frame taken from the handle's filtered image plane (doubles holding 0 .. 255) instead of the host: one conversion launch on
 * the context's stream behind an event on the handle's, released as above; nothing crosses PCIe, nothing is read back, the call does not synchronise.
 * The frame's shape must be the camera's (PRE3_E_ARG); PRE3_E_STATE: a handle without a loaded frame. */
PRE3_API int pre3_set_image_frame(pre3_ctx *ctx, pre3_sr_frame *f);

/* ---- patch-feature initialisation from FAST corners --------------------------------------------------------------
 * mex_files/Fast_Cr_Ver1/initialize_a_feature.m:27-215 on the FAST branch in one call, between steps: needs (x_k_k, p_k_k), the camera, the resident
 * image and a loaded pre3_sr_frame of the image's shape on the context's device, whose filtered planes supply the depth.  One launch (k_fast_box)
 * behind the existing projection at x_k_k (:48) runs up to `attempts` attempts; per attempt
 *   :64-68    the box centre, (row, column) 1-based, with BoxLimX = [1 nCols], BoxLimY = [1 nRows] (the fork's 144 x 176 generalised):
 *             row = round(u1 ((nRows - 1) - 42 - 60)) + 51, column = round(u2 ((nCols - 1) - 42 - 40)) + 41 -- from centres[2 a], centres[2 a + 1], or
 *             (_seeded) from words 0 and 1 of the Philox block with key [seed, 5] and counter [a, 0, seq, 0] (pre3_philox.h);
 *   :93-105   the 61 x 41 box as an image of its own: the segment test at `threshold`, fast_nonmax at `barrier` (-1: the reference's 10 and 20);
 *   :164-174  "features in the box" over the landmarks with an h, strict inequalities.  strict_reference = 1: u (the column) against the ROW centre
 *             +/- 30 and v against the COLUMN centre +/- 20, as written; 0: the axes matched;
 *   :176-180  the first maximum in scan order of a box with a corner and no feature, shifted into the image (:152-157);
 *   :188-194  gate 0 of pre3_sr_frame_keypoints at that pixel (x NaN, df < 0.4, conf <= 0.5 cmax); a refusal ends the call with no feature and
 *             no further attempt.
 * Waits once, on the result.  On PRE3_FAST_INITIALISED the call then queues, without a second wait, pre3_map_add_inverse_depth for the one feature
 * (rho = 1 / df) and pre3_patch_cut for the new landmark: the context comes out exactly as if the caller had made those two calls with the returned
 * uv and rho.  The h of the projection are dropped (:211-213): a following stage projects for itself.
 * PRE3_E_ARG before anything is queued: a null frame or result, a frame of another shape or device, std_pxl, attempts outside 1 .. 10, an image
 * smaller than 103 x 83, a centre outside the range that can be drawn.  PRE3_E_STATE likewise: no image, no x_k_k, an unloaded frame.  PRE3_E_NOMEM
 * likewise: no room for one more landmark.  PRE3_E_NUMERIC after the wait, the map untouched: the corner's rho is not finite (a NaN y or z passes
 * the depth gate, as in the reference). */
#define PRE3_FAST_MAX_ATTEMPTS 10      /* initialize_a_feature.m:34 */
#define PRE3_FAST_INITIALISED 0
#define PRE3_FAST_NO_BOX 1             /* every attempt met a box without a corner or with a predicted feature (:176-183) */
#define PRE3_FAST_NO_DEPTH_NAN 2       /* inittialize_depth_my_version.m:40 */
#define PRE3_FAST_NO_DEPTH_NEAR 3      /* :74 df < 0.4 */
#define PRE3_FAST_NO_DEPTH_CONF 4      /* :74 conf <= 0.5 cmax */
typedef struct pre3_fast_init_result {
    int32_t status, attempts;          /* PRE3_FAST_*; attempts used, 1-based */
    int32_t uv[2];                     /* the corner (column, row), 1-based, in the image; zero for PRE3_FAST_NO_BOX */
    int32_t landmark, pad;             /* the new landmark's index, -1 unless PRE3_FAST_INITIALISED */
    double rho, xyz[3];                /* 1 / df and [-x, -y, z] of the pixel: pre3_sr_frame_keypoints' gate-0 outputs, bit for bit; zero when refused */
    int32_t centres[2 * PRE3_FAST_MAX_ATTEMPTS];      /* the (row, column) centres tried; zero behind `attempts` */
} pre3_fast_init_result;
PRE3_API int pre3_init_feature_fast(pre3_ctx *ctx, pre3_sr_frame *frame, double std_pxl, int strict_reference, int threshold, int barrier,
                                    const int32_t *centres /* 2 x attempts */, int attempts, pre3_fast_init_result *out);
PRE3_API int pre3_init_feature_fast_seeded(pre3_ctx *ctx, pre3_sr_frame *frame, double std_pxl, int strict_reference, int threshold, int barrier,
                                           uint64_t seed, uint64_t seq, pre3_fast_init_result *out);
/* initialize_n_features_FAST.m:55-145: the maxima (threshold -1: 5, barrier -1: 20, :69-82) of the image inside the 20-pixel band (:62-64), every
 * one through gate 0 (:118-127), the survivors added in scan order in ONE pre3_map_add_inverse_depth with ONE pre3_patch_cut, queued behind the
 * call's one wait.  K_out maxima; uv_out[2 K] (column, row, 1-based, in the image), rho_out[K] (zero when refused), verdict_out[K]
 * (PRE3_FAST_INITIALISED = kept, or PRE3_FAST_NO_DEPTH_*) -- each may be NULL, else holds PRE3_FAST_MAX_CORNERS entries; n_added_out survivors.
 * Errors as above; more survivors than the context has room for, or more than PRE3_FAST_MAX_CORNERS maxima: PRE3_E_NOMEM, the map untouched. */
PRE3_API int pre3_init_features_fast_all(pre3_ctx *ctx, pre3_sr_frame *frame, double std_pxl, int threshold, int barrier, int32_t *K_out,
                                         int32_t *n_added_out, int32_t *uv_out, double *rho_out, int32_t *verdict_out);

/* ---- the prediction fed from a resident VO pair: u never leaves the device -----------------------------------------------------
 * fv.m:47 + Calculate_V_Omega_RANSAC_dr_ye.m:41-50 + predict_state_and_covariance.m:27-143 in one call: the VO front end between the keypoint records of
 * prev and cur -- exactly pre3_vo_pair_seeded's launches, draw rule and (seed, seq), on cur's stream with prev lent to it --, then the prediction
 * (x_k_k, p_k_k) -> (x_k_km1, p_k_km1) on the context's stream with the increment read from the pair's device result block: cur is lent to the context's
 * stream for that launch and reclaimed behind it, so the next pair call's clearing of the same work block, a pre3_sr_frame_load or a
 * pre3_sr_frame_keypoints on either handle stays behind the read of u.  The increment rule is evaluated on the device: u = [T; R2q(R)] of the pair when
 * its solution state is 1, else [0 0 0 1 0 0 0] -- fewer than four matches (nothing behind the match stage has written the result block, and it is not
 * read), no consensus (sta = 4), sta = 2 / 0 / -1.
 * With pnum_out == NULL and res_out == NULL the call queues everything and returns without synchronising any stream (pre3_heading_from_frame's no-wait
 * form); with either output it ends in ONE host wait, and *pnum_out and *res_out are pre3_vo_pair_seeded's, bit for bit.
 * Afterwards x_k_km1, P, the prediction's parameters, a pending HI down-date's rows (PRE3_OPT_PEND_HI) and a pending update.m:42-46 pass are bit-identical
 * to pre3_vo_pair_seeded(prev, cur, thresh, seed, seq, ..., &res) followed by pre3_predict(ctx, res.u), and the context's flags change as pre3_predict
 * changes them: pending work is carried, not flushed.  (For sta = 2 / 0 / -1 the chain's res.u holds R2q of the identity with negative zeros in
 * u[4..6]; this call takes +0 there.  The values are equal; zero entries of the prediction's parameters may differ in sign.)
 * The two pairs pre3_vo_pair_seeded refuses after its wait -- no matched point beyond 0.4 m (PRE3_E_NUMERIC), a match or a keypoint outside its range
 * (PRE3_E_HIP) -- cannot be refused by a call that does not wait: the prediction is made with the identity increment, which is what the reference's own
 * rule gives every pair that does not end in sta = 1, and x, P and every flag of the context are those of a prediction that has happened.  The no-wait
 * form leaves a value of its own in the context's numeric error word: the next call that reads the error words (pre3_get_state, a step, a reader)
 * returns PRE3_E_NUMERIC once, with a message that names the refused pair, and the word is cleared with that report.  The waiting form returns the code
 * and the message pre3_vo_pair_seeded would, clears the word itself and leaves the context usable, holding that identity prediction.
 * n1 == 0 or n2 == 0 is a result: no pair launches, the ordinary prediction with the identity increment, pnum = 0 and sta = 4.
 * PRE3_E_ARG / PRE3_E_STATE before anything is queued, with the context and both handles unchanged: a null context, everything pre3_vo_pair_seeded
 * refuses before it queues, a handle on another device than the context, a context whose covariance buffer does not hold (x_k_k, p_k_k).
 * Calls that share a handle or the context must be serialised by the caller. */
PRE3_API int pre3_predict_pair_seeded(pre3_ctx *ctx, pre3_sr_frame *prev, pre3_sr_frame *cur, double thresh, uint64_t seed, uint64_t seq,
                                      int32_t *pnum_out, pre3_vo_result *res_out);

/* ---- the prediction's process noise: caller-set, or from the VO pair's inliers on the device ------------------------------------
 * predict_state_and_covariance.m:98-102: Pn (7 x 7, row-major; it is symmetric) of every prediction this context makes -- pre3_predict, pre3_step*,
 * pre3_step_all, pre3_step_seeded, pre3_predict_pair_seeded -- in Q = G Pn G' (:120).  NULL returns to the constant of :98-102, which a context on
 * which nothing was ever set uses exactly as before, bit for bit.  Checked on the host before anything is queued: every entry finite,
 * Pn[i][j] == Pn[j][i], no negative diagonal entry; otherwise PRE3_E_ARG with the context and its setting unchanged.  The block changes in stream order,
 * behind the predictions already queued; nothing is synchronised, and deferred or pending work (PRE3_OPT_DEFER_HI / PRE3_OPT_PEND_HI) is left alone and
 * carried by the predictions as before.  pre3_set_state does not reset the setting; the stateless pre3_predict_dense / pre3_predict_state_and_covariance
 * and snapshots do not know it. */
PRE3_API int pre3_set_process_noise(pre3_ctx *ctx, const double *Pn /* [49] or NULL */);
/* *source_out: 0 the constant, 1 the caller's.  Pn_out[49]: the values in force (source 0: the constant as the prediction's launch builds it on the
 * device; that form synchronises the context's stream).  Either output may be NULL. */
PRE3_API int pre3_get_process_noise(pre3_ctx *ctx, double *Pn_out, int *source_out);

/* aux_code/calc_cov_RANSAC_dr_ye.m:17-30 + aux_code/cov_pose_shift_calc.m:4-40 -- the Pn of predict_state_and_covariance.m:115 --, stateless and fed from
 * the host: pset1 = op_pset1, pset2 = op_pset2 (3 x pnum, column-major), u = [trans; R2q(rot)] of a cached RANSAC_RESULT_%d_%d.mat, inlier[pnum] int32
 * 0/1 (NULL: every point counts).  The SR4000's per-point range and angle noise is propagated through the rigid fit to the 7 x 7 covariance of [T; q]:
 * cov = H^-1 M H^-1 with H = sum H_i the Hessian of E = sum 1/2 |T + R(q) pset2_i - pset1_i|^2 in [T; q] and M = sum B_i Sigma_i B_i' (pre3_vocov.h).
 * This is the implicit-function covariance of the fit; cov_pose_shift_calc.m:14,19's pinv of each point's own rank-deficient Hessian is not built.
 * *status_out: 0 not computed (pnum < 4), 1 valid, 2 unusable (a non-finite inlier coordinate, a Cholesky pivot of H at or below 7 eps times its
 * diagonal entry, a non-finite result).  cov_out[49] (row-major, symmetric) is written on status 1 only.  n_inliers_out may be NULL.  Synchronises. */
PRE3_API int pre3_vo_cov(int device, int pnum, const double *pset1, const double *pset2, const int32_t *inlier, const double u[7], double *cov_out,
                         int32_t *status_out, int32_t *n_inliers_out);

/* pre3_vo_pair_seeded (vodometry_dr_ye.m:84-236) with calc_cov_RANSAC_dr_ye.m:17-30 behind it: one more launch (k_vo_cov) behind the final fit on the same
 * stream, reading the winner's inlier list, pset1 / pset2 and u where they lie; still one host wait.  Every output shared with pre3_vo_pair_seeded is
 * bit-equal to that call's, as are its refusals and errors.  *cov_status_out: 0 not computed (pnum < 4, sta != 1, a refused pair), 1, 2 as pre3_vo_cov's;
 * cov_out[49] is written on status 1 only and is then bit-equal to pre3_vo_cov fed this call's pset1, pset2, inlier list and res->u.  Either may be NULL. */
PRE3_API int pre3_vo_pair_cov_seeded(pre3_sr_frame *prev, pre3_sr_frame *cur, double thresh, uint64_t seed, uint64_t seq, int32_t *pnum_out,
                                     double *match_out, double *pset1_out, double *pset2_out, int32_t *draws_out, int32_t *capped_out,
                                     int32_t *cnum_out, int32_t *state_out, int32_t *inlier_out, pre3_vo_result *res, double *cov_out,
                                     int32_t *cov_status_out);

/* pre3_predict_pair_seeded with the pair's own covariance as this one prediction's Pn (predict_state_and_covariance.m:115): k_vo_cov behind the pair's
 * final fit, and the prediction's launch takes its block when status == 1 and the pair's u is taken (sta == 1, not refused); otherwise the context's own
 * noise -- the caller's (pre3_set_process_noise) or the constant.  u and Pn both stay on the device.  With all four outputs NULL nothing is synchronised;
 * with any of them the call waits once.  The context's noise setting is unchanged afterwards, and the context is bit-identical to the chain
 * pre3_vo_pair_cov_seeded -> (status == 1 and sta == 1: pre3_set_process_noise(cov)) -> pre3_predict(res.u) -> the previous setting restored.
 * Refusals, argument and state errors are pre3_predict_pair_seeded's. */
PRE3_API int pre3_predict_pair_cov_seeded(pre3_ctx *ctx, pre3_sr_frame *prev, pre3_sr_frame *cur, double thresh, uint64_t seed, uint64_t seq,
                                          int32_t *pnum_out, pre3_vo_result *res_out, double *cov_out, int32_t *cov_status_out);

/* ---- dense ICP between two point clouds: the refinement of the VO pair's pose ---------------------------------------------------
 * TestScripts/icp_with_init.m:34-120 (Mian's ICP seeded with Rinit, Tinit; the icp(Ya, Yb) lines of TestScripts/ICP_RANSAC*.m and
 * RANSAC_CALC_VER_test.m:77-78, which the reference leaves commented out): data1 the model, data2 the source, both 3 x n column-major; data2 <- Rinit data2
 * + Tinit (:34-35); per iteration the exact nearest model point of every source point (dsearchn without its triangulation: d = dx dx + dy dy + dz dz
 * summed in that order, D = sqrt(d), a tie to the lowest model index), D > 2 res dropped (:51), one pair per model index -- the smallest D, on equal D
 * the highest source index: sortrows and the 2005 code's unique, which kept the LAST occurrence (:53-56) --, reg (:103-120: means, K = Sshifted
 * Mshifted' / n, R1 = V U' with the det < 0 repair, t1 = mm - R1 ms), data2 <- R1 data2 + t1 in place, R <- R1 R, t <- R1 t + t1; the two loops of
 * :47-68 and :74-99 literally (maxIter 30 and `n > maxIter` after the increment: at most 31 iterations each, 62 in all); error = min(e1, e2) (:100).
 * One deliberate departure: length(corr) is max(p, 3) for a p x 3 array and the reference fails at p = 0; here an iteration that finds p < 3 pairs ends
 * the run with sta = 2 and the transform accumulated so far.  All fp64 on the device, no contraction; 5 launches per iteration, all 62 iterations queued
 * at once (a launch behind the end of the run returns at once), ONE host wait.  Results are bit-equal from run to run. */
#define PRE3_ICP_MAX_ITERATIONS 62
typedef struct pre3_icp_result {
    double R[9], t[3];          /* the accumulated registration of the seeded source (row-major): registered = R (Rinit data2 + Tinit) + t */
    double Rtot[9], ttot[3];    /* R Rinit, R Tinit + t: data1 ~ Rtot data2 + ttot */
    double u[7];                /* [ttot; R2q(Rtot)] as pre3_vo_result's u (Calculate_V_Omega_RANSAC_dr_ye.m:40-50) */
    double error;               /* :100 */
    int32_t sta;                /* 0 not run (pre3_icp_pair_seeded: the pair did not end in sta == 1; nothing else is written), 1 ended by the reference's
                                   rule, 2 an iteration found fewer than three pairs (or, in the *_frames forms, a cloud kept fewer than three points) */
    int32_t p;                  /* rows of corr: the last iteration's pairs */
    int32_t iters1, iters2;     /* iterations of :47-68 and of :74-99 (one that found p < 3 included) */
    int32_t n_model, n_source;  /* points of either cloud (the *_frames forms: pixels kept) */
    int32_t pad;
} pre3_icp_result;
/* Stateless, host in and host out.  Rinit[9] row-major, Tinit[3] (NULL: identity / zero).  Outputs, each may be NULL: out; corr_out[p][3] = (model,
 * source, D) per row, indices 1-based, ascending in the model index (sized by the caller for min(n1, n2) rows); data2_out 3 x n2, the registered source;
 * log_out[62][3] = (phase, p, sum(D) / (p res)) per iteration run, zero rows behind.  PRE3_E_ARG before anything is queued: n1 < 3, n2 < 3, res not
 * positive and finite.  A non-finite coordinate is found on the device: PRE3_E_NUMERIC after the wait, no output written. */
PRE3_API int pre3_icp(int device, const double *data1, int n1, const double *data2, int n2, double res, const double Rinit[9], const double Tinit[3],
                      pre3_icp_result *out, double *corr_out, double *data2_out, double *log_out);
/* out = { source points per workgroup of the nearest-neighbour launch, model points per workgroup (the chunk staged in LDS), source points per lane,
 * the iteration cap } */
PRE3_API int pre3_icp_limits(int32_t out[4]);
/* pre3_icp on two resident frames: the model is every pixel of prev's filtered planes as [-x; -y; z] (ransac_dr_ye.m:17-18, the frame the VO pair's
 * R, T live in) in column-major pixel order, the source cur's pixels at rows and columns 0, stride, 2 stride, ... in the same order.  A pixel with a
 * non-finite coordinate or z <= 0 is dropped from either side by an order-preserving compaction on the device; no plane is read back.  out->n_model /
 * n_source are the kept counts; corr's indices are positions in the kept lists, corr_pix_out[p][2] the 0-based column-major pixel indices (model,
 * source) of the same rows; data2_out is sized for the candidate count ceil(rows / stride) ceil(cols / stride).  On cur's stream with prev lent to it.
 * PRE3_E_ARG / PRE3_E_STATE before anything is queued, the handles unchanged: a null handle, prev == cur, different devices or sizes, nothing loaded,
 * stride < 1, res not positive and finite. */
PRE3_API int pre3_icp_frames(pre3_sr_frame *prev, pre3_sr_frame *cur, int stride, double res, const double Rinit[9], const double Tinit[3],
                             pre3_icp_result *out, double *corr_out, int32_t *corr_pix_out, double *data2_out, double *log_out);
/* vodometry_dr_ye.m:139-236 with icp_with_init.m behind it: pre3_vo_pair_seeded's launches, then pre3_icp_frames' on the same stream with Rinit, Tinit
 * read from the pair's result block on the device.  A pair that does not end in sta == 1 (fewer than four matches included): the ICP launches return at
 * once, icp->sta = 0 and no other ICP output is written.  One host wait.  The pair's outputs, refusals and errors are pre3_vo_pair_seeded's, bit for
 * bit; the ICP's outputs are bit-equal to pre3_icp_frames fed res->rot, res->trans. */
PRE3_API int pre3_icp_pair_seeded(pre3_sr_frame *prev, pre3_sr_frame *cur, double thresh, uint64_t seed, uint64_t seq, int stride, double res,
                                  int32_t *pnum_out, double *match_out, double *pset1_out, double *pset2_out, int32_t *draws_out, int32_t *capped_out,
                                  int32_t *cnum_out, int32_t *state_out, int32_t *inlier_out, pre3_vo_result *vo_res, pre3_icp_result *icp,
                                  double *corr_out, int32_t *corr_pix_out, double *data2_out, double *log_out);
/* measurement only: the nearest-neighbour launch of one iteration on resident clouds, averaged over reps */
PRE3_API int pre3_icp_nn_bench(int device, const double *data1, int n1, const double *data2, int n2, int reps, double *ms_per_launch_out);

/* ---- the closed-form covariance of the ICP's increment over its final correspondences -------------------------------------------
 * aux_code/d2E_*_4cov.m, dE_*_4cov.m and Calc_derivatives_for_covariance.m (the derivatives of the rigid fit's energy) with
 * aux_code/cov_pose_shift_calc.m:24-40 (the SR4000's per-point range and angle noise), evaluated over the pairs TestScripts/icp_with_init.m:76-89 ends
 * with: pre3_vo_cov's cov = H^-1 M H^-1 (pre3_vocov.h), with f_p = data1(:, corr(k, 1)) the model point and f_n = data2(:, corr(k, 2)) the ORIGINAL
 * source point -- data2 as pre3_icp took it, before Rinit / Tinit and before any registration step -- and r = T + R(q) f_n - f_p, u = [T; q] = the run's
 * u (data1 ~ Rtot data2 + ttot).  Stateless, host in and host out: data1 3 x n1, data2 3 x n2 (column-major), corr[p][2] int32 1-based (model, source)
 * rows, u[7].  Two launches: one partial sum per 256 pairs, then one workgroup that adds the partials in a tree whose shape depends on p alone, factors H
 * and solves; all fp64, no floating-point atomics, bit-equal from run to run.  *status_out: 0 not computed (p < 4), 1 valid, 2 unusable (a non-finite
 * coordinate in a pair, a Cholesky pivot of H at or below 7 eps times its diagonal entry, a non-finite result).  cov_out[49] (row-major, symmetric) is
 * written on status 1 only; *n_out (may be NULL) the pairs summed.  PRE3_E_ARG before anything is queued: a null cloud, list, u or status_out, an empty
 * cloud, p < 0 or beyond 256 x 256 x limits[1] pairs, an index outside its cloud.  Synchronises.
 * The estimate propagates sensor noise only: on two independent samplings of one surface it gives a sigma_T of millimetres while the registration itself
 * ends centimetres from the true pose, so as a process noise it is optimistic. */
PRE3_API int pre3_icp_cov(int device, const double *data1, int n1, const double *data2, int n2, const int32_t *corr, int p, const double u[7],
                          double *cov_out, int32_t *status_out, int32_t *n_out);
/* out = { pairs per workgroup of the partial-sum launch, partials a thread of the finishing workgroup adds at the largest supported p } */
PRE3_API int pre3_icp_cov_limits(int32_t out[2]);
/* measurement only: pre3_icp_cov's two launches on resident operands (p >= 4), back to back between two events, averaged over reps */
PRE3_API int pre3_icp_cov_bench(int device, const double *data1, int n1, const double *data2, int n2, const int32_t *corr, int p, const double u[7],
                                int reps, double *ms_per_pair_of_launches_out);
/* pre3_icp_pair_seeded with both covariances behind it, still one host wait: k_vo_cov behind the pair's final fit (pre3_vo_pair_cov_seeded's), and the two
 * launches of pre3_icp_cov behind the ICP's last launch, reading the final pairs, the model, u and -- through the kept-pixel list -- cur's filtered planes
 * as [-x; -y; z] where they lie.  Every output shared with pre3_icp_pair_seeded is bit-equal to that call's, as are its refusals and errors; cov_pair_out
 * and *cov_pair_status_out are pre3_vo_pair_cov_seeded's.  *cov_icp_status_out: 0 not computed (the ICP did not end in sta == 1, or p < 4), 1, 2 as
 * pre3_icp_cov's; cov_icp_out[49] is written on status 1 only and is then bit-equal to pre3_icp_cov fed the two clouds gathered through corr_pix_out, this
 * call's pairs and icp->u.  Each of the four may be NULL. */
PRE3_API int pre3_icp_pair_cov_seeded(pre3_sr_frame *prev, pre3_sr_frame *cur, double thresh, uint64_t seed, uint64_t seq, int stride, double res,
                                      int32_t *pnum_out, double *match_out, double *pset1_out, double *pset2_out, int32_t *draws_out,
                                      int32_t *capped_out, int32_t *cnum_out, int32_t *state_out, int32_t *inlier_out, pre3_vo_result *vo_res,
                                      pre3_icp_result *icp, double *corr_out, int32_t *corr_pix_out, double *data2_out, double *log_out,
                                      double *cov_pair_out, int32_t *cov_pair_status_out, double *cov_icp_out, int32_t *cov_icp_status_out);

/* The prediction fed from the ICP-refined pair on the device (fv.m:47 + Calculate_V_Omega_RANSAC_dr_ye.m:41-50 + predict_state_and_covariance.m:27-143,
 * :115 with TestScripts/icp_with_init.m's refinement in between -- the RANSAC_CALC_VER_test.m:77-78 the reference leaves commented out): the launches of
 * pre3_icp_pair_cov_seeded on cur's stream, then k_predict on the context's with u and Pn chosen on the device; neither u nor a covariance crosses PCIe.
 *   u:  the pair not taken (pre3_predict_pair_seeded's rule: pnum < 4, a refused pair, sta != 1): the identity increment, refusals reported exactly as
 *       pre3_predict_pair_seeded reports them.  The pair taken: the ICP's u when icp sta == 1, every entry of it is finite and icp error <= max_error
 *       (+inf: no gate); otherwise the pair's own u.
 *   Pn: `noise` is one of */
#define PRE3_NOISE_CONTEXT 0    /* the context's own noise: pre3_set_process_noise's, or the constant */
#define PRE3_NOISE_PAIR 1       /* the pair's RANSAC covariance under pre3_predict_pair_cov_seeded's rule, else the context's */
#define PRE3_NOISE_ICP 2        /* the ICP's covariance when the ICP's u is taken and its status is 1; else as PRE3_NOISE_PAIR */
#define PRE3_NOISE_ICP_FLOOR 3  /* as PRE3_NOISE_ICP, but Pn = cov_icp + the context's noise, one fp64 addition per entry */
/* PRE3_NOISE_ICP is the published closed-form estimator and is optimistic: it propagates sensor noise only (see pre3_icp_cov).  PRE3_NOISE_ICP_FLOOR lets
 * pre3_set_process_noise act as a floor under it.
 * taken_out[2] = { which u: 0 identity, 1 the pair's, 2 the ICP's; which noise: a PRE3_NOISE_* value }.  cov_out[2][49] / cov_status_out[2]: the pair's
 * and the ICP's covariance and status as pre3_icp_pair_cov_seeded hands them out (cov written on status 1 only).  With every output NULL nothing is
 * synchronised; otherwise the call waits once.  Afterwards the context (x_k_km1, P, the prediction's parameters, pending rows, flags) is bit-identical
 * to the chain pre3_icp_pair_cov_seeded -> the rule above on the host -> pre3_set_process_noise(the taken Pn) when one is taken -> pre3_predict(the
 * taken u) -> the previous setting restored (as for pre3_predict_pair_seeded, the identity's zeros are +0), and the context's noise setting is unchanged.
 * (One combination has no such chain: PRE3_NOISE_ICP_FLOOR on a context that runs on the constant, whose quaternion block is symmetric only to the last
 * place as the launch builds it, so pre3_set_process_noise would refuse the sum; the prediction adds the two blocks entry by entry all the same.)
 * PRE3_E_ARG / PRE3_E_STATE before anything is queued, the context and both handles unchanged: everything pre3_predict_pair_seeded and
 * pre3_icp_pair_seeded refuse there, max_error NaN or <= 0, noise outside 0 .. 3.  The ICP's device block belongs to cur's handle and outlives the
 * prediction's read.  Calls that share a handle or the context must be serialised by the caller. */
PRE3_API int pre3_predict_icp_pair_seeded(pre3_ctx *ctx, pre3_sr_frame *prev, pre3_sr_frame *cur, double thresh, uint64_t seed, uint64_t seq, int stride,
                                          double res, double max_error, int noise, int32_t *pnum_out, pre3_vo_result *vo_res_out,
                                          pre3_icp_result *icp_out, double *cov_out, int32_t *cov_status_out, int32_t *taken_out);

/* ---- the camera pose from 3-D / 2-D correspondences: EPnP, its RANSAC ------------------------------------------------------------
 * aux_code/EPnP_matlab/EPnP/efficient_pnp.m:34-175 (Moreno-Noguer, Lepetit, Fua, ICCV 2007) for kernel dimensions 1, 2 and 3 -- the solver
 * mex_files/RANSAC_CALCULATION/RANSAC_CALC_VER2.m:187-191 leaves commented out: the pose of 3-D points of one frame against the PIXELS of another, with
 * no use of the second frame's depth.  Control points Cw = [e1; e2; e3; 0] (define_control_points.m: not centred on the data), M of
 * compute_M_ver2.m:32-52 from A = [f 0 Cx; 0 f Cy; 0 0 1], the kernel vectors of kernel_noise.m:19-22 by a cyclic Jacobi eigensolver, scale and
 * sign by compute_norm_sign_scaling_factor.m:26-61 (the whole Xc negated if any z < 0), getrotT (:179-205; R = -R, the whole matrix, if det R < 0),
 * the mean pixel distance of :210-226 (no test on depth); dimension 3 is entered only if min(err) > 20 px after the first two (:98); the answer is
 * [min_err, best] = min(err), the first index on ties (:171).  eig leaves a vector's sign open and the z < 0 rule makes a mixed-sign answer depend on
 * it, so each kernel vector's entry of largest magnitude is made positive first.  Dimension 4 (:129-169) is NOT built -- its result depends on the basis
 * null() happens to return: where the reference would enter it (min(err) > 20 after dimension 3) the answer is the best of the three with sta = 2.
 * All fp64; every sum over the points is a tree whose shape depends on the count alone: bit-equal from run to run. */
typedef struct pre3_pnp_result {
    double R[9], T[3];      /* row-major; Xc = R Xw + T (efficient_pnp.m:171-174) */
    double u[7];            /* the pair's convention: [-R'T; R2q(R')] -- pset1 ~ rot pset2 + trans, what pre3_predict takes; the identity unless sta is 1 or 2 */
    double err[3];          /* err(1..3); NaN where a dimension was not computed */
    int32_t best;           /* 0-based dimension of the answer */
    int32_t sta;            /* 1 ok; 2 best of three, the reference would go on to dimension 4; -1 a non-finite intermediate; 0 not computed */
    int32_t n;              /* correspondences the answer was computed from */
    int32_t n_support;      /* RANSAC forms: the winner's support; else n */
} pre3_pnp_result;
/* Stateless, host in and host out, synchronises.  Xw[3 x n], U[2 x n] column-major (one correspondence a column).  undistort = 0 uses the pixels as they
 * are (the commented-out line's cam.K); undistort = 1 passes every pixel through undistort_fm_my_version.m:56-81's ten Newton steps first -- the form to
 * use on real frames: the SR4000's k1 = -0.84656 moves a corner pixel by more than ten pixels.  PRE3_E_ARG: n < 6 or beyond pre3_pnp_limits, a null pointer,
 * cam->f <= 0.  A non-finite coordinate gives sta = -1. */
PRE3_API int pre3_epnp(int device, const pre3_cam *cam, int undistort, int n, const double *Xw, const double *U, pre3_pnp_result *res);
/* n_hyp in [1, limits[1]] six-point hypotheses, all evaluated (no early exit: the reference has no PnP RANSAC and its count rule is not borrowed).
 * draws[n_hyp][6]: 0-based indices, distinct within a row (else PRE3_E_ARG).  Every hypothesis is solved as pre3_epnp solves six correspondences and all n
 * are scored under its answer: an inlier has a reprojection distance < thr_px and a camera-frame z > 0.  support_out[n_hyp], state_out[n_hyp] (the
 * hypothesis' sta; a non-finite pose: support 0, state -1), hyp_res_out[n_hyp] (may be NULL; n_support = the hypothesis' support).  The winner: the largest
 * support, then the smallest sum of inlier distances, then the lowest index (RANSAC_CALC_VER2.m:165-172's rule); inlier_out[n] its 0/1 flags.  res: the
 * EPnP refit over the winner's inliers, read on the device; support below 6: sta = 0, n_support as found.  Stateless, host in and host out, synchronises: the two uploads, three launches, one copy back.
 * With sta 0 or -1 (here and in pre3_epnp) R is the identity, T zero and u the identity increment.
 * PRE3_E_ARG besides pre3_epnp's: n_hyp out of range, thr_px not positive and finite, a null table. */
PRE3_API int pre3_pnp_ransac(int device, const pre3_cam *cam, int undistort, int n, const double *Xw, const double *U, int n_hyp, const int32_t *draws,
                             double thr_px, int32_t *support_out, int32_t *state_out, int32_t *inlier_out, pre3_pnp_result *hyp_res_out, pre3_pnp_result *res);
/* the same with the table drawn on the device in front (one more launch): six distinct of n per hypothesis on Philox stream 6, counter
 * [hypothesis, block, seq, 0] -- ranks in [0,n), [0,n-1), ..., each shifted past the earlier picks (DESIGN.md section 18's rule for three, continued).
 * draws_out[n_hyp][6] may be NULL.  Bit-identical to pre3_pnp_ransac fed that table. */
PRE3_API int pre3_pnp_ransac_seeded(int device, const pre3_cam *cam, int undistort, int n, const double *Xw, const double *U, int n_hyp, uint64_t seed,
                                    uint64_t seq, double thr_px, int32_t *draws_out, int32_t *support_out, int32_t *state_out, int32_t *inlier_out,
                                    pre3_pnp_result *hyp_res_out, pre3_pnp_result *res);
/* RANSAC_CALC_VER2.m:191 in place: pre3_vo_pair_seeded's launches, and behind them on the same stream the EPnP of pre3_epnp over the pair's inliers,
 * read on the device through the pair's inlier flags -- Xw = pset1, prev's range points [-x; -y; z]; U = entries 0 and 1 of cur's kept keypoint frame at
 * match(2, i), the uv pre3_map_policy_frames_seeded hands the map -- so the pose uses no depth of cur.  Still ONE host wait.  Every output shared with
 * pre3_vo_pair_seeded is bit-equal to that call's, as are its refusals and errors; pix2_out[2 x pnum] (may be NULL) the pixels of all matches; pnp is
 * bit-equal to pre3_epnp on pset1_out and pix2_out gathered at the inliers, with n_support the pair's, and pnp->u is in the pair's convention (comparable
 * with res->u).  The pair's sta != 1, fewer than four matches or fewer than six inliers: pnp->sta = 0, R and u the identity.  PRE3_E_ARG besides the
 * pair's: a null cam or pnp, cam->f <= 0. */
PRE3_API int pre3_vo_pair_pnp_seeded(pre3_sr_frame *prev, pre3_sr_frame *cur, double thresh, uint64_t seed, uint64_t seq, const pre3_cam *cam, int undistort,
                                     int32_t *pnum_out, double *match_out, double *pset1_out, double *pset2_out, int32_t *draws_out, int32_t *capped_out,
                                     int32_t *cnum_out, int32_t *state_out, int32_t *inlier_out, pre3_vo_result *res, double *pix2_out, pre3_pnp_result *pnp);
/* out = { the largest n, the largest n_hyp } */
PRE3_API int pre3_pnp_limits(int32_t out[2]);
/* measurement only: pre3_pnp_ransac_seeded's four launches on resident operands, back to back between two events, averaged over reps */
PRE3_API int pre3_pnp_bench(int device, const pre3_cam *cam, int undistort, int n, const double *Xw, const double *U, int n_hyp, uint64_t seed, uint64_t seq,
                            double thr_px, int reps, double *ms_per_ransac_out);

/* ---- relocalising a lost filter: the EPnP pose of the whole map against the scan as this frame's prediction --------------------
 * The project's own follow-up of sections 9 and 35: the reference has no relocalisation.  The call REPLACES the prediction of the frame on which the
 * caller has judged the filter lost (that judgement is not made here).  On the context's stream, no host wait between the stages:
 *   1. siftmatch(bank(128 x N), Descriptor_RAW(128 x K2), thresh) over ALL N landmarks -- the double class, the ratio test in float, the first index on
 *      ties: the match list of pre3_siftmatch_f64 on pre3_get_descriptors and the scan.  No window gate, no descriptor refresh; h, H, S, z, the flags
 *      and the bank are not touched.
 *   2. per match (k1, k2), in ascending k1: Xw = the landmark's point at x_k_k, bit-equal to pre3_get_landmarks' xyz (both landmark types), and
 *      U = entries 0 and 1 of the scan's SCALE_ORIENT_POS_RAW at k2 -- what pre3_ic_search installs as z.  A match whose point is not finite (an
 *      inverse depth of 0) is left out, order kept; two landmarks may match one keypoint, both stay.
 *   3. pre3_pnp_ransac_seeded's four launches over those n_corr correspondences, the count read on the device: draws draw_rule_pnp(seed, seq, n_corr, h).
 *      n_corr < 6: no hypothesis is solved, winner = -1, pnp.sta = 0.
 *   4. the prediction, with u and Pn chosen on the device: the pose is taken iff pnp.sta == 1 and pnp.n_support >= min_support.  Taken: with
 *      [r*; q*] = pnp.u = [-R'T; R2q(R')] and [r; q] = x_k_k[0:7], dX = R(q)'(r* - r), dq = conj(q) (x) q* / |q|^2, negated if its scalar part is
 *      negative (q stays in the hemisphere the cross-covariances of P were built in), and Pn = Pn_reloc, a wide noise of the caller's so that P stays a
 *      consistent covariance.  Not taken: u = [0 0 0 1 0 0 0] and the context's own noise (pre3_set_process_noise's, or the constant).
 * The ordinary step (pre3_ic_search, pre3_step*) follows as after any prediction.  A deferred HI update is completed first, P follows pre3_predict, and
 * the context's noise setting is unchanged afterwards.  Bit-equal to the chain pre3_get_landmarks, pre3_siftmatch_f64, a gather of the finite matches,
 * pre3_pnp_ransac_seeded, pre3_set_process_noise(Pn_reloc) when taken, pre3_predict(u), the noise setting restored.  Nothing crosses PCIe but the result
 * block; ONE host wait, none when res_out, pairs_out and inlier_out are all NULL.  No allocation: the work block is sized at pre3_create.
 * pairs_out: the first 2 * n_matches entries are written; inlier_out: the winner's 0/1 flags over the n_corr correspondences.
 * PRE3_E_STATE (nothing queued, the context unchanged): no descriptor bank, no scan (or an empty one), the covariance buffer does not hold (x_k_k, p_k_k).
 * PRE3_E_ARG (the same): N < 6 or beyond pre3_reloc_limits, n_hyp outside 1 .. 700, thr_px or thresh not positive and finite, min_support < 6,
 * Pn_reloc null or refused by pre3_set_process_noise's checks (finite, no negative diagonal entry, exactly symmetric), no camera set. */
typedef struct pre3_reloc_result {
    pre3_pnp_result pnp;     /* the refit over the winner's inliers, as pre3_pnp_ransac_seeded's res */
    double u[7];             /* the increment the prediction applied (identity when not taken) */
    int32_t n_matches;       /* matches of siftmatch(bank, scan) */
    int32_t n_corr;          /* of those, correspondences with a finite 3-D point: the PnP's n */
    int32_t winner;          /* winning hypothesis, -1 if none ran */
    int32_t taken;           /* 1: pose taken; 0: identity u and the context's own noise */
} pre3_reloc_result;
PRE3_API int pre3_relocalise_seeded(pre3_ctx *ctx, double thresh, int n_hyp, uint64_t seed, uint64_t seq, double thr_px, int undistort, int min_support,
                                    const double *Pn_reloc /* [49] */, pre3_reloc_result *res_out,
                                    int32_t *pairs_out /* [2 * N] (k1, k2) 0-based, may be NULL */, int32_t *inlier_out /* [N] over the correspondences, may be NULL */);
/* out = { the largest N, the largest n_hyp } the call takes */
PRE3_API int pre3_reloc_limits(int32_t out[2]);

/* ---- the PnP pose refined by Gauss-Newton, its covariance, and relocalising under it ---------------------------------------------
 * The project's own follow-up of sections 35 and 36.  EPnP minimises a linearised quantity, not the reprojection error it is scored by; the reference
 * puts a Gauss-Newton stage behind the same solver (aux_code/EPnP_matlab/EPnP/efficient_pnp_gauss.m:191-225) and keeps its result "if Gauss Newton
 * improves results" -- over the betas against control-point distances, another quantity and without a covariance; only its taking rule is followed.
 * Here: Gauss-Newton on the reprojection error over the six pose parameters, d = (tau, omega) on the camera side (R <- E R, T <- E T + tau,
 * E = exp([omega]x)), exactly n_iter plain steps over a fixed point set, no damping and no early exit; cost[k] = r'r (px^2, undistorted pixels when
 * undistort = 1) before step k and cost[n_iter] after the last.  The refined pose is taken iff n_iter >= 1, every intermediate is finite, every point has
 * z > 0 at the refined pose and cost[n_iter] < cost[0]; otherwise the input pose is kept.  cov6 = sigma2 (J'J)^-1 at the pose the call ends on, in
 * (tau, omega); sigma2 = sigma_px^2, or cost / (2 n - 6) when sigma_px == 0.  cov = Jm cov6 Jm' is the covariance of u (rank 6; null vector [0; q*]).
 * THE COVARIANCE TREATS THE 3-D POINTS AS EXACT: it carries pixel noise only, neither the landmarks' own uncertainty nor their correlation with the
 * pose.  Like pre3_icp_cov's it is optimistic; on a real map use PRE3_RELOC_NOISE_POSE_FLOOR.
 * All fp64, every sum over the points the fixed tree of pre3_epnp: bit-equal from run to run. */
#define PRE3_PNP_REFINE_MAX_ITER 10
typedef struct pre3_pnp_refine_result {
    double R[9], T[3];      /* the pose the call ends on: refined (sta 1) or the input's (every other sta) */
    double u[7];            /* its [-R'T; R2q(R')]; with sta 0 or -1 the input's */
    double cost[11];        /* r'r before step k, after the last at [n_iter]; NaN beyond n_iter (all NaN with sta 0) */
    double cov6[36];        /* row-major, (tau, omega); NaN with sta 0 or -1 */
    double cov[49];         /* row-major, of u; NaN with sta 0 or -1 */
    double sigma2;          /* the s^2 the covariances carry; NaN with sta 0 or -1 */
    int32_t sta;            /* 1 refined pose taken, covariance valid; 2 input pose kept, covariance valid; -1 no covariance (a pivot of J'J at or below
                               7 eps times its diagonal entry, a non-finite coordinate or result, a depth <= 0 at the pose the call ends on); 0 not computed
                               (the pose fed in has sta outside {1, 2}, or fewer than six points) */
    int32_t n;              /* points the sums ran over */
    int32_t n_iter;
    int32_t pad;
} pre3_pnp_refine_result;
/* Stateless, host in and host out, one launch, synchronises.  Xw, U, undistort as pre3_epnp; R0[9] row-major, T0[3]: the starting pose.
 * PRE3_E_ARG: pre3_epnp's refusals, n_iter outside 0 .. 10, sigma_px negative or not finite, a null R0 or T0. */
PRE3_API int pre3_pnp_refine(int device, const pre3_cam *cam, int undistort, int n, const double *Xw, const double *U, const double *R0, const double *T0,
                             int n_iter, double sigma_px, pre3_pnp_refine_result *res);
/* pre3_pnp_ransac_seeded's four launches, then the refinement over the winner's inlier list from the refit's result block, both read on the device.
 * Still ONE host wait.  Every output shared with pre3_pnp_ransac_seeded is bit-equal to that call's; ref is bit-equal to pre3_pnp_refine on the
 * correspondences gathered at inlier_out, started from res->R, res->T (res->sta outside {1, 2}: ref->sta = 0). */
PRE3_API int pre3_pnp_ransac_refined_seeded(int device, const pre3_cam *cam, int undistort, int n, const double *Xw, const double *U, int n_hyp, uint64_t seed,
                                            uint64_t seq, double thr_px, int32_t *draws_out, int32_t *support_out, int32_t *state_out, int32_t *inlier_out,
                                            pre3_pnp_result *hyp_res_out, pre3_pnp_result *res, int n_iter, double sigma_px, pre3_pnp_refine_result *ref);
/* pre3_relocalise_seeded with the refinement between the refit and the prediction (one more launch, still one wait, none with every output NULL).
 * Whether the pose is taken: pre3_relocalise_seeded's rule on the EPnP refit, unchanged.  u: from ref.u when ref.sta == 1, else from pnp.u.  The noise
 * of a taken pose: */
#define PRE3_RELOC_NOISE_CALLER 0      /* Pn_reloc, as pre3_relocalise_seeded */
#define PRE3_RELOC_NOISE_POSE 1        /* Jd ref.cov Jd', Jd = blkdiag(R(q)', L(conj q) / |q|^2) at x_k_k's q -- ref.cov carried through the rule that makes
                                          the increment of u -- when ref.sta is 1 or 2; else Pn_reloc */
#define PRE3_RELOC_NOISE_POSE_FLOOR 2  /* the same plus Pn_reloc entry by entry, one fp64 addition each: the caller's block is a floor */
/* Not taken: the identity u and the context's own noise.  Afterwards the context is bit-identical to the chain pre3_get_landmarks, pre3_siftmatch_f64,
 * the gather, pre3_pnp_ransac_refined_seeded, the two rules on the host, pre3_set_process_noise(Pn) when taken, pre3_predict(u), the setting restored.
 * Refusals: pre3_relocalise_seeded's, and PRE3_E_ARG for n_iter outside 0 .. 10, sigma_px negative or not finite, noise outside 0 .. 2. */
typedef struct pre3_reloc_refined_result {
    pre3_reloc_result base;          /* as pre3_relocalise_seeded's, u the increment this call applied */
    pre3_pnp_refine_result ref;
    double Pn[49];                   /* the process noise the prediction used */
    int32_t noise_taken;             /* its source: PRE3_RELOC_NOISE_CALLER, _POSE or _POSE_FLOOR; -1 the context's own (the pose not taken) */
    int32_t pad;
} pre3_reloc_refined_result;
PRE3_API int pre3_relocalise_refined_seeded(pre3_ctx *ctx, double thresh, int n_hyp, uint64_t seed, uint64_t seq, double thr_px, int undistort, int min_support,
                                            int n_iter, double sigma_px, int noise, const double *Pn_reloc /* [49] */, pre3_reloc_refined_result *res_out,
                                            int32_t *pairs_out /* [2 * N], may be NULL */, int32_t *inlier_out /* [N], may be NULL */);

/* ---- a10: sift/siftmatch.c:83-132,139-250 ------------------------------------------------------- */
/* L1: ND x K1, L2: ND x K2, one descriptor per column (column-major, as mxGetData returns them).
 * pairs_out[2*K1] receives 1-based (k1,k2) doubles in increasing k1 exactly as the MEX writes them
 * (:241-242); score_out[K1] (may be NULL) the best squared distance; *M_out the number of matches.
 * Accumulation follows the class promotion of :61-64 (double, float, int, int); the ratio test is in
 * float (:122).  Ties keep the first index (:110-116). */
PRE3_API int pre3_siftmatch_f64(int device, int ND, int K1, const double *L1, int K2, const double *L2, double thresh,
                                double *pairs_out, double *score_out, int *M_out);
PRE3_API int pre3_siftmatch_f32(int device, int ND, int K1, const float *L1, int K2, const float *L2, double thresh,
                                double *pairs_out, double *score_out, int *M_out);
PRE3_API int pre3_siftmatch_u8(int device, int ND, int K1, const uint8_t *L1, int K2, const uint8_t *L2, double thresh,
                               double *pairs_out, double *score_out, int *M_out);
PRE3_API int pre3_siftmatch_i8(int device, int ND, int K1, const int8_t *L1, int K2, const int8_t *L2, double thresh,
                               double *pairs_out, double *score_out, int *M_out);

/* Sharded matcher (database columns [k2_begin,k2_end) of L2 on this GPU): per query the local best,
 * second best (as double) and the GLOBAL 0-based index of the best, for the all-gather + merge of
 * DESIGN.md section "multi-GPU".  cls: 0 f64, 1 f32, 2 u8, 3 i8.  best/second/arg: host arrays [K1]. */
PRE3_API int pre3_siftmatch_partial(int device, int cls, int ND, int K1, const void *L1, int K2_local, const void *L2_local,
                                    int k2_offset, double *best, double *second, int32_t *arg);
/* merge G shards' partials (best[g*K1+k1] ...) and apply the ratio test; same outputs as pre3_siftmatch_* */
PRE3_API int pre3_siftmatch_merge(int cls, int G, int K1, const double *best, const double *second, const int32_t *arg,
                                  double thresh, double *pairs_out, double *score_out, int *M_out);

/* Device-resident database shard of the sharded matcher (uint8 class: BASELINE.json configs[3]).  The queries L1 (replicated on every
 * rank) and this rank's database slice L2_local = columns [k2_offset, k2_offset + K2_local) of the whole L2 are packed once into HBM.
 * pre3_match_shard_run leaves the slice's per-query partials on the DEVICE as double[3][K1] = best | second | global arg (arg < 0: none)
 * and returns their address: the caller all-gathers them with RCCL (device memory, no host staging) into double[G][3][K1] and hands that
 * DEVICE buffer to pre3_match_shard_merge, which merges (ties -> lowest index), applies Lowe's test in float (siftmatch.c:122) and
 * compacts the matches in increasing k1 on the device; only the M pairs cross PCIe.  Results are identical to pre3_siftmatch_u8 on the
 * whole database for any number of shards. */
typedef struct pre3_match_shard pre3_match_shard;
PRE3_API int pre3_match_shard_create(pre3_match_shard **out, int device, int ND, int K1, const uint8_t *L1, int K2_local, const uint8_t *L2_local, int k2_offset);
/* the same for any class the matrix cores serve: cls 0 double (what matching_sift_based.m:104-118 passes), 1 float, 2 uint8.  double / float
 * need ND <= 128 and K1 * K2_local >= 65536 (else PRE3_E_ARG: use pre3_siftmatch_partial); the ratio test is siftmatch.c:122's for every class */
PRE3_API int pre3_match_shard_create_cls(pre3_match_shard **out, int device, int cls, int ND, int K1, const void *L1, int K2_local, const void *L2_local, int k2_offset);
PRE3_API int pre3_match_shard_run(pre3_match_shard *s, void **partial_dev, int *n_doubles);
PRE3_API int pre3_match_shard_merge(pre3_match_shard *s, int G, const void *gathered_dev, double thresh, double *pairs_out, double *score_out, int *M_out);
PRE3_API int pre3_match_shard_destroy(pre3_match_shard *s);

/* ---- the RCCL communicator: collectives enqueued by the library on its own stream ------------------------------------------------------
 * SURVEY section 8(e) / BASELINE.json north_star ("RCCL all-reduce of inlier counts over xGMI"): the two stages that shard exchange data once
 * per round.  With a communicator attached, the library itself enqueues that collective between its kernels, on the stream they run on:
 *   pre3_ransac_sharded    H*P / H*P*H' of the slice's measurements, scoring of hypotheses [lo, hi) of this rank, ncclAllReduce (int32 sum, in
 *                          place, supports + inlier bitmasks in ONE call), the selection kernel (ransac_hypotheses.m:41-62 replayed on the
 *                          reduced buffers) -- one host wait (the pinned mailbox) per round;
 *   pre3_match_shard_match distance kernel on the resident slice, ncclAllGather of the per-query partials, merge + Lowe's test + compaction,
 *                          result block written to pinned host memory by the merge kernel -- one host wait per match.
 * One process per GPU.  Rank 0 makes the 128-byte id (pre3_comm_unique_id) and the host program hands it to the other ranks by any means
 * (3pre_amd/comm.py: torch.distributed broadcast; INTEGRATION.md: MPI_Bcast / a file); every rank then calls pre3_comm_create (collective:
 * it returns when all `world` ranks have called it).  world == 1 is allowed (the collectives run, over one rank).
 * RCCL is bound at run time: librccl.so.1 as already loaded in the process (e.g. PyTorch's copy), else from the loader path, else
 * /opt/rocm/lib; the environment's PRE3_RCCL_LIB overrides.  Without it these calls return PRE3_E_COMM; nothing else in libpre3 needs it.
 * A collective whose peer has died never completes: the wait of pre3_ransac_sharded / pre3_match_shard_match polls ncclCommGetAsyncError,
 * aborts the communicator when it reports one and returns PRE3_E_COMM.  A peer that merely stalls -- or never entered the collective -- is
 * caught by a wall-clock deadline on every host wait that has a collective in front of it (pre3_comm_set_timeout; default 10 s): on expiry
 * the communicator is aborted (ncclCommAbort: the collective the stream is stuck in returns), marked broken, and the call returns
 * PRE3_E_COMM; the context (or shard) stays usable once a fresh communicator is attached.  No wait of the library ends in an unbounded
 * synchronisation behind a collective: with a communicator attached EVERY drain of the context's stream -- pre3_sync, pre3_set_state, the
 * staging blocks of pre3_set_scan / pre3_set_descriptors / map management, pre3_set_comm, pre3_destroy -- polls the stream against the same
 * deadline (round 6).  The abort runs on a thread that pre3_set_comm, pre3_comm_destroy, pre3_destroy and pre3_match_shard_destroy join (bounded:
 * 10 s or the deadline, whichever is longer) before the handle or any buffer the collective touches goes away; while the stream has not
 * drained after an abort, calls that need it idle keep returning PRE3_E_COMM.  A rank whose own part of a round fails BEFORE the collective (a bad table, a failed launch) still
 * enters it, with an empty slice and a "missing" word that travels with the data: every rank then returns PRE3_E_COMM for that round. */
#define PRE3_COMM_ID_BYTES 128
typedef struct pre3_comm pre3_comm;
PRE3_API int pre3_comm_unique_id(void *id_out /* PRE3_COMM_ID_BYTES */);
PRE3_API int pre3_comm_create(pre3_comm **out, int device, const void *id, int rank, int world);
PRE3_API int pre3_comm_destroy(pre3_comm *comm);
PRE3_API int pre3_comm_info(pre3_comm *comm, int *rank, int *world, int *rccl_version, char *lib_path, int lib_path_len);
PRE3_API int pre3_comm_set_timeout(pre3_comm *comm, int milliseconds);      /* deadline of the host waits behind this communicator's collectives (default 10000) */
/* attach: the context / the shard borrows `comm` (must be on the same device; NULL detaches).  pre3_comm_init = create + attach, owned by the
 * context and destroyed with it. */
PRE3_API int pre3_set_comm(pre3_ctx *ctx, pre3_comm *comm);
PRE3_API int pre3_comm_init(pre3_ctx *ctx, const void *id, int rank, int world);
PRE3_API int pre3_match_shard_set_comm(pre3_match_shard *s, pre3_comm *comm);
/* pre3_ransac with the hypotheses dealt to the communicator's ranks (contiguous slices, sizes differing by at most one): same arguments, same
 * outputs on every rank, bit-identical to pre3_ransac for any number of ranks.  Every rank must hold the same state, measurements and draws. */
PRE3_API int pre3_ransac_sharded(pre3_ctx *ctx, int n_draw, int k, const int32_t *hyp, double threshold, int early_exit,
                                 int32_t *support, int32_t *li_mask, int32_t stats[4]);
/* one whole sharded match (run + all-gather + merge); outputs as pre3_match_shard_merge.  Without a communicator: the slice alone (G = 1). */
PRE3_API int pre3_match_shard_match(pre3_match_shard *s, double thresh, double *pairs_out, double *score_out, int *M_out);

/* ---- a11: kNearestNeighbors.m:29-39 ------------------------------------------------------------- */
/* data: N x D, query: M x D, MATLAB column-major.  ids_out (M x k, column-major, 1-based doubles),
 * dist_out (M x k, Euclidean).  Ties: lowest index first (MATLAB's stable sort). */
/* the stateless matcher / kNN calls keep their device scratch in a small pool between calls, pre3_predict_dense its context; this frees the idle part */
PRE3_API int pre3_release_scratch(void);
PRE3_API int pre3_knn_f64(int device, int D, int N, const double *data, int M, const double *query, int k,
                          double *ids_out, double *dist_out);

/* ---- measurement hooks (bench.py) ---------------------------------------------------------------- */
/* HIP-event timing on the ctx stream: the timed region of bench.py and the per-launch duration of
 * the covariance down-date kernel (K9) are measured with these, not with torch events.  An event's record is a barrier packet with a
 * completion signal in the stream: the launch behind it starts ~6 us late, so a bracket costs ~12 us of stream time -- time one launch in N. */
PRE3_API int pre3_timer_start(pre3_ctx *ctx);
PRE3_API int pre3_timer_stop(pre3_ctx *ctx, double *ms_out);             /* synchronises */
PRE3_API int pre3_kernel_timing(pre3_ctx *ctx, int enable);             /* 1: bracket every K9 launch of >= 128 rows (the matrix-bound ones) with events; N > 1: one such launch in N; 0: off */
PRE3_API int pre3_kernel_timing_read(pre3_ctx *ctx, int *launches_out, double *total_ms_out, double *flops_out,
                                     double *bytes_out);                /* synchronises, then resets */
/* Of the launches pre3_kernel_timing_read reports: how many were launches of the persistent factorisation that carry the down-date inside
 * (PRE3_OPT_K9_OVERLAP: the bracket then spans update.m:32-38 -- factorisation, solve, x-update and P - W'W -- of an update of the predicted
 * state), and the factorisation + solve flops (r^3/3 + n r^2) those launches executed besides the SYRK count.  Call it BEFORE
 * pre3_kernel_timing_read (both reset their sums). */
PRE3_API int pre3_kernel_timing_info(pre3_ctx *ctx, int *fused_launches_out, double *fact_flops_out);
/* run only the K9 down-date P <- P - W'W with a synthetic W of r rows `reps` times (roofline probe) */
PRE3_API int pre3_bench_downdate(pre3_ctx *ctx, int r, int reps, double *ms_per_launch_out);
/* Matcher probe (bench.py's `matcher` object, tests/test_gpu_match_rank.py): descriptors uploaded and packed ONCE, then `reps` back-to-back
 * launches of the distance + best/second-best stage bracketed by HIP events -- the kernel time of siftmatch.c:91-129's loop without the
 * per-call upload, packing and result copy of pre3_siftmatch_*.  cls: 0 double, 1 float, 2 uint8 (pre3_match_bench_create: uint8).
 * info[3] = { route taken (0 exact kernels, 1 int8 matrix cores, 2 bf16 rank + exact re-evaluation), queries the ranked route had to scan
 * in full, candidates it listed over all queries }; fetch: per query best / second-best squared distance and 0-based argument,
 * as siftmatch.c:110-116 leaves them.  Handles are independent of any pre3_ctx; NULL on failure (pre3_last_error). */
PRE3_API void *pre3_match_bench_create(int device, int ND, int K1, const uint8_t *L1, int K2, const uint8_t *L2);
PRE3_API void *pre3_match_bench_create_cls(int device, int cls, int ND, int K1, const void *L1, int K2, const void *L2);
PRE3_API int pre3_match_bench_info(void *h, int32_t info[3]);
PRE3_API int pre3_match_bench_run(void *h, int reps, double *ms_per_launch_out);
PRE3_API int pre3_match_bench_fetch(void *h, double *best, double *second, int32_t *arg);
PRE3_API void pre3_match_bench_destroy(void *h);

#ifdef __cplusplus
}
#endif
#endif /* PRE3_H */
