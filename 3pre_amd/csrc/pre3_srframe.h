// pre3_srframe.h -- the resident SR4000 frame handle (pre3_sr.hip owns it; pre3_sift.hip fills its keypoint block on the device).
#pragma once
#include "pre3_internal.h"

namespace pre3 {
struct SiftWork;
void sift_work_free(SiftWork *w);                            // pre3_sift.hip
}

struct pre3_sr_frame {
    int device = 0, rows = 0, cols = 0;
    int loaded = 0, mode = 0, has_conf = 0;
    // the compensation: the setting the next load takes, and the form the resident frame was conditioned with
    int comp_form = 0, frame_form = 0;
    double comp_cutoff = 1.0;
    hipStream_t stream = nullptr;
    double *raw = nullptr;          // [5][npix]: z, x, y, amplitude, confidence -- as uploaded
    double *filt = nullptr;         // [4][npix]: x, y, z, image
    double *maxima = nullptr;       // imax, cmax, n_bad (pixels with conf < cutoff, counted under form 1 only)
    void *stage = nullptr;          // pinned (mem.stage): the five planes of a load, or the keypoints of a call
    void *kp = nullptr;             // device (mem.kp): the keypoint stage's input and output block
    int32_t *pinned_n = nullptr;    // n_kept
    // the last keypoint call's result, still in `kp` (sr_frame_keypoint_view): kp_valid 0 = none yet, or stale after a load
    int kp_valid = 0, kp_K = 0, kp_ldf = 0, kp_ND = 0, kp_gate = 0, kp_n = 0;
    int kp_K_in = 0;                        // the raw set of that call, once its transfer is queued: [kp_K_in][ldf] frames at offset 0 of kp,
    size_t kp_o_des_in = 0;                 // [kp_K_in][ND] descriptors here (sr_frame_keypoint_view: K_in, frm_in, des_in)
    bool kp_raw_ok = true;                  // its descriptors passed the ranked IC route's bounds on their way through `stage`
    size_t kp_o_frm = 0, kp_o_des = 0;      // offsets of frm_out / des_out inside kp
    size_t kp_o_xyz = 0, kp_o_rho = 0, kp_o_idx = 0;      // ... of xyz_out / rho_out (written by gate 0 only) and keep_idx
    hipEvent_t pair_ev = nullptr;   // carries the hand-offs to and from a consumer's stream (sr_frame_lend, sr_frame_reclaim)
    // the SIFT extractor's plan, scale space and lists (pre3_sift.hip), allocated on its first use
    pre3::SiftWork *sift = nullptr;
    // the text stage (pre3_dattext.hip), allocated on its first use: [text | chunk records | token offsets | status], and the plane block the parse
    // writes, which swaps with `raw` when a text is accepted
    void *text_dev = nullptr;
    double *spare = nullptr;
    // the owners (pre3_own.h): raw, filt, maxima, pinned_n and spare sit on `fixed`; the others grow on demand, each zeroed on the handle's stream when
    // it is new.  pair_dev / pair_pin: the pair stage's work block and its pinned image (pre3_vopair.hip), allocated on its first use
    // icp_dev: the device block of the ICP run pre3_predict_icp_pair_seeded queues on this handle (cur); the prediction reads it behind the call's return
    struct { pre3::BlockList fixed; pre3::PinBlock stage, pair_pin; pre3::DevBlock kp, pair_dev, text_dev, icp_dev; } mem;
};

namespace pre3 {
// the keypoint block's layout for a raw set of K frames of ldf entries and K descriptors of ND: [frm | des] in front, the gate's outputs behind
struct KpLayout { size_t b_frm, b_des, o_frm_out, o_des_out, o_xyz, o_rho, o_idx, o_n, total; };
KpLayout kp_layout(int K, int ldf, int ND);
// the keypoint block grown to `total` bytes (zeroed on the handle's stream when it is new).  The caller has waited for the stream.
int sr_frame_kp_reserve(pre3_sr_frame *f, size_t total);
int sr_grow_stage(pre3_sr_frame *f, size_t bytes);
int sr_condition_run(pre3_sr_frame *f, int mode, bool has_conf);                       // the maxima and conditioning launches over `raw`
int sr_frame_text_work(pre3_sr_frame *f, size_t work_bytes, size_t spare_bytes);        // pre3_dattext.hip's blocks
}  // namespace pre3
