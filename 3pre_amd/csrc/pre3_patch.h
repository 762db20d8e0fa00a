// pre3_patch.h -- the patch branch of search_IC_matches.m:45-51 (predict_features_appearance.m + mex_files/CorePar_Ver1/matching.m) on the device:
// the resident image, the per-landmark patch bank and the host side of the launches in pre3_patch.hip.
#pragma once
#include "pre3_internal.h"

namespace pre3 {

constexpr int PATCH_INIT_HALF = 20, PATCH_INIT_W = 41, PATCH_BYTES = 41 * 41;   // add_feature_to_info_vector_my_version.m:29: patch_when_initialized
constexpr int PATCH_HALF = 6, PATCH_W = 13, PATCH_PIX = 169;                    // :30: the patch that is correlated
constexpr int PATCH_META = 16;                   // doubles per landmark: uv(2), r_wc(3), R_wc(9, column-major), has (0 / 1), pad
constexpr int PATCH_MAX_DIM = 1024;              // rows and columns of the resident image: k_patch_search keeps three words per window column in LDS
constexpr int PATCH_STAGE_BYTES = 16384;         // k_patch_search stages a window (bounding box + halo) of up to this many bytes in LDS, else reads L2

// everything the feature owns, allocated with the first pre3_set_image / pre3_set_patches; a context without one issues no launch of this file
struct PatchState {
    uint8_t *img = nullptr; int rows = 0, cols = 0; bool img_set = false;     // column-major bytes, padded to 16
    bool bank_set = false;
    uint8_t *pb = nullptr, *pb_alt = nullptr;        // [capN][PATCH_BYTES]
    double *meta = nullptr, *meta_alt = nullptr;     // [capN][PATCH_META]
    unsigned char *up = nullptr; size_t up_bytes = 0;   // device landing block of a staged upload (16-byte aligned)
    double *warp = nullptr; int32_t *wstatus = nullptr;  // [capN][169], [capN]
    void *blk = nullptr, *blk_host = nullptr; size_t blk_bytes = 0;   // the search's result block and its pinned image
    hipEvent_t ev[4] = { nullptr, nullptr, nullptr, nullptr }; bool ev_valid = false;   // pre3_kernel_timing: brackets of k_patch_warp / k_patch_search
    struct { BlockList fixed; DevBlock img; } mem;   // the owners: everything above but img sits on `fixed`; img is replaced when the camera's shape changes
};

int patch_set_image(pre3_ctx *c, int nRows, int nCols, const uint8_t *im);
int patch_get_image(pre3_ctx *c, int nRows, int nCols, uint8_t *im);
int patch_set_image_frame(pre3_ctx *c, pre3_sr_frame *f);
int patch_set_patches(pre3_ctx *c, int first, int count, const uint8_t *patch, const double *uv, const double *r_wc, const double *R_wc);
int patch_get_patches(pre3_ctx *c, int first, int count, uint8_t *patch, double *uv, double *r_wc, double *R_wc, int32_t *has);
int patch_cut(pre3_ctx *c, int first, int count, const int32_t *uv);
int patch_predict(pre3_ctx *c, double focal_over_d, double *patch_out, int32_t *status_out);
int patch_search(pre3_ctx *c, double focal_over_d, double corr_threshold, int strict_reference, int32_t *m_out, int32_t *meas_idx_out, double *z_out,
                 double *corr_out, int32_t *ncand_out, int32_t *status_out);
int patch_timing(pre3_ctx *c, double *warp_ms, double *search_ms);
// the bank follows the map: one launch behind the congruence, reading its d_src list (src[i] = old index of new landmark i, -1: new); queued only
// when a bank exists (pre3_map.hip: apply_map)
int patch_follow_map(pre3_ctx *c, int N_new, const int32_t *d_src);
void patch_drop_bank(pre3_ctx *c);        // pre3_set_map: a new map has no patches
void free_patch(pre3_ctx *c);

}  // namespace pre3
