// pre3_knobs.h -- every PRE3_* environment switch of libpre3, declared once: name, default, when it is read, what it does.  Each is an A/B switch
// for a measured design decision (or a debug / test aid); the defaults are what bench.py measures.  The launchers call the accessors generated
// below (pre3::knob::hp_mb() ...) and never getenv.  Plain C++17, no HIP: tests/test_knobs.py builds this header with the host compiler alone,
// prints the table and ties the names the tests set to it.  (Compile-time switches -- PRE3_CRIT_ASYNC, CHA_* ... -- are not here: DESIGN.md section 8a.)
//
// X(accessor, environment name, default, kind, meaning).  Integer kinds -- unset: the default; set: atoi of the text (an empty string is 0):
//   once     read at the accessor's first use, kept for the life of the process
//   call     read at every call (the matcher / IC-search tests flip these inside one process)
//   create   read by pre3_create for each context it makes; != 0 is "on"
// and three of their own:
//   present  bool, on whenever the variable exists, whatever its text; read once
//   is1      bool, on only when atoi of the text is 1; read at every call
//   text     const char *, null when unset; read at every call
#pragma once
#include <stdlib.h>

#define PRE3_KNOBS(X) \
    /* ---- context creation (pre3_api.hip) */ \
    X(tail,              "PRE3_TAIL",              0,  create,  "initial PRE3_OPT_STEP_TAIL: rescue stage + HI update inside the persistent launch; off by default (measured: DESIGN.md section 5d)") \
    X(k9_b3,             "PRE3_K9_B3",             1,  create,  "fp32 contexts, initial PRE3_OPT_K9_BF16X3: three-way bf16 split on the bf16 matrix cores (k_split_w + k_downdate_b3); 0: f32-MFMA down-date, f32 pending updates and trailing tiles") \
    X(pend_hi,           "PRE3_PEND_HI",           0,  create,  "fp32 contexts, initial PRE3_OPT_PEND_HI: the HI update's down-date stays pending across the step boundary (DESIGN.md section 5e); needs 2 .. CP_MAX_NRB + 1 panels of row capacity") \
    /* ---- entry, waits, debug (pre3_api.hip, pre3_step.hip, pre3_comm.hip) */ \
    X(fuse_jn,           "PRE3_FUSE_JN",           1,  once,    "the rows/cols 3..6 <- Jn pass of a HI update completed at the start of a step rides in that step's prediction launch (0: k_jnorm_P as its own launch; same bits)") \
    X(scan_trace,        "PRE3_SCAN_TRACE",        0,  once,    "pre3_set_scan: host-side phase clock on stderr (event wait, copy + bounds check, positions, enqueue)") \
    X(step_trace,        "PRE3_STEP_TRACE",        0,  present, "host-side stage clock (debug): where the host spends a step, on stderr every 100 steps") \
    X(test_hooks,        "PRE3_TEST_HOOKS",        0,  is1,     "arms pre3_test_stall / pre3_match_shard_test_stall (tests of the communicator's deadline) pre3_test_downdate (K9 alone on the caller's W) and pre3_test_factor_solve (factorisation and solve alone on the caller's S, B, nu); not a performance switch") \
    X(rccl_lib,          "PRE3_RCCL_LIB",          nullptr, text, "path of the RCCL library pre3_comm_* binds (default: librccl.so.1 as already loaded, else from the loader path, else /opt/rocm/lib)") \
    /* ---- the step's stage order (pre3_step.hip) */ \
    X(inline_g,          "PRE3_INLINE_G",          1,  once,    "RANSAC round: no H*P*H' launch (6.6 us in front of the scoring); the scorer and the LI gather compute their entries with k_ell_G's sum (0: k_ell_G / k_ell_G_hyp as launches; same bits)") \
    X(fuse_rows,         "PRE3_FUSE_ROWS",         1,  once,    "updates of a subset: the ELL rows are built inside the H*P launch (0: k_build_rows + k_ell_HP; same bits)") \
    X(chol_spec0,        "PRE3_CHOL_SPEC0",        1,  once,    "LI update inside pre3_step: the factorisation (fp32: the whole persistent launch; else panel 0) is launched before the host has polled the row count (0: after)") \
    X(pend_max_rows,     "PRE3_PEND_MAX_ROWS",     128, once,   "pending HI rows above which the down-date goes out at once; 128 = 2 NB = never (two pending panels cost the next H*P launch ~19 us more, one ~5; 64 measured 5922 against 5954 steps/s)") \
    X(ride_rescue,       "PRE3_RIDE_RESCUE",       1,  once,    "the rescue's projection rides in the LI update's K9 launch (0: projection + gate as one launch of their own, A/B)") \
    X(ride_proj,         "PRE3_RIDE_PROJ",         1,  once,    "the projection of every landmark rides in the prediction's launch (0: its own launch, A/B)") \
    X(ride_innov,        "PRE3_RIDE_INNOV",        1,  once,    "S_i (which also clears last frame's inlier flags) rides in the H*P launch of the RANSAC stage (0: its own launch)") \
    /* ---- prediction, projection, gate, selection (pre3_geom.hip) */ \
    X(gate_ride,         "PRE3_GATE_RIDE",         1,  once,    "the rescue's chi2 gate rides in the Jnorm pass's launch (0: a launch of its own behind it, rounds 3-4)") \
    X(select_gather,     "PRE3_SELECT_GATHER",     1,  once,    "pre3_step: the selection stage rides in the LI gather's launch (k_select_gather); 0: k_ransac_select + k_gather_li (same bits)") \
    X(select_gather_lds, "PRE3_SELECT_GATHER_LDS", 1,  once,    "k_select_gather in its LDS-staged form where the rows of H*P fit in 55 KB (0: the form gathering from global memory; same bits)") \
    /* ---- H*P, the per-panel factorisation, the down-date, k_hi_fused (pre3_update.hip) */ \
    X(k9_wt,             "PRE3_K9_WT",             1,  once,    "k_downdate_b3 and the one-tile K9 store P write-through (neutral at N = 2000: 1851 vs 1855 us; part of the HI update's down-date at N = 500)") \
    X(hp_mb,             "PRE3_HP_MB",             1,  once,    "H*P build: several measurements per workgroup (k_ell_HP_build_mb; shares the pose rows' loads, no faster: a ~7.7 us latency chain); 0: one per workgroup (k_ell_HP_build; same bits)") \
    X(pend_mb,           "PRE3_PEND_MB",           4,  once,    "measurements per workgroup of the pending H*P form: 4 (17.1 -> 16.5 us with their landmark rows gathered two at a time); 8 halves the loads of W~ but leaves 156 workgroups for 256 CUs (18.7 us), 2 doubles them (21.5 us)") \
    X(chol_pro_b3,       "PRE3_CHOL_PRO_B3",       1,  once,    "with the bf16-split down-date: pending updates / trailing tiles of the per-panel factorisation from bf16 planes (0: f32 MFMA; the planes of W then come from riders)") \
    X(chol_early,        "PRE3_CHOL_EARLY",        1,  once,    "per-panel factorisation: the last panel of an update whose row count is no multiple of 64 skips the chain steps behind its last real sub-panel (0: all of them; same bits)") \
    X(chol_trail_split,  "PRE3_CHOL_TRAIL_SPLIT",  4,  once,    "trailing updates with more than this x 2 x #CUs tiles go out as a launch of their own (no LDS, 8 workgroups per CU); 0: never") \
    X(chol_trail_p,      "PRE3_CHOL_TRAIL_P",      4,  once,    "panels per trailing sweep, clamped to 1 .. 4 (1: the one-panel sweep; same bits)") \
    X(chol_trail_t128,   "PRE3_CHOL_TRAIL_T128",   2,  once,    "the sweep's W part in 128 x 128 super-tiles with the operands staged through LDS (k_chol_trail_b3l); 0: 64 x 64 tiles (k_chol_trail_b3; same bits)") \
    X(k9_wgs,            "PRE3_K9_WGS",            3,  once,    "f32/f64 MFMA down-date, persistent form: workgroups per CU") \
    X(k9_form,           "PRE3_K9_FORM",           0,  once,    "f32/f64 MFMA down-date: force the one-tile (1) or the persistent (2) form (experiments)") \
    X(hi_fused,          "PRE3_HI_FUSED",          1,  once,    "pre3_step: collection + HI update as k_hi_fused + a device-gated down-date; 0: k_collect_hi, host poll, four launches (same bits)") \
    X(hi_fused_two,      "PRE3_HI_FUSED_TWO",      1,  once,    "k_hi_fused takes up to 64 landmarks (two panels) when the row capacity holds them (0: one panel, A/B)") \
    X(hf_deal,           "PRE3_HF_DEAL",           1,  once,    "k_hi_fused's S dealt over the workgroups in the two-panel case (0: every workgroup builds all of S, round 5)") \
    X(hf_deal_min,       "PRE3_HF_DEAL_MIN",       18, once,    "landmarks from which on S is dealt (measured, k_hi_fused at 4 .. 32 landmarks: dealt 14.4 14.7 15.7 16.3 17.0 17.5 19.1 us, every workgroup for itself 12.3 13.4 14.7 16.4 17.4 18.6 22.8)") \
    /* ---- the persistent factorisation (pre3_cholp.hip) */ \
    X(chol_form,         "PRE3_CHOL_FORM",         1,  once,    "fp32 factorisation + solve: 1 = one persistent launch (k_cholp) where its guarantees hold (at most 2 live fp32 contexts per device), 0 = per-panel launches always, 2 = persistent even with more contexts (their launches must then not overlap in time)") \
    X(k9_overlap,        "PRE3_K9_OVERLAP",        1,  once,    "the down-date and the x-update run inside k_cholp on as many tile groups as CUs are left; 0: k_downdate_b3 behind it (same bits)") \
    X(dd_max,            "PRE3_DD_MAX",            -1, once,    "tests: at most this many tile groups inside the persistent launch -- the rest goes to k_downdate_b3 (negative: as many as fit)") \
    X(cholp_xu,          "PRE3_CHOLP_XU",          1,  once,    "the strips of a launch that carries consumers also compute x_k_k (0: the x-update riders of the K9 launch, which then still goes out; no in-launch tail)") \
    X(dd_mode,           "PRE3_DD_MODE",           17, once,    "the consumers: bit 0: sc1 LDS-DMA of the planes; bit 1: an acquire per panel (experiment); bit 2: P warm-up; bit 4: write-through stores of P") \
    X(cholp_poll,        "PRE3_CHOLP_POLL",        0,  once,    "crit's wave 11: shader clocks per chain step spent polling (0: one poll per step, rounds 3-4)") \
    X(cholp_poll_from,   "PRE3_CHOLP_POLL_FROM",   3,  once,    "the chain step from which on crit's wave 11 spends PRE3_CHOLP_POLL") \
    X(row_late,          "PRE3_ROW_LATE",          0,  once,    "a row's L(i, J) flag held back to its last panel's tiles; measured (round 6): 5625 vs 5644 steps/s -- crit does not wait for the rows at present") \
    X(crit_early,        "PRE3_CRIT_EARLY",        1,  once,    "crit's last chain stops behind the last real sub-panel") \
    X(strip_rl,          "PRE3_STRIP_RL",          1,  once,    "right-looking flag-driven strips") \
    X(cholp_proj,        "PRE3_CHOLP_PROJ",        1,  once,    "without the tail: the strips end with the rescue stage's projection when the step wants the gate to ride with the Jnorm pass (GateRide)") \
    /* ---- matcher, IC search, map management (pre3_match.hip, pre3_map.hip) */ \
    X(match_float_form,  "PRE3_MATCH_FLOAT_FORM",  1,  call,    "float / double matcher: 0: exact VALU kernels only, 1: auto (matrix-core paths chosen by the data), 2: never the int8 route (A/B, tests)") \
    X(ic_rank,           "PRE3_IC_RANK",           1,  call,    "pre3_ic_search: siftmatch on the matrix cores (bf16 rank + exact re-evaluation); 0: the exact VALU kernel (A/B, tests; same bits)") \
    X(ic_fused,          "PRE3_IC_FUSED",          1,  call,    "pre3_ic_search: the fused route (k_ic_match_small + k_ic_gate_fused); 0: the ranked / exact routes (A/B, tests)") \
    X(ic_ride,           "PRE3_IC_RIDE",           1,  once,    "the fused route's matcher rides in the projection + S_i launch in front of the gate (0: a launch of its own, which can skip the tiles without a predicted landmark)") \
    X(map_one_pass,      "PRE3_MAP_ONE_PASS",      1,  once,    "map management: the congruence in one pass into the second buffer (k_map_one); 0: k_map_rows + k_map_cols (+ k_map_add_noise); same bits")

namespace pre3 {
namespace knob {

inline int env_int(const char *name, int def) { const char *e = getenv(name); return e ? atoi(e) : def; }

#define PRE3_KNOB_once(acc, env, def)    inline int acc() { static const int v = env_int(env, def); return v; }
#define PRE3_KNOB_call(acc, env, def)    inline int acc() { return env_int(env, def); }
#define PRE3_KNOB_create(acc, env, def)  PRE3_KNOB_call(acc, env, def)
#define PRE3_KNOB_present(acc, env, def) inline bool acc() { static const bool v = getenv(env) != nullptr; return v; }
#define PRE3_KNOB_is1(acc, env, def)     inline bool acc() { return env_int(env, def) == 1; }
#define PRE3_KNOB_text(acc, env, def)    inline const char *acc() { return getenv(env); }
#define PRE3_KNOB_ACCESSOR(acc, env, def, kind, meaning) PRE3_KNOB_##kind(acc, env, def)
PRE3_KNOBS(PRE3_KNOB_ACCESSOR)
#undef PRE3_KNOB_ACCESSOR

}  // namespace knob
}  // namespace pre3
