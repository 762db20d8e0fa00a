/* pre3_test_hooks.h -- NOT part of the public interface (include/pre3.h): two hooks for tests/test_gpu_comm.py, one for
 * tests/test_gpu_k9_alone.py and one for tests/test_gpu_chol_alone.py, exported from libpre3.so but inert unless the environment has PRE3_TEST_HOOKS=1 (they return PRE3_E_STATE otherwise).
 *
 * pre3_test_stall(ctx, 0) / pre3_match_shard_test_stall(s, 0): park a one-thread kernel on the context's / the shard's stream that spins until it is
 * released (..., 1) -- it also lets go by itself after ~20 s -- so that a test can stand in for a peer that stalls inside a collective.
 * pre3_match_shard_test_stall(s, 2): the next match's distance kernels "fail" (a rank-local failure in front of the all-gather).
 *
 * Reserved mailbox words: word 15 of the context's pinned mailbox (pre3_ctx::mail_host; words 0..9 carry the step's counts and sequence numbers, 16..19 the
 * staging blocks') and word 3 of the shard's result-block mailbox (words 0..2: the match's sequence number, count and missing-slice word) belong to these
 * hooks and to nothing else.
 *
 * pre3_test_downdate(ctx, r, W, launches): the down-date P <- P - W'W (K9) on the caller's W and on nothing else, `launches` times in a row.  W is r x n,
 * row-major, host memory; it is converted to the context's dtype and written to rows 0 .. r-1 of the update workspace (row stride ldw; columns n .. ldw-1
 * and rows r .. round_up(r, 64)-1 zeroed), then launch_downdate runs without the x-update rider -- the first launch splits the bf16 planes, the later ones
 * find them, as in pre3_bench_downdate -- and the stream is drained.  P is read back with pre3_get_state.  PRE3_E_ARG (nothing touched) for r < 1,
 * round_up(r, 64) above the context's row capacity, launches < 1, a null pointer or a non-finite entry of W.
 *
 * pre3_test_factor_solve(ctx, r, S, B, nu, mode, predicted_prior, L_out, W_out): the factorisation S = L L' and the solve L W = [B | nu] (update.m:32-33)
 * on the caller's S (r x r, symmetric), B (r x n) and nu (r), all row-major host doubles converted to the context's dtype.  S goes to the factorisation's
 * workspace at stride r_pad = round_up(r, 64), both triangles, with the identity on the padded diagonal; B to rows 0 .. r-1 of the update workspace, nu to its
 * column ld, zeros everywhere else.  Then launch_chol_solve runs as run_update calls it, without the x-update; predicted_prior != 0 lets a one-panel case
 * take the persistent form, as an update of the predicted state does.
 *   mode 0: nothing else runs -- the persistent launch goes out without down-date consumers (PRE3_OPT_K9_OVERLAP off for this call), P is not touched.
 *   mode 1: launch_downdate follows as in run_update, on the bf16 planes the factorisation wrote (consumers as the context has them); read P with
 *           pre3_get_state.
 * The stream is drained; PRE3_E_NUMERIC if a pivot was not positive.  L_out (nullable): r x r, the lower triangle of L, zeros above.  W_out (nullable):
 * r_pad x (n + 1), L^-1 B with L^-1 nu as the last column, the padded rows included.  PRE3_E_ARG (nothing touched) for r < 1, r_pad above the context's
 * row capacity, a mode other than 0 / 1, a null input pointer or a non-finite entry after conversion.
 *
 * pre3_test_live_blocks(out): the device blocks, device bytes, pinned blocks and pinned bytes of the whole process that are live right now, counted
 * where pre3_own.h's seam allocates and frees (the ScratchPool of the stateless entry points is not in it). */
#pragma once
#include "../../include/pre3.h"
#ifdef __cplusplus
extern "C" {
#endif
PRE3_API int pre3_test_stall(pre3_ctx *ctx, int release);
PRE3_API int pre3_match_shard_test_stall(pre3_match_shard *s, int release);
PRE3_API int pre3_test_downdate(pre3_ctx *ctx, int r, const double *W, int launches);
PRE3_API int pre3_test_factor_solve(pre3_ctx *ctx, int r, const double *S, const double *B, const double *nu, int mode, int predicted_prior, double *L_out, double *W_out);
PRE3_API int pre3_test_live_blocks(int64_t out[4]);
#ifdef __cplusplus
}
#endif
