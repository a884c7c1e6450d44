/* xgpr_hip_indel_scan.h -- C ABI of libxgpr_hip.so, eighth part: the exact effect of every single-token deletion and
 * insertion on a weighted sum of the sequence and graph kernels' random features (Conv1d*, Graph*), and the per-window
 * scores that sum they are built from.
 *
 * The conventions, the error codes and xgpr_last_error() are those of xgpr_hip.h, which this header includes: device
 * pointers unless a name ends in `_host`, nothing retained or allocated, every call asynchronous and stream-ordered,
 * 0 on success and a negative code otherwise.
 *
 * Why an eighth header: as for the second to the seventh -- the sets of names declared in the earlier headers are pinned,
 * name by name, to tables inside existing test files.  The entry points below are bound through xgpr_amd/_lib.py
 * INDEL_SCAN_SIGNATURES and held to the same guarantees by tests of their own (tests/test_indel_scan_host.py,
 * tests/test_gpu_indel_scan_memory_contract.py).
 */
#ifndef XGPR_HIP_INDEL_SCAN_H
#define XGPR_HIP_INDEL_SCAN_H

#include "xgpr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The notation is that of xgpr_hip_subst_scan.h: sequence i has length s, nk = s - conv_width + 1 windows
 * win_j = table[t[j .. j + conv_width)] flattened, p = W win are a window's projections, the window score is
 *
 *     c(win) = sum_f (w[2f] cos p_f + w[2f+1] sin p_f)            (w[0] dropped under fit_intercept: column 0 is the constant)
 *
 * r(k) = sqrt(1 / num_freqs) / {1, sqrt(k), k}[scaling_type], T = sum_{j < nk} c(win_j) and m = sum_col w[col] z_col over
 * the feature row z of xgpr_conv_token_rows_f32.  Graph kernels are conv_width == 1.
 *
 * ---- xgpr_conv_token_window_scores_f32: scores[n, L] float64, OVERWRITTEN as a whole: scores[i, j] = c(win_j) for j < nk
 * and exactly 0.0 beyond.  r(nk) sum_j scores[i, j] (+ w[0] under fit_intercept) is m(sequence i).
 *
 * ---- xgpr_conv_token_indel_scan_f32 reads those scores (written by the call above with the same operands) and writes
 *
 *     del[i, p]    = m(t without position p) - m(t)                     = r' (A_p - R_p) + (r' - r(nk)) T,       r'  = r(nk - 1)
 *     ins[i, g, v] = m(t with table row v inserted before g) - m(t)     = r'' (A_gv - R'_g) + (r'' - r(nk)) T,   r'' = r(nk + 1)
 *
 * for 0 <= p < s and 0 <= g <= s (g == s appends), 0 <= v < vocab -- exact, not first-order.  R_p is the sum of the scores
 * of the windows j in [max(0, p - conv_width + 1), min(p, nk - 1)] that cover p, A_p the sum of c over the mutant's windows
 * j' in [max(0, p - conv_width + 1), min(p - 1, nk - 2)] that span the junction; R'_g is the sum of the scores of the
 * windows j in [max(0, g - conv_width + 1), min(g - 1, nk - 1)] that straddle the gap, A_gv the sum of c over the mutant's
 * windows j'' in [max(0, g - conv_width + 1), min(g, nk)] that hold the new token.  Every other window is only shifted.
 * del[n, L] and ins[n, L + 1, vocab] float64 are each OVERWRITTEN as a whole: del[i, p] for p >= s and ins[i, g, :] for
 * g > s are exactly 0.0.  A sequence with s == conv_width has no window left after a deletion: del[i, p] for p < s is a
 * quiet NaN, and nothing else is affected.  The mutant of an insertion may be longer than L: it is never written.
 * Either of del / ins may be NULL: that half is skipped and the other half's bits are unchanged.
 * tokens[n, L] uint8 (values < vocab; tokens past a sequence's length are never read), table[vocab, C] float32 ALREADY
 * multiplied by sigma, w[2 num_freqs] float64: ONE vector shared by all sequences.  seqlen_host / seqlen_dev: the int32
 * lengths [n] on the host (validated there) and on the device, as for xgpr_conv_token_rows_f32.
 * Arithmetic: per window the float32 cos / sin arguments of xgpr_conv_token_rows_f32, bit for bit; the products with the
 * float64 weights and all sums are float64, in a fixed order (per 1024-frequency tile a fixed tree, tiles and windows
 * ascending, four partial sums added as ((s0 + s1) + s2) + s3; R in ascending j; T in an order that depends on nk alone; at
 * scaling_type 0 the T term is exactly zero and not formed).  No atomics: results are bit-identical from run to run, a
 * sequence's result depends on that sequence alone -- not on n or its position in the batch -- and two identical table
 * rows give bit-identical columns of ins.
 * workspace: xgpr_rbf_workspace_bytes(radem_shape2) bytes (the packed sign masks) for either call; nothing else.
 * xgpr_conv_token_indel_scan_ok(width, vocab, C, num_freqs) is 1 where the kernels serve a window of
 * width = conv_width * C elements over that table: exactly where xgpr_conv_token_subst_scan_ok is 1.
 * Checks of both calls, before anything is launched, in this order: n < 0, L < 1, C < 1 or a scaling_type outside 0 .. 2:
 * XGPR_ERR_ARRAY_DIMS; conv_width < 1 or > L: XGPR_ERR_CONV_WIDTH; num_freqs < 1 or > radem_shape2, or radem_shape2 not
 * a multiple of the padded width: XGPR_ERR_RFFS_FREQS; with n > 0, seqlen_host NULL or a length < conv_width or > L:
 * XGPR_ERR_SEQLEN_RANGE; vocab outside 1 .. 256: XGPR_ERR_ARRAY_DIMS; a shape the _ok predicate refuses:
 * XGPR_ERR_UNSUPPORTED (the caller materialises the mutants and calls xgpr_conv_token_rows_f32); n == 0: returns 0,
 * nothing launched; a workspace smaller than xgpr_rbf_workspace_bytes(radem_shape2), a NULL array, or del and ins both
 * NULL: XGPR_ERR_WORKSPACE; n * (L + 1) >= 2^24 (one workgroup per gap): XGPR_ERR_UNSUPPORTED, split the batch.
 * (The scores call has no scaling_type: its scores are not normalised.) */
int xgpr_conv_token_indel_scan_ok(long width, long vocab, long C, long num_freqs);
int xgpr_conv_token_window_scores_f32(const uint8_t *tokens, const float *table, const double *w, double *scores,
                                      const int8_t *radem, const float *chi, const int32_t *seqlen_host,
                                      const int32_t *seqlen_dev, long n, long L, long vocab, long C, long num_freqs,
                                      long radem_shape2, int conv_width, int fit_intercept, void *workspace,
                                      size_t workspace_bytes, void *stream);
int xgpr_conv_token_indel_scan_f32(const uint8_t *tokens, const float *table, const double *w, const double *scores,
                                   double *del, double *ins, const int8_t *radem, const float *chi,
                                   const int32_t *seqlen_host, const int32_t *seqlen_dev, long n, long L, long vocab, long C,
                                   long num_freqs, long radem_shape2, int conv_width, int scaling_type, int fit_intercept,
                                   void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* XGPR_HIP_INDEL_SCAN_H */
