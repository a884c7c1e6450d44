/* xgpr_hip_subst_scan.h -- C ABI of libxgpr_hip.so, seventh part: the exact effect of every single-token substitution on a
 * weighted sum of the sequence and graph kernels' random features (Conv1d*, Graph*): one value per position and token.
 *
 * The conventions, the error codes and xgpr_last_error() are those of xgpr_hip.h, which this header includes: device
 * pointers unless a name ends in `_host`, nothing retained or allocated, every call asynchronous and stream-ordered,
 * 0 on success and a negative code otherwise.
 *
 * Why a seventh header: as for the second to the sixth -- the sets of names declared in the earlier headers are pinned,
 * name by name, to tables inside existing test files.  The entry points below are bound through xgpr_amd/_lib.py
 * SUBST_SCAN_SIGNATURES and held to the same guarantees by tests of their own (tests/test_subst_scan_host.py,
 * tests/test_gpu_subst_scan_memory_contract.py).
 */
#ifndef XGPR_HIP_SUBST_SCAN_H
#define XGPR_HIP_SUBST_SCAN_H

#include "xgpr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- m(sequence with t[l] := v) - m(sequence)  for  m = sum_col w[col] z_col  over the feature row z of
 * xgpr_conv_token_rows_f32, for every position l and every token v (no counterpart in the reference).  The notation is
 * that of xgpr_hip_seq_input_grad.h: sequence i has length s, nk = s - conv_width + 1 k-mers and tokens t[0 .. s); window j
 * is table[t[j .. j + conv_width)] flattened; p = W win are a window's projections (W the SORF matrix times chi) and
 * r = sqrt(1 / num_freqs) / {1, sqrt(nk), nk}[scaling_type].  With the window score
 *
 *     c(win) = sum_f (w[2f] cos p_f + w[2f+1] sin p_f)            (w[0] dropped under fit_intercept: column 0 is the constant)
 *
 * and J(l) the windows j with max(0, l - conv_width + 1) <= j <= min(l, nk - 1) -- the only ones a substitution at l
 * changes; the normaliser depends on the length alone --
 *
 *     out[i, l, v] = r ( sum_{j in J(l)} c(win_j with the token at offset l - j replaced by v)  -  sum_{j in J(l)} c(win_j) )
 *
 * for 0 <= l < s and 0 <= v < vocab: exact, not first-order.  Graph kernels are conv_width == 1.
 * tokens[n, L] uint8 (values < vocab; tokens past a sequence's length are never read), table[vocab, C] float32 ALREADY
 * multiplied by sigma, w[2 num_freqs] float64: ONE vector shared by all sequences.  out[n, L, vocab] float64 is
 * OVERWRITTEN as a whole: positions l >= s hold exactly 0.0, and out[i, l, t[l]] is exactly +0.0 (the unmutated sum is
 * formed through the same code path as every other v and subtracted).  seqlen_host / seqlen_dev: the int32 lengths [n] on
 * the host (validated there) and on the device, as for xgpr_conv_token_rows_f32.
 * Arithmetic: per variant window the float32 cos / sin arguments of xgpr_conv_token_rows_f32, bit for bit (float32
 * butterflies); the products with the float64 weights and all sums are float64, in a fixed order (per 1024-frequency tile a
 * fixed tree, tiles and windows ascending, four partial sums added as ((s0 + s1) + s2) + s3).  No atomics: results are
 * bit-identical from run to run, a sequence's result depends on that sequence alone -- not on n or its position in the
 * batch -- and two identical table rows give bit-identical columns of out.
 * workspace: xgpr_rbf_workspace_bytes(radem_shape2) bytes (the packed sign masks); nothing else.
 * xgpr_conv_token_subst_scan_ok(width, vocab, C, num_freqs) is 1 where the kernel serves a window of
 * width = conv_width * C elements over that table: xgpr_conv_token_input_grad_ok(width, vocab, C) (padded width up to 1024,
 * a table of at most 4608 floats) and num_freqs >= 1.
 * Checks, before anything is launched, in this order: n < 0, L < 1, C < 1 or a scaling_type outside 0 .. 2:
 * XGPR_ERR_ARRAY_DIMS; conv_width < 1 or > L: XGPR_ERR_CONV_WIDTH; num_freqs < 1 or > radem_shape2, or radem_shape2 not
 * a multiple of the padded width: XGPR_ERR_RFFS_FREQS; with n > 0, seqlen_host NULL or a length < conv_width or > L:
 * XGPR_ERR_SEQLEN_RANGE; vocab outside 1 .. 256: XGPR_ERR_ARRAY_DIMS; a shape the _ok predicate refuses:
 * XGPR_ERR_UNSUPPORTED (the caller materialises the mutants and calls xgpr_conv_token_rows_f32); n == 0: returns 0,
 * nothing launched; a workspace smaller than xgpr_rbf_workspace_bytes(radem_shape2) or a NULL array:
 * XGPR_ERR_WORKSPACE; n * L >= 2^24 (one workgroup per position): XGPR_ERR_UNSUPPORTED, split the batch. */
int xgpr_conv_token_subst_scan_ok(long width, long vocab, long C, long num_freqs);
int xgpr_conv_token_subst_scan_f32(const uint8_t *tokens, const float *table, const double *w, double *out,
                                   const int8_t *radem, const float *chi, const int32_t *seqlen_host,
                                   const int32_t *seqlen_dev, long n, long L, long vocab, long C, long num_freqs,
                                   long radem_shape2, int conv_width, int scaling_type, int fit_intercept,
                                   void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* XGPR_HIP_SUBST_SCAN_H */
