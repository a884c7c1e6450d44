/* xgpr_hip_pair_scan.h -- C ABI of libxgpr_hip.so, eleventh part: the exact NON-ADDITIVE part (epistasis) of every pair of
 * single-token substitutions closer than conv_width, on a weighted sum of the sequence and graph kernels' random features
 * (Conv1d*, Graph*): one value per position, distance and pair of tokens.
 *
 * The conventions, the error codes and xgpr_last_error() are those of xgpr_hip.h, which this header includes: device
 * pointers unless a name ends in `_host`, nothing retained or allocated, every call asynchronous and stream-ordered,
 * 0 on success and a negative code otherwise.
 *
 * Why an eleventh header: as for the second to the tenth -- the sets of names declared in the earlier headers are pinned,
 * name by name, to tables inside existing test files.  The entry points below are bound through xgpr_amd/_lib.py
 * PAIR_SCAN_SIGNATURES and held to the same guarantees by tests of their own (tests/test_pair_scan_host.py,
 * tests/test_gpu_pair_scan_memory_contract.py).
 */
#ifndef XGPR_HIP_PAIR_SCAN_H
#define XGPR_HIP_PAIR_SCAN_H

#include "xgpr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- The notation is that of xgpr_hip_subst_scan.h: sequence i has length s, nk = s - conv_width + 1 k-mers and tokens
 * t[0 .. s); c(win) is a window's score, J(l) the windows that cover position l, r the row constant, m = sum_col w[col] z_col, and
 * sub = what xgpr_conv_token_subst_scan_f32 writes.  For positions l1 < l2 = l1 + d and tokens v1, v2
 *
 *     m(t[l1 := v1, l2 := v2]) - m(t) = sub[i, l1, v1] + sub[i, l2, v2] + eps[i, l1, d, v1, v2]
 *     eps[i, l1, d, v1, v2] = r sum_{j in J(l1) & J(l2)} [ c(win_j with both) - c(win_j with v1 at l1) - c(win_j with v2 at l2) + c(win_j) ]
 *     J(l1) & J(l2) = { j : max(0, l2 - conv_width + 1) <= j <= min(l1, nk - 1) }
 *
 * exactly (no counterpart in the reference).  No window covers two positions conv_width or more apart: eps is identically zero
 * there, and the band 1 <= d <= conv_width - 1 is the whole of the non-additive part.
 * out[n, L, conv_width - 1, vocab, vocab] float64 is OVERWRITTEN as a whole: out[i, l1, d - 1, v1, v2] = eps[i, l1, d, v1, v2].
 * tokens, table (ALREADY multiplied by sigma), w (ONE float64 vector [2 num_freqs] shared by all sequences), radem, chi,
 * seqlen_host / seqlen_dev and the workspace -- xgpr_rbf_workspace_bytes(radem_shape2) bytes (the packed sign masks), nothing
 * else -- are those of xgpr_conv_token_subst_scan_f32.
 * Guarantees: slots with l1 >= s or l1 + d >= s hold exactly 0.0; the planes v1 == t[l1] and v2 == t[l2] hold exactly +0.0,
 * by construction: with G[v1, v2] the sum of c over the shared windows with both tokens in place, formed through one code
 * path for every pair, an output is r ((G[v1, v2] - G[v1, o2]) - (G[o1, v2] - G[o1, o2])) for o1 = t[l1], o2 = t[l2] -- on an
 * own-token plane (x - y) - (x - y) or 0 - 0 on identical bits.  Two identical table rows a, b give out[..., a, :] bit-equal to
 * out[..., b, :] and out[..., :, a] bit-equal to out[..., :, b].  No atomics: results are bit-identical from run to run, and a
 * sequence's block depends on that sequence, the table and w alone -- not on n or its position in the batch.
 * Arithmetic: per variant window the float32 cos / sin arguments of xgpr_conv_token_rows_f32, bit for bit; the products with
 * the float64 weights and all sums are float64, in a fixed order: G per 1024-frequency tile a fixed tree, tiles and windows
 * ascending, four partial sums added as ((s0 + s1) + s2) + s3; then the double difference as written above, then times r.
 * xgpr_conv_token_pair_scan_ok(width, vocab, C, num_freqs) is xgpr_conv_token_subst_scan_ok(width, vocab, C, num_freqs).
 * Checks, before anything is launched, in the order and with the codes of xgpr_conv_token_subst_scan_f32: n < 0, L < 1, C < 1
 * or a scaling_type outside 0 .. 2: XGPR_ERR_ARRAY_DIMS; conv_width < 1 or > L: XGPR_ERR_CONV_WIDTH; num_freqs < 1 or >
 * radem_shape2, or radem_shape2 not a multiple of the padded width: XGPR_ERR_RFFS_FREQS; with n > 0, seqlen_host NULL or a
 * length < conv_width or > L: XGPR_ERR_SEQLEN_RANGE; vocab outside 1 .. 256: XGPR_ERR_ARRAY_DIMS; a shape the _ok predicate
 * refuses: XGPR_ERR_UNSUPPORTED (the caller materialises the double mutants and calls xgpr_conv_token_rows_f32); n == 0, or
 * conv_width == 1 (graph kernels: out has no elements and may be NULL): returns 0, nothing launched; a workspace smaller than
 * xgpr_rbf_workspace_bytes(radem_shape2) or a NULL array: XGPR_ERR_WORKSPACE; n * L * (conv_width - 1) * vocab >= 2^24 (one
 * workgroup per row of out): XGPR_ERR_UNSUPPORTED, split the batch. */
int xgpr_conv_token_pair_scan_ok(long width, long vocab, long C, long num_freqs);
int xgpr_conv_token_pair_scan_f32(const uint8_t *tokens, const float *table, const double *w, double *out,
                                  const int8_t *radem, const float *chi, const int32_t *seqlen_host,
                                  const int32_t *seqlen_dev, long n, long L, long vocab, long C, long num_freqs,
                                  long radem_shape2, int conv_width, int scaling_type, int fit_intercept,
                                  void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* XGPR_HIP_PAIR_SCAN_H */
