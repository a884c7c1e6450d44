/* xgpr_hip/edit_proj.h -- C ABI of libxgpr_hip.so, thirteenth part: the projection  z'^T pm  of the first nvar feature
 * columns of EVERY single-token substitution, deletion and insertion of the sequence and graph kernels (Conv1d*, Graph*)
 * on a caller's matrix pm [nvar, K] -- the linear map next to the quadratic forms of xgpr_hip_subst_var_scan.h and
 * xgpr_hip_indel_var_scan.h.  With pm a square-root factor of the posterior covariance of the weights the result is a factor
 * of the JOINT posterior covariance of the whole single-edit neighbourhood; with pm = factor E (E standard normal) it is
 * joint posterior draws of every edit; with pm = var z* it is every edit's covariance with chosen sequences.
 *
 * The conventions, the error codes and xgpr_last_error() are those of xgpr_hip.h, which this header includes: device
 * pointers unless a name ends in `_host`, nothing retained or allocated, every call asynchronous and stream-ordered,
 * 0 on success and a negative code otherwise.
 *
 * Why a thirteenth header, and why in a subdirectory: see the opening comment of xgpr_hip/pool_edits.h.  The entry points
 * below are bound through xgpr_amd/_lib.py EDIT_PROJ_ABI and held to the guarantees of the others by tests of their own
 * (tests/test_edit_proj_host.py, tests/test_gpu_edit_proj_memory_contract.py).
 */
#ifndef XGPR_HIP_EDIT_PROJ_H
#define XGPR_HIP_EDIT_PROJ_H

#include "../xgpr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- The notation is that of xgpr_hip_subst_var_scan.h and xgpr_hip_indel_var_scan.h: sequence i has length s and nk = s -
 * conv_width + 1 windows; r(k) = sqrt(1 / num_freqs) / {1, sqrt(k), k}[scaling_type]; delta is the float64 row by which an
 * edit moves the first nvar columns before the normaliser (column 0 := 0 under fit_intercept), formed by the SAME kernels
 * as for the variance scans, bit for bit.  A mutant's columns are  z' = b + r' delta  -- exactly, not to first order --
 * with b = z_i, r' = r(nk) for a substitution and b = rho z_i + (1 - rho) e0, r' = r(nk -+ 1), rho = r' / r(nk) for a
 * deletion / an insertion.  The operator writes
 *
 *     out[i, l, v, k]     = b[i, k]     + r(nk)     (delta[i, l, v] . pm[:, k])        0 <= l < s
 *     out_del[i, p, k]    = b_del[i, k] + r(nk - 1) (delta_del[i, p] . pm[:, k])       0 <= p < s
 *     out_ins[i, g, v, k] = b_ins[i, k] + r(nk + 1) (delta_ins[i, g, v] . pm[:, k])    0 <= g <= s
 *
 * which is z'^T pm where the caller passes b[i] = z_i^T pm (substitutions) and, per indel row set, b~[i] = (rho z_i +
 * (1 - rho) e0)^T pm with that row set's rho; nothing is rescaled by the library: for any pm and b the result is the
 * expression above.
 * tokens, table, radem, chi, seqlen_host / seqlen_dev: as for xgpr_conv_token_indel_var_scan_f32.  pm[nvar, K] float64 with
 * row stride pm_stride >= K (elements); b, b_del, b_ins [n, K] float64, dense.  out[n, L, vocab, K], out_del[n, L, K] and
 * out_ins[n, L + 1, vocab, K], float64 and dense, are each OVERWRITTEN as a whole: positions l, p >= s and gaps g > s hold
 * K times exactly 0.0, and the deletions p < s of a sequence with s == conv_width -- its mutant has no window -- hold K
 * quiet NaNs.  At a sequence's own token delta is exactly +0.0 and the row is b[i] bit for bit (a b of -0.0 reads +0.0).
 * Either indel group (b_del, out_del) or (b_ins, out_ins) may be NULL as a whole: that row set is not computed.
 * nvar: even, 2 <= nvar <= 2 num_freqs; the kernels serve nvar <= 2048 and 1 <= K <= 2048.
 * slab_rows: as for the variance scans (0: the library's default; otherwise a multiple of 16).
 * Arithmetic: delta as for the variance scans; delta . pm[:, k] on the float64 matrix cores, k ascending over the rows of
 * pm, one chain of matrix-core multiply-adds per output value; then one multiply by r' and one add of b, in that order.  No
 * atomics: results are bit-identical from run to run, and a row's bits depend on its own sequence, the table, the draws, pm,
 * b and the column alone -- not on n, on the position in the batch, on slab_rows, on whether the other row set was requested
 * or on K (column k of a call with K columns equals column k of a call with the first K' > k columns of pm); two identical
 * table rows give bit-identical rows.
 * workspace: xgpr_conv_token_edit_proj_workspace_bytes(radem_shape2, nvar, slab_rows) bytes, exactly what the variance
 * scans need: the packed sign masks (xgpr_rbf_workspace_bytes(radem_shape2)) and slab_rows rows of nvar float64; 8-byte
 * aligned.  Its contents never enter the result.  The function returns 0 for an nvar or a slab_rows the call would refuse.
 * xgpr_conv_token_edit_proj_ok(width, vocab, C, num_freqs, nvar, K) is 1 where the kernels serve the shape:
 * xgpr_conv_token_subst_var_scan_ok(width, vocab, C, num_freqs, nvar) and 1 <= K <= 2048.
 * Checks, before anything is launched, in this order: n < 0, L < 1, C < 1 or a scaling_type outside 0 .. 2:
 * XGPR_ERR_ARRAY_DIMS; conv_width < 1 or > L: XGPR_ERR_CONV_WIDTH; num_freqs < 1 or > radem_shape2, or radem_shape2 not
 * a multiple of the padded width: XGPR_ERR_RFFS_FREQS; nvar odd, < 2 or > 2 num_freqs: XGPR_ERR_ARRAY_DIMS; K < 1:
 * XGPR_ERR_ARRAY_DIMS; pm_stride < K: XGPR_ERR_ARRAY_SIZES; slab_rows negative, or neither 0 nor a multiple of 16:
 * XGPR_ERR_ARRAY_DIMS; with n > 0, seqlen_host NULL or a length < conv_width or > L: XGPR_ERR_SEQLEN_RANGE; vocab outside
 * 1 .. 256: XGPR_ERR_ARRAY_DIMS; a shape the _ok predicate refuses: XGPR_ERR_UNSUPPORTED (the caller materialises the
 * mutants); n == 0: returns 0, nothing launched; a workspace that is NULL, misaligned or smaller than _workspace_bytes, a
 * NULL array, an indel group given by halves or both groups NULL: XGPR_ERR_WORKSPACE; n * L >= 2^24 (indels: n * (L + 1)):
 * XGPR_ERR_UNSUPPORTED, split the batch.  A refused call writes nothing. */
int xgpr_conv_token_edit_proj_ok(long width, long vocab, long C, long num_freqs, long nvar, long K);
size_t xgpr_conv_token_edit_proj_workspace_bytes(long radem_shape2, long nvar, long slab_rows);
int xgpr_conv_token_subst_proj_f32(const uint8_t *tokens, const float *table, const double *pm, long pm_stride,
                                   const double *b, double *out, const int8_t *radem, const float *chi,
                                   const int32_t *seqlen_host, const int32_t *seqlen_dev, long n, long L, long vocab, long C,
                                   long num_freqs, long radem_shape2, long nvar, long K, int conv_width, int scaling_type,
                                   int fit_intercept, long slab_rows, void *workspace, size_t workspace_bytes,
                                   void *stream);
int xgpr_conv_token_indel_proj_f32(const uint8_t *tokens, const float *table, const double *pm, long pm_stride,
                                   const double *b_del, const double *b_ins, double *out_del, double *out_ins,
                                   const int8_t *radem, const float *chi, const int32_t *seqlen_host,
                                   const int32_t *seqlen_dev, long n, long L, long vocab, long C, long num_freqs,
                                   long radem_shape2, long nvar, long K, int conv_width, int scaling_type,
                                   int fit_intercept, long slab_rows, void *workspace, size_t workspace_bytes,
                                   void *stream);

#ifdef __cplusplus
}
#endif
#endif /* XGPR_HIP_EDIT_PROJ_H */
