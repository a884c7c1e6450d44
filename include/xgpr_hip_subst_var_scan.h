/* xgpr_hip_subst_var_scan.h -- C ABI of libxgpr_hip.so, ninth part: the exact quadratic form  z'^T Vm z'  -- the predictive
 * variance up to its constants -- of every single-token substitution of the sequence and graph kernels (Conv1d*, Graph*): one
 * value per position and token.
 *
 * The conventions, the error codes and xgpr_last_error() are those of xgpr_hip.h, which this header includes: device
 * pointers unless a name ends in `_host`, nothing retained or allocated, every call asynchronous and stream-ordered,
 * 0 on success and a negative code otherwise.
 *
 * Why a ninth header: as for the second to the eighth -- the sets of names declared in the earlier headers are pinned,
 * name by name, to tables inside existing test files.  The entry points below are bound through xgpr_amd/_lib.py
 * SUBST_VAR_SCAN_SIGNATURES and held to the same guarantees by tests of their own (tests/test_subst_var_scan_host.py,
 * tests/test_gpu_subst_var_scan_memory_contract.py).
 */
#ifndef XGPR_HIP_SUBST_VAR_SCAN_H
#define XGPR_HIP_SUBST_VAR_SCAN_H

#include "xgpr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- The notation is that of xgpr_hip_subst_scan.h: sequence i has length s, nk = s - conv_width + 1 windows and tokens
 * t[0 .. s); J(l) are the windows j with max(0, l - conv_width + 1) <= j <= min(l, nk - 1); p = W win are a window's
 * projections and r = sqrt(1 / num_freqs) / {1, sqrt(nk), nk}[scaling_type].  The variance reads the first nvar columns z of
 * the feature row of xgpr_conv_token_rows_f32: column 2f is r sum_j cos p_f, column 2f + 1 is r sum_j sin p_f, and column 0
 * is the constant 1 under fit_intercept.  With
 *
 *     phi(win)[2f] = cos p_f,   phi(win)[2f + 1] = sin p_f       for columns < nvar      (column 0 := 0 under fit_intercept)
 *     delta[i, l, v] = sum_{j in J(l)} phi(win_j with the token at offset l - j replaced by v)  -  sum_{j in J(l)} phi(win_j)
 *
 * the mutant's columns are z' = z_i + r delta[i, l, v] -- exactly, not to first order -- and
 *
 *     out[i, l, v] = q[i]  +  2 r (delta . u[i])  +  r^2 (delta^T vm delta)            for 0 <= l < s, 0 <= v < vocab
 *
 * which is z'^T vm z' where the caller passes u[i] = vm z_i and q[i] = z_i . u[i] and vm is symmetric; nothing is symmetrised:
 * for any vm, u and q the result is the expression above, with delta^T vm delta = sum_a sum_b delta_a vm[a, b] delta_b.
 * tokens, table, radem, chi, seqlen_host / seqlen_dev: as for xgpr_conv_token_subst_scan_f32.  vm[nvar, nvar] float64 with
 * row stride vm_stride >= nvar (elements), u[n, nvar] and q[n] float64.  out[n, L, vocab] float64 is OVERWRITTEN as a
 * whole: positions l >= s hold exactly 0.0, and at out[i, l, t[l]] delta is exactly +0.0 (the own token goes through the same
 * code path as every other v and is subtracted), so that entry is q[i] bit for bit.
 * nvar: even, 2 <= nvar <= 2 num_freqs; the kernels serve nvar <= 2048 (the first 1024-frequency tile).
 * slab_rows: how many mutant rows (slot, token) -- rows of the [n L vocab, nvar] matrix of deltas, in the order of out -- the
 * workspace holds at a time: 0 selects the library's default (128 MiB of rows, at least 16 and at most 65536 rows); any
 * other value must be a multiple of 16 and at least 16.  The rows of out are processed slab by slab, two launches each.
 * Arithmetic: per variant window the float32 cos / sin arguments of xgpr_conv_token_rows_f32, bit for bit; the cos / sin
 * values are widened and summed in float64 over J(l) in ascending j, the own token's sums subtracted once; delta vm on the
 * float64 matrix cores (v_mfma_f64_16x16x4_f64), columns of vm in ascending order; its products with delta summed per lane
 * in ascending column order and then over 16 lanes in a fixed tree; delta . u per lane in ascending column order, then a
 * fixed tree; out = (q + (2 r) (delta . u)) + (r r) (delta^T vm delta).  No atomics: results are bit-identical from run to
 * run, depend on the sequence alone -- not on n, on its position in the batch or on slab_rows -- and two identical table rows
 * give bit-identical columns of out.
 * workspace: xgpr_conv_token_subst_var_scan_workspace_bytes(radem_shape2, nvar, slab_rows) bytes, exactly: the packed sign
 * masks (xgpr_rbf_workspace_bytes(radem_shape2)) and slab_rows rows of nvar float64; 8-byte aligned.  Its contents never
 * enter the result.  The function returns 0 for an nvar or a slab_rows the call would refuse.
 * xgpr_conv_token_subst_var_scan_ok(width, vocab, C, num_freqs, nvar) is 1 where the kernels serve the shape:
 * xgpr_conv_token_subst_scan_ok(width, vocab, C, num_freqs), nvar even, 2 <= nvar <= 2 num_freqs and nvar <= 2048.
 * Checks, before anything is launched, in this order: n < 0, L < 1, C < 1 or a scaling_type outside 0 .. 2:
 * XGPR_ERR_ARRAY_DIMS; conv_width < 1 or > L: XGPR_ERR_CONV_WIDTH; num_freqs < 1 or > radem_shape2, or radem_shape2 not
 * a multiple of the padded width: XGPR_ERR_RFFS_FREQS; nvar odd, < 2 or > 2 num_freqs: XGPR_ERR_ARRAY_DIMS; vm_stride < nvar:
 * XGPR_ERR_ARRAY_SIZES; slab_rows negative, or neither 0 nor a multiple of 16: XGPR_ERR_ARRAY_DIMS; with n > 0, seqlen_host
 * NULL or a length < conv_width or > L: XGPR_ERR_SEQLEN_RANGE; vocab outside 1 .. 256: XGPR_ERR_ARRAY_DIMS; a shape the _ok
 * predicate refuses: XGPR_ERR_UNSUPPORTED (the caller materialises the mutants); n == 0: returns 0, nothing launched; a
 * workspace that is NULL, misaligned or smaller than _workspace_bytes, or a NULL array: XGPR_ERR_WORKSPACE; n * L >= 2^24:
 * XGPR_ERR_UNSUPPORTED, split the batch. */
int xgpr_conv_token_subst_var_scan_ok(long width, long vocab, long C, long num_freqs, long nvar);
size_t xgpr_conv_token_subst_var_scan_workspace_bytes(long radem_shape2, long nvar, long slab_rows);
int xgpr_conv_token_subst_var_scan_f32(const uint8_t *tokens, const float *table, const double *vm, long vm_stride,
                                       const double *u, const double *q, double *out, const int8_t *radem, const float *chi,
                                       const int32_t *seqlen_host, const int32_t *seqlen_dev, long n, long L, long vocab,
                                       long C, long num_freqs, long radem_shape2, long nvar, int conv_width, int scaling_type,
                                       int fit_intercept, long slab_rows, void *workspace, size_t workspace_bytes,
                                       void *stream);

#ifdef __cplusplus
}
#endif
#endif /* XGPR_HIP_SUBST_VAR_SCAN_H */
