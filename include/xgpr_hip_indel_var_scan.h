/* xgpr_hip_indel_var_scan.h -- C ABI of libxgpr_hip.so, tenth part: the exact quadratic form  z'^T Vm z'  -- the predictive
 * variance up to its constants -- of every single-token deletion and insertion of the sequence and graph kernels (Conv1d*,
 * Graph*): one value per position, and one per gap and token.
 *
 * The conventions, the error codes and xgpr_last_error() are those of xgpr_hip.h, which this header includes: device
 * pointers unless a name ends in `_host`, nothing retained or allocated, every call asynchronous and stream-ordered,
 * 0 on success and a negative code otherwise.
 *
 * Why a tenth header: as for the second to the ninth -- the sets of names declared in the earlier headers are pinned,
 * name by name, to tables inside existing test files.  The entry points below are bound through xgpr_amd/_lib.py
 * INDEL_VAR_SCAN_SIGNATURES and held to the same guarantees by tests of their own (tests/test_indel_var_scan_host.py,
 * tests/test_gpu_indel_var_scan_memory_contract.py).
 */
#ifndef XGPR_HIP_INDEL_VAR_SCAN_H
#define XGPR_HIP_INDEL_VAR_SCAN_H

#include "xgpr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- The notation is that of xgpr_hip_indel_scan.h and xgpr_hip_subst_var_scan.h: sequence i has length s, nk = s -
 * conv_width + 1 windows win_j and tokens t[0 .. s); r(k) = sqrt(1 / num_freqs) / {1, sqrt(k), k}[scaling_type];
 * phi(win)[2f] = cos p_f, phi(win)[2f + 1] = sin p_f for columns < nvar (column 0 := 0 under fit_intercept); z_i are the first
 * nvar columns of the sequence's feature row (column 0 is the constant 1 under fit_intercept) and e0 is the unit vector of
 * column 0 under fit_intercept, 0 otherwise.  A mutant with nk' = nk -+ 1 windows has the normaliser r' = r(nk'); with
 * rho = r' / r(nk) (exactly 1 at scaling_type 0) and  b = rho z_i + (1 - rho) e0  its columns are  z' = b + r' delta  --
 * exactly, not to first order -- where
 *
 *     deletion  of p      : delta = sum_{j' in A_p} phi(mutant window j')       -  sum_{j in R_p} phi(win_j)
 *     insertion of v at g : delta = sum_{j'' in A_{g,v}} phi(mutant window j'') -  sum_{j in R'_g} phi(win_j)
 *
 * over the window ranges of xgpr_hip_indel_scan.h (R_p: the windows that cover p; A_p: the mutant's junction windows; R'_g:
 * the windows that straddle gap g; A_{g,v}: the mutant's windows that hold the inserted token), and
 *
 *     out_del[i, p]    = q_del[i] + 2 r' (delta . u_del[i]) + r'^2 (delta^T vm delta)      r' = r(nk - 1),  0 <= p < s
 *     out_ins[i, g, v] = q_ins[i] + 2 r' (delta . u_ins[i]) + r'^2 (delta^T vm delta)      r' = r(nk + 1),  0 <= g <= s
 *
 * which is z'^T vm z' where the caller passes, per row set, u[i] = 1/2 (vm + vm^T) b and q[i] = b^T vm b with that row set's
 * rho; nothing is symmetrised or rescaled by the library: for any vm, u and q the result is the expression above.
 * tokens, table, radem, chi, seqlen_host / seqlen_dev: as for xgpr_conv_token_indel_scan_f32.  vm[nvar, nvar] float64 with
 * row stride vm_stride >= nvar (elements); u_del, u_ins [n, nvar] and q_del, q_ins [n] float64.  out_del[n, L] and
 * out_ins[n, L + 1, vocab] float64 are each OVERWRITTEN as a whole: positions p >= s and gaps g > s hold exactly 0.0, and
 * the deletions p < s of a sequence with s == conv_width -- its mutant has no window -- hold a quiet NaN at every
 * scaling_type.  The gap g == s appends; the byte behind an appended token is never addressed.
 * Either group (u_del, q_del, out_del) or (u_ins, q_ins, out_ins) may be NULL as a whole: that row set is not computed.
 * nvar: even, 2 <= nvar <= 2 num_freqs; the kernels serve nvar <= 2048 (the first 1024-frequency tile).
 * slab_rows: how many mutant rows -- rows of out_del, then rows of out_ins -- the workspace holds at a time: 0 selects the
 * library's default (128 MiB of rows, at least 16 and at most 65536 rows); any other value must be a multiple of 16 and at
 * least 16.  Each row set is processed slab by slab, two launches each.
 * Arithmetic: per window the float32 cos / sin arguments of xgpr_conv_token_rows_f32, bit for bit; the cos / sin values are
 * widened and summed in float64 in ascending j, the added windows and the removed windows apart, and subtracted once; the
 * rest as for xgpr_conv_token_subst_var_scan_f32 with r' in place of r: out = (q + (2 r') (delta . u)) + (r' r') (delta^T vm
 * delta).  No atomics: results are bit-identical from run to run, depend on the sequence alone -- not on n, on its position in
 * the batch, on slab_rows or on whether the other row set was requested -- and two identical table rows give bit-identical
 * columns of out_ins.
 * workspace: xgpr_conv_token_indel_var_scan_workspace_bytes(radem_shape2, nvar, slab_rows) bytes, exactly: the packed sign
 * masks (xgpr_rbf_workspace_bytes(radem_shape2)) and slab_rows rows of nvar float64; 8-byte aligned.  Its contents never
 * enter the result.  The function returns 0 for an nvar or a slab_rows the call would refuse.
 * xgpr_conv_token_indel_var_scan_ok(width, vocab, C, num_freqs, nvar) is 1 where the kernels serve the shape:
 * xgpr_conv_token_indel_scan_ok(width, vocab, C, num_freqs), nvar even, 2 <= nvar <= 2 num_freqs and nvar <= 2048.
 * Checks, before anything is launched, in this order: n < 0, L < 1, C < 1 or a scaling_type outside 0 .. 2:
 * XGPR_ERR_ARRAY_DIMS; conv_width < 1 or > L: XGPR_ERR_CONV_WIDTH; num_freqs < 1 or > radem_shape2, or radem_shape2 not
 * a multiple of the padded width: XGPR_ERR_RFFS_FREQS; nvar odd, < 2 or > 2 num_freqs: XGPR_ERR_ARRAY_DIMS; vm_stride < nvar:
 * XGPR_ERR_ARRAY_SIZES; slab_rows negative, or neither 0 nor a multiple of 16: XGPR_ERR_ARRAY_DIMS; with n > 0, seqlen_host
 * NULL or a length < conv_width or > L: XGPR_ERR_SEQLEN_RANGE; vocab outside 1 .. 256: XGPR_ERR_ARRAY_DIMS; a shape the _ok
 * predicate refuses: XGPR_ERR_UNSUPPORTED (the caller materialises the mutants); n == 0: returns 0, nothing launched; a
 * workspace that is NULL, misaligned or smaller than _workspace_bytes, a NULL array, a group given by halves or both groups
 * NULL: XGPR_ERR_WORKSPACE; n * (L + 1) >= 2^24: XGPR_ERR_UNSUPPORTED, split the batch. */
int xgpr_conv_token_indel_var_scan_ok(long width, long vocab, long C, long num_freqs, long nvar);
size_t xgpr_conv_token_indel_var_scan_workspace_bytes(long radem_shape2, long nvar, long slab_rows);
int xgpr_conv_token_indel_var_scan_f32(const uint8_t *tokens, const float *table, const double *vm, long vm_stride,
                                       const double *u_del, const double *q_del, const double *u_ins, const double *q_ins,
                                       double *out_del, double *out_ins, const int8_t *radem, const float *chi,
                                       const int32_t *seqlen_host, const int32_t *seqlen_dev, long n, long L, long vocab,
                                       long C, long num_freqs, long radem_shape2, long nvar, int conv_width, int scaling_type,
                                       int fit_intercept, long slab_rows, void *workspace, size_t workspace_bytes,
                                       void *stream);

#ifdef __cplusplus
}
#endif
#endif /* XGPR_HIP_INDEL_VAR_SCAN_H */
