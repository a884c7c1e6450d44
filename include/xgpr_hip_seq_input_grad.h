/* xgpr_hip_seq_input_grad.h -- C ABI of libxgpr_hip.so, fourth part: the derivative of a weighted sum of random features
 * with respect to the INPUT for the sequence and graph kernels (Conv1d*, Graph*): one value per position and channel.
 *
 * The conventions, the error codes and xgpr_last_error() are those of xgpr_hip.h, which this header includes: device
 * pointers unless a name ends in `_host`, nothing retained or allocated, every call asynchronous and stream-ordered,
 * 0 on success and a negative code otherwise.
 *
 * Why a fourth header: as for xgpr_hip_pool.h and xgpr_hip_input_grad.h -- the sets of names declared in the earlier
 * headers are pinned, name by name, to tables inside existing test files.  The entry points below are bound through
 * xgpr_amd/_lib.py SEQ_INPUT_GRAD_SIGNATURES and held to the same guarantees by tests of their own
 * (tests/test_seq_input_grad_host.py, tests/test_gpu_seq_input_grad_memory_contract.py).
 */
#ifndef XGPR_HIP_SEQ_INPUT_GRAD_H
#define XGPR_HIP_SEQ_INPUT_GRAD_H

#include "xgpr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- d / dx of  m(x) = sum_col w[col] z_col(x)  over the feature row z(x) of xgpr_conv_feature_rows_f32 (no counterpart
 * in the reference).  A sequence x[L, C] of length s has nk = s - conv_width + 1 k-mers; window j is
 * x[j : j + conv_width, :] flattened.  With p_j = W (sigma win_j) the projections (W the SORF matrix times chi),
 * r = sqrt(1 / num_freqs) / {1, sqrt(nk), nk}[scaling_type] (the same constant with and without the intercept) and
 * z[2f] = r sum_j cos p_{j,f}, z[2f+1] = r sum_j sin p_{j,f}:
 *
 *     g[l, c] = d m / d x[l, c] = sigma  sum_{j = max(0, l-conv_width+1)}^{min(l, nk-1)}  (W^T u_j)[(l - j) C + c],
 *     u_{j,f} = r (w[2f+1] cos p_{j,f} - w[2f] sin p_{j,f})
 *
 * with W^T the transposed SORF of xgpr_rbf_input_grad_f32.  Graph kernels are conv_width == 1.
 * x[n, L, C] float32 arrives ALREADY multiplied by sigma, as for the feature operators (sigma is passed for the chain
 * rule only); g[n, L, C] float64 is OVERWRITTEN as a whole: positions l >= s hold exactly 0.0.  seqlen_host /
 * seqlen_dev: the int32 lengths [n] on the host (validated there) and on the device, as for
 * xgpr_conv_feature_rows_f32.  w, w_row_stride, w_cols and fit_intercept mean what they mean for
 * xgpr_rbf_input_grad_f32: w_row_stride == 0 is ONE weight vector w[w_cols] for all sequences, otherwise w is
 * [n, w_row_stride] and what lies between w_cols and the stride is never read; only the first w_cols columns carry
 * weight (even, 2 <= w_cols <= 2 num_freqs); under fit_intercept w[0] is dropped.
 * The token form takes tokens[n, L] (uint8, values < vocab) and table[vocab, C] float32 (ALREADY multiplied by sigma) in
 * place of x and returns, bit for bit, what the dense form returns on table[tokens]; tokens past a sequence's length
 * are never read.
 * Arithmetic: per window that of xgpr_rbf_input_grad_f32 (float32 butterflies, u_j formed in float64 and rounded once,
 * tiles and repetitions summed in float64 in a fixed order); the windows' gradients are added per position in float64 in
 * ascending j.  No atomics: results are bit-identical from run to run, and a sequence's result depends on that
 * sequence alone -- not on n, its position in the batch, or whether the weights arrive shared or per row.
 * workspace: xgpr_rbf_workspace_bytes(radem_shape2) bytes (the packed sign masks).
 * xgpr_conv_input_grad_ok(width, num_freqs) is 1 where the kernel serves a window of width = conv_width * C elements:
 * padded width up to 1024.  xgpr_conv_token_input_grad_ok(width, vocab, C): that and xgpr_conv_token_rows_ok (a table of
 * at most 4608 floats).
 * Checks, before anything is launched, in this order: n < 0, L < 1, C < 1 or a scaling_type outside 0 .. 2:
 * XGPR_ERR_ARRAY_DIMS; conv_width < 1 or > L: XGPR_ERR_CONV_WIDTH; num_freqs < 1 or > radem_shape2, or radem_shape2 not
 * a multiple of the padded width: XGPR_ERR_RFFS_FREQS; w_cols odd or < 2: XGPR_ERR_ODD_OUTPUT; w_cols > 2 num_freqs or
 * 0 < w_row_stride < w_cols: XGPR_ERR_ARRAY_SIZES; with n > 0, seqlen_host NULL or a length < conv_width or > L:
 * XGPR_ERR_SEQLEN_RANGE; tokens: vocab outside 1 .. 256: XGPR_ERR_ARRAY_DIMS; a shape the _ok predicate refuses:
 * XGPR_ERR_UNSUPPORTED (the caller unfolds the windows into rows of xgpr_rbf_input_grad_f32); n == 0: returns 0,
 * nothing launched; a workspace smaller than xgpr_rbf_workspace_bytes(radem_shape2) or a NULL array:
 * XGPR_ERR_WORKSPACE. */
int xgpr_conv_input_grad_ok(long width, long num_freqs);
int xgpr_conv_token_input_grad_ok(long width, long vocab, long C);
int xgpr_conv_input_grad_f32(const float *x, const double *w, double *g, const int8_t *radem, const float *chi,
                             const int32_t *seqlen_host, const int32_t *seqlen_dev, long n, long L, long C,
                             long w_row_stride, long w_cols, long num_freqs, long radem_shape2, double sigma,
                             int conv_width, int scaling_type, int fit_intercept, void *workspace,
                             size_t workspace_bytes, void *stream);
int xgpr_conv_token_input_grad_f32(const uint8_t *tokens, const float *table, const double *w, double *g,
                                   const int8_t *radem, const float *chi, const int32_t *seqlen_host,
                                   const int32_t *seqlen_dev, long n, long L, long vocab, long C, long w_row_stride,
                                   long w_cols, long num_freqs, long radem_shape2, double sigma, int conv_width,
                                   int scaling_type, int fit_intercept, void *workspace, size_t workspace_bytes,
                                   void *stream);

#ifdef __cplusplus
}
#endif
#endif /* XGPR_HIP_SEQ_INPUT_GRAD_H */
