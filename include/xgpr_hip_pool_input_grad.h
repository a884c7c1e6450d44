/* xgpr_hip_pool_input_grad.h -- C ABI of libxgpr_hip.so, fifth part: the backward of the two-layer kernel's FIRST layer
 * (random convolution filters, ReLU, max-pool over the k-mers) with respect to the INPUT: one value per position and
 * channel.
 *
 * The conventions, the error codes and xgpr_last_error() are those of xgpr_hip.h, which this header includes: device
 * pointers unless a name ends in `_host`, nothing retained or allocated, every call asynchronous and stream-ordered,
 * 0 on success and a negative code otherwise.
 *
 * Why a fifth header: as for the second, third and fourth -- the sets of names declared in the earlier headers are
 * pinned, name by name, to tables inside existing test files.  The entry points below are bound through
 * xgpr_amd/_lib.py POOL_INPUT_GRAD_SIGNATURES and held to the same guarantees by tests of their own
 * (tests/test_pool_input_grad_host.py, tests/test_gpu_pool_input_grad_memory_contract.py).
 */
#ifndef XGPR_HIP_POOL_INPUT_GRAD_H
#define XGPR_HIP_POOL_INPUT_GRAD_H

#include "xgpr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- d m / d x through q(x), the pooled row of xgpr_conv1d_maxpool_f32 on a zeroed output (no counterpart in the
 * reference).  A sequence x[L, C] of length s has nk = s - conv_width + 1 k-mers; window j is x[j : j + conv_width, :]
 * flattened.  With p_{j,f} = chi_f SORF(win_j)_f and q_f = max(0, max_j p_{j,f}), for g[i, f] = d m / d q_f of any
 * scalar m:
 *
 *     argmax[i, f] = a_f = the FIRST j with p_{j,f} = max_j' p_{j',f} if that maximum is > 0, else -1
 *     out[l, c] = d m / d x[l, c] = sum_{j = max(0, l-conv_width+1)}^{min(l, nk-1)} (W^T u_j)[(l - j) C + c],
 *     u_{j,f} = g_f [a_f == j]
 *
 * with W^T the transposed SORF of xgpr_rbf_input_grad_f32 over this layer's draws.  The subgradient convention is fixed:
 * the first k-mer that attains the maximum wins (a strict > in ascending j), a maximum <= 0 contributes nothing (ReLU
 * inactive).  The projections are those of xgpr_conv1d_maxpool_f32 bit for bit, so argmax >= 0 exactly where that
 * operator's value is > 0.
 * x[n, L, C] float32 is UNSCALED, as for the max-pool operator (the lengthscale multiplies q, not x).  g is float64
 * [n, g_row_stride] with g_row_stride >= num_freqs; g_row_stride == 0 is ONE vector g[num_freqs] for all sequences;
 * what lies between num_freqs and the stride is never read.  out[n, L, C] float64 and argmax[n, num_freqs] int32 are
 * OVERWRITTEN as a whole: positions l >= s of out hold exactly 0.0.  argmax is required.  seqlen_host / seqlen_dev: the
 * int32 lengths [n] on the host (validated there) and on the device.  radem_shape2 == ceil(num_freqs / P) P with P the
 * padded window width, as for the max-pool operator.
 * The token form takes tokens[n, L] (uint8, values < vocab) and table[vocab, C] float32 in place of x and returns, bit
 * for bit, what the dense form returns on table[tokens]; tokens past a sequence's length are never read.
 * Arithmetic: float32 butterflies; g_f rounded ONCE to float32 and multiplied by chi_f in float32; tiles and repetitions
 * summed in float64 in a fixed order; the windows' gradients added per position in float64 in ascending j.  No atomics:
 * results are bit-identical from run to run, and a sequence's result depends on that sequence alone -- not on n, its
 * position in the batch, or whether g arrives shared or per row.
 * workspace: xgpr_rbf_workspace_bytes(radem_shape2) bytes (the packed sign masks).
 * xgpr_conv_maxpool_input_grad_ok(width) is 1 where the kernel serves a window of width = conv_width * C elements:
 * padded width up to 1024.  xgpr_conv_token_maxpool_input_grad_ok(width, vocab, C): that and xgpr_conv_token_rows_ok (a
 * table of at most 4608 floats).
 * Checks, before anything is launched, in this order: n < 0, L < 1 or C < 1: XGPR_ERR_ARRAY_DIMS; conv_width < 1 or
 * > L: XGPR_ERR_CONV_WIDTH; num_freqs < 1 or radem_shape2 != ceil(num_freqs / P) P: XGPR_ERR_RFFS_FREQS;
 * 0 < g_row_stride < num_freqs: XGPR_ERR_ARRAY_SIZES; with n > 0, seqlen_host NULL or a length < conv_width or > L:
 * XGPR_ERR_SEQLEN_RANGE; tokens: vocab outside 1 .. 256: XGPR_ERR_ARRAY_DIMS; a shape the _ok predicate refuses:
 * XGPR_ERR_UNSUPPORTED; n == 0: returns 0, nothing launched; a workspace smaller than
 * xgpr_rbf_workspace_bytes(radem_shape2) or a NULL array: XGPR_ERR_WORKSPACE. */
int xgpr_conv_maxpool_input_grad_ok(long width);
int xgpr_conv_token_maxpool_input_grad_ok(long width, long vocab, long C);
int xgpr_conv_maxpool_input_grad_f32(const float *x, const double *g, double *out, int32_t *argmax, const int8_t *radem,
                                     const float *chi, const int32_t *seqlen_host, const int32_t *seqlen_dev, long n,
                                     long L, long C, long g_row_stride, long num_freqs, long radem_shape2,
                                     int conv_width, void *workspace, size_t workspace_bytes, void *stream);
int xgpr_conv_token_maxpool_input_grad_f32(const uint8_t *tokens, const float *table, const double *g, double *out,
                                           int32_t *argmax, const int8_t *radem, const float *chi,
                                           const int32_t *seqlen_host, const int32_t *seqlen_dev, long n, long L,
                                           long vocab, long C, long g_row_stride, long num_freqs, long radem_shape2,
                                           int conv_width, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* XGPR_HIP_POOL_INPUT_GRAD_H */
