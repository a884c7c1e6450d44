/* xgpr_hip_input_grad.h -- C ABI of libxgpr_hip.so, third part: the derivative of a weighted sum of random features
 * with respect to the INPUT (the transposed SORF), for the fixed-vector kernels RBF / Matern / Cauchy.
 *
 * The conventions, the error codes and xgpr_last_error() are those of xgpr_hip.h, which this header includes: device
 * pointers unless a name ends in `_host`, nothing retained or allocated, every call asynchronous and stream-ordered,
 * 0 on success and a negative code otherwise.
 *
 * Why a third header: as for xgpr_hip_pool.h -- the sets of names declared in the first two headers are pinned, name by
 * name, to tables inside existing test files.  The entry points below are bound through xgpr_amd/_lib.py
 * INPUT_GRAD_SIGNATURES and held to the same guarantees by tests of their own (tests/test_input_grad_host.py,
 * tests/test_gpu_input_grad_memory_contract.py).
 */
#ifndef XGPR_HIP_INPUT_GRAD_H
#define XGPR_HIP_INPUT_GRAD_H

#include "xgpr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- d / dx of  m(x) = sum_j w[j] z_j(x)  over the feature row z(x) of xgpr_rbf_feature_gen_f32 (no counterpart in the
 * reference).  With p = W (sigma x) the projections (W the SORF matrix times chi), c the operator's float-typed constant
 * and z[2f] = c cos p_f, z[2f+1] = c sin p_f:
 *
 *     g = d m / d x = sigma W^T u,      u_f = c (w[2f+1] cos p_f - w[2f] sin p_f)
 *
 * x[n, d] float32 arrives ALREADY multiplied by sigma, as for every feature operator (sigma is passed for the chain rule
 * only); g[n, d] float64 is OVERWRITTEN.  Under fit_intercept w[0] is dropped: column 0 of the features is the constant
 * 1.  Only the first w_cols columns carry weight (w_cols even, 2 <= w_cols <= 2 num_freqs; tiles of frequencies past it
 * are skipped): the gradient of the predictive variance uses the first `variance_rffs` columns.
 * w_row_stride == 0: ONE weight vector w[w_cols] float64 for all rows; otherwise w is [n, w_row_stride] with
 * w_row_stride >= w_cols, and what lies between w_cols and the stride is never read.
 * Arithmetic: the float32 cos / sin arguments are those of the feature operators bit for bit; u_f is formed in float64
 * and rounded once to float32, the transposed transform runs on float32 butterflies, the sums over repetitions and tiles
 * and the product with sigma are float64.  No atomics: results are bit-identical from run to run, and a row's result
 * does not depend on n or on the row's position.
 * xgpr_rbf_input_grad_ok(d, num_freqs) is 1 where the kernel serves the shape: padded width of d up to 1024.
 * Checks, before anything is launched: n < 0 or d < 1: XGPR_ERR_ARRAY_DIMS; num_freqs < 1 or > radem_shape2, or
 * radem_shape2 not a multiple of the padded width: XGPR_ERR_RFFS_FREQS; w_cols odd or < 2: XGPR_ERR_ODD_OUTPUT; w_cols >
 * 2 num_freqs or 0 < w_row_stride < w_cols: XGPR_ERR_ARRAY_SIZES; padded width beyond 1024: XGPR_ERR_UNSUPPORTED (the
 * caller composes the gradient from the feature operator and three transforms); n == 0: returns 0, nothing launched; a
 * workspace smaller than xgpr_rbf_workspace_bytes(radem_shape2) or a NULL array: XGPR_ERR_WORKSPACE. */
int xgpr_rbf_input_grad_ok(long d, long num_freqs);
int xgpr_rbf_input_grad_f32(const float *x, const double *w, double *g, const int8_t *radem, const float *chi,
                            long n, long d, long w_row_stride, long w_cols, long num_freqs, long radem_shape2,
                            double sigma, int fit_intercept, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* XGPR_HIP_INPUT_GRAD_H */
