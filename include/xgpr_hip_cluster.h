/* xgpr_hip_cluster.h -- C ABI of libxgpr_hip.so, sixth part: the two contractions of a Lloyd (k-means) iteration over float32
 * feature rows -- the nearest centre of every row, and the per-cluster sums of the rows.
 *
 * The conventions, the error codes and xgpr_last_error() are those of xgpr_hip.h, which this header includes: device
 * pointers unless a name ends in `_host`, nothing retained or allocated, every call asynchronous and stream-ordered,
 * 0 on success and a negative code otherwise.
 *
 * Why a sixth header: as for the second to fifth -- the sets of names declared in the earlier headers are pinned, name by
 * name, to tables inside existing test files.  The entry points below are bound through xgpr_amd/_lib.py
 * CLUSTER_SIGNATURES and held to the same guarantees by tests of their own (tests/test_cluster_host.py,
 * tests/test_gpu_kmeans_memory_contract.py).
 */
#ifndef XGPR_HIP_CLUSTER_H
#define XGPR_HIP_CLUSTER_H

#include "xgpr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- kernel k-means on random features (no counterpart in the reference: docs/advanced/auxiliary_tutorial.rst names the use
 * and stops at the feature generator).  rows[n, num_rffs] float32 is any row array this library writes
 * (xgpr_rbf_feature_cache_f32, xgpr_conv_feature_rows_f32, xgpr_conv_token_rows_f32, or float64 features rounded to float32),
 * TAKEN AS IT IS: no scale, no intercept column.  A caller that wants feature units multiplies centres by the rows' scale.
 *
 * xgpr_kmeans_ok(num_rffs, k) is 1 where both operators serve the shape: num_rffs >= 4, num_rffs % 4 == 0, 1 <= k <= 256.
 *
 * xgpr_kmeans_assign_f32: centers[k, num_rffs] float64, row-major.  With
 *     cn_k  = sum_m centers[k, m]^2                        (computed here, in a fixed order, into the workspace)
 *     s_ik  = cn_k - 2 sum_m rows[i, m] centers[k, m]
 * labels[i] (int32) = the LOWEST k that minimises s_ik in this operator's own arithmetic (a strict < in ascending k), and
 * dist2[i] (float64, may be NULL) = max(0, sum_m rows[i, m]^2 + s_{i, labels[i]}).  Both are OVERWRITTEN as a whole.
 * Arithmetic: every product and sum in float64, the rows widened exactly (v_mfma_f64_16x16x4_f64 for the contraction).  Every
 * centre column runs through the same instruction sequence: two centres with identical contents give bit-identical s_ik and
 * the lower index is chosen.
 * workspace: xgpr_kmeans_assign_workspace_bytes(n, num_rffs, k) bytes.
 *
 * xgpr_kmeans_update_f32: sums[k', m] (+)= sum over {i : labels[i] == k'} of rows[i, m] in float64, counts[k'] (int64) (+)=
 * the number of such rows.  A label outside [0, k) (for example -1, "unassigned") is skipped: it touches nothing of sums or
 * counts.  accumulate == 0: EVERY element of sums and counts is written (zeros for an empty cluster); accumulate != 0: the
 * results are added to what the arrays hold (a shard longer than one window of rows).
 * workspace: xgpr_kmeans_update_workspace_bytes(n, num_rffs, k) bytes (one [k, num_rffs] float64 slab per range of rows; 0 for
 * n == 0, and then workspace may be NULL).
 *
 * Both: no floating-point atomics; a fixed summation order, so results are bit-identical from run to run for a given
 * (n, num_rffs, k).  rows, centers and sums are 16-byte aligned.  n == 0 returns 0 (update with accumulate == 0 still
 * writes its zeros).
 * Checks, before anything is launched, in this order: n < 0, num_rffs < 1 or k < 1: XGPR_ERR_ARRAY_DIMS; a shape
 * xgpr_kmeans_ok refuses: XGPR_ERR_UNSUPPORTED; assign with n == 0: returns 0; a NULL array (update: sums and counts always,
 * rows and labels with n > 0) or a misaligned one: XGPR_ERR_WORKSPACE; a workspace that is NULL, misaligned or smaller than
 * advertised: XGPR_ERR_WORKSPACE; n >= 2^31 - 1024: XGPR_ERR_UNSUPPORTED. */
int xgpr_kmeans_ok(long num_rffs, long k);
size_t xgpr_kmeans_assign_workspace_bytes(long n, long num_rffs, long k);
int xgpr_kmeans_assign_f32(const float *rows, const double *centers, int32_t *labels, double *dist2, long n, long num_rffs,
                           long k, void *workspace, size_t workspace_bytes, void *stream);
size_t xgpr_kmeans_update_workspace_bytes(long n, long num_rffs, long k);
int xgpr_kmeans_update_f32(const float *rows, const int32_t *labels, double *sums, long long *counts, long n, long num_rffs,
                           long k, int accumulate, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* XGPR_HIP_CLUSTER_H */
