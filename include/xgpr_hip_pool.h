/* xgpr_hip_pool.h -- C ABI of libxgpr_hip.so, second part: the entry points of the pooled first layer of the
 * two-layer convolution kernel (Conv1dTwoLayer).
 *
 * The conventions, the error codes and xgpr_last_error() are those of xgpr_hip.h, which this header includes: device
 * pointers unless a name ends in `_host`, nothing retained or allocated, every call asynchronous and stream-ordered,
 * 0 on success and a negative code otherwise.
 *
 * Why a second header: the set of names declared in xgpr_hip.h is pinned, name by name, to tables that live inside
 * existing test files (the ctypes table and the device-memory contract).  An entry point added by a change that may
 * not touch those tables is declared here, bound through xgpr_amd/_lib.py POOL_SIGNATURES, and held to the same
 * guarantees by tests of its own (tests/test_pool_header_host.py, tests/test_gpu_pool_memory_contract.py).  A change
 * that may edit the tables folds this header back into xgpr_hip.h.
 */
#ifndef XGPR_HIP_POOL_H
#define XGPR_HIP_POOL_H

#include "xgpr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- token-indexed input for cudaConv1dMaxpool (no counterpart in the reference, which takes dense arrays only: this
 * replaces "expand table[tokens] to float32 [n, L, C] on the host, then xgpr_conv1d_maxpool_f32").  tokens[n, L] (uint8,
 * row-major) index the rows of table[vocab, C] (float32, row-major, vocab 1 .. 256); element e of the window of k-mer j
 * is table[tokens[i, j + e / C]][e % C].  out[n, num_rffs] float32 is READ AND WRITTEN: out = max(out, chi *
 * sorf(window)) over the k-mers, so the caller zero-fills it (that is the ReLU of the first layer).  The result is
 * BIT-IDENTICAL to xgpr_conv1d_maxpool_f32 on the expanded array (same kernel body after the window fetch).
 * Checks, in the sibling's order: out_rows == n, num_freqs == num_rffs, radem_shape2 == reps * P exactly (P =
 * conv_width * C padded to a power of two), nseq == n, conv_width in 1 .. L; sequence lengths are validated on the
 * host (seqlen_host) before any launch, seqlen_dev is their device copy.  And the token entries' checks: vocab outside
 * 1 .. 256 or C < 1: XGPR_ERR_ARRAY_DIMS; a NULL tokens / table / out pointer or a workspace smaller than the sign
 * masks: XGPR_ERR_WORKSPACE; a shape where xgpr_conv_token_rows_ok(conv_width * C, vocab, C) is 0 (a window beyond
 * 1024 elements, a table beyond 4608 floats): XGPR_ERR_UNSUPPORTED -- the caller expands slice by slice and calls the
 * dense sibling.  Nothing is launched on an error.  Token values must be < vocab (not checked on the device);
 * positions beyond a sequence's length are never read.
 * Workspace: xgpr_conv_workspace_bytes(radem_shape2, conv_width * C, 4, nseq), as for the dense operator (sign masks,
 * then the longest-first order of nseq sequences); with less than the order needs the order is skipped (results
 * unchanged). */
int xgpr_conv_token_maxpool_f32(const uint8_t *tokens, const float *table, float *out, const int8_t *radem,
                                const float *chi, const int32_t *seqlen_host, const int32_t *seqlen_dev,
                                long n, long L, long vocab, long C, long out_rows, long num_rffs, long num_freqs,
                                long radem_shape2, long nseq, int conv_width,
                                void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* XGPR_HIP_POOL_H */
