/* xgpr_hip/pool_edits.h -- C ABI of libxgpr_hip.so, twelfth part: the pooled first-layer row of the two-layer
 * convolution kernel (Conv1dTwoLayer) for EVERY single-token substitution, deletion and insertion of a token sequence.
 *
 * The conventions, the error codes and xgpr_last_error() are those of xgpr_hip.h, which this header includes: device
 * pointers unless a name ends in `_host`, nothing retained or allocated, every call asynchronous and stream-ordered,
 * 0 on success and a negative code otherwise.
 *
 * Why a twelfth header, and why in a subdirectory: as for the second to the eleventh, the sets of names declared in the
 * earlier headers are pinned, name by name, to tables inside existing test files; and one existing test
 * (tests/test_pair_scan_host.py) pins the NUMBER of .h files directly in include/ and of tables in xgpr_amd/_lib.py whose
 * name ends in SIGNATURES.  A change that may not touch those tests therefore declares its entry points here, in
 * include/xgpr_hip/, binds them through xgpr_amd/_lib.py POOL_EDITS_ABI, and holds them to the same guarantees by tests
 * of their own (tests/test_pool_edits_host.py, tests/test_gpu_pool_edits_memory_contract.py).
 */
#ifndef XGPR_HIP_POOL_EDITS_H
#define XGPR_HIP_POOL_EDITS_H

#include "../xgpr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- q(mutant) for every single edit, without writing a mutant (no counterpart in the reference).  tokens[n, L] (uint8,
 * values < vocab) index the rows of table[vocab, C] float32, UNSCALED as for xgpr_conv_token_maxpool_f32.  Sequence i has
 * length s and nk = s - conv_width + 1 k-mers; nkmax = L - conv_width + 1; F = num_rffs filters.  With p_{j,f} =
 * chi_f SORF(win_j)_f -- the projections of xgpr_conv_token_maxpool_f32 bit for bit -- the pooled value is
 * q_f = max(0, max_j p_{j,f}), and because a maximum is order-free the pooled row of a mutant is
 *
 *     row = max(PM[i, a], SM[i, b], max over the windows the edit creates)
 *     PM[i, j, f] = max(0, p_{0,f} .. p_{j-1,f})      SM[i, j, f] = max(0, p_{j,f} .. p_{nk-1,f})
 *
 * xgpr_conv_token_maxpool_tables_f32 writes pm and sm, float32 [n, nkmax + 1, F], both OVERWRITTEN as a whole:
 * PM[i, 0] = 0, SM[i, nk] = 0, rows j > nk are exact zeros.  PM[i, j] is what xgpr_conv_token_maxpool_f32 leaves in a zeroed
 * row for the sequence cut to its first j windows, SM[i, j] for the sequence from token j on.
 *
 * xgpr_conv_token_maxpool_edits_f32 reads them and writes the rows of the slots [slot_lo, slot_lo + nslots) of the
 * flattened (sequence, slot) index into out, which holds nslots slots (the caller slabs the output, L V F 4 bytes per
 * sequence for the substitutions):
 *
 *     mode XGPR_POOL_EDIT_SUBST  slot l of L:      out[., v, :] = q(token l replaced by table row v)        [nslots, vocab, F]
 *          new windows j in [max(0, l-cw+1), min(l, nk-1)];  a = jlo, b = jhi + 1
 *     mode XGPR_POOL_EDIT_DEL    slot p of L:      out[., :]    = q(token p removed)                        [nslots, F]
 *          new windows j' in [max(0, p-cw+1), min(p-1, nk-2)];  a = jlo, b = min(p, nk-1) + 1;  nk == 1: the row is NaN
 *     mode XGPR_POOL_EDIT_INS    slot g of L + 1:  out[., v, :] = q(row v inserted before g; g = s appends) [nslots, vocab, F]
 *          new windows j'' in [max(0, g-cw+1), min(g, nk)];  a = jlo, b = min(g-1, nk-1) + 1
 *
 * Slots past the sequence (l, p >= s; g > s) are exact zero rows.  A substitution's own token gives the sequence's own row.
 * Values and the sign of zero: every value EQUALS, as a real number, what xgpr_conv_token_maxpool_f32 leaves in a zeroed
 * row for the written-out mutant, and is BIT-IDENTICAL to it wherever it is not zero.  The SIGN OF A ZERO IS UNSPECIFIED:
 * the operator's update acc = acc > p ? acc : p lets a product of -0.0 replace +0.0, so the sign of a zero depends on the
 * order of the windows (an exact zero product needs an all-zero table row, e.g. a padding token); the same holds for pm and
 * sm.  No atomics: results are bit-identical from run to run and a sequence's rows depend on that sequence alone.
 * seqlen_host / seqlen_dev: the int32 lengths [n] on the host (validated there) and on the device; tokens past a
 * sequence's length are never read.  radem_shape2 == ceil(num_rffs / P) P with P the padded window width.
 * workspace: xgpr_rbf_workspace_bytes(radem_shape2) bytes, the packed sign masks (what xgpr_conv_workspace_bytes returns for
 * the max-pool operator is never less: one buffer serves both); each call packs them again.
 * xgpr_conv_token_maxpool_edits_ok(width, vocab, C, num_rffs) is 1 where the kernels serve a window of width =
 * conv_width * C elements: the shapes of xgpr_conv_token_maxpool_input_grad_ok (padded width up to 1024, a table of at
 * most 4608 floats) with num_rffs >= 1.
 * Checks, before anything is launched, in the order and with the codes of xgpr_conv_token_maxpool_f32 (the edits: first a
 * mode other than the three: XGPR_ERR_ARRAY_DIMS): vocab outside 1 .. 256 or C < 1: XGPR_ERR_ARRAY_DIMS; n == 0:
 * XGPR_ERR_NO_DATAPOINTS; num_rffs odd or < 2: XGPR_ERR_ODD_OUTPUT; num_rffs > radem_shape2: XGPR_ERR_RFFS_FREQS; nseq !=
 * n: XGPR_ERR_SEQLEN_SIZE; conv_width < 1 or > L: XGPR_ERR_CONV_WIDTH; radem_shape2 != ceil(num_rffs / P) P:
 * XGPR_ERR_RFFS_FREQS; seqlen_host NULL or a length < conv_width or > L: XGPR_ERR_SEQLEN_RANGE; seqlen_dev or another
 * array NULL: XGPR_ERR_WORKSPACE; a shape xgpr_conv_token_maxpool_edits_ok refuses: XGPR_ERR_UNSUPPORTED; a workspace
 * smaller than the sign masks: XGPR_ERR_WORKSPACE; the edits: a slot range outside [0, n * slots per sequence]:
 * XGPR_ERR_ARRAY_SIZES, nslots == 0: returns 0; more than 2^24 - 1 slots (tables: n (nkmax + 1) windows) in one launch:
 * XGPR_ERR_UNSUPPORTED. */
#define XGPR_POOL_EDIT_DEL   1
#define XGPR_POOL_EDIT_INS   2
#define XGPR_POOL_EDIT_SUBST 3
int xgpr_conv_token_maxpool_edits_ok(long width, long vocab, long C, long num_rffs);
int xgpr_conv_token_maxpool_tables_f32(const uint8_t *tokens, const float *table, float *pm, float *sm, const int8_t *radem,
                                       const float *chi, const int32_t *seqlen_host, const int32_t *seqlen_dev, long n,
                                       long L, long vocab, long C, long num_rffs, long radem_shape2, long nseq,
                                       int conv_width, void *workspace, size_t workspace_bytes, void *stream);
int xgpr_conv_token_maxpool_edits_f32(const uint8_t *tokens, const float *table, const float *pm, const float *sm,
                                      float *out, const int8_t *radem, const float *chi, const int32_t *seqlen_host,
                                      const int32_t *seqlen_dev, long n, long L, long vocab, long C, long num_rffs,
                                      long radem_shape2, long nseq, int conv_width, int mode, long slot_lo, long nslots,
                                      void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* XGPR_HIP_POOL_EDITS_H */
