/* xgpr_hip/site_scan.h -- C ABI of libxgpr_hip.so, fourteenth part: the exact COMBINATORIAL site-saturation scan of the
 * sequence and graph kernels (Conv1d*, Graph*): K chosen positions, every one of the vocab^K variants, as a sum of small
 * tables -- one per set of sites that a k-mer window can see together.
 *
 * The conventions, the error codes and xgpr_last_error() are those of xgpr_hip.h, which this header includes: device
 * pointers unless a name ends in `_host`, nothing retained or allocated, every call asynchronous and stream-ordered,
 * 0 on success and a negative code otherwise.
 *
 * Why a fourteenth header, and why in a subdirectory: see the opening comment of xgpr_hip/pool_edits.h.  The entry points
 * below are bound through xgpr_amd/_lib.py SITE_SCAN_ABI and held to the guarantees of the others by tests of their own
 * (tests/test_site_scan_host.py, tests/test_gpu_site_scan_memory_contract.py).
 */
#ifndef XGPR_HIP_SITE_SCAN_H
#define XGPR_HIP_SITE_SCAN_H

#include "../xgpr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- The notation is that of xgpr_hip_subst_scan.h: sequence i has length s, nk = s - conv_width + 1 k-mers and tokens
 * t[0 .. s); c(win) is a window's score, r the row constant, m = sum_col w[col] z_col.  The sites p_0 < ... < p_{K-1} are
 * shared by all n sequences of a call.  As the window start j slides over 0 .. L - conv_width the sites that window j covers
 * are a contiguous range of the site list, and one set of sites is covered for one contiguous range of j: a RUN rho with
 * windows j_lo .. j_hi and sites p_a .. p_{a+g-1}.  All windows of a run depend on the same g sites; their summed score is one
 * table [vocab^g], stored at offset off_rho of a row of out, the entry of the assignment (a_0 .. a_{g-1}) at index
 * sum_m a_m vocab^(g-1-m) (the run's last site is contiguous).  out[n, T] float64, T = sum_rho vocab^g, is OVERWRITTEN as a
 * whole:
 *
 *     out[i, off_rho + idx] = r sum_{j = j_lo .. min(j_hi, nk - 1)} [ c(win_j with a_m at p_{a+m}, all m) - c(win_j) ]
 *
 * and for EVERY assignment A of the K sites
 *
 *     m(t[p_k := A_k for all k]) - m(t) = sum_rho out[i, off_rho + idx_rho(A)]
 *
 * exactly (no counterpart in the reference): a window that covers a site belongs to exactly one run and sees that run's
 * sites alone; every other window cancels.
 *
 * xgpr_conv_token_site_scan_layout is host only and launches nothing: the runs of a site list in ascending window order --
 * run_first_window / run_last_window over 0 .. L - conv_width, run_first_site (an index into sites_host), run_sites (g) and
 * run_offset (off_rho) --, at most max_runs of them; it returns the run count (at most 2 K - 1) or a negative code.  T is the
 * last offset plus the last table's size vocab^g.  All five output arrays may be NULL to query the count alone.  Checks, in
 * order: L < 1: XGPR_ERR_ARRAY_DIMS; conv_width < 1 or > L: XGPR_ERR_CONV_WIDTH; vocab outside 1 .. 256, K < 1, K > 16,
 * sites_host NULL, a site outside 0 .. L - 1 or sites not strictly ascending: XGPR_ERR_ARRAY_DIMS; a T that does not fit 62
 * bits: XGPR_ERR_UNSUPPORTED; an output array given and max_runs below the run count: XGPR_ERR_ARRAY_DIMS.
 *
 * xgpr_conv_token_site_scan_f32: tokens, table (ALREADY multiplied by sigma), w (ONE float64 vector [2 num_freqs] shared by
 * all sequences), radem, chi and seqlen_host / seqlen_dev are those of xgpr_conv_token_pair_scan_f32.  The workspace is
 * xgpr_conv_token_site_scan_workspace_bytes(radem_shape2, n, K) bytes: the packed sign masks
 * (xgpr_rbf_workspace_bytes(radem_shape2)) and n (2 K - 1) doubles, one per sequence and possible run (see below).
 * Guarantees: a run with no window inside sequence i (j_lo > nk - 1) holds exactly +0.0; the entry of the sequence's own
 * tokens holds exactly +0.0 in every run, by construction and not by masking: with G[idx] the sum of c over the run's windows
 * with the assignment in place, formed through one code path for every assignment, the sequence's own included, G[own] is
 * copied to the workspace before anything is overwritten and an output is r (G[idx] - G[own]) -- x - x on identical bits at
 * the own assignment.  Two identical table rows a, b give bit-equal slices a and b along every site axis of every run.  No
 * atomics: results are bit-identical from run to run, and a sequence's row depends on that sequence, the table, w and the
 * sites alone -- not on n or its position in the batch.
 * Arithmetic: per variant window the float32 cos / sin arguments of xgpr_conv_token_rows_f32, bit for bit; the products with
 * the float64 weights and all sums are float64, in a fixed order: G per 1024-frequency tile a fixed tree, tiles and windows
 * ascending, four partial sums added as ((s0 + s1) + s2) + s3; then minus G[own], then times r.
 * One workgroup serves one (sequence, run, assignment of the run's first g - 1 sites): n sum_rho vocab^(g-1) rows per launch.
 * xgpr_conv_token_site_scan_ok(width, vocab, C, num_freqs, max_cover) is xgpr_conv_token_subst_scan_ok(width, vocab, C,
 * num_freqs) and 1 <= max_cover <= 4, max_cover being the largest number of sites in one run.
 * Checks, before anything is launched, in this order: those of xgpr_conv_token_pair_scan_f32 with its codes, down to vocab
 * (n < 0, L < 1, C < 1 or a scaling_type outside 0 .. 2: XGPR_ERR_ARRAY_DIMS; conv_width < 1 or > L: XGPR_ERR_CONV_WIDTH;
 * num_freqs < 1 or > radem_shape2, or radem_shape2 not a multiple of the padded width: XGPR_ERR_RFFS_FREQS; with n > 0,
 * seqlen_host NULL or a length < conv_width or > L: XGPR_ERR_SEQLEN_RANGE; vocab outside 1 .. 256: XGPR_ERR_ARRAY_DIMS);
 * K < 1, K > 16, sites_host NULL, a site outside 0 .. L - 1 or sites not strictly ascending: XGPR_ERR_ARRAY_DIMS; a site >=
 * some sequence's length: XGPR_ERR_SEQLEN_RANGE; a shape the _ok predicate refuses, a run of more than 4 sites among them:
 * XGPR_ERR_UNSUPPORTED (the caller writes the variants out and calls xgpr_conv_token_rows_f32); n == 0: returns 0, nothing
 * launched; a workspace smaller than xgpr_conv_token_site_scan_workspace_bytes(radem_shape2, n, K) or a NULL array:
 * XGPR_ERR_WORKSPACE; n sum_rho vocab^(g-1) >= 2^24: XGPR_ERR_UNSUPPORTED, split the batch.  A refused call writes nothing. */
int xgpr_conv_token_site_scan_ok(long width, long vocab, long C, long num_freqs, int max_cover);
long xgpr_conv_token_site_scan_layout(const int32_t *sites_host, int K, long L, int conv_width, long vocab,
                                      int32_t *run_first_window, int32_t *run_last_window, int32_t *run_first_site,
                                      int32_t *run_sites, int64_t *run_offset, int max_runs);
size_t xgpr_conv_token_site_scan_workspace_bytes(long radem_shape2, long n, int K);
int xgpr_conv_token_site_scan_f32(const uint8_t *tokens, const float *table, const double *w, double *out,
                                  const int8_t *radem, const float *chi, const int32_t *seqlen_host,
                                  const int32_t *seqlen_dev, const int32_t *sites_host, int K, long n, long L, long vocab,
                                  long C, long num_freqs, long radem_shape2, int conv_width, int scaling_type,
                                  int fit_intercept, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* XGPR_HIP_SITE_SCAN_H */
