// edit_scan.inc -- part of xgpr_hip.hip (included inside its anonymous namespace, after seq_input_grad.inc): the exact effect of every
// single-token SUBSTITUTION, DELETION and INSERTION on a weighted sum of the SEQUENCE and GRAPH kernels' random features
// (xgpr_conv_token_subst_scan_f32, include/xgpr_hip_subst_scan.h; xgpr_conv_token_window_scores_f32, xgpr_conv_token_indel_scan_f32,
// include/xgpr_hip_indel_scan.h; DESIGN.md 3.20, 3.21).
//
// Sequence i has length s, nk = s - conv_width + 1 k-mer windows win_j = t[j .. j + cw) and tokens t[0 .. s); the table [V, C] is
// already multiplied by sigma.  A window win with projections p = W win scores  c(win) = sum_f (w[2f] cos p_f + w[2f+1] sin p_f)
// (w[0] dropped under the intercept);  r(k) = sqrt(1 / F) / {1, sqrt k, k}  and  T = sum_{j < nk} c(win_j).  An edit changes only the
// windows that touch its site -- an indel shifts the others, and a shifted window has the same content -- so with scores[i, j] = c(win_j):
//     subst[i, l, v] = r(nk) ( sum_{j in J(l)} c(win_j with the token at offset l - j replaced by v)  -  the same sum at v = t[l] )
//         J(l)  = { j : max(0, l - cw + 1) <= j <= min(l, nk - 1) }                           the windows that cover l
//     del[i, p]      = r' (A_p - R_p)       + (r' - r(nk)) T      r'  = r(nk - 1)
//         R_p   = sum of scores over j in [max(0, p - cw + 1), min(p, nk - 1)]                the windows that cover p
//         A_p   = sum of c over the mutant's windows j' in [max(0, p - cw + 1), min(p - 1, nk - 2)], t[j' .. p) then t[p + 1 .. j' + cw + 1)
//     ins[i, g, v]   = r'' (A_{g,v} - R'_g) + (r'' - r(nk)) T     r'' = r(nk + 1)
//         R'_g  = sum of scores over j in [max(0, g - cw + 1), min(g - 1, nk - 1)]            the windows that straddle gap g
//         A_g,v = sum of c over the mutant's windows j'' in [max(0, g - cw + 1), min(g, nk)], which hold table row v at offset g - j''
// exactly  m(mutant) - m(sequence)  for m = features . w -- not to first order.  At scaling_type 0 the T term is exactly zero and is
// not formed.
//
// One kernel template, four modes.  All of them give one workgroup of four waves to one output slot -- (sequence, window) for the
// scores, (sequence, position) for deletions and substitutions, (sequence, gap) for insertions: one protein spreads over the chip.
// The slot's windows are outermost, in ascending j: a window's token bytes are fetched ONCE through the token window policy
// (IndelTokenWindows remaps each register's position offset: no mutant is written), wave w takes the tiles b = w, w + 4, ..., holds the
// tile's float64 weight pairs in registers, and for every value v of the slot gathers the window (take, or take_subst for the variant
// with token v), runs the forward half of the gradient tile (input_grad_forward + tile_sincos: the float32 cos / sin arguments of
// xgpr_conv_token_rows_f32 bit for bit), forms the lane's part of the score in float64 in ascending register order, reduces it over the
// wave (wave_sum: a fixed tree) and adds it to the wave's own slot acc[w][v] in LDS.  No slot is shared between waves, so there are no
// atomics and the order of the additions into a slot is (j ascending, b ascending).  After the last window the four waves meet once
// and the sums are formed in the fixed order ((w0 + w1) + w2) + w3.  The substitution scan's wild type v = t[l] goes through exactly
// this path like every other v and thread v stores r (S_v - S_{t[l]}): the own token's entry is x - x = +0.0 bitwise, and two
// identical table rows give the same bits.  R_p / R'_g are read from the score array in ascending j by one thread; T is re-summed by
// every indel workgroup from the score array in an order that depends on nk alone (thread t takes j = t, t + 256, ..., then wave_sum,
// then the four waves in order): every output is a bitwise function of its own sequence, the table and the weights.  Slots past the
// sequence store 0.0 and leave before any barrier.  No second kernel, no workspace beyond the packed sign masks.
// ------------------------------------------------------------------------------------
enum { EDIT_SCORES = 0, EDIT_DEL = 1, EDIT_INS = 2, EDIT_SUBST = 3 };
// the two facts that tell the modes apart
constexpr bool edit_per_token(int mode) { return mode == EDIT_INS || mode == EDIT_SUBST; }     // a slot holds V values, not one
constexpr bool edit_reads_scores(int mode) { return mode == EDIT_DEL || mode == EDIT_INS; }    // the epilogue needs R and T

struct EditScanArgs {
    InputGradArgs ig;             // x, g, sigma unused; w = the ONE shared vector [2 F]; d = conv_width * C; scale = sqrt(1 / F)
    WaveArgs win;                 // what the token window policy reads: tokens, x = the table, vocab, row_stride = L, d, kmer_stride, conv_width, seqlen
    const double *scores;         // [n, L]: read by the deletion and insertion modes
    double *out;                  // scores [n, L], del [n, L], ins [n, L + 1, V] or subst [n, L, V]
    int L; int scaling_type;
};

__device__ __forceinline__ double indel_norm(double scale, int scaling_type, int k) {
    return scaling_type == 1 ? scale / sqrt((double)k) : scaling_type == 2 ? scale / (double)k : scale;
}

template <int LOG2P, int MODE>
__global__ __launch_bounds__(256) void conv_token_edit_scan_kernel(EditScanArgs s) {
    constexpr bool TP = LOG2P >= 7;
    constexpr bool PER_TOKEN = edit_per_token(MODE), READS = edit_reads_scores(MODE);
    __shared__ __attribute__((aligned(16))) float tab[TOK_TABLE_FLOATS + 4];
    __shared__ __attribute__((aligned(16))) float tbuf[TP ? 4 * TBUF_FLOATS : 4];
    __shared__ double acc[4][PER_TOKEN ? 256 : 1];       // acc[w][v]: wave w's sum (for token v; vocab <= 256)
    __shared__ double tot[4], rem;                       // T's four partial sums; R_p / R'_g  (READS only: otherwise neither written nor allocated)
    const InputGradArgs &a = s.ig;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int S = MODE == EDIT_INS ? s.L + 1 : s.L;      // output slots per sequence
    const long i = blockIdx.x / (unsigned)S;
    const int e = (int)(blockIdx.x - (unsigned)i * (unsigned)S);   // window j, position p / l or gap g
    const int V = s.win.vocab, cw = s.win.conv_width;
    const int len = s.win.seqlen[i];
    const int nk = len - cw + 1;
    const int no = PER_TOKEN ? V : 1;                    // values per slot
    double *orow = s.out + ((long)i * S + e) * no;
    // (both exits are uniform over the workgroup: nobody waits at a barrier below)
    if (MODE == EDIT_SCORES ? e >= nk : MODE == EDIT_INS ? e > len : e >= len) {
        for (int v = threadIdx.x; v < no; v += 256) orow[v] = 0.0;
        return;
    }
    if (MODE == EDIT_DEL && nk == 1) {                   // the mutant has no window: its features are 0 / 0
        if (threadIdx.x == 0) orow[0] = __builtin_nan("");
        return;
    }
    const int nt = V * s.win.kmer_stride;                // <= TOK_TABLE_FLOATS (edit_scan_ok)
    for (int t = threadIdx.x; t < nt; t += 256) tab[t] = s.win.x[t];
    if (threadIdx.x == 0) tab[nt] = 0.0f;
    if (PER_TOKEN || threadIdx.x == 0) {
        #pragma unroll
        for (int w = 0; w < 4; w++) acc[w][PER_TOKEN ? threadIdx.x : 0] = 0.0;
    }
    // the windows the slot transforms (those of the mutant that the edit adds), and those of the sequence that an indel removes
    int jlo = e, jhi = e;
    if constexpr (MODE != EDIT_SCORES) jlo = e - cw + 1 > 0 ? e - cw + 1 : 0;
    if constexpr (MODE == EDIT_SUBST) jhi = e < nk - 1 ? e : nk - 1;
    if constexpr (MODE == EDIT_INS) jhi = e < nk ? e : nk;
    if constexpr (MODE == EDIT_DEL) jhi = e - 1 < nk - 2 ? e - 1 : nk - 2;
    if constexpr (READS) {
        const int rhi = MODE == EDIT_INS ? (e - 1 < nk - 1 ? e - 1 : nk - 1) : (e < nk - 1 ? e : nk - 1);
        const double *srow = s.scores + i * s.L;
        if (s.scaling_type != 0) {
            double tp = 0.0;
            for (int j = threadIdx.x; j < nk; j += 256) tp += srow[j];
            tp = wave_sum(tp);
            if (lane == 0) tot[wv] = tp;
        }
        if (threadIdx.x == 0) {
            double rsum = 0.0;
            for (int j = jlo; j <= rhi; j++) rsum += srow[j];
            rem = rsum;
        }
    }
    __syncthreads();

    float *tb = tbuf + wv * (TP ? TBUF_FLOATS : 1);
    const float chs = TP ? a.chi_scale * sorf_kept_sign(lane) : a.chi_scale;     // the sign tile_sorf kept, into chi (exact)
    IndelTokenWindows<LOG2P> win;
    win.tab = reinterpret_cast<const char *>(tab);
    win.begin(s.win, i, lane);
    for (int j = jlo; j <= jhi; j++) {
        const unsigned q = (unsigned)(e - j);            // the edit's position offset inside window j
        // the window's token bytes: once per (slot, window), for all tokens and tiles
        if constexpr (MODE == EDIT_INS) win.issue_ins(j, q);
        else if constexpr (MODE == EDIT_DEL) win.issue_del(j, q);
        else win.issue(j);
        for (int bb = wv; bb < a.nb; bb += 4) {
            const int b = __builtin_amdgcn_readfirstlane(bb);
            cmask_t mk = as_cmask(a.masks + (long)b * 16);
            // the tile's weight pairs (w[0] dropped under the intercept; frequencies >= F carry no weight)
            double wc[16], ws[16];
            const long f0 = (long)b * 1024 + lane;
            #pragma unroll
            for (int r = 0; r < 16; r++) {
                const long f = f0 + r * 64;
                const bool in = f < a.F;
                const long fc = in ? f : 0;
                const double w0 = a.w[2 * fc], w1 = a.w[2 * fc + 1];
                wc[r] = (in && !(a.fit_intercept && f == 0)) ? w0 : 0.0;
                ws[r] = in ? w1 : 0.0;
            }
            for (int v = 0; v < no; v++) {
                float t[16], arg[16], sn[16], cs[16];
                if constexpr (PER_TOKEN) {
                    if constexpr (!TP) mk = launder(mk); // (the 48 sign masks are re-read per token, not held in 96 scalar registers)
                    win.take_subst(t, q, (unsigned)v);
                } else win.take(t);
                input_grad_forward<LOG2P>(t, arg, a, mk, b, chs, tb, lane);
                tile_sincos(arg, sn, cs);
                double p = 0.0;
                #pragma unroll
                for (int r = 0; r < 16; r++) {
                    p += wc[r] * (double)cs[r];
                    p += ws[r] * (double)sn[r];
                }
                const double u = wave_sum(p);
                if (lane == 0) acc[wv][v] += u;          // (this wave's slot: in order, no other wave touches it)
            }
        }
    }
    // (the tile exchanges of tile_sorf are inline assembly the compiler's wait-count pass does not see: the wait in front of the
    // cross-wave barrier is explicit -- DESIGN.md 5)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();
    if constexpr (MODE == EDIT_SCORES) {
        if (threadIdx.x == 0) orow[0] = ((acc[0][0] + acc[1][0]) + acc[2][0]) + acc[3][0];
    } else if constexpr (MODE == EDIT_SUBST) {
        const double rs = indel_norm(a.scale, s.scaling_type, nk);
        const int own = s.win.tokens[i * s.win.row_stride + e];      // e < len: inside the sequence
        const double wt = ((acc[0][own] + acc[1][own]) + acc[2][own]) + acc[3][own];
        for (int v = threadIdx.x; v < V; v += 256)
            orow[v] = rs * ((((acc[0][v] + acc[1][v]) + acc[2][v]) + acc[3][v]) - wt);
    } else {
        const double rm = indel_norm(a.scale, s.scaling_type, MODE == EDIT_INS ? nk + 1 : nk - 1);
        double shift = 0.0;                              // (r' - r) T: exactly zero without a normaliser, and not formed
        if (s.scaling_type != 0)
            shift = (rm - indel_norm(a.scale, s.scaling_type, nk)) * (((tot[0] + tot[1]) + tot[2]) + tot[3]);
        for (int v = threadIdx.x; v < no; v += 256)
            orow[v] = rm * ((((acc[0][v] + acc[1][v]) + acc[2][v]) + acc[3][v]) - rem) + shift;
    }
}

// 1: the kernel serves a window of `width` = conv_width * C elements over a table [vocab, C] (both exported predicates)
int edit_scan_ok(long width, long vocab, long C, long num_freqs) {
    return num_freqs >= 1 && conv_token_input_grad_ok_impl(width, vocab, C) ? 1 : 0;
}
int conv_token_subst_scan_ok_impl(long width, long vocab, long C, long num_freqs) { return edit_scan_ok(width, vocab, C, num_freqs); }
int conv_token_indel_scan_ok_impl(long width, long vocab, long C, long num_freqs) { return edit_scan_ok(width, vocab, C, num_freqs); }

// what the checks of the two operators do not share: the output slots per sequence (L + gaps) and the two messages that name them
struct EditScanOp { int gaps; const char *unsupported, *too_many; };
constexpr EditScanOp SUBST_OP = {0, "the substitution scan serves windows of up to 1024 elements and tables of up to 4608 floats (see xgpr_conv_token_subst_scan_ok)",
                                 "too many positions for one launch (n * L < 2^24)"};
constexpr EditScanOp INDEL_OP = {1, "the indel scan serves windows of up to 1024 elements and tables of up to 4608 floats (see xgpr_conv_token_indel_scan_ok)",
                                 "too many positions for one launch (n * (L + 1) < 2^24)"};   // (the window scores included)

// the checks of the entry points, in the documented order, in two halves (the pair scan, pair_scan.inc, has an exit of its own between
// them): the shape, down to the _ok predicate ...
int edit_scan_shape_check(const EditScanOp &op, const int32_t *seqlen_host, long n, long L, long vocab, long C, long num_freqs, long R,
                          int conv_width, int scaling_type) {
    if (n < 0 || L < 1 || C < 1) return fail(XGPR_ERR_ARRAY_DIMS, "incorrect array dims passed");
    if (scaling_type < 0 || scaling_type > 2) return fail(XGPR_ERR_ARRAY_DIMS, "scaling_type must be 0, 1 or 2");
    if (conv_width <= 0 || L < conv_width) return fail(XGPR_ERR_CONV_WIDTH, "invalid conv_width");
    const long win = (long)conv_width * C;
    const long P = padded_width(win);
    if (num_freqs < 1 || num_freqs > R || R % P != 0) return fail(XGPR_ERR_RFFS_FREQS, "incorrect number of rffs and or freqs.");
    if (n > 0) {
        int rc = check_seqlens(seqlen_host, n, n, L, conv_width);
        if (rc) return rc;
    }
    if (vocab < 1 || vocab > 256) return fail(XGPR_ERR_ARRAY_DIMS, "token table: vocab must be 1 .. 256 (uint8 tokens)");
    if (!edit_scan_ok(win, vocab, C, num_freqs)) return fail(XGPR_ERR_UNSUPPORTED, op.unsupported);
    return 0;
}
// ... and, where something will be launched, the workspace and the arrays; `bufs_ok`: every array the call needs is there; `outs_ok`: an output too
int edit_scan_buffer_check(const void *workspace, size_t wbytes, long R, bool bufs_ok, bool outs_ok) {
    if (!workspace || wbytes < masks_bytes(R)) return fail(XGPR_ERR_WORKSPACE, "workspace too small (see xgpr_rbf_workspace_bytes)");
    if (!bufs_ok) return fail(XGPR_ERR_WORKSPACE, "NULL array pointer");
    if (!outs_ok) return fail(XGPR_ERR_WORKSPACE, "NULL array pointer (del and ins are both NULL: nothing to compute)");
    return 0;
}
int edit_scan_check(const EditScanOp &op, const int32_t *seqlen_host, long n, long L, long vocab, long C, long num_freqs, long R,
                    int conv_width, int scaling_type, const void *workspace, size_t wbytes, bool bufs_ok, bool outs_ok, bool *launch) {
    *launch = false;
    int rc = edit_scan_shape_check(op, seqlen_host, n, L, vocab, C, num_freqs, R, conv_width, scaling_type);
    if (rc || n == 0) return rc;
    rc = edit_scan_buffer_check(workspace, wbytes, R, bufs_ok, outs_ok);
    if (rc) return rc;
    if (n > 2147483647L || n * (L + op.gaps) > 16777215L) return fail(XGPR_ERR_UNSUPPORTED, op.too_many);
    *launch = true;
    return 0;
}

EditScanArgs edit_scan_args(const uint8_t *tokens, const float *table, const double *w, const float *chi, const int32_t *seqlen_dev,
                            long n, long L, long vocab, long C, long num_freqs, long R, int conv_width, int scaling_type,
                            int fit_intercept, void *workspace) {
    const long win = (long)conv_width * C;
    EditScanArgs s = {};
    s.win = wave_args(table, chi, workspace, n, L, win, num_freqs, R);
    s.win.tokens = tokens; s.win.vocab = (int)vocab;
    s.win.seqlen = seqlen_dev; s.win.kmer_stride = (int)C; s.win.conv_width = conv_width;
    InputGradArgs &a = s.ig;
    a.w = w; a.masks = s.win.masks; a.chi = chi;
    a.n = n; a.w_row_stride = 0; a.F = num_freqs; a.w_cols = 2 * num_freqs;
    a.d = (int)win; a.MW = s.win.MW;
    a.nb = (int)((num_freqs + 1023) / 1024);
    a.fit_intercept = fit_intercept;
    a.nc = s.win.nc; a.chi_scale = s.win.chi_scale;
    a.scale = sqrt(1.0 / (double)num_freqs);      // the sequence kernels' constant: the same with and without the intercept
    s.L = (int)L; s.scaling_type = scaling_type;
    return s;
}

// one launch of `blocks` output slots into `out`
template <int MODE>
int edit_scan_launch(EditScanArgs s, double *out, long blocks, hipStream_t st) {
    s.out = out;
    return dispatch_lg<1, 10>(ilog2(padded_width(s.ig.d)), TOO_WIDE_WAVE, [&](auto LG) {
        return launch(conv_token_edit_scan_kernel<decltype(LG)::value, MODE>, dim3((unsigned)blocks), dim3(256), 0, st,
                      "conv_token_edit_scan_kernel launch", s);
    });
}

int subst_scan_impl(const uint8_t *tokens, const float *table, const double *w, double *out, const int8_t *radem, const float *chi,
                    const int32_t *seqlen_host, const int32_t *seqlen_dev, long n, long L, long vocab, long C, long num_freqs, long R,
                    int conv_width, int scaling_type, int fit_intercept, void *workspace, size_t wbytes, void *stream) {
    bool go;
    int rc = edit_scan_check(SUBST_OP, seqlen_host, n, L, vocab, C, num_freqs, R, conv_width, scaling_type, workspace, wbytes,
                             tokens && table && w && out && radem && chi && seqlen_dev, true, &go);
    if (rc || !go) return rc;
    hipStream_t st = (hipStream_t)stream;
    EditScanArgs s = edit_scan_args(tokens, table, w, chi, seqlen_dev, n, L, vocab, C, num_freqs, R, conv_width, scaling_type, fit_intercept,
                                    workspace);
    rc = pack_masks(radem, (uint64_t *)workspace, R, s.ig.MW, st);
    if (rc) return rc;
    return edit_scan_launch<EDIT_SUBST>(s, out, n * L, st);
}

int window_scores_impl(const uint8_t *tokens, const float *table, const double *w, double *scores, const int8_t *radem, const float *chi,
                       const int32_t *seqlen_host, const int32_t *seqlen_dev, long n, long L, long vocab, long C, long num_freqs, long R,
                       int conv_width, int fit_intercept, void *workspace, size_t wbytes, void *stream) {
    bool go;
    int rc = edit_scan_check(INDEL_OP, seqlen_host, n, L, vocab, C, num_freqs, R, conv_width, 0, workspace, wbytes,
                             tokens && table && w && scores && radem && chi && seqlen_dev, true, &go);
    if (rc || !go) return rc;
    hipStream_t st = (hipStream_t)stream;
    EditScanArgs s = edit_scan_args(tokens, table, w, chi, seqlen_dev, n, L, vocab, C, num_freqs, R, conv_width, 0, fit_intercept, workspace);
    rc = pack_masks(radem, (uint64_t *)workspace, R, s.ig.MW, st);
    if (rc) return rc;
    return edit_scan_launch<EDIT_SCORES>(s, scores, n * L, st);
}

int indel_scan_impl(const uint8_t *tokens, const float *table, const double *w, const double *scores, double *del, double *ins,
                    const int8_t *radem, const float *chi, const int32_t *seqlen_host, const int32_t *seqlen_dev, long n, long L,
                    long vocab, long C, long num_freqs, long R, int conv_width, int scaling_type, int fit_intercept, void *workspace,
                    size_t wbytes, void *stream) {
    bool go;
    int rc = edit_scan_check(INDEL_OP, seqlen_host, n, L, vocab, C, num_freqs, R, conv_width, scaling_type, workspace, wbytes,
                             tokens && table && w && scores && radem && chi && seqlen_dev, del || ins, &go);
    if (rc || !go) return rc;
    hipStream_t st = (hipStream_t)stream;
    EditScanArgs s = edit_scan_args(tokens, table, w, chi, seqlen_dev, n, L, vocab, C, num_freqs, R, conv_width, scaling_type, fit_intercept,
                                    workspace);
    s.scores = scores;
    rc = pack_masks(radem, (uint64_t *)workspace, R, s.ig.MW, st);
    if (rc) return rc;
    if (del) rc = edit_scan_launch<EDIT_DEL>(s, del, n * L, st);
    if (!rc && ins) rc = edit_scan_launch<EDIT_INS>(s, ins, n * (L + 1), st);
    return rc;
}
