// indel_scan.inc -- part of xgpr_hip.hip (included inside its anonymous namespace, after subst_scan.inc): the exact effect of every
// single-token DELETION and INSERTION on a weighted sum of the SEQUENCE and GRAPH kernels' random features
// (xgpr_conv_token_window_scores_f32, xgpr_conv_token_indel_scan_f32, include/xgpr_hip_indel_scan.h; DESIGN.md 3.21).
//
// The notation is subst_scan.inc's: sequence i has length s, nk = s - conv_width + 1 windows win_j = t[j .. j + cw), the window score is
// c(win) = sum_f (w[2f] cos p_f + w[2f+1] sin p_f) with p = W win (w[0] dropped under the intercept), r(k) = sqrt(1 / F) / {1, sqrt k, k}
// and T = sum_{j < nk} c(win_j).  An indel shifts the windows that do not touch the edit site and a shifted window has the same content,
// so with scores[i, j] = c(win_j):
//     del[i, p]    = r' (A_p - R_p)       + (r' - r(nk)) T      r'  = r(nk - 1)
//         R_p   = sum of scores over j in [max(0, p - cw + 1), min(p, nk - 1)]            the windows that cover p
//         A_p   = sum of c over the mutant's windows j' in [max(0, p - cw + 1), min(p - 1, nk - 2)], t[j' .. p) then t[p + 1 .. j' + cw + 1)
//     ins[i, g, v] = r'' (A_{g,v} - R'_g) + (r'' - r(nk)) T     r'' = r(nk + 1)
//         R'_g  = sum of scores over j in [max(0, g - cw + 1), min(g - 1, nk - 1)]        the windows that straddle gap g
//         A_g,v = sum of c over the mutant's windows j'' in [max(0, g - cw + 1), min(g, nk)], which hold table row v at offset g - j''
// exactly m(mutant) - m(sequence) for m = features . w.  At scaling_type 0 the T term is exactly zero and is not formed.
//
// One kernel template, three modes.  All of them give one workgroup of four waves to one output slot -- (sequence, window) for the
// scores, (sequence, position) for deletions, (sequence, gap) for insertions -- and share the body of conv_token_subst_scan_kernel:
// windows outermost in ascending order, a window's token bytes fetched ONCE through the token window policy (IndelTokenWindows remaps
// each register's position offset: no mutant is written), wave w takes the tiles b = w, w + 4, ..., holds the tile's float64 weight
// pairs in registers, runs input_grad_forward + tile_sincos (the float32 cos / sin arguments of xgpr_conv_token_rows_f32 bit for bit),
// sums its lanes' parts in float64 in ascending register order, then over the wave (wave_sum: a fixed tree), into the wave's own LDS
// slot; the four slots meet as ((w0 + w1) + w2) + w3.  Insertions run the token v innermost, exactly as the substitution scan does.
// R_p / R'_g are read from the score array in ascending j by one thread; T is re-summed by every scan workgroup from the score array in
// an order that depends on nk alone (thread t takes j = t, t + 256, ..., then wave_sum, then the four waves in order): every output is
// a bitwise function of its own sequence, the table and the weights.  No atomics, no workspace beyond the packed sign masks.
// ------------------------------------------------------------------------------------
enum { INDEL_SCORES = 0, INDEL_DEL = 1, INDEL_INS = 2 };

struct IndelScanArgs {
    InputGradArgs ig;             // as in SubstScanArgs
    WaveArgs win;
    const double *scores;         // [n, L]: read by the two scan modes
    double *out;                  // scores [n, L], del [n, L] or ins [n, L + 1, V]
    int L; int scaling_type;
};

__device__ __forceinline__ double indel_norm(double scale, int scaling_type, int k) {
    return scaling_type == 1 ? scale / sqrt((double)k) : scaling_type == 2 ? scale / (double)k : scale;
}

template <int LOG2P, int MODE>
__global__ __launch_bounds__(256) void conv_token_indel_scan_kernel(IndelScanArgs s) {
    constexpr bool TP = LOG2P >= 7;
    constexpr bool INS = MODE == INDEL_INS;
    __shared__ __attribute__((aligned(16))) float tab[TOK_TABLE_FLOATS + 4];
    __shared__ __attribute__((aligned(16))) float tbuf[TP ? 4 * TBUF_FLOATS : 4];
    __shared__ double acc[4][INS ? 256 : 1];             // acc[w][v]: wave w's sum (for inserted token v)
    __shared__ double tot[4], rem;                       // T's four partial sums; R_p / R'_g
    const InputGradArgs &a = s.ig;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned S = (unsigned)(INS ? s.L + 1 : s.L);  // output slots per sequence
    const long i = blockIdx.x / S;
    const int e = (int)(blockIdx.x - (unsigned)i * S);   // window j, position p or gap g
    const int V = s.win.vocab, cw = s.win.conv_width;
    const int len = s.win.seqlen[i];
    const int nk = len - cw + 1;
    const int no = INS ? V : 1;                          // values per slot
    double *orow = s.out + ((long)i * S + e) * no;
    // (both exits are uniform over the workgroup: nobody waits at a barrier below)
    if (MODE == INDEL_SCORES ? e >= nk : MODE == INDEL_DEL ? e >= len : e > len) {
        for (int v = threadIdx.x; v < no; v += 256) orow[v] = 0.0;
        return;
    }
    if (MODE == INDEL_DEL && nk == 1) {                  // the mutant has no window: its features are 0 / 0
        if (threadIdx.x == 0) orow[0] = __builtin_nan("");
        return;
    }
    const int nt = V * s.win.kmer_stride;                // <= TOK_TABLE_FLOATS (conv_token_indel_scan_ok)
    for (int t = threadIdx.x; t < nt; t += 256) tab[t] = s.win.x[t];
    if (threadIdx.x == 0) tab[nt] = 0.0f;
    if (INS || threadIdx.x == 0) {
        #pragma unroll
        for (int w = 0; w < 4; w++) acc[w][INS ? threadIdx.x : 0] = 0.0;
    }
    // the windows of the sequence that the edit removes, and those of the mutant that it adds
    int jlo = e, jhi = e, rhi = e;
    if constexpr (MODE != INDEL_SCORES) {
        jlo = e - cw + 1 > 0 ? e - cw + 1 : 0;
        if constexpr (INS) { jhi = e < nk ? e : nk; rhi = e - 1 < nk - 1 ? e - 1 : nk - 1; }
        else { jhi = e - 1 < nk - 2 ? e - 1 : nk - 2; rhi = e < nk - 1 ? e : nk - 1; }
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
        const unsigned q = (unsigned)(e - j);            // the edit's position offset inside mutant window j
        if constexpr (MODE == INDEL_SCORES) win.issue(j);
        else if constexpr (INS) win.issue_ins(j, q);     // the window's token bytes: once per (gap, window), for all tokens and tiles
        else win.issue_del(j, q);
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
                if constexpr (INS) {
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
    if constexpr (MODE == INDEL_SCORES) {
        if (threadIdx.x == 0) orow[0] = ((acc[0][0] + acc[1][0]) + acc[2][0]) + acc[3][0];
    } else {
        const double rm = indel_norm(a.scale, s.scaling_type, INS ? nk + 1 : nk - 1);
        double shift = 0.0;                              // (r' - r) T: exactly zero without a normaliser, and not formed
        if (s.scaling_type != 0)
            shift = (rm - indel_norm(a.scale, s.scaling_type, nk)) * (((tot[0] + tot[1]) + tot[2]) + tot[3]);
        for (int v = threadIdx.x; v < no; v += 256)
            orow[v] = rm * ((((acc[0][v] + acc[1][v]) + acc[2][v]) + acc[3][v]) - rem) + shift;
    }
}

// 1: the kernels serve a window of `width` = conv_width * C elements over a table [vocab, C] (the substitution scan's condition)
int conv_token_indel_scan_ok_impl(long width, long vocab, long C, long num_freqs) {
    return conv_token_subst_scan_ok_impl(width, vocab, C, num_freqs);
}

// the checks the two entry points share, in subst_scan_impl's order; `bufs_ok`: every array the call needs is there
int indel_check(const int32_t *seqlen_host, long n, long L, long vocab, long C, long num_freqs, long R, int conv_width, int scaling_type,
                const void *workspace, size_t wbytes, bool bufs_ok, bool outs_ok, bool *launch) {
    *launch = false;
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
    if (!conv_token_indel_scan_ok_impl(win, vocab, C, num_freqs))
        return fail(XGPR_ERR_UNSUPPORTED, "the indel scan serves windows of up to 1024 elements and tables of up to 4608 floats (see xgpr_conv_token_indel_scan_ok)");
    if (n == 0) return 0;
    if (!workspace || wbytes < masks_bytes(R)) return fail(XGPR_ERR_WORKSPACE, "workspace too small (see xgpr_rbf_workspace_bytes)");
    if (!bufs_ok) return fail(XGPR_ERR_WORKSPACE, "NULL array pointer");
    if (!outs_ok) return fail(XGPR_ERR_WORKSPACE, "NULL array pointer (del and ins are both NULL: nothing to compute)");
    if (n > 2147483647L || n * (L + 1) > 16777215L) return fail(XGPR_ERR_UNSUPPORTED, "too many positions for one launch (n * (L + 1) < 2^24)");
    *launch = true;
    return 0;
}

IndelScanArgs indel_args(const uint8_t *tokens, const float *table, const double *w, const float *chi, const int32_t *seqlen_dev, long n,
                         long L, long vocab, long C, long num_freqs, long R, int conv_width, int scaling_type, int fit_intercept,
                         void *workspace) {
    const long win = (long)conv_width * C;
    IndelScanArgs s = {};
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

template <int MODE>
int indel_launch(const IndelScanArgs &s, long blocks, long P, hipStream_t st) {
    return dispatch_lg<1, 10>(ilog2(P), TOO_WIDE_WAVE, [&](auto LG) {
        return launch(conv_token_indel_scan_kernel<decltype(LG)::value, MODE>, dim3((unsigned)blocks), dim3(256), 0, st,
                      "conv_token_indel_scan_kernel launch", s);
    });
}

int window_scores_impl(const uint8_t *tokens, const float *table, const double *w, double *scores, const int8_t *radem, const float *chi,
                       const int32_t *seqlen_host, const int32_t *seqlen_dev, long n, long L, long vocab, long C, long num_freqs, long R,
                       int conv_width, int fit_intercept, void *workspace, size_t wbytes, void *stream) {
    bool go;
    int rc = indel_check(seqlen_host, n, L, vocab, C, num_freqs, R, conv_width, 0, workspace, wbytes,
                         tokens && table && w && scores && radem && chi && seqlen_dev, true, &go);
    if (rc || !go) return rc;
    hipStream_t st = (hipStream_t)stream;
    IndelScanArgs s = indel_args(tokens, table, w, chi, seqlen_dev, n, L, vocab, C, num_freqs, R, conv_width, 0, fit_intercept, workspace);
    s.out = scores;
    rc = pack_masks(radem, (uint64_t *)workspace, R, s.ig.MW, st);
    if (rc) return rc;
    return indel_launch<INDEL_SCORES>(s, n * L, padded_width((long)conv_width * C), st);
}

int indel_scan_impl(const uint8_t *tokens, const float *table, const double *w, const double *scores, double *del, double *ins,
                    const int8_t *radem, const float *chi, const int32_t *seqlen_host, const int32_t *seqlen_dev, long n, long L,
                    long vocab, long C, long num_freqs, long R, int conv_width, int scaling_type, int fit_intercept, void *workspace,
                    size_t wbytes, void *stream) {
    bool go;
    int rc = indel_check(seqlen_host, n, L, vocab, C, num_freqs, R, conv_width, scaling_type, workspace, wbytes,
                         tokens && table && w && scores && radem && chi && seqlen_dev, del || ins, &go);
    if (rc || !go) return rc;
    hipStream_t st = (hipStream_t)stream;
    IndelScanArgs s = indel_args(tokens, table, w, chi, seqlen_dev, n, L, vocab, C, num_freqs, R, conv_width, scaling_type, fit_intercept,
                                 workspace);
    s.scores = scores;
    rc = pack_masks(radem, (uint64_t *)workspace, R, s.ig.MW, st);
    if (rc) return rc;
    const long P = padded_width((long)conv_width * C);
    if (del) {
        s.out = del;
        rc = indel_launch<INDEL_DEL>(s, n * L, P, st);
        if (rc) return rc;
    }
    if (ins) {
        s.out = ins;
        rc = indel_launch<INDEL_INS>(s, n * (L + 1), P, st);
    }
    return rc;
}
