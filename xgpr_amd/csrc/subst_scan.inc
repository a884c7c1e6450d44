// subst_scan.inc -- part of xgpr_hip.hip (included inside its anonymous namespace, after seq_input_grad.inc): the exact effect of every
// single-token substitution on a weighted sum of the SEQUENCE and GRAPH kernels' random features (xgpr_conv_token_subst_scan_f32,
// include/xgpr_hip_subst_scan.h; DESIGN.md 3.20).
//
// Sequence i has length s, nk = s - conv_width + 1 k-mer windows and tokens t[0 .. s); the table [V, C] is already multiplied by sigma.
// A window win with projections p = W win scores  c(win) = sum_f (w[2f] cos p_f + w[2f+1] sin p_f)  (w[0] dropped under the intercept).
// A substitution at position l changes only the windows J(l) = { j : max(0, l - conv_width + 1) <= j <= min(l, nk - 1) }, and the k-mer
// normaliser depends on the length alone, so with r = sqrt(1 / F) / {1, sqrt(nk), nk}
//     out[i, l, v] = r ( sum_{j in J(l)} c(win_j with the token at offset l - j replaced by v)  -  the same sum at v = t[l] )
// is  m(sequence with t[l] := v) - m(sequence)  for m = features . w, exactly -- not to first order.
//
// One workgroup of four waves per (sequence, position): one protein spreads over the chip.  The covering windows are outermost, in
// ascending j: the window's token bytes are fetched ONCE through the token window policy (SubstTokenWindows::issue), wave w takes the
// tiles b = w, w + 4, ..., holds the tile's float64 weight pairs in registers, and for every v = 0 .. V - 1 gathers the variant window
// (take_subst), runs the forward half of the gradient tile (input_grad_forward + tile_sincos: the float32 cos / sin arguments of
// xgpr_conv_token_rows_f32 bit for bit), forms the lane's part of the score in float64 in ascending register order, reduces it over the
// wave (wave_sum: a fixed tree) and adds it to the wave's own slot acc[w][v] in LDS.  No slot is shared between waves, so there are no
// atomics and the order of the additions into a slot is (j ascending, b ascending).  The wild type v = t[l] goes through exactly this
// path like every other v.  After the last window the four waves meet once, the sums are formed in the fixed order
// ((w0 + w1) + w2) + w3, and thread v stores r (S_v - S_{t[l]}): the own token's entry is x - x = +0.0 bitwise, and two identical table
// rows give the same bits.  Positions l >= s store 0.0 and leave before any barrier.  No second kernel, no workspace beyond the
// packed sign masks.
// ------------------------------------------------------------------------------------
struct SubstScanArgs {
    InputGradArgs ig;             // x, g, sigma unused; w = the ONE shared vector [2 F]; d = conv_width * C; scale = sqrt(1 / F)
    WaveArgs win;                 // what the token window policy reads: tokens, x = the table, vocab, row_stride = L, d, kmer_stride, conv_width, seqlen
    double *out;                  // [n, L, V]
    int L; int scaling_type;
};

template <int LOG2P>
__global__ __launch_bounds__(256) void conv_token_subst_scan_kernel(SubstScanArgs s) {
    constexpr bool TP = LOG2P >= 7;
    __shared__ __attribute__((aligned(16))) float tab[TOK_TABLE_FLOATS + 4];
    __shared__ __attribute__((aligned(16))) float tbuf[TP ? 4 * TBUF_FLOATS : 4];
    __shared__ double acc[4][256];                       // acc[w][v]: wave w's sum for token v (vocab <= 256)
    const InputGradArgs &a = s.ig;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long i = blockIdx.x / (unsigned)s.L;
    const int l = (int)(blockIdx.x - (unsigned)i * (unsigned)s.L);
    const int V = s.win.vocab, cw = s.win.conv_width;
    const int len = s.win.seqlen[i];
    double *orow = s.out + ((long)i * s.L + l) * V;
    if (l >= len) {                                      // (uniform over the workgroup: nobody waits at a barrier below)
        for (int v = threadIdx.x; v < V; v += 256) orow[v] = 0.0;
        return;
    }
    const int nt = V * s.win.kmer_stride;                // <= TOK_TABLE_FLOATS (conv_token_subst_scan_ok)
    for (int t = threadIdx.x; t < nt; t += 256) tab[t] = s.win.x[t];
    if (threadIdx.x == 0) tab[nt] = 0.0f;
    #pragma unroll
    for (int w = 0; w < 4; w++) acc[w][threadIdx.x] = 0.0;
    __syncthreads();

    float *tb = tbuf + wv * (TP ? TBUF_FLOATS : 1);
    const float chs = TP ? a.chi_scale * sorf_kept_sign(lane) : a.chi_scale;     // the sign tile_sorf kept, into chi (exact)
    const int nk = len - cw + 1;
    const int jlo = l - cw + 1 > 0 ? l - cw + 1 : 0, jhi = l < nk - 1 ? l : nk - 1;
    SubstTokenWindows<LOG2P> win;
    win.tab = reinterpret_cast<const char *>(tab);
    win.begin(s.win, i, lane);
    for (int j = jlo; j <= jhi; j++) {
        win.issue(j);                                    // the window's token bytes: once per (l, j), for all variants and tiles
        const unsigned q = (unsigned)(l - j);
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
            for (int v = 0; v < V; v++) {
                float t[16], arg[16], sn[16], cs[16];
                if constexpr (!TP) mk = launder(mk);     // (the 48 sign masks are re-read per variant, not held in 96 scalar registers)
                win.take_subst(t, q, (unsigned)v);
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
    double rs = a.scale;
    if (s.scaling_type == 1) rs = a.scale / sqrt((double)nk);
    else if (s.scaling_type == 2) rs = a.scale / (double)nk;
    const int own = s.win.tokens[i * s.win.row_stride + l];      // l < len: inside the sequence
    const double wt = ((acc[0][own] + acc[1][own]) + acc[2][own]) + acc[3][own];
    for (int v = threadIdx.x; v < V; v += 256)
        orow[v] = rs * ((((acc[0][v] + acc[1][v]) + acc[2][v]) + acc[3][v]) - wt);
}

// 1: the kernel serves a window of `width` = conv_width * C elements over a table [vocab, C]
int conv_token_subst_scan_ok_impl(long width, long vocab, long C, long num_freqs) {
    return num_freqs >= 1 && conv_token_input_grad_ok_impl(width, vocab, C) ? 1 : 0;
}

int subst_scan_impl(const uint8_t *tokens, const float *table, const double *w, double *out, const int8_t *radem, const float *chi,
                    const int32_t *seqlen_host, const int32_t *seqlen_dev, long n, long L, long vocab, long C, long num_freqs, long R,
                    int conv_width, int scaling_type, int fit_intercept, void *workspace, size_t wbytes, void *stream) {
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
    if (!conv_token_subst_scan_ok_impl(win, vocab, C, num_freqs))
        return fail(XGPR_ERR_UNSUPPORTED, "the substitution scan serves windows of up to 1024 elements and tables of up to 4608 floats (see xgpr_conv_token_subst_scan_ok)");
    if (n == 0) return 0;
    if (!workspace || wbytes < masks_bytes(R)) return fail(XGPR_ERR_WORKSPACE, "workspace too small (see xgpr_rbf_workspace_bytes)");
    if (!tokens || !table || !w || !out || !radem || !chi || !seqlen_dev) return fail(XGPR_ERR_WORKSPACE, "NULL array pointer");
    if (n > 2147483647L || n * L > 16777215L) return fail(XGPR_ERR_UNSUPPORTED, "too many positions for one launch (n * L < 2^24)");
    hipStream_t st = (hipStream_t)stream;
    const int lg = ilog2(P);
    SubstScanArgs s = {};
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
    s.out = out; s.L = (int)L; s.scaling_type = scaling_type;
    int rc = pack_masks(radem, (uint64_t *)workspace, R, a.MW, st);
    if (rc) return rc;
    return dispatch_lg<1, 10>(lg, TOO_WIDE_WAVE, [&](auto LG) {
        return launch(conv_token_subst_scan_kernel<decltype(LG)::value>, dim3((unsigned)(n * L)), dim3(256), 0, st,
                      "conv_token_subst_scan_kernel launch", s);
    });
}
