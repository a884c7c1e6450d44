// seq_input_grad.inc -- part of xgpr_hip.hip (included inside its anonymous namespace, after input_grad.inc): the input gradient of a
// weighted sum of the SEQUENCE and GRAPH kernels' random features, per position and channel (xgpr_conv_input_grad_f32 /
// xgpr_conv_token_input_grad_f32, include/xgpr_hip_seq_input_grad.h; DESIGN.md 3.17).
//
// A sequence x[L, C] (already multiplied by sigma) of length s has nk = s - conv_width + 1 k-mers; window j is x[j : j + conv_width, :]
// flattened (d = conv_width C elements).  With p_j = W win_j and the feature constant r = sqrt(1 / F) / {1, sqrt(nk), nk} the sum
// m = sum_col w[col] z[col] over the feature row of xgpr_conv_feature_rows_f32 has
//     d m / d x[l, c] = sigma  sum_{j = max(0, l - conv_width + 1)}^{min(l, nk - 1)}  (W^T u_j)[(l - j) C + c],
//     u_{j,f} = r (w[2f+1] cos p_{j,f} - w[2f] sin p_{j,f})
// with W^T the transposed SORF of input_grad.inc: every window is one row of that kernel, and the windows' gradients overlap-add.
//
// One workgroup of four waves per sequence, k-mers outermost.  Per k-mer j wave w takes the tiles b = w, w + 4, ... through
// input_grad_tile (input_grad.inc: forward, middle, three backward rounds), adds the results to sixteen float64 partials, folds them
// over the repetitions of a tile, and the four waves meet in LDS, where the sums are formed in the fixed order ((w0 + w1) + w2) + w3.
// The thread that owns window element e = q C + c adds that sum to slot ((j + q) mod conv_width) C + c of a ring of conv_width C
// doubles: position j + q, channel c.  Position j has then received its last window (windows arrive in ascending j): the q = 0 threads
// store sigma times the finished sum to g[i, j, :] and clear the slot for position j + conv_width.  After the last k-mer the
// conv_width - 1 positions nk .. s - 1 still in the ring are stored and positions >= s are written as 0.0: g is OVERWRITTEN as a
// whole, there are no atomics, and a sequence's result depends on that sequence alone.  With nk < conv_width the ring never wraps.
// The window of k-mer j + 1 is fetched while k-mer j is transformed, through the window policies of the feature operators
// (DenseWindows / TokenWindows, wave_kernels.inc): token input differs from dense input in where a window's floats come from, and in
// nothing else -- the two forms agree bit for bit.
// ------------------------------------------------------------------------------------
struct SeqInputGradArgs {
    InputGradArgs ig;             // x unused; d = conv_width * C; g = the [n, L, C] output; scale = sqrt(1 / F)
    WaveArgs win;                 // what the window policies read: x or (tokens, table, vocab), row_stride, d, kmer_stride, conv_width, seqlen
    int L; int scaling_type;
};

// What a tile contributes for k-mer j is a policy of the overlap-add body below (TILE): operator()(v, &cur, j, b, tb, lane) leaves the
// tile's part of W^T u_j in v (layout C) and returns false where the tile adds nothing for this k-mer (wave-uniform).  SeqGradTile is
// the sequence kernels' tile, input_grad_tile on the held window; the max-pool backward (pool_input_grad.inc) brings its own.
template <int LOG2P> struct SeqGradTile {
    static constexpr bool WINDOWS = true;               // the tile reads the k-mer windows
    const InputGradArgs &a; const double *wrow; double rs; float chs;
    template <class WIN>
    __device__ __forceinline__ bool operator()(float (&v)[16], const WIN *cur, int, int b, float *tb, int lane) const {
        cur->take(v);
        input_grad_tile<LOG2P>(v, a, wrow, rs, b, chs, tb, lane);
        return true;
    }
};

// The k-mer loop, the cross-wave meeting, the ring and the stores of one sequence (blockIdx.x), for any TILE.
template <int LOG2P, class WIN, class TILE>
__device__ __forceinline__ void seq_overlap_add_body(const SeqInputGradArgs &s, WIN &win, const TILE &tile, float *tb) {
    constexpr int P = 1 << LOG2P;
    constexpr int RP = P >= 64 ? P / 64 : 1;            // registers that hold distinct window elements (layout C)
    constexpr int RED = P >= 64 ? P : 64;
    constexpr int NE = (P + 255) / 256;                 // window elements per thread in the overlap-add
    const InputGradArgs &a = s.ig;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long i = blockIdx.x;
    __shared__ double red[4][RED];
    __shared__ double ring[RED];
    const int C = s.win.kmer_stride, cw = s.win.conv_width, d = a.d;
    const int len = s.win.seqlen[i];
    const int nk = len - cw + 1;
    double *grow = a.g + i * (long)s.L * C;

    // window element e = threadIdx.x + 256 k of this thread: position offset q, channel c (no division in the k-mer loop)
    int eq[NE], ec[NE];
    #pragma unroll
    for (int k = 0; k < NE; k++) {
        const int e = (int)threadIdx.x + 256 * k;
        eq[k] = e / C; ec[k] = e - eq[k] * C;
        if (e < d) ring[e] = 0.0;      // (ordered before the first add by the barrier in front of it)
    }

    if constexpr (TILE::WINDOWS) {
        win.begin(s.win, i, lane);
        win.issue(0);
    }
    int jm = 0;                                          // j mod conv_width
    for (int j = 0; j < nk; j++) {
        double acc[16];
        #pragma unroll
        for (int r = 0; r < 16; r++) acc[r] = 0.0;
        auto owned_tiles = [&](const WIN *cur) {
            for (int bb = wv; bb < a.nb; bb += 4) {
                const int b = __builtin_amdgcn_readfirstlane(bb);
                float v[16];
                if (!tile(v, cur, j, b, tb, lane)) continue;
                #pragma unroll
                for (int r = 0; r < 16; r++) acc[r] += (double)v[r];
            }
        };
        if constexpr (TILE::WINDOWS) {
            WIN cur = win;                               // window j; the next one is fetched under this one's transforms
            win.issue(j + 1 < nk ? j + 1 : j);
            owned_tiles(&cur);
        } else owned_tiles(nullptr);                     // (a tile that reads no window is handed none)
        // ---- the repetitions of a tile: element e of the tile is window element e mod P
        #pragma unroll
        for (int r = RP; r < 16; r++) acc[r & (RP - 1)] += acc[r];
        if constexpr (P < 64) {
            #pragma unroll
            for (int off = P; off < 64; off <<= 1) acc[0] += __shfl_xor(acc[0], off, 64);
            if (lane < P) red[wv][lane] = acc[0];
        } else {
            #pragma unroll
            for (int r = 0; r < RP; r++) red[wv][64 * r + lane] = acc[r];
        }
        // (the tile exchanges of tile_sorf are inline assembly the compiler's wait-count pass does not see: the wait in front of the
        // cross-wave barrier is explicit -- DESIGN.md 5)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __syncthreads();
        // ---- overlap-add: every ring slot belongs to exactly one thread per k-mer
        #pragma unroll
        for (int k = 0; k < NE; k++) {
            const int e = (int)threadIdx.x + 256 * k;
            if (e < d) {
                int p = jm + eq[k];
                p = p >= cw ? p - cw : p;
                const int slot = p * C + ec[k];
                double t = ring[slot] + (((red[0][e] + red[1][e]) + red[2][e]) + red[3][e]);
                if (eq[k] == 0) { grow[(long)j * C + ec[k]] = t * a.sigma; t = 0.0; }      // position j is complete
                ring[slot] = t;
            }
        }
        jm = jm + 1 == cw ? 0 : jm + 1;
        __syncthreads();      // red is rewritten by the next k-mer
    }
    // ---- positions nk .. len - 1 are still in the ring; past the length the gradient is exactly zero
    for (int e = threadIdx.x; e < (s.L - nk) * C; e += 256) {
        const int q = e / C, c = e - q * C, l = nk + q;
        grow[(long)l * C + c] = l < len ? ring[(l % cw) * C + c] * a.sigma : 0.0;
    }
}

template <int LOG2P, class WIN>
__device__ __forceinline__ void seq_input_grad_body(const SeqInputGradArgs &s, WIN &win) {
    constexpr bool TP = LOG2P >= 7;
    __shared__ __attribute__((aligned(16))) float tbuf[TP ? 4 * TBUF_FLOATS : 4];
    float *tb = tbuf + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) * (TP ? TBUF_FLOATS : 1);
    const InputGradArgs &a = s.ig;
    const int lane = threadIdx.x & 63;
    const long i = blockIdx.x;
    const int nk = s.win.seqlen[i] - s.win.conv_width + 1;
    const float chs = TP ? a.chi_scale * sorf_kept_sign(lane) : a.chi_scale;     // the sign tile_sorf kept, into chi (exact)
    double rs = a.scale;
    if (s.scaling_type == 1) rs = a.scale / sqrt((double)nk);
    else if (s.scaling_type == 2) rs = a.scale / (double)nk;
    const SeqGradTile<LOG2P> tile = {a, a.w + i * a.w_row_stride, rs, chs};
    seq_overlap_add_body<LOG2P>(s, win, tile, tb);
}

template <int LOG2P>
__global__ __launch_bounds__(256) void conv_input_grad_kernel(SeqInputGradArgs s) {
    DenseWindows<LOG2P> win;
    seq_input_grad_body<LOG2P>(s, win);
}

// the token form: s.win.x is the table [vocab, C] (sigma-scaled), copied into LDS with one 0.0f behind it as in wave_conv_tok_kernel
template <int LOG2P>
__global__ __launch_bounds__(256) void conv_token_input_grad_kernel(SeqInputGradArgs s) {
    __shared__ __attribute__((aligned(16))) float tab[TOK_TABLE_FLOATS + 4];
    const int nt = s.win.vocab * s.win.kmer_stride;     // <= TOK_TABLE_FLOATS (conv_token_input_grad_ok)
    for (int t = threadIdx.x; t < nt; t += 256) tab[t] = s.win.x[t];
    if (threadIdx.x == 0) tab[nt] = 0.0f;
    __syncthreads();
    TokenWindows<LOG2P> win;
    win.tab = reinterpret_cast<const char *>(tab);
    seq_input_grad_body<LOG2P>(s, win);
}

// 1: the kernel serves a window of `width` = conv_width * C elements
int conv_input_grad_ok_impl(long width, long num_freqs) {
    return width >= 1 && num_freqs >= 1 && padded_width(width) <= 1024 ? 1 : 0;
}
int conv_token_input_grad_ok_impl(long width, long vocab, long C) {
    return conv_input_grad_ok_impl(width, 1) && conv_token_rows_ok(width, vocab, C) ? 1 : 0;
}

// Both entry points: the dense form reads x [n, L, C]; in the token form x is the table [vocab, C] and tokens [n, L] index its rows.
int seq_input_grad_impl(const uint8_t *tokens, bool token_form, const float *x, const double *w, double *g, const int8_t *radem,
                        const float *chi, const int32_t *seqlen_host, const int32_t *seqlen_dev, long n, long L, long vocab, long C,
                        long w_row_stride, long w_cols, long num_freqs, long R, double sigma, int conv_width, int scaling_type,
                        int fit_intercept, void *workspace, size_t wbytes, void *stream) {
    if (n < 0 || L < 1 || C < 1) return fail(XGPR_ERR_ARRAY_DIMS, "incorrect array dims passed");
    if (scaling_type < 0 || scaling_type > 2) return fail(XGPR_ERR_ARRAY_DIMS, "scaling_type must be 0, 1 or 2");
    if (conv_width <= 0 || L < conv_width) return fail(XGPR_ERR_CONV_WIDTH, "invalid conv_width");
    const long win = (long)conv_width * C;
    const long P = padded_width(win);
    if (num_freqs < 1 || num_freqs > R || R % P != 0) return fail(XGPR_ERR_RFFS_FREQS, "incorrect number of rffs and or freqs.");
    if (w_cols < 2 || (w_cols & 1) != 0) return fail(XGPR_ERR_ODD_OUTPUT, "w_cols must be an even number >= 2");
    if (w_cols > 2 * num_freqs) return fail(XGPR_ERR_ARRAY_SIZES, "w_cols exceeds the number of features");
    if (w_row_stride != 0 && w_row_stride < w_cols) return fail(XGPR_ERR_ARRAY_SIZES, "w_row_stride is shorter than w_cols");
    if (n > 0) {
        int rc = check_seqlens(seqlen_host, n, n, L, conv_width);
        if (rc) return rc;
    }
    if (token_form) {
        if (vocab < 1 || vocab > 256) return fail(XGPR_ERR_ARRAY_DIMS, "token table: vocab must be 1 .. 256 (uint8 tokens)");
        if (!conv_token_input_grad_ok_impl(win, vocab, C))
            return fail(XGPR_ERR_UNSUPPORTED, "token input serves windows of up to 1024 elements and tables of up to 4608 floats (see xgpr_conv_token_input_grad_ok)");
    } else if (!conv_input_grad_ok_impl(win, num_freqs)) return fail(XGPR_ERR_UNSUPPORTED, TOO_WIDE_WAVE);
    if (n == 0) return 0;
    if (!workspace || wbytes < masks_bytes(R)) return fail(XGPR_ERR_WORKSPACE, "workspace too small (see xgpr_rbf_workspace_bytes)");
    if (!x || !w || !g || !radem || !chi || !seqlen_dev || (token_form && !tokens)) return fail(XGPR_ERR_WORKSPACE, "NULL array pointer");
    if (n > 2147483647L || L * C > 2147483647L) return fail(XGPR_ERR_UNSUPPORTED, "too many datapoints for one launch");
    hipStream_t st = (hipStream_t)stream;
    const int lg = ilog2(P);
    SeqInputGradArgs s = {};
    s.win = wave_args(x, chi, workspace, n, token_form ? L : L * C, win, num_freqs, R);
    s.win.tokens = tokens; s.win.vocab = (int)vocab;
    s.win.seqlen = seqlen_dev; s.win.kmer_stride = (int)C; s.win.conv_width = conv_width;
    InputGradArgs &a = s.ig;
    a.w = w; a.g = g; a.masks = s.win.masks; a.chi = chi;
    a.n = n; a.w_row_stride = w_row_stride; a.F = num_freqs; a.w_cols = w_cols;
    a.d = (int)win; a.MW = s.win.MW;
    const long live = w_cols / 2 < num_freqs ? w_cols / 2 : num_freqs;
    a.nb = (int)((live + 1023) / 1024);
    a.fit_intercept = fit_intercept;
    a.nc = s.win.nc; a.chi_scale = s.win.chi_scale;
    a.scale = sqrt(1.0 / (double)num_freqs);      // the sequence kernels' constant: the same with and without the intercept
    a.sigma = sigma;
    s.L = (int)L; s.scaling_type = scaling_type;
    int rc = pack_masks(radem, (uint64_t *)workspace, R, a.MW, st);
    if (rc) return rc;
    return dispatch_lg<1, 10>(lg, TOO_WIDE_WAVE, [&](auto LG) {
        if (token_form)
            return launch(conv_token_input_grad_kernel<decltype(LG)::value>, dim3((unsigned)n), dim3(256), 0, st,
                          "conv_token_input_grad_kernel launch", s);
        return launch(conv_input_grad_kernel<decltype(LG)::value>, dim3((unsigned)n), dim3(256), 0, st, "conv_input_grad_kernel launch", s);
    });
}
