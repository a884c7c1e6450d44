// pool_input_grad.inc -- part of xgpr_hip.hip (included inside its anonymous namespace, after seq_input_grad.inc): the backward of the
// two-layer kernel's FIRST layer, the random convolution filters under ReLU and max-pool (xgpr_conv_maxpool_input_grad_f32 /
// xgpr_conv_token_maxpool_input_grad_f32, include/xgpr_hip_pool_input_grad.h; DESIGN.md 3.18).
//
// A sequence x[L, C] (unscaled) of length s has nk = s - conv_width + 1 k-mers; with p_{j,f} = chi_f SORF(win_j)_f the pooled value is
// q_f = max(0, max_j p_{j,f}), as xgpr_conv1d_maxpool_f32 writes it into a zeroed row.  For g_f = d m / d q_f of any scalar m
//     a_f = the FIRST j with p_{j,f} = max_j' p_{j',f} if that maximum is > 0, else -1 (ReLU inactive),
//     d m / d x[l, c] = sum_{j = max(0, l - conv_width + 1)}^{min(l, nk - 1)} (W^T u_j)[(l - j) C + c],   u_{j,f} = g_f [a_f == j]
// with W^T the transposed SORF of input_grad.inc.  One workgroup of four waves per sequence, two passes in one launch:
//   pass 1 (argmax)    tiles outermost: wave w takes the tiles b = w, w + 4, ... and per tile walks the k-mers through input_grad_forward
//                      -- tile_sorf and p = v (chi chs), the max-pool operator's values bit for bit -- with a running maximum that starts
//                      at 0 and moves on a strict >: the first k-mer wins a tie and a maximum <= 0 leaves -1.  One tile's 16 + 16
//                      registers are live whatever the number of filters.  The wave writes a_f to argmax[i, :].
//   pass 2 (backward)  seq_overlap_add_body (seq_input_grad.inc) with PoolGradTile: k-mers outermost; per owned tile
//                      t_f = (float)g_f (chi_f x the folded normaliser) where a_f == j and 0 elsewhere, then input_grad_backward, the
//                      float64 partials, the fold over repetitions, the ((w0 + w1) + w2) + w3 meeting, the ring and the stores -- the
//                      sequence kernels' own, with sigma = 1.  A tile without a hit for k-mer j is skipped on a wave-uniform test.
// Every lane reads back in pass 2 exactly the argmax entries it wrote in pass 1 (tile b, register r, lane l is filter 1024 b + 64 r + l
// in both); the fence and workgroup barrier between the passes make the hand-off visible to the whole workgroup all the same.
// No atomics; out and argmax are OVERWRITTEN as a whole; a sequence's result depends on that sequence alone.
// ------------------------------------------------------------------------------------
struct PoolInputGradArgs {
    SeqInputGradArgs s;           // ig.w = g [n, >= F] float64 (w_row_stride 0: one shared vector), ig.g = out, ig.sigma = 1, scaling_type 0
    int32_t *argmax;              // [n, F]
};

template <int LOG2P> struct PoolGradTile {
    static constexpr bool WINDOWS = false;              // the backward pass reads argmax, not the windows
    const InputGradArgs &a; const double *grow; const int32_t *arow;
    template <class WIN>
    __device__ __forceinline__ bool operator()(float (&v)[16], const WIN *, int j, int b, float *, int lane) const {
        const long f0 = (long)b * 1024 + lane;
        unsigned hits = 0;                              // bit r: register r's filter was won by k-mer j
        #pragma unroll
        for (int r = 0; r < 16; r++) {
            const long f = f0 + r * 64;
            if (f < a.F && arow[f < a.F ? f : 0] == j) hits |= 1u << r;
        }
        if (__builtin_amdgcn_ballot_w64(hits != 0) == 0) return false;      // the transform of zeros adds nothing
        #pragma unroll
        for (int r = 0; r < 16; r++) {
            const bool hit = (hits >> r) & 1u;
            const long fc = hit ? f0 + r * 64 : 0;
            const float t = (float)grow[fc] * (a.chi[fc] * a.chi_scale);      // g rounded once
            v[r] = hit ? t : 0.0f;                      // (a NaN or infinity in an unused g does not reach the transform)
        }
        input_grad_backward<LOG2P>(v, as_cmask(a.masks + (long)b * 16), a.MW, a.nc, lane);
        return true;
    }
};

template <int LOG2P, class WIN>
__device__ __forceinline__ void pool_input_grad_body(const PoolInputGradArgs &p, WIN &win) {
    constexpr bool TP = LOG2P >= 7;
    __shared__ __attribute__((aligned(16))) float tbuf[TP ? 4 * TBUF_FLOATS : 4];
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float *tb = tbuf + wv * (TP ? TBUF_FLOATS : 1);
    const SeqInputGradArgs &s = p.s;
    const InputGradArgs &a = s.ig;
    const int lane = threadIdx.x & 63;
    const long i = blockIdx.x;
    const int nk = s.win.seqlen[i] - s.win.conv_width + 1;
    const float chs = TP ? a.chi_scale * sorf_kept_sign(lane) : a.chi_scale;     // the sign tile_sorf kept, into chi (exact)
    int32_t *arow = p.argmax + i * a.F;

    // ---- pass 1: per owned tile the running maximum over the k-mers and the first k-mer that attains it
    win.begin(s.win, i, lane);
    for (int bb = wv; bb < a.nb; bb += 4) {
        const int b = __builtin_amdgcn_readfirstlane(bb);
        float best[16]; int at[16];
        #pragma unroll
        for (int r = 0; r < 16; r++) { best[r] = 0.0f; at[r] = -1; }
        cmask_t mk = as_cmask(a.masks + (long)b * 16);
        win.issue(0);
        for (int j = 0; j < nk; j++) {
            mk = launder(mk);                           // (the masks are re-read per k-mer, not hoisted into 96 scalar registers)
            float v[16], pr[16];
            win.take(v);
            win.issue(j + 1 < nk ? j + 1 : j);          // the next window is fetched under this one's transform
            input_grad_forward<LOG2P>(v, pr, a, mk, b, chs, tb, lane);
            #pragma unroll
            for (int r = 0; r < 16; r++) {
                const bool up = pr[r] > best[r];
                best[r] = up ? pr[r] : best[r];
                at[r] = up ? j : at[r];
            }
        }
        const long f0 = (long)b * 1024 + lane;
        #pragma unroll
        for (int r = 0; r < 16; r++) {
            const long f = f0 + r * 64;
            if (f < a.F) arow[f] = at[r];
        }
    }
    // (tile_sorf's exchanges are inline assembly: the explicit wait, as in front of every cross-wave barrier -- DESIGN.md 5)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __threadfence_block();
    __syncthreads();

    // ---- pass 2: the windows' gradients, overlap-added per position
    const PoolGradTile<LOG2P> tile = {a, a.w + i * a.w_row_stride, arow};
    seq_overlap_add_body<LOG2P>(s, win, tile, tb);
}

template <int LOG2P>
__global__ __launch_bounds__(256) void conv_maxpool_input_grad_kernel(PoolInputGradArgs p) {
    DenseWindows<LOG2P> win;
    pool_input_grad_body<LOG2P>(p, win);
}

// the token form: s.win.x is the table [vocab, C] (unscaled), copied into LDS with one 0.0f behind it as in wave_conv_tok_kernel
template <int LOG2P>
__global__ __launch_bounds__(256) void conv_token_maxpool_input_grad_kernel(PoolInputGradArgs p) {
    __shared__ __attribute__((aligned(16))) float tab[TOK_TABLE_FLOATS + 4];
    const int nt = p.s.win.vocab * p.s.win.kmer_stride;     // <= TOK_TABLE_FLOATS (conv_token_maxpool_input_grad_ok)
    for (int t = threadIdx.x; t < nt; t += 256) tab[t] = p.s.win.x[t];
    if (threadIdx.x == 0) tab[nt] = 0.0f;
    __syncthreads();
    TokenWindows<LOG2P> win;
    win.tab = reinterpret_cast<const char *>(tab);
    pool_input_grad_body<LOG2P>(p, win);
}

// 1: the kernel serves a window of `width` = conv_width * C elements
int conv_maxpool_input_grad_ok_impl(long width) { return width >= 1 && padded_width(width) <= 1024 ? 1 : 0; }
int conv_token_maxpool_input_grad_ok_impl(long width, long vocab, long C) {
    return conv_maxpool_input_grad_ok_impl(width) && conv_token_rows_ok(width, vocab, C) ? 1 : 0;
}

// Both entry points: the dense form reads x [n, L, C]; in the token form x is the table [vocab, C] and tokens [n, L] index its rows.
int pool_input_grad_impl(const uint8_t *tokens, bool token_form, const float *x, const double *g, double *out, int32_t *argmax,
                         const int8_t *radem, const float *chi, const int32_t *seqlen_host, const int32_t *seqlen_dev, long n, long L,
                         long vocab, long C, long g_row_stride, long num_freqs, long R, int conv_width, void *workspace, size_t wbytes,
                         void *stream) {
    if (n < 0 || L < 1 || C < 1) return fail(XGPR_ERR_ARRAY_DIMS, "incorrect array dims passed");
    if (conv_width <= 0 || L < conv_width) return fail(XGPR_ERR_CONV_WIDTH, "invalid conv_width");
    const long win = (long)conv_width * C;
    const long P = padded_width(win);
    const long reps = num_freqs >= 1 ? (num_freqs + P - 1) / P : 0;
    if (num_freqs < 1 || R != reps * P) return fail(XGPR_ERR_RFFS_FREQS, "incorrect number of rffs and or freqs.");
    if (g_row_stride != 0 && g_row_stride < num_freqs) return fail(XGPR_ERR_ARRAY_SIZES, "g_row_stride is shorter than num_freqs");
    if (n > 0) {
        int rc = check_seqlens(seqlen_host, n, n, L, conv_width);
        if (rc) return rc;
    }
    if (token_form) {
        if (vocab < 1 || vocab > 256) return fail(XGPR_ERR_ARRAY_DIMS, "token table: vocab must be 1 .. 256 (uint8 tokens)");
        if (!conv_token_maxpool_input_grad_ok_impl(win, vocab, C))
            return fail(XGPR_ERR_UNSUPPORTED, "token input serves windows of up to 1024 elements and tables of up to 4608 floats (see xgpr_conv_token_maxpool_input_grad_ok)");
    } else if (!conv_maxpool_input_grad_ok_impl(win)) return fail(XGPR_ERR_UNSUPPORTED, TOO_WIDE_WAVE);
    if (n == 0) return 0;
    if (!workspace || wbytes < masks_bytes(R)) return fail(XGPR_ERR_WORKSPACE, "workspace too small (see xgpr_rbf_workspace_bytes)");
    if (!x || !g || !out || !argmax || !radem || !chi || !seqlen_dev || (token_form && !tokens))
        return fail(XGPR_ERR_WORKSPACE, "NULL array pointer");
    if (n > 2147483647L || L * C > 2147483647L) return fail(XGPR_ERR_UNSUPPORTED, "too many datapoints for one launch");
    hipStream_t st = (hipStream_t)stream;
    const int lg = ilog2(P);
    PoolInputGradArgs p = {};
    p.argmax = argmax;
    SeqInputGradArgs &s = p.s;
    s.win = wave_args(x, chi, workspace, n, token_form ? L : L * C, win, num_freqs, R);
    s.win.tokens = tokens; s.win.vocab = (int)vocab;
    s.win.seqlen = seqlen_dev; s.win.kmer_stride = (int)C; s.win.conv_width = conv_width;
    InputGradArgs &a = s.ig;
    a.w = g; a.g = out; a.masks = s.win.masks; a.chi = chi;
    a.n = n; a.w_row_stride = g_row_stride; a.F = num_freqs; a.w_cols = num_freqs;
    a.d = (int)win; a.MW = s.win.MW; a.nb = s.win.nb;
    a.nc = s.win.nc; a.chi_scale = s.win.chi_scale;
    a.scale = 1.0; a.sigma = 1.0;
    s.L = (int)L; s.scaling_type = 0;
    int rc = pack_masks(radem, (uint64_t *)workspace, R, a.MW, st);
    if (rc) return rc;
    return dispatch_lg<1, 10>(lg, TOO_WIDE_WAVE, [&](auto LG) {
        if (token_form)
            return launch(conv_token_maxpool_input_grad_kernel<decltype(LG)::value>, dim3((unsigned)n), dim3(256), 0, st,
                          "conv_token_maxpool_input_grad_kernel launch", p);
        return launch(conv_maxpool_input_grad_kernel<decltype(LG)::value>, dim3((unsigned)n), dim3(256), 0, st,
                      "conv_maxpool_input_grad_kernel launch", p);
    });
}
