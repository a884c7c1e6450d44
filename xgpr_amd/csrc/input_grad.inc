// input_grad.inc -- part of xgpr_hip.hip (included inside its anonymous namespace, after launchers.inc): the input gradient of a
// weighted sum of the fixed-vector kernels' random features (xgpr_rbf_input_grad_f32, include/xgpr_hip_input_grad.h; DESIGN.md 3.16).
//
// For a row x (already multiplied by sigma) with projections p = W x the sum  mu = sum_f c (w[2f] cos p_f + w[2f+1] sin p_f)  has
//     d mu / d x = sigma W^T u,     u_f = c (w[2f+1] cos p_f - w[2f] sin p_f)
// and W^T is the TRANSPOSED SORF: per repetition S = c^3 H D2 H D1 H D0 (c = 2^(-k/2), D_s the sign diagonals), so
// S^T = c^3 D0 H D1 H D2 H, applied to chi (.) u; the repetitions' results are summed and the first d entries kept.
//
// One workgroup of four waves per row; wave w takes the tiles b = w, w + 4, ... (1024 frequencies each) and per tile
//   forward   wave_load, tile_sorf, the chi product and tile_sincos -- the front end of wave_rbf_kernel<LOG2P, OUT_CACHE> through the
//             same device functions, so the float32 cos / sin arguments are those of the feature operators bit for bit;
//   middle    u_f in double from the float64 weights and the widened cos / sin (w[0] dropped under the intercept: column 0 of the
//             features is the constant 1; frequencies >= F and columns >= w_cols are zero), rounded ONCE to float, times chi[f] in float;
//   backward  three rounds of { wave_fht ; sign flip (x normaliser for odd log2 P) } in the order 2, 1, 0 on the tile in layout C --
//             register r of lane l is element 64 r + l, the layout of the packed sign masks; every one of the tile's 1024 / P
//             repetitions is transformed on its own, as in the forward direction.  For even log2 P the normaliser c^3 is an exact
//             power of two and rides on chi (a.chi_scale), as the forward side folds it;
//   sum       each lane adds its sixteen results to sixteen float64 partials (layout C).
// After its last tile a wave folds the partials over the repetitions of a tile (registers r = e mod P / 64; lanes l mod P below 64),
// the four waves meet once in LDS and the sums are formed in the fixed order ((w0 + w1) + w2) + w3, multiplied by sigma in double and
// stored: no atomics, and a row's result depends on nothing but that row (not on n, not on its position in the batch).
// ------------------------------------------------------------------------------------
struct InputGradArgs {
    const float *x; const double *w; double *g;
    const uint64_t *masks; const float *chi;
    long n; long w_row_stride; long F; long w_cols;
    int d; int MW; int nb;        // masks per diagonal; tiles that hold a column below w_cols
    int fit_intercept;
    float nc; float chi_scale;    // fill_norms
    double scale;                 // the float-typed feature constant, widened (rbf_scale<float>)
    double sigma;
};

// The backward half of a tile, shared by input_grad_tile below and the max-pool backward (pool_input_grad.inc): H, D2, H, D1, H, D0
// on every repetition of the tile in layout C.  On entry v holds t_f = (float)u_f * chi[f] (x the folded normaliser).
template <int LOG2P>
__device__ __forceinline__ void input_grad_backward(float (&v)[16], const cmask_t mk, int MW, float nc, int lane) {
    #pragma unroll
    for (int s = 2; s >= 0; s--) {
        wave_fht<LOG2P>(v, lane);
        uint64_t m[16];
        #pragma unroll
        for (int r = 0; r < 16; r++) m[r] = mk[(long)s * MW + r];
        #pragma unroll
        for (int r = 0; r < 16; r++) {
            const float t = (LOG2P & 1) ? v[r] * nc : v[r];
            v[r] = __builtin_amdgcn_inverse_ballot_w64(m[r]) ? -t : t;
        }
    }
}

// The forward half of a tile, shared the same way: tile_sorf on the tile the caller loaded (layout C), then the projections
// arg_f = v_f * (chi[f] * chs) exactly as the feature and max-pool operators form them (frequencies >= F take chi[0]: never used).
// mk: the tile's packed sign masks, as_cmask(a.masks + 16 b).
template <int LOG2P>
__device__ __forceinline__ void input_grad_forward(float (&v)[16], float (&arg)[16], const InputGradArgs &a, const cmask_t mk, int b,
                                                   float chs, float *tb, int lane) {
    constexpr bool TP = LOG2P >= 7;
    uint32_t sw[3] = {0, 0, 0};
    if constexpr (TP) load_sign_words(sw, a.masks, a.MW, b, lane);
    tile_sorf<LOG2P, TP, TP, false>(v, mk, sw, tb, a.MW, a.nc, lane);
    const long f0 = (long)b * 1024 + lane;
    #pragma unroll
    for (int r = 0; r < 16; r++) {
        const long f = f0 + r * 64;
        const float ch = a.chi[f < a.F ? f : 0];
        arg[r] = v[r] * (ch * chs);
    }
}

// One tile (1024 frequencies, tile b) of the gradient, shared by the fixed-vector kernel below and the sequence kernel
// (seq_input_grad.inc).  On entry v holds the sigma-scaled row -- or k-mer window -- replicated over the tile's 1024 / P transforms
// (wave_load's layout C); on return it holds the tile's part of W^T u in layout C, every repetition on its own.  `scale` is the
// feature constant of u (the sequence kernels divide it by the k-mer normaliser), `chs` chi's factor with the sign tile_sorf kept.
template <int LOG2P>
__device__ __forceinline__ void input_grad_tile(float (&v)[16], const InputGradArgs &a, const double *wrow, double scale, int b, float chs,
                                                float *tb, int lane) {
    const long hcols = a.w_cols >> 1;                    // frequencies with a weight pair
    const cmask_t mk = as_cmask(a.masks + (long)b * 16);
    // ---- forward: the feature operators' front end (the tile is loaded by the caller)
    float arg[16], sn[16], cs[16];
    input_grad_forward<LOG2P>(v, arg, a, mk, b, chs, tb, lane);
    const long f0 = (long)b * 1024 + lane;
    tile_sincos(arg, sn, cs);
    // ---- middle: t_f = (float)u_f * chi[f] (x the folded normaliser: exact)
    #pragma unroll
    for (int r = 0; r < 16; r++) {
        const long f = f0 + r * 64;
        const bool in = f < a.F && f < hcols;
        const long fc = in ? f : 0;
        const double w0 = wrow[2 * fc], w1 = wrow[2 * fc + 1];
        const double wc = (in && !(a.fit_intercept && f == 0)) ? w0 : 0.0;
        const double ws = in ? w1 : 0.0;
        const double u = scale * (ws * (double)cs[r] - wc * (double)sn[r]);
        const float bk = in ? a.chi[fc] * a.chi_scale : 0.0f;
        v[r] = (float)u * bk;
    }
    // ---- backward: H, D2, H, D1, H, D0 on every repetition of the tile
    input_grad_backward<LOG2P>(v, mk, a.MW, a.nc, lane);
}

template <int LOG2P>
__global__ __launch_bounds__(256) void rbf_input_grad_kernel(InputGradArgs a) {
    constexpr int P = 1 << LOG2P;
    constexpr bool TP = LOG2P >= 7;
    constexpr int RP = P >= 64 ? P / 64 : 1;            // registers that hold distinct input dimensions (layout C)
    constexpr int RED = P >= 64 ? P : 64;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long i = blockIdx.x;
    __shared__ __attribute__((aligned(16))) float tbuf[TP ? 4 * TBUF_FLOATS : 4];
    __shared__ double red[4][RED];
    float *tb = tbuf + wv * (TP ? TBUF_FLOATS : 1);
    const float *xrow = a.x + i * (long)a.d;
    const double *wrow = a.w + i * a.w_row_stride;
    const float chs = TP ? a.chi_scale * sorf_kept_sign(lane) : a.chi_scale;     // the sign tile_sorf kept, into chi (exact)
    double acc[16];
    #pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = 0.0;

    for (int bb = wv; bb < a.nb; bb += 4) {
        const int b = __builtin_amdgcn_readfirstlane(bb);
        float v[16];
        wave_load<LOG2P>(v, xrow, a.d, lane);
        input_grad_tile<LOG2P>(v, a, wrow, a.scale, b, chs, tb, lane);
        #pragma unroll
        for (int r = 0; r < 16; r++) acc[r] += (double)v[r];
    }

    // ---- the repetitions of a tile: element e of the tile is input dimension e mod P
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
    double *grow = a.g + i * (long)a.d;
    for (int e = threadIdx.x; e < a.d; e += 256)
        grow[e] = (((red[0][e] + red[1][e]) + red[2][e]) + red[3][e]) * a.sigma;
}

// 1: the wave-tile kernel serves this shape
int rbf_input_grad_ok_impl(long d, long num_freqs) {
    return d >= 1 && num_freqs >= 1 && padded_width(d) <= 1024 ? 1 : 0;
}

int rbf_input_grad_impl(const float *x, const double *w, double *g, const int8_t *radem, const float *chi, long n, long d,
                        long w_row_stride, long w_cols, long num_freqs, long R, double sigma, int fit_intercept, void *workspace,
                        size_t wbytes, void *stream) {
    if (n < 0 || d < 1) return fail(XGPR_ERR_ARRAY_DIMS, "incorrect array dims passed");
    if (num_freqs < 1 || num_freqs > R) return fail(XGPR_ERR_RFFS_FREQS, "incorrect number of rffs and or freqs.");
    if (w_cols < 2 || (w_cols & 1) != 0) return fail(XGPR_ERR_ODD_OUTPUT, "w_cols must be an even number >= 2");
    if (w_cols > 2 * num_freqs) return fail(XGPR_ERR_ARRAY_SIZES, "w_cols exceeds the number of features");
    if (w_row_stride != 0 && w_row_stride < w_cols) return fail(XGPR_ERR_ARRAY_SIZES, "w_row_stride is shorter than w_cols");
    const long P = padded_width(d);
    if (R % P != 0) return fail(XGPR_ERR_RFFS_FREQS, "incorrect number of rffs and or freqs.");
    if (!rbf_input_grad_ok_impl(d, num_freqs)) return fail(XGPR_ERR_UNSUPPORTED, TOO_WIDE_WAVE);
    if (n == 0) return 0;
    if (!workspace || wbytes < masks_bytes(R)) return fail(XGPR_ERR_WORKSPACE, "workspace too small (see xgpr_rbf_workspace_bytes)");
    if (!x || !w || !g || !radem || !chi) return fail(XGPR_ERR_WORKSPACE, "NULL array pointer");
    if (n > 2147483647L) return fail(XGPR_ERR_UNSUPPORTED, "too many datapoints for one launch");
    hipStream_t st = (hipStream_t)stream;
    const int lg = ilog2(P);
    InputGradArgs a = {};
    a.x = x; a.w = w; a.g = g; a.masks = (const uint64_t *)workspace; a.chi = chi;
    a.n = n; a.w_row_stride = w_row_stride; a.F = num_freqs; a.w_cols = w_cols;
    a.d = (int)d; a.MW = masks_per_diag(R);
    const long live = w_cols / 2 < num_freqs ? w_cols / 2 : num_freqs;
    a.nb = (int)((live + 1023) / 1024);
    a.fit_intercept = fit_intercept;
    {
        WaveArgs norms = {};
        fill_norms(norms, lg);
        a.nc = norms.nc; a.chi_scale = norms.chi_scale;
    }
    a.scale = rbf_scale<float>(num_freqs, fit_intercept);
    a.sigma = sigma;
    int rc = pack_masks(radem, (uint64_t *)workspace, R, a.MW, st);
    if (rc) return rc;
    return dispatch_lg<1, 10>(lg, TOO_WIDE_WAVE, [&](auto LG) {
        return launch(rbf_input_grad_kernel<decltype(LG)::value>, dim3((unsigned)n), dim3(256), 0, st, "rbf_input_grad_kernel launch", a);
    });
}
