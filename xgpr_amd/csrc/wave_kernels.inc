// wave_kernels.inc -- part of xgpr_hip.hip (included inside its anonymous namespace, in order): wave-tile kernels: feature generation, convolution operators, the two-wave fused CG matvec / z^T y.
// ---- cudaRBFFeatureGen: one wave per (datapoint, tile); 4 waves per workgroup.  With CACHE the
// kernel writes the float32 (cos, sin) pairs before scaling -- the exact values the float64
// output is the widening of -- into a.outf [n, 2F] (the resident feature cache).
// OUT_GRAD_ROWS (xgpr_rbf_grad_rows_f32): OUT_GRAD's arithmetic with another epilogue -- the float values OUT_GRAD widens at its
// double2 stores go out as float2 pairs into two float32 row arrays, a.outf (features) and a.gradf (d features / d sigma), with
// the intercept column written here (1.0f / 0.0f): complete rows, both overwritten.
enum { OUT_F64 = 0, OUT_CACHE = 1, OUT_GRAD = 2, OUT_GRAD_ROWS = 3 };

template <int LOG2P, int OUT>
__global__ __launch_bounds__(256) void wave_rbf_kernel(WaveArgs a) {
    constexpr bool CACHE = OUT == OUT_CACHE;
    const int lane = threadIdx.x & 63;
    const long item = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) + (long)blockIdx.x * 4;
    if (item >= a.n * a.nb) return;
    const long i = item / a.nb;
    const int b = __builtin_amdgcn_readfirstlane((int)(item % a.nb));
    float v[16];
    // Address forms: everything this wave touches is "wave-uniform 64-bit base (scalar unit) + 32-bit lane offset
    // (+ immediate)"; the offsets are laundered so that the compiler does not fold them back into per-lane 64-bit pointers
    // (a fifth of this kernel's vector instructions were address arithmetic, bounds compares and selects).
    unsigned lane4 = 4u * lane, lane8 = 8u * lane;
    asm volatile("" : "+v"(lane4), "+v"(lane8));
    const float *xrow = a.x + i * a.row_stride;
    // (the float64 operator keeps the general forms: it is bound by its write stream, and with the leaner front end --
    // 54 instead of 76 registers, eight waves per SIMD instead of six -- it measured 3 % SLOWER, 1.70 against 1.65 ms per
    // 131072 x 8192 rows; the float32 cache rows, which are bound by this arithmetic, got 11 % faster: 1.13 -> 1.00 ms)
    constexpr bool LEAN = OUT != OUT_F64;
    if (LEAN && LOG2P >= 6 && a.d == (1 << LOG2P)) {    // wave-uniform: a full-width row needs no bounds selects
        constexpr int RP = (1 << LOG2P) / 64;
        #pragma unroll
        for (int r = 0; r < RP; r++) v[r] = *reinterpret_cast<const float *>(reinterpret_cast<const char *>(xrow) + lane4 + 256 * r);
        #pragma unroll
        for (int r = RP; r < 16; r++) v[r] = v[r & (RP - 1)];
    } else wave_load<LOG2P>(v, xrow, a.d, lane);
    constexpr bool TP = LOG2P >= 7;
#ifndef XGPR_ABL_RBF_PAD
#define XGPR_ABL_RBF_PAD 0          // (development: extra LDS per workgroup caps the waves resident per SIMD)
#endif
    __shared__ __attribute__((aligned(16))) float tbuf[(TP ? 4 * TBUF_FLOATS : 4) + (OUT == OUT_F64 ? XGPR_ABL_RBF_PAD : 0)];
    uint32_t sw[3] = {0, 0, 0};
    if constexpr (TP) load_sign_words(sw, a.masks, a.MW, b, lane);
    tile_sorf<LOG2P, TP, TP, false>(v, as_cmask(a.masks + (long)b * 16), sw, tbuf + (threadIdx.x >> 6) * (TP ? TBUF_FLOATS : 1),
                                    a.MW, a.nc, lane);
    const long f0 = (long)b * 1024 + lane;
    const bool full = f0 - lane + 1024 <= a.F;      // wave-uniform: the whole tile is inside F
    const float chs = TP ? a.chi_scale * sorf_kept_sign(lane) : a.chi_scale;     // the sign tile_sorf kept, into chi (exact)
    float arg[16], sn[16], cs[16];
    if (LEAN && full) {
        const char *chi_t = reinterpret_cast<const char *>(a.chi + (long)b * 1024);
        #pragma unroll
        for (int r = 0; r < 16; r++) arg[r] = v[r] * (*reinterpret_cast<const float *>(chi_t + lane4 + 256 * r) * chs);
    } else {
        #pragma unroll
        for (int r = 0; r < 16; r++) {
            const long f = f0 + r * 64;
            const float ch = a.chi[(full || f < a.F) ? f : 0];
            arg[r] = v[r] * (ch * chs);
        }
    }
    if constexpr (OUT == OUT_GRAD || OUT == OUT_GRAD_ROWS) {
        // cudaRBFGrad: shared_rfgen_ops.cpp:140-155 with its roundings back to float; the input is
        // not pre-multiplied by sigma, and the scale is a double here (rbf_ops.cpp:180-185)
        float gv[16];
        #pragma unroll
        for (int r = 0; r < 16; r++) { gv[r] = arg[r]; arg[r] = (float)(gv[r] * a.sigma); }
        tile_sincos(arg, sn, cs);
        if constexpr (OUT == OUT_GRAD_ROWS) {
            float *zrow = a.outf + i * 2 * a.F, *grow = a.gradf + i * 2 * a.F;
            const bool icpt = a.fit_intercept != 0;
            #pragma unroll
            for (int r = 0; r < 16; r++) {
                const long f = f0 + r * 64;
                if (full || f < a.F) {
                    const float cos_val = (float)(cs[r] * a.scale), sin_val = (float)(sn[r] * a.scale);
                    const float gs = sin_val * gv[r], gc = cos_val * gv[r];
                    const bool c0 = icpt && f == 0;                 // KernelBase.gradient_x: xtrans[:, 0] = 1, xgrad[:, 0] = 0
                    *reinterpret_cast<float2 *>(zrow + 2 * f) = make_float2(c0 ? 1.0f : cos_val, sin_val);
                    *reinterpret_cast<float2 *>(grow + 2 * f) = make_float2(c0 ? 0.0f : -gs, gc);
                }
            }
            return;
        }
        double *orow = a.out + i * 2 * a.F, *grow = a.grad + i * 2 * a.F;
        #pragma unroll
        for (int r = 0; r < 16; r++) {
            const long f = f0 + r * 64;
            if (full || f < a.F) {
                const float cos_val = (float)(cs[r] * a.scale), sin_val = (float)(sn[r] * a.scale);
                const float gs = sin_val * gv[r], gc = cos_val * gv[r];
                *reinterpret_cast<double2 *>(orow + 2 * f) = make_double2(cos_val, sin_val);
                *reinterpret_cast<double2 *>(grow + 2 * f) = make_double2(-(double)gs, gc);
            }
        }
        return;
    }
    tile_sincos(arg, sn, cs);
    if constexpr (CACHE) {
        float *crow = a.outf + i * 2 * a.F;
        if (full) {
            char *ct = reinterpret_cast<char *>(crow + (long)b * 2048);
            #pragma unroll
            for (int r = 0; r < 16; r++) *reinterpret_cast<float2 *>(ct + lane8 + 512 * r) = make_float2(cs[r], sn[r]);
            return;
        }
        #pragma unroll
        for (int r = 0; r < 16; r++) {
            const long f = f0 + r * 64;
            if (f < a.F) *reinterpret_cast<float2 *>(crow + 2 * f) = make_float2(cs[r], sn[r]);
        }
        return;
    }
    double *orow = a.out + i * 2 * a.F;
    if (full) {
        #pragma unroll
        for (int r = 0; r < 16; r++)
            *reinterpret_cast<double2 *>(orow + 2 * (f0 + r * 64)) = make_double2(cs[r] * a.scale, sn[r] * a.scale);
    } else {
        #pragma unroll
        for (int r = 0; r < 16; r++) {
            const long f = f0 + r * 64;
            if (f < a.F) *reinterpret_cast<double2 *>(orow + 2 * f) = make_double2(cs[r] * a.scale, sn[r] * a.scale);
        }
    }
}

// ---- processing order of the sequences of one convolution launch: longest first.  A wave runs for as long as its
// sequence has k-mers, workgroups are handed out in index order as earlier ones retire, and with the caller's order the
// long sequences that happen to sit at the end of a chunk leave most of the GPU idle while they finish (BASELINE
// configs[3] calls the operator on 1024 sequences at a time: ~2.7 rounds of waves, 15-20 % of the launch is tail).
// Counting sort by length in one workgroup: histogram in LDS, descending exclusive scan, scatter.  The order inside a
// length class depends on atomics; every (sequence, tile) is computed independently, so results do not.
__global__ __launch_bounds__(1024) void conv_order_kernel(const int32_t *__restrict__ seqlen, int32_t *order, long n, int maxlen) {
    extern __shared__ int hist[];                       // [maxlen + 1] counts, then start offsets
    for (int i = threadIdx.x; i <= maxlen; i += blockDim.x) hist[i] = 0;
    __syncthreads();
    for (long i = threadIdx.x; i < n; i += blockDim.x) atomicAdd(&hist[seqlen[i]], 1);
    __syncthreads();
    if (threadIdx.x == 0) {                             // <= a few thousand bins: a serial scan costs microseconds
        int run = 0;
        for (int l = maxlen; l >= 0; l--) { const int c = hist[l]; hist[l] = run; run += c; }
    }
    __syncthreads();
    for (long i = threadIdx.x; i < n; i += blockDim.x) order[atomicAdd(&hist[seqlen[i]], 1)] = (int32_t)i;
}

// ---- cudaConv1dFGen / cudaConv1dMaxpool: one wave per (sequence, tile), k-mers looped inside
// the wave in the reference's order, sums kept in registers, one read-modify-write at the end.
// MODE: 0 = cudaConv1dFGen, 1 = cudaConv1dMaxpool, 2 = cudaConvGrad -- separate instantiations, so that the
// 64 extra float64 accumulators of the gradient do not set the register allocation (and with it the occupancy:
// 1 wave per SIMD when the three shared one function) of the feature operator.
// MODE 3 = the float32 feature rows (xgpr_conv_feature_rows_f32): CONV_FGEN's front end and k-mer loop unchanged (chi in
// LDS, laundered sign words, prefetch of the next window, float64 sums in the same order); the epilogue OVERWRITES
// a.outf[i, 2 f ..] with (float)(0.0 + sum * rs) as (cos, sin) float2 pairs -- what CONV_FGEN leaves in a zeroed float64
// output, rounded once -- and puts 1.0f into column 0 under fit_intercept.  No load of the old value.
// MODE 4 = the float32 feature AND gradient rows (xgpr_conv_grad_rows_f32): CONV_GRAD's front end and k-mer loop unchanged (the
// per-k-mer roundings to float, the four float64 sums in the same order); the epilogue OVERWRITES a.outf[i, 2 f ..] and
// a.gradf[i, 2 f ..] with (float)(0.0 + sum) as float2 pairs -- what CONV_GRAD leaves in zeroed float64 out / grad, rounded
// once -- and puts 1.0f / 0.0f into column 0 under fit_intercept (KernelBase.gradient_x).  No load of the old values.
enum { CONV_FGEN = 0, CONV_MAXPOOL = 1, CONV_GRAD = 2, CONV_ROWS = 3, CONV_GRAD_ROWS = 4 };
constexpr bool conv_is_feat(int mode) { return mode == CONV_FGEN || mode == CONV_ROWS; }
constexpr bool conv_is_grad(int mode) { return mode == CONV_GRAD || mode == CONV_GRAD_ROWS; }
#ifdef XGPR_ABL_NOC2
#define XGPR_CONV_C2_ALL 0
#else
#define XGPR_CONV_C2_ALL 1          // the feature operator's tile takes the transposed-columns / rows-only path at EVERY window width <= 256
#endif

// Where the k-mer windows come from is a policy of the kernel body (WIN): begin(a, i, lane) once per sequence, issue(j) starts the
// fetch of window j into the policy's own registers, take(v) completes it into the tile (replicated over the tile's 1024 / P
// transforms).  DenseWindows: the float32 array x[n, L, C], wave_load_base / wave_expand as before.
template <int LOG2P> struct DenseWindows {
    const float *xrow; int d, kmer_stride, lane;
    float nx[TileBase<LOG2P>::N];
    __device__ __forceinline__ void begin(const WaveArgs &a, long i, int lane_) {
        xrow = a.x + i * a.row_stride; d = a.d; kmer_stride = a.kmer_stride; lane = lane_;
    }
    __device__ __forceinline__ void issue(int j) { wave_load_base<LOG2P>(nx, xrow + (long)j * kmer_stride, d, lane); }
    __device__ __forceinline__ void take(float (&v)[16]) const { wave_expand<LOG2P>(v, nx); }
};

// TokenWindows: tokens[n, L] (uint8) index the rows of a table[V, C] that the workgroup holds in LDS (wave_conv_tok_kernel).  Element e
// of window j is table[tokens[i, j + e / C]][e % C] for e < conv_width * C and 0.0f beyond.  (e / C, e % C) does not depend on j: begin()
// works them out once per wave for the lane's N = P / 64 window registers -- the position as the byte offset of the token load, the
// channel as a byte offset into the table image -- and the k-mer loop has no division.  Padding needs no select either: a padded
// element's position is past the window's conv_width token bytes, the buffer range check answers token 0, and its channel offset points
// at the one 0.0f kept behind the table (row 0 + that offset = the zero slot).  issue(j) puts the N token bytes of window j in flight
// (global memory: a sequence's L bytes stay in L2, and one byte load per register replaces the dense float load one for one); take(v)
// turns them into LDS addresses -- one multiply-add each -- and gathers.  Windows of 512 / 1024 elements keep position and channel
// offset packed in ONE register per window register (16 fewer live registers at 1024; see conv_tok_min_blocks).
// Token values are < V by the caller's contract (the dataset builders check it once).
constexpr int TOK_TABLE_FLOATS = 4608;      // V * C at most: 18 KiB beside the 34 KiB of chi and exchange buffers, three workgroups per CU
template <int LOG2P> struct TokenWindows {
    static constexpr int N = TileBase<LOG2P>::N;
    static constexpr bool PACK = N >= 8;
    const uint8_t *trow; const char *tab; int cw; unsigned c4;
    unsigned pos[N], cho[PACK ? 1 : N], tk[N];
    __device__ __forceinline__ void begin(const WaveArgs &a, long i, int lane) {
        constexpr int P = 1 << LOG2P;
        trow = a.tokens + i * a.row_stride; cw = a.conv_width; c4 = 4u * (unsigned)a.kmer_stride;
        const unsigned C = (unsigned)a.kmer_stride, zero4 = 4u * (unsigned)a.vocab * C;
        #pragma unroll
        for (int r = 0; r < N; r++) {
            const unsigned e = P >= 64 ? (unsigned)(r * 64 + lane) : (unsigned)(lane & (P - 1));
            const unsigned q = e / C;
            const bool ok = e < (unsigned)a.d;
            const unsigned p = ok ? q : 0xffffu, c = ok ? 4u * (e - q * C) : zero4;      // (conv_width <= 1024 < 0xffff: out of range)
            if constexpr (PACK) pos[r] = p | (c << 16);
            else { pos[r] = p; cho[r] = c; }
        }
    }
    __device__ __forceinline__ void issue(int j) {
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(trow + j), 0, cw, 0x00020000);
        #pragma unroll
        for (int r = 0; r < N; r++) tk[r] = __builtin_amdgcn_raw_buffer_load_b8(rs, (int)(PACK ? pos[r] & 0xffffu : pos[r]), 0, 0);
    }
    __device__ __forceinline__ void take(float (&v)[16]) const {
        float nx[N];
        #pragma unroll
        for (int r = 0; r < N; r++) nx[r] = *reinterpret_cast<const float *>(tab + (tk[r] * c4 + (PACK ? pos[r] >> 16 : cho[r])));
        wave_expand<LOG2P>(v, nx);
    }
};

// SubstTokenWindows: TokenWindows with one more way to complete a fetch (the substitution scan, edit_scan.inc).  take_subst(v, q, tok)
// is take(v) on the window whose token at position offset q is `tok`: the registers whose position offset equals q gather from table
// row `tok`, every other register from the row of the byte it fetched.  Padded registers carry the offset 0xffff and never match.  The
// fetched bytes are left as they are: one issue(j) serves every variant of window j.
template <int LOG2P> struct SubstTokenWindows : TokenWindows<LOG2P> {
    using Base = TokenWindows<LOG2P>;
    __device__ __forceinline__ void take_subst(float (&v)[16], unsigned q, unsigned tok) const {
        float nx[Base::N];
        #pragma unroll
        for (int r = 0; r < Base::N; r++) {
            const unsigned p = Base::PACK ? this->pos[r] & 0xffffu : this->pos[r];
            const unsigned t = p == q ? tok : this->tk[r];
            nx[r] = *reinterpret_cast<const float *>(this->tab + (t * this->c4 + (Base::PACK ? this->pos[r] >> 16 : this->cho[r])));
        }
        wave_expand<LOG2P>(v, nx);
    }
};

// IndelTokenWindows: the windows of a sequence with ONE token deleted or inserted (the indel scan, edit_scan.inc), fetched from the
// original bytes by remapping each register's position offset -- no mutant is written.  Window jm of the mutant starts at the original
// byte jm, and q is the edit's position offset inside it.
//   issue_del(jm, q)   offset k reads the original k + (k >= q): the tokens before the deleted one, then those after it.  The range
//                      is the conv_width + 1 original bytes that can be touched; padded registers (offset 0xffff) stay outside it.
//   issue_ins(jm, q)   offset k < q reads k, k > q reads k - 1; the register at k == q fetches a byte that take_subst(v, q, tok)
//                      (SubstTokenWindows) replaces by the inserted token.  Only conv_width - 1 original bytes belong to such a window and
//                      the range is set to them: the byte behind an appended token, which may lie past the array, is never addressed.
template <int LOG2P> struct IndelTokenWindows : SubstTokenWindows<LOG2P> {
    using Base = TokenWindows<LOG2P>;
    __device__ __forceinline__ void issue_del(int jm, unsigned q) {
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(this->trow + jm), 0, this->cw + 1, 0x00020000);
        #pragma unroll
        for (int r = 0; r < Base::N; r++) {
            const unsigned k = Base::PACK ? this->pos[r] & 0xffffu : this->pos[r];
            this->tk[r] = __builtin_amdgcn_raw_buffer_load_b8(rs, (int)(k + (k >= q ? 1u : 0u)), 0, 0);
        }
    }
    __device__ __forceinline__ void issue_ins(int jm, unsigned q) {
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(this->trow + jm), 0, this->cw - 1, 0x00020000);
        #pragma unroll
        for (int r = 0; r < Base::N; r++) {
            const unsigned k = Base::PACK ? this->pos[r] & 0xffffu : this->pos[r];
            this->tk[r] = __builtin_amdgcn_raw_buffer_load_b8(rs, (int)(k - (k > q ? 1u : 0u)), 0, 0);
        }
    }
};

constexpr int conv_min_blocks(int LOG2P, int MODE) {
    return (conv_is_grad(MODE) && LOG2P >= 7) ? 1 : (conv_is_feat(MODE) && (LOG2P >= 7 || XGPR_CONV_C2_ALL)) ? 3 : 2;
}

template <int LOG2P, int MODE, class WIN>
__device__ __forceinline__ void wave_conv_body(const WaveArgs &a, WIN &win) {
    constexpr bool MAXPOOL = MODE == CONV_MAXPOOL;
    const int lane = threadIdx.x & 63;
    const long item = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) + (long)blockIdx.x * 4;
    if (item >= a.n * a.nb) return;
    const long i = a.order ? a.order[item / a.nb] : item / a.nb;      // longest sequences first when an order was built
    const int b = __builtin_amdgcn_readfirstlane((int)(item % a.nb));
    const int nk = a.seqlen[i] - a.conv_width + 1;
    const long f0 = (long)b * 1024 + lane;
    constexpr bool TP = LOG2P >= 7;
    // the feature operator on the T path keeps chi (x folded normaliser) in LDS, in the swizzled rows-of-16 image
    // (4 ds_read_b128 per k-mer instead of 16 registers held through the transform): with the sign words laundered
    // below that is what lets it run three waves per SIMD, like the fused matvec (fused_ztz.inc)
    constexpr bool CHI_LDS = (TP || XGPR_CONV_C2_ALL) && conv_is_feat(MODE);
    // windows of up to 256 elements (BASELINE configs[3]: 9 x 21 = 189): the feature operator's tile leaves the transform
    // in the transposed-columns layout (wave_sorf_c2: no cross-lane stage) -- register r of lane l is frequency
    // 1024 b + c2_elem(l, r), not 1024 b + 64 r + l
#ifdef XGPR_ABL_NOC2
    constexpr bool C2 = false;
#else
    constexpr bool C2 = LOG2P <= 8;      // all three operators (round 5: windows of up to 64 elements too -- graph kernels, short k-mers)
#endif
    constexpr bool RONLY = C2 && LOG2P <= 6;                  // ... of up to 64 elements: the tile stays in the rows layout (32, 64: with DPP stages)
    const long fe0 = (long)b * 1024 + (RONLY ? 16 * lane : C2 ? c2_elem(lane, 0) : lane);
    constexpr int FE_STEP = RONLY ? 1 : C2 ? 16 : 64;
    float ch[CHI_LDS ? 1 : 16];
    __shared__ __attribute__((aligned(16))) float chibuf[CHI_LDS ? 4 * TBUF_FLOATS : 4];
    float *chl = chibuf + (threadIdx.x >> 6) * (CHI_LDS ? TBUF_FLOATS : 1);
    #pragma unroll
    for (int r = 0; r < 16; r++) {
        const long f = fe0 + r * FE_STEP;
        const float cv = f < a.F ? a.chi[f] * a.chi_scale * (TP && !C2 ? sorf_kept_sign(lane) : (RONLY && (rd_parity<LOG2P>(lane) & 1u)) ? -1.0f : 1.0f) : 0.0f;   // + the sign the transform keeps
        if constexpr (CHI_LDS) chl[lane * 16 + ((((r >> 2) ^ row_swz(lane)) << 2) | (r & 3))] = cv;
        else ch[r] = cv;
    }
    cmask_t mk = as_cmask(a.masks + (long)b * 16);
    __shared__ __attribute__((aligned(16))) float tbuf[(TP || C2) ? 4 * TBUF_FLOATS : 4];
    float *tb = tbuf + (threadIdx.x >> 6) * ((TP || C2) ? TBUF_FLOATS : 1);
    uint32_t sw[3] = {0, 0, 0};
    if constexpr (TP || C2) load_sign_words(sw, a.masks, a.MW, b, lane);
    if constexpr (RONLY) {      // (windows of 32 / 64 elements: rounds 2, 3 also undo the sign the DPP stages left on this lane; 0 otherwise)
        sw[1] ^= rd_parity<LOG2P>(lane) & 0xffffu;
        sw[2] ^= rd_parity<LOG2P>(lane) & 0xffffu;
    }
    // one round's flips through SGPR lane masks (the wave keeps its tile's signs for all k-mers of the sequence)
    constexpr int C2_MROUND = (C2 && conv_is_feat(MODE) && (LOG2P & 1) == 0) ? 2 : -1;
    uint64_t fmask[16] = {};
    if constexpr (C2_MROUND >= 0) sign_lane_masks(fmask, sw[C2_MROUND]);
    // one k-mer's transform: the tile enters in layout C (the coalesced window) and leaves in C2 / R (windows <= 256) or C with the kept sign
    auto sorf_tile = [&](float (&t)[16]) {
        if constexpr (C2) {
            __builtin_amdgcn_s_setprio(1);
            wave_sorf_c2<LOG2P, C2_MROUND>(t, sw, tb, a.nc, lane, fmask);
            __builtin_amdgcn_s_setprio(0);
        } else tile_sorf<LOG2P, TP, TP>(t, mk, sw, tb, a.MW, a.nc, lane);
    };
    // the window of k-mer j + 1 is fetched while k-mer j is transformed (the loads used to sit at the top of
    // every iteration, exposing a global-memory round trip per k-mer)
    win.begin(a, i, lane);
    win.issue(0);
    if constexpr (MAXPOOL) {
        float acc[16];
        float *orow = a.outf + i * a.F;
        #pragma unroll
        for (int r = 0; r < 16; r++) {
            const long f = fe0 + r * FE_STEP;
            acc[r] = f < a.F ? orow[f] : 0.0f;
        }
        for (int j = 0; j < nk; j++) {
            mk = launder(mk);
            float v[16];
            win.take(v);
            win.issue(j + 1 < nk ? j + 1 : j);                                                              // next window
            sorf_tile(v);
            #pragma unroll
            for (int r = 0; r < 16; r++) {
                float prod = v[r] * ch[r];
                acc[r] = acc[r] > prod ? acc[r] : prod;
            }
        }
        #pragma unroll
        for (int r = 0; r < 16; r++) {
            const long f = fe0 + r * FE_STEP;
            if (f < a.F) orow[f] = acc[r];
        }
    } else if constexpr (conv_is_grad(MODE)) {
        // cudaConvGrad: per k-mer the roundings of shared_rfgen_ops.cpp:140-155 (values rounded back
        // to float before they are accumulated), sums over k-mers in float64 in the reference's order
        double rs = a.scale;
        if (a.scaling_type == 1) rs = a.scale / sqrt((double)nk);
        else if (a.scaling_type == 2) rs = a.scale / (double)nk;
        double oc[16], os[16], gc[16], gs[16];
        #pragma unroll
        for (int r = 0; r < 16; r++) { oc[r] = 0.0; os[r] = 0.0; gc[r] = 0.0; gs[r] = 0.0; }
        for (int j = 0; j < nk; j++) {
            mk = launder(mk);
            float v[16], gv[16], sn[16], cs[16];
            win.take(v);
            win.issue(j + 1 < nk ? j + 1 : j);                                                              // next window
            sorf_tile(v);
            #pragma unroll
            for (int r = 0; r < 16; r++) { gv[r] = v[r] * ch[r]; v[r] = (float)(gv[r] * a.sigma); }
            tile_sincos(v, sn, cs);
            #pragma unroll
            for (int r = 0; r < 16; r++) {
                const float cos_val = (float)(cs[r] * rs), sin_val = (float)(sn[r] * rs);
                oc[r] += cos_val;
                os[r] += sin_val;
                gc[r] -= sin_val * gv[r];
                gs[r] += cos_val * gv[r];
            }
        }
        if constexpr (MODE == CONV_GRAD_ROWS) {
            // (store patterns per layout: see CONV_ROWS below -- the same addresses, in two row arrays)
            float *zrow = a.outf + i * 2 * a.F, *grow = a.gradf + i * 2 * a.F;
            const bool icpt = a.fit_intercept != 0;
            #pragma unroll
            for (int r = 0; r < 16; r++) {
                const long f = fe0 + r * FE_STEP;
                if (f < a.F) {
                    const bool c0 = icpt && f == 0;                 // KernelBase.gradient_x: xtrans[:, 0] = 1, xgrad[:, 0] = 0
                    const float zc = (float)(0.0 + oc[r]), zs = (float)(0.0 + os[r]);      // (0.0 + x: the sibling's `old + x` on zeroed outputs)
                    const float dc = (float)(0.0 + gc[r]), ds = (float)(0.0 + gs[r]);
                    *reinterpret_cast<float2 *>(zrow + 2 * f) = make_float2(c0 ? 1.0f : zc, zs);
                    *reinterpret_cast<float2 *>(grow + 2 * f) = make_float2(c0 ? 0.0f : dc, ds);
                }
            }
        } else {
            double *orow = a.out + i * 2 * a.F, *grow = a.grad + i * 2 * a.F;
            #pragma unroll
            for (int r = 0; r < 16; r++) {
                const long f = fe0 + r * FE_STEP;
                if (f < a.F) {
                    double2 *o = reinterpret_cast<double2 *>(orow + 2 * f), *g = reinterpret_cast<double2 *>(grow + 2 * f);
                    double2 ov = *o, gvv = *g;
                    ov.x += oc[r]; ov.y += os[r];
                    gvv.x += gc[r]; gvv.y += gs[r];
                    *o = ov; *g = gvv;
                }
            }
        }
    } else {
        double ac[16], as[16];
        #pragma unroll
        for (int r = 0; r < 16; r++) { ac[r] = 0.0; as[r] = 0.0; }
        for (int j = 0; j < nk; j++) {
            asm volatile("; XGPR_MARK loop_top");      // (assembly comments for tools/count_loop_insts.py)
            mk = launder(mk);
            if constexpr (TP || C2) asm volatile("" : "+v"(sw[0]), "+v"(sw[1]), "+v"(sw[2]));   // three registers, not 48 hoisted masks
            float v[16], sn[16], cs[16];
            win.take(v);
            win.issue(j + 1 < nk ? j + 1 : j);                                                              // next window
            sorf_tile(v);
            if constexpr (CHI_LDS) {
                wave_lds_sync();
                const int csz = row_swz(lane);
                #pragma unroll
                for (int q = 0; q < 4; q++) {
                    const float4 c4 = *reinterpret_cast<const float4 *>(chl + lane * 16 + ((q ^ csz) << 2));
                    v[4 * q] *= c4.x; v[4 * q + 1] *= c4.y; v[4 * q + 2] *= c4.z; v[4 * q + 3] *= c4.w;
                }
            } else {
                #pragma unroll
                for (int r = 0; r < 16; r++) v[r] *= ch[r];
            }
            tile_sincos(v, sn, cs);
            #pragma unroll
            for (int r = 0; r < 16; r++) {
                ac[r] += (double)cs[r];
                as[r] += (double)sn[r];
            }
            asm volatile("; XGPR_MARK loop_end");
        }
        double rs = a.scale;
        if (a.scaling_type == 1) rs = a.scale / sqrt((double)nk);
        else if (a.scaling_type == 2) rs = a.scale / (double)nk;
        if constexpr (MODE == CONV_ROWS) {
            // Store pattern per instruction (one r, 64 lanes x 8 bytes).  Layout C (windows 512 / 1024): f = 1024 b + 64 r + lane,
            // 512 contiguous bytes = four whole 128-byte lines.  Layout C2 (128 / 256): f = 1024 b + 256 (lane >> 4) + 16 r + (lane & 15),
            // four runs of 128 contiguous bytes (sixteen lanes each) 2 KB apart -- whole lines when the row is 128-byte aligned.
            // Rows layout (<= 64): f = 1024 b + 16 lane + r, 8 bytes per lane 128 bytes apart; the sixteen stores of a lane
            // complete its line back to back and merge in L2 (the float64 sibling writes 16 bytes 256 apart the same way).
            float *crow = a.outf + i * 2 * a.F;
            const bool icpt = a.fit_intercept != 0;
            #pragma unroll
            for (int r = 0; r < 16; r++) {
                const long f = fe0 + r * FE_STEP;
                if (f < a.F) {
                    float c = (float)(0.0 + ac[r] * rs);            // (0.0 + x: the sibling's `old + x` on a zeroed output)
                    const float sv = (float)(0.0 + as[r] * rs);
                    if (icpt && f == 0) c = 1.0f;
                    *reinterpret_cast<float2 *>(crow + 2 * f) = make_float2(c, sv);
                }
            }
        } else {
            double *orow = a.out + i * 2 * a.F;
            #pragma unroll
            for (int r = 0; r < 16; r++) {
                const long f = fe0 + r * FE_STEP;
                if (f < a.F) {
                    double2 *o = reinterpret_cast<double2 *>(orow + 2 * f);
                    double2 old = *o;
                    old.x += ac[r] * rs;
                    old.y += as[r] * rs;
                    *o = old;
                }
            }
        }
    }
}

template <int LOG2P, int MODE>
__global__ __launch_bounds__(256, conv_min_blocks(LOG2P, MODE)) void wave_conv_kernel(WaveArgs a) {
    DenseWindows<LOG2P> win;
    wave_conv_body<LOG2P, MODE>(a, win);
}

// the token forms (xgpr_conv_token_rows_f32 / xgpr_conv_token_grad_rows_f32 / xgpr_conv_token_maxpool_f32: MODE CONV_ROWS /
// CONV_GRAD_ROWS / CONV_MAXPOOL).  a.x is the table [vocab, kmer_stride] -- sigma-scaled for the feature rows, unscaled for the gradient
// rows and the max-pool, as x is --, a.tokens the uint8 [n, row_stride] array, a.d = conv_width * kmer_stride.  The workgroup copies the table into LDS once, with one 0.0f behind it, before any wave leaves.
// Windows of 512 / 1024 elements: the dense feature rows sit exactly at the 168 registers of three waves per SIMD, and the token form
// holds 8 / 16 index registers more through the loop -- bound to three waves it spills 6 / 30 registers to scratch; it is built for two.
constexpr int conv_tok_min_blocks(int LOG2P, int MODE) {
    return (MODE == CONV_ROWS && LOG2P >= 9) ? 2 : conv_min_blocks(LOG2P, MODE);
}

template <int LOG2P, int MODE>
__global__ __launch_bounds__(256, conv_tok_min_blocks(LOG2P, MODE)) void wave_conv_tok_kernel(WaveArgs a) {
    static_assert(MODE == CONV_ROWS || MODE == CONV_GRAD_ROWS || MODE == CONV_MAXPOOL,
                  "token input serves the float32 row writers and the max-pool operator");
    __shared__ __attribute__((aligned(16))) float tab[TOK_TABLE_FLOATS + 4];
    const int nt = a.vocab * a.kmer_stride;             // <= TOK_TABLE_FLOATS (conv_token_rows_ok)
    for (int t = threadIdx.x; t < nt; t += 256) tab[t] = a.x[t];
    if (threadIdx.x == 0) tab[nt] = 0.0f;
    __syncthreads();
    TokenWindows<LOG2P> win;
    win.tab = reinterpret_cast<const char *>(tab);
    wave_conv_body<LOG2P, MODE>(a, win);
}

// sum of a double over the 64 lanes, returned wave-uniform.  Rows of 16 lanes are reduced with
// DPP moves (row_shr 8/4/2/1 on the two dwords + v_add_f64: short VALU chains, no LDS round
// trips); the four row totals are read out of lanes 15, 31, 47, 63 and added in a fixed order.
__device__ __forceinline__ double dpp_shr_f64(double x, const int ctrl_sel) {
    int lo = __builtin_bit_cast(int2, x).x, hi = __builtin_bit_cast(int2, x).y;
    int lo2, hi2;
    if (ctrl_sel == 8) { lo2 = __builtin_amdgcn_update_dpp(0, lo, 0x118, 0xf, 0xf, true); hi2 = __builtin_amdgcn_update_dpp(0, hi, 0x118, 0xf, 0xf, true); }
    else if (ctrl_sel == 4) { lo2 = __builtin_amdgcn_update_dpp(0, lo, 0x114, 0xf, 0xf, true); hi2 = __builtin_amdgcn_update_dpp(0, hi, 0x114, 0xf, 0xf, true); }
    else if (ctrl_sel == 2) { lo2 = __builtin_amdgcn_update_dpp(0, lo, 0x112, 0xf, 0xf, true); hi2 = __builtin_amdgcn_update_dpp(0, hi, 0x112, 0xf, 0xf, true); }
    else { lo2 = __builtin_amdgcn_update_dpp(0, lo, 0x111, 0xf, 0xf, true); hi2 = __builtin_amdgcn_update_dpp(0, hi, 0x111, 0xf, 0xf, true); }
    int2 r; r.x = lo2; r.y = hi2;
    return __builtin_bit_cast(double, r);
}

__device__ __forceinline__ double readlane_f64(double x, int l) {
    int2 t = __builtin_bit_cast(int2, x);
    int2 r;
    r.x = __builtin_amdgcn_readlane(t.x, l);
    r.y = __builtin_amdgcn_readlane(t.y, l);
    return __builtin_bit_cast(double, r);
}

__device__ __forceinline__ double wave_sum(double u) {
    // row_shr:n gives lane i the value of lane i-n (0.0 shifted in): after the four steps lane 15
    // of every row holds the row total
    u += dpp_shr_f64(u, 8);
    u += dpp_shr_f64(u, 4);
    u += dpp_shr_f64(u, 2);
    u += dpp_shr_f64(u, 1);
    return (readlane_f64(u, 15) + readlane_f64(u, 31)) + (readlane_f64(u, 47) + readlane_f64(u, 63));
}

// ---- fused CG matvec / z^T y.  A workgroup holds G datapoints in flight; datapoint slot g is
// served by nb waves, wave (g, b) owning tile b = frequencies [1024 b, 1024 b + 1024): its f64
// accumulators stay in registers for the whole launch while the workgroup strides over its
// datapoints; the vector v (MATVEC) sits in LDS as (cos, sin) pairs, shared by the G slots.
// Per datapoint: SORF -> cos/sin (registers) -> partial dot with v -> nb partials meet in LDS
// (one barrier, double-buffered) -> rank-1 update of the accumulators.  Z is never written.
// At the end every slot writes its accumulators as one slab wpart[slot, :];
// reduce_slabs_kernel adds the slabs in slot order (deterministic).
template <int LOG2P, bool MATVEC, bool TPREQ>
__global__ __launch_bounds__(512, 2) void wave_ztz_kernel(WaveArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr bool TP = TPREQ && LOG2P >= 7;
    double2 *pv = reinterpret_cast<double2 *>(smem);                       // [nb * 1024] (cos, sin) of v
    const size_t pv_bytes = MATVEC ? (size_t)a.nb * 1024 * 16 : 0;
    double *part = reinterpret_cast<double *>(smem + pv_bytes);            // [2][16]
    float *tb = reinterpret_cast<float *>(smem + pv_bytes + 256) + (threadIdx.x >> 6) * (TP ? TBUF_FLOATS : 0);
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    int b, g;
    long slot, nslots;
    if (MATVEC) {                      // workgroup = G slots x nb tiles, coupled through LDS
        b = w % a.nb; g = w / a.nb;
        slot = (long)blockIdx.x * a.G + g;
        nslots = (long)gridDim.x * a.G;
    } else {                           // independent waves: flat (slot, tile) numbering over the grid
        const long gw = (long)blockIdx.x * (blockDim.x >> 6) + w;
        b = __builtin_amdgcn_readfirstlane((int)(gw % a.nb)); g = 0;
        slot = gw / a.nb;
        nslots = ((long)gridDim.x * (blockDim.x >> 6)) / a.nb;
    }
    const long iters = (a.n + nslots - 1) / nslots;
    const long f0 = (long)b * 1024 + lane;
    cmask_t mk = as_cmask(a.masks + (long)b * 16);
    uint32_t sw[3] = {0, 0, 0};
    if constexpr (TP) load_sign_words(sw, a.masks, a.MW, b, lane);

    if (MATVEC) {
        for (long f = threadIdx.x; f < (long)a.nb * 1024; f += blockDim.x)
            pv[f] = f < a.F ? *reinterpret_cast<const double2 *>(a.vec + 2 * f) : make_double2(0.0, 0.0);
        __syncthreads();
    }
    float ch[16];
    double ac[16], as[16];
    #pragma unroll
    for (int r = 0; r < 16; r++) {
        const long f = f0 + r * 64;
        ch[r] = f < a.F ? a.chi[f] * a.chi_scale : 0.0f;
        ac[r] = 0.0; as[r] = 0.0;
    }
    // Z[:, 0] = 1 (kernel_baseclass.py:296-297): feature (f = 0, cos) is 1 / scale before scaling
    const bool icpt = a.fit_intercept && b == 0 && lane == 0;
    const double inv_scale = 1.0 / a.scale;
    const double s2 = a.scale * a.scale;
    const double2 *pw = pv + (long)b * 1024 + lane;

    float v[16];
    if (slot < a.n) wave_load<LOG2P>(v, a.x + slot * a.row_stride, a.d, lane);
    for (long it = 0; it < iters; it++) {
        const long row = it * nslots + slot;
        const bool active = row < a.n;
        float cs[16], sn[16];
        if constexpr (!TP) mk = launder(mk);
        if (active) {
            tile_sorf<LOG2P, TP>(v, mk, sw, tb, a.MW, a.nc, lane);
            #pragma unroll
            for (int r = 0; r < 16; r++) v[r] *= ch[r];
            tile_sincos(v, sn, cs);
        } else {
            #pragma unroll
            for (int r = 0; r < 16; r++) { cs[r] = 0.0f; sn[r] = 0.0f; }
        }
        // next datapoint's x: issued before the f64 work so its latency is covered
        const long nrow = row + nslots;
        if (nrow < a.n) wave_load<LOG2P>(v, a.x + nrow * a.row_stride, a.d, lane);
        const double c0 = (icpt && active) ? inv_scale : (double)cs[0];
        double u;
        if (MATVEC) {
            double u0 = 0.0, u1 = 0.0;
            {
                const double2 p = pw[0];
                u0 = __builtin_fma(c0, p.x, u0);
                u1 = __builtin_fma((double)sn[0], p.y, u1);
            }
            #pragma unroll
            for (int r = 1; r < 16; r++) {
                const double2 p = pw[r * 64];
                u0 = __builtin_fma((double)cs[r], p.x, u0);
                u1 = __builtin_fma((double)sn[r], p.y, u1);
            }
            u = wave_sum(u0 + u1);
            if (lane == 0) part[(it & 1) * 16 + w] = u;
            __syncthreads();
            double t = 0.0;
            for (int bb = 0; bb < a.nb; bb++) t += part[(it & 1) * 16 + g * a.nb + bb];
            u = t * s2;
        } else {
            u = active ? a.vec[row] * a.scale : 0.0;   // y[row] * scale
        }
        if (active) {
            ac[0] = __builtin_fma(c0, u, ac[0]);
            as[0] = __builtin_fma((double)sn[0], u, as[0]);
            #pragma unroll
            for (int r = 1; r < 16; r++) {
                ac[r] = __builtin_fma((double)cs[r], u, ac[r]);
                as[r] = __builtin_fma((double)sn[r], u, as[r]);
            }
        }
    }
    double *slab = a.wpart + slot * 2 * a.F;
    #pragma unroll
    for (int r = 0; r < 16; r++) {
        const long f = f0 + r * 64;
        if (f < a.F) {
            double2 *o = reinterpret_cast<double2 *>(slab + 2 * f);
            double2 val = make_double2(ac[r], as[r]);
            if (a.add_to_slab) { const double2 old = *o; val.x += old.x; val.y += old.y; }
            *o = val;
        }
    }
}

