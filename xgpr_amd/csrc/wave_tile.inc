// wave_tile.inc -- part of xgpr_hip.hip (included inside its anonymous namespace, in order): wave tiles IN THE INPUT TYPE T (float or double),
// transform in registers + one wave-private LDS image per wave, for the operators the float32 kernels of wave_sorf.inc / fused_ztz.inc do
// not serve:
//   wave_tile_rbf_kernel<T, LOG2P, GRAD>   cudaRBFFeatureGen / cudaRBFGrad -- T = double: every padded width 2 <= P <= 8192
//                                          (xgpr_rbf_feature_gen_f64, xgpr_rbf_grad_f64: the double_precision = True kernels,
//                                          kernel_baseclass.py:278-285); T = float: the gradient at 2048 <= P <= 8192, the features at P = 8192
//   wave_tile_conv_kernel<T, LOG2P, MODE>  cudaConv1dFGen / cudaConvGrad / cudaConv1dMaxpool -- T = double: every padded window up to 4096;
//                                          T = float: windows of 2048 / 4096 elements
// (row drivers rbf_ops.cpp:27-221, rbf_convolution.cpp:23-282, conv1d_operations.cpp:23-168; SORF shared_rfgen_ops.cpp:51-78 with every
// product and sum in T).  Rounds 1-5 sent all of these through generic_sorf_kernel -- one workgroup per transform, radix-4 passes through
// LDS with a workgroup barrier each: the float64 feature operator took 1.53 ms per 32768 x 8192 rows, of which the double-precision cos/sin
// are only 0.26 (profiles/r6_f64_op_ab.txt).  Here one wave holds 1024 consecutive frequencies of a datapoint as 16 elements per lane and
// alternates, as the float32 kernels do (wave_sorf.inc), between
//   layout R (lane = t[9:4], register = t[3:0]): strides 1 .. 8 register-local, 16 and 32 = lane bits 0, 1 (quad_perm DPP -- on both halves
//            of a double -- with the butterfly as ONE fused multiply-add by +-1: exact product, one rounding -- the add / subtract bit for bit), and
//   layout C (lane = t[5:0], register = t[9:6]): strides 64 .. 512 register-local; also the layout of the coalesced stores,
// through a wave-private LDS image of rows of 16 elements at a pitch of 18 (double: 144 bytes -- the 16-byte stores of layout R are
// conflict-free, the 8-byte accesses of layout C share two of 64 banks).  Inside a tile no barrier: a wave's LDS operations execute in
// order.  Stage order h = 1, 2, 4, ... and `x *= radem * norm` per round exactly as the reference (no folding of the normaliser), so the
// argument of every cos / sin is bit-identical to the reference's in T.  cos / sin: double -- sincos_f64_fast (common.inc) below 2^20, the
// library's sincos beyond; float -- the any-width path's form.  XGPR_F64_PLAN=generic in the environment sends every shape of this file back
// to the any-width path (A/B timing).
// ------------------------------------------------------------------------------------
constexpr int W64_PITCH = 18;
constexpr int W64_DOUBLES = 64 * W64_PITCH;        // elements per wave image: 9216 bytes in double, 4608 in float

template <typename T> struct Pair2;
template <> struct Pair2<double> { using type = double2; };
template <> struct Pair2<float> { using type = float2; };

__device__ __forceinline__ double dpp_quad(double x, const int sel) {      // sel 1: lane ^ 1, sel 2: lane ^ 2 (inside a quad)
    const int2 t = __builtin_bit_cast(int2, x);
    int2 r;
    if (sel == 1) { r.x = __builtin_amdgcn_update_dpp(0, t.x, 0xB1, 0xf, 0xf, true); r.y = __builtin_amdgcn_update_dpp(0, t.y, 0xB1, 0xf, 0xf, true); }
    else { r.x = __builtin_amdgcn_update_dpp(0, t.x, 0x4E, 0xf, 0xf, true); r.y = __builtin_amdgcn_update_dpp(0, t.y, 0x4E, 0xf, 0xf, true); }
    return __builtin_bit_cast(double, r);
}
__device__ __forceinline__ float dpp_quad(float x, const int sel) {
    const int t = __builtin_bit_cast(int, x);
    const int r = sel == 1 ? __builtin_amdgcn_update_dpp(0, t, 0xB1, 0xf, 0xf, true) : __builtin_amdgcn_update_dpp(0, t, 0x4E, 0xf, 0xf, true);
    return __builtin_bit_cast(float, r);
}

__device__ __forceinline__ double fma_t(double x, double y, double z) { return __builtin_fma(x, y, z); }
__device__ __forceinline__ float fma_t(float x, float y, float z) { return __builtin_fmaf(x, y, z); }

template <int Q, typename T> __device__ __forceinline__ void bfly_regs(T (&v)[16]) {
    #pragma unroll
    for (int j = 0; j < 16; j++)
        if (!(j & Q)) { const T s = v[j] + v[j + Q], d = v[j] - v[j + Q]; v[j] = s; v[j + Q] = d; }
}

// Padded widths 2048 ... 8192 (round 6): a transform is NW = P / 1024 wave tiles held by NW waves of ONE workgroup (wave wv: tile wv mod NW;
// workgroups of four waves hold 4 / NW whole transforms at NW <= 4, a workgroup of 8 waves one transform at P = 8192 -- the fixed-vector operators only: the convolution kernels' accumulators do not fit beside it).  Strides 1024 and 2048 pair the same (lane, register) of different waves:
// they ride on the layout change back to R -- a wave reads the rows of ALL its transform's images and forms lower + upper / lower - upper
// (one fma with a wave-uniform +-1 per stage, rounded per stage as the reference's two separate stages are) -- and, in the last
// round, on a flat layout-C exchange.  The images are wave-private at every other point, so the orderings are two workgroup barriers around
// each cross read (five per transform); all LDS traffic here is plain C++, so the compiler's own waits before s_barrier are complete.
// Padded widths below 64: a tile is 1024 / P whole transforms, the strides stop at P / 2.
constexpr int wt_waves(int log2p) { return log2p > 12 ? (1 << (log2p - 10)) : 4; }      // waves per workgroup: 4, or one whole transform (8)

template <typename T, int LOG2P> struct WaveTile {
    static_assert(LOG2P >= 1 && LOG2P <= 13, "wave tiles in registers + LDS image: 2 <= P <= 8192 (sixteen waves per transform leave 128 registers per lane: spills)");
    using T2 = typename Pair2<T>::type;
    static constexpr int P = 1 << LOG2P;
    static constexpr int NW = P > 1024 ? P / 1024 : 1;                             // waves (tiles) per transform: 1, 2, 4, 8
    static constexpr int LOGNW = LOG2P > 10 ? LOG2P - 10 : 0;
    static constexpr bool WIDE = NW > 1;
    static constexpr int WAVES = wt_waves(LOG2P);
    static constexpr size_t LDS_BYTES = (size_t)WAVES * W64_DOUBLES * sizeof(T);
    int lane, tp;
    T *tb, *rrow, *ccol;
    const T *tg;
    T sx[4], sg1, sg2;
    __device__ __forceinline__ WaveTile(T *tbuf, int wv, int lane_) : lane(lane_), tp(wv & (NW - 1)) {
        tb = tbuf + wv * W64_DOUBLES;
        tg = tbuf + (wv & ~(NW - 1)) * W64_DOUBLES;                              // image of the transform's tile 0
        rrow = tb + lane * W64_PITCH;                                            // layout R: this lane's row of 16
        ccol = tb + (lane >> 4) * W64_PITCH + (lane & 15);                       // layout C: register r at + 4 r rows
        #pragma unroll
        for (int k = 0; k < 4; k++) sx[k] = ((tp >> k) & 1) ? (T)-1 : (T)1;      // stride 1024 << k: this tile is the upper / lower one
        sg1 = (lane & 1) ? (T)-1 : (T)1; sg2 = (lane & 2) ? (T)-1 : (T)1;
    }
    __device__ __forceinline__ void to_cols(T (&v)[16]) const {
        #pragma unroll
        for (int r = 0; r < 16; r += 2) { T2 t; t.x = v[r]; t.y = v[r + 1]; *reinterpret_cast<T2 *>(rrow + r) = t; }
        wave_lds_sync();
        #pragma unroll
        for (int r = 0; r < 16; r++) v[r] = ccol[4 * r * W64_PITCH];
        wave_lds_sync();
    }
    __device__ __forceinline__ void to_rows(T (&v)[16]) const {
        #pragma unroll
        for (int r = 0; r < 16; r++) ccol[4 * r * W64_PITCH] = v[r];
        wave_lds_sync();
        #pragma unroll
        for (int r = 0; r < 16; r += 2) { const T2 t = *reinterpret_cast<const T2 *>(rrow + r); v[r] = t.x; v[r + 1] = t.y; }
        wave_lds_sync();
    }
    // strides 1024 .. P / 2 of a wide transform at this lane's offset `off` of each image.  Stage k pairs tiles that differ in bit k; the
    // tiles this one meets in LATER stages share its lower bits, so their stage-k values are lower + upper / lower - upper with THIS
    // tile's sign: t[u] <- t[2u] +- t[2u + 1] level by level (NW - 1 fused multiply-adds by +-1, each rounded as the reference's stage is),
    // t[0] ends as this tile's value.  NW = 4: (tile 0 +- tile 1) +- (tile 2 +- tile 3).
    __device__ __forceinline__ void cross(T (&v)[16], const int off, const int step) const {
        #pragma unroll
        for (int r = 0; r < 16; r++) {
            const T *q = tg + off + r * step;
            T t[NW];
            #pragma unroll
            for (int u = 0; u < NW; u++) t[u] = q[u * W64_DOUBLES];
            #pragma unroll
            for (int k = 0; k < LOGNW; k++) {
                #pragma unroll
                for (int u = 0; u < (NW >> (k + 1)); u++) t[u] = fma_t(t[2 * u + 1], sx[k], t[2 * u]);
            }
            v[r] = t[0];
            if constexpr (NW >= 8) { if ((r & 1) == 1) __builtin_amdgcn_sched_barrier(0); }      // (2 x NW reads in flight, not 16 x NW: registers)
        }
    }
    __device__ __forceinline__ void to_rows_cross(T (&v)[16]) const {
        #pragma unroll
        for (int r = 0; r < 16; r++) ccol[4 * r * W64_PITCH] = v[r];
        __syncthreads();
        cross(v, lane * W64_PITCH, 1);
        __syncthreads();
    }
    // layout R: tile element 16 l + r is element (1024 tp + 16 l + r) mod P of the zero-padded row / window (rbf_ops.cpp:86-92)
    __device__ __forceinline__ void load(T (&v)[16], const T *xrow, const int d) const {
        int e0 = (1024 * tp + 16 * lane) & (P - 1);
        asm volatile("" : "+v"(e0));      // (inside a k-mer loop: sixteen offsets and sixteen bounds predicates are recomputed rather than held)
        #pragma unroll
        for (int r = 0; r < 16; r++) { const int e = (e0 + r) & (P - 1); const T t = xrow[e < d ? e : 0]; v[r] = e < d ? t : (T)0; }
    }
    // sixteen int8 signs of each diagonal in one 16-byte load; beyond the diagonal's length (a tile's last transforms when
    // R < 1024 (b + 1): frequencies that are never written) the sign is +1
    __device__ __forceinline__ void load_signs(int4 (&rw)[3], const int8_t *radem, const long R, const int b) const {
        const long t0 = (long)b * 1024 + 16 * lane;                               // this lane's first diagonal element (a multiple of 16; R % 64 == 0)
        #pragma unroll
        for (int s = 0; s < 3; s++) {
            rw[s] = make_int4(0x01010101, 0x01010101, 0x01010101, 0x01010101);
            if (t0 < R) rw[s] = *reinterpret_cast<const int4 *>(radem + (long)s * R + t0);
        }
    }
    // the three rounds of singleVectorSORF (shared_rfgen_ops.cpp:51-78) on a tile in layout R; leaves it in layout C
    __device__ __forceinline__ void sorf(T (&v)[16], const int4 (&rw)[3], const T nc) const {
        #pragma unroll
        for (int s = 0; s < 3; s++) {
            const int words[4] = {rw[s].x, rw[s].y, rw[s].z, rw[s].w};
            #pragma unroll
            for (int r = 0; r < 16; r++) {                                        // x *= radem * norm (shared_rfgen_ops.cpp:54-63)
                const int sgn = (int)(signed char)((words[r >> 2] >> (8 * (r & 3))) & 0xff);
                v[r] *= (T)sgn * nc;
            }
            bfly_regs<1>(v);
            if constexpr (P > 2) bfly_regs<2>(v);
            if constexpr (P > 4) bfly_regs<4>(v);
            if constexpr (P > 8) bfly_regs<8>(v);
            if constexpr (P > 16) {
                #pragma unroll
                for (int r = 0; r < 16; r++) v[r] = fma_t(v[r], sg1, dpp_quad(v[r], 1));      // stride 16: lower lane v + p, upper p - v
            }
            if constexpr (P > 32) {
                #pragma unroll
                for (int r = 0; r < 16; r++) v[r] = fma_t(v[r], sg2, dpp_quad(v[r], 2));      // stride 32
            }
            if constexpr (P > 64) {
                to_cols(v);
                bfly_regs<1>(v);
                if constexpr (P > 128) bfly_regs<2>(v);
                if constexpr (P > 256) bfly_regs<4>(v);
                if constexpr (P > 512) bfly_regs<8>(v);
                if constexpr (WIDE) {
                    if (s < 2) to_rows_cross(v);
                    else {                                                        // last round: stay in layout C (register r at 64 r + lane)
                        #pragma unroll
                        for (int r = 0; r < 16; r++) tb[64 * r + lane] = v[r];
                        __syncthreads();
                        cross(v, lane, 64);
                    }
                } else if (s < 2) to_rows(v);
            }
        }
        if constexpr (P <= 64) to_cols(v);
    }
};

// cos / sin of a tile's arguments in T: double -- sincos_f64_fast below 2^20, the library's beyond (one wave-level test: tile_has_big);
// float -- the any-width path's form (Math<float>)
template <typename T> __device__ __forceinline__ bool tile_has_big(const T (&v)[16]) {
    if constexpr (sizeof(T) == 8) {
        double amax = 0.0;
        #pragma unroll
        for (int r = 0; r < 16; r++) amax = __builtin_fmax(amax, __builtin_fabs(v[r]));      // (a NaN drops out of the maximum: the fast form returns NaN for it too)
        return __any(!(amax < SINCOS64_FAST_LIMIT));
    } else return false;
}
template <typename T> __device__ __forceinline__ void elem_sincos(const T x, const bool big, T &sn, T &cs) {
    if constexpr (sizeof(T) == 8) {
#ifdef XGPR_ABL_F64_LIBSINCOS
        Math<double>::sincos(x, sn, cs);
#else
        sincos_f64_fast(x, sn, cs);
        if (__builtin_expect(big, 0)) {
            if (!(__builtin_fabs(x) < SINCOS64_FAST_LIMIT)) Math<double>::sincos(x, sn, cs);
        }
#endif
    } else Math<T>::sincos(x, sn, cs);
}

// The front of the fixed-vector operators on wave tiles, ONE copy for wave_tile_rbf_kernel and wave_tile_rbf_cache_kernel (the cache's
// bit-for-bit contract with the feature operator rests on it): this wave's (datapoint i, tile b), the tile's SORF and the products
// with chi -- on return v[r] = prodVal of frequency 1024 b + 64 r + lane (layout C; shared_rfgen_ops.cpp:107).  Returns false for a
// wave past the last item: a narrow transform returns before any work, a wide one repeats a live item (the workgroup's barriers; the
// caller stores nothing for it).
template <typename T, int LOG2P>
__device__ __forceinline__ bool wt_rbf_front(const SorfArgs<T> &a, T *tbuf, T (&v)[16], long &i, int &b) {
    using WT = WaveTile<T, LOG2P>;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    long item = wv + (long)blockIdx.x * WT::WAVES;
    // wide transforms: every tile of the diagonal's length is computed (R is a multiple of P), the ones past F just store nothing
    const int nb = WT::WIDE ? (int)(a.R >> 10) : (int)((a.F + 1023) >> 10);
    const bool live = item < a.n * nb;
    if constexpr (!WT::WIDE) { if (!live) return false; }
    else if (!live) item -= 2;            // NW == 2, n * nb = 2 mod 4: the last workgroup's spare pair repeats the live pair (barriers; no stores)
    i = item / nb;
    b = __builtin_amdgcn_readfirstlane((int)(item % nb));
    const WT wt(tbuf, wv, lane);
    int4 rw[3];
    wt.load(v, a.x + i * a.row_stride, a.d);
    wt.load_signs(rw, a.radem, a.R, b);
    wt.sorf(v, rw, a.nc);
    #pragma unroll
    for (int r = 0; r < 16; r++) {
        const long f = (long)b * 1024 + 64 * r + lane;
        v[r] *= a.chi[f < a.F ? f : 0];                       // prodVal = xdata[i] * chiIn[i] (shared_rfgen_ops.cpp:107)
    }
    return live;
}

// T = double: the float64 feature operator (GRAD false) and the float64 gradient operator (GRAD true: cudaRBFGrad, rbf_ops.cpp:112-189,
// shared_rfgen_ops.cpp:140-155 with its roundings back to T).  T = float, GRAD true: the float32 gradient operator at padded widths
// 2048 / 4096 / 8192 (up to 1024 it runs on wave_rbf_kernel<LOG2P, OUT_GRAD>, the feature operator up to 4096 on ztz3_kernel's feature modes).
// wave_tile_rbf_grad_rows_kernel below repeats the GRAD branch for T = float with a float2 epilogue and is bit-for-bit bound to it
// (xgpr_rbf_grad_rows_f32): a change to the GRAD arithmetic here is made there too.
template <typename T, int LOG2P, bool GRAD>
__global__ __launch_bounds__(wt_waves(LOG2P) * 64) void wave_tile_rbf_kernel(SorfArgs<T> a) {
    using WT = WaveTile<T, LOG2P>;
    static_assert(GRAD || sizeof(T) == 8 || LOG2P > 12, "the float32 feature operator up to P = 4096 runs on ztz3_kernel's feature modes");
    extern __shared__ __attribute__((aligned(16))) unsigned char wt_lds[];            // WT::LDS_BYTES (one image per wave)
    T *tbuf = reinterpret_cast<T *>(wt_lds);
    const int lane = threadIdx.x & 63;
    T v[16];
    long i;
    int b;
    const bool live = wt_rbf_front<T, LOG2P>(a, tbuf, v, i, b);
    if constexpr (!WT::WIDE) { if (!live) return; }
    // layout C: register r of lane l is frequency 1024 b + 64 r + l -- one store instruction writes 64 consecutive (cos, sin) pairs
    double *orow = a.out + i * 2 * a.F;
    if constexpr (GRAD) {
        // (repeated in wave_tile_rbf_grad_rows_kernel: keep the two in step)
        // cudaRBFGrad (shared_rfgen_ops.cpp:140-155): the input is not pre-multiplied by sigma; every product is rounded back to T; the
        // scale is a double constant (rbf_ops.cpp:180-185)
        double *grow = a.grad + i * 2 * a.F;
        T pv[16];
        #pragma unroll
        for (int r = 0; r < 16; r++) pv[r] = (T)(v[r] * a.sigma);
        const bool big = tile_has_big(pv);
        #pragma unroll
        for (int r = 0; r < 16; r++) {
            const long f = (long)b * 1024 + 64 * r + lane;
            const T grad_val = v[r];
            T sn, cs;
            elem_sincos(pv[r], big, sn, cs);
            const T cos_val = (T)(cs * a.scale), sin_val = (T)(sn * a.scale);
            const T gs = sin_val * grad_val, gc = cos_val * grad_val;
            if (f < a.F && live) {
                *reinterpret_cast<double2 *>(orow + 2 * f) = make_double2(cos_val, sin_val);
                if (a.grad_split) { grow[2 * f] = -(double)gs; grow[2 * f + 1] = gc; }
                else *reinterpret_cast<double2 *>(grow + 2 * f) = make_double2(-(double)gs, gc);
            }
        }
    } else {
        const bool big = tile_has_big(v);
        #pragma unroll
        for (int r = 0; r < 16; r++) {
            const long f = (long)b * 1024 + 64 * r + lane;
            T sn, cs;
            elem_sincos(v[r], big, sn, cs);
            if (f < a.F && live) *reinterpret_cast<double2 *>(orow + 2 * f) = make_double2(cs * a.scale, sn * a.scale);
        }
    }
}

// The float32 feature cache rows (xgpr_rbf_feature_cache_f32) at P = 8192: the transform of wave_tile_rbf_kernel<float, 13, false>, the
// (cos, sin) pairs stored as float32 BEFORE scaling -- the values that kernel widens and multiplies by its constant -- into outf[i, 2 f ..].
template <int LOG2P>
__global__ __launch_bounds__(wt_waves(LOG2P) * 64) void wave_tile_rbf_cache_kernel(SorfArgs<float> a) {
    using WT = WaveTile<float, LOG2P>;
    static_assert(WT::WIDE, "the cache rows up to P = 4096 run on ztz3_kernel's feature modes");
    extern __shared__ __attribute__((aligned(16))) unsigned char wt_lds[];
    float *tbuf = reinterpret_cast<float *>(wt_lds);
    const int lane = threadIdx.x & 63;
    float v[16];
    long i;
    int b;
    const bool live = wt_rbf_front<float, LOG2P>(a, tbuf, v, i, b);
    float *orow = a.outf + i * 2 * a.F;
    #pragma unroll
    for (int r = 0; r < 16; r++) {
        const long f = (long)b * 1024 + 64 * r + lane;
        float sn, cs;
        elem_sincos(v[r], false, sn, cs);                     // (the feature mode's call for T = float)
        if (f < a.F && live) *reinterpret_cast<float2 *>(orow + 2 * f) = make_float2(cs, sn);
    }
}

// The float32 feature and gradient rows (xgpr_rbf_grad_rows_f32) at padded widths 2048 / 4096 / 8192: the front and the float products of
// wave_tile_rbf_kernel<float, LOG2P, true> expression for expression -- (float)(v * sigma), elem_sincos, (float)(cs * scale), sin_val *
// grad_val -- with the values that kernel widens at its double2 stores written as float2 pairs into a.outf[i, 2 f ..] (features) and
// a.gradf[i, 2 f ..] (d features / d sigma); column 0 is 1.0f / 0.0f under fit_intercept.  Complete rows, both overwritten.
template <int LOG2P>
__global__ __launch_bounds__(wt_waves(LOG2P) * 64) void wave_tile_rbf_grad_rows_kernel(SorfArgs<float> a) {
    using WT = WaveTile<float, LOG2P>;
    static_assert(WT::WIDE, "the gradient rows up to P = 1024 run on wave_rbf_kernel<LOG2P, OUT_GRAD_ROWS>");
    extern __shared__ __attribute__((aligned(16))) unsigned char wt_lds[];
    float *tbuf = reinterpret_cast<float *>(wt_lds);
    const int lane = threadIdx.x & 63;
    float v[16];
    long i;
    int b;
    const bool live = wt_rbf_front<float, LOG2P>(a, tbuf, v, i, b);
    float *zrow = a.outf + i * 2 * a.F, *grow = a.gradf + i * 2 * a.F;
    float pv[16];
    #pragma unroll
    for (int r = 0; r < 16; r++) pv[r] = (float)(v[r] * a.sigma);
    const bool big = tile_has_big(pv);                           // (false for float: the sibling's call, kept in the same form)
    const bool icpt = a.fit_intercept != 0;
    #pragma unroll
    for (int r = 0; r < 16; r++) {
        const long f = (long)b * 1024 + 64 * r + lane;
        const float grad_val = v[r];
        float sn, cs;
        elem_sincos(pv[r], big, sn, cs);
        const float cos_val = (float)(cs * a.scale), sin_val = (float)(sn * a.scale);
        const float gs = sin_val * grad_val, gc = cos_val * grad_val;
        if (f < a.F && live) {
            const bool c0 = icpt && f == 0;
            *reinterpret_cast<float2 *>(zrow + 2 * f) = make_float2(c0 ? 1.0f : cos_val, sin_val);
            *reinterpret_cast<float2 *>(grow + 2 * f) = make_float2(c0 ? 0.0f : -gs, gc);
        }
    }
}

// The convolution operators on the same tiles: one wave per (sequence, tile), the k-mers of the sequence in the reference's order (j
// ascending) with the float64 sums held in registers -- started from what the output holds and stored once, i.e. the same sequence of
// additions as `out += ...` per k-mer (rbf_convolution.cpp:23-140, :160-282; conv1d_operations.cpp:23-168).  T = double: every padded
// window width up to 4096; T = float: 2048 / 4096 (narrower float32 windows run on wave_conv_kernel).  Wide windows: the waves of a
// workgroup meet at barriers inside the k-mer loop, so every wave runs the loop to the workgroup's LONGEST sequence (a workgroup's four
// consecutive items span at most two sequences) and skips the sums past its own; six barriers per k-mer (the sixth keeps the next
// k-mer's first image write behind the partners' last flat read).
// MODE_CONV_ROWS (T = float, windows of 2048 / 4096 elements: xgpr_conv_feature_rows_f32): MODE_CONV with the sums started from 0.0 instead
// of a load of the zeroed output, rounded once to float32 and stored as (cos, sin) float2 pairs into a.outf[i, 2 f ..] -- layout C, one
// store instruction writes 64 consecutive pairs (512 bytes); column 0 is 1.0f under fit_intercept.
// MODE_CONV_GRAD_ROWS (T = float, the same windows: xgpr_conv_grad_rows_f32): MODE_CONV_GRAD with its four sums started from 0.0, rounded
// once and stored the same way into a.outf (features) and a.gradf (d features / d sigma); column 0 is 1.0f / 0.0f under fit_intercept.
template <typename T, int LOG2P, int MODE>
__global__ __launch_bounds__(wt_waves(LOG2P) * 64) void wave_tile_conv_kernel(SorfArgs<T> a) {
    using WT = WaveTile<T, LOG2P>;
    static_assert(MODE == MODE_CONV || MODE == MODE_CONV_GRAD || MODE == MODE_MAXPOOL || MODE == MODE_CONV_ROWS || MODE == MODE_CONV_GRAD_ROWS,
                  "convolution modes");
    static_assert(MODE != MODE_CONV_GRAD_ROWS || sizeof(T) == 4, "the gradient rows take float32 input");
    constexpr bool FEAT = MODE == MODE_CONV || MODE == MODE_CONV_ROWS;
    extern __shared__ __attribute__((aligned(16))) unsigned char wt_lds[];
    T *tbuf = reinterpret_cast<T *>(wt_lds);
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    long item = wv + (long)blockIdx.x * WT::WAVES;
    const int nb = WT::WIDE ? (int)(a.R >> 10) : (int)((a.F + 1023) >> 10);
    const long nitems = a.n * nb;
    bool live = item < nitems;
    if constexpr (!WT::WIDE) { if (!live) return; }
    else if (!live) item -= 2;
    const long i = item / nb;
    const int b = __builtin_amdgcn_readfirstlane((int)(item % nb));
    const int nk = a.seqlen[i] - a.conv_width + 1;
    int nk_wg = nk;
    if constexpr (WT::WIDE) {
        const long first = (long)blockIdx.x * WT::WAVES, last = first + WT::WAVES - 1 < nitems ? first + WT::WAVES - 1 : nitems - 1;
        const int k0 = a.seqlen[first / nb] - a.conv_width + 1, k1 = a.seqlen[last / nb] - a.conv_width + 1;
        nk_wg = k0 > k1 ? k0 : k1;
    }
    double rs = a.scale;
    if (MODE != MODE_MAXPOOL) {
        if (a.scaling_type == 1) rs = a.scale / sqrt((double)nk);
        else if (a.scaling_type == 2) rs = a.scale / (double)nk;
    }
    const WT wt(tbuf, wv, lane);
    int4 rw[3];
    wt.load_signs(rw, a.radem, a.R, b);
    constexpr int NACC = FEAT ? 2 : ((MODE == MODE_CONV_GRAD || MODE == MODE_CONV_GRAD_ROWS) ? 4 : 0);
    double acc[NACC > 0 ? NACC : 1][16];
    float mx[16];
    double *orow = a.out + i * 2 * a.F, *grow = a.grad + i * 2 * a.F;
    float *mrow = a.outf + i * a.F;
    #pragma unroll
    for (int r = 0; r < 16; r++) {
        const long f = (long)b * 1024 + 64 * r + lane;
        const bool in = f < a.F;
        if constexpr (MODE == MODE_MAXPOOL) mx[r] = in ? mrow[f] : 0.0f;
        else if constexpr (MODE == MODE_CONV_ROWS) { acc[0][r] = 0.0; acc[1][r] = 0.0; }
        else if constexpr (MODE == MODE_CONV_GRAD_ROWS) { acc[0][r] = 0.0; acc[1][r] = 0.0; acc[2][r] = 0.0; acc[3][r] = 0.0; }
        else {
            const double2 o = in ? *reinterpret_cast<const double2 *>(orow + 2 * f) : make_double2(0.0, 0.0);
            acc[0][r] = o.x; acc[1][r] = o.y;
            if constexpr (MODE == MODE_CONV_GRAD) {
                const double2 g = in ? *reinterpret_cast<const double2 *>(grow + 2 * f) : make_double2(0.0, 0.0);
                acc[2][r] = g.x; acc[3][r] = g.y;
            }
        }
    }
    const T *xseq = a.x + i * a.row_stride;
    for (int j = 0; j < nk_wg; j++) {
        const bool mine = j < nk;
        // (the sign words pass through an empty asm per k-mer: left visible, the 48 products `sign * norm` of the three rounds are hoisted
        // out of the loop -- 96 registers in double)
        #pragma unroll
        for (int s = 0; s < 3; s++) asm volatile("" : "+v"(rw[s].x), "+v"(rw[s].y), "+v"(rw[s].z), "+v"(rw[s].w));
        T v[16];
        wt.load(v, xseq + (long)(mine ? j : nk - 1) * a.kmer_stride, a.d);
        wt.sorf(v, rw, a.nc);
        // (chi re-read per k-mer through an offset the compiler cannot see through: sixteen L1 hits against 32 registers held across the
        // loop in double -- the float64 gradient mode at P = 4096 spilled with them)
        unsigned f0 = (unsigned)lane;
        asm volatile("" : "+v"(f0));
        #pragma unroll
        for (int r = 0; r < 16; r++) {
            const long f = (long)b * 1024 + 64 * r + f0;
            v[r] *= a.chi[f < a.F ? f : 0];
        }
        if constexpr (MODE == MODE_MAXPOOL) {
            // conv1d_operations.cpp:160-166
            #pragma unroll
            for (int r = 0; r < 16; r++) { const float prod = (float)v[r]; if (mine) mx[r] = mx[r] > prod ? mx[r] : prod; }
        } else if constexpr (FEAT) {
            const bool big = tile_has_big(v);
            #pragma unroll
            for (int r = 0; r < 16; r++) {
                T sn, cs;
                elem_sincos(v[r], big, sn, cs);
                if (mine) { acc[0][r] += cs * rs; acc[1][r] += sn * rs; }
                if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);      // (four evaluations in flight, not sixteen: the accumulators need the registers)
            }
        } else {
            // shared_rfgen_ops.cpp:140-155, including the roundings back to T
            T pv[16];
            #pragma unroll
            for (int r = 0; r < 16; r++) pv[r] = (T)(v[r] * a.sigma);
            const bool big = tile_has_big(pv);
            #pragma unroll
            for (int r = 0; r < 16; r++) {
                const T grad_val = v[r];
                T sn, cs;
                elem_sincos(pv[r], big, sn, cs);
                const T cos_val = (T)(cs * rs), sin_val = (T)(sn * rs);
                const T gs = sin_val * grad_val, gc = cos_val * grad_val;
                if (mine) { acc[0][r] += cos_val; acc[1][r] += sin_val; acc[2][r] -= gs; acc[3][r] += gc; }
                if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);
            }
        }
        if constexpr (WT::WIDE) __syncthreads();
    }
    #pragma unroll
    for (int r = 0; r < 16; r++) {
        const long f = (long)b * 1024 + 64 * r + lane;
        if (f < a.F && live) {
            if constexpr (MODE == MODE_MAXPOOL) mrow[f] = mx[r];
            else if constexpr (MODE == MODE_CONV_ROWS) {
                const float c = (a.fit_intercept && f == 0) ? 1.0f : (float)acc[0][r];
                *reinterpret_cast<float2 *>(a.outf + i * 2 * a.F + 2 * f) = make_float2(c, (float)acc[1][r]);
            } else if constexpr (MODE == MODE_CONV_GRAD_ROWS) {
                const bool c0 = a.fit_intercept && f == 0;
                *reinterpret_cast<float2 *>(a.outf + i * 2 * a.F + 2 * f) = make_float2(c0 ? 1.0f : (float)acc[0][r], (float)acc[1][r]);
                *reinterpret_cast<float2 *>(a.gradf + i * 2 * a.F + 2 * f) = make_float2(c0 ? 0.0f : (float)acc[2][r], (float)acc[3][r]);
            } else {
                *reinterpret_cast<double2 *>(orow + 2 * f) = make_double2(acc[0][r], acc[1][r]);
                if constexpr (MODE == MODE_CONV_GRAD) *reinterpret_cast<double2 *>(grow + 2 * f) = make_double2(acc[2][r], acc[3][r]);
            }
        }
    }
}
