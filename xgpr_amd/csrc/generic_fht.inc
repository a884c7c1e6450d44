// generic_fht.inc -- part of xgpr_hip.hip (included inside its anonymous namespace, in order): any-width LDS path: bare FHT / SRHT, fused SRHT + sample, generic SORF operators.
// ------------------------------------------------------------------------------------
// generic (any width) path: one workgroup per transform, butterflies in LDS.
// Used for P > 1024, for double precision, for the gradient ops and as the bare FHT / SRHT.
// ------------------------------------------------------------------------------------

// In-place FHT of every aligned P-block of buf[0:len) (len a multiple of P), stages in the
// reference's order h = 1, 2, 4, ...; two stages per barrier (radix-4 pass = stage h then
// stage 2h with identical operand pairing, so every rounding matches the radix-2 chain).
template <typename T>
__device__ __forceinline__ void lds_fht(T *buf, int len, int P, int tid, int nt) {
    int h = 1;
    for (; (h << 1) < P; h <<= 2) {
        for (int idx = tid; idx < (len >> 2); idx += nt) {
            int lo = idx & (h - 1);
            int j = ((idx - lo) << 2) | lo;
            T a = buf[j], b = buf[j + h], c = buf[j + 2 * h], d = buf[j + 3 * h];
            T ab = a + b, amb = a - b, cd = c + d, cmd = c - d;
            buf[j] = ab + cd;
            buf[j + h] = amb + cmd;
            buf[j + 2 * h] = ab - cd;
            buf[j + 3 * h] = amb - cmd;
        }
        __syncthreads();
    }
    if (h < P) {
        for (int idx = tid; idx < (len >> 1); idx += nt) {
            int lo = idx & (h - 1);
            int j = ((idx - lo) << 1) | lo;
            T a = buf[j], b = buf[j + h];
            buf[j] = a + b;
            buf[j + h] = a - b;
        }
        __syncthreads();
    }
}

// bare FHT / SRHT over a flat array of `total` elements made of vectors of length P.
// Each workgroup owns CH consecutive elements (CH a multiple of P, or CH < P when P exceeds
// the LDS capacity, in which case the stages h >= CH are finished by global_stage_kernel).
template <typename T, bool SRHT>
__global__ void generic_fht_kernel(T *x, const int8_t *__restrict__ radem, long total, int P, int CH, T nc) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T *buf = reinterpret_cast<T *>(smem);
    const int tid = threadIdx.x, nt = blockDim.x;
    const long base = (long)blockIdx.x * CH;
    for (int e = tid; e < CH; e += nt) {
        long idx = base + e;
        T val = idx < total ? x[idx] : (T)0;
        if (SRHT && idx < total) val *= radem[idx & (long)(P - 1)] * nc;
        buf[e] = val;
    }
    __syncthreads();
    lds_fht<T>(buf, CH, P < CH ? P : CH, tid, nt);
    for (int e = tid; e < CH; e += nt) {
        long idx = base + e;
        if (idx < total) x[idx] = buf[e];
    }
}

// SRHT of each row of z[n, m] (zero padded to P) followed by the column sample, out of place:
// out[i, c] = FHT(z_i * radem * nc)[sampler[c]], c < ncols (srht_compressor.py:87-97, where the
// reference pads, transforms the whole chunk in place and then gathers).  A workgroup walks rows
// blockIdx.x, blockIdx.x + gridDim.x, ...; each row is read once and only ncols of the P transformed
// values are written.  With y != nullptr the same read also accumulates the chunk's z^T y
// (rand_nys_constructors.py:115) -- thread t keeps the columns t, t + nt, ... in registers and the
// workgroup's partial sums go to zty_part[blockIdx.x, m] for an ordered reduction.
constexpr int SRHT_ZTY_COLS = 16;      // columns per thread: P <= 16 * blockDim

template <typename T>
__global__ void srht_sample_kernel(const T *__restrict__ z, const int8_t *__restrict__ radem,
                                   const long *__restrict__ sampler, T *out, const double *__restrict__ y,
                                   double *zty_part, long n, long m, int P, long ncols, long ldo, T nc) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T *buf = reinterpret_cast<T *>(smem);
    const int tid = threadIdx.x, nt = blockDim.x;
    double acc[SRHT_ZTY_COLS];
    #pragma unroll
    for (int q = 0; q < SRHT_ZTY_COLS; q++) acc[q] = 0.0;
    for (long row = blockIdx.x; row < n; row += gridDim.x) {
        const T *zr = z + row * m;
        const double yi = y ? y[row] : 0.0;
        #pragma unroll
        for (int q = 0; q < SRHT_ZTY_COLS; q++) {
            const int e = tid + q * nt;
            if (e < P) {
                const T v = e < m ? zr[e] : (T)0;
                acc[q] = __builtin_fma(yi, (double)v, acc[q]);
                buf[e] = v * (radem[e] * nc);
            }
        }
        __syncthreads();
        lds_fht<T>(buf, P, P, tid, nt);
        T *orow = out + row * ldo;
        for (long c = tid; c < ncols; c += nt) orow[c] = buf[sampler[c]];
        __syncthreads();                 // buf is rewritten for the next row
    }
    if (y) {
        double *slab = zty_part + (long)blockIdx.x * m;
        #pragma unroll
        for (int q = 0; q < SRHT_ZTY_COLS; q++) {
            const int e = tid + q * nt;
            if (e < m) slab[e] = acc[q];
        }
    }
}

// one butterfly stage of stride h straight in global memory (only for P > LDS capacity)
template <typename T>
__global__ void global_stage_kernel(T *x, long npairs, long h) {
    long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= npairs) return;
    long lo = idx & (h - 1);
    long j = ((idx - lo) << 1) | lo;
    T a = x[j], b = x[j + h];
    x[j] = a + b;
    x[j + h] = a - b;
}

// MODE_RBF_CACHE: the float32 feature cache rows (xgpr_rbf_feature_cache_f32) -- (cos, sin) before scaling, the values MODE_RBF
// widens and multiplies by its constant (T = float only)
// MODE_CONV_ROWS: the float32 feature rows of the sequence kernels (xgpr_conv_feature_rows_f32) on the wave tiles of wave_tile.inc --
// MODE_CONV's sums started from zero, rounded once and stored as float32.  This kernel does not take the mode: it keeps its sums in the
// float64 output between k-mers, so the any-width windows stage MODE_CONV through a float64 slice and round (launchers.inc).
// MODE_CONV_GRAD_ROWS: the float32 feature and gradient rows of the sequence kernels (xgpr_conv_grad_rows_f32), MODE_CONV_GRAD's sums
// rounded once into outf / gradf -- on the wave tiles only, as MODE_CONV_ROWS; the any-width windows stage MODE_CONV_GRAD and round.
enum { MODE_RBF = 0, MODE_RBF_GRAD = 1, MODE_CONV = 2, MODE_CONV_GRAD = 3, MODE_MAXPOOL = 4, MODE_RBF_CACHE = 5, MODE_CONV_ROWS = 6,
       MODE_CONV_GRAD_ROWS = 7 };

template <typename T> struct SorfArgs {
    const T *x; double *out; double *grad; float *outf;
    const int8_t *radem; const T *chi; const int32_t *seqlen;
    long n; long row_stride; long F; long R;
    int d;            // elements copied per transform (input width, or conv_width * C)
    int kmer_stride;  // C for the conv ops
    int conv_width; int P; int reps; int scaling_type;
    T nc; double scale; double sigma;
    T *scratch;       // GLOBALBUF only: one P-element buffer per workgroup, in global memory
    int fit_intercept;   // the float32 row modes only: column 0 of every row is 1.0f (0.0f in the gradient rows)
    int grad_split;      // wave_tile_rbf_kernel<.., GRAD>: grad is only 8-byte aligned, its (-sin, cos) pairs go out as two 8-byte stores
    float *gradf;        // wave_tile_rbf_grad_rows_kernel, MODE_CONV_GRAD_ROWS: the float32 gradient rows (the feature rows go to outf)
};

// one workgroup per (datapoint i = blockIdx.x, repeat k = blockIdx.y); for the conv ops the
// k-mer loop runs inside the workgroup in the reference's order (j ascending), each thread
// owning its output elements, so the f64 accumulation order equals the reference's.
template <typename T, int MODE, bool GLOBALBUF>
__global__ void generic_sorf_kernel(SorfArgs<T> a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // widths beyond the LDS capacity (P > 32768 float / 16384 double) run the same code on a
    // per-workgroup buffer in global memory (__syncthreads orders it at workgroup scope)
    T *buf = GLOBALBUF ? a.scratch + (long)blockIdx.x * a.P : reinterpret_cast<T *>(smem);
    const int tid = threadIdx.x, nt = blockDim.x;
    const int P = a.P;
    constexpr bool CONVLIKE = (MODE == MODE_CONV || MODE == MODE_CONV_GRAD || MODE == MODE_MAXPOOL);
  for (long item = blockIdx.x; item < a.n * a.reps; item += gridDim.x) {
    const long i = item / a.reps;
    const int k = (int)(item % a.reps);
    int nk = 1;
    double rs = a.scale;
    if (CONVLIKE) {
        nk = a.seqlen[i] - a.conv_width + 1;
        if (MODE != MODE_MAXPOOL) {
            if (a.scaling_type == 1) rs = a.scale / sqrt((double)nk);
            else if (a.scaling_type == 2) rs = a.scale / (double)nk;
        }
    }
    const int out0 = k * P;
    long endp = a.F < (long)(k + 1) * P ? a.F : (long)(k + 1) * P;
    const int cnt = (int)(endp - out0);
    const int8_t *re = a.radem + out0;

    for (int j = 0; j < nk; j++) {
        const T *xe = a.x + i * a.row_stride + (long)j * a.kmer_stride;
        for (int e = tid; e < P; e += nt) buf[e] = e < a.d ? xe[e] : (T)0;
        for (int s = 0; s < 3; s++) {
            // same thread touches the same elements as in the load above / the pass below
            for (int e = tid; e < P; e += nt) buf[e] *= re[(long)s * a.R + e] * a.nc;
            __syncthreads();
            lds_fht<T>(buf, P, P, tid, nt);
        }
        for (int e = tid; e < cnt; e += nt) {
            const T chv = a.chi[out0 + e];
            if (MODE == MODE_RBF_CACHE) {
                T sn, cs;
                Math<T>::sincos(buf[e] * chv, sn, cs);
                *reinterpret_cast<float2 *>(a.outf + i * 2 * a.F + 2 * (long)(out0 + e)) = make_float2((float)cs, (float)sn);
            } else if (MODE == MODE_RBF || MODE == MODE_CONV) {
                T prod = buf[e] * chv;
                T sn, cs;
                Math<T>::sincos(prod, sn, cs);
                double *o = a.out + i * 2 * a.F + 2 * (long)(out0 + e);
                if (MODE == MODE_RBF) {
                    double2 val = make_double2(cs * rs, sn * rs);
                    *reinterpret_cast<double2 *>(o) = val;
                } else {
                    o[0] += cs * rs;
                    o[1] += sn * rs;
                }
            } else if (MODE == MODE_RBF_GRAD || MODE == MODE_CONV_GRAD) {
                // shared_rfgen_ops.cpp:140-155, including the roundings back to T
                T grad_val = buf[e] * chv;
                T prod_val = (T)(grad_val * a.sigma);
                T sn, cs;
                Math<T>::sincos(prod_val, sn, cs);
                T cos_val = (T)(cs * rs);
                T sin_val = (T)(sn * rs);
                double *o = a.out + i * 2 * a.F + 2 * (long)(out0 + e);
                double *g = a.grad + i * 2 * a.F + 2 * (long)(out0 + e);
                T gs = sin_val * grad_val, gc = cos_val * grad_val;
                if (MODE == MODE_RBF_GRAD) {
                    o[0] = cos_val; o[1] = sin_val;
                    g[0] = -(double)gs; g[1] = gc;
                } else {
                    o[0] += cos_val; o[1] += sin_val;
                    g[0] -= gs; g[1] += gc;
                }
            } else {  // MODE_MAXPOOL: conv1d_operations.cpp:160-166
                float prod = (float)(buf[e] * chv);
                float *o = a.outf + i * a.F + out0 + e;
                float old = *o;
                *o = old > prod ? old : prod;
            }
        }
        __syncthreads();
    }
  }
}

