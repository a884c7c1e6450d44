// zcache_half.inc -- part of xgpr_hip.hip (included inside its anonymous namespace, in order): the resident feature cache as IEEE binary16 rows: the packer that rounds float32 rows, and the streaming CG matvec over the packed rows.
// ---- An opt-in mode (cache_features="half"), no reference counterpart.  The streaming matvec of zcache.inc is bound by the bytes of
// the float32 rows; the same rows rounded to binary16 (round to nearest even, subnormals kept: a value moves by at most
// max(2^-11 |z|, 2^-25)) are half the bytes.  The solve then is ridge regression on the ROUNDED features -- exactly: the kernel widens every
// stored value back to float64 without error, and every product and sum is float64 as in zcache_ztz_kernel.

// float32 -> binary16 on a contiguous block of `count` values: 16-byte loads, 8-byte stores, grid-strided, the last count % 4 values one
// per thread.  Any float32 row writer of the library followed by this kernel is a source of binary16 rows.
__device__ __forceinline__ unsigned pack_f16_pair(float lo, float hi) {
    const unsigned l = __builtin_bit_cast(unsigned short, (_Float16)lo), h = __builtin_bit_cast(unsigned short, (_Float16)hi);
    return l | (h << 16);
}

__global__ __launch_bounds__(256) void rows_pack_f16_kernel(const float *__restrict__ rows, uint16_t *__restrict__ out, long count) {
    const long nq = count >> 2;
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
    const float4 *src = reinterpret_cast<const float4 *>(rows);
    uint2 *dst = reinterpret_cast<uint2 *>(out);
    long i = t;
    for (; i + 3 * stride < nq; i += 4 * stride) {           // four loads in flight per thread
        float4 v[4];
        #pragma unroll
        for (int q = 0; q < 4; q++) v[q] = src[i + q * stride];
        #pragma unroll
        for (int q = 0; q < 4; q++) dst[i + q * stride] = make_uint2(pack_f16_pair(v[q].x, v[q].y), pack_f16_pair(v[q].z, v[q].w));
    }
    for (; i < nq; i += stride) {
        const float4 v = src[i];
        dst[i] = make_uint2(pack_f16_pair(v.x, v.y), pack_f16_pair(v.z, v.w));
    }
    if (t < count - 4 * nq) out[4 * nq + t] = __builtin_bit_cast(unsigned short, (_Float16)rows[4 * nq + t]);
}

// ---- CG matvec over the binary16 cache: w = sum_i z_i (z_i . v), z_i = scale * widen(zc[i]).  Ownership, accumulation and reduction are
// zcache_ztz_kernel's (wave b of a datapoint slot owns tile b of 1024 frequencies, float64 accumulators in registers, v in LDS as float64,
// one barrier per datapoint, slabs reduced in order); num_freqs <= 8192.  What differs:
//   * a frequency is one 32-bit word (cos in the low half, sin in the high half), and a load holds FPL of them: FPL = 4 (16-byte loads:
//     num_freqs % 4 == 0 and a 16-byte-aligned base), 2 (8-byte loads: num_freqs even, 8-byte-aligned base) or 1.  Lane l, load q holds
//     frequencies 1024 b + 64 FPL q + FPL l + j, j < FPL; a row of a tile is 16 words per lane whatever FPL is.
//   * with FPL consecutive frequencies per lane the lane's reads of v would be FPL x 16 bytes apart from the next lane's: 4-way bank
//     conflicts on ds_read_b128 at FPL = 4 (a group of 16 lanes covers the 64 banks four times).  v is therefore stored in FPL planes,
//     frequency f in plane f % FPL at index f / FPL: the lanes of a wave read consecutive 16-byte entries of one plane, conflict-free.
//   * a ring entry is 16 registers instead of 32, so the same bytes in flight are twice the datapoints: RING is the launcher's choice.
struct Zc16Args {
    const uint16_t *zc; const double *vec; double *wpart;
    long n; long F; int nb; int G; int fit_intercept;
    double inv_scale, scale2;       // 1 / scale and scale^2, rounded on the host
};

__device__ __forceinline__ double zc16_lo(unsigned w) { return (double)(float)__builtin_bit_cast(_Float16, (unsigned short)(w & 0xffffu)); }
__device__ __forceinline__ double zc16_hi(unsigned w) { return (double)(float)__builtin_bit_cast(_Float16, (unsigned short)(w >> 16)); }

template <int FPL, int RING>
__global__ __launch_bounds__(512, 2) void zcache16_ztz_kernel(Zc16Args a) {
    constexpr int NL = 16 / FPL;                                                  // loads per lane and row
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double2 *pv = reinterpret_cast<double2 *>(smem);                              // [FPL][nb * 1024 / FPL] (cos, sin) of v
    double *part = reinterpret_cast<double *>(smem + (size_t)a.nb * 1024 * 16);   // [2][G][8], zero padded
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int b = w % a.nb, g = w / a.nb;
    const long slot = (long)blockIdx.x * a.G + g;
    const long nslots = (long)gridDim.x * a.G;
    const long iters = (a.n + nslots - 1) / nslots;
    const int plane = a.nb * (1024 / FPL);
    for (long f = threadIdx.x; f < (long)a.nb * 1024; f += blockDim.x)
        pv[(f % FPL) * plane + f / FPL] = f < a.F ? *reinterpret_cast<const double2 *>(a.vec + 2 * f) : make_double2(0.0, 0.0);
    if (threadIdx.x < 2 * 8 * 8) part[threadIdx.x] = 0.0;
    __syncthreads();
    const long fb = (long)b * 1024 + FPL * lane;         // first frequency of load q is fb + 64 FPL q
    const double2 *pl = pv + b * (1024 / FPL) + lane;    // word e = q FPL + j of a row meets pl[j * plane + 64 q]
    double ac[32];
    #pragma unroll
    for (int j = 0; j < 32; j++) ac[j] = 0.0;
    const bool icpt = a.fit_intercept && b == 0 && lane == 0;
    const double inv_scale = a.inv_scale, s2 = a.scale2;
    const unsigned *words = reinterpret_cast<const unsigned *>(a.zc);

    auto load_row = [&](long row, unsigned (&dst)[16]) {
        const unsigned *zr = words + row * a.F;
        #pragma unroll
        for (int q = 0; q < NL; q++) {
            const long f = fb + 64 * FPL * q;            // F % FPL == 0: a load is inside the row or outside it
            if (FPL == 4) {
                const uint4 r = f < a.F ? *reinterpret_cast<const uint4 *>(zr + f) : make_uint4(0u, 0u, 0u, 0u);
                dst[4 * q] = r.x; dst[4 * q + 1] = r.y; dst[4 * q + 2] = r.z; dst[4 * q + 3] = r.w;
            } else if (FPL == 2) {
                const uint2 r = f < a.F ? *reinterpret_cast<const uint2 *>(zr + f) : make_uint2(0u, 0u);
                dst[2 * q] = r.x; dst[2 * q + 1] = r.y;
            } else {
                dst[q] = f < a.F ? zr[f] : 0u;
            }
        }
    };
    unsigned buf[RING][16];
    #pragma unroll
    for (int k = 0; k < RING; k++) {
        #pragma unroll
        for (int e = 0; e < 16; e++) buf[k][e] = 0u;
        if (k * nslots + slot < a.n) load_row(k * nslots + slot, buf[k]);
    }
    for (long it0 = 0; it0 < iters; it0 += RING) {
        #pragma unroll
        for (int k = 0; k < RING; k++) {
            const long it = it0 + k;
            if (it >= iters) break;                      // uniform over the workgroup
            const long row = it * nslots + slot;
            const bool active = row < a.n;
            double zd[32];                               // the row widened once, for the dot product and for the update
            #pragma unroll
            for (int e = 0; e < 16; e++) { zd[2 * e] = zc16_lo(buf[k][e]); zd[2 * e + 1] = zc16_hi(buf[k][e]); }
            if (icpt) zd[0] = inv_scale;
            const long nrow = (it + RING) * nslots + slot;
            if (nrow < a.n) load_row(nrow, buf[k]);      // refill this ring entry: its words are in zd now
            double u0 = 0.0, u1 = 0.0;
            #pragma unroll
            for (int e = 0; e < 16; e++) {
                const double2 p = pl[(e % FPL) * plane + 64 * (e / FPL)];
                u0 = __builtin_fma(zd[2 * e], p.x, u0);
                u1 = __builtin_fma(zd[2 * e + 1], p.y, u1);
            }
            const double u = wave_sum(u0 + u1);
            double *pp = part + ((it & 1) * 8 + g) * 8;
            if (lane == 0) pp[b] = active ? u : 0.0;
            __syncthreads();
            const double2 t01 = *reinterpret_cast<const double2 *>(pp), t23 = *reinterpret_cast<const double2 *>(pp + 2);
            const double2 t45 = *reinterpret_cast<const double2 *>(pp + 4), t67 = *reinterpret_cast<const double2 *>(pp + 6);
            const double us = (((t01.x + t01.y) + (t23.x + t23.y)) + ((t45.x + t45.y) + (t67.x + t67.y))) * s2;
            if (active) {
                #pragma unroll
                for (int j = 0; j < 32; j++) ac[j] = __builtin_fma(zd[j], us, ac[j]);
            }
        }
    }
    double *slab = a.wpart + slot * 2 * a.F;
    #pragma unroll
    for (int e = 0; e < 16; e++) {
        const long f = fb + 64 * FPL * (e / FPL) + e % FPL;
        if (f < a.F) *reinterpret_cast<double2 *>(slab + 2 * f) = make_double2(ac[2 * e], ac[2 * e + 1]);
    }
}
