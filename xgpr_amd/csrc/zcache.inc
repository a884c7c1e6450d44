// zcache.inc -- part of xgpr_hip.hip (included inside its anonymous namespace, in order): streaming CG matvec over the resident float32 feature cache; ordered slab reduction.
// ---- CG matvec over a resident float32 feature cache: w = sum_i z_i (z_i . v) with z_i read from
// HBM instead of regenerated.  288 GB of HBM hold the cache of a whole shard (32 KB per datapoint at
// M = 8192), and streaming it is faster than regenerating the features on the vector pipe.  Same
// ownership as wave_ztz_kernel (wave b of a datapoint slot owns tile b, float64 accumulators in
// registers, v in LDS, one barrier per datapoint, slabs reduced in order).  The kernel is bound by
// bytes in flight (HBM latency under load is several microseconds), so every wave keeps a ring of
// RING datapoints in registers: RING - 1 of them loading while one is consumed.  The lane <->
// frequency map is chosen for 16-byte loads: lane l, load q holds frequencies
// f = 1024 b + 128 q + 2 l and f + 1 as (cos, sin, cos, sin).
struct ZcArgs {
    const float *zc; const double *vec; double *wpart;
    long n; long F; int nb; int G; int fit_intercept; double scale;
    double inv_scale, scale2;       // 1 / scale and scale^2, rounded on the host (kernel arguments, not registers)
};

template <bool VEC4, int RING>
__global__ __launch_bounds__(512, 2) void zcache_ztz_kernel(ZcArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double2 *pv = reinterpret_cast<double2 *>(smem);                              // [nb * 1024] (cos, sin) of v
    double *part = reinterpret_cast<double *>(smem + (size_t)a.nb * 1024 * 16);   // [2][G][8], zero padded
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int b = w % a.nb, g = w / a.nb;
    const long slot = (long)blockIdx.x * a.G + g;
    const long nslots = (long)gridDim.x * a.G;
    const long iters = (a.n + nslots - 1) / nslots;
    for (long f = threadIdx.x; f < (long)a.nb * 1024; f += blockDim.x)
        pv[f] = f < a.F ? *reinterpret_cast<const double2 *>(a.vec + 2 * f) : make_double2(0.0, 0.0);
    if (threadIdx.x < 2 * 8 * 8) part[threadIdx.x] = 0.0;
    __syncthreads();
    const long fb = (long)b * 1024 + 2 * lane;           // first frequency of load q is fb + 128 q
    double ac[32];
    #pragma unroll
    for (int j = 0; j < 32; j++) ac[j] = 0.0;
    const bool icpt = a.fit_intercept && b == 0 && lane == 0;
    const double inv_scale = a.inv_scale, s2 = a.scale2;

    auto load_row = [&](long row, float4 (&dst)[8]) {
        const float *zr = a.zc + row * 2 * a.F;
        #pragma unroll
        for (int q = 0; q < 8; q++) {
            const long f = fb + 128 * q;
            if (VEC4) {
                dst[q] = f + 1 < a.F ? *reinterpret_cast<const float4 *>(zr + 2 * f) : make_float4(0.f, 0.f, 0.f, 0.f);
            } else {
                float2 lo = f < a.F ? *reinterpret_cast<const float2 *>(zr + 2 * f) : make_float2(0.f, 0.f);
                float2 hi = f + 1 < a.F ? *reinterpret_cast<const float2 *>(zr + 2 * f + 2) : make_float2(0.f, 0.f);
                dst[q] = make_float4(lo.x, lo.y, hi.x, hi.y);
            }
        }
    };
    float4 buf[RING][8];
    #pragma unroll
    for (int k = 0; k < RING; k++) {
        #pragma unroll
        for (int q = 0; q < 8; q++) buf[k][q] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k * nslots + slot < a.n) load_row(k * nslots + slot, buf[k]);
    }
    for (long it0 = 0; it0 < iters; it0 += RING) {
        #pragma unroll
        for (int k = 0; k < RING; k++) {
            const long it = it0 + k;
            if (it >= iters) break;                      // uniform over the workgroup
            const long row = it * nslots + slot;
            const bool active = row < a.n;
            double u0 = 0.0, u1 = 0.0;
            #pragma unroll
            for (int q = 0; q < 8; q++) {
                const double2 p0 = pv[fb + 128 * q], p1 = pv[fb + 128 * q + 1];
                const double c0 = (icpt && q == 0) ? inv_scale : (double)buf[k][q].x;
                u0 = __builtin_fma(c0, p0.x, u0);
                u1 = __builtin_fma((double)buf[k][q].y, p0.y, u1);
                u0 = __builtin_fma((double)buf[k][q].z, p1.x, u0);
                u1 = __builtin_fma((double)buf[k][q].w, p1.y, u1);
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
                for (int q = 0; q < 8; q++) {
                    const double c0 = (icpt && q == 0) ? inv_scale : (double)buf[k][q].x;
                    ac[4 * q] = __builtin_fma(c0, us, ac[4 * q]);
                    ac[4 * q + 1] = __builtin_fma((double)buf[k][q].y, us, ac[4 * q + 1]);
                    ac[4 * q + 2] = __builtin_fma((double)buf[k][q].z, us, ac[4 * q + 2]);
                    ac[4 * q + 3] = __builtin_fma((double)buf[k][q].w, us, ac[4 * q + 3]);
                }
            }
            const long nrow = (it + RING) * nslots + slot;
            if (nrow < a.n) load_row(nrow, buf[k]);      // refill this ring entry
        }
    }
    double *slab = a.wpart + slot * 2 * a.F;
    #pragma unroll
    for (int q = 0; q < 8; q++) {
        const long f = fb + 128 * q;
        if (f < a.F) *reinterpret_cast<double2 *>(slab + 2 * f) = make_double2(ac[4 * q], ac[4 * q + 1]);
        if (f + 1 < a.F) *reinterpret_cast<double2 *>(slab + 2 * f + 2) = make_double2(ac[4 * q + 2], ac[4 * q + 3]);
    }
}

// Wide rows, 8192 < num_freqs <= 16384 (M up to 32768; a cache row is 64-128 KB): still ONE pass over the
// cache.  A datapoint's row (128 KB), its float64 accumulators (256 KB) and v (256 KB) together exceed a
// CU's registers + LDS, so: one 8-wave workgroup per CU, wave w owns tiles w and w + 8, 128 accumulator
// registers per lane, the float32 row in 64 more, v of tiles 0..7 in LDS (128 KB) and v of tiles 8..15
// re-read from L2 for every datapoint (all workgroups read the same 128 KB), four batches per datapoint, the
// first requested under the previous datapoint's tail.  Everything in the datapoint loop is branch-free (clamped addresses,
// zero weights for rows past the end) so that the compiler can count its waits instead of draining the
// memory pipeline.  A row of a CU's share is 5 us of HBM time at 6.4 TB/s against < 1 us of arithmetic,
// so the loads of the next row are simply issued as soon as the current row's registers are free.
typedef unsigned int zc_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int zc_u32x2 __attribute__((ext_vector_type(2)));

// Buffer loads: a wave-uniform descriptor (base, byte count) + a 32-bit per-lane byte offset; whatever lies
// past the byte count reads as zero, which is exactly the padding the incomplete last tile needs.
__device__ __forceinline__ float4 zc_load16(__amdgpu_buffer_rsrc_t rs, unsigned off) {
    const zc_u32x4 r = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)off, 0, 0);
    return make_float4(as_f((int)r.x), as_f((int)r.y), as_f((int)r.z), as_f((int)r.w));
}
__device__ __forceinline__ float2 zc_load8(__amdgpu_buffer_rsrc_t rs, unsigned off) {
    const zc_u32x2 r = __builtin_amdgcn_raw_buffer_load_b64(rs, (int)off, 0, 0);
    return make_float2(as_f((int)r.x), as_f((int)r.y));
}
__device__ __forceinline__ double2 zc_load16d(__amdgpu_buffer_rsrc_t rs, unsigned off) {
    const zc_u32x4 r = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)off, 0, 0);
    return make_double2(__hiloint2double((int)r.y, (int)r.x), __hiloint2double((int)r.w, (int)r.z));
}

template <bool VEC4>
__global__ __launch_bounds__(512, 1) void zcache_ztz_wide_kernel(ZcArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double2 *pv = reinterpret_cast<double2 *>(smem);                              // [8 * 1024] (cos, sin) of v, tiles 0..7
    double *part = reinterpret_cast<double *>(smem + (size_t)8 * 1024 * 16);      // [2][8]
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long slot = blockIdx.x, nslots = gridDim.x;                             // nslots <= n
    const long iters = (a.n + nslots - 1) / nslots;
    for (long f = threadIdx.x; f < 8 * 1024; f += blockDim.x)
        pv[f] = *reinterpret_cast<const double2 *>(a.vec + 2 * f);                // F > 8192: tiles 0..7 are complete
    if (threadIdx.x < 16) part[threadIdx.x] = 0.0;
    __syncthreads();
    const unsigned fa = (unsigned)w * 1024u + 2u * lane;   // tile w:     load q holds frequencies fa + 128 q, + 1
    const unsigned fb = fa + 8u * 1024u;                   // tile w + 8: may be incomplete
    // one descriptor per tile (its byte count is what is left of the row, so the incomplete last tile reads
    // zeros) and per-lane offsets that differ only in the instruction's immediate field
    const long tb = 1024L * (w + 8);                       // first frequency of tile w + 8
    const long left = a.F - tb < 0 ? 0 : (a.F - tb > 1024 ? 1024 : a.F - tb);
    const unsigned zoff = 16u * lane, voff = 32u * lane;
    const __amdgpu_buffer_rsrc_t vrs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(a.vec + 2 * tb), 0, (int)(16 * left), 0x00020000);
    double aa[32], ab[32];
    #pragma unroll
    for (int j = 0; j < 32; j++) { aa[j] = 0.0; ab[j] = 0.0; }
    const bool icpt = a.fit_intercept && w == 0 && lane == 0;
    const double inv_scale = a.inv_scale, s2 = a.scale2;

    float4 ba[8], bb[8];
    auto load_tile = [&](long row, int second, float4 (&dst)[8]) {
        const float *tile = a.zc + row * 2 * a.F + (second ? 2 * tb : 2048L * w);
        const __amdgpu_buffer_rsrc_t rs =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(tile), 0, second ? (int)(8 * left) : 8192, 0x00020000);
        #pragma unroll
        for (int q = 0; q < 8; q++) {
            if (VEC4) {
                dst[q] = zc_load16(rs, zoff + 1024u * q);
            } else {
                const float2 lo = zc_load8(rs, zoff + 1024u * q), hi = zc_load8(rs, zoff + 1024u * q + 8u);
                dst[q] = make_float4(lo.x, lo.y, hi.x, hi.y);
            }
        }
    };
    // batch b of v for tile w + 8: loads q = 2b and 2b + 1, frequencies f and f + 1 of each
    auto load_v = [&](int b, double2 (&dst)[4]) {
        #pragma unroll
        for (int j = 0; j < 2; j++) {
            dst[2 * j] = zc_load16d(vrs, voff + 2048u * (2 * b + j));
            dst[2 * j + 1] = zc_load16d(vrs, voff + 2048u * (2 * b + j) + 16u);
        }
    };
    double2 vc[4];
    load_tile(slot, 0, ba); load_tile(slot, 1, bb); load_v(0, vc);
    for (long it = 0; it < iters; it++) {
        const long row = it * nslots + slot;
        const bool active = row < a.n;
        double u0 = 0.0, u1 = 0.0;
        #pragma unroll
        for (int q = 0; q < 8; q++) {
            const double2 p0 = pv[fa + 128 * q], p1 = pv[fa + 128 * q + 1];
            const double c0 = (icpt && q == 0) ? inv_scale : (double)ba[q].x;
            u0 = __builtin_fma(c0, p0.x, u0);
            u1 = __builtin_fma((double)ba[q].y, p0.y, u1);
            u0 = __builtin_fma((double)ba[q].z, p1.x, u0);
            u1 = __builtin_fma((double)ba[q].w, p1.y, u1);
        }
        // batch 0 was requested at the end of the previous iteration; the later batches are requested as the
        // registers free up (requesting one batch ahead needs 16 more registers: 8 spilled, 8 % slower)
        #pragma unroll
        for (int b = 0; b < 4; b++) {
            if (b > 0) load_v(b, vc);
            #pragma unroll
            for (int j = 0; j < 2; j++) {
                const int q = 2 * b + j;
                u0 = __builtin_fma((double)bb[q].x, vc[2 * j].x, u0);
                u1 = __builtin_fma((double)bb[q].y, vc[2 * j].y, u1);
                u0 = __builtin_fma((double)bb[q].z, vc[2 * j + 1].x, u0);
                u1 = __builtin_fma((double)bb[q].w, vc[2 * j + 1].y, u1);
            }
        }
        const double u = wave_sum(u0 + u1);
        double *pp = part + (it & 1) * 8;
        if (lane == 0) pp[w] = u;
        __syncthreads();
        const double2 t01 = *reinterpret_cast<const double2 *>(pp), t23 = *reinterpret_cast<const double2 *>(pp + 2);
        const double2 t45 = *reinterpret_cast<const double2 *>(pp + 4), t67 = *reinterpret_cast<const double2 *>(pp + 6);
        const double tot = (((t01.x + t01.y) + (t23.x + t23.y)) + ((t45.x + t45.y) + (t67.x + t67.y))) * s2;
        const double us = active ? tot : 0.0;            // the last pass re-reads row n - 1 with weight zero
        long nrow = (it + 1) * nslots + slot;
        nrow = nrow < a.n ? nrow : a.n - 1;
        // the float32 row stays in registers between the two phases; do not let the compiler keep its
        // float64 conversions alive across the barrier instead (128 more registers)
        #pragma unroll
        for (int q = 0; q < 8; q++) {
            asm volatile("" : "+v"(ba[q].x), "+v"(ba[q].y), "+v"(ba[q].z), "+v"(ba[q].w));
            asm volatile("" : "+v"(bb[q].x), "+v"(bb[q].y), "+v"(bb[q].z), "+v"(bb[q].w));
        }
        #pragma unroll
        for (int q = 0; q < 8; q++) {
            const double c0 = (icpt && q == 0) ? inv_scale : (double)ba[q].x;
            aa[4 * q] = __builtin_fma(c0, us, aa[4 * q]);
            aa[4 * q + 1] = __builtin_fma((double)ba[q].y, us, aa[4 * q + 1]);
            aa[4 * q + 2] = __builtin_fma((double)ba[q].z, us, aa[4 * q + 2]);
            aa[4 * q + 3] = __builtin_fma((double)ba[q].w, us, aa[4 * q + 3]);
        }
        load_tile(nrow, 0, ba);                          // refill each half as soon as it has been consumed
        #pragma unroll
        for (int q = 0; q < 8; q++) {
            ab[4 * q] = __builtin_fma((double)bb[q].x, us, ab[4 * q]);
            ab[4 * q + 1] = __builtin_fma((double)bb[q].y, us, ab[4 * q + 1]);
            ab[4 * q + 2] = __builtin_fma((double)bb[q].z, us, ab[4 * q + 2]);
            ab[4 * q + 3] = __builtin_fma((double)bb[q].w, us, ab[4 * q + 3]);
        }
        load_tile(nrow, 1, bb);
        load_v(0, vc);
    }
    double *slab = a.wpart + slot * 2 * a.F;
    #pragma unroll
    for (int q = 0; q < 8; q++) {
        const long f = fa + 128 * q, g = fb + 128 * q;
        *reinterpret_cast<double2 *>(slab + 2 * f) = make_double2(aa[4 * q], aa[4 * q + 1]);
        *reinterpret_cast<double2 *>(slab + 2 * f + 2) = make_double2(aa[4 * q + 2], aa[4 * q + 3]);
        if (g < a.F) *reinterpret_cast<double2 *>(slab + 2 * g) = make_double2(ab[4 * q], ab[4 * q + 1]);
        if (g + 1 < a.F) *reinterpret_cast<double2 *>(slab + 2 * g + 2) = make_double2(ab[4 * q + 2], ab[4 * q + 3]);
    }
}

// w_out[m] = sum over slabs (fixed order) of wpart[slab, m]; 64 columns x 4 slab phases per
// workgroup, each thread 8 independent partial sums to keep loads in flight.
__global__ __launch_bounds__(256) void reduce_slabs_kernel(const double *__restrict__ wpart, double *w_out, long M,
                                                           long nslabs) {
    __shared__ double red[4][64];
    const int col = threadIdx.x & 63, ph = threadIdx.x >> 6;
    const long m = (long)blockIdx.x * 64 + col;
    double s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (m < M) {
        long k = ph;
        for (; k + 28 < nslabs; k += 32) {
            #pragma unroll
            for (int q = 0; q < 8; q++) s[q] += wpart[(k + 4 * q) * M + m];
        }
        double tail = 0.0;
        for (; k < nslabs; k += 4) tail += wpart[k * M + m];
        s[0] += tail;
    }
    red[ph][col] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
    __syncthreads();
    if (ph == 0 && m < M) w_out[m] = (red[0][col] + red[1][col]) + (red[2][col] + red[3][col]);
}

// The same reduction for a short vector (M = the preconditioner's rank: a few hundred columns): 16 columns x 16 slab
// phases per workgroup, so that M / 16 workgroups share the slabs instead of M / 64 and a thread adds nslabs / 16 values
// rather than nslabs / 4 (512 slabs x 512 columns: 7.7 us with the kernel above, which is all latency).  Fixed order:
// phase ph adds slabs ph, ph + 16, ...; the phases are added pairwise in index order.
__global__ __launch_bounds__(256) void reduce_slabs_short_kernel(const double *__restrict__ wpart, double *w_out, long M,
                                                                 long nslabs) {
    __shared__ double red[16][16];
    const int col = threadIdx.x & 15, ph = threadIdx.x >> 4;
    const long m = (long)blockIdx.x * 16 + col;
    double s[4] = {0, 0, 0, 0};
    if (m < M) {
        long k = ph;
        for (; k + 48 < nslabs; k += 64) {
            #pragma unroll
            for (int q = 0; q < 4; q++) s[q] += wpart[(k + 16 * q) * M + m];
        }
        double tail = 0.0;
        for (; k < nslabs; k += 16) tail += wpart[k * M + m];
        s[0] += tail;
    }
    red[ph][col] = (s[0] + s[1]) + (s[2] + s[3]);
    __syncthreads();
    if (ph == 0 && m < M) {
        double t[16];
        #pragma unroll
        for (int i = 0; i < 16; i++) t[i] = red[i][col];
        #pragma unroll
        for (int w = 8; w >= 1; w >>= 1) {
            #pragma unroll
            for (int i = 0; i < w; i++) t[i] = t[2 * i] + t[2 * i + 1];
        }
        w_out[m] = t[0];
    }
}


// ---- z^T y from float32 feature rows (the resident cache or a regenerated window): slab s of wpart [nslabs, M] receives
// sum over rows [s * rows_per_slab, (s + 1) * rows_per_slab) of z_i[m] y_i, z_i = scale * zc[i] (z_i[0] = 1 under fit_intercept),
// accumulated in float64 in row order; reduce_slabs_kernel then adds the slabs in a fixed order.  Workgroup (c, s): 512 columns, thread
// t columns 512 c + 2 t and + 1 (one 8-byte load per row: M is even), four rows' loads issued before their arithmetic.
__global__ __launch_bounds__(256) void zcache_zty_kernel(const float *__restrict__ zc, const double *__restrict__ y, double *wpart,
                                                         long n, long M, long rows_per_slab, int fit_intercept, double scale) {
    const long c = (long)blockIdx.x * 512 + 2 * threadIdx.x;
    if (c >= M) return;
    const long r0 = (long)blockIdx.y * rows_per_slab;
    const long r1 = r0 + rows_per_slab < n ? r0 + rows_per_slab : n;
    const bool icpt = fit_intercept && c == 0;
    double a0 = 0.0, a1 = 0.0;
    long r = r0;
    for (; r + 4 <= r1; r += 4) {
        float2 z[4];
        double yv[4];
        #pragma unroll
        for (int q = 0; q < 4; q++) { z[q] = *reinterpret_cast<const float2 *>(zc + (r + q) * M + c); yv[q] = y[r + q]; }
        #pragma unroll
        for (int q = 0; q < 4; q++) {
            const double ys = yv[q] * scale;
            a0 = icpt ? a0 + yv[q] : __builtin_fma((double)z[q].x, ys, a0);
            a1 = __builtin_fma((double)z[q].y, ys, a1);
        }
    }
    for (; r < r1; r++) {
        const float2 z = *reinterpret_cast<const float2 *>(zc + r * M + c);
        const double ys = y[r] * scale;
        a0 = icpt ? a0 + y[r] : __builtin_fma((double)z.x, ys, a0);
        a1 = __builtin_fma((double)z.y, ys, a1);
    }
    *reinterpret_cast<double2 *>(wpart + (long)blockIdx.y * M + c) = make_double2(a0, a1);
}
