// gram.inc -- part of xgpr_hip.hip (included inside its anonymous namespace, in order): the dense Z^T Z accumulation of exact mode / variance / crude tuning on the matrix cores, from float32 feature rows.
// ------------------------------------------------------------------------------------
// C[msub, msub] (+)= Z[:, :msub]^T Z[:, :msub]     (scoring_toolkit/exact_nmll_calcs.py:42-78 calc_design_mat,
// :116-139 calc_var_design_mat, scoring_toolkit/lb_optimizer.py:68-117), Z = scale * zc with Z[:, 0] = 1 under
// fit_intercept -- BOTH operands are the float32 rows the feature kernels produce (the resident cache or a regenerated
// window), widened on the way to v_mfma_f64_16x16x4_f64; float64 Z is never written.
//
// The plan is sketch_gemm_lds_kernel's (128 x 128 workgroup tiles, a wave owns 128 x 16, 16-row chunks of both operand
// tiles by LDS-DMA, one conversion per 8 MFMAs for the column operand) with two differences:
//   * the ROW operand arrives as float32 too.  Converted next to the MFMAs it would cost 8 more conversions per
//     8 MFMAs -- and float64 vector instructions run on the matrix pipe's time (sketch_gemm.inc) --, so the
//     workgroup converts each chunk of it ONCE, cooperatively, LDS -> LDS (4 elements per thread and chunk), into the
//     float64 image the MFMA operand reads expect.  The staging runs one chunk further ahead for it (rings of three
//     float32 buffers, two float64 images), so that chunk ch + 1 is converted while chunk ch is multiplied and the
//     loop keeps ONE barrier per chunk (with a second barrier between landing and use: 68.6 TFLOP/s; ...).
//   * only tiles on or above the diagonal are computed (the result is symmetric; mirrored at the store), and the
//     T (T + 1) / 2 tiles are not a multiple of the resident workgroups (2080 tiles on 512 slots at M = 8192: the last
//     round would run 6 % full), so the work is cut stream-K fashion: the sequence of (tile, chunk) units is divided
//     EVENLY over the workgroups; a workgroup that starts in the middle of a tile writes that partial into its own
//     spill slab, and gram_fixup_kernel adds the slabs into C in workgroup order -- deterministic.
// ------------------------------------------------------------------------------------
struct GramArgs {
    const float *zc; long ldz;           // feature rows [n, ldz]
    double *C; long ldc;                 // [msub, ldc]
    long nchunks;                        // n / 16
    int T; long ntiles;                  // tiles per side (msub / 128), T (T + 1) / 2
    long units_per_wg;                   // ceil(ntiles * nchunks / gridDim.x)
    double *spill;                       // [gridDim.x][128 * 128]
    double scale; int fit_intercept; int accumulate;
};

constexpr int GR_A64 = 16 * 128 * 8;                 // float64 image of the row operand chunk (x 2)
constexpr int GR_A32 = 16 * 128 * 4;                 // its float32 staging (x 3)
constexpr int GR_B32 = 16 * 128 * 4;                 // the column operand chunk, pairs of rows (r, r + 2) per KiB (x 3).  No
                                                     // padding between the pairs here (two workgroups of 80 KiB fill the CU's
                                                     // LDS exactly): the column operand's reads are 2-way conflicted, four
                                                     // 4-byte reads per wave and chunk
constexpr int GR_OFF_A32 = 2 * GR_A64, GR_OFF_B32 = GR_OFF_A32 + 3 * GR_A32;
constexpr int GR_LDS = GR_OFF_B32 + 3 * GR_B32;      // 81920 bytes

// tile number -> (ti <= tj), row-major over the upper triangle
__device__ __forceinline__ void gram_tile(int T, long t, int &ti, int &tj) {
    int i = 0;
    int rem = (int)t;                     // (tiles per triangle fit 32 bits; a 64-bit ordered compare would run on the vector unit)
    while (rem >= T - i) { rem -= T - i; i++; }
    ti = i; tj = i + rem;
}

__global__ __launch_bounds__(512, 4) void gram_lds_kernel(GramArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int jw = 16 * w;
    const long total = a.ntiles * a.nchunks;
    long u = (long)blockIdx.x * a.units_per_wg;
    long uend = u + a.units_per_wg;
    if (uend > total) uend = total;
    const unsigned lds0 = (unsigned)(size_t)(lds_ptr_t)smem;
    auto dma16 = [&](unsigned voff, const char *sbase, unsigned dst) {
        asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" : : "v"(voff), "s"(sbase), "s"(dst) : "memory", "m0");
    };
    // per-lane DMA offsets: row operand rows 2 w (lanes 0..31) and 2 w + 1 (lanes 32..63), 4 floats per lane; column
    // operand as in sketch_gemm_lds_kernel (slot w = rows 4 (w / 2) + w % 2 and that + 2)
    const unsigned aoff_l = (unsigned)((lane >> 5) * a.ldz * 4 + 16 * (lane & 31));
    const unsigned boff_l = (unsigned)(2 * (lane >> 5) * a.ldz * 4 + 16 * (lane & 31));
    const long cstep = 16 * a.ldz * 4;
    const unsigned char *abase = smem + g * 1024 + 16 * c;
    const unsigned char *bbase0 = smem + GR_OFF_B32 + (g & 1) * 1024 + (g >> 1) * 512 + 4 * (jw + c);

    // (32-bit count of the units left: an ordered 64-bit compare would run on the vector unit and hold its operand in
    // vector registers through the chunk loops)
    int left = uend > u ? (int)(uend - u) : 0;
    while (left > 0) {
        const long tile = u / a.nchunks;
        const int c0 = (int)(u - tile * a.nchunks);
        int nch = (int)(a.nchunks - c0);
        if (nch > left) nch = left;
        nch = __builtin_amdgcn_readfirstlane(nch);
        int ti, tj;
        gram_tile(a.T, tile, ti, tj);
        const long it0 = (long)ti * 128, jt0 = (long)tj * 128;
        const bool icpt_a = a.fit_intercept && it0 == 0;                 // feature 0 is in the row operand's tile
        const bool icpt_wave = a.fit_intercept && jt0 + jw == 0;         // ... / is this wave's first column

        double4_t acc[8];
        #pragma unroll
        for (int e = 0; e < 8; e++) acc[e] = (double4_t){0.0, 0.0, 0.0, 0.0};
        const char *abase_g = reinterpret_cast<const char *>(a.zc + ((long)c0 * 16 + 2 * w) * a.ldz + it0);
        const char *bbase_g = reinterpret_cast<const char *>(a.zc + ((long)c0 * 16 + 4 * (w >> 1) + (w & 1)) * a.ldz + jt0);
        auto stage = [&](int ch, int slot) {
            dma16(aoff_l, abase_g + ch * cstep, lds0 + GR_OFF_A32 + slot * GR_A32 + w * 1024);
            dma16(boff_l, bbase_g + ch * cstep, lds0 + GR_OFF_B32 + slot * GR_B32 + w * 1024);
        };
        // (cross_gram_lds_kernel, cross_gram.inc, is a COPY of this wait + barrier, of the conversion and of the chunk schedule below: a fix
        // to the vmcnt / barrier placement or to the schedule is made in both)
#ifdef XGPR_ABL_GR_NOBAR
        auto landed = [&]() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); };      // (timing ablation, wrong results)
#else
        auto landed = [&]() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); __syncthreads(); };
#endif

        double2_t av[2][4];
        float bf[2];
        // ICW: this wave's first column is the intercept; ICA: feature 0 is in the row operand's tile.  Every vector
        // instruction between the MFMAs costs the matrix pipe time here (tools/gram_ceiling.sh: the conversion's 8 + the
        // 12 address / select instructions of a rolled loop were worth 5.5 % of the kernel), so the ring positions are
        // compile-time -- the chunk loop is unrolled by 6 = lcm(3 staging slots, 2 images), every LDS address is one base
        // register + an immediate -- and the intercept select exists only in the instantiations that have an intercept.
        // (ICW is a per-WAVE fact, so it is a runtime predicate inside the ICA instantiation -- it implies ICA: tiles lie on
        // or above the diagonal -- and every wave of the workgroup runs the SAME instantiation, i.e. the same barrier
        // instructions; tile row 0 pays one wave-uniform select per k-step for it, the other tiles nothing)
        auto run = [&](auto ica_tag, const bool icw) {
            constexpr bool ICA = decltype(ica_tag)::value;
            // float32 staging -> float64 image of the row operand: 2 x (8 bytes in, 16 bytes out) per thread,
            // contiguous over the lanes on both sides; the intercept column is set here (its unscaled value is 1)
            const unsigned char *cv_in = smem + GR_OFF_A32 + threadIdx.x * 8;
            unsigned char *cv_out = smem + threadIdx.x * 16;
            // (placed BEHIND the first k-step's MFMAs of a chunk: the wave waits for its two LDS reads while its own MFMAs
            // run, not in front of them -- tools/gram_ceiling.sh)
            float2 cvf[2];
            auto cv_load = [&](int slot) {
#ifndef XGPR_ABL_GR_NOCONV
                #pragma unroll
                for (int p = 0; p < 2; p++)                // element 512 p + threadIdx.x: row 8 p + (threadIdx.x >> 6), pair threadIdx.x & 63
                    cvf[p] = *reinterpret_cast<const float2 *>(cv_in + slot * GR_A32 + p * 4096);
#endif
            };
            auto cv_store = [&](int img) {
#ifndef XGPR_ABL_GR_NOCONV                                  // (timing ablation, wrong results: tools/gram_ceiling.sh)
                #pragma unroll
                for (int p = 0; p < 2; p++) {
                    double2_t d = {(double)cvf[p].x, (double)cvf[p].y};
                    if constexpr (ICA) { if ((threadIdx.x & 63) == 0) d.x = 1.0; }
                    *reinterpret_cast<double2_t *>(cv_out + img * GR_A64 + p * 8192) = d;
                }
#endif
            };
            auto ldops = [&](int img, int slot, int q, int s) {
                #pragma unroll
                for (int e = 0; e < 4; e++)
                    av[s][e] = *reinterpret_cast<const double2_t *>(abase + img * GR_A64 + q * 4096 + e * 256);
                bf[s] = *reinterpret_cast<const float *>(bbase0 + slot * GR_B32 + 2 * q * 1024);
            };
            auto mm = [&](int s) {
                double b = (double)bf[s];
                if constexpr (ICA) { if (icw) b = c == 0 ? 1.0 : b; }
                #pragma unroll
                for (int e = 0; e < 4; e++) {
                    acc[2 * e] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s][e].x, b, acc[2 * e], 0, 0, 0);
                    acc[2 * e + 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s][e].y, b, acc[2 * e + 1], 0, 0, 0);
                }
            };
            // Operands of k-step q + 1 are read BEFORE the MFMAs of k-step q are issued, and the last k-step of a chunk
            // runs behind the barrier, after the first reads of the next chunk (as in sketch_gemm_lds_kernel; copied in cross_gram.inc)
            auto chunk = [&](int ch, auto k_tag) {
                constexpr int K = decltype(k_tag)::value;                  // ch % 6
                constexpr int slot = K % 3, nslot = (K + 1) % 3, n2slot = (K + 2) % 3, img = K & 1;
                if (ch + 2 < nch) stage(ch + 2, n2slot);   // (that slot held chunk ch - 1: multiplied and converted before the last barrier)
                ldops(img, slot, 1, 1);
                __builtin_amdgcn_sched_barrier(0);
                mm(0);
                if (ch + 1 < nch) { cv_load(nslot); cv_store(img ^ 1); }   // chunk ch + 1's image, converted in the shadow of this k-step's MFMAs; read after the next barrier
                ldops(img, slot, 2, 0);
                __builtin_amdgcn_sched_barrier(0);
                mm(1);
                ldops(img, slot, 3, 1);
                __builtin_amdgcn_sched_barrier(0);
                mm(0);
                landed();                  // chunk ch + 2 has landed, chunk ch + 1's image is complete, chunk ch's buffers are free
                if (ch + 1 < nch) ldops(img ^ 1, nslot, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                mm(1);
            };
            cv_load(0);
            cv_store(0);
            __syncthreads();
            ldops(0, 0, 0, 0);
            int ch = 0;
            for (; ch + 6 <= nch; ch += 6) {
                chunk(ch, sk_int<0>{}); chunk(ch + 1, sk_int<1>{}); chunk(ch + 2, sk_int<2>{});
                chunk(ch + 3, sk_int<3>{}); chunk(ch + 4, sk_int<4>{}); chunk(ch + 5, sk_int<5>{});
            }
            if (ch < nch) chunk(ch, sk_int<0>{});
            if (ch + 1 < nch) chunk(ch + 1, sk_int<1>{});
            if (ch + 2 < nch) chunk(ch + 2, sk_int<2>{});
            if (ch + 3 < nch) chunk(ch + 3, sk_int<3>{});
            if (ch + 4 < nch) chunk(ch + 4, sk_int<4>{});
        };
        stage(0, 0);
        if (nch > 1) stage(1, 1);
        landed();
        if (icpt_a) run(sk_tag<true>{}, icpt_wave);                  // (icpt_wave: this wave's column 0 is feature 0, tile (0, 0))
        else run(sk_tag<false>{}, false);

        // ---- store: D register r of row tile 2 e' + o holds C[it0 + 32 e' + 2 (g + 4 r) + o][jt0 + jw + c], unscaled
        const bool owner = c0 == 0;                       // this workgroup has the tile from its first chunk on
        int c_s = c;                                      // (formed again per segment: no 64-bit copy of the column index is held through the chunk loops)
        asm volatile("" : "+v"(c_s));
        const long j = jt0 + jw + c_s;
        double scale_s = a.scale;                         // (re-read from the scalar registers here: no copy of it is held in vector registers through the chunk loop)
        asm volatile("" : "+s"(scale_s));
        const double scj = (a.fit_intercept && j == 0) ? 1.0 : scale_s;
        double *sp = a.spill + (long)blockIdx.x * 128 * 128;
        #pragma unroll
        for (int e = 0; e < 4; e++)
            #pragma unroll
            for (int r = 0; r < 4; r++) {
                const long i = it0 + 32 * e + 2 * (g + 4 * r);
                const double v0 = acc[2 * e][r] * scj * ((a.fit_intercept && i == 0) ? 1.0 : scale_s);
                const double v1 = acc[2 * e + 1][r] * scj * scale_s;
                if (owner) {
                    double *p0 = a.C + i * a.ldc + j, *p1 = p0 + a.ldc;
                    if (a.accumulate) { *p0 += v0; *p1 += v1; } else { *p0 = v0; *p1 = v1; }
                    if (ti != tj) {
                        double2_t *q = reinterpret_cast<double2_t *>(a.C + j * a.ldc + i);
                        double2_t m = {v0, v1};
                        if (a.accumulate) { const double2_t o = *q; m.x += o.x; m.y += o.y; }
                        *q = m;
                    }
                } else {
                    sp[(i - it0) * 128 + (j - jt0)] = v0;
                    sp[(i - it0 + 1) * 128 + (j - jt0)] = v1;
                }
            }
        u += nch;
        left -= nch;
        __syncthreads();                                  // the images are reused by the next segment
    }
}

// adds the spilled partials into C: one workgroup per tile, its partials in workgroup order (the units of a tile are
// contiguous, so the workgroups that start inside tile t are those whose first unit lies strictly inside its range)
__global__ __launch_bounds__(256) void gram_fixup_kernel(GramArgs a, long nwg) {
    const long tile = blockIdx.x;
    int ti, tj;
    gram_tile(a.T, tile, ti, tj);
    const long lo = tile * a.nchunks, hi = lo + a.nchunks;
    long w0 = lo / a.units_per_wg + 1;                     // first workgroup whose first unit is > lo
    for (long w = w0; w < nwg && w * a.units_per_wg < hi; w++) {
        const double *sp = a.spill + w * 128 * 128;
        for (int idx = threadIdx.x; idx < 128 * 128; idx += 256) {
            const long i = (long)ti * 128 + idx / 128, j = (long)tj * 128 + idx % 128;
            const double v = sp[idx];
            a.C[i * a.ldc + j] += v;
            if (ti != tj) a.C[j * a.ldc + i] += v;
        }
        __syncthreads();
    }
}

// the last n % 16 datapoints (fewer than one chunk): plain float64 FMAs, one thread per entry on or above the diagonal
__global__ __launch_bounds__(256) void gram_tail_kernel(const float *__restrict__ zc, long ldz, int rows, double *C, long ldc,
                                                        long msub, double scale, int fit_intercept) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (j >= msub || j < i) return;
    double s = 0.0;
    for (int k = 0; k < rows; k++) {
        const double zi = (fit_intercept && i == 0) ? 1.0 : (double)zc[k * ldz + i] * scale;
        const double zj = (fit_intercept && j == 0) ? 1.0 : (double)zc[k * ldz + j] * scale;
        s = __builtin_fma(zi, zj, s);
    }
    C[i * ldc + j] += s;
    if (i != j) C[j * ldc + i] += s;
}
