// cross_gram.inc -- part of xgpr_hip.hip (included inside its anonymous namespace, after gram.inc): the symmetrised two-operand Gram of the
// exact NMLL gradient on the matrix cores, from two float32 row arrays.
// ------------------------------------------------------------------------------------
// C[M, M] (+)= A^T B + B^T A     (scoring_toolkit/nmll_gradient_tools.py:70 `inner_deriv += dz_dsigma.T @ xfeatures` over the chunks,
// followed by :88 `inner_deriv += transpose(inner_deriv)`), A = the gradient rows and B = the feature rows xgpr_rbf_grad_rows_f32 writes:
// COMPLETE rows (intercept column and scale applied by the writer), so there is no intercept or scale predicate anywhere here.
//
// The plan is gram_lds_kernel's (gram.inc: 128 x 128 tiles on or above the diagonal, a wave owns 128 x 16, 16-row chunks by LDS-DMA, the
// row operand converted once per chunk LDS -> LDS, rings of three float32 buffers and two float64 images, one barrier per chunk, stream-K
// cut with spill slabs and gram_fixup_kernel) with its two DMA streams fed from two pointers: a tile's unit sequence has TWO halves of
// nchunks chunks each -- the first reads (row operand A, column operand B), the second (B, A) -- and both accumulate into the same
// registers.  Same LDS (80 KiB), same registers, same chunk loop; twice the units of Z^T Z, which is the work of the one full GEMM it
// replaces.  The operand pointers of a chunk are picked on the scalar unit (the chunk number is wave-uniform): nothing is added
// between the MFMAs.
//
// Symmetry, bit for bit: an off-diagonal tile is mirrored at the store.  A DIAGONAL tile holds both (i, j) and (j, i), whose sums run over
// the same products in a different order (a_i b_j first in one, b_j a_i ... second in the other), so only its entries with j >= i are
// used and mirrored -- in C by the owner, inside the spill slab by a workgroup that starts in the middle of the tile (gram_fixup_kernel
// adds whole slabs).  The summation order is fixed by the launch geometry: two runs give the same bits.
// ------------------------------------------------------------------------------------
struct CrossGramArgs {
    const float *A, *B; long ld;         // row arrays [n, ld], same leading dimension
    double *C; long ldc;                 // [M, ldc]
    long nchunks;                        // n / 16: chunks per half
    int T; long ntiles;                  // tiles per side (M / 128), T (T + 1) / 2
    long units_per_wg;                   // ceil(ntiles * 2 nchunks / gridDim.x)
    double *spill;                       // [gridDim.x][128 * 128]
    int accumulate;
};

__global__ __launch_bounds__(512, 4) void cross_gram_lds_kernel(CrossGramArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int jw = 16 * w;
    const long upt = 2 * a.nchunks;                      // units per tile
    const long total = a.ntiles * upt;
    long u = (long)blockIdx.x * a.units_per_wg;
    long uend = u + a.units_per_wg;
    if (uend > total) uend = total;
    const unsigned lds0 = (unsigned)(size_t)(lds_ptr_t)smem;
    auto dma16 = [&](unsigned voff, const char *sbase, unsigned dst) {
        asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" : : "v"(voff), "s"(sbase), "s"(dst) : "memory", "m0");
    };
    // per-lane DMA offsets as in gram_lds_kernel: row operand rows 2 w / 2 w + 1, column operand slot w = rows 4 (w / 2) + w % 2 and that + 2
    const unsigned aoff_l = (unsigned)((lane >> 5) * a.ld * 4 + 16 * (lane & 31));
    const unsigned boff_l = (unsigned)(2 * (lane >> 5) * a.ld * 4 + 16 * (lane & 31));
    const long cstep = 16 * a.ld * 4;
    const unsigned char *abase = smem + g * 1024 + 16 * c;
    const unsigned char *bbase0 = smem + GR_OFF_B32 + (g & 1) * 1024 + (g >> 1) * 512 + 4 * (jw + c);

    int left = uend > u ? (int)(uend - u) : 0;
    while (left > 0) {
        const long tile = u / upt;
        const int c0 = (int)(u - tile * upt);            // first unit of this segment inside the tile's 2 nchunks
        int nch = (int)(upt - c0);
        if (nch > left) nch = left;
        nch = __builtin_amdgcn_readfirstlane(nch);
        int ti, tj;
        gram_tile(a.T, tile, ti, tj);
        const long it0 = (long)ti * 128, jt0 = (long)tj * 128;
        // segment chunk ch is unit c0 + ch: below nchunks the first half (rows of A against columns of B at chunk c0 + ch), from
        // there on the second (rows of B against columns of A at chunk c0 + ch - nchunks).  The second half's bases carry the
        // - nchunks, so both halves address chunk `ch` of the segment the same way.
        const int nfirst = __builtin_amdgcn_readfirstlane(c0 < (int)a.nchunks ? (int)a.nchunks - c0 : 0);
        const long rrow = 2 * w, crow = 4 * (w >> 1) + (w & 1);
        const long r1 = (long)c0 * 16, r2 = ((long)c0 - a.nchunks) * 16;
        const long row_a1 = ((r1 + rrow) * a.ld + it0) * 4, col_b1 = ((r1 + crow) * a.ld + jt0) * 4;
        const long row_b2 = ((r2 + rrow) * a.ld + it0) * 4, col_a2 = ((r2 + crow) * a.ld + jt0) * 4;
        const char *pa = reinterpret_cast<const char *>(a.A), *pb = reinterpret_cast<const char *>(a.B);

        double4_t acc[8];
        #pragma unroll
        for (int e = 0; e < 8; e++) acc[e] = (double4_t){0.0, 0.0, 0.0, 0.0};
        auto stage = [&](int ch, int slot) {
            const bool second = ch >= nfirst;                              // wave-uniform: scalar selects
            const char *rowp = (second ? pb + row_b2 : pa + row_a1) + ch * cstep;
            const char *colp = (second ? pa + col_a2 : pb + col_b1) + ch * cstep;
            dma16(aoff_l, rowp, lds0 + GR_OFF_A32 + slot * GR_A32 + w * 1024);
            dma16(boff_l, colp, lds0 + GR_OFF_B32 + slot * GR_B32 + w * 1024);
        };
        // every LDS-DMA landing: explicit wait for this wave's DMAs, then the workgroup barrier (gram.inc)
        auto landed = [&]() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); __syncthreads(); };

        double2_t av[2][4];
        float bf[2];
        {
            // float32 staging -> float64 image of the row operand: 2 x (8 bytes in, 16 bytes out) per thread
            const unsigned char *cv_in = smem + GR_OFF_A32 + threadIdx.x * 8;
            unsigned char *cv_out = smem + threadIdx.x * 16;
            float2 cvf[2];
            auto cv_load = [&](int slot) {
                #pragma unroll
                for (int p = 0; p < 2; p++) cvf[p] = *reinterpret_cast<const float2 *>(cv_in + slot * GR_A32 + p * 4096);
            };
            auto cv_store = [&](int img) {
                #pragma unroll
                for (int p = 0; p < 2; p++) {
                    const double2_t d = {(double)cvf[p].x, (double)cvf[p].y};
                    *reinterpret_cast<double2_t *>(cv_out + img * GR_A64 + p * 8192) = d;
                }
            };
            auto ldops = [&](int img, int slot, int q, int s) {
                #pragma unroll
                for (int e = 0; e < 4; e++)
                    av[s][e] = *reinterpret_cast<const double2_t *>(abase + img * GR_A64 + q * 4096 + e * 256);
                bf[s] = *reinterpret_cast<const float *>(bbase0 + slot * GR_B32 + 2 * q * 1024);
            };
            auto mm = [&](int s) {
                const double b = (double)bf[s];
                #pragma unroll
                for (int e = 0; e < 4; e++) {
                    acc[2 * e] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s][e].x, b, acc[2 * e], 0, 0, 0);
                    acc[2 * e + 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s][e].y, b, acc[2 * e + 1], 0, 0, 0);
                }
            };
            // the chunk schedule of gram_lds_kernel, unchanged: operands of k-step q + 1 are read before the MFMAs of k-step q, the last
            // k-step of a chunk runs behind the barrier
            auto chunk = [&](int ch, auto k_tag) {
                constexpr int K = decltype(k_tag)::value;                  // ch % 6
                constexpr int slot = K % 3, nslot = (K + 1) % 3, n2slot = (K + 2) % 3, img = K & 1;
                if (ch + 2 < nch) stage(ch + 2, n2slot);   // (that slot held chunk ch - 1: multiplied and converted before the last barrier)
                ldops(img, slot, 1, 1);
                __builtin_amdgcn_sched_barrier(0);
                mm(0);
                if (ch + 1 < nch) { cv_load(nslot); cv_store(img ^ 1); }
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
            stage(0, 0);
            if (nch > 1) stage(1, 1);
            landed();
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
        }

        // ---- store: D register r of row tile 2 e' + o holds C[it0 + 32 e' + 2 (g + 4 r) + o][jt0 + jw + c]
        const bool owner = c0 == 0;                       // this workgroup has the tile from its first unit on
        const bool diag = ti == tj;
        int c_s = c;                                      // (formed again per segment: no 64-bit copy of the column index is held through the chunk loops)
        asm volatile("" : "+v"(c_s));
        const long j = jt0 + jw + c_s;
        double *sp = a.spill + (long)blockIdx.x * 128 * 128;
        auto put = [&](double *p, double v) { if (a.accumulate) *p += v; else *p = v; };
        #pragma unroll
        for (int e = 0; e < 4; e++)
            #pragma unroll
            for (int r = 0; r < 4; r++) {
                const long i = it0 + 32 * e + 2 * (g + 4 * r);
                const double v0 = acc[2 * e][r], v1 = acc[2 * e + 1][r];
                if (!diag) {
                    if (owner) {
                        put(a.C + i * a.ldc + j, v0);
                        put(a.C + (i + 1) * a.ldc + j, v1);
                        double2_t *q = reinterpret_cast<double2_t *>(a.C + j * a.ldc + i);
                        double2_t m = {v0, v1};
                        if (a.accumulate) { const double2_t o = *q; m.x += o.x; m.y += o.y; }
                        *q = m;
                    } else {
                        sp[(i - it0) * 128 + (j - jt0)] = v0;
                        sp[(i - it0 + 1) * 128 + (j - jt0)] = v1;
                    }
                } else {                                  // entries with j >= i only, mirrored (header)
                    const long li = i - it0, lj = j - jt0;
                    if (owner) {
                        if (j >= i) put(a.C + i * a.ldc + j, v0);
                        if (j > i) put(a.C + j * a.ldc + i, v0);
                        if (j >= i + 1) put(a.C + (i + 1) * a.ldc + j, v1);
                        if (j > i + 1) put(a.C + j * a.ldc + i + 1, v1);
                    } else {
                        if (lj >= li) sp[li * 128 + lj] = v0;
                        if (lj > li) sp[lj * 128 + li] = v0;
                        if (lj >= li + 1) sp[(li + 1) * 128 + lj] = v1;
                        if (lj > li + 1) sp[lj * 128 + li + 1] = v1;
                    }
                }
            }
        u += nch;
        left -= nch;
        __syncthreads();                                  // the images are reused by the next segment
    }
}

// the last n % 16 rows (fewer than one chunk): plain float64 FMAs, one thread per entry on or above the diagonal, mirrored
__global__ __launch_bounds__(256) void cross_gram_tail_kernel(const float *__restrict__ A, const float *__restrict__ B, long ld, int rows,
                                                              double *C, long ldc, long M) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (j >= M || j < i) return;
    double s = 0.0;
    for (int k = 0; k < rows; k++) {
        s = __builtin_fma((double)A[k * ld + i], (double)B[k * ld + j], s);
        s = __builtin_fma((double)B[k * ld + i], (double)A[k * ld + j], s);
    }
    C[i * ldc + j] += s;
    if (i != j) C[j * ldc + i] += s;
}
