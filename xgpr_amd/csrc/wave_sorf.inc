// wave_sorf.inc -- part of xgpr_hip.hip (included inside its anonymous namespace, in order): Rademacher sign masks and the wave-level FHT / SORF (register-only and two-layout forms).
// ------------------------------------------------------------------------------------
// Rademacher sign masks: masks[s * MW + g] bit l = (radem[s, 0, 64 g + l] < 0); one 64-bit
// lane mask per (diagonal s, group of 64 frequencies), zero beyond R.  MW is R rounded up to
// a multiple of 1024, over 64 -- so a wave tile's 16 masks per diagonal are always in range.
// The masks are wave-uniform, so the kernels read them with scalar loads and apply them with
// one v_cndmask per element.
// ------------------------------------------------------------------------------------
__global__ void pack_radem_kernel(const int8_t *__restrict__ radem, uint64_t *masks, long R, int MW) {
    const int lane = threadIdx.x & 63;
    const long item = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (item >= 3L * MW) return;
    const int s = (int)(item / MW);
    const long g = item % MW;
    const long f = g * 64 + lane;
    int8_t val = f < R ? radem[(long)s * R + f] : (int8_t)1;
    uint64_t m = __ballot(val < 0);
    if (lane == 0) masks[item] = m;
}

// ------------------------------------------------------------------------------------
// wave-level FHT (P <= 1024, float)
// ------------------------------------------------------------------------------------
__device__ __forceinline__ void bfly(float &a, float &b) {
    float s = a + b, d = a - b;
    a = s; b = d;
}

// Cross-lane butterfly of lane stride H = 1, 2 with the upper lanes' results NEGATED, in ONE instruction per
// register:  v <- partner * sgn + v  (v_fmac_f32 with the partner as its DPP operand), sgn = -1 on lanes with bit H
// set and +1 elsewhere: x + partner on the lower lane, x - partner = -(partner - x) on the upper one.  The product
// with +-1 is exact and the fused add rounds once, so up to that sign the result is the add / subtract of xstage
// bit for bit.  A Hadamard stage is linear, and every later stage of the same transform pairs elements whose lanes
// agree in bit H, so the sign simply rides along: after stages 1 and 2 lane l holds (-1)^(bit0(l) + bit1(l)) times
// the true value, and whoever applies the next per-element sign flip (the next round's Rademacher diagonal, chi)
// folds that factor in for free.  Saves the v_xor per register that xstage spends on the butterfly's sign.
template <int H> __device__ __forceinline__ void xstage_neg(float (&v)[16], float sgn) {
    static_assert(H == 1 || H == 2, "quad_perm stages only");
#define XGPR_XN(CTRL)                                                                                         \
        asm volatile(                                                                                         \
            "s_nop 1\n\t"                                                                                     \
            "v_fmac_f32_dpp %0, %0, %8 " CTRL " row_mask:0xf bank_mask:0xf\n\t"                                \
            "v_fmac_f32_dpp %1, %1, %8 " CTRL " row_mask:0xf bank_mask:0xf\n\t"                                \
            "v_fmac_f32_dpp %2, %2, %8 " CTRL " row_mask:0xf bank_mask:0xf\n\t"                                \
            "v_fmac_f32_dpp %3, %3, %8 " CTRL " row_mask:0xf bank_mask:0xf\n\t"                                \
            "v_fmac_f32_dpp %4, %4, %8 " CTRL " row_mask:0xf bank_mask:0xf\n\t"                                \
            "v_fmac_f32_dpp %5, %5, %8 " CTRL " row_mask:0xf bank_mask:0xf\n\t"                                \
            "v_fmac_f32_dpp %6, %6, %8 " CTRL " row_mask:0xf bank_mask:0xf\n\t"                                \
            "v_fmac_f32_dpp %7, %7, %8 " CTRL " row_mask:0xf bank_mask:0xf\n\t"                                \
            "s_nop 1"                                                                                         \
            : "+v"(v[r0]), "+v"(v[r0 + 1]), "+v"(v[r0 + 2]), "+v"(v[r0 + 3]), "+v"(v[r0 + 4]), "+v"(v[r0 + 5]),  \
              "+v"(v[r0 + 6]), "+v"(v[r0 + 7])                                                                \
            : "v"(sgn))
    #pragma unroll
    for (int r0 = 0; r0 < 16; r0 += 8) {
        if constexpr (H == 1) { XGPR_XN("quad_perm:[1,0,3,2]"); }
        else { XGPR_XN("quad_perm:[2,3,0,1]"); }
    }
#undef XGPR_XN
}
// the sign the two negated stages leave on a lane: all-ones where bit0(l) + bit1(l) is odd
__device__ __forceinline__ uint32_t xneg_parity(int lane) { return (((lane >> 1) ^ lane) & 1) ? 0xffffffffu : 0u; }

// cross-lane butterfly of stride H (< 64) on all 16 registers: lanes with bit H clear get
// x + partner, lanes with bit H set get partner - x, partner = lane ^ H.
template <int H> __device__ __forceinline__ void xstage(float (&v)[16], int lane) {
    if constexpr (H == 1 || H == 2 || H == 8) {
        // two instructions per register: the own term with the butterfly's sign folded in (v_xor), then the
        // partner as the DPP operand of the add itself (quad_perm, row_ror:8) -- the compiler leaves a separate
        // v_mov_b32_dpp in front of the add, a third of this stage's issue slots.  Eight registers per
        // block: the eight xors in front also cover the VALU-write -> DPP-read hazard on both sides.
        const int sm = (lane & H) ? (int)0x80000000 : 0;
#define XGPR_XQ(CTRL)                                                                                         \
        asm volatile(                                                                                         \
            "v_xor_b32 %8, %16, %0\n\tv_xor_b32 %9, %16, %1\n\tv_xor_b32 %10, %16, %2\n\tv_xor_b32 %11, %16, %3\n\t"   \
            "v_xor_b32 %12, %16, %4\n\tv_xor_b32 %13, %16, %5\n\tv_xor_b32 %14, %16, %6\n\tv_xor_b32 %15, %16, %7\n\t" \
            "v_add_f32_dpp %0, %0, %8 " CTRL " row_mask:0xf bank_mask:0xf\n\t"                                \
            "v_add_f32_dpp %1, %1, %9 " CTRL " row_mask:0xf bank_mask:0xf\n\t"                                \
            "v_add_f32_dpp %2, %2, %10 " CTRL " row_mask:0xf bank_mask:0xf\n\t"                               \
            "v_add_f32_dpp %3, %3, %11 " CTRL " row_mask:0xf bank_mask:0xf\n\t"                               \
            "v_add_f32_dpp %4, %4, %12 " CTRL " row_mask:0xf bank_mask:0xf\n\t"                               \
            "v_add_f32_dpp %5, %5, %13 " CTRL " row_mask:0xf bank_mask:0xf\n\t"                               \
            "v_add_f32_dpp %6, %6, %14 " CTRL " row_mask:0xf bank_mask:0xf\n\t"                               \
            "v_add_f32_dpp %7, %7, %15 " CTRL " row_mask:0xf bank_mask:0xf\n\t"                               \
            "s_nop 1"                                                                                         \
            : "+v"(v[r0]), "+v"(v[r0 + 1]), "+v"(v[r0 + 2]), "+v"(v[r0 + 3]), "+v"(v[r0 + 4]), "+v"(v[r0 + 5]),  \
              "+v"(v[r0 + 6]), "+v"(v[r0 + 7]), "=&v"(t0), "=&v"(t1), "=&v"(t2), "=&v"(t3), "=&v"(t4), "=&v"(t5), \
              "=&v"(t6), "=&v"(t7)                                                                            \
            : "v"(sm))
        #pragma unroll
        for (int r0 = 0; r0 < 16; r0 += 8) {
            float t0, t1, t2, t3, t4, t5, t6, t7;
            if constexpr (H == 1) { XGPR_XQ("quad_perm:[1,0,3,2]"); }
            else if constexpr (H == 2) { XGPR_XQ("quad_perm:[2,3,0,1]"); }
            else { XGPR_XQ("row_ror:8"); }
        }
#undef XGPR_XQ
    } else if constexpr (H == 4) {
        // lane^4 is row_ror:12 (lane+4) for DPP banks 0,2 and row_ror:4 (lane-4) for banks 1,3:
        // two bank-masked DPP ops write the butterfly directly.  s_nop 1 covers the
        // VALU-write -> DPP-read hazard on both sides (the compiler cannot see into the asm).
        #pragma unroll
        for (int r0 = 0; r0 < 16; r0 += 8) {
            float o0, o1, o2, o3, o4, o5, o6, o7;
            asm volatile(
                "s_nop 1\n\t"
                "v_add_f32_dpp %0, %8, %8 row_ror:12 row_mask:0xf bank_mask:0x5\n\t"
                "v_add_f32_dpp %1, %9, %9 row_ror:12 row_mask:0xf bank_mask:0x5\n\t"
                "v_add_f32_dpp %2, %10, %10 row_ror:12 row_mask:0xf bank_mask:0x5\n\t"
                "v_add_f32_dpp %3, %11, %11 row_ror:12 row_mask:0xf bank_mask:0x5\n\t"
                "v_add_f32_dpp %4, %12, %12 row_ror:12 row_mask:0xf bank_mask:0x5\n\t"
                "v_add_f32_dpp %5, %13, %13 row_ror:12 row_mask:0xf bank_mask:0x5\n\t"
                "v_add_f32_dpp %6, %14, %14 row_ror:12 row_mask:0xf bank_mask:0x5\n\t"
                "v_add_f32_dpp %7, %15, %15 row_ror:12 row_mask:0xf bank_mask:0x5\n\t"
                "v_sub_f32_dpp %0, %8, %8 row_ror:4 row_mask:0xf bank_mask:0xa\n\t"
                "v_sub_f32_dpp %1, %9, %9 row_ror:4 row_mask:0xf bank_mask:0xa\n\t"
                "v_sub_f32_dpp %2, %10, %10 row_ror:4 row_mask:0xf bank_mask:0xa\n\t"
                "v_sub_f32_dpp %3, %11, %11 row_ror:4 row_mask:0xf bank_mask:0xa\n\t"
                "v_sub_f32_dpp %4, %12, %12 row_ror:4 row_mask:0xf bank_mask:0xa\n\t"
                "v_sub_f32_dpp %5, %13, %13 row_ror:4 row_mask:0xf bank_mask:0xa\n\t"
                "v_sub_f32_dpp %6, %14, %14 row_ror:4 row_mask:0xf bank_mask:0xa\n\t"
                "v_sub_f32_dpp %7, %15, %15 row_ror:4 row_mask:0xf bank_mask:0xa\n\t"
                "s_nop 1"
                : "=&v"(o0), "=&v"(o1), "=&v"(o2), "=&v"(o3), "=&v"(o4), "=&v"(o5), "=&v"(o6), "=&v"(o7)
                : "v"(v[r0]), "v"(v[r0 + 1]), "v"(v[r0 + 2]), "v"(v[r0 + 3]), "v"(v[r0 + 4]), "v"(v[r0 + 5]),
                  "v"(v[r0 + 6]), "v"(v[r0 + 7]));
            v[r0] = o0; v[r0 + 1] = o1; v[r0 + 2] = o2; v[r0 + 3] = o3;
            v[r0 + 4] = o4; v[r0 + 5] = o5; v[r0 + 6] = o6; v[r0 + 7] = o7;
        }
    } else {
        // H = 16 / 32: v_permlane16_swap / v_permlane32_swap on a register pair (A, B) puts the
        // two butterfly operands of both registers into the same lanes: swap, add/sub, swap back.
        #pragma unroll
        for (int r = 0; r < 16; r += 2) {
            int a = as_i(v[r]), b = as_i(v[r + 1]);
            if constexpr (H == 16) {
                auto t = __builtin_amdgcn_permlane16_swap(a, b, false, false);
                float s = as_f(t[0]) + as_f(t[1]), d = as_f(t[0]) - as_f(t[1]);
                auto u = __builtin_amdgcn_permlane16_swap(as_i(s), as_i(d), false, false);
                v[r] = as_f(u[0]); v[r + 1] = as_f(u[1]);
            } else {
                auto t = __builtin_amdgcn_permlane32_swap(a, b, false, false);
                float s = as_f(t[0]) + as_f(t[1]), d = as_f(t[0]) - as_f(t[1]);
                auto u = __builtin_amdgcn_permlane32_swap(as_i(s), as_i(d), false, false);
                v[r] = as_f(u[0]); v[r + 1] = as_f(u[1]);
            }
        }
    }
}

// FHT of every length-P transform in the wave tile, stages h = 1, 2, ..., P/2 in order.
template <int LOG2P> __device__ __forceinline__ void wave_fht(float (&v)[16], int lane) {
    constexpr int P = 1 << LOG2P;
    if constexpr (P > 1) xstage<1>(v, lane);
    if constexpr (P > 2) xstage<2>(v, lane);
    if constexpr (P > 4) xstage<4>(v, lane);
    if constexpr (P > 8) xstage<8>(v, lane);
    if constexpr (P > 16) xstage<16>(v, lane);
    if constexpr (P > 32) xstage<32>(v, lane);
    #pragma unroll
    for (int q = 1; q < P / 64; q <<= 1) {
        #pragma unroll
        for (int r = 0; r < 16; r++)
            if (!(r & q)) bfly(v[r], v[r + q]);
    }
}

// Scalar view of the packed sign masks: constant address space, so the (wave-uniform) loads
// are s_load_dwordx16 into SGPRs and each mask is applied with one v_cndmask.
typedef const __attribute__((address_space(4))) uint64_t *cmask_t;

__device__ __forceinline__ cmask_t as_cmask(const uint64_t *p) { return (cmask_t)p; }

// Inside a per-datapoint loop: stops the compiler from hoisting the 48 mask loads out of the
// loop (96 live SGPRs would be spilled to VGPR lanes); re-reading 384 B from the scalar cache
// per datapoint costs no vector-ALU issue slots.
__device__ __forceinline__ cmask_t launder(cmask_t p) {
    asm volatile("" : "+s"(p));
    return p;
}

// three rounds of { x *= radem * norm ; FHT }.  mk points at this tile's first mask of
// diagonal 0; diagonal s is MW masks further on.  For even log2(P) the normaliser is an
// exact power of two and is folded into chi by the caller (exact), so only the sign flip
// remains; for odd log2(P) the rounded constant is applied per round as the reference does.
template <int LOG2P>
__device__ __forceinline__ void wave_sorf(float (&v)[16], cmask_t mk, int MW, float nc, int lane) {
    uint64_t m[16];
    #pragma unroll
    for (int r = 0; r < 16; r++) m[r] = mk[r];
    #pragma unroll
    for (int s = 0; s < 3; s++) {
        #pragma unroll
        for (int r = 0; r < 16; r++) {
            float t = (LOG2P & 1) ? v[r] * nc : v[r];
            v[r] = __builtin_amdgcn_inverse_ballot_w64(m[r]) ? -t : t;
        }
        if (s < 2) {
            // next round's 16 masks: issued here, after this round's were consumed (the empty asm
            // ties the loads to the data), so they arrive under the FHT and at most two rounds of
            // masks are ever live in SGPRs
            asm volatile("" : "+s"(mk) : "v"(v[0]));
            #pragma unroll
            for (int r = 0; r < 16; r++) m[r] = mk[(s + 1) * MW + r];
        }
        wave_fht<LOG2P>(v, lane);
    }
}

// ---- two-layout SORF for 128 <= P <= 1024 ("T path").  The vector pipe is what bounds these kernels, and a cross-lane
// butterfly costs it 2-4x a register-local one (DPP ops occupy it twice as long as a plain add, v_permlane*_swap four
// times).  So the tile alternates between two register layouts through a wave-private LDS buffer:
//   layout C ("columns", the tile layout everything else uses): lane = t[5:0], register = t[9:6]
//   layout R ("rows"):                                          lane = t[9:4], register = t[3:0]
// In R strides 1..8 are register-local and strides 16, 32 are quad_perm DPP (lane bits 0, 1); in C strides >= 64 are
// register-local: 8 of the 10 stages of an FHT-1024 need no cross-lane instruction.  Stage order is still
// h = 1, 2, 4, ..., so the result is bit-identical to wave_sorf (tools/sorf_variants.hip, tests/test_gpu_ops.py).
typedef __attribute__((address_space(3))) void *lds_ptr_t;

// Rademacher flips of a lane's 16 elements in layout R: bit j of swd -> sign of v[j].  The sign position is reached
// with one shift (j = 15) and then a doubling per element: v_add_u32 issues faster than v_lshlrev_b32 on this part
// (tools/valu_price.hip: 1.0 against 1.4), and written as x + x the compiler turns the doublings back into sixteen
// independent shifts, hence the assembly -- four to a block, so that few hazard nops come with it.
__device__ __forceinline__ float flip_by(float x, uint32_t m) {
    return as_f((int)__builtin_amdgcn_bitop3_b32(m, (uint32_t)as_i(x), 0x80000000u, 0x6c));
}
template <bool MUL>
__device__ __forceinline__ void flip_signs16(float (&v)[16], uint32_t swd, float nc) {
    uint32_t m3 = swd << 16, m2, m1, m0, nx;
    #pragma unroll
    for (int j = 15; j >= 3; j -= 4) {
        asm("v_add_u32 %0, %4, %4\n\tv_add_u32 %1, %0, %0\n\tv_add_u32 %2, %1, %1\n\tv_add_u32 %3, %2, %2"
            : "=&v"(m2), "=&v"(m1), "=&v"(m0), "=&v"(nx) : "v"(m3));
        // (mask & 0x80000000) ^ value as ONE v_bitop3_b32 (truth table 0x6c); written as and + xor the compiler only
        // sometimes fuses them
        v[j] = flip_by(MUL ? v[j] * nc : v[j], m3);
        v[j - 1] = flip_by(MUL ? v[j - 1] * nc : v[j - 1], m2);
        v[j - 2] = flip_by(MUL ? v[j - 2] * nc : v[j - 2], m1);
        v[j - 3] = flip_by(MUL ? v[j - 3] * nc : v[j - 3], m0);
        m3 = nx;
    }
}


__device__ __forceinline__ int row_swz(int p) { return ((p >> 1) & 3) ^ ((p >> 4) & 3); }

__device__ __forceinline__ void wave_lds_sync() {
    // a wave's LDS operations execute in order: only the compiler has to be kept from reordering across the point
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ------------------------------------------------------------------------------------
// The exchange between the two layouts ("x4").  LDS time is the second budget of these kernels (MI355X_MICROARCH.md,
// LDS: a ds_write_b32 costs the CU 4 cycles per wave-instruction -- 2 for the array, 2 more to move its ADDRESS
// register --, a ds_write_b128 13, against 2 for ds_write_addtid_b32, which takes its address from M0 + offset +
// 4 * lane).  BOTH directions therefore store with sixteen ds_write_addtid_b32 -- register i of all 64 lanes is one
// contiguous 256-byte chunk whose base is an immediate -- and read with what the other layout's registers allow:
//     R -> C: chunk j at dword x4_a(j) (lane = row p = b + 4 r); C lane (b, j) reads r = 0 .. 15 at x4_a(j) + b + 4 r
//             as eight ds_read2_b32: 32 + 32 = 64 LDS cycles per tile
//     C -> R: chunk r at dword x4_b(r) (lane = 16 b + j); R lane (b, r) reads j = 4 g .. 4 g + 3 as ONE ds_read_b128 at
//             x4_b(r) + 16 b + 4 g: 32 + 16 = 48 cycles
// against 84 / 80 for the ds_write_b128 + ds_read_b32 / ds_write_b32 + ds_read_b128 pairs this replaced, and with no
// address registers on the store side.  The chunk bases carry the bank swizzle (x4_a = 66 j: two dwords of padding per
// chunk; x4_b mod 16 = 4 (r & 3), chunks ordered so that the padding is 12 dwords in all): every pattern is
// conflict-free under the per-instruction lane groups, enumerated by tools/x4_layout_check.py.
// ------------------------------------------------------------------------------------
constexpr int X4_DWORDS = 1088;      // (1056 for the two maps above; 1084 for x4_d below)
__host__ __device__ constexpr int x4_a(int j) { return 66 * j; }
__host__ __device__ constexpr int x4_b(int r) { return 64 * (4 * (r & 3) + (r >> 2)) + 4 * (r & 3); }

template <bool TO_COLS, int H>
__device__ __forceinline__ void x4_store8(const float (&v)[16], unsigned tb_bytes) {
#define X4_OFF(i) "i"(4 * (TO_COLS ? x4_a(H + i) : x4_b(H + i)))
    asm volatile(
        "s_mov_b32 m0, %8\n\ts_nop 0\n\t"
        "ds_write_addtid_b32 %0 offset:%9\n\tds_write_addtid_b32 %1 offset:%10\n\t"
        "ds_write_addtid_b32 %2 offset:%11\n\tds_write_addtid_b32 %3 offset:%12\n\t"
        "ds_write_addtid_b32 %4 offset:%13\n\tds_write_addtid_b32 %5 offset:%14\n\t"
        "ds_write_addtid_b32 %6 offset:%15\n\tds_write_addtid_b32 %7 offset:%16"
        : : "v"(v[H]), "v"(v[H + 1]), "v"(v[H + 2]), "v"(v[H + 3]), "v"(v[H + 4]), "v"(v[H + 5]), "v"(v[H + 6]),
            "v"(v[H + 7]), "s"(tb_bytes), X4_OFF(0), X4_OFF(1), X4_OFF(2), X4_OFF(3), X4_OFF(4), X4_OFF(5), X4_OFF(6),
            X4_OFF(7)
        : "memory", "m0");
#undef X4_OFF
}

// per-lane read bases (dwords into the wave's buffer) of the two directions
__device__ __forceinline__ int x4_cols_base(int lane) { return x4_a(lane & 15) + (lane >> 4); }
__device__ __forceinline__ int x4_rows_base(int lane) { return x4_b(lane >> 2) + 16 * (lane & 3); }

// (the wave's LDS operations execute in order and the asm is a compiler barrier: nothing else is needed between
// the stores and the reads, or between the reads and the next stores)
template <bool TO_COLS> __device__ __forceinline__ void x4_store(const float (&v)[16], unsigned tb_bytes) {
#ifndef XGPR_ABL_VALUONLY
    x4_store8<TO_COLS, 0>(v, tb_bytes);
    x4_store8<TO_COLS, 8>(v, tb_bytes);
#endif
}
__device__ __forceinline__ void x4_load_cols(float (&v)[16], const float *cbase) {
#ifdef XGPR_ABL_VALUONLY
    #pragma unroll
    for (int g = 0; g < 16; g++) asm volatile("" : "+v"(v[g]));
    return;
#endif
    #pragma unroll
    for (int r = 0; r < 16; r++) v[r] = cbase[4 * r];
}
__device__ __forceinline__ void x4_load_rows(float (&v)[16], const float *rbase) {
#ifdef XGPR_ABL_VALUONLY
    #pragma unroll
    for (int g = 0; g < 16; g++) asm volatile("" : "+v"(v[g]));
    return;
#endif
    #pragma unroll
    for (int g = 0; g < 4; g++) {
        const float4 t = *reinterpret_cast<const float4 *>(rbase + 4 * g);
        v[4 * g] = t.x; v[4 * g + 1] = t.y; v[4 * g + 2] = t.z; v[4 * g + 3] = t.w;
    }
}

constexpr int TBUF_FLOATS = X4_DWORDS;       // the wave-private exchange buffer, in floats

// stores registers 0 .. N - 1 only (N = 2, 4, 8): the first exchange of a tile whose P / 64 distinct input registers
// are replicated over the 1024 / P transforms it holds
template <int N> __device__ __forceinline__ void x4_store_first(const float (&v)[16], unsigned tb_bytes) {
    static_assert(N == 1 || N == 2 || N == 4 || N == 8, "");
#define X4_OFFB(i) "i"(4 * x4_b(i))
    if constexpr (N == 1)           // P <= 64: one distinct register, lane l holds element l mod P -- the chunk is the row, replicated
        asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tds_write_addtid_b32 %0 offset:%2"
                     : : "v"(v[0]), "s"(tb_bytes), X4_OFFB(0) : "memory", "m0");
    else if constexpr (N == 2)
        asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tds_write_addtid_b32 %0 offset:%3\n\tds_write_addtid_b32 %1 offset:%4"
                     : : "v"(v[0]), "v"(v[1]), "s"(tb_bytes), X4_OFFB(0), X4_OFFB(1) : "memory", "m0");
    else if constexpr (N == 4)
        asm volatile("s_mov_b32 m0, %4\n\ts_nop 0\n\tds_write_addtid_b32 %0 offset:%5\n\tds_write_addtid_b32 %1 offset:%6\n\t"
                     "ds_write_addtid_b32 %2 offset:%7\n\tds_write_addtid_b32 %3 offset:%8"
                     : : "v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3]), "s"(tb_bytes), X4_OFFB(0), X4_OFFB(1), X4_OFFB(2), X4_OFFB(3)
                     : "memory", "m0");
    else x4_store8<false, 0>(v, tb_bytes);
#undef X4_OFFB
}
// read base of an R lane for that first exchange: its row's data sits in chunk r mod N
template <int N> __device__ __forceinline__ int x4_rows_base_first(int lane) {
    return x4_b((lane >> 2) & (N - 1)) + 16 * (lane & 3);      // (N = 1: dwords 16 (l & 3) .. + 15 of the one chunk = elements (16 l + j) mod 64)
}

// Register-local butterfly stages as PACKED adds on the natural register pairs (2 k, 2 k + 1): one v_pk_add_f32 does
// two butterfly outputs, and with the VOP3P operand selectors a stride-1 butterfly (a, b) -> (a + b, a - b) inside one
// pair is a single instruction (low result = src0.lo + src1.hi, high result = src0.lo - src1.hi).  The packed add
// occupies the vector pipe exactly as long as two plain adds (tools/valu_microbench.hip: 2.04 ns against 2 x 0.97), but
// this kernel is not bound by pipe occupancy alone: at three waves per SIMD a wave issues at most one vector instruction
// every four cycles, and what it runs at is its own instruction COUNT -- the SLP vectoriser's pairing (288 of the 384
// add / subs as 144 v_pk_add_f32 plus ~60 v_mov_b32 to line up its pairs) measured 2.8 % faster than 384 plain
// instructions, and this form needs no moves: 192 instructions per tile.  a + (-b) is a - b bit for bit.
typedef float v2f_t __attribute__((ext_vector_type(2)));

template <int Q> __device__ __forceinline__ void bfly_stage(float (&v)[16]) {
#ifdef XGPR_ABL_SLPBFLY
    #pragma unroll
    for (int j = 0; j < 16; j++)
        if (!(j & Q)) bfly(v[j], v[j + Q]);
#else
    if constexpr (Q == 1) {
        #pragma unroll
        for (int k = 0; k < 8; k++) {
            v2f_t p = {v[2 * k], v[2 * k + 1]}, d;
            asm("v_pk_add_f32 %0, %1, %1 op_sel:[0,1] op_sel_hi:[0,1] neg_hi:[0,1]" : "=v"(d) : "v"(p));
            v[2 * k] = d.x; v[2 * k + 1] = d.y;
        }
    } else {
        constexpr int QP = Q / 2;                      // stride in pairs
        #pragma unroll
        for (int k = 0; k < 8; k++) {
            if (k & QP) continue;
            v2f_t a = {v[2 * k], v[2 * k + 1]}, b = {v[2 * (k + QP)], v[2 * (k + QP) + 1]}, sm, df;
            asm("v_pk_add_f32 %0, %1, %2" : "=v"(sm) : "v"(a), "v"(b));
            asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(df) : "v"(a), "v"(b));
            v[2 * k] = sm.x; v[2 * k + 1] = sm.y;
            v[2 * (k + QP)] = df.x; v[2 * (k + QP) + 1] = df.y;
        }
    }
#endif
}

// the rows-layout half of a round: sign flip (x normaliser for odd log2 P), strides 1..8 register-local, strides 16
// and 32 as quad_perm DPP (lane bits 0, 1 in layout R) in the one-instruction form that leaves the factor
// (-1)^(bit0 + bit1) of the lane on the result (xstage_neg): the caller folds it into the next round's sign word and,
// after the last round, into chi
template <int LOG2P>
__device__ __forceinline__ void rows_half(float (&v)[16], uint32_t swd, float nc, float sg1, float sg2) {
    flip_signs16<(LOG2P & 1) != 0>(v, swd, nc);
    bfly_stage<1>(v); bfly_stage<2>(v); bfly_stage<4>(v); bfly_stage<8>(v);
#ifdef XGPR_ABL_SWAPLAYOUT       // timing-only switch (results wrong): strides 16 / 32 as two permlane-swap layout changes + two local stages
    #pragma unroll
    for (int r = 0; r < 16; r += 2) {
        auto t = __builtin_amdgcn_permlane16_swap(as_i(v[r]), as_i(v[r + 1]), false, false);
        v[r] = as_f(t[0]); v[r + 1] = as_f(t[1]);
    }
    #pragma unroll
    for (int r = 0; r < 16; r += 4) {
        auto t = __builtin_amdgcn_permlane32_swap(as_i(v[r]), as_i(v[r + 2]), false, false);
        v[r] = as_f(t[0]); v[r + 2] = as_f(t[1]);
        auto u = __builtin_amdgcn_permlane32_swap(as_i(v[r + 1]), as_i(v[r + 3]), false, false);
        v[r + 1] = as_f(u[0]); v[r + 3] = as_f(u[1]);
    }
    bfly_stage<1>(v); bfly_stage<2>(v);
    (void)sg1; (void)sg2;
#elif !defined(XGPR_ABL_NODPP)          // timing-only switch (results wrong): what the two quad_perm stages cost
    xstage_neg<1>(v, sg1);
    xstage_neg<2>(v, sg2);
#endif
}

// the columns-layout half: strides 64 .. P / 2, register-local
template <int LOG2P> __device__ __forceinline__ void cols_half(float (&v)[16]) {
    constexpr int P = 1 << LOG2P;
    if constexpr (P > 64) bfly_stage<1>(v);
    if constexpr (P > 128) bfly_stage<2>(v);
    if constexpr (P > 256) bfly_stage<4>(v);
    if constexpr (P > 512) bfly_stage<8>(v);
}

// sign words of a tile in layout R: bit j of sw[s] = sign of element 16 * lane + j of diagonal s,
// i.e. 16-bit slice `lane` of the tile's sixteen 64-bit masks (little endian)
__device__ __forceinline__ void load_sign_words(uint32_t (&sw)[3], const uint64_t *masks, int MW, int b, int lane) {
    const uint16_t *m16 = reinterpret_cast<const uint16_t *>(masks);
    #pragma unroll
    for (int s = 0; s < 3; s++) sw[s] = m16[((long)s * MW + (long)b * 16) * 4 + lane];
}

// KEEP_SIGN: leave the last round's xstage_neg factor on the result -- element e of the tile (layout C: lane =
// e mod 64) then carries (-1)^(bit4(lane) + bit5(lane)), see sorf_kept_sign -- for callers that fold it into chi.
__device__ __forceinline__ float sorf_kept_sign(int lane) { return (((lane >> 4) ^ (lane >> 5)) & 1) ? -1.0f : 1.0f; }

// v enters and leaves in layout C; sw are the words of load_sign_words (unmodified)
template <int LOG2P, bool KEEP_SIGN = false>
__device__ __forceinline__ void wave_sorf_t(float (&v)[16], const uint32_t (&sw)[3], float *tb, float nc, int lane) {
    static_assert(LOG2P >= 7 && LOG2P <= 10, "two-layout SORF is for 128 <= P <= 1024");
    constexpr int P = 1 << LOG2P;
    // strides 16 and 32 (lane bits 0, 1 in layout R) go through xstage_neg: one instruction per register, and the
    // sign it leaves on a lane is folded into the next round's Rademacher word (rounds 2, 3) or undone once (round 3)
    const float sg1 = (lane & 1) ? -1.0f : 1.0f, sg2 = (lane & 2) ? -1.0f : 1.0f;
    const uint32_t par = xneg_parity(lane);
    // (wave-uniform by construction -- the buffer is per wave --, made so for the compiler: it goes into M0)
    const unsigned tb_bytes = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(size_t)(lds_ptr_t)tb);
    const float *cbase = tb + x4_cols_base(lane), *rbase = tb + x4_rows_base(lane);
    #pragma unroll
    for (int s = 0; s < 3; s++) {
        if constexpr (P < 1024) {
            if (s == 0) {       // only P / 64 of the 16 input registers are distinct (the tile holds 1024 / P transforms)
                x4_store_first<P / 64>(v, tb_bytes);
                x4_load_rows(v, tb + x4_rows_base_first<P / 64>(lane));
            } else {
                x4_store<false>(v, tb_bytes);
                x4_load_rows(v, rbase);
            }
        } else {
            x4_store<false>(v, tb_bytes);
            x4_load_rows(v, rbase);
        }
        rows_half<LOG2P>(v, s == 0 ? sw[0] : sw[s] ^ (par & 0xffffu), nc, sg1, sg2);
        if (s == 2 && !KEEP_SIGN) {
            #pragma unroll
            for (int j = 0; j < 16; j++) v[j] = as_f(as_i(v[j]) ^ (int)(par & 0x80000000u));
        }
        x4_store<true>(v, tb_bytes);
        x4_load_cols(v, cbase);
        cols_half<LOG2P>(v);
    }
}

// ------------------------------------------------------------------------------------
// P <= 256: NO cross-lane stage at all.  A transform of 128 or 256 elements has 7 or 8 butterfly stages and a lane holds
// 16 elements, so two layouts cover every stride register-locally -- if the second one takes the index bits the first
// leaves over:
//   layout R  (as above):            lane = t[9:4] = 16 t[9:8] + t[7:4],  register = t[3:0]      strides 1, 2, 4, 8
//   layout C2 ("transposed columns"): lane = 16 t[9:8] + t[3:0],          register = t[7:4]      strides 16, 32, 64, 128
// (t[9:8] = which of the tile's 1024 / P transforms; for P = 128 bit 7 belongs to it as well and stride 128 is not a
// stage).  Against the C layout of the larger widths that removes the two quad_perm DPP stages of every round (96
// v_fmac_f32_dpp per tile: 19 % of the priced vector time of the convolution kernel at P = 256,
// profiles/r4_conv_inst_table.json), the parity bookkeeping they need, and makes BOTH exchanges the cheap kind: R <-> C2
// is a 16 x 16 transpose inside every group of 16 lanes, the same map in both directions -- sixteen
// ds_write_addtid_b32 (register i of all lanes = chunk i at dword x4_d(i)), then lane l reads ITS sixteen values as four
// ds_read_b128 at x4_d(l & 15) + 16 (l >> 4): 32 + 16 LDS cycles each way (the R -> C exchange above costs 64).
// Stage order and roundings are unchanged (h = 1, 2, 4, ...): results are bit-identical to wave_sorf / wave_sorf_t.
// Chunk bases: 64-dword chunks in slot order with 4 s(i) dwords of skew, s(i) = 4 (i & 3) + {2, 0, 1, 3}[i >> 2]: the
// sixteen lanes of every ds_read_b128 lane group land on sixteen different 4-bank slots (tools/x4_layout_check.py).
// The tile leaves in C2: element index of (lane, register r) = c2_elem(lane, r), NOT 64 r + lane.
// ------------------------------------------------------------------------------------
__host__ __device__ constexpr int x4_d(int i) { return 68 * (4 * (i & 3) + ((0x3102 >> (4 * (i >> 2))) & 15)); }
__host__ __device__ constexpr int c2_elem(int lane, int r) { return ((lane >> 4) << 8) | (r << 4) | (lane & 15); }
__device__ __forceinline__ int x4t_base(int lane) { return x4_d(lane & 15) + 16 * (lane >> 4); }

template <int H>
__device__ __forceinline__ void x4t_store8(const float (&v)[16], unsigned tb_bytes) {
#define X4_OFFD(i) "i"(4 * x4_d(H + i))
    asm volatile(
        "s_mov_b32 m0, %8\n\ts_nop 0\n\t"
        "ds_write_addtid_b32 %0 offset:%9\n\tds_write_addtid_b32 %1 offset:%10\n\t"
        "ds_write_addtid_b32 %2 offset:%11\n\tds_write_addtid_b32 %3 offset:%12\n\t"
        "ds_write_addtid_b32 %4 offset:%13\n\tds_write_addtid_b32 %5 offset:%14\n\t"
        "ds_write_addtid_b32 %6 offset:%15\n\tds_write_addtid_b32 %7 offset:%16"
        : : "v"(v[H]), "v"(v[H + 1]), "v"(v[H + 2]), "v"(v[H + 3]), "v"(v[H + 4]), "v"(v[H + 5]), "v"(v[H + 6]),
            "v"(v[H + 7]), "s"(tb_bytes), X4_OFFD(0), X4_OFFD(1), X4_OFFD(2), X4_OFFD(3), X4_OFFD(4), X4_OFFD(5), X4_OFFD(6),
            X4_OFFD(7)
        : "memory", "m0");
#undef X4_OFFD
}
__device__ __forceinline__ void x4t_store(const float (&v)[16], unsigned tb_bytes) {
#ifndef XGPR_ABL_VALUONLY
    x4t_store8<0>(v, tb_bytes);
    x4t_store8<8>(v, tb_bytes);
#endif
}
// (the read side is x4_load_rows(v, tb + x4t_base(lane)): four ds_read_b128 of consecutive dwords)

// the two halves of a round without cross-lane stages.  Layout R's register-local stages: strides 1, 2, 4, 8 -- as many of them as the
// transform has (P < 16: the lane's sixteen registers hold 16 / P whole transforms)
template <int LOG2P> __device__ __forceinline__ void local_stages(float (&v)[16]) {
    bfly_stage<1>(v);
    if constexpr (LOG2P > 1) bfly_stage<2>(v);
    if constexpr (LOG2P > 2) bfly_stage<4>(v);
    if constexpr (LOG2P > 3) bfly_stage<8>(v);
}
template <int LOG2P>
__device__ __forceinline__ void rows_half_t(float (&v)[16], uint32_t swd, float nc) {
    flip_signs16<(LOG2P & 1) != 0>(v, swd, nc);
    local_stages<LOG2P>(v);
}
template <int LOG2P> __device__ __forceinline__ void cols_half_t(float (&v)[16]) {
    static_assert(LOG2P <= 8, "the transposed-columns layout serves P <= 256");
    if constexpr (LOG2P > 4) bfly_stage<1>(v);                        // stride 16
    if constexpr (LOG2P > 5) bfly_stage<2>(v);                        // stride 32
    if constexpr (LOG2P > 6) bfly_stage<4>(v);                        // stride 64
    if constexpr (LOG2P > 7) bfly_stage<8>(v);                        // stride 128
}

// Rademacher flips of a lane's 16 elements (layout R) through sixteen wave-uniform 64-bit lane masks in SGPRs: bit l of
// fm[j] = sign of element j of lane l (sign_lane_masks builds them from the lane's sign word by ballots).  One v_cndmask_b32
// with a negated source per element, against the v_add_u32 + v_bitop3_b32 pair of flip_signs16 -- for callers whose wave keeps
// one tile's signs for a whole loop and has 32 SGPRs to spare (fused_ztz.inc: 1.5 % of the fused matvec per round converted).
__device__ __forceinline__ void sign_lane_masks(uint64_t (&fm)[16], uint32_t swd) {
    #pragma unroll
    for (int j = 0; j < 16; j++) fm[j] = __builtin_amdgcn_ballot_w64(((swd >> j) & 1u) != 0u);
}
__device__ __forceinline__ void flip_signs16_masks(float (&v)[16], const uint64_t (&fm)[16]) {
    #pragma unroll
    for (int j = 0; j < 16; j++) v[j] = __builtin_amdgcn_inverse_ballot_w64(fm[j]) ? -v[j] : v[j];
}

// v enters in layout C (the coalesced load, replicated over the tile's transforms) and LEAVES in layout C2;
// sw are the words of load_sign_words, unmodified (no stage leaves a sign behind).  MROUND >= 0: that round's flips go
// through the SGPR lane masks fm (even log2 P only: no normaliser to multiply in)
// P = 32, 64: rows only TOO -- strides 16 / 32 are lane bits 0 / 1 of layout R (quad_perm DPP: xstage_neg), one / two such stages per round
// cost less than the two exchanges a column half would need (fused matvec: 5-10 % at d = 64 / 32, LDS active 0.56 -> 0.2).  The stages leave
// (-1)^(bit0 [+ bit1]) of the lane on the result: rd_parity; the CALLER folds it into the sign words of rounds 2 and 3 once
// (sw[s] ^= rd_parity & 0xffff) and into chi.
template <int LOG2P> __device__ __forceinline__ uint32_t rd_parity(int lane) {
    if constexpr (LOG2P == 6) return xneg_parity(lane);
    else if constexpr (LOG2P == 5) return (lane & 1) ? 0xffffffffu : 0u;
    else return 0u;
}

template <int LOG2P, int MROUND = -1>
__device__ __forceinline__ void wave_sorf_c2(float (&v)[16], const uint32_t (&sw)[3], float *tb, float nc, int lane,
                                             const uint64_t (&fm)[16]) {
    static_assert(MROUND < 0 || (LOG2P & 1) == 0, "mask flips carry no normaliser");
    constexpr int P = 1 << LOG2P;
    constexpr int N0 = P >= 128 ? P / 64 : 1;           // distinct input registers (layout C, replicated over the tile's transforms)
    constexpr bool RONLY = LOG2P <= 6;                  // P <= 64: the tile stays in layout R (P = 32, 64: with DPP stages; sw pre-folded)
    const unsigned tb_bytes = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(size_t)(lds_ptr_t)tb);
    const float *tbase = tb + x4t_base(lane);
    const float sg1 = (lane & 1) ? -1.0f : 1.0f, sg2 = (lane & 2) ? -1.0f : 1.0f;
    #pragma unroll
    for (int s = 0; s < 3; s++) {
        if (s == 0) {           // C -> R: only N0 of the 16 input registers are distinct
            x4_store_first<N0>(v, tb_bytes);
            x4_load_rows(v, tb + x4_rows_base_first<N0>(lane));
        } else if (!RONLY) {    // C2 -> R
            x4t_store(v, tb_bytes);
            x4_load_rows(v, tbase);
        }
        if (s == MROUND) {
            flip_signs16_masks(v, fm);
            local_stages<LOG2P>(v);
        } else rows_half_t<LOG2P>(v, sw[s], nc);
        if constexpr (LOG2P >= 5 && LOG2P <= 6) xstage_neg<1>(v, sg1);
        if constexpr (LOG2P == 6) xstage_neg<2>(v, sg2);
        if constexpr (!RONLY) {
            x4t_store(v, tb_bytes);         // R -> C2
            x4_load_rows(v, tbase);
            cols_half_t<LOG2P>(v);
        }
    }
}

// one entry point for the kernels: T path for P >= 128 when a buffer is supplied, register path otherwise
// The transform runs at raised wave priority: with two waves per SIMD the arbiter then lets the wave that is in
// its exchange-heavy transform issue ahead of the one doing cos/sin or the float64 update, which shortens the
// chains of dependent LDS round trips (fused matvec: 2.44 -> 2.38 ms per 262144 rows; any level above the
// rest of the kernel measures the same).
// RAISE = false: no priority change -- the stand-alone feature operator, whose waves have nothing to wait for each
// other about and whose 16 KiB of stores per item should leave as early as possible, measures 4-5 % better without
// (1.72 -> 1.64 ms per 131072 x 8192 float64 rows).
template <int LOG2P, bool TP, bool KEEP_SIGN = false, bool RAISE = true>
__device__ __forceinline__ void tile_sorf(float (&v)[16], cmask_t mk, const uint32_t (&sw)[3], float *tb, int MW,
                                          float nc, int lane) {
    static_assert(!KEEP_SIGN || (TP && LOG2P >= 7), "only the two-layout path leaves a sign to keep");
    if (RAISE) __builtin_amdgcn_s_setprio(1);
    if constexpr (TP && LOG2P >= 7) wave_sorf_t<LOG2P, KEEP_SIGN>(v, sw, tb, nc, lane);
    else wave_sorf<LOG2P>(v, mk, MW, nc, lane);
    if (RAISE) __builtin_amdgcn_s_setprio(0);
}

// load one datapoint (or k-mer window) into the wave tile: element (64 r + l) mod P, zero
// padded from d up to P, replicated over the tile's 1024 / P transforms.  The padded lanes
// read element 0 and are zeroed by a select, so there is no branch around the loads.
template <int LOG2P>
__device__ __forceinline__ void wave_load(float (&v)[16], const float *__restrict__ xe, int d, int lane) {
    constexpr int P = 1 << LOG2P;
    if constexpr (P >= 64) {
        constexpr int RP = P / 64;
        #pragma unroll
        for (int r = 0; r < RP; r++) {
            const int e = r * 64 + lane;
            const bool ok = e < d;
            float t = xe[ok ? e : 0];
            v[r] = ok ? t : 0.0f;
        }
        #pragma unroll
        for (int r = RP; r < 16; r++) v[r] = v[r & (RP - 1)];
    } else {
        const int e = lane & (P - 1);
        const bool ok = e < d;
        float t = xe[ok ? e : 0];
        t = ok ? t : 0.0f;
        #pragma unroll
        for (int r = 0; r < 16; r++) v[r] = t;
    }
}

// wave_load in two steps, so that a k-mer loop can issue the loads of the NEXT window before it starts on the
// current one (only the P / 64 distinct registers are kept in flight): wave_load_base fetches, wave_expand
// replicates over the tile's 1024 / P transforms.  wave_load == wave_expand(wave_load_base).
template <int LOG2P> struct TileBase { static constexpr int N = (1 << LOG2P) >= 64 ? (1 << LOG2P) / 64 : 1; };

// The window [xe, xe + d) is described by a buffer resource (raw, num_records = 4 d bytes): elements past d read as 0.0f
// by the hardware's range check -- no compare / select per register, and ONE lane offset for all registers (the
// 256-byte steps ride in the instruction's immediate).  xe must be wave-uniform (the resource lives in SGPRs).
// These are ordinary compiler-visible loads: the compiler counts them and places the s_waitcnt itself.  (Rounds 2-3
// issued register-targeted loads from inline assembly here; the compiler cannot see that such a register is not yet
// written and moved copies of them in front of the wait -- tools/lint_asm_loads.py keeps that form out of the tree.)
template <int LOG2P>
__device__ __forceinline__ void wave_load_base(float (&nx)[TileBase<LOG2P>::N], const float *__restrict__ xe, int d, int lane) {
    constexpr int P = 1 << LOG2P;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(xe), 0, d * 4, 0x00020000);
    if constexpr (P >= 64) {
        #pragma unroll
        for (int r = 0; r < P / 64; r++) nx[r] = as_f(__builtin_amdgcn_raw_buffer_load_b32(rs, lane * 4 + r * 256, 0, 0));
    } else {
        nx[0] = as_f(__builtin_amdgcn_raw_buffer_load_b32(rs, (lane & (P - 1)) * 4, 0, 0));
    }
}

template <int LOG2P>
__device__ __forceinline__ void wave_expand(float (&v)[16], const float (&nx)[TileBase<LOG2P>::N]) {
    constexpr int N = TileBase<LOG2P>::N;
    #pragma unroll
    for (int r = 0; r < 16; r++) v[r] = nx[r & (N - 1)];
}

// cos/sin of the 16 arguments of a tile.  The common path is branch-free; the rare large
// arguments (|v| >= 2^18, inf, nan) are fixed up behind ONE wave-level test.
__device__ __forceinline__ void tile_sincos_scalar(const float (&arg)[16], float (&sn)[16], float (&cs)[16]) {
    // one running maximum of |arg| (v_max3_f32: two arguments per instruction) instead of sixteen compares.  A NaN
    // argument drops out of the maximum and takes the common path, which returns NaN for it as the rare path would.
    float amax = 0.0f;
    #pragma unroll
    for (int r = 0; r < 16; r += 2) {
        sincos_f32_core(arg[r], sn[r], cs[r]);
        sincos_f32_core(arg[r + 1], sn[r + 1], cs[r + 1]);
        amax = __builtin_fmaxf(__builtin_fmaxf(fabsf(arg[r]), fabsf(arg[r + 1])), amax);
    }
    const bool big = !(amax < SINCOS_FAST_LIMIT);
    if (__builtin_expect(__any(big), 0)) {
        #pragma unroll
        for (int r = 0; r < 16; r++) {
            float s2, c2;
            sincos_f32_big(arg[r], s2, c2);
            const bool b = !(fabsf(arg[r]) < SINCOS_FAST_LIMIT);
            sn[r] = b ? s2 : sn[r];
            cs[r] = b ? c2 : cs[r];
            __builtin_amdgcn_sched_barrier(0);   // cold path: one element at a time, no extra registers
        }
    }
}

// cos/sin of the 16 arguments of a tile, the form the kernels use: the range reduction of sincos_f32_core on register pairs: t = v * c_hi - rint(v * c_hi) + v * c_lo as
// v_pk_mul_f32 / v_pk_fma_f32 / v_pk_fma_f32 (the constants ride in one 64-bit pair, picked by the operand selectors),
// IEEE-identical to the scalar forms: 9 instead of 12 instructions per two frequencies.
__device__ __forceinline__ void tile_sincos(const float (&arg)[16], float (&sn)[16], float (&cs)[16]) {
#ifdef XGPR_ABL_PLAINSINCOS
    tile_sincos_scalar(arg, sn, cs);
#else
    const float inv2pi_hi = 0.15915494f, inv2pi_lo = (float)(0.15915494309189535 - (double)0.15915494f);
    v2f_t cc = {inv2pi_hi, inv2pi_lo};
    asm volatile("" : "+v"(cc));               // one register pair, not re-materialised per use
    float amax = 0.0f;
    float t[16];
    #pragma unroll
    for (int r = 0; r < 16; r += 2) {
        const v2f_t v = {arg[r], arg[r + 1]};
        v2f_t q, k, u;
        asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(q) : "v"(v), "v"(cc));
        k.x = __builtin_rintf(q.x); k.y = __builtin_rintf(q.y);
        asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[1,0,1] neg_lo:[0,0,1] neg_hi:[0,0,1]" : "=v"(u) : "v"(v), "v"(cc), "v"(k));
        asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "=v"(u) : "v"(v), "v"(cc), "0"(u));
        t[r] = u.x; t[r + 1] = u.y;
        amax = __builtin_fmaxf(__builtin_fmaxf(fabsf(arg[r]), fabsf(arg[r + 1])), amax);
    }
    // rare path (2^18 <= |v|, inf, nan), behind ONE wave-level test and BEFORE the 32 results exist, so that it costs
    // the kernels no registers: the angle in revolutions is redone in double precision (sincos_turns_big)
    const bool big = !(amax < SINCOS_FAST_LIMIT);
    if (__builtin_expect(__any(big), 0)) {
        asm volatile("; XGPR_MARK cold_begin");
        #pragma unroll
        for (int r = 0; r < 16; r++) {
            const float t2 = sincos_turns_big(arg[r]);
            t[r] = !(fabsf(arg[r]) < SINCOS_FAST_LIMIT) ? t2 : t[r];
            asm volatile("" : "+v"(t[r]));       // one element at a time: the select is done before the next one starts
            __builtin_amdgcn_sched_barrier(0);
        }
        asm volatile("; XGPR_MARK cold_end");
    }
    #pragma unroll
    for (int r = 0; r < 16; r++) {
        sn[r] = __builtin_amdgcn_sinf(t[r]);
        cs[r] = __builtin_amdgcn_cosf(t[r]);
    }
#endif
}

struct WaveArgs {
    const float *x; double *out; float *outf;
    const uint64_t *masks; const float *chi; const int32_t *seqlen;
    const double *vec; double *wpart;
    long n; long row_stride; long F;
    int d; int kmer_stride; int conv_width; int scaling_type;
    int MW; int nb;           // masks per diagonal; wave tiles (1024 frequencies) per datapoint
    int G;                    // matvec: datapoints in flight per workgroup
    int fit_intercept;
    float nc; float chi_scale; // per-round normaliser (odd log2 P) / folded normaliser^3 (even)
    double scale;
    double *tpart;            // two-pass matvec: per-(datapoint, tile) partial dots [rows, nb]
    int add_to_slab;          // two-pass matvec: slabs accumulate over row windows
    double *grad; double sigma;   // gradient operators
    const int32_t *order;         // convolution operators: processing order of the sequences (or null)
    int dma1;                     // three-wave kernel: rows are not whole aligned 16-byte groups -- fetch them float by float
    float *gradf;                 // OUT_GRAD_ROWS: the float32 gradient rows (the feature rows go to outf)
    const uint8_t *tokens; int vocab;   // token forms of the sequence kernels: tokens [n, row_stride]; x is then the table [vocab, kmer_stride]
};

