// edit_proj.inc -- part of xgpr_hip.hip (included inside its anonymous namespace, after var_scan.inc): the LINEAR map next to the
// quadratic form of var_scan.inc -- z'^T P of every single-token SUBSTITUTION, DELETION and INSERTION for a caller's matrix
// P [nvar, K] over the first nvar feature columns of the SEQUENCE and GRAPH kernels (xgpr_conv_token_subst_proj_f32,
// xgpr_conv_token_indel_proj_f32, include/xgpr_hip/edit_proj.h; DESIGN.md 3.26).
//
// Notation of var_scan.inc.  A mutant's columns are z' = b + r' delta (b = z_i and r' = r for a substitution), so
//     out[row, :] = b~[i, :] + r' (delta[row, :] P)          with the caller's b~[i] = b^T P, one row of K values per sequence and row set.
// The row sets, the slabs, the workspace and the delta kernels are those of var_scan.inc, UNCHANGED (var_scan_slabs launches them); the
// slab's second kernel is
//   var_proj_kernel<MAP>    four waves, one 16-row tile each, under the row map of the row set.  Y = Delta P on v_mfma_f64_16x16x4_f64 with
//       the operand maps, the panel staging and the double buffering of sv_quad_body: 64 columns of P at a time, P passing through LDS in
//       panels of 32 k x 64 columns (k >= nvar and columns >= K are zeros in the panel and are never read from P or Delta).  After a column
//       block's last panel lane (c, g) holds Y[row g + 4 r][column 16 ct + c] in D register r of tile ct and stores
//       out[row, col] = b~[i, col] + r' Y: one multiply, one add, 16 consecutive doubles per row and tile.  No reduction across lanes, no
//       atomics, no second pass.  Dead rows -- past the slab, or of a slot past its sequence's length -- are never read from the workspace
//       and store K times +0.0, or K quiet NaNs for the deletions p < s of a sequence with s == conv_width; a wave with no live row issues
//       no MFMA, a workgroup with none stores and leaves.
// A row's bits depend on its own delta, P, b~ and r' alone: every column is one chain of MFMAs over k ascending, whatever n, the slab cut,
// the row's place in a tile or the number of column blocks.
// ------------------------------------------------------------------------------------
constexpr long EP_MAX_K = 2048;

struct EditProjArgs {
    VarScanArgs v;                // s, delta, row_lo, row_hi, nvar as for the variance scans; vm, u, q, out unused
    const double *pm, *b;         // [nvar, K] with row stride pm_stride; [n, K]
    double *out;                  // [rows of the row set, K]
    long pm_stride;
    int K;
};

template <class MAP>
__global__ __launch_bounds__(256) void var_proj_kernel(EditProjArgs q) {
    constexpr int NT = 256;
    constexpr int VPT = SV_KC * SV_CB / NT;              // panel elements staged per thread
    __shared__ __attribute__((aligned(16))) double vs[2][SV_KC * SV_VS];
    const VarScanArgs &p = q.v;
    const EditScanArgs &s = p.s;
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nvar = p.nvar, K = q.K;
    const long t0 = p.row_lo + (long)blockIdx.x * 64 + 16 * w;       // the wave's first row of out
    // ---- the lane's A row: row c of the tile
    const long ga = t0 + c;
    int live = 0;
    long ia = 0;
    int nka = 1;
    double dead = 0.0;
    if (ga < p.row_hi) {
        const SvRow info = MAP::at(p, ga);
        ia = info.live ? info.i : 0;
        nka = info.nk;
        live = info.live;
        dead = info.dead;
    }
    // a workgroup none of whose 64 rows is live stores its rows' zeros (or NaNs) and leaves; a wave without a live row keeps staging P
    // and meeting the barriers, but skips its matrix instructions (both decisions are uniform where they must be)
    if (!__syncthreads_or(live)) {
        for (int r = 0; r < 16; r++) {
            const double d = __shfl(dead, r);            // (lane r < 16: c == r, the row the lane looked up)
            const long row = t0 + r;
            if (row < p.row_hi)
                for (int col = lane; col < K; col += 64) q.out[row * K + col] = d;
        }
        return;
    }
    const bool wave_live = __any(live) != 0;
    const double *arow = live ? p.delta + (ga - p.row_lo) * (long)nvar : p.delta;      // (not live: row 0, read and discarded)
    const double ra = indel_norm(s.ig.scale, s.scaling_type, nka);
    // ---- the lane's D rows: rows g + 4 r
    int live_d[4];
    double r_d[4], dead_d[4];
    const double *brow[4];
    double *orow[4];
    #pragma unroll
    for (int r = 0; r < 4; r++) {
        live_d[r] = __shfl(live, g + 4 * r);
        r_d[r] = __shfl(ra, g + 4 * r);
        dead_d[r] = __shfl(dead, g + 4 * r);
        const long id = __shfl((int)ia, g + 4 * r);               // (n < 2^31: var_scan_check)
        const long row = t0 + g + 4 * r;
        brow[r] = q.b + id * K;
        orow[r] = row < p.row_hi ? q.out + row * K : nullptr;
    }
    const int nkc = (nvar + SV_KC - 1) / SV_KC, ncb = (K + SV_CB - 1) / SV_CB;
    const int steps = nkc * ncb;                         // column blocks outermost, k panels inside

    auto load_v = [&](int st, double (&dst)[VPT]) {
        const int cb = st / nkc, kc = st - cb * nkc;
        #pragma unroll
        for (int e = 0; e < VPT; e++) {
            const int idx = threadIdx.x + NT * e;
            const long k = (long)kc * SV_KC + idx / SV_CB, col = (long)cb * SV_CB + idx % SV_CB;
            const bool ok = k < nvar && col < K;
            const double v = q.pm[ok ? k * q.pm_stride + col : 0];
            dst[e] = ok ? v : 0.0;
        }
    };
    auto store_v = [&](int buf, const double (&src)[VPT]) {
        #pragma unroll
        for (int e = 0; e < VPT; e++) {
            const int idx = threadIdx.x + NT * e;
            vs[buf][(idx / SV_CB) * SV_VS + idx % SV_CB] = src[e];
        }
    };
    auto load_a = [&](int st, double (&dst)[SV_KS][4]) {
        const int kc = st % nkc;
        #pragma unroll
        for (int ks = 0; ks < SV_KS; ks++) {
            #pragma unroll
            for (int e = 0; e < 4; e++) {
                const int k = kc * SV_KC + 16 * ks + 4 * g + e;
                const bool ok = live && k < nvar;
                const double v = arow[ok ? k : 0];
                dst[ks][e] = ok ? v : 0.0;
            }
        }
    };

    double4_t acc[4];
    #pragma unroll
    for (int ct = 0; ct < 4; ct++) acc[ct] = (double4_t){0.0, 0.0, 0.0, 0.0};

    double cur[SV_KS][4], nxt[SV_KS][4], vreg[VPT];
    load_v(0, vreg);
    load_a(0, cur);
    store_v(0, vreg);
    __syncthreads();
    for (int st = 0; st < steps; st++) {
        const bool more = st + 1 < steps;                // workgroup-uniform
        if (more) { load_v(st + 1, vreg); load_a(st + 1, nxt); }
        const int cb = st / nkc, kc = st - cb * nkc;
        const double *vb = vs[st & 1];
        if (wave_live) {
            #pragma unroll
            for (int ks = 0; ks < SV_KS; ks++) {
                #pragma unroll
                for (int e = 0; e < 4; e++) {
                    double b[4];
                    #pragma unroll
                    for (int ct = 0; ct < 4; ct++) b[ct] = vb[(16 * ks + 4 * g + e) * SV_VS + 16 * ct + c];
                    #pragma unroll
                    for (int ct = 0; ct < 4; ct++) acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(cur[ks][e], b[ct], acc[ct], 0, 0, 0);
                }
            }
        }
        if (kc == nkc - 1) {                             // the column block is complete: its 64 columns of every row of the tile
            #pragma unroll
            for (int ct = 0; ct < 4; ct++) {
                const int col = cb * SV_CB + 16 * ct + c;
                #pragma unroll
                for (int r = 0; r < 4; r++) {
                    if (orow[r] && col < K) {
                        if (live_d[r]) {
                            const double ry = r_d[r] * acc[ct][r];
                            orow[r][col] = brow[r][col] + ry;
                        } else {
                            orow[r][col] = dead_d[r];
                        }
                    }
                }
                acc[ct] = (double4_t){0.0, 0.0, 0.0, 0.0};
            }
        }
        if (more) {
            store_v((st + 1) & 1, vreg);
            #pragma unroll
            for (int ks = 0; ks < SV_KS; ks++) {
                #pragma unroll
                for (int e = 0; e < 4; e++) cur[ks][e] = nxt[ks][e];
            }
        }
        __syncthreads();
    }
}

int edit_proj_ok(long width, long vocab, long C, long num_freqs, long nvar, long K) {
    return var_scan_ok(width, vocab, C, num_freqs, nvar) && K >= 1 && K <= EP_MAX_K ? 1 : 0;
}

constexpr VarScanOp SUBST_PROJ_OP = {0, "the substitution projection serves windows of up to 1024 elements, tables of up to 4608 floats, "
                                        "nvar <= 2048 and K <= 2048 (see xgpr_conv_token_edit_proj_ok)",
                                     "workspace too small or misaligned (see xgpr_conv_token_edit_proj_workspace_bytes)",
                                     "too many positions for one launch (n * L < 2^24)"};
constexpr VarScanOp INDEL_PROJ_OP = {1, "the indel projection serves windows of up to 1024 elements, tables of up to 4608 floats, "
                                        "nvar <= 2048 and K <= 2048 (see xgpr_conv_token_edit_proj_ok)",
                                     "workspace too small or misaligned (see xgpr_conv_token_edit_proj_workspace_bytes)",
                                     "too many positions for one launch (n * (L + 1) < 2^24)"};

// the second kernel of var_scan_slabs: the slab's rows of `out` from the slab's rows of delta
inline auto proj_launcher(const EditProjArgs &q, hipStream_t st) {
    return [q, st](const VarScanArgs &p, auto map, unsigned blocks) {
        EditProjArgs a = q;
        a.v = p;
        return launch(var_proj_kernel<decltype(map)>, dim3(blocks), dim3(256), 0, st, "var_proj_kernel launch", a);
    };
}

// what the two entry points share behind their checks: the arguments of the delta kernels and the packed masks
int edit_proj_begin(EditProjArgs &q, const uint8_t *tokens, const float *table, const double *pm, long pm_stride, const int8_t *radem,
                    const float *chi, const int32_t *seqlen_dev, long n, long L, long vocab, long C, long num_freqs, long R, long nvar, long K,
                    int conv_width, int scaling_type, int fit_intercept, void *workspace, hipStream_t st) {
    q.v.s = edit_scan_args(tokens, table, nullptr, chi, seqlen_dev, n, L, vocab, C, num_freqs, R, conv_width, scaling_type, fit_intercept,
                           workspace);
    q.v.delta = reinterpret_cast<double *>(static_cast<char *>(workspace) + masks_bytes(R));
    q.v.nvar = (int)nvar;
    q.pm = pm; q.pm_stride = pm_stride; q.K = (int)K;
    return pack_masks(radem, (uint64_t *)workspace, R, q.v.s.ig.MW, st);
}

int subst_proj_impl(const uint8_t *tokens, const float *table, const double *pm, long pm_stride, const double *b, double *out,
                    const int8_t *radem, const float *chi, const int32_t *seqlen_host, const int32_t *seqlen_dev, long n, long L, long vocab,
                    long C, long num_freqs, long R, long nvar, long K, int conv_width, int scaling_type, int fit_intercept, long slab_rows,
                    void *workspace, size_t wbytes, void *stream) {
    bool go;
    int rc = var_scan_check(SUBST_PROJ_OP, seqlen_host, n, L, vocab, C, num_freqs, R, nvar, nvar, conv_width, scaling_type, slab_rows,
                            workspace, wbytes, tokens && table && pm && b && out && radem && chi && seqlen_dev, true, &go, K, pm_stride);
    if (rc || !go) return rc;
    hipStream_t st = (hipStream_t)stream;
    EditProjArgs q = {};
    rc = edit_proj_begin(q, tokens, table, pm, pm_stride, radem, chi, seqlen_dev, n, L, vocab, C, num_freqs, R, nvar, K, conv_width,
                         scaling_type, fit_intercept, workspace, st);
    if (rc) return rc;
    q.b = b; q.out = out;
    return var_scan_slabs<EDIT_SUBST>(q.v, n * L * vocab, vocab, var_slab_rows(nvar, slab_rows), ilog2(padded_width((long)conv_width * C)),
                                      st, proj_launcher(q, st));
}

int indel_proj_impl(const uint8_t *tokens, const float *table, const double *pm, long pm_stride, const double *b_del, const double *b_ins,
                    double *out_del, double *out_ins, const int8_t *radem, const float *chi, const int32_t *seqlen_host,
                    const int32_t *seqlen_dev, long n, long L, long vocab, long C, long num_freqs, long R, long nvar, long K, int conv_width,
                    int scaling_type, int fit_intercept, long slab_rows, void *workspace, size_t wbytes, void *stream) {
    const bool del = b_del && out_del, ins = b_ins && out_ins;
    const bool halves = (!del && (b_del || out_del)) || (!ins && (b_ins || out_ins));        // a group given by halves
    bool go;
    int rc = var_scan_check(INDEL_PROJ_OP, seqlen_host, n, L, vocab, C, num_freqs, R, nvar, nvar, conv_width, scaling_type, slab_rows,
                            workspace, wbytes, tokens && table && pm && radem && chi && seqlen_dev && !halves, del || ins, &go, K, pm_stride);
    if (rc || !go) return rc;
    hipStream_t st = (hipStream_t)stream;
    EditProjArgs q = {};
    rc = edit_proj_begin(q, tokens, table, pm, pm_stride, radem, chi, seqlen_dev, n, L, vocab, C, num_freqs, R, nvar, K, conv_width,
                         scaling_type, fit_intercept, workspace, st);
    if (rc) return rc;
    const long slab = var_slab_rows(nvar, slab_rows);
    const int lg = ilog2(padded_width((long)conv_width * C));
    if (del) {
        q.b = b_del; q.out = out_del;
        rc = var_scan_slabs<EDIT_DEL>(q.v, n * L, 1, slab, lg, st, proj_launcher(q, st));
        if (rc) return rc;
    }
    if (ins) {
        q.b = b_ins; q.out = out_ins;
        rc = var_scan_slabs<EDIT_INS>(q.v, n * (L + 1) * vocab, vocab, slab, lg, st, proj_launcher(q, st));
    }
    return rc;
}
