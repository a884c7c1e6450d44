// indel_var_scan.inc -- part of xgpr_hip.hip (included inside its anonymous namespace, after subst_var_scan.inc): the exact quadratic
// form z'^T Vm z' of every single-token DELETION and INSERTION over the first nvar feature columns of the SEQUENCE and GRAPH kernels
// (xgpr_conv_token_indel_var_scan_f32, include/xgpr_hip_indel_var_scan.h; DESIGN.md 3.23).
//
// Notation of edit_scan.inc and subst_var_scan.inc.  An indel changes the window count, nk' = nk -+ 1, and with it the normaliser:
// r' = r(nk'), rho = r' / r(nk).  The mutant's columns are  z' = b + r' delta  with  b = rho z_i + (1 - rho) e0  (the caller's) and
//     deletion  of p      : delta = sum_{j' in A_p} phi(mutant window j')      -  sum_{j in R_p} phi(win_j)
//     insertion of v at g : delta = sum_{j'' in A_{g,v}} phi(mutant window j'') -  sum_{j in R'_g} phi(win_j)
// over the window ranges of edit_scan.inc, so  out = q~ + 2 r' (delta . u~) + r'^2 (delta^T Vm delta)  with the caller's
// u~ = 1/2 (Vm + Vm^T) b, q~ = b^T Vm b: one pair (u~, q~) per sequence for the deletions and one for the insertions.
//
// The rows of out_del are g = i L + p, those of out_ins g = (i (L + 1) + gap) V + v.  Each row set is cut into slabs of `slab_rows`
// rows and a host loop launches two kernels per slab, as subst_var_scan_impl does:
//   indel_var_delta_kernel<LOG2P, EDIT_INS>   one workgroup of four waves per (sequence, gap) that has a row in the slab; the waves
//       split the tokens as subst_var_delta_kernel does.  A wave first sums phi over the straddling windows R'_g (issue / take), then for
//       each of its tokens over the mutant's windows A_{g,v} (issue_ins / take_subst), both in float64 in ascending j, and stores the
//       difference as the float64 row delta[g - row_lo, 0 .. nvar).  The byte behind an appended token is never addressed (issue_ins).
//   indel_var_delta_kernel<LOG2P, EDIT_DEL>   a slot has ONE row: one wave per slot, four slots per workgroup, so that the table image
//       is loaded into LDS once per four slots.  Every wave meets the barrier behind the table load; a wave whose slot is past the
//       slab, past its sequence's length or belongs to a sequence of conv_width tokens writes nothing.  The wave sums phi over the
//       junction windows A_p (issue_del / take), then over the covering windows R_p (issue / take), and stores the difference.
//   The float32 cos / sin arguments are those of xgpr_conv_token_rows_f32 bit for bit; a row's bits depend on its own sequence, the
//   table and the draws alone.
//   indel_var_del_quad_kernel / indel_var_ins_quad_kernel   sv_quad_body (subst_var_scan.inc) under the row maps below: dead rows are
//       never read from the workspace, enter the MFMAs as zeros and store +0.0 -- or a quiet NaN for the deletions p < s of a sequence
//       with s == conv_width, whose mutant has no window (as xgpr_conv_token_indel_scan_f32 does at every scaling_type).
// No atomics.
// ------------------------------------------------------------------------------------

// deletions: V = 1, L slots per sequence, live p < s (and a window left), normaliser over nk - 1
struct DelRowMap {
    static __device__ __forceinline__ SvRow at(const SubstVarArgs &p, long row) {
        const EditScanArgs &s = p.s;
        SvRow o;
        o.i = row / s.L;
        const int e = (int)(row - o.i * s.L);
        const int len = s.win.seqlen[o.i];
        const int nk = len - s.win.conv_width + 1;
        o.live = (e < len && nk > 1) ? 1 : 0;
        o.nk = o.live ? nk - 1 : 1;
        o.dead = e < len ? __builtin_nan("") : 0.0;
        return o;
    }
};

// insertions: L + 1 slots per sequence, live g <= s, normaliser over nk + 1
struct InsRowMap {
    static __device__ __forceinline__ SvRow at(const SubstVarArgs &p, long row) {
        const EditScanArgs &s = p.s;
        SvRow o;
        const long slot = row / s.win.vocab;
        o.i = slot / (s.L + 1);
        const int e = (int)(slot - o.i * (s.L + 1));
        const int len = s.win.seqlen[o.i];
        o.live = e <= len ? 1 : 0;
        o.nk = len - s.win.conv_width + 2;
        o.dead = 0.0;
        return o;
    }
};

__global__ __launch_bounds__(256) void indel_var_del_quad_kernel(SubstVarArgs p) { sv_quad_body<DelRowMap>(p); }
__global__ __launch_bounds__(256) void indel_var_ins_quad_kernel(SubstVarArgs p) { sv_quad_body<InsRowMap>(p); }

template <int LOG2P, int MODE>
__global__ __launch_bounds__(256) void indel_var_delta_kernel(SubstVarArgs p) {
    static_assert(MODE == EDIT_DEL || MODE == EDIT_INS, "the two indel row sets");
    constexpr bool TP = LOG2P >= 7;
    constexpr bool INS = MODE == EDIT_INS;
    __shared__ __attribute__((aligned(16))) float tab[TOK_TABLE_FLOATS + 4];
    __shared__ __attribute__((aligned(16))) float tbuf[TP ? 4 * TBUF_FLOATS : 4];
    const EditScanArgs &s = p.s;
    const InputGradArgs &a = s.ig;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int V = s.win.vocab, cw = s.win.conv_width;
    const int S = INS ? s.L + 1 : s.L;                   // output slots per sequence
    // insertions: the workgroup's gap; deletions: the wave's position (its row of the slab)
    const long slot = INS ? p.slot_lo + blockIdx.x : p.row_lo + 4L * blockIdx.x + wv;
    bool live = INS || slot < p.row_hi;
    long i = 0;
    int e = 0, len = 0;
    if (live) {
        i = slot / S;
        e = (int)(slot - i * S);
        len = s.win.seqlen[i];
    }
    const int nk = len - cw + 1;
    if constexpr (INS) {
        if (e > len) return;                             // (uniform over the workgroup; the quadratic-form kernel stores the zeros)
    } else {
        live = live && e < len && nk > 1;                // (a wave that is not live still loads its part of the table and meets the barrier)
    }
    const int nt = V * s.win.kmer_stride;                // <= TOK_TABLE_FLOATS (edit_scan_ok)
    for (int t = threadIdx.x; t < nt; t += 256) tab[t] = s.win.x[t];
    if (threadIdx.x == 0) tab[nt] = 0.0f;
    __syncthreads();
    if (!live) return;                                   // (no barrier below)
    const int jlo = e - cw + 1 > 0 ? e - cw + 1 : 0;
    // the windows of the sequence that the edit removes, and those of the mutant that it adds
    const int rhi = INS ? (e - 1 < nk - 1 ? e - 1 : nk - 1) : (e < nk - 1 ? e : nk - 1);
    const int ahi = INS ? (e < nk ? e : nk) : (e - 1 < nk - 2 ? e - 1 : nk - 2);
    float *tb = tbuf + wv * (TP ? TBUF_FLOATS : 1);
    const float chs = TP ? a.chi_scale * sorf_kept_sign(lane) : a.chi_scale;
    IndelTokenWindows<LOG2P> win;
    win.tab = reinterpret_cast<const char *>(tab);
    win.begin(s.win, i, lane);
    cmask_t mk = as_cmask(a.masks);                      // tile 0
    // the cos / sin sums of windows jlo .. hi, j ascending.  KIND 0: the sequence's own windows; 1: the mutant's, token v inserted
    // at the gap; 2: the mutant's, the position deleted
    auto sums = [&](auto kind, int hi, unsigned v, double (&sc)[16], double (&ss)[16]) {
        constexpr int KIND = decltype(kind)::value;
        #pragma unroll
        for (int r = 0; r < 16; r++) { sc[r] = 0.0; ss[r] = 0.0; }
        for (int j = jlo; j <= hi; j++) {
            float t[16], arg[16], sn[16], cs[16];
            if constexpr (!TP) mk = launder(mk);
            const unsigned q = (unsigned)(e - j);        // the edit's position offset inside window j
            if constexpr (KIND == 0) { win.issue(j); win.take(t); }
            else if constexpr (KIND == 1) { win.issue_ins(j, q); win.take_subst(t, q, v); }
            else { win.issue_del(j, q); win.take(t); }
            input_grad_forward<LOG2P>(t, arg, a, mk, 0, chs, tb, lane);
            tile_sincos(arg, sn, cs);
            #pragma unroll
            for (int r = 0; r < 16; r++) {
                sc[r] += (double)cs[r];
                ss[r] += (double)sn[r];
            }
        }
    };
    auto store = [&](double *drow, const double (&ac)[16], const double (&as)[16], const double (&rc)[16], const double (&rs)[16]) {
        #pragma unroll
        for (int r = 0; r < 16; r++) {
            const int f = lane + 64 * r;
            if (2 * f < p.nvar) {                        // nvar is even: both columns of the pair exist
                const double dc = ac[r] - rc[r];
                drow[2 * f] = (a.fit_intercept && f == 0) ? 0.0 : dc;
                drow[2 * f + 1] = as[r] - rs[r];
            }
        }
    };
    double oc[16], os[16], vc[16], vs[16];
    if constexpr (INS) {
        // this wave's tokens with a row in the slab: v = wv, wv + 4, ... inside [vlo, vhi)
        const long g0 = slot * V;
        const int vlo = p.row_lo > g0 ? (int)(p.row_lo - g0) : 0;
        const int vhi = p.row_hi - g0 < V ? (int)(p.row_hi - g0) : V;
        int vfirst = wv;
        while (vfirst < vlo) vfirst += 4;
        if (vfirst >= vhi) return;
        sums(std::integral_constant<int, 0>{}, rhi, 0u, oc, os);
        for (int v = vfirst; v < vhi; v += 4) {
            sums(std::integral_constant<int, 1>{}, ahi, (unsigned)v, vc, vs);
            store(p.delta + (g0 + v - p.row_lo) * (long)p.nvar, vc, vs, oc, os);
        }
    } else {
        sums(std::integral_constant<int, 2>{}, ahi, 0u, vc, vs);
        sums(std::integral_constant<int, 0>{}, rhi, 0u, oc, os);
        store(p.delta + (slot - p.row_lo) * (long)p.nvar, vc, vs, oc, os);
    }
}

int conv_token_indel_var_scan_ok_impl(long width, long vocab, long C, long num_freqs, long nvar) {
    return conv_token_subst_var_scan_ok_impl(width, vocab, C, num_freqs, nvar);
}

size_t conv_token_indel_var_scan_workspace_bytes_impl(long R, long nvar, long slab_rows) {
    return conv_token_subst_var_scan_workspace_bytes_impl(R, nvar, slab_rows);
}

// the slabs of one row set: `rows` rows of `per_slot` rows per slot
template <int MODE>
int indel_var_slabs(SubstVarArgs p, long rows, long per_slot, long slab, int lg, hipStream_t st) {
    for (long lo = 0; lo < rows; lo += slab) {
        p.row_lo = lo;
        p.row_hi = lo + slab < rows ? lo + slab : rows;
        p.slot_lo = lo / per_slot;
        const long slots = (p.row_hi - 1) / per_slot - p.slot_lo + 1;
        const long blocks = MODE == EDIT_INS ? slots : (slots + 3) / 4;
        int rc = dispatch_lg<1, 10>(lg, TOO_WIDE_WAVE, [&](auto LG) {
            return launch(indel_var_delta_kernel<decltype(LG)::value, MODE>, dim3((unsigned)blocks), dim3(256), 0, st,
                          "indel_var_delta_kernel launch", p);
        });
        if (rc) return rc;
        const dim3 grid((unsigned)((p.row_hi - lo + 63) / 64));
        rc = MODE == EDIT_INS ? launch(indel_var_ins_quad_kernel, grid, dim3(256), 0, st, "indel_var_ins_quad_kernel launch", p)
                              : launch(indel_var_del_quad_kernel, grid, dim3(256), 0, st, "indel_var_del_quad_kernel launch", p);
        if (rc) return rc;
    }
    return 0;
}

int indel_var_scan_impl(const uint8_t *tokens, const float *table, const double *vm, long vm_stride, const double *u_del, const double *q_del,
                        const double *u_ins, const double *q_ins, double *out_del, double *out_ins, const int8_t *radem, const float *chi,
                        const int32_t *seqlen_host, const int32_t *seqlen_dev, long n, long L, long vocab, long C, long num_freqs, long R,
                        long nvar, int conv_width, int scaling_type, int fit_intercept, long slab_rows, void *workspace, size_t wbytes,
                        void *stream) {
    // the checks, in the documented order
    if (n < 0 || L < 1 || C < 1) return fail(XGPR_ERR_ARRAY_DIMS, "incorrect array dims passed");
    if (scaling_type < 0 || scaling_type > 2) return fail(XGPR_ERR_ARRAY_DIMS, "scaling_type must be 0, 1 or 2");
    if (conv_width <= 0 || L < conv_width) return fail(XGPR_ERR_CONV_WIDTH, "invalid conv_width");
    const long win = (long)conv_width * C;
    const long P = padded_width(win);
    if (num_freqs < 1 || num_freqs > R || R % P != 0) return fail(XGPR_ERR_RFFS_FREQS, "incorrect number of rffs and or freqs.");
    if (nvar < 2 || (nvar & 1) != 0 || nvar > 2 * num_freqs)
        return fail(XGPR_ERR_ARRAY_DIMS, "nvar must be an even number, 2 .. 2 * num_freqs");
    if (vm_stride < nvar) return fail(XGPR_ERR_ARRAY_SIZES, "vm_stride is shorter than nvar");
    if (slab_rows < 0 || slab_rows % 16 != 0) return fail(XGPR_ERR_ARRAY_DIMS, "slab_rows must be 0 or a multiple of 16");
    if (n > 0) {
        int rc = check_seqlens(seqlen_host, n, n, L, conv_width);
        if (rc) return rc;
    }
    if (vocab < 1 || vocab > 256) return fail(XGPR_ERR_ARRAY_DIMS, "token table: vocab must be 1 .. 256 (uint8 tokens)");
    if (!conv_token_indel_var_scan_ok_impl(win, vocab, C, num_freqs, nvar))
        return fail(XGPR_ERR_UNSUPPORTED, "the indel variance scan serves windows of up to 1024 elements, tables of up to 4608 floats and "
                                          "nvar <= 2048 (see xgpr_conv_token_indel_var_scan_ok)");
    if (n == 0) return 0;
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 7) != 0 || wbytes < conv_token_indel_var_scan_workspace_bytes_impl(R, nvar, slab_rows))
        return fail(XGPR_ERR_WORKSPACE, "workspace too small or misaligned (see xgpr_conv_token_indel_var_scan_workspace_bytes)");
    if (!tokens || !table || !vm || !radem || !chi || !seqlen_dev) return fail(XGPR_ERR_WORKSPACE, "NULL array pointer");
    const bool del = u_del && q_del && out_del, ins = u_ins && q_ins && out_ins;
    if ((!del && (u_del || q_del || out_del)) || (!ins && (u_ins || q_ins || out_ins)))      // a group given by halves
        return fail(XGPR_ERR_WORKSPACE, "NULL array pointer");
    if (!del && !ins) return fail(XGPR_ERR_WORKSPACE, "NULL array pointer (the deletion and the insertion group are both NULL: nothing to compute)");
    if (n > 2147483647L || n * (L + 1) > 16777215L) return fail(XGPR_ERR_UNSUPPORTED, "too many positions for one launch (n * (L + 1) < 2^24)");

    hipStream_t st = (hipStream_t)stream;
    SubstVarArgs p = {};
    p.s = edit_scan_args(tokens, table, nullptr, chi, seqlen_dev, n, L, vocab, C, num_freqs, R, conv_width, scaling_type, fit_intercept,
                         workspace);
    p.delta = reinterpret_cast<double *>(static_cast<char *>(workspace) + masks_bytes(R));
    p.vm = vm; p.vm_stride = vm_stride; p.nvar = (int)nvar;
    int rc = pack_masks(radem, (uint64_t *)workspace, R, p.s.ig.MW, st);
    if (rc) return rc;
    const long slab = subst_var_slab_rows(nvar, slab_rows);
    const int lg = ilog2(P);
    if (del) {
        p.u = u_del; p.q = q_del; p.out = out_del;
        rc = indel_var_slabs<EDIT_DEL>(p, n * L, 1, slab, lg, st);
        if (rc) return rc;
    }
    if (ins) {
        p.u = u_ins; p.q = q_ins; p.out = out_ins;
        rc = indel_var_slabs<EDIT_INS>(p, n * (L + 1) * vocab, vocab, slab, lg, st);
    }
    return rc;
}
