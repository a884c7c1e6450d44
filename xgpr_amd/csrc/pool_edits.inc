// pool_edits.inc -- part of xgpr_hip.hip (included inside its anonymous namespace, after pool_input_grad.inc): the pooled first-layer
// row of the two-layer kernel for EVERY single-token substitution, deletion and insertion of a token sequence, without writing a
// mutant (xgpr_conv_token_maxpool_tables_f32 / xgpr_conv_token_maxpool_edits_f32, include/xgpr_hip/pool_edits.h; DESIGN.md 3.25).
//
// Sequence i has length s, nk = s - cw + 1 k-mer windows, nkmax = L - cw + 1, F filters; the table [V, C] is unscaled (sigma acts
// after the pool).  With p_{j,f} = chi_f SORF(win_j)_f the pooled value is q_f = max(0, max_j p_{j,f}).  A maximum is order-free, so
// the pooled row of a mutant is the maximum of three things: the windows left of the edit, the windows right of it -- an indel only
// shifts them, and a shifted window has the same content -- and the windows the edit creates:
//     PM[i, j, f] = max(0, p_{0,f} .. p_{j-1,f})        SM[i, j, f] = max(0, p_{j,f} .. p_{nk-1,f})        (rows j > nk: 0)
//     row = max(PM[i, a], SM[i, b], max over the mutant's new windows)
//         substitution at l     new windows j   in [max(0, l-cw+1), min(l, nk-1)]    (token at offset l - j replaced)     a = jlo, b = jhi + 1
//         deletion of p         new windows j'  in [max(0, p-cw+1), min(p-1, nk-2)]  (t[j' .. p) then t[p+1 .. j'+cw+1))  a = jlo, b = min(p, nk-1) + 1
//         insertion before g    new windows j'' in [max(0, g-cw+1), min(g, nk)]      (table row v at offset g - j'')      a = jlo, b = min(g-1, nk-1) + 1
// the ranges of edit_scan.inc.  A deletion at nk == 1 leaves no k-mer: the row is NaN.  Slots past the sequence (l, p >= s; g > s) are
// exact zero rows.
//
// Tables, two launches: the projection pass gives one WAVE to a (sequence, window) pair -- one protein spreads over the chip --, which
// runs the window through input_grad_forward for every tile (the max-pool operator's p bit for bit, as pass 1 of pool_input_grad.inc)
// and stores p into SM[i, j]; the running-max pass gives one thread to a (sequence, filter) pair, coalesced over f: ascending j into
// PM with the operator's own update  acc = acc > p ? acc : p  from 0 -- PM[i, j] is the operator's accumulator after j windows, bits
// and all --, then descending in place over SM.  Rows past nk are written as zeros: both arrays are OVERWRITTEN as a whole.
// Edits, one kernel template over the three modes: one workgroup of four waves per output slot; the unit of work is a (tile b, token v)
// pair, u = b * values + v, and wave w takes the units w, w + 4, ...: at one tile the V tokens still fill the four waves.  Per unit
// sixteen running maxima start from PM[i, a] and SM[i, b], the unit's windows go through the token window policy (IndelTokenWindows:
// issue / issue_del / issue_ins, take / take_subst, the next window's bytes fetched under this one's transform) and input_grad_forward,
// the update is the operator's own, and the unit's filters are stored once, coalesced.  No LDS accumulators, no cross-wave meeting,
// no atomics: every output is a function of its own sequence, the table and the draws alone.
// Sign of zero: the operator's update lets a -0.0 product replace +0.0, so the sign of a zero depends on the order of the windows (an
// exact zero product needs an all-zero table row, e.g. a padding token).  Every value equals the written-out route's as a real
// number, and bit for bit wherever it is not zero; the sign of a zero is unspecified.
// ------------------------------------------------------------------------------------
struct PoolEditsArgs {
    InputGradArgs ig;             // masks, chi, F, d = conv_width * C, MW, nb, nc, chi_scale (x, w, g, sigma unused)
    WaveArgs win;                 // what the token window policy reads: tokens, x = the table, vocab, row_stride = L, d, kmer_stride, conv_width, seqlen
    float *pm, *sm;               // [n, nkmax + 1, F]: written by the two table kernels, read by the edits kernel
    float *out;                   // the edits kernel's rows: nslots slots of (V or 1) rows of F
    long i_lo; int e_lo;          // the first slot of the launch: sequence slot_lo / S and slot slot_lo % S (S: slots per sequence)
    int L;
};

__device__ __forceinline__ float pool_max(float acc, float p) { return acc > p ? acc : p; }      // the max-pool operator's update

// the table [V, C] into LDS with one 0.0f behind it, as in wave_conv_tok_kernel (every thread of the workgroup calls this)
__device__ __forceinline__ void pool_edits_load_table(float *tab, const WaveArgs &w) {
    const int nt = w.vocab * w.kmer_stride;             // <= TOK_TABLE_FLOATS (conv_token_maxpool_edits_ok)
    for (int t = threadIdx.x; t < nt; t += 256) tab[t] = w.x[t];
    if (threadIdx.x == 0) tab[nt] = 0.0f;
    __syncthreads();
}

// ---- tables, pass 1: SM[i, j, :] = p_j for the k-mers j < nk; one wave per (sequence, window), four windows per workgroup
template <int LOG2P>
__global__ __launch_bounds__(256) void conv_token_maxpool_proj_kernel(PoolEditsArgs s) {
    constexpr bool TP = LOG2P >= 7;
    __shared__ __attribute__((aligned(16))) float tab[TOK_TABLE_FLOATS + 4];
    __shared__ __attribute__((aligned(16))) float tbuf[TP ? 4 * TBUF_FLOATS : 4];
    const InputGradArgs &a = s.ig;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int cw = s.win.conv_width;
    const int nkmax = s.L - cw + 1;
    const unsigned groups = (unsigned)(nkmax + 3) / 4u;
    const long i = blockIdx.x / groups;
    const int j = (int)(blockIdx.x - (unsigned)i * groups) * 4 + wv;
    pool_edits_load_table(tab, s.win);
    // (the only workgroup barrier is behind us: a wave without a k-mer leaves on its own)
    if (j >= s.win.seqlen[i] - cw + 1) return;
    float *tb = tbuf + wv * (TP ? TBUF_FLOATS : 1);
    const float chs = TP ? a.chi_scale * sorf_kept_sign(lane) : a.chi_scale;     // the sign tile_sorf kept, into chi (exact)
    TokenWindows<LOG2P> win;
    win.tab = reinterpret_cast<const char *>(tab);
    win.begin(s.win, i, lane);
    win.issue(j);                                        // the window's token bytes: once, for all tiles
    float *prow = s.sm + ((long)i * (nkmax + 1) + j) * a.F;
    for (int bb = 0; bb < a.nb; bb++) {
        const int b = __builtin_amdgcn_readfirstlane(bb);
        const cmask_t mk = as_cmask(a.masks + (long)b * 16);
        float v[16], pr[16];
        win.take(v);
        input_grad_forward<LOG2P>(v, pr, a, mk, b, chs, tb, lane);
        const long f0 = (long)b * 1024 + lane;
        #pragma unroll
        for (int r = 0; r < 16; r++) {
            const long f = f0 + r * 64;
            if (f < a.F) prow[f] = pr[r];
        }
    }
}

// ---- tables, pass 2: the running maxima, one thread per (sequence, filter); ascending into PM first (it reads the projections the
// descending pass then overwrites in place)
__global__ __launch_bounds__(256) void conv_token_maxpool_scan_kernel(float *pm, float *sm, const int32_t *seqlen, long n, long F,
                                                                       int nkmax, int conv_width) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n * F) return;
    const long i = t / F, f = t - i * F;
    const int nk = seqlen[i] - conv_width + 1;           // 1 .. nkmax (validated on the host)
    float *p = pm + i * (nkmax + 1) * F + f, *q = sm + i * (nkmax + 1) * F + f;
    float run = 0.0f;
    p[0] = 0.0f;
    for (int j = 0; j < nk; j++) {
        run = pool_max(run, q[(long)j * F]);
        p[(long)(j + 1) * F] = run;
    }
    for (int j = nk + 1; j <= nkmax; j++) p[(long)j * F] = 0.0f;
    for (int j = nkmax; j >= nk; j--) q[(long)j * F] = 0.0f;
    run = 0.0f;
    for (int j = nk - 1; j >= 0; j--) {
        run = pool_max(run, q[(long)j * F]);
        q[(long)j * F] = run;
    }
}

// ---- edits: one workgroup per output slot, (tile, token) units round-robin over its four waves
template <int LOG2P, int MODE>
__global__ __launch_bounds__(256) void conv_token_maxpool_edits_kernel(PoolEditsArgs s) {
    static_assert(MODE == EDIT_SUBST || MODE == EDIT_DEL || MODE == EDIT_INS, "the three single edits");
    constexpr bool TP = LOG2P >= 7;
    constexpr bool PER_TOKEN = edit_per_token(MODE);
    __shared__ __attribute__((aligned(16))) float tab[TOK_TABLE_FLOATS + 4];
    __shared__ __attribute__((aligned(16))) float tbuf[TP ? 4 * TBUF_FLOATS : 4];
    const InputGradArgs &a = s.ig;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int S = MODE == EDIT_INS ? s.L + 1 : s.L;      // output slots per sequence
    // (the launcher splits slot_lo into sequence and slot: the kernel divides 32-bit numbers only)
    const unsigned sl = (unsigned)s.e_lo + blockIdx.x;   // < S + 2^24
    const long i = s.i_lo + (long)(sl / (unsigned)S);
    const int e = (int)(sl % (unsigned)S);               // position l / p or gap g
    const int V = s.win.vocab, cw = s.win.conv_width;
    const int len = s.win.seqlen[i];
    const int nk = len - cw + 1, nkmax = s.L - cw + 1;
    const int no = PER_TOKEN ? V : 1;                    // values (rows of F) per slot
    float *orow = s.out + (long)blockIdx.x * no * a.F;
    // (both exits are uniform over the workgroup and lie in front of its one barrier)
    if (MODE == EDIT_INS ? e > len : e >= len) {
        for (long t = threadIdx.x; t < (long)no * a.F; t += 256) orow[t] = 0.0f;
        return;
    }
    if (MODE == EDIT_DEL && nk == 1) {                   // the mutant has no window
        for (long t = threadIdx.x; t < a.F; t += 256) orow[t] = __builtin_nanf("");
        return;
    }
    pool_edits_load_table(tab, s.win);
    // the windows the edit creates, and the rows of the two tables that hold everything it leaves alone
    const int jlo = e - cw + 1 > 0 ? e - cw + 1 : 0;
    int jhi, tb_row;
    if constexpr (MODE == EDIT_SUBST) { jhi = e < nk - 1 ? e : nk - 1; tb_row = jhi + 1; }
    else if constexpr (MODE == EDIT_DEL) { jhi = e - 1 < nk - 2 ? e - 1 : nk - 2; tb_row = (e < nk - 1 ? e : nk - 1) + 1; }
    else { jhi = e < nk ? e : nk; tb_row = (e - 1 < nk - 1 ? e - 1 : nk - 1) + 1; }
    const float *pmrow = s.pm + ((long)i * (nkmax + 1) + jlo) * a.F;
    const float *smrow = s.sm + ((long)i * (nkmax + 1) + tb_row) * a.F;

    float *tb = tbuf + wv * (TP ? TBUF_FLOATS : 1);
    const float chs = TP ? a.chi_scale * sorf_kept_sign(lane) : a.chi_scale;     // the sign tile_sorf kept, into chi (exact)
    IndelTokenWindows<LOG2P> win;
    win.tab = reinterpret_cast<const char *>(tab);
    win.begin(s.win, i, lane);
    auto issue = [&](int j) {                            // window j of the mutant; e - j: the edit's position offset inside it
        if constexpr (MODE == EDIT_INS) win.issue_ins(j, (unsigned)(e - j));
        else if constexpr (MODE == EDIT_DEL) win.issue_del(j, (unsigned)(e - j));
        else win.issue(j);
    };
    const int units = a.nb * no;
    for (int uu = wv; uu < units; uu += 4) {
        const int u = __builtin_amdgcn_readfirstlane(uu);
        const int b = __builtin_amdgcn_readfirstlane((int)((unsigned)u / (unsigned)no)), v = u - b * no;
        cmask_t mk = as_cmask(a.masks + (long)b * 16);
        const long f0 = (long)b * 1024 + lane;
        float acc[16];
        #pragma unroll
        for (int r = 0; r < 16; r++) {
            const long f = f0 + r * 64;
            const long fc = f < a.F ? f : 0;
            acc[r] = pool_max(pmrow[fc], smrow[fc]);
        }
        if (jlo <= jhi) issue(jlo);
        for (int j = jlo; j <= jhi; j++) {
            if constexpr (!TP) mk = launder(mk);        // (the 48 sign masks are re-read per window, not held in 96 scalar registers)
            float t[16], pr[16];
            if constexpr (PER_TOKEN) win.take_subst(t, (unsigned)(e - j), (unsigned)v);
            else win.take(t);
            if (j < jhi) issue(j + 1);                   // the next window is fetched under this one's transform
            input_grad_forward<LOG2P>(t, pr, a, mk, b, chs, tb, lane);
            #pragma unroll
            for (int r = 0; r < 16; r++) acc[r] = pool_max(acc[r], pr[r]);
        }
        float *o = orow + (long)v * a.F;
        #pragma unroll
        for (int r = 0; r < 16; r++) {
            const long f = f0 + r * 64;
            if (f < a.F) o[f] = acc[r];
        }
    }
}

// 1: the kernels serve a window of `width` = conv_width * C elements over a table [vocab, C] and `num_rffs` >= 1 filters
int conv_token_maxpool_edits_ok_impl(long width, long vocab, long C, long num_rffs) {
    return num_rffs >= 1 && conv_token_maxpool_input_grad_ok_impl(width, vocab, C) ? 1 : 0;
}

constexpr const char *POOL_EDITS_REFUSED =
    "the single-edit pool serves windows of up to 1024 elements and tables of up to 4608 floats (see xgpr_conv_token_maxpool_edits_ok)";

// the checks both entry points share, in the order and with the codes of xgpr_conv_token_maxpool_f32; `arrays_ok`: every array the
// call needs is there
int pool_edits_check(const int32_t *seqlen_host, const int32_t *seqlen_dev, long n, long L, long vocab, long C, long num_rffs, long R,
                     long nseq, int conv_width, const void *workspace, size_t wbytes, bool arrays_ok) {
    if (vocab < 1 || vocab > 256) return fail(XGPR_ERR_ARRAY_DIMS, "token table: vocab must be 1 .. 256 (uint8 tokens)");
    if (C < 1) return fail(XGPR_ERR_ARRAY_DIMS, "token table: needs at least one column");
    const long win = (long)conv_width * C;
    const long P = padded_width(win > 0 ? win : 1);
    const long reps = (num_rffs + P - 1) / P;
    int rc = check_sorf_shape(n, num_rffs, num_rffs, R, P, 1, [&] {
        if (nseq != n) return fail(XGPR_ERR_SEQLEN_SIZE, "wrong array sizes");
        if (L < conv_width || conv_width <= 0) return fail(XGPR_ERR_CONV_WIDTH, "invalid conv_width");
        return 0;
    });
    if (rc) return rc;
    if (R != reps * P) return fail(XGPR_ERR_RFFS_FREQS, "incorrect number of rffs and or freqs.");
    rc = check_seqlens(seqlen_host, nseq, n, L, conv_width);
    if (rc) return rc;
    if (!seqlen_dev) return fail(XGPR_ERR_WORKSPACE, "seqlen_dev (device copy of the sequence lengths) is required");
    if (!arrays_ok) return fail(XGPR_ERR_WORKSPACE, "NULL array pointer");
    if (!conv_token_maxpool_edits_ok_impl(win, vocab, C, num_rffs)) return fail(XGPR_ERR_UNSUPPORTED, POOL_EDITS_REFUSED);
    if (!workspace || wbytes < masks_bytes(R)) return fail(XGPR_ERR_WORKSPACE, "workspace too small (see xgpr_conv_workspace_bytes)");
    return 0;
}

PoolEditsArgs pool_edits_args(const uint8_t *tokens, const float *table, float *pm, float *sm, const float *chi,
                              const int32_t *seqlen_dev, long n, long L, long vocab, long C, long num_rffs, long R, int conv_width,
                              void *workspace) {
    const long win = (long)conv_width * C;
    PoolEditsArgs s = {};
    s.win = wave_args(table, chi, workspace, n, L, win, num_rffs, R);
    s.win.tokens = tokens; s.win.vocab = (int)vocab;
    s.win.seqlen = seqlen_dev; s.win.kmer_stride = (int)C; s.win.conv_width = conv_width;
    InputGradArgs &a = s.ig;
    a.masks = s.win.masks; a.chi = chi;
    a.n = n; a.F = num_rffs; a.w_cols = num_rffs;
    a.d = (int)win; a.MW = s.win.MW; a.nb = s.win.nb;
    a.nc = s.win.nc; a.chi_scale = s.win.chi_scale;
    a.scale = 1.0; a.sigma = 1.0;
    s.pm = pm; s.sm = sm; s.L = (int)L;
    return s;
}

int pool_tables_impl(const uint8_t *tokens, const float *table, float *pm, float *sm, const int8_t *radem, const float *chi,
                     const int32_t *seqlen_host, const int32_t *seqlen_dev, long n, long L, long vocab, long C, long num_rffs, long R,
                     long nseq, int conv_width, void *workspace, size_t wbytes, void *stream) {
    int rc = pool_edits_check(seqlen_host, seqlen_dev, n, L, vocab, C, num_rffs, R, nseq, conv_width, workspace, wbytes,
                              tokens && table && pm && sm && radem && chi);
    if (rc) return rc;
    const long nkmax = L - conv_width + 1;
    const long blocks = n * ((nkmax + 3) / 4), threads = n * num_rffs;
    if (n > 2147483647L || n * (nkmax + 1) > 16777215L || (threads + 255) / 256 > 2147483647L)
        return fail(XGPR_ERR_UNSUPPORTED, "too many windows for one launch (n * (L - conv_width + 2) < 2^24)");
    hipStream_t st = (hipStream_t)stream;
    PoolEditsArgs s = pool_edits_args(tokens, table, pm, sm, chi, seqlen_dev, n, L, vocab, C, num_rffs, R, conv_width, workspace);
    rc = pack_masks(radem, (uint64_t *)workspace, R, s.ig.MW, st);
    if (rc) return rc;
    rc = dispatch_lg<1, 10>(ilog2(padded_width(s.ig.d)), TOO_WIDE_WAVE, [&](auto LG) {
        return launch(conv_token_maxpool_proj_kernel<decltype(LG)::value>, dim3((unsigned)blocks), dim3(256), 0, st,
                      "conv_token_maxpool_proj_kernel launch", s);
    });
    if (rc) return rc;
    return launch(conv_token_maxpool_scan_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st,
                  "conv_token_maxpool_scan_kernel launch", pm, sm, seqlen_dev, n, num_rffs, (int)nkmax, conv_width);
}

int pool_edits_impl(const uint8_t *tokens, const float *table, const float *pm, const float *sm, float *out, const int8_t *radem,
                    const float *chi, const int32_t *seqlen_host, const int32_t *seqlen_dev, long n, long L, long vocab, long C,
                    long num_rffs, long R, long nseq, int conv_width, int mode, long slot_lo, long nslots, void *workspace,
                    size_t wbytes, void *stream) {
    if (mode != EDIT_SUBST && mode != EDIT_DEL && mode != EDIT_INS)
        return fail(XGPR_ERR_ARRAY_DIMS, "mode must be 1 (deletions), 2 (insertions) or 3 (substitutions)");
    int rc = pool_edits_check(seqlen_host, seqlen_dev, n, L, vocab, C, num_rffs, R, nseq, conv_width, workspace, wbytes,
                              tokens && table && pm && sm && out && radem && chi);
    if (rc) return rc;
    const long S = mode == EDIT_INS ? L + 1 : L;
    if (slot_lo < 0 || nslots < 0 || slot_lo > n * S || nslots > n * S - slot_lo)
        return fail(XGPR_ERR_ARRAY_SIZES, "slot range outside the n * (L or L + 1) slots of the batch");
    if (nslots == 0) return 0;
    if (n > 2147483647L || nslots > 16777215L) return fail(XGPR_ERR_UNSUPPORTED, "too many slots for one launch (nslots < 2^24)");
    hipStream_t st = (hipStream_t)stream;
    PoolEditsArgs s = pool_edits_args(tokens, table, const_cast<float *>(pm), const_cast<float *>(sm), chi, seqlen_dev, n, L, vocab, C,
                                      num_rffs, R, conv_width, workspace);
    s.out = out; s.i_lo = slot_lo / S; s.e_lo = (int)(slot_lo % S);
    rc = pack_masks(radem, (uint64_t *)workspace, R, s.ig.MW, st);
    if (rc) return rc;
    return dispatch_lg<1, 10>(ilog2(padded_width(s.ig.d)), TOO_WIDE_WAVE, [&](auto LG) {
        constexpr int LGV = decltype(LG)::value;
        if (mode == EDIT_SUBST)
            return launch(conv_token_maxpool_edits_kernel<LGV, EDIT_SUBST>, dim3((unsigned)nslots), dim3(256), 0, st,
                          "conv_token_maxpool_edits_kernel launch", s);
        if (mode == EDIT_DEL)
            return launch(conv_token_maxpool_edits_kernel<LGV, EDIT_DEL>, dim3((unsigned)nslots), dim3(256), 0, st,
                          "conv_token_maxpool_edits_kernel launch", s);
        return launch(conv_token_maxpool_edits_kernel<LGV, EDIT_INS>, dim3((unsigned)nslots), dim3(256), 0, st,
                      "conv_token_maxpool_edits_kernel launch", s);
    });
}
