// var_scan.inc -- part of xgpr_hip.hip (included inside its anonymous namespace, after edit_scan.inc): the exact quadratic form
// z'^T Vm z' of every single-token SUBSTITUTION, DELETION and INSERTION over the first nvar feature columns of the SEQUENCE and GRAPH
// kernels (xgpr_conv_token_subst_var_scan_f32, include/xgpr_hip_subst_var_scan.h; xgpr_conv_token_indel_var_scan_f32,
// include/xgpr_hip_indel_var_scan.h; DESIGN.md 3.22, 3.23).
//
// Notation of edit_scan.inc.      phi(win)[2f] = cos p_f,  phi(win)[2f + 1] = sin p_f      (columns < nvar; column 0 := 0 under the intercept)
// A substitution at l moves the columns z of sequence i by r delta, with
//     delta[i, l, v] = sum_{j in J(l)} phi(win_j with the token at offset l - j replaced by v)  -  sum_{j in J(l)} phi(win_j)
// so  out[i, l, v] = q_i + 2 r (delta . u_i) + r^2 (delta^T Vm delta)  with the caller's u_i = Vm z_i, q_i = z_i . u_i.
// An indel changes the window count, nk' = nk -+ 1, and with it the normaliser: r' = r(nk'), rho = r' / r(nk).  The mutant's columns
// are  z' = b + r' delta  with  b = rho z_i + (1 - rho) e0  (the caller's) and
//     deletion  of p      : delta = sum_{j' in A_p} phi(mutant window j')      -  sum_{j in R_p} phi(win_j)
//     insertion of v at g : delta = sum_{j'' in A_{g,v}} phi(mutant window j'') -  sum_{j in R'_g} phi(win_j)
// over the window ranges of edit_scan.inc, so  out = q~ + 2 r' (delta . u~) + r'^2 (delta^T Vm delta)  with the caller's
// u~ = 1/2 (Vm + Vm^T) b, q~ = b^T Vm b: one pair (u~, q~) per sequence for the deletions and one for the insertions.
//
// Three row sets: the substitutions' rows of `out` are g = (i L + l) V + v, those of out_del g = i L + p, those of out_ins
// g = (i (L + 1) + gap) V + v.  Each row set is cut into slabs of `slab_rows` rows (a slab may begin and end inside a slot's V rows),
// and one host loop (var_scan_slabs) launches two kernels per slab, back to back on the stream:
//   subst_var_delta_kernel<LOG2P>   one workgroup of four waves per (sequence, position) that has a row in the slab.  nvar <= 2048: only
//       tile 0 exists, so the waves split the TOKENS (v = w, w + 4, ...), not the tiles.  A wave first forms the own token's cos / sin
//       sums over J(l) in ascending j -- through take_subst like every other token (recomputed per wave: no exchange, no barrier) --,
//       then for each of its tokens with a row in the slab the same sums, and stores the differences as the float64 row
//       delta[g - row_lo, 0 .. nvar) of the workspace: exactly +0.0 at the own token.  Slots past a length write nothing.  (The kernel
//       is the insertion arm below with another gather, exit and baseline; merged into it, its instantiations gained two scalar
//       instructions in the prologue, and it is kept apart: DESIGN.md 3.23, profiles/var_scan_refactor.json.)
//   var_delta_kernel<LOG2P, EDIT_INS>   one workgroup of four waves per (sequence, gap) that has a row in the slab; the waves split the
//       tokens in the same way.  A wave first sums phi over the straddling windows R'_g (issue / take), then for each of its tokens
//       over the mutant's windows A_{g,v} (issue_ins / take_subst), both in float64 in ascending j, and stores the difference as the
//       float64 row delta[g - row_lo, 0 .. nvar).  The byte behind an appended token is never addressed (issue_ins).
//   var_delta_kernel<LOG2P, EDIT_DEL>   a slot has ONE row: one wave per slot, four slots per workgroup, so that the table image
//       is loaded into LDS once per four slots.  Every wave meets the barrier behind the table load; a wave whose slot is past the
//       slab, past its sequence's length or belongs to a sequence of conv_width tokens writes nothing.  The wave sums phi over the
//       junction windows A_p (issue_del / take), then over the covering windows R_p (issue / take), and stores the difference.
//   The float32 cos / sin arguments are those of xgpr_conv_token_rows_f32 bit for bit (IndelTokenWindows, input_grad_forward,
//   tile_sincos); a row's bits depend on its own sequence, the table and the draws alone.
//   var_quad_kernel<MAP>    four waves, one 16-row tile each, under the row map of the row set.  Y = Delta Vm on
//       v_mfma_f64_16x16x4_f64 (operand maps at the top of cluster.inc: Delta's rows are the A operand, Vm[k, j] the B operand), 64
//       columns of Vm at a time, Vm passing through LDS in panels of 32 k x 64 columns (two buffers, one barrier per panel: 32 MFMAs
//       per wave between two barriers).  After a column block's last panel lane (c, g) multiplies D register r = Y[row g + 4 r][column]
//       by Delta[row][column] and adds it to its partial s[r]: columns ascending.  delta . u rides on the first column block (the lane's
//       four A values times u, k ascending).  Epilogue: s over the 16 lanes of a row (xor 1, 2, 4, 8), delta . u over the four lane
//       groups (xor 16, 32), out = (q + (2 r) du) + (r r) s.  Dead rows -- past the slab, or of a slot past its sequence's length --
//       are never read from the workspace, enter the MFMAs as zeros and store +0.0 -- or a quiet NaN for the deletions p < s of a
//       sequence with s == conv_width, whose mutant has no window (as xgpr_conv_token_indel_scan_f32 does at every scaling_type); a wave
//       with no live row issues no MFMA, a workgroup with none leaves at once; k and columns >= nvar are zeros in the LDS panel and
//       are never read from Delta.
// No atomics; a row's bits depend on its own delta, Vm, u_i, q_i and r alone: not on n, the slab cut or the row's place in a tile.
// ------------------------------------------------------------------------------------
constexpr long SV_MAX_NVAR = 2048;                 // one 1024-frequency tile
constexpr long SV_DEFAULT_BYTES = 128L << 20;      // of delta rows under slab_rows == 0 ...
constexpr long SV_DEFAULT_MAX_ROWS = 65536;        // ... and at most this many rows
constexpr int SV_KC = 32;                          // k per LDS panel of Vm: 32 MFMAs per wave between two barriers (two panels: 34 KiB of LDS)
constexpr int SV_KS = SV_KC / 16;                  // ... in sub-steps of 16: lane group g holds k = 16 ks + 4 g + e
constexpr int SV_CB = 64;                          // columns per block: four accumulator tiles per wave
constexpr int SV_VS = SV_CB + 4;                   // +32 B per k row of the panel, as in cluster.inc

struct VarScanArgs {
    EditScanArgs s;               // as for the mean scans; s.ig.w and s.out unused
    double *delta;                // workspace rows [slab_rows, nvar]
    const double *vm, *u, *q;
    double *out;                  // [n L V], [n L] or [n (L + 1) V]
    long vm_stride;
    long row_lo, row_hi;          // the slab's rows of out
    long slot_lo;                 // row_lo / (rows per slot)
    int nvar;
};

template <int LOG2P>
__global__ __launch_bounds__(256) void subst_var_delta_kernel(VarScanArgs p) {
    constexpr bool TP = LOG2P >= 7;
    __shared__ __attribute__((aligned(16))) float tab[TOK_TABLE_FLOATS + 4];
    __shared__ __attribute__((aligned(16))) float tbuf[TP ? 4 * TBUF_FLOATS : 4];
    const EditScanArgs &s = p.s;
    const InputGradArgs &a = s.ig;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long slot = p.slot_lo + blockIdx.x;
    const long i = slot / s.L;
    const int e = (int)(slot - i * s.L);
    const int V = s.win.vocab, cw = s.win.conv_width;
    const int len = s.win.seqlen[i];
    const int nk = len - cw + 1;
    if (e >= len) return;                                // (uniform over the workgroup; the quadratic-form kernel stores the zeros)
    const int nt = V * s.win.kmer_stride;                // <= TOK_TABLE_FLOATS (edit_scan_ok)
    for (int t = threadIdx.x; t < nt; t += 256) tab[t] = s.win.x[t];
    if (threadIdx.x == 0) tab[nt] = 0.0f;
    __syncthreads();
    const int jlo = e - cw + 1 > 0 ? e - cw + 1 : 0;
    const int jhi = e < nk - 1 ? e : nk - 1;
    float *tb = tbuf + wv * (TP ? TBUF_FLOATS : 1);
    const float chs = TP ? a.chi_scale * sorf_kept_sign(lane) : a.chi_scale;
    IndelTokenWindows<LOG2P> win;
    win.tab = reinterpret_cast<const char *>(tab);
    win.begin(s.win, i, lane);
    cmask_t mk = as_cmask(a.masks);                      // tile 0
    // the cos / sin sums of the slot's windows with token v at the slot: j ascending
    auto sums = [&](unsigned v, double (&sc)[16], double (&ss)[16]) {
        #pragma unroll
        for (int r = 0; r < 16; r++) { sc[r] = 0.0; ss[r] = 0.0; }
        for (int j = jlo; j <= jhi; j++) {
            float t[16], arg[16], sn[16], cs[16];
            if constexpr (!TP) mk = launder(mk);
            win.issue(j);
            win.take_subst(t, (unsigned)(e - j), v);
            input_grad_forward<LOG2P>(t, arg, a, mk, 0, chs, tb, lane);
            tile_sincos(arg, sn, cs);
            #pragma unroll
            for (int r = 0; r < 16; r++) {
                sc[r] += (double)cs[r];
                ss[r] += (double)sn[r];
            }
        }
    };
    // this wave's tokens with a row in the slab: v = wv, wv + 4, ... inside [vlo, vhi)
    const long g0 = slot * V;
    const int vlo = p.row_lo > g0 ? (int)(p.row_lo - g0) : 0;
    const int vhi = p.row_hi - g0 < V ? (int)(p.row_hi - g0) : V;
    int vfirst = wv;
    while (vfirst < vlo) vfirst += 4;
    if (vfirst >= vhi) return;                           // (no barrier below)
    const unsigned own = s.win.tokens[i * s.win.row_stride + e];     // e < len: inside the sequence
    double oc[16], os[16];
    sums(own, oc, os);
    for (int v = vfirst; v < vhi; v += 4) {
        double vc[16], vs[16];
        sums((unsigned)v, vc, vs);
        double *drow = p.delta + (g0 + v - p.row_lo) * (long)p.nvar;
        #pragma unroll
        for (int r = 0; r < 16; r++) {
            const int f = lane + 64 * r;
            if (2 * f < p.nvar) {                        // nvar is even: both columns of the pair exist
                const double dc = vc[r] - oc[r];
                drow[2 * f] = (a.fit_intercept && f == 0) ? 0.0 : dc;
                drow[2 * f + 1] = vs[r] - os[r];
            }
        }
    }
}

template <int LOG2P, int MODE>
__global__ __launch_bounds__(256) void var_delta_kernel(VarScanArgs p) {
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

// What the quadratic form needs to know of a row of out, supplied by a row map (MAP::at(p, row), row < p.row_hi): its sequence, whether
// it is live (a dead row is never read from the workspace and enters the MFMAs as zeros), the window count of the mutant's normaliser
// (indel_norm) and the value a dead row stores.
struct SvRow { long i; int live; int nk; double dead; };

// substitutions: V rows per position, L positions per sequence, live l < s, the sequence's own normaliser, dead rows store +0.0
struct SubstRowMap {
    static __device__ __forceinline__ SvRow at(const VarScanArgs &p, long row) {
        const EditScanArgs &s = p.s;
        SvRow o;
        const long slot = row / s.win.vocab;
        o.i = slot / s.L;
        const int l = (int)(slot - o.i * s.L);
        const int len = s.win.seqlen[o.i];
        o.nk = len - s.win.conv_width + 1;
        o.live = l < len ? 1 : 0;
        o.dead = 0.0;
        return o;
    }
};

// deletions: V = 1, L slots per sequence, live p < s (and a window left), normaliser over nk - 1
struct DelRowMap {
    static __device__ __forceinline__ SvRow at(const VarScanArgs &p, long row) {
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
    static __device__ __forceinline__ SvRow at(const VarScanArgs &p, long row) {
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

template <class MAP>
__device__ __forceinline__ void sv_quad_body(const VarScanArgs &p) {
    constexpr int NT = 256;
    constexpr int VPT = SV_KC * SV_CB / NT;              // panel elements staged per thread
    __shared__ __attribute__((aligned(16))) double vs[2][SV_KC * SV_VS];
    const EditScanArgs &s = p.s;
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nvar = p.nvar;
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
    // a workgroup none of whose 64 rows is live (positions past a length) stores its zeros and leaves; a wave without a live row keeps
    // staging Vm and meeting the barriers, but skips its matrix instructions (both decisions are uniform where they must be)
    if (!__syncthreads_or(live)) {
        const long row = t0 + lane;
        if (lane < 16 && row < p.row_hi) p.out[row] = dead;          // (lane < 16: c == lane, the row the lane looked up)
        return;
    }
    const bool wave_live = __any(live) != 0;
    const double *arow = live ? p.delta + (ga - p.row_lo) * (long)nvar : p.delta;      // (not live: row 0, read and discarded)
    const double *urow = p.u + ia * (long)nvar;
    // ---- the lane's D rows: rows g + 4 r
    int live_d[4];
    const double *drow[4];
    #pragma unroll
    for (int r = 0; r < 4; r++) {
        live_d[r] = __shfl(live, g + 4 * r);
        drow[r] = live_d[r] ? p.delta + (t0 + g + 4 * r - p.row_lo) * (long)nvar : p.delta;
    }
    const int nkc = (nvar + SV_KC - 1) / SV_KC, ncb = (nvar + SV_CB - 1) / SV_CB;
    const int steps = nkc * ncb;                         // column blocks outermost, k panels inside

    auto load_v = [&](int st, double (&dst)[VPT]) {
        const int cb = st / nkc, kc = st - cb * nkc;
        #pragma unroll
        for (int e = 0; e < VPT; e++) {
            const int idx = threadIdx.x + NT * e;
            const long k = (long)kc * SV_KC + idx / SV_CB, col = (long)cb * SV_CB + idx % SV_CB;
            const bool ok = k < nvar && col < nvar;
            const double v = p.vm[ok ? k * p.vm_stride + col : 0];
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
    double sq[4] = {0.0, 0.0, 0.0, 0.0};
    double du = 0.0;

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
        if (cb == 0 && wave_live) {                      // delta . u: this lane's four k of the panel, ascending
            #pragma unroll
            for (int ks = 0; ks < SV_KS; ks++) {
                #pragma unroll
                for (int e = 0; e < 4; e++) {
                    const int k = kc * SV_KC + 16 * ks + 4 * g + e;
                    const bool ok = live && k < nvar;
                    const double uv = urow[ok ? k : 0];
                    du += cur[ks][e] * (ok ? uv : 0.0);
                }
            }
        }
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
        if (wave_live && kc == nkc - 1) {                          // the column block is complete: Y o Delta, columns ascending
            #pragma unroll
            for (int ct = 0; ct < 4; ct++) {
                const int col = cb * SV_CB + 16 * ct + c;
                #pragma unroll
                for (int r = 0; r < 4; r++) {
                    const bool ok = live_d[r] && col < nvar;
                    const double dv = drow[r][ok ? col : 0];
                    sq[r] += acc[ct][r] * (ok ? dv : 0.0);
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

    // ---- epilogue.  A row's partial quadratic forms sit in its 16 lanes c; delta . u of row c in the four lanes {c, c + 16, c + 32, c + 48}
    #pragma unroll
    for (int r = 0; r < 4; r++) {
        #pragma unroll
        for (int off = 1; off < 16; off <<= 1) sq[r] += __shfl_xor(sq[r], off);
    }
    du += __shfl_xor(du, 16);
    du += __shfl_xor(du, 32);
    const double ra = indel_norm(s.ig.scale, s.scaling_type, nka);
    const double qa = live ? p.q[ia] : 0.0;
    const double base = live ? qa + (2.0 * ra) * du : dead;      // row c's first two terms, or what it stores as a dead row
    const double r2 = ra * ra;
    #pragma unroll
    for (int r = 0; r < 4; r++) {
        const double b = __shfl(base, g + 4 * r), rr = __shfl(r2, g + 4 * r);
        const long row = t0 + g + 4 * r;
        if (c == 0 && row < p.row_hi) p.out[row] = live_d[r] ? b + rr * sq[r] : b;
    }
}

template <class MAP>
__global__ __launch_bounds__(256) void var_quad_kernel(VarScanArgs p) { sv_quad_body<MAP>(p); }

int var_scan_ok(long width, long vocab, long C, long num_freqs, long nvar) {
    return edit_scan_ok(width, vocab, C, num_freqs) && nvar >= 2 && (nvar & 1) == 0 && nvar <= 2 * num_freqs && nvar <= SV_MAX_NVAR ? 1 : 0;
}

// the rows a slab holds: the caller's value, or the default for this nvar
long var_slab_rows(long nvar, long slab_rows) {
    if (slab_rows != 0) return slab_rows;
    long rows = SV_DEFAULT_BYTES / (nvar * (long)sizeof(double)) / 16 * 16;
    if (rows > SV_DEFAULT_MAX_ROWS) rows = SV_DEFAULT_MAX_ROWS;
    return rows < 16 ? 16 : rows;
}

size_t var_scan_workspace_bytes_impl(long R, long nvar, long slab_rows) {
    if (R < 1 || nvar < 2 || (nvar & 1) != 0 || slab_rows < 0 || slab_rows % 16 != 0) return 0;
    return masks_bytes(R) + (size_t)var_slab_rows(nvar, slab_rows) * (size_t)nvar * sizeof(double);
}

// what the checks of the two operators do not share: the output slots per sequence (L + gaps) and the three messages that name them
struct VarScanOp { int gaps; const char *unsupported, *workspace, *too_many; };
constexpr VarScanOp SUBST_VAR_OP = {0, "the substitution variance scan serves windows of up to 1024 elements, tables of up to 4608 floats and "
                                       "nvar <= 2048 (see xgpr_conv_token_subst_var_scan_ok)",
                                    "workspace too small or misaligned (see xgpr_conv_token_subst_var_scan_workspace_bytes)",
                                    "too many positions for one launch (n * L < 2^24)"};
constexpr VarScanOp INDEL_VAR_OP = {1, "the indel variance scan serves windows of up to 1024 elements, tables of up to 4608 floats and "
                                       "nvar <= 2048 (see xgpr_conv_token_indel_var_scan_ok)",
                                    "workspace too small or misaligned (see xgpr_conv_token_indel_var_scan_workspace_bytes)",
                                    "too many positions for one launch (n * (L + 1) < 2^24)"};

// the checks of the entry points, in the documented order; `bufs_ok`: every array the call needs is there (and no output group is given
// by halves); `outs_ok`: an output group too
int var_scan_check(const VarScanOp &op, const int32_t *seqlen_host, long n, long L, long vocab, long C, long num_freqs, long R, long nvar,
                   long vm_stride, int conv_width, int scaling_type, long slab_rows, const void *workspace, size_t wbytes, bool bufs_ok,
                   bool outs_ok, bool *launch, long K = 1, long pm_stride = 1) {
    *launch = false;
    if (n < 0 || L < 1 || C < 1) return fail(XGPR_ERR_ARRAY_DIMS, "incorrect array dims passed");
    if (scaling_type < 0 || scaling_type > 2) return fail(XGPR_ERR_ARRAY_DIMS, "scaling_type must be 0, 1 or 2");
    if (conv_width <= 0 || L < conv_width) return fail(XGPR_ERR_CONV_WIDTH, "invalid conv_width");
    const long win = (long)conv_width * C;
    if (num_freqs < 1 || num_freqs > R || R % padded_width(win) != 0) return fail(XGPR_ERR_RFFS_FREQS, "incorrect number of rffs and or freqs.");
    if (nvar < 2 || (nvar & 1) != 0 || nvar > 2 * num_freqs)
        return fail(XGPR_ERR_ARRAY_DIMS, "nvar must be an even number, 2 .. 2 * num_freqs");
    if (vm_stride < nvar) return fail(XGPR_ERR_ARRAY_SIZES, "vm_stride is shorter than nvar");
    if (K < 1) return fail(XGPR_ERR_ARRAY_DIMS, "K must be at least 1");                     // (the projections of edit_proj.inc alone)
    if (pm_stride < K) return fail(XGPR_ERR_ARRAY_SIZES, "pm_stride is shorter than K");
    if (slab_rows < 0 || slab_rows % 16 != 0) return fail(XGPR_ERR_ARRAY_DIMS, "slab_rows must be 0 or a multiple of 16");
    if (n > 0) {
        int rc = check_seqlens(seqlen_host, n, n, L, conv_width);
        if (rc) return rc;
    }
    if (vocab < 1 || vocab > 256) return fail(XGPR_ERR_ARRAY_DIMS, "token table: vocab must be 1 .. 256 (uint8 tokens)");
    if (!var_scan_ok(win, vocab, C, num_freqs, nvar) || K > SV_MAX_NVAR) return fail(XGPR_ERR_UNSUPPORTED, op.unsupported);
    if (n == 0) return 0;
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 7) != 0 || wbytes < var_scan_workspace_bytes_impl(R, nvar, slab_rows))
        return fail(XGPR_ERR_WORKSPACE, op.workspace);
    if (!bufs_ok) return fail(XGPR_ERR_WORKSPACE, "NULL array pointer");
    if (!outs_ok) return fail(XGPR_ERR_WORKSPACE, "NULL array pointer (the deletion and the insertion group are both NULL: nothing to compute)");
    if (n > 2147483647L || n * (L + op.gaps) > 16777215L) return fail(XGPR_ERR_UNSUPPORTED, op.too_many);
    *launch = true;
    return 0;
}

// the slabs of one row set: `rows` rows of `per_slot` rows per slot.  `second(p, MAP{}, blocks)` launches the slab's second kernel over
// `blocks` workgroups of 64 rows under the row map of the row set: the quadratic form (quad_launcher: into p.out under p.u, p.q) or the
// projection of edit_proj.inc
template <int MODE, class SECOND>
int var_scan_slabs(VarScanArgs p, long rows, long per_slot, long slab, int lg, hipStream_t st, SECOND second) {
    using MAP = std::conditional_t<MODE == EDIT_SUBST, SubstRowMap, std::conditional_t<MODE == EDIT_DEL, DelRowMap, InsRowMap>>;
    for (long lo = 0; lo < rows; lo += slab) {
        p.row_lo = lo;
        p.row_hi = lo + slab < rows ? lo + slab : rows;
        p.slot_lo = lo / per_slot;
        const long slots = (p.row_hi - 1) / per_slot - p.slot_lo + 1;
        const long blocks = edit_per_token(MODE) ? slots : (slots + 3) / 4;
        int rc = dispatch_lg<1, 10>(lg, TOO_WIDE_WAVE, [&](auto LG) {
            if constexpr (MODE == EDIT_SUBST)
                return launch(subst_var_delta_kernel<decltype(LG)::value>, dim3((unsigned)blocks), dim3(256), 0, st,
                              "subst_var_delta_kernel launch", p);
            else
                return launch(var_delta_kernel<decltype(LG)::value, MODE>, dim3((unsigned)blocks), dim3(256), 0, st,
                              "var_delta_kernel launch", p);
        });
        if (rc) return rc;
        rc = second(p, MAP{}, (unsigned)((p.row_hi - lo + 63) / 64));
        if (rc) return rc;
    }
    return 0;
}

inline auto quad_launcher(hipStream_t st) {
    return [st](const VarScanArgs &p, auto map, unsigned blocks) {
        return launch(var_quad_kernel<decltype(map)>, dim3(blocks), dim3(256), 0, st, "var_quad_kernel launch", p);
    };
}

int subst_var_scan_impl(const uint8_t *tokens, const float *table, const double *vm, long vm_stride, const double *u, const double *q,
                        double *out, const int8_t *radem, const float *chi, const int32_t *seqlen_host, const int32_t *seqlen_dev, long n,
                        long L, long vocab, long C, long num_freqs, long R, long nvar, int conv_width, int scaling_type, int fit_intercept,
                        long slab_rows, void *workspace, size_t wbytes, void *stream) {
    bool go;
    int rc = var_scan_check(SUBST_VAR_OP, seqlen_host, n, L, vocab, C, num_freqs, R, nvar, vm_stride, conv_width, scaling_type, slab_rows,
                            workspace, wbytes, tokens && table && vm && u && q && out && radem && chi && seqlen_dev, true, &go);
    if (rc || !go) return rc;
    hipStream_t st = (hipStream_t)stream;
    VarScanArgs p = {};
    p.s = edit_scan_args(tokens, table, nullptr, chi, seqlen_dev, n, L, vocab, C, num_freqs, R, conv_width, scaling_type, fit_intercept,
                         workspace);
    p.delta = reinterpret_cast<double *>(static_cast<char *>(workspace) + masks_bytes(R));
    p.vm = vm; p.vm_stride = vm_stride; p.nvar = (int)nvar;
    rc = pack_masks(radem, (uint64_t *)workspace, R, p.s.ig.MW, st);
    if (rc) return rc;
    p.u = u; p.q = q; p.out = out;
    return var_scan_slabs<EDIT_SUBST>(p, n * L * vocab, vocab, var_slab_rows(nvar, slab_rows), ilog2(padded_width((long)conv_width * C)), st,
                                      quad_launcher(st));
}

int indel_var_scan_impl(const uint8_t *tokens, const float *table, const double *vm, long vm_stride, const double *u_del, const double *q_del,
                        const double *u_ins, const double *q_ins, double *out_del, double *out_ins, const int8_t *radem, const float *chi,
                        const int32_t *seqlen_host, const int32_t *seqlen_dev, long n, long L, long vocab, long C, long num_freqs, long R,
                        long nvar, int conv_width, int scaling_type, int fit_intercept, long slab_rows, void *workspace, size_t wbytes,
                        void *stream) {
    const bool del = u_del && q_del && out_del, ins = u_ins && q_ins && out_ins;
    const bool halves = (!del && (u_del || q_del || out_del)) || (!ins && (u_ins || q_ins || out_ins));      // a group given by halves
    bool go;
    int rc = var_scan_check(INDEL_VAR_OP, seqlen_host, n, L, vocab, C, num_freqs, R, nvar, vm_stride, conv_width, scaling_type, slab_rows,
                            workspace, wbytes, tokens && table && vm && radem && chi && seqlen_dev && !halves, del || ins, &go);
    if (rc || !go) return rc;
    hipStream_t st = (hipStream_t)stream;
    VarScanArgs p = {};
    p.s = edit_scan_args(tokens, table, nullptr, chi, seqlen_dev, n, L, vocab, C, num_freqs, R, conv_width, scaling_type, fit_intercept,
                         workspace);
    p.delta = reinterpret_cast<double *>(static_cast<char *>(workspace) + masks_bytes(R));
    p.vm = vm; p.vm_stride = vm_stride; p.nvar = (int)nvar;
    rc = pack_masks(radem, (uint64_t *)workspace, R, p.s.ig.MW, st);
    if (rc) return rc;
    const long slab = var_slab_rows(nvar, slab_rows);
    const int lg = ilog2(padded_width((long)conv_width * C));
    if (del) {
        p.u = u_del; p.q = q_del; p.out = out_del;
        rc = var_scan_slabs<EDIT_DEL>(p, n * L, 1, slab, lg, st, quad_launcher(st));
        if (rc) return rc;
    }
    if (ins) {
        p.u = u_ins; p.q = q_ins; p.out = out_ins;
        rc = var_scan_slabs<EDIT_INS>(p, n * (L + 1) * vocab, vocab, slab, lg, st, quad_launcher(st));
    }
    return rc;
}
