// site_scan.inc -- part of xgpr_hip.hip (included inside its anonymous namespace, after pair_scan.inc): the exact COMBINATORIAL
// site-saturation scan of K chosen positions on a weighted sum of the SEQUENCE and GRAPH kernels' random features
// (xgpr_conv_token_site_scan_f32, include/xgpr_hip/site_scan.h; DESIGN.md 3.27).
//
// Notation of edit_scan.inc.  The sites p_0 < ... < p_{K-1} are shared by all sequences of a call.  As the window start j slides over
// 0 .. L - cw, the sites a window covers are a contiguous range of the site list, and one set of sites is covered by one contiguous
// range of j: a RUN rho = (j_lo .. j_hi; sites p_a .. p_{a+g-1}).  A window of no run covers no site and cancels against the parent.
//     out[i, off_rho + idx] = r(nk) sum_{j = j_lo .. min(j_hi, nk - 1)} [ c(win_j with a_m at p_{a+m}, m < g) - c(win_j) ]
//         idx = sum_m a_m V^{g-1-m}                                                   (the run's LAST site is contiguous)
// and  m(t[p_k := A_k for all k]) - m(t) = sum_rho out[i, off_rho + idx_rho(A)]  exactly: every window that sees a site belongs to
// exactly one run, and sees the sites of that run alone.
//
// Three kernels, all writing `out` (and the corner array of the workspace) alone.
//   site_scan_grid_kernel   one workgroup of four waves per (sequence, run, assignment of the run's first g - 1 sites): the body of
//       pair_scan_grid_kernel with g - 1 patches instead of one.  The run's windows run outermost in ascending j; a window's token
//       bytes are fetched ONCE and patched g - 1 times in the policy's registers (PairTokenWindows::patch); wave w takes the tiles
//       b = w, w + 4, ..., holds the tile's float64 weight pairs in registers, and the last site's token v = 0 .. V - 1 runs
//       innermost through take_subst.  After the last window one barrier, and thread v stores the RAW sum
//       G[idx] = ((a0 + a1) + a2) + a3.  The sequence's own assignment goes through exactly this path like every other.
//   site_scan_corner_kernel one thread per sequence, for each of its runs: G at the sequence's own tokens -- the parent's sum over the run's
//       windows, formed by the code path of every variant -- is copied to corner[i, rho] in the workspace BEFORE anything is
//       overwritten.
//   site_scan_diff_kernel   one workgroup per row of the grid kernel: out <- r (G - corner).  The own assignment is x - x on identical
//       bits: +0.0 by construction, not by masking.
// No slot is shared between waves or workgroups: no atomics, the order of every sum is fixed ((j ascending, b ascending) into a slot,
// then the four waves in order), every row is a bitwise function of its own sequence, the table, the weights and the sites, and two
// identical table rows give identical bits along every site axis.  A run with no window inside the sequence stores 0.0 in the first
// kernel and is left alone by the third; both exits are uniform over the workgroup and come before any barrier.  The run table
// travels in the kernel arguments and is read with constant indices only (a select chain over SITE_MAX_RUNS entries): no scratch.
// ------------------------------------------------------------------------------------
constexpr int SITE_MAX_K = 16, SITE_MAX_RUNS = 2 * SITE_MAX_K - 1, SITE_MAX_COVER = 4;

// one run as the kernels see it: its windows, its site count, its first grid row inside a sequence, its offset into a row of out,
// the positions of its sites -- and, for the grid kernel, the position of its LAST site and those of the others from the last but
// one BACKWARDS (the order in which the digits of a row's prefix come off), SITE_NO_POS where the run has fewer: an offset no
// register of a window carries, so that a patch there changes nothing and the kernel needs no site count
constexpr int SITE_NO_POS = 0x40000000;
struct SiteRun { int jlo, jhi, g; unsigned row0; long off; int pos[SITE_MAX_COVER]; int plast; int ppos[SITE_MAX_COVER - 1]; };
// EditScanArgs has no room for the runs: wrapped, not extended
struct SiteScanArgs {
    EditScanArgs e;
    double *corner;               // workspace, after the packed sign masks: [n, nruns]
    long T;                       // elements of a row of out: sum over the runs of V^g
    unsigned rows;                // grid rows per sequence: sum over the runs of V^(g-1)
    int nruns;
    SiteRun run[SITE_MAX_RUNS];
};
static_assert(sizeof(SiteScanArgs) <= 4096, "the run table must fit the kernel argument segment");

// the run that holds grid row `e` of a sequence (the runs' row0 ascend); constant indices only
__device__ __forceinline__ SiteRun site_run_of_row(const SiteScanArgs &ss, unsigned e, int &rho) {
    SiteRun r = ss.run[0];
    rho = 0;
    #pragma unroll
    for (int k = 1; k < SITE_MAX_RUNS; k++)
        if (k < ss.nruns && e >= ss.run[k].row0) { r = ss.run[k]; rho = k; }
    return r;
}

// what a workgroup index means to the grid and the difference kernel
struct SiteSlot { long i; int rho, len, jhi; unsigned prefix; SiteRun run; bool live; };
__device__ __forceinline__ SiteSlot site_slot(const SiteScanArgs &ss, unsigned bx) {
    SiteSlot p;
    p.i = bx / ss.rows;
    const unsigned e = bx - (unsigned)p.i * ss.rows;
    p.run = site_run_of_row(ss, e, p.rho);
    p.prefix = e - p.run.row0;                           // sum_{m < g-1} a_m V^{g-2-m}
    p.len = ss.e.win.seqlen[p.i];
    const int nk = p.len - ss.e.win.conv_width + 1;
    p.jhi = p.run.jhi < nk - 1 ? p.run.jhi : nk - 1;
    p.live = p.run.jlo <= p.jhi;                         // (a run can start past a short sequence's last window)
    return p;
}

template <int LOG2P>
__global__ __launch_bounds__(256) void site_scan_grid_kernel(SiteScanArgs ss) {
    constexpr bool TP = LOG2P >= 7;
    __shared__ __attribute__((aligned(16))) float tab[TOK_TABLE_FLOATS + 4];
    __shared__ __attribute__((aligned(16))) float tbuf[TP ? 4 * TBUF_FLOATS : 4];
    __shared__ double acc[4][256];                       // acc[w][v]: wave w's sum for the last site's token v (vocab <= 256)
    const EditScanArgs &s = ss.e;
    const InputGradArgs &a = s.ig;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int V = s.win.vocab;
    const SiteSlot ps = site_slot(ss, blockIdx.x);       // blockIdx.x = i rows + row0 + prefix < 2^24
    double *orow = s.out + ps.i * ss.T + ps.run.off + (long)ps.prefix * V;
    // (uniform over the workgroup: nobody waits at the barriers below)
    if (!ps.live) {
        for (int v = threadIdx.x; v < V; v += 256) orow[v] = 0.0;
        return;
    }
    const long i = ps.i;
    // the tokens of the first g - 1 sites: the prefix's digits, the last but one site least significant (ppos is in that order)
    unsigned tokv[SITE_MAX_COVER - 1];
    unsigned rem = ps.prefix;
    #pragma unroll
    for (int m = 0; m < SITE_MAX_COVER - 1; m++) { tokv[m] = rem % (unsigned)V; rem /= (unsigned)V; }
    const int plast = ps.run.plast;
    const int nt = V * s.win.kmer_stride;                // <= TOK_TABLE_FLOATS (edit_scan_ok)
    for (int t = threadIdx.x; t < nt; t += 256) tab[t] = s.win.x[t];
    if (threadIdx.x == 0) tab[nt] = 0.0f;
    #pragma unroll
    for (int w = 0; w < 4; w++) acc[w][threadIdx.x] = 0.0;
    __syncthreads();

    float *tb = tbuf + wv * (TP ? TBUF_FLOATS : 1);
    const float chs = TP ? a.chi_scale * sorf_kept_sign(lane) : a.chi_scale;     // the sign tile_sorf kept, into chi (exact)
    PairTokenWindows<LOG2P> win;
    win.tab = reinterpret_cast<const char *>(tab);
    win.begin(s.win, i, lane);
    for (int j = ps.run.jlo; j <= ps.jhi; j++) {
        const unsigned ql = (unsigned)(plast - j);       // the last site's offset inside window j (every site of the run lies inside it)
        // the window's token bytes: once per (row, window), for all tokens of the last site and all tiles; then the first g - 1 sites
        win.issue(j);
        #pragma unroll
        for (int m = 0; m < SITE_MAX_COVER - 1; m++) win.patch((unsigned)(ps.run.ppos[m] - j), tokv[m]);   // (SITE_NO_POS: no match)
        for (int bb = wv; bb < a.nb; bb += 4) {
            const int b = __builtin_amdgcn_readfirstlane(bb);
            cmask_t mk = as_cmask(a.masks + (long)b * 16);
            // the tile's weight pairs (w[0] dropped under the intercept; frequencies >= F carry no weight)
            double wc[16], ws[16];
            const long f0 = (long)b * 1024 + lane;
            #pragma unroll
            for (int r = 0; r < 16; r++) {
                const long f = f0 + r * 64;
                const bool in = f < a.F;
                const long fc = in ? f : 0;
                const double w0 = a.w[2 * fc], w1 = a.w[2 * fc + 1];
                wc[r] = (in && !(a.fit_intercept && f == 0)) ? w0 : 0.0;
                ws[r] = in ? w1 : 0.0;
            }
            for (int v = 0; v < V; v++) {
                float t[16], arg[16], sn[16], cs[16];
                if constexpr (!TP) mk = launder(mk);     // (the 48 sign masks are re-read per token, not held in 96 scalar registers)
                win.take_subst(t, ql, (unsigned)v);
                input_grad_forward<LOG2P>(t, arg, a, mk, b, chs, tb, lane);
                tile_sincos(arg, sn, cs);
                double p = 0.0;
                #pragma unroll
                for (int r = 0; r < 16; r++) {
                    p += wc[r] * (double)cs[r];
                    p += ws[r] * (double)sn[r];
                }
                const double u = wave_sum(p);
                if (lane == 0) acc[wv][v] += u;          // (this wave's slot: in order, no other wave touches it)
            }
        }
    }
    // (the tile exchanges of tile_sorf are inline assembly the compiler's wait-count pass does not see: the wait in front of the
    // cross-wave barrier is explicit -- DESIGN.md 5)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();
    for (int v = threadIdx.x; v < V; v += 256) orow[v] = ((acc[0][v] + acc[1][v]) + acc[2][v]) + acc[3][v];
}

// corner[i, rho] <- G at the sequence's own tokens (0.0 for a run without a window: what the grid kernel stored); one thread per
// sequence, the runs in a loop the compiler unrolls (constant indices into the run table)
__global__ __launch_bounds__(256) void site_scan_corner_kernel(SiteScanArgs ss) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= ss.e.ig.n) return;
    const uint8_t *trow = ss.e.win.tokens + i * ss.e.win.row_stride;   // (every site lies inside every sequence: checked on the host)
    #pragma unroll
    for (int k = 0; k < SITE_MAX_RUNS; k++) {
        if (k >= ss.nruns) break;
        long idx = 0;
        #pragma unroll
        for (int m = 0; m < SITE_MAX_COVER; m++)
            if (m < ss.run[k].g) idx = idx * ss.e.win.vocab + trow[ss.run[k].pos[m]];
        ss.corner[i * ss.nruns + k] = ss.e.out[i * ss.T + ss.run[k].off + idx];
    }
}

__global__ __launch_bounds__(256) void site_scan_diff_kernel(SiteScanArgs ss) {
    const SiteSlot ps = site_slot(ss, blockIdx.x);
    if (!ps.live) return;                                // (uniform; the zeros of the first kernel stay)
    const int V = ss.e.win.vocab;
    double *orow = ss.e.out + ps.i * ss.T + ps.run.off + (long)ps.prefix * V;
    const double rs = indel_norm(ss.e.ig.scale, ss.e.scaling_type, ps.len - ss.e.win.conv_width + 1);
    const double corner = ss.corner[ps.i * ss.nruns + ps.rho];
    for (int v = threadIdx.x; v < V; v += 256) orow[v] = rs * (orow[v] - corner);
}

int conv_token_site_scan_ok_impl(long width, long vocab, long C, long num_freqs, int max_cover) {
    return edit_scan_ok(width, vocab, C, num_freqs) && max_cover >= 1 && max_cover <= SITE_MAX_COVER ? 1 : 0;
}

// ---- the runs of a site list, on the host
struct SiteLayout {
    int nruns, max_g;
    bool overflow;                                       // a table size or the row length does not fit 62 bits: the offsets are not valid
    int jlo[SITE_MAX_RUNS], jhi[SITE_MAX_RUNS], first[SITE_MAX_RUNS], g[SITE_MAX_RUNS];
    long off[SITE_MAX_RUNS], T;
};

int site_list_check(const int32_t *sites, int K, long L) {
    if (K < 1 || K > SITE_MAX_K || !sites) return fail(XGPR_ERR_ARRAY_DIMS, "site list: 1 .. 16 sites are served");
    for (int k = 0; k < K; k++) {
        if (sites[k] < 0 || sites[k] >= L) return fail(XGPR_ERR_ARRAY_DIMS, "site list: a site outside 0 .. L - 1");
        if (k && sites[k] <= sites[k - 1]) return fail(XGPR_ERR_ARRAY_DIMS, "site list: the sites must be strictly ascending");
    }
    return 0;
}

// (a checked site list, 1 <= cw <= L, vocab >= 1)
void site_layout(const int32_t *sites, int K, long L, int cw, long vocab, SiteLayout &lay) {
    lay = SiteLayout();
    const long jmax = L - cw;
    long j = sites[0] - cw + 1 > 0 ? sites[0] - cw + 1 : 0;
    int lo = 0, hi = 0;                                  // the sites window j covers: [lo, hi)
    for (; j <= jmax && j <= sites[K - 1]; j++) {
        while (lo < K && sites[lo] < j) lo++;
        while (hi < K && sites[hi] <= j + cw - 1) hi++;
        if (hi <= lo) continue;                          // (a window between two distant sites)
        const int r = lay.nruns - 1;
        if (r >= 0 && lay.first[r] == lo && lay.g[r] == hi - lo && lay.jhi[r] == j - 1) { lay.jhi[r] = (int)j; continue; }
        const int q = lay.nruns++;                       // (at most 2 K - 1: a run begins where a site enters or leaves)
        lay.jlo[q] = lay.jhi[q] = (int)j; lay.first[q] = lo; lay.g[q] = hi - lo;
        if (hi - lo > lay.max_g) lay.max_g = hi - lo;
        long size = 1;
        for (int m = 0; m < hi - lo; m++) {
            if (size > (1L << 62) / vocab) lay.overflow = true;
            else size *= vocab;
        }
        lay.off[q] = lay.T;
        if (lay.T > (1L << 62) - size) lay.overflow = true;
        else lay.T += size;
    }
}

long site_scan_layout_impl(const int32_t *sites, int K, long L, int conv_width, long vocab, int32_t *run_first_window,
                           int32_t *run_last_window, int32_t *run_first_site, int32_t *run_sites, int64_t *run_offset, int max_runs) {
    if (L < 1) return fail(XGPR_ERR_ARRAY_DIMS, "incorrect array dims passed");
    if (conv_width <= 0 || L < conv_width) return fail(XGPR_ERR_CONV_WIDTH, "invalid conv_width");
    if (vocab < 1 || vocab > 256) return fail(XGPR_ERR_ARRAY_DIMS, "token table: vocab must be 1 .. 256 (uint8 tokens)");
    int rc = site_list_check(sites, K, L);
    if (rc) return rc;
    SiteLayout lay;
    site_layout(sites, K, L, conv_width, vocab, lay);
    if (lay.overflow) return fail(XGPR_ERR_UNSUPPORTED, "site list: a run's table does not fit 62 bits");
    const bool fill = run_first_window || run_last_window || run_first_site || run_sites || run_offset;
    if (fill && max_runs < lay.nruns) return fail(XGPR_ERR_ARRAY_DIMS, "site list: max_runs is smaller than the run count");
    for (int q = 0; q < lay.nruns; q++) {
        if (run_first_window) run_first_window[q] = lay.jlo[q];
        if (run_last_window) run_last_window[q] = lay.jhi[q];
        if (run_first_site) run_first_site[q] = lay.first[q];
        if (run_sites) run_sites[q] = lay.g[q];
        if (run_offset) run_offset[q] = lay.off[q];
    }
    return lay.nruns;
}

size_t site_scan_workspace_bytes_impl(long R, long n, int K) {
    const long runs = K >= 1 ? 2L * K - 1 : 0;           // the corner array holds one double per sequence and run: at most 2 K - 1 runs
    return masks_bytes(R) + (size_t)(n > 0 ? n : 0) * (size_t)runs * sizeof(double);
}

constexpr EditScanOp SITE_OP = {0, "the site scan serves windows of up to 1024 elements and tables of up to 4608 floats (see xgpr_conv_token_site_scan_ok)",
                                "too many rows for one launch (n * sum over the runs of vocab^(sites - 1) < 2^24)"};

int site_scan_impl(const uint8_t *tokens, const float *table, const double *w, double *out, const int8_t *radem, const float *chi,
                   const int32_t *seqlen_host, const int32_t *seqlen_dev, const int32_t *sites_host, int K, long n, long L, long vocab,
                   long C, long num_freqs, long R, int conv_width, int scaling_type, int fit_intercept, void *workspace, size_t wbytes,
                   void *stream) {
    // the pair scan's checks down to vocab; the predicate's refusal (the last of them) waits until the site list has been looked at
    const int shape = edit_scan_shape_check(SITE_OP, seqlen_host, n, L, vocab, C, num_freqs, R, conv_width, scaling_type);
    if (shape && shape != XGPR_ERR_UNSUPPORTED) return shape;
    const std::string refusal = g_err;
    int rc = site_list_check(sites_host, K, L);
    if (rc) return rc;
    for (long i = 0; i < n; i++)
        if (sites_host[K - 1] >= seqlen_host[i]) return fail(XGPR_ERR_SEQLEN_RANGE, "site list: every site must lie inside every sequence");
    if (shape) { g_err = refusal; return shape; }
    SiteLayout lay;
    site_layout(sites_host, K, L, conv_width, vocab, lay);
    if (lay.max_g > SITE_MAX_COVER)
        return fail(XGPR_ERR_UNSUPPORTED, "the site scan serves up to 4 sites inside one window (see xgpr_conv_token_site_scan_ok)");
    if (n == 0) return 0;
    if (!workspace || wbytes < site_scan_workspace_bytes_impl(R, n, K))
        return fail(XGPR_ERR_WORKSPACE, "workspace too small (see xgpr_conv_token_site_scan_workspace_bytes)");
    if (!(tokens && table && w && out && radem && chi && seqlen_dev)) return fail(XGPR_ERR_WORKSPACE, "NULL array pointer");
    hipStream_t st = (hipStream_t)stream;
    SiteScanArgs ss = {};
    long rows = 0;                                       // (max_g <= 4 and vocab <= 256: no overflow)
    for (int q = 0; q < lay.nruns; q++) {
        long per = 1;
        for (int m = 1; m < lay.g[q]; m++) per *= vocab;
        if (rows > 16777215L) return fail(XGPR_ERR_UNSUPPORTED, SITE_OP.too_many);
        SiteRun &r = ss.run[q];
        r.jlo = lay.jlo[q]; r.jhi = lay.jhi[q]; r.g = lay.g[q]; r.row0 = (unsigned)rows; r.off = lay.off[q];
        for (int m = 0; m < lay.g[q]; m++) r.pos[m] = sites_host[lay.first[q] + m];
        r.plast = r.pos[lay.g[q] - 1];
        for (int m = 0; m < SITE_MAX_COVER - 1; m++) r.ppos[m] = m < lay.g[q] - 1 ? r.pos[lay.g[q] - 2 - m] : SITE_NO_POS;
        rows += per;
    }
    if (n > 16777215L || rows > 16777215L || n * rows > 16777215L) return fail(XGPR_ERR_UNSUPPORTED, SITE_OP.too_many);
    ss.e = edit_scan_args(tokens, table, w, chi, seqlen_dev, n, L, vocab, C, num_freqs, R, conv_width, scaling_type, fit_intercept, workspace);
    ss.e.out = out;
    ss.corner = reinterpret_cast<double *>(static_cast<char *>(workspace) + masks_bytes(R));
    ss.T = lay.T; ss.rows = (unsigned)rows; ss.nruns = lay.nruns;
    rc = pack_masks(radem, (uint64_t *)workspace, R, ss.e.ig.MW, st);
    if (rc) return rc;
    rc = dispatch_lg<1, 10>(ilog2(padded_width(ss.e.ig.d)), TOO_WIDE_WAVE, [&](auto LG) {
        return launch(site_scan_grid_kernel<decltype(LG)::value>, dim3((unsigned)(n * rows)), dim3(256), 0, st,
                      "site_scan_grid_kernel launch", ss);
    });
    if (rc) return rc;
    rc = launch(site_scan_corner_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, "site_scan_corner_kernel launch", ss);
    if (rc) return rc;
    return launch(site_scan_diff_kernel, dim3((unsigned)(n * rows)), dim3(256), 0, st, "site_scan_diff_kernel launch", ss);
}
