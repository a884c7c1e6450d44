// pair_scan.inc -- part of xgpr_hip.hip (included inside its anonymous namespace, after edit_scan.inc): the exact NON-ADDITIVE part of
// every pair of single-token substitutions closer than conv_width, on a weighted sum of the SEQUENCE and GRAPH kernels' random features
// (xgpr_conv_token_pair_scan_f32, include/xgpr_hip_pair_scan.h; DESIGN.md 3.24).
//
// Notation of edit_scan.inc.  For positions l1 < l2 = l1 + d of sequence i, tokens v1, v2 and o1 = t[l1], o2 = t[l2]:
//     eps[i, l1, d - 1, v1, v2] = r(nk) sum_{j in J(l1) & J(l2)} [ c(win_j with v1, v2) - c(win_j with v1) - c(win_j with v2) + c(win_j) ]
//         J(l1) & J(l2) = { j : max(0, l2 - cw + 1) <= j <= min(l1, nk - 1) }                the windows that cover BOTH positions
// -- with subst of edit_scan.inc,  m(t[l1 := v1, l2 := v2]) - m(t) = subst[l1, v1] + subst[l2, v2] + eps  exactly; a window that covers
// one of the two positions alone cancels in the double difference, and no window covers both at d >= cw: the band 1 <= d <= cw - 1 is
// the whole of it.  With  G[v1, v2] = sum_{j in J(l1) & J(l2)} c(win_j with v1 at l1 and v2 at l2):
//     eps = r ( (G[v1, v2] - G[v1, o2]) - (G[o1, v2] - G[o1, o2]) ).
//
// Two kernels, both writing `out` alone.
//   pair_scan_grid_kernel   one workgroup of four waves per (sequence, l1, d, v1): the body of conv_token_edit_scan_kernel's substitution
//       mode with one more step.  The shared windows run outermost in ascending j; a window's token bytes are fetched ONCE and the byte
//       at offset q1 = l1 - j is patched to v1 in the policy's registers (PairTokenWindows::patch: no mutant is written); wave w takes
//       the tiles b = w, w + 4, ..., holds the tile's float64 weight pairs in registers, and v2 = 0 .. V - 1 runs innermost through
//       take_subst(t, q2, v2): the forward half of the gradient tile (the float32 cos / sin arguments of xgpr_conv_token_rows_f32 bit for
//       bit), the lane's part of the score in float64 in ascending register order, wave_sum, lane 0 into the wave's own acc[w][v2].
//       After the last window one barrier, and thread v2 stores the RAW sum G[v1, v2] = ((a0 + a1) + a2) + a3 into out[i, l1, d - 1, v1, v2].
//       The pairs (v1, o2), (o1, v2) and (o1, o2) go through exactly this path like every other pair.
//   pair_scan_diff_kernel   one workgroup per (sequence, l1, d), IN PLACE on its V x V block: row G[o1, :], column G[:, o2] and
//       G[o1, o2] go to LDS, a barrier, and only then is every element overwritten with r ((G[v1, v2] - G[v1, o2]) - (G[o1, v2] - G[o1, o2])).
//       The planes v1 == o1 and v2 == o2 are (x - y) - (x - y) and 0 - 0 on identical bits: +0.0 by construction, not by masking.
// No slot is shared between waves or workgroups: no atomics, the order of every sum is fixed ((j ascending, b ascending) into a slot,
// then the four waves in order), every block is a bitwise function of its own sequence, the table and the weights, and two identical
// table rows give identical bits along both token axes.  Slots with l1 or l2 past the sequence store 0.0 in the first kernel and are
// left alone by the second; both exits are uniform over the workgroup and come before any barrier.  LDS is what the substitution mode
// holds; no workspace beyond the packed sign masks.
// ------------------------------------------------------------------------------------

// PairTokenWindows: one more step between a fetch and its variants.  patch(q, tok) makes the fetched window hold token `tok` at position
// offset q for every take / take_subst that follows, until the next issue.  Padded registers carry the offset 0xffff and never match.
template <int LOG2P> struct PairTokenWindows : IndelTokenWindows<LOG2P> {
    using Base = TokenWindows<LOG2P>;
    __device__ __forceinline__ void patch(unsigned q, unsigned tok) {
        #pragma unroll
        for (int r = 0; r < Base::N; r++) {
            const unsigned p = Base::PACK ? this->pos[r] & 0xffffu : this->pos[r];
            this->tk[r] = p == q ? tok : this->tk[r];
        }
    }
};

// what a workgroup index means to both kernels: (sequence, l1, d) and whether both positions lie inside the sequence
struct PairSlot { long i; int l1, l2, len; bool live; };
__device__ __forceinline__ PairSlot pair_slot(const EditScanArgs &s, unsigned slot) {
    const unsigned band = (unsigned)(s.win.conv_width - 1), per = (unsigned)s.L * band;
    PairSlot p;
    p.i = slot / per;
    const unsigned e = slot - (unsigned)p.i * per;
    p.l1 = (int)(e / band);
    p.l2 = p.l1 + 1 + (int)(e - (unsigned)p.l1 * band);
    p.len = s.win.seqlen[p.i];
    p.live = p.l2 < p.len;                               // (l1 < l2)
    return p;
}

template <int LOG2P>
__global__ __launch_bounds__(256) void pair_scan_grid_kernel(EditScanArgs s) {
    constexpr bool TP = LOG2P >= 7;
    __shared__ __attribute__((aligned(16))) float tab[TOK_TABLE_FLOATS + 4];
    __shared__ __attribute__((aligned(16))) float tbuf[TP ? 4 * TBUF_FLOATS : 4];
    __shared__ double acc[4][256];                       // acc[w][v2]: wave w's sum for token v2 (vocab <= 256)
    const InputGradArgs &a = s.ig;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int V = s.win.vocab, cw = s.win.conv_width;
    const unsigned slot = blockIdx.x / (unsigned)V;      // blockIdx.x = ((i L + l1) (cw - 1) + d - 1) V + v1 < 2^24: the row of out
    const unsigned v1 = blockIdx.x - slot * (unsigned)V;
    const PairSlot ps = pair_slot(s, slot);
    double *orow = s.out + (long)blockIdx.x * V;
    // (uniform over the workgroup: nobody waits at the barriers below)
    if (!ps.live) {
        for (int v = threadIdx.x; v < V; v += 256) orow[v] = 0.0;
        return;
    }
    const long i = ps.i;
    const int nk = ps.len - cw + 1;
    const int nt = V * s.win.kmer_stride;                // <= TOK_TABLE_FLOATS (edit_scan_ok)
    for (int t = threadIdx.x; t < nt; t += 256) tab[t] = s.win.x[t];
    if (threadIdx.x == 0) tab[nt] = 0.0f;
    #pragma unroll
    for (int w = 0; w < 4; w++) acc[w][threadIdx.x] = 0.0;
    // the windows that cover both positions: never empty (l2 - cw + 1 <= l1 and <= nk - 1, as d < cw and l2 < len)
    const int jlo = ps.l2 - cw + 1 > 0 ? ps.l2 - cw + 1 : 0;
    const int jhi = ps.l1 < nk - 1 ? ps.l1 : nk - 1;
    __syncthreads();

    float *tb = tbuf + wv * (TP ? TBUF_FLOATS : 1);
    const float chs = TP ? a.chi_scale * sorf_kept_sign(lane) : a.chi_scale;     // the sign tile_sorf kept, into chi (exact)
    PairTokenWindows<LOG2P> win;
    win.tab = reinterpret_cast<const char *>(tab);
    win.begin(s.win, i, lane);
    for (int j = jlo; j <= jhi; j++) {
        const unsigned q2 = (unsigned)(ps.l2 - j);       // the second position's offset inside window j
        // the window's token bytes: once per (slot, v1, window), for all v2 and tiles; then v1 at the first position's offset
        win.issue(j);
        win.patch((unsigned)(ps.l1 - j), v1);
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
                win.take_subst(t, q2, (unsigned)v);
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

__global__ __launch_bounds__(256) void pair_scan_diff_kernel(EditScanArgs s) {
    __shared__ double row[256], col[256];                // G[o1, :] and G[:, o2]
    const int V = s.win.vocab;
    const PairSlot ps = pair_slot(s, blockIdx.x);
    if (!ps.live) return;                                // (uniform; the zeros of the first kernel stay.  The tokens past a length are never read)
    double *G = s.out + (long)blockIdx.x * V * V;
    const uint8_t *trow = s.win.tokens + ps.i * s.win.row_stride;
    const int o1 = trow[ps.l1], o2 = trow[ps.l2];
    for (int v = threadIdx.x; v < V; v += 256) {
        row[v] = G[(long)o1 * V + v];
        col[v] = G[(long)v * V + o2];
    }
    // IN PLACE: everything an element's new value needs from OTHER elements of the block is in LDS before the first store -- the
    // barrier separates all those reads from all writes --, and the element itself is read by the one thread that overwrites it.
    __syncthreads();
    const double rs = indel_norm(s.ig.scale, s.scaling_type, ps.len - s.win.conv_width + 1);
    const double corner = row[o2];                       // G[o1, o2]
    for (int e = threadIdx.x; e < V * V; e += 256) {
        const int a = e / V, b = e - a * V;
        G[e] = rs * ((G[e] - col[a]) - (row[b] - corner));
    }
}

int conv_token_pair_scan_ok_impl(long width, long vocab, long C, long num_freqs) { return edit_scan_ok(width, vocab, C, num_freqs); }

constexpr EditScanOp PAIR_OP = {0, "the pair scan serves windows of up to 1024 elements and tables of up to 4608 floats (see xgpr_conv_token_pair_scan_ok)",
                                "too many rows for one launch (n * L * (conv_width - 1) * vocab < 2^24)"};

int pair_scan_impl(const uint8_t *tokens, const float *table, const double *w, double *out, const int8_t *radem, const float *chi,
                   const int32_t *seqlen_host, const int32_t *seqlen_dev, long n, long L, long vocab, long C, long num_freqs, long R,
                   int conv_width, int scaling_type, int fit_intercept, void *workspace, size_t wbytes, void *stream) {
    int rc = edit_scan_shape_check(PAIR_OP, seqlen_host, n, L, vocab, C, num_freqs, R, conv_width, scaling_type);
    if (rc || n == 0 || conv_width == 1) return rc;      // (conv_width 1: no two positions share a window, out has no elements)
    rc = edit_scan_buffer_check(workspace, wbytes, R, tokens && table && w && out && radem && chi && seqlen_dev, true);
    if (rc) return rc;
    const long band = conv_width - 1;
    if (n > 16777215L || L > 16777215L || n * L > 16777215L || n * L * band * vocab > 16777215L) return fail(XGPR_ERR_UNSUPPORTED, PAIR_OP.too_many);
    hipStream_t st = (hipStream_t)stream;
    EditScanArgs s = edit_scan_args(tokens, table, w, chi, seqlen_dev, n, L, vocab, C, num_freqs, R, conv_width, scaling_type, fit_intercept,
                                    workspace);
    s.out = out;
    rc = pack_masks(radem, (uint64_t *)workspace, R, s.ig.MW, st);
    if (rc) return rc;
    rc = dispatch_lg<1, 10>(ilog2(padded_width(s.ig.d)), TOO_WIDE_WAVE, [&](auto LG) {
        return launch(pair_scan_grid_kernel<decltype(LG)::value>, dim3((unsigned)(n * L * band * vocab)), dim3(256), 0, st,
                      "pair_scan_grid_kernel launch", s);
    });
    if (rc) return rc;
    return launch(pair_scan_diff_kernel, dim3((unsigned)(n * L * band)), dim3(256), 0, st, "pair_scan_diff_kernel launch", s);
}
