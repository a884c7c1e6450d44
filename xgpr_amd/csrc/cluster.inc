// cluster.inc -- part of xgpr_hip.hip (included inside its anonymous namespace, after zblock.inc): the two contractions of a Lloyd
// iteration over float32 feature rows (include/xgpr_hip_cluster.h, DESIGN.md 3.19).
// ------------------------------------------------------------------------------------
//   kmeans_assign_kernel:  labels[i] = argmin_k cn_k - 2 z_i . c_k     (contract features on the float64 matrix cores; a wave owns
//                                                                       16 RT rows, the centres pass through LDS 16 features at a time)
//   kmeans_update_kernel:  part[range][k'][m] = sum of the rows of the range that carry label k'   (a lane owns a feature column, a
//                                                                       wave 64 of them and up to 32 labels; its accumulator lives in LDS)
// Operand maps of v_mfma_f64_16x16x4_f64 as in zblock.inc: A lane l -> A[i = l & 15][k = l >> 4], B lane l -> B[k = l >> 4][j = l & 15],
// D register r -> D[i = (l >> 4) + 4 r][j = l & 15].  The rows are the A operand (a lane loads 16 bytes = 4 consecutive features and
// spends one per instruction), the centres the B operand: column j of tile ct is centre 16 ct + j.  Every centre column goes through
// the same instruction sequence, so two centres with identical contents get bit-identical scores and the lower index wins.
// Nothing here uses a floating-point atomic: every sum has one order, fixed by (n, num_rffs, k).
// ------------------------------------------------------------------------------------
constexpr int KM_MAX_K = 256;     // 16 column tiles of 8 accumulator registers per lane
constexpr int KM_FC = 16;         // features per LDS chunk of the centres (one float4 per lane and row tile)
constexpr long KM_UPD_TARGET_WGS = 1024;   // workgroups the update launch aims for (row ranges x column groups)
constexpr long KM_UPD_MAX_RANGES = 256;    // ... and its caps on row ranges: the workspace holds one [k, num_rffs] float64 slab per range,
constexpr long KM_UPD_MAX_WS_BYTES = 256L << 20;   // at most this many bytes of them (one range at least)
constexpr long KM_UPD_MIN_ROWS = 256;      // rows per range at least (short launches: fewer ranges)

int kmeans_ok_impl(long M, long k) { return (M >= 4 && M % 4 == 0 && k >= 1 && k <= KM_MAX_K) ? 1 : 0; }

// cn[k] = sum_m centers[k, m]^2: one wave per centre, lane l sums m = l, l + 64, ... in ascending m, then a fixed butterfly
__global__ __launch_bounds__(64) void kmeans_center_norms_kernel(const double *__restrict__ centers, double *cn, long M) {
    const int lane = threadIdx.x;
    const double *c = centers + (long)blockIdx.x * M;
    double s = 0.0;
    for (long m = lane; m < M; m += 64) s += c[m] * c[m];
    #pragma unroll
    for (int off = 1; off < 64; off <<= 1) s += __shfl_xor(s, off);
    if (lane == 0) cn[blockIdx.x] = s;
}

struct KmAssignArgs {
    const float *rows; const double *centers; const double *cn; int32_t *labels; double *dist2;
    long n; long M; int k;
};

// CT column tiles (k <= 16 CT), RT row tiles per wave; 8 waves per workgroup (two per SIMD, as the block projection).
template <int CT, int RT>
__global__ __launch_bounds__(512) void kmeans_assign_kernel(KmAssignArgs a) {
    constexpr int NT = 512;
    constexpr int KP = 16 * CT;
    constexpr int VS = KP + 4;                          // +32 B per feature row: lane groups g and g + 1 land 128 B apart
    constexpr int VPT = (KM_FC * KP + NT - 1) / NT;     // centre elements staged per thread per chunk
    __shared__ __attribute__((aligned(16))) double vs[2][KM_FC * VS];
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long rbase = (long)blockIdx.x * (128L * RT) + 16 * RT * w;
    const float *rp[RT];
    #pragma unroll
    for (int rt = 0; rt < RT; rt++) {
        long row = rbase + 16 * rt + c;
        if (row >= a.n) row = a.n - 1;                  // clamped rows are computed and never stored
        rp[rt] = a.rows + row * a.M;
    }
    double4_t acc[RT][CT];
    double zz[RT];
    #pragma unroll
    for (int rt = 0; rt < RT; rt++) {
        zz[rt] = 0.0;
        #pragma unroll
        for (int ct = 0; ct < CT; ct++) acc[rt][ct] = (double4_t){0.0, 0.0, 0.0, 0.0};
    }
    const long nchunks = (a.M + KM_FC - 1) / KM_FC;

    auto load_a = [&](long ch, float4 (&dst)[RT]) {
        long f = ch * KM_FC + 4 * g;
        if (f > a.M - 4) f = a.M - 4;                   // past the last feature: the centres' chunk supplies the zeros
        #pragma unroll
        for (int rt = 0; rt < RT; rt++) dst[rt] = *reinterpret_cast<const float4 *>(rp[rt] + f);
    };
    auto load_v = [&](long ch, double (&dst)[VPT]) {
        #pragma unroll
        for (int e = 0; e < VPT; e++) {
            const int idx = threadIdx.x + NT * e;
            const int col = idx / KM_FC;
            const long f = ch * KM_FC + idx % KM_FC;
            const bool ok = idx < KM_FC * KP && col < a.k && f < a.M;
            const double v = a.centers[ok ? (long)col * a.M + f : 0];
            dst[e] = ok ? v : 0.0;
        }
    };
    auto store_v = [&](int buf, const double (&src)[VPT]) {
        #pragma unroll
        for (int e = 0; e < VPT; e++) {
            const int idx = threadIdx.x + NT * e;
            if (idx < KM_FC * KP) vs[buf][(idx % KM_FC) * VS + idx / KM_FC] = src[e];
        }
    };
    auto compute = [&](long ch, const float4 (&cur)[RT], int buf) {
        const double *vb = vs[buf];
        if (ch * KM_FC + 4 * g < a.M) {                 // sum of squares of this lane's four features, on the vector unit
            #pragma unroll
            for (int rt = 0; rt < RT; rt++) {
                #pragma unroll
                for (int e = 0; e < 4; e++) {
                    const double x = elem(cur[rt], e);
                    zz[rt] += x * x;
                }
            }
        }
        #pragma unroll
        for (int e = 0; e < 4; e++) {
            double b[CT];
            #pragma unroll
            for (int ct = 0; ct < CT; ct++) b[ct] = vb[(4 * g + e) * VS + 16 * ct + c];
            #pragma unroll
            for (int rt = 0; rt < RT; rt++) {
                const double av = elem(cur[rt], e);
                #pragma unroll
                for (int ct = 0; ct < CT; ct++)
                    acc[rt][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, b[ct], acc[rt][ct], 0, 0, 0);
            }
        }
    };

    // two LDS buffers, one barrier per chunk: chunk ch + 1 is loaded (registers) before and stored (LDS) after the MFMAs of chunk ch
    float4 cur[RT], nxt[RT];
    double vreg[VPT];
    load_v(0, vreg);
    load_a(0, cur);
    store_v(0, vreg);
    __syncthreads();
    for (long ch = 0; ch < nchunks; ch++) {
        const bool more = ch + 1 < nchunks;             // workgroup-uniform
        if (more) { load_v(ch + 1, vreg); load_a(ch + 1, nxt); }
        compute(ch, cur, (int)(ch & 1));
        if (more) {
            store_v((int)((ch + 1) & 1), vreg);
            #pragma unroll
            for (int rt = 0; rt < RT; rt++) cur[rt] = nxt[rt];
        }
        __syncthreads();
    }

    // ---- epilogue.  Row 16 rt + c's sum of squares sits in the four lanes {c, c + 16, c + 32, c + 48}: (g0 + g1) + (g2 + g3).
    #pragma unroll
    for (int rt = 0; rt < RT; rt++) {
        zz[rt] += __shfl_xor(zz[rt], 16);
        zz[rt] += __shfl_xor(zz[rt], 32);
    }
    double cnv[CT];
    #pragma unroll
    for (int ct = 0; ct < CT; ct++) cnv[ct] = a.cn[16 * ct + c < a.k ? 16 * ct + c : 0];
    constexpr int NONE = 0x7fffffff;
    #pragma unroll
    for (int rt = 0; rt < RT; rt++) {
        #pragma unroll
        for (int r = 0; r < 4; r++) {
            // D register r: row 16 rt + g + 4 r, column 16 ct + c.  This lane's columns in ascending order, strict <
            double best = 0.0;
            int bi = NONE;
            #pragma unroll
            for (int ct = 0; ct < CT; ct++) {
                const int col = 16 * ct + c;
                const double s = cnv[ct] - 2.0 * acc[rt][ct][r];
                if (col < a.k && (bi == NONE || s < best)) { best = s; bi = col; }
            }
            // ... then the 16 lanes of the row: the smaller score, on equal scores the lower index
            #pragma unroll
            for (int off = 1; off < 16; off <<= 1) {
                const double os = __shfl_xor(best, off);
                const int oi = __shfl_xor(bi, off);
                if (oi != NONE && (bi == NONE || os < best || (os == best && oi < bi))) { best = os; bi = oi; }
            }
            const double zrow = __shfl(zz[rt], g + 4 * r);          // the row's sum of squares (any lane with c' = g + 4 r)
            const long row = rbase + 16 * rt + g + 4 * r;
            if (c == 0 && row < a.n) {
                a.labels[row] = bi;
                if (a.dist2) {
                    const double d = zrow + best;
                    a.dist2[row] = d > 0.0 ? d : 0.0;
                }
            }
        }
    }
}

template <int CT, int RT>
int kmeans_assign_launch(const KmAssignArgs &a, hipStream_t st) {
    const long per = 128L * RT;
    hipLaunchKernelGGL((kmeans_assign_kernel<CT, RT>), dim3((unsigned)((a.n + per - 1) / per)), dim3(512), 0, st, a);
    HIP_TRY(hipGetLastError(), "kmeans_assign_kernel launch");
    return 0;
}

size_t kmeans_assign_workspace_bytes_impl(long n, long M, long k) {
    if (n <= 0 || M <= 0 || k < 1) return 0;
    return align_up((size_t)k * sizeof(double), 256);               // the centres' squared norms
}

int kmeans_assign_impl(const float *rows, const double *centers, int32_t *labels, double *dist2, long n, long M, long k, void *workspace,
                       size_t wbytes, void *stream) {
    if (n < 0 || M < 1 || k < 1) return fail(XGPR_ERR_ARRAY_DIMS, "incorrect array dims passed");
    if (!kmeans_ok_impl(M, k))
        return fail(XGPR_ERR_UNSUPPORTED, "k-means serves num_rffs a multiple of 4 and 1 .. 256 centres (see xgpr_kmeans_ok)");
    if (n == 0) return 0;
    if (!rows || !centers || !labels) return fail(XGPR_ERR_WORKSPACE, "NULL array pointer");
    if (!aligned16(rows) || !aligned16(centers)) return fail(XGPR_ERR_WORKSPACE, "rows and centers must be 16-byte aligned");
    if (!workspace || wbytes < kmeans_assign_workspace_bytes_impl(n, M, k) || !aligned16(workspace))
        return fail(XGPR_ERR_WORKSPACE, "workspace too small (see xgpr_kmeans_assign_workspace_bytes)");
    if (n > 2147483647L - 1024) return fail(XGPR_ERR_UNSUPPORTED, "too many datapoints for one launch");
    hipStream_t st = (hipStream_t)stream;
    double *cn = reinterpret_cast<double *>(workspace);
    hipLaunchKernelGGL(kmeans_center_norms_kernel, dim3((unsigned)k), dim3(64), 0, st, centers, cn, M);
    HIP_TRY(hipGetLastError(), "kmeans_center_norms_kernel launch");
    const KmAssignArgs a{rows, centers, cn, labels, dist2, n, M, (int)k};
    if (k <= 16) return kmeans_assign_launch<1, 4>(a, st);
    if (k <= 32) return kmeans_assign_launch<2, 4>(a, st);
    if (k <= 64) return kmeans_assign_launch<4, 4>(a, st);
    if (k <= 128) return kmeans_assign_launch<8, 2>(a, st);
    return kmeans_assign_launch<16, 1>(a, st);
}

// ------------------------------------------------------------------------------------ update
// A wave owns 64 feature columns (lane l: column l) and KG consecutive labels, with a [KG, 64] float64 accumulator of its own in LDS
// (lane l only ever touches column l of it: no barrier).  A workgroup is WC waves across columns x WL waves across label groups over
// the same rows: with many centres the [k, 64] accumulator is split over the WL waves, each of which walks all the rows of the range
// (the workgroup's repeated loads of a row hit the vector cache) and adds the rows of its own labels -- so that eight waves per CU keep
// loads in flight at k = 256 instead of one.  blockIdx.y is the row range, walked in ascending order by every wave.
template <int KG, int WC, int WL>
__global__ __launch_bounds__(64 * WC * WL) void kmeans_update_kernel(const float *__restrict__ rows, const int32_t *__restrict__ labels,
                                                                     double *part, long n, long M, int k, long rows_per_range) {
    __shared__ double acc[WC * WL][KG][64];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int wc = w % WC, wl = w / WC;
    const long col0 = ((long)blockIdx.x * WC + wc) * 64;
    const int lb = wl * KG;                              // this wave's labels: [lb, min(lb + KG, k))
    if (col0 >= M || lb >= k) return;                    // wave-uniform; no barrier below
    const int kg = k - lb < KG ? k - lb : KG;
    const long col = col0 + lane;
    const bool live = col < M;
    const long rbeg = (long)blockIdx.y * rows_per_range;
    long rend = rbeg + rows_per_range;
    if (rend > n) rend = n;
    for (int j = 0; j < kg; j++) acc[w][j][lane] = 0.0;
    const float *p = rows + (live ? col : M - 1);
    // 16 rows of loads in flight per wave.  (Measured and not kept: blocks of 32 rows with the next block's loads issued before the
    // current block is added -- no faster at any measured shape: profiles/kmeans_prefetch_form.json, DESIGN.md 3.19.)
    constexpr int U = 16;
    for (long i = rbeg; i < rend; i += U) {
        float x[U];
        int lab[U];
        #pragma unroll
        for (int u = 0; u < U; u++) {
            const long r = i + u < rend ? i + u : rend - 1;          // clamped rows carry label -1
            lab[u] = i + u < rend ? labels[r] : -1;
            x[u] = p[r * M];
        }
        #pragma unroll
        for (int u = 0; u < U; u++) {
            const unsigned rel = (unsigned)lab[u] - (unsigned)lb;    // (a label outside [0, k) is skipped by every wave)
            if (rel < (unsigned)kg) acc[w][rel][lane] += (double)x[u];
        }
    }
    if (live) {
        double *slab = part + ((long)blockIdx.y * k + lb) * M + col;
        for (int j = 0; j < kg; j++) slab[(long)j * M] = acc[w][j][lane];
    }
}

// sums[i] (+)= sum over the row ranges, in range order, of part[range][i]
__global__ __launch_bounds__(256) void kmeans_reduce_sums_kernel(const double *__restrict__ part, double *sums, long total, long nranges,
                                                                 int accumulate) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    double s = 0.0;
    for (long r = 0; r < nranges; r++) s += part[r * total + i];
    sums[i] = accumulate ? sums[i] + s : s;
}

// counts[k'] (+)= the number of labels equal to k': integer atomics in LDS (exact in any order), one workgroup
__global__ __launch_bounds__(1024) void kmeans_counts_kernel(const int32_t *__restrict__ labels, long long *counts, long n, int k,
                                                             int accumulate) {
    __shared__ unsigned hist[KM_MAX_K];
    for (int j = threadIdx.x; j < KM_MAX_K; j += 1024) hist[j] = 0u;
    __syncthreads();
    for (long i = threadIdx.x; i < n; i += 1024) {
        const int lab = labels[i];
        if ((unsigned)lab < (unsigned)k) atomicAdd(&hist[lab], 1u);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < k; j += 1024) counts[j] = (accumulate ? counts[j] : 0LL) + (long long)hist[j];
}

struct KmUpdGeom { int cfg; int WC; long nbx; long nranges; long rows_per; size_t bytes; };
KmUpdGeom kmeans_update_geometry(long n, long M, long k) {
    KmUpdGeom gm{};
    gm.cfg = k <= 16 ? 0 : k <= 32 ? 1 : k <= 64 ? 2 : k <= 128 ? 3 : 4;       // (KG, WC, WL) = (16, 8, 1) (32, 8, 1) (32, 4, 2) (32, 2, 4) (32, 1, 8)
    gm.WC = gm.cfg <= 1 ? 8 : gm.cfg == 2 ? 4 : gm.cfg == 3 ? 2 : 1;
    const long nslabs = (M + 63) / 64;
    gm.nbx = (nslabs + gm.WC - 1) / gm.WC;
    if (n <= 0) { gm.nranges = 0; gm.rows_per = 16; gm.bytes = 0; return gm; }
    const long slab_bytes = k * M * (long)sizeof(double);
    long nr = (KM_UPD_TARGET_WGS + gm.nbx - 1) / gm.nbx;
    if (nr > KM_UPD_MAX_RANGES) nr = KM_UPD_MAX_RANGES;
    if (nr > KM_UPD_MAX_WS_BYTES / slab_bytes) nr = KM_UPD_MAX_WS_BYTES / slab_bytes;
    const long by_rows = (n + KM_UPD_MIN_ROWS - 1) / KM_UPD_MIN_ROWS;
    if (nr > by_rows) nr = by_rows;
    if (nr < 1) nr = 1;
    gm.rows_per = ((n + nr - 1) / nr + 15) / 16 * 16;
    gm.nranges = (n + gm.rows_per - 1) / gm.rows_per;
    gm.bytes = (size_t)gm.nranges * (size_t)slab_bytes;
    return gm;
}

size_t kmeans_update_workspace_bytes_impl(long n, long M, long k) {
    if (n <= 0 || M <= 0 || k < 1 || k > KM_MAX_K) return 0;
    return kmeans_update_geometry(n, M, k).bytes;
}

template <int KG, int WC, int WL>
int kmeans_update_launch(const float *rows, const int32_t *labels, double *part, long n, long M, int k, const KmUpdGeom &gm, hipStream_t st) {
    hipLaunchKernelGGL((kmeans_update_kernel<KG, WC, WL>), dim3((unsigned)gm.nbx, (unsigned)gm.nranges), dim3(64 * WC * WL), 0, st, rows, labels,
                       part, n, M, k, gm.rows_per);
    HIP_TRY(hipGetLastError(), "kmeans_update_kernel launch");
    return 0;
}

int kmeans_update_impl(const float *rows, const int32_t *labels, double *sums, long long *counts, long n, long M, long k, int accumulate,
                       void *workspace, size_t wbytes, void *stream) {
    if (n < 0 || M < 1 || k < 1) return fail(XGPR_ERR_ARRAY_DIMS, "incorrect array dims passed");
    if (!kmeans_ok_impl(M, k))
        return fail(XGPR_ERR_UNSUPPORTED, "k-means serves num_rffs a multiple of 4 and 1 .. 256 centres (see xgpr_kmeans_ok)");
    if (!sums || !counts || (n > 0 && (!rows || !labels))) return fail(XGPR_ERR_WORKSPACE, "NULL array pointer");
    if (!aligned16(sums) || (n > 0 && !aligned16(rows))) return fail(XGPR_ERR_WORKSPACE, "rows and sums must be 16-byte aligned");
    const KmUpdGeom gm = kmeans_update_geometry(n, M, k);
    if (gm.bytes > 0 && (!workspace || wbytes < gm.bytes || !aligned16(workspace)))
        return fail(XGPR_ERR_WORKSPACE, "workspace too small (see xgpr_kmeans_update_workspace_bytes)");
    if (n > 2147483647L - 1024) return fail(XGPR_ERR_UNSUPPORTED, "too many datapoints for one launch");
    if (n == 0 && accumulate) return 0;
    hipStream_t st = (hipStream_t)stream;
    double *part = reinterpret_cast<double *>(workspace);
    if (n > 0) {
        int rc;
        switch (gm.cfg) {
            case 0: rc = kmeans_update_launch<16, 8, 1>(rows, labels, part, n, M, (int)k, gm, st); break;
            case 1: rc = kmeans_update_launch<32, 8, 1>(rows, labels, part, n, M, (int)k, gm, st); break;
            case 2: rc = kmeans_update_launch<32, 4, 2>(rows, labels, part, n, M, (int)k, gm, st); break;
            case 3: rc = kmeans_update_launch<32, 2, 4>(rows, labels, part, n, M, (int)k, gm, st); break;
            default: rc = kmeans_update_launch<32, 1, 8>(rows, labels, part, n, M, (int)k, gm, st); break;
        }
        if (rc) return rc;
    }
    const long total = k * M;
    hipLaunchKernelGGL(kmeans_reduce_sums_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, part, sums, total, gm.nranges,
                       accumulate);
    HIP_TRY(hipGetLastError(), "kmeans_reduce_sums_kernel launch");
    hipLaunchKernelGGL(kmeans_counts_kernel, dim3(1), dim3(1024), 0, st, labels, counts, n, (int)k, accumulate);
    HIP_TRY(hipGetLastError(), "kmeans_counts_kernel launch");
    return 0;
}
