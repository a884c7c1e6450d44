// cg_kernels.inc -- part of xgpr_hip.hip (included inside its anonymous namespace, in order): CG vector updates, preconditioner apply, self test.
// ------------------------------------------------------------------------------------
// CG vector updates for one right-hand side (fitting_toolkit/cg_tools.py:255-274), fused into
// two single-workgroup kernels: M is only 10^3..10^5, so one workgroup reduces and updates the
// whole vector in a few microseconds, deterministically, instead of ~20 library launches.
// ------------------------------------------------------------------------------------
__device__ __forceinline__ double block_sum(double v, double *red /* [16] */) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    v = wave_sum(v);
    __syncthreads();               // red may still be read from a previous call
    if (lane == 0) red[w] = v;
    __syncthreads();
    double t = 0.0;
    for (int i = 0; i < nw; i++) t += red[i];
    return t;
}

// step 1 (cg_tools.py:256-265): w += lambda^2 p ; alpha = (r.z)/(p.w) ; x += alpha p ;
// r_next = r - alpha w ; err = |r| / |r_0|  (the lagging error, from the CURRENT residual).
// scal[0] = r.z, scal[1] = alpha, scal[2] = err.
// stop_tol > 0 (iterations replayed from a HIP graph, queued ahead of the host's convergence check): the
// solve stops ON THE DEVICE -- once the error of the previous iteration (scal[2]) is below stop_tol this
// and every later step leaves all vectors untouched (scal[4] = stopped flag), so x holds exactly the
// iterate the host-checked loop returns; scal[5] counts the iterations applied and scal[8 + i] keeps the
// error of iteration i for the host to read whenever it gets to it.
// err_out (optional): where the host reads the error from -- pinned host memory the device writes directly, so
// an iteration needs no copy command of its own.
__global__ __launch_bounds__(1024) void cg_step1_kernel(double *w, const double *__restrict__ p, double *x,
                                                        const double *__restrict__ r, double *r_next,
                                                        const double *__restrict__ z, double *scal, double lam2,
                                                        double init_norm, long M, double stop_tol, double *err_out) {
    __shared__ double red[3][16];
    if (stop_tol > 0.0 && (scal[4] != 0.0 || scal[2] < stop_tol)) {
        if (threadIdx.x == 0) scal[4] = 1.0;
        return;
    }
    // Eight elements per thread and batch, ALL their loads issued before the first use (w is stored in the same loop,
    // so the compiler cannot move the next element's loads above it: the plain loop paid a global-memory round trip
    // per element, 16 us for M = 8192).  Accumulation order per thread is unchanged (k = 0, 1, ...): same sums.
    constexpr int CGU = 8;
    const bool single = M <= (long)CGU * blockDim.x;        // one batch: the operands stay in registers for the update
    double rz = 0.0, pw = 0.0, rr = 0.0;
    double pv[CGU], rv[CGU], wv[CGU], zv[CGU], xv[CGU];
    for (long base = 0; base < M; base += (long)CGU * blockDim.x) {
        #pragma unroll
        for (int k = 0; k < CGU; k++) {
            const long i = base + threadIdx.x + (long)k * blockDim.x;
            const bool ok = i < M;
            const long ic = ok ? i : 0;
            pv[k] = p[ic]; rv[k] = r[ic]; wv[k] = w[ic]; zv[k] = z[ic]; xv[k] = x[ic];
            if (!ok) { pv[k] = 0.0; rv[k] = 0.0; wv[k] = 0.0; zv[k] = 0.0; }
        }
        #pragma unroll
        for (int k = 0; k < CGU; k++) {
            const long i = base + threadIdx.x + (long)k * blockDim.x;
            const double wi = wv[k] + lam2 * pv[k];
            wv[k] = wi;
            if (i < M) w[i] = wi;
            rz += rv[k] * zv[k];
            pw += pv[k] * wi;
            rr += rv[k] * rv[k];
        }
    }
    {   // the three sums through one pair of barriers (same per-wave and cross-wave order as block_sum)
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
        rz = wave_sum(rz); pw = wave_sum(pw); rr = wave_sum(rr);
        if (lane == 0) { red[0][wv] = rz; red[1][wv] = pw; red[2][wv] = rr; }
        __syncthreads();
        rz = 0.0; pw = 0.0; rr = 0.0;
        for (int i = 0; i < nw; i++) { rz += red[0][i]; pw += red[1][i]; rr += red[2][i]; }
    }
    const double alpha = rz / pw;
    if (single) {
        #pragma unroll
        for (int k = 0; k < CGU; k++) {
            const long i = threadIdx.x + (long)k * blockDim.x;
            if (i < M) {
                x[i] = xv[k] + alpha * pv[k];
                r_next[i] = rv[k] - alpha * wv[k];
            }
        }
    } else {
        for (long i = threadIdx.x; i < M; i += blockDim.x) {
            x[i] += alpha * p[i];
            r_next[i] = r[i] - alpha * w[i];
        }
    }
    if (threadIdx.x == 0) {
        const double err = sqrt(rr) / init_norm;
        scal[0] = rz; scal[1] = alpha; scal[2] = err;
        if (err_out) { *err_out = err; __threadfence_system(); }
        if (stop_tol > 0.0) {
            const long it = (long)scal[5];
            scal[8 + it] = err;
            scal[5] = (double)(it + 1);
        }
    }
}

// step 2 (cg_tools.py:271-274): beta = (r_next.z_next)/(r.z) ; p_next = z_next + beta p.  scal[3] = beta.
__global__ __launch_bounds__(1024) void cg_step2_kernel(const double *__restrict__ r_next, const double *__restrict__ z_next,
                                                        const double *__restrict__ p, double *p_next, double *scal, long M,
                                                        double stop_tol) {
    __shared__ double red[16];
    if (stop_tol > 0.0 && scal[4] != 0.0) return;
    constexpr int CGU = 8;                              // as in step 1: a batch's loads in flight together
    const bool single = M <= (long)CGU * blockDim.x;
    double rz = 0.0;
    double zv[CGU], pv[CGU];
    for (long base = 0; base < M; base += (long)CGU * blockDim.x) {
        double rv[CGU];
        #pragma unroll
        for (int k = 0; k < CGU; k++) {
            const long i = base + threadIdx.x + (long)k * blockDim.x;
            const bool ok = i < M;
            const long ic = ok ? i : 0;
            rv[k] = r_next[ic]; zv[k] = z_next[ic]; pv[k] = p[ic];
            if (!ok) { rv[k] = 0.0; zv[k] = 0.0; }
        }
        #pragma unroll
        for (int k = 0; k < CGU; k++) rz += rv[k] * zv[k];
    }
    rz = block_sum(rz, red);
    const double beta = rz / scal[0];
    if (single) {
        #pragma unroll
        for (int k = 0; k < CGU; k++) {
            const long i = threadIdx.x + (long)k * blockDim.x;
            if (i < M) p_next[i] = zv[k] + beta * pv[k];
        }
    } else {
        for (long i = threadIdx.x; i < M; i += blockDim.x) p_next[i] = z_next[i] + beta * p[i];
    }
    if (threadIdx.x == 0) scal[3] = beta;
}

// ------------------------------------------------------------------------------------
// The same two steps for a BLOCK of right-hand sides (the approximate NMLL's 26-column solve, xgp_regression.py:338-367;
// cg_tools.py:255-274 with k > 1): vectors are [M, k] row-major (column j of row i at i * k + j, as the block matvec
// takes and returns them).  Per column j: rz[j] carries r.z from step 1 to step 2; alpha_out[j], beta_out[j] and err_out[j]
// (device or pinned host memory) are this iteration's slots of the caller's [iterations, k] tables -- the solve keeps
// no per-iteration tensors and the host reads the errors one iteration behind.
// ------------------------------------------------------------------------------------
// Each step is two launches over row blocks (CGBLK_ROWS rows x all k <= 32 columns per workgroup: rows of [M, k] are
// contiguous, a wave reads 2 rows x 8 k bytes per load): the first forms per-block partial sums of the dot products, the
// second adds the partials in block order -- every workgroup for itself, a few KB from L2 -- and updates its rows.  No
// cross-workgroup hand-off inside a launch; fixed summation order.  (One workgroup per column, the first form, read one
// element per 8 k-byte row and took 67 + 35 us per iteration at M = 8192, k = 26; eight columns per workgroup 147 + 67:
// tools/block_tail_probe.py.)
constexpr int CGBLK_ROWS = 128;
constexpr int CGBLK_KMAX = 32;

// sums over this workgroup's rows of up to three per-element products, per column: part[blk][q][c]
__device__ __forceinline__ void cgblk_store_partials(const double (&s)[3], int nq, double *part_blk, int k, double (*red)[8][CGBLK_KMAX]) {
    const int c = threadIdx.x & 31, slot = threadIdx.x >> 5;
    for (int q = 0; q < nq; q++) red[q][slot][c] = s[q];
    __syncthreads();
    if (slot == 0 && c < k) {
        for (int q = 0; q < nq; q++) {
            double t = 0.0;
            for (int i = 0; i < 8; i++) t += red[q][i][c];
            part_blk[q * k + c] = t;
        }
    }
}

// every thread: the sum over blocks (in block order) of part[blk][q][c] for its column c
__device__ __forceinline__ double cgblk_sum_partials(const double *__restrict__ part, int nq, int q, int c, int k, long nblk) {
    double t[4] = {0.0, 0.0, 0.0, 0.0};
    long b = 0;
    for (; b + 3 < nblk; b += 4) {
        #pragma unroll
        for (int e = 0; e < 4; e++) t[e] += part[((b + e) * nq + q) * k + c];
    }
    double tail = 0.0;
    for (; b < nblk; b++) tail += part[(b * nq + q) * k + c];
    return ((t[0] + t[1]) + (t[2] + t[3])) + tail;
}

__global__ __launch_bounds__(256) void cg_step1a_block_kernel(double *w, const double *__restrict__ p, const double *__restrict__ r,
                                                              const double *__restrict__ z, double *part, double lam2, long M, int k) {
    __shared__ double red[3][8][CGBLK_KMAX];
    const int c = threadIdx.x & 31, slot = threadIdx.x >> 5;
    const long i0 = (long)blockIdx.x * CGBLK_ROWS;
    double s[3] = {0.0, 0.0, 0.0};
    constexpr int NR = CGBLK_ROWS / 8;
    double pv[NR], rv[NR], wv[NR], zv[NR];
    #pragma unroll
    for (int q = 0; q < NR; q++) {
        const long i = i0 + slot + 8 * q;
        const bool ok = i < M && c < k;
        const long e = ok ? i * k + c : 0;
        pv[q] = p[e]; rv[q] = r[e]; wv[q] = w[e]; zv[q] = z[e];
        if (!ok) { pv[q] = 0.0; rv[q] = 0.0; wv[q] = 0.0; zv[q] = 0.0; }
    }
    #pragma unroll
    for (int q = 0; q < NR; q++) {
        const long i = i0 + slot + 8 * q;
        const double wi = wv[q] + lam2 * pv[q];
        if (i < M && c < k) w[i * k + c] = wi;
        s[0] += rv[q] * zv[q];
        s[1] += pv[q] * wi;
        s[2] += rv[q] * rv[q];
    }
    cgblk_store_partials(s, 3, part + (long)blockIdx.x * 3 * k, k, red);
}

__global__ __launch_bounds__(256) void cg_step1b_block_kernel(const double *__restrict__ w, const double *__restrict__ p, double *x,
                                                              const double *__restrict__ r, double *r_next,
                                                              const double *__restrict__ part, double *rz_out, double *alpha_out,
                                                              double *err_out, const double *__restrict__ init_norm, long M, int k) {
    const int c = threadIdx.x & 31, slot = threadIdx.x >> 5;
    const long i0 = (long)blockIdx.x * CGBLK_ROWS;
    const long nblk = gridDim.x;
    const int cc = c < k ? c : 0;
    const double rz = cgblk_sum_partials(part, 3, 0, cc, k, nblk);
    const double pw = cgblk_sum_partials(part, 3, 1, cc, k, nblk);
    const double alpha = rz / pw;
    constexpr int NR = CGBLK_ROWS / 8;
    double pv[NR], rv[NR], wv[NR], xv[NR];
    #pragma unroll
    for (int q = 0; q < NR; q++) {
        const long i = i0 + slot + 8 * q;
        const long e = (i < M && c < k) ? i * k + c : 0;
        pv[q] = p[e]; rv[q] = r[e]; wv[q] = w[e]; xv[q] = x[e];
    }
    #pragma unroll
    for (int q = 0; q < NR; q++) {
        const long i = i0 + slot + 8 * q;
        if (i < M && c < k) {
            x[i * k + c] = xv[q] + alpha * pv[q];
            r_next[i * k + c] = rv[q] - alpha * wv[q];
        }
    }
    if (blockIdx.x == 0 && slot == 0 && c < k) {
        const double rr = cgblk_sum_partials(part, 3, 2, c, k, nblk);
        rz_out[c] = rz;
        alpha_out[c] = alpha;
        err_out[c] = sqrt(rr) / init_norm[c];
        __threadfence_system();
    }
}

__global__ __launch_bounds__(256) void cg_step2a_block_kernel(const double *__restrict__ r_next, const double *__restrict__ z_next,
                                                              double *part, long M, int k) {
    __shared__ double red[3][8][CGBLK_KMAX];
    const int c = threadIdx.x & 31, slot = threadIdx.x >> 5;
    const long i0 = (long)blockIdx.x * CGBLK_ROWS;
    double s[3] = {0.0, 0.0, 0.0};
    constexpr int NR = CGBLK_ROWS / 8;
    double rv[NR], zv[NR];
    #pragma unroll
    for (int q = 0; q < NR; q++) {
        const long i = i0 + slot + 8 * q;
        const bool ok = i < M && c < k;
        const long e = ok ? i * k + c : 0;
        rv[q] = r_next[e]; zv[q] = z_next[e];
        if (!ok) { rv[q] = 0.0; zv[q] = 0.0; }
    }
    #pragma unroll
    for (int q = 0; q < NR; q++) s[0] += rv[q] * zv[q];
    cgblk_store_partials(s, 1, part + (long)blockIdx.x * k, k, red);
}

__global__ __launch_bounds__(256) void cg_step2b_block_kernel(const double *__restrict__ z_next, const double *__restrict__ p,
                                                              double *p_next, const double *__restrict__ part,
                                                              const double *__restrict__ rz_in, double *beta_out, long M, int k) {
    const int c = threadIdx.x & 31, slot = threadIdx.x >> 5;
    const long i0 = (long)blockIdx.x * CGBLK_ROWS;
    const int cc = c < k ? c : 0;
    const double beta = cgblk_sum_partials(part, 1, 0, cc, k, gridDim.x) / rz_in[cc];
    constexpr int NR = CGBLK_ROWS / 8;
    double zv[NR], pv[NR];
    #pragma unroll
    for (int q = 0; q < NR; q++) {
        const long i = i0 + slot + 8 * q;
        const long e = (i < M && c < k) ? i * k + c : 0;
        zv[q] = z_next[e]; pv[q] = p[e];
    }
    #pragma unroll
    for (int q = 0; q < NR; q++) {
        const long i = i0 + slot + 8 * q;
        if (i < M && c < k) p_next[i * k + c] = zv[q] + beta * pv[q];
    }
    if (blockIdx.x == 0 && slot == 0 && c < k) beta_out[c] = beta;
}

// The two products of the block apply on the float64 matrix cores (v_mfma_f64_16x16x4_f64; operand maps as in zblock.inc:
// A lane l -> A[i = l & 15][kk = l >> 4], B lane l -> B[kk = l >> 4][j = l & 15], D register r -> D[(l >> 4) + 4 r][l & 15]).
//   utr:  part[rb][j, c] = sum over the rows of block rb of U[i, j] R[i, c]      a wave owns 16 columns j of U, CT x 16 columns c
//   uz:   Z[i, c] = R[i, c] + sum_j U[i, j] ((inv_eig[j] prefactor - 1) T[j, c])  a wave owns 16 rows i
// Out-of-range rows / columns are read clamped and meet a zero from the other operand or are not stored.
template <int CT>
__global__ __launch_bounds__(512) void precond_utr_mfma_kernel(const double *__restrict__ u, const double *__restrict__ r,
                                                               double *part, long M, long rank, int k, long rows_per) {
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long js = ((long)blockIdx.x * 8 + w) * 16;
    if (js >= rank) return;                                  // (wave-uniform; no barriers in this kernel)
    const long i0 = (long)blockIdx.y * rows_per;
    const long i1 = i0 + rows_per < M ? i0 + rows_per : M;
    const long jc = js + c < rank ? js + c : rank - 1;
    const bool jok = js + c < rank;
    double4_t acc[CT];
    #pragma unroll
    for (int ct = 0; ct < CT; ct++) acc[ct] = (double4_t){0.0, 0.0, 0.0, 0.0};
    constexpr int UNR = 8;                                   // row groups in flight
    for (long ib = i0; ib < i1; ib += 4 * UNR) {
        double a[UNR], b[UNR][CT];
        #pragma unroll
        for (int q = 0; q < UNR; q++) {
            const long row = ib + 4 * q + g;
            const bool rok = row < i1;
            const long rc = rok ? row : i1 - 1;
            a[q] = u[rc * rank + jc];
            if (!jok) a[q] = 0.0;
            #pragma unroll
            for (int ct = 0; ct < CT; ct++) {
                const int col = 16 * ct + c;
                const double v = r[rc * k + (col < k ? col : 0)];
                b[q][ct] = (rok && col < k) ? v : 0.0;
            }
        }
        #pragma unroll
        for (int q = 0; q < UNR; q++)
            #pragma unroll
            for (int ct = 0; ct < CT; ct++)
                acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q], b[q][ct], acc[ct], 0, 0, 0);
    }
    double *out = part + (long)blockIdx.y * rank * k;
    #pragma unroll
    for (int ct = 0; ct < CT; ct++)
        #pragma unroll
        for (int rr = 0; rr < 4; rr++) {
            const long j = js + g + 4 * rr;
            const int col = 16 * ct + c;
            if (j < rank && col < k) out[j * k + col] = acc[ct][rr];
        }
}

template <int CT>
__global__ __launch_bounds__(256) void precond_uz_mfma_kernel(const double *__restrict__ u, const double *__restrict__ t,
                                                              const double *__restrict__ inv_eig, double prefactor,
                                                              const double *__restrict__ r, double *z, long M, long rank, int k) {
    // the four waves of a workgroup share 16 rows and split the contraction over j (wave w takes the 16-column chunks
    // w, w + 4, ...): 4 x the waves of one-wave-per-row-tile (which left half the SIMDs empty and every load's latency
    // exposed: 97 us at M = 8192, rank = 512); their partial tiles meet in LDS and are added in wave order
    __shared__ double red[4][CT][4][64];
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long i0 = (long)blockIdx.x * 16;
    const long row = i0 + c < M ? i0 + c : M - 1;            // A row of this lane (clamped rows are never stored)
    const double *urow = u + row * rank;
    double4_t acc[CT];
    #pragma unroll
    for (int ct = 0; ct < CT; ct++) acc[ct] = (double4_t){0.0, 0.0, 0.0, 0.0};
    const bool vec = (rank & 3) == 0 && (reinterpret_cast<uintptr_t>(u) & 31) == 0;     // 16-byte loads of consecutive j
    for (long j0 = 16L * w; j0 < rank; j0 += 64) {
        // instruction e contracts over j in { j0 + 4 g + e : g = 0..3 }: lane (g, c) holds U[row c][j0 + 4 g + e]
        double a4[4];
        const long jb = j0 + 4 * g;
        if (vec && jb + 3 < rank) {
            const double2 p0 = *reinterpret_cast<const double2 *>(urow + jb), p1 = *reinterpret_cast<const double2 *>(urow + jb + 2);
            a4[0] = p0.x; a4[1] = p0.y; a4[2] = p1.x; a4[3] = p1.y;
        } else {
            #pragma unroll
            for (int e = 0; e < 4; e++) a4[e] = jb + e < rank ? urow[jb + e] : 0.0;
        }
        double b[4][CT];
        #pragma unroll
        for (int e = 0; e < 4; e++) {
            const long jj = jb + e;
            const long jq = jj < rank ? jj : rank - 1;
            const double cf = inv_eig[jq] * prefactor - 1.0;
            #pragma unroll
            for (int ct = 0; ct < CT; ct++) {
                const int col = 16 * ct + c;
                const double v = t[jq * k + (col < k ? col : 0)] * cf;
                b[e][ct] = (jj < rank && col < k) ? v : 0.0;
            }
        }
        #pragma unroll
        for (int e = 0; e < 4; e++)
            #pragma unroll
            for (int ct = 0; ct < CT; ct++)
                acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a4[e], b[e][ct], acc[ct], 0, 0, 0);
    }
    #pragma unroll
    for (int ct = 0; ct < CT; ct++)
        #pragma unroll
        for (int rr = 0; rr < 4; rr++) red[w][ct][rr][lane] = acc[ct][rr];
    __syncthreads();
    // wave w finishes D register w of every column tile: rows i0 + g + 4 w
    const long i = i0 + g + 4 * w;
    #pragma unroll
    for (int ct = 0; ct < CT; ct++) {
        const int col = 16 * ct + c;
        const double s = ((red[0][ct][w][lane] + red[1][ct][w][lane]) + red[2][ct][w][lane]) + red[3][ct][w][lane];
        if (i < M && col < k) z[i * k + col] = r[i * k + col] + s;
    }
}

// ------------------------------------------------------------------------------------
// Preconditioner apply for one right-hand side (rand_nys_preconditioners.py:66-72):
//   z = U (inv_eig * prefactor .* U^T r) + (r - U U^T r) = r + U ((inv_eig * prefactor - 1) .* (U^T r)),
// U [M, rank] float64 row-major.  Two HBM/MALL-bound passes over U (33.5 MB at M = 8192, rank = 512):
// (1) per-row-block partial column sums, (2) slab reduce (shared with the matvec), (3) one wave
// per row: z_i = r_i + U_i . s.  The library GEMV these replace ran at 0.24 ms per product.
// ------------------------------------------------------------------------------------
constexpr int PRE_BLOCKS = 512;      // M = 8192: 16 rows per workgroup (two batches of loads in flight per thread); more blocks only move the time into the slab reduction

__global__ __launch_bounds__(256) void precond_utr_kernel(const double *__restrict__ u, const double *__restrict__ r,
                                                          double *part, long M, long rank) {
    const long rows_per = (M + gridDim.x - 1) / gridDim.x;
    const long i0 = (long)blockIdx.x * rows_per;
    const long i1 = i0 + rows_per < M ? i0 + rows_per : M;
    if ((rank & 1) == 0 && (reinterpret_cast<uintptr_t>(u) & 15) == 0) {
        // two adjacent columns per thread (16-byte loads: u 16-byte aligned, as every row is then; part is, the launcher
        // checks the workspace); rows in order, so the sums do not depend on the path
        for (long j = 2 * threadIdx.x; j < rank; j += 2 * blockDim.x) {
            double a0 = 0.0, a1 = 0.0;
            #pragma unroll 8
            for (long i = i0; i < i1; i++) {
                const double2 uv = *reinterpret_cast<const double2 *>(u + i * rank + j);
                const double ri = r[i];
                a0 = __builtin_fma(uv.x, ri, a0);
                a1 = __builtin_fma(uv.y, ri, a1);
            }
            *reinterpret_cast<double2 *>(part + (long)blockIdx.x * rank + j) = make_double2(a0, a1);
        }
        return;
    }
    for (long j = threadIdx.x; j < rank; j += blockDim.x) {
        double acc = 0.0;
        #pragma unroll 8
        for (long i = i0; i < i1; i++) acc = __builtin_fma(u[i * rank + j], r[i], acc);
        part[(long)blockIdx.x * rank + j] = acc;
    }
}

__global__ __launch_bounds__(256) void precond_uz_kernel(const double *__restrict__ u, const double *__restrict__ t,
                                                         const double *__restrict__ inv_eig, double prefactor,
                                                         const double *__restrict__ r, double *z, long M, long rank) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const double *ur = u + row * rank;
    double acc = 0.0;
    for (long j = lane; j < rank; j += 64) acc = __builtin_fma(ur[j], (inv_eig[j] * prefactor - 1.0) * t[j], acc);
    acc = wave_sum(acc);
    if (lane == 0) z[row] = r[row] + acc;
}

// ------------------------------------------------------------------------------------
// The classifier's cost function between its two contractions (nonlinear_cg_toolkit.py:243-262): per datapoint row of
// pred [n, ncls] -- subtract the row maximum, 2.71828 ** (.) (the reference's constant, not e), normalise; the loss
// takes -log(max(p[label], 1e-16)); the label's entry loses 1 (pred becomes the residual the back-projection
// contracts).  One thread per row, the row (8 ncls bytes) read three times through L1; per-workgroup loss partials in
// thread order, added by the caller.  Replaces ten elementwise launches over [n, ncls] and their temporaries.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void softmax_residual_kernel(double *pred, const long *__restrict__ labels, long n, int ncls,
                                                               double *loss_part) {
    __shared__ double red[16];
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    double mine = 0.0;
    if (i < n) {
        double *row = pred + i * ncls;
        double mx = row[0];
        for (int c = 1; c < ncls; c++) mx = row[c] > mx ? row[c] : mx;
        double sum = 0.0;
        for (int c = 0; c < ncls; c++) { const double e = pow(2.71828, row[c] - mx); row[c] = e; sum += e; }
        const long lab = labels[i];
        for (int c = 0; c < ncls; c++) {
            const double pr = row[c] / sum;
            if (c == lab) mine = -log(pr < 1e-16 ? 1e-16 : pr);
            row[c] = c == lab ? pr - 1.0 : pr;
        }
        // a label outside [0, ncls) matches no class: the row would silently add nothing to the loss and lose no 1 (the
        // gather / scatter the reference's chain uses fails on such an index) -- make it visible instead
        if (lab < 0 || lab >= ncls) mine = __builtin_nan("");
    }
    const double t = block_sum(mine, red);
    if (threadIdx.x == 0) loss_part[blockIdx.x] = t;
}

// ---- self test of the cross-lane stages: v[r] = lane + 64 r, one stage of stride H,
// registers 0 and 1 written out.  Expected: bit H of lane clear -> 2 lane + H + 128 r, set -> -H.
__global__ void selftest_kernel(int32_t *out) {
    const int lane = threadIdx.x & 63;
    float v[16];
    #pragma unroll
    for (int q = 0; q < 6; q++) {
        #pragma unroll
        for (int r = 0; r < 16; r++) v[r] = (float)(lane + 64 * r);
        if (q == 0) xstage<1>(v, lane);
        else if (q == 1) xstage<2>(v, lane);
        else if (q == 2) xstage<4>(v, lane);
        else if (q == 3) xstage<8>(v, lane);
        else if (q == 4) xstage<16>(v, lane);
        else xstage<32>(v, lane);
        #pragma unroll
        for (int r = 0; r < 16; r++) out[(q * 16 + r) * 64 + lane] = (int32_t)v[r];
    }
}

