// launchers.inc -- part of xgpr_hip.hip (included inside its anonymous namespace, in order): launch helpers, validation, typed implementations behind the C entry points.
// ------------------------------------------------------------------------------------
// launch helpers
// ------------------------------------------------------------------------------------
constexpr long LDS_CAP_BYTES = 128 * 1024;   // per-workgroup LDS the generic path will ask for

template <typename T> long lds_cap_elems() { return LDS_CAP_BYTES / (long)sizeof(T); }

template <typename K> int allow_big_lds(K kernel, size_t bytes) {
    if (bytes > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return hip_fail(e, "hipFuncSetAttribute(MaxDynamicSharedMemorySize)");
    }
    return 0;
}

// One launch: the dynamic-LDS attribute where the kernel needs more than 64 KiB, the launch, the launch error under `what`.
template <typename K, typename... Args>
int launch(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t st, const char *what, Args... args) {
    int rc = allow_big_lds(kernel, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
    HIP_TRY(hipGetLastError(), what);
    return 0;
}

// A runtime flag as a template argument: f(std::true_type{}) or f(std::false_type{}).
template <class F> int dispatch_bool(bool flag, F &&f) { return flag ? f(std::true_type{}) : f(std::false_type{}); }

// The padded width as a template argument: f(std::integral_constant<int, LG>{}) for LO <= lg <= HI, `too_wide` otherwise.  The
// bounds of a call site ARE the set of widths its kernel is instantiated for.
template <int LO, int HI, class F> int dispatch_lg(int lg, const char *too_wide, F &&f) {
    if constexpr (LO > HI) {
        return fail(XGPR_ERR_UNSUPPORTED, too_wide);
    } else {
        if (lg == LO) return f(std::integral_constant<int, LO>{});
        return dispatch_lg<LO + 1, HI>(lg, too_wide, f);
    }
}
constexpr const char *TOO_WIDE_WAVE = "padded width > 1024 on this wave-tile kernel";
constexpr const char *TOO_WIDE_Z3 = "padded width > 4096 on the wave path";      // the three-wave kernel (fused_ztz.inc) also serves 2048 and 4096 (round 6)
constexpr const char *TOO_WIDE_WT = "padded width > 8192 on the wave-tile path"; // the wave-tile kernels in the input type (wave_tile.inc)
constexpr int NO_ARM = 1;   // from a dispatch_lg callback: no instantiation for these arguments at this width, the caller goes on to its next plan

int threads_for(long P) { return P >= 4096 ? 1024 : (P >= 512 ? 256 : 64); }

template <typename T, bool SRHT>
int launch_fht(T *x, const int8_t *radem, long nvec, long P, hipStream_t st) {
    const long total = nvec * P;
    const long cap = lds_cap_elems<T>();
    long CH;
    if (P <= cap) {
        CH = P >= 1024 ? P : 1024;   // several short vectors per workgroup
    } else {
        CH = cap;
    }
    const long nblocks = (total + CH - 1) / CH;
    const T nc = SRHT ? norm_constant<T>(P) : (T)1;
    int rc = launch(generic_fht_kernel<T, SRHT>, dim3((unsigned)nblocks), dim3(threads_for(CH)), (size_t)CH * sizeof(T), st,
                    "generic_fht_kernel launch", x, radem, total, (int)P, (int)CH, nc);
    if (rc) return rc;
    for (long h = CH; h < P; h <<= 1) {
        const long npairs = total / 2;
        rc = launch(global_stage_kernel<T>, dim3((unsigned)((npairs + 255) / 256)), dim3(256), 0, st, "global_stage_kernel launch", x, npairs, h);
        if (rc) return rc;
    }
    return 0;
}

constexpr long GENERIC_SCRATCH_SLOTS = 256;

// bytes of global scratch the generic path needs for padded width P (0 when it fits in LDS)
size_t generic_scratch_bytes(long P, size_t elem) {
    return (size_t)P * elem > (size_t)LDS_CAP_BYTES ? (size_t)GENERIC_SCRATCH_SLOTS * P * elem : 0;
}

template <typename T, int MODE>
int launch_generic_sorf(SorfArgs<T> a, void *workspace, size_t wbytes, hipStream_t st) {
    long items = a.n * a.reps;
    if ((long)a.P > lds_cap_elems<T>()) {
        const size_t need = generic_scratch_bytes(a.P, sizeof(T));
        if (!workspace || wbytes < need || !aligned16(workspace))
            return fail(XGPR_ERR_WORKSPACE, "workspace too small (see xgpr_sorf_workspace_bytes)");
        a.scratch = reinterpret_cast<T *>(workspace);
        const long nblocks = items < GENERIC_SCRATCH_SLOTS ? items : GENERIC_SCRATCH_SLOTS;
        return launch(generic_sorf_kernel<T, MODE, true>, dim3((unsigned)nblocks), dim3(1024), 0, st, "generic_sorf_kernel launch", a);
    }
    const long nblocks = items < (1L << 20) ? items : (1L << 20);
    return launch(generic_sorf_kernel<T, MODE, false>, dim3((unsigned)nblocks), dim3(threads_for(a.P)), (size_t)a.P * sizeof(T), st,
                  "generic_sorf_kernel launch", a);
}

int pack_masks(const int8_t *radem, uint64_t *masks, long R, int MW, hipStream_t st) {
    const long items = 3L * MW;
    return launch(pack_radem_kernel, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, st, "pack_radem_kernel launch", radem, masks, R, MW);
}

int masks_per_diag(long R) { return (int)(align_up((size_t)R, 1024) / 64); }
size_t masks_bytes(long R) { return align_up((size_t)3 * masks_per_diag(R) * sizeof(uint64_t), 256); }

// `items` wave tiles, `waves` of them per workgroup (the independent-wave kernels: 4 waves; wave_tile.inc: WaveTile<T, LG>::WAVES)
template <typename K, typename A> int launch_wave_tile(K kernel, const A &a, long items, int waves, size_t lds, hipStream_t st, const char *what) {
    const long nblocks = (items + waves - 1) / waves;
    if (nblocks > 2147483647L) return fail(XGPR_ERR_UNSUPPORTED, "too many datapoints for one launch");
    return launch(kernel, dim3((unsigned)nblocks), dim3((unsigned)(waves * 64)), lds, st, what, a);
}

// the ordered sum of the partial-result slabs every slab-writing kernel ends with
int reduce_slabs(const double *wpart, double *w_out, long num_rffs, long nslabs, hipStream_t st) {
    return launch(reduce_slabs_kernel, dim3((unsigned)((num_rffs + 63) / 64)), dim3(256), 0, st, "reduce_slabs_kernel launch", wpart, w_out,
                  num_rffs, nslabs);
}

void fill_norms(WaveArgs &a, int lg) {
    const float nc = norm_constant<float>(1L << lg);
    if (lg & 1) { a.nc = nc; a.chi_scale = 1.0f; }
    else { a.nc = 1.0f; a.chi_scale = nc * nc * nc; }   // exact power of two
}

// The fields every launch of the wave kernels shares (one wave = 1024 frequencies of a datapoint; `workspace` holds the packed sign
// masks at its head: pack_masks stays the caller's own call).  The caller adds what is its own: outputs, grad, sigma, scale, seqlen,
// the window fields of the sequence kernels.
WaveArgs wave_args(const float *x, const float *chi, const void *workspace, long n, long row_stride, long d, long num_freqs, long R) {
    WaveArgs a = {};
    a.x = x; a.masks = (const uint64_t *)workspace; a.chi = chi;
    a.n = n; a.row_stride = row_stride; a.F = num_freqs; a.d = (int)d;
    a.MW = masks_per_diag(R); a.nb = (int)((num_freqs + 1023) / 1024);
    fill_norms(a, ilog2(padded_width(d)));
    return a;
}

// ... and of the kernels that read the Rademacher array itself (the any-width path, wave_tile.inc): P, reps, nc as well
template <typename T>
SorfArgs<T> sorf_args(const T *x, const int8_t *radem, const T *chi, long n, long row_stride, long d, long num_freqs, long R) {
    const long P = padded_width(d);
    SorfArgs<T> a = {};
    a.x = x; a.radem = radem; a.chi = chi;
    a.n = n; a.row_stride = row_stride; a.F = num_freqs; a.R = R; a.d = (int)d;
    a.P = (int)P; a.reps = (int)((num_freqs + P - 1) / P); a.nc = norm_constant<T>(P);
    return a;
}

// ------------------------------------------------------------------------------------
// validation shared by the entry points (mirrors the reference's throw sites)
// ------------------------------------------------------------------------------------
int check_seqlens(const int32_t *seqlen_host, long nseq, long n, long L, int conv_width) {
    if (nseq != n) return fail(XGPR_ERR_SEQLEN_SIZE, "wrong array sizes");
    if (L < conv_width || conv_width <= 0) return fail(XGPR_ERR_CONV_WIDTH, "invalid conv_width");
    if (!seqlen_host) return fail(XGPR_ERR_SEQLEN_RANGE, "seqlen_host is required (sequence lengths are validated on the host)");
    int32_t mn = 2147483647, mx = 0;
    for (long i = 0; i < nseq; i++) {
        if (seqlen_host[i] > mx) mx = seqlen_host[i];
        if (seqlen_host[i] < mn) mn = seqlen_host[i];
    }
    if (mx > L || mn < conv_width)
        return fail(XGPR_ERR_SEQLEN_RANGE, "All sequence lengths must be >= conv width and < array size.");
    return 0;
}

// The shape checks every SORF entry point shares, in the reference's order (rbf_ops.cpp:49-62): the first failing one is reported.
// `between`: the entry point's own checks that the reference makes after the frequency check and before the padded-width one (array
// sizes of the gradient, sequence count, conv_width).  rffs_per_freq: 2 (cos, sin); 1 for max-pool.
template <class Between>
int check_sorf_shape(long n, long num_rffs, long num_freqs, long R, long P, int rffs_per_freq, Between &&between) {
    if (n == 0) return fail(XGPR_ERR_NO_DATAPOINTS, "no datapoints");
    if (num_rffs < 2 || (num_rffs & 1) != 0) return fail(XGPR_ERR_ODD_OUTPUT, "last dim of output must be even number");
    if (rffs_per_freq * num_freqs != num_rffs || num_freqs > R) return fail(XGPR_ERR_RFFS_FREQS, "incorrect number of rffs and or freqs.");
    if (int rc = between()) return rc;
    if (R % P != 0) return fail(XGPR_ERR_RFFS_FREQS, "incorrect number of rffs and or freqs.");
    return 0;
}
int check_sorf_shape(long n, long num_rffs, long num_freqs, long R, long P) {
    return check_sorf_shape(n, num_rffs, num_freqs, R, P, 2, [] { return 0; });
}

// rbf_ops.cpp:64-69: the constant is rounded to T there; rbf_ops.cpp:180-185: a double constant in the gradient op (T = double: the
// cast is the identity)
template <typename T> double rbf_scale(long num_freqs, int fit_intercept) {
    T s = fit_intercept ? (T)sqrt(1.0 / ((double)num_freqs - 0.5)) : (T)sqrt(1.0 / (double)num_freqs);
    return (double)s;
}

// ------------------------------------------------------------------------------------
// typed implementations behind the C entry points
// ------------------------------------------------------------------------------------
template <typename T>
int fht_impl(T *x, long n, long dim1, long dim2, void *stream) {
    if (n == 0) return fail(XGPR_ERR_NO_DATAPOINTS, "no datapoints");
    if (dim2 < 2) return fail(XGPR_ERR_NOT_POW2, "last dim not power of 2 > 1");
    if ((dim2 & (dim2 - 1)) != 0) return fail(XGPR_ERR_NOT_POW2, "last dim not power of 2");
    if (dim1 < 1) return fail(XGPR_ERR_ARRAY_DIMS, "incorrect array dims passed");
    return launch_fht<T, false>(x, nullptr, n * dim1, dim2, (hipStream_t)stream);
}

template <typename T>
int srht_impl(T *x, const int8_t *radem, long n, long dim, long radem_len, void *stream) {
    if (n == 0) return fail(XGPR_ERR_NO_DATAPOINTS, "no datapoints");
    if (dim != radem_len) return fail(XGPR_ERR_ARRAY_DIMS, "incorrect array dims passed");
    if (dim < 2) return fail(XGPR_ERR_NOT_POW2, "last dim not power of 2 > 1");
    if ((dim & (dim - 1)) != 0) return fail(XGPR_ERR_NOT_POW2, "last dim not power of 2");
    return launch_fht<T, true>(x, radem, n, dim, (hipStream_t)stream);
}

// The feature rows on the three-wave persistent plan (fused_ztz.inc, Z3_FEAT64 / Z3_FEAT32): returns 1 when launched, 0
// when the shape is outside that kernel or the plan is not the faster one (the caller then runs wave_rbf_kernel), < 0
// on error.  Measured per 131072 rows (round 4, gpurun_out/r4/feat_ab.log): the float32 cache rows 0.93 ms against 1.00
// at cfg3's shape and 0.436 against 0.46 at cfg2's -- taken; the float64 operator 1.72 against 1.62-1.68 (0.81 / 0.83 at
// cfg2's shape): both plans sit at the same ~5.3-5.6 TB/s of write stream whatever the arithmetic in front of it, so the
// operator keeps wave_rbf_kernel.  XGPR_FEAT_PLAN=wave / =z3 in the environment force one plan for both (A/B timing).
// one launch of the three-wave kernel (fused_ztz.inc) in mode MODE at padded width 2^LG; a.dma1 picks the row fetch
template <int LG, int MODE>
int launch_ztz3(const WaveArgs &a, long ncols, int ngroups, size_t lds, hipStream_t st, const char *what) {
    constexpr bool feat = MODE == Z3_FEAT64 || MODE == Z3_FEAT32;
    return dispatch_bool(a.dma1 != 0, [&](auto DMA1) {
        return launch(ztz3_kernel<LG, MODE, decltype(DMA1)::value>, dim3((unsigned)ncols, (unsigned)ngroups), dim3(z3_waves(LG, feat) * 64),
                      lds, st, what, a);
    });
}

template <int MODE>
int launch_ztz3_feat(WaveArgs a, long P, int lg, hipStream_t st) {
    static const int forced = [] { const char *e = getenv("XGPR_FEAT_PLAN"); return !e ? 0 : e[0] == 'w' ? 1 : e[0] == 'z' ? 2 : 0; }();
    const bool wide = P > 1024;                            // (no other wave-tile plan there: both feature modes run here)
    const int nbt = wide ? ztz3_compute_tiles(P, a.F) : a.nb;
    if (!wide && (forced == 1 || (forced == 0 && MODE == Z3_FEAT64))) return 0;
    if (nbt < 2 || P < 32 || P > 4096) return 0;          // (P <= 16: the rows-only tile would store 8-byte pieces 128 bytes apart)
    a.dma1 = ztz3_dma1(a.x, a.d);
    int nbg = wide ? ((nbt <= 4) ? nbt : ztz3_group_tiles(nbt, P))
                   : (nbt <= 6 && Z3_WAVES % nbt == 0 && ztz3_slots(nbt, P, true) * nbt >= 10) ? nbt : ztz3_group_tiles(nbt, P);
    if (ztz3_lds_bytes(nbg, P, true) > 160 * 1024) nbg = 4;
    if (ztz3_lds_bytes(nbg, P, true) > 160 * 1024) return 0;
    const int ngroups = (nbt + nbg - 1) / nbg;
    a.nb = nbg; a.G = ztz3_slots(nbg, P, true);
    long ncols = device_cus() / ngroups > 0 ? device_cus() / ngroups : 1;
    const long by_rows = (a.n + a.G - 1) / a.G;
    if (ncols > by_rows) ncols = by_rows;
    const size_t lds3 = ztz3_lds_bytes(nbg, P, true);
    const int rc = dispatch_lg<5, 12>(lg, TOO_WIDE_Z3, [&](auto LG) {
        return launch_ztz3<decltype(LG)::value, MODE>(a, ncols, ngroups, lds3, st, "ztz3_kernel (feature rows) launch");
    });
    return rc ? rc : 1;
}

// XGPR_F64_PLAN=generic in the environment: the shapes of wave_tile.inc run on the any-width path instead (A/B timing)
bool wave_tile_plan_off() {
    static const bool off = [] { const char *e = getenv("XGPR_F64_PLAN"); return e && e[0] == 'g'; }();
    return off;
}

template <typename T>
int rbf_impl(const T *x, double *out, double *grad, const int8_t *radem, const T *chi, long n, long d,
             long out_rows, long num_rffs, long grad_rows, long grad_cols, long num_freqs, long R,
             double sigma, int fit_intercept, bool want_grad, void *workspace, size_t wbytes, void *stream) {
    const long P = padded_width(d);
    if (out_rows != n) return fail(XGPR_ERR_NO_DATAPOINTS, "no datapoints");
    int rc = check_sorf_shape(n, num_rffs, num_freqs, R, P, 2, [&] {
        return want_grad && (grad_rows != out_rows || grad_cols != num_rffs) ? fail(XGPR_ERR_ARRAY_SIZES, "Wrong array sizes.") : 0;
    });
    if (rc) return rc;
    if (!aligned16(out)) return fail(XGPR_ERR_WORKSPACE, "output pointer must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int lg = ilog2(P);

    if constexpr (sizeof(T) == 4) {
        // one wave per tile of 1024 frequencies: wave_rbf_kernel up to P = 1024 (there a missing workspace is an error); at 2048 / 4096
        // the feature operator on the three-wave kernel's wide transforms (fused_ztz.inc, Z3_FEAT64), taken only with a workspace that
        // holds the masks -- without one, and for the gradient, the plans further down serve these widths
        const bool have_masks = workspace && wbytes >= masks_bytes(R);
        if (P <= 1024 && !have_masks) return fail(XGPR_ERR_WORKSPACE, "workspace too small (see xgpr_rbf_workspace_bytes)");
        if (P <= 1024 || (P <= 4096 && !want_grad && have_masks)) {
            WaveArgs a = wave_args(x, chi, workspace, n, d, d, num_freqs, R);
            a.out = out;
            a.scale = rbf_scale<float>(num_freqs, fit_intercept);
            if (want_grad) {
                if (!aligned16(grad)) return fail(XGPR_ERR_WORKSPACE, "gradient pointer must be 16-byte aligned");
                a.grad = grad; a.sigma = sigma;
                a.scale = rbf_scale<double>(num_freqs, fit_intercept);
            }
            rc = pack_masks(radem, (uint64_t *)workspace, R, a.MW, st);
            if (rc) return rc;
            const long nblocks = (n * a.nb + 3) / 4;
            if (P <= 1024 && nblocks > 2147483647L) return fail(XGPR_ERR_UNSUPPORTED, "too many datapoints for one launch");
            if (!want_grad) {
                const int rcf = launch_ztz3_feat<Z3_FEAT64>(a, P, lg, st);
                if (rcf != 0) return rcf < 0 ? rcf : 0;
            }
            if (P <= 1024)
                return dispatch_lg<1, 10>(lg, TOO_WIDE_WAVE, [&](auto LG) {
                    return dispatch_bool(want_grad, [&](auto GRAD) {
                        return launch(wave_rbf_kernel<decltype(LG)::value, decltype(GRAD)::value ? OUT_GRAD : OUT_F64>, dim3((unsigned)nblocks),
                                      dim3(256), 0, st, "wave_rbf_kernel launch", a);
                    });
                });
        }
    }
    SorfArgs<T> a = sorf_args(x, radem, chi, n, d, d, num_freqs, R);
    a.out = out; a.grad = grad; a.sigma = sigma;
    a.scale = want_grad ? rbf_scale<double>(num_freqs, fit_intercept) : rbf_scale<T>(num_freqs, fit_intercept);
    {
        // wave tiles in registers + an LDS image (wave_tile.inc): the float64 feature and gradient operators at P <= 8192, the float32
        // gradient operator at 2048 <= P <= 8192 and the float32 feature operator at P = 8192 (narrower ones are served above);
        // XGPR_F64_PLAN=generic keeps the any-width path (A/B)
        const bool generic64 = wave_tile_plan_off();
        const bool mine = sizeof(T) == 8 ? P <= 8192 : (((want_grad && P > 1024) || P > 4096) && P <= 8192);
        if (mine && !generic64 && R % 64 == 0 && (reinterpret_cast<uintptr_t>(radem) & 15) == 0) {
            // the gradient mode stores pairs 16 bytes at a time to grad as well as to out (checked above): a grad view that is only
            // 8-byte aligned gets two 8-byte stores per pair from the same kernel -- the any-width path evaluates cos / sin with the
            // library's routine, so sending the view there would make the last bit of the result depend on the pointer
            a.grad_split = want_grad && !aligned16(grad);
            const long items = n * (P > 1024 ? R / 1024 : (num_freqs + 1023) / 1024);
            rc = dispatch_lg<1, 13>(lg, TOO_WIDE_WT, [&](auto LGc) {
                constexpr int LG = decltype(LGc)::value;
                if constexpr (sizeof(T) == 8 || LG > 10) {
                    using WT = WaveTile<T, LG>;
                    if (want_grad)
                        return launch_wave_tile(wave_tile_rbf_kernel<T, LG, true>, a, items, WT::WAVES, WT::LDS_BYTES, st, "wave_tile_rbf_kernel launch");
                    if constexpr (sizeof(T) == 8 || LG > 12)
                        return launch_wave_tile(wave_tile_rbf_kernel<T, LG, false>, a, items, WT::WAVES, WT::LDS_BYTES, st, "wave_tile_rbf_kernel launch");
                }
                return NO_ARM;
            });
            if (rc != NO_ARM) return rc;
        }
    }
    if (want_grad) return launch_generic_sorf<T, MODE_RBF_GRAD>(a, workspace, wbytes, st);
    return launch_generic_sorf<T, MODE_RBF>(a, workspace, wbytes, st);
}

// ---- float32 feature rows of the sequence kernels (xgpr_conv_feature_rows_f32, mode MODE_CONV_ROWS of conv_impl): outf = zc[n, num_rffs].
// Windows up to 1024 elements: wave_conv_kernel<LG, CONV_ROWS>; 2048 / 4096: wave_tile_conv_kernel<float, LG, MODE_CONV_ROWS>; every other
// shape (wider windows, or a Rademacher array the wave tiles cannot read 16 bytes at a time): the float64 operator itself, slice by
// slice into a float64 staging area behind the operator's own workspace, then one rounding pass -- the any-width kernel keeps its sums
// in the float64 output between k-mers, so a float32 store there would need a second accumulator scheme for one rarely used path.
size_t conv_rows_stage_offset(long R, long P, long nseq) {
    const size_t a = masks_bytes(R), b = generic_scratch_bytes(P, sizeof(float));
    return align_up((a > b ? a : b) + align_up((size_t)(nseq > 0 ? nseq : 0) * sizeof(int32_t), 256), 256);
}
constexpr size_t CONV_ROWS_STAGE_BYTES = (size_t)256 << 20;      // float64 staging of the any-width windows: at most this much is asked for

// (2048 / 4096 too: the staged route serves them when radem is not 16-byte aligned.)  narrays: 1 for the feature rows; 2 for the feature
// AND gradient rows (xgpr_conv_grad_rows_f32, mode MODE_CONV_GRAD_ROWS of conv_impl: outf = zrows[n, num_rffs], gradf = grows[n, num_rffs]
// -- the dispatch of the feature rows with the gradient operator's kernels: windows up to 1024 elements wave_conv_kernel<LG,
// CONV_GRAD_ROWS>, 2048 / 4096 wave_tile_conv_kernel<float, LG, MODE_CONV_GRAD_ROWS>, every other shape the float64 gradient operator
// slice by slice into TWO float64 staging arrays (out, grad) -- together within CONV_ROWS_STAGE_BYTES -- and one rounding pass each).
size_t conv_rows_workspace_bytes(long R, long width, long num_rffs, long nseq, int narrays) {
    const long P = padded_width(width);
    size_t b = conv_rows_stage_offset(R, P, nseq);
    if (P > 1024 && nseq > 0 && num_rffs > 0) {
        const size_t row = (size_t)num_rffs * sizeof(double), per_array = CONV_ROWS_STAGE_BYTES / narrays;
        size_t rows = per_array / row > 0 ? per_array / row : 1;
        if (rows > (size_t)nseq) rows = (size_t)nseq;
        b += narrays * align_up(rows * row, 256);
    }
    return b;
}

__global__ __launch_bounds__(256) void round_rows_kernel(const double2 *__restrict__ src, float2 *__restrict__ dst, long npairs,
                                                         long pairs_per_row, int fit_intercept) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= npairs) return;
    const double2 v = src[idx];
    const float c = (fit_intercept && idx % pairs_per_row == 0) ? 1.0f : (float)v.x;
    dst[idx] = make_float2(c, (float)v.y);
}

// the staged route of both row modes: zrows, and grows as well when it is not NULL
int conv_rows_staged(const float *x, float *zrows, float *grows, const int8_t *radem, const float *chi, const int32_t *seqlen_host,
                     const int32_t *seqlen_dev, long n, long L, long C, long num_rffs, long num_freqs, long R, double sigma,
                     int conv_width, int scaling_type, int fit_intercept, void *workspace, size_t wbytes, hipStream_t st);

// the sequence kernels' mode as wave_conv_kernel's template argument: f(std::integral_constant<int, CONV_*>{})
template <class F> int dispatch_conv_mode(int mode, F &&f) {
    switch (mode) {
        case MODE_CONV_GRAD: return f(std::integral_constant<int, CONV_GRAD>{});
        case MODE_CONV_GRAD_ROWS: return f(std::integral_constant<int, CONV_GRAD_ROWS>{});
        case MODE_CONV_ROWS: return f(std::integral_constant<int, CONV_ROWS>{});
        case MODE_MAXPOOL: return f(std::integral_constant<int, CONV_MAXPOOL>{});
        default: return f(std::integral_constant<int, CONV_FGEN>{});
    }
}

// One launch of the sequence kernels on wave tiles (windows of up to 1024 elements), dense or token input: the sign masks, the
// longest-first order when the caller's workspace has room for it (xgpr_conv_workspace_bytes) and there is more than one round of
// waves to balance, then the kernel through `launch_kernel(args, nblocks)`.
template <class F>
int launch_wave_conv(WaveArgs a, const int8_t *radem, long R, long L, void *workspace, size_t wbytes, hipStream_t st, F &&launch_kernel) {
    const long n = a.n;
    int rc = pack_masks(radem, (uint64_t *)workspace, R, a.MW, st);
    if (rc) return rc;
    const long nblocks = (n * a.nb + 3) / 4;
    if (nblocks > 2147483647L) return fail(XGPR_ERR_UNSUPPORTED, "too many datapoints for one launch");
    const size_t order_off = masks_bytes(R);
    if (n >= 64 && n <= 2147483647L && L <= 12000 && wbytes >= order_off + (size_t)n * sizeof(int32_t)) {
        int32_t *order = reinterpret_cast<int32_t *>(reinterpret_cast<unsigned char *>(workspace) + order_off);
        rc = launch(conv_order_kernel, dim3(1), dim3(1024), (size_t)(L + 1) * sizeof(int), st, "conv_order_kernel launch", a.seqlen,
                    order, n, (int)L);
        if (rc) return rc;
        a.order = order;
    }
    return launch_kernel(a, nblocks);
}

template <typename T>
int conv_impl(const T *x, double *out, double *grad, float *outf, const int8_t *radem, const T *chi,
              const int32_t *seqlen_host, const int32_t *seqlen_dev, long n, long L, long C, long out_rows,
              long num_rffs, long grad_rows, long grad_cols, long num_freqs, long R, long nseq, double sigma,
              int conv_width, int scaling_type, int mode, void *workspace, size_t wbytes, void *stream, int fit_intercept = 0,
              float *gradf = nullptr) {
    const bool rows_mode = mode == MODE_CONV_ROWS || mode == MODE_CONV_GRAD_ROWS;      // float32 rows out: no float64 output to check
    const bool grad_mode = mode == MODE_CONV_GRAD || mode == MODE_CONV_GRAD_ROWS;
    if (rows_mode && sizeof(T) != 4) return fail(XGPR_ERR_UNSUPPORTED, "float32 feature rows take float32 input");
    if (out_rows != n) return fail(XGPR_ERR_NO_DATAPOINTS, "no datapoints");
    const long win = (long)conv_width * C;
    const long P = padded_width(win);
    const int reps = (int)((num_freqs + P - 1) / P);
    int rc = check_sorf_shape(n, num_rffs, num_freqs, R, P, mode == MODE_MAXPOOL ? 1 : 2, [&] {
        if (mode == MODE_CONV_GRAD && (grad_rows != out_rows || grad_cols != num_rffs))
            return fail(XGPR_ERR_ARRAY_SIZES, "Wrong array sizes.");
        if (nseq != n) return fail(XGPR_ERR_SEQLEN_SIZE, "wrong array sizes");
        if (L < conv_width || conv_width <= 0) return fail(XGPR_ERR_CONV_WIDTH, "invalid conv_width");
        return 0;
    });
    if (rc) return rc;
    if (mode == MODE_MAXPOOL && R != (long)reps * P) return fail(XGPR_ERR_RFFS_FREQS, "incorrect number of rffs and or freqs.");
    rc = check_seqlens(seqlen_host, nseq, n, L, conv_width);
    if (rc) return rc;
    if (!seqlen_dev) return fail(XGPR_ERR_WORKSPACE, "seqlen_dev (device copy of the sequence lengths) is required");
    hipStream_t st = (hipStream_t)stream;
    if (rows_mode && (!outf || (reinterpret_cast<uintptr_t>(outf) & 7) != 0))
        return fail(XGPR_ERR_WORKSPACE, "feature rows pointer must be 8-byte aligned");
    if (mode == MODE_CONV_GRAD_ROWS && (!gradf || (reinterpret_cast<uintptr_t>(gradf) & 7) != 0))
        return fail(XGPR_ERR_WORKSPACE, "gradient rows pointer must be 8-byte aligned");
    const int lg = ilog2(P);

    if constexpr (sizeof(T) == 4) {
        if (P <= 1024) {
            if (mode != MODE_MAXPOOL && !rows_mode && !aligned16(out)) return fail(XGPR_ERR_WORKSPACE, "output pointer must be 16-byte aligned");
            if (mode == MODE_CONV_GRAD && !aligned16(grad)) return fail(XGPR_ERR_WORKSPACE, "gradient pointer must be 16-byte aligned");
            if (!workspace || wbytes < masks_bytes(R)) return fail(XGPR_ERR_WORKSPACE, "workspace too small (see xgpr_rbf_workspace_bytes)");
            WaveArgs a = wave_args(x, chi, workspace, n, L * C, win, num_freqs, R);
            a.out = out; a.outf = outf; a.seqlen = seqlen_dev; a.kmer_stride = (int)C;
            a.conv_width = conv_width; a.scaling_type = scaling_type; a.fit_intercept = fit_intercept;
            a.scale = sqrt(1.0 / (double)num_freqs);
            if (grad_mode) { a.grad = grad; a.gradf = gradf; a.sigma = sigma; }
            return launch_wave_conv(a, radem, R, L, workspace, wbytes, st, [&](const WaveArgs &wa, long nblocks) {
                return dispatch_lg<1, 10>(lg, TOO_WIDE_WAVE, [&](auto LG) {
                    return dispatch_conv_mode(mode, [&](auto CM) {
                        return launch(wave_conv_kernel<decltype(LG)::value, decltype(CM)::value>, dim3((unsigned)nblocks), dim3(256), 0, st,
                                      "wave_conv_kernel launch", wa);
                    });
                });
            });
        }
    }
    SorfArgs<T> a = sorf_args(x, radem, chi, n, L * C, win, num_freqs, R);
    a.out = out; a.grad = grad; a.outf = outf; a.gradf = gradf; a.seqlen = seqlen_dev; a.kmer_stride = (int)C;
    a.conv_width = conv_width; a.scaling_type = scaling_type;
    a.scale = sqrt(1.0 / (double)num_freqs); a.sigma = sigma; a.fit_intercept = fit_intercept;
    {
        // wave tiles in registers + an LDS image (wave_tile.inc): float64 input at every padded window width up to 4096, float32 input at
        // 2048 / 4096 (narrower float32 windows were served above); XGPR_F64_PLAN=generic keeps the any-width path (A/B)
        const bool generic64 = wave_tile_plan_off();
        const bool mine = sizeof(T) == 8 ? P <= 4096 : (P > 1024 && P <= 4096);      // (8 / 16 waves per transform leave too few registers for the accumulators)
        const bool aligned = mode == MODE_MAXPOOL || rows_mode || (aligned16(out) && (mode != MODE_CONV_GRAD || aligned16(grad)));
        if (mine && !generic64 && aligned && R % 64 == 0 && (reinterpret_cast<uintptr_t>(radem) & 15) == 0) {
            const long items = n * (P > 1024 ? R / 1024 : (num_freqs + 1023) / 1024);
            rc = dispatch_lg<1, 13>(lg, TOO_WIDE_WT, [&](auto LGc) {
                constexpr int LG = decltype(LGc)::value;
                if constexpr ((sizeof(T) == 8 || LG > 10) && LG <= 12) {
                    using WT = WaveTile<T, LG>;
                    const char *what = "wave_tile_conv_kernel launch";
                    if (mode == MODE_CONV) return launch_wave_tile(wave_tile_conv_kernel<T, LG, MODE_CONV>, a, items, WT::WAVES, WT::LDS_BYTES, st, what);
                    if constexpr (sizeof(T) == 4) {      // the float32 row modes
                        if (mode == MODE_CONV_ROWS)
                            return launch_wave_tile(wave_tile_conv_kernel<T, LG, MODE_CONV_ROWS>, a, items, WT::WAVES, WT::LDS_BYTES, st, what);
                        if (mode == MODE_CONV_GRAD_ROWS)
                            return launch_wave_tile(wave_tile_conv_kernel<T, LG, MODE_CONV_GRAD_ROWS>, a, items, WT::WAVES, WT::LDS_BYTES, st, what);
                    }
                    if (mode == MODE_CONV_GRAD)
                        return launch_wave_tile(wave_tile_conv_kernel<T, LG, MODE_CONV_GRAD>, a, items, WT::WAVES, WT::LDS_BYTES, st, what);
                    return launch_wave_tile(wave_tile_conv_kernel<T, LG, MODE_MAXPOOL>, a, items, WT::WAVES, WT::LDS_BYTES, st, what);
                }
                return NO_ARM;
            });
            if (rc != NO_ARM) return rc;
        }
    }
    if (rows_mode) {
        if constexpr (sizeof(T) == 4)
            return conv_rows_staged(x, outf, mode == MODE_CONV_GRAD_ROWS ? gradf : nullptr, radem, chi, seqlen_host, seqlen_dev, n, L, C,
                                    num_rffs, num_freqs, R, sigma, conv_width, scaling_type, fit_intercept, workspace, wbytes, st);
        else return fail(XGPR_ERR_UNSUPPORTED, "float32 feature rows take float32 input");
    }
    if (mode == MODE_CONV) return launch_generic_sorf<T, MODE_CONV>(a, workspace, wbytes, st);
    if (mode == MODE_CONV_GRAD) return launch_generic_sorf<T, MODE_CONV_GRAD>(a, workspace, wbytes, st);
    return launch_generic_sorf<T, MODE_MAXPOOL>(a, workspace, wbytes, st);
}

int conv_rows_staged(const float *x, float *zrows, float *grows, const int8_t *radem, const float *chi, const int32_t *seqlen_host,
                     const int32_t *seqlen_dev, long n, long L, long C, long num_rffs, long num_freqs, long R, double sigma,
                     int conv_width, int scaling_type, int fit_intercept, void *workspace, size_t wbytes, hipStream_t st) {
    const long P = padded_width((long)conv_width * C);
    const size_t off = conv_rows_stage_offset(R, P, n), row = (size_t)num_rffs * sizeof(double);
    const size_t room = (!workspace || wbytes < off) ? 0 : wbytes - off;
    // one array: all the room; two arrays: half each, a multiple of 256 bytes (both 16-byte aligned, as the float64 operator's double2
    // accesses need)
    const size_t per_array = grows ? room / 2 / 256 * 256 : room;
    if (!workspace || !aligned16(workspace) || per_array < row)
        return fail(XGPR_ERR_WORKSPACE, grows ? "workspace too small (see xgpr_conv_grad_rows_workspace_bytes)"
                                              : "workspace too small (see xgpr_conv_feature_rows_workspace_bytes)");
    const char *memset_what = grows ? "hipMemsetAsync (gradient rows staging)" : "hipMemsetAsync (feature rows staging)";
    double *stage_z = reinterpret_cast<double *>(reinterpret_cast<unsigned char *>(workspace) + off);
    double *stage_g = grows ? reinterpret_cast<double *>(reinterpret_cast<unsigned char *>(workspace) + off + per_array) : nullptr;
    long rows = (long)(per_array / row);
    if (rows > n) rows = n;
    for (long lo = 0; lo < n; lo += rows) {
        const long cnt = n - lo < rows ? n - lo : rows;
        HIP_TRY(hipMemsetAsync(stage_z, 0, (size_t)cnt * row, st), memset_what);
        if (grows) HIP_TRY(hipMemsetAsync(stage_g, 0, (size_t)cnt * row, st), memset_what);
        int rc = conv_impl<float>(x + lo * L * C, stage_z, stage_g, nullptr, radem, chi, seqlen_host + lo, seqlen_dev + lo, cnt, L, C, cnt,
                                  num_rffs, cnt, num_rffs, num_freqs, R, cnt, sigma, conv_width, scaling_type,
                                  grows ? MODE_CONV_GRAD : MODE_CONV, workspace, off, (void *)st);
        if (rc) return rc;
        // KernelBase.gradient_x: xgrad[:, 0] = 0 under an intercept (the rounding pass below writes the 1.0f of the features itself)
        if (grows && fit_intercept)
            HIP_TRY(hipMemset2DAsync(stage_g, row, 0, sizeof(double), (size_t)cnt, st), "hipMemset2DAsync (gradient rows staging)");
        const long npairs = cnt * (num_rffs / 2);
        const long nblocks = (npairs + 255) / 256;
        if (nblocks > 2147483647L) return fail(XGPR_ERR_UNSUPPORTED, "staging slice too large for one rounding launch");
        rc = launch(round_rows_kernel, dim3((unsigned)nblocks), dim3(256), 0, st, "round_rows_kernel launch",
                    reinterpret_cast<const double2 *>(stage_z), reinterpret_cast<float2 *>(zrows + lo * num_rffs), npairs, num_rffs / 2, fit_intercept);
        if (rc) return rc;
        if (grows) {
            rc = launch(round_rows_kernel, dim3((unsigned)nblocks), dim3(256), 0, st, "round_rows_kernel launch",
                        reinterpret_cast<const double2 *>(stage_g), reinterpret_cast<float2 *>(grows + lo * num_rffs), npairs, num_rffs / 2, 0);
            if (rc) return rc;
        }
    }
    return 0;
}

// ---- token input for the float32 row writers (xgpr_conv_token_rows_f32 / xgpr_conv_token_grad_rows_f32): tokens[n, L] (uint8) index the
// rows of table[vocab, C]; the rows are those of the dense siblings on the expanded array table[tokens], bit for bit.  Served by
// wave_conv_tok_kernel where conv_token_rows_ok says so (a window of up to 1024 elements, a table that fits its LDS image); every other
// shape is an error here and the caller expands (ConvSORFKernel does, slice by slice).
int conv_token_rows_ok(long width, long vocab, long C) {
    if (vocab < 1 || vocab > 256 || C < 1 || width < C || width % C != 0) return 0;
    return padded_width(width) <= 1024 && vocab * C <= TOK_TABLE_FLOATS ? 1 : 0;
}

int conv_token_impl(const uint8_t *tokens, const float *table, float *zrows, float *grows, bool grad_mode, const int8_t *radem,
                    const float *chi, const int32_t *seqlen_host, const int32_t *seqlen_dev, long n, long L, long vocab, long C,
                    long num_rffs, long num_freqs, long R, long nseq, double sigma, int conv_width, int scaling_type, int fit_intercept,
                    void *workspace, size_t wbytes, void *stream) {
    if (vocab < 1 || vocab > 256) return fail(XGPR_ERR_ARRAY_DIMS, "token table: vocab must be 1 .. 256 (uint8 tokens)");
    if (C < 1) return fail(XGPR_ERR_ARRAY_DIMS, "token table: needs at least one column");
    const long win = (long)conv_width * C;
    const long P = padded_width(win > 0 ? win : 1);
    int rc = check_sorf_shape(n, num_rffs, num_freqs, R, P, 2, [&] {
        if (nseq != n) return fail(XGPR_ERR_SEQLEN_SIZE, "wrong array sizes");
        if (L < conv_width || conv_width <= 0) return fail(XGPR_ERR_CONV_WIDTH, "invalid conv_width");
        return 0;
    });
    if (rc) return rc;
    rc = check_seqlens(seqlen_host, nseq, n, L, conv_width);
    if (rc) return rc;
    if (!seqlen_dev) return fail(XGPR_ERR_WORKSPACE, "seqlen_dev (device copy of the sequence lengths) is required");
    if (!tokens || !table) return fail(XGPR_ERR_WORKSPACE, "tokens and table are required");
    if (!zrows || (reinterpret_cast<uintptr_t>(zrows) & 7) != 0) return fail(XGPR_ERR_WORKSPACE, "feature rows pointer must be 8-byte aligned");
    if (grad_mode && (!grows || (reinterpret_cast<uintptr_t>(grows) & 7) != 0))
        return fail(XGPR_ERR_WORKSPACE, "gradient rows pointer must be 8-byte aligned");
    if (!conv_token_rows_ok(win, vocab, C))
        return fail(XGPR_ERR_UNSUPPORTED, "token input serves windows of up to 1024 elements and tables of up to 4608 floats (see xgpr_conv_token_rows_ok)");
    if (!workspace || wbytes < masks_bytes(R)) return fail(XGPR_ERR_WORKSPACE, "workspace too small (see xgpr_conv_feature_rows_workspace_bytes)");
    hipStream_t st = (hipStream_t)stream;
    WaveArgs a = wave_args(table, chi, workspace, n, L, win, num_freqs, R);
    a.tokens = tokens; a.vocab = (int)vocab;
    a.outf = zrows; a.seqlen = seqlen_dev; a.kmer_stride = (int)C;
    a.conv_width = conv_width; a.scaling_type = scaling_type; a.fit_intercept = fit_intercept;
    a.scale = sqrt(1.0 / (double)num_freqs);
    if (grad_mode) { a.gradf = grows; a.sigma = sigma; }
    const int lg = ilog2(P);
    return launch_wave_conv(a, radem, R, L, workspace, wbytes, st, [&](const WaveArgs &wa, long nblocks) {
        return dispatch_lg<1, 10>(lg, TOO_WIDE_WAVE, [&](auto LG) {
            return dispatch_bool(grad_mode, [&](auto GR) {
                constexpr int CM = decltype(GR)::value ? CONV_GRAD_ROWS : CONV_ROWS;
                return launch(wave_conv_tok_kernel<decltype(LG)::value, CM>, dim3((unsigned)nblocks), dim3(256), 0, st,
                              "wave_conv_tok_kernel launch", wa);
            });
        });
    });
}

// ---- token input for the max-pool operator (xgpr_conv_token_maxpool_f32): xgpr_conv1d_maxpool_f32 on table[tokens], bit for bit.  Its
// checks are conv_impl's for MODE_MAXPOOL (one feature per frequency, radem_shape2 == reps * P) and conv_token_impl's for the table.
int conv_token_maxpool_impl(const uint8_t *tokens, const float *table, float *out, const int8_t *radem, const float *chi,
                            const int32_t *seqlen_host, const int32_t *seqlen_dev, long n, long L, long vocab, long C, long out_rows,
                            long num_rffs, long num_freqs, long R, long nseq, int conv_width, void *workspace, size_t wbytes,
                            void *stream) {
    if (vocab < 1 || vocab > 256) return fail(XGPR_ERR_ARRAY_DIMS, "token table: vocab must be 1 .. 256 (uint8 tokens)");
    if (C < 1) return fail(XGPR_ERR_ARRAY_DIMS, "token table: needs at least one column");
    if (out_rows != n) return fail(XGPR_ERR_NO_DATAPOINTS, "no datapoints");
    const long win = (long)conv_width * C;
    const long P = padded_width(win > 0 ? win : 1);
    const int reps = (int)((num_freqs + P - 1) / P);
    int rc = check_sorf_shape(n, num_rffs, num_freqs, R, P, 1, [&] {
        if (nseq != n) return fail(XGPR_ERR_SEQLEN_SIZE, "wrong array sizes");
        if (L < conv_width || conv_width <= 0) return fail(XGPR_ERR_CONV_WIDTH, "invalid conv_width");
        return 0;
    });
    if (rc) return rc;
    if (R != (long)reps * P) return fail(XGPR_ERR_RFFS_FREQS, "incorrect number of rffs and or freqs.");
    rc = check_seqlens(seqlen_host, nseq, n, L, conv_width);
    if (rc) return rc;
    if (!seqlen_dev) return fail(XGPR_ERR_WORKSPACE, "seqlen_dev (device copy of the sequence lengths) is required");
    if (!tokens || !table || !out) return fail(XGPR_ERR_WORKSPACE, "tokens, table and out are required");
    if (!conv_token_rows_ok(win, vocab, C))
        return fail(XGPR_ERR_UNSUPPORTED, "token input serves windows of up to 1024 elements and tables of up to 4608 floats (see xgpr_conv_token_rows_ok)");
    if (!workspace || wbytes < masks_bytes(R)) return fail(XGPR_ERR_WORKSPACE, "workspace too small (see xgpr_conv_workspace_bytes)");
    hipStream_t st = (hipStream_t)stream;
    WaveArgs a = wave_args(table, chi, workspace, n, L, win, num_freqs, R);
    a.tokens = tokens; a.vocab = (int)vocab;
    a.outf = out; a.seqlen = seqlen_dev; a.kmer_stride = (int)C; a.conv_width = conv_width;
    a.scale = sqrt(1.0 / (double)num_freqs);
    const int lg = ilog2(P);
    return launch_wave_conv(a, radem, R, L, workspace, wbytes, st, [&](const WaveArgs &wa, long nblocks) {
        return dispatch_lg<1, 10>(lg, TOO_WIDE_WAVE, [&](auto LG) {
            return launch(wave_conv_tok_kernel<decltype(LG)::value, CONV_MAXPOOL>, dim3((unsigned)nblocks), dim3(256), 0, st,
                          "wave_conv_tok_kernel launch", wa);
        });
    });
}

constexpr long ZTZ_MAX_SLABS = 2048;
constexpr long ZTZ_ROW_WINDOW = 131072;    // two-pass matvec: rows per (dot, update) launch pair

// Which shapes take two feature passes (dot pass, update pass: ztz_two_pass): more than 8192 frequencies -- one workgroup
// cannot hold v for all tiles of a datapoint -- and, since round 5, EIGHT tiles per datapoint (7168 < num_freqs <= 8192, e.g.
// 16384 RFFs): eight does not divide the three-wave kernel's twelve waves, the single pass fell back to the two-wave
// kernel at 3.66 ns per tile (d = 1024), and two passes of the three-wave kernel in tile groups of four measure faster
// (profiles/r5_nb8_two_pass_ab.txt: 3.84 -> 2.40 ms per 131 072 rows at d = 1024, 1-5 % at narrower rows; with five or seven
// tiles the two-wave single pass stays ahead, 1.73 against 2.35 ms).  XGPR_ZTZ_NB8=1 in the environment keeps the single pass
// (A/B timing).
bool ztz_takes_two_passes(long d, long P, long num_freqs, bool x_aligned) {
    if (num_freqs > 8192) return true;
    static const bool keep_one = [] { const char *e = getenv("XGPR_ZTZ_NB8"); return e && e[0] == '1'; }();
    static const long min_freqs = [] { const char *e = getenv("XGPR_ZTZ_TWO_PASS_ABOVE"); return e ? atol(e) : 7168L; }();   // (timing experiments)
    (void)d; (void)x_aligned;
    if (P > 1024) return ztz3_compute_tiles(P, num_freqs) > 4;       // wide transforms: one group holds at most four tiles
    return !keep_one && num_freqs > min_freqs && P >= 2 && P <= 1024;
}

// (the row-window buffer of the two passes is reserved wherever ANY padded width could take them: more than four tiles -- wide
// transforms -- or the environment's threshold; the size is independent of the input width, which this query is not given)
size_t ztz_workspace_bytes(long num_rffs, long R) {
    size_t b = masks_bytes(R) + (size_t)ZTZ_MAX_SLABS * num_rffs * sizeof(double);
    if (num_rffs / 2 > 4096 || ztz_takes_two_passes(1024, 1024, num_rffs / 2, true))
        b += (size_t)ZTZ_ROW_WINDOW * ((num_rffs / 2 + 1023) / 1024) * sizeof(double);
    return b;
}

// independent-wave kernels: 4 waves per workgroup, two waves per SIMD over the chip, a whole number
// of datapoint slots (nb waves each), at most ZTZ_MAX_SLABS slots and no more slots than datapoints
void flat_geometry(int nb, long n, int &waves_per_wg, long &nblocks, long &nslots) {
    waves_per_wg = 4;
    long waves = (long)device_cus() * 8;
    nslots = waves / nb > 0 ? waves / nb : 1;
    if (nslots > ZTZ_MAX_SLABS) nslots = ZTZ_MAX_SLABS;
    if (nslots > n) nslots = n;
    // nslots * nb must be a multiple of 4
    while ((nslots * nb) % 4 != 0) nslots++;
    nblocks = nslots * nb / 4;
}

int ztz_two_pass(const float *x, const int8_t *radem, const float *chi, const double *vec, double *w_out, long n,
                 long d, long num_rffs, long num_freqs, long R, int fit_intercept, void *workspace, hipStream_t st);

template <bool MATVEC>
int ztz_impl(const float *x, const int8_t *radem, const float *chi, const double *vec, double *w_out, long n,
             long d, long num_rffs, long num_freqs, long R, int fit_intercept, void *workspace, size_t wbytes,
             void *stream) {
    const long P = padded_width(d);
    int rc = check_sorf_shape(n, num_rffs, num_freqs, R, P);
    if (rc) return rc;
    if (P > 4096) return fail(XGPR_ERR_UNSUPPORTED, "fused matvec supports padded width <= 4096");
    if (num_freqs > 65536) return fail(XGPR_ERR_UNSUPPORTED, "fused matvec supports num_freqs <= 65536");
    if ((MATVEC && !aligned16(vec)) || !aligned16(w_out)) return fail(XGPR_ERR_WORKSPACE, "vector pointers must be 16-byte aligned");
    const size_t mb = masks_bytes(R);
    const size_t need = ztz_workspace_bytes(num_rffs, R);
    if (!workspace || wbytes < need || !aligned16(workspace))
        return fail(XGPR_ERR_WORKSPACE, "workspace too small (see xgpr_ztz_matvec_workspace_bytes)");
    hipStream_t st = (hipStream_t)stream;
    if (MATVEC && ztz_takes_two_passes(d, P, num_freqs, aligned16(x)))
        return ztz_two_pass(x, radem, chi, vec, w_out, n, d, num_rffs, num_freqs, R, fit_intercept, workspace, st);

    WaveArgs a = wave_args(x, chi, workspace, n, d, d, num_freqs, R);
    a.vec = vec;
    a.wpart = reinterpret_cast<double *>(reinterpret_cast<unsigned char *>(workspace) + mb);
    // 8 waves per workgroup where possible (2 per SIMD, the register budget of this kernel): the
    // G datapoint slots of a workgroup share one copy of v in LDS
    a.G = a.nb >= 8 ? 1 : 8 / a.nb;
    if ((long)a.G > n) a.G = (int)n;
    a.fit_intercept = fit_intercept;
    a.scale = rbf_scale<float>(num_freqs, fit_intercept);
    const int lg = ilog2(P);
    rc = radem ? pack_masks(radem, (uint64_t *)workspace, R, a.MW, st) : 0;   // NULL: masks already in the workspace
    if (rc) return rc;

    // the three-waves-per-SIMD kernel (fused_ztz.inc) wherever its shape conditions hold, for the matvec and for
    // z^T y alike; XGPR_ZTZ_WAVES=2 in the environment keeps the two-wave kernel (A/B timing, tools/bench_fused.py)
    static const bool force2 = [] { const char *e = getenv("XGPR_ZTZ_WAVES"); return e && e[0] == '2'; }();
    // z^T y needs no datapoint-wide sum, so tile counts the single group cannot hold (7, 8, more than 8192 frequencies) run as
    // several tile groups on blockIdx.y -- every group fetches the row for itself and writes its own tiles of the column's slab --
    // instead of on the two-wave kernel (d = 64, M = 32768: 3.5 -> ~2 ms per 131 072 rows)
    int ngroups3 = 1;
    const bool wide = P > 1024;
    if (wide) a.nb = ztz3_compute_tiles(P, num_freqs);            // whole transforms
    bool z3 = (!force2 || wide) && ztz3_ok(x, d, P, a.nb);
    if (!MATVEC && (!force2 || wide) && !z3 && a.nb >= 2 && P >= 2 && P <= 4096) {
        int nbg = ztz3_group_tiles(a.nb, P);
        if (ztz3_lds_bytes(nbg, P) > 160 * 1024) nbg = 4;
        if (ztz3_lds_bytes(nbg, P) <= 160 * 1024) {
            ngroups3 = (a.nb + nbg - 1) / nbg;
            a.nb = nbg;
            z3 = true;
        }
    }
    if (z3) {
        a.G = ztz3_slots(a.nb, P);
        a.dma1 = ztz3_dma1(x, d);
        long nblocks3 = device_cus() / ngroups3 > 0 ? device_cus() / ngroups3 : 1;
        const long by_rows = (n + a.G - 1) / a.G;
        if (nblocks3 > by_rows) nblocks3 = by_rows;
        if (nblocks3 * a.G > ZTZ_MAX_SLABS) nblocks3 = ZTZ_MAX_SLABS / a.G;
        const size_t lds3 = ztz3_lds_bytes(a.nb, P);
        rc = dispatch_lg<1, 12>(lg, TOO_WIDE_Z3, [&](auto LG) {
            return launch_ztz3<decltype(LG)::value, MATVEC ? Z3_MATVEC : Z3_ZTY>(a, nblocks3, ngroups3, lds3, st, "ztz3_kernel launch");
        });
        if (rc) return rc;
        return reduce_slabs(a.wpart, w_out, num_rffs, nblocks3, st);         // one slab per workgroup (its G slots are added up in LDS)
    }

    if (wide) return fail(XGPR_ERR_UNSUPPORTED, "fused matvec: no plan for this shape at padded width > 1024");
    int waves_per_wg = a.nb * a.G;
    int wg_per_cu = 8 / waves_per_wg > 0 ? 8 / waves_per_wg : 1;     // 2 waves per SIMD
    long nblocks = (long)device_cus() * wg_per_cu;
    long nslabs;
    if (MATVEC) {
        const long max_by_rows = (n + a.G - 1) / a.G;
        if (nblocks > max_by_rows) nblocks = max_by_rows;
        if (nblocks * a.G > ZTZ_MAX_SLABS) nblocks = ZTZ_MAX_SLABS / a.G;
        nslabs = nblocks * a.G;
    } else {
        flat_geometry(a.nb, n, waves_per_wg, nblocks, nslabs);
        wg_per_cu = 2;
    }
    const size_t lds_base = (MATVEC ? (size_t)a.nb * 1024 * 16 : 0) + 256;
    const size_t lds_t = lds_base + (size_t)waves_per_wg * TBUF_FLOATS * sizeof(float);
    // the two-layout FHT needs 5 KiB of LDS per wave; without room for it (M = 16384) the register-only FHT runs
    const bool tp = lg >= 7 && lds_t * wg_per_cu <= 160 * 1024;
    const size_t lds = tp ? lds_t : lds_base;
    rc = dispatch_lg<1, 10>(lg, TOO_WIDE_WAVE, [&](auto LG) {
        return dispatch_bool(tp, [&](auto TP) {
            return launch(wave_ztz_kernel<decltype(LG)::value, MATVEC, decltype(TP)::value>, dim3((unsigned)nblocks), dim3(waves_per_wg * 64),
                          lds, st, "wave_ztz_kernel launch", a);
        });
    });
    if (rc) return rc;
    return reduce_slabs(a.wpart, w_out, num_rffs, nslabs, st);
}

// Z^T(Z v) for more tiles per datapoint than one workgroup holds (ztz_takes_two_passes): per window of rows, (1) the dot
// pass (ztz3_kernel<., Z3_DOT>) writes the per-tile partial dots, (2) the update pass (Z3_UPD) recomputes the features
// and accumulates z_i * (z_i . v) into its slabs; then the slabs are reduced as in the single-pass path.  Costs one extra
// SORF + sincos per feature but has no coupling between the tile groups of a datapoint, so it works for any number of tiles.
int ztz_two_pass(const float *x, const int8_t *radem, const float *chi, const double *vec, double *w_out, long n,
                 long d, long num_rffs, long num_freqs, long R, int fit_intercept, void *workspace, hipStream_t st) {
    const long P = padded_width(d);
    const size_t mb = masks_bytes(R);
    WaveArgs a = wave_args(x, chi, workspace, n, d, d, num_freqs, R);       // (x and n: per row window, below)
    a.vec = vec;
    a.wpart = reinterpret_cast<double *>(reinterpret_cast<unsigned char *>(workspace) + mb);
    a.tpart = a.wpart + (size_t)ZTZ_MAX_SLABS * num_rffs;
    a.G = 1; a.fit_intercept = fit_intercept;
    a.scale = rbf_scale<float>(num_freqs, fit_intercept);
    const int lg = ilog2(P);
    int rc = radem ? pack_masks(radem, (uint64_t *)workspace, R, a.MW, st) : 0;   // NULL: masks already in the workspace
    if (rc) return rc;
    // the three-wave plan (fused_ztz.inc, Z3_DOT / Z3_UPD): workgroups of 12 waves = slots x a group of `nbg` consecutive
    // tiles, blockIdx.y = tile group; x by LDS-DMA, chi and v in LDS, no scratch.  Slab i collects workgroup column i.
    // (Rounds 1-5 kept a two-wave form of both passes -- wave_dot_kernel + wave_ztz_kernel with tpart -- behind
    // XGPR_ZTZ_WAVES=2; no shape reached it since round 3 and it is gone.)
    if (P < 2) return fail(XGPR_ERR_UNSUPPORTED, "fused matvec: padded width < 2");
    const int nbt = P > 1024 ? ztz3_compute_tiles(P, num_freqs) : a.nb;
    int nbg = ztz3_group_tiles(nbt, P);
    if (ztz3_lds_bytes(nbg, P) > 160 * 1024) nbg = 4;
    const int ngroups = (nbt + nbg - 1) / nbg;
    a.nb = nbg; a.G = ztz3_slots(nbg, P);
    long ncols = device_cus() / ngroups > 0 ? device_cus() / ngroups : 1;
    if (ncols * a.G > ZTZ_MAX_SLABS) ncols = ZTZ_MAX_SLABS / a.G;
    const size_t lds3 = ztz3_lds_bytes(nbg, P);
    for (long row0 = 0; row0 < n; row0 += ZTZ_ROW_WINDOW) {
        const long rows = n - row0 < ZTZ_ROW_WINDOW ? n - row0 : ZTZ_ROW_WINDOW;
        a.x = x + row0 * d;
        a.dma1 = ztz3_dma1(a.x, d);
        a.n = rows;
        a.add_to_slab = row0 > 0;
        rc = dispatch_lg<1, 12>(lg, TOO_WIDE_Z3, [&](auto LG) {
            const int rcd = launch_ztz3<decltype(LG)::value, Z3_DOT>(a, ncols, ngroups, lds3, st, "ztz3_kernel (dot pass) launch");
            return rcd ? rcd : launch_ztz3<decltype(LG)::value, Z3_UPD>(a, ncols, ngroups, lds3, st, "ztz3_kernel (update pass) launch");
        });
        if (rc) return rc;
    }
    return reduce_slabs(a.wpart, w_out, num_rffs, ncols, st);
}

int zcache_build_impl(const float *x, float *zc, const int8_t *radem, const float *chi, long n, long d,
                      long num_rffs, long num_freqs, long R, void *workspace, size_t wbytes, void *stream) {
    const long P = padded_width(d);
    int rc = check_sorf_shape(n, num_rffs, num_freqs, R, P);
    if (rc) return rc;
    if (!workspace || wbytes < masks_bytes(R)) return fail(XGPR_ERR_WORKSPACE, "workspace too small (see xgpr_rbf_workspace_bytes)");
    if ((reinterpret_cast<uintptr_t>(zc) & 7) != 0) return fail(XGPR_ERR_WORKSPACE, "cache pointer must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (P > 4096) {
        // the transforms of the float32 feature operator at the same width (rbf_impl): wave tiles at P = 8192 under that operator's own
        // conditions, the any-width path otherwise (in LDS up to 32768 floats, beyond that in the workspace's global scratch:
        // xgpr_sorf_workspace_bytes)
        if (d > 2147483647L) return fail(XGPR_ERR_UNSUPPORTED, "the feature cache: input width beyond 2^31 - 1");
        SorfArgs<float> s = sorf_args(x, radem, chi, n, d, d, num_freqs, R);
        s.outf = zc;
        if (P == 8192 && !wave_tile_plan_off() && R % 64 == 0 && (reinterpret_cast<uintptr_t>(radem) & 15) == 0) {
            using WT = WaveTile<float, 13>;
            return launch_wave_tile(wave_tile_rbf_cache_kernel<13>, s, n * (R / 1024), WT::WAVES, WT::LDS_BYTES, st,
                                    "wave_tile_rbf_cache_kernel launch");
        }
        return launch_generic_sorf<float, MODE_RBF_CACHE>(s, workspace, wbytes, st);
    }
    WaveArgs a = wave_args(x, chi, workspace, n, d, d, num_freqs, R);
    a.outf = zc;
    const int lg = ilog2(P);
    rc = pack_masks(radem, (uint64_t *)workspace, R, a.MW, st);
    if (rc) return rc;
    {
        const int rcf = launch_ztz3_feat<Z3_FEAT32>(a, P, lg, st);
        if (rcf != 0) return rcf < 0 ? rcf : 0;
    }
    if (P > 1024) return fail(XGPR_ERR_UNSUPPORTED, "the feature cache: no plan for this shape at padded width > 1024");
    const long nblocks = (n * a.nb + 3) / 4;
    if (nblocks > 2147483647L) return fail(XGPR_ERR_UNSUPPORTED, "too many datapoints for one launch");
    return dispatch_lg<1, 10>(lg, TOO_WIDE_WAVE, [&](auto LG) {
        return launch(wave_rbf_kernel<decltype(LG)::value, OUT_CACHE>, dim3((unsigned)nblocks), dim3(256), 0, st, "wave_rbf_kernel (cache) launch", a);
    });
}

// ---- float32 feature AND gradient rows of the fixed-vector kernels (xgpr_rbf_grad_rows_f32): the float32 gradient operator's kernels
// (rbf_impl with want_grad: wave_rbf_kernel up to P = 1024, wave tiles at 2048 / 4096 / 8192) with a float2 epilogue into two row arrays.
// Wider inputs are refused with the feature cache's code for a shape it has no plan for: the caller keeps the float64 operator.
int rbf_grad_rows_impl(const float *x, float *zrows, float *grows, const int8_t *radem, const float *chi, long n, long d,
                       long num_rffs, long num_freqs, long R, double sigma, int fit_intercept, void *workspace, size_t wbytes,
                       void *stream) {
    const long P = padded_width(d);
    int rc = check_sorf_shape(n, num_rffs, num_freqs, R, P);
    if (rc) return rc;
    if (P > 8192) return fail(XGPR_ERR_UNSUPPORTED, "the gradient rows: no plan at padded width > 8192");
    if (!zrows || !grows || (reinterpret_cast<uintptr_t>(zrows) & 7) != 0 || (reinterpret_cast<uintptr_t>(grows) & 7) != 0)
        return fail(XGPR_ERR_WORKSPACE, "row pointers must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const double scale = rbf_scale<double>(num_freqs, fit_intercept);
    const int lg = ilog2(P);
    if (P <= 1024) {
        if (!workspace || wbytes < masks_bytes(R)) return fail(XGPR_ERR_WORKSPACE, "workspace too small (see xgpr_rbf_workspace_bytes)");
        WaveArgs a = wave_args(x, chi, workspace, n, d, d, num_freqs, R);
        a.outf = zrows; a.gradf = grows;
        a.scale = scale; a.sigma = sigma; a.fit_intercept = fit_intercept;
        const long nblocks = (n * a.nb + 3) / 4;
        if (nblocks > 2147483647L) return fail(XGPR_ERR_UNSUPPORTED, "too many datapoints for one launch");
        rc = pack_masks(radem, (uint64_t *)workspace, R, a.MW, st);
        if (rc) return rc;
        return dispatch_lg<1, 10>(lg, TOO_WIDE_WAVE, [&](auto LG) {
            return launch(wave_rbf_kernel<decltype(LG)::value, OUT_GRAD_ROWS>, dim3((unsigned)nblocks), dim3(256), 0, st,
                          "wave_rbf_kernel (gradient rows) launch", a);
        });
    }
    if (R % 64 != 0 || (reinterpret_cast<uintptr_t>(radem) & 15) != 0)
        return fail(XGPR_ERR_UNSUPPORTED, "the gradient rows: the wave tiles read the Rademacher array 16 bytes at a time");
    SorfArgs<float> s = sorf_args(x, radem, chi, n, d, d, num_freqs, R);
    s.outf = zrows; s.gradf = grows;
    s.sigma = sigma; s.scale = scale; s.fit_intercept = fit_intercept;
    const long items = n * (R / 1024);
    return dispatch_lg<11, 13>(lg, TOO_WIDE_WT, [&](auto LGc) {
        using WT = WaveTile<float, decltype(LGc)::value>;
        return launch_wave_tile(wave_tile_rbf_grad_rows_kernel<decltype(LGc)::value>, s, items, WT::WAVES, WT::LDS_BYTES, st,
                                "wave_tile_rbf_grad_rows_kernel launch");
    });
}

int zcache_matvec_impl(const float *zc, const double *vec, double *w_out, long n, long num_rffs, int fit_intercept,
                       double scale_override, void *workspace, size_t wbytes, void *stream) {
    if (n == 0) return fail(XGPR_ERR_NO_DATAPOINTS, "no datapoints");
    if (num_rffs < 2 || (num_rffs & 1) != 0) return fail(XGPR_ERR_ODD_OUTPUT, "last dim of output must be even number");
    const long F = num_rffs / 2;
    if (F > 16384) return fail(XGPR_ERR_UNSUPPORTED, "cached matvec supports num_freqs <= 16384");
    if (!aligned16(vec) || !aligned16(w_out) || !aligned16(zc)) return fail(XGPR_ERR_WORKSPACE, "pointers must be 16-byte aligned");
    const size_t need = (size_t)ZTZ_MAX_SLABS * num_rffs * sizeof(double);
    if (!workspace || wbytes < need || !aligned16(workspace))
        return fail(XGPR_ERR_WORKSPACE, "workspace too small (see xgpr_ztz_matvec_workspace_bytes)");
    hipStream_t st = (hipStream_t)stream;
    ZcArgs a = {};
    a.zc = zc; a.vec = vec; a.wpart = reinterpret_cast<double *>(workspace);
    a.n = n; a.F = F; a.nb = (int)((F + 1023) / 1024);
    a.G = 8 / a.nb;                                // 8 waves per workgroup = 2 per SIMD, deep register rings
    if ((long)a.G > n) a.G = (int)n;
    a.fit_intercept = fit_intercept;
    a.scale = scale_override > 0.0 ? scale_override : rbf_scale<float>(F, fit_intercept);
    a.inv_scale = 1.0 / a.scale; a.scale2 = a.scale * a.scale;
    if (a.nb > 8) {
        // wide rows: one 8-wave workgroup per CU, two tiles per wave (zcache_ztz_wide_kernel)
        a.G = 1;
        long nwg = device_cus();
        if (nwg > n) nwg = n;
        if (nwg > ZTZ_MAX_SLABS) nwg = ZTZ_MAX_SLABS;
        const size_t wlds = (size_t)8 * 1024 * 16 + 2 * 8 * sizeof(double);
        const int rc = dispatch_bool(F % 2 == 0, [&](auto EVEN) {
            return launch(zcache_ztz_wide_kernel<decltype(EVEN)::value>, dim3((unsigned)nwg), dim3(512), wlds, st, "zcache_ztz_wide_kernel launch", a);
        });
        return rc ? rc : reduce_slabs(a.wpart, w_out, num_rffs, nwg, st);
    }
    const int waves = a.nb * a.G;
    long nblocks = device_cus();
    const long max_by_rows = (n + a.G - 1) / a.G;
    if (nblocks > max_by_rows) nblocks = max_by_rows;
    if (nblocks * a.G > ZTZ_MAX_SLABS) nblocks = ZTZ_MAX_SLABS / a.G;
    constexpr int RING = 2;     // measured: 6.3 TB/s with 2 (222 VGPRs), 6.0 with 3, 3.8 with 4 (spills)
    const size_t lds = (size_t)a.nb * 1024 * 16 + 2 * 8 * 8 * sizeof(double);
    const int rc = dispatch_bool(F % 2 == 0, [&](auto EVEN) {
        return launch(zcache_ztz_kernel<decltype(EVEN)::value, RING>, dim3((unsigned)nblocks), dim3(waves * 64), lds, st, "zcache_ztz_kernel launch", a);
    });
    return rc ? rc : reduce_slabs(a.wpart, w_out, num_rffs, nblocks * a.G, st);
}

// float32 rows -> binary16 rows (xgpr_rows_pack_f16): a grid of at most 8 workgroups per CU strides over the block
int rows_pack_f16_impl(const float *rows, uint16_t *out, long count, void *stream) {
    if (count <= 0) return fail(XGPR_ERR_NO_DATAPOINTS, "no datapoints");
    if (!aligned16(rows) || (reinterpret_cast<uintptr_t>(out) & 7) != 0)
        return fail(XGPR_ERR_WORKSPACE, "float32 rows must be 16-byte aligned and binary16 rows 8-byte aligned");
    long nblocks = (count / 4 + 255) / 256;
    if (nblocks < 1) nblocks = 1;
    if (nblocks > 8L * device_cus()) nblocks = 8L * device_cus();
    return launch(rows_pack_f16_kernel, dim3((unsigned)nblocks), dim3(256), 0, (hipStream_t)stream, "rows_pack_f16_kernel launch", rows, out, count);
}

int zcache_matvec_f16_impl(const uint16_t *zc, const double *vec, double *w_out, long n, long num_rffs, int fit_intercept,
                           double scale_override, void *workspace, size_t wbytes, void *stream) {
    if (n == 0) return fail(XGPR_ERR_NO_DATAPOINTS, "no datapoints");
    if (num_rffs < 2 || (num_rffs & 1) != 0) return fail(XGPR_ERR_ODD_OUTPUT, "last dim of output must be even number");
    const long F = num_rffs / 2;
    if (F > 8192) return fail(XGPR_ERR_UNSUPPORTED, "cached matvec over binary16 rows supports num_freqs <= 8192");
    if (!aligned16(vec) || !aligned16(w_out) || (reinterpret_cast<uintptr_t>(zc) & 3) != 0)
        return fail(XGPR_ERR_WORKSPACE, "vector pointers must be 16-byte aligned, the binary16 cache 4-byte aligned");
    const size_t need = (size_t)ZTZ_MAX_SLABS * num_rffs * sizeof(double);
    if (!workspace || wbytes < need || !aligned16(workspace))
        return fail(XGPR_ERR_WORKSPACE, "workspace too small (see xgpr_ztz_matvec_workspace_bytes)");
    hipStream_t st = (hipStream_t)stream;
    Zc16Args a = {};
    a.zc = zc; a.vec = vec; a.wpart = reinterpret_cast<double *>(workspace);
    a.n = n; a.F = F; a.nb = (int)((F + 1023) / 1024);
    a.G = 8 / a.nb;                                // as zcache_matvec_impl: 8 waves per workgroup = 2 per SIMD
    if ((long)a.G > n) a.G = (int)n;
    a.fit_intercept = fit_intercept;
    const double scale = scale_override > 0.0 ? scale_override : rbf_scale<float>(F, fit_intercept);
    a.inv_scale = 1.0 / scale; a.scale2 = scale * scale;
    const int waves = a.nb * a.G;
    long nblocks = device_cus();
    const long max_by_rows = (n + a.G - 1) / a.G;
    if (nblocks > max_by_rows) nblocks = max_by_rows;
    if (nblocks * a.G > ZTZ_MAX_SLABS) nblocks = ZTZ_MAX_SLABS / a.G;
    // Rows start on a 4-byte boundary for every even num_rffs; a load is as wide as the row length and the base allow: FPL = 4 / 2 / 1
    // frequencies (16 / 8 / 4 bytes).  RING datapoints in flight per wave, measured on one MI355X in one process with every candidate
    // instantiated, five rounds of ten launches alternating with the float32 kernel (profiles/half_cache_sweep.json), ms per matvec,
    // median (min .. max) -- float32 rows, zcache_ztz_kernel: 5.136 (5.127 .. 5.137) / 0.687 (0.686 .. 0.693) / 2.729 (2.723 .. 2.735):
    //   FPL RING VGPRs | 1e6 x 8192            | 125 000 x 8192        | 250 000 x 16384
    //    2   2   200   | 3.170 (3.160 .. 3.181) | 0.440 (0.438 .. 0.444) | 1.677 (1.620 .. 1.684)
    //    2   3   216   | 3.033 (3.018 .. 3.048) | 0.401 (0.400 .. 0.404) | 1.568 (1.526 .. 1.577)
    //    2   4   232   | 2.966 (2.954 .. 2.973) | 0.393 (0.387 .. 0.396) | 1.526 (1.494 .. 1.531)
    //    2   5   248   | 2.924 (2.922 .. 2.932) | 0.386 (0.381 .. 0.395) | 1.500 (1.475 .. 1.505)
    //    4   2   204   | 3.174 (3.161 .. 3.237) | 0.405 (0.404 .. 0.409) | 1.545 (1.542 .. 1.608)
    //    4   3   220   | 2.823 (2.788 .. 2.830) | 0.368 (0.367 .. 0.373) | 1.448 (1.400 .. 1.450)
    //    4   4   236   | 2.721 (2.715 .. 2.767) | 0.362 (0.358 .. 0.367) | 1.393 (1.381 .. 1.410)
    //    4   5   252   | 2.708 (2.698 .. 2.709) | 0.357 (0.355 .. 0.367) | 1.376 (1.363 .. 1.391)
    // (RING = 6 spills at every width.)  16-byte loads win at every depth from 3 on (v in planes: zcache_half.inc).  RING = 5 is 0.5 - 1.4 %
    // ahead of 4 with overlapping ranges at two of the three shapes, four registers below the limit of two waves per SIMD; RING = 4
    // keeps 20 registers of headroom and is what is built.  4-byte loads (odd num_freqs, or a base that is only 4-byte aligned) spend
    // more registers on addresses: RING = 4 spills there, 3 does not (242 VGPRs).
    const uintptr_t base = reinterpret_cast<uintptr_t>(zc);
    const int fpl = (F % 4 == 0 && (base & 15) == 0) ? 4 : (F % 2 == 0 && (base & 7) == 0) ? 2 : 1;
    const size_t lds = (size_t)a.nb * 1024 * 16 + 2 * 8 * 8 * sizeof(double);
    const dim3 grid((unsigned)nblocks), block((unsigned)(waves * 64));
    const char *what = "zcache16_ztz_kernel launch";
    const int rc = fpl == 4 ? launch(zcache16_ztz_kernel<4, 4>, grid, block, lds, st, what, a)
                 : fpl == 2 ? launch(zcache16_ztz_kernel<2, 4>, grid, block, lds, st, what, a)
                            : launch(zcache16_ztz_kernel<1, 3>, grid, block, lds, st, what, a);
    return rc ? rc : reduce_slabs(a.wpart, w_out, num_rffs, nblocks * a.G, st);
}

// z^T y over float32 feature rows (xgpr_zcache_zty_f32): ~8 workgroups per CU of 512 columns x a contiguous range of rows, partial
// sums in slabs of the workspace (the matvec's ZTZ_MAX_SLABS x M doubles), added in slab order -- the geometry depends on n, M and the
// device only, so the result is reproducible bit for bit
int zcache_zty_impl(const float *zc, const double *y, double *out, long n, long num_rffs, int fit_intercept, double scale_override,
                    void *workspace, size_t wbytes, void *stream) {
    if (n == 0) return fail(XGPR_ERR_NO_DATAPOINTS, "no datapoints");
    if (num_rffs < 2 || (num_rffs & 1) != 0) return fail(XGPR_ERR_ODD_OUTPUT, "last dim of output must be even number");
    if (((reinterpret_cast<uintptr_t>(zc) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(out)) & 7) != 0)
        return fail(XGPR_ERR_WORKSPACE, "cache, y and output pointers must be 8-byte aligned");
    const size_t need = (size_t)ZTZ_MAX_SLABS * num_rffs * sizeof(double);
    if (!workspace || wbytes < need || !aligned16(workspace))
        return fail(XGPR_ERR_WORKSPACE, "workspace too small (see xgpr_ztz_matvec_workspace_bytes)");
    hipStream_t st = (hipStream_t)stream;
    const long F = num_rffs / 2;
    const double scale = scale_override > 0.0 ? scale_override : rbf_scale<float>(F, fit_intercept);
    const long ncb = (num_rffs + 511) / 512;
    long nslabs = (8 * device_cus() + ncb - 1) / ncb;
    if (nslabs > ZTZ_MAX_SLABS) nslabs = ZTZ_MAX_SLABS;
    if (nslabs > n) nslabs = n;
    const long rows_per_slab = (n + nslabs - 1) / nslabs;
    nslabs = (n + rows_per_slab - 1) / rows_per_slab;
    double *wpart = reinterpret_cast<double *>(workspace);
    const int rc = launch(zcache_zty_kernel, dim3((unsigned)ncb, (unsigned)nslabs), dim3(256), 0, st, "zcache_zty_kernel launch", zc, y, wpart,
                          n, num_rffs, rows_per_slab, fit_intercept, scale);
    return rc ? rc : reduce_slabs(wpart, out, num_rffs, nslabs, st);
}

struct ZbGeom { int kp; long mblk; long nrb; long rows_per_range; size_t t_bytes; size_t slab_bytes;
                int rt; int msplit; long feats_per_split; size_t tpart_bytes; int tw; };

ZbGeom zb_geometry(long n, long num_rffs, long k) {
    ZbGeom gm;
    gm.kp = k <= 16 ? 16 : 32;
    gm.mblk = (num_rffs + ZB_WFEATS - 1) / ZB_WFEATS;
    long target = (2L * device_cus() + gm.mblk - 1) / gm.mblk;      // row ranges wanted: ~2 workgroups per CU
    const long max_ranges = (n + ZB_ROWS - 1) / ZB_ROWS;
    if (target > max_ranges) target = max_ranges;
    if (target < 1) target = 1;
    gm.rows_per_range = ((n + target - 1) / target + ZB_ROWS - 1) / ZB_ROWS * ZB_ROWS;
    gm.nrb = (n + gm.rows_per_range - 1) / gm.rows_per_range;
    gm.t_bytes = ((size_t)n * gm.kp * sizeof(double) + 255) / 256 * 256;
    gm.slab_bytes = (size_t)gm.nrb * num_rffs * gm.kp * sizeof(double);
    // T kernel: 16 RT datapoints per wave, 8 waves; RT = 4 reuses each LDS operand most, smaller RT
    // keeps every CU busy when the shard (or window) is short
    const long cus = device_cus();
    gm.rt = n >= 2 * cus * 512 ? 4 : n >= 2 * cus * 256 ? 2 : 1;
    static const int force_rt = [] { const char *e = getenv("XGPR_ZB_RT"); return e ? atoi(e) : 0; }();   // timing experiments
    if (force_rt == 1 || force_rt == 2 || force_rt == 4) gm.rt = force_rt;
    gm.tw = 8;
#ifdef XGPR_ZB_T12          // (development build: twelve-wave workgroups of RT = 2 for long launches -- measured slower, zblock.inc)
    if (gm.rt == 4 && force_rt == 0) { gm.rt = 2; gm.tw = 12; }
#endif
    // Short launches (a classifier chunk, an NMLL shard of a few thousand rows): one workgroup walks ALL M features of its
    // 128 rows in one serial chain -- 245 us at M = 8192 whether the launch has 2048 rows or 32768 (round 4:
    // profiles/r4_mall_probe.json), on 16 .. 256 of 256 CUs.  Below two workgroups per CU the contraction over M is split
    // across blockIdx.y so that the launch fills the chip (~512 workgroups), never finer than 512 features (16 LDS chunks:
    // the ring's fill / drain is ~3 of them); the partials are added in split order by zblock_t_reduce_kernel.
    // XGPR_ZB_SPLIT=n in the environment forces n splits (1 = the unsplit kernel; timing experiments).
    gm.msplit = 1; gm.feats_per_split = num_rffs;
    const long tiles = (n + 16 * gm.tw * gm.rt - 1) / (16 * gm.tw * gm.rt);
    long want = gm.rt == 1 ? (2 * cus + tiles - 1) / tiles : 1;
    static const int force_split = [] { const char *e = getenv("XGPR_ZB_SPLIT"); return e ? atoi(e) : 0; }();
    if (force_split >= 1) want = force_split;
    const long max_split = num_rffs / 512 > 0 ? num_rffs / 512 : 1;
    if (want > max_split) want = max_split;
    if (want > 64) want = 64;
    if (want > 1) {
        gm.feats_per_split = ((num_rffs + want - 1) / want + 127) / 128 * 128;
        gm.msplit = (int)((num_rffs + gm.feats_per_split - 1) / gm.feats_per_split);
        if (gm.msplit <= 1) { gm.msplit = 1; gm.feats_per_split = num_rffs; }
    }
    gm.tpart_bytes = gm.msplit > 1 ? (size_t)gm.msplit * n * gm.kp * sizeof(double) : 0;
    return gm;
}

enum { ZB_MATVEC = 0, ZB_PROJECT = 1, ZB_BACKPROJECT = 2 };


// mode ZB_MATVEC:      out[M, k] (+)= s^2 Zc^T (Zc in),  in = V [M, k]
// mode ZB_PROJECT:     out[n, k]  =  s Zc in,            in = V [M, k]      (T kernel only)
// mode ZB_BACKPROJECT: out[M, k] (+)= s Zc^T in,         in = R [n, k]      (W kernel + reduce)
int zcache_block_impl(int mode, const float *zc, const double *in, double *out, long n, long num_rffs, long k,
                      int fit_intercept, double scale_override, int accumulate, void *workspace, size_t wbytes,
                      void *stream) {
    if (n <= 0) return fail(XGPR_ERR_NO_DATAPOINTS, "no datapoints");
    if (num_rffs < 4 || (num_rffs & 3) != 0) return fail(XGPR_ERR_UNSUPPORTED, "block matvec needs num_rffs to be a multiple of 4");
    if (k < 1 || k > 32) return fail(XGPR_ERR_UNSUPPORTED, "block matvec takes 1..32 right-hand sides per call");
    if (!aligned16(zc)) return fail(XGPR_ERR_WORKSPACE, "cache pointer must be 16-byte aligned");
    ZbGeom gm = zb_geometry(n, num_rffs, k);
    if (mode == ZB_PROJECT) {
        // the projection uses the workspace for the partials of a split launch only (at its head); none: the unsplit kernel
        if (!workspace) { gm.msplit = 1; gm.feats_per_split = num_rffs; gm.tpart_bytes = 0; }
        else if (wbytes < gm.tpart_bytes || !aligned16(workspace))
            return fail(XGPR_ERR_WORKSPACE, "workspace too small (see xgpr_zcache_block_project_workspace_bytes)");
    } else if (!workspace || wbytes < gm.t_bytes + gm.slab_bytes + gm.tpart_bytes || !aligned16(workspace))
        return fail(XGPR_ERR_WORKSPACE, "workspace too small (see xgpr_zcache_block_workspace_bytes)");
    hipStream_t st = (hipStream_t)stream;
    ZbArgs a = {};
    a.zc = zc; a.V = in;
    a.n = n; a.M = num_rffs; a.k = (int)k; a.fit_intercept = fit_intercept;
    a.scale = scale_override > 0.0 ? scale_override : rbf_scale<float>(num_rffs / 2, fit_intercept);
    a.rows_per_range = gm.rows_per_range;
    a.ldt = gm.kp; a.tscale = 1.0;
    if (mode == ZB_MATVEC) {
        a.T = reinterpret_cast<double *>(workspace);
    } else if (mode == ZB_PROJECT) {
        a.T = out; a.ldt = k; a.tscale = a.scale;
    } else {
        a.T = const_cast<double *>(in); a.ldt = k;
    }
    if (mode != ZB_PROJECT)
        a.wpart = reinterpret_cast<double *>(reinterpret_cast<unsigned char *>(workspace) + gm.t_bytes);
    a.msplit = gm.msplit; a.feats_per_split = gm.feats_per_split;
    a.tpart = gm.msplit > 1 ? reinterpret_cast<double *>(reinterpret_cast<unsigned char *>(workspace) +
                                                         (mode == ZB_PROJECT ? 0 : gm.t_bytes + gm.slab_bytes)) : nullptr;
    const int rt = gm.rt;
    const long tblocks = (n + 16 * gm.tw * rt - 1) / (16 * gm.tw * rt);
    if (tblocks > 2147483647L || gm.nrb > 65535) return fail(XGPR_ERR_UNSUPPORTED, "too many datapoints for one launch");
    const dim3 tg((unsigned)tblocks, (unsigned)gm.msplit), wg((unsigned)gm.mblk, (unsigned)gm.nrb), blk(512);
    // 17 .. 28 right-hand sides: one 16-column tile + nb4 groups of four columns (v_mfma_f64_4x4x4_4b_f64)
    const int nb4 = (k > 16 && k <= 28) ? (int)((k - 16 + 3) / 4) : 0;
#define ZB_LAUNCH_T(CT, RT, NB) hipLaunchKernelGGL((zblock_t_kernel<CT, RT, NB>), tg, blk, 0, st, a)
#ifdef XGPR_ZB_T12
#define ZB_LAUNCH_T_RT(CT, NB) { if (gm.tw == 12) hipLaunchKernelGGL((zblock_t_kernel<CT, 2, NB, 12>), tg, dim3(768), 0, st, a); \
                                 else if (rt == 4) ZB_LAUNCH_T(CT, 4, NB); else if (rt == 2) ZB_LAUNCH_T(CT, 2, NB); else ZB_LAUNCH_T(CT, 1, NB); }
#else
#define ZB_LAUNCH_T_RT(CT, NB) { if (rt == 4) ZB_LAUNCH_T(CT, 4, NB); else if (rt == 2) ZB_LAUNCH_T(CT, 2, NB); else ZB_LAUNCH_T(CT, 1, NB); }
#endif
    if (mode != ZB_BACKPROJECT) {
        if (gm.kp == 16) ZB_LAUNCH_T_RT(1, 0)
        else if (nb4 == 1) ZB_LAUNCH_T_RT(1, 1)
        else if (nb4 == 2) ZB_LAUNCH_T_RT(1, 2)
        else if (nb4 == 3) ZB_LAUNCH_T_RT(1, 3)
        else ZB_LAUNCH_T_RT(2, 0)
        HIP_TRY(hipGetLastError(), "zblock_t_kernel launch");
        if (gm.msplit > 1) {
            const long total = n * a.ldt;
            hipLaunchKernelGGL(zblock_t_reduce_kernel, dim3((unsigned)((total + 511) / 512)), dim3(256), 0, st, a.tpart, a.T, total,
                               gm.msplit, a.tscale);
            HIP_TRY(hipGetLastError(), "zblock_t_reduce_kernel launch");
        }
    }
#undef ZB_LAUNCH_T_RT
#undef ZB_LAUNCH_T
    if (mode == ZB_PROJECT) return 0;
    if (gm.kp == 16) hipLaunchKernelGGL((zblock_w_kernel<1, 0>), wg, blk, 0, st, a);
    else if (nb4 == 1) hipLaunchKernelGGL((zblock_w_kernel<1, 1>), wg, blk, 0, st, a);
    else if (nb4 == 2) hipLaunchKernelGGL((zblock_w_kernel<1, 2>), wg, blk, 0, st, a);
    else if (nb4 == 3) hipLaunchKernelGGL((zblock_w_kernel<1, 3>), wg, blk, 0, st, a);
    else hipLaunchKernelGGL((zblock_w_kernel<2, 0>), wg, blk, 0, st, a);
    HIP_TRY(hipGetLastError(), "zblock_w_kernel launch");
    const long total = num_rffs * gm.kp;
    hipLaunchKernelGGL(reduce_block_slabs_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a.wpart, out,
                       num_rffs, gm.kp, (int)k, gm.nrb, mode == ZB_MATVEC ? a.scale * a.scale : a.scale, accumulate);
    HIP_TRY(hipGetLastError(), "reduce_block_slabs_kernel launch");
    return 0;
}

template <typename T>
int mini_ard_impl(const T *x, double *out, const T *weights, const int32_t *sigma_map, const double *sigma_vals,
                  double *grad, long n, long d, long out_rows, long num_rffs, long num_freqs, long w_cols, long map_len,
                  long sig_len, long grad_rows, long grad_cols, long num_lengthscales, int fit_intercept, void *stream) {
    if (n == 0 || out_rows != n) return fail(XGPR_ERR_NO_DATAPOINTS, "no datapoints");
    if (grad_rows != out_rows || grad_cols != num_rffs) return fail(XGPR_ERR_ARRAY_SIZES, "Wrong array sizes.");
    if (w_cols != d) return fail(XGPR_ERR_ARRAY_SIZES, "Wrong array sizes.");
    if (num_rffs != 2 * num_freqs || map_len != w_cols) return fail(XGPR_ERR_ARRAY_SIZES, "Wrong array sizes.");
    if (sig_len != map_len) return fail(XGPR_ERR_ARRAY_SIZES, "Wrong array sizes.");
    if (num_lengthscales < 1 || num_lengthscales > ARD_MAX_GROUPS)
        return fail(XGPR_ERR_UNSUPPORTED, "MiniARD gradient supports up to 8 lengthscale groups");
    const long yblocks = (n + 3) / 4;
    if (yblocks > 65535) return fail(XGPR_ERR_UNSUPPORTED, "too many datapoints for one launch (chunk the input)");
    // the constant is typed T in the reference (ard_ops.cpp:86-91)
    const double norm = (double)(T)std::sqrt(1.0 / (fit_intercept ? (double)num_freqs - 0.5 : (double)num_freqs));
    hipLaunchKernelGGL(mini_ard_grad_kernel<T>, dim3((unsigned)((num_freqs + 63) / 64), (unsigned)yblocks), dim3(256), 0,
                       (hipStream_t)stream, x, out, weights, sigma_map, sigma_vals, grad, n, d, num_freqs,
                       (int)num_lengthscales, norm);
    HIP_TRY(hipGetLastError(), "mini_ard_grad_kernel launch");
    return 0;
}

constexpr long SRHT_ZTY_MAX_BLOCKS = 512;

template <typename T>
int srht_sample_impl(const T *z, const int8_t *radem, const long *sampler, T *out, const double *y, double *zty_out,
                     long n, long m, long P, long ncols, long ldo, void *workspace, size_t wbytes, void *stream) {
    if (n <= 0 || m <= 0) return fail(XGPR_ERR_ARRAY_DIMS, "incorrect array dims passed");
    if (P < 2 || (P & (P - 1)) != 0 || m > P) return fail(XGPR_ERR_NOT_POW2, "last dim not power of 2 > 1");
    if (ncols < 1 || ncols > P || ldo < ncols) return fail(XGPR_ERR_ARRAY_DIMS, "incorrect array dims passed");
    if (P > lds_cap_elems<T>()) return fail(XGPR_ERR_UNSUPPORTED, "fused SRHT + sample needs the padded row to fit in LDS");
    const int nt = threads_for(P);
    if (P > (long)SRHT_ZTY_COLS * nt) return fail(XGPR_ERR_UNSUPPORTED, "fused SRHT + sample: padded width too large");
    long nblocks = 2L * device_cus();
    if (nblocks > n) nblocks = n;
    if (nblocks > SRHT_ZTY_MAX_BLOCKS) nblocks = SRHT_ZTY_MAX_BLOCKS;
    double *part = nullptr;
    if (y) {
        if (!zty_out) return fail(XGPR_ERR_ARRAY_DIMS, "incorrect array dims passed");
        if (!workspace || wbytes < (size_t)nblocks * m * sizeof(double) || !aligned16(workspace))
            return fail(XGPR_ERR_WORKSPACE, "workspace too small (see xgpr_srht_sample_workspace_bytes)");
        part = reinterpret_cast<double *>(workspace);
    }
    hipStream_t st = (hipStream_t)stream;
    const int rc = launch(srht_sample_kernel<T>, dim3((unsigned)nblocks), dim3(nt), (size_t)P * sizeof(T), st, "srht_sample_kernel launch", z,
                          radem, sampler, out, y, part, n, m, (int)P, ncols, ldo, norm_constant<T>(P));
    if (rc || !y) return rc;
    return reduce_slabs(part, zty_out, m, nblocks, st);
}


// ---- SRHT + sample from float32 feature rows (sketch_gemm.inc)
int srht_sample_rows_impl(const float *zc, const int8_t *radem, const long *sampler, double *out, const double *y,
                          double *zty_out, long n, long m, long P, long ncols, long ldo, double scale, int fit_intercept,
                          void *workspace, size_t wbytes, void *stream) {
    if (n <= 0 || m <= 0) return fail(XGPR_ERR_ARRAY_DIMS, "incorrect array dims passed");
    if (P < 2 || (P & (P - 1)) != 0 || m > P) return fail(XGPR_ERR_NOT_POW2, "last dim not power of 2 > 1");
    if (ncols < 1 || ncols > P || ldo < ncols) return fail(XGPR_ERR_ARRAY_DIMS, "incorrect array dims passed");
    const long PB = P > 8192 ? 8192 : P;
    const long NB = P / PB;
    if (NB > 4 || (NB > 1 && NB * ncols > 8192))
        return fail(XGPR_ERR_UNSUPPORTED, "fused SRHT + sample: padded width x sampled columns beyond the LDS budget");
    const int nt = NB > 1 ? 1024 : threads_for(PB);
    if (PB > (long)SRHT32_Q * nt) return fail(XGPR_ERR_UNSUPPORTED, "fused SRHT + sample: padded width too large");
    if (NB > 1 && y && m % 4 != 0) return fail(XGPR_ERR_UNSUPPORTED, "fused SRHT + sample with z^T y: num_rffs must be a multiple of 4");
    long nblocks = (NB > 1 ? 1L : 2L) * device_cus();
    if (nblocks > n) nblocks = n;
    if (nblocks > SRHT_ZTY_MAX_BLOCKS) nblocks = SRHT_ZTY_MAX_BLOCKS;
    double *part = nullptr;
    if (y) {
        if (!zty_out) return fail(XGPR_ERR_ARRAY_DIMS, "incorrect array dims passed");
        if (!workspace || wbytes < (size_t)SRHT_ZTY_MAX_BLOCKS * m * sizeof(double) || !aligned16(workspace))
            return fail(XGPR_ERR_WORKSPACE, "workspace too small (see xgpr_srht_sample_workspace_bytes)");
        part = reinterpret_cast<double *>(workspace);
    }
    if (scale <= 0.0) scale = rbf_scale<float>(m / 2, fit_intercept);
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)PB * sizeof(double) + (NB > 1 ? (size_t)NB * ncols * sizeof(double) : 0);
    const double nc = norm_constant<double>(P);
    // padded widths 4096 .. 16384 with 16-byte-aligned rows: the register-pass kernel (four stages per LDS round trip)
    static const bool no16 = [] { const char *e = getenv("XGPR_SRHT_RADIX4"); return e && e[0] == '1'; }();
    if (NB == 1 && !no16 && (P == 4096 || P == 8192) && m % 4 == 0 && aligned16(zc)) {
        const size_t lds16 = (size_t)(P / 16 + P / 256) * 16 * sizeof(double);
        long nb16 = (lds16 * 2 <= 160 * 1024 ? 2L : 1L) * device_cus();
        if (nb16 > n) nb16 = n;
        if (nb16 > SRHT_ZTY_MAX_BLOCKS) nb16 = SRHT_ZTY_MAX_BLOCKS;
        auto go = [&](auto kern) {
            return launch(kern, dim3((unsigned)nb16), dim3((unsigned)(P / 16)), lds16, st, "srht_sample_rows16_kernel launch", zc, radem, sampler,
                          out, y, part, n, m, ncols, ldo, nc, scale, fit_intercept);
        };
        const int rc = P == 4096 ? go(srht_sample_rows16_kernel<12>) : go(srht_sample_rows16_kernel<13>);
        if (rc || !y) return rc;
        return reduce_slabs(part, zty_out, m, nb16, st);
    }
    // rows of 2 or 4 blocks of 8192 with at most 2048 sampled columns: the register passes block by block
    const bool blocks16 = NB > 1 && !no16 && PB == 8192 && ldo <= 2048 && m % 4 == 0 && aligned16(zc) && aligned16(radem);
    if (blocks16) {
        const size_t lds16 = (size_t)(PB / 16 + PB / 256) * 16 * sizeof(double);
        long nb16 = 2L * device_cus();
        if (nb16 > n) nb16 = n;
        auto go = [&](auto kern) {
            return launch(kern, dim3((unsigned)nb16), dim3(512), lds16, st, "srht_sample_rows16_blocks_kernel launch", zc, radem, sampler, out, n, m,
                          ncols, ldo, nc, scale, fit_intercept);
        };
        const int rc = NB == 2 ? go(srht_sample_rows16_blocks_kernel<2>) : go(srht_sample_rows16_blocks_kernel<4>);
        if (rc) return rc;
    } else {
        auto go = [&](auto kern) {
            return launch(kern, dim3((unsigned)nblocks), dim3(nt), lds, st, "srht_sample_rows_kernel launch", zc, radem, sampler, out, y, part, n, m,
                          (int)PB, ncols, ldo, nc, scale, fit_intercept);
        };
        const int rc = NB == 1 ? go(srht_sample_rows_kernel<1>) : NB == 2 ? go(srht_sample_rows_kernel<2>) : go(srht_sample_rows_kernel<4>);
        if (rc) return rc;
    }
    if (y) {
        long nslabs = nblocks;
        if (NB > 1) {
            // z^T y of the block-by-block case: row ranges x feature blocks, then the same ordered slab reduction
            nslabs = (n + 1023) / 1024;
            if (nslabs > SRHT_ZTY_MAX_BLOCKS) nslabs = SRHT_ZTY_MAX_BLOCKS;
            const long rpr = (n + nslabs - 1) / nslabs;
            nslabs = (n + rpr - 1) / rpr;
            hipLaunchKernelGGL(rows_zty_kernel, dim3((unsigned)((m / 4 + 255) / 256), (unsigned)nslabs), dim3(256), 0, st, zc, y,
                               part, n, m, rpr, scale, fit_intercept);
            HIP_TRY(hipGetLastError(), "rows_zty_kernel launch");
        }
        return reduce_slabs(part, zty_out, m, nslabs, st);
    }
    return 0;
}

// ---- the matrix-core contraction over float32 feature rows (sketch_gemm.inc)
struct SkGeom { int tiles_i, tiles_j, tmb; long nsplit, k_per_split; long slab_stride; size_t ws_bytes; long nwg; };

SkGeom sk_geometry(long I, long J, long K, long ldc, int trans_out) {
    SkGeom gm;
    gm.tiles_i = (int)((I + SK_TI - 1) / SK_TI);
    gm.tiles_j = (int)((J + 127) / 128);
    // a block of the tile map = tmb column tiles x all row tiles ~ one workgroup per CU, tmb a multiple of 8 (XCDs)
    long tmb = (SK_ET == 2 ? 2L : 1L) * device_cus() / gm.tiles_i;     // one block of the map ~ the resident workgroups
    tmb = tmb / 8 * 8;
    if (tmb < 8) tmb = 8;
    gm.tmb = (int)tmb;
    const long blocks = (gm.tiles_j + tmb - 1) / tmb;
    gm.nwg = blocks * tmb * gm.tiles_i;
    static const bool alt_map = [] { const char *e = getenv("XGPR_SK_MAP"); return e && e[0] == '1'; }();
    if (alt_map) { gm.tmb = -1; gm.nwg = (long)(gm.tiles_j + 7) / 8 * 8 * gm.tiles_i; }
    const long tiles = (long)gm.tiles_i * gm.tiles_j;
    // two workgroups per CU (four waves per SIMD for the LDS-staged kernel): contraction ranges make up the count
    long nsplit = 1;
    if (tiles < 2L * device_cus()) nsplit = (2L * device_cus() + tiles - 1) / tiles;
    static const long force_split = [] { const char *e = getenv("XGPR_SK_SPLIT"); return e ? atol(e) : 0L; }();
    if (force_split > 0) nsplit = force_split;
    // Long contraction ranges let the workgroups that share operand tiles through an XCD's L2 (the row tiles of one column
    // tile; the readers of one A tile) drift apart over thousands of chunks, until the later one misses: at cfg3's window
    // 2 ranges fetch 12.7 GB through the fabric, 16 ranges 9.6, 32 ranges 8.9 (algorithmic 4.9; floor of this decomposition
    // with eight non-coherent L2s: Z once + A once per XCD = 8.6) at the same 75.5-75.8 TFLOP/s (tools/sk_split_ab.sh).
    // So: ranges of ~8192 datapoints, as long as the partial-result slabs stay within 1 GiB.
    if (force_split <= 0) {
        const long by_len = K / 8192, slab_bytes = (trans_out ? J : I) * ldc * 8;
        long by_mem = slab_bytes > 0 ? (1L << 30) / slab_bytes : 1;
        if (by_mem < 1) by_mem = 1;
        const long want = by_len < by_mem ? by_len : by_mem;
        if (want > nsplit) nsplit = want;
    }
    const long max_split = (K + 255) / 256;                 // at least 256 contraction indices per range
    if (nsplit > max_split) nsplit = max_split;
    if (nsplit < 1) nsplit = 1;
    gm.k_per_split = ((K + nsplit - 1) / nsplit + 15) / 16 * 16;
    gm.nsplit = (K + gm.k_per_split - 1) / gm.k_per_split;
    gm.slab_stride = (trans_out ? J : I) * ldc;
    // one range and no accumulation could store straight into C; the slab keeps one code path (and C untouched
    // until the ordered reduction)
    gm.ws_bytes = (size_t)gm.nsplit * gm.slab_stride * sizeof(double);
    return gm;
}

int sketch_gemm_impl(const double *A, long lda, const float *zc, long n, long num_rffs, double *C, long ldc, long I,
                     int bt, int trans_out, double scale, int fit_intercept, int accumulate, void *workspace,
                     size_t wbytes, void *stream) {
    if (n <= 0 || num_rffs < 2 || I < 1) return fail(XGPR_ERR_ARRAY_DIMS, "incorrect array dims passed");
    if ((num_rffs & 1) != 0) return fail(XGPR_ERR_ODD_OUTPUT, "last dim of output must be even number");
    if (lda < I || lda % 64 != 0) return fail(XGPR_ERR_ARRAY_DIMS, "sketch gemm: lda must be a multiple of 64 >= I");
    if (bt && num_rffs % 4 != 0) return fail(XGPR_ERR_UNSUPPORTED, "sketch gemm (bt): num_rffs must be a multiple of 4");
    const long J = bt ? n : num_rffs, K = bt ? num_rffs : n;
    if (ldc < (trans_out ? I : J) || (!trans_out && ldc % 2 != 0))
        return fail(XGPR_ERR_ARRAY_DIMS, "sketch gemm: ldc too small (or odd for a row-major result)");
    if (!aligned16(A) || !aligned16(zc) || !aligned16(C)) return fail(XGPR_ERR_WORKSPACE, "pointers must be 16-byte aligned");
    const SkGeom gm = sk_geometry(I, J, K, ldc, trans_out);
    if (!workspace || wbytes < gm.ws_bytes || !aligned16(workspace))
        return fail(XGPR_ERR_WORKSPACE, "workspace too small (see xgpr_sketch_gemm_workspace_bytes)");
    if (gm.nwg > 2147483647L || gm.nsplit > 65535) return fail(XGPR_ERR_UNSUPPORTED, "sketch gemm: problem too large for one launch");
    if (scale <= 0.0) scale = rbf_scale<float>(num_rffs / 2, fit_intercept);
    hipStream_t st = (hipStream_t)stream;
    SkArgs a = {};
    a.A = A; a.lda = lda; a.zc = zc; a.ldz = num_rffs; a.C = reinterpret_cast<double *>(workspace); a.ldc = ldc;
    a.I = I; a.J = J; a.K = K; a.k_per_split = gm.k_per_split; a.slab_stride = gm.slab_stride; a.nfeat = num_rffs;
    a.scale = scale; a.fit_intercept = fit_intercept; a.tiles_j = gm.tiles_j; a.tiles_i = gm.tiles_i; a.tmb = gm.tmb;
    const dim3 grid((unsigned)gm.nwg, (unsigned)gm.nsplit), blk(512);
    // contract datapoints over full 128 x 128 tiles: operand tiles shared through LDS (sketch_gemm_lds_kernel); the
    // rows beyond the last multiple of 16 of a single range follow through the direct kernel.  XGPR_SK_DIRECT=1 keeps
    // the direct kernel everywhere (timing comparisons).
    static const bool direct_only = [] { const char *e = getenv("XGPR_SK_DIRECT"); return e && e[0] == '1'; }();
    const bool lds_ok = !bt && !direct_only && J % 128 == 0 && lda % 128 == 0 && aligned16(zc) && num_rffs % 4 == 0 &&
                        (gm.nsplit > 1 ? true : K >= 16);
    if (lds_ok) {
        const long k16 = gm.nsplit > 1 ? K : K / 16 * 16;           // ranges are multiples of 16 by construction ...
        SkArgs al = a;
        al.K = k16;
        if (gm.nsplit > 1 && K % 16 != 0) al.K = K / 16 * 16;       // ... except the end of the last one
        const int rc = dispatch_bool(trans_out != 0, [&](auto TR) {
            return launch(sketch_gemm_lds_kernel<decltype(TR)::value>, grid, blk, 2 * SKL_BUF_BYTES, st, "sketch_gemm_lds_kernel launch", al);
        });
        if (rc) return rc;
        const long nrows_ = trans_out ? J : I, ncols_ = trans_out ? I : J;
        hipLaunchKernelGGL(sk_reduce_kernel, dim3((unsigned)((nrows_ * ncols_ + 255) / 256)), dim3(256), 0, st, a.C, C, nrows_,
                           ncols_, ldc, gm.slab_stride, (int)gm.nsplit, accumulate);
        HIP_TRY(hipGetLastError(), "sk_reduce_kernel launch");
        const long tail = K - al.K;
        if (tail == 0) return 0;
        // the last K % 16 datapoints: one more (tiny) contraction, accumulated
        return sketch_gemm_impl(A + al.K * lda, lda, zc + al.K * num_rffs, tail, num_rffs, C, ldc, I, 0, trans_out, scale,
                                fit_intercept, 1, workspace, wbytes, stream);
    }
    // contract features: the LDS-staged form needs whole 16-feature chunks and a row pitch of Q that covers full tiles
    const bool lds_bt_ok = bt && !direct_only && lda % 128 == 0 && K % 16 == 0 && gm.k_per_split % 16 == 0 &&
                           num_rffs * 64 < 2147483647L;
    // (all three forms report a failed launch under the same name)
    const int rc = dispatch_bool(trans_out != 0, [&](auto TR) {
        if (lds_bt_ok) return launch(sketch_gemm_lds_bt_kernel<decltype(TR)::value>, grid, blk, 2 * SKB_BUF_BYTES, st, "sketch_gemm_kernel launch", a);
        return dispatch_bool(bt != 0, [&](auto BT) {
            return launch(sketch_gemm_kernel<decltype(BT)::value, decltype(TR)::value>, grid, blk, 0, st, "sketch_gemm_kernel launch", a);
        });
    });
    if (rc) return rc;
    const long nrows = trans_out ? J : I, ncols = trans_out ? I : J;
    hipLaunchKernelGGL(sk_reduce_kernel, dim3((unsigned)((nrows * ncols + 255) / 256)), dim3(256), 0, st, a.C, C, nrows, ncols,
                       ldc, gm.slab_stride, (int)gm.nsplit, accumulate);
    HIP_TRY(hipGetLastError(), "sk_reduce_kernel launch");
    return 0;
}

// ---- Z^T Z on the matrix cores from float32 feature rows (gram.inc)
long gram_workgroups(long msub, long n) {
    const long T = msub / 128, total = T * (T + 1) / 2 * (n / 16);
    long nwg = 2L * device_cus();                     // two 512-thread workgroups per CU (four waves per SIMD)
    if (nwg > total) nwg = total;
    return nwg > 0 ? nwg : 1;
}
size_t gram_workspace_bytes(long msub, long n) { return (size_t)gram_workgroups(msub, n) * 128 * 128 * sizeof(double); }

int gram_impl(const float *zc, long n, long num_rffs, double *C, long ldc, long msub, double scale, int fit_intercept,
              int accumulate, void *workspace, size_t wbytes, void *stream) {
    if (n <= 0 || num_rffs < 2 || msub < 1 || msub > num_rffs) return fail(XGPR_ERR_ARRAY_DIMS, "incorrect array dims passed");
    if ((num_rffs & 1) != 0) return fail(XGPR_ERR_ODD_OUTPUT, "last dim of output must be even number");
    if (msub % 128 != 0 || num_rffs % 4 != 0) return fail(XGPR_ERR_UNSUPPORTED, "gram: msub must be a multiple of 128 and num_rffs of 4");
    if (ldc < msub || ldc % 2 != 0) return fail(XGPR_ERR_ARRAY_DIMS, "gram: ldc must be even and >= msub");
    if (!aligned16(zc) || !aligned16(C)) return fail(XGPR_ERR_WORKSPACE, "pointers must be 16-byte aligned");
    if (!workspace || wbytes < gram_workspace_bytes(msub, n) || !aligned16(workspace))
        return fail(XGPR_ERR_WORKSPACE, "workspace too small (see xgpr_ztz_gram_workspace_bytes)");
    if (scale <= 0.0) scale = rbf_scale<float>(num_rffs / 2, fit_intercept);
    hipStream_t st = (hipStream_t)stream;
    GramArgs a = {};
    a.zc = zc; a.ldz = num_rffs; a.C = C; a.ldc = ldc; a.nchunks = n / 16;
    a.T = (int)(msub / 128); a.ntiles = (long)a.T * (a.T + 1) / 2;
    a.spill = reinterpret_cast<double *>(workspace);
    a.scale = scale; a.fit_intercept = fit_intercept; a.accumulate = accumulate;
    if (a.nchunks > 0) {
        const long total = a.ntiles * a.nchunks;
        long nwg = gram_workgroups(msub, n);
        a.units_per_wg = (total + nwg - 1) / nwg;
        nwg = (total + a.units_per_wg - 1) / a.units_per_wg;
        int rc = launch(gram_lds_kernel, dim3((unsigned)nwg), dim3(512), GR_LDS, st, "gram_lds_kernel launch", a);
        if (rc) return rc;
        rc = launch(gram_fixup_kernel, dim3((unsigned)a.ntiles), dim3(256), 0, st, "gram_fixup_kernel launch", a, nwg);
        if (rc) return rc;
    } else if (!accumulate) {          // fewer rows than one chunk: the tail kernel adds into zeros (the padding columns stay untouched)
        HIP_TRY(hipMemset2DAsync(C, (size_t)ldc * sizeof(double), 0, (size_t)msub * sizeof(double), (size_t)msub, st), "gram: clearing C");
    }
    const int tail = (int)(n % 16);
    if (tail > 0) {
        hipLaunchKernelGGL(gram_tail_kernel, dim3((unsigned)((msub + 255) / 256), (unsigned)msub), dim3(256), 0, st,
                           zc + (n - tail) * num_rffs, num_rffs, tail, C, ldc, msub, scale, fit_intercept);
        HIP_TRY(hipGetLastError(), "gram_tail_kernel launch");
    }
    return 0;
}

// ---- A^T B + B^T A on the matrix cores from two float32 row arrays (cross_gram.inc)
long cross_gram_workgroups(long M, long n) {
    const long T = M / 128, total = T * (T + 1) / 2 * 2 * (n / 16);
    long nwg = 2L * device_cus();                     // two 512-thread workgroups per CU, as gram_workgroups
    if (nwg > total) nwg = total;
    return nwg > 0 ? nwg : 1;
}
size_t cross_gram_workspace_bytes(long M, long n) { return (size_t)cross_gram_workgroups(M, n) * 128 * 128 * sizeof(double); }

int cross_gram_impl(const float *A, const float *B, long n, long num_rffs, double *C, long ldc, int accumulate, void *workspace,
                    size_t wbytes, void *stream) {
    const long M = num_rffs;
    if (n <= 0 || M < 2) return fail(XGPR_ERR_ARRAY_DIMS, "incorrect array dims passed");
    if (M % 128 != 0) return fail(XGPR_ERR_UNSUPPORTED, "cross gram: num_rffs must be a multiple of 128");
    if (ldc < M || ldc % 2 != 0) return fail(XGPR_ERR_ARRAY_DIMS, "cross gram: ldc must be even and >= num_rffs");
    if (!A || !B || !aligned16(A) || !aligned16(B) || !aligned16(C)) return fail(XGPR_ERR_WORKSPACE, "pointers must be 16-byte aligned");
    if (!workspace || wbytes < cross_gram_workspace_bytes(M, n) || !aligned16(workspace))
        return fail(XGPR_ERR_WORKSPACE, "workspace too small (see xgpr_cross_gram_workspace_bytes)");
    hipStream_t st = (hipStream_t)stream;
    CrossGramArgs a = {};
    a.A = A; a.B = B; a.ld = M; a.C = C; a.ldc = ldc; a.nchunks = n / 16;
    a.T = (int)(M / 128); a.ntiles = (long)a.T * (a.T + 1) / 2;
    a.spill = reinterpret_cast<double *>(workspace);
    a.accumulate = accumulate;
    if (a.nchunks > 0) {
        const long total = a.ntiles * 2 * a.nchunks;
        long nwg = cross_gram_workgroups(M, n);
        a.units_per_wg = (total + nwg - 1) / nwg;
        nwg = (total + a.units_per_wg - 1) / a.units_per_wg;
        int rc = launch(cross_gram_lds_kernel, dim3((unsigned)nwg), dim3(512), GR_LDS, st, "cross_gram_lds_kernel launch", a);
        if (rc) return rc;
        // gram_fixup_kernel as it is: a tile here is a run of 2 nchunks units, its slabs are whole (mirrored) tiles
        GramArgs f = {};
        f.C = C; f.ldc = ldc; f.nchunks = 2 * a.nchunks; f.T = a.T; f.ntiles = a.ntiles; f.units_per_wg = a.units_per_wg;
        f.spill = a.spill;
        rc = launch(gram_fixup_kernel, dim3((unsigned)a.ntiles), dim3(256), 0, st, "gram_fixup_kernel (cross gram) launch", f, nwg);
        if (rc) return rc;
    } else if (!accumulate) {          // fewer rows than one chunk: the tail kernel adds into zeros
        HIP_TRY(hipMemset2DAsync(C, (size_t)ldc * sizeof(double), 0, (size_t)M * sizeof(double), (size_t)M, st), "cross gram: clearing C");
    }
    const int tail = (int)(n % 16);
    if (tail > 0) {
        hipLaunchKernelGGL(cross_gram_tail_kernel, dim3((unsigned)((M + 255) / 256), (unsigned)M), dim3(256), 0, st,
                           A + (n - tail) * M, B + (n - tail) * M, M, tail, C, ldc, M);
        HIP_TRY(hipGetLastError(), "cross_gram_tail_kernel launch");
    }
    return 0;
}
