"""Host-side counterparts of the reference's kernel objects for the hot path.

Mirrors (paths relative to /root/reference/src/xGPR/kernels/):
  * ``KernelBaseclass`` transform_x / transform_x_y          kernel_baseclass.py:269-324
  * ``SORFKernelBaseclass`` (RBF, Matern, Cauchy)             basic_kernels/sorf_kernel_baseclass.py:36-126,
                                                              matern.py:26-58, cauchy.py:21-45
  * ``ConvKernelBaseclass`` (Conv1d*/Graph* RBF/Matern/Cauchy) convolution_kernels/conv_kernel_baseclass.py:41-147
  * ``SRHTCompressor``                                        srht_compressor.py:37-97

The random draws (Rademacher diagonals, chi / chi-square / exponential samples, the SRHT
column permutation) are made on the host with exactly the numpy / scipy calls the reference
makes -- they are *inputs* of the GPU path and must be bit-identical (tests/golden/g6_draws.npz).
Everything that touches datapoints runs in libxgpr_hip.so on the device.
"""
from math import ceil

import numpy as np
import torch
from scipy.stats import chi as _chi

from . import xgpr_hip_rfgen_ext as ext
from .dataset import TokenBatch


def padded_dims(width):
    return 2 ** ceil(np.log2(max(width, 2)))


def scale_input(x, sigma, out_dtype=torch.float32):
    """``input_x *= self.hyperparams[1]`` (sorf_kernel_baseclass.py:117) on a private copy.
    hyperparams[1] is an np.float64 *scalar*: under numpy >= 2 (NEP 50, the version the golden
    vectors were produced with) the product is formed in float64 and rounded back to the
    array's dtype."""
    return (x.to(torch.float64) * float(sigma)).to(out_dtype).contiguous()


class KernelBase:
    """State shared by all hot-path kernels (kernel_baseclass.py:49-99)."""

    def __init__(self, num_rffs, xdim, kernel_spec_parms=None, device="cuda"):
        kernel_spec_parms = kernel_spec_parms or {}
        if num_rffs < 2:
            raise RuntimeError("num_rffs should always be >= 2.")
        if not (num_rffs / 2).is_integer():
            raise RuntimeError("For sine-cosine kernels (e.g. matern, rbf) the number of random "
                               "fourier features must be an integer multiple of two.")
        self.num_freqs = int(num_rffs / 2)
        self.num_rffs = int(num_rffs)
        self.kernel_spec_parms = dict(kernel_spec_parms)
        self.random_seed = 123           # subclasses overwrite it with the seed they draw with
        self.fit_intercept = kernel_spec_parms.get("intercept", True) is not False
        self._xdim = tuple(xdim)
        self.hyperparams = np.ones((2))
        self.device = device
        self.double_precision = False

    # ---- hyperparameters (kernel_baseclass.py:219-266)
    def get_hyperparams(self, logspace=True):
        return np.log(self.hyperparams) if logspace else self.hyperparams

    def set_hyperparams(self, hyperparams, logspace=True):
        self.hyperparams = np.exp(hyperparams) if logspace else np.asarray(hyperparams, dtype=np.float64)

    def get_lambda(self):
        return self.hyperparams[0]

    def get_num_rffs(self):
        return self.num_rffs

    def _to_device(self, radem, chi_arr):
        self.radem_diag = torch.from_numpy(np.ascontiguousarray(radem)).to(self.device)
        self.chi_arr = torch.from_numpy(np.ascontiguousarray(chi_arr)).to(self.device)

    def _as_device(self, input_x):
        if isinstance(input_x, np.ndarray):
            input_x = torch.from_numpy(np.ascontiguousarray(input_x))
        if isinstance(input_x, TokenBatch):          # the float64 operators take the dense array: a chunk of it is small and transient
            return input_x.to(self.device).dense()
        return input_x.to(self.device)

    def _as_device_f32(self, input_x):
        """the private float32 copy every transform starts from (kernel_baseclass.py:274-288): float64 inputs
        are rounded to float32 BEFORE sigma is applied, as the reference does"""
        return self._as_device(input_x).to(torch.float32)

    def scaled_f32(self, input_x):
        """The private float32 copy of a chunk multiplied by sigma, on the device (what every transform starts from); a
        TokenBatch keeps its tokens and has its table scaled -- elementwise the same values."""
        if isinstance(input_x, TokenBatch):
            return input_x.to(self.device).scaled(self.hyperparams[1])
        return scale_input(self._as_device_f32(input_x), self.hyperparams[1])

    def transform_x(self, input_x, sequence_length=None):
        """kernel_baseclass.py:269-299: private float32 copy -> kernel_specific_transform ->
        ``xtrans[:, 0] = 1`` when fitting an intercept.  Returns a float64 device tensor."""
        xin = scale_input(self._as_device_f32(input_x), self.hyperparams[1])
        xtrans = self.kernel_specific_transform(xin, sequence_length)
        if self.fit_intercept:
            xtrans[:, 0] = 1.
        return xtrans

    def gradient_x(self, input_x, sequence_length=None):
        """kernel_baseclass.py:328-361: features and d(features)/d(sigma) from the *unscaled* input
        (the gradient operators apply sigma themselves).  Returns float64 [n, M], [n, M, 1]."""
        xin = self._as_device_f32(input_x).to(torch.float32, copy=True).contiguous()
        xtrans, xgrad = self.kernel_specific_gradient(xin, sequence_length)
        if self.fit_intercept:
            xtrans[:, 0] = 1.
            xgrad[:, 0, :] = 0.
        return xtrans, xgrad

    def gradient_x_y(self, input_x, input_y, sequence_length=None):
        """kernel_baseclass.py:364-377."""
        xtrans, dz_dsigma = self.gradient_x(input_x, sequence_length)
        if isinstance(input_y, np.ndarray):
            input_y = torch.from_numpy(input_y)
        return xtrans, dz_dsigma, input_y.to(self.device, torch.float64)

    def transform_x_y(self, input_x, input_y, sequence_length=None):
        """kernel_baseclass.py:303-324 (regression branch)."""
        xtrans = self.transform_x(input_x, sequence_length)
        if isinstance(input_y, np.ndarray):
            input_y = torch.from_numpy(input_y)
        return xtrans, input_y.to(self.device, torch.float64)

    # the weights argument of the input-gradient methods (SORFKernel, ConvSORFKernel)
    def _input_grad_weights(self, weights, w_cols, n):
        w = weights if isinstance(weights, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(weights))
        w = w.to(self.device, torch.float64)
        if w.dim() not in (1, 2) or (w.dim() == 2 and w.shape[0] != n):
            raise RuntimeError("weights must be one vector, or one row per datapoint.")
        if w.dim() == 1 or w.stride(1) != 1:
            w = w.contiguous()
        w_cols = min(w.shape[-1], self.num_rffs) if w_cols is None else int(w_cols)
        if w_cols < 2 or w_cols % 2 or w_cols > min(w.shape[-1], self.num_rffs):
            raise RuntimeError("w_cols must be even, >= 2 and within the weights and the features.")
        return w, w_cols


def composed_input_gradient(x_scaled, weights, w_cols, radem_diag, chi_arr, num_rffs, fit_intercept, sigma, scale):
    """d/dx of ``features(x) @ weights`` for rows ``x_scaled`` [n, d] (float32, already multiplied by sigma) from existing device
    operators, at every width: float64 features with the intercept OFF (with it on, column 0 no longer holds cos p_0) rescaled
    from the operator's float-typed constant to ``scale``, chi (.) u zero-padded to whole transforms, three rounds of
    { FHT ; signs x normaliser } in the order 2, 1, 0 as ``MiniARDKernel.precompute_weights`` applies them to the identity, the
    sum over the transforms and the product with sigma.  ``weights`` one vector or one row per row of ``x_scaled``; under
    ``fit_intercept`` column 0 carries no weight."""
    n, d = x_scaled.shape
    nf, p = num_rffs // 2, padded_dims(d)
    nblocks = radem_diag.shape[2] // p
    z = torch.empty((n, num_rffs), dtype=torch.float64, device=x_scaled.device)
    ext.hipRBFFeatureGen(x_scaled, z, radem_diag, chi_arr, False)
    z *= scale / float(np.float32(np.sqrt(1.0 / nf)))
    h = w_cols // 2
    wc, ws = weights[..., 0:w_cols:2].clone(), weights[..., 1:w_cols:2]
    if fit_intercept:
        wc[..., 0] = 0.
    t = torch.zeros((n, nblocks * p), dtype=torch.float64, device=x_scaled.device)
    t[:, :h] = (ws * z[:, 0:w_cols:2] - wc * z[:, 1:w_cols:2]) * chi_arr[:h].to(torch.float64)
    return (transposed_sorf_rows(t, radem_diag, p)[:, :d] * sigma).contiguous()


def transposed_sorf_rows(t, radem_diag, p):
    """The backward half of ``composed_input_gradient``, shared with ``Conv1dTwoLayerKernel.first_layer_gradient_composed``:
    ``t`` [n, nblocks * p] float64 holds chi (.) u zero-padded to whole transforms; three rounds of { FHT ; signs x normaliser }
    in the order 2, 1, 0, then the sum over the transforms -> [n, p]."""
    n, nblocks = t.shape[0], t.shape[1] // p
    t = t.reshape(n * nblocks, p)
    norm_constant = 1.0 / (2.0 ** (np.log2(p) / 2.0))
    radem = radem_diag.to(torch.float64)
    for r in (2, 1, 0):
        ext.hipFastHadamardTransform2D(t)
        t = (t.view(n, nblocks, p) * (radem[r, 0].view(1, nblocks, p) * norm_constant)).reshape(n * nblocks, p)
    return t.view(n, nblocks, p).sum(dim=1)


class SORFKernel(KernelBase):
    """RBF / Matern / Cauchy on fixed-length vectors."""

    def __init__(self, kernel_choice, xdim, num_rffs, random_seed=123, device="cuda",
                 kernel_spec_parms=None):
        kernel_spec_parms = kernel_spec_parms or {}
        super().__init__(num_rffs, xdim, kernel_spec_parms, device)
        self.random_seed = random_seed
        if len(xdim) != 2:
            raise ValueError("The dimensionality of the input is inappropriate for "
                             "the kernel you have selected.")
        self.kernel_choice = kernel_choice
        pdims = padded_dims(xdim[-1])
        radem_array = np.asarray([-1, 1], dtype=np.int8)
        rng = np.random.default_rng(random_seed)
        nblocks = ceil(self.num_freqs / pdims) if pdims < self.num_freqs else 1
        radem = rng.choice(radem_array, size=(3, 1, nblocks * pdims), replace=True)
        chi_arr = _chi.rvs(df=pdims, size=self.num_freqs, random_state=random_seed).astype(np.float32)
        chi_arr = _rescale_chi(kernel_choice, chi_arr, random_seed, kernel_spec_parms, self)
        self._to_device(radem, chi_arr)

    def kernel_specific_transform(self, input_x, sequence_length=None):
        """sorf_kernel_baseclass.py:104-126; ``input_x`` is already sigma-scaled here."""
        output_x = torch.empty((input_x.shape[0], self.num_rffs), dtype=torch.float64, device=self.device)
        ext.hipRBFFeatureGen(input_x, output_x, self.radem_diag, self.chi_arr, self.fit_intercept)
        return output_x

    def kernel_specific_gradient(self, input_x, sequence_length=None):
        """sorf_kernel_baseclass.py:136-162."""
        n = input_x.shape[0]
        output_x = torch.zeros((n, self.num_rffs), dtype=torch.float64, device=self.device)
        dz_dsigma = torch.zeros((n, self.num_rffs, 1), dtype=torch.float64, device=self.device)
        ext.hipRBFGrad(input_x, output_x, dz_dsigma, self.radem_diag, self.chi_arr,
                       float(self.hyperparams[1]), self.fit_intercept)
        return output_x, dz_dsigma

    # ---- fused per-shard reductions (what the reference does chunk by chunk with a
    # materialised Z: fitting_toolkit/cg_tools.py:189-191, scoring_toolkit/exact_nmll_calcs.py:35-37)
    supports_fused = True

    def ztz_matvec(self, x_scaled, vec, out, workspace=None, masks_packed=False):
        ext.hipZtZMatvec(x_scaled, self.radem_diag, self.chi_arr, vec, out, self.fit_intercept, workspace, masks_packed)

    def zty(self, x_scaled, y, out, workspace=None):
        ext.hipZtY(x_scaled, self.radem_diag, self.chi_arr, y, out, self.fit_intercept, workspace)

    # ---- resident feature cache: keep the shard's Z in HBM as float32 (cos, sin) pairs and stream
    # it on every CG iteration instead of regenerating it (an option the 288 GB of HBM3E allow;
    # the reference cannot hold Z and regenerates it, cg_tools.py:189-191)
    def cache_ok(self):
        """k = 1 streaming kernel up to num_freqs = 16384 (a workgroup holds all tiles of a datapoint: one tile
        per wave up to 8192, two beyond); past that the resident cache is applied through the two block
        contractions with one column."""
        return self.rows_ok() and (self.num_freqs <= 16384 or self.block_ok())

    def cache_pays(self):
        """Whether streaming the resident cache beats regenerating the features in a k = 1 solve: the launcher's own
        predicate (xgpr_ztz_matvec_plan).  On the three-wave single-pass kernel regenerating a 1024-frequency tile takes
        ~1.30 ns (cfg3: 5.19 ms per 1e6 rows) while the cache streams it in ~1.33 ns (32.8 GB at 6.2 TB/s: 5.32 ms) --
        regenerating wins or ties (cfg2: 0.32 / 0.33 ms) and leaves the HBM free.  Every other plan loses to the stream:
        the two-wave kernel (one tile per datapoint at padded width >= 128, seven tiles), the two feature passes (eight
        tiles per datapoint, or more than 8192 frequencies; cfg5's share: 9.1 / 6.1 ms) and the wide transforms of padded
        width 2048 / 4096 (cross-wave stages: slower per tile than the stream).  bench.py reports both modes
        (`cached_z_mode`)."""
        return ext.ztz_matvec_plan(self._xdim[-1], self.num_freqs) != 1 or padded_dims(self._xdim[-1]) > 1024

    def build_feature_cache(self, dataset):
        x_scaled = dataset.scaled_x(self.hyperparams[1])
        zc = torch.empty((x_scaled.shape[0], self.num_rffs), dtype=torch.float32, device=self.device)
        ext.hipRBFFeatureCache(x_scaled, zc, self.radem_diag, self.chi_arr)
        return zc

    def ztz_matvec_cached(self, zcache, vec, out, workspace):
        if self.num_freqs <= 16384:
            ext.hipZCacheMatvec(zcache, vec, out, self.fit_intercept, workspace)
            return
        need = block_workspace_bytes(zcache.shape[0], self.num_rffs, 1)
        if getattr(self, "_cache_bws", None) is None or self._cache_bws.numel() < need:
            self._cache_bws = torch.empty(need, dtype=torch.uint8, device=zcache.device)
        ext.hipZCacheBlockMatvec(zcache, vec[:, None], out[:, None], self.fit_intercept, self._cache_bws)

    # ---- the resident cache as IEEE binary16 rows (cache_features="half", opt-in): half the bytes per iteration and per
    # shard; the solve is ridge regression on the features rounded to 11 significant bits
    def half_cache_ok(self):
        """Whether the k <= 2 matvec can stream this kernel's rows rounded to binary16: a HIP device, ``rows_ok`` and one tile
        per wave (num_freqs <= 8192)."""
        return torch.device(self.device).type == "cuda" and self.rows_ok() and ext.half_cache_ok(self.num_freqs)

    def ztz_matvec_cached_f16(self, zc16, vec, out, workspace):
        ext.hipZCacheMatvecHalf(zc16, vec, out, self.fit_intercept, workspace)

    # ---- block of right-hand sides (approximate-NMLL probes, k = 26): float64 matrix cores over
    # the float32 cache, either the resident one or a window of rows regenerated into scratch
    def block_ok(self):
        """The block operators read float32 rows: regenerated ones wherever ``rows_ok`` (and, at padded width <= 4096 with
        more than 65536 frequencies, float64 feature chunks rounded to float32); they need num_rffs % 4 == 0."""
        return (self.rows_ok() or padded_dims(self._xdim[-1]) <= FUSED_MAX_WIDTH) and self.num_rffs % 4 == 0

    def fill_feature_cache(self, x_scaled, zcache):
        ext.hipRBFFeatureCache(x_scaled, zcache, self.radem_diag, self.chi_arr)

    def rows_ok(self):
        """Whether ``fill_feature_cache`` can write this kernel's float32 rows: wherever the fused kernels run (padded
        width <= 4096), and at every wider padded width up to 65536 frequencies (wave tiles at 8192, the any-width
        path beyond).  There the solver's passes read regenerated rows or the resident cache instead of float64 Z."""
        return self.fused_ok() or (padded_dims(self._xdim[-1]) > FUSED_MAX_WIDTH and self.num_freqs <= 65536)

    def grad_rows_ok(self):
        """Whether ``fill_grad_rows`` can write this kernel's float32 feature AND gradient rows, and the exact NMLL
        gradient's accumulations can run on them (nmll.calc_gradient_terms): a HIP device, ``rows_ok``, padded width up
        to 8192 (wider inputs keep the float64 gradient operator) and whole 128 x 128 tiles for the two Gram kernels."""
        return (torch.device(self.device).type == "cuda" and self.rows_ok()
                and padded_dims(self._xdim[-1]) <= ext.GRAD_ROWS_MAX_WIDTH and ext.cross_gram_ok(self.num_rffs)
                and self.radem_diag.data_ptr() % 16 == 0)

    def fill_grad_rows(self, x_unscaled, zrows, grows):
        """zrows, grows [w, M] float32 <- the complete feature rows and d(features)/d(sigma) rows of the UNSCALED float32
        inputs (what ``gradient_x`` returns, exactly: every entry of it is a float32 value); intercept column included."""
        ext.hipRBFGradRows(x_unscaled, zrows, grows, self.radem_diag, self.chi_arr, float(self.hyperparams[1]),
                           self.fit_intercept)

    def zty_cached(self, zcache, y, out, workspace):
        """out <- Z^T y from float32 rows of this kernel (the resident cache or a regenerated window)."""
        ext.hipZCacheZtY(zcache, y, out, self.fit_intercept, workspace)

    def ztz_block_cached(self, zcache, vecs, out, workspace, accumulate=False):
        _block_matvec(zcache, vecs, out, workspace, self.fit_intercept, 0.0, accumulate)

    def row_cache_params(self):
        """(fit_intercept, scale): Z = scale * cache rows with Z[:, 0] = 1 when fit_intercept -- what the operators
        that consume float32 rows directly (hipSRHTSampleRows, hipSketchGemm) are told."""
        return self.fit_intercept, float(np.float32(np.sqrt(1.0 / (self.num_freqs - 0.5 if self.fit_intercept
                                                                   else self.num_freqs))))

    def cache_rows_to_features(self, zrows):
        """float64 feature rows (what transform_x returns) from rows of the float32 cache: the cache holds
        the (cos, sin) values before scaling, the operator widens them and multiplies by its float-typed
        constant (rbf_ops.cpp:68-72)."""
        scale = float(np.float32(np.sqrt(1.0 / (self.num_freqs - 0.5 if self.fit_intercept else self.num_freqs))))
        z = zrows.to(torch.float64) * scale
        if self.fit_intercept:
            z[:, 0] = 1.
        return z

    # ---- derivative of a weighted sum of the features with respect to the INPUT: the transposed SORF
    def input_gradient(self, input_x, weights, w_cols=None):
        """float64 device tensor [n, d]: d/dx of ``transform_x(x) @ weights`` at every row of the UNSCALED ``input_x``.
        ``weights`` float64, one vector [>= w_cols] for all rows or one row per datapoint [n, >= w_cols]; only the first
        ``w_cols`` feature columns (even; default all the weights cover) carry weight.  With the intercept, column 0 of the
        features is the constant 1 and ``weights[..., 0]`` does not enter.  One HIP kernel at padded width <= 1024
        (``ext.rbf_input_grad_ok``); wider inputs are composed from the feature operator and three transforms."""
        xs = self.scaled_f32(input_x)
        w, w_cols = self._input_grad_weights(weights, w_cols, xs.shape[0])
        if ext.rbf_input_grad_ok(xs.shape[1], self.num_freqs):
            out = torch.empty(tuple(xs.shape), dtype=torch.float64, device=self.device)
            ext.hipRBFInputGrad(xs, w, out, self.radem_diag, self.chi_arr, float(self.hyperparams[1]), self.fit_intercept,
                                w_cols=w_cols)
            return out
        return self.input_gradient_composed(xs, w, w_cols)

    def input_gradient_composed(self, x_scaled, weights, w_cols):
        """The same gradient from existing device operators, at every width (``composed_input_gradient``)."""
        return composed_input_gradient(x_scaled, weights, w_cols, self.radem_diag, self.chi_arr, self.num_rffs, self.fit_intercept,
                                       float(self.hyperparams[1]), self.row_cache_params()[1])

    def fused_ok(self):
        """The fused kernels cover padded width <= 4096 (single pass up to num_freqs = 7168 -- 4096 at padded widths
        2048 / 4096, whose transforms span two / four wave tiles --, the two-pass form beyond, up to 65536)."""
        return padded_dims(self._xdim[-1]) <= FUSED_MAX_WIDTH and self.num_freqs <= 65536

    def workspace_bytes(self):
        return ext.ztz_workspace_bytes(self.num_rffs, self.radem_diag.shape[2])


FUSED_MAX_WIDTH = 4096   # padded input width of the fused regenerate-and-reduce kernels (fused_ok, include/xgpr_hip.h); beyond it
                         # the fixed-vector kernels' solver passes run on float32 rows (rows_ok: regenerated windows or the cache)

BLOCK_COLS = 32          # right-hand sides per call of the block matvec (include/xgpr_hip.h)


def _block_matvec(zcache, vecs, out, workspace, fit_intercept, scale, accumulate):
    """out[M, k] (+)= Z^T (Z vecs) in column groups of BLOCK_COLS; vecs / out C-contiguous float64."""
    k = vecs.shape[1]
    if k <= BLOCK_COLS:
        ext.hipZCacheBlockMatvec(zcache, vecs, out, fit_intercept, workspace, scale, accumulate)
        return
    for j0 in range(0, k, BLOCK_COLS):
        j1 = min(k, j0 + BLOCK_COLS)
        v = vecs[:, j0:j1].contiguous()
        o = out[:, j0:j1].contiguous()
        ext.hipZCacheBlockMatvec(zcache, v, o, fit_intercept, workspace, scale, accumulate)
        out[:, j0:j1] = o


def block_workspace_bytes(nrows, num_rffs, k):
    return ext.zcache_block_workspace_bytes(nrows, num_rffs, min(k, BLOCK_COLS))


def _rescale_chi(kernel_choice, chi_arr, random_seed, parms, obj):
    """Matern: matern.py:45-54 (conv twins conv1d_matern.py:58-62, graph_matern.py:51-55);
    Cauchy: cauchy.py:39-41 (conv1d_cauchy.py:52-54, graph_cauchy.py:45-47).  The rescale is
    applied in place to the float32 array, as in the reference."""
    if kernel_choice.endswith("Matern"):
        if "matern_nu" not in parms:
            raise ValueError("Tried to initialize a Matern kernel without supplying nu.")
        obj.matern_nu = parms["matern_nu"]
        if obj.matern_nu < 1 / 2 or obj.matern_nu > 5 / 2:
            raise ValueError("nu must be >= 1/2 and <= 5/2.")
        rng = np.random.default_rng(random_seed)
        chisamples = np.sqrt(rng.chisquare(2 * obj.matern_nu, size=chi_arr.shape[0]) / (obj.matern_nu * 2))
        chi_arr /= chisamples
    elif kernel_choice.endswith("Cauchy"):
        rng = np.random.default_rng(random_seed)
        dstsamples = np.sqrt(rng.exponential(size=chi_arr.shape[0]))
        chi_arr *= dstsamples
    return chi_arr


class ConvSORFKernel(KernelBase):
    """Conv1dRBF / Conv1dMatern / Conv1dCauchy and the Graph* kernels (conv_width = 1,
    graph_rbf.py:42-43)."""

    def __init__(self, kernel_choice, xdim, num_rffs, random_seed=123, device="cuda",
                 kernel_spec_parms=None):
        kernel_spec_parms = kernel_spec_parms or {}
        super().__init__(num_rffs, xdim, kernel_spec_parms, device)
        self.random_seed = random_seed
        if len(xdim) != 3:
            raise RuntimeError("Tried to initialize a Conv1d kernel with a 2d x-"
                               "array! x should be a 3d array for Conv1d.")
        self.kernel_choice = kernel_choice
        if kernel_choice.startswith("Graph"):
            self.conv_width = 1
        else:
            if "conv_width" not in kernel_spec_parms:
                raise ValueError("conv_width must be included as a kernel-specific "
                                 "parameter if using a sequence kernel.")
            self.conv_width = kernel_spec_parms["conv_width"]
        averaging = kernel_spec_parms.get("averaging", "none")
        if averaging not in ("none", "sqrt", "full"):
            raise RuntimeError("Unrecognized value for 'averaging' supplied, "
                               "should be one of 'none', 'sqrt', 'full'.")
        self.scaling_type = {"none": 0, "sqrt": 1, "full": 2}[averaging]
        rng = np.random.default_rng(random_seed)
        pdims = padded_dims(self.conv_width * xdim[2])
        init_calc_freqsize = ceil(self.num_freqs / pdims) * pdims
        radem_array = np.asarray([-1, 1], dtype=np.int8)
        radem = rng.choice(radem_array, size=(3, 1, init_calc_freqsize), replace=True)
        chi_arr = _chi.rvs(df=pdims, size=self.num_freqs, random_state=random_seed).astype(np.float32)
        chi_arr = _rescale_chi(kernel_choice, chi_arr, random_seed, kernel_spec_parms, self)
        self._to_device(radem, chi_arr)

    supports_fused = False

    def fused_ok(self):
        return False

    # ---- float32 feature rows.  Convolution features cost K k-mers x a full SORF per sequence; the shard's Z
    # (kernel_baseclass.py:269-299 output, intercept column set) rounded to float32 -- entries are sums of float32
    # cos/sin values, so this adds at most 6e-8 relative per entry -- is what every solver pass reads: the resident
    # cache, written once per sigma and streamed from HBM afterwards, or, when it is not kept, windows of rows
    # regenerated into a reused scratch buffer (cg.row_windows).  Both are written by ``fill_feature_rows``
    # (hipConvFeatureRows: float32 stores straight from the k-mer loop's float64 sums); float64 Z is only
    # materialised by ``transform_x`` itself, for callers that ask for it.
    def cache_ok(self):
        return self.num_freqs <= 16384

    def seq_rows_ok(self):
        """Whether ``fill_feature_rows`` can write this kernel's float32 rows: on a HIP device, for every shape the
        float64 operator serves."""
        return torch.device(self.device).type == "cuda"

    def _host_lengths(self, x_scaled, sequence_length):
        if sequence_length is None:
            raise RuntimeError("sequence_length is required for convolution kernels.")
        if x_scaled.shape[2] != self._xdim[2]:
            raise RuntimeError("Unexpected input shape supplied.")
        if isinstance(sequence_length, torch.Tensor):
            sequence_length = sequence_length.cpu().numpy()
        return np.ascontiguousarray(sequence_length.astype(np.int32, copy=False))

    def token_rows_ok(self, batch):
        """Whether the token operators serve ``batch`` for this kernel (ext.conv_token_rows_ok: a window of up to 1024
        elements, a table that fits the kernels' LDS image); otherwise its rows come from dense slices."""
        return (self.seq_rows_ok() and batch.is_cuda and batch.tokens.is_contiguous()
                and ext.conv_token_rows_ok(self.conv_width * batch.shape[2], batch.table.shape[0], batch.shape[2]) == 1)

    def _dense_slices(self, batch, lengths):
        """(lo, hi, dense float32 slice, its lengths) over a TokenBatch the token operators do not serve: at most
        ``CACHE_BUILD_ROWS`` sequences are expanded at a time."""
        for lo in range(0, batch.shape[0], self.CACHE_BUILD_ROWS):
            hi = min(lo + self.CACHE_BUILD_ROWS, batch.shape[0])
            yield lo, hi, batch[lo:hi].dense().contiguous(), lengths[lo:hi]

    def fill_feature_rows(self, x_scaled, sequence_length, rows_out):
        """rows_out [n, num_rffs] float32 <- ``transform_x`` of the (already sigma-scaled, float32) sequences, rounded
        to float32: overwritten, bit-identical to ``transform_x(...).to(torch.float32)``.  ``x_scaled`` may be a
        TokenBatch over the sigma-scaled table: the token operator reads it as it is (same bits as the dense array)."""
        lengths = self._host_lengths(x_scaled, sequence_length)
        if isinstance(x_scaled, TokenBatch):
            if self.token_rows_ok(x_scaled):
                ext.hipConvTokenRows(x_scaled.tokens, x_scaled.table, rows_out, self.radem_diag, self.chi_arr, lengths,
                                     self.conv_width, self.scaling_type, self.fit_intercept)
                return
            for lo, hi, xd, lens in self._dense_slices(x_scaled, lengths):
                ext.hipConvFeatureRows(xd, rows_out[lo:hi], self.radem_diag, self.chi_arr, lens, self.conv_width,
                                       self.scaling_type, self.fit_intercept)
            return
        ext.hipConvFeatureRows(x_scaled, rows_out, self.radem_diag, self.chi_arr, lengths, self.conv_width, self.scaling_type,
                               self.fit_intercept)

    # ---- derivative of a weighted sum of the features with respect to the INPUT, per position and channel
    COMPOSED_GRAD_ELEMS = 1 << 25    # float64 elements of per-window weights (or window rows) the unfold route holds per slice

    def input_gradient(self, input_x, sequence_length, weights, w_cols=None):
        """float64 device tensor [n, L, C]: d/dx of ``transform_x(x, sequence_length) @ weights`` at every position and channel of
        the UNSCALED sequences ``input_x`` (dense [n, L, C], or a TokenBatch: the gradient is then with respect to the table rows
        the tokens select, position by position -- a saliency map).  Positions past a sequence's length are exactly 0.
        ``weights`` and ``w_cols`` as for ``SORFKernel.input_gradient``.  One HIP kernel where ``ext.conv_input_grad_ok`` /
        ``ext.conv_token_input_grad_ok`` hold (windows of up to 1024 elements; a token table the LDS image holds); tokens over a
        larger table are expanded slice by slice, wider windows take ``input_gradient_composed``."""
        xs = self.scaled_f32(input_x)
        lengths = self._host_lengths(xs, sequence_length)
        n, L, C = xs.shape
        w, w_cols = self._input_grad_weights(weights, w_cols, n)
        sigma = float(self.hyperparams[1])
        if isinstance(xs, TokenBatch):
            out = torch.empty((n, L, C), dtype=torch.float64, device=self.device)
            if (xs.is_cuda and xs.tokens.is_contiguous()
                    and ext.conv_token_input_grad_ok(self.conv_width * C, xs.table.shape[0], C) == 1):
                ext.hipConvTokenInputGrad(xs.tokens, xs.table, w, out, self.radem_diag, self.chi_arr, lengths, sigma,
                                          self.conv_width, self.scaling_type, self.fit_intercept, w_cols=w_cols)
                return out
            for lo, hi, xd, lens in self._dense_slices(xs, lengths):
                out[lo:hi] = self._dense_input_gradient(xd, lens, w if w.dim() == 1 else w[lo:hi], w_cols)
            return out
        return self._dense_input_gradient(xs, lengths, w, w_cols)

    def _dense_input_gradient(self, x_scaled, lengths, w, w_cols):
        if ext.conv_input_grad_ok(self.conv_width * x_scaled.shape[2], self.num_freqs) != 1:
            return self.input_gradient_composed(x_scaled, lengths, w, w_cols)
        out = torch.empty(tuple(x_scaled.shape), dtype=torch.float64, device=self.device)
        ext.hipConvInputGrad(x_scaled, w, out, self.radem_diag, self.chi_arr, lengths, float(self.hyperparams[1]), self.conv_width,
                             self.scaling_type, self.fit_intercept, w_cols=w_cols)
        return out

    def input_gradient_composed(self, x_scaled, lengths, weights, w_cols):
        """The same gradient by the unfold route, at every window width, from existing operators: a bounded slice of sequences
        is unfolded into its L - conv_width + 1 window rows each, the rows go to ``hipRBFInputGrad`` (``composed_input_gradient``
        beyond its widths) with per-row weights already divided by the sequence's k-mer normaliser -- zero for the windows past a
        sequence's last k-mer --, and the rows' gradients are folded back with conv_width slice additions in float64, window
        offset 0 first.  ``x_scaled`` dense float32 [n, L, C], already multiplied by sigma; ``lengths`` int32 on the host."""
        n, L, C = x_scaled.shape
        cw, nf, sigma = self.conv_width, self.num_freqs, float(self.hyperparams[1])
        d, nkmax = cw * C, L - cw + 1
        if int(lengths.min()) < cw or int(lengths.max()) > L:
            raise RuntimeError("All sequence lengths must be >= conv width and < array size.")
        nk = torch.from_numpy(lengths.astype(np.float64) - (cw - 1)).to(self.device)
        scale = float(np.sqrt(1.0 / nf))
        direct = ext.rbf_input_grad_ok(d, nf) == 1
        # the row operator's constant with the intercept off is the float-typed sqrt(1 / F): the ratio to this kernel's rides on the weights
        ratio = scale / float(np.float32(np.sqrt(1.0 / nf))) if direct else 1.0
        norm = (torch.ones_like(nk), torch.sqrt(nk), nk)[self.scaling_type] / ratio
        live = torch.arange(nkmax, device=self.device)[None, :] < nk[:, None]             # [n, nkmax]: window j is a k-mer
        out = torch.zeros((n, L, C), dtype=torch.float64, device=self.device)
        step = max(1, self.COMPOSED_GRAD_ELEMS // (nkmax * max(w_cols, padded_dims(d))))
        for lo in range(0, n, step):
            hi = min(lo + step, n)
            rows = x_scaled[lo:hi].unfold(1, cw, 1).permute(0, 1, 3, 2).reshape((hi - lo) * nkmax, d).contiguous()
            wseq = (weights[None, :w_cols] if weights.dim() == 1 else weights[lo:hi, :w_cols]) / norm[lo:hi, None]
            wrows = (wseq[:, None, :] * live[lo:hi, :, None]).reshape((hi - lo) * nkmax, w_cols)
            if self.fit_intercept:
                wrows[:, 0] = 0.
            if direct:
                g = torch.empty((rows.shape[0], d), dtype=torch.float64, device=self.device)
                ext.hipRBFInputGrad(rows, wrows, g, self.radem_diag, self.chi_arr, sigma, False, w_cols=w_cols)
            else:
                g = composed_input_gradient(rows, wrows, w_cols, self.radem_diag, self.chi_arr, self.num_rffs, False, sigma, scale)
            g = g.view(hi - lo, nkmax, cw, C)
            for q in range(cw):
                out[lo:hi, q:q + nkmax, :] += g[:, :, q, :]
        out *= (torch.arange(L, device=self.device)[None, :] < torch.from_numpy(lengths).to(self.device)[:, None])[:, :, None]
        return out

    # ---- the exact effect of every single-token substitution on a weighted sum of the features
    COMPOSED_SCAN_ELEMS = 1 << 25    # float32 elements of mutant feature rows the composed route holds per slice

    def _scan_inputs(self, batch, sequence_length, weights):
        if not isinstance(batch, TokenBatch):
            raise RuntimeError("substitution_scan needs sequences given as tokens (a TokenBatch).")
        xs = self.scaled_f32(batch)
        lengths = self._host_lengths(xs, sequence_length)
        if lengths.shape[0] != xs.shape[0]:
            raise RuntimeError("sequence_length must hold one length per sequence.")
        w = weights if isinstance(weights, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(weights))
        w = w.to(self.device, torch.float64).contiguous()
        if w.dim() != 1 or w.shape[0] != self.num_rffs:
            raise RuntimeError("weights must be one vector of num_rffs values.")
        return xs, lengths, w

    def _scan_operator_ok(self, xs, predicate):
        return bool(xs.is_cuda and xs.tokens.is_contiguous()
                    and predicate(self.conv_width * xs.shape[2], xs.table.shape[0], xs.shape[2], self.num_freqs) == 1)

    def substitution_scan(self, batch, sequence_length, weights):
        """float64 device tensor [n, L, V]: ``transform_x(sequence with token l replaced by v) @ weights`` minus
        ``transform_x(sequence) @ weights`` for every position l and every row v of the TokenBatch's table -- the exact effect of
        every single substitution, not its first-order estimate (``input_gradient``).  Exactly 0 at a sequence's own token and
        past its length.  ``weights``: one vector of num_rffs values.  A substitution at l changes only the conv_width windows
        that cover l, so one HIP kernel transforms L V conv_width windows instead of the L V (L - conv_width + 1) of L V mutant
        sequences, and writes no mutant (``ext.hipConvTokenSubstScan``); where ``ext.conv_token_subst_scan_ok`` is 0 (windows
        of more than 1024 elements, a table the LDS image does not hold) or the tokens are not contiguous the result comes from
        ``substitution_scan_composed``."""
        xs, lengths, w = self._scan_inputs(batch, sequence_length, weights)
        n, L, _ = xs.shape
        V = xs.table.shape[0]
        if not self._scan_operator_ok(xs, ext.conv_token_subst_scan_ok):
            return self._scan_composed(xs, lengths, w)
        out = torch.empty((n, L, V), dtype=torch.float64, device=self.device)
        ext.hipConvTokenSubstScan(xs.tokens, xs.table.contiguous(), w, out, self.radem_diag, self.chi_arr, lengths, self.conv_width,
                                  self.scaling_type, self.fit_intercept)
        return out

    def substitution_scan_composed(self, batch, sequence_length, weights):
        """The same result from existing operators, at every window width and table size: a bounded slice of (sequence,
        position, token) mutants is written out as token rows, ``fill_feature_rows`` makes their float32 feature rows,
        ``hipZCacheBlockProject`` with one column their weighted sums, and the unmutated sequence's value is subtracted.  At most
        ``COMPOSED_SCAN_ELEMS`` float32 row elements are held at a time."""
        return self._scan_composed(*self._scan_inputs(batch, sequence_length, weights))

    def _scan_composed(self, xs, lengths, w):
        n, L, _ = xs.shape
        V, dev = xs.table.shape[0], self.device
        self._check_lengths(lengths, n, L)
        project = self._projector(xs.table, w)
        tokens, lens_dev = xs.tokens.contiguous(), torch.from_numpy(lengths).to(dev)
        step = max(1, self.COMPOSED_SCAN_ELEMS // self.num_rffs)

        base = torch.empty(n, dtype=torch.float64, device=dev)
        for lo in range(0, n, step):
            base[lo:lo + step] = project(tokens[lo:lo + step], lengths[lo:lo + step])
        out = torch.empty((n, L, V), dtype=torch.float64, device=dev)
        flat = out.view(-1)
        for lo in range(0, n * L * V, step):
            ids = torch.arange(lo, min(lo + step, n * L * V), device=dev)
            seq, pos, tok = ids // (L * V), (ids // V) % L, ids % V
            mut = tokens[seq]
            mut[torch.arange(ids.shape[0], device=dev), pos] = tok.to(torch.uint8)
            flat[lo:lo + step] = project(mut, lengths[seq.cpu().numpy()]) - base[seq]
        # the own token and the positions past a length: the mutant is the sequence itself
        pos = torch.arange(L, device=dev)
        same = (pos[None, :] >= lens_dev[:, None])[:, :, None] | (torch.arange(V, device=dev)[None, None, :] == tokens.long()[:, :, None])
        return out.masked_fill_(same, 0.0)

    # ---- the exact non-additive part of every pair of substitutions closer than conv_width
    PAIR_SCAN_ROWS = 1 << 24         # rows [V] of the output one launch serves (xgpr_conv_token_pair_scan_f32: one workgroup each)

    def pair_substitution_scan(self, batch, sequence_length, weights):
        """float64 device tensor [n, L, conv_width - 1, V, V]: entry [i, l1, d - 1, v1, v2] is ``transform_x(sequence with token
        l1 replaced by v1 and token l1 + d by v2) @ weights`` minus ``transform_x(sequence) @ weights`` minus the two entries
        [i, l1, v1] and [i, l1 + d, v2] of ``substitution_scan`` -- what two substitutions do together beyond what each does alone.
        Exactly 0 where either token is the sequence's own and where either position is past its length; two substitutions
        conv_width or more apart share no window and add exactly, so the band is the whole of it (no entry at all for the graph
        kernels).  Only the conv_width - d windows that cover both positions are transformed, and no mutant is written
        (``ext.hipConvTokenPairScan``); a batch of more than ``PAIR_SCAN_ROWS`` output rows goes to the operator in slices.  Where
        ``ext.conv_token_pair_scan_ok`` is 0 (windows of more than 1024 elements, a table the LDS image does not hold) or the
        tokens are not contiguous the result comes from ``pair_substitution_scan_composed``."""
        xs, lengths, w = self._scan_inputs(batch, sequence_length, weights)
        n, L, _ = xs.shape
        V, band = xs.table.shape[0], self.conv_width - 1
        if not self._scan_operator_ok(xs, ext.conv_token_pair_scan_ok):
            return self._pair_scan_composed(xs, lengths, w)
        out = torch.empty((n, L, band, V, V), dtype=torch.float64, device=self.device)
        table = xs.table.contiguous()
        step = max(1, (self.PAIR_SCAN_ROWS - 1) // max(1, L * band * V))
        for lo in range(0, max(n, 1), step):             # (n == 0: one call, for its checks)
            ext.hipConvTokenPairScan(xs.tokens[lo:lo + step], table, w, out[lo:lo + step], self.radem_diag, self.chi_arr,
                                     lengths[lo:lo + step], self.conv_width, self.scaling_type, self.fit_intercept)
        return out

    def pair_substitution_scan_composed(self, batch, sequence_length, weights):
        """The same result from existing operators, at every window width and table size: bounded slices of written-out single
        and double mutants go through ``fill_feature_rows`` and ``hipZCacheBlockProject`` with one column, and an entry is
        ``(m(both) - m(v1 alone)) - (m(v2 alone) - m(sequence))``.  Only the slots inside a sequence are written out; the own-token
        planes and the slots past a length are set to exact zeros.  At most ``COMPOSED_SCAN_ELEMS`` float32 row elements are
        held at a time."""
        return self._pair_scan_composed(*self._scan_inputs(batch, sequence_length, weights))

    def _pair_scan_composed(self, xs, lengths, w):
        n, L, _ = xs.shape
        V, dev, band = xs.table.shape[0], self.device, self.conv_width - 1
        self._check_lengths(lengths, n, L)
        out = torch.zeros((n, L, band, V, V), dtype=torch.float64, device=dev)
        if out.numel() == 0:
            return out
        project = self._projector(xs.table, w)
        tokens, lens_dev = xs.tokens.contiguous(), torch.from_numpy(lengths).to(dev)
        step = max(1, self.COMPOSED_SCAN_ELEMS // self.num_rffs)

        def mutants(seq, edits):
            mut = tokens[seq]
            rows = torch.arange(seq.shape[0], device=dev)
            for pos, tok in edits:
                mut[rows, pos] = tok.to(torch.uint8)
            return project(mut, lengths[seq.cpu().numpy()])

        base = torch.empty(n, dtype=torch.float64, device=dev)
        for lo in range(0, n, step):
            base[lo:lo + step] = project(tokens[lo:lo + step], lengths[lo:lo + step])
        pos = torch.arange(L, device=dev)
        # m of every single mutant inside a sequence, once: [n, L, V]
        single = torch.zeros((n, L, V), dtype=torch.float64, device=dev)
        slots = (pos[None, :] < lens_dev[:, None]).nonzero()
        for lo in range(0, slots.shape[0] * V, step):
            ids = torch.arange(lo, min(lo + step, slots.shape[0] * V), device=dev)
            (seq, l), v = slots[ids // V].T, ids % V
            single[seq, l, v] = mutants(seq, [(l, v)])
        # ... and of every double mutant with both positions inside it
        second = pos[:, None] + 1 + torch.arange(band, device=dev)[None, :]              # [L, band]: l2 of slot (l1, d - 1)
        slots = (second[None, :, :] < lens_dev[:, None, None]).nonzero()
        for lo in range(0, slots.shape[0] * V * V, step):
            ids = torch.arange(lo, min(lo + step, slots.shape[0] * V * V), device=dev)
            (seq, l1, dd), v1, v2 = slots[ids // (V * V)].T, (ids // V) % V, ids % V
            l2 = l1 + dd + 1
            out[seq, l1, dd, v1, v2] = (mutants(seq, [(l1, v1), (l2, v2)]) - single[seq, l1, v1]) - (single[seq, l2, v2] - base[seq])
        # either token the sequence's own: the double mutant is a single one
        own = tokens.long()
        tok = torch.arange(V, device=dev)
        out.masked_fill_((tok[None, None, :] == own[:, :, None])[:, :, None, :, None], 0.0)
        return out.masked_fill_((tok[None, None, None, :] == own[:, second.clamp(max=L - 1)][:, :, :, None])[:, :, :, None, :], 0.0)

    # ---- every variant of K chosen sites, as a sum of one small table per set of sites a window sees together
    SITE_SCAN_ROWS = 1 << 24         # grid rows one launch serves (xgpr_conv_token_site_scan_f32: one workgroup each)
    SITE_SCAN_VARIANTS = 1 << 22     # V^K the composed route writes out per sequence, at the most

    def _site_list(self, sites, L, lengths):
        s = np.asarray(sites)
        if s.ndim != 1 or s.shape[0] < 1 or s.dtype.kind not in "iu":
            raise RuntimeError("sites must be a non-empty list of integer positions.")
        s = s.astype(np.int64)
        if (np.diff(s) <= 0).any() or int(s[0]) < 0 or int(s[-1]) >= L:
            raise RuntimeError("sites must be strictly ascending positions inside the array.")
        if lengths.shape[0] and int(s[-1]) >= int(lengths.min()):
            raise RuntimeError("every site must lie inside every sequence of the batch.")
        return [int(p) for p in s]

    def site_scan(self, batch, sequence_length, weights, sites):
        """``SiteLibrary`` of the K positions ``sites`` (strictly ascending, shared by the batch and inside every sequence): every
        one of the V^K variants of every sequence, as ``transform_x(variant) @ weights`` minus ``transform_x(sequence) @ weights``,
        held as one table per RUN -- a set of sites that one range of windows covers together -- of V^g entries, g the sites of
        the run.  A variant's value is the sum of one entry per run, exactly, for ANY number of sites inside a window (the
        singles-plus-pairs recipe of ``pair_substitution_scan`` is exact for two).  Only the windows that cover a site are
        transformed, each for the assignments of the sites it covers, and no variant is written (``ext.hipConvTokenSiteScan``);
        the entry of a sequence's own tokens is exactly 0 in every table.  A batch of more than ``SITE_SCAN_ROWS`` grid rows
        goes to the operator in slices.  Where ``ext.conv_token_site_scan_ok`` is 0 (windows of more than 1024 elements, a table
        the LDS image does not hold, more than 4 sites inside one window), with more than 16 sites or where the tokens are not
        contiguous the result comes from ``site_scan_composed``."""
        from .acquisition import SiteLibrary, site_runs
        xs, lengths, w = self._scan_inputs(batch, sequence_length, weights)
        n, L, _ = xs.shape
        V = xs.table.shape[0]
        sites = self._site_list(sites, L, lengths)
        runs = site_runs(sites, L, self.conv_width)
        cover = max(g for _, _, _, g in runs)
        rows = sum(V ** (g - 1) for _, _, _, g in runs) if cover <= 4 else self.SITE_SCAN_ROWS
        if (len(sites) > 16 or rows >= self.SITE_SCAN_ROWS
                or not self._scan_operator_ok(xs, lambda *a: ext.conv_token_site_scan_ok(*a, cover))):
            return self._site_scan_composed(xs, lengths, w, sites)
        layout, T = ext.conv_token_site_scan_layout(sites, L, self.conv_width, V)
        out = torch.empty((n, T), dtype=torch.float64, device=self.device)
        table = xs.table.contiguous()
        step = max(1, (self.SITE_SCAN_ROWS - 1) // rows)
        for lo in range(0, max(n, 1), step):             # (n == 0: one call, for its checks)
            ext.hipConvTokenSiteScan(xs.tokens[lo:lo + step], table, w, out[lo:lo + step], self.radem_diag, self.chi_arr,
                                     lengths[lo:lo + step], sites, self.conv_width, self.scaling_type, self.fit_intercept)
        tables = [out[:, r["offset"]:r["offset"] + V ** r["sites"]].reshape((n,) + (V,) * r["sites"]) for r in layout]
        return SiteLibrary(sites, V, [range(r["first_site"], r["first_site"] + r["sites"]) for r in layout], tables)

    def site_scan_composed(self, batch, sequence_length, weights, sites):
        """The same library from existing operators, at every window width and table size, as ONE run over all K sites: bounded
        slices of written-out variants go through ``fill_feature_rows`` and ``hipZCacheBlockProject`` with one column, and an
        entry is m(variant) - m(sequence); the own assignment is set to an exact zero.  At most ``COMPOSED_SCAN_ELEMS`` float32
        row elements are held at a time; more than ``SITE_SCAN_VARIANTS`` = 2^22 variants per sequence are refused."""
        xs, lengths, w = self._scan_inputs(batch, sequence_length, weights)
        return self._site_scan_composed(xs, lengths, w, self._site_list(sites, xs.shape[1], lengths))

    def _site_scan_composed(self, xs, lengths, w, sites):
        from .acquisition import SiteLibrary
        n, L, _ = xs.shape
        V, K, dev = xs.table.shape[0], len(sites), self.device
        self._check_lengths(lengths, n, L)
        if V ** K > self.SITE_SCAN_VARIANTS:
            raise RuntimeError(f"site_scan_composed would write out {V}^{K} variants per sequence, more than SITE_SCAN_VARIANTS = "
                               f"{self.SITE_SCAN_VARIANTS}: the composed route serves small libraries only (the operator route "
                               "needs windows of up to 1024 elements and at most 4 sites inside one window).")
        nv = V ** K
        project = self._projector(xs.table, w)
        tokens = xs.tokens.contiguous()
        step = max(1, self.COMPOSED_SCAN_ELEMS // self.num_rffs)
        base = torch.empty(n, dtype=torch.float64, device=dev)
        for lo in range(0, n, step):
            base[lo:lo + step] = project(tokens[lo:lo + step], lengths[lo:lo + step])
        out = torch.empty((n, nv), dtype=torch.float64, device=dev)
        flat = out.view(-1)
        own = torch.zeros(n, dtype=torch.long, device=dev)
        for p in sites:
            own = own * V + tokens[:, p].long()
        for lo in range(0, n * nv, step):
            ids = torch.arange(lo, min(lo + step, n * nv), device=dev)
            seq, var = ids // nv, ids % nv
            mut = tokens[seq]
            rows = torch.arange(ids.shape[0], device=dev)
            for k, p in enumerate(sites):
                mut[rows, p] = ((var // V ** (K - 1 - k)) % V).to(torch.uint8)
            flat[lo:lo + step] = project(mut, lengths[seq.cpu().numpy()]) - base[seq]
        if n:
            out[torch.arange(n, device=dev), own] = 0.0  # the own assignment: the variant is the sequence itself
        return SiteLibrary(sites, V, [range(K)], [out.reshape((n,) + (V,) * K)])

    # ---- the exact quadratic form of the predictive variance of every single-token substitution
    def _var_scan_inputs(self, batch, sequence_length, var):
        if not isinstance(batch, TokenBatch):
            raise RuntimeError("substitution_variance_scan needs sequences given as tokens (a TokenBatch).")
        xs = self.scaled_f32(batch)
        lengths = self._host_lengths(xs, sequence_length)
        if lengths.shape[0] != xs.shape[0]:
            raise RuntimeError("sequence_length must hold one length per sequence.")
        vm = var if isinstance(var, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(var))
        vm = vm.to(self.device, torch.float64)
        if vm.dim() != 2 or vm.shape[0] != vm.shape[1] or not 1 <= vm.shape[0] <= self.num_rffs:
            raise RuntimeError("var must be a square matrix over the first 1 .. num_rffs feature columns.")
        return xs, lengths, vm

    def _var_scan_columns(self, xs, lengths, vm, ok, check_lengths=False):
        """What the two variance scans feed their operator from -> (``var`` padded with a zero row and column to an even size, the
        sequences' own first columns: float32 rows of ``fill_feature_rows``, widened), or None where the operator's predicate ``ok``
        is 0 or the tokens are not contiguous: the composed route.  ``check_lengths``: hold the lengths to the array on this route."""
        n, L, C = xs.shape
        V, nvar = xs.table.shape[0], vm.shape[0]
        npad = nvar + (nvar & 1)
        if not (xs.is_cuda and xs.tokens.is_contiguous() and ok(self.conv_width * C, V, C, self.num_freqs, npad) == 1):
            return None
        if check_lengths:
            self._check_lengths(lengths, n, L)
        vp = torch.zeros((npad, npad), dtype=torch.float64, device=self.device)
        vp[:nvar, :nvar] = vm
        rows = torch.empty((n, self.num_rffs), dtype=torch.float32, device=self.device)
        self.fill_feature_rows(xs, lengths, rows)
        return vp, rows[:, :npad].to(torch.float64)

    def substitution_variance_scan(self, batch, sequence_length, var):
        """float64 device tensor [n, L, V]: ``z'^T var z'`` for the first ``nvar = var.shape[0]`` columns z' of
        ``transform_x(sequence with token l replaced by v)``, for every position l and every row v of the TokenBatch's table --
        what ``xGPRegression.predict`` turns into the variance (lambda^2 + lambda^2 z'^T var z').  Exactly 0 past a sequence's
        length; the sequence's own quadratic form at its own token.  A substitution at l moves z by r times a vector built from
        the conv_width windows that cover l alone, so one pair of HIP kernels per slab of mutants (``ext.hipConvTokenSubstVarScan``)
        transforms L V conv_width windows of one 1024-frequency tile and contracts the [L V, nvar] matrix of those vectors with
        ``var`` on the float64 matrix cores; the sequences' own columns come from ``fill_feature_rows`` (float32 rows, widened).
        An odd nvar is padded with a zero row and column.  Where ``ext.conv_token_subst_var_scan_ok`` is 0 (windows of more than
        1024 elements, a table the LDS image does not hold, nvar > 2048) or the tokens are not contiguous the result comes from
        ``substitution_variance_scan_composed``."""
        xs, lengths, vm = self._var_scan_inputs(batch, sequence_length, var)
        n, L, _ = xs.shape
        V = xs.table.shape[0]
        columns = self._var_scan_columns(xs, lengths, vm, ext.conv_token_subst_var_scan_ok)
        if columns is None:
            return self._var_scan_composed(xs, lengths, vm)
        vp, z = columns
        zv = z @ vp.T                                    # row i: var z_i
        u = (0.5 * (zv + z @ vp)).contiguous()           # (= var z_i for a symmetric var; the cross terms of any var)
        q = (z * zv).sum(dim=1).contiguous()
        out = torch.empty((n, L, V), dtype=torch.float64, device=self.device)
        ext.hipConvTokenSubstVarScan(xs.tokens, xs.table.contiguous(), vp, u, q, out, self.radem_diag, self.chi_arr, lengths,
                                     self.conv_width, self.scaling_type, self.fit_intercept)
        return out

    def substitution_variance_scan_composed(self, batch, sequence_length, var):
        """The same result from existing operators, at every window width, table size and nvar: a bounded slice of (sequence,
        position, token) mutants is written out as token rows, ``fill_feature_rows`` makes their float32 feature rows, and the
        quadratic form of their first nvar columns with ``var`` is taken in float64 with torch.  At most ``COMPOSED_SCAN_ELEMS``
        float32 row elements are held at a time."""
        return self._var_scan_composed(*self._var_scan_inputs(batch, sequence_length, var))

    def _var_scan_composed(self, xs, lengths, vm):
        n, L, _ = xs.shape
        V, dev, nvar = xs.table.shape[0], self.device, vm.shape[0]
        self._check_lengths(lengths, n, L)
        tokens, lens_dev = xs.tokens.contiguous(), torch.from_numpy(lengths).to(dev)
        step = max(1, self.COMPOSED_SCAN_ELEMS // self.num_rffs)

        def quad(tok, lens):
            rows = torch.empty((tok.shape[0], self.num_rffs), dtype=torch.float32, device=dev)
            self.fill_feature_rows(TokenBatch(tok.contiguous(), xs.table), lens, rows)
            xv = rows[:, :nvar].to(torch.float64)
            return (xv * (xv @ vm.T)).sum(dim=1)

        out = torch.empty((n, L, V), dtype=torch.float64, device=dev)
        flat = out.view(-1)
        for lo in range(0, n * L * V, step):
            ids = torch.arange(lo, min(lo + step, n * L * V), device=dev)
            seq, pos, tok = ids // (L * V), (ids // V) % L, ids % V
            mut = tokens[seq]
            # (a position past the length: the token lands outside the sequence and is never read; zeroed below)
            mut[torch.arange(ids.shape[0], device=dev), pos] = tok.to(torch.uint8)
            flat[lo:lo + step] = quad(mut, lengths[seq.cpu().numpy()])
        past = torch.arange(L, device=dev)[None, :] >= lens_dev[:, None]
        return out.masked_fill_(past[:, :, None], 0.0)

    # ---- the exact effect of every single-token deletion and insertion on a weighted sum of the features
    def window_scores(self, batch, sequence_length, weights):
        """float64 device tensor [n, L]: the share of every k-mer window in ``transform_x(sequence) @ weights`` before the k-mer
        normaliser -- ``scores[i, j] = sum_f (w[2f] cos p_f + w[2f+1] sin p_f)`` over the projections p of window j
        (``weights[0]`` dropped under the intercept), exactly 0 for j >= nk = length - conv_width + 1.
        ``sqrt(1 / num_freqs) / {1, sqrt(nk), nk} * scores[i].sum()`` plus ``weights[0]`` under the intercept is
        ``transform_x(sequence i) @ weights``.  One HIP kernel (``ext.hipConvTokenWindowScores``) where
        ``ext.conv_token_indel_scan_ok`` holds; elsewhere every window goes through ``fill_feature_rows`` as a sequence of its own."""
        xs, lengths, w = self._scan_inputs(batch, sequence_length, weights)
        if not self._scan_operator_ok(xs, ext.conv_token_indel_scan_ok):
            return self._window_scores_composed(xs, lengths, w)
        scores = torch.empty(xs.shape[:2], dtype=torch.float64, device=self.device)
        ext.hipConvTokenWindowScores(xs.tokens, xs.table.contiguous(), w, scores, self.radem_diag, self.chi_arr, lengths, self.conv_width,
                                     self.fit_intercept)
        return scores

    def indel_scan(self, batch, sequence_length, weights):
        """(deletions [n, L], insertions [n, L + 1, V]), float64 device tensors: ``transform_x(mutant) @ weights`` minus
        ``transform_x(sequence) @ weights`` for the sequence without its token at position p, and for the sequence with row v of the
        TokenBatch's table inserted before position g (g = length appends) -- exact.  Exactly 0 for p >= length and g > length;
        the deletions of a sequence of exactly conv_width tokens (no window left) are NaN.  An indel only shifts the windows that
        do not touch the edit site, so the HIP kernels (``ext.hipConvTokenWindowScores`` + ``ext.hipConvTokenIndelScan``)
        transform about conv_width windows per edit and the nk windows of the sequence once, rescale the total by the new
        k-mer normaliser, and write no mutant; where ``ext.conv_token_indel_scan_ok`` is 0 or the tokens are not contiguous the
        result comes from ``indel_scan_composed``."""
        xs, lengths, w = self._scan_inputs(batch, sequence_length, weights)
        if not self._scan_operator_ok(xs, ext.conv_token_indel_scan_ok):
            return self._indel_composed(xs, lengths, w)
        n, L, _ = xs.shape
        table = xs.table.contiguous()
        scores = torch.empty((n, L), dtype=torch.float64, device=self.device)
        dele = torch.empty((n, L), dtype=torch.float64, device=self.device)
        ins = torch.empty((n, L + 1, table.shape[0]), dtype=torch.float64, device=self.device)
        ext.hipConvTokenWindowScores(xs.tokens, table, w, scores, self.radem_diag, self.chi_arr, lengths, self.conv_width, self.fit_intercept)
        ext.hipConvTokenIndelScan(xs.tokens, table, w, scores, dele, ins, self.radem_diag, self.chi_arr, lengths, self.conv_width,
                                  self.scaling_type, self.fit_intercept)
        return dele, ins

    def indel_scan_composed(self, batch, sequence_length, weights):
        """The same result from existing operators, at every window width and table size: bounded slices of deletion and insertion
        mutants are written out as token rows of L + 1 positions, ``fill_feature_rows`` makes their float32 feature rows,
        ``hipZCacheBlockProject`` with one column their weighted sums, the unmutated sequence's value is subtracted, and the zeros
        and NaNs of the contract are applied.  At most ``COMPOSED_SCAN_ELEMS`` float32 row elements are held at a time."""
        return self._indel_composed(*self._scan_inputs(batch, sequence_length, weights))

    def _projector(self, table, w):
        """f(token rows, int32 host lengths) -> their feature rows times w (column 0 dropped under the intercept), float64 [m]."""
        wcol = w.clone()
        if self.fit_intercept:
            wcol[0] = 0.                                 # column 0 is the constant 1 of every row
        wcol = wcol[:, None].contiguous()

        def project(tok, lens):
            rows = torch.empty((tok.shape[0], self.num_rffs), dtype=torch.float32, device=self.device)
            self.fill_feature_rows(TokenBatch(tok.contiguous(), table), lens, rows)
            val = torch.empty((tok.shape[0], 1), dtype=torch.float64, device=self.device)
            ext.hipZCacheBlockProject(rows, wcol, val, False, 1.0)
            return val[:, 0]
        return project

    def _check_lengths(self, lengths, n, L):
        if n and (int(lengths.min()) < self.conv_width or int(lengths.max()) > L):
            raise RuntimeError("All sequence lengths must be >= conv width and < array size.")

    def _window_scores_composed(self, xs, lengths, w):
        n, L, _ = xs.shape
        cw, dev = self.conv_width, self.device
        self._check_lengths(lengths, n, L)
        project = self._projector(xs.table, w)
        wins = xs.tokens.unfold(1, cw, 1)                # [n, L - cw + 1, cw]: every window as a sequence of one window
        nw = wins.shape[1]
        live = torch.arange(nw, device=dev)[None, :] < (torch.from_numpy(lengths).to(dev)[:, None] - cw + 1)
        idx = live.reshape(-1).nonzero()[:, 0]
        flat = wins.reshape(n * nw, cw)
        vals = torch.empty(idx.shape[0], dtype=torch.float64, device=dev)
        step = max(1, self.COMPOSED_SCAN_ELEMS // self.num_rffs)
        for lo in range(0, idx.shape[0], step):
            ids = idx[lo:lo + step]
            vals[lo:lo + step] = project(flat[ids], np.full(ids.shape[0], cw, dtype=np.int32))
        out = torch.zeros((n, L), dtype=torch.float64, device=dev)
        # (a row of one window is sqrt(1 / F) (cos, sin) under every averaging)
        out[:, :nw][live] = vals / float(np.sqrt(1.0 / self.num_freqs))
        return out

    def _indel_composed(self, xs, lengths, w):
        n, L, _ = xs.shape
        V, cw, dev = xs.table.shape[0], self.conv_width, self.device
        self._check_lengths(lengths, n, L)
        project = self._projector(xs.table, w)
        tokens, lens_dev = xs.tokens.contiguous(), torch.from_numpy(lengths).to(dev).long()
        step = max(1, self.COMPOSED_SCAN_ELEMS // self.num_rffs)
        k = torch.arange(L + 1, device=dev)[None, :]

        base = torch.empty(n, dtype=torch.float64, device=dev)
        for lo in range(0, n, step):
            base[lo:lo + step] = project(tokens[lo:lo + step], lengths[lo:lo + step])
        dele = torch.empty((n, L), dtype=torch.float64, device=dev)
        flat = dele.view(-1)
        for lo in range(0, n * L, step):
            ids = torch.arange(lo, min(lo + step, n * L), device=dev)
            seq, pos = ids // L, ids % L
            pos = torch.where(lens_dev[seq] > cw, pos, L + 1)                   # (no mutant: the sequence itself, overwritten below)
            src = (k + (k >= pos[:, None]).long()).clamp_(max=L - 1)            # position k of the mutant reads k + (k >= p)
            mut = torch.gather(tokens[seq], 1, src)
            mlen = (lens_dev[seq] - 1).clamp_(min=cw)                           # (entries with no mutant are overwritten below)
            flat[lo:lo + step] = project(mut, mlen.to(torch.int32).cpu().numpy()) - base[seq]
        ins = torch.empty((n, L + 1, V), dtype=torch.float64, device=dev)
        flat = ins.view(-1)
        for lo in range(0, n * (L + 1) * V, step):
            ids = torch.arange(lo, min(lo + step, n * (L + 1) * V), device=dev)
            seq, gap, tok = ids // ((L + 1) * V), (ids // V) % (L + 1), ids % V
            src = (k - (k > gap[:, None]).long()).clamp_(max=L - 1)             # k < g reads k, k > g reads k - 1 ...
            mut = torch.gather(tokens[seq], 1, src)
            mut[torch.arange(ids.shape[0], device=dev), gap] = tok.to(torch.uint8)      # ... and k == g is the new token
            mlen = lens_dev[seq] + (gap <= lens_dev[seq]).long()               # (no such gap: the sequence itself, overwritten below)
            flat[lo:lo + step] = project(mut, mlen.to(torch.int32).cpu().numpy()) - base[seq]
        # the contract's zeros (no such position or gap) and NaNs (a deletion that leaves no window)
        pos = torch.arange(L, device=dev)[None, :]
        dele.masked_fill_((lens_dev[:, None] == cw) & (pos < lens_dev[:, None]), float("nan"))
        dele.masked_fill_(pos >= lens_dev[:, None], 0.0)
        ins.masked_fill_((k > lens_dev[:, None])[:, :, None], 0.0)
        return dele, ins

    # ---- the exact quadratic form of the predictive variance of every single-token deletion and insertion
    def indel_variance_scan(self, batch, sequence_length, var):
        """(deletions [n, L], insertions [n, L + 1, V]), float64 device tensors: ``z'^T var z'`` for the first
        ``nvar = var.shape[0]`` columns z' of ``transform_x(mutant)``, for the sequence without its token at position p and for the
        sequence with row v of the TokenBatch's table inserted before position g (g = length appends) -- what
        ``xGPRegression.predict`` turns into the variance.  Exactly 0 for p >= length and g > length; the deletions of a sequence of
        exactly conv_width tokens (no window left) are NaN.  An indel changes the window count and with it the k-mer normaliser:
        the mutant's columns are b + r' delta with b the sequence's own columns rescaled by rho = r' / r (column 0 stays the
        constant 1 under the intercept) and delta built from the about 2 conv_width - 1 windows at the edit site, so one pair of
        HIP kernels per slab of mutants (``ext.hipConvTokenIndelVarScan``) transforms those windows of one 1024-frequency tile and
        contracts the delta rows with ``var`` on the float64 matrix cores.  The sequences' own columns come from
        ``fill_feature_rows`` (float32 rows, widened), rho from the host lengths in float64; any ``var`` is accepted through
        1/2 (var + var^T) in the cross term, and an odd nvar is padded with a zero row and column.  Where
        ``ext.conv_token_indel_var_scan_ok`` is 0 (windows of more than 1024 elements, a table the LDS image does not hold,
        nvar > 2048) or the tokens are not contiguous the result comes from ``indel_variance_scan_composed``."""
        xs, lengths, vm = self._var_scan_inputs(batch, sequence_length, var)
        n, L, _ = xs.shape
        V = xs.table.shape[0]
        columns = self._var_scan_columns(xs, lengths, vm, ext.conv_token_indel_var_scan_ok, check_lengths=True)
        if columns is None:
            return self._indel_var_composed(xs, lengths, vm)
        vp, z = columns
        nk = lengths.astype(np.float64) - self.conv_width + 1
        halves = []
        for nkm in (np.maximum(nk - 1, 1), nk + 1):      # (nk - 1 == 0: no mutant, the outputs are NaN whatever rho is)
            ratio = nk / nkm
            rho = {0: np.ones_like(ratio), 1: np.sqrt(ratio), 2: ratio}[self.scaling_type]
            b = z * torch.from_numpy(rho).to(self.device)[:, None]
            if self.fit_intercept:
                b[:, 0] = 1.0                            # rho 1 + (1 - rho): the constant column is not rescaled
            bv = b @ vp.T                                # row i: var b_i
            halves += [(0.5 * (bv + b @ vp)).contiguous(), (b * bv).sum(dim=1).contiguous()]
        dele = torch.empty((n, L), dtype=torch.float64, device=self.device)
        ins = torch.empty((n, L + 1, V), dtype=torch.float64, device=self.device)
        ext.hipConvTokenIndelVarScan(xs.tokens, xs.table.contiguous(), vp, halves[0], halves[1], halves[2], halves[3], dele, ins,
                                     self.radem_diag, self.chi_arr, lengths, self.conv_width, self.scaling_type, self.fit_intercept)
        return dele, ins

    def indel_variance_scan_composed(self, batch, sequence_length, var):
        """The same result from existing operators, at every window width, table size and nvar: bounded slices of deletion and
        insertion mutants are written out as token rows of L + 1 positions, ``fill_feature_rows`` makes their float32 feature rows,
        the quadratic form of their first nvar columns with ``var`` is taken in float64 with torch, and the zeros and NaNs of the
        contract are applied.  At most ``COMPOSED_SCAN_ELEMS`` float32 row elements are held at a time."""
        return self._indel_var_composed(*self._var_scan_inputs(batch, sequence_length, var))

    def _indel_var_composed(self, xs, lengths, vm):
        n, L, _ = xs.shape
        V, cw, dev, nvar = xs.table.shape[0], self.conv_width, self.device, vm.shape[0]
        self._check_lengths(lengths, n, L)
        tokens, lens_dev = xs.tokens.contiguous(), torch.from_numpy(lengths).to(dev).long()
        step = max(1, self.COMPOSED_SCAN_ELEMS // self.num_rffs)
        k = torch.arange(L + 1, device=dev)[None, :]

        def quad(tok, lens):
            rows = torch.empty((tok.shape[0], self.num_rffs), dtype=torch.float32, device=dev)
            self.fill_feature_rows(TokenBatch(tok.contiguous(), xs.table), lens, rows)
            xv = rows[:, :nvar].to(torch.float64)
            return (xv * (xv @ vm.T)).sum(dim=1)

        dele = torch.empty((n, L), dtype=torch.float64, device=dev)
        flat = dele.view(-1)
        for lo in range(0, n * L, step):
            ids = torch.arange(lo, min(lo + step, n * L), device=dev)
            seq, pos = ids // L, ids % L
            pos = torch.where(lens_dev[seq] > cw, pos, L + 1)                   # (no mutant: the sequence itself, overwritten below)
            src = (k + (k >= pos[:, None]).long()).clamp_(max=L - 1)            # position k of the mutant reads k + (k >= p)
            mut = torch.gather(tokens[seq], 1, src)
            mlen = (lens_dev[seq] - 1).clamp_(min=cw)                           # (entries with no mutant are overwritten below)
            flat[lo:lo + step] = quad(mut, mlen.to(torch.int32).cpu().numpy())
        ins = torch.empty((n, L + 1, V), dtype=torch.float64, device=dev)
        flat = ins.view(-1)
        for lo in range(0, n * (L + 1) * V, step):
            ids = torch.arange(lo, min(lo + step, n * (L + 1) * V), device=dev)
            seq, gap, tok = ids // ((L + 1) * V), (ids // V) % (L + 1), ids % V
            src = (k - (k > gap[:, None]).long()).clamp_(max=L - 1)             # k < g reads k, k > g reads k - 1 ...
            mut = torch.gather(tokens[seq], 1, src)
            mut[torch.arange(ids.shape[0], device=dev), gap] = tok.to(torch.uint8)      # ... and k == g is the new token
            mlen = lens_dev[seq] + (gap <= lens_dev[seq]).long()               # (no such gap: the sequence itself, overwritten below)
            flat[lo:lo + step] = quad(mut, mlen.to(torch.int32).cpu().numpy())
        # the contract's zeros (no such position or gap) and NaNs (a deletion that leaves no window)
        pos = torch.arange(L, device=dev)[None, :]
        dele.masked_fill_((lens_dev[:, None] == cw) & (pos < lens_dev[:, None]), float("nan"))
        dele.masked_fill_(pos >= lens_dev[:, None], 0.0)
        ins.masked_fill_((k > lens_dev[:, None])[:, :, None], 0.0)
        return dele, ins

    # ---- the projection of every single edit's columns on a caller's matrix: the joint posterior of the neighbourhood
    def _proj_scan_inputs(self, batch, sequence_length, proj):
        if not isinstance(batch, TokenBatch):
            raise RuntimeError("the projection scans need sequences given as tokens (a TokenBatch).")
        xs = self.scaled_f32(batch)
        lengths = self._host_lengths(xs, sequence_length)
        if lengths.shape[0] != xs.shape[0]:
            raise RuntimeError("sequence_length must hold one length per sequence.")
        pm = proj if isinstance(proj, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(proj))
        pm = pm.to(self.device, torch.float64)
        if pm.dim() != 2 or not 1 <= pm.shape[0] <= self.num_rffs or pm.shape[1] < 1:
            raise RuntimeError("proj must be a matrix [nvar, K] over the first 1 .. num_rffs feature columns, K >= 1.")
        return xs, lengths, pm

    def _proj_scan_columns(self, xs, lengths, pm):
        """What the two projection scans feed their operator from -> (``proj`` padded with a zero row to an even nvar, the sequences'
        own first columns: float32 rows of ``fill_feature_rows``, widened), or None where ``ext.conv_token_edit_proj_ok`` is 0 or the
        tokens are not contiguous: the composed route."""
        n, L, C = xs.shape
        nvar, K = pm.shape
        npad = nvar + (nvar & 1)
        if not (xs.is_cuda and xs.tokens.is_contiguous()
                and ext.conv_token_edit_proj_ok(self.conv_width * C, xs.table.shape[0], C, self.num_freqs, npad, K) == 1):
            return None
        self._check_lengths(lengths, n, L)
        pp = torch.zeros((npad, K), dtype=torch.float64, device=self.device)
        pp[:nvar] = pm
        rows = torch.empty((n, self.num_rffs), dtype=torch.float32, device=self.device)
        self.fill_feature_rows(xs, lengths, rows)
        return pp, rows[:, :npad].to(torch.float64)

    def substitution_projection_scan(self, batch, sequence_length, proj):
        """float64 device tensor [n, L, V, K]: ``z'^T proj`` for the first ``nvar = proj.shape[0]`` columns z' of
        ``transform_x(sequence with token l replaced by v)``, for every position l and every row v of the TokenBatch's table.  With
        ``proj`` a factor of ``var`` (factor factor^T = var) the rows are a factor of the JOINT posterior covariance of all the
        mutants -- ``substitution_variance_scan`` is their squared norms --; with ``proj = factor @ E`` for standard normal E they
        are joint draws; with ``proj = var @ z*`` covariances with chosen sequences.  Exactly 0 past a sequence's length; the
        sequence's own projection at its own token.  The delta kernels of ``substitution_variance_scan`` and one matrix-core kernel
        per slab of mutants (``ext.hipConvTokenSubstProj``); the sequences' own columns come from ``fill_feature_rows`` (float32
        rows, widened); an odd nvar is padded with a zero row.  Where ``ext.conv_token_edit_proj_ok`` is 0 (windows of more than
        1024 elements, a table the LDS image does not hold, nvar or K > 2048) or the tokens are not contiguous the result comes from
        ``substitution_projection_scan_composed``."""
        xs, lengths, pm = self._proj_scan_inputs(batch, sequence_length, proj)
        columns = self._proj_scan_columns(xs, lengths, pm)
        if columns is None:
            return self._subst_proj_composed(xs, lengths, pm)
        pp, z = columns
        n, L, _ = xs.shape
        out = torch.empty((n, L, xs.table.shape[0], pm.shape[1]), dtype=torch.float64, device=self.device)
        ext.hipConvTokenSubstProj(xs.tokens, xs.table.contiguous(), pp, (z @ pp).contiguous(), out, self.radem_diag, self.chi_arr,
                                  lengths, self.conv_width, self.scaling_type, self.fit_intercept)
        return out

    def indel_projection_scan(self, batch, sequence_length, proj):
        """(deletions [n, L, K], insertions [n, L + 1, V, K]), float64 device tensors: ``z'^T proj`` for the first
        ``nvar = proj.shape[0]`` columns z' of ``transform_x(mutant)``, for the sequence without its token at position p and for
        the sequence with row v of the TokenBatch's table inserted before position g (g = length appends); see
        ``substitution_projection_scan`` for what ``proj`` makes of it.  Exactly 0 for p >= length and g > length; the deletions of
        a sequence of exactly conv_width tokens (no window left) are NaN.  The mutant's columns are b + r' delta as in
        ``indel_variance_scan`` (rho from the host lengths in float64); the delta kernels of that scan and one matrix-core kernel
        per slab (``ext.hipConvTokenIndelProj``).  Where ``ext.conv_token_edit_proj_ok`` is 0 or the tokens are not contiguous the
        result comes from ``indel_projection_scan_composed``."""
        xs, lengths, pm = self._proj_scan_inputs(batch, sequence_length, proj)
        columns = self._proj_scan_columns(xs, lengths, pm)
        if columns is None:
            return self._indel_proj_composed(xs, lengths, pm)
        pp, z = columns
        n, L, _ = xs.shape
        V, K = xs.table.shape[0], pm.shape[1]
        nk = lengths.astype(np.float64) - self.conv_width + 1
        base = []
        for nkm in (np.maximum(nk - 1, 1), nk + 1):      # (nk - 1 == 0: no mutant, the outputs are NaN whatever rho is)
            ratio = nk / nkm
            rho = {0: np.ones_like(ratio), 1: np.sqrt(ratio), 2: ratio}[self.scaling_type]
            b = z * torch.from_numpy(rho).to(self.device)[:, None]
            if self.fit_intercept:
                b[:, 0] = 1.0                            # rho 1 + (1 - rho): the constant column is not rescaled
            base.append((b @ pp).contiguous())
        dele = torch.empty((n, L, K), dtype=torch.float64, device=self.device)
        ins = torch.empty((n, L + 1, V, K), dtype=torch.float64, device=self.device)
        ext.hipConvTokenIndelProj(xs.tokens, xs.table.contiguous(), pp, base[0], base[1], dele, ins, self.radem_diag, self.chi_arr,
                                  lengths, self.conv_width, self.scaling_type, self.fit_intercept)
        return dele, ins

    def substitution_projection_scan_composed(self, batch, sequence_length, proj):
        """The same result from existing operators, at every window width, table size, nvar and K: a bounded slice of (sequence,
        position, token) mutants is written out as token rows, ``fill_feature_rows`` makes their float32 feature rows, and their
        first nvar columns are multiplied with ``proj`` in float64 with torch.  At most ``COMPOSED_SCAN_ELEMS`` float32 row
        elements are held at a time."""
        return self._subst_proj_composed(*self._proj_scan_inputs(batch, sequence_length, proj))

    def indel_projection_scan_composed(self, batch, sequence_length, proj):
        """The same result from existing operators: bounded slices of deletion and insertion mutants are written out as token
        rows of L + 1 positions, ``fill_feature_rows`` makes their float32 feature rows, their first nvar columns are multiplied
        with ``proj`` in float64 with torch, and the zeros and NaNs of the contract are applied.  At most ``COMPOSED_SCAN_ELEMS``
        float32 row elements are held at a time."""
        return self._indel_proj_composed(*self._proj_scan_inputs(batch, sequence_length, proj))

    def _row_projector(self, table, pm):
        """f(token rows, int32 host lengths) -> the first nvar columns of their feature rows times pm, float64 [m, K]."""
        def project(tok, lens):
            rows = torch.empty((tok.shape[0], self.num_rffs), dtype=torch.float32, device=self.device)
            self.fill_feature_rows(TokenBatch(tok.contiguous(), table), lens, rows)
            return rows[:, :pm.shape[0]].to(torch.float64) @ pm
        return project

    def _subst_proj_composed(self, xs, lengths, pm):
        n, L, _ = xs.shape
        V, dev, K = xs.table.shape[0], self.device, pm.shape[1]
        self._check_lengths(lengths, n, L)
        project = self._row_projector(xs.table, pm)
        tokens, lens_dev = xs.tokens.contiguous(), torch.from_numpy(lengths).to(dev)
        step = max(1, self.COMPOSED_SCAN_ELEMS // max(self.num_rffs, K))
        out = torch.empty((n, L, V, K), dtype=torch.float64, device=dev)
        flat = out.view(-1, K)
        for lo in range(0, n * L * V, step):
            ids = torch.arange(lo, min(lo + step, n * L * V), device=dev)
            seq, pos, tok = ids // (L * V), (ids // V) % L, ids % V
            mut = tokens[seq]
            # (a position past the length: the token lands outside the sequence and is never read; zeroed below)
            mut[torch.arange(ids.shape[0], device=dev), pos] = tok.to(torch.uint8)
            flat[lo:lo + step] = project(mut, lengths[seq.cpu().numpy()])
        past = torch.arange(L, device=dev)[None, :] >= lens_dev[:, None]
        return out.masked_fill_(past[:, :, None, None], 0.0)

    def _indel_proj_composed(self, xs, lengths, pm):
        n, L, _ = xs.shape
        V, cw, dev, K = xs.table.shape[0], self.conv_width, self.device, pm.shape[1]
        self._check_lengths(lengths, n, L)
        project = self._row_projector(xs.table, pm)
        tokens, lens_dev = xs.tokens.contiguous(), torch.from_numpy(lengths).to(dev).long()
        step = max(1, self.COMPOSED_SCAN_ELEMS // max(self.num_rffs, K))
        k = torch.arange(L + 1, device=dev)[None, :]
        dele = torch.empty((n, L, K), dtype=torch.float64, device=dev)
        flat = dele.view(-1, K)
        for lo in range(0, n * L, step):
            ids = torch.arange(lo, min(lo + step, n * L), device=dev)
            seq, pos = ids // L, ids % L
            pos = torch.where(lens_dev[seq] > cw, pos, L + 1)                   # (no mutant: the sequence itself, overwritten below)
            src = (k + (k >= pos[:, None]).long()).clamp_(max=L - 1)            # position k of the mutant reads k + (k >= p)
            mut = torch.gather(tokens[seq], 1, src)
            mlen = (lens_dev[seq] - 1).clamp_(min=cw)                           # (entries with no mutant are overwritten below)
            flat[lo:lo + step] = project(mut, mlen.to(torch.int32).cpu().numpy())
        ins = torch.empty((n, L + 1, V, K), dtype=torch.float64, device=dev)
        flat = ins.view(-1, K)
        for lo in range(0, n * (L + 1) * V, step):
            ids = torch.arange(lo, min(lo + step, n * (L + 1) * V), device=dev)
            seq, gap, tok = ids // ((L + 1) * V), (ids // V) % (L + 1), ids % V
            src = (k - (k > gap[:, None]).long()).clamp_(max=L - 1)             # k < g reads k, k > g reads k - 1 ...
            mut = torch.gather(tokens[seq], 1, src)
            mut[torch.arange(ids.shape[0], device=dev), gap] = tok.to(torch.uint8)      # ... and k == g is the new token
            mlen = lens_dev[seq] + (gap <= lens_dev[seq]).long()               # (no such gap: the sequence itself, overwritten below)
            flat[lo:lo + step] = project(mut, mlen.to(torch.int32).cpu().numpy())
        # the contract's zeros (no such position or gap) and NaNs (a deletion that leaves no window)
        pos = torch.arange(L, device=dev)[None, :]
        dele.masked_fill_(((lens_dev[:, None] == cw) & (pos < lens_dev[:, None]))[:, :, None], float("nan"))
        dele.masked_fill_((pos >= lens_dev[:, None])[:, :, None], 0.0)
        ins.masked_fill_((k > lens_dev[:, None])[:, :, None, None], 0.0)
        return dele, ins

    def grad_rows_ok(self):
        """Whether ``fill_grad_rows`` can write this kernel's float32 feature AND gradient rows, and the exact NMLL
        gradient's accumulations can run on them (nmll.calc_gradient_terms): a HIP device -- the writer serves every
        window width the float64 gradient operator serves -- and whole 128 x 128 tiles for the two Gram kernels."""
        return torch.device(self.device).type == "cuda" and ext.cross_gram_ok(self.num_rffs)

    def fill_grad_rows(self, x_unscaled, zrows, grows, sequence_length):
        """zrows, grows [w, M] float32 <- the complete feature rows and d(features)/d(sigma) rows of the UNSCALED float32
        sequences: ``gradient_x`` rounded once to float32 (its entries are float64 sums over k-mers of float32 values),
        intercept column included.  Both overwritten."""
        lengths, sigma = self._host_lengths(x_unscaled, sequence_length), float(self.hyperparams[1])
        if isinstance(x_unscaled, TokenBatch):       # (the UNSCALED table, as x is)
            if self.token_rows_ok(x_unscaled):
                ext.hipConvTokenGradRows(x_unscaled.tokens, x_unscaled.table, zrows, grows, self.radem_diag, self.chi_arr,
                                         lengths, sigma, self.conv_width, self.scaling_type, self.fit_intercept)
                return
            for lo, hi, xd, lens in self._dense_slices(x_unscaled, lengths):
                ext.hipConvGradRows(xd, zrows[lo:hi], grows[lo:hi], self.radem_diag, self.chi_arr, lens, sigma,
                                    self.conv_width, self.scaling_type, self.fit_intercept)
            return
        ext.hipConvGradRows(x_unscaled, zrows, grows, self.radem_diag, self.chi_arr, lengths, sigma, self.conv_width,
                            self.scaling_type, self.fit_intercept)

    def transform_x(self, input_x, sequence_length=None, rows_out=None, pre_scaled=False):
        """kernel_baseclass.py:269-299 -> float64 [n, M] as for every kernel.  With ``rows_out`` (float32 [n, M] on the
        device) the same features are written there as float32 rows by ``fill_feature_rows`` -- no float64 array is made --
        and ``rows_out`` is returned; ``pre_scaled``: ``input_x`` already is the float32 sigma-scaled copy
        (``dataset.scaled_x``), so it is not scaled again."""
        if rows_out is None:
            return super().transform_x(input_x, sequence_length)
        xin = input_x if pre_scaled else self.scaled_f32(input_x)
        self.fill_feature_rows(xin, sequence_length, rows_out)
        return rows_out

    CACHE_BUILD_ROWS = 8192          # sequences per float64 slice where the cache is still the rounding of float64 features
                                     # (_cache_from_transform_x: a CPU device, a dataset class without a resident shard)

    def build_feature_cache(self, dataset):
        if not hasattr(dataset, "get_xdata") or not hasattr(dataset, "scaled_x") or not self.seq_rows_ok():
            return _cache_from_transform_x(self, dataset)
        # one call over the shard: no float64 temporary, and the longest-first order (conv_order_kernel) spans the
        # whole shard -- a wave runs for as long as its sequence has k-mers, and in the caller's order the long
        # sequences at the end of a launch leave most of the GPU idle
        n = dataset.get_local_ndatapoints()
        zc = torch.empty((n, self.num_rffs), dtype=torch.float32, device=self.device)
        if n > 0:
            # (no sequence lengths: the reference's "sequence_length is required" error)
            self.transform_x(dataset.scaled_x(self.hyperparams[1]), dataset.get_sequence_lengths(), rows_out=zc,
                             pre_scaled=True)
        return zc

    def zty_cached(self, zcache, y, out, workspace):
        """out <- Z^T y from complete float32 rows of this kernel (the resident cache or a regenerated window)."""
        ext.hipZCacheZtY(zcache, y, out, False, workspace, 1.0)

    def ztz_matvec_cached(self, zcache, vec, out, workspace):
        ext.hipZCacheMatvecScaled(zcache, vec, out, 1.0, workspace)

    def half_cache_ok(self):
        """Whether the k <= 2 matvec can stream this kernel's rows rounded to binary16 (cache_features="half")."""
        return self.seq_rows_ok() and ext.half_cache_ok(self.num_freqs)

    def ztz_matvec_cached_f16(self, zc16, vec, out, workspace):
        """the rows are complete (intercept column included): the scaled entry with 1.0"""
        ext.hipZCacheMatvecHalfScaled(zc16, vec, out, 1.0, workspace)

    def block_ok(self):
        return self.num_rffs % 4 == 0

    def ztz_block_cached(self, zcache, vecs, out, workspace, accumulate=False):
        _block_matvec(zcache, vecs, out, workspace, False, 1.0, accumulate)

    def row_cache_params(self):
        """the convolution cache holds complete feature rows (intercept column included): Z = 1.0 * rows"""
        return False, 1.0

    def cache_rows_to_features(self, zrows):
        """the convolution cache holds complete feature rows rounded to float32"""
        return zrows.to(torch.float64)

    def workspace_bytes(self):
        return ext.ztz_workspace_bytes(self.num_rffs, self.radem_diag.shape[2])

    def kernel_specific_gradient(self, input_x, sequence_length):
        """conv_kernel_baseclass.py:157-190."""
        if sequence_length is None:
            raise RuntimeError("sequence_length is required for convolution kernels.")
        if input_x.shape[2] != self._xdim[2]:
            raise RuntimeError("Unexpected input shape supplied.")
        if isinstance(sequence_length, torch.Tensor):
            sequence_length = sequence_length.cpu().numpy()
        slen = np.ascontiguousarray(sequence_length.astype(np.int32, copy=False))
        n = input_x.shape[0]
        xtrans = torch.zeros((n, self.num_rffs), dtype=torch.float64, device=self.device)
        dz_dsigma = torch.zeros((n, self.num_rffs, 1), dtype=torch.float64, device=self.device)
        ext.hipConvGrad(input_x, xtrans, self.radem_diag, self.chi_arr, slen, dz_dsigma,
                        float(self.hyperparams[1]), self.conv_width, self.scaling_type)
        return xtrans, dz_dsigma

    def kernel_specific_transform(self, input_x, sequence_length):
        """conv_kernel_baseclass.py:116-147."""
        if sequence_length is None:
            raise RuntimeError("sequence_length is required for convolution kernels.")
        if input_x.shape[2] != self._xdim[2]:
            raise RuntimeError("Unexpected input shape supplied.")
        if isinstance(sequence_length, torch.Tensor):
            sequence_length = sequence_length.cpu().numpy()
        slen = np.ascontiguousarray(sequence_length.astype(np.int32, copy=False))
        xtrans = torch.zeros((input_x.shape[0], self.num_rffs), dtype=torch.float64, device=self.device)
        ext.hipConv1dFGen(input_x, xtrans, self.radem_diag, self.chi_arr, slen,
                          self.conv_width, self.scaling_type)
        return xtrans


def _cache_from_transform_x(kernel, dataset):
    """The float32 cache of complete feature rows as the rounding of ``transform_x`` output (the two-layer kernel; the
    sequence kernels on a CPU device or over a dataset class without a resident shard): in windows of up to
    ``ConvSORFKernel.CACHE_BUILD_ROWS`` sequences rather than the dataset's chunks (1024 sequences in BASELINE configs[3]) -- one wave per
    (sequence, tile) runs for as long as its sequence has k-mers, and with 3 launch-rounds of waves per chunk the long
    sequences at the end of a launch leave most of the GPU idle."""
    n = dataset.get_local_ndatapoints()
    zc = torch.empty((n, kernel.num_rffs), dtype=torch.float32, device=kernel.device)
    if not hasattr(dataset, "get_xdata"):        # any other dataset class: its own chunks
        lo = 0
        for xdata, ldata in dataset.get_chunked_x_data():
            zc[lo:lo + xdata.shape[0]] = kernel.transform_x(xdata, ldata).to(torch.float32)
            lo += xdata.shape[0]
        return zc
    xall, lall = dataset.get_xdata(), dataset.get_sequence_lengths()
    step = max(1, min(ConvSORFKernel.CACHE_BUILD_ROWS, (1 << 30) // (8 * kernel.num_rffs)))      # float64 temporary <= 1 GiB
    for lo in range(0, n, step):
        hi = min(lo + step, n)
        # (no sequence lengths: transform_x raises the reference's "sequence_length is required" error)
        zc[lo:hi] = kernel.transform_x(xall[lo:hi], None if lall is None else lall[lo:hi]).to(torch.float32)
    return zc


class LinearKernel:
    """kernels/basic_kernels/linear.py: Bayesian linear regression -- the "features" are the input itself
    (rounded to float32 by the private copy of kernel_baseclass.py:274-288, widened to float64), with a
    leading column of ones for the intercept.  No random features, no operator of the library; here so that
    every kernel name of the reference's registry (kernels/__init__.py:21-33) resolves."""
    supports_fused = False
    kernel_choice = "Linear"

    def __init__(self, xdim, num_rffs=None, random_seed=123, device="cuda", kernel_spec_parms=None):
        kernel_spec_parms = kernel_spec_parms or {}
        if len(xdim) > 2:
            raise ValueError("The Linear kernel is only applicable for fixed vector input.")
        self.fit_intercept = kernel_spec_parms.get("intercept", True) is not False
        self.num_rffs = xdim[1] + (1 if self.fit_intercept else 0)
        self._xdim, self.device, self.random_seed = tuple(xdim), device, random_seed
        self.kernel_spec_parms = dict(kernel_spec_parms)
        self.hyperparams = np.ones((1))

    get_hyperparams = KernelBase.get_hyperparams
    set_hyperparams = KernelBase.set_hyperparams
    get_lambda = KernelBase.get_lambda
    get_num_rffs = KernelBase.get_num_rffs
    transform_x_y = KernelBase.transform_x_y
    gradient_x_y = KernelBase.gradient_x_y
    _as_device = KernelBase._as_device
    _as_device_f32 = KernelBase._as_device_f32

    def fused_ok(self):
        return False

    def transform_x(self, input_x, sequence_length=None):
        xin = self._as_device_f32(input_x).to(torch.float32)
        if not self.fit_intercept:
            return xin.to(torch.float64)
        xtrans = torch.zeros((xin.shape[0], xin.shape[1] + 1), dtype=torch.float64, device=self.device)
        xtrans[:, 1:] = xin
        xtrans[:, 0] = 1.
        return xtrans

    def gradient_x(self, input_x, sequence_length=None):
        xtrans = self.transform_x(input_x)
        return xtrans, torch.zeros((xtrans.shape[0], 0, 0), dtype=torch.float64, device=self.device)

    def input_gradient(self, input_x, weights, w_cols=None):
        """float64 device tensor [n, d]: d/dx of ``transform_x(x) @ weights`` -- the weight columns that multiply x (the
        intercept column is skipped), one vector for all rows or one row per datapoint; feature columns at or beyond
        ``w_cols`` carry no weight.  The features are the input itself, so there is no operator to run."""
        n, d = input_x.shape[0], self._xdim[1]
        w = weights if isinstance(weights, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(weights))
        w = w.to(self.device, torch.float64)
        if w.dim() not in (1, 2) or (w.dim() == 2 and w.shape[0] != n):
            raise RuntimeError("weights must be one vector, or one row per datapoint.")
        w_cols = min(w.shape[-1], self.num_rffs) if w_cols is None else int(w_cols)
        if w_cols < 1 or w_cols > min(w.shape[-1], self.num_rffs):
            raise RuntimeError("w_cols must be >= 1 and within the weights and the features.")
        first = 1 if self.fit_intercept else 0
        out = torch.zeros((n, d), dtype=torch.float64, device=self.device)
        if w_cols > first:
            out[:, :w_cols - first] = w[..., first:w_cols]
        return out


class Conv1dTwoLayerKernel(KernelBase):
    """kernels/convolution_kernels/l2_conv1d.py:16-222: a convolution layer with global max-pooling
    (hipConv1dMaxpool: ``init_rffs`` ReLU'd random convolution filters per sequence) whose output feeds an RBF
    kernel (hipRBFFeatureGen / hipRBFGrad); sigma scales the pooled features."""

    def __init__(self, xdim, num_rffs, random_seed=123, device="cuda", kernel_spec_parms=None):
        kernel_spec_parms = kernel_spec_parms or {}
        if "conv_width" not in kernel_spec_parms:
            raise ValueError("conv_width must be included as a kernel-specific "
                             "parameter if using a sequence kernel.")
        if "init_rffs" not in kernel_spec_parms:
            raise ValueError("init_rffs must be included as a kernel-specific "
                             "parameter if using the 2 layer conv1d kernel.")
        if len(xdim) != 3:
            raise RuntimeError("Tried to initialize a Conv1d kernel with a 2d x-"
                               "array! x should be a 3d array for Conv1d.")
        self.init_rffs = kernel_spec_parms["init_rffs"]
        if self.init_rffs % 2 != 0:
            raise RuntimeError("Number of init rffs should be an even number.")
        super().__init__(num_rffs, xdim, kernel_spec_parms, device)
        self.random_seed = random_seed
        self.kernel_choice = "Conv1dTwoLayer"
        rng = np.random.default_rng(random_seed)
        self.conv_width = kernel_spec_parms["conv_width"]
        pdims = padded_dims(self.conv_width * xdim[2])
        init_calc_featsize = ceil(self.init_rffs / pdims) * pdims
        radem_array = np.asarray([-1, 1], dtype=np.int8)
        radem1 = rng.choice(radem_array, size=(3, 1, init_calc_featsize), replace=True)
        chi1 = _chi.rvs(df=pdims, size=self.init_rffs, random_state=random_seed).astype(np.float32)
        pdims2 = padded_dims(self.init_rffs)
        nblocks = ceil(self.num_freqs / pdims2) if pdims2 < self.num_freqs else 1
        radem2 = rng.choice(radem_array, size=(3, 1, nblocks * pdims2), replace=True)
        chi2 = _chi.rvs(df=pdims2, size=self.num_freqs, random_state=random_seed).astype(np.float32)
        self.radem_diag1 = torch.from_numpy(np.ascontiguousarray(radem1)).to(device)
        self.chi_arr1 = torch.from_numpy(chi1).to(device)
        self._to_device(radem2, chi2)            # radem_diag / chi_arr = the second (RBF) layer

    supports_fused = False

    def fused_ok(self):
        return False

    def _pool_into(self, input_x, slen, out):
        """out [n, init_rffs] float32 (zero-filled by the caller: that is the ReLU) <- the max-pooled filters of ``input_x``:
        a float32 [n, L, C] device tensor, or a TokenBatch on the device -- read as it is where the token operator serves its
        shape (same bits as the dense array), otherwise expanded at most ``CACHE_BUILD_ROWS`` sequences at a time."""
        if not isinstance(input_x, TokenBatch):
            ext.hipConv1dMaxpool(input_x, out, self.radem_diag1, self.chi_arr1, slen, self.conv_width)
        elif (torch.device(self.device).type == "cuda" and input_x.is_cuda and input_x.tokens.is_contiguous()
              and ext.conv_token_rows_ok(self.conv_width * input_x.shape[2], input_x.table.shape[0], input_x.shape[2]) == 1):
            ext.hipConvTokenMaxpool(input_x.tokens, input_x.table, out, self.radem_diag1, self.chi_arr1, slen, self.conv_width)
        else:
            for lo in range(0, input_x.shape[0], ConvSORFKernel.CACHE_BUILD_ROWS):
                hi = min(lo + ConvSORFKernel.CACHE_BUILD_ROWS, input_x.shape[0])
                ext.hipConv1dMaxpool(input_x[lo:hi].dense().contiguous(), out[lo:hi], self.radem_diag1, self.chi_arr1,
                                     slen[lo:hi], self.conv_width)

    def _first_layer(self, input_x, sequence_length, out=None):
        if sequence_length is None:
            raise ValueError("sequence_length is required for convolution kernels.")
        if input_x.shape[2] != self._xdim[2]:
            raise RuntimeError("Unexpected input shape supplied.")
        if isinstance(sequence_length, torch.Tensor):
            sequence_length = sequence_length.cpu().numpy()
        slen = np.ascontiguousarray(sequence_length.astype(np.int32, copy=False))
        if out is None:
            out = torch.zeros((input_x.shape[0], self.init_rffs), dtype=torch.float32, device=self.device)
        self._pool_into(input_x, slen, out)
        return out

    def _private_f32(self, input_x):
        """The private float32 copy of a chunk on the device (kernel_baseclass.py:274-288); a TokenBatch moves to the device
        as it is -- the first layer reads tokens."""
        if isinstance(input_x, TokenBatch):
            return input_x.to(self.device)
        return self._as_device_f32(input_x).to(torch.float32, copy=True).contiguous()

    POOL_SLICE_ROWS = 65536          # sequences per call when a whole shard is pooled: a float64 or non-contiguous input is
                                     # converted slice by slice, never as a second shard-sized temporary

    def pool(self, input_x, sequence_length):
        """float32 [n, init_rffs]: the first layer of the kernel, max-pooled ReLU'd random convolution filters
        (l2_conv1d.py:150-185 before sigma is applied).  It depends on no hyperparameter, so a dataset can keep it
        (``DeviceDataset.pooled``).  ``input_x``: [n, L, C] floats (array or tensor, any device) or a TokenBatch; both are
        pooled in slices of ``POOL_SLICE_ROWS`` sequences."""
        if sequence_length is None:
            raise ValueError("sequence_length is required for convolution kernels.")
        if isinstance(input_x, np.ndarray):
            input_x = torch.from_numpy(input_x)
        n = input_x.shape[0]
        out = torch.zeros((n, self.init_rffs), dtype=torch.float32, device=self.device)
        for lo in range(0, n, self.POOL_SLICE_ROWS):
            hi = min(lo + self.POOL_SLICE_ROWS, n)
            xin = input_x[lo:hi]
            xin = xin.to(self.device) if isinstance(xin, TokenBatch) else xin.to(self.device, torch.float32).contiguous()
            self._first_layer(xin, sequence_length[lo:hi], out[lo:hi])
        return out

    def second_layer(self):
        """The second layer as a fixed-vector kernel over the pooled features: an RBF ``SORFKernel`` of xdim (n, init_rffs)
        whose ``transform_x`` / ``gradient_x`` of ``pool(x, sl)`` are this kernel's of (x, sl), bit for bit -- both end in the
        same operator call on the same sigma-scaled rows.  One view per kernel object (the dataset caches key on the kernel
        object); it shares the draws (the same tensors), the intercept flag, the feature count, the device and the
        hyperparameters, which either object may set."""
        if getattr(self, "_second", None) is None:
            self._second = _SecondLayerView(self)
        return self._second

    def transform_x(self, input_x, sequence_length=None):
        """kernel_baseclass.py:269-299 with l2_conv1d.py:150-185."""
        xin = self._private_f32(input_x)
        featurized_x = scale_input(self._first_layer(xin, sequence_length), self.hyperparams[1])
        xtrans = torch.zeros((featurized_x.shape[0], self.num_rffs), dtype=torch.float64, device=self.device)
        ext.hipRBFFeatureGen(featurized_x, xtrans, self.radem_diag, self.chi_arr, self.fit_intercept)
        if self.fit_intercept:
            xtrans[:, 0] = 1.
        return xtrans

    def gradient_x(self, input_x, sequence_length=None):
        """kernel_baseclass.py:328-361; token input goes to the first layer as it is."""
        xtrans, xgrad = self.kernel_specific_gradient(self._private_f32(input_x), sequence_length)
        if self.fit_intercept:
            xtrans[:, 0] = 1.
            xgrad[:, 0, :] = 0.
        return xtrans, xgrad

    def kernel_specific_gradient(self, input_x, sequence_length=None):
        """l2_conv1d.py:189-222."""
        featurized_x = self._first_layer(input_x, sequence_length)
        output_x = torch.zeros((input_x.shape[0], self.num_rffs), dtype=torch.float64, device=self.device)
        dz_dsigma = torch.zeros((input_x.shape[0], self.num_rffs, 1), dtype=torch.float64, device=self.device)
        ext.hipRBFGrad(featurized_x, output_x, dz_dsigma, self.radem_diag, self.chi_arr,
                       float(self.hyperparams[1]), self.fit_intercept)
        return output_x, dz_dsigma

    def grad_rows_ok(self):
        """As ``SORFKernel.grad_rows_ok`` for the second (RBF) layer, whose input is the ``init_rffs`` pooled features: a
        HIP device, a padded width hipRBFGradRows has a plan for, whole 128 x 128 tiles for the two Gram kernels."""
        return (torch.device(self.device).type == "cuda" and padded_dims(self.init_rffs) <= ext.GRAD_ROWS_MAX_WIDTH
                and ext.cross_gram_ok(self.num_rffs) and self.radem_diag.data_ptr() % 16 == 0)

    def fill_grad_rows(self, x_unscaled, zrows, grows, sequence_length):
        """zrows, grows [w, M] float32 <- ``gradient_x`` of the UNSCALED float32 sequences, exactly: the gradient is
        hipRBFGrad over the max-pooled float32 first-layer features, every entry of which is a float32 value.  A TokenBatch
        is pooled from its tokens (``_pool_into``)."""
        ext.hipRBFGradRows(self._first_layer(x_unscaled, sequence_length), zrows, grows, self.radem_diag, self.chi_arr,
                           float(self.hyperparams[1]), self.fit_intercept)

    # ---- derivative with respect to the INPUT, per position and channel: the second layer's input gradient
    # pushed back through the max-pool, the ReLU and the transposed SORF of the convolution filters
    COMPOSED_GRAD_ELEMS = ConvSORFKernel.COMPOSED_GRAD_ELEMS

    def _lengths(self, input_x, sequence_length):
        if sequence_length is None:
            raise ValueError("sequence_length is required for convolution kernels.")
        if input_x.shape[2] != self._xdim[2]:
            raise RuntimeError("Unexpected input shape supplied.")
        if isinstance(sequence_length, torch.Tensor):
            sequence_length = sequence_length.cpu().numpy()
        return np.ascontiguousarray(np.asarray(sequence_length).astype(np.int32, copy=False))

    def first_layer_gradient(self, input_x, sequence_length, g, return_argmax=False):
        """float64 device tensor [n, L, C]: d m / d x for any scalar m with ``g[i, f]`` = d m / d pool(x)[i, f] (float64, one
        vector [init_rffs] for all sequences or one row per sequence) at the UNSCALED sequences ``input_x`` (dense [n, L, C] or a
        TokenBatch).  Filter f sends g_f to the FIRST k-mer that attains its maximum, and nothing where that maximum is <= 0
        (ReLU inactive); the windows' gradients overlap-add per position and positions past a length are exactly 0.  With
        ``return_argmax`` also the int32 [n, init_rffs] winning k-mers (-1: inactive).  One HIP kernel where
        ``ext.conv_maxpool_input_grad_ok`` / ``ext.conv_token_maxpool_input_grad_ok`` hold; tokens over a larger table are
        expanded slice by slice; windows beyond 1024 elements, or a device without HIP, take ``first_layer_gradient_composed``."""
        xin = self._private_f32(input_x)
        lengths = self._lengths(xin, sequence_length)
        n, L, C = xin.shape
        gw = g if isinstance(g, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(g))
        gw = gw.to(self.device, torch.float64)
        if gw.dim() not in (1, 2) or (gw.dim() == 2 and gw.shape[0] != n) or gw.shape[-1] < self.init_rffs:
            raise RuntimeError("g must be one vector of init_rffs values, or one such row per sequence.")
        if gw.dim() == 1 or gw.stride(1) != 1:
            gw = gw.contiguous()
        out = torch.empty((n, L, C), dtype=torch.float64, device=self.device)
        argmax = torch.empty((n, self.init_rffs), dtype=torch.int32, device=self.device)
        on_hip = torch.device(self.device).type == "cuda"
        width = self.conv_width * C
        if isinstance(xin, TokenBatch):
            if (on_hip and xin.is_cuda and xin.tokens.is_contiguous()
                    and ext.conv_token_maxpool_input_grad_ok(width, xin.table.shape[0], C) == 1):
                ext.hipConvTokenMaxpoolInputGrad(xin.tokens, xin.table, gw, out, argmax, self.radem_diag1, self.chi_arr1, lengths,
                                                 self.conv_width)
            else:
                for lo in range(0, n, ConvSORFKernel.CACHE_BUILD_ROWS):
                    hi = min(lo + ConvSORFKernel.CACHE_BUILD_ROWS, n)
                    self._dense_first_layer_gradient(xin[lo:hi].dense().contiguous(), lengths[lo:hi],
                                                     gw if gw.dim() == 1 else gw[lo:hi], out[lo:hi], argmax[lo:hi], on_hip)
        else:
            self._dense_first_layer_gradient(xin, lengths, gw, out, argmax, on_hip)
        return (out, argmax) if return_argmax else out

    def _dense_first_layer_gradient(self, x, lengths, g, out, argmax, on_hip):
        if on_hip and ext.conv_maxpool_input_grad_ok(self.conv_width * x.shape[2]) == 1:
            ext.hipConvMaxpoolInputGrad(x, g, out, argmax, self.radem_diag1, self.chi_arr1, lengths, self.conv_width)
        else:
            o, a = self.first_layer_gradient_composed(x, lengths, g)
            out.copy_(o)
            argmax.copy_(a)

    def first_layer_gradient_composed(self, x, lengths, g):
        """(gradient [n, L, C] float64, argmax [n, init_rffs] int32) by the unfold route, at every window width, from existing
        operators: a bounded slice of sequences is unfolded into one-k-mer "sequences", ``hipConv1dMaxpool`` writes their ReLU'd
        projections into zero-filled rows, the first-index argmax over a sequence's k-mers masks g (.) chi, the rows go through
        ``transposed_sorf_rows`` and are folded back with conv_width slice additions in float64, window offset 0 first.
        ``x`` dense float32 [n, L, C], unscaled; ``lengths`` int32 on the host; ``g`` float64, one vector or one row each."""
        n, L, C = x.shape
        cw, F = self.conv_width, self.init_rffs
        d, nkmax = cw * C, L - cw + 1
        if int(lengths.min()) < cw or int(lengths.max()) > L:
            raise RuntimeError("All sequence lengths must be >= conv width and < array size.")
        p = padded_dims(d)
        R = self.radem_diag1.shape[2]
        nk = torch.from_numpy(lengths.astype(np.int64) - (cw - 1)).to(self.device)
        live = torch.arange(nkmax, device=self.device)[None, :] < nk[:, None]             # [n, nkmax]: window j is a k-mer
        chi = self.chi_arr1.to(torch.float64)
        out = torch.zeros((n, L, C), dtype=torch.float64, device=self.device)
        argmax = torch.empty((n, F), dtype=torch.int32, device=self.device)
        one_kmer = np.full(nkmax, cw, dtype=np.int32)
        step = max(1, self.COMPOSED_GRAD_ELEMS // (nkmax * max(R, F)))
        for lo in range(0, n, step):
            hi = min(lo + step, n)
            m = hi - lo
            wins = x[lo:hi].unfold(1, cw, 1).permute(0, 1, 3, 2).reshape(m * nkmax, cw, C).contiguous()
            proj = torch.zeros((m * nkmax, F), dtype=torch.float32, device=self.device)
            ext.hipConv1dMaxpool(wins, proj, self.radem_diag1, self.chi_arr1, np.tile(one_kmer, m), cw)
            proj = proj.view(m, nkmax, F) * live[lo:hi, :, None]                         # max(0, p_j) at the k-mers, 0 past them
            best, at = proj.max(dim=1)
            at = torch.argmax((proj == best[:, None, :]).to(torch.uint8), dim=1)          # the FIRST k-mer that attains it
            at = torch.where(best > 0, at, torch.full_like(at, -1))
            argmax[lo:hi] = at.to(torch.int32)
            gc = (g[None, :F] if g.dim() == 1 else g[lo:hi, :F]) * chi[None, :]
            hit = at[:, None, :] == torch.arange(nkmax, device=self.device)[None, :, None]
            t = torch.zeros((m, nkmax, R), dtype=torch.float64, device=self.device)
            t[:, :, :F] = torch.where(hit, gc[:, None, :].expand(m, nkmax, F), torch.zeros((), dtype=torch.float64, device=self.device))
            gw = transposed_sorf_rows(t.view(m * nkmax, R), self.radem_diag1, p)[:, :d].reshape(m, nkmax, cw, C)
            for q in range(cw):
                out[lo:hi, q:q + nkmax, :] += gw[:, :, q, :]
        out *= (torch.arange(L, device=self.device)[None, :] < torch.from_numpy(lengths).to(self.device)[:, None])[:, :, None]
        return out, argmax

    def input_gradient(self, input_x, sequence_length, weights, w_cols=None, pooled=None):
        """float64 device tensor [n, L, C]: d/dx of ``transform_x(x, sequence_length) @ weights`` at every position and channel of
        the UNSCALED sequences (dense or a TokenBatch); same signature and conventions as ``ConvSORFKernel.input_gradient``.
        The sequences are pooled once (or ``pooled`` = ``pool(input_x, sequence_length)`` is taken as given), the second layer's
        ``input_gradient`` of the pooled rows -- it carries sigma -- is the g of ``first_layer_gradient``."""
        if pooled is None:
            pooled = self.pool(input_x, sequence_length)
        g = self.second_layer().input_gradient(pooled, weights, w_cols)
        return self.first_layer_gradient(input_x, sequence_length, g)

    # ---- the exact effect of every single substitution, deletion and insertion: a maximum is order-free, so the
    # pooled row of a mutant is max(prefix maxima left of the edit, suffix maxima right of it, the ~conv_width windows it creates)
    EDITS = ("substitutions", "deletions", "insertions")
    POOL_EDITS_ELEMS = 1 << 26       # float32 elements of mutant pooled rows one slab holds (either route)
    EDIT_ROWS_ELEMS = 1 << 24        # float64 elements of second-layer features held at a time when a slab is reduced

    def _edit_inputs(self, batch, sequence_length, edit):
        if edit not in self.EDITS:
            raise RuntimeError("edit must be one of 'substitutions', 'deletions', 'insertions'.")
        if not isinstance(batch, TokenBatch):
            raise RuntimeError("pool_edits needs sequences given as tokens (a TokenBatch).")
        xs = batch.to(self.device)
        lengths = self._lengths(xs, sequence_length)
        n, L = xs.shape[0], xs.shape[1]
        if lengths.shape[0] != n:
            raise RuntimeError("sequence_length must hold one length per sequence.")
        if n and (int(lengths.min()) < self.conv_width or int(lengths.max()) > L):
            raise RuntimeError("All sequence lengths must be >= conv width and < array size.")
        return xs, lengths

    def _edit_geometry(self, xs, edit):
        """-> (slots per sequence, rows per slot, slots per slab): slabs are cut on slot boundaries."""
        L, V = xs.shape[1], xs.table.shape[0]
        slots, per = (L + 1 if edit == "insertions" else L), (1 if edit == "deletions" else V)
        return slots, per, int(min(max(1, self.POOL_EDITS_ELEMS // (per * self.init_rffs)), (1 << 24) - 1))

    def _pool_edits_operator_ok(self, xs):
        return bool(torch.device(self.device).type == "cuda" and xs.is_cuda and xs.tokens.is_contiguous()
                    and ext.conv_token_maxpool_edits_ok(self.conv_width * xs.shape[2], xs.table.shape[0], xs.shape[2],
                                                        self.init_rffs) == 1)

    def pool_edits(self, batch, sequence_length, edit):
        """Generator of (slot_lo, rows): the pooled first-layer rows (float32, what ``pool`` gives for the written-out mutant: equal
        everywhere, bit for bit wherever not zero) of EVERY single-token mutant of the TokenBatch ``batch``, slab by slab.  ``edit``
        "substitutions": slot = (sequence, position l), rows [nslots, V, init_rffs] -- token l replaced by table row v;
        "deletions": slot = (sequence, position p), rows [nslots, init_rffs] -- NaN for a sequence of exactly conv_width tokens;
        "insertions": slot = (sequence, gap g of L + 1), rows [nslots, V, init_rffs] -- row v inserted before g, g = the length
        appends.  Slots are numbered sequence-major, a slab holds at most ``POOL_EDITS_ELEMS`` elements, and slots past a sequence's
        length are exact zero rows.  The prefix / suffix maxima of the sequences' own windows are built once per call
        (``ext.hipConvTokenMaxpoolTables``) and a mutant costs its about conv_width new windows (``ext.hipConvTokenMaxpoolEdits``)
        instead of all of its windows; no mutant is written.  Where ``ext.conv_token_maxpool_edits_ok`` is 0, the tokens are not
        contiguous or there is no HIP device the slabs come from ``pool_edits_composed``."""
        xs, lengths = self._edit_inputs(batch, sequence_length, edit)
        if not self._pool_edits_operator_ok(xs):
            yield from self._pool_edits_composed(xs, lengths, edit)
            return
        n, L = xs.shape[0], xs.shape[1]
        slots, per, step = self._edit_geometry(xs, edit)
        F, table = self.init_rffs, xs.table.contiguous()
        pm = torch.empty((n, L - self.conv_width + 2, F), dtype=torch.float32, device=self.device)
        sm = torch.empty_like(pm)
        if n:
            ext.hipConvTokenMaxpoolTables(xs.tokens, table, pm, sm, self.radem_diag1, self.chi_arr1, lengths, self.conv_width)
        for lo in range(0, n * slots, step):
            cnt = min(step, n * slots - lo)
            rows = torch.empty((cnt, F) if edit == "deletions" else (cnt, per, F), dtype=torch.float32, device=self.device)
            ext.hipConvTokenMaxpoolEdits(xs.tokens, table, pm, sm, rows, self.radem_diag1, self.chi_arr1, lengths, self.conv_width,
                                         edit, lo, cnt)
            yield lo, rows

    def pool_edits_composed(self, batch, sequence_length, edit):
        """The same slabs from existing operators, at every window width and table size: a slab's mutants are written out as
        token rows (L + 1 positions for the indels) and pooled with ``_pool_into``; then the contract's zero rows (no such position
        or gap) and NaN rows (a deletion that leaves no window) are set.  Same slab boundaries as ``pool_edits``."""
        xs, lengths = self._edit_inputs(batch, sequence_length, edit)
        yield from self._pool_edits_composed(xs, lengths, edit)

    def _pool_edits_composed(self, xs, lengths, edit):
        n, L = xs.shape[0], xs.shape[1]
        cw, F, dev = self.conv_width, self.init_rffs, self.device
        slots, per, step = self._edit_geometry(xs, edit)
        tokens, lens_dev = xs.tokens.contiguous(), torch.from_numpy(lengths).to(dev).long()
        k = torch.arange(L + 1, device=dev)[None, :]
        for lo in range(0, n * slots, step):
            cnt = min(step, n * slots - lo)
            ids = torch.arange(lo * per, (lo + cnt) * per, device=dev)
            seq, site, tok = ids // (slots * per), (ids // per) % slots, ids % per
            slen = lens_dev[seq]
            if edit == "substitutions":
                mut = tokens[seq]
                mut[torch.arange(ids.shape[0], device=dev), site] = tok.to(torch.uint8)      # (past the length: never read)
                mlen, gone, nan = slen, site >= slen, None
            elif edit == "deletions":
                pos = torch.where(slen > cw, site, L + 1)                                 # (no mutant: the sequence itself, overwritten below)
                mut = torch.gather(tokens[seq], 1, (k + (k >= pos[:, None]).long()).clamp_(max=L - 1))
                mlen, gone = (slen - 1).clamp_(min=cw), site >= slen
                nan = (slen == cw) & ~gone
            else:
                mut = torch.gather(tokens[seq], 1, (k - (k > site[:, None]).long()).clamp_(max=L - 1))
                mut[torch.arange(ids.shape[0], device=dev), site] = tok.to(torch.uint8)
                mlen, gone, nan = slen + (site <= slen).long(), site > slen, None
            rows = torch.zeros((ids.shape[0], F), dtype=torch.float32, device=dev)
            self._pool_into(TokenBatch(mut.contiguous(), xs.table), mlen.to(torch.int32).cpu().numpy(), rows)
            if nan is not None:
                rows.masked_fill_(nan[:, None], float("nan"))
            rows.masked_fill_(gone[:, None], 0.0)
            yield lo, rows if edit == "deletions" else rows.view(cnt, per, F)

    def _edit_rows_results(self, rows, w, var, proj=None):
        """Pooled rows [m, init_rffs] float32 -> (features . w [m], z_v^T var z_v [m] or None, z_p^T proj [m, K] or None) in float64,
        through the second layer's own operators (``second_layer().transform_x``: sigma and the RBF features) at most
        ``EDIT_ROWS_ELEMS`` feature elements at a time.  The ONE place where a slab of either row source becomes results."""
        m = rows.shape[0]
        second = self.second_layer()
        mean = torch.empty(m, dtype=torch.float64, device=self.device)
        quad = None if var is None else torch.empty(m, dtype=torch.float64, device=self.device)
        pr = None if proj is None else torch.empty((m, proj.shape[1]), dtype=torch.float64, device=self.device)
        step = max(1, self.EDIT_ROWS_ELEMS // self.num_rffs)
        for lo in range(0, m, step):
            z = second.transform_x(rows[lo:lo + step])
            mean[lo:lo + step] = (z * w[None, :]).sum(dim=1)
            if var is not None:
                zv = z[:, :var.shape[0]]
                quad[lo:lo + step] = (zv * (var @ zv.T).T).sum(dim=1)
            if proj is not None:
                pr[lo:lo + step] = z[:, :proj.shape[0]] @ proj       # (the rows are there: a host-side product, no kernel of its own)
        return mean, quad, pr

    def edit_scan(self, batch, sequence_length, weights, edit, var=None, composed=False, proj=None):
        """float64 device tensor -- [n, L, V] for ``edit`` "substitutions", [n, L] for "deletions", [n, L + 1, V] for "insertions" --:
        ``transform_x(mutant) @ weights`` minus ``transform_x(sequence) @ weights`` for every single-token mutant of the
        TokenBatch, exact (the mutants' pooled rows are those of ``pool``; see ``pool_edits``).  Exactly 0 at a substitution's own
        token and for positions / gaps past the length; NaN for the deletions of a sequence of exactly conv_width tokens.  With
        ``var`` (nvar x nvar, float64) the return is (scan, quad): quad holds z'^T var z' of the mutant's first nvar second-layer
        features, the quadratic form of ``predict(get_var=True)`` (0 past the length, NaN where scan is).  With ``proj`` ([nvar, K],
        float64) a further tensor closes the return: z'^T proj of the mutant's first nvar second-layer features, [..., K] (0 past
        the length, NaN where scan is; the sequence's own projection at its own token) -- see
        ``ConvSORFKernel.substitution_projection_scan``.  ``composed`` takes the rows from ``pool_edits_composed``; both sources go
        through ``_edit_rows_results`` with the same slab boundaries."""
        xs, lengths = self._edit_inputs(batch, sequence_length, edit)
        w = weights if isinstance(weights, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(weights))
        w = w.to(self.device, torch.float64).contiguous()
        if w.dim() != 1 or w.shape[0] != self.num_rffs:
            raise RuntimeError("weights must be one vector of num_rffs values.")
        vm = None
        if var is not None:
            vm = (var if isinstance(var, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(var))).to(self.device, torch.float64)
            if vm.dim() != 2 or vm.shape[0] != vm.shape[1] or not 1 <= vm.shape[0] <= self.num_rffs:
                raise RuntimeError("var must be a square matrix over the first nvar <= num_rffs features.")
        pm = None
        if proj is not None:
            pm = (proj if isinstance(proj, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(proj))).to(self.device, torch.float64)
            if pm.dim() != 2 or not 1 <= pm.shape[0] <= self.num_rffs or pm.shape[1] < 1:
                raise RuntimeError("proj must be a matrix [nvar, K] over the first nvar <= num_rffs features, K >= 1.")
        n, L, V, dev = xs.shape[0], xs.shape[1], xs.table.shape[0], self.device
        slots, per, _ = self._edit_geometry(xs, edit)
        base = torch.zeros(0, dtype=torch.float64, device=dev)
        if n:
            base = self._edit_rows_results(self._first_layer(xs, lengths), w, None)[0]
        scan = torch.empty(n * slots * per, dtype=torch.float64, device=dev)
        quad = None if vm is None else torch.empty_like(scan)
        prj = None if pm is None else torch.empty((scan.shape[0], pm.shape[1]), dtype=torch.float64, device=dev)
        source = self._pool_edits_composed if composed or not self._pool_edits_operator_ok(xs) else self.pool_edits
        for lo, rows in source(xs, lengths, edit):
            rows = rows.reshape(-1, self.init_rffs)
            if edit == "deletions":
                rows = torch.nan_to_num(rows, nan=0.0)                                    # (set to NaN by definition below)
            mean, qd, pr = self._edit_rows_results(rows, w, vm, pm)
            ids = torch.arange(lo * per, lo * per + rows.shape[0], device=dev)
            scan[ids] = mean - base[ids // (slots * per)]
            if quad is not None:
                quad[ids] = qd
            if prj is not None:
                prj[ids] = pr
        shape = (n, slots) if edit == "deletions" else (n, slots, V)
        scan = scan.view(shape)
        lens_dev = torch.from_numpy(lengths).to(dev).long()
        site = torch.arange(slots, device=dev)[None, :]
        gone = site > lens_dev[:, None] if edit == "insertions" else site >= lens_dev[:, None]
        nan = (lens_dev[:, None] == self.conv_width) & ~gone if edit == "deletions" else None
        outs = [scan] if quad is None else [scan, quad.view(shape)]
        for t in outs:
            if nan is not None:
                t.masked_fill_(nan, float("nan"))
            t.masked_fill_(gone if edit == "deletions" else gone[:, :, None], 0.0)
        if edit == "substitutions":                      # the own token: the mutant is the sequence itself
            scan.masked_fill_(torch.arange(V, device=dev)[None, None, :] == xs.tokens.long()[:, :, None], 0.0)
        if prj is None:
            return scan if quad is None else (scan, outs[1])
        prj = prj.view(shape + (pm.shape[1],))
        if nan is not None:
            prj.masked_fill_(nan[:, :, None], float("nan"))
        prj.masked_fill_(gone[:, :, None] if edit == "deletions" else gone[:, :, None, None], 0.0)
        return (scan, prj) if quad is None else (scan, outs[1], prj)

    # the resident float32 cache holds complete feature rows, as for the other sequence kernels
    def cache_ok(self):
        return self.num_freqs <= 16384

    def block_ok(self):
        return self.num_rffs % 4 == 0

    def build_feature_cache(self, dataset):
        return _cache_from_transform_x(self, dataset)

    ztz_matvec_cached = ConvSORFKernel.ztz_matvec_cached
    ztz_block_cached = ConvSORFKernel.ztz_block_cached
    cache_rows_to_features = ConvSORFKernel.cache_rows_to_features
    workspace_bytes = ConvSORFKernel.workspace_bytes


class _SecondLayerView(SORFKernel):
    """``Conv1dTwoLayerKernel.second_layer()``: the RBF layer of a two-layer kernel as a ``SORFKernel`` over the pooled
    features.  Nothing is drawn: ``radem_diag`` and ``chi_arr`` ARE the owner's second-layer tensors, and ``hyperparams`` is
    the owner's attribute, read and written through -- the tuning routines set hyperparameters on the kernel they are
    handed, and both objects must see them."""

    def __init__(self, owner):
        KernelBase.__init__(self, owner.num_rffs, (owner._xdim[0], owner.init_rffs), owner.kernel_spec_parms, owner.device)
        self.owner = owner
        self.random_seed = owner.random_seed
        self.kernel_choice = "RBF"
        self.fit_intercept = owner.fit_intercept
        self.radem_diag, self.chi_arr = owner.radem_diag, owner.chi_arr

    @property
    def hyperparams(self):
        return self.owner.hyperparams

    @hyperparams.setter
    def hyperparams(self, value):
        if getattr(self, "owner", None) is not None:      # (KernelBase.__init__ assigns its default before the owner is known)
            self.owner.hyperparams = value

    def sibling(self, num_rffs):
        """The second layer of a two-layer kernel of the same family, seed, settings and hyperparameters with ``num_rffs``
        features (preconditioner.check_rank_ratio samples kernels beyond 8192 features with an 8192-feature one): its first
        layer draws what the owner's drew, so it reads the same pooled dataset."""
        twin = Conv1dTwoLayerKernel(self.owner._xdim, num_rffs, self.owner.random_seed, self.owner.device,
                                    self.owner.kernel_spec_parms)
        twin.set_hyperparams(self.owner.get_hyperparams(logspace=False), logspace=False)
        return twin.second_layer()


class MiniARDKernel(KernelBase):
    """kernels/ARD_kernels/mini_ard.py:16-287: an RBF kernel with one inverse lengthscale per group of
    input features (groups delimited by ``split_points``).  hyperparams = [lambda, sigma_1 .. sigma_G].
    Features: input scaled per feature, then the SORF operator; gradient: dense precomputed weights
    (three FHT rounds on the identity, built on the device with hipFastHadamardTransform2D in float64)
    through hipMiniARDGrad."""

    def __init__(self, xdim, num_rffs, random_seed=123, device="cuda", double_precision=False,
                 kernel_spec_parms=None):
        kernel_spec_parms = kernel_spec_parms or {}
        super().__init__(num_rffs, xdim, kernel_spec_parms, device)
        self.random_seed = random_seed
        self.double_precision = double_precision
        if len(self._xdim) != 2:
            raise ValueError("The dimensionality of the input is inappropriate for "
                             "the kernel you have selected.")
        if "split_points" not in kernel_spec_parms:
            raise ValueError("For the MiniARD kernel, 'kernel_specific_params' "
                             "must contain a list called 'split_points'.")
        if not isinstance(kernel_spec_parms["split_points"], list):
            raise ValueError("For the MiniARD kernel, 'split_points' must be a list.")
        self.kernel_choice = "MiniARD"
        self.split_pts = np.sort([0] + kernel_spec_parms["split_points"] + [xdim[1]])
        self._check_split_points(xdim)
        self.hyperparams = np.ones((self.split_pts.shape[0]))
        self.padded_dims = padded_dims(xdim[-1])
        radem_array = np.asarray([-1, 1], dtype=np.int8)
        rng = np.random.default_rng(random_seed)
        self.nblocks = ceil(self.num_freqs / self.padded_dims) if self.padded_dims < self.num_freqs else 1
        radem = rng.choice(radem_array, size=(3, 1, self.nblocks * self.padded_dims), replace=True)
        chi_arr = _chi.rvs(df=self.padded_dims, size=self.num_freqs, random_state=random_seed)
        if not double_precision:
            chi_arr = chi_arr.astype(np.float32)
        self._to_device(radem, chi_arr)
        self.precomputed_weights = None
        self._set_ard_arrays()

    def _check_split_points(self, xdim):
        """mini_ard.py:113-133."""
        if self.split_pts.shape[0] - 2 < 1:
            raise ValueError("There must be at least one split point to use MiniARD.")
        if self.split_pts[0] < 0:
            raise ValueError("The first split point must be > 0.")
        if self.split_pts[-1] > xdim[1]:
            raise ValueError("The last split point must be < shape[1] of the input data.")
        if np.diff(self.split_pts).min() == 0:
            raise ValueError("At least two of the split points supplied are identical.")

    def _set_ard_arrays(self):
        """mini_ard.py:158-168 (kernel_specific_set_hyperparams)."""
        full = np.zeros((self._xdim[-1]))
        key = np.zeros((self._xdim[-1]), dtype=np.int32)
        for i in range(1, self.split_pts.shape[0]):
            full[self.split_pts[i - 1]:self.split_pts[i]] = self.hyperparams[i]
            key[self.split_pts[i - 1]:self.split_pts[i]] = i - 1
        self.full_ard_weights = torch.from_numpy(full).to(self.device)
        self.ard_position_key = torch.from_numpy(key).to(self.device)

    def set_hyperparams(self, hyperparams, logspace=True):
        super().set_hyperparams(hyperparams, logspace)
        self._set_ard_arrays()

    supports_fused = False

    def fused_ok(self):
        return False

    def _typed(self, t):
        return t.to(torch.float64 if self.double_precision else torch.float32).contiguous()

    def transform_x(self, input_x, sequence_length=None):
        """kernel_baseclass.py:269-299 with mini_ard.py:171-194 (no sigma pre-multiplication: the
        per-feature weights carry the lengthscales)."""
        xin = self._typed(self._as_device(input_x))                 # the private typed copy (:274-288)
        xtrans = self._typed(xin.to(torch.float64) * self.full_ard_weights[None, :])
        output_x = torch.zeros((xtrans.shape[0], self.num_rffs), dtype=torch.float64, device=self.device)
        ext.hipRBFFeatureGen(xtrans, output_x, self.radem_diag, self._typed(self.chi_arr), self.fit_intercept)
        if self.fit_intercept:
            output_x[:, 0] = 1.
        return output_x

    def precompute_weights(self):
        """mini_ard.py:196-238, on the device in float64."""
        p = self.padded_dims
        norm_constant = 1.0 / (2.0 ** (np.log2(p) / 2.0))
        padded_chi = torch.zeros(self.nblocks * p, dtype=torch.float64, device=self.device)
        padded_chi[:self.chi_arr.shape[0]] = self.chi_arr.to(torch.float64)
        radem = self.radem_diag.to(torch.float64)
        blocks = []
        for i in range(self.nblocks):
            ident = torch.eye(p, dtype=torch.float64, device=self.device)
            lo, hi = i * p, (i + 1) * p
            for r in range(3):
                ident *= radem[r:r + 1, 0, lo:hi] * norm_constant
                ext.hipFastHadamardTransform2D(ident)
            ident *= padded_chi[lo:hi]
            blocks.append(ident.T[:, :self._xdim[-1]])
        self.precomputed_weights = self._typed(torch.cat(blocks)[:self.num_freqs, :])

    def kernel_specific_gradient(self, input_x, sequence_length=None):
        """mini_ard.py:240-275."""
        if self.precomputed_weights is None:
            self.precompute_weights()
        nl = self.split_pts.shape[0] - 1
        xtrans = torch.zeros((input_x.shape[0], self.num_rffs), dtype=torch.float64, device=self.device)
        dz_dsigma = torch.zeros((input_x.shape[0], self.num_rffs, nl), dtype=torch.float64, device=self.device)
        ext.hipMiniARDGrad(input_x, xtrans, self.precomputed_weights, self.ard_position_key,
                           self.full_ard_weights, dz_dsigma, self.fit_intercept)
        return xtrans, dz_dsigma

    def gradient_x(self, input_x, sequence_length=None):
        xin = self._typed(self._as_device(input_x))
        xtrans, xgrad = self.kernel_specific_gradient(xin, sequence_length)
        if self.fit_intercept:
            xtrans[:, 0] = 1.
            xgrad[:, 0, :] = 0.
        return xtrans, xgrad


_FIXED = ("RBF", "Matern", "Cauchy")
_CONV = ("Conv1dRBF", "Conv1dMatern", "Conv1dCauchy", "GraphRBF", "GraphMatern", "GraphCauchy")


def make_kernel(kernel_choice, xdim, num_rffs, random_seed=123, device="cuda", kernel_spec_parms=None):
    """Counterpart of KERNEL_NAME_TO_CLASS (kernels/__init__.py:21-33) for the SORF kernels."""
    if kernel_choice in _FIXED:
        return SORFKernel(kernel_choice, xdim, num_rffs, random_seed, device, kernel_spec_parms)
    if kernel_choice in _CONV:
        return ConvSORFKernel(kernel_choice, xdim, num_rffs, random_seed, device, kernel_spec_parms)
    if kernel_choice == "MiniARD":
        return MiniARDKernel(xdim, num_rffs, random_seed, device, False, kernel_spec_parms)
    if kernel_choice == "Conv1dTwoLayer":
        return Conv1dTwoLayerKernel(xdim, num_rffs, random_seed, device, kernel_spec_parms)
    if kernel_choice == "Linear":
        return LinearKernel(xdim, num_rffs, random_seed, device, kernel_spec_parms)
    raise RuntimeError(f"kernel '{kernel_choice}' is outside the hot path this package implements "
                       f"(supported: {_FIXED + _CONV + ('MiniARD', 'Conv1dTwoLayer', 'Linear')})")


class SRHTCompressor:
    """srht_compressor.py:37-97 -- double precision, as the preconditioner uses it."""

    def __init__(self, compression_size, input_size, device="cuda", random_seed=123):
        if compression_size >= input_size or compression_size <= 1:
            raise RuntimeError("The compression size should be < the number of rffs and > 1.")
        self.compression_size, self.input_size = compression_size, input_size
        self.padded_dims = padded_dims(input_size)
        radem_array = np.asarray([-1, 1], dtype=np.int8)
        rng = np.random.default_rng(random_seed)
        radem = rng.choice(radem_array, size=(self.padded_dims), replace=True)
        col_sampler = rng.permutation(self.padded_dims)
        self.device = device
        self.radem = torch.from_numpy(radem).to(device)
        self.col_sampler = torch.from_numpy(col_sampler).to(device)
        self.truncated_sampler = self.col_sampler[:compression_size].contiguous()
        self._zty_ws = None

    def fused_ok(self, features):
        return (features.is_cuda and features.dtype == torch.float64 and features.is_contiguous()
                and ext.srht_sample_ok(self.padded_dims, torch.float64))

    def transform_x_zty(self, features, ydata, zty_out, out=None):
        """The compressed chunk AND ``features.T @ ydata`` (into zty_out) from one read of the chunk
        (rand_nys_constructors.py:113-117)."""
        if self.fused_ok(features):
            if out is None:
                out = torch.empty((features.shape[0], self.compression_size), dtype=torch.float64,
                                  device=features.device)
            if self._zty_ws is None:
                self._zty_ws = torch.empty(ext.srht_sample_workspace_bytes(self.input_size), dtype=torch.uint8,
                                           device=features.device)
            ext.hipSRHTSample(features, self.radem, self.truncated_sampler, out, self.compression_size,
                              ydata, zty_out, self._zty_ws)
            return out[:, :self.compression_size]
        torch.matmul(features.T, ydata, out=zty_out)
        return self.transform_x(features, out=out)

    def transform_x(self, features, no_compression=False, out=None):
        """srht_compressor.py:87-97.  ``out``: optional preallocated float64 [n, >= compression_size] array
        whose leading columns receive the result (the fused pad + SRHT + gather operator writes into it)."""
        if features.dim() != 2 or features.shape[1] != self.input_size:
            raise RuntimeError("Input with unexpected size passed to a compressor module.")
        if not no_compression and self.fused_ok(features):
            if out is None:
                out = torch.empty((features.shape[0], self.compression_size), dtype=torch.float64,
                                  device=features.device)
            ext.hipSRHTSample(features, self.radem, self.truncated_sampler, out, self.compression_size)
            return out[:, :self.compression_size]
        if features.shape[1] < self.padded_dims:
            xfeatures = torch.zeros((features.shape[0], self.padded_dims), dtype=torch.float64,
                                    device=self.device)
            xfeatures[:, :features.shape[1]] = features
        else:
            xfeatures = features.to(torch.float64, copy=True).contiguous()
        ext.hipSRHT(xfeatures, self.radem)
        if no_compression:
            return xfeatures[:, self.col_sampler]
        if out is not None:
            out[:, :self.compression_size] = xfeatures[:, self.truncated_sampler]
            return out[:, :self.compression_size]
        return xfeatures[:, self.truncated_sampler]
