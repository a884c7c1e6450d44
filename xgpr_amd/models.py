"""The reference's two model classes as thin state holders over this package's functions, so that a script
written against xGPR reads the same here:

    xGPRegression      <-> xgp_regression.py (fit / predict / exact_nmll / exact_nmll_gradient /
                            approximate_nmll / tune_hyperparams, build_preconditioner, set_hyperparams)
    xGPClassification  <-> xgp_classification.py (fit / predict)

Differences, all deliberate: datasets are the HBM-resident ones of ``xgpr_amd.dataset`` (built with
``build_regression_dataset`` / ``build_classification_dataset`` / ``build_offline_np_dataset``), the device is the
HIP device (there is no CPU mode), and inputs / outputs at the API boundary are numpy arrays as in the reference.
Everything numerical lives in kernels.py, cg.py, preconditioner.py, exact.py, nmll.py, classification.py, tuning.py.
"""
import numpy as np
import torch

from . import nmll as _nmll
from .cg import cg_fit_lib_internal, refuse_half_cache
from .classification import fit_classifier, predict_proba
from .exact import calc_weights_exact, calc_variance_exact
from .dataset import TokenBatch, token_batch
from .kernels import Conv1dTwoLayerKernel, ConvSORFKernel, LinearKernel, SORFKernel, make_kernel
from .preconditioner import RandNysPreconditioner, autoselect_preconditioner
from .crude_tuning import tune_hyperparams_crude as _tune_crude
from .tuning import default_bounds as _default_bounds, tune_hyperparams as _tune

MAX_VARIANCE_RFFS = 4096            # constants.py:2
MAX_CLOSED_FORM_RFFS = 8192         # constants.py:3
DEFAULT_KERNEL_SPEC_PARMS = {"matern_nu": 5 / 2, "intercept": True, "averaging": "none"}      # constants.py:7-8


def token_input(input_x, token_table, device):
    """``predict`` input: a TokenBatch as it is; with ``token_table`` an integer array [N, L] of tokens in [0, V) over that
    table, as a TokenBatch on ``device`` (the checks of the dataset builders); anything else unchanged."""
    if token_table is None:
        return input_x
    xt = torch.from_numpy(np.ascontiguousarray(input_x)) if isinstance(input_x, np.ndarray) else input_x
    return token_batch(xt, token_table).to(device)


class _ModelBase:
    """model_baseclass.py:68-125 (constructor arguments), :171-222 (hyperparameters), :225-260
    (build_preconditioner)."""
    is_regression = True

    def __init__(self, num_rffs=256, variance_rffs=16, kernel_choice="RBF", device="cuda", kernel_settings=None,
                 verbose=True, random_seed=123):
        if kernel_settings is not None and not isinstance(kernel_settings, dict):
            raise RuntimeError("kernel_settings must be a dict.")
        if variance_rffs > MAX_VARIANCE_RFFS:
            raise RuntimeError("Currently to keep computational expense at acceptable levels variance rffs is "
                               f"capped at {MAX_VARIANCE_RFFS}.")
        self.num_rffs, self.variance_rffs = num_rffs, variance_rffs
        self.kernel_choice, self.device = kernel_choice, device
        self.kernel_spec_parms = dict(DEFAULT_KERNEL_SPEC_PARMS if kernel_settings is None else kernel_settings)
        self.verbose, self.random_seed = verbose, random_seed
        self.kernel = None
        self.weights = self.var = self.gamma = None
        self.trainy_mean, self.trainy_std = 0.0, 1.0

    # The two-layer kernel's solver passes run on its second layer over the dataset's resident pooled first layer
    # (Conv1dTwoLayerKernel.second_layer / DeviceDataset.pooled): a fixed-vector RBF problem.  False keeps every pass on the
    # two-layer kernel and the original dataset.
    pool_first_layer = True

    def _solver_pair(self, dataset):
        """-> (kernel, dataset) the solver passes are handed.  The weights live in the same feature space either way."""
        kernel = self.kernel
        if (self.pool_first_layer and getattr(kernel, "kernel_choice", None) == "Conv1dTwoLayer"
                and hasattr(kernel, "second_layer") and torch.device(kernel.device).type == "cuda"
                and hasattr(dataset, "pooled")):
            return kernel.second_layer(), dataset.pooled(kernel)
        return kernel, dataset

    def _initialize_kernel(self, dataset):
        if self.kernel is None:
            self.kernel = make_kernel(self.kernel_choice, dataset.get_xdim(), self.num_rffs, self.random_seed,
                                      self.device, self.kernel_spec_parms)

    def set_hyperparams(self, hyperparams=None, dataset=None):
        """model_baseclass.py:171-213: log-space hyperparameters; the kernel is created from the dataset's
        dimensions on first use."""
        if self.kernel is None:
            if dataset is None:
                raise RuntimeError("A dataset is required if the kernel has not already been initialized.")
            self._initialize_kernel(dataset)
        if hyperparams is not None:
            if not isinstance(hyperparams, np.ndarray) or hyperparams.shape != self.kernel.get_hyperparams().shape:
                raise RuntimeError("The hyperparameters must be a numpy array of the kernel's hyperparameter shape.")
            self.kernel.set_hyperparams(hyperparams, logspace=True)
        self.weights = self.var = self.gamma = None

    def get_hyperparams(self):
        return None if self.kernel is None else self.kernel.get_hyperparams()

    def build_preconditioner(self, dataset, max_rank=512, method="srht"):
        """-> (preconditioner, achieved_ratio)"""
        self._initialize_kernel(dataset)
        if max_rank < 1:
            raise RuntimeError("Invalid value for max_rank.")
        if max_rank >= self.kernel.get_num_rffs():
            raise RuntimeError("Max rank should be < the number of rffs.")
        kernel, dataset = self._solver_pair(dataset)
        pre = RandNysPreconditioner(kernel, dataset, max_rank, self.verbose, self.random_seed, method,
                                    is_regression=self.is_regression)
        return pre, pre.achieved_ratio

    def _to_device(self, arr):
        return arr if isinstance(arr, (torch.Tensor, TokenBatch)) else torch.from_numpy(np.ascontiguousarray(arr))


class xGPRegression(_ModelBase):
    def fit(self, dataset, preconditioner=None, tol=1e-6, max_iter=500, mode="cg", suppress_var=False,
            max_rank=3000, min_rank=512, autoselect_target_ratio=30., always_use_srht2=False, run_diagnostics=False,
            cache_features="auto"):
        """xgp_regression.py:381-493.  ``cache_features``: "auto" (default), True, False as ``cg_fit_lib_internal``; "half"
        (opt-in) keeps the CG solve's resident feature rows as IEEE binary16 -- half the memory and bytes per iteration, a
        solve on features rounded to 11 significant bits."""
        self._initialize_kernel(dataset)
        self.trainy_mean, self.trainy_std = dataset.get_ymean(), dataset.get_ystd()
        self.weights = self.var = None
        kernel, dataset = self._solver_pair(dataset)
        if mode == "exact":
            if kernel.get_num_rffs() > MAX_CLOSED_FORM_RFFS:
                raise RuntimeError(f"You specified 'exact' fitting, but the number of rffs is > {MAX_CLOSED_FORM_RFFS}.")
            self.weights, n_iter, losses = calc_weights_exact(dataset, kernel)
        elif mode == "cg":
            if preconditioner is None:
                preconditioner, _, _ = autoselect_preconditioner(
                    kernel, dataset, min_rank, max_rank, 512, always_use_srht2, autoselect_target_ratio,
                    self.random_seed, True, self.verbose)
            self.weights, n_iter, losses = cg_fit_lib_internal(kernel, dataset, tol, max_iter, preconditioner,
                                                               self.verbose, cache_features=cache_features)
        else:
            raise RuntimeError("Unrecognized fitting mode supplied. Must provide one of 'cg', 'exact'.")
        if not suppress_var:
            nvar = min(self.variance_rffs, kernel.get_num_rffs())
            self.var = calc_variance_exact(kernel, dataset, nvar)
        if run_diagnostics:
            return n_iter, losses

    def predict(self, input_x, sequence_lengths=None, get_var=False, chunk_size=2000, token_table=None):
        """xgp_regression.py:77-148 -> numpy predictions (and variances).  ``input_x`` may be a TokenBatch, or with
        ``token_table`` an integer token array [N, L]: the mean goes through the token feature rows, the variance through
        dense chunks."""
        input_x = token_input(input_x, token_table, self.device)
        if self.weights is None:
            raise RuntimeError("Model has not yet been successfully fitted.")
        if get_var and self.var is None:
            raise RuntimeError("Variance was requested but suppress_var was selected when fitting.")
        if not get_var and sequence_lengths is not None and getattr(self.kernel, "seq_rows_ok", lambda: False)():
            # sequence kernels, mean only: float32 feature rows through the one-column projection (no float64 features)
            from .exact import predict_mean
            return predict_mean(self.kernel, self.weights, input_x, self.trainy_mean, self.trainy_std, sequence_lengths,
                                chunk_size).cpu().numpy()
        lambda_ = float(self.kernel.get_lambda())
        preds, var = [], []
        for i in range(0, input_x.shape[0], chunk_size):
            sl = None if sequence_lengths is None else sequence_lengths[i:i + chunk_size]
            xfeatures = self.kernel.transform_x(input_x[i:i + chunk_size], sl)
            preds.append((xfeatures * self.weights[None, :]).sum(dim=1))
            if get_var:
                xv = xfeatures[:, :self.var.shape[0]]
                pred_var = (self.var @ xv.T).T
                var.append(lambda_ ** 2 + lambda_ ** 2 * (xv * pred_var).sum(dim=1))
        preds = torch.cat(preds).cpu().numpy() * self.trainy_std + self.trainy_mean
        if not get_var:
            return preds
        var = torch.cat(var).cpu().numpy()
        var[var < 0] = 0
        return preds, var * self.trainy_std ** 2

    def predict_gradient(self, input_x, get_var=False, chunk_size=2000, sequence_lengths=None, token_table=None,
                         subgradient=False):
        """The derivative of ``predict`` with respect to the input (no counterpart in the reference) -> numpy d mean / d x; with
        ``get_var`` also d variance / d x, of the same shape.  Fixed-vector kernels RBF / Matern / Cauchy: [N, d] (DESIGN.md
        3.16).  Sequence and graph kernels (Conv1d*, Graph*), which need ``sequence_lengths``: [N, L, C], one value per position
        and channel, exactly 0 past a sequence's length; ``input_x`` may be a TokenBatch, or with ``token_table`` an integer token
        array [N, L] -- the result is then the saliency map over the table's channels.  With random features the
        derivative is exact (the transposed SORF applied to the weighted sine / cosine terms).  Linear: the weights themselves, [N, d].
        Conv1dTwoLayer is not differentiable where two k-mers tie for a filter's maximum or that maximum is 0: what exists there
        is a SUBGRADIENT under a fixed convention -- a filter's gradient goes to the first k-mer that attains its maximum, and
        nowhere if that maximum is not positive -- and the caller asks for it by name, ``subgradient=True``;
        without it the two-layer kernel is refused as before.  The flag changes nothing for the other kernels.
        The variance gradient is that of the UNCLIPPED expression lambda^2 + lambda^2 z_v^T V z_v: where ``predict``
        clips a negative variance to zero, the gradient returned here is still that of the expression."""
        if self.weights is None:
            raise RuntimeError("Model has not yet been successfully fitted.")
        if get_var and self.var is None:
            raise RuntimeError("Variance was requested but suppress_var was selected when fitting.")
        two_layer, linear = type(self.kernel) is Conv1dTwoLayerKernel, type(self.kernel) is LinearKernel
        seq = type(self.kernel) is ConvSORFKernel or two_layer
        if (type(self.kernel) is not SORFKernel and not seq and not linear) or (two_layer and not subgradient):
            raise RuntimeError("predict_gradient is available for the fixed-vector kernels RBF, Matern and Cauchy, for Linear, for the "
                               "sequence and graph kernels Conv1d* / Graph*, and with subgradient=True for Conv1dTwoLayer (the "
                               "max-pool's first-window convention); MiniARD is not supported "
                               f"(this model's kernel is '{self.kernel_choice}').")
        if seq and sequence_lengths is None:
            raise RuntimeError("sequence_lengths is required for the sequence and graph kernels.")
        input_x = self._to_device(token_input(input_x, token_table, self.device) if seq else input_x)
        lambda_ = float(self.kernel.get_lambda())
        gmean, gvar = [], []
        for i in range(0, input_x.shape[0], chunk_size):
            chunk = input_x[i:i + chunk_size]
            sl = (np.asarray(sequence_lengths[i:i + chunk_size]),) if seq else ()
            if two_layer:                        # one pooling per chunk: the second layer's features and gradients read it
                pooled = self.kernel.pool(chunk, *sl)
                extra, features = {"pooled": pooled}, lambda: self.kernel.second_layer().transform_x(pooled)
            else:
                extra, features = {}, lambda: self.kernel.transform_x(chunk, *sl)
            gmean.append(self.kernel.input_gradient(chunk, *sl, self.weights, **extra))
            if get_var:
                nvar = self.var.shape[0]
                xv = features()[:, :nvar]
                if linear:
                    wv = 2.0 * lambda_ ** 2 * (xv @ self.var)
                else:
                    wv = torch.zeros((xv.shape[0], nvar + (nvar & 1)), dtype=torch.float64, device=xv.device)
                    wv[:, :nvar] = 2.0 * lambda_ ** 2 * (xv @ self.var)
                gvar.append(self.kernel.input_gradient(chunk, *sl, wv, w_cols=wv.shape[1], **extra))
        gmean = torch.cat(gmean).cpu().numpy() * self.trainy_std
        if not get_var:
            return gmean
        return gmean, torch.cat(gvar).cpu().numpy() * self.trainy_std ** 2

    def predict_substitutions(self, input_x, sequence_lengths=None, token_table=None, chunk_size=64, get_var=False):
        """The exact effect of every single substitution on ``predict`` (no counterpart in the reference) -> numpy float64
        [N, L, V]: entry [i, l, v] is the predicted mean of sequence i with its token at position l replaced by row v of the
        token table, minus the predicted mean of sequence i itself, in the units of y (times the training y's standard
        deviation; the offset cancels).  Exactly 0 at a sequence's own token and past its length.  ``input_x`` is a TokenBatch,
        or with ``token_table`` an integer token array [N, L]; ``sequence_lengths`` is required.  Available for the sequence and
        graph kernels Conv1dRBF / Conv1dMatern / Conv1dCauchy and GraphRBF / GraphMatern / GraphCauchy, whose feature row is a
        sum over k-mer windows: a substitution changes only the conv_width windows that cover it, so the scan costs
        L V conv_width window transforms, not the L V (L - conv_width + 1) of L V mutant sequences, and no mutant is written
        (``predict_gradient`` gives the first-order estimate).  ``chunk_size`` sequences go to the device at a
        time.  With ``get_var=True`` the return is (scan, variances): variances[i, l, v] is the predictive VARIANCE of that
        mutant as ``predict(get_var=True)`` gives it -- trainy_std^2 max(0, lambda^2 + lambda^2 z'^T var z') --, exactly 0 past a
        sequence's length and the sequence's own variance at its own token.  It has a per-window decomposition too: the
        substitution moves the variance columns z by a vector built from the conv_width covering windows alone, so the quadratic
        form needs those windows' first tile and one nvar x nvar contraction per mutant, not the mutants' feature rows
        (``ConvSORFKernel.substitution_variance_scan``).  ``predict_single_edits`` returns the same array for these
        kernels and serves Conv1dTwoLayer too."""
        if self.weights is None:
            raise RuntimeError("Model has not yet been successfully fitted.")
        if get_var and self.var is None:
            raise RuntimeError("Variance was requested but suppress_var was selected when fitting.")
        if type(self.kernel) is not ConvSORFKernel:
            raise RuntimeError("predict_substitutions is available for the sequence and graph kernels Conv1dRBF, Conv1dMatern, "
                               "Conv1dCauchy, GraphRBF, GraphMatern and GraphCauchy on token input; Conv1dTwoLayer, the "
                               "fixed-vector kernels, Linear and MiniARD are not supported "
                               f"(this model's kernel is '{self.kernel_choice}').")
        if sequence_lengths is None:
            raise RuntimeError("sequence_lengths is required for the sequence and graph kernels.")
        input_x = token_input(input_x, token_table, self.device)
        if not isinstance(input_x, TokenBatch):
            raise RuntimeError("predict_substitutions needs token input: a TokenBatch, or integer tokens [N, L] with token_table.")
        sequence_lengths = np.asarray(sequence_lengths)
        if sequence_lengths.shape[0] != input_x.shape[0]:
            raise RuntimeError("The shape[0] of sequence_lengths must match the shape[0] of input_x.")
        scans = [self.kernel.substitution_scan(input_x[i:i + chunk_size], sequence_lengths[i:i + chunk_size], self.weights)
                 for i in range(0, input_x.shape[0], chunk_size)]
        scan = (torch.cat(scans).cpu().numpy() * self.trainy_std if scans
                else np.zeros((0, input_x.shape[1], input_x.table.shape[0])))
        if not get_var:
            return scan
        lambda_ = float(self.kernel.get_lambda())
        quads = [self.kernel.substitution_variance_scan(input_x[i:i + chunk_size], sequence_lengths[i:i + chunk_size], self.var)
                 for i in range(0, input_x.shape[0], chunk_size)]
        if not quads:
            return scan, np.zeros(scan.shape)
        var = lambda_ ** 2 + lambda_ ** 2 * torch.cat(quads).cpu().numpy()
        var[var < 0] = 0
        var[np.arange(input_x.shape[1])[None, :] >= sequence_lengths[:, None]] = 0
        return scan, var * self.trainy_std ** 2

    def _token_scan_input(self, name, input_x, sequence_lengths, token_table, two_layer=False):
        """The refusals ``predict_substitutions`` makes, for the other position-by-position scans -> (TokenBatch, lengths).
        ``two_layer``: the scan serves Conv1dTwoLayer as well."""
        if self.weights is None:
            raise RuntimeError("Model has not yet been successfully fitted.")
        if two_layer and type(self.kernel) not in (ConvSORFKernel, Conv1dTwoLayerKernel):
            raise RuntimeError(f"{name} is available for the sequence and graph kernels Conv1dRBF, Conv1dMatern, Conv1dCauchy, "
                               "GraphRBF, GraphMatern and GraphCauchy and for Conv1dTwoLayer on token input; the fixed-vector "
                               f"kernels, Linear and MiniARD are not supported (this model's kernel is '{self.kernel_choice}').")
        if not two_layer and type(self.kernel) is not ConvSORFKernel:
            raise RuntimeError(f"{name} is available for the sequence and graph kernels Conv1dRBF, Conv1dMatern, "
                               "Conv1dCauchy, GraphRBF, GraphMatern and GraphCauchy on token input; Conv1dTwoLayer, the "
                               "fixed-vector kernels, Linear and MiniARD are not supported "
                               f"(this model's kernel is '{self.kernel_choice}').")
        if sequence_lengths is None:
            raise RuntimeError("sequence_lengths is required for the sequence and graph kernels.")
        input_x = token_input(input_x, token_table, self.device)
        if not isinstance(input_x, TokenBatch):
            raise RuntimeError(f"{name} needs token input: a TokenBatch, or integer tokens [N, L] with token_table.")
        sequence_lengths = np.asarray(sequence_lengths)
        if sequence_lengths.shape[0] != input_x.shape[0]:
            raise RuntimeError("The shape[0] of sequence_lengths must match the shape[0] of input_x.")
        return input_x, sequence_lengths

    def predict_substitution_pairs(self, input_x, sequence_lengths=None, token_table=None, chunk_size=4):
        """The exact non-additive part (epistasis) of every pair of substitutions closer than conv_width (no counterpart in the
        reference) -> numpy float64 [N, L, conv_width - 1, V, V], in the units of y (times the training y's standard deviation).
        With ``sub = predict_substitutions(...)`` and ``pairs`` this result, the predicted mean of sequence i with its token at
        l1 replaced by v1 and its token at l2 = l1 + d replaced by v2 is

            mean(double) = predict + sub[i, l1, v1] + sub[i, l2, v2] + (pairs[i, l1, d - 1, v1, v2] if d < conv_width else 0)

        exactly: the feature row is a sum over k-mer windows, only the conv_width - d windows that cover both positions see both
        substitutions, and two positions conv_width or more apart share none (for the graph kernels the third axis is empty).
        Exactly 0 where either token is the sequence's own and where either position is past the sequence's length.  Input,
        kernels and refusals as for ``predict_substitutions``.  One HIP kernel transforms the shared windows alone and writes no
        mutant (``ConvSORFKernel.pair_substitution_scan``).  The output is large -- 14.5 MB per sequence of a
        512-position array at conv_width 9 and V = 21 --, which is why ``chunk_size``, the sequences that go to the device at a
        time, is small.  (The single edits of every sequence kernel, Conv1dTwoLayer included: ``predict_single_edits``.)"""
        input_x, sequence_lengths = self._token_scan_input("predict_substitution_pairs", input_x, sequence_lengths, token_table)
        n, L, V = input_x.shape[0], input_x.shape[1], input_x.table.shape[0]
        out = np.zeros((n, L, self.kernel.conv_width - 1, V, V))
        for i in range(0, n, chunk_size):
            scan = self.kernel.pair_substitution_scan(input_x[i:i + chunk_size], sequence_lengths[i:i + chunk_size], self.weights)
            out[i:i + chunk_size] = scan.cpu().numpy() * self.trainy_std
        return out

    def predict_site_library(self, input_x, sites, sequence_lengths=None, token_table=None, chunk_size=4):
        """Every variant of the K positions ``sites`` of every sequence -- a combinatorial site-saturation library, V^K variants
        per parent -- as a ``SiteLibrary`` (no counterpart in the reference): one small table per RUN, a set of sites that one
        range of k-mer windows covers together, in the units of y (times the training y's standard deviation), and ``base`` =
        ``predict`` of the parents, so that

            mean(variant) = lib.base[:, None] + lib.gather(assignments)

        exactly, for ANY number of chosen sites inside one window -- where ``predict_substitutions`` plus
        ``predict_substitution_pairs`` is exact for two.  ``lib.topk(k)`` gives the k best variants of each parent without
        forming V^K; ``lib.dense()`` the whole library where it is small enough.  ``sites`` are strictly ascending positions
        shared by all sequences and inside every one of them (a per-sequence site list: one call per sequence).  The entry
        of a parent's own tokens is exactly 0 in every table.  Input, kernels and refusals as for ``predict_substitutions``.
        Only the windows that cover a site are transformed, each for the assignments of the sites it covers, and no variant is
        written (``ConvSORFKernel.site_scan``, which names the shapes that are written out instead).  The
        tables are CPU tensors; ``chunk_size`` sequences go to the device at a time."""
        from .acquisition import SiteLibrary
        input_x, sequence_lengths = self._token_scan_input("predict_site_library", input_x, sequence_lengths, token_table)
        libs = [self.kernel.site_scan(input_x[i:i + chunk_size], sequence_lengths[i:i + chunk_size], self.weights, sites)
                for i in range(0, max(input_x.shape[0], 1), chunk_size)]
        tables = [torch.cat([lib.tables[q] for lib in libs]).cpu() * float(self.trainy_std) for q in range(len(libs[0].tables))]
        base = torch.from_numpy(np.asarray(self.predict(input_x, sequence_lengths=sequence_lengths), dtype=np.float64).reshape(-1))
        return SiteLibrary(libs[0].sites, libs[0].vocab, libs[0].runs, tables, base=base)

    def predict_indels(self, input_x, sequence_lengths=None, token_table=None, chunk_size=64, get_var=False):
        """The exact effect of every single deletion and insertion on ``predict`` (no counterpart in the reference) -> numpy
        float64 (deletions [N, L], insertions [N, L + 1, V]): deletions[i, p] is the predicted mean of sequence i without its
        token at position p, insertions[i, g, v] that of sequence i with row v of the token table inserted before position g
        (g = the length appends), each minus the predicted mean of sequence i itself, in the units of y (times the training
        y's standard deviation; the offset cancels).  Exactly 0 for p >= the length and g > the length; NaN for the deletions of
        a sequence of exactly conv_width tokens, whose mutant has no k-mer.  Input and kernels as for ``predict_substitutions``.
        An indel only shifts the windows away from the edit, so the scan transforms about conv_width windows per edit plus
        the sequence's own windows once, and rescales the total by the mutant's k-mer normaliser; no mutant is written
        (DESIGN.md 3.21).  With ``get_var=True`` the return is (deletions, insertions, deletion_variances,
        insertion_variances): the predictive VARIANCE of every such mutant as ``predict(get_var=True)`` gives it -- trainy_std^2
        max(0, lambda^2 + lambda^2 z'^T var z') --, exactly 0 for p >= the length and g > the length and NaN where the deletions
        are NaN.  The identity of ``predict_substitutions(get_var=True)`` holds with the mutant's normaliser r': the sequence's own
        variance columns are rescaled by r' / r and moved by r' times a vector built from the windows at the edit site alone
        (``ConvSORFKernel.indel_variance_scan``).  ``predict_single_edits`` returns the same arrays for these kernels
        and serves Conv1dTwoLayer too."""
        if get_var and self.weights is not None and self.var is None:
            raise RuntimeError("Variance was requested but suppress_var was selected when fitting.")
        input_x, sequence_lengths = self._token_scan_input("predict_indels", input_x, sequence_lengths, token_table)
        n, L, V = input_x.shape[0], input_x.shape[1], input_x.table.shape[0]
        scans = [self.kernel.indel_scan(input_x[i:i + chunk_size], sequence_lengths[i:i + chunk_size], self.weights)
                 for i in range(0, n, chunk_size)]
        if not scans:
            none = (np.zeros((0, L)), np.zeros((0, L + 1, V)))
            return none + (np.zeros((0, L)), np.zeros((0, L + 1, V))) if get_var else none
        means = (torch.cat([s[0] for s in scans]).cpu().numpy() * self.trainy_std,
                 torch.cat([s[1] for s in scans]).cpu().numpy() * self.trainy_std)
        if not get_var:
            return means
        lambda_ = float(self.kernel.get_lambda())
        quads = [self.kernel.indel_variance_scan(input_x[i:i + chunk_size], sequence_lengths[i:i + chunk_size], self.var)
                 for i in range(0, n, chunk_size)]
        out = []
        for half, first in ((0, L), (1, L + 1)):
            var = lambda_ ** 2 + lambda_ ** 2 * torch.cat([q[half] for q in quads]).cpu().numpy()
            var[var < 0] = 0                                 # (a NaN stays a NaN)
            var[np.arange(first)[None, :] >= sequence_lengths[:, None] + half] = 0
            out.append(var * self.trainy_std ** 2)
        return means + tuple(out)

    def predict_single_edits(self, input_x, sequence_lengths=None, token_table=None, get_var=False, chunk_size=16):
        """The exact effect of EVERY single-token edit on ``predict``, for every sequence kernel (no counterpart in the reference)
        -> dict of numpy float64 arrays in the units of y: "substitutions" [N, L, V], "deletions" [N, L] and "insertions"
        [N, L + 1, V], each the predicted mean of the mutant minus that of the sequence itself, as ``predict_substitutions`` and
        ``predict_indels`` define them -- exactly 0 at a sequence's own token and past its length, NaN for the deletions of a
        sequence of exactly conv_width tokens.  With ``get_var`` also "substitutions_var", "deletions_var" and "insertions_var": the
        predictive variance of every mutant as ``predict(get_var=True)`` gives it, trainy_std^2 max(0, lambda^2 + lambda^2 z'^T var z'),
        0 past the length and NaN where the deletions are.  For the sequence and graph kernels Conv1d* / Graph* the arrays ARE those
        of ``predict_substitutions`` and ``predict_indels``.  For Conv1dTwoLayer the mutants' pooled first-layer rows come from the
        prefix and suffix maxima of the sequence's own windows and the about conv_width windows an edit creates -- a maximum is
        order-free, so this is exact and no mutant is written -- and go through the second layer slab by slab (DESIGN.md 3.25;
        ``Conv1dTwoLayerKernel.edit_scan``).  Input as for ``predict_substitutions``: a TokenBatch, or integer tokens [N, L] with
        ``token_table``; ``sequence_lengths`` is required.  ``chunk_size`` sequences go to the device at a time."""
        if get_var and self.weights is not None and self.var is None:
            raise RuntimeError("Variance was requested but suppress_var was selected when fitting.")
        names = ("substitutions", "deletions", "insertions")
        if type(self.kernel) is not Conv1dTwoLayerKernel:
            input_x, sequence_lengths = self._token_scan_input("predict_single_edits", input_x, sequence_lengths, token_table,
                                                               two_layer=True)
            sub = self.predict_substitutions(input_x, sequence_lengths, chunk_size=chunk_size, get_var=get_var)
            ind = self.predict_indels(input_x, sequence_lengths, chunk_size=chunk_size, get_var=get_var)
            if not get_var:
                return dict(zip(names, (sub,) + tuple(ind)))
            return dict(zip(names + tuple(nm + "_var" for nm in names), (sub[0], ind[0], ind[1], sub[1], ind[2], ind[3])))
        input_x, sequence_lengths = self._token_scan_input("predict_single_edits", input_x, sequence_lengths, token_table, two_layer=True)
        n, L, V = input_x.shape[0], input_x.shape[1], input_x.table.shape[0]
        lambda_ = float(self.kernel.get_lambda())
        out = {}
        for name, shape in zip(names, ((n, L, V), (n, L), (n, L + 1, V))):
            mean = np.zeros(shape)
            var = np.zeros(shape) if get_var else None
            for i in range(0, n, chunk_size):
                res = self.kernel.edit_scan(input_x[i:i + chunk_size], sequence_lengths[i:i + chunk_size], self.weights, name,
                                            var=self.var if get_var else None)
                mean[i:i + chunk_size] = (res[0] if get_var else res).cpu().numpy()
                if get_var:
                    var[i:i + chunk_size] = res[1].cpu().numpy()
            out[name] = mean * self.trainy_std
            if get_var:
                var = lambda_ ** 2 + lambda_ ** 2 * var
                var[var < 0] = 0                                 # (a NaN stays a NaN)
                first = np.arange(shape[1])[None, :]
                var[first > sequence_lengths[:, None] if name == "insertions" else first >= sequence_lengths[:, None]] = 0
                out[name + "_var"] = var * self.trainy_std ** 2
        return out

    # ---- the joint posterior over the single-edit neighbourhood: draws and batch picks (acquisition.py)
    def _factor_of_var(self):
        """F [nvar, nvar] with F F^T = 1/2 (var + var^T), negative eigenvalues clipped to 0 (``torch.linalg.eigh``); computed once
        per ``self.var`` and kept next to it."""
        cached = getattr(self, "_var_factor", None)
        if cached is None or cached[0] is not self.var:
            vals, vecs = torch.linalg.eigh(0.5 * (self.var + self.var.T))
            cached = self._var_factor = (self.var, (vecs * torch.sqrt(vals.clamp(min=0.0))[None, :]).contiguous())
        return cached[1]

    def _joint_scan_input(self, name, input_x, sequence_lengths, token_table):
        if self.weights is not None and self.var is None:
            raise RuntimeError("Variance was requested but suppress_var was selected when fitting.")
        return self._token_scan_input(name, input_x, sequence_lengths, token_table, two_layer=True)

    def _edit_projections(self, input_x, sequence_lengths, proj):
        """(means, projections) of every single edit of a few sequences, device tensors in the order substitutions, deletions,
        insertions: the mutants' means minus the sequences' own in units of the standardised y, and z'^T proj [..., K]."""
        if type(self.kernel) is Conv1dTwoLayerKernel:
            res = [self.kernel.edit_scan(input_x, sequence_lengths, self.weights, name, proj=proj)
                   for name in ("substitutions", "deletions", "insertions")]
            return [r[0] for r in res], [r[1] for r in res]
        means = (self.kernel.substitution_scan(input_x, sequence_lengths, self.weights),) \
            + tuple(self.kernel.indel_scan(input_x, sequence_lengths, self.weights))
        projs = (self.kernel.substitution_projection_scan(input_x, sequence_lengths, proj),) \
            + tuple(self.kernel.indel_projection_scan(input_x, sequence_lengths, proj))
        return list(means), list(projs)

    def single_edit_neighbourhoods(self, input_x, sequence_lengths=None, token_table=None):
        """Iterator of ``acquisition.SingleEditPosterior``, one per sequence (no counterpart in the reference): the JOINT posterior
        of every single substitution, deletion and insertion of that sequence -- means in the units of y, and a factor [E, nvar]
        of the latent posterior covariance, trainy_std^2 lambda^2 z'^T var z'', whose squared row norms plus ``noise`` are the
        variances of ``predict_single_edits(get_var=True)``.  The factor is the mutants' variance columns times a square-root
        factor of ``var`` (``torch.linalg.eigh``, cached), from the projection scans: the window sums of the variance scans and
        one matrix-core product per slab, no mutant written (``ConvSORFKernel.substitution_projection_scan``; Conv1dTwoLayer:
        ``edit_scan(proj=...)``).  One sequence at a time: E nvar 8 bytes are held.  Input, kernels and refusals as for
        ``predict_single_edits(get_var=True)``."""
        from .acquisition import SingleEditPosterior
        input_x, sequence_lengths = self._joint_scan_input("single_edit_neighbourhoods", input_x, sequence_lengths, token_table)
        L, V = input_x.shape[1], input_x.table.shape[0]
        amp = self.trainy_std * float(self.kernel.get_lambda())
        factor = self._factor_of_var()

        def neighbourhoods():
            for i in range(input_x.shape[0]):
                xb, lens = input_x[i:i + 1], sequence_lengths[i:i + 1]
                s = int(lens[0])
                own = float(self.predict(xb, lens)[0])
                means, projs = self._edit_projections(xb, lens, factor)
                mean = torch.cat([m.reshape(-1) for m in means]) * self.trainy_std + own
                fac = torch.cat([p.reshape(-1, factor.shape[1]) for p in projs]) * amp
                pos = torch.arange(L + 1, device=mean.device)
                toks = torch.arange(V, device=mean.device)
                sub = (pos[:L, None] < s) & (toks[None, :] != xb.tokens[0].long()[:, None])
                dele = (pos[:L] < s) & (s > self.kernel.conv_width)
                ins = (pos[:, None] <= s).expand(L + 1, V)
                valid = torch.cat([sub.reshape(-1), dele, ins.reshape(-1)])
                past = torch.cat([(pos[:L, None] >= s).expand(L, V).reshape(-1), pos[:L] >= s, ~ins.reshape(-1)])
                yield SingleEditPosterior(mean.masked_fill_(past, 0.0), fac, amp ** 2, valid, L, V)
        return neighbourhoods()

    def sample_single_edits(self, input_x, sequence_lengths=None, token_table=None, n_samples=16, random_seed=123, chunk_size=16):
        """Joint posterior draws of EVERY single edit (Thompson sampling; no counterpart in the reference) -> the dict of
        ``predict_single_edits`` with a trailing axis of ``n_samples``: "substitutions" [N, L, V, S], "deletions" [N, L, S] and
        "insertions" [N, L + 1, V, S], numpy float64.  Entry [..., k] is the k-th draw of the mutant's latent value in the units
        of y, mean + trainy_std lambda z'^T F eps_k with F F^T = var and ONE eps_k ~ N(0, I) (``acquisition.standard_normal(nvar,
        n_samples, random_seed)``) for every edit of every sequence, so the draws carry the covariance between mutants: column k
        is what ``SingleEditPosterior.sample`` gives.  Exactly 0 past a sequence's length, NaN for the deletions of a sequence of
        conv_width tokens, the sequence's own draw at its own token.  One projection scan with K = n_samples columns,
        ``proj = F @ eps``: no neighbourhood object and no [E, nvar] factor is formed.  Input, kernels and refusals as for
        ``predict_single_edits(get_var=True)``; ``chunk_size`` sequences go to the device at a time."""
        from .acquisition import standard_normal
        input_x, sequence_lengths = self._joint_scan_input("sample_single_edits", input_x, sequence_lengths, token_table)
        n, L, V = input_x.shape[0], input_x.shape[1], input_x.table.shape[0]
        factor = self._factor_of_var()
        proj = factor @ standard_normal(factor.shape[1], n_samples, random_seed).to(factor.device)
        amp = self.trainy_std * float(self.kernel.get_lambda())
        names = ("substitutions", "deletions", "insertions")
        out = {nm: np.zeros(shape + (n_samples,)) for nm, shape in zip(names, ((n, L, V), (n, L), (n, L + 1, V)))}
        for i in range(0, n, chunk_size):
            xb, lens = input_x[i:i + chunk_size], sequence_lengths[i:i + chunk_size]
            own = torch.from_numpy(np.asarray(self.predict(xb, lens), dtype=np.float64)).to(proj.device)
            means, projs = self._edit_projections(xb, lens, proj)
            for nm, m, p in zip(names, means, projs):
                draws = (m * self.trainy_std + own.view((-1,) + (1,) * (m.dim() - 1)))[..., None] + amp * p
                site = np.arange(m.shape[1])[None, :]
                draws = draws.cpu().numpy()
                draws[site > lens[:, None] if nm == "insertions" else site >= lens[:, None]] = 0
                out[nm][i:i + chunk_size] = draws
        return out

    def select_single_edit_batch(self, input_x, sequence_lengths=None, token_table=None, batch_size=8, beta=2.0, maximize=True):
        """A plate of ``batch_size`` single-edit mutants per sequence that are informative TOGETHER (no counterpart in the reference)
        -> one list per sequence, as ``SingleEditPosterior.select_batch`` returns it: dicts (index, kind, position, token, mean,
        sd) in the order picked.  Greedy GP-BUCB on the joint posterior of ``single_edit_neighbourhoods``: each pick maximises
        mean + beta sd (``maximize`` False: minimises mean - beta sd) with sd conditioned on the earlier picks, so the same
        position with three similar residues is not picked three times as a top-B of marginal UCBs would."""
        return [nb.select_batch(batch_size, beta=beta, maximize=maximize)
                for nb in self.single_edit_neighbourhoods(input_x, sequence_lengths, token_table)]

    def predict_window_scores(self, input_x, sequence_lengths=None, token_table=None, chunk_size=64):
        """The share of every k-mer window in ``predict`` (no counterpart in the reference) -> numpy float64 [N, L]: entry
        [i, j] is what window j = tokens j .. j + conv_width - 1 of sequence i adds to the predicted mean, in the units of y;
        exactly 0 for j >= length - conv_width + 1.  A row's sum plus the training y's mean (plus ``weights[0]`` times its
        standard deviation when the kernel fits an intercept) is ``predict``.  Input and kernels as for ``predict_indels``."""
        input_x, sequence_lengths = self._token_scan_input("predict_window_scores", input_x, sequence_lengths, token_table)
        k = self.kernel
        out = []
        for i in range(0, input_x.shape[0], chunk_size):
            lens = sequence_lengths[i:i + chunk_size]
            nk = torch.from_numpy(np.maximum(np.asarray(lens, dtype=np.int64) - k.conv_width + 1, 1)).to(self.device, torch.float64)
            r = float(np.sqrt(1.0 / k.num_freqs)) / (nk if k.scaling_type == 2 else torch.sqrt(nk) if k.scaling_type == 1
                                                     else torch.ones_like(nk))
            out.append(r[:, None] * k.window_scores(input_x[i:i + chunk_size], lens, self.weights))
        if not out:
            return np.zeros((0, input_x.shape[1]))
        return torch.cat(out).cpu().numpy() * self.trainy_std

    def exact_nmll(self, hyperparams, dataset):
        self.set_hyperparams(hyperparams, dataset)
        return _nmll.exact_nmll(*self._solver_pair(dataset))

    def exact_nmll_gradient(self, hyperparams, dataset, subsample=1):
        self.set_hyperparams(hyperparams, dataset)
        return _nmll.exact_nmll_gradient(*self._solver_pair(dataset), subsample)

    def approximate_nmll(self, hyperparams, dataset, manual_settings=None):
        self.set_hyperparams(hyperparams, dataset)
        return _nmll.approximate_nmll(*self._solver_pair(dataset), None, manual_settings, self.random_seed)

    def tune_hyperparams(self, dataset, bounds=None, max_iter=50, tuning_method="Powell", starting_hyperparams=None,
                         tol=1e-2, n_restarts=1, nmll_method="exact", manual_settings=None):
        self._initialize_kernel(dataset)
        self.weights = self.var = None
        if bounds is None:                   # the two-layer kernel's own bounds, whichever object the routine is handed
            bounds = _default_bounds(self.kernel)
        return _tune(*self._solver_pair(dataset), bounds, max_iter, tuning_method, starting_hyperparams, tol, n_restarts,
                     nmll_method, manual_settings, self.random_seed, self.verbose)

    def tune_hyperparams_crude(self, dataset, bounds=None, random_seed=123, max_bayes_iter=30, subsample=1):
        """xgp_regression.py:497-561."""
        self._initialize_kernel(dataset)
        self.weights = self.var = None
        if bounds is None:
            bounds = _default_bounds(self.kernel)
        return _tune_crude(*self._solver_pair(dataset), bounds, random_seed, max_bayes_iter, subsample, self.verbose)


class xGPClassification(_ModelBase):
    is_regression = False

    def __init__(self, num_rffs=256, kernel_choice="RBF", device="cuda", kernel_settings=None, verbose=True,
                 random_seed=123):
        super().__init__(num_rffs, 0, kernel_choice, device, kernel_settings, verbose, random_seed)

    def fit(self, dataset, preconditioner=None, tol=1e-3, max_iter=500, max_rank=3000, min_rank=512,
            autoselect_target_ratio=30., always_use_srht2=False, run_diagnostics=False, cache_features="auto"):
        """xgp_classification.py:111-200."""
        refuse_half_cache(cache_features, "xGPClassification.fit")
        self._initialize_kernel(dataset)
        kernel, dataset = self._solver_pair(dataset)
        if preconditioner is None:
            preconditioner, _, _ = autoselect_preconditioner(
                kernel, dataset, min_rank, max_rank, 512, always_use_srht2, autoselect_target_ratio,
                self.random_seed, False, self.verbose)
        self.weights, self.gamma, n_iter, losses = fit_classifier(kernel, dataset, preconditioner, tol, max_iter,
                                                                  self.verbose, cache_features)
        if run_diagnostics:
            return n_iter, losses

    def predict(self, input_x, sequence_lengths=None, chunk_size=2000, token_table=None):
        """xgp_classification.py:59-109 -> numpy [N, classes] probabilities.  Token input as ``xGPRegression.predict``."""
        if self.gamma is None:
            raise RuntimeError("Model has not been fitted yet.")
        input_x = token_input(input_x, token_table, self.device)
        return predict_proba(self.kernel, self.weights, self.gamma, self._to_device(input_x), sequence_lengths,
                             chunk_size).cpu().numpy()


class KernelFGen:
    """kernel_fgen.py / auxiliary_baseclass.py:27-92: random features of a chosen kernel for use outside a model
    (kernel k-means, PCA): no intercept column, kernel-specific hyperparameters supplied by the caller."""

    def __init__(self, num_rffs, hyperparams, num_features, kernel_choice="RBF", device="cuda", kernel_settings=None,
                 random_seed=123, verbose=True):
        settings = dict(DEFAULT_KERNEL_SPEC_PARMS if kernel_settings is None else kernel_settings)
        settings["intercept"] = False
        three_d = kernel_choice.startswith(("Conv1d", "Graph"))
        xdim = (1, settings.get("conv_width", 10), num_features) if three_d else (1, num_features)
        self.kernel = make_kernel(kernel_choice, xdim, num_rffs, random_seed, device, settings)
        self.device, self.verbose = device, verbose
        full = self.kernel.get_hyperparams()
        if full.shape[0] > 1:
            full[1:] = hyperparams
        self.kernel.set_hyperparams(full, logspace=True)

    def predict(self, input_x, sequence_lengths=None, chunk_size=2000, token_table=None):
        """-> numpy [N, num_rffs].  Token input (a TokenBatch, or integer tokens with ``token_table``) is expanded chunk by
        chunk; the two-layer kernel pools it from the tokens (``Conv1dTwoLayerKernel.transform_x``)."""
        input_x = token_input(input_x, token_table, self.device)
        preds = []
        for i in range(0, input_x.shape[0], chunk_size):
            sl = None if sequence_lengths is None else sequence_lengths[i:i + chunk_size]
            preds.append(self.kernel.transform_x(input_x[i:i + chunk_size], sl))
        return torch.cat(preds).cpu().numpy()


class FastConv1d:
    """static_layers/fast_conv.py with kernels/convolution_kernels/conv_feature_extractor.py:37-108: the static
    convolution + global max-pool feature extractor (hipConv1dMaxpool) for sequences."""

    def __init__(self, seq_width, device="cuda", random_seed=123, conv_width=9, num_features=512):
        from math import ceil
        from scipy.stats import chi as _chi
        from .kernels import padded_dims
        self.seq_width, self.num_features, self.conv_width, self.device = seq_width, num_features, conv_width, device
        rng = np.random.default_rng(random_seed)
        pdims = padded_dims(conv_width * seq_width)
        radem = rng.choice(np.asarray([-1, 1], dtype=np.int8), size=(3, 1, ceil(num_features / pdims) * pdims),
                           replace=True)
        chi_arr = _chi.rvs(df=pdims, size=num_features, random_state=random_seed).astype(np.float32)
        self.radem_diag = torch.from_numpy(np.ascontiguousarray(radem)).to(device)
        self.chi_arr = torch.from_numpy(chi_arr).to(device)

    def predict(self, x_array, sequence_lengths, chunk_size=2000, token_table=None):
        """-> numpy float32 [N, num_features].  ``x_array`` may be a TokenBatch, or with ``token_table`` an integer token
        array [N, L]: pooled from the tokens (hipConvTokenMaxpool) where the token operator serves the shape, otherwise
        expanded chunk by chunk."""
        from . import xgpr_hip_rfgen_ext as ext
        x_array = token_input(x_array, token_table, self.device)
        if sequence_lengths.shape[0] != x_array.shape[0]:
            raise RuntimeError("The shape[0] of sequence_lengths must match the shape[0] of x_array.")
        if x_array.shape[2] != self.seq_width:
            raise ValueError("Unexpected number of features per timepoint / sequence element on this input.")
        feats = []
        for i in range(0, x_array.shape[0], chunk_size):
            xin = x_array[i:i + chunk_size]
            slen = np.ascontiguousarray(np.asarray(sequence_lengths[i:i + chunk_size]).astype(np.int32))
            out = torch.zeros((xin.shape[0], self.num_features), dtype=torch.float32, device=self.device)
            if isinstance(xin, TokenBatch):
                xin = xin.to(self.device)
                if ext.conv_token_rows_ok(self.conv_width * self.seq_width, xin.table.shape[0], self.seq_width) == 1:
                    ext.hipConvTokenMaxpool(xin.tokens.contiguous(), xin.table.contiguous(), out, self.radem_diag, self.chi_arr,
                                            slen, self.conv_width)
                    feats.append(out)
                    continue
                xin = xin.dense()
            xin = torch.from_numpy(np.ascontiguousarray(xin)) if isinstance(xin, np.ndarray) else xin
            xin = xin.to(self.device, torch.float32).contiguous()
            ext.hipConv1dMaxpool(xin, out, self.radem_diag, self.chi_arr, slen, self.conv_width)
            feats.append(out)
        return torch.cat(feats).cpu().numpy()
