"""Kernel k-means and kernel PCA on random features, on the device: the second use of the features that the reference's
auxiliary tutorial names (docs/advanced/auxiliary_tutorial.rst) and leaves to "your package of choice" after
``KernelFGen.predict``.

Both models read FLOAT32 FEATURE ROWS -- what the solver passes stream -- and never a float64 feature matrix on the host:

  * RBF, Matern, Cauchy, Conv1d* and Graph* write their rows with the kernels' own row writers (``cg.fill_rows``), from tokens
    where given; the rows hold the features divided by ``kernel.row_cache_params()[1]`` (row units).
  * a kernel without float32 rows (MiniARD, Linear, Conv1dTwoLayer) runs ``transform_x(...).to(torch.float32)`` chunk by chunk,
    scale 1 -- the fallback the block matvec uses.

The rows are written once and kept when they fit ``CACHE_BUDGET_BYTES`` (``cache_rows``), otherwise every pass regenerates them
window by window (``WINDOW_BYTES``).  A Lloyd iteration is two operators: ``hipKMeansAssign`` (nearest centre,
float64 matrix cores) and ``hipKMeansUpdate`` (per-cluster sums, accumulated across windows); kernel PCA is ``hipZCacheZtY``,
``hipZtZGram`` and ``hipZCacheBlockProject`` put together.  The kernel object is built exactly as ``KernelFGen`` builds its own:
no intercept column, kernel-specific hyperparameters from the caller.
"""
import numpy as np
import torch

from . import xgpr_hip_rfgen_ext as ext
from .cg import any_rows_ok, fill_rows, seq_rows_ok, window_ranges
from .models import KernelFGen, token_input

WINDOW_BYTES = 4 << 30            # float32 rows regenerated per window when the rows are not kept
CACHE_BUDGET_BYTES = 16 << 30     # cache_rows="auto": keep the rows when 4 n num_rffs is at most this
FALLBACK_CHUNK_ROWS = 8192        # rows per float64 transform_x chunk of the kernels without float32 rows
MAX_CLUSTERS = 256                # include/xgpr_hip_cluster.h
MAX_COMPONENTS = 32               # columns of one hipZCacheBlockProject call


class RowSource:
    """The float32 feature rows of ``kernel`` over one input, resident or regenerated window by window.  ``scale``: features =
    scale * rows."""

    def __init__(self, kernel, input_x, sequence_lengths, cache_rows):
        self.kernel, self.m = kernel, kernel.get_num_rffs()
        self.device = torch.device(kernel.device)
        if self.device.type != "cuda":
            raise RuntimeError("The clustering operators run on a HIP device only.")
        self.native = any_rows_ok(kernel)
        if self.native:
            self.x = kernel.scaled_f32(input_x)               # float32 scaled by sigma, or a TokenBatch over the scaled table
            self.scale = float(kernel.row_cache_params()[1])
            self.lens = None
            if seq_rows_ok(kernel):
                if sequence_lengths is None:
                    raise RuntimeError("sequence_length is required for convolution kernels.")
                self.lens = kernel._host_lengths(self.x, sequence_lengths)
        else:
            self.x, self.scale, self.lens = input_x, 1.0, sequence_lengths
        self.n = int(self.x.shape[0])
        if self.n < 1:
            raise RuntimeError("no datapoints")
        win = max(1024, min(self.n, WINDOW_BYTES // (4 * self.m)))
        self.win = win if self.native else min(win, FALLBACK_CHUNK_ROWS)
        self._scratch = None
        self.cache = None
        if cache_rows is True or (cache_rows == "auto" and 4 * self.n * self.m <= CACHE_BUDGET_BYTES):
            self.cache = torch.empty((self.n, self.m), dtype=torch.float32, device=self.device)
            for lo, hi, lens in window_ranges(self.n, self.win, self.lens):
                self._fill(lo, hi, lens, self.cache[lo:hi])

    def _fill(self, lo, hi, lens, out):
        if self.native:
            fill_rows(self.kernel, self.x[lo:hi], lens, out)
        else:
            out.copy_(self.kernel.transform_x(self.x[lo:hi], lens).to(torch.float32))

    def windows(self):
        """(lo, hi, rows float32 [hi - lo, num_rffs]) in order; a regenerated window is valid until the next one is asked for."""
        if self.cache is not None:
            yield 0, self.n, self.cache
            return
        if self._scratch is None:
            self._scratch = torch.empty((min(self.win, self.n), self.m), dtype=torch.float32, device=self.device)
        for lo, hi, lens in window_ranges(self.n, self.win, self.lens):
            rows = self._scratch[:hi - lo]
            self._fill(lo, hi, lens, rows)
            yield lo, hi, rows

    def row(self, i):
        """Row ``i`` widened to float64 [num_rffs] (a private copy)."""
        if self.cache is not None:
            return self.cache[i].to(torch.float64)
        out = torch.empty((1, self.m), dtype=torch.float32, device=self.device)
        self._fill(i, i + 1, None if self.lens is None else self.lens[i:i + 1], out)
        return out[0].to(torch.float64)


class _Base:
    def __init__(self, num_rffs, hyperparams, num_features, kernel_choice, device, kernel_settings, random_seed, verbose):
        self.kernel = KernelFGen(num_rffs, hyperparams, num_features, kernel_choice, device, kernel_settings, random_seed,
                                 verbose).kernel
        self.num_rffs, self.device, self.random_seed, self.verbose = int(num_rffs), device, random_seed, verbose

    def _source(self, input_x, sequence_lengths, token_table, cache_rows):
        return RowSource(self.kernel, token_input(input_x, token_table, self.device), sequence_lengths, cache_rows)


class KernelKMeans(_Base):
    """Lloyd's k-means on the random features of a kernel.  After ``fit``: ``cluster_centers_`` (numpy float64
    [n_clusters, num_rffs], feature units), ``labels_`` (int32), ``inertia_`` and ``inertia_history_`` (feature units),
    ``counts_`` (int64) and ``n_iter_`` (centre updates made).

    One iteration: assign every row to its nearest centre (ties to the lowest index); stop, centres untouched, when no label
    changed or the inertia fell by less than ``tol`` relative; otherwise every non-empty cluster's centre moves to the mean of
    its rows (an EMPTY cluster keeps its previous centre, and ``counts_`` reports the zero).  After ``max_iter`` updates one
    more assignment is made, so ``labels_`` and ``inertia_`` always belong to ``cluster_centers_``."""

    def __init__(self, n_clusters, num_rffs, hyperparams, num_features, kernel_choice="RBF", device="cuda", kernel_settings=None,
                 random_seed=123, max_iter=100, tol=1e-4, init="k-means++", verbose=True):
        if int(num_rffs) % 4 != 0:
            raise RuntimeError(f"KernelKMeans needs num_rffs to be a multiple of 4 (got {num_rffs}).")
        if not 1 <= int(n_clusters) <= MAX_CLUSTERS:
            raise RuntimeError(f"KernelKMeans serves 1 to {MAX_CLUSTERS} clusters (got n_clusters = {n_clusters}).")
        super().__init__(num_rffs, hyperparams, num_features, kernel_choice, device, kernel_settings, random_seed, verbose)
        self.n_clusters, self.max_iter, self.tol, self.init = int(n_clusters), int(max_iter), float(tol), init

    # ---- the two passes over the row source
    def _assign(self, src, centers, labels, dist2):
        for lo, hi, rows in src.windows():
            ext.hipKMeansAssign(rows, centers, labels[lo:hi], None if dist2 is None else dist2[lo:hi])

    def _update(self, src, labels, sums, counts):
        first = True
        for lo, hi, rows in src.windows():
            ext.hipKMeansUpdate(rows, labels[lo:hi], sums, counts, accumulate=not first)
            first = False

    def _init_centers(self, src):
        """float64 device [K, num_rffs] in ROW units."""
        K, m = self.n_clusters, self.num_rffs
        if not isinstance(self.init, str):
            init = np.asarray(self.init, dtype=np.float64)
            if init.shape != (K, m):
                raise RuntimeError(f"init must be a float64 array of shape ({K}, {m}).")
            return torch.from_numpy(np.ascontiguousarray(init / src.scale)).to(src.device)
        if self.init != "k-means++":
            raise RuntimeError('init must be "k-means++" or an array of centres.')
        # k-means++ (Arthur and Vassilvitskii 2007): every new centre is a data row drawn with probability proportional to the
        # running minimum of the squared distance to the centres chosen so far
        rng = np.random.default_rng(self.random_seed)
        centers = torch.empty((K, m), dtype=torch.float64, device=src.device)
        labels = torch.empty(src.n, dtype=torch.int32, device=src.device)
        dist2 = torch.empty(src.n, dtype=torch.float64, device=src.device)
        mind = None
        pick = int(rng.integers(src.n))
        for j in range(K):
            centers[j] = src.row(pick)
            if j + 1 == K:
                break
            self._assign(src, centers[j:j + 1], labels, dist2)
            mind = dist2.clone() if mind is None else torch.minimum(mind, dist2)
            cum = np.cumsum(mind.cpu().numpy())
            pick = int(rng.integers(src.n)) if not cum[-1] > 0 else min(int(np.searchsorted(cum, rng.random() * cum[-1], side="right")),
                                                                         src.n - 1)
        return centers

    def fit(self, input_x, sequence_lengths=None, token_table=None, cache_rows="auto"):
        src = self._source(input_x, sequence_lengths, token_table, cache_rows)
        K, m, dev = self.n_clusters, self.num_rffs, src.device
        centers = self._init_centers(src)
        labels = torch.empty(src.n, dtype=torch.int32, device=dev)
        prev = torch.empty_like(labels)
        dist2 = torch.empty(src.n, dtype=torch.float64, device=dev)
        sums = torch.empty((K, m), dtype=torch.float64, device=dev)
        counts = torch.empty(K, dtype=torch.int64, device=dev)
        history, n_iter, prev_inertia = [], 0, None
        while True:
            self._assign(src, centers, labels, dist2)
            inertia = float(dist2.sum())
            history.append(inertia)
            if n_iter >= self.max_iter:
                break
            if prev_inertia is not None and (bool((labels == prev).all()) or prev_inertia - inertia < self.tol * prev_inertia):
                break
            self._update(src, labels, sums, counts)
            live = counts > 0
            centers[live] = sums[live] / counts[live].to(torch.float64)[:, None]
            prev.copy_(labels)
            prev_inertia = inertia
            n_iter += 1
            if self.verbose:
                print(f"k-means iteration {n_iter}: inertia {inertia * src.scale ** 2:.6e}")
        s2 = src.scale ** 2
        self.cluster_centers_ = (centers * src.scale).cpu().numpy()
        self.labels_ = labels.cpu().numpy()
        self.inertia_history_ = [h * s2 for h in history]
        self.inertia_ = self.inertia_history_[-1]
        self.counts_ = torch.bincount(labels.long(), minlength=K).cpu().numpy().astype(np.int64)
        self.n_iter_ = n_iter
        self._scale = src.scale
        return self

    def fit_predict(self, input_x, sequence_lengths=None, token_table=None, cache_rows="auto"):
        return self.fit(input_x, sequence_lengths, token_table, cache_rows).labels_

    def predict(self, input_x, sequence_lengths=None, token_table=None, chunk_size=2000):
        """int32 numpy labels of new data: the nearest of ``cluster_centers_``."""
        if not hasattr(self, "cluster_centers_"):
            raise RuntimeError("fit has not been called.")
        x = token_input(input_x, token_table, self.device)
        centers = torch.from_numpy(np.ascontiguousarray(self.cluster_centers_ / self._scale)).to(self.device)
        out = []
        for lo in range(0, x.shape[0], chunk_size):
            sl = None if sequence_lengths is None else sequence_lengths[lo:lo + chunk_size]
            src = RowSource(self.kernel, x[lo:lo + chunk_size], sl, True)
            labels = torch.empty(src.n, dtype=torch.int32, device=src.device)
            self._assign(src, centers, labels, None)
            out.append(labels)
        return torch.cat(out).cpu().numpy()


class KernelPCA(_Base):
    """Principal components of the random features of a kernel.  After ``fit``: ``components_`` (numpy float64
    [n_components, num_rffs], unit rows; the entry of largest magnitude of each is positive), ``explained_variance_`` (the
    eigenvalues of the features' covariance Z^T Z / n - mu mu^T, descending) and ``mean_`` (feature units)."""

    def __init__(self, n_components, num_rffs, hyperparams, num_features, kernel_choice="RBF", device="cuda", kernel_settings=None,
                 random_seed=123, verbose=True):
        if not 1 <= int(n_components) <= MAX_COMPONENTS:
            raise RuntimeError(f"KernelPCA serves 1 to {MAX_COMPONENTS} components (got {n_components}).")
        if int(num_rffs) % 128 != 0:
            raise RuntimeError(f"KernelPCA needs num_rffs to be a multiple of 128, the Gram kernel's tile (got {num_rffs}).")
        super().__init__(num_rffs, hyperparams, num_features, kernel_choice, device, kernel_settings, random_seed, verbose)
        self.n_components = int(n_components)

    def fit(self, input_x, sequence_lengths=None, token_table=None, cache_rows="auto"):
        src = self._source(input_x, sequence_lengths, token_table, cache_rows)
        m, dev = self.num_rffs, src.device
        total = torch.zeros(m, dtype=torch.float64, device=dev)
        part = torch.empty_like(total)
        gram = torch.zeros((m, m), dtype=torch.float64, device=dev)
        ws = torch.empty(ext.ztz_workspace_bytes(m, 2), dtype=torch.uint8, device=dev)
        gws = None
        for lo, hi, rows in src.windows():
            ones = torch.ones(hi - lo, dtype=torch.float64, device=dev)
            ext.hipZCacheZtY(rows, ones, part, False, ws, scale=1.0)
            total += part
            gws = ext.hipZtZGram(rows, gram, False, scale=1.0, accumulate=lo > 0, workspace=gws)
        mu = total / src.n                                           # row units
        cov = (gram / src.n - torch.outer(mu, mu)) * src.scale ** 2
        evals, evecs = torch.linalg.eigh(cov)
        top = torch.arange(m - 1, m - 1 - self.n_components, -1, device=dev)
        comps = evecs[:, top].T.contiguous()                         # [n_components, m]
        big = comps.abs().argmax(dim=1)
        sign = torch.sign(comps[torch.arange(self.n_components, device=dev), big])
        comps = comps * torch.where(sign == 0, torch.ones_like(sign), sign)[:, None]
        self._components = comps
        self._mean = mu * src.scale
        self._scale = src.scale
        self.components_ = comps.cpu().numpy()
        self.explained_variance_ = evals[top].cpu().numpy()
        self.mean_ = self._mean.cpu().numpy()
        return self

    def transform(self, input_x, sequence_lengths=None, token_table=None, chunk_size=2000):
        """numpy float64 [N, n_components]: (Z - mean) V, computed as Z V - mean V over float32 rows."""
        if not hasattr(self, "components_"):
            raise RuntimeError("fit has not been called.")
        x = token_input(input_x, token_table, self.device)
        v = self._components.T.contiguous()                          # [m, n_components]
        shift = self._mean @ v
        out = []
        for lo in range(0, x.shape[0], chunk_size):
            sl = None if sequence_lengths is None else sequence_lengths[lo:lo + chunk_size]
            src = RowSource(self.kernel, x[lo:lo + chunk_size], sl, True)
            t = torch.empty((src.n, self.n_components), dtype=torch.float64, device=src.device)
            ext.hipZCacheBlockProject(src.cache, v, t, False, scale=self._scale)
            out.append(t - shift[None, :])
        return torch.cat(out).cpu().numpy()

    def fit_transform(self, input_x, sequence_lengths=None, token_table=None, cache_rows="auto"):
        return self.fit(input_x, sequence_lengths, token_table, cache_rows).transform(input_x, sequence_lengths, token_table)
