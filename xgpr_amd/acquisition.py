"""The JOINT posterior over one sequence's single-edit neighbourhood, and what a design round does with it: joint draws
(Thompson sampling) and a plate of B mutants that are not near-duplicates (greedy GP-BUCB) -- DESIGN.md 3.26.

``xGPRegression.single_edit_neighbourhoods`` builds one ``SingleEditPosterior`` per sequence from the projection scans
(``ConvSORFKernel.substitution_projection_scan`` / ``indel_projection_scan``, ``Conv1dTwoLayerKernel.edit_scan(proj=...)``).
The class itself is plain tensor algebra on whatever device its tensors live on, so it runs -- and is tested -- on the CPU.

``SiteLibrary`` is the result of a combinatorial site-saturation scan (``ConvSORFKernel.site_scan``,
``xGPRegression.predict_site_library``): every variant of K chosen sites as a sum of small tables, with ``dense``,
``gather`` and an exact ``topk`` that never forms V^K -- plain tensor algebra as well.
"""
import torch

KINDS = ("substitution", "deletion", "insertion")


def standard_normal(rows, cols, random_seed):
    """float64 CPU tensor [rows, cols] of standard normal draws: the same numbers for the same seed on every device, so that
    ``SingleEditPosterior.sample`` and ``xGPRegression.sample_single_edits`` draw the same epsilon."""
    gen = torch.Generator(device="cpu")
    gen.manual_seed(int(random_seed))
    return torch.randn((rows, cols), dtype=torch.float64, generator=gen)


class SingleEditPosterior:
    """One sequence's single-edit neighbourhood under the fitted model: E = L V + L + (L + 1) V edits over an array of L
    positions and a table of V tokens, in the order [substitutions (l, v) | deletions p | insertions (g, v)].

    mean   [E]     every edit's predicted mean in the units of y
    factor [E, K]  factor factor^T = the latent posterior covariance of the edits, trainy_std^2 lambda^2 z'^T var z''
    noise          trainy_std^2 lambda^2: what ``predict(get_var=True)`` adds to the latent variance
    valid  [E]     False past the sequence's length, at the sequence's own token (the mutant is the sequence itself) and for a
                   deletion that leaves no window; such rows are never picked
    """

    def __init__(self, mean, factor, noise, valid, positions, vocab):
        E = positions * vocab + positions + (positions + 1) * vocab
        if mean.shape != (E,) or factor.dim() != 2 or factor.shape[0] != E or valid.shape != (E,):
            raise RuntimeError("mean [E], factor [E, K] and valid [E] must hold E = L V + L + (L + 1) V edits.")
        self.mean, self.factor, self.valid = mean, factor, valid.to(torch.bool)
        self.noise = float(noise)
        self.positions, self.vocab = int(positions), int(vocab)

    def __len__(self):
        return self.mean.shape[0]

    def unravel(self, idx):
        """Index of an edit -> (kind, position, token): ("substitution", l, v), ("deletion", p, None) or ("insertion", g, v)."""
        idx, L, V = int(idx), self.positions, self.vocab
        if not 0 <= idx < len(self):
            raise IndexError("no such edit")
        if idx < L * V:
            return KINDS[0], idx // V, idx % V
        idx -= L * V
        if idx < L:
            return KINDS[1], idx, None
        idx -= L
        return KINDS[2], idx // V, idx % V

    def variance(self):
        """[E]: the latent posterior variance of every edit (``predict(get_var=True)`` gives this plus ``noise``)."""
        return (self.factor * self.factor).sum(dim=1)

    def covariance(self, rows_a, rows_b=None):
        """[len(rows_a), len(rows_b)]: the latent posterior covariance between two sets of edits (``rows_b`` None: ``rows_a``)."""
        fa = self.factor[rows_a]
        return fa @ (fa if rows_b is None else self.factor[rows_b]).T

    def sample(self, n_samples=16, random_seed=123):
        """[E, n_samples]: joint draws of the edits' latent values, mean + factor epsilon with ONE epsilon ~ N(0, I_K) per draw
        shared by every edit (``standard_normal(K, n_samples, random_seed)``)."""
        eps = standard_normal(self.factor.shape[1], n_samples, random_seed).to(self.factor.device)
        return self.mean[:, None] + self.factor @ eps

    def select_batch(self, batch_size, beta=2.0, maximize=True):
        """Greedy GP-BUCB: ``batch_size`` times, pick the valid edit not yet taken with the largest mean + beta sd (``maximize``
        False: the smallest mean - beta sd), sd^2 = the latent variance CONDITIONED on a noisy observation at every earlier pick
        plus ``noise``; then condition on the pick.  A Gaussian's conditional covariance does not depend on the observed value,
        so no outcome is needed.  In factor space the posterior of epsilon after t picks is N(., I - sum_s d_s d_s^T) with
        d_t = A f / sqrt(f^T A f + noise), A f = f - sum_s d_s (d_s . f) for the pick's factor row f: one K-vector and one
        ``factor @ d_t`` per pick, never an E x E matrix.  -> list of dicts (index, kind, position, token, mean, sd), mean and sd
        as they stood when the edit was picked; shorter than ``batch_size`` where fewer edits are valid."""
        var = self.variance()
        free = self.valid.clone()
        sign = 1.0 if maximize else -1.0
        dirs, picks = [], []
        for _ in range(int(batch_size)):
            if not bool(free.any()):
                break
            sd = torch.sqrt(var.clamp(min=0.0) + self.noise)
            score = torch.where(free, sign * self.mean + beta * sd, torch.full_like(sd, float("-inf")))
            j = int(torch.argmax(score))
            kind, pos, tok = self.unravel(j)
            picks.append(dict(index=j, kind=kind, position=pos, token=tok, mean=float(self.mean[j]), sd=float(sd[j])))
            free[j] = False
            af = self.factor[j].clone()
            for d in dirs:
                af -= d * (d @ self.factor[j])
            d = af / torch.sqrt((af @ self.factor[j]).clamp(min=0.0) + self.noise)
            dirs.append(d)
            c = self.factor @ d
            var = var - c * c
        return picks


def site_runs(sites, positions, conv_width):
    """The runs of a strictly ascending site list over an array of ``positions`` tokens: as the window start j
    slides over 0 .. positions - conv_width, the sites that window j covers are a contiguous range of the list, and one set is
    covered for one contiguous range of j -> list of (first_window, last_window, first_site, count) in ascending window order.
    The host mirror of ``xgpr_conv_token_site_scan_layout``."""
    runs = []
    for j in range(max(0, sites[0] - conv_width + 1), min(positions - conv_width, sites[-1]) + 1):
        cov = [k for k, p in enumerate(sites) if j <= p < j + conv_width]
        if not cov:
            continue
        if runs and runs[-1][1] == j - 1 and runs[-1][2:] == (cov[0], len(cov)):
            runs[-1] = (runs[-1][0], j) + runs[-1][2:]
        else:
            runs.append((j, j, cov[0], len(cov)))
    return runs


class SiteLibrary:
    """Every variant of K chosen sites of n parent sequences over a table of V tokens -- V^K per parent -- held as a sum of small
    tables: a variant's predicted mean minus its parent's is the sum of ONE entry from each table.

    sites   tuple of the K positions, ascending
    vocab   V
    runs    tuple of tuples of indices into ``sites``: the sites a table depends on (ascending)
    tables  list of float64 tensors, tables[q] of shape [n, V, ..., V] with one axis per site of runs[q]
    base    [n] or None: the parents' own value; ``base[:, None] + gather(a)`` is then each variant's value

    An assignment is K tokens, one per site in the order of ``sites``; its FLAT INDEX is sum_k a_k V^(K-1-k) (the first site most
    significant), which is also its lexicographic rank.  Plain tensor algebra on whatever device the tables live on."""

    DENSE_ELEMS = 1 << 27            # elements dense() -- and topk() per component -- may form

    def __init__(self, sites, vocab, runs, tables, base=None):
        self.sites, self.vocab = tuple(int(p) for p in sites), int(vocab)
        self.runs = tuple(tuple(int(k) for k in r) for r in runs)
        self.tables, self.base = list(tables), base
        if len(self.runs) != len(self.tables):
            raise RuntimeError("one table per run.")
        K = len(self.sites)
        for r, t in zip(self.runs, self.tables):
            if not r or list(r) != sorted(set(r)) or r[0] < 0 or r[-1] >= K:
                raise RuntimeError("a run must name ascending sites of the library.")
            if tuple(t.shape[1:]) != (self.vocab,) * len(r) or t.shape[0] != self.tables[0].shape[0]:
                raise RuntimeError("tables[q] must have the shape [n, V, ..., V] with one axis per site of runs[q].")
        if base is not None and (not self.tables or tuple(base.shape) != (self.n,)):
            raise RuntimeError("base must hold one value per parent sequence.")

    @property
    def n(self):
        return self.tables[0].shape[0] if self.tables else 0

    def components(self):
        """Groups of sites linked through shared runs -> list of tuples of indices into ``sites``, each ascending, in the order of
        their first site.  Two components share no window: their contributions add independently."""
        parent = list(range(len(self.sites)))

        def find(k):
            while parent[k] != k:
                k = parent[k]
            return k
        for r in self.runs:
            for k in r[1:]:
                a, b = find(r[0]), find(k)
                parent[max(a, b)] = min(a, b)
        groups = {}
        for k in range(len(self.sites)):
            groups.setdefault(find(k), []).append(k)
        return [tuple(groups[k]) for k in sorted(groups)]

    def _dense_over(self, comp):
        """[n, V, ..., V] over the sites ``comp`` (ascending indices): the sum, in run order, of the tables whose sites lie in it."""
        V, n = self.vocab, self.n
        if n * V ** len(comp) > self.DENSE_ELEMS:
            raise RuntimeError(f"{len(comp)} linked sites of {V} tokens for {n} sequences are more than SiteLibrary.DENSE_ELEMS = "
                               f"{self.DENSE_ELEMS} elements: use gather() or topk().")
        ref = self.tables[0]
        out = torch.zeros((n,) + (V,) * len(comp), dtype=ref.dtype, device=ref.device)
        axis = {k: a for a, k in enumerate(comp)}
        for r, t in zip(self.runs, self.tables):
            if r[0] in axis:
                shape = [n] + [1] * len(comp)
                for k in r:
                    shape[1 + axis[k]] = V
                out = out + t.reshape(shape)
        return out

    def dense(self):
        """[n, V, ..., V] with K axes: every variant's value minus its parent's.  Refused above ``DENSE_ELEMS`` elements."""
        return self._dense_over(tuple(range(len(self.sites))))

    def gather(self, assignments):
        """[n, m]: the value, minus the parent's, of the m variants ``assignments`` [m, K] (integer tokens): one entry per run,
        added in run order."""
        a = torch.as_tensor(assignments).to(self.tables[0].device, torch.long)
        if a.dim() != 2 or a.shape[1] != len(self.sites):
            raise RuntimeError("assignments must be [m, K]: one token per site.")
        if a.numel() and (int(a.min()) < 0 or int(a.max()) >= self.vocab):
            raise RuntimeError("assignments must hold tokens 0 .. V - 1.")
        out = torch.zeros((self.n, a.shape[0]), dtype=self.tables[0].dtype, device=a.device)
        for r, t in zip(self.runs, self.tables):
            idx = torch.zeros(a.shape[0], dtype=torch.long, device=a.device)
            for k in r:
                idx = idx * self.vocab + a[:, k]
            out = out + t.reshape(self.n, -1)[:, idx]
        return out

    @staticmethod
    def _best(values, assign, k, largest):
        """The k best of ``values`` [n, c] with their ``assign`` [n, c, K]; ties go to the lexicographically smaller assignment."""
        n, c, K = assign.shape
        order = torch.arange(c, device=values.device)[None, :].expand(n, c)
        for col in range(K - 1, -1, -1):                 # (least significant site first: every pass is stable)
            order = torch.gather(order, 1, torch.sort(torch.gather(assign[:, :, col], 1, order), dim=1, stable=True)[1])
        key = torch.gather(-values if largest else values, 1, order)
        order = torch.gather(order, 1, torch.sort(key, dim=1, stable=True)[1])[:, :k]
        return torch.gather(values, 1, order), torch.gather(assign, 1, order[:, :, None].expand(n, order.shape[1], K))

    def topk(self, k, largest=True):
        """The k best variants of every parent -> (values [n, k'], assignments [n, k', K]), k' = min(k, V^K), best first, values
        minus the parent's (add ``base``).  Exact, and without forming V^K: components share no window, so each is made dense
        on its own sites (at most ``DENSE_ELEMS`` elements each), its k best are kept, and the kept candidates of one component
        after another are combined and cut back to k -- a variant among the k best overall is made of parts that are each among
        the k best of their component.  Ties break to the LOWER FLAT INDEX (the lexicographically smaller assignment), in every
        component and in the merge alike: what a stable sort of ``dense().reshape(n, -1)`` gives."""
        k = int(k)
        if k < 1:
            raise RuntimeError("k must be at least 1.")
        K, V, n = len(self.sites), self.vocab, self.n
        dev = self.tables[0].device
        vals = torch.zeros((n, 1), dtype=self.tables[0].dtype, device=dev)
        assign = torch.zeros((n, 1, K), dtype=torch.long, device=dev)
        for comp in self.components():
            dense = self._dense_over(comp).reshape(n, -1)
            c = dense.shape[1]
            digits = torch.zeros((c, K), dtype=torch.long, device=dev)
            flat = torch.arange(c, device=dev)
            for pos, site in enumerate(comp):
                digits[:, site] = (flat // V ** (len(comp) - 1 - pos)) % V
            cv, ca = self._best(dense, digits[None].expand(n, c, K), k, largest)
            # every kept candidate so far with every kept candidate of this component (their sites are disjoint)
            sums = (vals[:, :, None] + cv[:, None, :]).reshape(n, -1)
            both = (assign[:, :, None, :] + ca[:, None, :, :]).reshape(n, -1, K)
            vals, assign = self._best(sums, both, k, largest)
        return vals, assign
