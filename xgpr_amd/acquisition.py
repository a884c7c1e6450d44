"""The JOINT posterior over one sequence's single-edit neighbourhood, and what a design round does with it: joint draws
(Thompson sampling) and a plate of B mutants that are not near-duplicates (greedy GP-BUCB) -- DESIGN.md 3.26.

``xGPRegression.single_edit_neighbourhoods`` builds one ``SingleEditPosterior`` per sequence from the projection scans
(``ConvSORFKernel.substitution_projection_scan`` / ``indel_projection_scan``, ``Conv1dTwoLayerKernel.edit_scan(proj=...)``).
The class itself is plain tensor algebra on whatever device its tensors live on, so it runs -- and is tested -- on the CPU.
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
