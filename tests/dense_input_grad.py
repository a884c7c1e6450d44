"""Dense-matrix reference of the input gradient of a weighted feature sum (xgpr_rbf_input_grad_f32) -- TEST HELPER, numpy only, in
``np.longdouble`` on top of tests/dense_reference.py (its Hadamard matrices, ``projections`` and ``mini_ard_weights``; no butterflies).

Definition (x a row ALREADY multiplied by sigma, p = projections(x), c = rbf_scale(F, intercept), w the weights of the feature
columns -- one vector or one row per datapoint --, only the first w_cols columns carrying weight):

    u_f = c (w[2 f + 1] cos p_f - w[2 f] sin p_f)          (w[0] dropped under the intercept: column 0 is the constant 1)
    g   = sigma (u @ W),    W = mini_ard_weights(d, radem, chi)   [F, d]: W[f, k] = d p_f / d x_k

``rbf_input_grad`` evaluates u @ W without forming W (F transforms of unit rows: minutes at P = 1024): row by row of u it applies,
per repetition, S^T = c^3 D0 H D1 H D2 H to chi (.) u -- the very products ``mini_ard_weights`` forms, in the other association.
``by_weights=True`` computes sigma (u @ mini_ard_weights(...)) literally; tests/test_input_grad_host.py holds the two forms together
at the small shapes.

``mistake=`` plants ONE structural error (sensitivity test only):
    "forward_signs"   the sign diagonals of the transposed transform in the forward order 0, 1, 2
    "swap_partner"    cos and sin exchanged in u
    "keep_w0"         w[0] kept under the intercept
    "no_sigma"        the factor sigma missing
    "rep0_signs"      repetition 0's signs reused for every repetition
"""
from math import ceil, log2

import numpy as np

import dense_reference as dr
from dense_reference import LD, U32, U64, LIBM_ULPS

MISTAKES = ("forward_signs", "swap_partner", "keep_w0", "no_sigma", "rep0_signs")


def split_weights(w, n, F, intercept, w_cols=None, mistake=None):
    """-> (wc, ws) [n, F]: the weights of the cos and sin columns, zero beyond w_cols, w[0] dropped under the intercept."""
    w = np.asarray(w, dtype=LD)
    if w.ndim == 1:
        w = np.broadcast_to(w, (n, w.shape[0]))
    w_cols = min(w.shape[1], 2 * F) if w_cols is None else int(w_cols)
    assert w_cols % 2 == 0 and 2 <= w_cols <= min(w.shape[1], 2 * F) and w.shape[0] == n
    h = w_cols // 2
    wc, ws = np.zeros((n, F), dtype=LD), np.zeros((n, F), dtype=LD)
    wc[:, :h], ws[:, :h] = w[:, 0:w_cols:2], w[:, 1:w_cols:2]
    if intercept and mistake != "keep_w0":
        wc[:, 0] = 0
    return wc, ws


def feature_sum_terms(x_scaled, w, radem, chi, intercept, w_cols=None, mistake=None):
    """-> (u [n, F], p [n, F]) of the definition above."""
    x = np.asarray(x_scaled, dtype=LD)
    F = chi.shape[0]
    p = dr.projections(x, radem, chi)
    wc, ws = split_weights(w, x.shape[0], F, intercept, w_cols, mistake)
    cosv, sinv = np.cos(p), np.sin(p)
    if mistake == "swap_partner":
        cosv, sinv = sinv, cosv
    return dr.rbf_scale(F, intercept) * (ws * cosv - wc * sinv), p


def transposed_sorf(t, radem, d, mistake=None):
    """sum over repetitions of (S_rep^T t_rep)[:d] for rows t [n, F] (zero-padded to whole repetitions)."""
    t = np.asarray(t, dtype=LD)
    n, F = t.shape
    P = dr.padded_width(d)
    scale = np.sqrt(LD(1) / LD(P))
    out = np.zeros((n, d), dtype=LD)
    for rep in range(ceil(F / P)):
        off = rep * P
        m = min(P, F - off)
        y = np.zeros((n, P), dtype=LD)
        y[:, :m] = t[:, off:off + m]
        soff = 0 if mistake == "rep0_signs" else off
        for s in ((0, 1, 2) if mistake == "forward_signs" else (2, 1, 0)):
            y = dr.apply_hadamard(y) * scale * radem[s, 0, soff:soff + P].astype(LD)
        out += y[:, :d]
    return out


def rbf_input_grad(x_scaled_f32, w, radem, chi, sigma, intercept, w_cols=None, mistake=None, by_weights=False):
    """-> g [n, d] longdouble = sigma (u @ mini_ard_weights(d, radem, chi))."""
    x = np.asarray(x_scaled_f32, dtype=LD)
    d = x.shape[1]
    u, _ = feature_sum_terms(x, w, radem, chi, intercept, w_cols, mistake)
    if by_weights:
        assert mistake in (None, "swap_partner", "keep_w0", "no_sigma")
        g = u @ dr.mini_ard_weights(d, radem, chi)
    else:
        g = transposed_sorf(u * np.asarray(chi, dtype=LD), radem, d, mistake)
    return g if mistake == "no_sigma" else g * LD(sigma)


# ------------------------------------------------------------------------------------------------------------------
# A-priori cap, in the model of the comment block of dense_reference.py (u = 2^-24 the operator's butterflies and products,
# u64 = 2^-53 its float64 steps), derived from the operation count; per row, then the maximum over rows:
# * the float32 argument of cos / sin is the feature operators':  dp = _projection_cap(u, P, ||x||_2, chimax);
# * u_f = c (w1 cos p - w0 sin p): cos / sin 1-Lipschitz and within 2 LIBM_ULPS u of exact, widened; two products, one difference
#   and the product with c in float64 (3 u64 on terms of size <= 1); the constant c is stored in float (relative u):
#       du_f = c (|w_2f| + |w_2f+1|) ((1 + u) (dp + 2 LIBM_ULPS u + 3 u64) + u)
# * t_f = fl(fl32(u_f) chi_f): one rounding to float, one for the product:
#       dt_f = |chi_f| (du_f (1 + 2 u) + 2 u |u_f|)
# * a repetition's transposed transform is the forward one's operation count (three rounds of sign x constant, log2 P stages) and
#   orthogonal: computed on t^ = t + dt it is within G ||t^||_2 of S^T t^, G = (1 + u)^(3 (log2 P + 2)) - 1 (+ the reference's own
#   products where longdouble is not taken as exact), and S^T dt has norm ||dt||_2:
#       per repetition and component   G (||t_rep||_2 + ||dt_rep||_2) + ||dt_rep||_2
# * the repetitions are summed (caps add) in float64: nrep - 1 additions of partial sums bounded by sum_rep (||t_rep||_2 +
#   ||dt_rep||_2) (1 + G), one product with sigma, stored as computed:  (nrep + 1) u64 times that bound;
# * everything times sigma.
# ------------------------------------------------------------------------------------------------------------------
def cap_input_grad(x_scaled_f32, w, radem, chi, sigma, intercept, w_cols=None):
    x = np.asarray(x_scaled_f32, dtype=LD)
    n, d = x.shape
    F, P = chi.shape[0], dr.padded_width(d)
    u = U32
    chia = np.abs(np.asarray(chi, dtype=LD))
    c = dr.rbf_scale(F, intercept)
    uf, _ = feature_sum_terms(x, w, radem, chi, intercept, w_cols)
    wc, ws = split_weights(w, n, F, intercept, w_cols)
    norms = np.sqrt((x ** 2).sum(axis=1))
    G = dr._growth(u, 3 * (log2(P) + 2)) + 3 * dr._reference_round_error(P)
    best = 0.0
    for i in range(n):
        dp = dr._projection_cap(u, P, float(norms[i]), float(chia.max()))
        du = c * (np.abs(wc[i]) + np.abs(ws[i])) * ((1 + u) * (dp + 2 * LIBM_ULPS * u + 3 * U64) + u)
        dt = chia * (du * (1 + 2 * u) + 2 * u * np.abs(uf[i]))
        t = chia * np.abs(uf[i])
        total, partial = LD(0), LD(0)
        nrep = ceil(F / P)
        for rep in range(nrep):
            sl = slice(rep * P, min(F, (rep + 1) * P))
            tn, dtn = np.sqrt((t[sl] ** 2).sum()), np.sqrt((dt[sl] ** 2).sum())
            total += G * (tn + dtn) + dtn
            partial += (tn + dtn) * (1 + G)
        total += (nrep + 1) * U64 * partial
        best = max(best, float(total * LD(sigma)))
    return best


def make_case(n, d, F, per_row, seed, stride_pad=0):
    """Seeded operands in the shapes the kernels draw them: x uniform(-1, 1) float32, sigma = 2.1 / sqrt(d), signs [3, 1, R] with R the
    whole repetitions covering F, chi from scipy.stats.chi(P) as float32, standard-normal float64 weights -- one vector [2 F], or one row
    per datapoint [n, 2 F + stride_pad] (the pad is NaN: never to be read).  -> (x_scaled float32, w, radem, chi, sigma)."""
    from scipy.stats import chi as chi_dist
    rng = np.random.default_rng([n, d, F, int(per_row), seed])
    P = dr.padded_width(d)
    R = ceil(F / P) * P if P < F else P
    x = rng.uniform(-1, 1, size=(n, d)).astype(np.float32)
    sigma = 2.1 / np.sqrt(d)
    xs = (x.astype(np.float64) * sigma).astype(np.float32)
    radem = rng.choice(np.asarray([-1, 1], dtype=np.int8), size=(3, 1, R))
    chi = chi_dist.rvs(df=P, size=F, random_state=rng).astype(np.float32)
    if per_row:
        w = np.full((n, 2 * F + stride_pad), np.nan)
        w[:, :2 * F] = rng.standard_normal((n, 2 * F))
    else:
        w = rng.standard_normal(2 * F)
    return xs, w, radem, chi, float(sigma)
