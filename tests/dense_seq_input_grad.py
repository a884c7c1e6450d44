"""Dense-matrix reference of the input gradient of the sequence / graph kernels' weighted feature sum (xgpr_conv_input_grad_f32,
xgpr_conv_token_input_grad_f32) -- TEST HELPER, numpy only, in ``np.longdouble``: the overlap-add of tests/dense_input_grad.py's
``rbf_input_grad`` over the windows of tests/dense_reference.py's ``_windows``.

Definition (x[L, C] ALREADY multiplied by sigma, length s, nk = s - conv_width + 1 k-mers, window j = x[j : j + conv_width, :]
flattened, F frequencies, r = sqrt(1 / F) / {1, sqrt(nk), nk}[scaling] -- the same constant with and without the intercept):

    g[l, c] = sum_{j = max(0, l - conv_width + 1)}^{min(l, nk - 1)} G[j, (l - j) C + c],
    G[j]    = rbf_input_grad(window j, w / {1, sqrt(nk), nk}, intercept=False)          (w[0] zeroed by hand under the intercept)

and g[l, :] = 0 for l >= s.  ``rbf_input_grad`` is called with intercept=False because its constant under the intercept,
sqrt(1 / (F - 1/2)), is the fixed-vector kernels' and not these kernels'.

``mistake=`` plants ONE structural error (sensitivity test only):
    "keep_w0"            w[0] kept under the intercept
    "no_norm"            the k-mer normaliser missing (nothing to see at scaling 0)
    "norm_by_L"          the normaliser taken from L instead of the sequence's length
    "shift"              window j added at position j + 1
    "last_only"          only a window's last position added
    "transpose_window"   the window's gradient read as [C, conv_width]
"""
from math import ceil

import numpy as np

import dense_input_grad as dig
import dense_reference as dr
from dense_reference import LD, U64

MISTAKES = ("keep_w0", "no_norm", "norm_by_L", "shift", "last_only", "transpose_window")


def _normaliser(nk, scaling):
    return {0: LD(1), 1: np.sqrt(LD(nk)), 2: LD(nk)}[scaling]


def _row_weights(w, i, nk, scaling, intercept, mistake=None, L=None, conv_width=None):
    """The weight vector handed to the fixed-vector reference for the windows of sequence i."""
    w = np.asarray(w, dtype=LD)
    wi = np.array(w if w.ndim == 1 else w[i], dtype=LD)
    if intercept and mistake != "keep_w0":
        wi[0] = 0
    if mistake == "no_norm":
        return wi
    return wi / _normaliser(L - conv_width + 1 if mistake == "norm_by_L" else nk, scaling)


def seq_input_grad(x_scaled, seqlen, w, radem, chi, sigma, conv_width, scaling, intercept, w_cols=None, mistake=None):
    """-> g [n, L, C] longdouble."""
    x = np.asarray(x_scaled, dtype=LD)
    n, L, C = x.shape
    out = np.zeros((n, L, C), dtype=LD)
    for i in range(n):
        s = int(seqlen[i])
        nk = s - conv_width + 1
        wi = _row_weights(w, i, nk, scaling, intercept, mistake, L, conv_width)
        win = dr._windows(x[i], s, conv_width)
        G = dig.rbf_input_grad(win, wi, radem, chi, sigma, False, w_cols=w_cols).reshape(nk, conv_width, C)
        if mistake == "transpose_window":
            G = G.reshape(nk, C, conv_width).transpose(0, 2, 1)
        for j in range(nk):
            if mistake == "last_only":
                out[i, j + conv_width - 1] += G[j, conv_width - 1]
            elif mistake == "shift":
                hi = min(j + 1 + conv_width, L)
                out[i, j + 1:hi] += G[j, :hi - j - 1]
            else:
                out[i, j:j + conv_width] += G[j]
    return out


# ------------------------------------------------------------------------------------------------------------------
# A-priori cap: derived, not tuned.  The operator's arithmetic per window IS the fixed-vector operator's (one shared device
# function), so a window's gradient is within cap_input_grad(windows as float32, the same weights, intercept=False) of exact; the
# only difference in u -- the constant r is a float64 quotient here (relative 2 u64) and not a float (relative u) -- is covered by
# that cap's `+ u` term.  A position receives min(conv_width, nk) windows at the most: their caps add, and the additions are float64:
# at most min(conv_width, nk) of them on partial sums bounded by the sum itself (to first order; the factor below is relative to the
# cap, which dominates by eight orders of magnitude).  Maximum over the sequences.
# ------------------------------------------------------------------------------------------------------------------
def cap_seq_input_grad(x_scaled_f32, seqlen, w, radem, chi, sigma, conv_width, scaling, intercept, w_cols=None):
    x = np.asarray(x_scaled_f32, dtype=np.float32)
    best = 0.0
    for i in range(x.shape[0]):
        s = int(seqlen[i])
        nk = s - conv_width + 1
        wi = _row_weights(w, i, nk, scaling, intercept)
        win = dr._windows(x[i], s, conv_width).astype(np.float32)
        m = min(conv_width, nk)
        best = max(best, m * dig.cap_input_grad(win, wi, radem, chi, sigma, False, w_cols=w_cols) * (1 + m * U64))
    return best


def make_case(n, L, C, conv_width, F, per_row, seed, lengths=None, stride_pad=0):
    """Seeded operands in the shapes the kernels draw them: x uniform(-1, 1) float32 [n, L, C], sigma = 2.1 / sqrt(conv_width C),
    lengths cycling through ``lengths`` (default: L, conv_width, and values between), signs [3, 1, R], chi from scipy.stats.chi(P),
    standard-normal float64 weights: one vector [2 F] or one row per sequence [n, 2 F + stride_pad] with NaN in the pad.
    -> (x_scaled float32, seqlen int32, w, radem, chi, sigma)."""
    from scipy.stats import chi as chi_dist
    rng = np.random.default_rng([n, L, C, conv_width, F, int(per_row), seed])
    d = conv_width * C
    P = dr.padded_width(d)
    R = ceil(F / P) * P if P < F else P
    x = rng.uniform(-1, 1, size=(n, L, C)).astype(np.float32)
    sigma = 2.1 / np.sqrt(d)
    xs = (x.astype(np.float64) * sigma).astype(np.float32)
    if lengths is None:
        lengths = [L, conv_width, (L + conv_width) // 2, max(conv_width, L - 1)]
    seqlen = np.asarray([lengths[i % len(lengths)] for i in range(n)], dtype=np.int32)
    radem = rng.choice(np.asarray([-1, 1], dtype=np.int8), size=(3, 1, R))
    chi = chi_dist.rvs(df=P, size=F, random_state=rng).astype(np.float32)
    if per_row:
        w = np.full((n, 2 * F + stride_pad), np.nan)
        w[:, :2 * F] = rng.standard_normal((n, 2 * F))
    else:
        w = rng.standard_normal(2 * F)
    return xs, seqlen, w, radem, chi, float(sigma)
