"""Dense-matrix reference of every feature operator, written from the definitions -- TEST HELPER, numpy only.

Third leg of the parity checks, independent of ``oracle/`` and of ``xgpr_amd``: no butterflies, no code shared with
either.  Everything is computed in ``np.longdouble`` with dense Sylvester-Hadamard matrices

    H_P[i, j] = (-1)^popcount(i & j),                      i, j < P = 2^k

applied as plain matrix products (for P > 2048 in Kronecker form, H_P = H_a (x) H_b with a b = P: the row reshaped to
a x b, then H_a X H_b with two dense factors).

Definitions (x a row of ``width`` numbers, zero-padded to P; radem[3, 1, R] signs; chi[F] scales; rep the repetition):

    SORF       y <- x;  three rounds s = 0, 1, 2 of   y <- H_P (y * radem[s, 0, off:off+P]) 2^(-k/2)
    projection p[rep P + j] = chi[rep P + j] * sorf(x, radem, rep P, P)[j]          for j < min(P, F - rep P)
    features   out[2 f] = cos(p[f]) c,  out[2 f + 1] = sin(p[f]) c,  c = sqrt(1/F)  (sqrt(1/(F - 1/2)) with the intercept)
    gradient   a = sigma p[f] (x NOT pre-multiplied by sigma):  features cos(a) c, sin(a) c;
               grad[2 f] = -sin(a) p[f] c,  grad[2 f + 1] = cos(a) p[f] c
    sequences  a window is conv_width x C consecutive elements of the sequence; the first seqlen - conv_width + 1 windows
               (k-mers) are summed: out[2 f] = sum_w cos(p_w[f]) c_row, ... with c_row = sqrt(1/F) / {1, sqrt(nkmers), nkmers}
               for scaling 0, 1, 2; the gradient is the same sum of the per-window gradient terms
    max-pool   out[f] = max(0, max_w p_w[f]) stored as float32
    SRHT       y = H_P (x * radem) 2^(-k/2);    bare FHT  y = H_P x   (2-D rows, or every row of a 3-D array)
    MiniARD    W[j, k] = projection of the unit row e_k at frequency j (a dense [F, d] matrix); sigma_map[k] the lengthscale
               group of input column k, sigma_vals[k] the inverse lengthscale of that column, nl the number of groups:
                   a[i, j]   = sum_k sigma_vals[k] x[i, k] W[j, k]
                   G_l[i, j] = sum_{k: sigma_map[k] = l} x[i, k] W[j, k]
               features out[i, 2 j] = c cos a, out[i, 2 j + 1] = c sin a;
               grad[i, 2 j, l] = -G_l c sin a,  grad[i, 2 j + 1, l] = G_l c cos a       (grad is [n, 2 F, nl])

``mistake=`` arguments exist for the sensitivity test only (tests/test_dense_reference_cpu.py): each plants ONE
structural error in the definition above, so that the test can show the chosen shapes would expose it.
"""
import functools
from math import ceil, log2

import numpy as np

LD = np.longdouble
LD_EPS = float(np.finfo(LD).eps)
U32 = 2.0 ** -24          # unit roundoffs
U64 = 2.0 ** -53
ULD = LD_EPS / 2
DENSE_MAX = 2048          # beyond it the Kronecker form

# glibc documents at most 1 ulp for sinf / cosf / sin / cos (manual, "Errors in Math Functions", x86_64); one ulp of a result in
# [-1, 1] is at most 2 u.  The only constant of the caps below that is not derived from the operation count.
LIBM_ULPS = 1.0


def padded_width(width):
    return 2 ** ceil(log2(max(int(width), 2)))


@functools.lru_cache(maxsize=None)
def hadamard(P):
    """H_P from the definition (-1)^popcount(i & j)."""
    assert P >= 1 and P & (P - 1) == 0
    idx = np.arange(P, dtype=np.int64)
    both = idx[:, None] & idx[None, :]
    parity = np.zeros_like(both)
    while both.any():
        parity ^= both & 1
        both >>= 1
    h = (1 - 2 * parity).astype(LD)
    h.setflags(write=False)
    return h


def kron_split(P):
    k = int(log2(P))
    a = 1 << (k // 2)
    return a, P // a


def apply_hadamard_dense(rows):
    rows = np.asarray(rows, dtype=LD)
    return rows @ hadamard(rows.shape[-1])          # H is symmetric


def apply_hadamard_kron(rows):
    """i = ia b + ib  =>  popcount(i & j) = popcount(ia & ja) + popcount(ib & jb)  =>  Y = H_a X H_b on the a x b reshape."""
    rows = np.asarray(rows, dtype=LD)
    P = rows.shape[-1]
    a, b = kron_split(P)
    xm = rows.reshape(rows.shape[:-1] + (a, b))
    return (hadamard(a) @ xm @ hadamard(b)).reshape(rows.shape)


def apply_hadamard(rows):
    return apply_hadamard_dense(rows) if np.shape(rows)[-1] <= DENSE_MAX else apply_hadamard_kron(rows)


def fht(x):
    """Bare transform over the last axis (2-D and 3-D operator alike)."""
    return apply_hadamard(np.asarray(x, dtype=LD))


def srht(x, radem):
    x = np.asarray(x, dtype=LD)
    P = x.shape[-1]
    return apply_hadamard(x * np.asarray(radem, dtype=LD)) * np.sqrt(LD(1) / LD(P))


def _pad(rows, P, mistake=None):
    rows = np.asarray(rows, dtype=LD)
    out = np.zeros(rows.shape[:-1] + (P,), dtype=LD)
    w = rows.shape[-1]
    out[..., :w] = rows
    if mistake == "pad_last":
        out[..., w:] = rows[..., w - 1:w]
    return out


def sorf(rows, radem, off, P, mistake=None):
    y = _pad(rows, P, mistake)
    scale = np.sqrt(LD(1) / LD(P))                  # 2^(-log2(P) / 2)
    for s in range(3):
        y = apply_hadamard(y * radem[s, 0, off:off + P].astype(LD)) * scale
    return y


def projections(rows, radem, chi, mistake=None):
    """p[m, F] for rows [m, width]: chi[rep P + j] * sorf(row, radem, rep P, P)[j]."""
    rows = np.asarray(rows, dtype=LD)
    F = chi.shape[0]
    P = padded_width(rows.shape[-1])
    chi = np.asarray(chi, dtype=LD)
    out = np.zeros((rows.shape[0], F), dtype=LD)
    for rep in range(ceil(F / P)):
        off = rep * P
        m = min(P, F - off)
        moff = off
        if mistake == "offset" and rep > 0:           # rep * F_tile - 1 with F_tile = min(P, F) frequencies per full tile
            moff = rep * min(P, F) - 1
        out[:, off:off + m] = chi[moff:moff + m] * sorf(rows, radem, moff, P, mistake)[:, :m]
    return out


def _interleave(c, s):
    out = np.empty(c.shape[:-1] + (2 * c.shape[-1],), dtype=LD)
    out[..., 0::2] = c
    out[..., 1::2] = s
    return out


def rbf_scale(F, intercept):
    return np.sqrt(LD(1) / (LD(F) - LD(0.5))) if intercept else np.sqrt(LD(1) / LD(F))


def rbf_features(x, radem, chi, intercept, mistake=None, proj=None):
    """``proj``: projections(x, radem, chi) computed earlier for the same inputs (they do not depend on the intercept)."""
    p = projections(x, radem, chi, mistake) if proj is None else proj
    c = rbf_scale(chi.shape[0], intercept)
    return _interleave(np.cos(p) * c, np.sin(p) * c)


def rbf_grad(x, radem, chi, sigma, intercept, mistake=None, proj=None):
    """-> (features [n, 2F], grad [n, 2F])."""
    p = projections(x, radem, chi, mistake) if proj is None else proj
    c = rbf_scale(chi.shape[0], intercept)
    a = LD(sigma) * p
    return _interleave(np.cos(a) * c, np.sin(a) * c), _interleave(-np.sin(a) * p * c, np.cos(a) * p * c)


def mini_ard_weights(d, radem, chi, by_definition=False):
    """W[F, d] of the MiniARD gradient operator: W[j, k] is the projection of the unit row e_k at frequency j, that is
    ``projections(np.eye(d), radem, chi).T`` (``by_definition=True`` computes exactly that).  By default the same numbers row by row
    instead of column by column: with S = c^3 H D2 H D1 H D0 the SORF matrix of a repetition (c = 2^(-k/2), D_s the sign diagonals),
    (S e_k)[j] = (S^T e_j)[k] and S^T = c^3 D0 H D1 H D2 H -- F transforms of unit rows instead of d of them (d = 2049 pads to 4096;
    the test of this module compares the two forms at the smaller shapes)."""
    d = int(d)
    if by_definition:
        return projections(np.eye(d), radem, chi).T
    F, P = chi.shape[0], padded_width(d)
    out = np.zeros((F, d), dtype=LD)
    scale = np.sqrt(LD(1) / LD(P))
    for rep in range(ceil(F / P)):
        off = rep * P
        m = min(P, F - off)
        y = np.eye(P, dtype=LD)[:m]
        for s in (2, 1, 0):
            y = apply_hadamard(y) * scale * radem[s, 0, off:off + P].astype(LD)
        out[off:off + m] = np.asarray(chi[off:off + m], dtype=LD)[:, None] * y[:, :d]
    return out


def mini_ard_grad(x, W, sigma_map, sigma_vals, intercept, nl, mistake=None):
    """-> (features [n, 2F], grad [n, 2F, nl]); sigma_map[d] the group of every input column, sigma_vals[d] its sigma."""
    x, W = np.asarray(x, dtype=LD), np.asarray(W, dtype=LD)
    smap, sv = np.asarray(sigma_map, dtype=np.int64), np.asarray(sigma_vals, dtype=LD)
    n, d = x.shape
    F = W.shape[0]
    if mistake == "group_edge":                         # every column takes the group of its left neighbour
        smap = np.concatenate([smap[:1], smap[:-1]])
    if mistake == "drop_last":
        x = x.copy()
        x[:, d - 1] = 0
    c = rbf_scale(F, intercept and mistake != "no_half")
    a = (x * sv) @ W.T
    cs, sn = np.cos(a) * c, np.sin(a) * c
    if mistake == "swap_partner":
        cs, sn = sn, cs
    group = np.zeros((nl, n, F), dtype=LD)
    for l in range(nl):
        xl = x * (smap == l)
        group[l] = (xl * sv if mistake == "sigma_in_grad" else xl) @ W.T
    if mistake == "layout":
        grad = np.stack([_interleave(-group[l] * sn, group[l] * cs) for l in range(nl)], axis=1).reshape(n, 2 * F, nl)
    else:
        grad = np.stack([_interleave(-group[l] * sn, group[l] * cs) for l in range(nl)], axis=2)
    if mistake == "swap_partner":
        cs, sn = sn, cs
    return _interleave(cs, sn), grad


def _windows(seq, seqlen, conv_width, mistake=None):
    """[nkmers, conv_width * C]: the first seqlen - conv_width + 1 windows of one sequence [L, C]."""
    nk = int(seqlen) - conv_width + 1
    if mistake == "kmer_more":
        nk += 1
    elif mistake == "kmer_fewer":
        nk -= 1
    seq = np.asarray(seq, dtype=LD)
    if nk + conv_width - 1 > seq.shape[0]:            # (the planted extra window of a full-length sequence runs into zeros)
        seq = np.concatenate([seq, np.zeros((nk + conv_width - 1 - seq.shape[0], seq.shape[1]), dtype=LD)])
    return np.stack([seq[w:w + conv_width].reshape(-1) for w in range(nk)]) if nk > 0 \
        else np.zeros((0, conv_width * seq.shape[1]), dtype=LD)


def conv_projections(x, seqlen, radem, chi, conv_width, mistake=None):
    """One [nkmers_i, F] array of projections per sequence (they do not depend on the scaling type or on sigma)."""
    return [projections(_windows(x[i], seqlen[i], conv_width, mistake), radem, chi, mistake) for i in range(x.shape[0])]


def conv_row_scale(F, nkmers, scaling):
    c = np.sqrt(LD(1) / LD(F))
    return c / {0: LD(1), 1: np.sqrt(LD(nkmers)), 2: LD(nkmers)}[scaling]


def conv_features(x, seqlen, radem, chi, conv_width, scaling, mistake=None, proj=None):
    n, F = x.shape[0], chi.shape[0]
    out = np.zeros((n, 2 * F), dtype=LD)
    proj = conv_projections(x, seqlen, radem, chi, conv_width, mistake) if proj is None else proj
    for i in range(n):
        p = proj[i]
        c = conv_row_scale(F, int(seqlen[i]) - conv_width + 1, scaling)
        out[i] = _interleave(np.cos(p).sum(axis=0) * c, np.sin(p).sum(axis=0) * c)
    return out


def conv_grad(x, seqlen, radem, chi, sigma, conv_width, scaling, mistake=None, proj=None):
    n, F = x.shape[0], chi.shape[0]
    out, grad = np.zeros((n, 2 * F), dtype=LD), np.zeros((n, 2 * F), dtype=LD)
    proj = conv_projections(x, seqlen, radem, chi, conv_width, mistake) if proj is None else proj
    for i in range(n):
        p = proj[i]
        c = conv_row_scale(F, int(seqlen[i]) - conv_width + 1, scaling)
        a = LD(sigma) * p
        out[i] = _interleave(np.cos(a).sum(axis=0) * c, np.sin(a).sum(axis=0) * c)
        grad[i] = _interleave((-np.sin(a) * p).sum(axis=0) * c, (np.cos(a) * p).sum(axis=0) * c)
    return out, grad


def conv_maxpool(x, seqlen, radem, chi, conv_width, mistake=None, proj=None):
    """-> float32 [n, F] (the stored type), and the unrounded longdouble values."""
    n, F = x.shape[0], chi.shape[0]
    out = np.zeros((n, F), dtype=LD)
    proj = conv_projections(x, seqlen, radem, chi, conv_width, mistake) if proj is None else proj
    for i in range(n):
        p = proj[i]
        if p.shape[0]:
            out[i] = np.maximum(p.max(axis=0), LD(0))
    return out.astype(np.float32), out


def design_matrix(x, radem, chi, intercept, proj=None):
    """Z of the solver's products: the features with column 0 set to 1 under the intercept."""
    z = rbf_features(x, radem, chi, intercept, proj=proj)
    if intercept:
        z[:, 0] = 1
    return z


def deinterleaved(out):
    """[cos block | sin block] instead of interleaved pairs (a planted mistake of the sensitivity test)."""
    return np.concatenate([out[..., 0::2], out[..., 1::2]], axis=-1)


# ------------------------------------------------------------------------------------------------------------------
# A-priori forward-error caps.
#
# Model: the operator under test evaluates the same formulas in a binary format of unit roundoff u (2^-24 or 2^-53),
# k = log2 P.
#
# * One butterfly stage computes A_j y with one rounding per output: fl(A_j y) = A_j y + e, |e_i| <= u |(A_j y)_i|, so
#   ||e||_2 <= u ||A_j y||_2.  Writing a normalised round as 2^(-k/2) A_k ... A_1 D y (D the sign diagonal times the
#   rounded constant fl(2^(-k/2)): one rounding for the constant, one for the product, k for the stages), the computed
#   round is within ((1 + u)^(k + 2) - 1) ||y||_2 of the exact one in the 2-norm, and the exact round is orthogonal, so norms
#   carry over unchanged.  Three rounds: every component of the computed SORF output is within
#       E = ((1 + u)^(3 (k + 2)) - 1) ||x||_2
#   of the exact one, and |y_j| <= ||x||_2.
# * projection p = chi_j y_j with one rounding: dp = |chi_j| (E (1 + u) + u ||x||_2); pmax is the largest |p| of the case.
# * cos / sin are 1-Lipschitz and the library returns them within LIBM_ULPS ulp (<= 2 LIBM_ULPS u absolute); the constant c
#   is stored in the kernel's type (relative u) and the product is formed in double (u64):
#       one feature term:  c ((1 + u) (dp + 2 LIBM_ULPS u + u64) + u).
# * a sum over nk k-mers adds the terms' caps; accumulating nk terms of size <= c_row in a format of roundoff ua adds at
#   most (nk - 1) ua nk c_row; the row constant c / sqrt(nk) or c / nk is formed in double (two roundings: 2 u64 relative).
# * max over k-mers and the clip at zero are 1-Lipschitz: dp, plus the rounding of the stored float32, u32 (pmax + dp).
# * gradient: argument a = fl(sigma p^) -> da = sigma dp + u sigma (pmax + dp); trigonometric value times c rounded to the
#   type: ds = c (da + 2 LIBM_ULPS u + u64) + u c; the product of the two computed factors, rounded once:
#       |s^ p^ - s p| <= (c + ds) dp + pmax ds + u (c + ds) (pmax + dp).
# * the output store adds u_out |value| when it is narrower than the arithmetic (float32 rows: u32 nk c_row).
# * where longdouble has fewer than 64 significand bits (eps >= 2e-19) the reference's own dot products are added to E
#   (terms of length n: gamma_n = n u_ld / (1 - n u_ld) per component after normalisation; three rounds of them).
# * products with a vector: t = Z v, w = Z^T t with |dZ| <= cz elementwise, |Z| <= zmax:  |dt| <= cz ||v||_1,
#   |t| <= zmax ||v||_1, |dw| <= n (cz (|t| + |dt|) + zmax |dt|), plus the float64 dot products of the one who forms them
#   ((n + m) u64 n zmax^2 ||v||_1).
# * MiniARD gradient operator (no butterflies: a dense product with the given W, which operator and reference receive alike).
#   Documented arithmetic: every product x_ik W_jk is rounded once in the type T (u); the product with sigma_k, both sums over
#   k and cos / sin are float64; the constant c is rounded to T and then multiplied in float64; G s is rounded once in float64.
#   With A = max_ij sum_k |sigma_k x_ik W_jk| and B = max_ijl sum_{k in l} |x_ik W_jk| (from the reference's own inputs):
#   - argument: term k carries (1 + d_k)(1 + t_k), |d_k| <= u, |t_k| <= (1 + u64)^d - 1 (one rounding for sigma_k *, at most d - 1
#     for the additions), and (1 + u)(1 + u64)^d - 1 <= (u + (d + 1) u64)(1 + u) while d^2 u64 <= 1:
#         da = (u + (d + 1) u64) (1 + u) A
#   - group sum: the same without the product with sigma:      dG = (u + d u64) (1 + u) B
#   - c cos a, c sin a: the trigonometric value is within da (1-Lipschitz) + 2 LIBM_ULPS u64 (library), |value| <= 1; the
#     constant is c (1 + d), |d| <= u; the float64 product adds u64:
#         ds = c ((1 + u) (da + 2 LIBM_ULPS u64 + u64) + u)
#   - gradient: the product of the two computed factors |s^| <= c + ds, |G^| <= B + dG, rounded once in float64:
#         dg = (c + ds) dG + B ds + u64 (c + ds) (B + dG)
#   - where longdouble cannot be taken as exact its own d-term dot products (gamma_d A, gamma_d B) are added to da and dG.
# Every cap is the maximum over rows / windows (largest norm) and frequencies (largest |chi|): one number per case.
# ------------------------------------------------------------------------------------------------------------------

def _reference_round_error(P):
    """gamma_n of the reference's own dense products when longdouble cannot be taken as exact; 0 otherwise."""
    if LD_EPS < 2e-19:
        return 0.0
    n = P if P <= DENSE_MAX else sum(kron_split(P))
    return (n + 2) * ULD / (1 - (n + 2) * ULD)


def _growth(u, m):
    """(1 + u)^m - 1 (1 + 2^-53 is not a float64: through log1p / expm1)."""
    return float(np.expm1(m * np.log1p(u)))


def unit_roundoff(dtype):
    return {np.dtype(np.float32): U32, np.dtype(np.float64): U64}[np.dtype(dtype)]


def cap_fht(dtype, x):
    """Bare transform: k roundings, H = sqrt(P) x orthogonal."""
    u, P = unit_roundoff(dtype), x.shape[-1]
    norm = float(np.sqrt((np.asarray(x, dtype=LD) ** 2).sum(axis=-1)).max())
    return (_growth(u, log2(P)) + _reference_round_error(P)) * np.sqrt(P) * norm


def cap_srht(dtype, x):
    u, P = unit_roundoff(dtype), x.shape[-1]
    norm = float(np.sqrt((np.asarray(x, dtype=LD) ** 2).sum(axis=-1)).max())
    return (_growth(u, log2(P) + 2) + _reference_round_error(P)) * norm


def _projection_cap(u, P, norm, chimax):
    e = (_growth(u, 3 * (log2(P) + 2)) + 3 * _reference_round_error(P)) * norm
    return chimax * (e * (1 + u) + u * norm)


def max_row_norm(rows):
    return float(np.sqrt((np.asarray(rows, dtype=LD) ** 2).sum(axis=-1)).max())


def max_window_norm(x, seqlen, conv_width):
    best = LD(0)
    for i in range(x.shape[0]):
        sq = (np.asarray(x[i, :int(seqlen[i])], dtype=LD) ** 2).sum(axis=1)
        for w in range(int(seqlen[i]) - conv_width + 1):
            best = max(best, sq[w:w + conv_width].sum())
    return float(np.sqrt(best))


def cap_features(dtype, P, norm, chimax, c, nk=1, u_acc=U64, u_out=0.0):
    """Feature operators: c the (row) constant, nk the k-mer count, u_acc the roundoff of the accumulator, u_out the roundoff
    of a narrower stored type (0: stored as computed)."""
    u = unit_roundoff(dtype)
    dp = _projection_cap(u, P, norm, chimax)
    term = c * ((1 + u) * (dp + 2 * LIBM_ULPS * u + U64) + u + 2 * U64)
    total = nk * term + (nk - 1) * u_acc * nk * c
    return total + u_out * (nk * c + total)


def cap_grad(dtype, P, norm, chimax, c, sigma, pmax, nk=1, u_acc=U64):
    """-> (cap of the features of the gradient operator, cap of the gradient).  pmax: the largest |p| of the case, taken from the
    dense reference itself (the worst case |chi|_max ||x||_2 is far above it)."""
    u = unit_roundoff(dtype)
    dp = _projection_cap(u, P, norm, chimax)
    da = sigma * dp + u * sigma * (pmax + dp)
    ds = c * (da + 2 * LIBM_ULPS * u + 3 * U64) + u * c
    dg = (c + ds) * dp + pmax * ds + u * (c + ds) * (pmax + dp)
    return nk * ds + (nk - 1) * u_acc * nk * c, nk * dg + (nk - 1) * u_acc * nk * (c + ds) * (pmax + dp)


def cap_maxpool(dtype, P, norm, chimax, pmax):
    dp = _projection_cap(unit_roundoff(dtype), P, norm, chimax)
    return dp + U32 * (pmax + dp)


def cap_rbf(dtype, x, chi, intercept, u_out=0.0):
    F, P = chi.shape[0], padded_width(x.shape[1])
    return cap_features(dtype, P, max_row_norm(x), float(np.abs(chi).max()), float(rbf_scale(F, intercept)), u_out=u_out)


def cap_rbf_grad(dtype, x, chi, sigma, intercept, pmax):
    F, P = chi.shape[0], padded_width(x.shape[1])
    return cap_grad(dtype, P, max_row_norm(x), float(np.abs(chi).max()), float(rbf_scale(F, intercept)), float(sigma), pmax)


def mini_ard_sums(x, W, sigma_map, sigma_vals, nl):
    """A = max_ij sum_k |sigma_k x_ik W_jk|,  B = max_ijl sum_{k in l} |x_ik W_jk|."""
    ax, aw = np.abs(np.asarray(x, dtype=LD)), np.abs(np.asarray(W, dtype=LD))
    smap = np.asarray(sigma_map, dtype=np.int64)
    big_a = float(((ax * np.abs(np.asarray(sigma_vals, dtype=LD))) @ aw.T).max())
    big_b = max(float(((ax * (smap == l)) @ aw.T).max()) for l in range(nl))
    return big_a, big_b


def cap_mini_ard(dtype, x, W, sigma_map, sigma_vals, intercept, nl):
    """-> (cap of the features, cap of the gradient) of the MiniARD gradient operator."""
    u, d = unit_roundoff(dtype), x.shape[1]
    c = float(rbf_scale(W.shape[0], intercept))
    big_a, big_b = mini_ard_sums(x, W, sigma_map, sigma_vals, nl)
    own = 0.0 if LD_EPS < 2e-19 else (d + 2) * ULD / (1 - (d + 2) * ULD)
    da = (u + (d + 1) * U64) * (1 + u) * big_a + own * big_a
    dG = (u + d * U64) * (1 + u) * big_b + own * big_b
    ds = c * ((1 + u) * (da + 2 * LIBM_ULPS * U64 + U64) + u)
    dg = (c + ds) * dG + big_b * ds + U64 * (c + ds) * (big_b + dG)
    return ds, dg


def _conv_case(x, seqlen, chi, conv_width):
    F, P = chi.shape[0], padded_width(conv_width * x.shape[2])
    return F, P, max_window_norm(x, seqlen, conv_width), sorted({int(s) - conv_width + 1 for s in seqlen})


def cap_conv(dtype, x, seqlen, chi, conv_width, scaling, u_acc=U64, u_out=0.0):
    """The maximum over the rows' k-mer counts (nk c_row grows with nk for scaling 0 and 1)."""
    F, P, norm, nks = _conv_case(x, seqlen, chi, conv_width)
    cm = float(np.abs(chi).max())
    return max(cap_features(dtype, P, norm, cm, float(conv_row_scale(F, nk, scaling)), nk, u_acc, u_out) for nk in nks)


def cap_conv_grad(dtype, x, seqlen, chi, sigma, conv_width, scaling, pmax, u_acc=U64):
    F, P, norm, nks = _conv_case(x, seqlen, chi, conv_width)
    cm = float(np.abs(chi).max())
    caps = [cap_grad(dtype, P, norm, cm, float(conv_row_scale(F, nk, scaling)), float(sigma), pmax, nk, u_acc) for nk in nks]
    return max(c[0] for c in caps), max(c[1] for c in caps)


def cap_conv_maxpool(dtype, x, seqlen, chi, conv_width, pmax):
    P = padded_width(conv_width * x.shape[2])
    return cap_maxpool(dtype, P, max_window_norm(x, seqlen, conv_width), float(np.abs(chi).max()), pmax)


def cap_matvec(cz, zmax, n, m, v):
    """Z^T (Z v) from a Z within cz of the exact one elementwise (|Z| <= zmax), formed in float64."""
    v1 = float(np.abs(np.asarray(v, dtype=LD)).sum())
    dt, t = cz * v1, zmax * v1
    return n * (cz * (t + dt) + zmax * dt) + (n + m) * U64 * n * zmax * zmax * v1


def cap_zty(cz, zmax, n, y):
    y1 = float(np.abs(np.asarray(y, dtype=LD)).sum())
    return cz * y1 + n * U64 * zmax * y1
