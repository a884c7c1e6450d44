"""Dense-matrix reference of the backward of the two-layer kernel's first layer (xgpr_conv_maxpool_input_grad_f32,
xgpr_conv_token_maxpool_input_grad_f32) -- TEST HELPER, numpy only, in ``np.longdouble``: tests/dense_reference.py's
``conv_projections`` forward, the transposed SORF of tests/dense_input_grad.py backward.

Definition (x[L, C] UNSCALED, length s, nk = s - conv_width + 1 k-mers, window j = x[j : j + conv_width, :] flattened,
p[j, f] = conv_projections, q_f = max(0, max_j p[j, f]), g_f = d m / d q_f):

    a_f = min{ j : p[j, f] = max_j' p[j', f] }  if that maximum is > 0, else -1
    grad[l, c] = sum_{j = max(0, l - conv_width + 1)}^{min(l, nk - 1)} (W1^T u_j)[(l - j) C + c],   u[j, f] = g_f [a_f == j]

and grad[l, :] = 0 for l >= s.  ``gap[i, f]`` is the distance from the maximum to the largest projection of filter f over the k-mers
whose window differs from the winner's (inf if there is none): identical windows tie exactly and do not count (``argmax_and_gap``).

``mistake=`` plants ONE structural error (sensitivity test only):
    "last_argmax"          the LAST k-mer that attains the maximum wins
    "no_relu"              a maximum <= 0 still routes its gradient
    "argmax_of_abs"        the k-mer of largest |p| wins
    "shift"                window j added at position j + 1
    "forward_sign_order"   the sign diagonals of the transposed transform in the forward order 0, 1, 2
    "transpose_window"     the window's gradient read as [C, conv_width]
    "all_windows"          no mask: every k-mer receives g
"""
from math import ceil, log2

import numpy as np

import dense_input_grad as dig
import dense_reference as dr
from dense_reference import LD, U32, U64

MISTAKES = ("last_argmax", "no_relu", "argmax_of_abs", "shift", "forward_sign_order", "transpose_window", "all_windows")


def _row(g, i):
    g = np.asarray(g, dtype=LD)
    return g if g.ndim == 1 else g[i]


def window_ids(seq, seqlen, conv_width):
    """[nk] int: equal for the k-mers whose windows are identical element by element."""
    win = dr._windows(seq, seqlen, conv_width)
    return np.unique(win, axis=0, return_inverse=True)[1].reshape(-1)


def argmax_and_gap(p, mistake=None, ids=None):
    """p [nk, F] -> (a [F] int32, gap [F], top [F]) of the definition above.  The gap is taken to the largest projection among the
    k-mers whose window DIFFERS from the winner's (``ids``: window_ids; None: every other k-mer with a strictly smaller projection).
    Identical windows tie exactly on any operator and do not count; two different windows whose projections coincide -- one-hot or
    periodic inputs produce them: the same +-chi terms summed in another order -- have gap 0, because nothing makes a float32
    operator round them alike."""
    key = np.abs(p) if mistake == "argmax_of_abs" else p
    top = key.max(axis=0)
    hit = key == top[None, :]
    nk = p.shape[0]
    first = np.argmax(hit, axis=0)
    a = (nk - 1 - np.argmax(hit[::-1], axis=0)) if mistake == "last_argmax" else first
    if mistake != "no_relu":
        a = np.where(p[a, np.arange(p.shape[1])] > 0, a, -1)
    same = hit if ids is None else np.asarray(ids)[:, None] == np.asarray(ids)[first][None, :]
    second = np.where(same, LD(-np.inf), key).max(axis=0)
    with np.errstate(invalid="ignore"):
        gap = np.where(np.isfinite(second), top - second, LD(np.inf)).astype(np.float64)
    return a.astype(np.int32), gap, p.max(axis=0)


def _overlap_add(out_i, G, conv_width, L, mistake=None):
    for j in range(G.shape[0]):
        if mistake == "shift":
            hi = min(j + 1 + conv_width, L)
            out_i[j + 1:hi] += G[j, :hi - j - 1]
        else:
            out_i[j:j + conv_width] += G[j]


def pool_input_grad(x, seqlen, g, radem, chi, conv_width, mistake=None, argmax=None, proj=None):
    """-> (grad [n, L, C] longdouble, argmax [n, F] int32, gap [n, F] float64).  ``g`` one vector [>= F] or one row per sequence;
    ``argmax`` given: routed by it instead of the reference's own (the returned argmax and gap stay the reference's)."""
    x = np.asarray(x, dtype=LD)
    n, L, C = x.shape
    F = chi.shape[0]
    d = conv_width * C
    proj = dr.conv_projections(x, seqlen, radem, chi, conv_width) if proj is None else proj
    out = np.zeros((n, L, C), dtype=LD)
    amax, gaps = np.zeros((n, F), dtype=np.int32), np.zeros((n, F))
    chil = np.asarray(chi, dtype=LD)
    for i in range(n):
        p = proj[i]
        nk = p.shape[0]
        amax[i], gaps[i], _ = argmax_and_gap(p, mistake, window_ids(x[i], seqlen[i], conv_width))
        a = amax[i] if argmax is None else np.asarray(argmax[i])
        gi = _row(g, i)[:F]
        hit = np.ones((nk, F), dtype=bool) if mistake == "all_windows" else a[None, :] == np.arange(nk)[:, None]
        t = np.where(hit, (gi * chil)[None, :], LD(0))
        G = dig.transposed_sorf(t, radem, d, "forward_signs" if mistake == "forward_sign_order" else None).reshape(nk, conv_width, C)
        if mistake == "transpose_window":
            G = G.reshape(nk, C, conv_width).transpose(0, 2, 1)
        _overlap_add(out[i], G, conv_width, L, mistake)
        out[i, int(seqlen[i]):] = 0
    return out, amax, gaps


def ambiguous(x_f32, seqlen, radem, chi, conv_width, proj=None, literal=False):
    """bool [n, F]: the pairs where a float32 operator may legitimately pick another window, or another side of the ReLU:
    gap <= 2 cap_conv_maxpool(float32, ...) or |maximum| <= that cap.  ``literal``: the gap to the largest STRICTLY smaller
    projection, which overlooks different windows whose projections coincide in long double (see ``argmax_and_gap``)."""
    x = np.asarray(x_f32, dtype=LD)
    proj = dr.conv_projections(x, seqlen, radem, chi, conv_width) if proj is None else proj
    pmax = max(float(np.abs(p).max()) for p in proj)
    cap = dr.cap_conv_maxpool(np.float32, x, seqlen, chi, conv_width, pmax)
    amb = np.zeros((x.shape[0], chi.shape[0]), dtype=bool)
    for i, p in enumerate(proj):
        _, gap, top = argmax_and_gap(p, ids=None if literal else window_ids(x[i], seqlen[i], conv_width))
        amb[i] = (gap <= 2 * cap) | (np.abs(top.astype(np.float64)) <= cap)
    return amb


# ------------------------------------------------------------------------------------------------------------------
# A-priori cap: derived, not tuned -- cap_input_grad's model (tests/dense_input_grad.py) with the forward-projection term
# removed, since the argmax is held fixed (the ambiguous pairs are excluded by the caller).  u = 2^-24, u64 = 2^-53.
# * t_f = fl(fl32(g_f) chi_f) where a_f == j: one rounding of g to float, one for the product: dt_f = |chi_f g_f| ((1 + u)^2 - 1);
# * a repetition's transposed transform: computed on t^ = t + dt it is within G ||t^||_2 of S^T t^,
#   G = (1 + u)^(3 (log2 P + 2)) - 1 (+ the reference's own products where longdouble is not taken as exact), and S^T dt has norm
#   ||dt||_2:  per repetition and component  G (||t_rep|| + ||dt_rep||) + ||dt_rep||;
# * the repetitions are summed in float64: (nrep + 1) u64 times sum_rep (||t_rep|| + ||dt_rep||) (1 + G);
# * a position receives min(conv_width, nk) windows at the most: the largest window cap of the sequence times that count, through
#   as many float64 additions.  Maximum over the sequences.
# ------------------------------------------------------------------------------------------------------------------
def cap_pool_input_grad(g, argmax, seqlen, chi, conv_width, C):
    F, P = chi.shape[0], dr.padded_width(conv_width * C)
    u = U32
    G = dr._growth(u, 3 * (log2(P) + 2)) + 3 * dr._reference_round_error(P)
    e2 = dr._growth(u, 2)
    chia = np.abs(np.asarray(chi, dtype=LD))
    nrep = ceil(F / P)
    best = 0.0
    for i in range(len(seqlen)):
        nk = int(seqlen[i]) - conv_width + 1
        tg = chia * np.abs(_row(g, i)[:F])
        a = np.asarray(argmax[i])
        worst = LD(0)
        for j in range(nk):
            t = np.where(a == j, tg, LD(0))
            total, partial = LD(0), LD(0)
            for rep in range(nrep):
                tn = np.sqrt((t[rep * P:min(F, (rep + 1) * P)] ** 2).sum())
                dtn = e2 * tn
                total += G * (tn + dtn) + dtn
                partial += (tn + dtn) * (1 + G)
            worst = max(worst, total + (nrep + 1) * U64 * partial)
        m = min(conv_width, nk)
        best = max(best, float(m * worst * (1 + m * U64)))
    return best


def push_bound(err, argmax, seqlen, radem, chi, conv_width, L, C):
    """An error of at most ``err`` in every g[i, f] pushed through the first layer under ``argmax``: the maximum over positions and
    channels of sum_j sum_f |W1[f, (l - j) C + c]| err [a_f == j], with W1 = mini_ard_weights (dense: small shapes only)."""
    d = conv_width * C
    W = np.abs(dr.mini_ard_weights(d, radem, chi))            # [F, d]
    best = 0.0
    for i in range(len(seqlen)):
        nk = int(seqlen[i]) - conv_width + 1
        a = np.asarray(argmax[i])
        out = np.zeros((L, C), dtype=LD)
        Gw = np.stack([(W * (a == j)[:, None]).sum(axis=0) for j in range(nk)]).reshape(nk, conv_width, C) * LD(err)
        _overlap_add(out, Gw, conv_width, L)
        best = max(best, float(out.max()))
    return best


def make_case(n, L, C, conv_width, F, per_row, seed, lengths=None, stride_pad=0, one_hot=False):
    """Seeded operands in the shapes the kernel draws them: x standard normal float32 [n, L, C] (or one-hot rows), lengths cycling
    through ``lengths`` (default: L, conv_width, and values between), signs [3, 1, R] with R the whole repetitions covering F, chi
    from scipy.stats.chi(P), standard-normal float64 g: one vector [F] or one row per sequence [n, F + stride_pad] with NaN in the pad.
    -> (x float32, seqlen int32, g, radem, chi)."""
    from scipy.stats import chi as chi_dist
    rng = np.random.default_rng([n, L, C, conv_width, F, int(per_row), seed])
    P = dr.padded_width(conv_width * C)
    R = ceil(F / P) * P
    if one_hot:
        x = np.eye(C, dtype=np.float32)[rng.integers(0, C, size=(n, L))]
    else:
        x = rng.standard_normal((n, L, C)).astype(np.float32)
    if lengths is None:
        lengths = [L, conv_width, (L + conv_width) // 2, max(conv_width, L - 1)]
    seqlen = np.asarray([lengths[i % len(lengths)] for i in range(n)], dtype=np.int32)
    radem = rng.choice(np.asarray([-1, 1], dtype=np.int8), size=(3, 1, R))
    chi = chi_dist.rvs(df=P, size=F, random_state=rng).astype(np.float32)
    if per_row:
        g = np.full((n, F + stride_pad), np.nan)
        g[:, :F] = rng.standard_normal((n, F))
    else:
        g = rng.standard_normal(F)
    return x, seqlen, g, radem, chi
