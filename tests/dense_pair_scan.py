"""Dense-matrix reference of the pairwise substitution (epistasis) scan of the sequence / graph kernels (xgpr_conv_token_pair_scan_f32)
-- TEST HELPER, numpy only, in ``np.longdouble``, from tests/dense_reference.py's ``projections`` and ``_windows`` and the operand
sets of tests/dense_subst_scan.py (``make_case``); nothing shared with oracle/.

Definition (notation of tests/dense_subst_scan.py: table[V, C] ALREADY multiplied by sigma, tokens t[0 .. s), nk = s - conv_width + 1
windows, c(win) the window score, r = sqrt(1 / F) / {1, sqrt(nk), nk}[scaling]).  For l1 < l2 = l1 + d < s and 1 <= d < conv_width:

    J            = { j : max(0, l2 - conv_width + 1) <= j <= min(l1, nk - 1) }                 the windows that cover both positions
    out[i, l1, d - 1, v1, v2] = r sum_{j in J} [ c(win_j with v1 at l1 and v2 at l2) - c(win_j with v1 at l1) - c(win_j with v2 at l2) + c(win_j) ]

and 0 where l2 >= s.  The projections are linear in the window: with S[q, v] = projections(e_q (x) table[v]), the conv_width V
single-slot projections, a variant's are  p_j + S[q1, v1] - S[q1, t[l1]] + S[q2, v2] - S[q2, t[l2]]  at q1 = l1 - j, q2 = l2 - j.  With
the four variants of a window written that way the own-token planes come out as zero up to the reference's own rounding.

A window's V x V scores are formed by angle addition in complex long double --  c = Re sum_f (wc_f - i ws_f) e^{i p_f} e^{i a_f[v1]}
e^{i b_f[v2]},  one [V, F] x [F, V] product per window -- which is what keeps V = 21 at F = 1030 and V = 256 within seconds;
``direct=True`` takes cos and sin of the summed projections instead (tests/test_pair_scan_host.py holds the two forms together).

``mistake=`` plants ONE structural error (sensitivity test only):
    "q2_offset"     v2 placed at offset l2 - j + 1 (the window dropped where that is past it)
    "first_window"  only the first shared window
    "norm_by_L"     the normaliser taken from L instead of the sequence's length
    "keep_w0"       w[0] kept under the intercept
    "no_singles"    the two single-substitution terms not subtracted: c(both) - c(win_j)
    "v1_at_l2"      v1 placed at l2 and v2 at l1
    "band_shift"    slot d - 1 filled for l2 = l1 + d + 1
"""
import numpy as np

import dense_reference as dr
import dense_subst_scan as dss
from dense_reference import LD, U64

MISTAKES = ("q2_offset", "first_window", "norm_by_L", "keep_w0", "no_singles", "v1_at_l2", "band_shift")
CLD = np.clongdouble


def pair_scan(tokens, table_scaled, seqlen, w, radem, chi, conv_width, scaling, intercept, mistake=None, direct=False):
    """-> out [n, L, conv_width - 1, V, V] longdouble."""
    tab = np.asarray(table_scaled, dtype=LD)
    V, C = tab.shape
    n, L = tokens.shape
    cw, F = conv_width, chi.shape[0]
    out = np.zeros((n, L, cw - 1, V, V), dtype=LD)
    if cw == 1:
        return out
    w = np.array(w, dtype=LD)
    if intercept and mistake != "keep_w0":
        w[0] = 0
    wc, ws = w[0::2], w[1::2]
    slots = np.zeros((cw, V, cw * C), dtype=LD)
    for q in range(cw):
        slots[q, :, q * C:(q + 1) * C] = tab
    S = dr.projections(slots.reshape(cw * V, cw * C), radem, chi).reshape(cw, V, F)
    ES = np.cos(S) + 1j * np.sin(S)                                         # e^{i S[q, v]}, complex long double
    assert ES.dtype == CLD
    for i in range(n):
        s = int(seqlen[i])
        nk = s - cw + 1
        t = np.asarray(tokens[i, :s], dtype=np.int64)
        p = dr.projections(dr._windows(tab[t], s, cw), radem, chi)          # [nk, F]
        Z = (wc - 1j * ws)[None, :] * (np.cos(p) + 1j * np.sin(p))          # Re(Z e^{i delta}) summed over f = the score of the moved window
        r = np.sqrt(LD(1) / LD(F)) / dss._normaliser(L - cw + 1 if mistake == "norm_by_L" else nk, scaling)
        for l1 in range(s):
            for d in range(1, cw):
                l2 = l1 + d + (1 if mistake == "band_shift" else 0)
                if l2 >= s:
                    continue
                o1, o2 = t[l1], t[l2]
                jlo, jhi = max(0, l2 - cw + 1), min(l1, nk - 1)
                if mistake == "first_window":
                    jhi = min(jhi, jlo)
                acc = np.zeros((V, V), dtype=LD)
                for j in range(jlo, jhi + 1):
                    q1, q2 = l1 - j, l2 - j + (1 if mistake == "q2_offset" else 0)
                    if q2 >= cw:
                        continue
                    if direct:
                        a = S[q1] - S[q1, o1][None, :]                      # [V, F]: what v1 at q1 adds to the projections
                        b = S[q2] - S[q2, o2][None, :]
                        G = dss._score(p[j][None, None, :] + a[:, None, :] + b[None, :, :], wc, ws)
                    else:
                        a = ES[q1] * np.conj(ES[q1, o1])[None, :]
                        b = ES[q2] * np.conj(ES[q2, o2])[None, :]
                        G = ((Z[j][None, :] * a) @ b.T).real
                    # G[v1, v2] = c(win_j with v1 at q1 and v2 at q2); row o1 and column o2 are the single variants, G[o1, o2] the window
                    if mistake == "no_singles":
                        acc += G - G[o1, o2]
                    else:
                        acc += (G - G[:, o2][:, None]) - (G[o1, :][None, :] - G[o1, o2])
                out[i, l1, d - 1] = r * (acc.T if mistake == "v1_at_l2" else acc)
    return out


# ------------------------------------------------------------------------------------------------------------------
# A-priori cap: derived, not tuned; the derivation of tests/dense_subst_scan.py carried to four sums.  A variant window's cos / sin
# values are those of the float32 feature operators, each within cap1 = cap_features(float32, P, norm, |chi|max, c = 1, nk = 1) of exact
# (`norm`: sqrt(conv_width) times the largest row norm of the table bounds every variant window, with one token replaced or two), so a
# window score errs by at most  score = sum|w| cap1 + (2 F + 1) u64 sum|w|.  An output combines FOUR grid sums G of m <= min(conv_width - d,
# nk) <= min(conv_width - 1, nk) window scores each: 4 m score errors, and per G  m + 2 float64 roundings (into the wave slots, then the
# slots combined) on values bounded by m sum|w|.  The double difference is three subtractions on values bounded by 4 m sum|w| and the
# product with r one more rounding of such a value: 4 u64 4 m sum|w|.  Maximum over the sequences (r and m depend on the length).
# ------------------------------------------------------------------------------------------------------------------
def cap_pair_scan(table_scaled_f32, seqlen, w, chi, conv_width, scaling, intercept):
    tab = np.asarray(table_scaled_f32, dtype=np.float32)
    F, P = chi.shape[0], dr.padded_width(conv_width * tab.shape[1])
    w = np.abs(np.asarray(w, dtype=np.float64))
    sw = float(w[1:].sum() if intercept else w.sum())
    norm = float(np.sqrt(conv_width) * dr.max_row_norm(tab))
    cap1 = dr.cap_features(np.float32, P, norm, float(np.abs(chi).max()), 1.0, nk=1)
    score = sw * (cap1 + (2 * F + 1) * U64)
    best = 0.0
    for s in sorted({int(v) for v in seqlen}):
        nk = s - conv_width + 1
        m = max(1, min(conv_width - 1, nk))
        r = float(dr.conv_row_scale(F, nk, scaling))
        best = max(best, r * (4 * (m * score + (m + 2) * U64 * m * sw) + 4 * U64 * 4 * m * sw))
    return best


def check(got, ref, cap):
    """The comparison of the GPU test: no element excused.  -> the largest |got - ref|."""
    return dss.check(got, ref, cap)


# (name, make_case arguments, conv_width, scaling, intercept): the shapes of tests/test_gpu_pair_scan.py, shared with the host test,
# which holds the reference alone to `cap <= 1e-2 max|out|` on every non-degenerate one of them.  Every case scans l1 = 0 and l2 on a
# sequence's last token; the lengths named below add a sequence of ONE window (nk = 1) and one with fewer windows than conv_width.
CASES = [
    ("w16_c4_cw3", dict(n=3, L=9, C=4, V=6, conv_width=3, F=8, lengths=[9, 3, 4]), 0, True),                   # F below P; the non-TP path
    ("w64_onehot21_cw3", dict(n=3, L=10, C=21, V=21, conv_width=3, F=8, onehot=True), 1, False),
    ("w128_c21_cw6", dict(n=2, L=14, C=21, V=21, conv_width=6, F=1030, onehot=True, lengths=[14, 6]), 2, True),   # first TP width; two tiles, the second ragged
    ("w256_c21_cw9", dict(n=1, L=13, C=21, V=4, conv_width=9, F=5000, lengths=[13]), 1, True),                    # a wave takes two tiles
    ("w512_c60_cw8", dict(n=2, L=10, C=60, V=4, conv_width=8, F=600, lengths=[10, 8], extra_reps=2), 2, False),  # packed registers, band 7
    ("w1024_c120_cw8", dict(n=2, L=11, C=120, V=4, conv_width=8, F=1030, lengths=[11, 9]), 0, False),
    ("cw20_c3", dict(n=1, L=24, C=3, V=3, conv_width=20, F=100, lengths=[24]), 1, False),                        # a long band
    ("vocab256_c18", dict(n=1, L=4, C=18, V=256, conv_width=3, F=70, lengths=[4]), 0, False),                    # v1 over the whole grid axis
    ("vocab1", dict(n=2, L=6, C=5, V=1, conv_width=2, F=70), 0, True),                                           # all zeros
    ("dup_rows", dict(n=2, L=8, C=6, V=5, conv_width=4, F=200, dup_rows=(1, 3)), 1, True),                       # two identical rows
    ("graph_cw1", dict(n=3, L=7, C=10, V=9, conv_width=1, F=300, lengths=[7, 1, 4]), 1, True),                   # an empty output
    ("n65", dict(n=65, L=6, C=4, V=3, conv_width=2, F=40), 2, True),
    ("n1", dict(n=1, L=12, C=8, V=4, conv_width=5, F=1500), 0, False),
]
DEGENERATE = ("vocab1", "graph_cw1")


def case(name):
    for nm, kw, scaling, intercept in CASES:
        if nm == name:
            return dss.make_case(**kw), kw["conv_width"], scaling, intercept
    raise KeyError(name)


def reference(name, mistake=None, direct=False):
    """(operands, conv_width, scaling, intercept, reference, cap) of a case."""
    c, cw, scaling, icpt = case(name)
    ref = pair_scan(c["tokens"], c["table"], c["seqlen"], c["w"], c["radem"], c["chi"], cw, scaling, icpt, mistake=mistake, direct=direct)
    return c, cw, scaling, icpt, ref, cap_pair_scan(c["table"], c["seqlen"], c["w"], c["chi"], cw, scaling, icpt)
    return out
