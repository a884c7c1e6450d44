"""Dense-matrix reference of the single-substitution scan of the sequence / graph kernels (xgpr_conv_token_subst_scan_f32) -- TEST
HELPER, numpy only, in ``np.longdouble``, from tests/dense_reference.py's ``projections`` and ``_windows``; nothing shared with
oracle/.

Definition (table[V, C] ALREADY multiplied by sigma, tokens t[0 .. s), nk = s - conv_width + 1 windows, window j =
table[t[j .. j + conv_width)] flattened, p = projections(window), F frequencies, r = sqrt(1 / F) / {1, sqrt(nk), nk}[scaling]):

    c(win)       = sum_f (w[2f] cos p_f + w[2f+1] sin p_f)                    (w[0] dropped under the intercept)
    J(l)         = { j : max(0, l - conv_width + 1) <= j <= min(l, nk - 1) }
    out[i, l, v] = r ( sum_{j in J(l)} c(win_j with the token at offset l - j replaced by v)  -  sum_{j in J(l)} c(win_j) )

for l < s, and 0 for l >= s.  The projections are linear in the window: a variant's are p_j + S[q, v] - S[q, t[l]] with
S[q, v] = projections(e_q (x) table[v]), the conv_width V single-slot projections, computed once per case.

``mistake=`` plants ONE structural error (sensitivity test only):
    "offset"          the token substituted at offset l - j + 1 (none where that is past the window)
    "first_window"    only the first covering window
    "norm_by_L"       the normaliser taken from L instead of the sequence's length
    "keep_w0"         w[0] kept under the intercept
    "no_wild"         the unmutated sum not subtracted
    "table_transposed"  table row v read as column v
"""
from math import ceil

import numpy as np

import dense_reference as dr
from dense_reference import LD, U64

MISTAKES = ("offset", "first_window", "norm_by_L", "keep_w0", "no_wild", "table_transposed")


def _normaliser(nk, scaling):
    return {0: LD(1), 1: np.sqrt(LD(nk)), 2: LD(nk)}[scaling]


def _score(p, wc, ws):
    return (np.cos(p) * wc + np.sin(p) * ws).sum(axis=-1)


def subst_scan(tokens, table_scaled, seqlen, w, radem, chi, conv_width, scaling, intercept, mistake=None):
    """-> out [n, L, V] longdouble."""
    tab = np.asarray(table_scaled, dtype=LD)
    V, C = tab.shape
    n, L = tokens.shape
    cw, F = conv_width, chi.shape[0]
    w = np.array(w, dtype=LD)
    if intercept and mistake != "keep_w0":
        w[0] = 0
    wc, ws = w[0::2], w[1::2]
    sub = tab
    if mistake == "table_transposed":
        sub = np.zeros_like(tab)
        m = min(V, C)
        sub[:m, :m] = tab[:m, :m].T
    # single-slot projections: S[q, v] of the table the windows are built from, Sv[q, v] of the table the substitute is read from
    slots = np.zeros((cw, V, cw * C), dtype=LD)
    vslots = np.zeros((cw, V, cw * C), dtype=LD)
    for q in range(cw):
        slots[q, :, q * C:(q + 1) * C] = tab
        vslots[q, :, q * C:(q + 1) * C] = sub
    S = dr.projections(slots.reshape(cw * V, cw * C), radem, chi).reshape(cw, V, F)
    Sv = S if sub is tab else dr.projections(vslots.reshape(cw * V, cw * C), radem, chi).reshape(cw, V, F)
    out = np.zeros((n, L, V), dtype=LD)
    for i in range(n):
        s = int(seqlen[i])
        nk = s - cw + 1
        t = np.asarray(tokens[i, :s], dtype=np.int64)
        p = dr.projections(dr._windows(tab[t], s, cw), radem, chi)          # [nk, F]
        base = _score(p, wc, ws)                                            # [nk]
        r = np.sqrt(LD(1) / LD(F)) / _normaliser(L - cw + 1 if mistake == "norm_by_L" else nk, scaling)
        for l in range(s):
            jlo, jhi = max(0, l - cw + 1), min(l, nk - 1)
            if mistake == "first_window":
                jhi = jlo
            acc = np.zeros(V, dtype=LD)
            for j in range(jlo, jhi + 1):
                q = l - j + (1 if mistake == "offset" else 0)
                if q < cw:
                    acc += _score(p[j][None, :] + Sv[q] - S[q, t[j + q]][None, :], wc, ws)
                else:
                    acc += base[j]
                if mistake != "no_wild":
                    acc -= base[j]
            out[i, l] = r * acc
    return out


# ------------------------------------------------------------------------------------------------------------------
# A-priori cap: derived, not tuned.  The operator forms a variant window's cos / sin values as the float32 feature operators do, so
# each is within  cap1 = cap_features(float32, P, norm, |chi|max, c = 1, nk = 1)  of exact, with `norm` a bound on EVERY variant
# window's 2-norm: sqrt(conv_width) times the largest row norm of the (float32) table.  A window score multiplies 2 F such values by
# the float64 weights and adds them in float64: |error| <= sum|w| cap1 + (2 F + 1) u64 sum|w| (products and partial sums are bounded
# by sum|w|).  An output adds |J(l)| <= min(conv_width, nk) variant scores per wave slot, combines the slots, subtracts as many
# unmutated scores' sum and multiplies by r: m = 2 min(conv_width, nk) score errors, and m + 2 float64 roundings on values bounded by
# m sum|w|.  Maximum over the sequences (r and m depend on the length).
# ------------------------------------------------------------------------------------------------------------------
def cap_subst_scan(table_scaled_f32, seqlen, w, chi, conv_width, scaling, intercept):
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
        m = 2 * min(conv_width, nk)
        r = float(dr.conv_row_scale(F, nk, scaling))
        best = max(best, r * (m * score + (m + 2) * U64 * m * sw))
    return best


def check(got, ref, cap):
    """The comparison of the GPU test: no element excused.  -> the largest |got - ref|."""
    err = float(np.abs(np.asarray(got, dtype=LD) - ref).max()) if ref.size else 0.0
    assert np.isfinite(np.asarray(got, dtype=np.float64)).all()
    assert err <= cap, (err, cap)
    return err


def make_case(n, L, C, V, conv_width, F, seed=0, lengths=None, onehot=False, extra_reps=0, dup_rows=None):
    """Seeded operands: a table [V, C] -- uniform(-1, 1), or one-hot rows --, scaled so that a row's norm is about 1 (a substitution
    moves a projection by about a radian); tokens uniform in [0, V), positions past a length filled with 255 where V < 256 (never read);
    lengths cycling through ``lengths`` (default: L, conv_width, values between, one with nk < conv_width where L allows); signs
    [3, 1, R] with ``extra_reps`` unused transforms; chi from scipy.stats.chi(P); weights standard normal times rank^-1.5 under a
    random order of the columns, column 0 among the three heaviest: sum|w| stays within a small multiple of |w|_2, which is what keeps the
    a-priori cap (proportional to sum|w|) two orders below the outputs (proportional to |w|_2) at every width.  ``dup_rows`` = (a, b): table row b is a copy of row a.
    -> dict(tokens uint8, table float32 (scaled), seqlen int32, w float64, radem int8, chi float32)."""
    from scipy.stats import chi as chi_dist
    rng = np.random.default_rng([n, L, C, V, conv_width, F, seed])
    d = conv_width * C
    P = dr.padded_width(d)
    R = max(P, ceil(F / P) * P) + extra_reps * P
    if onehot:
        table = np.zeros((V, C))
        table[np.arange(V), np.arange(V) % C] = 1.0
        table = (table * 1.1).astype(np.float32)
    else:
        table = (rng.uniform(-1, 1, size=(V, C)) * (1.0 / np.sqrt(C / 3.0))).astype(np.float32)
    if dup_rows is not None:
        table[dup_rows[1]] = table[dup_rows[0]]
    if lengths is None:
        lengths = [L, conv_width, (L + conv_width) // 2, max(conv_width, L - 1), min(L, 2 * conv_width - 2) if conv_width > 1 else 1]
    seqlen = np.asarray([lengths[i % len(lengths)] for i in range(n)], dtype=np.int32)
    tokens = rng.integers(0, V, size=(n, L)).astype(np.uint8)
    if V < 256:
        tokens[np.arange(L)[None, :] >= seqlen[:, None]] = 255
    radem = rng.choice(np.asarray([-1, 1], dtype=np.int8), size=(3, 1, R))
    chi = chi_dist.rvs(df=P, size=F, random_state=rng).astype(np.float32)
    order = rng.permutation(2 * F)
    k = int(np.where(order == 0)[0][0])
    order[[k, 2 % (2 * F)]] = order[[2 % (2 * F), k]]                # column 0 takes rank 3
    w = np.zeros(2 * F)
    w[order] = rng.standard_normal(2 * F) * (1.0 + np.arange(2 * F)) ** -1.5
    w[0] = np.copysign(max(abs(w[0]), 0.1), w[0] if w[0] != 0 else 1.0)
    return dict(tokens=tokens, table=table, seqlen=seqlen, w=w, radem=radem, chi=chi)


# (name, make_case arguments, conv_width, scaling, intercept): the shapes of tests/test_gpu_subst_scan.py, shared with the host test,
# which holds the reference alone to `cap <= 1e-2 max|out|` on every one of them.
CASES = [
    ("w16_c4_cw3", dict(n=3, L=9, C=4, V=6, conv_width=3, F=8, lengths=[9, 3, 4]), 0, True),                       # F below P; padded width 16
    ("w64_onehot21_cw3", dict(n=3, L=10, C=21, V=21, conv_width=3, F=8, onehot=True), 1, False),  # F = 8 at P = 64
    ("w128_c21_cw6", dict(n=3, L=14, C=21, V=21, conv_width=6, F=1030, onehot=True, lengths=[14, 6, 8]), 2, True),  # two tiles, ragged; LOG2P = 7
    ("w256_c21_cw9", dict(n=3, L=20, C=21, V=7, conv_width=9, F=5000, lengths=[20, 9, 13]), 1, True),                # a wave takes two tiles
    ("w1024_c21_cw48", dict(n=3, L=50, C=21, V=3, conv_width=48, F=1030, lengths=[50, 48, 49]), 0, False),   # packed registers
    ("w512_c16_cw20", dict(n=2, L=24, C=16, V=4, conv_width=20, F=600, extra_reps=2), 2, False),   # N = 8; radem larger than needed
    ("graph_cw1", dict(n=3, L=7, C=10, V=9, conv_width=1, F=300, lengths=[7, 1, 4]), 1, True),  # conv_width = 1
    ("vocab1", dict(n=2, L=6, C=5, V=1, conv_width=2, F=70), 0, True),                          # all zeros
    ("vocab256_c18", dict(n=2, L=6, C=18, V=256, conv_width=3, F=130), 0, False),               # the largest table
    ("dup_rows", dict(n=2, L=8, C=6, V=5, conv_width=4, F=200, dup_rows=(1, 3)), 1, True),      # two identical rows
    ("n65", dict(n=65, L=6, C=4, V=3, conv_width=2, F=40), 2, True),
    ("n1", dict(n=1, L=12, C=8, V=4, conv_width=5, F=1500), 0, False),
]


def case(name):
    for nm, kw, scaling, intercept in CASES:
        if nm == name:
            return make_case(**kw), kw["conv_width"], scaling, intercept
    raise KeyError(name)
