"""Dense-matrix reference of the window scores and the single-deletion / single-insertion scan of the sequence / graph kernels
(xgpr_conv_token_window_scores_f32, xgpr_conv_token_indel_scan_f32) -- TEST HELPER, numpy only, in ``np.longdouble``, from
tests/dense_reference.py's ``projections``; nothing shared with oracle/.

Definition (table[V, C] ALREADY multiplied by sigma, tokens t[0 .. s), nk = s - conv_width + 1 windows, window j =
table[t[j .. j + conv_width)] flattened, p = projections(window), F frequencies, r(k) = sqrt(1 / F) / {1, sqrt(k), k}[scaling]):

    c(win)       = sum_f (w[2f] cos p_f + w[2f+1] sin p_f)                    (w[0] dropped under the intercept)
    m(t)         = r(nk) sum_{j < nk} c(win_j)
    scores[i, j] = c(win_j) for j < nk, 0 beyond
    del[i, p]    = m(t without position p) - m(t)                      p < s;  0 beyond;  NaN where s == conv_width
    ins[i, g, v] = m(t with token v inserted before position g) - m(t)  g <= s; 0 beyond

``indel_scan`` is BRUTE FORCE: every mutant is built as a token sequence and m is evaluated on ALL its windows; the only shortcut is
the linearity of the projections in the window (a window's projections are the sum of its conv_width single-slot projections
S[q, token], computed once per case).  ``decomposed`` evaluates the contract's decomposition (removed windows R, added windows A, the
total T under the new normaliser) instead -- what the kernels implement -- and ``mistake=`` plants ONE structural error in it
(sensitivity test only):
    "junction_short"        the deletion's junction windows stop one short of min(p - 1, nk - 2)
    "remap_wrong_side"      a junction window's offset k reads k + (k > q) instead of k + (k >= q): the deleted token is kept, the next dropped
    "old_norm"              the sequence's own normaliser r(nk) used for the mutant
    "norm_by_length"        the mutant's normaliser taken from its length s -+ 1 instead of its window count nk -+ 1
    "keep_w0"               w[0] kept under the intercept
    "ins_removes_covering"  an insertion at g removes the windows that cover position g instead of those that straddle the gap
    "append_past_end"       the gap g = s treated as past the end (zeros)
"""
import functools

import numpy as np

import dense_reference as dr
from dense_reference import LD, U64
from dense_subst_scan import CASES as SUBST_CASES, make_case

MISTAKES = ("junction_short", "remap_wrong_side", "old_norm", "norm_by_length", "keep_w0", "ins_removes_covering", "append_past_end")


# (name, make_case arguments, scaling, intercept): the cases of tests/dense_subst_scan.py -- the same shapes, scalings and intercept flags,
# every padded width class 16 ... 1024 -- with the ragged lengths of two of them moved so that every ragged case holds L, conv_width (the
# mutant of a deletion has no window: NaN) and conv_width + 1 (a deletion leaves one window).
_LENGTHS = {"w128_c21_cw6": [14, 6, 7], "w256_c21_cw9": [20, 9, 10]}
CASES = [(nm, dict(kw, lengths=_LENGTHS[nm]) if nm in _LENGTHS else kw, scaling, icpt) for nm, kw, scaling, icpt in SUBST_CASES]


def case(name):
    for nm, kw, scaling, intercept in CASES:
        if nm == name:
            return make_case(**kw), kw["conv_width"], scaling, intercept
    raise KeyError(name)


def _r(F, k, scaling):
    return np.sqrt(LD(1) / LD(F)) / {0: LD(1), 1: np.sqrt(LD(k)), 2: LD(k)}[scaling]


class _Scorer:
    """c(window) for windows given as token tuples, through the single-slot projections S[q, v]."""

    def __init__(self, table_scaled, w, radem, chi, conv_width, intercept, keep_w0=False):
        tab = np.asarray(table_scaled, dtype=LD)
        V, C = tab.shape
        self.cw, self.F, self.V = conv_width, chi.shape[0], V
        w = np.array(w, dtype=LD)
        if intercept and not keep_w0:
            w[0] = 0
        self.wc, self.ws = w[0::2], w[1::2]
        slots = np.zeros((conv_width, V, conv_width * C), dtype=LD)
        for q in range(conv_width):
            slots[q, :, q * C:(q + 1) * C] = tab
        self.S = dr.projections(slots.reshape(conv_width * V, conv_width * C), radem, chi).reshape(conv_width, V, self.F)
        self.q = np.arange(conv_width)
        self.memo = {}

    def windows(self, wins):
        """wins [m, cw] int -> c of each, [m] longdouble."""
        wins = np.asarray(wins, dtype=np.int64).reshape(-1, self.cw)
        if wins.shape[0] == 0:
            return np.zeros(0, dtype=LD)
        p = self.S[self.q[None, :], wins].sum(axis=1)                            # [m, F]
        return (np.cos(p) * self.wc + np.sin(p) * self.ws).sum(axis=-1)

    def sequence(self, t):
        """The scores of all windows of token sequence t.  c is a pure function of a window's tokens: a value is computed once per
        distinct window and remembered (the mutants of one sequence share most of their windows)."""
        keys = [tuple(int(v) for v in t[j:j + self.cw]) for j in range(len(t) - self.cw + 1)]
        new = sorted(set(keys) - set(self.memo))
        if new:
            self.memo.update(zip(new, self.windows(np.asarray(new, dtype=np.int64))))
        return np.asarray([self.memo[k] for k in keys], dtype=LD)


def window_scores(tokens, table_scaled, seqlen, w, radem, chi, conv_width, intercept, scorer=None):
    """-> scores [n, L] longdouble.  (``scorer``: a _Scorer of the same operands, to share its single-slot projections.)"""
    sc = scorer or _Scorer(table_scaled, w, radem, chi, conv_width, intercept)
    n, L = tokens.shape
    out = np.zeros((n, L), dtype=LD)
    for i in range(n):
        s = int(seqlen[i])
        out[i, :s - conv_width + 1] = sc.sequence(tokens[i, :s])
    return out


def indel_scan(tokens, table_scaled, seqlen, w, radem, chi, conv_width, scaling, intercept, scorer=None):
    """-> (del [n, L], ins [n, L + 1, V]) longdouble, by brute force over the mutants."""
    sc = scorer or _Scorer(table_scaled, w, radem, chi, conv_width, intercept)
    n, L = tokens.shape
    V, cw, F = sc.V, conv_width, sc.F
    dele = np.zeros((n, L), dtype=LD)
    ins = np.zeros((n, L + 1, V), dtype=LD)

    def m(t):
        nk = len(t) - cw + 1
        return _r(F, nk, scaling) * sc.sequence(t).sum() if nk > 0 else LD("nan")

    for i in range(n):
        s = int(seqlen[i])
        t = [int(v) for v in tokens[i, :s]]
        base = m(t)
        for p in range(s):
            dele[i, p] = m(t[:p] + t[p + 1:]) - base
        for g in range(s + 1):
            for v in range(V):
                ins[i, g, v] = m(t[:g] + [v] + t[g:]) - base
    return dele, ins


def decomposed(tokens, table_scaled, seqlen, w, radem, chi, conv_width, scaling, intercept, mistake=None):
    """The contract's decomposition (include/xgpr_hip_indel_scan.h), in long double -> (del, ins); ``mistake`` plants one error."""
    sc = _Scorer(table_scaled, w, radem, chi, conv_width, intercept, keep_w0=mistake == "keep_w0")
    n, L = tokens.shape
    V, cw, F = sc.V, conv_width, sc.F
    dele = np.zeros((n, L), dtype=LD)
    ins = np.zeros((n, L + 1, V), dtype=LD)
    for i in range(n):
        s = int(seqlen[i])
        nk = s - cw + 1
        t = np.asarray(tokens[i, :s], dtype=np.int64)
        scores = sc.sequence(t)
        T, r = scores.sum(), _r(F, nk, scaling)
        # deletions
        kd = s - 1 if mistake == "norm_by_length" else nk - 1
        for p in range(s):
            if nk == 1:
                dele[i, p] = LD("nan")
                continue
            rm = r if mistake == "old_norm" else _r(F, kd, scaling)
            lo, hi = max(0, p - cw + 1), min(p - 1, nk - 2) - (1 if mistake == "junction_short" else 0)
            A = LD(0)
            for j in range(lo, hi + 1):
                q = p - j
                k = np.arange(cw)
                A += sc.windows(t[j + k + ((k > q) if mistake == "remap_wrong_side" else (k >= q))])[0]
            R = scores[lo:min(p, nk - 1) + 1].sum()
            dele[i, p] = rm * (A - R) + (rm - r) * T
        # insertions
        ki = s + 1 if mistake == "norm_by_length" else nk + 1
        rm = r if mistake == "old_norm" else _r(F, ki, scaling)
        for g in range(s + 1):
            if g == s and mistake == "append_past_end":
                continue
            lo = max(0, g - cw + 1)
            R = scores[lo:min(g if mistake == "ins_removes_covering" else g - 1, nk - 1) + 1].sum()
            for v in range(V):
                A = LD(0)
                for j in range(lo, min(g, nk) + 1):
                    q = g - j
                    A += sc.windows(np.concatenate([t[j:j + q], [v], t[j + q:j + cw - 1]]))[0]
                ins[i, g, v] = rm * (A - R) + (rm - r) * T
    return dele, ins


# ------------------------------------------------------------------------------------------------------------------
# A-priori caps: derived, not tuned.  The per-score bound is that of tests/dense_subst_scan.py: the operator forms a window's cos /
# sin values as the float32 feature operators do, each within  cap1 = cap_features(float32, P, norm, |chi|max, c = 1, nk = 1)  of exact
# with `norm` a bound on EVERY window's 2-norm (mutant windows included): sqrt(conv_width) times the largest row norm of the table; a
# score multiplies 2 F such values by the float64 weights and adds them in float64:
#     score = sum|w| (cap1 + (2 F + 1) u64)                                (products and partial sums are bounded by sum|w|)
# A stored window score adds the combination of the four wave slots: 4 roundings on values bounded by sum|w|.
# An output r' (A - R) + (r' - r) T holds m local scores -- |A| + |R| <= 2 min(conv_width, nk) - 1 for a deletion,
# <= 2 min(conv_width, nk + 1) - 1 for an insertion, hence <= 2 conv_width - 1 -- added and subtracted in float64 (m + 2 roundings on
# values bounded by m sum|w|), times r'; the T term holds nk scores (nk + 2 roundings on values bounded by nk sum|w|) times |r' - r|,
# zero at scaling 0; the normalisers (a square root, a division, a difference), the two products and the final sum are 6 more roundings
# on values bounded by |r'| m sum|w| + |r' - r| nk sum|w|.  Maximum over the sequences (r, r' and m depend on the length).
# ------------------------------------------------------------------------------------------------------------------
def _score_bound(table_scaled_f32, w, chi, conv_width, intercept):
    tab = np.asarray(table_scaled_f32, dtype=np.float32)
    F, P = chi.shape[0], dr.padded_width(conv_width * tab.shape[1])
    w = np.abs(np.asarray(w, dtype=np.float64))
    sw = float(w[1:].sum() if intercept else w.sum())
    norm = float(np.sqrt(conv_width) * dr.max_row_norm(tab))
    cap1 = dr.cap_features(np.float32, P, norm, float(np.abs(chi).max()), 1.0, nk=1)
    return sw * (cap1 + (2 * F + 1) * U64), sw


def cap_window_scores(table_scaled_f32, w, chi, conv_width, intercept):
    score, sw = _score_bound(table_scaled_f32, w, chi, conv_width, intercept)
    return score + 4 * U64 * sw


def cap_indel_scan(table_scaled_f32, seqlen, w, chi, conv_width, scaling, intercept):
    """-> (cap of the deletions, cap of the insertions); the deletions of a sequence with s == conv_width are NaN and carry no cap."""
    score, sw = _score_bound(table_scaled_f32, w, chi, conv_width, intercept)
    score += 4 * U64 * sw                                                   # (R and T read stored scores)
    F = chi.shape[0]
    best = [0.0, 0.0]
    for s in sorted({int(v) for v in seqlen}):
        nk = s - conv_width + 1
        r = float(_r(F, nk, scaling))
        for which, km in ((0, nk - 1), (1, nk + 1)):
            if km < 1:
                continue
            rm = float(_r(F, km, scaling))
            m = 2 * min(conv_width, nk + which) - 1
            local = rm * (m * score + (m + 2) * U64 * m * sw)
            total = abs(rm - r) * (nk * score + (nk + 2) * U64 * nk * sw)
            best[which] = max(best[which], local + total + 6 * U64 * (rm * m + abs(rm - r) * nk) * sw)
    return best[0], best[1]


def zero_mask(seqlen, L, gaps=False):
    """[n, L] (deletions, window scores of full-width) or [n, L + 1] (gaps): True where the contract says exactly 0."""
    seqlen = np.asarray(seqlen, dtype=np.int64)
    return np.arange(L + 1 if gaps else L)[None, :] >= (seqlen[:, None] + (1 if gaps else 0))


def check(got, ref, cap, zeros=None):
    """The comparison of the GPU test: no element excused.  NaN exactly where the reference has NaN and nowhere else; bitwise +0.0
    where ``zeros`` (a mask over the leading axes) is set; everything else finite and within ``cap``.  -> the largest |got - ref|."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    nan = np.isnan(np.asarray(ref, dtype=np.float64))
    assert np.array_equal(np.isnan(got), nan), "NaN positions differ"
    assert np.isfinite(got[~nan]).all()
    if zeros is not None:
        z = got[zeros]
        assert (z == 0).all() and not np.signbit(z).any(), "a contract zero is not +0.0"
        assert (np.asarray(ref)[zeros] == 0).all()
    err = float(np.abs(got.astype(LD) - ref)[~nan].max()) if (~nan).any() else 0.0
    assert err <= cap, (err, cap)
    return err


@functools.lru_cache(maxsize=None)
def reference(name):
    """(operands, conv_width, scaling, intercept, scores, del, ins, cap_scores, cap_del, cap_ins) of a case: computed once, shared
    by the tests of a process, left unchanged."""
    c, cw, scaling, icpt = case(name)
    a = (c["tokens"], c["table"], c["seqlen"], c["w"], c["radem"], c["chi"], cw)
    scorer = _Scorer(c["table"], c["w"], c["radem"], c["chi"], cw, icpt)
    sc = window_scores(*a, icpt, scorer=scorer)
    dele, ins = indel_scan(*a, scaling, icpt, scorer=scorer)
    cd, ci = cap_indel_scan(c["table"], c["seqlen"], c["w"], c["chi"], cw, scaling, icpt)
    for arr in (sc, dele, ins):
        arr.setflags(write=False)
    return c, cw, scaling, icpt, sc, dele, ins, cap_window_scores(c["table"], c["w"], c["chi"], cw, icpt), cd, ci
