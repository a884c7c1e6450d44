"""Dense reference of the combinatorial site scan of the sequence / graph kernels (xgpr_conv_token_site_scan_f32) -- TEST HELPER,
numpy only, in ``np.longdouble``, from tests/dense_reference.py's ``projections`` and the operand sets of tests/dense_subst_scan.py
(``make_case``); nothing shared with oracle/.

Definition (notation of tests/dense_subst_scan.py: table[V, C] ALREADY multiplied by sigma, tokens t[0 .. s), nk = s - conv_width + 1
windows, c(win) the window score, r = sqrt(1 / F) / {1, sqrt(nk), nk}[scaling]).  For sites p_0 < ... < p_{K-1} and EVERY assignment
A in [0, V)^K, at flat index sum_k A_k V^(K-1-k):

    full[i, A] = r sum_{j < nk} [ c(window j of t[p_k := A_k for all k]) - c(window j of t) ]

``full_scan`` forms exactly that and DOES NOT GO THROUGH RUNS: every variant is written out as tokens, cut into its nk windows, the
distinct token windows are projected once each (a window's score depends on its tokens alone), and a variant's windows are
subtracted from the parent's one by one -- a window no site touches is the parent's own and gives an exact zero.

``run_tables`` is the decomposition under test, in long double: ``site_runs`` (the Python mirror of
xgpr_conv_token_site_scan_layout) and, per run with windows j_lo .. j_hi and sites p_a .. p_{a+g-1}, the table [V^g]

    table[i][rho][idx] = r sum_{j = j_lo .. min(j_hi, nk - 1)} [ c(win_j with a_m at p_{a+m}, all m) - c(win_j) ],  idx = sum_m a_m V^(g-1-m)

and ``gather_full`` sums one entry per run for every assignment.  tests/test_site_scan_host.py holds the two together.

``mistake=`` plants ONE structural error into ``run_tables`` (sensitivity test only):
    "run_boundary"   every run's last window dropped where it has more than one, its first window taken twice otherwise
    "swapped_sites"  the tokens of a run's first two sites placed at each other's positions
    "truncate_at_L"  a run's windows cut at the array's last window instead of the sequence's
    "keep_w0"        w[0] kept under the intercept
    "no_parent"      the parent's window scores not subtracted
    "strides"        the entry of (a_0 .. a_{g-1}) stored at sum_m a_m V^m
"""
import itertools

import numpy as np

import dense_reference as dr
import dense_subst_scan as dss
from dense_reference import LD, U64

MISTAKES = ("run_boundary", "swapped_sites", "truncate_at_L", "keep_w0", "no_parent", "strides")


def site_runs(sites, L, cw):
    """-> list of (first_window, last_window, first_site, count) in ascending window order: window j covers the sites in
    [j, j + cw); consecutive windows with the same covered set form one run; windows that cover none form none."""
    runs = []
    for j in range(L - cw + 1):
        cov = [k for k, p in enumerate(sites) if j <= p <= j + cw - 1]
        if not cov:
            continue
        key = (cov[0], len(cov))
        if runs and runs[-1][1] == j - 1 and (runs[-1][2], runs[-1][3]) == key:
            runs[-1] = (runs[-1][0], j, key[0], key[1])
        else:
            runs.append((j, j, key[0], key[1]))
    return runs


def run_offsets(runs, V):
    """-> (offset of every run in a row of the operator's output, the row's length T)."""
    offs, T = [], 0
    for _, _, _, g in runs:
        offs.append(T)
        T += V ** g
    return offs, T


def assignments(V, K):
    """[V^K, K] int64, row = flat index: the first site most significant."""
    return np.asarray(list(itertools.product(range(V), repeat=K)), dtype=np.int64).reshape(V ** K, K)


def _weights(w, intercept, mistake):
    w = np.array(w, dtype=LD)
    if intercept and mistake != "keep_w0":
        w[0] = 0
    return w[0::2], w[1::2]


def _window_scores(token_windows, tab, radem, chi, wc, ws):
    """The score of every token window [m, cw] -> [m] long double; distinct windows are projected once."""
    uniq, inv = np.unique(token_windows, axis=0, return_inverse=True)
    x = tab[uniq].reshape(uniq.shape[0], -1)
    sc = np.zeros(uniq.shape[0], dtype=LD)
    for lo in range(0, uniq.shape[0], 4096):
        sc[lo:lo + 4096] = dss._score(dr.projections(x[lo:lo + 4096], radem, chi), wc, ws)
    return sc[np.asarray(inv).reshape(-1)]


def full_scan(tokens, table_scaled, seqlen, w, radem, chi, sites, conv_width, scaling, intercept):
    """-> [n, V^K] longdouble, from the definition (see the module docstring)."""
    tab = np.asarray(table_scaled, dtype=LD)
    V, cw, F, K = tab.shape[0], conv_width, chi.shape[0], len(sites)
    n = tokens.shape[0]
    wc, ws = _weights(w, intercept, None)
    A = assignments(V, K)
    out = np.zeros((n, V ** K), dtype=LD)
    for i in range(n):
        s = int(seqlen[i])
        nk = s - cw + 1
        t = np.asarray(tokens[i, :s], dtype=np.int64)
        var = np.repeat(t[None, :], V ** K, axis=0)
        var[:, list(sites)] = A                                              # every variant written out
        wins = np.lib.stride_tricks.sliding_window_view(var, cw, axis=1)     # [V^K, nk, cw]
        sc = _window_scores(np.concatenate([wins.reshape(-1, cw), np.lib.stride_tricks.sliding_window_view(t, cw)]), tab, radem, chi, wc, ws)
        parent = sc[V ** K * nk:]                                            # [nk]
        r = np.sqrt(LD(1) / LD(F)) / dss._normaliser(nk, scaling)
        out[i] = r * (sc[:V ** K * nk].reshape(V ** K, nk) - parent[None, :]).sum(axis=1)
    return out


def run_tables(tokens, table_scaled, seqlen, w, radem, chi, sites, conv_width, scaling, intercept, mistake=None):
    """-> (runs, tables): tables[q] [n, V^g] longdouble, the layout of the operator's output (see the module docstring)."""
    tab = np.asarray(table_scaled, dtype=LD)
    V, cw, F = tab.shape[0], conv_width, chi.shape[0]
    n, L = tokens.shape
    wc, ws = _weights(w, intercept, mistake)
    runs = site_runs(sites, L, cw)
    tables = []
    for jlo, jhi, a, g in runs:
        A = assignments(V, g)
        pos = [sites[a + m] for m in range(g)]
        if mistake == "swapped_sites" and g > 1:
            pos[0], pos[1] = pos[1], pos[0]
        tb = np.zeros((n, V ** g), dtype=LD)
        for i in range(n):
            s = int(seqlen[i])
            nk = s - cw + 1
            t = np.asarray(tokens[i], dtype=np.int64) % V                    # (positions past the length: read by "truncate_at_L" alone)
            last = min(jhi, (L - cw) if mistake == "truncate_at_L" else nk - 1)
            js = list(range(jlo, last + 1))
            if mistake == "run_boundary" and js:
                js = js[:-1] if len(js) > 1 else js + js
            if not js:
                continue
            var = np.repeat(t[None, :], V ** g, axis=0)
            var[:, pos] = A
            wins = np.stack([var[:, j:j + cw] for j in js], axis=1)          # [V^g, |js|, cw]
            own = np.stack([t[j:j + cw] for j in js])
            sc = _window_scores(np.concatenate([wins.reshape(-1, cw), own]), tab, radem, chi, wc, ws)
            parent = sc[V ** g * len(js):]
            if mistake == "no_parent":
                parent = np.zeros_like(parent)
            r = np.sqrt(LD(1) / LD(F)) / dss._normaliser(nk, scaling)
            val = r * (sc[:V ** g * len(js)].reshape(V ** g, len(js)) - parent[None, :]).sum(axis=1)
            if mistake == "strides":
                val = val.reshape((V,) * g).transpose(tuple(reversed(range(g)))).reshape(-1)
            tb[i] = val
        tables.append(tb)
    return runs, tables


def gather_full(runs, tables, V, K):
    """[n, V^K]: for every assignment of the K sites the sum of one entry per run, in long double (or the tables' dtype widened)."""
    A = assignments(V, K)
    n = tables[0].shape[0]
    out = np.zeros((n, V ** K), dtype=LD)
    for (_, _, a, g), tb in zip(runs, tables):
        idx = np.zeros(V ** K, dtype=np.int64)
        for m in range(g):
            idx = idx * V + A[:, a + m]
        out += np.asarray(tb, dtype=LD)[:, idx]
    return out


# ------------------------------------------------------------------------------------------------------------------
# A-priori cap: derived, not tuned; the derivation of tests/dense_subst_scan.py carried to a run.  A variant window's cos / sin values
# are those of the float32 feature operators, each within cap1 = cap_features(float32, P, norm, |chi|max, c = 1, nk = 1) of exact
# (`norm`: sqrt(conv_width) times the largest row norm of the table bounds every variant window, whatever tokens it holds), so a
# window score errs by at most  score = sum|w| cap1 + (2 F + 1) u64 sum|w|.  An entry of a run with m windows inside the sequence is
# r (G - G_own): 2 m score errors; per G  m + 2 float64 roundings (into the wave slots, then the slots combined) on values bounded by
# m sum|w|; the subtraction and the product with r two more roundings of a value bounded by 2 m sum|w|.  A run's cap is the maximum
# over the sequences (r and m depend on the length); a full assignment adds one entry per run, so its cap is the sum of the runs' caps
# taken per sequence, again maximised over the sequences (the test adds the entries in long double: no further rounding).
# ------------------------------------------------------------------------------------------------------------------
def cap_site_scan(table_scaled_f32, seqlen, w, chi, sites, L, conv_width, scaling, intercept):
    """-> (cap of every run's table [nruns], cap of a full assignment)."""
    tab = np.asarray(table_scaled_f32, dtype=np.float32)
    F, P = chi.shape[0], dr.padded_width(conv_width * tab.shape[1])
    w = np.abs(np.asarray(w, dtype=np.float64))
    sw = float(w[1:].sum() if intercept else w.sum())
    norm = float(np.sqrt(conv_width) * dr.max_row_norm(tab))
    cap1 = dr.cap_features(np.float32, P, norm, float(np.abs(chi).max()), 1.0, nk=1)
    score = sw * (cap1 + (2 * F + 1) * U64)
    runs = site_runs(sites, L, conv_width)
    per_run, total = np.zeros(len(runs)), 0.0
    for s in sorted({int(v) for v in seqlen}):
        nk = s - conv_width + 1
        r = float(dr.conv_row_scale(F, nk, scaling))
        caps = []
        for jlo, jhi, _, _ in runs:
            m = max(0, min(jhi, nk - 1) - jlo + 1)
            caps.append(r * (2 * m * score + 2 * (m + 2) * U64 * m * sw + 2 * U64 * 2 * m * sw))
        per_run = np.maximum(per_run, caps)
        total = max(total, float(np.sum(caps)))
    return per_run, total


def check(got, ref, cap):
    """The comparison of the GPU test: no element excused.  -> the largest |got - ref|."""
    return dss.check(got, ref, cap)


# (name, make_case arguments, sites, scaling, intercept): the shapes of tests/test_gpu_site_scan.py, shared with the host test, which
# holds the reference alone to `cap <= 1e-2 max|full|` on every non-degenerate one of them.  Every site lies inside every sequence.
CASES = [
    # the non-TP path, g = 3; in the sequences of 5 and 6 tokens the later runs are truncated or have no window at all
    ("w16_c4_cw3", dict(n=3, L=9, C=4, V=6, conv_width=3, F=8, lengths=[9, 5, 6]), (2, 3, 4), 0, True),
    # first TP width; two tiles, the second ragged; position 0 and (in the sequence of 6) the last token, which has ONE window
    ("w128_c21_cw6", dict(n=2, L=14, C=21, V=21, conv_width=6, F=1030, onehot=True, lengths=[14, 6]), (0, 5), 2, True),
    ("w512_c60_cw8", dict(n=2, L=10, C=60, V=4, conv_width=8, F=600, lengths=[10, 8], extra_reps=2), (1, 4, 7), 2, False),   # packed registers
    ("w1024_c120_cw8", dict(n=2, L=11, C=120, V=4, conv_width=8, F=1030, lengths=[11, 9]), (0, 3, 8), 0, False),
    ("g4_cw9", dict(n=2, L=16, C=5, V=4, conv_width=9, F=300, lengths=[16, 12]), (3, 4, 6, 10), 1, True),                   # four sites in one window
    ("two_components", dict(n=2, L=20, C=6, V=3, conv_width=4, F=200, lengths=[20, 17]), (2, 3, 15, 16), 1, False),
    ("one_site", dict(n=3, L=10, C=21, V=21, conv_width=3, F=8, onehot=True), (2,), 1, False),                              # K = 1: the substitution scan
    ("vocab256_c5", dict(n=1, L=5, C=5, V=256, conv_width=3, F=40, lengths=[5]), (2, 3), 0, False),                         # two adjacent sites
    ("vocab1", dict(n=2, L=6, C=5, V=1, conv_width=2, F=70), (1,), 0, True),                                                # all zeros
    ("graph_cw1", dict(n=3, L=7, C=10, V=9, conv_width=1, F=300, lengths=[7, 4, 5]), (0, 2, 3), 1, True),                   # purely additive
    ("dup_rows", dict(n=2, L=8, C=6, V=5, conv_width=4, F=200, dup_rows=(1, 3)), (1, 2, 3), 1, True),                       # two identical rows
    ("n65", dict(n=65, L=6, C=4, V=3, conv_width=2, F=40), (0, 1), 2, True),
]
DEGENERATE = ("vocab1",)


def case(name):
    for nm, kw, sites, scaling, intercept in CASES:
        if nm == name:
            return dss.make_case(**kw), sites, kw["conv_width"], scaling, intercept
    raise KeyError(name)


def reference(name, mistake=None):
    """(operands, sites, conv_width, scaling, intercept, runs, tables, per-run caps, full-assignment cap) of a case."""
    c, sites, cw, scaling, icpt = case(name)
    runs, tables = run_tables(c["tokens"], c["table"], c["seqlen"], c["w"], c["radem"], c["chi"], sites, cw, scaling, icpt, mistake=mistake)
    caps, total = cap_site_scan(c["table"], c["seqlen"], c["w"], c["chi"], sites, c["tokens"].shape[1], cw, scaling, icpt)
    return c, sites, cw, scaling, icpt, runs, tables, caps, total


def full_reference(name):
    """[n, V^K] longdouble from the definition."""
    c, sites, cw, scaling, icpt = case(name)
    return full_scan(c["tokens"], c["table"], c["seqlen"], c["w"], c["radem"], c["chi"], sites, cw, scaling, icpt)
