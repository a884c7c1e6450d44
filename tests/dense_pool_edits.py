"""The index algebra of the two-layer kernel's single-edit pool (xgpr_amd/csrc/pool_edits.inc) as a numpy model, and
brute force over written-out mutants to hold it to.  A plain helper module (not a conftest).

The window function is arbitrary and deterministic -- integer-valued, from a hash of the window's tokens and the filter index --, so
every comparison is exact: what is checked is WHICH windows enter a mutant's maximum, not how a window is transformed.

    PM[j] = max(0, p_0 .. p_{j-1})      SM[j] = max(0, p_j .. p_{nk-1})      row = max(PM[a], SM[b], the mutant's new windows)

``MISTAKES`` are planted index errors ``edit_rows`` can be asked to make; tests/test_pool_edits_host.py asserts that the comparison
with brute force catches each of them."""
import numpy as np

MODES = ("substitutions", "deletions", "insertions")
MISTAKES = ("jhi_off_by_one", "b_off_by_one", "ins_removed_at_g0", "ins_removed_at_gs", "del_nk1")


def window_values(win, F):
    """[F] float64, integers in [-50, 50]: the "projections" of one window (a sequence of tokens)."""
    h = 1469598103934665603
    for k, t in enumerate(win):
        h = ((h ^ ((int(t) + 1) * (k + 3))) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    f = np.arange(F, dtype=np.uint64)
    mixed = (np.full(F, h, dtype=np.uint64) + f * np.uint64(40503)) * np.uint64(2654435761)      # (uint64 arrays wrap)
    return ((mixed >> np.uint64(17)) % np.uint64(101)).astype(np.float64) - 50.0


def pooled(seq, cw, F):
    """max(0, max over the windows of ``seq``); all NaN for a sequence shorter than one window."""
    nk = len(seq) - cw + 1
    if nk < 1:
        return np.full(F, np.nan)
    row = np.zeros(F)
    for j in range(nk):
        row = np.maximum(row, window_values(seq[j:j + cw], F))
    return row


def mutant(seq, mode, site, v):
    seq = list(seq)
    if mode == "substitutions":
        return seq[:site] + [v] + seq[site + 1:]
    if mode == "deletions":
        return seq[:site] + seq[site + 1:]
    return seq[:site] + [v] + seq[site:]


def geometry(L, V, mode):
    """-> (slots per sequence, values per slot)"""
    return (L + 1 if mode == "insertions" else L), (1 if mode == "deletions" else V)


def brute(tokens, s, cw, V, F, mode):
    """[slots, values, F]: every mutant written out and pooled; zero rows past the sequence."""
    L = len(tokens)
    slots, per = geometry(L, V, mode)
    out = np.zeros((slots, per, F))
    seq = list(tokens[:s])
    for site in range(slots):
        if site > s or (mode != "insertions" and site >= s):
            continue
        for v in range(per):
            out[site, v] = pooled(mutant(seq, mode, site, v), cw, F)
    return out


def tables(tokens, s, cw, F):
    """PM, SM [nk + 1, F]"""
    nk = s - cw + 1
    p = np.stack([window_values(tokens[j:j + cw], F) for j in range(nk)])
    pm, sm = np.zeros((nk + 1, F)), np.zeros((nk + 1, F))
    for j in range(nk):
        pm[j + 1] = np.maximum(pm[j], p[j])
    for j in range(nk - 1, -1, -1):
        sm[j] = np.maximum(sm[j + 1], p[j])
    return pm, sm


def edit_ranges(mode, site, s, cw, mistake=None):
    """-> (jlo, jhi, a, b): the mutant's new windows [jlo, jhi] and the rows of PM and SM, as the kernel computes them."""
    nk = s - cw + 1
    jlo = max(0, site - cw + 1)
    if mode == "substitutions":
        jhi = min(site, nk - 1)
        b = jhi + 1
    elif mode == "deletions":
        jhi = min(site - 1, nk - 2)
        b = min(site, nk - 1) + 1
    else:
        jhi = min(site, nk)
        b = min(site - 1, nk - 1) + 1
        if mistake == "ins_removed_at_g0" and site == 0:
            b = 1                                        # takes window 0 for straddled: nothing straddles the gap in front
        if mistake == "ins_removed_at_gs" and site == s:
            jhi = min(site, nk - 1)                      # the append treated like a gap inside: the mutant's one more window is lost
    a = jlo
    if mistake == "jhi_off_by_one":
        jhi -= 1                                         # the last covering window is left as it was
    if mistake == "b_off_by_one":
        b += 1                                           # drops the first window right of the edit
    return jlo, jhi, a, min(b, nk)


def edit_rows(tokens, s, cw, V, F, mode, mistake=None):
    """[slots, values, F] through the identity: two table rows and the mutant's new windows."""
    L = len(tokens)
    slots, per = geometry(L, V, mode)
    out = np.zeros((slots, per, F))
    seq = list(tokens[:s])
    nk = s - cw + 1
    pm, sm = tables(seq, s, cw, F)
    for site in range(slots):
        if site > s or (mode != "insertions" and site >= s):
            continue
        if mode == "deletions" and nk == 1 and mistake != "del_nk1":
            out[site] = np.nan
            continue
        jlo, jhi, a, b = edit_ranges(mode, site, s, cw, mistake)
        for v in range(per):
            mut = mutant(seq, mode, site, v)
            row = np.maximum(pm[a], sm[b])
            for j in range(jlo, jhi + 1):
                row = np.maximum(row, window_values(mut[j:j + cw], F))
            out[site, v] = row
    return out


def same(a, b):
    """Equal as real numbers, NaN in the same places."""
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def make_tokens(L, V, seed):
    return np.random.default_rng(seed).integers(0, V, size=L).tolist()
