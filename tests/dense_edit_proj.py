"""Dense-matrix reference of the single-edit PROJECTION of the sequence / graph kernels (xgpr_conv_token_subst_proj_f32,
xgpr_conv_token_indel_proj_f32) -- TEST HELPER, numpy only, in ``np.longdouble``, built from tests/dense_subst_var_scan.py and
tests/dense_indel_var_scan.py (their operand sets, ``_phi``, ``_times``, ``exact_rows``, ``_Windows``) with the SAME delta; nothing shared
with oracle/.

Definition (notation of those two files; the first nvar feature columns only; pm [nvar, K]):

    sub[i, l, v, :] = z(t with token l replaced by v)^T pm                       l < s;  0 beyond
    del[i, p, :]    = z(t without position p)^T pm                               p < s;  0 beyond;  NaN where s == conv_width
    ins[i, g, v, :] = z(t with token v inserted before g)^T pm                   g <= s; 0 beyond

``subst_proj`` / ``indel_proj`` with ``direct=True`` form the mutant's columns z' and multiply (the indels by BRUTE FORCE over all the
windows of the written-out mutant, with its own normaliser); by default they evaluate the contract's form (include/xgpr_hip/edit_proj.h),
what the kernels implement:   out = b~ + r' (delta pm),   b~ = (rho z_i + (1 - rho) e0)^T pm   (rho = 1, r' = r for a substitution).
``mistake=`` plants ONE structural error in that form (sensitivity test only):
    "pm_transposed"   delta pm^T (square pm)
    "r_dropped"       out = b~ + delta pm
    "keep_col0"       column 0 of delta moves under the intercept
    "no_rescale"      indels: b~ = z_i^T pm, the sequence's columns are not rescaled
    "old_norm"        indels: the sequence's own normaliser r(nk) on delta
"""
import functools

import numpy as np

import dense_indel_scan as dis
import dense_indel_var_scan as div
import dense_reference as dr
import dense_subst_var_scan as dv
from dense_reference import LD, U64

SUBST_MISTAKES = ("pm_transposed", "r_dropped", "keep_col0")
INDEL_MISTAKES = ("pm_transposed", "r_dropped", "keep_col0", "no_rescale", "old_norm")


def subst_delta(c, nvar, conv_width, scaling, intercept, keep_col0=False):
    """-> (delta [n, L, V, nvar], r [n]) longdouble: the delta of dense_subst_var_scan.var_scan."""
    tab = np.asarray(c["table"], dtype=LD)
    tokens, seqlen, radem = c["tokens"], c["seqlen"], c["radem"]
    chi = c["chi"][:nvar // 2]
    V, C = tab.shape
    n, L = tokens.shape
    cw, F = conv_width, c["chi"].shape[0]
    slots = np.zeros((cw, V, cw * C), dtype=LD)
    for q in range(cw):
        slots[q, :, q * C:(q + 1) * C] = tab
    S = dr.projections(slots.reshape(cw * V, cw * C), radem, chi).reshape(cw, V, nvar // 2)
    delta = np.zeros((n, L, V, nvar), dtype=LD)
    rr = np.zeros(n, dtype=LD)
    for i in range(n):
        s = int(seqlen[i])
        nk = s - cw + 1
        t = np.asarray(tokens[i, :s], dtype=np.int64)
        p = dr.projections(dr._windows(tab[t], s, cw), radem, chi)
        base = dv._phi(p, nvar)
        rr[i] = dr.conv_row_scale(F, nk, scaling)
        for l in range(s):
            for j in range(max(0, l - cw + 1), min(l, nk - 1) + 1):
                q = l - j
                delta[i, l] += dv._phi(p[j][None, :] + S[q] - S[q, t[l]][None, :], nvar) - base[j][None, :]
        if intercept and not keep_col0:
            delta[i, :, :, 0] = 0
    return delta, rr


def subst_proj(c, pm, conv_width, scaling, intercept, mistake=None, direct=False, z=None):
    """-> (out [n, L, V, K], b [n, K]) longdouble; ``z``: the sequences' columns behind b (default: exact)."""
    pm = np.asarray(pm, dtype=LD)
    nvar, K = pm.shape
    n, L = c["tokens"].shape
    V = c["table"].shape[0]
    z = np.asarray(dv.exact_rows(c, nvar, conv_width, scaling, intercept) if z is None else z, dtype=LD)
    delta, rr = subst_delta(c, nvar, conv_width, scaling, intercept, keep_col0=mistake == "keep_col0")
    b = z @ pm
    r = rr[:, None, None, None]
    if direct:
        out = dv._times((z[:, None, None, :] + r * delta).reshape(n * L * V, nvar), pm).reshape(n, L, V, K)
    else:
        y = dv._times(delta.reshape(n * L * V, nvar), pm.T if mistake == "pm_transposed" else pm).reshape(n, L, V, K)
        out = b[:, None, None, :] + (1 if mistake == "r_dropped" else r) * y
    out[np.arange(L)[None, :] >= np.asarray(c["seqlen"])[:, None]] = 0
    return out, b


def indel_deltas(c, nvar, conv_width, intercept, keep_col0=False):
    """Per sequence (delta_del [s, nvar] or None where s == conv_width, delta_ins [(s + 1) V, nvar]) longdouble: the delta of
    dense_indel_var_scan.decomposed."""
    cw = conv_width
    W = div._Windows(c, nvar, cw)
    V = c["table"].shape[0]
    k = np.arange(cw)
    out = []
    for i in range(c["tokens"].shape[0]):
        s = int(c["seqlen"][i])
        nk = s - cw + 1
        t = np.asarray(c["tokens"][i, :s], dtype=np.int64)
        own = W.phi(np.lib.stride_tricks.sliding_window_view(t, cw))
        dd = None
        if nk > 1:
            dd = np.zeros((s, nvar), dtype=LD)
            for p in range(s):
                lo, hi = max(0, p - cw + 1), min(p - 1, nk - 2)
                for j in range(lo, hi + 1):
                    dd[p] += W.phi(t[j + k + (k >= p - j)])[0]
                dd[p] -= own[lo:min(p, nk - 1) + 1].sum(axis=0)
        di = np.zeros((s + 1, V, nvar), dtype=LD)
        for g in range(s + 1):
            lo = max(0, g - cw + 1)
            R = own[lo:min(g - 1, nk - 1) + 1].sum(axis=0)
            for v in range(V):
                for j in range(lo, min(g, nk) + 1):
                    q = g - j
                    di[g, v] += W.phi(np.concatenate([t[j:j + q], [v], t[j + q:j + cw - 1]]))[0]
                di[g, v] -= R
        di = di.reshape((s + 1) * V, nvar)
        if intercept and not keep_col0:
            di[:, 0] = 0
            if dd is not None:
                dd[:, 0] = 0
        out.append((dd, di))
    return out


def indel_base(c, pm, conv_width, scaling, intercept, z=None, mistake=None):
    """b~ = (rho z_i + (1 - rho) e0)^T pm per row set -> (b_del [n, K], b_ins [n, K]) longdouble; rho = 1 for the deletions of a
    sequence with s == conv_width (no mutant), as dense_indel_var_scan.operands."""
    pm = np.asarray(pm, dtype=LD)
    nvar, cw, F = pm.shape[0], conv_width, c["chi"].shape[0]
    z = np.asarray(dv.exact_rows(c, nvar, cw, scaling, intercept) if z is None else z, dtype=LD)
    nk = np.asarray(c["seqlen"], dtype=np.int64) - cw + 1
    out = []
    for nkm in (np.maximum(nk - 1, 1), nk + 1):
        rho = np.asarray([dis._r(F, int(b), scaling) / dis._r(F, int(a), scaling) for a, b in zip(nk, nkm)], dtype=LD)
        if mistake == "no_rescale":
            rho = np.ones_like(rho)
        b = z * rho[:, None]
        if intercept:
            b[:, 0] = 1
        out.append(b @ pm)
    return out[0], out[1]


def indel_proj(c, pm, conv_width, scaling, intercept, mistake=None, direct=False, z=None):
    """-> (del [n, L, K], ins [n, L + 1, V, K], b_del [n, K], b_ins [n, K]) longdouble."""
    pm = np.asarray(pm, dtype=LD)
    nvar, K = pm.shape
    cw, F = conv_width, c["chi"].shape[0]
    n, L = c["tokens"].shape
    V = c["table"].shape[0]
    b_del, b_ins = indel_base(c, pm, cw, scaling, intercept, z=z, mistake=mistake)
    dele = np.zeros((n, L, K), dtype=LD)
    ins = np.zeros((n, L + 1, V, K), dtype=LD)
    if direct:
        W = div._Windows(c, nvar, cw)

        def zrow(t):
            row = dis._r(F, len(t) - cw + 1, scaling) * W.total(t)
            if intercept:
                row[0] = 1
            return row

        for i in range(n):
            s = int(c["seqlen"][i])
            t = [int(v) for v in c["tokens"][i, :s]]
            if s == cw:
                dele[i, :s] = LD("nan")
            else:
                dele[i, :s] = dv._times(np.stack([zrow(t[:p] + t[p + 1:]) for p in range(s)]), pm)
            rows = np.stack([zrow(t[:g] + [v] + t[g:]) for g in range(s + 1) for v in range(V)])
            ins[i, :s + 1] = dv._times(rows, pm).reshape(s + 1, V, K)
        return dele, ins, b_del, b_ins
    mat = pm.T if mistake == "pm_transposed" else pm
    deltas = indel_deltas(c, nvar, cw, intercept, keep_col0=mistake == "keep_col0")
    for i in range(n):
        s = int(c["seqlen"][i])
        nk = s - cw + 1
        dd, di = deltas[i]
        r = dis._r(F, nk, scaling)
        for which, d in ((0, dd), (1, di)):
            if d is None:
                dele[i, :s] = LD("nan")
                continue
            rm = r if mistake == "old_norm" else dis._r(F, nk + (1 if which else -1), scaling)
            y = (b_ins if which else b_del)[i][None, :] + (1 if mistake == "r_dropped" else rm) * dv._times(d, mat)
            if which:
                ins[i, :s + 1] = y.reshape(s + 1, V, K)
            else:
                dele[i, :s] = y
    return dele, ins, b_del, b_ins


# ------------------------------------------------------------------------------------------------------------------
# A-priori cap: derived, not tuned -- the LINEAR term of dense_subst_var_scan.cap_var_scan with u replaced by a column of pm and without
# the factor 2.  Each cos / sin value of a variant window is within  cap1 = cap_features(float32, P, norm, |chi|max, c = 1, nk = 1)  of
# exact; an entry of delta adds m values (substitution: m = 2 min(conv_width, nk); deletion: 2 min(conv_width, nk) - 1; insertion:
# 2 min(conv_width, nk + 1) - 1, as dense_indel_var_scan.cap_var_scan counts them) in float64 and subtracts once,
#     eps = m cap1 + (m + 1) m u64,          |delta|_inf <= m.
# Column k of out = b + r' (delta . pm[:, k]):  the value errors give  r' eps |pm[:, k]|_1;  the nvar-term float64 sum of terms bounded by
# m |pm|  (nvar + 1) u64 r' m |pm[:, k]|_1;  forming r', the product and the sum -- 3 roundings on values bounded by |b| + r' m |pm[:, k]|_1;
# b enters rounded to float64: u64 |b|.  Under the intercept column 0 of delta is exactly zero and the 1-norm leaves row 0 of pm out.
# Where the test feeds the operator a b formed from float32 feature ROWS (``carried``: the kernel-object route) each column of z is
# within  cz = cap_features(float32, P, norm, chimax, r, nk, u_out = u32)  of exact and rho -- a float64 division and square root on the
# host -- within 3 u64 rho, so b's columns are within cb = rho (cz + 3 u64 zmax) and b~[k] within cb |pm[:, k]|_1 (ALL rows: column 0 of z
# is exact under the intercept, which only helps).  One cap per sequence and column.
# ------------------------------------------------------------------------------------------------------------------
def _cap(c, pm, b, conv_width, scaling, intercept, which, carried=False, z=None):
    """which: None substitutions, 0 deletions, 1 insertions -> cap [n, K] float64 (0 where the sequence has no such mutant)."""
    tab = np.asarray(c["table"], dtype=np.float32)
    chi = c["chi"]
    F, P = chi.shape[0], dr.padded_width(conv_width * tab.shape[1])
    pa = np.abs(np.asarray(pm, dtype=np.float64))
    nvar = pa.shape[0]
    p1 = (pa[1:] if intercept else pa).sum(axis=0)
    norm = float(np.sqrt(conv_width) * dr.max_row_norm(tab))
    chimax = float(np.abs(chi).max())
    cap1 = dr.cap_features(np.float32, P, norm, chimax, 1.0, nk=1)
    out = np.zeros((len(c["seqlen"]), pa.shape[1]))
    for i, s in enumerate(int(v) for v in c["seqlen"]):
        nk = s - conv_width + 1
        km = nk if which is None else nk + (1 if which else -1)
        if km < 1:
            continue
        m = 2 * min(conv_width, nk) if which is None else 2 * min(conv_width, nk + which) - 1
        r = float(dis._r(F, km, scaling))
        eps = m * cap1 + (m + 1) * m * U64
        bi = np.abs(np.asarray(b[i], dtype=np.float64))
        out[i] = r * eps * p1 + (nvar + 1) * U64 * r * m * p1 + 3 * U64 * (bi + r * m * p1) + U64 * bi
        if carried:
            r0 = float(dis._r(F, nk, scaling))
            cz = dr.cap_features(np.float32, P, norm, chimax, r0, nk=nk, u_out=dr.U32)
            zmax = float(np.abs(np.asarray(z[i], dtype=np.float64)).max())
            out[i] += (r / r0) * (cz + 3 * U64 * zmax) * pa.sum(axis=0)
    return out


def cap_subst(c, pm, b, conv_width, scaling, intercept, carried=False, z=None):
    return _cap(c, pm, b, conv_width, scaling, intercept, None, carried, z)


def cap_indel(c, pm, b_del, b_ins, conv_width, scaling, intercept, carried=False, z=None):
    return (_cap(c, pm, b_del, conv_width, scaling, intercept, 0, carried, z),
            _cap(c, pm, b_ins, conv_width, scaling, intercept, 1, carried, z))


# The written-out route (``*_projection_scan_composed``): every column of a mutant's float32 feature row is within
# cz = cap_features(float32, P, norm, chimax, r', nk', u_out = u32)  of exact and bounded by zb = max(r' nk', 1 under the intercept); its
# product with column k of pm in float64 errs by  cz |pm[:, k]|_1  plus the rounding of its nvar terms, (nvar + 1) u64 zb |pm[:, k]|_1.
def cap_written_out(c, pm, conv_width, scaling, intercept, which):
    """which as for ``_cap`` -> cap [K]: the maximum over the sequences' mutants."""
    tab = np.asarray(c["table"], dtype=np.float32)
    chi = c["chi"]
    F, P = chi.shape[0], dr.padded_width(conv_width * tab.shape[1])
    pa = np.abs(np.asarray(pm, dtype=np.float64)).sum(axis=0)
    nvar = np.asarray(pm).shape[0]
    norm = float(np.sqrt(conv_width) * dr.max_row_norm(tab))
    best = np.zeros(pa.shape[0])
    for s in sorted({int(v) for v in c["seqlen"]}):
        km = s - conv_width + 1 + (0 if which is None else (1 if which else -1))
        if km < 1:
            continue
        r = float(dis._r(F, km, scaling))
        cz = dr.cap_features(np.float32, P, norm, float(np.abs(chi).max()), r, nk=km, u_out=dr.U32)
        zb = max(r * km, 1.0 if intercept else 0.0)
        best = np.maximum(best, cz * pa + (nvar + 1) * U64 * zb * pa)
    return best


def check(got, ref, cap, zeros):
    """The comparison of the GPU test, no element excused: ``cap`` [n, K] per sequence and column.  NaN exactly where the reference
    has NaN, bitwise +0.0 in the slots of ``zeros`` ([n, slots]: dense_indel_scan.zero_mask), the rest finite and within cap.
    -> (largest |got - ref|, largest |got - ref| / cap)."""
    got = np.ascontiguousarray(got, dtype=np.float64)
    ref = np.asarray(ref)
    cap = np.asarray(cap).reshape((ref.shape[0],) + (1,) * (ref.ndim - 2) + (ref.shape[-1],))
    nan = np.isnan(np.asarray(ref, dtype=np.float64))
    assert np.array_equal(np.isnan(got), nan), "NaN pattern differs"
    dead = np.broadcast_to(np.asarray(zeros).reshape(zeros.shape + (1,) * (ref.ndim - 2)), ref.shape)
    assert not np.any(got.view(np.uint64)[dead]), "a dead row is not all +0.0"
    live = ~nan & ~dead
    assert np.isfinite(got[live]).all()
    err = np.abs(np.asarray(got, dtype=LD) - ref)
    capb = np.broadcast_to(cap, ref.shape)
    bad = live & (err > capb)
    assert not bad.any(), f"{int(bad.sum())} elements beyond the cap, worst {float((err[live] / np.maximum(capb[live], 1e-300)).max()):.3g} x"
    if not live.any():
        return 0.0, 0.0
    return float(err[live].max()), float((err[live] / np.maximum(capb[live], 1e-300)).max())


def factor_of(vm):
    """The Cholesky factor of a case's own vm (float64): pm with pm pm^T = vm."""
    return np.linalg.cholesky(np.asarray(vm, dtype=np.float64))


@functools.lru_cache(maxsize=None)
def subst_case(name):
    """dense_subst_var_scan.case(name) with pm = chol(vm), the reference, the exact b rounded to float64 and the cap [n, K]: computed
    once per process and shared; nothing in it is written to."""
    k = dict(dv.case(name))
    pm = factor_of(k["vm"])
    out, b = subst_proj(k["c"], pm, k["cw"], k["scaling"], k["icpt"], z=k["z"])
    b64 = np.ascontiguousarray(np.asarray(b, dtype=np.float64))
    k.update(pm=pm, ref=out, b=b, b64=b64, cap=cap_subst(k["c"], pm, b64, k["cw"], k["scaling"], k["icpt"]))
    out.setflags(write=False)
    return k


@functools.lru_cache(maxsize=None)
def indel_case(name):
    """dense_indel_var_scan.case(name) with pm = chol(vm), the references, the exact b~ rounded to float64 and the caps [n, K]."""
    k = dict(div.case(name))
    pm = factor_of(k["vm"])
    dele, ins, bd, bi = indel_proj(k["c"], pm, k["cw"], k["scaling"], k["icpt"], z=k["ops"]["z"])
    bd64, bi64 = (np.ascontiguousarray(np.asarray(x, dtype=np.float64)) for x in (bd, bi))
    cd, ci = cap_indel(k["c"], pm, bd64, bi64, k["cw"], k["scaling"], k["icpt"])
    k.update(pm=pm, ref_del=dele, ref_ins=ins, b_del=bd64, b_ins=bi64, cap_del=cd, cap_ins=ci)
    for arr in (dele, ins):
        arr.setflags(write=False)
    return k
