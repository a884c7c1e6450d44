"""Dense-matrix reference of the substitution VARIANCE scan of the sequence / graph kernels (xgpr_conv_token_subst_var_scan_f32) --
TEST HELPER, numpy only, in ``np.longdouble``, built like tests/dense_subst_scan.py from tests/dense_reference.py's ``projections``
and ``_windows`` and the single-slot projections; nothing shared with oracle/.

Definition (notation of tests/dense_subst_scan.py; the first nvar feature columns only, column 2f = cos, 2f + 1 = sin):

    phi(win)[2f] = cos p_f,  phi(win)[2f + 1] = sin p_f                      (column 0 := 0 under the intercept)
    z_i          = r sum_{j < nk} phi(win_j)                                  (column 0 := 1 under the intercept)
    delta[i,l,v] = sum_{j in J(l)} phi(win_j with the token at offset l - j replaced by v)  -  sum_{j in J(l)} phi(win_j)
    z'           = z_i + r delta[i, l, v]
    Q[i, l, v]   = z'^T Vm z'                                                 for l < s, and 0 for l >= s

``var_scan`` forms z' and evaluates the quadratic form DIRECTLY; ``expansion=True`` evaluates the operator's three terms
q_i + 2 r delta . u_i + r^2 delta^T Vm delta instead (the host test holds the two together).

``mistake=`` plants ONE structural error (sensitivity test only):
    "no_cross"         the term 2 r delta . u dropped
    "r_once"           r in place of r^2 on the quadratic term
    "keep_col0"        column 0 moves under the intercept
    "first_window"     only the first covering window
    "vm_upper"         only the upper triangle of Vm is read
    "cos_sin_swapped"  delta's columns 2f and 2f + 1 exchanged
"""
import functools

import numpy as np

import dense_reference as dr
import dense_subst_scan as dss
from dense_reference import LD, U64

MISTAKES = ("no_cross", "r_once", "keep_col0", "first_window", "vm_upper", "cos_sin_swapped")


def _phi(p, nvar, swapped=False):
    """[..., nf] projections -> [..., nvar] columns (cos, sin interleaved)."""
    out = np.empty(p.shape[:-1] + (nvar,), dtype=LD)
    out[..., 1 if swapped else 0::2] = np.cos(p)
    out[..., 0 if swapped else 1::2] = np.sin(p)
    return out


def exact_rows(c, nvar, conv_width, scaling, intercept):
    """z [n, nvar] longdouble: the first nvar feature columns of the case's sequences."""
    tab = np.asarray(c["table"], dtype=LD)
    chi = c["chi"][:nvar // 2]
    F = c["chi"].shape[0]
    z = np.zeros((c["tokens"].shape[0], nvar), dtype=LD)
    for i, s in enumerate(int(v) for v in c["seqlen"]):
        t = np.asarray(c["tokens"][i, :s], dtype=np.int64)
        p = dr.projections(dr._windows(tab[t], s, conv_width), c["radem"], chi)
        z[i] = dr.conv_row_scale(F, s - conv_width + 1, scaling) * _phi(p, nvar).sum(axis=0)
        if intercept:
            z[i, 0] = 1
    return z


FIXED_FROM = 1024       # nvar from which ``_times`` takes the fixed-point route
_LIMB, _LIMBS = 20, 3    # 60 fractional bits: a truncation of 2^-61 of the operand's largest entry, the longdouble product's own order


def _limbs(x):
    """x (longdouble) -> (three float64 arrays of integers below 2^20 in modulus, scale): x ~ scale sum_k limb_k 2^(-20 (k + 1))."""
    x = np.asarray(x, dtype=LD)
    big = np.abs(x).max()
    scale = LD(2) ** int(np.ceil(np.log2(float(big)))) if big > 0 else LD(1)
    rest, out = x / scale, []                            # |rest| <= 1
    for _ in range(_LIMBS):
        rest = rest * LD(2 ** _LIMB)
        limb = np.rint(rest)
        out.append(np.asarray(limb, dtype=np.float64))
        rest = rest - limb                               # exact: |rest| <= 1/2
    return out, scale


def _times(a, b):
    """a @ b in longdouble.  From FIXED_FROM columns on, by fixed point: both operands are cut into three 20-bit limbs (integers held
    in float64), the nine limb products run as float64 matrix products -- EXACT: a product is below 2^40 and a sum of up to 2^12 of
    them below 2^53 -- and are recombined in longdouble.  Only the operands' truncation at 2^-60 of their largest entry is lost, the
    order of the rounding of the plain longdouble product (which takes 16 s at nvar = 2048); tests/test_subst_var_scan_host.py holds
    the two routes together."""
    if a.shape[1] < FIXED_FROM:
        return a @ b
    assert a.shape[1] <= 4096
    la, sa = _limbs(a)
    lb, sb = _limbs(b)
    out = np.zeros((a.shape[0], b.shape[1]), dtype=LD)
    for i in range(_LIMBS):
        for j in range(_LIMBS):
            out += np.asarray(la[i] @ lb[j], dtype=LD) * LD(2) ** (-_LIMB * (i + j + 2))
    return out * sa * sb


def var_scan(c, vm, conv_width, scaling, intercept, mistake=None, expansion=False):
    """-> (Q [n, L, V], q [n], u [n, nvar], z [n, nvar]) longdouble; ``c`` a dict of dense_subst_scan.make_case, ``vm`` [nvar, nvar]."""
    tab = np.asarray(c["table"], dtype=LD)
    tokens, seqlen, radem = c["tokens"], c["seqlen"], c["radem"]
    vm = np.asarray(vm, dtype=LD)
    nvar = vm.shape[0]
    chi = c["chi"][:nvar // 2]
    V, C = tab.shape
    n, L = tokens.shape
    cw, F = conv_width, c["chi"].shape[0]
    slots = np.zeros((cw, V, cw * C), dtype=LD)
    for q in range(cw):
        slots[q, :, q * C:(q + 1) * C] = tab
    S = dr.projections(slots.reshape(cw * V, cw * C), radem, chi).reshape(cw, V, nvar // 2)
    z = exact_rows(c, nvar, cw, scaling, intercept)
    u = z @ vm.T
    qq = (z * u).sum(axis=1)
    swapped = mistake == "cos_sin_swapped"
    delta = np.zeros((n, L, V, nvar), dtype=LD)
    rr = np.zeros(n, dtype=LD)
    for i in range(n):
        s = int(seqlen[i])
        nk = s - cw + 1
        t = np.asarray(tokens[i, :s], dtype=np.int64)
        p = dr.projections(dr._windows(tab[t], s, cw), radem, chi)          # [nk, nf]
        base = _phi(p, nvar, swapped)                                        # [nk, nvar]
        rr[i] = dr.conv_row_scale(F, nk, scaling)
        for l in range(s):
            jlo, jhi = max(0, l - cw + 1), min(l, nk - 1)
            if mistake == "first_window":
                jhi = jlo
            for j in range(jlo, jhi + 1):
                q = l - j
                delta[i, l] += _phi(p[j][None, :] + S[q] - S[q, t[l]][None, :], nvar, swapped) - base[j][None, :]
        if intercept and mistake != "keep_col0":
            delta[i, :, :, 0] = 0
    r = rr[:, None, None]
    mat = np.triu(vm) if mistake == "vm_upper" else vm
    flat = delta.reshape(n * L * V, nvar)
    if expansion or mistake in ("no_cross", "r_once"):
        quad = (_times(flat, mat) * flat).sum(axis=1).reshape(n, L, V)
        cross = (delta * u[:, None, None, :]).sum(axis=-1)
        Q = qq[:, None, None] + (0 if mistake == "no_cross" else 2 * r * cross) + (r if mistake == "r_once" else r * r) * quad
    else:
        zp = (z[:, None, None, :] + r[..., None] * delta).reshape(n * L * V, nvar)
        Q = (_times(zp, mat) * zp).sum(axis=1).reshape(n, L, V)
    Q[np.arange(L)[None, :] >= np.asarray(seqlen)[:, None]] = 0
    return Q, qq, u, z


# ------------------------------------------------------------------------------------------------------------------
# A-priori cap: derived, not tuned.  The operator forms a variant window's cos / sin values as the float32 feature operators do, so
# each is within  cap1 = cap_features(float32, P, norm, |chi|max, c = 1, nk = 1)  of exact (tests/dense_subst_scan.py).  An entry of
# delta adds |J(l)| <= min(conv_width, nk) variant values and as many own values in float64 and subtracts: m = 2 min(conv_width, nk)
# value errors and m + 1 float64 roundings on partial sums bounded by m,
#     eps = m cap1 + (m + 1) m u64,          |delta|_inf <= m.
# The three terms:  2 r delta . u  errs by  2 r eps |u_i|_1  plus the rounding of an nvar-term float64 sum of terms bounded by m |u|,
# (nvar + 1) u64 2 r m |u_i|_1;  r^2 delta^T Vm delta  errs by  r^2 eps (2 m + eps) sum|Vm|  plus the rounding of its nvar^2 terms, summed
# as nvar-term sums of nvar-term sums: (2 nvar + 2) u64 r^2 m^2 sum|Vm|.  Forming 2 r, r r, the two products and the two additions: 6
# roundings on values bounded by B = |q| + 2 r m |u|_1 + r^2 m^2 sum|Vm|.  u and q enter rounded to float64 (``carried`` False): u64 |q| +
# 2 r m u64 |u|_1.  Where the test feeds the operator u, q computed from float32 feature ROWS (``carried`` True: the kernel-object
# route), z itself is within  cz = cap_features(float32, P, norm, chimax, r, nk, u_out = u32)  of exact per column, so u = Vm z errs
# by at most cz max_a sum_b |Vm[a, b]| per entry and q by cz (2 |z|_1-weighted) -- bounded through  dq = cz sum|Vm| (2 zmax + cz)  and
# du_1 = cz sum|Vm|  (in 1-norm), entering as  dq + 2 r m du_1.  Under the intercept column 0 of delta is exactly zero and |u|_1 leaves
# u[0] out.  Maximum over the sequences.
# ------------------------------------------------------------------------------------------------------------------
def cap_var_scan(c, vm, u, q, conv_width, scaling, intercept, carried=False, z=None):
    tab = np.asarray(c["table"], dtype=np.float32)
    chi = c["chi"]
    F, P = chi.shape[0], dr.padded_width(conv_width * tab.shape[1])
    nvar = vm.shape[0]
    svm = float(np.abs(np.asarray(vm, dtype=np.float64)).sum())
    norm = float(np.sqrt(conv_width) * dr.max_row_norm(tab))
    chimax = float(np.abs(chi).max())
    cap1 = dr.cap_features(np.float32, P, norm, chimax, 1.0, nk=1)
    best = 0.0
    for i, s in enumerate(int(v) for v in c["seqlen"]):
        nk = s - conv_width + 1
        m = 2 * min(conv_width, nk)
        r = float(dr.conv_row_scale(F, nk, scaling))
        eps = m * cap1 + (m + 1) * m * U64
        ui = np.abs(np.asarray(u[i], dtype=np.float64))
        u1 = float(ui[1:].sum() if intercept else ui.sum())
        qi = abs(float(q[i]))
        bound = 2 * r * eps * u1 + (nvar + 1) * U64 * 2 * r * m * u1
        bound += r * r * eps * (2 * m + eps) * svm + (2 * nvar + 2) * U64 * r * r * m * m * svm
        bound += 6 * U64 * (qi + 2 * r * m * u1 + r * r * m * m * svm)
        bound += U64 * qi + 2 * r * m * U64 * u1
        if carried:
            cz = dr.cap_features(np.float32, P, norm, chimax, r, nk=nk, u_out=dr.U32)
            zmax = float(np.abs(np.asarray(z[i], dtype=np.float64)).max())
            bound += cz * svm * (2 * zmax + cz) + 2 * r * m * cz * svm
        best = max(best, bound)
    return best


# The written-out route (ConvSORFKernel.substitution_variance_scan_composed, xGPRegression.predict): every column of a mutant's
# feature row is within  cz = cap_features(float32, P, norm, chimax, r, nk, u_out = u32)  of exact -- float32 rows; a float64 row formed
# from float32 transforms errs by less -- and bounded by zb = max(r nk, 1 under the intercept); the quadratic form of its first nvar
# columns in float64 errs by  cz (2 zb + cz) sum|Vm|  plus the rounding of its nvar^2 terms, (2 nvar + 2) u64 zb^2 sum|Vm|.
def cap_written_out(c, vm, conv_width, scaling, intercept):
    tab = np.asarray(c["table"], dtype=np.float32)
    chi = c["chi"]
    F, P = chi.shape[0], dr.padded_width(conv_width * tab.shape[1])
    nvar = vm.shape[0]
    svm = float(np.abs(np.asarray(vm, dtype=np.float64)).sum())
    norm = float(np.sqrt(conv_width) * dr.max_row_norm(tab))
    best = 0.0
    for s in sorted({int(v) for v in c["seqlen"]}):
        nk = s - conv_width + 1
        r = float(dr.conv_row_scale(F, nk, scaling))
        cz = dr.cap_features(np.float32, P, norm, float(np.abs(chi).max()), r, nk=nk, u_out=dr.U32)
        zb = max(r * nk, 1.0 if intercept else 0.0)
        best = max(best, cz * (2 * zb + cz) * svm + (2 * nvar + 2) * U64 * zb * zb * svm)
    return best


def check(got, ref, cap):
    """The comparison of the GPU test: no element excused.  -> the largest |got - ref|."""
    return dss.check(got, ref, cap)


def make_vm(nvar, seed=0, decay=0.0, z=None):
    """Seeded symmetric Vm: diagonal in [0.75, 1.25], off-diagonal entries uniform with absolute row sums of about 1/2 -- a
    well-conditioned stand-in that keeps sum|Vm| proportional to nvar.  ``decay`` > 0: D Vm D with D = diag(rank^-decay), the columns
    ranked by the largest |z[:, a]| of the case's own (exact) feature rows -- a posterior that is confident about the columns the
    sequences excite.  The a-priori cap is proportional to |Vm z|_1, the outputs to |delta . Vm z|: with a flat spectrum their ratio
    grows like sqrt(nvar), and the cases of wide windows (a larger per-value cap) then miss ``cap <= 1e-2 max|Q - q|``; those cases take
    decay = 1, as the weights of dense_subst_scan.make_case decay for the same reason."""
    rng = np.random.default_rng([nvar, seed, 77])
    a = rng.uniform(-1, 1, size=(nvar, nvar))
    a = (a + a.T) / 2
    np.fill_diagonal(a, 0)
    a /= max(nvar - 1, 1) * 0.67                         # E|(x + y) / 2| = 1 / 3 for uniform x, y: row sums of about 1 / 2
    a[np.arange(nvar), np.arange(nvar)] = rng.uniform(0.75, 1.25, size=nvar)
    if decay > 0:
        score = np.abs(np.asarray(z, dtype=np.float64)).max(axis=0)
        rank = np.empty(nvar)
        rank[np.argsort(-score, kind="stable")] = np.arange(nvar)
        d = (1.0 + rank) ** -decay
        a = a * d[:, None] * d[None, :]
    return a


# (name of the operand set in dense_subst_scan.CASES, nvar, vm_stride - nvar, decay of make_vm)
CASES = [
    ("w16_c4_cw3", 16, 0, 0.0),               # 2 F: every column; intercept
    ("w64_onehot21_cw3", 2, 0, 0.0),          # one frequency
    ("w128_c21_cw6", 130, 0, 1.0),            # not a multiple of 4, 16 or 64; intercept
    ("w256_c21_cw9", 2048, 0, 1.0),           # a full tile; intercept
    ("w1024_c21_cw48", 512, 0, 1.0),
    ("w512_c16_cw20", 66, 6, 1.0),            # Vm rows strided
    ("graph_cw1", 34, 0, 0.0),
    ("vocab1", 4, 0, 0.0),
    ("vocab256_c18", 64, 0, 0.0),
    ("dup_rows", 130, 0, 0.0),
    ("n65", 18, 0, 0.0),
    ("n1", 512, 0, 0.0),
]


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(c, cw, scaling, intercept, nvar, pad, vm float64, ref Q, q64, u64 (the exact q, u rounded to float64), z, cap): computed
    once per process and shared; nothing in it is written to."""
    nvar, pad, decay = next((nv, pd, dc) for nm, nv, pd, dc in CASES if nm == name)
    c, cw, scaling, icpt = dss.case(name)
    vm = make_vm(nvar, decay=decay, z=exact_rows(c, nvar, cw, scaling, icpt) if decay > 0 else None)
    Q, q, u, z = var_scan(c, vm, cw, scaling, icpt)
    q64, u64 = np.asarray(q, dtype=np.float64), np.ascontiguousarray(np.asarray(u, dtype=np.float64))
    cap = cap_var_scan(c, vm, u64, q64, cw, scaling, icpt)
    return dict(c=c, cw=cw, scaling=scaling, icpt=icpt, nvar=nvar, pad=pad, vm=vm, ref=Q, q=q, q64=q64, u64=u64, z=z, cap=cap)
