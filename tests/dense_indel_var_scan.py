"""Dense-matrix reference of the indel VARIANCE scan of the sequence / graph kernels (xgpr_conv_token_indel_var_scan_f32) -- TEST
HELPER, numpy only, in ``np.longdouble``, from tests/dense_reference.py's ``projections`` and the helpers of
tests/dense_subst_var_scan.py (``_phi``, ``_times``, ``make_vm``, ``exact_rows``) on the operand sets and length lists of
tests/dense_indel_scan.py; nothing shared with oracle/.

Definition (notation of tests/dense_indel_scan.py and tests/dense_subst_var_scan.py; the first nvar feature columns only):

    z(t)         = r(nk_t) sum_{j < nk_t} phi(window j of t)                    (column 0 := 1 under the intercept)
    del[i, p]    = z(t without position p)^T Vm z(t without position p)         p < s;  0 beyond;  NaN where s == conv_width
    ins[i, g, v] = z(t with token v inserted before g)^T Vm z(the same)         g <= s; 0 beyond

``var_scan`` is BRUTE FORCE: every mutant is built as a token sequence, z is taken over ALL its windows with its own normaliser and
the quadratic form is evaluated directly (``dense_subst_var_scan._times``: fixed point from nvar = 1024); the only shortcut is the
linearity of the projections in the window.  ``decomposed`` evaluates the contract's three terms instead (include/
xgpr_hip_indel_var_scan.h) -- b = rho z_i + (1 - rho) e0, u~ = 1/2 (Vm + Vm^T) b, q~ = b^T Vm b, delta over the added and the removed
windows, Q = q~ + 2 r' delta . u~ + r'^2 delta^T Vm delta -- what the kernels implement, and ``mistake=`` plants ONE structural error
in it (sensitivity test only):
    "old_norm"            the sequence's own normaliser r(nk) on delta
    "no_rescale"          b = z_i: the sequence's columns are not rescaled
    "rescale_col0"        b = rho z_i: column 0 is rescaled too under the intercept
    "junction_short"      the deletion's junction windows stop one short of min(p - 1, nk - 2)
    "del_keeps_covering"  a deletion does not remove the windows that cover p
    "no_cross"            the term 2 r' delta . u~ dropped
    "r_once"              r' in place of r'^2 on the quadratic term
    "append_past_end"     the gap g = s treated as past the end (zeros)
    "cos_sin_swapped"     delta's columns 2f and 2f + 1 exchanged
"""
import functools

import numpy as np

import dense_indel_scan as dis
import dense_reference as dr
import dense_subst_var_scan as dv
from dense_reference import LD, U64

MISTAKES = ("old_norm", "no_rescale", "rescale_col0", "junction_short", "del_keeps_covering", "no_cross", "r_once", "append_past_end",
            "cos_sin_swapped")


class _Windows:
    """phi of windows given as token rows, through the single-slot projections S[q, v] of the first nvar / 2 frequencies."""

    def __init__(self, c, nvar, conv_width, swapped=False):
        tab = np.asarray(c["table"], dtype=LD)
        V, C = tab.shape
        self.cw, self.nvar, self.swapped = conv_width, nvar, swapped
        slots = np.zeros((conv_width, V, conv_width * C), dtype=LD)
        for q in range(conv_width):
            slots[q, :, q * C:(q + 1) * C] = tab
        self.S = dr.projections(slots.reshape(conv_width * V, conv_width * C), c["radem"], c["chi"][:nvar // 2]).reshape(conv_width, V, nvar // 2)
        self.q = np.arange(conv_width)

    def phi(self, wins):
        """wins [m, cw] int -> [m, nvar] longdouble."""
        wins = np.asarray(wins, dtype=np.int64).reshape(-1, self.cw)
        if wins.shape[0] == 0:
            return np.zeros((0, self.nvar), dtype=LD)
        return dv._phi(self.S[self.q[None, :], wins].sum(axis=1), self.nvar, self.swapped)

    def total(self, t):
        """sum of phi over ALL windows of the token sequence t -> [nvar]."""
        t = np.asarray(t, dtype=np.int64)
        return self.phi(np.lib.stride_tricks.sliding_window_view(t, self.cw)).sum(axis=0)


def _quad(rows, vm):
    return (dv._times(rows, vm) * rows).sum(axis=1)


def var_scan(c, vm, conv_width, scaling, intercept):
    """-> (del [n, L], ins [n, L + 1, V]) longdouble, by brute force over the mutants."""
    vm = np.asarray(vm, dtype=LD)
    nvar, cw, F = vm.shape[0], conv_width, c["chi"].shape[0]
    W = _Windows(c, nvar, cw)
    n, L = c["tokens"].shape
    V = c["table"].shape[0]
    dele = np.zeros((n, L), dtype=LD)
    ins = np.zeros((n, L + 1, V), dtype=LD)

    def z(t):
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
            dele[i, :s] = _quad(np.stack([z(t[:p] + t[p + 1:]) for p in range(s)]), vm)
        rows = np.stack([z(t[:g] + [v] + t[g:]) for g in range(s + 1) for v in range(V)])
        ins[i, :s + 1] = _quad(rows, vm).reshape(s + 1, V)
    return dele, ins


def operands(c, vm, conv_width, scaling, intercept, z=None, mistake=None):
    """What the caller of the operator supplies -> dict(u_del, q_del, u_ins, q_ins, z), longdouble: per row set u~ = 1/2 (Vm + Vm^T) b
    and q~ = b^T Vm b for b = rho z_i + (1 - rho) e0.  ``z``: the sequences' columns (default: exact).  The deletion pair of a
    sequence with s == conv_width (no mutant) is formed with rho = 1."""
    vm = np.asarray(vm, dtype=LD)
    nvar, cw, F = vm.shape[0], conv_width, c["chi"].shape[0]
    z = np.asarray(dv.exact_rows(c, nvar, cw, scaling, intercept) if z is None else z, dtype=LD)
    sym = (vm + vm.T) / 2
    out = dict(z=z)
    nk = np.asarray(c["seqlen"], dtype=np.int64) - cw + 1
    for which, nkm in (("del", np.maximum(nk - 1, 1)), ("ins", nk + 1)):
        rho = np.asarray([dis._r(F, int(b), scaling) / dis._r(F, int(a), scaling) for a, b in zip(nk, nkm)], dtype=LD)
        if mistake == "no_rescale":
            rho = np.ones_like(rho)
        b = z * rho[:, None]
        if intercept and mistake != "rescale_col0":
            b[:, 0] = 1
        out["u_" + which] = b @ sym
        out["q_" + which] = ((b @ vm) * b).sum(axis=1)
    return out


def decomposed(c, vm, conv_width, scaling, intercept, mistake=None):
    """The contract's three terms, in long double -> (del, ins); ``mistake`` plants one error."""
    vm = np.asarray(vm, dtype=LD)
    nvar, cw, F = vm.shape[0], conv_width, c["chi"].shape[0]
    W = _Windows(c, nvar, cw, swapped=mistake == "cos_sin_swapped")
    ops = operands(c, vm, cw, scaling, intercept, mistake=mistake)
    n, L = c["tokens"].shape
    V = c["table"].shape[0]
    dele = np.zeros((n, L), dtype=LD)
    ins = np.zeros((n, L + 1, V), dtype=LD)
    k = np.arange(cw)

    def terms(delta, rm, r, u, q):
        delta = np.array(delta, dtype=LD).reshape(-1, nvar)
        if intercept:
            delta[:, 0] = 0
        rd = r if mistake == "old_norm" else rm
        cross = 0 if mistake == "no_cross" else 2 * rd * (delta @ u)
        return q + cross + (rd if mistake == "r_once" else rd * rd) * _quad(delta, vm)

    for i in range(n):
        s = int(c["seqlen"][i])
        nk = s - cw + 1
        t = np.asarray(c["tokens"][i, :s], dtype=np.int64)
        own = W.phi(np.lib.stride_tricks.sliding_window_view(t, cw))              # [nk, nvar]
        r = dis._r(F, nk, scaling)
        # deletions
        if nk == 1:
            dele[i, :s] = LD("nan")
        else:
            rm = dis._r(F, nk - 1, scaling)
            deltas = []
            for p in range(s):
                lo, hi = max(0, p - cw + 1), min(p - 1, nk - 2) - (1 if mistake == "junction_short" else 0)
                A = np.zeros(nvar, dtype=LD)
                for j in range(lo, hi + 1):
                    A += W.phi(t[j + k + (k >= p - j)])[0]
                R = 0 if mistake == "del_keeps_covering" else own[lo:min(p, nk - 1) + 1].sum(axis=0)
                deltas.append(A - R)
            dele[i, :s] = terms(deltas, rm, r, ops["u_del"][i], ops["q_del"][i])
        # insertions
        rm = dis._r(F, nk + 1, scaling)
        deltas = []
        gaps = s if mistake == "append_past_end" else s + 1
        for g in range(gaps):
            lo = max(0, g - cw + 1)
            R = own[lo:min(g - 1, nk - 1) + 1].sum(axis=0)
            for v in range(V):
                A = np.zeros(nvar, dtype=LD)
                for j in range(lo, min(g, nk) + 1):
                    q = g - j
                    A += W.phi(np.concatenate([t[j:j + q], [v], t[j + q:j + cw - 1]]))[0]
                deltas.append(A - R)
        ins[i, :gaps] = terms(deltas, rm, r, ops["u_ins"][i], ops["q_ins"][i]).reshape(gaps, V)
    return dele, ins


# ------------------------------------------------------------------------------------------------------------------
# A-priori cap: derived, not tuned; the derivation of tests/dense_subst_var_scan.py with the indel's window sets and normaliser.  Each
# cos / sin value is within  cap1 = cap_features(float32, P, norm, |chi|max, c = 1, nk = 1)  of exact.  An entry of delta adds the
# values of the added windows (<= min(conv_width, nk + 1) for an insertion, <= min(conv_width, nk) - 1 for a deletion) and of the removed
# ones (<= min(conv_width, nk + 1) - 1, <= min(conv_width, nk)) in float64 and subtracts once:  m = 2 min(conv_width, nk) - 1  values for a
# deletion and  m = 2 min(conv_width, nk + 1) - 1  for an insertion (dense_indel_scan.cap_indel_scan counts the same windows), at most
# 2 conv_width - 1:  m value errors and m + 1 float64 roundings on partial sums bounded by m,
#     eps = m cap1 + (m + 1) m u64,          |delta|_inf <= m.
# With r' = r(nk -+ 1), the mutant's normaliser, formed on the device by a square root and a division from sqrt(1 / F) -- 3 relative
# roundings, carried by both terms that hold r' (twice by r'^2) --, the three terms err as in tests/dense_subst_var_scan.py with r' for
# r, u~ for u and q~ for q:  2 r' eps |u~|_1 + (nvar + 1) u64 2 r' m |u~|_1;  r'^2 eps (2 m + eps) sum|Vm| + (2 nvar + 2) u64 r'^2 m^2
# sum|Vm|;  6 roundings on values bounded by B = |q~| + 2 r' m |u~|_1 + r'^2 m^2 sum|Vm|;  u~, q~ rounded to float64:  u64 |q~| + 2 r' m
# u64 |u~|_1.  rho = r' / r enters through b = rho z_i + (1 - rho) e0 alone, i.e. through u~ and q~.  Where the test feeds the operator
# u~, q~ formed from float32 feature ROWS (``carried`` True: the kernel-object route), z is within  cz = cap_features(float32, P, norm,
# chimax, r, nk, u_out = u32)  of exact per column and rho -- a float64 division and square root on the host -- within 3 u64 rho, so b is
# within  cb = rho (cz + 3 u64 zmax)  per column and bounded by bmax = max(rho zmax, 1);  q~ then errs by  dq = cb sum|Vm| (2 bmax + cb)
# and u~ in 1-norm by  du_1 = cb sum|Vm|,  entering as  dq + 2 r' m du_1.  Under the intercept column 0 of delta is exactly zero and
# |u~|_1 leaves u~[0] out.  Maximum over the sequences that have the mutant; a cap for the deletions and one for the insertions.
# ------------------------------------------------------------------------------------------------------------------
def cap_var_scan(c, vm, ops, conv_width, scaling, intercept, carried=False):
    """-> (cap of the deletions, cap of the insertions); ``ops``: the dict of ``operands`` (any float type)."""
    tab = np.asarray(c["table"], dtype=np.float32)
    chi = c["chi"]
    F, P = chi.shape[0], dr.padded_width(conv_width * tab.shape[1])
    nvar = vm.shape[0]
    svm = float(np.abs(np.asarray(vm, dtype=np.float64)).sum())
    norm = float(np.sqrt(conv_width) * dr.max_row_norm(tab))
    chimax = float(np.abs(chi).max())
    cap1 = dr.cap_features(np.float32, P, norm, chimax, 1.0, nk=1)
    best = [0.0, 0.0]
    for i, s in enumerate(int(v) for v in c["seqlen"]):
        nk = s - conv_width + 1
        r = float(dis._r(F, nk, scaling))
        for which, key, km in ((0, "del", nk - 1), (1, "ins", nk + 1)):
            if km < 1:
                continue
            rm = float(dis._r(F, km, scaling))
            m = 2 * min(conv_width, nk + which) - 1
            eps = m * cap1 + (m + 1) * m * U64
            ui = np.abs(np.asarray(ops["u_" + key][i], dtype=np.float64))
            u1 = float(ui[1:].sum() if intercept else ui.sum())
            qi = abs(float(ops["q_" + key][i]))
            big = qi + 2 * rm * m * u1 + rm * rm * m * m * svm
            bound = 2 * rm * eps * u1 + (nvar + 1) * U64 * 2 * rm * m * u1
            bound += rm * rm * eps * (2 * m + eps) * svm + (2 * nvar + 2) * U64 * rm * rm * m * m * svm
            bound += 3 * U64 * (2 * rm * m * u1 + 2 * rm * rm * m * m * svm)
            bound += 6 * U64 * big
            bound += U64 * qi + 2 * rm * m * U64 * u1
            if carried:
                rho = rm / r
                cz = dr.cap_features(np.float32, P, norm, chimax, r, nk=nk, u_out=dr.U32)
                zmax = float(np.abs(np.asarray(ops["z"][i], dtype=np.float64)).max())
                cb = rho * (cz + 3 * U64 * zmax)
                bmax = max(rho * zmax, 1.0)
                bound += cb * svm * (2 * bmax + cb) + 2 * rm * m * cb * svm
            best[which] = max(best[which], bound)
    return best[0], best[1]


# The written-out route (ConvSORFKernel.indel_variance_scan_composed, xGPRegression.predict): the bound of
# dense_subst_var_scan.cap_written_out at the mutants' window counts nk -+ 1.
def cap_written_out(c, vm, conv_width, scaling, intercept):
    tab = np.asarray(c["table"], dtype=np.float32)
    chi = c["chi"]
    F, P = chi.shape[0], dr.padded_width(conv_width * tab.shape[1])
    nvar = vm.shape[0]
    svm = float(np.abs(np.asarray(vm, dtype=np.float64)).sum())
    norm = float(np.sqrt(conv_width) * dr.max_row_norm(tab))
    best = [0.0, 0.0]
    for s in sorted({int(v) for v in c["seqlen"]}):
        for which, km in ((0, s - conv_width), (1, s - conv_width + 2)):
            if km < 1:
                continue
            r = float(dis._r(F, km, scaling))
            cz = dr.cap_features(np.float32, P, norm, float(np.abs(chi).max()), r, nk=km, u_out=dr.U32)
            zb = max(r * km, 1.0 if intercept else 0.0)
            best[which] = max(best[which], cz * (2 * zb + cz) * svm + (2 * nvar + 2) * U64 * zb * zb * svm)
    return best[0], best[1]


def check(got, ref, cap, zeros):
    """The comparison of the GPU test (dense_indel_scan.check): NaN exactly where the reference has NaN, bitwise +0.0 where ``zeros`` is
    set, everything else finite and within ``cap``; no element excused.  -> the largest |got - ref|."""
    return dis.check(got, ref, cap, zeros=zeros)


# (name of the operand set in dense_indel_scan.CASES, nvar, vm_stride - nvar, decay of make_vm): the list of dense_subst_var_scan.CASES
# -- with a steeper decay of Vm on three of the wide-window cases, whose caps would otherwise miss 1e-2 of the spread
# (tests/test_indel_var_scan_host.py): an indel's delta holds up to 2 conv_width - 1 values where a substitution's holds conv_width
_DECAY = {"w128_c21_cw6": 1.5, "w256_c21_cw9": 1.5, "w512_c16_cw20": 1.5}
# ... and the deletions of w512_c16_cw20 (scaling 2, a small spread) still miss it at nvar = 66 under any decay: that case takes the strided
# nvar = 18 and n65, which has room, the 66 in exchange -- the list of nvar is the same
_NVAR = {"w512_c16_cw20": 18, "n65": 66}
CASES = [(nm, _NVAR.get(nm, nv), pd, _DECAY.get(nm, dc)) for nm, nv, pd, dc in dv.CASES]


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(c, cw, scaling, icpt, nvar, pad, vm float64, ref_del, ref_ins, ops (longdouble operands), u_del, q_del, u_ins, q_ins (the
    exact u~, q~ rounded to float64), cap_del, cap_ins): computed once per process and shared; nothing in it is written to."""
    nvar, pad, decay = next((nv, pd, dc) for nm, nv, pd, dc in CASES if nm == name)
    c, cw, scaling, icpt = dis.case(name)
    z = dv.exact_rows(c, nvar, cw, scaling, icpt)
    vm = dv.make_vm(nvar, decay=decay, z=z if decay > 0 else None)
    dele, ins = var_scan(c, vm, cw, scaling, icpt)
    ops = operands(c, vm, cw, scaling, icpt, z=z)
    out = dict(c=c, cw=cw, scaling=scaling, icpt=icpt, nvar=nvar, pad=pad, vm=vm, ref_del=dele, ref_ins=ins, ops=ops)
    for key in ("u_del", "q_del", "u_ins", "q_ins"):
        out[key] = np.ascontiguousarray(np.asarray(ops[key], dtype=np.float64))
    out["cap_del"], out["cap_ins"] = cap_var_scan(c, vm, out, cw, scaling, icpt)
    for arr in (dele, ins):
        arr.setflags(write=False)
    return out
