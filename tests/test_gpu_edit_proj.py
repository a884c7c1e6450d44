"""The single-edit projection on the device (xgpr_conv_token_subst_proj_f32, xgpr_conv_token_indel_proj_f32,
ConvSORFKernel.*_projection_scan / *_projection_scan_composed, xGPRegression.single_edit_neighbourhoods / sample_single_edits)
against the long-double reference of tests/dense_edit_proj.py, within its a-priori caps -- one per sequence and column, derived from
the operation count (tests/test_edit_proj_host.py holds them to 1e-2 of every column's signal and shows what they separate) -- or bit
for bit where a test says so.  No element is excused.  Every comparison prints one ``EDITPROJ`` line with measured error, cap and ratio;
the first test leaves the largest ratios of the operator's comparisons in profiles/edit_proj_errors.txt."""
import ctypes
import os

import numpy as np
import pytest
import torch

import dense_edit_proj as dep
import dense_indel_scan as dis
import dense_indel_var_scan as div
import dense_reference as dr
import dense_subst_var_scan as dv
from dense_reference import LD, U64
from guarded import same_bits
from test_gpu_indel_var_scan import _kernel, _kernel_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
CASE_NAMES = [c[0] for c in dv.CASES]
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
RATIOS = {}


@pytest.fixture(scope="module")
def ext():
    from xgpr_amd import xgpr_hip_rfgen_ext as e
    return e


def _pm(pm, pad=0):
    """pm on the device, its rows strided where ``pad`` says so (NaN behind every row)."""
    full = np.full((pm.shape[0], pm.shape[1] + pad), np.nan)
    full[:, :pm.shape[1]] = pm
    return torch.from_numpy(full).to(DEV)[:, :pm.shape[1]]


def _operands(c, rows):
    rows = np.arange(c["tokens"].shape[0]) if rows is None else np.asarray(rows)
    tokens = np.ascontiguousarray(c["tokens"][rows])
    dev = [torch.from_numpy(tokens).to(DEV), torch.from_numpy(c["table"]).to(DEV)]
    tail = (torch.from_numpy(c["radem"]).to(DEV), torch.from_numpy(c["chi"]).to(DEV), np.ascontiguousarray(c["seqlen"][rows]))
    return rows, tokens.shape, dev, tail


def run_subst(ext, k, pm, b, rows=None, slab_rows=0, pad=0):
    """The ext call on the case's sequences (``rows``: a subset, in that order); the output starts as NaN."""
    c = k["c"]
    rows, (n, L), dev, tail = _operands(c, rows)
    out = torch.full((n, L, c["table"].shape[0], pm.shape[1]), float("nan"), dtype=F64, device=DEV)
    ext.hipConvTokenSubstProj(*dev, _pm(pm, pad), torch.from_numpy(np.ascontiguousarray(b[rows])).to(DEV), out, *tail, k["cw"], k["scaling"],
                              k["icpt"], slab_rows=slab_rows)
    return out


def run_indel(ext, k, pm, bd, bi, rows=None, slab_rows=0, pad=0, dele=True, ins=True):
    c = k["c"]
    rows, (n, L), dev, tail = _operands(c, rows)
    V, K = c["table"].shape[0], pm.shape[1]
    up = lambda b: torch.from_numpy(np.ascontiguousarray(b[rows])).to(DEV)
    od = torch.full((n, L, K), float("nan"), dtype=F64, device=DEV) if dele else None
    oi = torch.full((n, L + 1, V, K), float("nan"), dtype=F64, device=DEV) if ins else None
    ext.hipConvTokenIndelProj(*dev, _pm(pm, pad), up(bd) if dele else None, up(bi) if ins else None, od, oi, *tail, k["cw"], k["scaling"],
                              k["icpt"], slab_rows=slab_rows)
    return od, oi


def _zeros(c):
    L = c["tokens"].shape[1]
    return dis.zero_mask(c["seqlen"], L), dis.zero_mask(c["seqlen"], L, gaps=True)


def report(tag, case, got, ref, cap, zeros):
    """dep.check (NaN and +0.0 patterns exact, every live element within its cap) and one EDITPROJ line -> the largest error / cap."""
    err, ratio = dep.check(got, ref, cap, zeros)
    print(f"EDITPROJ {tag:<14} {str(case):<44} hip-dense {err:.3e}  cap {float(np.max(cap)):.3e}  ratio {ratio:.4f}")
    assert ratio <= 1.0
    return ratio


@pytest.mark.parametrize("name", CASE_NAMES)
def test_operator_against_the_dense_reference_at_k_nvar(ext, name):
    """pm = chol(the case's vm): K = nvar columns, a factor of the neighbourhood's covariance; pm strided where the case says so."""
    k = dep.subst_case(name)
    zd, zi = _zeros(k["c"])
    out = run_subst(ext, k, k["pm"], k["b64"], pad=k["pad"])
    RATIOS[(name, "sub")] = report("operator sub", (name, k["nvar"]), out.cpu().numpy(), k["ref"], k["cap"], zd)
    assert same_bits(out, run_subst(ext, k, k["pm"], k["b64"], pad=k["pad"])), "two runs differ"
    k = dep.indel_case(name)
    od, oi = run_indel(ext, k, k["pm"], k["b_del"], k["b_ins"], pad=k["pad"])
    RATIOS[(name, "del")] = report("operator del", (name, k["nvar"]), od.cpu().numpy(), k["ref_del"], k["cap_del"], zd)
    RATIOS[(name, "ins")] = report("operator ins", (name, k["nvar"]), oi.cpu().numpy(), k["ref_ins"], k["cap_ins"], zi)
    if len(RATIOS) == 3 * len(CASE_NAMES):                               # the whole list ran: leave the summary
        worst = max(RATIOS, key=RATIOS.get)
        lines = ["# tests/test_gpu_edit_proj.py: the operator at K = nvar against the long-double reference, largest measured error / a-priori cap\n"]
        lines += [f"{key[0]:<20} {key[1]}  ratio {RATIOS[key]:.4f}\n" for key in sorted(RATIOS)]
        lines.append(f"largest ratio {RATIOS[worst]:.4f} ({worst[0]}, {worst[1]})\n")
        try:                                                             # (results are bitwise reproducible: the same text every run)
            with open(os.path.join(ROOT, "profiles", "edit_proj_errors.txt"), "w") as f:
                f.writelines(lines)
        except OSError:                                                  # a read-only checkout: the EDITPROJ lines above say the same
            pass


NARROW = ["w16_c4_cw3", "w128_c21_cw6", "w512_c16_cw20", "n65", "graph_cw1"]


def _narrow(name):
    """A seeded pm [nvar, 65] for the case's operands, with the reference and the caps: (subst dict, indel dict)."""
    if name not in _narrow.cache:
        out = []
        for k in (dict(dv.case(name)), dict(div.case(name))):
            pm = np.random.default_rng([k["nvar"], 6565]).normal(size=(k["nvar"], 65)) / np.sqrt(k["nvar"])
            c, args = k["c"], (k["cw"], k["scaling"], k["icpt"])
            if "ref" in k:
                ref, b = dep.subst_proj(c, pm, *args, z=k["z"])
                b64 = np.asarray(b, dtype=np.float64)
                k.update(pm=pm, ref=ref, b64=b64, cap=dep.cap_subst(c, pm, b64, *args))
            else:
                rd, ri, bd, bi = dep.indel_proj(c, pm, *args, z=k["ops"]["z"])
                bd, bi = np.asarray(bd, dtype=np.float64), np.asarray(bi, dtype=np.float64)
                cd, ci = dep.cap_indel(c, pm, bd, bi, *args)
                k.update(pm=pm, ref_del=rd, ref_ins=ri, b_del=bd, b_ins=bi, cap_del=cd, cap_ins=ci)
            out.append(k)
        _narrow.cache[name] = tuple(out)
    return _narrow.cache[name]


_narrow.cache = {}


@pytest.mark.parametrize("name", NARROW)
def test_operator_at_1_3_and_65_columns_and_a_strided_pm(ext, name):
    """K = 65 crosses a 64-column block; K = 1 and 3 are its first columns (column k does not depend on K: checked bit for bit, and
    each against the reference); pm_stride > K at every K."""
    ks, ki = _narrow(name)
    zd, zi = _zeros(ks["c"])
    wide = run_subst(ext, ks, ks["pm"], ks["b64"])
    wd, wi = run_indel(ext, ki, ki["pm"], ki["b_del"], ki["b_ins"])
    for K, pad in ((65, 0), (65, 7), (64, 0), (3, 0), (3, 1), (1, 0), (1, 5)):
        out = run_subst(ext, ks, ks["pm"][:, :K], ks["b64"][:, :K], pad=pad)
        od, oi = run_indel(ext, ki, ki["pm"][:, :K], ki["b_del"][:, :K], ki["b_ins"][:, :K], pad=pad)
        assert same_bits(out, wide[..., :K].contiguous()) and same_bits(od, wd[..., :K].contiguous()) and same_bits(oi, wi[..., :K].contiguous()), (K, pad)
        if pad == 0:
            report(f"K={K} sub", name, out.cpu().numpy(), ks["ref"][..., :K], ks["cap"][:, :K], zd)
            report(f"K={K} del", name, od.cpu().numpy(), ki["ref_del"][..., :K], ki["cap_del"][:, :K], zd)
            report(f"K={K} ins", name, oi.cpu().numpy(), ki["ref_ins"][..., :K], ki["cap_ins"][:, :K], zi)


def test_own_token_rows_are_b_bit_for_bit_and_dead_rows_exact(ext):
    """delta is exactly +0.0 at a sequence's own token: the row is b[i]; +0.0 bitwise past a length; a quiet NaN at the deletions of the
    s == conv_width sequence and nowhere else -- where the indel variance scan has them."""
    from test_gpu_indel_var_scan import run_operator
    for name in ("w256_c21_cw9", "graph_cw1", "dup_rows", "w128_c21_cw6"):
        ks, ki = dep.subst_case(name), dep.indel_case(name)
        c = ks["c"]
        n, L = c["tokens"].shape
        out = run_subst(ext, ks, ks["pm"], ks["b64"]).cpu().numpy()
        for i in range(n):
            for l in range(int(c["seqlen"][i])):
                assert out[i, l, c["tokens"][i, l]].tobytes() == ks["b64"][i].tobytes(), (name, i, l)
        zd, zi = _zeros(c)
        od, oi = (t.cpu().numpy() for t in run_indel(ext, ki, ki["pm"], ki["b_del"], ki["b_ins"]))
        assert not out[zd].view(np.uint64).any() and not od[zd].view(np.uint64).any() and not oi[zi].view(np.uint64).any()
        vd, _ = run_operator(ext, div.case(name))
        nan = np.isnan(vd.cpu().numpy())
        assert np.array_equal(np.isnan(od), np.broadcast_to(nan[:, :, None], od.shape)) and not np.isnan(oi).any() and not np.isnan(out).any()
        if nan.any():
            assert ((od[nan].view(np.uint64) >> np.uint64(51)) & np.uint64(1)).all()          # quiet


def test_two_identical_table_rows_give_bit_equal_rows(ext):
    ks, ki = dep.subst_case("dup_rows"), dep.indel_case("dup_rows")
    assert (ks["c"]["table"][1] == ks["c"]["table"][3]).all()
    out = run_subst(ext, ks, ks["pm"], ks["b64"])
    _, oi = run_indel(ext, ki, ki["pm"], ki["b_del"], ki["b_ins"])
    for t in (out, oi):
        assert same_bits(t[:, :, 1].contiguous(), t[:, :, 3].contiguous()) and not same_bits(t[:, :, 1].contiguous(), t[:, :, 2].contiguous())


@pytest.mark.parametrize("name", ["n65", "w256_c21_cw9", "w128_c21_cw6"])
def test_the_slab_size_does_not_enter(ext, name):
    """slab_rows = 16: many slabs, slab edges inside a slot's V rows (V = 3, 7, 21), row counts that are no multiple of 16, the last row
    tile not full; 48: three tiles, a cut inside a slot's 21 rows."""
    ks, ki = _narrow(name) if name in NARROW else (dep.subst_case(name), dep.indel_case(name))
    pm_s, pm_i = ks["pm"][:, :65], ki["pm"][:, :65]
    bs, bd, bi = ks["b64"][:, :65], ki["b_del"][:, :65], ki["b_ins"][:, :65]
    w = run_subst(ext, ks, pm_s, bs)
    wd, wi = run_indel(ext, ki, pm_i, bd, bi)
    for slab in (16, 48):
        sd, si = run_indel(ext, ki, pm_i, bd, bi, slab_rows=slab)
        assert same_bits(run_subst(ext, ks, pm_s, bs, slab_rows=slab), w) and same_bits(sd, wd) and same_bits(si, wi), slab


@pytest.mark.parametrize("name", ["w256_c21_cw9", "w1024_c21_cw48", "n65"])
def test_a_sequence_alone_and_inside_a_batch(ext, name):
    ks, ki = dep.subst_case(name), dep.indel_case(name)
    pm_s, pm_i = ks["pm"][:, :66], ki["pm"][:, :66]
    bs, bd, bi = ks["b64"][:, :66], ki["b_del"][:, :66], ki["b_ins"][:, :66]
    n = ks["c"]["tokens"].shape[0]
    w = run_subst(ext, ks, pm_s, bs)
    wd, wi = run_indel(ext, ki, pm_i, bd, bi)
    for i in sorted({0, 1 % n, n // 2, n - 1}):
        ad, ai = run_indel(ext, ki, pm_i, bd, bi, rows=[i])
        assert same_bits(run_subst(ext, ks, pm_s, bs, rows=[i])[0], w[i]) and same_bits(ad[0], wd[i]) and same_bits(ai[0], wi[i]), i
    rev = np.arange(n)[::-1]                                    # every sequence at another index
    rd, ri = run_indel(ext, ki, pm_i, bd, bi, rows=rev)
    assert same_bits(run_subst(ext, ks, pm_s, bs, rows=rev).flip(0).contiguous(), w)
    assert same_bits(rd.flip(0).contiguous(), wd) and same_bits(ri.flip(0).contiguous(), wi)
    od, none = run_indel(ext, ki, pm_i, bd, bi, ins=False)      # one row set alone
    assert none is None and same_bits(od, wd)
    none, oi = run_indel(ext, ki, pm_i, bd, bi, dele=False)
    assert none is None and same_bits(oi, wi)


@pytest.mark.parametrize("name", ["w16_c4_cw3", "w128_c21_cw6", "w256_c21_cw9", "dup_rows", "n1", "vocab256_c18"])
def test_row_norms_at_the_factor_are_the_variance_scans(ext, name):
    """pm pm^T = vm: a row's sum of squares is the quadratic form the variance scan writes.  Bound: the variance scan's cap plus this
    operator's propagated through the square, 2 |psi|_1 cap + K cap^2 (psi: the exact row, cap: the sequence's largest column cap); the
    sum of squares itself is taken in long double here."""
    from test_gpu_indel_var_scan import run_operator
    from test_gpu_subst_var_scan import run_operator as run_subst_var
    kv, ks = dv.case(name), dep.subst_case(name)
    kiv, ki = div.case(name), dep.indel_case(name)
    quad_s = run_subst_var(ext, kv).cpu().numpy()
    quad_d, quad_i = (t.cpu().numpy() for t in run_operator(ext, kiv))
    out = run_subst(ext, ks, ks["pm"], ks["b64"], pad=ks["pad"]).cpu().numpy()
    od, oi = (t.cpu().numpy() for t in run_indel(ext, ki, ki["pm"], ki["b_del"], ki["b_ins"], pad=ki["pad"]))
    K = ks["pm"].shape[1]
    for which, rows, ref, cap, quad, vcap in (("sub", out, ks["ref"], ks["cap"], quad_s, kv["cap"]),
                                              ("del", od, ki["ref_del"], ki["cap_del"], quad_d, kiv["cap_del"]),
                                              ("ins", oi, ki["ref_ins"], ki["cap_ins"], quad_i, kiv["cap_ins"])):
        sq = (rows.astype(LD) ** 2).sum(axis=-1)
        capi = cap.max(axis=1).reshape((-1,) + (1,) * (sq.ndim - 1))
        bound = vcap + 2 * np.abs(ref).sum(axis=-1) * capi + K * capi * capi
        ok = ~np.isnan(quad)
        assert np.array_equal(ok, ~np.isnan(np.asarray(sq, dtype=np.float64)))
        ratio = float((np.abs(sq - quad)[ok] / np.asarray(bound, dtype=np.float64)[ok]).max()) if ok.any() else 0.0
        print(f"EDITPROJ norms {which:<9} {name:<44} largest |sum psi^2 - quad| / bound {ratio:.3e}")
        assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------ validation on the device
def test_every_refusal_launches_nothing(ext):
    """The refusals of the header, in its order, with real device arrays: the error is returned and the outputs and the workspace keep
    their bits."""
    from xgpr_amd import _lib
    import test_subst_var_scan_host as host
    k = dep.indel_case("w16_c4_cw3")
    c, nvar, K = k["c"], k["nvar"], 5
    n, L = c["tokens"].shape
    V, C = c["table"].shape
    F, R = c["chi"].shape[0], c["radem"].shape[2]
    dev = {key: torch.from_numpy(c[key]).to(DEV) for key in ("tokens", "table", "radem", "chi")}
    pm = torch.from_numpy(np.ascontiguousarray(k["pm"][:, :K])).to(DEV)
    bs = [torch.from_numpy(np.ascontiguousarray(k[key][:, :K])).to(DEV) for key in ("b_del", "b_del", "b_ins")]
    lens_dev = torch.from_numpy(c["seqlen"]).to(DEV)
    outs = [torch.full(shape, float("nan"), dtype=F64, device=DEV) for shape in ((n, L, V, K), (n, L, K), (n, L + 1, V, K))]
    ws = torch.full((ext.conv_token_edit_proj_workspace_bytes(R, nvar, 0),), 0xA5, dtype=torch.uint8, device=DEV)
    before = [o.clone() for o in outs] + [ws.clone()]
    unchanged = lambda: all(same_bits(a, b) for a, b in zip(outs, before)) and bool((ws == before[3]).all())
    codes = host._codes()

    def call(indel, **kw):
        a = dict(n=n, L=L, vocab=V, C=C, F=F, R=R, nvar=nvar, K=K, stride=K, cw=k["cw"], scaling=k["scaling"], slab=0, lens=c["seqlen"],
                 ws=ws.data_ptr(), wb=ws.numel(), pm=pm.data_ptr(), b=bs[0].data_ptr(), out=outs[0].data_ptr(), bd=bs[1].data_ptr(),
                 bi=bs[2].data_ptr(), od=outs[1].data_ptr(), oi=outs[2].data_ptr())
        a.update(kw)
        lens = np.ascontiguousarray(a["lens"], dtype=np.int32)
        tail = (dev["radem"].data_ptr(), dev["chi"].data_ptr(), ctypes.c_void_p(lens.ctypes.data), lens_dev.data_ptr(), a["n"], a["L"],
                a["vocab"], a["C"], a["F"], a["R"], a["nvar"], a["K"], a["cw"], a["scaling"], int(k["icpt"]), a["slab"], a["ws"], a["wb"], None)
        lib = _lib.load()
        if indel:
            rc = lib.xgpr_conv_token_indel_proj_f32(dev["tokens"].data_ptr(), dev["table"].data_ptr(), a["pm"], a["stride"], a["bd"], a["bi"],
                                                    a["od"], a["oi"], *tail)
        else:
            rc = lib.xgpr_conv_token_subst_proj_f32(dev["tokens"].data_ptr(), dev["table"].data_ptr(), a["pm"], a["stride"], a["b"], a["out"], *tail)
        torch.cuda.synchronize()
        return int(rc)

    ordered = [(dict(n=-1), "ARRAY_DIMS"), (dict(scaling=3), "ARRAY_DIMS"), (dict(cw=L + 1), "CONV_WIDTH"), (dict(F=R + 1), "RFFS_FREQS"),
               (dict(nvar=nvar - 1), "ARRAY_DIMS"), (dict(K=0), "ARRAY_DIMS"), (dict(stride=K - 1), "ARRAY_SIZES"), (dict(slab=24), "ARRAY_DIMS"),
               (dict(lens=[L + 1] * n), "SEQLEN_RANGE"), (dict(vocab=257), "ARRAY_DIMS"), (dict(vocab=256, C=19, R=64), "UNSUPPORTED"),
               (dict(wb=ws.numel() - 1), "WORKSPACE"), (dict(ws=None), "WORKSPACE"), (dict(pm=None), "WORKSPACE")]
    for indel in (False, True):
        extra = [(dict(od=None), "WORKSPACE"), (dict(bi=None), "WORKSPACE"), (dict(bd=None, od=None, bi=None, oi=None), "WORKSPACE")] if indel \
            else [(dict(b=None), "WORKSPACE"), (dict(out=None), "WORKSPACE")]
        for kw, code in ordered + extra:
            assert call(indel, **kw) == codes[code], (indel, kw, _lib.last_error())
            assert unchanged(), kw
        for (kw0, code0), (kw1, _) in zip(ordered[:-3], ordered[1:-2]):          # two at once: the earlier one in the order is reported
            if not set(kw0) & set(kw1):
                assert call(indel, **kw0, **kw1) == codes[code0], (kw0, kw1)
                assert unchanged()
        assert call(indel, n=0) == 0 and unchanged()                             # no sequences: nothing launched
    assert call(False) == 0 and call(True) == 0                                  # ... and the unchanged calls run
    assert all(not same_bits(a, b) for a, b in zip(outs, before[:3])) and bool(torch.isfinite(outs[0]).all())


# ------------------------------------------------------------------------------------------------ the kernel object
def _padded(pm):
    out = np.zeros((pm.shape[0] + (pm.shape[0] & 1), pm.shape[1]))
    out[:pm.shape[0]] = pm
    return out


def _row_bounds(k, c):
    """A bound on |z'|_2^2 over every mutant's first columns: F frequencies of (r' nk')^2 (cos^2 + sin^2) each, and the intercept."""
    F = c["chi"].shape[0]
    nk = int(c["seqlen"].max()) - k.conv_width + 2
    return 1.0 + F * float(dis._r(F, nk, k.scaling_type) * nk) ** 2


@pytest.mark.parametrize("choice,averaging,nvar,K", [("Conv1dRBF", "sqrt", 32, 32), ("Conv1dMatern", "full", 15, 3), ("GraphRBF", "full", 64, 65),
                                                     ("Conv1dCauchy", "none", 130, 1), ("GraphMatern", "sqrt", 21, 21)])
def test_kernel_scan_against_the_composed_route(ext, choice, averaging, nvar, K):
    """Each route within its own cap of the dense reference: the operator fed from float32 rows (``carried``), the written-out route
    (``cap_written_out``); an odd nvar is padded with a zero row."""
    from xgpr_amd.dataset import TokenBatch
    n, L, C, cw, M, V = 4, 9, 6, 4, 600, 5
    k = _kernel(choice, n, L, C, cw, M, averaging=averaging)
    table, c = _kernel_case(k, n, L, V, 41, (9, 4, 6, 5) if k.conv_width > 1 else (9, 1, 6, 2))
    pm = np.random.default_rng([nvar, K, 9]).normal(size=(nvar, K)) / np.sqrt(nvar)
    batch = TokenBatch(torch.from_numpy(c["tokens"]).to(DEV), torch.from_numpy(table).to(DEV))
    sub = k.substitution_projection_scan(batch, c["seqlen"], pm)
    dele, ins = k.indel_projection_scan(batch, c["seqlen"], pm)
    assert all(g.dtype == F64 and g.is_cuda for g in (sub, dele, ins))
    assert tuple(sub.shape) == (n, L, V, K) and tuple(dele.shape) == (n, L, K) and tuple(ins.shape) == (n, L + 1, V, K)
    k.COMPOSED_SCAN_ELEMS = 37 * M                               # several slices, the last one ragged
    pmd = torch.from_numpy(pm).to(DEV)
    csub = k.substitution_projection_scan_composed(batch, c["seqlen"], pmd)
    cdel, cins = k.indel_projection_scan_composed(batch, c["seqlen"], pmd)
    pp, args = _padded(pm), (k.conv_width, k.scaling_type, k.fit_intercept)
    z = dv.exact_rows(c, pp.shape[0], *args)
    rs, b = dep.subst_proj(c, pp, *args, z=z)
    rd, ri, bd, bi = dep.indel_proj(c, pp, *args, z=z)
    caps = (dep.cap_subst(c, pp, b, *args, carried=True, z=z),) + dep.cap_indel(c, pp, bd, bi, *args, carried=True, z=z)
    zd, zi = _zeros(c)
    tag = (choice, averaging, nvar, K)
    for which, g, f, ref, cap, zeros, w in (("sub", sub, csub, rs, caps[0], zd, None), ("del", dele, cdel, rd, caps[1], zd, 0),
                                            ("ins", ins, cins, ri, caps[2], zi, 1)):
        ccap = np.broadcast_to(dep.cap_written_out(c, pp, *args, w)[None, :], cap.shape)
        report("kernel " + which, tag, g.cpu().numpy(), ref, cap, zeros)
        report("composed " + which, tag, f.cpu().numpy(), ref, ccap, zeros)
    # tokens that are not contiguous take the composed route
    wide = torch.from_numpy(np.concatenate([c["tokens"], c["tokens"]], axis=1)).to(DEV)
    assert not wide[:, :L].is_contiguous()
    again = k.indel_projection_scan(TokenBatch(wide[:, :L], batch.table), c["seqlen"], pm)
    assert same_bits(again[0], cdel) and same_bits(again[1], cins)
    assert same_bits(k.substitution_projection_scan(TokenBatch(wide[:, :L], batch.table), c["seqlen"], pm), csub)
    with pytest.raises(RuntimeError, match="TokenBatch"):
        k.substitution_projection_scan(table[c["tokens"]], c["seqlen"], pm)
    with pytest.raises(RuntimeError, match=r"\[nvar, K\]"):
        k.indel_projection_scan(batch, c["seqlen"], pm[:, 0])


def test_beyond_the_operator_the_kernel_object_takes_the_composed_route(ext):
    """K above 2048: the predicate is 0, the ext call refuses and writes nothing, the kernel object still answers."""
    from xgpr_amd.dataset import TokenBatch
    n, L, C, cw, M, V = 2, 6, 4, 3, 64, 3
    k = _kernel("Conv1dRBF", n, L, C, cw, M, icpt=False)
    table, c = _kernel_case(k, n, L, V, 43, (6, 4))
    nvar, K = 16, 2049
    assert ext.conv_token_edit_proj_ok(cw * C, V, C, M // 2, nvar, K) == 0 and ext.conv_token_edit_proj_ok(cw * C, V, C, M // 2, nvar, 2048) == 1
    pm = np.random.default_rng(44).normal(size=(nvar, K))
    out = torch.zeros((n, L, V, K), dtype=F64, device=DEV)
    with pytest.raises(RuntimeError, match="K <= 2048"):
        ext.hipConvTokenSubstProj(torch.from_numpy(c["tokens"]).to(DEV), torch.from_numpy(c["table"]).to(DEV), torch.from_numpy(pm).to(DEV),
                                  torch.zeros((n, K), dtype=F64, device=DEV), out, k.radem_diag, k.chi_arr, c["seqlen"], cw, k.scaling_type, False)
    assert float(out.abs().max()) == 0.0
    batch = TokenBatch(torch.from_numpy(c["tokens"]).to(DEV), torch.from_numpy(table).to(DEV))
    got = (k.substitution_projection_scan(batch, c["seqlen"], pm),) + tuple(k.indel_projection_scan(batch, c["seqlen"], pm))
    args = (cw, k.scaling_type, False)
    refs = (dep.subst_proj(c, pm, *args)[0],) + dep.indel_proj(c, pm, *args)[:2]
    zd, zi = _zeros(c)
    for which, g, ref, zeros, w in zip(("sub", "del", "ins"), got, refs, (zd, zd, zi), (None, 0, 1)):
        ccap = np.broadcast_to(dep.cap_written_out(c, pm, *args, w)[None, :], (n, K))
        report("composed " + which, ("K", K), g.cpu().numpy(), ref, ccap, zeros)


# ------------------------------------------------------------------------------------------------ the model
N, L_, C_, CW, V_, NVAR = 40, 12, 4, 3, 5, 16


def _fit(kernel_choice):
    from xgpr_amd.dataset import build_regression_dataset
    from xgpr_amd.models import xGPRegression
    rng = np.random.default_rng(45)
    table = rng.uniform(-1, 1, size=(V_, C_)).astype(np.float32)
    tokens = rng.integers(0, V_, size=(N, L_)).astype(np.int64)
    seqlen = rng.integers(CW, L_ + 1, size=N).astype(np.int32)
    seqlen[:3] = (L_, CW, 7)
    x = table[tokens].astype(np.float64)
    y = np.asarray([x[i, :s, 0].sum() - x[i, :s, 1].mean() for i, s in enumerate(seqlen)]) + 3.0 + 0.05 * rng.standard_normal(N)
    ds = build_regression_dataset(tokens, y * 2.5, seqlen, chunk_size=25, device=DEV, token_table=table)
    settings = {"averaging": "sqrt", "intercept": True, "conv_width": CW}
    if kernel_choice == "Conv1dTwoLayer":
        settings.update(averaging="none", init_rffs=32)
    model = xGPRegression(num_rffs=64, variance_rffs=NVAR, kernel_choice=kernel_choice, device=DEV, verbose=False, kernel_settings=settings)
    model.set_hyperparams(np.log(np.asarray([0.3, 0.6])), ds)
    model.fit(ds, mode="exact")
    return model, seqlen, tokens, table


@pytest.fixture(scope="module", params=["Conv1dRBF", "Conv1dTwoLayer"])
def fitted(request):
    return _fit(request.param)


def _written_out(tokens, seqlen, i, edits):
    """The mutants of sequence i as token rows of L + 1 positions -> (rows, lengths)."""
    rows, lens = np.zeros((len(edits), L_ + 1), dtype=np.int64), []
    for j, (kind, pos, tok) in enumerate(edits):
        t = list(tokens[i, :seqlen[i]])
        t = t[:pos] + [tok] + t[pos + 1:] if kind == "substitution" else t[:pos] + t[pos + 1:] if kind == "deletion" else t[:pos] + [tok] + t[pos:]
        rows[j, :len(t)] = t
        lens.append(len(t))
    return rows, np.asarray(lens, dtype=np.int32)


def test_the_neighbourhood_against_predict(fitted):
    """variance() + noise is ``predict_single_edits(get_var=True)``; the mean is its mean plus ``predict``; the covariance of chosen edits
    is std^2 lambda^2 z_a^T var z_b of the written-out mutants' features; ``sample_single_edits`` is mean + factor eps for the same seed.

    Bounds.  With Z2 >= |z'|_2^2 for every mutant (Conv1dRBF: 1 + F (r' nk')^2; the two-layer kernel's rows are RBF features: 2), the
    factor F of var comes from a symmetric eigendecomposition, backward stable to  E = 16 nvar^2 u64 |var|_F  in norm (negative
    eigenvalues of the positive definite var are rounding of that size), so quadratic and bilinear forms move by at most  E Z2.  Their
    float64 evaluation: an nvar^2-term sum in any order carries (nvar^2 + nvar + 2) u64 times the sum of its terms' magnitudes, and the
    variance scan evaluates the form as q + 2 r' delta.u + r'^2 delta^T var delta with |r' delta|_2 <= |z'|_2 + |b|_2 <= 2 sqrt(Z2), terms of
    at most (1 + 4 + 4) |var|_F Z2 together; both sides: 18 (nvar^2 + nvar + 2) u64 |var|_F Z2.  The VARIANCE needs no more than that: both
    routes form the mutant's columns from the same float32 rows and the same delta bits.  The COVARIANCE is held against the float64
    features of the written-out mutants (Conv1dRBF: another route to the columns): each column within cz (dense_reference.cap_features
    at the mutant's normaliser) of exact on either side, so a form moves by  cz sqrt(nvar) |var|_2 (2 sqrt(Z2) + cz sqrt(nvar))  per route;
    the two-layer kernel's two routes share the pooled rows and the second layer.  The draws: the two routes multiply the same columns
    with F eps and with F, then eps: 4 (nvar + 2) u64 on terms bounded by 3 sqrt(Z2) |F|_F |eps_k|_2."""
    from xgpr_amd.acquisition import standard_normal
    from xgpr_amd.kernels import Conv1dTwoLayerKernel
    model, seqlen, tokens, table = fitted
    k = model.kernel
    two = type(k) is Conv1dTwoLayerKernel
    std, lam = float(model.trainy_std), float(k.get_lambda())
    scale = std ** 2 * lam ** 2
    var = model.var.cpu().numpy()
    vf, v2 = float(np.linalg.norm(var)), float(np.linalg.norm(var, 2))
    rows3 = slice(0, 3)
    edits = model.predict_single_edits(tokens[rows3], seqlen[rows3], token_table=table, get_var=True)
    own = model.predict(tokens[rows3], seqlen[rows3], token_table=table)
    draws = model.sample_single_edits(tokens[rows3], seqlen[rows3], token_table=table, n_samples=4, random_seed=77)
    eps = standard_normal(NVAR, 4, 77).numpy()
    nbs = list(model.single_edit_neighbourhoods(tokens[rows3], seqlen[rows3], token_table=table))
    assert len(nbs) == 3
    if two:
        Z2, route = 2.0, 0.0
    else:
        F = k.num_freqs
        nkm = L_ - CW + 2
        rmax = float(dis._r(F, nkm, k.scaling_type))
        Z2 = 1.0 + F * (rmax * nkm) ** 2
        P = dr.padded_width(CW * C_)
        norm = float(np.sqrt(CW) * dr.max_row_norm((table.astype(np.float64) * float(k.hyperparams[1])).astype(np.float32)))
        cz = max(dr.cap_features(np.float32, P, norm, float(k.chi_arr.abs().max()), float(dis._r(F, m, k.scaling_type)), nk=m, u_out=dr.U32)
                 for m in range(1, nkm + 1))
        route = 2 * cz * np.sqrt(NVAR) * v2 * (2 * np.sqrt(Z2) + cz * np.sqrt(NVAR))
    form = (16 * NVAR ** 2 + 18 * (NVAR ** 2 + NVAR + 2)) * U64 * vf * Z2
    fnorm = float(np.linalg.norm(model._factor_of_var().cpu().numpy()))
    for i, nb in enumerate(nbs):
        s = int(seqlen[i])
        assert len(nb) == L_ * V_ + L_ + (L_ + 1) * V_ and nb.factor.shape == (len(nb), NVAR) and abs(nb.noise - scale) <= 4 * U64 * scale
        flat = lambda key: np.concatenate([edits["substitutions" + key][i].reshape(-1), edits["deletions" + key][i].reshape(-1),
                                           edits["insertions" + key][i].reshape(-1)])
        valid = nb.valid.cpu().numpy()
        want_valid = np.array([(kind == "substitution" and pos < s and tok != tokens[i, pos]) or (kind == "deletion" and pos < s and s > CW)
                               or (kind == "insertion" and pos <= s) for kind, pos, tok in map(nb.unravel, range(len(nb)))])
        assert np.array_equal(valid, want_valid)
        mean, pvar = nb.mean.cpu().numpy(), flat("_var")
        assert float(np.abs(mean - (flat("") + own[i]))[valid].max()) <= 8 * U64 * (abs(own[i]) + float(np.abs(flat(""))[valid].max()))
        got = nb.variance().cpu().numpy() + nb.noise
        err = float(np.abs(got - pvar)[valid].max())
        print(f"EDITPROJ model var     {model.kernel_choice:<16} seq {i}: |variance() + noise - predict_single_edits| {err:.3e}  bound {scale * form:.3e}"
              f"  ratio {err / (scale * form):.4f}")
        assert err <= scale * form
        # the covariance of chosen edits against the features of the written-out mutants
        pick = np.flatnonzero(valid)[:: max(1, int(valid.sum()) // 6)][:6]
        rows, lens = _written_out(tokens, seqlen, i, [nb.unravel(j) for j in pick])
        from xgpr_amd.models import token_input
        z = k.transform_x(token_input(rows, table, DEV), lens)[:, :NVAR].to(F64).cpu().numpy()
        dense = scale * (z @ var @ z.T)
        cov = nb.covariance(torch.from_numpy(pick).to(nb.factor.device)).cpu().numpy()
        err = float(np.abs(cov - dense).max())
        print(f"EDITPROJ model cov     {model.kernel_choice:<16} seq {i}: |covariance - z_a var z_b| {err:.3e}  bound {scale * (form + route):.3e}"
              f"  ratio {err / (scale * (form + route)):.4f}")
        assert err <= scale * (form + route)
        # the draws
        mine = nb.sample(4, random_seed=77).cpu().numpy()
        theirs = np.concatenate([draws[nm][i].reshape(-1, 4) for nm in ("substitutions", "deletions", "insertions")])
        assert np.array_equal(np.isnan(mine), np.isnan(theirs))
        ok = ~np.isnan(mine)
        bound = std * lam * 4 * (NVAR + 2) * U64 * 3 * np.sqrt(Z2) * fnorm * np.linalg.norm(eps, axis=0) + 8 * U64 * float(np.abs(mine[ok]).max())
        err = np.where(ok, np.abs(mine - theirs), 0.0).max(axis=0)
        print(f"EDITPROJ model draws   {model.kernel_choice:<16} seq {i}: largest |sample - sample_single_edits| / bound {float((err / bound).max()):.4f}")
        assert (err <= bound).all()
    # a plate: never an invalid edit, never one twice, and not the marginal top-B where that holds near-duplicates
    plates = model.select_single_edit_batch(tokens[rows3], seqlen[rows3], token_table=table, batch_size=6)
    for i, plate in enumerate(plates):
        valid = nbs[i].valid.cpu().numpy()
        assert len(plate) == 6 and len({p["index"] for p in plate}) == 6 and all(valid[p["index"]] for p in plate)
        assert plate == nbs[i].select_batch(6)


def test_the_neighbourhood_s_factor_against_the_dense_reference():
    """Conv1dRBF: the factor rows of sequence 0 .. 2 are amp times the reference projection on the model's own factor of var, within
    the operator's cap fed from float32 rows."""
    model, seqlen, tokens, table = _fit("Conv1dRBF")
    k = model.kernel
    amp = float(model.trainy_std) * float(k.get_lambda())
    pm = model._factor_of_var().cpu().numpy()
    scaled = (table.astype(np.float64) * float(k.hyperparams[1])).astype(np.float32)
    c = dict(tokens=tokens[:3].astype(np.uint8), table=scaled, seqlen=seqlen[:3], radem=k.radem_diag.cpu().numpy(), chi=k.chi_arr.cpu().numpy())
    args = (k.conv_width, k.scaling_type, k.fit_intercept)
    z = dv.exact_rows(c, NVAR, *args)
    rs, b = dep.subst_proj(c, pm, *args, z=z)
    rd, ri, bd, bi = dep.indel_proj(c, pm, *args, z=z)
    caps = (dep.cap_subst(c, pm, b, *args, carried=True, z=z),) + dep.cap_indel(c, pm, bd, bi, *args, carried=True, z=z)
    zd, zi = _zeros(c)
    for i, nb in enumerate(model.single_edit_neighbourhoods(tokens[:3], seqlen[:3], token_table=table)):
        f = nb.factor.cpu().numpy() / amp
        parts = np.split(f, [L_ * V_, L_ * V_ + L_])
        for which, got, ref, cap, zeros in (("sub", parts[0].reshape(1, L_, V_, NVAR), rs, caps[0], zd),
                                            ("del", parts[1].reshape(1, L_, NVAR), rd, caps[1], zd),
                                            ("ins", parts[2].reshape(1, L_ + 1, V_, NVAR), ri, caps[2], zi)):
            report("model " + which, ("Conv1dRBF", i), got, ref[i:i + 1], cap[i:i + 1] + 4 * U64 * np.abs(np.nan_to_num(np.asarray(ref[i:i + 1], dtype=np.float64))).max(),
                   zeros[i:i + 1])
