"""The indel variance scan of the sequence / graph kernels on the device (xgpr_conv_token_indel_var_scan_f32,
ConvSORFKernel.indel_variance_scan / indel_variance_scan_composed, xGPRegression.predict_indels(get_var=True)) against the long-double
brute-force reference of tests/dense_indel_var_scan.py, within its a-priori caps ``cap_var_scan`` (derived from the operation count;
tests/test_indel_var_scan_host.py holds the caps to 1e-2 of every case's largest |Q - q~| and shows what they separate) -- or bit for
bit where a test says so.  No element is excused.  Every comparison prints one ``INDELVAR`` line with measured error and cap; the
first test leaves the largest ratio of the operator's comparisons in profiles/indel_var_scan_errors.txt."""
import ctypes
import os

import numpy as np
import pytest
import torch

import dense_indel_scan as dis
import dense_indel_var_scan as div
import dense_reference as dr
import dense_subst_var_scan as dv
from guarded import same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
CASE_NAMES = [c[0] for c in div.CASES]
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
RATIOS = {}


@pytest.fixture(scope="module")
def ext():
    from xgpr_amd import xgpr_hip_rfgen_ext as e
    return e


def _vm(k):
    """Vm on the device, its rows strided where the case says so (NaN behind every row)."""
    full = np.full((k["nvar"], k["nvar"] + k["pad"]), np.nan)
    full[:, :k["nvar"]] = k["vm"]
    return torch.from_numpy(full).to(DEV)[:, :k["nvar"]]


def run_operator(ext, k, rows=None, slab_rows=0, dele=True, ins=True):
    """The ext call on the case's sequences (``rows``: a subset, in that order) with the exact u~, q~ rounded to float64; the outputs
    start as NaN.  -> (del or None, ins or None)."""
    c = k["c"]
    rows = np.arange(c["tokens"].shape[0]) if rows is None else np.asarray(rows)
    tokens = np.ascontiguousarray(c["tokens"][rows])
    n, L = tokens.shape
    V = c["table"].shape[0]
    up = lambda key: torch.from_numpy(np.ascontiguousarray(k[key][rows])).to(DEV)
    od = torch.full((n, L), float("nan"), dtype=F64, device=DEV) if dele else None
    oi = torch.full((n, L + 1, V), float("nan"), dtype=F64, device=DEV) if ins else None
    ext.hipConvTokenIndelVarScan(torch.from_numpy(tokens).to(DEV), torch.from_numpy(c["table"]).to(DEV), _vm(k),
                                 up("u_del") if dele else None, up("q_del") if dele else None, up("u_ins") if ins else None,
                                 up("q_ins") if ins else None, od, oi, torch.from_numpy(c["radem"]).to(DEV),
                                 torch.from_numpy(c["chi"]).to(DEV), np.ascontiguousarray(c["seqlen"][rows]), k["cw"], k["scaling"], k["icpt"],
                                 slab_rows=slab_rows)
    return od, oi


def report(tag, case, got, ref, cap):
    ok = ~np.isnan(np.asarray(ref, dtype=np.float64))
    err = float(np.abs(got.astype(dr.LD) - ref)[ok].max()) if ok.any() else 0.0
    big = float(np.abs(ref[ok]).max()) if ok.any() else 0.0
    print(f"INDELVAR {tag:<12} {str(case):<44} hip-dense {err:.3e}  cap {cap:.3e}  ratio {err / cap:.4f}  max|ref| {big:.3e}")
    return err


def _zeros(c):
    L = c["tokens"].shape[1]
    return dis.zero_mask(c["seqlen"], L), dis.zero_mask(c["seqlen"], L, gaps=True)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_operator_against_the_dense_reference(ext, name):
    k = div.case(name)
    c = k["c"]
    od, oi = run_operator(ext, k)
    zd, zi = _zeros(c)
    for which, out, zeros in (("del", od, zd), ("ins", oi, zi)):
        got, ref, cap = out.cpu().numpy(), k["ref_" + which], k["cap_" + which]
        err = report("operator " + which, (name, k["nvar"]), got, ref, cap)
        RATIOS[(name, which)] = err / cap
        assert err <= cap
        assert div.check(got, ref, cap, zeros) <= cap                    # NaN exactly at the deletions of s == conv_width; +0.0 past a length
    ad, ai = run_operator(ext, k)
    assert same_bits(od, ad) and same_bits(oi, ai), "two runs differ"
    if len(RATIOS) == 2 * len(CASE_NAMES):                               # the whole list ran: leave the summary
        worst = max(RATIOS, key=RATIOS.get)
        lines = ["# tests/test_gpu_indel_var_scan.py: the operator against the long-double reference, measured error / a-priori cap\n"]
        lines += [f"{key[0]:<20} {key[1]}  ratio {RATIOS[key]:.4f}\n" for key in sorted(RATIOS)]
        lines.append(f"largest ratio {RATIOS[worst]:.4f} ({worst[0]}, {worst[1]})\n")
        try:                                                             # (results are bitwise reproducible: the same text every run)
            with open(os.path.join(ROOT, "profiles", "indel_var_scan_errors.txt"), "w") as f:
                f.writelines(lines)
        except OSError:                                                  # a read-only checkout: the INDELVAR lines above say the same
            pass


def test_zeros_and_nans_are_exact(ext):
    """+0.0 bitwise at p >= s and g > s; a quiet NaN at the deletions of the s == conv_width sequence and nowhere else."""
    for name in ("w256_c21_cw9", "graph_cw1", "dup_rows"):
        k = div.case(name)
        c = k["c"]
        od, oi = (t.cpu().numpy() for t in run_operator(ext, k))
        zd, zi = _zeros(c)
        assert od[zd].tobytes() == np.zeros(int(zd.sum())).tobytes() and oi[zi].tobytes() == np.zeros(int(zi.sum()) * oi.shape[2]).tobytes()
        L = c["tokens"].shape[1]
        want = (c["seqlen"][:, None] == k["cw"]) & (np.arange(L)[None, :] < c["seqlen"][:, None])
        assert want.any() and np.array_equal(np.isnan(od), want) and not np.isnan(oi).any()
        assert ((od[want].view(np.uint64) >> np.uint64(51)) & np.uint64(1)).all()          # quiet


def test_two_identical_table_rows_give_bit_equal_columns(ext):
    k = div.case("dup_rows")
    assert (k["c"]["table"][1] == k["c"]["table"][3]).all()
    _, oi = run_operator(ext, k)
    assert same_bits(oi[:, :, 1].contiguous(), oi[:, :, 3].contiguous())
    assert not same_bits(oi[:, :, 1].contiguous(), oi[:, :, 2].contiguous())


@pytest.mark.parametrize("name", ["n65", "w256_c21_cw9", "w128_c21_cw6"])
def test_the_slab_size_does_not_enter(ext, name):
    """slab_rows = 16: many slabs, slab edges inside a gap's V rows (V = 3, 7, 21), deletion row counts that are no multiple of 16
    (w128_c21_cw6: 42 rows), the last row tile not full; 48: three tiles, a cut inside a gap's 21 rows."""
    k = div.case(name)
    n, L = k["c"]["tokens"].shape
    if name == "w128_c21_cw6":
        assert (n * L) % 16 and 48 % k["c"]["table"].shape[0]
    wd, wi = run_operator(ext, k)
    for slab in (16, 48):
        sd, si = run_operator(ext, k, slab_rows=slab)
        assert same_bits(sd, wd) and same_bits(si, wi), slab


@pytest.mark.parametrize("name", ["w256_c21_cw9", "w1024_c21_cw48", "n65"])
def test_a_sequence_alone_and_inside_a_batch(ext, name):
    k = div.case(name)
    n = k["c"]["tokens"].shape[0]
    wd, wi = run_operator(ext, k)
    for i in sorted({0, 1 % n, n // 2, n - 1}):
        ad, ai = run_operator(ext, k, rows=[i])
        assert same_bits(ad[0], wd[i]) and same_bits(ai[0], wi[i]), i
    bd, bi = run_operator(ext, k, rows=np.arange(n)[::-1])      # every sequence at another index
    assert same_bits(bd.flip(0).contiguous(), wd) and same_bits(bi.flip(0).contiguous(), wi)


@pytest.mark.parametrize("name", ["w128_c21_cw6", "graph_cw1", "n65"])
def test_one_output_alone_and_both_together(ext, name):
    k = div.case(name)
    wd, wi = run_operator(ext, k)
    od, none = run_operator(ext, k, ins=False)
    assert none is None and same_bits(od, wd)
    none, oi = run_operator(ext, k, dele=False)
    assert none is None and same_bits(oi, wi)


# ------------------------------------------------------------------------------------------------ validation on the device
def test_every_refusal_launches_nothing(ext):
    """The refusals of the header, in its order, with real device arrays: the error is returned and the outputs and the workspace keep
    their bits."""
    from xgpr_amd import _lib
    import test_subst_var_scan_host as host
    k = div.case("w16_c4_cw3")
    c, nvar = k["c"], k["nvar"]
    n, L = c["tokens"].shape
    V, C = c["table"].shape
    F, R = c["chi"].shape[0], c["radem"].shape[2]
    dev = {key: torch.from_numpy(c[key]).to(DEV) for key in ("tokens", "table", "radem", "chi")}
    vm = torch.from_numpy(k["vm"]).to(DEV)
    ops = {key: torch.from_numpy(k[key]).to(DEV) for key in ("u_del", "q_del", "u_ins", "q_ins")}
    lens_dev = torch.from_numpy(c["seqlen"]).to(DEV)
    od = torch.full((n, L), float("nan"), dtype=F64, device=DEV)
    oi = torch.full((n, L + 1, V), float("nan"), dtype=F64, device=DEV)
    ws = torch.full((ext.conv_token_indel_var_scan_workspace_bytes(R, nvar, 0),), 0xA5, dtype=torch.uint8, device=DEV)
    before = (od.clone(), oi.clone(), ws.clone())
    unchanged = lambda: same_bits(od, before[0]) and same_bits(oi, before[1]) and bool((ws == before[2]).all())
    codes = host._codes()

    def call(**kw):
        a = dict(n=n, L=L, vocab=V, C=C, F=F, R=R, nvar=nvar, stride=nvar, cw=k["cw"], scaling=k["scaling"], slab=0, lens=c["seqlen"],
                 ws=ws.data_ptr(), wb=ws.numel(), od=od.data_ptr(), oi=oi.data_ptr(), vm=vm.data_ptr(), ud=ops["u_del"].data_ptr(),
                 qd=ops["q_del"].data_ptr(), ui=ops["u_ins"].data_ptr(), qi=ops["q_ins"].data_ptr())
        a.update(kw)
        lens = np.ascontiguousarray(a["lens"], dtype=np.int32)
        rc = _lib.load().xgpr_conv_token_indel_var_scan_f32(
            dev["tokens"].data_ptr(), dev["table"].data_ptr(), a["vm"], a["stride"], a["ud"], a["qd"], a["ui"], a["qi"], a["od"], a["oi"],
            dev["radem"].data_ptr(), dev["chi"].data_ptr(), ctypes.c_void_p(lens.ctypes.data), lens_dev.data_ptr(), a["n"], a["L"],
            a["vocab"], a["C"], a["F"], a["R"], a["nvar"], a["cw"], a["scaling"], int(k["icpt"]), a["slab"], a["ws"], a["wb"], None)
        torch.cuda.synchronize()
        return int(rc)

    ordered = [(dict(n=-1), "ARRAY_DIMS"), (dict(scaling=3), "ARRAY_DIMS"), (dict(cw=L + 1), "CONV_WIDTH"), (dict(F=R + 1), "RFFS_FREQS"),
               (dict(nvar=nvar - 1), "ARRAY_DIMS"), (dict(nvar=2 * F + 2), "ARRAY_DIMS"), (dict(stride=nvar - 2), "ARRAY_SIZES"),
               (dict(slab=24), "ARRAY_DIMS"), (dict(lens=[L + 1] * n), "SEQLEN_RANGE"), (dict(vocab=257), "ARRAY_DIMS"),
               (dict(vocab=256, C=19, R=64), "UNSUPPORTED"), (dict(wb=ws.numel() - 1), "WORKSPACE"), (dict(ws=None), "WORKSPACE"),
               (dict(vm=None), "WORKSPACE"), (dict(od=None), "WORKSPACE"), (dict(qi=None), "WORKSPACE"),
               (dict(ud=None, qd=None, od=None, ui=None, qi=None, oi=None), "WORKSPACE")]
    for kw, code in ordered:
        assert call(**kw) == codes[code], (kw, _lib.last_error())
        assert unchanged(), kw
    for (kw0, code0), (kw1, _) in zip(ordered[:-5], ordered[1:-4]):          # two at once: the earlier one in the order is reported
        if set(kw0) & set(kw1):
            continue
        assert call(**kw0, **kw1) == codes[code0], (kw0, kw1)
        assert unchanged()
    assert call() == 0                                                       # ... and the unchanged call runs
    assert not same_bits(od, before[0]) and not same_bits(oi, before[1]) and bool(torch.isfinite(oi).all())


# ------------------------------------------------------------------------------------------------ the kernel object
def _kernel(choice, n, L, C, cw, M, icpt=True, averaging="sqrt"):
    from xgpr_amd.kernels import ConvSORFKernel
    k = ConvSORFKernel(choice, (n, L, C), M, 123, DEV, {"matern_nu": 5 / 2, "intercept": icpt, "conv_width": cw, "averaging": averaging})
    k.set_hyperparams(np.asarray([0.9, 2.1 / np.sqrt(C)]), logspace=False)
    return k


def _kernel_case(k, n, L, V, seed, lengths):
    """-> (unscaled table, case dict over the scaled table as KernelBase.scaled_f32 forms it)."""
    rng = np.random.default_rng(seed)
    C = k._xdim[2]
    table = rng.uniform(-1, 1, size=(V, C)).astype(np.float32)
    tokens = rng.integers(0, V, size=(n, L)).astype(np.uint8)
    seqlen = np.asarray([lengths[i % len(lengths)] for i in range(n)], dtype=np.int32)
    scaled = (table.astype(np.float64) * float(k.hyperparams[1])).astype(np.float32)
    return table, dict(tokens=tokens, table=scaled, seqlen=seqlen, radem=k.radem_diag.cpu().numpy(), chi=k.chi_arr.cpu().numpy())


def _padded(vm):
    """An odd-sized Vm with the zero row and column the kernel object adds."""
    nvar = vm.shape[0]
    out = np.zeros((nvar + (nvar & 1),) * 2)
    out[:nvar, :nvar] = vm
    return out


def _route_caps(k, c, vm):
    """(reference del, ins; caps of the operator route fed from float32 rows; caps of the written-out route)."""
    vp = _padded(vm)
    rd, ri = div.var_scan(c, vp, k.conv_width, k.scaling_type, k.fit_intercept)
    ops = div.operands(c, vp, k.conv_width, k.scaling_type, k.fit_intercept)
    caps = div.cap_var_scan(c, vp, ops, k.conv_width, k.scaling_type, k.fit_intercept, carried=True)
    return (rd, ri), caps, div.cap_written_out(c, vp, k.conv_width, k.scaling_type, k.fit_intercept)


@pytest.mark.parametrize("choice,averaging,nvar,symmetric", [("Conv1dRBF", "sqrt", 32, True), ("Conv1dMatern", "full", 15, True),
                                                             ("GraphRBF", "full", 64, False), ("Conv1dCauchy", "none", 130, False),
                                                             ("GraphMatern", "sqrt", 21, True)])
def test_kernel_scan_against_the_composed_route(ext, choice, averaging, nvar, symmetric):
    from xgpr_amd.dataset import TokenBatch
    n, L, C, cw, M, V = 4, 9, 6, 4, 600, 5
    k = _kernel(choice, n, L, C, cw, M, averaging=averaging)
    table, c = _kernel_case(k, n, L, V, 41, (9, 4, 6, 5) if k.conv_width > 1 else (9, 1, 6, 2))
    vm = dv.make_vm(nvar, seed=3)
    if not symmetric:
        vm = vm + np.triu(np.random.default_rng(7).uniform(-0.2, 0.2, size=vm.shape) / nvar, 1)
        assert (vm != vm.T).any()
    batch = TokenBatch(torch.from_numpy(c["tokens"]).to(DEV), torch.from_numpy(table).to(DEV))
    got = k.indel_variance_scan(batch, c["seqlen"], vm)
    assert all(g.dtype == F64 and g.is_cuda for g in got) and tuple(got[0].shape) == (n, L) and tuple(got[1].shape) == (n, L + 1, V)
    k.COMPOSED_SCAN_ELEMS = 37 * M                               # several slices, the last one ragged
    fb = k.indel_variance_scan_composed(batch, c["seqlen"], torch.from_numpy(vm).to(DEV))
    refs, caps, ccaps = _route_caps(k, c, vm)
    tag = (choice, averaging, nvar)
    for which, g, f, ref, cap, ccap, zeros in zip(("del", "ins"), got, fb, refs, caps, ccaps, _zeros(c)):
        g, f = g.cpu().numpy(), f.cpu().numpy()
        e1, e2 = report("kernel " + which, tag, g, ref, cap), report("composed " + which, tag, f, ref, ccap)
        assert e1 <= cap and e2 <= ccap
        assert div.check(g, ref, cap, zeros) <= cap and div.check(f, ref, ccap, zeros) <= ccap
        ok = ~np.isnan(g)
        assert float(np.abs(g - f)[ok].max()) <= cap + ccap
    # tokens that are not contiguous take the composed route
    wide = torch.from_numpy(np.concatenate([c["tokens"], c["tokens"]], axis=1)).to(DEV)
    assert not wide[:, :L].is_contiguous()
    again = k.indel_variance_scan(TokenBatch(wide[:, :L], batch.table), c["seqlen"], vm)
    assert same_bits(again[0], fb[0]) and same_bits(again[1], fb[1])
    with pytest.raises(RuntimeError, match="TokenBatch"):
        k.indel_variance_scan(table[c["tokens"]], c["seqlen"], vm)
    with pytest.raises(RuntimeError, match="square matrix"):
        k.indel_variance_scan(batch, c["seqlen"], vm[:, :-1])


def test_beyond_the_operator_the_kernel_object_takes_the_composed_route(ext):
    """nvar above one tile: the predicate is 0, the ext call refuses and writes nothing, the kernel object still answers."""
    from xgpr_amd.dataset import TokenBatch
    n, L, C, cw, M, V = 2, 6, 4, 3, 4200, 3
    k = _kernel("Conv1dRBF", n, L, C, cw, M, icpt=False)
    table, c = _kernel_case(k, n, L, V, 43, (6, 4))
    nvar = 2050
    assert ext.conv_token_indel_var_scan_ok(cw * C, V, C, M // 2, nvar) == 0 and ext.conv_token_indel_var_scan_ok(cw * C, V, C, M // 2, 2048) == 1
    rng = np.random.default_rng(44)
    vm = np.diag(rng.uniform(0.75, 1.25, size=nvar))
    vm[0, nvar - 1] = vm[nvar - 1, 0] = 0.25
    od, oi = torch.zeros((n, L), dtype=F64, device=DEV), torch.zeros((n, L + 1, V), dtype=F64, device=DEV)
    u, q = torch.zeros((n, nvar), dtype=F64, device=DEV), torch.zeros(n, dtype=F64, device=DEV)
    with pytest.raises(RuntimeError, match="nvar <= 2048"):
        ext.hipConvTokenIndelVarScan(torch.from_numpy(c["tokens"]).to(DEV), torch.from_numpy(c["table"]).to(DEV), torch.from_numpy(vm).to(DEV),
                                     u, q, u, q, od, oi, k.radem_diag, k.chi_arr, c["seqlen"], cw, k.scaling_type, False)
    assert float(od.abs().max()) == 0.0 and float(oi.abs().max()) == 0.0
    batch = TokenBatch(torch.from_numpy(c["tokens"]).to(DEV), torch.from_numpy(table).to(DEV))
    got = k.indel_variance_scan(batch, c["seqlen"], vm)
    refs = div.var_scan(c, vm, cw, k.scaling_type, False)
    ccaps = div.cap_written_out(c, vm, cw, k.scaling_type, False)
    for which, g, ref, ccap in zip(("del", "ins"), got, refs, ccaps):
        assert report("composed " + which, ("nvar", nvar), g.cpu().numpy(), ref, ccap) <= ccap


# ------------------------------------------------------------------------------------------------ predict_indels(get_var=True)
N, L_, C_, CW, V_ = 40, 12, 4, 3, 5


@pytest.fixture(scope="module")
def fitted():
    from xgpr_amd.dataset import build_regression_dataset
    from xgpr_amd.models import xGPRegression
    rng = np.random.default_rng(45)
    table = rng.uniform(-1, 1, size=(V_, C_)).astype(np.float32)
    tokens = rng.integers(0, V_, size=(N, L_)).astype(np.uint8)
    seqlen = rng.integers(CW, L_ + 1, size=N).astype(np.int32)
    seqlen[:3] = (L_, CW, 7)
    x = table[tokens].astype(np.float64)
    y = np.asarray([x[i, :s, 0].sum() - x[i, :s, 1].mean() for i, s in enumerate(seqlen)]) + 3.0 + 0.05 * rng.standard_normal(N)
    ds = build_regression_dataset(x, y * 2.5, sequence_lengths=seqlen, chunk_size=25, device=DEV)
    settings = {"averaging": "sqrt", "intercept": True, "conv_width": CW}
    model = xGPRegression(num_rffs=64, variance_rffs=16, kernel_choice="Conv1dRBF", device=DEV, verbose=False, kernel_settings=settings)
    model.set_hyperparams(np.log(np.asarray([0.3, 0.6])), ds)
    model.fit(ds, mode="exact")
    return model, ds, seqlen, tokens, table


def test_predict_indels_with_variance(fitted):
    model, _, seqlen, tokens, table = fitted
    k = model.kernel
    std, lam = float(model.trainy_std), float(k.get_lambda())
    mean_only = model.predict_indels(tokens, sequence_lengths=seqlen, token_table=table, chunk_size=16)
    dele, ins, vd, vi = model.predict_indels(tokens, sequence_lengths=seqlen, token_table=table, chunk_size=16, get_var=True)
    assert dele.tobytes() == mean_only[0].tobytes() and ins.tobytes() == mean_only[1].tobytes()          # the mean half: the default call
    assert vd.dtype == np.float64 and vd.shape == (N, L_) and vi.dtype == np.float64 and vi.shape == (N, L_ + 1, V_)
    zd, zi = dis.zero_mask(seqlen, L_), dis.zero_mask(seqlen, L_, gaps=True)
    assert (vd[zd] == 0).all() and (vi[zi] == 0).all() and np.array_equal(np.isnan(vd), np.isnan(dele)) and np.isnan(vd).any()
    assert not np.isnan(vi).any() and (vi >= 0).all() and (vd[~np.isnan(vd)] >= 0).all() and float(vi.max()) > 0
    # a handful of mutants of three sequences, written out by the test, through predict(get_var=True)
    scaled = (table.astype(np.float64) * float(k.hyperparams[1])).astype(np.float32)
    c = dict(tokens=tokens[:3], table=scaled, seqlen=seqlen[:3], radem=k.radem_diag.cpu().numpy(), chi=k.chi_arr.cpu().numpy())
    vm = model.var.cpu().numpy()
    assert vm.shape == (16, 16)
    _, caps, ccaps = _route_caps(k, c, vm)
    scale = std ** 2 * lam ** 2
    muts, lens, got = [], [], []
    for i, p in ((0, 0), (0, 5), (0, L_ - 1), (2, 3), (2, 6)):                     # deletions
        t = list(tokens[i, :seqlen[i]])
        muts.append(t[:p] + t[p + 1:])
        got.append((vd[i, p], caps[0] + ccaps[0]))
    for i, g, v in ((1, 0, 2), (1, CW, 4), (2, 7, 0), (2, 2, 3), (2, 0, 1)):       # insertions; (1, CW, .) and (2, 7, .) append
        t = list(tokens[i, :seqlen[i]])
        muts.append(t[:g] + [v] + t[g:])
        got.append((vi[i, g, v], caps[1] + ccaps[1]))
    width = max(len(m) for m in muts)
    assert width <= L_                                                             # (the appended full-length mutant needs L + 1: left to the dense reference)
    arr = np.zeros((len(muts), L_), dtype=np.uint8)
    for j, m in enumerate(muts):
        arr[j, :len(m)] = m
        lens.append(len(m))
    want = model.predict(arr, sequence_lengths=np.asarray(lens, dtype=np.int32), token_table=table, get_var=True)[1]
    for j, (value, bound) in enumerate(got):
        print(f"INDELVAR model        mutant {j}: scan {value:.6e}  predict(get_var=True) {want[j]:.6e}  bound {scale * bound:.3e}")
        assert abs(value - want[j]) <= scale * bound                               # (max(0, .) moves two values no further apart)
    # ... and the dense reference itself, in the units of y^2, on every entry of the three sequences
    refs, _, _ = _route_caps(k, c, vm)
    for which, var, ref, cap, zeros in (("del", vd[:3], refs[0], caps[0], zd[:3]), ("ins", vi[:3], refs[1], caps[1], zi[:3])):
        dense = std ** 2 * np.maximum(0, lam ** 2 + lam ** 2 * ref)
        dense[zeros] = 0
        ok = ~np.isnan(np.asarray(dense, dtype=np.float64))
        err = report("model " + which, "predict_indels(get_var=True)", var, dense, scale * cap)
        assert err <= scale * cap + 4 * dr.U64 * float(np.abs(dense[ok]).max())


def test_predict_indels_without_a_variance(fitted):
    from xgpr_amd.models import xGPRegression
    model, ds, seqlen, tokens, table = fitted
    bare = xGPRegression(num_rffs=64, variance_rffs=16, kernel_choice="Conv1dRBF", device=DEV, verbose=False,
                         kernel_settings={"averaging": "sqrt", "intercept": True, "conv_width": CW})
    bare.set_hyperparams(np.log(np.asarray([0.3, 0.6])), ds)
    bare.fit(ds, mode="exact", suppress_var=True)
    with pytest.raises(RuntimeError, match="suppress_var"):
        bare.predict_indels(tokens[:3], sequence_lengths=seqlen[:3], token_table=table, get_var=True)
    got = bare.predict_indels(tokens[:3], sequence_lengths=seqlen[:3], token_table=table)      # the default call is untouched
    assert isinstance(got, tuple) and len(got) == 2 and got[0].shape == (3, L_) and got[1].shape == (3, L_ + 1, V_)
