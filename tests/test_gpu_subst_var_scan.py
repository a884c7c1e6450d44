"""The substitution variance scan of the sequence / graph kernels on the device (xgpr_conv_token_subst_var_scan_f32,
ConvSORFKernel.substitution_variance_scan / substitution_variance_scan_composed, xGPRegression.predict_substitutions(get_var=True))
against the long-double dense reference of tests/dense_subst_var_scan.py, within its a-priori cap ``cap_var_scan`` (derived from the
operation count; tests/test_subst_var_scan_host.py holds the cap to 1e-2 of every case's largest |Q - q_i| and shows what it
separates) -- or bit for bit where a test says so.  No element is excused.  Every comparison prints one ``SUBSTVAR`` line with measured
error and cap; profiles/subst_var_scan_errors.txt is the collection of those lines from one run."""
import ctypes

import numpy as np
import pytest
import torch

import dense_reference as dr
import dense_subst_var_scan as dv
from guarded import same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
CASE_NAMES = [c[0] for c in dv.CASES]


@pytest.fixture(scope="module")
def ext():
    from xgpr_amd import xgpr_hip_rfgen_ext as e
    return e


def _vm(k):
    """Vm on the device, its rows strided where the case says so (NaN behind every row)."""
    full = np.full((k["nvar"], k["nvar"] + k["pad"]), np.nan)
    full[:, :k["nvar"]] = k["vm"]
    return torch.from_numpy(full).to(DEV)[:, :k["nvar"]]


def run_operator(ext, k, rows=None, slab_rows=0):
    """The ext call on the case's sequences (``rows``: a subset, in that order) with the exact u, q rounded to float64; the output
    starts as NaN."""
    c = k["c"]
    rows = np.arange(c["tokens"].shape[0]) if rows is None else np.asarray(rows)
    tokens = np.ascontiguousarray(c["tokens"][rows])
    out = torch.full((tokens.shape[0], tokens.shape[1], c["table"].shape[0]), float("nan"), dtype=F64, device=DEV)
    ext.hipConvTokenSubstVarScan(torch.from_numpy(tokens).to(DEV), torch.from_numpy(c["table"]).to(DEV), _vm(k),
                                 torch.from_numpy(np.ascontiguousarray(k["u64"][rows])).to(DEV),
                                 torch.from_numpy(np.ascontiguousarray(k["q64"][rows])).to(DEV), out,
                                 torch.from_numpy(c["radem"]).to(DEV), torch.from_numpy(c["chi"]).to(DEV),
                                 np.ascontiguousarray(c["seqlen"][rows]), k["cw"], k["scaling"], k["icpt"], slab_rows=slab_rows)
    return out


def report(tag, case, got, ref, cap):
    err = float(np.abs(got.astype(dr.LD) - ref).max()) if ref.size else 0.0
    print(f"SUBSTVAR {tag:<10} {str(case):<40} hip-dense {err:.3e}  cap {cap:.3e}  ratio {err / cap:.4f}  max|ref| {float(np.abs(ref).max()):.3e}")
    return err


def exact_entries(got, tokens, seqlen, q64):
    """q_i, bitwise, at every sequence's own token, and +0.0, bitwise, at every position past its length."""
    for i, s in enumerate(seqlen):
        own = got[i, np.arange(s), tokens[i, :s]]
        if own.tobytes() != np.full(s, q64[i]).tobytes():
            return False
        tail = got[i, s:]
        if (tail != 0).any() or np.signbit(tail).any():
            return False
    return True


@pytest.mark.parametrize("name", CASE_NAMES)
def test_operator_against_the_dense_reference(ext, name):
    k = dv.case(name)
    c = k["c"]
    out = run_operator(ext, k)
    got = out.cpu().numpy()
    assert report("operator", (name, k["nvar"]), got, k["ref"], k["cap"]) <= k["cap"]
    assert dv.check(got, k["ref"], k["cap"]) <= k["cap"]
    assert exact_entries(got, c["tokens"], c["seqlen"], k["q64"])
    assert same_bits(out, run_operator(ext, k)), "two runs differ"


def test_two_identical_table_rows_give_bit_equal_columns(ext):
    k = dv.case("dup_rows")
    assert (k["c"]["table"][1] == k["c"]["table"][3]).all()
    out = run_operator(ext, k)
    assert same_bits(out[:, :, 1].contiguous(), out[:, :, 3].contiguous())
    assert not same_bits(out[:, :, 1].contiguous(), out[:, :, 2].contiguous())


@pytest.mark.parametrize("name", ["n65", "w256_c21_cw9", "w128_c21_cw6"])
def test_the_slab_size_does_not_enter(ext, name):
    """slab_rows = 16: many slabs, slab edges inside a position's V rows (V = 3, 7, 21), the last row tile not full; 48: three tiles."""
    k = dv.case(name)
    whole = run_operator(ext, k)
    for slab in (16, 48):
        assert same_bits(run_operator(ext, k, slab_rows=slab), whole), slab


@pytest.mark.parametrize("name", ["w256_c21_cw9", "w1024_c21_cw48", "n65"])
def test_a_sequence_alone_and_inside_a_batch(ext, name):
    k = dv.case(name)
    n = k["c"]["tokens"].shape[0]
    whole = run_operator(ext, k)
    for i in sorted({0, n // 2, n - 1}):
        assert same_bits(run_operator(ext, k, rows=[i])[0], whole[i]), i
    back = run_operator(ext, k, rows=np.arange(n)[::-1])      # every sequence at another index
    assert same_bits(back.flip(0).contiguous(), whole)


# ------------------------------------------------------------------------------------------------ validation on the device
def test_every_refusal_launches_nothing(ext):
    """The refusals of the header, in its order, with real device arrays: the error is raised and ``out`` keeps its bits."""
    from xgpr_amd import _lib
    import test_subst_var_scan_host as host
    k = dv.case("w16_c4_cw3")
    c, nvar = k["c"], k["nvar"]
    n, L = c["tokens"].shape
    V, C = c["table"].shape
    F, R = c["chi"].shape[0], c["radem"].shape[2]
    dev = {key: torch.from_numpy(c[key]).to(DEV) for key in ("tokens", "table", "radem", "chi")}
    vm, u, q = torch.from_numpy(k["vm"]).to(DEV), torch.from_numpy(k["u64"]).to(DEV), torch.from_numpy(k["q64"]).to(DEV)
    lens_dev = torch.from_numpy(c["seqlen"]).to(DEV)
    out = torch.full((n, L, V), float("nan"), dtype=F64, device=DEV)
    before = out.clone()
    ws = torch.empty(ext.conv_token_subst_var_scan_workspace_bytes(R, nvar, 0), dtype=torch.uint8, device=DEV)
    codes = host._codes()

    def call(**kw):
        a = dict(n=n, L=L, vocab=V, C=C, F=F, R=R, nvar=nvar, stride=nvar, cw=k["cw"], scaling=k["scaling"], slab=0, lens=c["seqlen"],
                 ws=ws.data_ptr(), wb=ws.numel(), out=out.data_ptr(), vm=vm.data_ptr())
        a.update(kw)
        lens = np.ascontiguousarray(a["lens"], dtype=np.int32)
        rc = _lib.load().xgpr_conv_token_subst_var_scan_f32(
            dev["tokens"].data_ptr(), dev["table"].data_ptr(), a["vm"], a["stride"], u.data_ptr(), q.data_ptr(), a["out"],
            dev["radem"].data_ptr(), dev["chi"].data_ptr(), ctypes.c_void_p(lens.ctypes.data), lens_dev.data_ptr(), a["n"], a["L"],
            a["vocab"], a["C"], a["F"], a["R"], a["nvar"], a["cw"], a["scaling"], int(k["icpt"]), a["slab"], a["ws"], a["wb"], None)
        torch.cuda.synchronize()
        return int(rc)

    ordered = [(dict(n=-1), "ARRAY_DIMS"), (dict(scaling=3), "ARRAY_DIMS"), (dict(cw=L + 1), "CONV_WIDTH"), (dict(F=R + 1), "RFFS_FREQS"),
               (dict(nvar=nvar - 1), "ARRAY_DIMS"), (dict(nvar=2 * F + 2), "ARRAY_DIMS"), (dict(stride=nvar - 2), "ARRAY_SIZES"),
               (dict(slab=24), "ARRAY_DIMS"), (dict(lens=[L + 1] * n), "SEQLEN_RANGE"), (dict(vocab=257), "ARRAY_DIMS"),
               (dict(vocab=256, C=19, R=64), "UNSUPPORTED"), (dict(wb=ws.numel() - 1), "WORKSPACE"), (dict(ws=None), "WORKSPACE"),
               (dict(vm=None), "WORKSPACE"), (dict(out=None), "WORKSPACE")]
    for kw, code in ordered:
        assert call(**kw) == codes[code], (kw, _lib.last_error())
        assert same_bits(out, before), kw
    for (kw0, code0), (kw1, _) in zip(ordered[:-3], ordered[1:-2]):          # two at once: the earlier one in the order is reported
        if set(kw0) & set(kw1):
            continue
        assert call(**kw0, **kw1) == codes[code0], (kw0, kw1)
        assert same_bits(out, before)
    assert call() == 0                                                       # ... and the unchanged call runs
    assert not same_bits(out, before) and bool(torch.isfinite(out).all())


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
    """(dense reference, cap of the operator route fed from float32 rows, cap of the written-out route)."""
    vp = _padded(vm)
    ref, q, u, z = dv.var_scan(c, vp, k.conv_width, k.scaling_type, k.fit_intercept)
    cap = dv.cap_var_scan(c, vp, np.asarray(u, dtype=np.float64), np.asarray(q, dtype=np.float64), k.conv_width, k.scaling_type,
                          k.fit_intercept, carried=True, z=z)
    return ref, cap, dv.cap_written_out(c, vp, k.conv_width, k.scaling_type, k.fit_intercept)


@pytest.mark.parametrize("choice,averaging,nvar", [("Conv1dRBF", "sqrt", 32), ("Conv1dMatern", "full", 15), ("GraphRBF", "full", 64),
                                                   ("Conv1dCauchy", "none", 130)])
def test_kernel_scan_against_the_composed_route(ext, choice, averaging, nvar):
    from xgpr_amd.dataset import TokenBatch
    n, L, C, cw, M, V = 4, 9, 6, 4, 600, 5
    k = _kernel(choice, n, L, C, cw, M, averaging=averaging)
    table, c = _kernel_case(k, n, L, V, 41, (9, 4, 6, 8) if k.conv_width > 1 else (9, 1, 6, 8))
    vm = dv.make_vm(nvar, seed=3)
    batch = TokenBatch(torch.from_numpy(c["tokens"]).to(DEV), torch.from_numpy(table).to(DEV))
    got = k.substitution_variance_scan(batch, c["seqlen"], vm)
    assert got.dtype == F64 and tuple(got.shape) == (n, L, V) and got.is_cuda
    k.COMPOSED_SCAN_ELEMS = 37 * M                               # several slices, the last one ragged
    fb = k.substitution_variance_scan_composed(batch, c["seqlen"], torch.from_numpy(vm).to(DEV))
    ref, cap, ccap = _route_caps(k, c, vm)
    tag = (choice, averaging, nvar)
    e1, e2 = report("kernel", tag, got.cpu().numpy(), ref, cap), report("composed", tag, fb.cpu().numpy(), ref, ccap)
    assert e1 <= cap and e2 <= ccap
    assert float((got - fb).abs().max()) <= cap + ccap
    past = np.arange(L)[None, :] >= c["seqlen"][:, None]
    assert (got.cpu().numpy()[past] == 0).all() and (fb.cpu().numpy()[past] == 0).all()
    # tokens that are not contiguous take the composed route
    wide = torch.from_numpy(np.concatenate([c["tokens"], c["tokens"]], axis=1)).to(DEV)
    assert not wide[:, :L].is_contiguous()
    again = k.substitution_variance_scan(TokenBatch(wide[:, :L], batch.table), c["seqlen"], vm)
    assert same_bits(again, fb)
    with pytest.raises(RuntimeError, match="TokenBatch"):
        k.substitution_variance_scan(table[c["tokens"]], c["seqlen"], vm)
    with pytest.raises(RuntimeError, match="square matrix"):
        k.substitution_variance_scan(batch, c["seqlen"], vm[:, :-1])


def test_beyond_the_operator_the_kernel_object_takes_the_composed_route(ext):
    """nvar above one tile: the predicate is 0, the ext call refuses and writes nothing, the kernel object still answers."""
    from xgpr_amd.dataset import TokenBatch
    n, L, C, cw, M, V = 2, 6, 4, 3, 4200, 3
    k = _kernel("Conv1dRBF", n, L, C, cw, M, icpt=False)
    table, c = _kernel_case(k, n, L, V, 43, (6, 4))
    nvar = 2050
    assert ext.conv_token_subst_var_scan_ok(cw * C, V, C, M // 2, nvar) == 0 and ext.conv_token_subst_var_scan_ok(cw * C, V, C, M // 2, 2048) == 1
    rng = np.random.default_rng(44)
    vm = np.diag(rng.uniform(0.75, 1.25, size=nvar))
    vm[0, nvar - 1] = vm[nvar - 1, 0] = 0.25
    out = torch.zeros((n, L, V), dtype=F64, device=DEV)
    with pytest.raises(RuntimeError, match="nvar <= 2048"):
        ext.hipConvTokenSubstVarScan(torch.from_numpy(c["tokens"]).to(DEV), torch.from_numpy(c["table"]).to(DEV), torch.from_numpy(vm).to(DEV),
                                     torch.zeros((n, nvar), dtype=F64, device=DEV), torch.zeros(n, dtype=F64, device=DEV), out, k.radem_diag,
                                     k.chi_arr, c["seqlen"], cw, k.scaling_type, False)
    assert float(out.abs().max()) == 0.0
    batch = TokenBatch(torch.from_numpy(c["tokens"]).to(DEV), torch.from_numpy(table).to(DEV))
    got = k.substitution_variance_scan(batch, c["seqlen"], vm).cpu().numpy()
    ref = dv.var_scan(c, vm, cw, k.scaling_type, False)[0]
    ccap = dv.cap_written_out(c, vm, cw, k.scaling_type, False)
    assert report("composed", ("nvar", nvar), got, ref, ccap) <= ccap


# ------------------------------------------------------------------------------------------------ predict_substitutions(get_var=True)
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


def test_predict_substitutions_with_variance(fitted):
    model, _, seqlen, tokens, table = fitted
    k = model.kernel
    std, lam = float(model.trainy_std), float(k.get_lambda())
    mean_only = model.predict_substitutions(tokens, sequence_lengths=seqlen, token_table=table, chunk_size=16)
    scan, var = model.predict_substitutions(tokens, sequence_lengths=seqlen, token_table=table, chunk_size=16, get_var=True)
    assert scan.tobytes() == mean_only.tobytes() and scan.shape == mean_only.shape             # the mean half: the get_var=False call
    assert isinstance(var, np.ndarray) and var.dtype == np.float64 and var.shape == (N, L_, V_)
    assert (var >= 0).all() and (var[np.arange(L_)[None, :] >= seqlen[:, None]] == 0).all() and float(var.max()) > 0
    # all L V mutants of three sequences through predict(get_var=True)
    three = tokens[:3]
    mut = np.repeat(three, L_ * V_, axis=0).reshape(3, L_, V_, L_)
    for l in range(L_):
        mut[:, l, :, l] = np.arange(V_, dtype=np.uint8)[None, :]
    lens = np.repeat(seqlen[:3], L_ * V_)
    want = model.predict(mut.reshape(-1, L_), sequence_lengths=lens, token_table=table, get_var=True)[1].reshape(3, L_, V_)
    want[np.arange(L_)[None, :] >= seqlen[:3, None]] = 0.0
    own = model.predict(three, sequence_lengths=seqlen[:3], token_table=table, get_var=True)[1]
    scaled = (table.astype(np.float64) * float(k.hyperparams[1])).astype(np.float32)
    c = dict(tokens=three, table=scaled, seqlen=seqlen[:3], radem=k.radem_diag.cpu().numpy(), chi=k.chi_arr.cpu().numpy())
    vm = model.var.cpu().numpy()
    assert vm.shape == (16, 16)
    ref, cap, ccap = _route_caps(k, c, vm)
    bound = std ** 2 * lam ** 2 * (cap + ccap)                     # (max(0, .) moves two values no further apart)
    err = float(np.abs(var[:3] - want).max())
    print(f"SUBSTVAR model      {'scan - predict(get_var=True)':<40} diff {err:.3e}  bound {bound:.3e}  max|want| {float(np.abs(want).max()):.3e}"
          f"  spread {float(np.abs(want - own[:, None, None])[want != 0].max()):.3e}")
    assert err <= bound
    # ... and the dense reference itself, in the units of y^2
    dense = std ** 2 * np.maximum(0, lam ** 2 + lam ** 2 * ref)
    dense[np.arange(L_)[None, :] >= seqlen[:3, None]] = 0
    scale = std ** 2 * lam ** 2
    assert report("model", "predict_substitutions(get_var=True)", var[:3], dense, scale * cap) <= scale * cap + 4 * dr.U64 * float(dense.max())
    for i in range(3):                                             # the own token: the sequence's own variance
        s = int(seqlen[i])
        assert float(np.abs(var[i, np.arange(s), three[i, :s]] - own[i]).max()) <= bound


def test_predict_substitutions_without_a_variance(fitted):
    from xgpr_amd.models import xGPRegression
    model, ds, seqlen, tokens, table = fitted
    bare = xGPRegression(num_rffs=64, variance_rffs=16, kernel_choice="Conv1dRBF", device=DEV, verbose=False,
                         kernel_settings={"averaging": "sqrt", "intercept": True, "conv_width": CW})
    bare.set_hyperparams(np.log(np.asarray([0.3, 0.6])), ds)
    bare.fit(ds, mode="exact", suppress_var=True)
    with pytest.raises(RuntimeError, match="suppress_var"):
        bare.predict_substitutions(tokens[:3], sequence_lengths=seqlen[:3], token_table=table, get_var=True)
    got = bare.predict_substitutions(tokens[:3], sequence_lengths=seqlen[:3], token_table=table)      # the default call is untouched
    assert isinstance(got, np.ndarray) and got.shape == (3, L_, V_)
