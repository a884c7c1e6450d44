"""The combinatorial site scan of the sequence / graph kernels on the device (xgpr_conv_token_site_scan_f32, ConvSORFKernel.site_scan /
site_scan_composed, xGPRegression.predict_site_library) against the long-double references of tests/dense_site_scan.py: every run
table against ``run_tables`` within its run's a-priori cap, and -- what the tables are for -- the sum of one entry per run for EVERY
assignment of the sites against ``full_scan``, which writes every variant out and knows nothing of runs, within the cap of a full
assignment (``cap_site_scan``, derived from the operation count; tests/test_site_scan_host.py holds the caps to 1e-2 of every case's
largest output and shows what they separate) -- or bit for bit where a test says so.  No element is excused.  Every comparison prints
one ``SITE`` line with measured error, cap and ratio."""
import functools

import numpy as np
import pytest
import torch

import dense_pair_scan as dp
import dense_reference as dr
import dense_site_scan as ds
import dense_subst_scan as dss
from dense_reference import LD, U32
from guarded import same_bits
from test_gpu_subst_scan import _fit, _kernel, _kernel_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64


@pytest.fixture(scope="module")
def ext():
    from xgpr_amd import xgpr_hip_rfgen_ext as e
    return e


@functools.lru_cache(maxsize=None)
def reference(name):
    """(operands, sites, conv_width, scaling, intercept, runs, run tables, run caps, full cap, full reference) of a case: computed
    once, shared, left unchanged."""
    got = ds.reference(name) + (ds.full_reference(name),)
    for a in got[6] + [got[9]]:
        a.setflags(write=False)
    return got


def run_operator(ext, c, sites, cw, scaling, icpt, rows=None):
    """The ext call on the case's sequences (``rows``: a subset, in that order); the output starts as NaN."""
    rows = np.arange(c["tokens"].shape[0]) if rows is None else np.asarray(rows)
    tokens = np.ascontiguousarray(c["tokens"][rows])
    V = c["table"].shape[0]
    T = ds.run_offsets(ds.site_runs(sites, tokens.shape[1], cw), V)[1]
    out = torch.full((tokens.shape[0], T), float("nan"), dtype=F64, device=DEV)
    ext.hipConvTokenSiteScan(torch.from_numpy(tokens).to(DEV), torch.from_numpy(c["table"]).to(DEV), torch.from_numpy(c["w"]).to(DEV), out,
                             torch.from_numpy(c["radem"]).to(DEV), torch.from_numpy(c["chi"]).to(DEV),
                             np.ascontiguousarray(c["seqlen"][rows]), sites, cw, scaling, icpt)
    return out


def split(out, runs, V):
    """The operator's rows [n, T] -> one array [n, V^g] per run."""
    offs, T = ds.run_offsets(runs, V)
    assert out.shape[1] == T
    return [out[:, o:o + V ** r[3]] for o, r in zip(offs, runs)]


def report(tag, case, got, ref, cap):
    err = float(np.abs(np.asarray(got, dtype=LD) - ref).max()) if ref.size else 0.0
    big = float(np.abs(ref).max()) if ref.size else 0.0
    print(f"SITE {tag:<10} {str(case):<44} hip-dense {err:.3e}  cap {cap:.3e}  ratio {err / cap:.4f}  max|ref| {big:.3e}")
    return err


def own_index(tokens, pos, V):
    idx = 0
    for p in pos:
        idx = idx * V + int(tokens[p])
    return idx


def exact_zeros(tables, runs, sites, tokens, seqlen, cw):
    """+0.0, bitwise, at the own assignment of every run of every sequence, and in the whole table of a run that has no window
    inside the sequence."""
    V = round(tables[0].shape[1] ** (1.0 / runs[0][3]))
    for (jlo, _, a, g), tb in zip(runs, tables):
        for i in range(tb.shape[0]):
            z = tb[i] if jlo > int(seqlen[i]) - cw else tb[i, own_index(tokens[i], sites[a:a + g], V):][:1]
            if (z != 0).any() or np.signbit(z).any():
                return False
    return True


@pytest.mark.parametrize("name", [c[0] for c in ds.CASES])
def test_operator_against_the_dense_reference(ext, name):
    c, sites, cw, scaling, icpt, runs, tables, caps, total, full = reference(name)
    V, K = c["table"].shape[0], len(sites)
    out = run_operator(ext, c, sites, cw, scaling, icpt)        # (pre-filled with NaN: overwritten as a whole)
    got = split(out.cpu().numpy(), runs, V)
    for q, (tb, ref) in enumerate(zip(got, tables)):            # every run's table ...
        assert report(f"run {q}", name, tb, ref, caps[q]) <= caps[q]
        assert ds.check(tb, ref, caps[q]) <= caps[q]
    summed = ds.gather_full(runs, got, V, K)                    # ... and every variant against the definition
    assert report("library", name, summed, full, total) <= total
    assert ds.check(summed, full, total) <= total
    assert exact_zeros(got, runs, sites, c["tokens"], c["seqlen"], cw)
    assert same_bits(out, run_operator(ext, c, sites, cw, scaling, icpt)), "two runs differ"
    if name in ds.DEGENERATE:
        assert (out == 0).all()
    else:
        assert float(out.abs().max()) > 0


def test_runs_without_a_window_hold_zeros(ext):
    c, sites, cw, scaling, icpt, runs = reference("w16_c4_cw3")[:6]
    got = split(run_operator(ext, c, sites, cw, scaling, icpt).cpu().numpy(), runs, c["table"].shape[0])
    dead = [(i, q) for i in range(3) for q, r in enumerate(runs) if r[0] > int(c["seqlen"][i]) - cw]
    assert len(dead) >= 2
    for i, q in dead:
        assert (got[q][i] == 0).all() and not np.signbit(got[q][i]).any()
    live = [(i, q) for i in range(3) for q in range(len(runs)) if (i, q) not in dead]
    assert all(float(np.abs(got[q][i]).max()) > 0 for i, q in live)


def test_two_identical_table_rows_give_bit_equal_slices_on_every_site_axis(ext):
    c, sites, cw, scaling, icpt, runs = reference("dup_rows")[:6]
    assert (c["table"][1] == c["table"][3]).all()
    V = c["table"].shape[0]
    out = run_operator(ext, c, sites, cw, scaling, icpt)
    seen = set()
    for (_, _, _, g), tb in zip(runs, split(out, runs, V)):
        t = tb.reshape((tb.shape[0],) + (V,) * g)
        for ax in range(1, g + 1):
            assert same_bits(t.select(ax, 1).contiguous(), t.select(ax, 3).contiguous())
            assert not same_bits(t.select(ax, 1).contiguous(), t.select(ax, 2).contiguous())
            seen.add((g, ax))
    assert {(3, 1), (3, 2), (3, 3), (2, 1), (2, 2), (1, 1)} <= seen


@pytest.mark.parametrize("name", ["w128_c21_cw6", "w1024_c120_cw8", "n65"])
def test_a_sequence_alone_and_inside_a_reversed_batch(ext, name):
    c, sites, cw, scaling, icpt = reference(name)[:5]
    n = c["tokens"].shape[0]
    whole = run_operator(ext, c, sites, cw, scaling, icpt)
    for i in sorted({0, n // 2, n - 1}):
        assert same_bits(run_operator(ext, c, sites, cw, scaling, icpt, rows=[i])[0], whole[i]), i
    back = run_operator(ext, c, sites, cw, scaling, icpt, rows=np.arange(n)[::-1])      # every sequence at another index
    assert same_bits(back.flip(0).contiguous(), whole)


# ------------------------------------------------------------------------------------------------ against the earlier scans
def _scans(ext, c, cw, scaling, icpt):
    n, L = c["tokens"].shape
    V = c["table"].shape[0]
    dev = [torch.from_numpy(c[k]).to(DEV) for k in ("tokens", "table", "w")]
    tail = (torch.from_numpy(c["radem"]).to(DEV), torch.from_numpy(c["chi"]).to(DEV), c["seqlen"], cw, scaling, icpt)
    sub = torch.empty((n, L, V), dtype=F64, device=DEV)
    ext.hipConvTokenSubstScan(*dev, sub, *tail)
    pairs = torch.empty((n, L, cw - 1, V, V), dtype=F64, device=DEV)
    ext.hipConvTokenPairScan(*dev, pairs, *tail)
    return sub.cpu().numpy(), pairs.cpu().numpy()


def test_one_site_is_the_substitution_scan(ext):
    c, sites, cw, scaling, icpt, runs, _, _, total, _ = reference("one_site")
    V = c["table"].shape[0]
    got = ds.gather_full(runs, split(run_operator(ext, c, sites, cw, scaling, icpt).cpu().numpy(), runs, V), V, 1)
    sub, _ = _scans(ext, c, cw, scaling, icpt)
    cap = total + dss.cap_subst_scan(c["table"], c["seqlen"], c["w"], c["chi"], cw, scaling, icpt)
    assert report("K = 1", "one_site vs hipConvTokenSubstScan", got, sub[:, sites[0], :].astype(LD), cap) <= cap


@pytest.mark.parametrize("sites", [(1, 3), (1, 6)])
def test_two_sites_are_the_single_scans_and_the_pair_scan(ext, sites):
    """Distance 2 < conv_width 4: sub + sub + pairs; distance 5: no shared window, sub + sub."""
    kw = dict(n=2, L=8, C=6, V=5, conv_width=4, F=200, lengths=[8, 7])
    c, cw, scaling, icpt = dss.make_case(**kw), 4, 1, True
    V = 5
    runs = ds.site_runs(sites, 8, cw)
    got = ds.gather_full(runs, split(run_operator(ext, c, sites, cw, scaling, icpt).cpu().numpy(), runs, V), V, 2)
    sub, pairs = _scans(ext, c, cw, scaling, icpt)
    want = (sub[:, sites[0], :, None].astype(LD) + sub[:, sites[1], None, :].astype(LD))
    cap = ds.cap_site_scan(c["table"], c["seqlen"], c["w"], c["chi"], sites, 8, cw, scaling, icpt)[1] \
        + 2 * dss.cap_subst_scan(c["table"], c["seqlen"], c["w"], c["chi"], cw, scaling, icpt)
    d = sites[1] - sites[0]
    if d < cw:
        want = want + pairs[:, sites[0], d - 1].astype(LD)
        cap += dp.cap_pair_scan(c["table"], c["seqlen"], c["w"], c["chi"], cw, scaling, icpt)
        assert float(np.abs(pairs[:, sites[0], d - 1]).max()) > 100 * cap            # the term is there to be missed
    else:
        assert all(g == 1 for _, _, _, g in runs)
    assert report("K = 2", f"sites {sites} vs sub + sub (+ pairs)", got, want.reshape(2, V * V), cap) <= cap


# ------------------------------------------------------------------------------------------------ the kernel object
def _batch(tokens, table):
    from xgpr_amd.dataset import TokenBatch
    return TokenBatch(torch.from_numpy(tokens).to(DEV), torch.from_numpy(table).to(DEV))


def _library_rows(lib):
    return torch.cat([t.reshape(t.shape[0], -1) for t in lib.tables], dim=1)


@pytest.mark.parametrize("choice", ["Conv1dRBF", "Conv1dMatern", "Conv1dCauchy", "GraphRBF"])
def test_kernel_site_scan_is_the_ext_call_bit_for_bit(ext, choice):
    n, L, C, cw, M, V = 4, 9, 6, 4, 600, 5
    sites = (1, 2, 3, 5)
    k = _kernel(choice, n, L, C, cw, M, averaging="full" if choice == "GraphRBF" else "sqrt")
    tokens, table, scaled, seqlen, w = _kernel_case(k, n, L, V, 51, (9, 6, 7, 8))
    batch = _batch(tokens, table)
    lib = k.site_scan(batch, seqlen, w, sites)
    runs = ds.site_runs(sites, L, k.conv_width)
    assert lib.sites == sites and lib.vocab == V and lib.base is None
    assert lib.runs == tuple(tuple(range(a, a + g)) for _, _, a, g in runs)
    assert all(t.dtype == F64 and t.is_cuda and tuple(t.shape) == (n,) + (V,) * g for t, (_, _, _, g) in zip(lib.tables, runs))
    out = torch.full((n, ds.run_offsets(runs, V)[1]), float("nan"), dtype=F64, device=DEV)
    ext.hipConvTokenSiteScan(batch.tokens, torch.from_numpy(scaled).to(DEV), torch.from_numpy(w).to(DEV), out, k.radem_diag, k.chi_arr,
                             seqlen, sites, k.conv_width, k.scaling_type, k.fit_intercept)
    assert same_bits(_library_rows(lib), out)
    radem, chi = k.radem_diag.cpu().numpy(), k.chi_arr.cpu().numpy()
    full = ds.full_scan(tokens, scaled, seqlen, w, radem, chi, sites, k.conv_width, k.scaling_type, k.fit_intercept)
    total = ds.cap_site_scan(scaled, seqlen, w, chi, sites, L, k.conv_width, k.scaling_type, k.fit_intercept)[1]
    A = ds.assignments(V, len(sites))
    got = lib.gather(A).cpu().numpy()                            # (one more float64 rounding per run)
    slack = len(runs) * dr.U64 * float(np.abs(full).max())
    assert report("kernel", (choice, C, k.conv_width, L, M // 2, n), got, full, total + slack) <= total + slack
    # a batch beyond one launch's rows goes to the operator in slices: the same bits
    k.SITE_SCAN_ROWS = 2 * sum(V ** (g - 1) for _, _, _, g in runs) + 1
    assert same_bits(_library_rows(k.site_scan(batch, seqlen, w, sites)), out)
    with pytest.raises(RuntimeError, match="sequence_length is required"):
        k.site_scan(batch, None, w, sites)
    with pytest.raises(RuntimeError, match="TokenBatch"):
        k.site_scan(table[tokens], seqlen, w, sites)
    with pytest.raises(RuntimeError, match="strictly ascending"):
        k.site_scan(batch, seqlen, w, (2, 1))
    with pytest.raises(RuntimeError, match="inside every sequence"):
        k.site_scan(batch, seqlen, w, (1, 6))


def _composed_cap(k, tokens, scaled, seqlen, w, sites):
    """The composed route: two float32 feature rows -- the variant and the sequence (each entry within cap_conv with u_out = U32 of
    exact) --, each multiplied by the weights in float64: twice sum|w| cap_conv, over the windows of every written-out variant."""
    V, K = scaled.shape[0], len(sites)
    A = ds.assignments(V, K)
    mut = np.repeat(tokens[:, None, :], V ** K, axis=1)
    mut[:, :, list(sites)] = A[None]
    lens = np.repeat(seqlen, V ** K)
    x = scaled[mut.reshape(-1, tokens.shape[1]) % V]             # (positions past a length hold 255: never part of a window)
    row = dr.cap_conv(np.float32, x, lens, k.chi_arr.cpu().numpy(), k.conv_width, k.scaling_type, u_out=U32)
    sw = float(np.abs(w[1:] if k.fit_intercept else w).sum())
    return 2 * sw * row


def _composed_check(k, lib, tokens, scaled, seqlen, w, sites, tag):
    V, K = scaled.shape[0], len(sites)
    assert lib.runs == (tuple(range(K)),) and tuple(lib.tables[0].shape) == (tokens.shape[0],) + (V,) * K
    full = ds.full_scan(tokens, scaled, seqlen, w, k.radem_diag.cpu().numpy(), k.chi_arr.cpu().numpy(), sites, k.conv_width,
                        k.scaling_type, k.fit_intercept)
    ccap = _composed_cap(k, tokens, scaled, seqlen, w, sites)
    got = lib.tables[0].reshape(tokens.shape[0], -1).cpu().numpy()
    assert report("composed", tag, got, full, ccap) <= ccap
    for i in range(tokens.shape[0]):
        z = got[i, own_index(tokens[i], sites, V)]
        assert z == 0 and not np.signbit(z)
    return got, full, ccap


def test_the_composed_route_against_the_reference_and_beyond_the_operator(ext):
    from xgpr_amd.dataset import TokenBatch
    n, L, C, cw, M, V = 3, 8, 6, 3, 400, 5
    sites = (1, 2, 6)
    k = _kernel("Conv1dRBF", n, L, C, cw, M)
    tokens, table, scaled, seqlen, w = _kernel_case(k, n, L, V, 52, (8, 7))
    batch = _batch(tokens, table)
    k.COMPOSED_SCAN_ELEMS = 37 * M                               # several slices, the last one ragged
    fb, full, ccap = _composed_check(k, k.site_scan_composed(batch, seqlen, w, sites), tokens, scaled, seqlen, w, sites, (C, cw, L, M // 2, n))
    op = k.site_scan(batch, seqlen, w, sites)
    assert len(op.runs) > 1
    total = ds.cap_site_scan(scaled, seqlen, w, k.chi_arr.cpu().numpy(), sites, L, cw, k.scaling_type, k.fit_intercept)[1]
    slack = len(op.runs) * dr.U64 * float(np.abs(full).max())
    assert float(np.abs(op.gather(ds.assignments(V, 3)).cpu().numpy() - fb).max()) <= total + slack + ccap
    # a window of 9 x 128 = 1152 elements (P = 2048): the operator refuses, the kernel object takes the composed route
    n, L, C, cw, M, V = 2, 10, 128, 9, 128, 3
    sites = (0, 4, 8)
    k = _kernel("Conv1dRBF", n, L, C, cw, M, icpt=False)
    tokens, table, scaled, seqlen, w = _kernel_case(k, n, L, V, 53, (9, 10))
    assert ext.conv_token_site_scan_ok(cw * C, V, C, M // 2, 3) == 0
    T = ds.run_offsets(ds.site_runs(sites, L, cw), V)[1]
    out = torch.zeros((n, T), dtype=F64, device=DEV)
    with pytest.raises(RuntimeError, match="the site scan serves windows of up to 1024 elements"):
        ext.hipConvTokenSiteScan(torch.from_numpy(tokens).to(DEV), torch.from_numpy(scaled).to(DEV), torch.from_numpy(w).to(DEV), out,
                                 k.radem_diag, k.chi_arr, seqlen, sites, cw, 1, False)
    assert float(out.abs().max()) == 0.0                         # nothing is written
    batch = _batch(tokens, table)
    got, _, _ = _composed_check(k, k.site_scan(batch, seqlen, w, sites), tokens, scaled, seqlen, w, sites, (C, cw, L, M // 2, n))
    # tokens that are not contiguous take the composed route as well
    wide = torch.from_numpy(np.concatenate([tokens, tokens], axis=1)).to(DEV)
    assert not wide[:, :L].is_contiguous()
    again = k.site_scan(TokenBatch(wide[:, :L], batch.table), seqlen, w, sites)
    assert again.runs == ((0, 1, 2),) and np.array_equal(again.tables[0].reshape(n, -1).cpu().numpy(), got)
    # five sites inside one window, at V = 2: beyond the operator's four
    n, L, C, cw, M, V = 2, 8, 6, 6, 256, 2
    sites = (1, 2, 3, 4, 5)
    k = _kernel("Conv1dRBF", n, L, C, cw, M)
    tokens, table, scaled, seqlen, w = _kernel_case(k, n, L, V, 54, (8, 6))
    assert ext.conv_token_site_scan_ok(cw * C, V, C, M // 2, 4) == 1 and ext.conv_token_site_scan_ok(cw * C, V, C, M // 2, 5) == 0
    out = torch.zeros((n, ds.run_offsets(ds.site_runs(sites, L, cw), V)[1]), dtype=F64, device=DEV)
    with pytest.raises(RuntimeError, match="up to 4 sites inside one window"):
        ext.hipConvTokenSiteScan(torch.from_numpy(tokens).to(DEV), torch.from_numpy(scaled).to(DEV), torch.from_numpy(w).to(DEV), out,
                                 k.radem_diag, k.chi_arr, seqlen, sites, cw, k.scaling_type, True)
    assert float(out.abs().max()) == 0.0
    _composed_check(k, k.site_scan(_batch(tokens, table), seqlen, w, sites), tokens, scaled, seqlen, w, sites, ("five sites", C, cw, L))
    k.SITE_SCAN_VARIANTS = 31
    with pytest.raises(RuntimeError, match="SITE_SCAN_VARIANTS"):
        k.site_scan(_batch(tokens, table), seqlen, w, sites)


def test_the_operators_refusals(ext):
    c, sites, cw, scaling, icpt, runs = reference("w16_c4_cw3")[:6]
    n, L = c["tokens"].shape
    V = c["table"].shape[0]
    dev = {k: torch.from_numpy(c[k]).to(DEV) for k in ("tokens", "table", "w", "radem", "chi")}
    T = ds.run_offsets(runs, V)[1]
    out = torch.zeros((n, T), dtype=F64, device=DEV)

    def call(**kw):
        a = dict(dev, out=out, seqlen=c["seqlen"], cw=cw, sites=sites)
        a.update(kw)
        ext.hipConvTokenSiteScan(a["tokens"], a["table"], a["w"], a["out"], a["radem"], a["chi"], a["seqlen"], a["sites"], a["cw"], scaling, icpt)

    with pytest.raises(RuntimeError, match="Wrong array sizes"):
        call(out=torch.zeros((n, T + 1), dtype=F64, device=DEV))
    with pytest.raises(TypeError, match="2 dims"):
        call(out=torch.zeros((n, T, 1), dtype=F64, device=DEV))
    with pytest.raises(TypeError, match="dtype"):
        call(out=out.float())
    with pytest.raises(RuntimeError, match="Wrong array sizes"):
        call(w=dev["w"][:-2].contiguous())
    with pytest.raises(RuntimeError, match="strictly ascending"):
        call(sites=(3, 2, 4))
    other = torch.zeros((n, ds.run_offsets(ds.site_runs((2, 3, 5), L, cw), V)[1]), dtype=F64, device=DEV)
    with pytest.raises(RuntimeError, match="inside every sequence"):
        call(sites=(2, 3, 5), out=other)                                   # the sequence of 5 tokens ends before it
    assert float(other.abs().max()) == 0.0
    with pytest.raises(RuntimeError):
        call(seqlen=np.asarray([9, 2, 6], dtype=np.int32))                 # a length below conv_width
    with pytest.raises(RuntimeError):
        call(seqlen=c["seqlen"][:2].copy())
    assert float(out.abs().max()) == 0.0                                   # no refusal wrote anything


# ------------------------------------------------------------------------------------------------ predict_site_library end to end
N, L_, C_, CW, V_ = 40, 12, 4, 3, 5          # the shape of tests/test_gpu_subst_scan.py's _fit


@pytest.fixture(scope="module")
def fitted():
    return _fit("Conv1dRBF")


def _variants(tokens, sites, V):
    A = ds.assignments(V, len(sites))
    mut = np.repeat(tokens[:, None, :], A.shape[0], axis=1)
    mut[:, :, list(sites)] = A[None].astype(np.uint8)
    return A, mut


@pytest.mark.parametrize("sites", [(2, 3, 8), (2, 3, 4)])
def test_predict_site_library_conv1d(fitted, sites):
    """base + gather = predict of ALL V^3 written-out variants: two sites that share windows and one apart, and three inside one
    window -- where singles plus pairs are no longer the whole of it."""
    model, _, _, seqlen, tokens, table = fitted
    k = model.kernel
    std = float(model.trainy_std)
    keep = np.nonzero(seqlen > sites[-1])[0][:6]                 # (a site list is shared: the sequences that hold every site)
    assert 0 in keep and len(keep) >= 3 and len({int(s) for s in seqlen[keep]}) > 1
    toks, lens = tokens[keep], seqlen[keep]
    lib = model.predict_site_library(toks, sites, sequence_lengths=lens, token_table=table)
    assert lib.sites == sites and lib.vocab == V_ and all(t.dtype == F64 and not t.is_cuda for t in lib.tables)
    A, mut = _variants(toks, sites, V_)
    vl = np.repeat(lens, A.shape[0])
    want = model.predict(mut.reshape(-1, L_), sequence_lengths=vl, token_table=table).reshape(len(keep), -1)
    assert np.array_equal(lib.base.numpy(), model.predict(toks, sequence_lengths=lens, token_table=table))
    got = (lib.base[:, None] + lib.gather(A)).numpy()
    # the bound of test_predict_substitution_pairs_conv1d, for this scan: the tables within the cap of a full assignment, predict's
    # float32 rows of the variant and of the sequence within cap_conv each
    scaled = (table.astype(np.float64) * float(k.hyperparams[1])).astype(np.float32)
    w = model.weights.cpu().numpy()
    chi = k.chi_arr.cpu().numpy()
    total = ds.cap_site_scan(scaled, lens, w, chi, sites, L_, k.conv_width, k.scaling_type, True)[1]
    row = dr.cap_conv(np.float32, scaled[mut.reshape(-1, L_) % V_], vl, chi, k.conv_width, k.scaling_type, u_out=U32)
    bound = (total + 2 * float(np.abs(w).sum()) * row) * std
    err = float(np.abs(got - want).max())
    # what the library holds beyond the additive model of single substitutions, and beyond singles plus pairs
    dense = lib.dense().numpy()
    own = [tuple(int(t) for t in toks[i, list(sites)]) for i in range(len(keep))]
    single = [np.stack([dense[i][tuple(slice(None) if m == ax else own[i][m] for m in range(3))] for i in range(len(keep))]) for ax in range(3)]
    additive = single[0][:, :, None, None] + single[1][:, None, :, None] + single[2][:, None, None, :]
    pair = []
    for a, b in ((0, 1), (0, 2), (1, 2)):
        two = np.stack([dense[i][tuple(slice(None) if m in (a, b) else own[i][m] for m in range(3))] for i in range(len(keep))])
        shape = [len(keep), 1, 1, 1]
        shape[1 + a] = shape[1 + b] = V_
        pair.append((two - single[a][:, :, None] - single[b][:, None, :]).reshape(shape))
    third = dense - additive - pair[0] - pair[1] - pair[2]
    print(f"SITE model      {str(sites):<44} library-predict {err:.3e}  bound {bound:.3e}  max|want - base| "
          f"{float(np.abs(want - lib.base.numpy()[:, None]).max()):.3e}  max|non-additive| {float(np.abs(dense - additive).max()):.3e}"
          f"  max|three-site term| {float(np.abs(third).max()):.3e}")
    assert err <= bound
    assert float(np.abs(dense - additive).max()) > 100 * bound   # the interaction the identity needs is far above what the check resolves
    if sites == (2, 3, 4):
        assert float(np.abs(third).max()) > 100 * bound          # ... and so is the part that singles plus pairs miss
        assert lib.components() == [(0, 1, 2)]
    else:
        assert float(np.abs(third).max()) <= 8 * bound           # the site apart shares no window with the other two
        assert lib.components() == [(0, 1), (2,)]
    # ... and the dense reference itself, in the units of y
    full = ds.full_scan(toks, scaled, lens, w, k.radem_diag.cpu().numpy(), chi, sites, k.conv_width, k.scaling_type, True) * std
    slack = (len(lib.runs) + 1) * dr.U64 * float(np.abs(full).max())
    assert report("model", sites, lib.gather(A).numpy(), full, total * std + slack) <= total * std + slack
    # the k best of every parent are the k best written-out variants
    vals, assign = lib.topk(5)
    order = np.argsort(-want, axis=1, kind="stable")[:, :5]
    best = np.take_along_axis(want, order, axis=1)
    assert float(np.abs((lib.base[:, None] + vals).numpy() - best).max()) <= bound
    # a TokenBatch is the same input, and so is another chunking
    from xgpr_amd.dataset import TokenBatch
    tb = TokenBatch(torch.from_numpy(toks), torch.from_numpy(table))
    again = model.predict_site_library(tb, sites, sequence_lengths=lens, chunk_size=5)
    assert all(torch.equal(a, b) for a, b in zip(again.tables, lib.tables)) and torch.equal(again.base, lib.base)


def test_predict_site_library_graph():
    model, _, _, seqlen, tokens, table = _fit("GraphRBF")
    assert model.kernel.conv_width == 1
    keep = np.nonzero(seqlen > 6)[0][:4]
    lib = model.predict_site_library(tokens[keep], (0, 3, 6), sequence_lengths=seqlen[keep], token_table=table)
    assert lib.runs == ((0,), (1,), (2,)) and lib.components() == [(0,), (1,), (2,)]     # purely additive
    sub = model.predict_substitutions(tokens[keep], sequence_lengths=seqlen[keep], token_table=table)
    k = model.kernel
    scaled = (table.astype(np.float64) * float(k.hyperparams[1])).astype(np.float32)
    w = model.weights.cpu().numpy()
    cap = 2 * dss.cap_subst_scan(scaled, seqlen[keep], w, k.chi_arr.cpu().numpy(), 1, k.scaling_type, True) * float(model.trainy_std)
    for q, p in enumerate((0, 3, 6)):
        assert float(np.abs(lib.tables[q].numpy() - sub[:, p, :]).max()) <= cap


def test_predict_site_library_refusals(fitted):
    from xgpr_amd.models import xGPRegression
    model, ds_, x, seqlen, tokens, table = fitted
    with pytest.raises(RuntimeError, match="sequence_lengths is required"):
        model.predict_site_library(tokens[:1], (1, 2), token_table=table)
    with pytest.raises(RuntimeError, match="needs token input"):
        model.predict_site_library(x[:1], (1, 2), sequence_lengths=seqlen[:1])
    with pytest.raises(RuntimeError, match="shape\\[0\\] of sequence_lengths"):
        model.predict_site_library(tokens[:3], (1, 2), sequence_lengths=seqlen[:2], token_table=table)
    with pytest.raises(RuntimeError, match="inside every sequence"):
        model.predict_site_library(tokens[:3], (1, 5), sequence_lengths=seqlen[:3], token_table=table)    # the second has 3 tokens
    with pytest.raises(RuntimeError, match="strictly ascending"):
        model.predict_site_library(tokens[:1], (2, 2), sequence_lengths=seqlen[:1], token_table=table)
    fresh = xGPRegression(num_rffs=128, variance_rffs=32, kernel_choice="Conv1dRBF", device=DEV, verbose=False,
                          kernel_settings={"conv_width": CW, "averaging": "sqrt", "intercept": True})
    with pytest.raises(RuntimeError, match="not yet been successfully fitted"):
        fresh.predict_site_library(tokens[:1], (1, 2), sequence_lengths=seqlen[:1], token_table=table)
    two = xGPRegression(num_rffs=128, variance_rffs=32, kernel_choice="Conv1dTwoLayer", device=DEV, verbose=False,
                        kernel_settings={"conv_width": CW, "init_rffs": 64, "intercept": True})
    two.set_hyperparams(dataset=ds_)
    two.weights = torch.zeros(128, dtype=F64, device=DEV)                  # (the refusal is about the kernel, not the fit)
    with pytest.raises(RuntimeError, match="predict_site_library is available for the sequence and graph kernels Conv1dRBF, Conv1dMatern"):
        two.predict_site_library(tokens[:1], (1, 2), sequence_lengths=seqlen[:1], token_table=table)
