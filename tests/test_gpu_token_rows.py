"""Token-indexed sequence input on the GPU (hipConvTokenRows / hipConvTokenGradRows and everything built on them).  The yardstick
needs no tolerance: after the window fetch the token kernels run the code of the dense writers, so every row must be
``torch.equal`` to what hipConvFeatureRows / hipConvGradRows write for the expanded array ``table[tokens]``.

Shapes.  n = 7 sequences of L = 40 positions: more than one workgroup of four waves as soon as there are two frequency tiles,
lengths that include exactly conv_width (one k-mer) and L.  (conv_width, C) covers the three tile layouts of wave_conv_kernel:
rows only (padded window <= 64), transposed columns (128 / 256) and coalesced (512 / 1024), with windows that are no whole
number of 64-lane registers.  V = 21 runs the issue's six windows.  V = 256 runs them where the table fits the kernels' LDS image
(256 x C <= 4608 floats, i.e. C <= 18: only (2, 3) of the six) and, so that every layout still sees token values up to 255, on
sibling windows with C = 16 / 18; the other five are asserted to be refused by the operator and served, bit for bit, by the
dense-slice fallback of ConvSORFKernel."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
N, L = 7, 40
ISSUE_WINDOWS = [(3, 21), (2, 3), (9, 21), (5, 26), (24, 21), (9, 57)]          # -> 64, 8, 256, 256, 512, 1024
V256_WINDOWS = [(2, 3), (4, 16), (16, 16), (9, 18), (28, 18), (40, 16)]         # -> 8, 64, 256, 256, 512, 1024
GRID = [(cw, C, 21) for cw, C in ISSUE_WINDOWS] + [(cw, C, 256) for cw, C in V256_WINDOWS]
GRAD_GRID = [(3, 21, 21), (9, 21, 21), (24, 21, 21), (40, 16, 256), (2, 3, 256)]   # one per layout, the widest window, the narrowest


@pytest.fixture(scope="module")
def ext():
    from xgpr_amd import xgpr_hip_rfgen_ext as e
    return e


def padded(width):
    return 1 << max(1, int(np.ceil(np.log2(width))))


def _operands(cw, C, V, num_freqs, seed=0):
    """tokens (padding beyond each length = V - 1), a second copy with other padding, table, radem, chi, host lengths."""
    rng = np.random.default_rng(1000 * cw + 10 * C + V + num_freqs + seed)
    lens = np.asarray([cw, L, min(cw + 1, L), max(L - 1, cw), (cw + L) // 2, cw, L], dtype=np.int32)
    tokens = rng.integers(0, V, size=(N, L)).astype(np.uint8)
    tokens[:, 0], tokens[:, cw - 1] = 0, V - 1                                     # both ends of the vocabulary inside every sequence
    other = tokens.copy()
    for i, n_i in enumerate(lens):
        tokens[i, n_i:] = V - 1
        other[i, n_i:] = 0
    table = rng.standard_normal((V, C)).astype(np.float32)                         # not one-hot: a wrong row or channel shows
    P = padded(cw * C)
    R = -(-num_freqs // P) * P
    radem = rng.choice(np.asarray([-1, 1], dtype=np.int8), size=(3, 1, R))
    chi = (0.2 + rng.random(num_freqs)).astype(np.float32)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return to(tokens), to(other), to(table), to(radem), to(chi), lens


@pytest.mark.parametrize("num_freqs", [300, 1500])
@pytest.mark.parametrize("cw,C,V", GRID)
def test_token_feature_rows_equal_the_dense_writer_bit_for_bit(ext, cw, C, V, num_freqs):
    from xgpr_amd.kernels import scale_input
    tokens, other, table, radem, chi, lens = _operands(cw, C, V, num_freqs)
    assert ext.conv_token_rows_ok(cw * C, V, C) == 1
    assert int(tokens.min()) == 0 and int(tokens.max()) == V - 1
    tab_s = scale_input(table, 0.7312)
    dense = tab_s[tokens.long()].contiguous()
    for icpt in (False, True):
        for scaling in (0, 1, 2):
            ref = torch.full((N, 2 * num_freqs), float("nan"), dtype=torch.float32, device=DEV)
            ext.hipConvFeatureRows(dense, ref, radem, chi, lens, cw, scaling, icpt)
            rows = torch.full_like(ref, float("nan"))                               # garbage beforehand: the operator overwrites
            ext.hipConvTokenRows(tokens, tab_s, rows, radem, chi, lens, cw, scaling, icpt)
            assert torch.equal(rows, ref), (icpt, scaling)
            assert bool(torch.isfinite(rows).all())
            # positions beyond a sequence's length are never read
            rows2 = torch.full_like(ref, float("nan"))
            ext.hipConvTokenRows(other, tab_s, rows2, radem, chi, lens, cw, scaling, icpt)
            assert torch.equal(rows2, ref), (icpt, scaling)


@pytest.mark.parametrize("num_freqs", [300, 1500])
@pytest.mark.parametrize("cw,C,V", GRAD_GRID)
def test_token_gradient_rows_equal_the_dense_writer_bit_for_bit(ext, cw, C, V, num_freqs):
    tokens, other, table, radem, chi, lens = _operands(cw, C, V, num_freqs, seed=7)
    dense = table[tokens.long()].contiguous()                                      # unscaled, as x is
    sigma = 0.7312
    for icpt in (False, True):
        for scaling in (0, 1, 2):
            zref, gref, z, g, z2, g2 = (torch.full((N, 2 * num_freqs), float("nan"), dtype=torch.float32, device=DEV) for _ in range(6))
            ext.hipConvGradRows(dense, zref, gref, radem, chi, lens, sigma, cw, scaling, icpt)
            ext.hipConvTokenGradRows(tokens, table, z, g, radem, chi, lens, sigma, cw, scaling, icpt)
            assert torch.equal(z, zref) and torch.equal(g, gref), (icpt, scaling)
            ext.hipConvTokenGradRows(other, table, z2, g2, radem, chi, lens, sigma, cw, scaling, icpt)
            assert torch.equal(z2, zref) and torch.equal(g2, gref), (icpt, scaling)


def test_a_larger_batch_takes_the_longest_first_order(ext):
    """n >= 64 sequences: the launcher sorts them longest first (conv_order_kernel), as for the dense writer."""
    rng = np.random.default_rng(3)
    n, cw, C, V, F = 150, 9, 21, 21, 1100
    lens = rng.integers(cw, L + 1, size=n).astype(np.int32)
    tokens = torch.from_numpy(rng.integers(0, V, size=(n, L)).astype(np.uint8)).to(DEV)
    table = torch.from_numpy(rng.standard_normal((V, C)).astype(np.float32)).to(DEV)
    radem = torch.from_numpy(rng.choice(np.asarray([-1, 1], dtype=np.int8), size=(3, 1, 1280))).to(DEV)
    chi = torch.from_numpy((0.2 + rng.random(F)).astype(np.float32)).to(DEV)
    ref = torch.empty((n, 2 * F), dtype=torch.float32, device=DEV)
    rows = torch.empty_like(ref)
    ext.hipConvFeatureRows(table[tokens.long()].contiguous(), ref, radem, chi, lens, cw, 1, True)
    ext.hipConvTokenRows(tokens, table, rows, radem, chi, lens, cw, 1, True)
    assert torch.equal(rows, ref)


def _conv_kernel(C, cw, rffs=512, name="Conv1dRBF"):
    from xgpr_amd.kernels import make_kernel
    kern = make_kernel(name, (N, L, C), rffs, 123, DEV, {"conv_width": cw, "averaging": "sqrt", "intercept": True, "matern_nu": 2.5})
    kern.set_hyperparams(np.array([0.5, 0.7312]), logspace=False)
    return kern


FALLBACKS = [(21, 100, 21)] + [(cw, C, 256) for cw, C in ISSUE_WINDOWS if 256 * C > 4608]      # a window of 2100 elements; tables over the cap


@pytest.mark.parametrize("cw,C,V", FALLBACKS)
def test_unserved_shapes_are_refused_by_the_operator_and_served_from_dense_slices(ext, cw, C, V):
    from xgpr_amd.dataset import TokenBatch
    tokens, _, table, _, _, lens = _operands(cw, C, V, 256)
    assert ext.conv_token_rows_ok(cw * C, V, C) == 0
    kern = _conv_kernel(C, cw)
    tb = TokenBatch(tokens, table)
    assert not kern.token_rows_ok(tb)
    m = kern.get_num_rffs()
    out = torch.full((N, m), float("nan"), dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="xgpr_conv_token_rows_ok"):
        ext.hipConvTokenRows(tokens, table, out, kern.radem_diag, kern.chi_arr, lens, cw, 1, True)
    assert bool(torch.isnan(out).all())                                            # nothing was launched
    ref = torch.empty_like(out)
    xs = tb.scaled(kern.hyperparams[1])
    kern.fill_feature_rows(xs.dense().contiguous(), lens, ref)
    kern.fill_feature_rows(xs, lens, out)
    assert torch.equal(out, ref)
    z, g, zr, gr = (torch.empty_like(out) for _ in range(4))
    kern.fill_grad_rows(tb.dense().contiguous(), zr, gr, lens)
    kern.fill_grad_rows(tb, z, g, lens)
    assert torch.equal(z, zr) and torch.equal(g, gr)


def test_graph_kernel_with_tokens(ext):
    """conv_width = 1: allowed (if pointless); windows of C elements."""
    from xgpr_amd.dataset import TokenBatch
    from xgpr_amd.kernels import make_kernel
    tokens, _, table, _, _, _ = _operands(1, 12, 21, 256)
    lens = np.asarray([1, L, 2, L - 1, 20, 1, L], dtype=np.int32)
    kern = make_kernel("GraphRBF", (N, L, 12), 512, 123, DEV, {"averaging": "none", "intercept": False})
    kern.set_hyperparams(np.array([0.5, 1.3]), logspace=False)
    tb = TokenBatch(tokens, table).scaled(kern.hyperparams[1])
    assert kern.token_rows_ok(tb)
    out, ref = (torch.empty((N, 512), dtype=torch.float32, device=DEV) for _ in range(2))
    kern.fill_feature_rows(tb.dense().contiguous(), lens, ref)
    kern.fill_feature_rows(tb, lens, out)
    assert torch.equal(out, ref)


# ---- model level: N = 300, L = 30, one-hot 21 x 21, conv_width 9, 512 RFFs, rank 64
@pytest.fixture(scope="module")
def protein():
    rng = np.random.default_rng(11)
    n, Lp, V = 300, 30, 21
    tokens = rng.integers(0, V, size=(n + 40, Lp)).astype(np.int64)
    lens = rng.integers(9, Lp + 1, size=n + 40).astype(np.int32)
    lens[:2] = (9, Lp)
    table = np.eye(V, dtype=np.float32)
    dense = table[tokens]
    w = rng.standard_normal(V)
    y = np.asarray([w[t[:k]].sum() / np.sqrt(k) for t, k in zip(tokens, lens)]) + 0.1 * rng.standard_normal(n + 40)
    return dict(n=n, tokens=tokens, lens=lens, table=table, dense=dense, y=y, labels=(y > np.median(y)).astype(np.int64))


def _fit(kind, ds, x_test, lens_test, **predict_kw):
    from xgpr_amd.models import xGPRegression
    mod = xGPRegression(num_rffs=512, kernel_choice=kind, variance_rffs=64, random_seed=123, device=DEV,
                        kernel_settings={"conv_width": 9, "averaging": "sqrt", "intercept": True, "matern_nu": 2.5}, verbose=False)
    mod.set_hyperparams(np.array([-0.7, 0.2]), ds)
    cache = mod.kernel.build_feature_cache(ds).clone()
    pre, _ = mod.build_preconditioner(ds, max_rank=64, method="srht")
    mod.fit(ds, preconditioner=pre, mode="cg", tol=1e-6, max_iter=200, suppress_var=False)
    weights = mod.weights.clone()
    mean = mod.predict(x_test, sequence_lengths=lens_test, **predict_kw)
    mean2, var = mod.predict(x_test, sequence_lengths=lens_test, get_var=True, **predict_kw)
    nll, grad = mod.exact_nmll_gradient(np.array([-0.7, 0.2]), ds)
    return dict(cache=cache, weights=weights, mean=mean, mean_var_path=mean2, var=var, nll=nll, grad=np.asarray(grad))


@pytest.mark.parametrize("kind", ["Conv1dRBF", "Conv1dMatern"])
def test_model_on_tokens_matches_the_dense_dataset(protein, kind):
    """Every solver pass reads identical rows and the slabs reduce in a fixed order: the fit, the predictions and the exact
    NMLL gradient are equal bit for bit -- provided two dense fits are (checked first; otherwise 1e-12 relative)."""
    from xgpr_amd.dataset import TokenBatch, build_regression_dataset
    p, n = protein, protein["n"]
    mk_dense = lambda: build_regression_dataset(p["dense"][:n], p["y"][:n], p["lens"][:n], chunk_size=128, device=DEV)
    ds_tok = build_regression_dataset(p["tokens"][:n], p["y"][:n], p["lens"][:n], chunk_size=128, device=DEV, token_table=p["table"])
    assert ds_tok.get_xdim() == (n, 30, 21) and isinstance(ds_tok.get_xdata(), TokenBatch)
    xt, lt = p["dense"][n:], p["lens"][n:]
    d1 = _fit(kind, mk_dense(), xt, lt)
    d2 = _fit(kind, mk_dense(), xt, lt)
    tok = _fit(kind, ds_tok, p["tokens"][n:], lt, token_table=p["table"])
    assert torch.equal(tok["cache"], d1["cache"])
    repeatable = (torch.equal(d1["weights"], d2["weights"]) and np.array_equal(d1["mean"], d2["mean"])
                  and np.array_equal(d1["grad"], d2["grad"]) and d1["nll"] == d2["nll"])
    print(f"{kind}: two dense fits bit-identical: {repeatable}")
    if repeatable:
        assert torch.equal(tok["weights"], d1["weights"])
        for key in ("mean", "mean_var_path", "var", "grad"):
            assert np.array_equal(tok[key], d1[key]), key
        assert tok["nll"] == d1["nll"]
    else:
        close = lambda a, b: np.abs(np.asarray(a) - np.asarray(b)).max() <= 1e-12 * np.abs(np.asarray(b)).max()
        assert close(tok["weights"].cpu().numpy(), d1["weights"].cpu().numpy())
        for key in ("mean", "mean_var_path", "var", "grad", "nll"):
            assert close(tok[key], d1[key]), key
    assert np.all(np.isfinite(tok["mean"])) and np.all(tok["var"] >= 0)


def test_classifier_on_tokens_matches_the_dense_dataset(protein):
    from xgpr_amd.dataset import TokenBatch, build_classification_dataset
    from xgpr_amd.models import xGPClassification
    p, n = protein, protein["n"]
    out = []
    for token in (False, True):
        if token:
            ds = build_classification_dataset(p["tokens"][:n], p["labels"][:n], p["lens"][:n], chunk_size=128, device=DEV,
                                              token_table=p["table"])
        else:
            ds = build_classification_dataset(p["dense"][:n], p["labels"][:n], p["lens"][:n], chunk_size=128, device=DEV)
        mod = xGPClassification(num_rffs=512, kernel_choice="Conv1dRBF", random_seed=123, device=DEV,
                                kernel_settings={"conv_width": 9, "averaging": "sqrt", "intercept": True}, verbose=False)
        mod.set_hyperparams(np.array([-0.7, 0.2]), ds)
        pre, _ = mod.build_preconditioner(ds, max_rank=64, method="srht")
        mod.fit(ds, preconditioner=pre, tol=1e-2, max_iter=100)
        if token:
            tb = TokenBatch(torch.from_numpy(p["tokens"][n:].astype(np.uint8)).to(DEV), torch.from_numpy(p["table"]).to(DEV))
            probs = mod.predict(tb, sequence_lengths=p["lens"][n:])
            assert np.array_equal(probs, mod.predict(p["tokens"][n:], sequence_lengths=p["lens"][n:], token_table=p["table"]))
        else:
            probs = mod.predict(p["dense"][n:], sequence_lengths=p["lens"][n:])
        out.append((mod.weights.clone(), probs))
    assert np.allclose(out[1][1].sum(axis=1), 1.0)
    assert np.abs(out[1][0].cpu().numpy() - out[0][0].cpu().numpy()).max() <= 1e-12 * np.abs(out[0][0].cpu().numpy()).max()
    assert np.abs(out[1][1] - out[0][1]).max() <= 1e-12


def test_footprint_of_a_token_dataset():
    """A condition, not a measurement: N = 512, L = 200, C = 21 (dense x: 8.6 MB), 64 RFFs.  Building the feature cache of the
    token dataset allocates less than half the dense array's bytes at its peak, and the dataset holds no float tensor of
    N * L * C elements."""
    from xgpr_amd.dataset import TokenBatch, build_regression_dataset
    from xgpr_amd.kernels import make_kernel
    rng = np.random.default_rng(2)
    n, Lf, V = 512, 200, 21
    tokens = rng.integers(0, V, size=(n, Lf))
    lens = rng.integers(9, Lf + 1, size=n)
    ds = build_regression_dataset(tokens, rng.standard_normal(n), lens, chunk_size=128, device=DEV, token_table=np.eye(V, dtype=np.float32))
    kern = make_kernel("Conv1dRBF", ds.get_xdim(), 64, 123, DEV, {"conv_width": 9, "averaging": "none", "intercept": True})
    kern.set_hyperparams(np.array([0.5, 0.9]), logspace=False)
    dense_bytes = n * Lf * V * 4
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    zc = kern.build_feature_cache(ds)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - before
    print(f"peak growth {grew} bytes, dense x {dense_bytes} bytes")
    assert grew < dense_bytes // 2
    assert tuple(zc.shape) == (n, 64) and bool(torch.isfinite(zc).all())

    def tensors(obj):
        for v in vars(obj).values():
            if isinstance(v, torch.Tensor):
                yield v
            elif isinstance(v, TokenBatch):
                yield from (v.tokens, v.table)
            elif isinstance(v, dict):
                yield from (t for t in v.values() if isinstance(t, torch.Tensor))
    held = list(tensors(ds))
    assert any(t.dtype == torch.uint8 and t.numel() == n * Lf for t in held)
    assert all(not (t.is_floating_point() and t.numel() >= n * Lf * V) for t in held)
