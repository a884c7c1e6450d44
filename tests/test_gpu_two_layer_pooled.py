"""The two-layer kernel on the fixed-vector solver path: its first layer pooled once per dataset (``DeviceDataset.pooled``), its
second layer handed to every solver pass as an RBF ``SORFKernel`` (``Conv1dTwoLayerKernel.second_layer``), token input pooled from
the tokens.  The baseline is the same model with ``pool_first_layer = False``: every pass on the two-layer kernel and the original
dataset.

Problems: 700 sequences, L = 16, C = 8, conv_width 3, M = 256, intercept on, init_rffs 64 and 70 (70: ``scaled_x`` pads the pooled rows
to 72 floats); and the same size as tokens over a 21 x 21 one-hot table.

Tolerances.  Feature and gradient maps: none -- both routes end in the same operator call on the same sigma-scaled float32 rows.
Gradient terms: 1e-12 x max|term|, the bar tests/test_gpu_seq_grad_rows.py sets for a change of summation order (both routes
accumulate the same float64 products of the same float32 rows).  exact_nmll: 1e-6 relative, the DESIGN section 5 bar.  CG: the true
relative residual |(Z^T Z + lambda^2 I) w - Z^T y| / |Z^T y| from float64 ``transform_x`` features must satisfy res_new <= 10 x
max(res_old, tol) at tol = 1e-6 -- the fused matvec is held to 1e-6 relative of the float64 product elsewhere in the suite, the size
of the tolerance, so the true residual may sit a small multiple above what CG believes; ten leaves room for the conditioning of this
small problem, a wrong feature map gives O(1) -- and the iteration counts must be within 2 of each other.  Classifier cost: 1e-6
relative; the two row formats differ by one float32 rounding per entry, 6e-8."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
N, L, C, CW, M = 700, 16, 8, 3, 256
V = 21
HP = np.array([0.5, 0.6])          # lambda, sigma
SIGMAS = (0.45, 0.6, 0.8)


@pytest.fixture(scope="module")
def ext():
    from xgpr_amd import xgpr_hip_rfgen_ext as e
    return e


def _settings(init_rffs):
    return {"conv_width": CW, "init_rffs": init_rffs, "intercept": True}


@functools.lru_cache(maxsize=None)
def _dense_data():
    rng = np.random.default_rng(17)
    x = rng.standard_normal((N, L, C)).astype(np.float32)
    sl = rng.integers(CW, L + 1, size=N).astype(np.int32)
    sl[0], sl[1] = CW, L
    y = np.sin(x[:, 0, :3].sum(axis=1)) + 0.1 * rng.standard_normal(N)
    labels = (np.arange(N) % 3).astype(np.int64)
    return x, sl, y, labels


@functools.lru_cache(maxsize=None)
def _token_data():
    rng = np.random.default_rng(23)
    tokens = rng.integers(0, V, size=(N, L)).astype(np.int64)
    sl = rng.integers(CW, L + 1, size=N).astype(np.int32)
    sl[0], sl[1] = CW, L
    table = np.eye(V, dtype=np.float32)
    y = np.sin(0.3 * tokens[:, :3].sum(axis=1)) + 0.1 * rng.standard_normal(N)
    return tokens, table, sl, y


def _dense_ds(classes=False):
    from xgpr_amd.dataset import build_classification_dataset, build_regression_dataset
    x, sl, y, labels = _dense_data()
    if classes:
        return build_classification_dataset(x, labels, sl, chunk_size=256, device=DEV)
    return build_regression_dataset(x, y, sl, chunk_size=256, device=DEV)


def _token_ds():
    from xgpr_amd.dataset import build_regression_dataset
    tokens, table, sl, y = _token_data()
    return build_regression_dataset(tokens, y, sl, chunk_size=256, device=DEV, token_table=table)


def _model(ds, init_rffs, pool=True, cls=None, hp=HP):
    from xgpr_amd.models import xGPRegression
    model = (cls or xGPRegression)(num_rffs=M, kernel_choice="Conv1dTwoLayer", device=DEV, kernel_settings=_settings(init_rffs),
                                   verbose=False)
    model.pool_first_layer = pool
    model.set_hyperparams(np.log(hp), ds)
    return model


def _kernel(xdim, init_rffs, hp=HP):
    from xgpr_amd.kernels import make_kernel
    k = make_kernel("Conv1dTwoLayer", xdim, M, 123, DEV, _settings(init_rffs))
    k.set_hyperparams(hp, logspace=False)
    return k


def _count_pooling(monkeypatch, ext):
    """Counts the sequences that go through the two pooling operators."""
    seen = {"rows": 0, "calls": 0}
    for name in ("hipConv1dMaxpool", "hipConvTokenMaxpool"):
        real = getattr(ext, name)

        def counted(x, *a, _real=real, **kw):
            seen["rows"] += x.shape[0]
            seen["calls"] += 1
            return _real(x, *a, **kw)
        monkeypatch.setattr(ext, name, counted)
    return seen


def _forbid(monkeypatch, ext, *names):
    calls = []

    def raiser(*a, **k):
        calls.append(1)
        raise AssertionError("the float64 feature operator was called on the fixed-vector route")
    for nm in names:
        monkeypatch.setattr(ext, nm, raiser)
    return calls


# ---------------------------------------------------------------------------------------------- bit identities
@pytest.mark.parametrize("init_rffs", [64, 70])
def test_second_layer_over_the_pooled_dataset_is_the_kernel_bit_for_bit(init_rffs):
    from xgpr_amd.kernels import SORFKernel
    x, sl, _, _ = _dense_data()
    ds = _dense_ds()
    k = _kernel(x.shape, init_rffs)
    s, p = k.second_layer(), ds.pooled(k)
    assert isinstance(s, SORFKernel) and p is ds.pooled(k)
    xp = p.get_xdata()
    assert xp.dtype == torch.float32 and tuple(xp.shape) == (N, init_rffs) and xp.is_cuda
    assert bool((xp >= 0).all()) and float(xp.max()) > 0                              # ReLU'd filters
    assert p.get_xdim() == (N, init_rffs) and p.get_sequence_lengths() is None
    assert tuple(p.scaled_x(k.hyperparams[1]).shape) == (N, (init_rffs + 3) // 4 * 4)
    for sigma in (0.6, 1.3):
        k.set_hyperparams(np.array([0.5, sigma]), logspace=False)
        assert torch.equal(s.transform_x(xp), k.transform_x(x, sl))
        z, g = k.gradient_x(x, sl)
        zs, gs = s.gradient_x(xp)
        assert torch.equal(zs, z) and torch.equal(gs, g) and float(g.abs().max()) > 0
        assert ds.pooled(k) is p
    assert torch.equal(k.pool(x, sl), xp) and torch.equal(k.pool(torch.from_numpy(x).double(), sl), xp)
    k.POOL_SLICE_ROWS = 256                                                           # three slices: the same rows
    assert torch.equal(k.pool(x, sl), xp)


def test_the_pooled_layer_from_tokens_equals_the_one_from_the_dense_expansion(monkeypatch, ext):
    tokens, table, sl, _ = _token_data()
    ds = _token_ds()
    k = _kernel((N, L, V), 64)
    dense = torch.from_numpy(table)[torch.from_numpy(tokens)]
    want = k.pool(dense, sl)
    seen = _count_pooling(monkeypatch, ext)
    called = []
    real = ext.hipConvTokenMaxpool
    monkeypatch.setattr(ext, "hipConvTokenMaxpool", lambda *a, **kw: (called.append(1), real(*a, **kw))[1])
    got = ds.pooled(k).get_xdata()
    assert called and torch.equal(got, want) and seen["rows"] == N
    assert torch.equal(k.transform_x(ds.get_xdata(), sl), k.transform_x(dense, sl))
    # a table the token operator does not serve: pooled from dense slices of at most CACHE_BUILD_ROWS sequences, the same bits
    from xgpr_amd.dataset import TokenBatch
    from xgpr_amd.kernels import ConvSORFKernel
    wide = torch.randn((256, 19), generator=torch.Generator().manual_seed(3)).to(DEV)
    tb = TokenBatch(torch.from_numpy(tokens.astype(np.uint8)).to(DEV), wide)
    kw = _kernel((N, L, 19), 64)
    assert ext.conv_token_rows_ok(CW * 19, 256, 19) == 0
    monkeypatch.setattr(ConvSORFKernel, "CACHE_BUILD_ROWS", 300)
    assert torch.equal(kw.pool(tb, sl), kw.pool(tb.dense(), sl))


# ---------------------------------------------------------------------------------------------- pooled once
def test_the_first_layer_runs_once_across_sigmas_preconditioner_and_fit(monkeypatch, ext):
    ds = _dense_ds()
    seen = _count_pooling(monkeypatch, ext)
    model = _model(ds, 64)
    for sigma in SIGMAS:
        score, grad = model.exact_nmll_gradient(np.log([0.5, sigma]), ds)
        assert np.isfinite(score) and np.all(np.isfinite(grad))
    pooled = ds.pooled(model.kernel)
    pre, _ = model.build_preconditioner(ds, max_rank=64)
    model.fit(ds, preconditioner=pre, tol=1e-6)
    assert model.weights is not None and model.var is not None
    assert seen["rows"] == N, seen                                                    # one pass over the shard
    assert ds.pooled(model.kernel) is pooled
    # the baseline pools again at every sigma
    ds2 = _dense_ds()
    old = _model(ds2, 64, pool=False)
    seen["rows"] = 0
    counts = []
    for sigma in SIGMAS:
        old.exact_nmll_gradient(np.log([0.5, sigma]), ds2)
        counts.append(seen["rows"])
    assert counts[0] >= N and counts[1] >= counts[0] + N and counts[2] >= counts[1] + N, counts
    assert getattr(ds2, "_pooled", None) is None


# ---------------------------------------------------------------------------------------------- tokens never expanded
def test_token_dataset_is_never_expanded(monkeypatch, ext):
    from xgpr_amd.dataset import TokenBatch
    from xgpr_amd.models import FastConv1d
    tokens, table, sl, _ = _token_data()
    ds = _token_ds()
    model = _model(ds, 64)
    fc = FastConv1d(V, device=DEV, conv_width=CW, num_features=70)
    tb = TokenBatch(torch.from_numpy(tokens[:100].astype(np.uint8)).to(DEV), torch.from_numpy(table).to(DEV))
    want_fc = fc.predict(tb.dense().cpu().numpy(), sl[:100])
    want_pred_features = model.kernel.transform_x(tb.dense(), sl[:100])

    def no_dense(self):
        raise AssertionError("TokenBatch.dense() was called")
    monkeypatch.setattr(TokenBatch, "dense", no_dense)
    score, grad = model.exact_nmll_gradient(np.log(HP), ds)
    assert np.isfinite(score) and np.all(np.isfinite(grad))
    pre, _ = model.build_preconditioner(ds, max_rank=64)
    model.fit(ds, preconditioner=pre, tol=1e-6)
    pred = model.predict(tb, sl[:100])
    pred2 = model.predict(tokens[:100], sl[:100], token_table=table)
    assert pred.shape == (100,) and np.all(np.isfinite(pred)) and np.array_equal(pred, pred2)
    want = (want_pred_features * model.weights[None, :]).sum(dim=1).cpu().numpy() * model.trainy_std + model.trainy_mean
    assert np.allclose(pred, want, rtol=1e-12, atol=0)
    assert np.array_equal(fc.predict(tb, sl[:100]), want_fc)
    assert np.array_equal(fc.predict(tokens[:100], sl[:100], token_table=table), want_fc)
    # the baseline's gradient rows read tokens too (fill_grad_rows called dense() on the whole shard before)
    old = _model(_token_ds(), 64, pool=False)
    s2, g2 = old.exact_nmll_gradient(np.log(HP), _token_ds())
    assert abs(s2 - score) <= 1e-6 * abs(score)


# ---------------------------------------------------------------------------------------------- the fused route
def test_cg_without_a_cache_runs_on_the_fused_matvec(monkeypatch, ext):
    ds = _dense_ds()
    model = _model(ds, 70)
    pre, _ = model.build_preconditioner(ds, max_rank=64)
    calls = _forbid(monkeypatch, ext, "hipRBFFeatureGen", "cudaRBFFeatureGen")
    fused = []
    real = ext.hipZtZMatvec
    monkeypatch.setattr(ext, "hipZtZMatvec", lambda *a, **kw: (fused.append(a[0].shape), real(*a, **kw))[1])
    # (the solve is what is under test: the variance of 16 features is no whole Gram tile and takes, as for every fixed-vector
    # kernel, float64 feature chunks)
    n_iter, _ = model.fit(ds, preconditioner=pre, tol=1e-6, mode="cg", cache_features=False, run_diagnostics=True,
                          suppress_var=True)
    assert not calls and model.weights is not None
    assert len(fused) >= n_iter >= 1 and all(tuple(s) == (N, 72) for s in fused), (len(fused), n_iter, fused[:2])


# ---------------------------------------------------------------------------------------------- NMLL
@pytest.mark.parametrize("init_rffs", [64, 70])
def test_gradient_terms_and_exact_nmll_agree_with_the_two_layer_route(init_rffs):
    from xgpr_amd import nmll
    x, _, _, _ = _dense_data()
    ds = _dense_ds()
    k = _kernel(x.shape, init_rffs, hp=np.array([0.7, 0.45]))
    assert nmll._grad_rows_route(ds, k)
    old = nmll.calc_gradient_terms(ds, k)
    s, p = k.second_layer(), ds.pooled(k)
    assert nmll._grad_rows_route(p, s)
    new = nmll.calc_gradient_terms(p, s)
    for i, (r, f) in enumerate(zip(new[:5], old[:5])):
        r, f = torch.as_tensor(r), torch.as_tensor(f)
        err, bar = float((r - f).abs().max()), 1e-12 * float(f.abs().max())
        print("init_rffs", init_rffs, "term", i, "err", err, "bar", bar)
        assert err <= bar, (i, err, bar)
    assert new[5] == old[5] == N
    a, b = nmll.exact_nmll(s, p), nmll.exact_nmll(k, ds)
    print("exact_nmll pooled", a, "two-layer", b)
    assert np.isfinite(b) and abs(a - b) <= 1e-6 * abs(b)
    ga, gb = nmll.exact_nmll_gradient(s, p), nmll.exact_nmll_gradient(k, ds)
    assert abs(ga[0] - gb[0]) <= 1e-6 * abs(gb[0])


# ---------------------------------------------------------------------------------------------- CG
def _true_residual(k, x, sl, ds, w):
    z = k.transform_x(x, sl)
    y = ds.normalized_y()
    rhs = z.T @ y
    lhs = z.T @ (z @ w) + float(k.get_lambda()) ** 2 * w
    return float(torch.linalg.norm(lhs - rhs) / torch.linalg.norm(rhs))


@pytest.mark.parametrize("init_rffs", [64, 70])
def test_cg_weights_of_the_pooled_route_solve_the_same_system(init_rffs):
    x, sl, _, _ = _dense_data()
    tol, out = 1e-6, {}
    for name, pool in (("old", False), ("new", True)):
        ds = _dense_ds()
        model = _model(ds, init_rffs, pool=pool)
        pre, _ = model.build_preconditioner(ds, max_rank=64)
        n_iter, _ = model.fit(ds, preconditioner=pre, tol=tol, mode="cg", run_diagnostics=True, suppress_var=True)
        out[name] = (_true_residual(model.kernel, x, sl, ds, model.weights), n_iter, model.weights)
    (res_old, it_old, w_old), (res_new, it_new, w_new) = out["old"], out["new"]
    print("init_rffs", init_rffs, "res_old", res_old, "iters_old", it_old, "res_new", res_new, "iters_new", it_new,
          "max|w_new - w_old| / max|w_old|", float((w_new - w_old).abs().max() / w_old.abs().max()))
    assert res_new <= 10 * max(res_old, tol), (res_new, res_old)
    assert abs(it_new - it_old) <= 2, (it_new, it_old)


# ---------------------------------------------------------------------------------------------- classifier
def test_classifier_cost_and_fit_on_the_pooled_pair():
    from xgpr_amd.classification import NonlinearCGClassification
    from xgpr_amd.models import xGPClassification
    x, _, _, _ = _dense_data()
    ds = _dense_ds(classes=True)
    k = _kernel(x.shape, 64)
    wmat = torch.from_numpy(np.random.default_rng(5).standard_normal((M, 3)) * 0.05).to(DEV)
    g_old, l_old = NonlinearCGClassification(ds, k).cost_fun_classification(wmat)
    g_new, l_new = NonlinearCGClassification(ds.pooled(k), k.second_layer()).cost_fun_classification(wmat)
    gerr = float((g_new - g_old).abs().max() / g_old.abs().max())
    print("loss old", l_old, "new", l_new, "gradient max relative difference", gerr)
    assert abs(l_new - l_old) <= 1e-6 * abs(l_old) and gerr <= 1e-6
    ds2 = _dense_ds(classes=True)
    model = _model(ds2, 64, cls=xGPClassification)
    pre, _ = model.build_preconditioner(ds2, max_rank=64)
    n_iter, losses = model.fit(ds2, preconditioner=pre, run_diagnostics=True)
    assert model.weights is not None and tuple(model.weights.shape) == (M, 3) and len(losses) >= 2
    assert all(b <= a for a, b in zip(losses, losses[1:])), losses
    assert getattr(ds2, "_pooled")[0] is model.kernel                                 # the fit ran on the pooled pair
    probs = model.predict(x[:50], _dense_data()[1][:50])
    assert probs.shape == (50, 3) and np.allclose(probs.sum(axis=1), 1.0)


# ---------------------------------------------------------------------------------------------- empty shard
def test_an_empty_local_shard_pools_nothing(monkeypatch, ext):
    from xgpr_amd.dataset import DeviceDataset
    x, sl, y, _ = _dense_data()
    empty = DeviceDataset(torch.from_numpy(x[:0]).to(DEV), torch.from_numpy(y[:0]).to(DEV), sl[:0], chunk_size=256, ndatapoints=N,
                          device=DEV)
    k = _kernel(x.shape, 70)
    seen = _count_pooling(monkeypatch, ext)
    p = empty.pooled(k)
    xp = p.get_xdata()
    assert seen["calls"] == 0 and tuple(xp.shape) == (0, 70) and xp.dtype == torch.float32 and xp.is_cuda
    assert p.get_ndatapoints() == N and p.get_local_ndatapoints() == 0 and empty.pooled(k) is p
