"""Float32 feature rows beyond padded width 4096 (d >= 4097), where no fused regenerate-and-reduce kernel runs: the feature
cache writer on wave tiles (P = 8192) and on the any-width path (P >= 16384, global scratch beyond 32768 floats), z^T y
from float32 rows (hipZCacheZtY), and the solver's passes over resident or regenerated rows against the same passes on
float64 Z materialised chunk by chunk (the route forced by switching the rows predicates off)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ext():
    from xgpr_amd import xgpr_hip_rfgen_ext as e
    return e


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def rel(a, b):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    return float(np.abs(a - b).max() / np.abs(b).max())


def rbf_scale(F, icpt):
    return float(np.float32(np.sqrt(1.0 / (F - 0.5 if icpt else F))))


# (d, rffs, icpt, n): P = 8192 (wave tiles), 16384 / 32768 (any-width path in LDS), 65536 (global scratch); num_freqs > 8192
# and an incomplete last tile (5000, 20000: 10000 frequencies)
@pytest.mark.parametrize("d,rffs,icpt,n", [(4097, 8192, True, 300), (5000, 4000, False, 77), (8192, 16384, True, 40),
                                           (8193, 8192, False, 33), (20000, 16384, True, 6), (40000, 2048, True, 3),
                                           (5000, 20000, False, 9)])
def test_wide_feature_cache_and_cached_matvec(ext, oracle, d, rffs, icpt, n):
    """cache * scale == hipRBFFeatureGen bit for bit at the same width; the matvec streamed from it equals Z^T (Z v) of the
    oracle's features; a second build is bit-identical."""
    from oracle import oracle as orc
    rng = np.random.default_rng(d + rffs)
    radem, chi = orc.draw_sorf_params(rffs, d, 11)
    x = (rng.standard_normal((n, d)) / np.sqrt(d)).astype(np.float32)
    zc = torch.empty((n, rffs), dtype=torch.float32, device=DEV)
    ext.hipRBFFeatureCache(dev(x), zc, dev(radem), dev(chi))
    zf = torch.empty((n, rffs), dtype=torch.float64, device=DEV)
    ext.hipRBFFeatureGen(dev(x), zf, dev(radem), dev(chi), icpt)
    scale = rbf_scale(rffs // 2, icpt)
    assert torch.equal(zc.double() * scale, zf)
    zc2 = torch.full_like(zc, float("nan"))
    ext.hipRBFFeatureCache(dev(x), zc2, dev(radem), dev(chi))
    assert torch.equal(zc, zc2)
    z = np.zeros((n, rffs))
    oracle.cpuRBFFeatureGen(x.copy(), z, radem, chi, icpt)
    if icpt:
        z[:, 0] = 1.0
    v = rng.standard_normal(rffs)
    ref = z.T @ (z @ v)
    out = torch.zeros(rffs, dtype=torch.float64, device=DEV)
    ws = torch.empty(ext.ztz_workspace_bytes(rffs, radem.shape[2]), dtype=torch.uint8, device=DEV)
    ext.hipZCacheMatvec(zc, dev(v), out, icpt, ws)
    assert np.abs(out.cpu().numpy() - ref).max() <= 1e-6 * np.abs(ref).max()


@pytest.mark.parametrize("d,rffs,icpt,n", [(5000, 4000, True, 777), (9000, 16386, False, 5001), (5000, 8192, True, 4)])
def test_zcache_zty(ext, oracle, d, rffs, icpt, n):
    """z^T y from float32 rows: 1e-12 of the float64 product of the same rows, 1e-6 of the oracle's features, reproducible bit
    for bit; the RBF-family scale (scale = 0) and an explicit positive scale over complete rows."""
    from oracle import oracle as orc
    rng = np.random.default_rng(d + n)
    radem, chi = orc.draw_sorf_params(rffs, d, 5)
    x = (rng.standard_normal((n, d)) / np.sqrt(d)).astype(np.float32)
    y = rng.standard_normal(n)
    zc = torch.empty((n, rffs), dtype=torch.float32, device=DEV)
    ext.hipRBFFeatureCache(dev(x), zc, dev(radem), dev(chi))
    ws = torch.empty(ext.ztz_workspace_bytes(rffs, radem.shape[2]), dtype=torch.uint8, device=DEV)
    out = torch.full((rffs,), float("nan"), dtype=torch.float64, device=DEV)
    ext.hipZCacheZtY(zc, dev(y), out, icpt, ws)
    zz = zc.double() * rbf_scale(rffs // 2, icpt)
    if icpt:
        zz[:, 0] = 1.0
    assert rel(out, zz.T @ dev(y)) <= 1e-12
    z = np.zeros((n, rffs))
    oracle.cpuRBFFeatureGen(x.copy(), z, radem, chi, icpt)
    if icpt:
        z[:, 0] = 1.0
    assert rel(out, z.T @ y) <= 1e-6
    out2 = torch.zeros_like(out)
    ext.hipZCacheZtY(zc, dev(y), out2, icpt, ws)
    assert torch.equal(out, out2)
    # complete feature rows / scale (positive scale: no intercept convention)
    s = 0.37
    ext.hipZCacheZtY(zc, dev(y), out2, False, ws, scale=s)
    assert rel(out2, (zc.double() * s).T @ dev(y)) <= 1e-12


def test_zcache_zty_argument_checks(ext):
    n, m = 16, 64
    y = torch.ones(n, dtype=torch.float64, device=DEV)
    out = torch.zeros(m, dtype=torch.float64, device=DEV)
    ws = torch.empty(ext.ztz_workspace_bytes(m, 64), dtype=torch.uint8, device=DEV)
    zc = torch.ones((n, m), dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="even"):
        ext.hipZCacheZtY(torch.ones((n, 7), dtype=torch.float32, device=DEV), y,
                         torch.zeros(7, dtype=torch.float64, device=DEV), True, ws)
    flat = torch.ones(n * m + 1, dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="aligned"):
        ext.hipZCacheZtY(flat[1:].view(n, m), y, out, True, ws)
    with pytest.raises(RuntimeError, match="workspace"):
        ext.hipZCacheZtY(zc, y, out, True, ws[:256])
    with pytest.raises(TypeError):
        ext.hipZCacheZtY(zc, y[:-1], out, True, ws)
    ext.hipZCacheZtY(zc, y, out, False, ws, scale=1.0)
    assert torch.equal(out, torch.full_like(out, float(n)))


def _problem(d, n=6000, seed=None):
    rng = np.random.default_rng(d if seed is None else seed)
    x = (rng.standard_normal((n, d)) / np.sqrt(d)).astype(np.float32)
    w = rng.standard_normal(d)
    return x, w, rng


def _f64_route(monkeypatch):
    from xgpr_amd.kernels import SORFKernel
    for name in ("rows_ok", "cache_ok", "block_ok"):
        monkeypatch.setattr(SORFKernel, name, lambda self: False)


@pytest.mark.parametrize("d,m,method", [(5000, 4096, "srht"), (5000, 8192, "srht_2"), (9000, 8192, "srht"),
                                        (9000, 4096, "srht_2")])
def test_wide_fit_equals_the_materialised_float64_path(d, m, method, monkeypatch):
    """The whole k = 1 solve at padded width 8192 / 16384 -- z^T y, the preconditioner's passes over float32 rows, the CG
    matvec on the resident cache ("auto" keeps it) and on regenerated windows -- against the same solve on float64 Z
    materialised chunk by chunk (rows_ok / cache_ok / block_ok switched off).  Same iteration count (within one), weights
    to 1e-5 (1e-6 between the two float32-row routes), z^T y to 1e-7; the k = 26 block matvec and the k = 1 matvec to 1e-6."""
    from xgpr_amd.kernels import make_kernel
    from xgpr_amd.dataset import build_regression_dataset
    from xgpr_amd.preconditioner import RandNysPreconditioner
    from xgpr_amd.cg import cg_fit_lib_internal, calc_zty, ConjugateGrad, holds_cache
    x, wtrue, rng = _problem(d)
    y = np.sin(3.0 * x @ wtrue) + 0.1 * rng.standard_normal(x.shape[0])
    ds = build_regression_dataset(x, y, chunk_size=2000, device=DEV)
    vec = torch.from_numpy(np.random.default_rng(1).standard_normal((m, 26))).to(DEV)
    out = {}
    for route in ("resident", "windows", "f64"):
        kern = make_kernel("RBF", x.shape, m, 123, DEV, {})
        kern.set_hyperparams(np.array([0.3, 1.2]), logspace=False)
        if route == "f64":
            _f64_route(monkeypatch)
            assert not kern.cache_ok() and not kern.block_ok()
        else:
            assert not kern.fused_ok() and kern.rows_ok() and kern.cache_ok() and kern.block_ok()
        zty, yty = calc_zty(ds, kern)
        pre = RandNysPreconditioner(kern, ds, 128, False, 123, method)
        w, niter, _ = cg_fit_lib_internal(kern, ds, 1e-7, 300, pre, False,
                                          cache_features="auto" if route == "resident" else False)
        if route == "resident":
            assert holds_cache(ds, kern)
            zty_res, _ = calc_zty(ds, kern)              # now from the resident rows
            assert rel(zty_res, zty) < 1e-12
        mv = torch.zeros_like(vec)
        ConjugateGrad(cache_features=False)._matvec(ds, kern, vec, mv, add_ridge=False)
        mv1 = torch.zeros((m, 1), dtype=torch.float64, device=DEV)
        ConjugateGrad(cache_features=route == "resident")._matvec(ds, kern, vec[:, :1].contiguous(), mv1, add_ridge=False)
        out[route] = (zty, yty, w, niter, mv, mv1)
        monkeypatch.undo()
    zb, yb, wb, nb, mb, m1b = out["f64"]
    for route in ("resident", "windows"):
        za, ya, wa, na, ma, m1a = out[route]
        assert rel(za, zb) < 1e-7 and abs(ya - yb) <= 1e-12 * abs(yb)
        assert abs(na - nb) <= 1
        assert rel(wa, wb) < 1e-5
        assert rel(ma, mb) < 1e-6 and rel(m1a, m1b) < 1e-6
    assert out["resident"][3] == out["windows"][3]
    assert rel(out["resident"][2], out["windows"][2]) < 1e-6


def test_wide_cg_windows_with_a_ragged_last_window(monkeypatch):
    """The k = 1 matvec and z^T y over several regenerated windows (the last one short) equal the single-window result."""
    from xgpr_amd.kernels import make_kernel
    from xgpr_amd.dataset import build_regression_dataset
    from xgpr_amd.cg import ConjugateGrad, calc_zty
    x, wtrue, rng = _problem(5000, n=2500)
    ds = build_regression_dataset(x, x @ wtrue, chunk_size=2000, device=DEV)
    kern = make_kernel("RBF", x.shape, 2048, 123, DEV, {})
    kern.set_hyperparams(np.array([0.3, 1.2]), logspace=False)
    vec = torch.from_numpy(rng.standard_normal((2048, 1))).to(DEV)
    one = torch.zeros_like(vec)
    ConjugateGrad(cache_features=False)._matvec(ds, kern, vec, one, add_ridge=False)
    zty1, _ = calc_zty(ds, kern)
    monkeypatch.setattr(ConjugateGrad, "BLOCK_WINDOW_BYTES", 1024 * 4 * 2048)      # windows of 1024 rows: 1024, 1024, 452
    many = torch.zeros_like(vec)
    ConjugateGrad(cache_features=False)._matvec(ds, kern, vec, many, add_ridge=False)
    zty3, _ = calc_zty(ds, kern)
    assert rel(many, one) < 1e-12 and rel(zty3, zty1) < 1e-12


def test_wide_nmll_exact_predict_and_classifier_equal_the_float64_path(monkeypatch):
    """At d = 5000 (padded width 8192): the approximate NMLL (k = 26 probes), the exact-mode fit, variance and predicted mean,
    and a small classifier agree with the same computations on float64 Z (rows predicates off)."""
    from xgpr_amd.kernels import make_kernel
    from xgpr_amd.dataset import build_regression_dataset, build_classification_dataset
    from xgpr_amd import nmll
    from xgpr_amd.exact import calc_weights_exact, calc_variance_exact, predict_mean, gram_route
    from xgpr_amd.preconditioner import RandNysPreconditioner
    from xgpr_amd.classification import fit_classifier, predict_proba
    d = 5000
    x, wtrue, rng = _problem(d, n=3000, seed=7)
    y = np.sin(3.0 * x @ wtrue) + 0.1 * rng.standard_normal(x.shape[0])
    xtest = dev(x[:300] + 0.01)
    ds = build_regression_dataset(x, y, chunk_size=1000, device=DEV)
    labels = (np.digitize(x @ wtrue, [-0.5, 0.5])).astype(np.int64)
    cds = build_classification_dataset(x, labels, chunk_size=1000, device=DEV)
    res = {}
    for f64 in (False, True):
        if f64:
            _f64_route(monkeypatch)
        kern = make_kernel("RBF", x.shape, 1024, 123, DEV, {})
        kern.set_hyperparams(np.array([0.3, 1.2]), logspace=False)
        det = {}
        pre = RandNysPreconditioner(kern, ds, 256, False, 123, "srht_2")
        approx = nmll.approximate_nmll(kern, ds, pre, {"nsamples": 25, "nmll_iter": 500, "nmll_tol": 1e-6}, 123,
                                       cache_features=False, details=det)
        assert (gram_route(ds, kern, 1024) is None) == f64
        w, _, _ = calc_weights_exact(ds, kern)
        var = calc_variance_exact(kern, ds, 128)
        pm = predict_mean(kern, w, xtest, ds.get_ymean(), ds.get_ystd())
        ckern = make_kernel("RBF", x.shape, 1024, 123, DEV, {})
        ckern.set_hyperparams(np.array([0.3, 1.2]), logspace=False)
        cpre = RandNysPreconditioner(ckern, cds, 256, False, 123, "srht", is_regression=False)
        cw, gamma, cniter, closses = fit_classifier(ckern, cds, cpre, tol=1e-2, max_iter=500, cache_features=False)
        probs = predict_proba(ckern, cw, gamma, xtest)
        res[f64] = (approx, det, w, var, pm, cw, cniter, closses, probs)
        monkeypatch.undo()
    (a0, d0, w0, v0, p0, c0, n0, l0, pr0), (a1, d1, w1, v1, p1, c1, n1, l1, pr1) = res[False], res[True]
    assert np.isclose(a0, a1, rtol=1e-6)
    assert abs(d0["niter"] - d1["niter"]) <= 1
    assert np.isclose(d0["logdet"], d1["logdet"], rtol=1e-5)
    assert rel(w0, w1) < 1e-5 and rel(v0, v1) < 1e-5
    assert np.allclose(p0.cpu().numpy(), p1.cpu().numpy(), rtol=1e-5, atol=1e-6)
    assert n0 == n1 and np.allclose(l0, l1, rtol=1e-5)
    assert rel(c0, c1) < 1e-4
    assert np.allclose(pr0.cpu().numpy(), pr1.cpu().numpy(), rtol=1e-4, atol=1e-6)


def test_wide_fit_beyond_the_streaming_kernel_without_block_operators(monkeypatch):
    """20001 frequencies (num_rffs = 40002): rows can be written, but the k = 1 matvec has neither the streaming kernel
    (<= 16384 frequencies) nor the block contractions (num_rffs % 4 != 0) -- cache_ok is False, so the CG solve keeps the
    float64 route while z^T y and the preconditioner use float32 rows.  The fit equals the fully float64 one."""
    from xgpr_amd.kernels import make_kernel
    from xgpr_amd.dataset import build_regression_dataset
    from xgpr_amd.preconditioner import RandNysPreconditioner
    from xgpr_amd.cg import cg_fit_lib_internal, calc_zty, ConjugateGrad, rows_matvec_ok
    m = 40002
    x, wtrue, rng = _problem(5000, n=1500, seed=3)
    y = np.sin(3.0 * x @ wtrue) + 0.1 * rng.standard_normal(x.shape[0])
    ds = build_regression_dataset(x, y, chunk_size=500, device=DEV)
    out = {}
    for f64 in (False, True):
        if f64:
            _f64_route(monkeypatch)
        kern = make_kernel("RBF", x.shape, m, 123, DEV, {})
        kern.set_hyperparams(np.array([0.3, 1.2]), logspace=False)
        assert not kern.cache_ok() and not kern.block_ok() and not rows_matvec_ok(kern)
        assert kern.rows_ok() != f64
        zty, _ = calc_zty(ds, kern)
        pre = RandNysPreconditioner(kern, ds, 128, False, 123, "srht")
        w, niter, _ = cg_fit_lib_internal(kern, ds, 1e-7, 300, pre, False, cache_features="auto")
        mv = torch.zeros((m, 1), dtype=torch.float64, device=DEV)
        ConjugateGrad(cache_features=True)._matvec(ds, kern, torch.ones((m, 1), dtype=torch.float64, device=DEV), mv,
                                                   add_ridge=False)
        out[f64] = (zty, w, niter, mv)
        monkeypatch.undo()
    (za, wa, na, ma), (zb, wb, nb, mb) = out[False], out[True]
    assert rel(za, zb) < 1e-7
    assert abs(na - nb) <= 1 and rel(wa, wb) < 1e-5
    assert rel(ma, mb) < 1e-12
