"""Host-side logic of the exact NMLL gradient's float32-rows route (no GPU): the shape predicates, the float64 formulation
for CPU tensors, and the ``subsample`` range check (reference nmll_gradient_tools.py:37-38)."""
import numpy as np
import pytest
import torch


def _kernel(d, m, device="cpu", name="RBF"):
    from xgpr_amd.kernels import make_kernel
    parms = {"intercept": True}
    if name == "Matern":
        parms["matern_nu"] = 1.5
    return make_kernel(name, (10, d), m, 123, device, parms)


def test_cross_gram_ok_is_the_rule_of_gram_ok():
    from xgpr_amd import xgpr_hip_rfgen_ext as ext
    assert [ext.cross_gram_ok(m) for m in (128, 256, 384, 8192)] == [True] * 4
    assert [ext.cross_gram_ok(m) for m in (2, 64, 126, 130, 192, 1000, 8190)] == [False] * 7
    for m in (64, 128, 130, 192, 512):
        assert ext.cross_gram_ok(m) == ext.gram_ok(m, m)


@pytest.mark.parametrize("d,m,want", [(9, 256, True), (84, 384, True), (1000, 2048, True), (1500, 512, True),
                                      (3000, 512, True), (5000, 256, True), (8192, 128, True),
                                      (8193, 256, False),        # padded width 16384
                                      (9, 250, False), (9, 192, False), (1500, 1000, False)])       # not whole 128 x 128 tiles
def test_grad_rows_ok_over_widths_and_feature_counts(d, m, want, monkeypatch):
    """The predicate's shape rule, evaluated as on a HIP device (the arrays themselves stay on the host here)."""
    kern = _kernel(d, m)
    assert not kern.grad_rows_ok()                  # a CPU kernel never takes the route
    monkeypatch.setattr(kern, "device", "cuda")
    assert kern.grad_rows_ok() == want
    if want:
        assert kern.rows_ok()


def test_window_rows_keep_both_windows_within_the_budget(monkeypatch):
    from xgpr_amd import nmll, preconditioner
    assert nmll._grad_window_rows(8192) == 65536                    # 2 x 65536 x 8192 x 4 bytes = 4 GiB
    for m in (128, 256, 8192, 32768):
        rows = nmll._grad_window_rows(m)
        assert rows % 4 == 0 and 2 * rows * m * 4 <= preconditioner.ROW_WINDOW_BYTES
    monkeypatch.setattr(preconditioner, "ROW_WINDOW_BYTES", 1 << 20)
    assert nmll._grad_window_rows(8192) == 4096                     # the floor: windows of at least 4096 rows


def test_other_kernels_have_no_rows_route():
    from xgpr_amd.kernels import make_kernel
    from xgpr_amd import nmll
    for name, parms in (("MiniARD", {"split_points": [3]}), ("Linear", {})):
        kern = make_kernel(name, (10, 8), 128, 123, "cpu", parms)
        assert not hasattr(kern, "grad_rows_ok")

    class _DS:
        def get_xdata(self):
            raise AssertionError("the route must not be probed further")
    assert not nmll._grad_rows_route(_DS(), kern)


def test_cpu_tensors_take_the_float64_formulation(monkeypatch):
    """On CPU tensors calc_gradient_terms walks the chunks through gradient_x_y (stubbed here: there is no CPU operator) and
    symmetrises at the end, exactly as before."""
    from xgpr_amd import nmll
    from xgpr_amd.dataset import build_regression_dataset
    rng = np.random.default_rng(3)
    n, d, m = 70, 6, 128
    x = rng.standard_normal((n, d)).astype(np.float32)
    y = rng.standard_normal(n)
    ds = build_regression_dataset(x, y, chunk_size=32, device="cpu")
    kern = _kernel(d, m)
    zfull = torch.from_numpy(rng.standard_normal((n, m)))
    gfull = torch.from_numpy(rng.standard_normal((n, m, 1)))
    seen = []

    def fake_gradient_x_y(xin, yin, ldata=None):
        lo = sum(seen)
        seen.append(xin.shape[0])
        return zfull[lo:lo + xin.shape[0]], gfull[lo:lo + xin.shape[0]], yin
    monkeypatch.setattr(kern, "gradient_x_y", fake_gradient_x_y)
    monkeypatch.setattr(kern, "fill_grad_rows", lambda *a: (_ for _ in ()).throw(AssertionError("rows route on CPU tensors")))
    ztz, zty, yty, dzty, inner, nd = nmll.calc_gradient_terms(ds, kern)
    assert seen == [32, 32, 6] and nd == n
    yn = ds.normalized_y()
    assert torch.allclose(ztz, zfull.T @ zfull, rtol=1e-12, atol=1e-12)
    assert torch.allclose(zty, zfull.T @ yn, rtol=1e-12, atol=1e-12)
    assert torch.allclose(dzty[:, 0], gfull[:, :, 0].T @ yn, rtol=1e-12, atol=1e-12)
    gz = gfull[:, :, 0].T @ zfull
    assert torch.allclose(inner[:, :, 0], gz + gz.T, rtol=1e-12, atol=1e-12)
    assert np.isclose(yty, float(yn @ yn))


def test_subsample_draws_on_cpu_tensors(monkeypatch):
    """The reference's rule on the chunked float64 formulation: one generator seeded with 123, one choice per chunk."""
    from xgpr_amd import nmll
    from xgpr_amd.dataset import build_regression_dataset
    rng = np.random.default_rng(4)
    n, d, m = 100, 6, 128
    x = rng.standard_normal((n, d)).astype(np.float32)
    ds = build_regression_dataset(x, rng.standard_normal(n), chunk_size=40, device="cpu")
    kern = _kernel(d, m)
    got = []

    def fake_gradient_x_y(xin, yin, ldata=None):
        got.append(xin.clone())
        k = xin.shape[0]
        return torch.zeros((k, m), dtype=torch.float64), torch.zeros((k, m, 1), dtype=torch.float64), yin
    monkeypatch.setattr(kern, "gradient_x_y", fake_gradient_x_y)
    terms = nmll.calc_gradient_terms(ds, kern, subsample=0.3)
    draw = np.random.default_rng(123)
    xt = torch.from_numpy(x)
    for lo, chunk in zip((0, 40, 80), got):
        rows = min(40, n - lo)
        idx = draw.choice(rows, max(1, int(0.3 * rows)), replace=False)
        assert torch.equal(chunk, xt[lo + idx])
    assert terms[5] == 12 + 12 + 6


@pytest.mark.parametrize("bad", [0.0, 0.009, 1.01, 2, -1])
def test_subsample_range_check(bad):
    from xgpr_amd import nmll

    class _Never:
        def __getattr__(self, name):
            raise AssertionError("the range check comes first")
    with pytest.raises(RuntimeError, match=r"Subsample must be in the range \[0.01, 1\]"):
        nmll.calc_gradient_terms(_Never(), _Never(), subsample=bad)
    with pytest.raises(RuntimeError, match="Subsample"):
        nmll._check_subsample(bad)
    for ok in (0.01, 0.5, 1, 1.0):
        nmll._check_subsample(ok)
