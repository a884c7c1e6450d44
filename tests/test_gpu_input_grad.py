"""The input gradient of the predictive mean and variance on the device (xgpr_rbf_input_grad_f32, SORFKernel.input_gradient,
xGPRegression.predict_gradient) against the long-double dense reference of tests/dense_input_grad.py, within its a-priori cap
``cap_input_grad`` (derived from the operation count, tests/test_input_grad_host.py shows what it separates).  Every comparison prints
one ``INGRAD`` line with measured error and cap; profiles/input_grad_errors.txt is the collection of those lines from one run."""
import numpy as np
import pytest
import torch

import dense_input_grad as dig
import dense_reference as dr
from dense_reference import U64

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64

DS = [2, 3, 9, 64, 100, 1000, 1024]         # P = 2 .. 1024, ragged widths, the 64- and 128-element layout changes, the full-width load
FS = [37, 300, 1024, 1324, 2048]            # less than a tile, F < P with one block, an exact tile, a ragged last tile, two full tiles
NS = [1, 5, 67]
MODES = ["shared", "rows", "rows_pad"]      # one vector; one row per datapoint with stride == w_cols; with stride > w_cols
WCOLS = ["full", "two", "second_tile"]      # 2 F; 2; a value ending inside the second tile (F >= 1324 only; 2 F elsewhere)


def _cases():
    out, k = [], 0
    for d in DS:
        for icpt in (True, False):
            for mode in MODES:
                F, n, wk = FS[k % 5], NS[(k + k // 5) % 3], WCOLS[(k + k // 3) % 3]
                if d >= 1000 and n == 67:
                    n = 5                                                  # (the long-double reference at P = 1024: seconds per 67 rows)
                if wk == "second_tile" and F < 1324:
                    wk = "full"
                out.append((d, F, n, icpt, mode, wk))
                k += 1
    return out


CASES = _cases()


def test_the_case_list_covers_every_axis_and_every_pair():
    assert {c[0] for c in CASES} == set(DS) and {c[1] for c in CASES} == set(FS) and {c[2] for c in CASES} == set(NS)
    assert {c[5] for c in CASES} == set(WCOLS)
    assert {(c[0], c[3], c[4]) for c in CASES} == {(d, i, m) for d in DS for i in (True, False) for m in MODES}


@pytest.fixture(scope="module")
def ext():
    from xgpr_amd import xgpr_hip_rfgen_ext as e
    return e


def w_cols_of(kind, F):
    return {"full": 2 * F, "two": 2, "second_tile": 2 * (1024 + 100)}[kind]


def device_weights(w, mode, w_cols):
    """shared: the vector; rows: a contiguous [n, w_cols] array (stride == w_cols); rows_pad: the [n, 2 F + 3] array whose pad is NaN."""
    if mode == "rows":
        w = np.ascontiguousarray(w[:, :w_cols])
    return torch.from_numpy(np.ascontiguousarray(w)).to(DEV)


def run_operator(ext, xs, w, radem, chi, sigma, icpt, w_cols):
    out = torch.full(xs.shape, float("nan"), dtype=F64, device=DEV)
    ext.hipRBFInputGrad(torch.from_numpy(xs).to(DEV), w, out, torch.from_numpy(radem).to(DEV), torch.from_numpy(chi).to(DEV), sigma, icpt,
                        w_cols=w_cols)
    return out


def report(tag, case, got, ref, cap):
    err = float(np.abs(got.astype(dr.LD) - ref).max())
    print(f"INGRAD {tag:<10} {str(case):<52} hip-dense {err:.3e}  cap {cap:.3e}  ratio {err / cap:.4f}")
    return err


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_operator_against_the_dense_reference(ext, case):
    d, F, n, icpt, mode, wk = case
    xs, w, radem, chi, sigma = dig.make_case(n, d, F, mode != "shared", seed=7, stride_pad=3 if mode == "rows_pad" else 0)
    w_cols = w_cols_of(wk, F)
    assert ext.rbf_input_grad_ok(d, F) == 1
    got = run_operator(ext, xs, device_weights(w, mode, w_cols), radem, chi, sigma, icpt, w_cols).cpu().numpy()
    ref = dig.rbf_input_grad(xs, w, radem, chi, sigma, icpt, w_cols=w_cols)
    cap = dig.cap_input_grad(xs, w, radem, chi, sigma, icpt, w_cols=w_cols)
    assert np.isfinite(got).all()
    assert report("operator", case, got, ref, cap) <= cap
    assert float(np.abs(ref).max()) > 100 * cap                            # (the comparison is not vacuous)


@pytest.mark.parametrize("d,F", [(9, 40), (100, 1324), (1024, 2048)])
def test_results_are_bit_identical_and_rows_are_independent(ext, d, F):
    """Two launches give equal bits; a row's result depends neither on n nor on its position: row 3 of 67 against the same row alone."""
    from guarded import same_bits
    n = 67
    xs, w, radem, chi, sigma = dig.make_case(n, d, F, True, seed=8)
    wd = device_weights(w, "rows", 2 * F)
    a = run_operator(ext, xs, wd, radem, chi, sigma, True, 2 * F)
    b = run_operator(ext, xs, wd, radem, chi, sigma, True, 2 * F)
    assert same_bits(a, b)
    alone = run_operator(ext, xs[3:4].copy(), wd[3:4].contiguous(), radem, chi, sigma, True, 2 * F)
    assert same_bits(a[3:4].contiguous(), alone)
    shared = run_operator(ext, xs, wd[3].contiguous(), radem, chi, sigma, True, 2 * F)      # ... nor on how the weights arrive
    assert same_bits(a[3:4].contiguous(), shared[3:4].contiguous())


def _kernel(choice, n, d, M, icpt=True, sigma=None):
    from xgpr_amd.kernels import SORFKernel
    k = SORFKernel(choice, (n, d), M, 123, DEV, {"matern_nu": 5 / 2, "intercept": icpt})
    k.set_hyperparams(np.asarray([0.9, 2.1 / np.sqrt(d) if sigma is None else sigma]), logspace=False)
    return k


def _kernel_operands(k, x):
    """x_scaled as SORFKernel.scaled_f32 forms it, and the kernel's own draws, on the host."""
    sigma = float(k.hyperparams[1])
    xs = (x.astype(np.float32).astype(np.float64) * sigma).astype(np.float32)
    return xs, k.radem_diag.cpu().numpy(), k.chi_arr.cpu().numpy(), sigma


def test_operator_against_the_composed_fallback_and_the_fallback_beyond_1024(ext):
    rng = np.random.default_rng(11)
    # d = 100, F = 1324: both routes, within the sum of their caps
    n, d, F = 5, 100, 1324
    k = _kernel("RBF", n, d, 2 * F)
    x = rng.uniform(-1, 1, size=(n, d))
    w = rng.standard_normal((n, 2 * F))
    xs, radem, chi, sigma = _kernel_operands(k, x)
    wd = torch.from_numpy(w).to(DEV)
    op = k.input_gradient(x, wd).cpu().numpy()
    fb = k.input_gradient_composed(torch.from_numpy(xs).to(DEV), wd, 2 * F).cpu().numpy()
    cap = dig.cap_input_grad(xs, w, radem, chi, sigma, True)
    ref = dig.rbf_input_grad(xs, w, radem, chi, sigma, True)
    report("op-vs-fb", (d, F, n), op, fb.astype(dr.LD), 2 * cap)
    assert float(np.abs(op - fb).max()) <= 2 * cap
    assert report("fallback", (d, F, n), fb, ref, cap) <= cap
    # d = 1500 (P = 2048): the operator refuses, the kernel object takes the composed route
    n, d, F = 2, 1500, 2100
    k = _kernel("RBF", n, d, 2 * F, icpt=False)
    x = rng.uniform(-1, 1, size=(n, d))
    w = rng.standard_normal(2 * F)
    xs, radem, chi, sigma = _kernel_operands(k, x)
    assert ext.rbf_input_grad_ok(d, F) == 0
    with pytest.raises(RuntimeError, match="padded width > 1024"):
        run_operator(ext, xs, torch.from_numpy(w).to(DEV), radem, chi, sigma, False, 2 * F)
    got = k.input_gradient(x, w).cpu().numpy()
    ref = dig.rbf_input_grad(xs, w, radem, chi, sigma, False)
    cap = dig.cap_input_grad(xs, w, radem, chi, sigma, False)
    assert report("fallback", (d, F, n), got, ref, cap) <= cap


@pytest.mark.parametrize("choice", ["RBF", "Matern", "Cauchy"])
def test_kernel_input_gradient(choice):
    n, d, M = 6, 20, 600
    k = _kernel(choice, n, d, M)
    rng = np.random.default_rng(12)
    x = rng.uniform(-1, 1, size=(n, d))
    w = rng.standard_normal(M)
    xs, radem, chi, sigma = _kernel_operands(k, x)
    got = k.input_gradient(x, w)
    assert got.dtype == F64 and tuple(got.shape) == (n, d) and got.is_cuda
    ref = dig.rbf_input_grad(xs, w, radem, chi, sigma, True)
    cap = dig.cap_input_grad(xs, w, radem, chi, sigma, True)
    assert report("kernel", (choice, d, M // 2, n), got.cpu().numpy(), ref, cap) <= cap
    with pytest.raises(RuntimeError):
        k.input_gradient(x, w, w_cols=7)


@pytest.fixture(scope="module")
def fitted():
    from xgpr_amd.dataset import build_regression_dataset
    from xgpr_amd.models import xGPRegression
    rng = np.random.default_rng(13)
    x = rng.uniform(-1, 1, size=(300, 20))
    y = np.sin(x[:, 0] * 2) + x[:, 1] * x[:, 2] + 3.0 + 0.05 * rng.standard_normal(300)
    ds = build_regression_dataset(x, y * 2.5, chunk_size=100, device=DEV)
    model = xGPRegression(num_rffs=256, variance_rffs=48, kernel_choice="RBF", device=DEV, verbose=False)
    model.set_hyperparams(np.log(np.asarray([0.3, 0.4])), ds)
    model.fit(ds, mode="exact")
    return model, ds, x


def test_predict_gradient(fitted):
    model, _, x = fitted
    xq = x[:40]
    k = model.kernel
    xs, radem, chi, sigma = _kernel_operands(k, xq)
    std = float(model.trainy_std)
    gm, gv = model.predict_gradient(xq, get_var=True, chunk_size=16)
    assert isinstance(gm, np.ndarray) and gm.shape == (40, 20) and gv.shape == (40, 20)
    assert np.array_equal(gm, model.predict_gradient(xq, chunk_size=16))
    # mean
    w = model.weights.cpu().numpy()
    ref = dig.rbf_input_grad(xs, w, radem, chi, sigma, True) * std
    cap = dig.cap_input_grad(xs, w, radem, chi, sigma, True) * std
    assert report("mean", ("RBF", 20, 128, 40), gm, ref, cap) <= cap + 4 * U64 * float(np.abs(ref).max())
    # variance: per-row weights 2 lambda^2 V z_v formed on the host from transform_x
    lam = float(k.get_lambda())
    var = model.var.cpu().numpy()
    nvar = var.shape[0]
    assert nvar == 48
    zv = k.transform_x(xq)[:, :nvar].cpu().numpy()
    wv = 2.0 * lam ** 2 * (zv @ var)
    ref = dig.rbf_input_grad(xs, wv, radem, chi, sigma, True, w_cols=nvar) * std ** 2
    cap = dig.cap_input_grad(xs, wv, radem, chi, sigma, True, w_cols=nvar) * std ** 2
    assert report("variance", ("RBF", 20, 128, 40), gv, ref, cap) <= cap + 4 * U64 * float(np.abs(ref).max())
    assert float(np.abs(gm).max()) > 0 and float(np.abs(gv).max()) > 0


def test_predict_gradient_refusals(fitted):
    from xgpr_amd.models import xGPRegression
    model, ds, x = fitted
    fresh = xGPRegression(num_rffs=256, variance_rffs=48, kernel_choice="RBF", device=DEV, verbose=False)
    with pytest.raises(RuntimeError, match="not yet been successfully fitted"):
        fresh.predict_gradient(x[:3])
    novar = xGPRegression(num_rffs=256, variance_rffs=48, kernel_choice="RBF", device=DEV, verbose=False)
    novar.set_hyperparams(np.log(np.asarray([0.3, 0.4])), ds)
    novar.fit(ds, mode="exact", suppress_var=True)
    assert novar.predict_gradient(x[:3]).shape == (3, 20)
    with pytest.raises(RuntimeError, match="suppress_var"):
        novar.predict_gradient(x[:3], get_var=True)
    ard = xGPRegression(num_rffs=256, variance_rffs=48, kernel_choice="MiniARD", device=DEV, verbose=False,
                        kernel_settings={"split_points": [7], "intercept": True})
    ard.set_hyperparams(dataset=ds)
    ard.weights = torch.zeros(256, dtype=F64, device=DEV)                  # (the refusal is about the kernel, not the fit)
    with pytest.raises(RuntimeError, match="RBF, Matern and Cauchy"):
        ard.predict_gradient(x[:3])
