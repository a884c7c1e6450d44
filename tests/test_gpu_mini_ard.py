"""MiniARD on the device, from the operator up to the model: hipMiniARDGrad against the dense-matrix reference
(tests/dense_reference.py) and the CPU oracle at the edge shapes of tests/test_dense_reference_cpu.py (``ARD``), the
MiniARDKernel object on both of its routes, the exact NMLL gradient of a multi-lengthscale kernel, and the solver passes that
MiniARD takes through the generic float64-Z branches (CG, preconditioner, exact fit, predict).

Every tolerance is a derived cap of tests/dense_reference.py, a number an existing test already uses for the same comparison
(named where it is used), or the measured error of the central difference with its stated margin."""
import numpy as np
import pytest
import torch

import dense_reference as dr
from test_dense_reference_cpu import (ARD, ARD_ABSENT, ARD_KERNELS, NMLL_ARD, ard_case, ard_weight_cap, central_difference, maxerr,
                                      nmll_ard_problem, oracle_mini_ard, report)

pytestmark = pytest.mark.gpu

DEV = "cuda"
BOTH = [np.float32, np.float64]
NAN = float("nan")


@pytest.fixture(scope="module")
def ext():
    from xgpr_amd import xgpr_hip_rfgen_ext as e
    return e


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def rel(a, b):
    """As tests/test_gpu_cg.py."""
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
    b = b.cpu().numpy() if isinstance(b, torch.Tensor) else b
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def guarded(n, *tail):
    """The first n rows of a NaN-filled buffer one row longer -> (view, buffer)."""
    buf = torch.full((n + 1,) + tail, NAN, dtype=torch.float64, device=DEV)
    return buf[:n], buf


# ---------------------------------------------------------------------------------------------------- the operator
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("icpt", [False, True])
@pytest.mark.parametrize("n,d,F,nl,kind", ARD)
def test_mini_ard_grad_operator(ext, oracle, n, d, F, nl, kind, icpt, dtype):
    """hipMiniARDGrad within the dense reference's cap and within the parity tolerances of
    test_g12_mini_ard_grad_and_kernel_vs_reference_ground_truth against the oracle; everything inside [n, 2F(, nl)] written,
    nothing past it, the slice of a group no column belongs to exactly zero, the inputs untouched."""
    case = ard_case(n, d, F, nl, kind)
    x, w = case.typed(dtype)
    rf, rg = case.ref(dtype, icpt)
    of, og = oracle_mini_ard(oracle, case, dtype, icpt)
    capf, capg = case.caps(dtype, icpt)
    ins = [dev(x), dev(w), dev(case.sigma_map), dev(case.sigma_vals)]
    before = [t.clone() for t in ins]
    out, out_buf = guarded(n, 2 * F)
    grad, grad_buf = guarded(n, 2 * F, nl)
    ext.hipMiniARDGrad(ins[0], out, ins[1], ins[2], ins[3], grad, icpt)
    torch.cuda.synchronize()
    hf, hg = host(out), host(grad)
    assert not np.isnan(hf).any() and not np.isnan(hg).any()
    assert np.isnan(host(out_buf[n])).all() and np.isnan(host(grad_buf[n])).all()
    for t, b in zip(ins, before):
        assert torch.equal(t.view(torch.uint8), b.view(torch.uint8))
    if kind == "absent":
        assert np.all(hg[:, :, ARD_ABSENT] == 0.0) and np.all(og[:, :, ARD_ABSENT] == 0.0)
    ef, eg = maxerr(hf, rf), maxerr(hg, rg)
    report(f"mini_ard.f i={int(icpt)}", case, dtype, maxerr(of, rf), capf, hip=ef)
    report(f"mini_ard.g i={int(icpt)}", case, dtype, maxerr(og, rg), capg, hip=eg)
    assert ef <= capf and eg <= capg
    assert maxerr(of, rf) <= capf and maxerr(og, rg) <= capg
    assert np.allclose(hf, of, rtol=1e-9, atol=1e-11)
    assert np.allclose(hg, og, rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("dtype", BOTH)
def test_mini_ard_grad_inputs_one_element_into_their_allocations(ext, dtype):
    """x and W as views one element (4 bytes float32, 8 bytes float64) into their allocations: bit-identical results."""
    n, d, F, nl, kind = ARD[4]
    case = ard_case(n, d, F, nl, kind)
    x, w = case.typed(dtype)
    smap, svals = dev(case.sigma_map), dev(case.sigma_vals)
    res = []
    for shift in (0, 1):
        xb = torch.zeros(n * d + 5, dtype=torch.float32 if dtype == np.float32 else torch.float64, device=DEV)
        wb = torch.zeros(F * d + 5, dtype=xb.dtype, device=DEV)
        lead = [b.data_ptr() % 16 // b.element_size() for b in (xb, wb)]          # elements past a 16-byte boundary
        xoff, woff = [(shift - l) % (16 // xb.element_size()) for l in lead]
        xv, wv = xb[xoff:xoff + n * d].view(n, d), wb[woff:woff + F * d].view(F, d)
        assert xv.data_ptr() % 16 == shift * xb.element_size() and wv.data_ptr() % 16 == shift * xb.element_size()
        xv.copy_(dev(x))
        wv.copy_(dev(w))
        out, _ = guarded(n, 2 * F)
        grad, _ = guarded(n, 2 * F, nl)
        ext.hipMiniARDGrad(xv, out, wv, smap, svals, grad, True)
        res.append((out.clone(), grad.clone()))
    assert not torch.isnan(res[0][0]).any() and not torch.isnan(res[0][1]).any()
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


# ---------------------------------------------------------------------------------------------------- the kernel object
def _kernel_pair(oracle, d, rffs, splits, dp, icpt, n=7):
    """MiniARDKernel and OracleMiniARDKernel with the same draws and hyperparameters, and an input of float32 values."""
    from oracle import oracle as omod
    from xgpr_amd.kernels import MiniARDKernel
    rng = np.random.default_rng([d, rffs, len(splits)])
    x = (rng.standard_normal((n, d)) / np.sqrt(d)).astype(np.float32).astype(np.float64)
    ngroups = len(splits) + 1
    hp = np.concatenate([[0.7], 0.5 + 1.5 * (rng.permutation(ngroups) + 0.5) / ngroups])
    kern = MiniARDKernel(x.shape, rffs, 123, DEV, dp, {"split_points": list(splits), "intercept": icpt})
    kern.set_hyperparams(hp, logspace=False)
    okern = omod.OracleMiniARDKernel(rffs, x.shape, list(splits), hp, 123, double_precision=dp, fit_intercept=icpt, ops=oracle)
    return kern, okern, x


@pytest.mark.parametrize("dp", [False, True])
@pytest.mark.parametrize("icpt", [False, True])
@pytest.mark.parametrize("d,rffs,splits", ARD_KERNELS)
def test_mini_ard_kernel_object(oracle, d, rffs, splits, icpt, dp):
    """precomputed_weights, transform_x (the SORF route) and gradient_x (the dense route) of MiniARDKernel, each against the
    dense reference within its cap; the two routes' features then agree within the sum of their caps."""
    kern, okern, x = _kernel_pair(oracle, d, rffs, splits, dp, icpt)
    dtype = np.float64 if dp else np.float32
    nl = len(splits) + 1
    kern.precompute_weights()
    okern.precompute_weights()
    w = host(kern.precomputed_weights)
    radem, chi = host(kern.radem_diag), host(kern.chi_arr)
    assert np.array_equal(radem, okern.radem_diag) and np.array_equal(chi, okern.chi_arr) and chi.dtype == dtype
    wref = dr.mini_ard_weights(d, radem, chi)
    err, cap = maxerr(w, wref), ard_weight_cap(dtype, d, chi, wref)
    report("mini_ard.W", (d, rffs), dtype, maxerr(okern.precomputed_weights, wref), cap, hip=err)
    assert err <= cap and w.dtype == dtype
    assert np.array_equal(w, okern.precomputed_weights)
    smap, svals = host(kern.ard_position_key), host(kern.full_ard_weights)
    assert np.array_equal(smap, okern.ard_position_key) and np.array_equal(svals, okern.full_ard_weights)
    # the SORF route: the input scaled per column and rounded to the kernel's type, then the RBF features
    xs = (x * svals[None, :]).astype(dtype)
    tref = dr.rbf_features(xs, radem, chi, icpt)
    if icpt:
        tref[:, 0] = 1
    tcap = dr.cap_rbf(dtype, xs, chi, icpt)
    tx = host(kern.transform_x(x))
    report(f"mini_ard.tx i={int(icpt)}", (d, rffs), dtype, maxerr(okern.transform_x(x), tref), tcap, hip=maxerr(tx, tref))
    assert maxerr(tx, tref) <= tcap
    # the dense route
    gf, gg = kern.gradient_x(x)
    gf, gg = host(gf), host(gg)
    assert gg.shape == (x.shape[0], rffs, nl)
    rf, rg = dr.mini_ard_grad(x.astype(dtype), w, smap, svals, icpt, nl)
    if icpt:
        rf[:, 0] = 1
        rg[:, 0, :] = 0
    capf, capg = dr.cap_mini_ard(dtype, x.astype(dtype), w, smap, svals, icpt, nl)
    of, og = okern.gradient_x(x)
    report(f"mini_ard.kf i={int(icpt)}", (d, rffs), dtype, maxerr(of, rf), capf, hip=maxerr(gf, rf))
    report(f"mini_ard.kg i={int(icpt)}", (d, rffs), dtype, maxerr(og, rg), capg, hip=maxerr(gg, rg))
    assert maxerr(gf, rf) <= capf and maxerr(gg, rg) <= capg
    # the two routes compute the same features (x W^T, sigma-weighted, is the projection of the scaled row): they agree within
    # the sum of their caps -- the property the reference's own MiniARD test rests on
    print(f"ROUTES mini_ard {(d, rffs)} {np.dtype(dtype).name} i={int(icpt)}: |transform_x - gradient_x features| "
          f"{np.abs(tx - gf).max():.3e}  caps {tcap:.3e} + {capf:.3e}")
    assert np.abs(tx - gf).max() <= tcap + capf


def test_mini_ard_nine_groups_transform_works_gradient_refused(oracle):
    """Nine lengthscale groups: the SORF route serves them, the gradient operator refuses with the launcher's message, and the
    refusal leaves nothing behind: a valid call right after it is correct."""
    from xgpr_amd.kernels import MiniARDKernel
    d, rffs = 64, 128
    kern9, okern9, x = _kernel_pair(oracle, d, rffs, [1, 2, 3, 4, 5, 6, 7, 8], False, True)
    scale = np.sqrt(1.0 / (rffs // 2 - 0.5))
    assert np.abs(host(kern9.transform_x(x)) - okern9.transform_x(x)).max() <= 4e-7 * scale           # the bar of test_g7_cg_iterates
    with pytest.raises(RuntimeError, match="MiniARD gradient supports up to 8 lengthscale groups"):
        kern9.gradient_x(x)
    kern, okern, x = _kernel_pair(oracle, d, rffs, ARD_KERNELS[2][2], False, True)
    f, g = kern.gradient_x(x)
    of, og = okern.gradient_x(x)
    assert isinstance(kern, MiniARDKernel)
    assert np.allclose(host(f), of, rtol=1e-9, atol=1e-11) and np.allclose(host(g), og, rtol=1e-9, atol=1e-9)


# ---------------------------------------------------------------------------------------------------- the NMLL gradient
# Deviation of the ORACLE's exact_nmll_gradient from the central difference of its own exact_nmll on this problem
# (test_oracle_mini_ard_nmll_gradient_against_central_difference prints it): the truncation error of the difference, not of
# the code.  The device gradient is held to 4 x that, in the absolute and in the relative term.
FD_MEASURED_ABS = 7.848e-04   # "NMLLFD mini_ard oracle: largest absolute deviation 7.848e-04  largest relative deviation 2.654e-06"
FD_MEASURED_REL = 2.654e-06   # (gradient entries of size 34 to 296, eps = 1e-3 in log space)
FD_MARGIN = 4.0


@pytest.fixture(scope="module")
def nmll_case():
    from xgpr_amd.dataset import build_regression_dataset
    from xgpr_amd.kernels import MiniARDKernel
    p = NMLL_ARD
    x, y = nmll_ard_problem()
    ds = build_regression_dataset(x, y, chunk_size=p["chunk"], device=DEV)

    def kernel(hp, dp=True):
        k = MiniARDKernel(x.shape, p["rffs"], 123, DEV, dp, {"split_points": list(p["splits"])})
        k.set_hyperparams(np.asarray(hp, dtype=np.float64), logspace=False)
        return k
    return dict(x=x, y=y, ds=ds, kernel=kernel, **p)


def test_mini_ard_nmll_gradient_equals_the_oracle(oracle, nmll_case):
    from oracle import oracle as omod
    from xgpr_amd import nmll
    c = nmll_case
    kern = c["kernel"](c["hparams"])
    assert kern.get_hyperparams().shape[0] == 4 and not nmll._grad_rows_route(c["ds"], kern)
    score, grad = nmll.exact_nmll_gradient(kern, c["ds"])
    ods = omod.OracleDataset(c["x"], c["y"], None, chunk_size=c["chunk"])
    okern = omod.OracleMiniARDKernel(c["rffs"], c["x"].shape, c["splits"], c["hparams"], 123, double_precision=True, ops=oracle)
    oscore, ograd = omod.exact_nmll_gradient(okern, ods)
    print(f"NMLL mini_ard: device {score!r} {grad}  oracle {oscore!r} {ograd}")
    assert grad.shape == (4,)
    assert np.isclose(score, oscore, rtol=1e-8) and np.allclose(grad, ograd, rtol=1e-8, atol=0.0)


def test_mini_ard_nmll_gradient_against_central_difference(nmll_case):
    from xgpr_amd import nmll
    c = nmll_case
    _, grad = nmll.exact_nmll_gradient(c["kernel"](c["hparams"]), c["ds"])
    fd = central_difference(lambda hp: nmll.exact_nmll(c["kernel"](hp), c["ds"]), c["hparams"], c["eps"])
    dev_abs = np.abs(grad - fd)
    print(f"NMLLFD mini_ard device: gradient {grad}  central difference {fd}  largest absolute deviation {dev_abs.max():.3e}  "
          f"largest relative deviation {(dev_abs / np.abs(fd)).max():.3e}")
    assert np.all(dev_abs <= FD_MARGIN * FD_MEASURED_ABS + FD_MARGIN * FD_MEASURED_REL * np.abs(fd))


def _host_gradient_terms(kern, ds, rows_per_chunk=None):
    """The sums of calc_gradient_terms formed on the host in float64 from kernel.gradient_x, chunk by chunk;
    ``rows_per_chunk``: the rows of every chunk that take part (all when None)."""
    m, nk = kern.get_num_rffs(), kern.get_hyperparams().shape[0] - 1
    ztz, zty, yty = np.zeros((m, m)), np.zeros(m), 0.0
    dzty, inner = np.zeros((m, nk)), np.zeros((m, m, nk))
    used = 0
    for ci, (xin, yin, _) in enumerate(ds.get_chunked_data()):
        if rows_per_chunk is not None:
            idx = torch.from_numpy(rows_per_chunk[ci]).to(DEV)
            xin, yin = xin[idx], yin[idx]
        z, dz = kern.gradient_x(xin)
        z, dz, yv = host(z), host(dz), host(yin)
        used += z.shape[0]
        ztz += z.T @ z
        zty += z.T @ yv
        yty += float(yv @ yv)
        for i in range(nk):
            dzty[:, i] += dz[:, :, i].T @ yv
            inner[:, :, i] += dz[:, :, i].T @ z
    inner += np.transpose(inner, (1, 0, 2))
    return ztz, zty, yty, dzty, inner, used


def _assert_terms(terms, want, rtol=1e-12):
    for i, (got, ref) in enumerate(zip(terms[:5], want[:5])):
        got = host(got) if isinstance(got, torch.Tensor) else np.asarray(got)
        assert np.abs(got - ref).max() <= rtol * np.abs(ref).max(), i
    assert terms[5] == want[5]


def test_mini_ard_gradient_terms_equal_host_sums(nmll_case):
    """calc_gradient_terms of a three-lengthscale kernel (the per-lengthscale accumulation loop, a ragged last chunk of 44 rows)."""
    from xgpr_amd import nmll
    c = nmll_case
    kern = c["kernel"](c["hparams"])
    terms = nmll.calc_gradient_terms(c["ds"], kern)
    assert tuple(terms[3].shape) == (c["rffs"], 3) and tuple(terms[4].shape) == (c["rffs"], c["rffs"], 3)
    _assert_terms(terms, _host_gradient_terms(kern, c["ds"]))


def test_mini_ard_subsample_draws_the_rows_rbf_draws(nmll_case):
    """subsample = 0.25: the rows are drawn before any kernel is asked, so MiniARD and RBF see the same ones -- the same count and
    bit for bit the same y^T y -- and they are the rows of the documented draw (one generator seeded with 123, one choice without
    replacement per chunk): MiniARD's terms equal the host sums over exactly those rows."""
    from xgpr_amd import nmll
    from xgpr_amd.kernels import make_kernel
    c = nmll_case
    kern = c["kernel"](c["hparams"])
    rbf = make_kernel("RBF", c["x"].shape, c["rffs"], 123, DEV, {})
    rbf.set_hyperparams(np.array([0.45, 0.8]), logspace=False)
    terms = nmll.calc_gradient_terms(c["ds"], kern, subsample=0.25)
    rterms = nmll.calc_gradient_terms(c["ds"], rbf, subsample=0.25)
    assert terms[5] == rterms[5] == 32 + 32 + 11 and terms[2] == rterms[2]
    rng = np.random.default_rng(123)
    picks = []
    for lo in range(0, c["n"], c["chunk"]):
        rows = min(c["chunk"], c["n"] - lo)
        picks.append(rng.choice(rows, max(1, int(0.25 * rows)), replace=False))
    _assert_terms(terms, _host_gradient_terms(kern, c["ds"], picks))


# ---------------------------------------------------------------------------------------------------- the generic solver branch
SOLVE = dict(n=600, d=20, splits=[5, 12], rffs=256, chunk=250, hparams=np.array([0.6, 0.7, 1.4, 0.9]))


@pytest.fixture(scope="module")
def solve_case():
    from xgpr_amd.dataset import build_regression_dataset
    from xgpr_amd.kernels import make_kernel
    p = SOLVE
    rng = np.random.default_rng(600)
    x = rng.uniform(-1, 1, size=(p["n"], p["d"])).astype(np.float32)
    y = np.sin(2 * x[:, 0]) + x[:, 7] * x[:, 8] + 0.5 * x[:, 15] + 0.1 * rng.standard_normal(p["n"])
    xtest = rng.uniform(-1, 1, size=(37, p["d"])).astype(np.float32)
    ds = build_regression_dataset(x, y, chunk_size=p["chunk"], device=DEV)
    kern = make_kernel("MiniARD", x.shape, p["rffs"], 123, DEV, {"split_points": list(p["splits"])})
    kern.set_hyperparams(p["hparams"], logspace=False)
    z = host(kern.transform_x(x))                                   # float64 features, one call
    yn = (y - y.mean()) / y.std()
    lam = p["hparams"][0]

    def ridge(diag):
        return np.linalg.solve(z.T @ z + diag * np.eye(p["rffs"]), z.T @ yn)
    return dict(x=x, y=y, xtest=xtest, ds=ds, kern=kern, z=z, yn=yn, lam=lam, ridge=ridge, **p)


@pytest.mark.parametrize("precond", [False, True])
def test_mini_ard_cg_fit_equals_ridge_regression(solve_case, precond):
    """cg_fit_lib_internal on the float64-Z branch of the matvec (and of the preconditioner's accumulation pass) against the
    closed form from the kernel's own features; the bar of test_linear_kernel_fit_equals_ridge_regression."""
    from xgpr_amd.cg import cg_fit_lib_internal, any_rows_ok
    from xgpr_amd.preconditioner import RandNysPreconditioner
    c = solve_case
    assert not c["kern"].fused_ok() and not any_rows_ok(c["kern"], c["ds"])
    pre = RandNysPreconditioner(c["kern"], c["ds"], 32, False, 123, "srht") if precond else None
    w, niter, _ = cg_fit_lib_internal(c["kern"], c["ds"], 1e-12, 500, pre, False)
    err = rel(w, c["ridge"](c["lam"] ** 2))
    print(f"SOLVE mini_ard cg precond={precond}: {niter} iterations, relative error {err:.3e}")
    assert err < 1e-8


def test_mini_ard_exact_fit_equals_ridge_regression(solve_case):
    """calc_weights_exact: as documented there (and as the reference does) lambda^2 reaches the diagonal twice, so the closed
    form it must equal is the ridge solution with 2 lambda^2."""
    from xgpr_amd.exact import calc_weights_exact, gram_route
    c = solve_case
    assert gram_route(c["ds"], c["kern"], c["rffs"]) is None           # the generic float64 branch
    w, _, _ = calc_weights_exact(c["ds"], c["kern"])
    assert rel(w, c["ridge"](2 * c["lam"] ** 2)) < 1e-8


def test_mini_ard_model_fit_predict_and_half_cache_request(solve_case):
    """xGPRegression with kernel_choice="MiniARD": set_hyperparams, fit, predict with the variance; the mean is Z_test w and the
    variance the reference formula on the host from the same features.  cache_features="half" is a request MiniARD cannot serve:
    as test_unsupported_width_falls_back_to_the_float32_cache establishes, it is answered like True -- no error, same weights."""
    from xgpr_amd.models import xGPRegression
    from xgpr_amd.cg import _resolve_cache_mode
    from xgpr_amd.preconditioner import RandNysPreconditioner
    c = solve_case
    nvar = 48
    models = {}
    for mode in ("auto", "half"):
        model = xGPRegression(num_rffs=c["rffs"], variance_rffs=nvar, kernel_choice="MiniARD", device=DEV, verbose=False, random_seed=123,
                              kernel_settings={"split_points": list(c["splits"])})
        model.set_hyperparams(np.log(c["hparams"]), c["ds"])
        assert np.array_equal(model.kernel.get_hyperparams(logspace=False), np.exp(np.log(c["hparams"])))
        pre = RandNysPreconditioner(model.kernel, c["ds"], 32, False, 123, "srht")
        model.fit(c["ds"], preconditioner=pre, tol=1e-12, cache_features=mode)
        assert getattr(c["ds"], "_zcache16", None) is None
        models[mode] = model
    assert _resolve_cache_mode("half", models["half"].kernel, c["ds"]) is True
    assert torch.equal(models["half"].weights, models["auto"].weights)
    model = models["auto"]
    w = host(model.weights)
    assert rel(w, c["ridge"](c["lam"] ** 2)) < 1e-8
    ztest = host(model.kernel.transform_x(c["xtest"]))
    preds, var = model.predict(c["xtest"], get_var=True, chunk_size=16)
    ymean, ystd = c["y"].mean(), c["y"].std()
    assert rel(preds, (ztest @ w) * ystd + ymean) < 1e-12            # a float64 contraction: the bar of test_block_matvec_vs_oracle
    zv, lam2 = c["z"][:, :nvar], c["lam"] ** 2
    vmat = np.linalg.pinv(zv.T @ zv + lam2 * np.eye(nvar), hermitian=True)
    xv = ztest[:, :nvar]
    vref = (lam2 + lam2 * np.einsum("ij,jk,ik->i", xv, vmat, xv)).clip(min=0) * ystd ** 2
    print(f"SOLVE mini_ard predict: variance relative error {rel(var, vref):.3e}")
    assert rel(var, vref) < 1e-8
