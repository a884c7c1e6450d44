"""The conditions on tests/dense_solver_steps.py that tests/test_gpu_solver_steps.py relies on, at every shape it uses; no GPU.

* A correct float64 implementation passes: the formulas in plain numpy float64, summed pairwise (np.sum) and strictly
  in sequence (np.cumsum(...)[-1]), stay inside every cap against the longdouble reference.  This is the condition on
  the input builders -- a shape that failed here would need other inputs, never a wider cap.
* A wrong one does not: every planted mistake that applies at a shape leaves a cap by at least 100x on some output, and
  every shape is hit by at least one.
* The stop_tol state machine: a stop after iteration 1, no stop within max_iterations, and stop_tol exactly equal to an
  iteration's error (the test is <, so equality goes on).
"""
import numpy as np
import pytest

import dense_solver_steps as D

LD = D.LD
SUMS = {"pairwise": lambda a: a.sum(axis=0), "sequential": lambda a: np.cumsum(a, axis=0)[-1]}
ALL_SINGLE = sorted(set(D.SINGLE_M + D.STOP_M + [D.CHAIN_M]))
PRECOND_ALL = [(m, r, None) for m, r in D.PRECOND_SHAPES + [D.PRECOND_UNALIGNED]] + list(D.PRECOND_BLOCK_SHAPES)


def f64(a):
    return np.asarray(a, dtype=np.float64)


def float64_steps(a, total):
    w = a["w"] + a["lam2"] * a["p"]
    rz = total(a["r"] * a["z"])
    alpha = rz / total(a["p"] * w)
    got = {"w": w, "x": a["x"] + alpha * a["p"], "r_next": a["r"] - alpha * w, "rz": rz, "alpha": alpha,
           "err": np.sqrt(total(a["r"] * a["r"])) / a["init_norm"]}
    got["z_next"] = got["r_next"] * a["dn"]
    got["beta"] = total(got["r_next"] * got["z_next"]) / rz
    got["p_next"] = got["z_next"] + got["beta"] * a["p"]
    return got


def mistaken_steps(a, mistake):
    got = dict(zip(("w", "x", "r_next", "rz", "alpha", "err"),
                   (f64(v) for v in D.cg_step1(a["w"], a["p"], a["x"], a["r"], a["z"], a["lam2"], a["init_norm"], mistake))))
    got["z_next"] = got["r_next"] * a["dn"]
    got["p_next"], got["beta"] = (f64(v) for v in D.cg_step2(got["r_next"], got["z_next"], a["p"], got["rz"], mistake))
    return got


def steps_inputs(M, k):
    return D.single_inputs(M) if k is None else D.block_inputs(M, k)


STEP_SHAPES = [(M, None) for M in ALL_SINGLE] + list(D.BLOCK_SHAPES)


# ---------------------------------------------------------------------------------------------------- builders
@pytest.mark.parametrize("M,k", STEP_SHAPES)
def test_sentinel_rows_carry_a_hundredth_of_every_dot_product(M, k):
    a = steps_inputs(M, k)
    rows = D.sentinel_rows(M) if k is None else D.block_sentinel_rows(M)
    w2, _, rn, _, _, _ = D.cg_step1(a["w"], a["p"], a["x"], a["r"], a["z"], a["lam2"], a["init_norm"])
    zn = f64(rn) * a["dn"]
    for name, prod in (("r.z", a["r"] * a["z"]), ("p.w", a["p"] * f64(w2)), ("r.r", a["r"] * a["r"]), ("r_next.z_next", f64(rn) * zn)):
        assert (prod >= 0).all(), name                                   # sum |a b| = |sum a b|
        share = prod[rows] / prod.sum(axis=0)
        assert share.min() >= 0.01, (name, float(share.min()))


def test_block_columns_differ_in_scale_alpha_and_norm():
    a = D.block_inputs(513, 31)
    _, _, _, rz, alpha, err = D.cg_step1(a["w"], a["p"], a["x"], a["r"], a["z"], a["lam2"], a["init_norm"])
    for v in (rz, alpha, err):
        v = np.sort(f64(v))
        assert (np.diff(v) > 1e-4 * v[1:]).all()


# ---------------------------------------------------------------------------------------------------- float64 inside the caps
@pytest.mark.parametrize("order", sorted(SUMS))
@pytest.mark.parametrize("M,k", STEP_SHAPES)
def test_float64_steps_stay_inside_the_caps(M, k, order):
    a = steps_inputs(M, k)
    ratios = D.step_ratios(a, float64_steps(a, SUMS[order]))
    assert max(ratios.values()) <= 1.0, ratios


def float64_precond(a, total, three):
    u, r = a["u"], a["r"]
    col = (lambda c: c[:, None]) if r.ndim == 2 else (lambda c: c)
    t = np.stack([total((u[:, j] * r.T).T) for j in range(u.shape[1])])
    if three:
        ut = np.stack([total((u[i] * (col(a["inv_eig"] * a["prefactor"]) * t).T).T) for i in range(u.shape[0])])
        uut = np.stack([total((u[i] * t.T).T) for i in range(u.shape[0])])
        return ut + (r - uut)
    s = col(a["inv_eig"] * a["prefactor"] - 1.0) * t
    return r + np.stack([total((u[i] * s.T).T) for i in range(u.shape[0])])


@pytest.mark.parametrize("order", sorted(SUMS))
@pytest.mark.parametrize("M,rank,k", PRECOND_ALL)
def test_float64_preconditioner_stays_inside_the_cap(M, rank, k, order):
    total = SUMS[order]
    a = D.precond_inputs(M, rank, k)
    ref = D.precond_apply(a["u"], a["inv_eig"], a["prefactor"], a["r"])
    folded = D.worst_ratio(float64_precond(a, total, False), ref, D.cap_precond(a["u"], a["inv_eig"], a["prefactor"], a["r"]))
    three = D.worst_ratio(float64_precond(a, total, True), ref,
                          D.cap_precond_float64_three_products(a["u"], a["inv_eig"], a["prefactor"], a["r"]))
    assert folded <= 1.0 and three <= 1.0, (folded, three)


@pytest.mark.parametrize("order", sorted(SUMS))
@pytest.mark.parametrize("scale", D.MATVEC_SCALES)
@pytest.mark.parametrize("n,m", D.MATVEC_SHAPES)
def test_float64_scaled_matvec_stays_inside_the_cap(n, m, scale, order):
    a = D.matvec_inputs(n, m)
    c = a["c"].astype(np.float64)
    total = SUMS[order]
    inner = total((c * a["v"]).T) * (scale * scale)
    got = total((c.T * inner).T)
    assert D.worst_ratio(got, D.scaled_matvec(a["c"], a["v"], scale), D.cap_scaled_matvec(a["c"], a["v"], scale)) <= 1.0


def float64_softmax(pred, labels):
    rows = np.arange(pred.shape[0])
    with np.errstate(under="ignore"):
        e = np.power(D.SOFTMAX_BASE, pred - pred.max(axis=1, keepdims=True))
    prob = e / e.sum(axis=1, keepdims=True)
    loss = -np.log(np.maximum(prob[rows, labels], D.CLIP)).sum()
    prob[rows, labels] -= 1.0
    return prob, loss


def softmax_verdict(got, loss, ref, ref_loss):
    """(worst entry error / bar, loss error / bar, entries where the reference is exactly 0 or -1 and got is not)."""
    exact = (ref == 0) | (ref == -1)
    wrong = int((f64(got)[exact] != f64(ref)[exact]).sum())
    entries = D.worst_ratio(got, ref, D.cap_softmax_entries())
    with np.errstate(invalid="ignore"):
        dl = abs(LD(loss) - ref_loss)
    lossr = 0.0 if dl == 0 else (float(dl / D.cap_softmax_loss(ref_loss)) if np.isfinite(dl) and ref_loss != 0 else np.inf)
    return entries, lossr, wrong


@pytest.mark.parametrize("n,ncls", D.SOFTMAX_SHAPES)
def test_float64_softmax_stays_inside_the_bars_and_is_exact_where_the_reference_is(n, ncls):
    a = D.softmax_inputs(n, ncls)
    ref, ref_loss = D.softmax_residual(a["pred"], a["labels"])
    got, loss = float64_softmax(a["pred"].copy(), a["labels"])
    entries, lossr, wrong = softmax_verdict(got, loss, ref, ref_loss)
    assert entries <= 1.0 and lossr <= 1.0 and wrong == 0
    if ncls > 1:
        assert int(((ref == 0) | (ref == -1)).sum()) > 0             # the 800 rows underflow in the reference too
    if n == 1 and ncls > 1:
        assert loss == float(-np.log(LD(np.float64(D.CLIP)))) == float(ref_loss)      # a label on an underflowed class


# ---------------------------------------------------------------------------------------------------- planted mistakes
@pytest.mark.parametrize("M,k", STEP_SHAPES)
def test_every_applicable_step_mistake_leaves_a_cap_by_100x(M, k):
    a = steps_inputs(M, k)
    assert max(D.step_ratios(a, mistaken_steps(a, None)).values()) <= 1.0            # the harness itself: no mistake, inside
    hit = [m for m in D.STEP_MISTAKES if D.mistake_applies(m, M, k)]
    assert hit
    for mistake in hit:
        ratios = D.step_ratios(a, mistaken_steps(a, mistake))
        assert max(ratios.values()) >= 100.0, (mistake, ratios)
    own = "drop_tail" if k is None else "drop_tail_block"                            # the loop-bound mistake of this kind of step:
    if own not in hit:                                                               # "does not apply" means it changes nothing
        assert max(D.step_ratios(a, mistaken_steps(a, own)).values()) <= 1.0, own


@pytest.mark.parametrize("M,rank,k", PRECOND_ALL)
def test_the_preconditioner_without_its_minus_one_leaves_the_cap(M, rank, k):
    a = D.precond_inputs(M, rank, k)
    args = (a["u"], a["inv_eig"], a["prefactor"], a["r"])
    assert D.worst_ratio(f64(D.precond_apply(*args, mistake="no_minus_one")), D.precond_apply(*args), D.cap_precond(*args)) >= 100.0


@pytest.mark.parametrize("scale", [s for s in D.MATVEC_SCALES if s != 1.0])
@pytest.mark.parametrize("n,m", D.MATVEC_SHAPES)
def test_scale_for_scale_squared_leaves_the_cap(n, m, scale):
    a = D.matvec_inputs(n, m)
    args = (a["c"], a["v"], scale)
    assert D.worst_ratio(f64(D.scaled_matvec(*args, mistake="scale_once")), D.scaled_matvec(*args), D.cap_scaled_matvec(*args)) >= 100.0


@pytest.mark.parametrize("n,ncls", D.SOFTMAX_SHAPES)
def test_a_softmax_mistake_leaves_the_bars_at_every_shape(n, ncls):
    a = D.softmax_inputs(n, ncls)
    ref, ref_loss = D.softmax_residual(a["pred"], a["labels"])
    found = []
    for mistake in D.SOFTMAX_MISTAKES:
        got, loss = D.softmax_residual(a["pred"], a["labels"], mistake=mistake)
        entries, lossr, wrong = softmax_verdict(f64(got), float(loss), ref, ref_loss)
        if max(entries, lossr) >= 100.0:
            found.append(mistake)
    assert found, "no planted mistake shows at this shape"
    if n >= 9 and ncls >= 2:
        assert set(found) == set(D.SOFTMAX_MISTAKES), found                           # with every kind of row present: all of them


# ---------------------------------------------------------------------------------------------------- chained solve, stop machine
little_solve = D.little_solve


@pytest.mark.parametrize("M", sorted(set(D.STOP_M + [D.CHAIN_M])))
def test_a_step_mistake_inside_the_chained_solve_leaves_the_measured_cap(M):
    ref, plain = little_solve(M, D.CHAIN_ITERS, 0.0, LD), little_solve(M, D.CHAIN_ITERS, 0.0, np.float64)
    dev, cap = D.chain_cap(ref, plain)
    assert all(d < 1e-12 for d in dev.values()), dev
    assert all(e2 < e1 for e1, e2 in zip(ref["err"], ref["err"][1:]))                 # the errors fall: a tolerance fits between two
    for mistake in ("stale_w", "err_from_next", "beta_new_rz", "drop_tail"):
        bad = little_solve(M, D.CHAIN_ITERS, 0.0, LD, step_mistake=mistake)
        worst = max(abs(float((b - r) / r)) / cap[name] for name in D.CHAIN_SCALARS for b, r in zip(bad[name], ref[name]))
        assert worst >= 100.0, (mistake, worst)


def test_stop_machine_stops_after_iteration_one():
    M, maxit = 300, 5
    plain = little_solve(M, 3, 0.0, np.float64)
    tol = 0.5 * (plain["err"][0] + plain["err"][1])
    out = little_solve(M, 4, tol, np.float64, max_iterations=maxit)
    assert out["applied"] == [True, True, False, False]
    s = out["scal"]
    assert s[4] == 1.0 and s[5] == 2.0 and s[6] == -6.0 and s[7] == -7.0
    assert s[8] == plain["err"][0] and s[9] == plain["err"][1] and np.all(s[10:] == 0.0)
    assert s[1] == plain["alpha"][1] and s[3] == plain["beta"][1] and s[2] == plain["err"][1]
    two = little_solve(M, 2, 0.0, np.float64)
    assert np.array_equal(out["x"], two["x"]) and out["cur"] == two["cur"] == 0
    c = D.chain_inputs(M)
    assert np.array_equal(out["w"], c["diag"] * out["p"][out["cur"]])                # a stopped iteration leaves the caller's w
    late = little_solve(M, 4, tol, np.float64, max_iterations=maxit, mistake="stop_one_late")
    assert late["applied"] == [True, True, True, False] and not np.array_equal(late["x"], out["x"])
    for Mbig in D.STOP_M:                                                             # the planted mistake shows at the GPU test's shapes
        p3 = little_solve(Mbig, 3, 0.0, np.float64)
        t = 0.5 * (p3["err"][0] + p3["err"][1])
        assert little_solve(Mbig, 4, t, LD, max_iterations=maxit)["applied"] == [True, True, False, False]
        assert little_solve(Mbig, 4, t, LD, max_iterations=maxit, mistake="stop_one_late")["applied"] == [True, True, True, False]


def test_stop_machine_never_stops_within_max_iterations():
    out = little_solve(300, 5, 1e-300, np.float64)
    assert out["applied"] == [True] * 5
    s = out["scal"]
    assert s[4] == 0.0 and s[5] == 5.0 and list(s[8:13]) == out["err"] and len(s) == 13


def test_stop_tol_equal_to_an_error_does_not_stop():
    plain = little_solve(300, 4, 0.0, np.float64)
    out = little_solve(300, 5, float(plain["err"][1]), np.float64)                     # err_1 < tol is false: iteration 2 is applied
    assert out["applied"] == [True, True, True, False, False] and out["scal"][5] == 3.0
    above = little_solve(300, 5, float(np.nextafter(plain["err"][1], np.inf)), np.float64)
    assert above["applied"] == [True, True, False, False, False]
