"""Extended-precision reference of the small kernels the solvers run between matvecs -- TEST HELPER, numpy only.

Independent of ``xgpr_amd``, ``oracle`` and torch: everything is evaluated in ``np.longdouble`` from the formulas of
include/xgpr_hip.h (the reference's line numbers as quoted there).

    step 1 (cg_tools.py:256-265)     w' = w + lam2 p;  rz = r.z;  alpha = rz / (p.w');  x' = x + alpha p;
                                     r_next = r - alpha w';  err = |r| / init_norm     (the lagging error: the CURRENT r)
    step 2 (cg_tools.py:271-274)     beta = (r_next.z_next) / rz;  p_next = z_next + beta p
    blocks (cg_tools.py:121-141)     the same per column of [M, k] arrays, init_norm [k]
    device-side stop                 step 1 of an iteration first looks at the error the PREVIOUS applied iteration left in
                                     scal[2]: below stop_tol (strictly) -> scal[4] = 1 and this and every later step touch
                                     nothing else; an applied step 1 writes scal[0..2], scal[8 + scal[5]] = err, scal[5] += 1;
                                     step 2 writes scal[3]; scal[6..7] belong to nobody
    preconditioner                   z = U ((inv_eig prefactor) .* (U^T r)) + (r - U (U^T r))          (three products, as
    (rand_nys_preconditioners.py:66-72)                                  the reference writes it; the kernels fold them)
    classifier cost                  per row: e_c = B^(pred_c - max_c pred_c) with B the float64 number 2.71828 (not e);
    (nonlinear_cg_toolkit.py:243-262)  p = e / sum e;  loss = -sum_rows log(max(p[label], 1e-16));  pred <- p - onehot(label).
                                     The operation is defined on float64, so a power below half the smallest float64
                                     subnormal IS zero (and one above the largest float64 is infinite): the reference
                                     flushes exactly there, nowhere else, and its zeros, minus ones and -log(1e-16) are exact
    cached matvec                    w = scale^2 C^T (C v),  C float32 rows

Error caps (``cap_*``): the standard model, fl(a op b) = (a op b)(1 + d), |d| <= u, u = 2^-53, and gamma_n = n u / (1 - n u):
a float64 dot product of n terms, in ANY order, with or without fused multiply-adds, is within gamma_n sum |a_i b_i| of the
exact one; quotients, square roots (one ulp = 2 u granted) and the elementwise updates add their own roundings, and errors
of earlier results are propagated through every later one.  Each cap is a function of the unit roundoff and is evaluated
twice -- at 2^-53 for the code under test, at the longdouble roundoff for this file's own evaluation -- and the two are
added.  No cap is fitted to anything a kernel returned.  The softmax entries alone keep the bars the project already uses
(1e-14 absolute per entry, 1e-12 relative on the loss): their error is the device pow's, not an operation count.

``mistake=`` arguments exist for the sensitivity test only (tests/test_solver_steps_host.py): each plants ONE structural
error, so that the test can show the shapes and inputs below would expose it.
"""
import numpy as np

LD = np.longdouble
U64 = 2.0 ** -53
ULD = float(np.finfo(LD).eps) / 2
BATCH = 8192                     # elements the single-vector steps hold in registers: 1024 threads x 8
ROWS = 128                       # rows per workgroup of the block steps; their partial sums are added four blocks at a time
SOFTMAX_BASE = 2.71828           # the reference's constant
CLIP = 1e-16
SOFTMAX_ENTRY_BAR = 1e-14        # tests/test_gpu_classifier.py
SOFTMAX_LOSS_BAR = 1e-12

# ---------------------------------------------------------------------------------------------------- shapes (one place)
SINGLE_M = [1, 63, 65, 1023, 1025, 8191, 8192, 8193, 9217, 16384, 16385, 24577, 32768, 40000]
SINGLE_TWICE = [8193, 40000]                     # a second call from the same inputs must give the same bits
STOP_M = [8193, 20000]
CHAIN_M, CHAIN_ITERS, CHAIN_LAM2 = 20000, 6, 0.01
BLOCK_SHAPES = [(127, 1), (128, 2), (129, 17), (512, 16), (513, 31), (901, 26), (1025, 32), (12288, 26), (33000, 9)]
PRECOND_SHAPES = [(1, 1), (5, 7), (511, 2), (512, 64), (513, 65), (1023, 37), (1025, 130), (2049, 3), (33000, 4)]
PRECOND_UNALIGNED = (1000, 514)
PRECOND_BLOCK_SHAPES = [(3, 2, 1), (15, 1, 5), (17, 3, 17), (130, 66, 32)]
PRECOND_PREFACTOR = 0.37
SOFTMAX_SHAPES = [(1, 1), (1, 2), (1, 257), (255, 1), (255, 3), (256, 2), (256, 31), (257, 33), (257, 257), (1000, 2), (1000, 31)]
MATVEC_SHAPES = [(1, 2), (40, 12), (5, 6146), (777, 3000)]
MATVEC_SCALES = [0.37, 1.0, 3.0]
LAM2 = 0.01

STEP_MISTAKES = ("drop_tail", "drop_tail_block", "stale_w", "err_from_next", "beta_new_rz", "col_shift", "norm_col0")
SOFTMAX_MISTAKES = ("base_e", "clip_after_log", "max_of_first", "label_keeps_one")


def gamma(n, u=U64):
    n = float(n)
    return n * u / (1.0 - n * u) if n * u < 1.0 else np.inf


def _ld(a):
    return np.asarray(a, dtype=LD)


def _both(fn):
    """A cap: the bound for float64 arithmetic plus the bound for this file's own longdouble evaluation."""
    return fn(U64) + fn(ULD)


# ---------------------------------------------------------------------------------------------------- the two steps
def _kept(M, mistake):
    """Rows the dot products see (a boolean mask), under the two loop-bound mistakes."""
    keep = np.ones(M, dtype=bool)
    if mistake == "drop_tail":
        keep[(M // BATCH) * BATCH if M > BATCH else M:] = False
    elif mistake == "drop_tail_block":
        nblk = -(-M // ROWS)
        keep[(nblk - nblk % 4) * ROWS:] = False
    return keep


def mistake_applies(mistake, M, k=None):
    """Whether a planted mistake changes anything at this shape (k None: one right-hand side)."""
    if mistake == "drop_tail":
        return k is None and M > BATCH and M % BATCH != 0
    if mistake == "drop_tail_block":
        return k is not None and (-(-M // ROWS)) % 4 != 0
    if mistake in ("col_shift", "norm_col0"):
        return k is not None and k >= 2
    return mistake in STEP_MISTAKES


def _dot(a, b, keep):
    return (a[keep] * b[keep]).sum(axis=0)


def cg_step1(w, p, x, r, z, lam2, init_norm, mistake=None):
    """-> w', x', r_next, rz, alpha, err.  Vectors [M] or [M, k]; for a block rz, alpha, err and init_norm are [k]."""
    w, p, x, r, z, lam2, init_norm = (_ld(a) for a in (w, p, x, r, z, lam2, init_norm))
    keep = _kept(w.shape[0], mistake)
    w2 = w + lam2 * p
    rz = _dot(r, z, keep)
    with np.errstate(invalid="ignore", divide="ignore"):     # a planted mistake may leave nothing to sum
        alpha = rz / _dot(p, w2, keep)
    used = np.roll(alpha, 1) if mistake == "col_shift" else alpha
    x2 = x + used * p
    r_next = r - used * (w if mistake == "stale_w" else w2)
    norm = init_norm[0] if mistake == "norm_col0" else init_norm
    src = r_next if mistake == "err_from_next" else r
    err = np.sqrt(_dot(src, src, keep)) / norm
    return w2, x2, r_next, rz, used, err


def cg_step2(r_next, z_next, p, rz, mistake=None):
    """-> p_next, beta."""
    r_next, z_next, p, rz = (_ld(a) for a in (r_next, z_next, p, rz))
    new = _dot(r_next, z_next, _kept(r_next.shape[0], mistake))
    if mistake == "beta_new_rz":
        rz = new
    elif mistake == "col_shift":
        rz = np.roll(rz, 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        beta = new / rz
    return z_next + beta * p, beta


def _rel_quotient(num_cap, num, den_cap, den, u):
    """Relative error bound of fl(num / den) when num and den carry the absolute errors num_cap and den_cap."""
    a = num_cap / np.abs(num)
    b = den_cap / np.abs(den)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(b < 1.0, (1.0 + a) * (1.0 + u) / (1.0 - b) - 1.0, np.inf)


def _caps_step1(w, p, x, r, z, lam2, init_norm, u):
    w, p, x, r, z, lam2, init_norm = (_ld(a) for a in (w, p, x, r, z, lam2, init_norm))
    n = w.shape[0]
    g = gamma(n, u)
    mag_w = np.abs(w) + np.abs(lam2 * p)                    # |w'| <= mag_w
    ew = 2.0 * u * (1.0 + u) * mag_w                        # fl(w + fl(lam2 p)), fused or not
    s_rz = np.abs(r * z).sum(axis=0)
    s_pw = (np.abs(p) * mag_w).sum(axis=0)
    rz, pw = (r * z).sum(axis=0), (p * (w + lam2 * p)).sum(axis=0)
    cap_rz = g * s_rz
    cap_pw = gamma(n + 2, u) * s_pw                         # the two roundings of every w' folded into the product's
    alpha = rz / pw
    cap_alpha = np.abs(alpha) * _rel_quotient(cap_rz, rz, cap_pw, pw, u)
    amax = np.abs(alpha) + cap_alpha
    cap_x = cap_alpha * np.abs(p) + 2.0 * u * (1.0 + u) * (np.abs(x) + amax * np.abs(p))
    wmax = mag_w + ew
    cap_rn = cap_alpha * wmax + np.abs(alpha) * ew + 2.0 * u * (1.0 + u) * (np.abs(r) + amax * wmax)
    err = np.sqrt((r * r).sum(axis=0)) / init_norm
    cap_err = gamma(n + 3, u) * err                         # rr within gamma_n of itself (all terms positive); sqrt, quotient
    return {"w": ew, "x": cap_x, "r_next": cap_rn, "rz": cap_rz, "alpha": cap_alpha, "err": cap_err}


def cap_step1(w, p, x, r, z, lam2, init_norm):
    """Caps of step 1's six outputs (a dict by output name), from its INPUTS as the kernel receives them."""
    a = _caps_step1(w, p, x, r, z, lam2, init_norm, U64)
    b = _caps_step1(w, p, x, r, z, lam2, init_norm, ULD)
    return {k: a[k] + b[k] for k in a}


def _caps_step2(r_next, z_next, p, rz, u):
    r_next, z_next, p, rz = (_ld(a) for a in (r_next, z_next, p, rz))
    n = r_next.shape[0]
    new = (r_next * z_next).sum(axis=0)
    cap_new = gamma(n, u) * np.abs(r_next * z_next).sum(axis=0)
    beta = new / rz
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.where(new != 0, cap_new / np.abs(new), 0.0)
    cap_beta = np.abs(beta) * ((1.0 + a) * (1.0 + u) - 1.0)
    cap_pn = cap_beta * np.abs(p) + 2.0 * u * (1.0 + u) * (np.abs(z_next) + (np.abs(beta) + cap_beta) * np.abs(p))
    return {"beta": cap_beta, "p_next": cap_pn}


def cap_step2(r_next, z_next, p, rz):
    """Caps of step 2's two outputs, from its inputs as the kernel receives them (rz: what step 1 left for it)."""
    a, b = _caps_step2(r_next, z_next, p, rz, U64), _caps_step2(r_next, z_next, p, rz, ULD)
    return {k: a[k] + b[k] for k in a}


STEP_OUTPUTS = ("w", "x", "r_next", "rz", "alpha", "err", "p_next", "beta")


def step_ratios(a, got):
    """Error / cap, worst entry per output, of one step 1 + step 2 on the inputs ``a`` (single_inputs / block_inputs).
    ``got`` holds float64 arrays: step 1's six outputs, then z_next -- the caller's r_next * a["dn"], rounded -- and step
    2's p_next and beta.  Step 1 is judged from a; step 2 from what it was actually given: got's r_next, z_next and rz."""
    ref = dict(zip(("w", "x", "r_next", "rz", "alpha", "err"), cg_step1(a["w"], a["p"], a["x"], a["r"], a["z"], a["lam2"], a["init_norm"])))
    cap = cap_step1(a["w"], a["p"], a["x"], a["r"], a["z"], a["lam2"], a["init_norm"])
    ref["p_next"], ref["beta"] = cg_step2(got["r_next"], got["z_next"], a["p"], got["rz"])
    cap.update(cap_step2(got["r_next"], got["z_next"], a["p"], got["rz"]))
    return {name: worst_ratio(got[name], ref[name], cap[name]) for name in STEP_OUTPUTS}


# ---------------------------------------------------------------------------------------------------- the device-side stop
def stop_machine(x, r0, p0, matvec, lam2, init_norm, stop_tol, iterations, scal, precond=None, dtype=LD, mistake=None,
                 step_mistake=None):
    """The solver loop of cg.py around the two steps, ``iterations`` queued iterations with ping-pong buffers, with the
    stop_tol contract as a state machine.  ``matvec(p)`` returns A p WITHOUT the ridge term; ``precond(r)`` returns z
    (None: z = r); ``scal`` is the initial image ([8 + max_iterations], scal[2] = inf for stop_tol > 0; [4] otherwise).
    Runs in ``dtype`` (longdouble: the reference; float64: plain numpy, for the chained test's measured deviation and
    for exact comparisons against stop_tol).  Returns a dict: applied (one bool per iteration), x, r and p (both
    buffers each; a buffer never written is None), cur, w (what the last iteration left in w), scal, and per applied
    iteration rz, alpha, beta, err.  ``mistake="stop_one_late"`` is the machine's own; ``step_mistake`` goes to the steps."""
    cast = (lambda a: np.asarray(a, dtype=dtype))
    x, lam2, init_norm = cast(x).copy(), cast(lam2), cast(init_norm)
    r, p = [cast(r0).copy(), None], [cast(p0).copy(), None]
    zbuf = [precond(r[0]) if precond else r[0], None]
    scal = np.array(scal, dtype=dtype)
    out = {"applied": [], "rz": [], "alpha": [], "beta": [], "err": []}
    cur, w, prev_errs = 0, None, [np.inf, np.inf]
    for _ in range(iterations):
        w = cast(matvec(p[cur]))
        if stop_tol > 0.0:
            seen = prev_errs[-2] if mistake == "stop_one_late" else scal[2]
            if scal[4] != 0.0 or seen < stop_tol:
                scal[4] = 1.0
                out["applied"].append(False)
                continue
        nxt = 1 - cur
        if dtype is LD:
            w, x, r[nxt], rz, alpha, err = cg_step1(w, p[cur], x, r[cur], zbuf[cur], lam2, init_norm, step_mistake)
        else:
            w = w + lam2 * p[cur]
            rz = (r[cur] * zbuf[cur]).sum()
            alpha = rz / (p[cur] * w).sum()
            x = x + alpha * p[cur]
            r[nxt] = r[cur] - alpha * w
            err = np.sqrt((r[cur] * r[cur]).sum()) / init_norm
        scal[0], scal[1], scal[2] = rz, alpha, err
        prev_errs.append(err)
        if stop_tol > 0.0:
            it = int(scal[5])
            scal[8 + it] = err
            scal[5] = it + 1
        zbuf[nxt] = precond(r[nxt]) if precond else r[nxt]
        if dtype is LD:
            p[nxt], beta = cg_step2(r[nxt], zbuf[nxt], p[cur], rz, step_mistake)
        else:
            beta = (r[nxt] * zbuf[nxt]).sum() / rz
            p[nxt] = zbuf[nxt] + beta * p[cur]
        scal[3] = beta
        out["applied"].append(True)
        for name, v in (("rz", rz), ("alpha", alpha), ("beta", beta), ("err", err)):
            out[name].append(v)
        cur = nxt
    out.update(x=x, r=r, p=p, cur=cur, w=w, scal=scal)
    return out


def stop_scal_image(max_iterations, fill67=(0.0, 0.0)):
    """The image the caller prepares for stop_tol > 0: zeros, scal[2] = +inf; [6..7] are nobody's (a test plants values)."""
    s = np.zeros(8 + max_iterations)
    s[2] = np.inf
    s[6], s[7] = fill67
    return s


def little_solve(M, iterations, stop_tol, dtype, max_iterations=None, **kw):
    """stop_machine on chain_inputs(M): x_0 = 0, p_0 = r_0, no preconditioner; scal[6..7] planted with -6, -7."""
    c = chain_inputs(M)
    scal = stop_scal_image(max_iterations or iterations, (-6.0, -7.0)) if stop_tol > 0 else np.zeros(4)
    return stop_machine(np.zeros(M), c["r0"], c["r0"], lambda p: c["diag"].astype(dtype) * p, CHAIN_LAM2, c["init_norm"],
                        stop_tol, iterations, scal, dtype=dtype, **kw)


CHAIN_SCALARS = ("rz", "alpha", "beta", "err")


def chain_deviation(got, ref):
    """Worst relative deviation per quantity of a chained run from the longdouble one: rz, alpha, beta, err over the
    iterations both applied, x relative to its largest entry."""
    dev = {name: max([abs(float((LD(g) - r) / r)) for g, r in zip(got[name], ref[name])], default=0.0) for name in CHAIN_SCALARS}
    dev["x"] = float(np.abs(_ld(got["x"]) - ref["x"]).max() / np.abs(ref["x"]).max())
    return dev


def chain_cap(ref, plain):
    """The cap of a chained run cannot be derived per operation (every iteration's rounding passes through the operator
    again); it is measured on the CPU: the deviation of the plain float64 numpy recurrence from the longdouble one at the
    same inputs, times 8 for the kernels' different summation orders, at least 64 u.  -> (deviation, cap), by quantity."""
    dev = chain_deviation(plain, ref)
    return dev, {name: max(8.0 * d, 64.0 * U64) for name, d in dev.items()}


# ---------------------------------------------------------------------------------------------------- preconditioner
def precond_apply(u, inv_eig, prefactor, r, mistake=None):
    """z = U (inv_eig prefactor .* U^T r) + (r - U U^T r), r [M] or [M, k]."""
    u, inv_eig, prefactor, r = (_ld(a) for a in (u, inv_eig, prefactor, r))
    t = u.T @ r
    coef = inv_eig * prefactor
    scaled = (coef * t.T).T
    if mistake == "no_minus_one":
        return u @ scaled + r
    return u @ scaled + (r - u @ t)


def _cap_precond(u, inv_eig, prefactor, r, ur):
    u, inv_eig, prefactor, r = (_ld(a) for a in (u, inv_eig, prefactor, r))
    M, rank = u.shape
    au = np.abs(u)
    a_t = au.T @ np.abs(r)                                  # sum_i |U_ij r_i|
    t = u.T @ r
    et = gamma(M, ur) * a_t                                 # U^T r: M terms, any order
    cp = np.abs(inv_eig * prefactor)
    cf = np.abs(inv_eig * prefactor - 1.0)
    ecf = ur * (1.0 + ur) * (cp + cf)                       # fl(fl(inv_eig prefactor) - 1)
    col = (lambda v, m: (v * m.T).T)                        # per-j factor times [rank] or [rank, k]
    moved = col(cf, et) + col(ecf, np.abs(t) + et)          # what the errors of t and of the coefficient move a term by
    big = col(cf + ecf, np.abs(t) + et)                     # |term_j| at most
    folded = au @ moved + gamma(rank + 3, ur) * (np.abs(r) + au @ big)      # the product, rank terms + the add of r_i
    three = gamma(M + rank + 4, ur) * (np.abs(r) + au @ col(cp + 1.0, a_t))  # the three-product form (this file's)
    return folded, three


def cap_precond(u, inv_eig, prefactor, r):
    """Cap of z: gamma_M on U^T r, gamma_rank on the row product (the kernels' folded form, its coefficient's two
    roundings propagated) at 2^-53, plus the three-product form's own bound at the longdouble roundoff."""
    return _cap_precond(u, inv_eig, prefactor, r, U64)[0] + _cap_precond(u, inv_eig, prefactor, r, ULD)[1]


def cap_precond_float64_three_products(u, inv_eig, prefactor, r):
    """The bound for a float64 evaluation in the reference's own three-product form (the host test's second leg)."""
    return _cap_precond(u, inv_eig, prefactor, r, U64)[1] + _cap_precond(u, inv_eig, prefactor, r, ULD)[1]


# ---------------------------------------------------------------------------------------------------- classifier cost
def softmax_residual(pred, labels, mistake=None):
    """-> residual [n, ncls] and loss (longdouble)."""
    pred, labels = _ld(pred), np.asarray(labels, dtype=np.int64)
    n, ncls = pred.shape
    rows = np.arange(n)
    mx = pred[:, 0] if mistake == "max_of_first" else pred.max(axis=1)
    base = np.exp(LD(1)) if mistake == "base_e" else LD(np.float64(SOFTMAX_BASE))
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        e = np.power(base, pred - mx[:, None])
        e = np.where(e < LD(2.0) ** -1075, LD(0), e)        # float64's pow returns zero there ...
        e = np.where(e > LD(np.finfo(np.float64).max), LD(np.inf), e)         # ... and infinity here
        prob = e / e.sum(axis=1, keepdims=True)
        pl = prob[rows, labels]
        if mistake == "clip_after_log":
            loss = np.maximum(-np.log(pl), LD(CLIP)).sum()
        else:
            loss = -np.log(np.maximum(pl, LD(np.float64(CLIP)))).sum()
    res = prob.copy()
    if mistake != "label_keeps_one":
        res[rows, labels] -= 1
    return res, loss


def cap_softmax_entries():
    return SOFTMAX_ENTRY_BAR


def cap_softmax_loss(loss):
    return SOFTMAX_LOSS_BAR * abs(float(loss))


# ---------------------------------------------------------------------------------------------------- cached matvec
def scaled_matvec(c, v, scale, mistake=None):
    c, v, scale = _ld(c), _ld(v), LD(np.float64(scale))
    return (scale if mistake == "scale_once" else scale * scale) * (c.T @ (c @ v))


def cap_scaled_matvec(c, v, scale):
    """gamma_m on the inner product, gamma_n on the outer sum, three roundings for scale^2 and its two uses."""
    c, v, scale = _ld(c), _ld(v), LD(np.float64(scale))
    n, m = c.shape
    mag = scale * scale * (np.abs(c).T @ (np.abs(c) @ np.abs(v)))
    return _both(lambda u: gamma(m + n + 3, u) * mag)


# ---------------------------------------------------------------------------------------------------- input builders
def sentinel_rows(M):
    return [i for i in (0, 1023, 1024, 8191, 8192, 16383, 16384, M - 1) if 0 <= i < M]


def block_sentinel_rows(M):
    return sorted({M - 1, (-(-M // ROWS) - 1) * ROWS})


def _plant(rng, arrs, rows, M):
    """Sentinel weight: r and p at these rows are +-sqrt(M / 10) (at least 1), of opposite signs so that r_next = r -
    alpha w' adds up instead of cancelling, and the positive factors d, d', d_next are 1 there."""
    amp = max(1.0, np.sqrt(M / 10.0))
    sign = rng.choice([-1.0, 1.0], size=(len(rows),) + arrs["r"].shape[1:])
    arrs["r"][rows] = amp * sign
    arrs["p"][rows] = -amp * sign
    for name in ("d", "dp", "dn"):
        arrs[name][rows] = 1.0


def single_inputs(M, seed=0):
    """One right-hand side: z = r d and w = p d' with d, d' in [0.5, 1.5] (sum |a b| = |sum a b| for r.z, p.w and, with
    z_next = r_next d_next, for step 2's product), sentinel rows as above.  -> dict of float64 arrays + lam2, init_norm."""
    rng = np.random.default_rng(1000 + 7 * M + seed)
    a = {"r": rng.standard_normal(M), "p": rng.standard_normal(M), "x": rng.standard_normal(M),
         "d": rng.uniform(0.5, 1.5, M), "dp": rng.uniform(0.5, 1.5, M), "dn": rng.uniform(0.5, 1.5, M)}
    _plant(rng, a, sentinel_rows(M), M)
    a["z"], a["w"] = a["r"] * a["d"], a["p"] * a["dp"]
    a["lam2"], a["init_norm"] = LAM2, float(np.linalg.norm(a["r"]) * 1.7)
    return a


def block_inputs(M, k, seed=0):
    """A block: column j of every vector is scaled by 10^((j mod 7) - 3), w by 1 + j / 4 more (so alpha differs from
    column to column) and has its own init_norm; rows M - 1 and the first of the last 128-row block are sentinels."""
    rng = np.random.default_rng(2000 + 7 * M + 131 * k + seed)
    a = {"r": rng.standard_normal((M, k)), "p": rng.standard_normal((M, k)), "x": rng.standard_normal((M, k)),
         "d": rng.uniform(0.5, 1.5, (M, k)), "dp": rng.uniform(0.5, 1.5, (M, k)), "dn": rng.uniform(0.5, 1.5, (M, k))}
    _plant(rng, a, block_sentinel_rows(M), M)
    j = np.arange(k)
    s = 10.0 ** ((j % 7) - 3)
    for name in ("r", "p", "x"):
        a[name] = a[name] * s
    a["z"], a["w"] = a["r"] * a["d"], a["p"] * a["dp"] * (1.0 + j / 4.0)
    a["lam2"], a["init_norm"] = LAM2, np.linalg.norm(a["r"], axis=0) * (1.3 + 0.1 * j)
    return a


def chain_inputs(M, seed=0):
    """The little solve of the stop and chained tests: operator diag + lam2 with diag in [0.5, 1.5], r_0 = p_0 random."""
    rng = np.random.default_rng(3000 + M + seed)
    diag, r0 = rng.uniform(0.5, 1.5, M), rng.standard_normal(M)
    return {"diag": diag, "r0": r0, "init_norm": float(np.linalg.norm(r0))}


def precond_inputs(M, rank, k=None, seed=0):
    """U with orthonormal columns where M >= rank (QR of a Gaussian matrix), a Gaussian matrix otherwise; inv_eig in
    [0.02, 10]; r Gaussian with the last row ten times larger."""
    rng = np.random.default_rng(4000 + 13 * M + rank + (k or 0) + seed)
    g = rng.standard_normal((M, rank))
    u = np.ascontiguousarray(np.linalg.qr(g)[0]) if M >= rank else g
    r = rng.standard_normal((M,) if k is None else (M, k))
    r[M - 1] *= 10.0
    return {"u": u, "inv_eig": rng.uniform(0.02, 10.0, rank), "prefactor": PRECOND_PREFACTOR, "r": r}


SOFTMAX_KINDS = ("800 label min", "all equal", "two-way tie", "1e-3 label max", "40 label min", "40 label max", "800 label max",
                 "1e-3 label min", "gaussian")


def softmax_inputs(n, ncls, seed=0):
    """Row i is of kind i mod 9 (SOFTMAX_KINDS): a spread s row has its minimum in column 0 and its maximum, exactly s above,
    in the last column (so the maximum is never column 0 where ncls >= 2); ties sit in the last two columns."""
    rng = np.random.default_rng(5000 + 11 * n + ncls + seed)
    pred = np.zeros((n, ncls))
    labels = np.zeros(n, dtype=np.int64)
    last = ncls - 1
    for i in range(n):
        kind = SOFTMAX_KINDS[i % len(SOFTMAX_KINDS)]
        off = float(rng.integers(-3, 4))
        if kind == "all equal":
            pred[i], labels[i] = off + 0.625, rng.integers(0, ncls)
        elif kind == "two-way tie":
            pred[i] = off - rng.uniform(0.0, 40.0, ncls)
            pred[i, max(last - 1, 0):] = off + 1.5
            labels[i] = last
        elif kind == "gaussian":
            pred[i], labels[i] = rng.standard_normal(ncls) * 8.0, rng.integers(0, ncls)
        else:
            spread = float(kind.split()[0])
            pred[i] = off + spread * rng.uniform(0.0, 1.0, ncls)
            pred[i, last] = off + spread
            pred[i, 0] = off if ncls > 1 else off + spread
            labels[i] = 0 if kind.endswith("min") else last
    return {"pred": pred, "labels": labels}


def matvec_inputs(n, m, seed=0):
    rng = np.random.default_rng(6000 + 17 * n + m + seed)
    return {"c": rng.uniform(-1.0, 1.0, (n, m)).astype(np.float32), "v": rng.standard_normal(m)}


# ---------------------------------------------------------------------------------------------------- comparison
def worst_ratio(got, ref, cap):
    """max over entries of |got - ref| / cap (0 / 0 counts as 0; anything not finite as infinite)."""
    got, ref, cap = _ld(got), _ld(ref), np.broadcast_to(_ld(cap), np.shape(ref))
    with np.errstate(divide="ignore", invalid="ignore"):
        dev = np.abs(got - ref)
        ratio = np.where(dev == 0, LD(0), dev / cap)
    ratio = np.where(np.isfinite(ratio), ratio, LD(np.inf))
    return float(ratio.max()) if ratio.size else 0.0
