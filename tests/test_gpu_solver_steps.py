"""The small kernels the solvers run between matvecs (csrc/cg_kernels.inc, hipZCacheMatvecScaled of zcache.inc) against the
longdouble reference of tests/dense_solver_steps.py, under its derived caps: inputs are built on the host by its seeded
builders and copied to the device, results are copied back and compared there.  tests/test_solver_steps_host.py shows, at
the same shapes, that plain float64 stays inside these caps and that every planted structural mistake leaves them.

Every case prints one line (shape, then the worst error / cap per output); with XGPR_SOLVER_STEPS_ERRORS=<file> in the
environment a run of this module also writes those lines to that file -- profiles/solver_steps_errors.txt is such a
run's record.  No number in it is an input to any test.
"""
import functools
import os

import numpy as np
import pytest
import torch

import dense_solver_steps as D
from test_solver_steps_host import softmax_verdict

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
LD = D.LD
LINES = []


@pytest.fixture(scope="module")
def ext():
    from xgpr_amd import xgpr_hip_rfgen_ext as e
    return e


@pytest.fixture(scope="module", autouse=True)
def errors_file():
    yield
    path = os.environ.get("XGPR_SOLVER_STEPS_ERRORS")
    if path:
        with open(path, "w") as f:
            f.write("# Per-case errors of tests/test_gpu_solver_steps.py on an MI355X (gfx950): HIP against the longdouble reference of\n"
                    "# tests/dense_solver_steps.py.  One line per case: the shape, then per output the worst |error| / cap (at most 1 passes);\n"
                    "# the chained runs give the measured deviation of plain float64 numpy from longdouble next to the GPU's.\n")
            f.write("".join(line + "\n" for line in LINES))


def note(line):
    LINES.append(line)
    print(line)


def fmt(ratios):
    return "  ".join(f"{name} {value:.1e}" for name, value in ratios.items())


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a, order="C"))                                    # a copy: the builders' arrays are shared and read-only
    return (t if dtype is None else t.to(dtype)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and bool((a.contiguous().view(torch.int64) == b.contiguous().view(torch.int64)).all())


@functools.lru_cache(maxsize=4)
def single_case(M):
    a = D.single_inputs(M)
    for v in a.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return a


# ---------------------------------------------------------------------------------------------------- one right-hand side
def run_single(ext, a, err_on_device, alias):
    """hipCGStep1 then hipCGStep2 -> the outputs as float64 numpy arrays (dense_solver_steps.step_ratios's ``got``), and the
    device tensors that must not have changed."""
    M = a["r"].shape[0]
    w, p, x, r = dev(a["w"]), dev(a["p"]), dev(a["x"]), dev(a["r"])
    z = r if alias else dev(a["z"])
    rn, pn = torch.full((M,), float("nan"), dtype=F64, device=DEV), torch.full((M,), float("nan"), dtype=F64, device=DEV)
    scal = torch.zeros(4, dtype=F64, device=DEV)
    err = torch.full((3,), -77.0, dtype=F64, device=DEV) if err_on_device else None
    ext.hipCGStep1(w, p, x, r, rn, z, scal, a["lam2"], a["init_norm"], err_out=None if err is None else err[1:2])
    got = {"w": host(w), "x": host(x), "r_next": host(rn)}
    got["z_next"] = got["r_next"] * a["dn"]
    ext.hipCGStep2(rn, dev(got["z_next"]), p, pn, scal)
    s = host(scal)
    got.update(rz=s[0], alpha=s[1], err=s[2], beta=s[3], p_next=host(pn))
    if err is not None:
        e = host(err)
        assert e[0] == -77.0 and e[2] == -77.0 and e[1] == s[2]                      # err_out: the same bits as scal[2], nothing beside it
    for name, t in (("p", p), ("r", r), ("z", z)):
        assert np.array_equal(host(t), a["r" if alias and name == "z" else name]), name       # the inputs are only read
    return got


@pytest.mark.parametrize("alias", [False, True], ids=["z-distinct", "z-is-r"])
@pytest.mark.parametrize("err_on_device", [True, False], ids=["err_out", "no-err_out"])
@pytest.mark.parametrize("M", D.SINGLE_M)
def test_single_steps_against_the_longdouble_reference(ext, M, err_on_device, alias):
    """Both sides of one batch of 8192 elements (registers / the loop that re-reads w, p and r), z and r as one tensor (no
    preconditioner: cg.py copies r into z) and as two, err_out given and not."""
    a = single_case(M)
    if alias:
        a = dict(a, z=a["r"])
    got = run_single(ext, a, err_on_device, alias)
    ratios = D.step_ratios(a, got)
    note(f"single   M={M:<6d} {'err_out' if err_on_device else 'no err_out':10s} {'z is r' if alias else 'z distinct':10s}  {fmt(ratios)}")
    assert max(ratios.values()) <= 1.0, ratios
    if M in D.SINGLE_TWICE:
        again = run_single(ext, a, err_on_device, alias)
        for name in got:
            assert np.array_equal(np.asarray(got[name]), np.asarray(again[name])), name          # deterministic


# ---------------------------------------------------------------------------------------------------- the little solve
class LittleSolve:
    """cg.py's loop around the two steps on the device: ping-pong r and p, z = r, the operator diag (torch.mul) + lam2."""

    def __init__(self, ext, M, scal0):
        c = D.chain_inputs(M)
        self.ext, self.M, self.init_norm = ext, M, c["init_norm"]
        self.d = dev(c["diag"])
        self.x, self.w = torch.zeros(M, dtype=F64, device=DEV), torch.full((M,), float("nan"), dtype=F64, device=DEV)
        self.r = [dev(c["r0"]), torch.full((M,), float("nan"), dtype=F64, device=DEV)]
        self.p = [dev(c["r0"]), torch.full((M,), float("nan"), dtype=F64, device=DEV)]
        self.scal = dev(scal0)
        self.err_out = torch.full((3,), -77.0, dtype=F64, device=DEV)
        self.cur = 0
        self.log = {name: [] for name in D.CHAIN_SCALARS}

    def iteration(self, stop_tol):
        """-> whether the device applied it (scal[5] moved, or, without stop_tol, always)."""
        cur, nxt = self.cur, 1 - self.cur
        before = float(self.scal[5]) if stop_tol > 0 else None
        torch.mul(self.d, self.p[cur], out=self.w)                                   # w arrives holding A p without lam2 p
        self.ext.hipCGStep1(self.w, self.p[cur], self.x, self.r[cur], self.r[nxt], self.r[cur], self.scal, D.CHAIN_LAM2, self.init_norm,
                            stop_tol=stop_tol, err_out=self.err_out[1:2])
        self.ext.hipCGStep2(self.r[nxt], self.r[nxt], self.p[cur], self.p[nxt], self.scal, stop_tol=stop_tol)
        s = host(self.scal)
        applied = True if stop_tol <= 0 else s[5] == before + 1
        if applied:
            for name, v in zip(D.CHAIN_SCALARS, (s[0], s[1], s[3], s[2])):
                self.log[name].append(v)
            self.cur = nxt
        return applied

    def vectors(self):
        return (self.x, self.r[0], self.r[1], self.p[0], self.p[1])


def test_six_chained_iterations_against_the_longdouble_recurrence(ext):
    """The only place where the kernels' outputs feed their own inputs and scal[0], written by step 1, is consumed by a later
    step 2.  The cap is measured on the CPU (dense_solver_steps.chain_cap)."""
    M, n = D.CHAIN_M, D.CHAIN_ITERS
    ref, plain = D.little_solve(M, n, 0.0, LD), D.little_solve(M, n, 0.0, np.float64)
    measured, cap = D.chain_cap(ref, plain)
    solve = LittleSolve(ext, M, np.zeros(4))
    for _ in range(n):
        assert solve.iteration(0.0)
    got = dict(solve.log, x=host(solve.x))
    gpu = D.chain_deviation(got, ref)
    note(f"chained  M={M} iterations={n}  " + "  ".join(f"{name} cpu {measured[name]:.3e} gpu {gpu[name]:.3e} cap {cap[name]:.3e}" for name in gpu))
    assert all(gpu[name] <= cap[name] for name in gpu), (gpu, cap)


@pytest.mark.parametrize("M", D.STOP_M)
def test_device_side_stop_beyond_one_batch_against_the_state_machine(ext, M):
    """stop_tol > 0 on the path that re-reads its operands: the applied iterations, the frozen vectors, the scal image, w left
    as the caller wrote it and err_out not written by a stopped step."""
    maxit, queued = 5, 4
    probe = LittleSolve(ext, M, np.zeros(4))
    for _ in range(3):
        probe.iteration(0.0)
    errs = probe.log["err"]
    assert errs[1] < errs[0]
    stop_tol = 0.5 * (errs[0] + errs[1])                                             # errs[1] < stop_tol < errs[0]

    ref = D.little_solve(M, queued, stop_tol, LD, max_iterations=maxit)
    measured, cap = D.chain_cap(D.little_solve(M, 2, 0.0, LD), D.little_solve(M, 2, 0.0, np.float64))
    solve = LittleSolve(ext, M, D.stop_scal_image(maxit, (-6.0, -7.0)))
    applied, frozen = [], None
    for i in range(queued):
        if frozen is None and i > 0 and not ref["applied"][i]:
            torch.cuda.synchronize()
            frozen = [t.detach().clone() for t in solve.vectors()]
            solve.err_out.fill_(-77.0)
        applied.append(bool(solve.iteration(stop_tol)))
        if frozen is not None:
            assert same_bits(solve.w, solve.d * solve.p[solve.cur])                  # w: what this test's own torch.mul wrote
            assert bool((solve.err_out == -77.0).all())                              # err_out: not written by a stopped step
    assert applied == ref["applied"] == [True, True, False, False]
    for t, before in zip(solve.vectors(), frozen):
        assert same_bits(t, before)
    assert solve.cur == ref["cur"]
    s, want = host(solve.scal), ref["scal"]
    assert s[4] == 1.0 and s[5] == 2.0 and s[6] == -6.0 and s[7] == -7.0 and np.all(s[10:] == 0.0)
    assert [float(v) for v in want[4:8]] == [1.0, 2.0, -6.0, -7.0] and np.all(want[10:] == 0)
    assert s[8] == errs[0] and s[9] == errs[1] and s[2] == s[9]                      # the plain run's bits
    image = {"rz": (0, "rz"), "alpha": (1, "alpha"), "err": (2, "err"), "beta": (3, "beta"), "err[0]": (8, "err"), "err[1]": (9, "err")}
    ratios = {name: abs(float((LD(s[i]) - want[i]) / want[i])) / cap[q] for name, (i, q) in image.items()}
    ratios["x"] = float(np.abs(host(solve.x).astype(LD) - ref["x"]).max() / np.abs(ref["x"]).max()) / cap["x"]
    note(f"stop     M={M:<6d} applied {''.join('TF'[not a] for a in applied)}  {fmt(ratios)}")
    assert max(ratios.values()) <= 1.0, ratios


# ---------------------------------------------------------------------------------------------------- blocks
def run_block(ext, a, err):
    M, k = a["r"].shape
    w, p, x, r, z = (dev(a[name]) for name in ("w", "p", "x", "r", "z"))
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=F64, device=DEV)
    rn, pn, rz, alpha, beta = nan(M, k), nan(M, k), nan(k), nan(k), nan(k)
    ws = torch.empty(ext.cg_block_workspace_bytes(M, k), dtype=torch.uint8, device=DEV)
    ext.hipCGStep1Block(w, p, x, r, rn, z, rz, alpha, err, dev(a["init_norm"]), a["lam2"], ws)
    got = {"w": host(w), "x": host(x), "r_next": host(rn), "rz": host(rz), "alpha": host(alpha)}
    got["z_next"] = got["r_next"] * a["dn"]
    ext.hipCGStep2Block(rn, dev(got["z_next"]), p, pn, rz, beta, ws)
    torch.cuda.synchronize()
    got.update(err=err.detach().cpu().numpy().copy(), beta=host(beta), p_next=host(pn))
    assert np.array_equal(got["rz"], host(rz))                                       # step 2 only reads rz
    return got


@pytest.mark.parametrize("M,k", D.BLOCK_SHAPES)
def test_block_steps_against_the_longdouble_reference(ext, M, k):
    """1 to 258 row blocks of 128 (every value of nblk % 4), k on both sides of 16 and at both ends; every column has its own
    scale, alpha and init_norm.  All eight outputs per column; err_out once on the device, once in pinned host memory."""
    a = D.block_inputs(M, k)
    got = run_block(ext, a, torch.full((k,), float("nan"), dtype=F64, device=DEV))
    ratios = D.step_ratios(a, got)                                                   # every cap is per column: the worst column counts
    note(f"block    M={M:<6d} k={k:<3d} {fmt(ratios)}")
    assert max(ratios.values()) <= 1.0, ratios
    pinned = torch.full((k + 2,), -77.0, dtype=F64).pin_memory()
    again = run_block(ext, a, pinned[1:k + 1])
    assert float(pinned[0]) == -77.0 and float(pinned[-1]) == -77.0                  # the sentinels survive
    for name in got:
        assert np.array_equal(got[name], again[name]), name                          # pinned err_out: the same bits as on the device


def test_block_steps_refuse_33_columns_and_leave_x(ext):
    M, k = 130, 33
    t = lambda seed: torch.randn(M, k, dtype=F64, generator=torch.Generator().manual_seed(seed)).to(DEV)
    w, p, x, r, rn, z = (t(i) for i in range(6))
    x0, w0 = x.clone(), w.clone()
    vec = [torch.ones(k, dtype=F64, device=DEV) for _ in range(4)]
    ws = torch.empty(ext.cg_block_workspace_bytes(M, 32) * 2, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="at most 32"):
        ext.hipCGStep1Block(w, p, x, r, rn, z, vec[0], vec[1], vec[2], vec[3], 0.01, ws)
    with pytest.raises(RuntimeError, match="at most 32"):
        ext.hipCGStep2Block(rn, z, p, x, vec[0], vec[1], ws)
    torch.cuda.synchronize()
    assert same_bits(x, x0) and same_bits(w, w0)


# ---------------------------------------------------------------------------------------------------- preconditioner
def precond_ratio(a, z):
    args = (a["u"], a["inv_eig"], a["prefactor"], a["r"])
    return D.worst_ratio(z, D.precond_apply(*args), D.cap_precond(*args))


@pytest.mark.parametrize("M,rank", D.PRECOND_SHAPES)
def test_precond_apply_against_the_three_product_reference(ext, M, rank):
    """M around the 512 workgroups of the first product (at 513 half of them have no rows and write zero partials), M < rank,
    odd and even ranks."""
    a = D.precond_inputs(M, rank)
    z = torch.full((M,), float("nan"), dtype=F64, device=DEV)
    ext.hipPrecondApply(dev(a["u"]), dev(a["inv_eig"]), a["prefactor"], dev(a["r"]), z)
    ratio = precond_ratio(a, host(z))
    note(f"precond  M={M:<6d} rank={rank:<4d} z {ratio:.1e}")
    assert ratio <= 1.0


def test_precond_apply_takes_u_at_any_8_byte_alignment(ext):
    """include/xgpr_hip.h promises nothing about u beyond its element type: a view 8 bytes into an allocation, at an even rank,
    takes the first product's one-column arm (the two-column arm's 16-byte loads are for 16-byte aligned u only) and gives
    the bits of the aligned copy -- the sums do not depend on the arm."""
    M, rank = D.PRECOND_UNALIGNED
    a = D.precond_inputs(M, rank)
    store = torch.zeros(M * rank + 3, dtype=F64, device=DEV)
    first = 1 if store.data_ptr() % 16 == 0 else 2                                   # the view starts 8 bytes past a 16-byte boundary
    view = store[first:first + M * rank].view(M, rank)
    view.copy_(dev(a["u"]))
    aligned = dev(a["u"])
    assert view.data_ptr() % 16 == 8 and aligned.data_ptr() % 16 == 0 and view.is_contiguous()
    inv_eig, r = dev(a["inv_eig"]), dev(a["r"])
    z1, z2 = torch.full((M,), float("nan"), dtype=F64, device=DEV), torch.full((M,), float("nan"), dtype=F64, device=DEV)
    ext.hipPrecondApply(aligned, inv_eig, a["prefactor"], r, z1)
    ext.hipPrecondApply(view, inv_eig, a["prefactor"], r, z2)
    ratio = precond_ratio(a, host(z1))
    note(f"precond  M={M:<6d} rank={rank:<4d} z {ratio:.1e}  (u 8 bytes off: {'same bits' if same_bits(z1, z2) else 'DIFFERENT'})")
    assert ratio <= 1.0 and same_bits(z1, z2)


@pytest.mark.parametrize("M,rank,k", D.PRECOND_BLOCK_SHAPES)
def test_precond_apply_block_below_one_tile(ext, M, rank, k):
    a = D.precond_inputs(M, rank, k)
    z = torch.full((M, k), float("nan"), dtype=F64, device=DEV)
    ext.hipPrecondApplyBlock(dev(a["u"]), dev(a["inv_eig"]), a["prefactor"], dev(a["r"]), z)
    zh = host(z)
    ratio = max(precond_ratio(dict(a, r=a["r"][:, j]), zh[:, j]) for j in range(k))  # per column, against the one-vector reference
    note(f"precondb M={M:<6d} rank={rank:<4d} k={k:<3d} z {ratio:.1e}")
    assert ratio <= 1.0


# ---------------------------------------------------------------------------------------------------- classifier cost
@pytest.mark.parametrize("n,ncls", D.SOFTMAX_SHAPES)
def test_softmax_residual_against_the_longdouble_reference(ext, n, ncls):
    """Independent of the device's math library: longdouble powers of the float64 number 2.71828.  One class; ties at the row
    maximum; spreads of 1e-3, 40 and 800 (exact underflow: residuals exactly 0 or -1, a label there adds exactly
    -log(1e-16)); n on both sides of one workgroup's 256 rows."""
    a = D.softmax_inputs(n, ncls)
    ref, ref_loss = D.softmax_residual(a["pred"], a["labels"])
    pred = dev(a["pred"])
    loss = ext.hipSoftmaxResidual(pred, dev(a["labels"]))
    entries, lossr, wrong = softmax_verdict(host(pred), float(loss), ref, ref_loss)
    note(f"softmax  n={n:<5d} classes={ncls:<4d} entries {entries:.1e}  loss {lossr:.1e}  exact entries wrong {wrong}")
    assert entries <= 1.0 and lossr <= 1.0 and wrong == 0
    if n == 1 and ncls > 1:
        assert float(loss) == float(ref_loss) == float(-np.log(LD(np.float64(D.CLIP))))          # the label's class underflowed
    if ncls == 1:
        assert float(loss) == 0.0


# ---------------------------------------------------------------------------------------------------- cached matvec
@pytest.mark.parametrize("scale", D.MATVEC_SCALES)
@pytest.mark.parametrize("n,m", D.MATVEC_SHAPES)
def test_scaled_cache_matvec_applies_the_square_of_scale(ext, n, m, scale):
    a = D.matvec_inputs(n, m)
    out = torch.full((m,), float("nan"), dtype=F64, device=DEV)
    freqs = m // 2
    ws = torch.empty(ext.ztz_workspace_bytes(m, max(2, freqs + (freqs & 1))), dtype=torch.uint8, device=DEV)
    ext.hipZCacheMatvecScaled(dev(a["c"]), dev(a["v"]), out, scale, ws)
    ratio = D.worst_ratio(host(out), D.scaled_matvec(a["c"], a["v"], scale), D.cap_scaled_matvec(a["c"], a["v"], scale))
    note(f"matvec   n={n:<5d} m={m:<5d} scale={scale:<5} w {ratio:.1e}")
    assert ratio <= 1.0
