"""The memory contract of every C-ABI operator that writes device memory (include/xgpr_hip.h): no write outside an output, no use
of workspace beyond the bytes the matching *_workspace_bytes function advertises, no dependence on what the workspace held, inputs
unmodified.

One table row per entry point and shape.  A row runs its operator twice in one process over one set of operands: once the plain
way -- separately allocated tensors, as the value tests do -- and once with every input, output and workspace inside the guarded
arena of tests/guarded.py (exact sizes, 0xFF poison, guard bands, internal workspaces through the patched seam).  Then
``arena.verify()``, and the guarded outputs must equal the plain ones bit for bit: every operator here is documented deterministic.
The shapes are taken from the value tests' parameter lists, so the plain numbers are held to the reference there and this file needs
no tolerance of its own -- except for the block CG steps, which have no list to borrow from and are compared with the float64 numpy
formulas at the 1e-12 bar of tests/test_gpu_cg.py::test_precond_apply_and_fused_cg_steps.

Every deliberately out-of-contract write of the negative controls lands inside the arena's own allocation (tests/guarded.py: the rear
guard is at least 1 MiB and at least the payload)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from guarded import Arena, Plain, patched_workspaces, same_bits
from test_dense_reference_cpu import ARD, GRAD_SCALE, ard_case, fixed_case, seq_case
from test_gpu_dispatch_arms import run_fixed, run_seq
from test_gpu_token_rows import GRAD_GRID, GRID
from test_gpu_token_rows import L as TOKEN_L
from test_gpu_token_rows import N as TOKEN_N

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64, F16, I8, I64 = torch.float32, torch.float64, torch.float16, torch.int8, torch.int64

ROWS = []          # (id, function, shape)
COVERED = set()    # entry points of include/xgpr_hip.h with at least one row (or a test of their own below)


def row(symbols, shapes):
    """Registers ``fn(ext, A, *shape) -> {name: output}`` once per shape; A is the plain allocator or the arena."""
    def wrap(fn):
        COVERED.update(symbols)
        for shape in shapes:
            ROWS.append(pytest.param(fn, shape, id=fn.__name__ + "-" + "-".join(str(int(s) if isinstance(s, bool) else s) for s in shape)))
        return fn
    return wrap


def covered_entry_points():
    return set(COVERED)


@pytest.fixture(scope="module")
def ext():
    from xgpr_amd import xgpr_hip_rfgen_ext as e
    return e


@functools.lru_cache(maxsize=12)
def _randn(seed, shape, dtype=F64):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=dtype)


@functools.lru_cache(maxsize=12)
def _rows(seed, n, m):
    """float32 feature rows in (-1, 1), as the value tests draw them."""
    return torch.rand((n, m), generator=torch.Generator().manual_seed(seed), dtype=F32) * 2 - 1


def _signs(seed, shape):
    return (torch.randint(0, 2, shape, generator=torch.Generator().manual_seed(seed), dtype=I8) * 2 - 1).to(I8)


def _pow2(width):
    return 1 << max(1, int(np.ceil(np.log2(width))))


def _equal(a, b):
    if isinstance(a, np.ndarray):
        return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint8).reshape(-1),
                                                                              np.ascontiguousarray(b).view(np.uint8).reshape(-1))
    return same_bits(a, b)


def both_ways(ext, monkeypatch, fn, shape):
    plain = fn(ext, Plain(DEV), *shape)
    arena = Arena(DEV)
    with monkeypatch.context() as mp:
        patched_workspaces(mp, ext, arena)
        guarded = fn(ext, arena, *shape)
        arena.verify()
    assert sorted(plain) == sorted(guarded) and len(plain) > 0
    for name in plain:
        assert _equal(plain[name], guarded[name]), f"{name}: the guarded run differs from the plain run"
    return plain, guarded, arena


# ---------------------------------------------------------------------------------------------- fixed-vector operators
@row(["xgpr_rbf_feature_gen_f32", "xgpr_rbf_feature_gen_f64", "xgpr_rbf_grad_f32", "xgpr_rbf_grad_f64", "xgpr_rbf_feature_cache_f32",
      "xgpr_rbf_grad_rows_f32", "xgpr_ztz_matvec_f32", "xgpr_zty_f32"],
     [(3, 2, False, 1), (16, 100, True, 5), (100, 3000, True, 777), (64, 6146, True, 5), (513, 4096, True, 5), (4000, 8192, True, 5)])
def fixed_vector(ext, A, d, rffs, icpt, n):
    return run_fixed(ext, fixed_case(n, d, rffs, GRAD_SCALE), icpt, A)


# ---------------------------------------------------------------------------------------------- sequence operators
def _seqlens(n, L, cw):
    lens = np.random.default_rng([n, L, cw]).integers(cw, L + 1, size=n)
    lens[0], lens[-1] = cw, L
    return tuple(int(v) for v in lens)


@row(["xgpr_conv1d_fgen_f32", "xgpr_conv1d_fgen_f64", "xgpr_conv_grad_f32", "xgpr_conv_grad_f64", "xgpr_conv1d_maxpool_f32",
      "xgpr_conv1d_maxpool_f64", "xgpr_conv_feature_rows_f32", "xgpr_conv_grad_rows_f32"],
     [(17, 4, 1, 64, 1, 21), (40, 21, 5, 600, 2, 7), (25, 8, 3, 2050, 0, 5), (30, 500, 3, 2600, 1, 37), (30, 21, 9, 256, 1, 70)])
def sequence(ext, A, L, C_, cw, rffs, sc, n):
    return run_seq(ext, seq_case(n, L, C_, cw, rffs, _seqlens(n, L, cw)), True, A, sc)


def _token_operands(cw, C_, V, num_freqs):
    rng = np.random.default_rng([cw, C_, V, num_freqs])
    lens = np.asarray([cw, TOKEN_L, min(cw + 1, TOKEN_L), max(TOKEN_L - 1, cw), (cw + TOKEN_L) // 2, cw, TOKEN_L], dtype=np.int32)
    tokens = rng.integers(0, V, size=(TOKEN_N, TOKEN_L)).astype(np.uint8)
    table = rng.standard_normal((V, C_)).astype(np.float32)
    P = _pow2(cw * C_)
    radem = rng.choice(np.asarray([-1, 1], dtype=np.int8), size=(3, 1, -(-num_freqs // P) * P))
    chi = (0.2 + rng.random(num_freqs)).astype(np.float32)
    return [torch.from_numpy(a) for a in (tokens, table, radem, chi)] + [lens]


def _smallest(grid):
    return sorted(grid, key=lambda g: (g[0] * g[1], g[2]))[:2]


@row(["xgpr_conv_token_rows_f32"], [g + (f,) for g in _smallest(GRID) for f in (300, 1500)])
def token_rows(ext, A, cw, C_, V, num_freqs):
    tokens, table, radem, chi, lens = _token_operands(cw, C_, V, num_freqs)
    assert ext.conv_token_rows_ok(cw * C_, V, C_) == 1
    rows = A.out((TOKEN_N, 2 * num_freqs), F32, name="rows")
    ext.hipConvTokenRows(A.inp(tokens, name="tokens"), A.inp(table, name="table"), rows, A.inp(radem, name="radem"), A.inp(chi, name="chi"),
                         lens, cw, 1, True)
    return {"rows": rows}


@row(["xgpr_conv_token_grad_rows_f32"], [g + (f,) for g in _smallest(GRAD_GRID) for f in (300, 1500)])
def token_grad_rows(ext, A, cw, C_, V, num_freqs):
    tokens, table, radem, chi, lens = _token_operands(cw, C_, V, num_freqs)
    z, g = A.out((TOKEN_N, 2 * num_freqs), F32, name="zrows"), A.out((TOKEN_N, 2 * num_freqs), F32, name="grows")
    ext.hipConvTokenGradRows(A.inp(tokens, name="tokens"), A.inp(table, name="table"), z, g, A.inp(radem, name="radem"),
                             A.inp(chi, name="chi"), lens, 0.7312, cw, 1, True)
    return {"zrows": z, "grows": g}


# ---------------------------------------------------------------------------------------------- MiniARD
@row(["xgpr_mini_ard_grad_f32", "xgpr_mini_ard_grad_f64"], [(0, "f32"), (0, "f64"), (4, "f32"), (4, "f64")])
def mini_ard(ext, A, index, tag):
    case = ard_case(*ARD[index])
    x, w = (torch.from_numpy(a) for a in case.typed(np.float32 if tag == "f32" else np.float64))
    out = A.out((case.n, case.rffs), F64, name="out")
    grad = A.out((case.n, case.rffs, case.nl), F64, name="grad")
    ext.hipMiniARDGrad(A.inp(x, offset_elems=1, name="x"), out, A.inp(w, offset_elems=1, name="W"),       # any element-aligned address
                       A.inp(torch.from_numpy(case.sigma_map), name="sigma_map"), A.inp(torch.from_numpy(case.sigma_vals), name="sigma_vals"),
                       grad, True)
    return {"out": out, "grad": grad}


# ---------------------------------------------------------------------------------------------- transforms
@row(["xgpr_fht_f32", "xgpr_fht_f64", "xgpr_srht_f32", "xgpr_srht_f64"], [(3, 8), (37, 64), (5, 512), (3, 16384), (2, 32768)])
def transforms(ext, A, n, P):
    got = {}
    radem = _signs(P, (P,))
    for dtype in (F32, F64):
        x = _randn(n * P, (n, P)).to(dtype)
        a = A.out((n, P), dtype, init=x, name=f"fht2d {dtype}")
        ext.hipFastHadamardTransform2D(a)
        b = A.out((n, 2, P // 2), dtype, init=x.reshape(n, 2, P // 2), name=f"fht3d {dtype}")
        ext.hipFastHadamardTransform(b)
        c = A.out((n, P), dtype, init=x, name=f"srht {dtype}")
        ext.hipSRHT(c, A.inp(radem, name="radem"))
        got.update({f"fht2d {dtype}": a, f"fht3d {dtype}": b, f"srht {dtype}": c})
    return got


@row(["xgpr_srht_sample_f32", "xgpr_srht_sample_f64"], [(3, 4, 2), (5, 300, 17), (9, 4097, 100)])
def srht_sample(ext, A, n, m, rank):
    P = _pow2(m)
    radem = _signs(m, (P,))
    sampler = torch.randperm(P, generator=torch.Generator().manual_seed(m))[:rank].to(I64)
    y = _randn(n, (n,))
    got = {}
    for dtype in (F32, F64):
        z = _randn(n * m, (n, m)).to(dtype)
        ins = lambda: (A.inp(z, name="z"), A.inp(radem, name="radem"), A.inp(sampler, name="sampler"))
        out = A.out((n, rank + 3), dtype, fill=7.0, name=f"out {dtype}")                    # a row pitch beyond ncols
        ext.hipSRHTSample(*ins(), out, rank)
        out2 = A.out((n, rank + 3), dtype, fill=7.0, name=f"out+zty {dtype}")
        zty = A.out((m,), F64, name=f"zty {dtype}")
        ext.hipSRHTSample(*ins(), out2, rank, A.inp(y, name="y"), zty, A.workspace(ext.srht_sample_workspace_bytes(m), name="srht ws"))
        assert torch.equal(out2[:, :rank], out[:, :rank])
        got.update({f"out {dtype}": out, f"out+zty {dtype}": out2, f"zty {dtype}": zty})
    return got


@row(["xgpr_srht_sample_rows_f32"], [(100, 1000, 100, False), (33, 20000, 1000, False), (40, 32768, 2048, True)])
def srht_sample_rows(ext, A, n, m, rank, icpt):
    P = _pow2(m)
    assert ext.srht_sample_rows_ok(P, rank, m)
    radem = _signs(m, (P,))
    sampler = torch.randperm(P, generator=torch.Generator().manual_seed(m))[:rank].to(I64)
    scale = float(np.float32(np.sqrt(1.0 / (m // 2 - (0.5 if icpt else 0.0)))))
    ldo = (rank + 63) // 64 * 64
    out = A.out((n, ldo), F64, fill=3.0, name="out")
    zty = A.out((m,), F64, name="zty")
    ext.hipSRHTSampleRows(A.inp(_rows(m, n, m), name="rows"), A.inp(radem, name="radem"), A.inp(sampler, name="sampler"), out, rank, icpt,
                          scale, A.inp(_randn(n, (n,)), name="y"), zty, A.workspace(ext.srht_sample_workspace_bytes(m), name="srht ws"))
    if ldo > rank:
        assert float(out[:, rank:].abs().max()) == 0.0                                      # columns ncols .. ldo - 1 are zeroed
    return {"out": out, "zty": zty}


# ---------------------------------------------------------------------------------------------- cached matvecs
def _matvec_ws(ext, A, m, name):
    freqs = m // 2
    return A.workspace(ext.ztz_workspace_bytes(m, max(2, freqs + (freqs & 1))), name=name)       # the Rademacher length of a width-2 input


@row(["xgpr_zcache_matvec_f32", "xgpr_zcache_matvec_scaled_f32", "xgpr_zcache_zty_f32", "xgpr_zcache_matvec_f16",
      "xgpr_zcache_matvec_scaled_f16"],
     [(2, False, 1), (12, True, 40), (6146, True, 5), (64, False, 9001), (3000, True, 777), (16384, False, 300)])
def cached_matvecs(ext, A, m, icpt, n):
    rows, v, y = _rows(m + n, n, m), _randn(m, (m,)), _randn(n, (n,))
    got = {}
    for name, call in (("matvec", lambda zc, o, ws: ext.hipZCacheMatvec(zc, A.inp(v, name="v"), o, icpt, ws)),
                       ("scaled", lambda zc, o, ws: ext.hipZCacheMatvecScaled(zc, A.inp(v, name="v"), o, 0.37, ws)),
                       ("zty", lambda zc, o, ws: ext.hipZCacheZtY(zc, A.inp(y, name="y"), o, icpt, ws)),
                       ("zty scaled", lambda zc, o, ws: ext.hipZCacheZtY(zc, A.inp(y, name="y"), o, False, ws, scale=0.37))):
        got[name] = A.out((m,), F64, name=name)
        call(A.inp(rows, name="rows"), got[name], _matvec_ws(ext, A, m, name + " ws"))
    if m // 2 <= ext.HALF_CACHE_MAX_FREQS and m < 16384:
        half = A.out((n, m), F16, name="half rows")
        ext.hipRowsToHalf(A.inp(rows, name="rows"), half)
        got["half rows"] = half
        h = half.detach().clone()
        for name, call in (("half", lambda zc, o, ws: ext.hipZCacheMatvecHalf(zc, A.inp(v, name="v"), o, icpt, ws)),
                           ("half scaled", lambda zc, o, ws: ext.hipZCacheMatvecHalfScaled(zc, A.inp(v, name="v"), o, 0.37, ws))):
            got[name] = A.out((m,), F64, name=name)
            call(A.inp(h, name="half rows in"), got[name], _matvec_ws(ext, A, m, name + " ws"))
    return got


@row(["xgpr_rows_pack_f16"], [(2,), (1022,), (65542,)])
def rows_to_half(ext, A, count):
    out = A.out((count,), F16, name="half")
    ext.hipRowsToHalf(A.inp(_randn(count, (count,), F32), name="rows"), out)
    return {"half": out}


# ---------------------------------------------------------------------------------------------- block products
@row(["xgpr_zcache_block_matvec_f32", "xgpr_zcache_block_project_f32", "xgpr_zcache_block_backproject_f32"],
     [(1, 8, 1, False), (15, 4, 3, True), (257, 2100, 26, False), (300, 640, 1, True), (133, 1024, 3, True), (2000, 8192, 10, False)])
def block_products(ext, A, n, m, k, icpt):
    rows, v, r = _rows(n + m + k, n, m), _randn(m * k, (m, k)), _randn(n * k + 1, (n, k))
    base_m, base_b = _randn(m * k + 2, (m, k)), _randn(m * k + 3, (m, k))
    zc, vecs, resid = (lambda: A.inp(rows, name="rows")), (lambda: A.inp(v, name="v")), (lambda: A.inp(r, name="resid"))
    ws = lambda nm: A.workspace(ext.zcache_block_workspace_bytes(n, m, k), name=nm)
    got = {"matvec": A.out((m, k), F64, name="matvec"), "matvec acc": A.out((m, k), F64, init=base_m, name="matvec acc"),
           "project": A.out((n, k), F64, name="project"), "project ws": A.out((n, k), F64, name="project ws"),
           "back": A.out((m, k), F64, name="back"), "back acc": A.out((m, k), F64, init=base_b, name="back acc")}
    ext.hipZCacheBlockMatvec(zc(), vecs(), got["matvec"], icpt, ws("matvec ws"), 0.25)
    ext.hipZCacheBlockMatvec(zc(), vecs(), got["matvec acc"], icpt, ws("matvec acc ws"), 0.25, accumulate=True)
    need = ext.zcache_block_project_workspace_bytes(n, m, k)
    ext.hipZCacheBlockProject(zc(), vecs(), got["project ws"], icpt, 0.25, A.workspace(need, name="project ws"))
    saved = ext.zcache_block_project_workspace_bytes
    ext.zcache_block_project_workspace_bytes = lambda *a: 0                                  # the wrapper then passes workspace = NULL
    try:
        ext.hipZCacheBlockProject(zc(), vecs(), got["project"], icpt, 0.25)
    finally:
        ext.zcache_block_project_workspace_bytes = saved
    ext.hipZCacheBlockBackproject(zc(), resid(), got["back"], icpt, ws("back ws"), 0.25)
    ext.hipZCacheBlockBackproject(zc(), resid(), got["back acc"], icpt, ws("back acc ws"), 0.25, accumulate=True)
    return got


# ---------------------------------------------------------------------------------------------- matrix-core contractions
@row(["xgpr_sketch_gemm_f64"],
     [(0, 70, 128, 5, True, 0.5, 64), (0, 1000, 516, 37, False, 1.0, 64), (0, 16, 256, 128, True, 0.07, 128), (0, 1031, 384, 129, True, 0.05, 128),
      (1, 1, 256, 129, True, 0.07, 128), (1, 65, 128, 5, True, 0.5, 64), (1, 130, 48, 128, False, 0.2, 128), (1, 130, 4096, 128, True, 0.02, 128)])
def sketch_gemm(ext, A, bt, n, m, r, icpt, scale, pad):
    jdim, kdim = (n, m) if bt else (m, n)
    lda = (r + pad - 1) // pad * pad
    a = torch.zeros((kdim, lda), dtype=F64)
    a[:, :r] = _randn(kdim * r, (kdim, r))
    ldc = (jdim + 1) // 2 * 2
    got = {}
    for trans, shape in ((False, (r, ldc)), (True, (jdim, lda))):
        for acc in (False, True):
            name = f"trans={int(trans)} acc={int(acc)}"
            init = torch.zeros(shape, dtype=F64)
            if acc:
                init[:, :(r if trans else jdim)] = _randn(r * jdim + trans, shape)[:, :(r if trans else jdim)]
            out = A.out(shape, F64, init=init, name=name)
            need = ext.sketch_gemm_workspace_bytes(r, jdim, kdim, shape[1], trans)
            ext.hipSketchGemm(A.inp(a, name="A"), A.inp(_rows(n + m, n, m), name="rows"), out, r, bool(bt), trans, icpt, scale, accumulate=acc,
                              workspace=A.workspace(need, name=name + " ws"))
            pad_cols = out[:, (r if trans else jdim):]
            if pad_cols.numel():
                assert float(pad_cols.abs().max()) == 0.0, name                             # zero stays zero in the padding columns
            got[name] = out
    return got


@row(["xgpr_ztz_gram_f64"], [(9, 128, 128, True, 0.25), (37, 256, 128, True, 0.5), (133, 128, 128, False, 0.5), (1000, 512, 256, False, 1.0),
                             (20000, 1024, 1024, False, 0.02)])
def ztz_gram(ext, A, n, m, msub, icpt, scale):
    need = int(ext._LIB.xgpr_ztz_gram_workspace_bytes(msub, n))
    got = {}
    for acc in (False, True):
        name = f"gram acc={int(acc)}"
        init = torch.full((msub, msub + 6), 7.0, dtype=F64)
        if acc:
            init[:, :msub] = _randn(msub, (msub, msub))
        out = A.out((msub, msub + 6), F64, init=init, name=name)
        ext.hipZtZGram(A.inp(_rows(n + m, n, m), name="rows"), out, icpt, scale, accumulate=acc, workspace=A.workspace(need, name=name + " ws"))
        assert bool((out[:, msub:] == 7.0).all()), name                                     # ldc > msub: the padding is untouched
        got[name] = out
    return got


@row(["xgpr_cross_gram_f64"], [(5, 128), (16, 256), (333, 384), (2051, 256), (49365, 128)])    # the last: the stream-K spill and fix-up
def cross_gram(ext, A, n, m):
    need = int(ext._LIB.xgpr_cross_gram_workspace_bytes(m, n))
    sym = _randn(m, (m, m))
    got = {}
    for acc in (False, True):
        name = f"cross acc={int(acc)}"
        init = torch.full((m, m + 6), -3.0, dtype=F64)
        if acc:
            init[:, :m] = sym + sym.T
        buf = A.out((m, m + 6), F64, init=init, name=name)
        ext.hipCrossGram(A.inp(_rows(n + m, n, m), name="a"), A.inp(_rows(n + m + 1, n, m), name="b"), buf[:, :m], accumulate=acc,
                         workspace=A.workspace(need, name=name + " ws"))
        assert bool((buf[:, m:] == -3.0).all()), name
        got[name] = buf
    return got


# ---------------------------------------------------------------------------------------------- preconditioner
@row(["xgpr_precond_apply_f64"], [(1, 1), (300, 37), (1000, 514), (700, 513)])
def precond_apply(ext, A, m, rank):
    z = A.out((m,), F64, name="z")
    ext.hipPrecondApply(A.inp(_randn(m * rank, (m, rank)), name="U"), A.inp(_randn(rank, (rank,)).abs() + 0.1, name="inv_eig"), 0.37,
                        A.inp(_randn(m + 1, (m,)), name="r"), z, A.workspace(ext.precond_workspace_bytes(rank), name="precond ws"))
    return {"z": z}


@row(["xgpr_precond_utr_block_f64", "xgpr_precond_apply_block_f64"], [(64, 7, 1), (70, 7, 1), (1000, 513, 32), (4097, 130, 16)])
def precond_blocks(ext, A, m, rank, k):
    u, r, inv_eig = _randn(m * rank, (m, rank)), _randn(m * k + 1, (m, k)), _randn(rank, (rank,)).abs() + 0.1
    t, z = A.out((rank, k), F64, name="t"), A.out((m, k), F64, name="z")
    ext.hipPrecondUtRBlock(A.inp(u, name="U"), A.inp(r, name="R"), t, A.workspace(ext.precond_utr_block_workspace_bytes(m, rank, k), name="utr ws"))
    ext.hipPrecondApplyBlock(A.inp(u, name="U"), A.inp(inv_eig, name="inv_eig"), 0.37, A.inp(r, name="R"), z,
                             A.workspace(ext.precond_apply_block_workspace_bytes(m, rank, k), name="apply ws"))
    return {"t": t, "z": z}


# ---------------------------------------------------------------------------------------------- classifier, CG steps
@row(["xgpr_softmax_residual_f64"], [(1, 2), (257, 10), (4099, 40)])
def softmax_residual(ext, A, n, ncls):
    """Through the C entry point: the wrapper allocates the per-workgroup partial sums itself."""
    pred = A.out((n, ncls), F64, init=_randn(n * ncls, (n, ncls)), name="pred")               # in place
    labels = A.inp(torch.randint(0, ncls, (n,), generator=torch.Generator().manual_seed(n), dtype=I64), name="labels")
    parts = A.out(((n + 255) // 256,), F64, name="loss partials")
    ext._lib.check(ext._LIB.xgpr_softmax_residual_f64(C.c_void_p(pred.data_ptr()), C.c_void_p(labels.data_ptr()), n, ncls,
                                                      C.c_void_p(parts.data_ptr()), ext._stream()))
    return {"pred": pred, "parts": parts}


def _cg_vectors(m, names, k=None):
    shape = (m,) if k is None else (m, k)
    return {nm: _randn(m * 7 + i + (k or 0), shape) for i, nm in enumerate(names)}


@row(["xgpr_cg_step1_f64", "xgpr_cg_step2_f64"], [(1,), (1025,), (8192,), (8193,)])           # both sides of one batch of 8 x 1024 elements
def cg_steps(ext, A, m):
    h = _cg_vectors(m, ("w", "p", "x", "r", "z", "z_next"))
    w, x = A.out((m,), F64, init=h["w"], name="w"), A.out((m,), F64, init=h["x"], name="x")   # in place
    p, r, z, zn = (A.inp(h[nm], name=nm) for nm in ("p", "r", "z", "z_next"))
    rn, pn = A.out((m,), F64, name="r_next"), A.out((m,), F64, name="p_next")
    scal, err = A.out((4,), F64, fill=0.0, name="scal"), A.out((1,), F64, name="err_out")
    ext.hipCGStep1(w, p, x, r, rn, z, scal, 0.01, 3.3, err_out=err)
    ext.hipCGStep2(rn, zn, p, pn, scal)
    return {"w": w, "x": x, "r_next": rn, "p_next": pn, "scal": scal, "err": err}


BLOCK_STEPS = [(1, 1), (129, 3), (513, 32), (640, 26)]      # 1, 2 and 5 row blocks of 128: the partial sum unrolled by 4 and its tail; k at both ends


@row(["xgpr_cg_step1_block_f64", "xgpr_cg_step2_block_f64"], BLOCK_STEPS)
def cg_block_steps(ext, A, m, k, err=None):
    h = _cg_vectors(m, ("w", "p", "x", "r", "z", "z_next"), k)
    w, x = A.out((m, k), F64, init=h["w"], name="w"), A.out((m, k), F64, init=h["x"], name="x")
    p, r, z, zn = (A.inp(h[nm], name=nm) for nm in ("p", "r", "z", "z_next"))
    rn, pn = A.out((m, k), F64, name="r_next"), A.out((m, k), F64, name="p_next")
    rz, alpha, beta = (A.out((k,), F64, name=nm) for nm in ("rz", "alpha", "beta"))
    err = A.out((k,), F64, name="err_out") if err is None else err
    nrm = A.inp(torch.linalg.norm(h["r"], dim=0) * 1.7, name="init_norm")
    need = ext.cg_block_workspace_bytes(m, k)
    ext.hipCGStep1Block(w, p, x, r, rn, z, rz, alpha, err, nrm, 0.01, A.workspace(need, name="step 1 ws"))
    ext.hipCGStep2Block(rn, zn, p, pn, rz, beta, A.workspace(need, name="step 2 ws"))
    return {"w": w, "x": x, "r_next": rn, "p_next": pn, "rz": rz, "alpha": alpha, "beta": beta, "err": err}


@pytest.mark.parametrize("fn,shape", ROWS)
def test_memory_contract(ext, monkeypatch, fn, shape):
    both_ways(ext, monkeypatch, fn, shape)


# ---------------------------------------------------------------------------------------------- the block steps' values
def _rel(got, want):
    got, want = np.asarray(got.cpu() if isinstance(got, torch.Tensor) else got), np.asarray(want)
    return float(np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-300))


@pytest.mark.parametrize("m,k", BLOCK_STEPS)
def test_block_cg_steps_equal_the_float64_formulas(ext, monkeypatch, m, k):
    """The formulas of tests/test_gpu_cg.py::test_precond_apply_and_fused_cg_steps per column, at its 1e-12 relative bar; err_out once
    on the device (the table row) and once in pinned host memory with a sentinel on each side."""
    h = {nm: t.numpy() for nm, t in _cg_vectors(m, ("w", "p", "x", "r", "z", "z_next"), k).items()}
    lam2 = 0.01
    nrm = np.linalg.norm(h["r"], axis=0) * 1.7
    w2 = h["w"] + lam2 * h["p"]
    rz = (h["r"] * h["z"]).sum(axis=0)
    alpha = rz / (h["p"] * w2).sum(axis=0)
    rn = h["r"] - alpha * w2
    beta = (rn * h["z_next"]).sum(axis=0) / rz
    want = {"w": w2, "x": h["x"] + alpha * h["p"], "r_next": rn, "p_next": h["z_next"] + beta * h["p"], "rz": rz, "alpha": alpha, "beta": beta,
            "err": np.linalg.norm(h["r"], axis=0) / nrm}
    pinned = torch.full((k + 2,), -77.0, dtype=F64).pin_memory()
    arena = Arena(DEV)
    with monkeypatch.context() as mp:
        patched_workspaces(mp, ext, arena)
        got = cg_block_steps(ext, arena, m, k, err=pinned[1:k + 1])
        arena.verify()
    assert float(pinned[0]) == -77.0 and float(pinned[-1]) == -77.0                          # the sentinels survive
    for name, ref in want.items():
        for j in range(k):
            col = (lambda a: a[..., j])
            assert _rel(col(got[name]), col(ref)) < 1e-12, (name, j)
    on_device = cg_block_steps(ext, Plain(DEV), m, k)
    for name in want:
        assert _equal(got[name].cpu(), on_device[name].cpu()), name                          # pinned err_out: the same bits as on the device


# ---------------------------------------------------------------------------------------------- the device-side stop
def test_cg_steps_leave_every_vector_untouched_after_the_device_side_stop(ext):
    """stop_tol > 0 (include/xgpr_hip.h): once the previous iteration's error is below stop_tol, this and all later steps leave every
    vector untouched; scal[4] = stopped flag, scal[5] = iterations applied, scal[8 + i] = error of iteration i."""
    m, maxit, lam2 = 1025, 5, 0.01
    arena = Arena(DEV)
    g = torch.Generator().manual_seed(11)
    diag = torch.rand(m, generator=g, dtype=F64) + 0.5                                      # the operator of this little solve: diag + lam2
    r0 = torch.randn(m, generator=g, dtype=F64)
    init_norm = float(torch.linalg.norm(r0))
    d = arena.inp(diag, name="diag")
    x = arena.out((m,), F64, fill=0.0, name="x")
    w = arena.out((m,), F64, name="w")
    r = [arena.out((m,), F64, init=r0, name="r0"), arena.out((m,), F64, name="r1")]
    p = [arena.out((m,), F64, init=r0, name="p0"), arena.out((m,), F64, name="p1")]
    scal0 = torch.zeros(8 + maxit, dtype=F64)
    scal0[2] = float("inf")
    scal = arena.out((8 + maxit,), F64, init=scal0, name="scal")

    def iteration(cur, stop_tol):
        nxt = 1 - cur
        torch.mul(d, p[cur], out=w)                                                          # w arrives holding A p without lam2 p
        ext.hipCGStep1(w, p[cur], x, r[cur], r[nxt], r[cur], scal, lam2, init_norm, stop_tol=stop_tol)     # no preconditioner: z = r
        ext.hipCGStep2(r[nxt], r[nxt], p[cur], p[nxt], scal, stop_tol=stop_tol)
        return nxt

    # the errors of a plain run decide the tolerance: larger than the second iteration's error, smaller than the first's
    probe = Arena(DEV)
    px, pw = probe.out((m,), F64, fill=0.0), probe.out((m,), F64)
    pr, pp = [probe.out((m,), F64, init=r0), probe.out((m,), F64)], [probe.out((m,), F64, init=r0), probe.out((m,), F64)]
    pscal = probe.out((4,), F64, fill=0.0)
    errs, cur = [], 0
    for _ in range(3):
        torch.mul(d, pp[cur], out=pw)
        ext.hipCGStep1(pw, pp[cur], px, pr[cur], pr[1 - cur], pr[cur], pscal, lam2, init_norm)
        ext.hipCGStep2(pr[1 - cur], pr[1 - cur], pp[cur], pp[1 - cur], pscal)
        errs.append(float(pscal[2]))
        cur = 1 - cur
    probe.verify()
    assert errs[1] < errs[0]
    stop_tol = 0.5 * (errs[0] + errs[1])                                                     # errs[1] < stop_tol < errs[0]

    cur = iteration(0, stop_tol)                    # iteration 0: applied (no previous error)
    cur = iteration(cur, stop_tol)                  # iteration 1: applied (previous error 1.0 >= stop_tol); its error is below stop_tol
    torch.cuda.synchronize()
    frozen = [t.detach().clone() for t in (x, r[0], r[1], p[0], p[1])]
    ap = d * p[cur]
    cur = iteration(cur, stop_tol)                  # iteration 2: stopped on the device; w keeps what this test's own torch.mul wrote
    assert same_bits(w, ap)
    w_before = w.detach().clone()
    ext.hipCGStep1(w, p[cur], x, r[cur], r[1 - cur], r[cur], scal, lam2, init_norm, stop_tol=stop_tol)
    ext.hipCGStep2(r[1 - cur], r[1 - cur], p[cur], p[1 - cur], scal, stop_tol=stop_tol)
    arena.verify()                                   # the guard behind scal included
    assert same_bits(w, w_before)
    for t, before in zip((x, r[0], r[1], p[0], p[1]), frozen):
        assert same_bits(t, before)
    s = scal.cpu().numpy()
    assert s[4] == 1.0 and s[5] == 2.0
    assert s[8] == errs[0] and s[9] == errs[1] and np.all(s[10:] == 0.0)                     # the applied iterations' errors, nothing beyond


# ---------------------------------------------------------------------------------------------- negative controls on the device
def test_the_arena_reports_a_packer_overrun_on_the_device(ext):
    """hipRowsToHalf on 1024 values into an output the arena believes to hold 1023: the 1024th lands in the rear guard (inside the
    arena's allocation) and verify() names the array."""
    arena = Arena(DEV)
    out = arena.out((1023,), F16, name="short half")
    full = torch.as_strided(out, (1024,), (1,), out.storage_offset())
    ext.hipRowsToHalf(arena.inp(_randn(1024, (1024,), F32) + 3.0, name="rows"), full)
    msgs = arena.violations()
    assert len(msgs) == 1 and msgs[0].startswith("short half ") and "rear guard changed, bytes +0 .. +1" in msgs[0], msgs
    with pytest.raises(AssertionError, match="short half"):
        arena.verify()


def test_the_arena_reports_use_of_the_last_workspace_bytes(ext):
    """The library is told the true workspace size, the arena that the workspace is 16 bytes shorter; a report is due exactly when the
    operator uses its last 16 bytes.
    hipZCacheBlockBackproject at (133, 1024, 3, intercept) does NOT: xgpr_zcache_block_workspace_bytes is t + slabs + the projection's
    partial sums, in that order, and the back-projection has no use for the last area (measured on the MI355X: 706560 bytes advertised,
    the last 16 still 0xFF afterwards, no report).  So for that operator the test only asserts that report and bytes agree, and the
    control that must fire is hipCGStep1Block at (129, 3): its partial sums part[block][q][column] (cg_kernels.inc) fill the advertised
    2 x 3 x 3 doubles to the last one.  (The packer control above is the one for outputs.)"""
    n, m, k = 133, 1024, 3
    need = ext.zcache_block_workspace_bytes(n, m, k)
    arena = Arena(DEV)
    ws = arena.workspace(need, name="short workspace", _registered=need - 16)
    out = arena.out((m, k), F64, name="back")
    ext.hipZCacheBlockBackproject(arena.inp(_rows(n + m + k, n, m), name="rows"), arena.inp(_randn(n * k + 1, (n, k)), name="resid"), out, True,
                                  ws, 0.25)
    torch.cuda.synchronize()
    used_tail = bool((ws[need - 16:] != 0xFF).any())
    msgs = arena.violations()
    print(f"backproject ({n}, {m}, {k}): advertised {need} bytes, last 16 bytes {'written' if used_tail else 'not written'}")
    if used_tail:
        assert len(msgs) == 1 and msgs[0].startswith("short workspace ") and "rear guard changed" in msgs[0], msgs
    else:
        assert msgs == []

    m, k = 129, 3
    need = ext.cg_block_workspace_bytes(m, k)
    assert need == 2 * 3 * 3 * 8
    arena = Arena(DEV)
    h = _cg_vectors(m, ("w", "p", "x", "r", "z"), k)
    w, x = arena.out((m, k), F64, init=h["w"], name="w"), arena.out((m, k), F64, init=h["x"], name="x")
    p, r, z = (arena.inp(h[nm], name=nm) for nm in ("p", "r", "z"))
    rn, rz, alpha, err = arena.out((m, k), F64, name="r_next"), arena.out((k,), F64, name="rz"), arena.out((k,), F64, name="alpha"), arena.out((k,), F64, name="err")
    nrm = arena.inp(torch.linalg.norm(h["r"], dim=0), name="init_norm")
    ext.hipCGStep1Block(w, p, x, r, rn, z, rz, alpha, err, nrm, 0.01, arena.workspace(need, name="short partial sums", _registered=need - 16))
    msgs = arena.violations()
    assert len(msgs) == 1 and msgs[0].startswith("short partial sums ") and "rear guard changed, bytes +0 .. +15" in msgs[0], msgs
    with pytest.raises(AssertionError, match="short partial sums"):
        arena.verify()


COVERED.update(["xgpr_cg_step1_f64", "xgpr_cg_step2_f64", "xgpr_rows_pack_f16"])
