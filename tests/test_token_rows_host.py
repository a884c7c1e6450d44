"""Token-indexed sequence input, the parts that need no GPU: TokenBatch semantics on CPU tensors, the checks of the dataset
builders, the host-only plan function, and the argument validation of the two token entry points through the C ABI (dummy
device pointers that are never dereferenced, as in test_launcher_validation_host.py: no row reaches a launch)."""
import numpy as np
import pytest
import torch

from xgpr_amd import _lib
from xgpr_amd import xgpr_hip_rfgen_ext as ext
from xgpr_amd.dataset import TokenBatch, build_classification_dataset, build_regression_dataset
from xgpr_amd.kernels import scale_input

A = 0x100000                     # a dummy 4096-byte-aligned address
BIG = 1 << 30
SEQLEN = np.asarray([5, 12, 7, 9], dtype=np.int32)            # valid for L = 12, conv_width <= 5
SEQLEN_SHORT = np.asarray([5, 12, 2, 9], dtype=np.int32)


def _batch(n=11, L=9, V=21, C=5, seed=0):
    g = torch.Generator().manual_seed(seed)
    tokens = torch.randint(0, V, (n, L), generator=g, dtype=torch.int64).to(torch.uint8)
    tokens[0, 0], tokens[-1, -1] = 0, V - 1
    table = torch.randn((V, C), generator=g, dtype=torch.float32)
    return TokenBatch(tokens, table)


def test_token_batch_shape_slicing_and_indexing():
    tb = _batch()
    assert tuple(tb.shape) == (11, 9, 5) and len(tb) == 11 and tb.dim() == 3
    dense = tb.dense()
    assert dense.dtype == torch.float32 and tuple(dense.shape) == (11, 9, 5)
    assert torch.equal(dense, tb.table[tb.tokens.long()])
    part = tb[3:8]
    assert isinstance(part, TokenBatch) and part.table is tb.table and tuple(part.shape) == (5, 9, 5)
    assert torch.equal(part.dense(), dense[3:8])
    assert torch.equal(tb[3:8, ...].dense(), dense[3:8])
    idx = torch.tensor([10, 0, 4, 4])
    for sel in (idx, idx.numpy(), idx.tolist()):
        picked = tb[sel]
        assert isinstance(picked, TokenBatch) and picked.table is tb.table
        assert torch.equal(picked.dense(), dense[idx])
    assert tuple(tb[5:5].shape) == (0, 9, 5)
    with pytest.raises(IndexError):
        tb[2]
    with pytest.raises(IndexError):
        tb[:, 1]


@pytest.mark.parametrize("sigma", [1.0, 0.5, 0.7312, 3.0000001, 1e-3])
def test_scaling_the_table_is_scaling_the_dense_array(sigma):
    tb = _batch(seed=3)
    scaled = tb.scaled(sigma)
    assert scaled.tokens is tb.tokens and scaled.table.dtype == torch.float32
    assert torch.equal(scaled.dense(), scale_input(tb.dense(), sigma))


def test_token_batch_rejects_other_dtypes():
    tb = _batch()
    with pytest.raises(RuntimeError):
        TokenBatch(tb.tokens.to(torch.int32), tb.table)
    with pytest.raises(RuntimeError):
        TokenBatch(tb.tokens, tb.table.to(torch.float64))
    with pytest.raises(RuntimeError):
        TokenBatch(tb.tokens, torch.zeros((257, 3)))


BUILDERS = [(build_regression_dataset, lambda n: np.linspace(-1.0, 1.0, n)),
            (build_classification_dataset, lambda n: np.arange(n) % 3)]


@pytest.mark.parametrize("build,ymake", BUILDERS)
def test_dataset_builders_check_token_input_once(build, ymake):
    n, L, V, C = 10, 8, 21, 4
    rng = np.random.default_rng(5)
    tokens = rng.integers(0, V, size=(n, L)).astype(np.int64)
    table = rng.standard_normal((V, C)).astype(np.float32)
    lens = rng.integers(3, L + 1, size=n)
    y = ymake(n)
    kw = dict(sequence_lengths=lens, chunk_size=4, device="cpu")
    with pytest.raises(RuntimeError, match="integer tokens"):
        build(tokens.astype(np.float32), y, token_table=table, **kw)
    bad = tokens.copy()
    bad[3, 2] = V
    with pytest.raises(RuntimeError, match=r"\[0, 21\)"):
        build(bad, y, token_table=table, **kw)
    bad[3, 2] = -1
    with pytest.raises(RuntimeError, match=r"\[0, 21\)"):
        build(bad, y, token_table=table, **kw)
    with pytest.raises(RuntimeError, match="sequence_lengths is required"):
        build(tokens, y, token_table=table, chunk_size=4, device="cpu")
    with pytest.raises(RuntimeError, match="2d floating-point"):
        build(tokens, y, token_table=table.reshape(V, C, 1), **kw)
    with pytest.raises(RuntimeError, match="2d floating-point"):
        build(tokens, y, token_table=np.arange(V * C).reshape(V, C), **kw)
    with pytest.raises(RuntimeError, match="1 to 256 rows"):
        build(tokens, y, token_table=np.zeros((257, C), dtype=np.float32), **kw)

    ds = build(tokens, y, token_table=table, **kw)
    assert ds.get_xdim() == (n, L, C)
    x = ds.get_xdata()
    assert isinstance(x, TokenBatch) and x.tokens.dtype == torch.uint8 and tuple(x.shape) == (n, L, C)
    dense = torch.from_numpy(table)[torch.from_numpy(tokens)]
    assert torch.equal(x.dense(), dense)
    # tokens and table are all the dataset keeps: no float tensor of N * L * C elements anywhere on it, scaled or not
    xs = ds.scaled_x(0.7312)
    assert isinstance(xs, TokenBatch) and torch.equal(xs.dense(), scale_input(dense, 0.7312))
    held = [v for v in vars(ds).values() if isinstance(v, torch.Tensor)] + [t for d in vars(ds).values() if isinstance(d, dict)
                                                                           for t in d.values() if isinstance(t, torch.Tensor)]
    assert all(not (t.is_floating_point() and t.numel() >= n * L * C) for t in held)
    # the chunk generators yield the dense chunks, with their lengths
    chunks = list(ds.get_chunked_x_data())
    assert [c.shape[0] for c, _ in chunks] == [4, 4, 2]
    assert all(isinstance(c, torch.Tensor) and c.dtype == torch.float32 for c, _ in chunks)
    assert torch.equal(torch.cat([c for c, _ in chunks]), dense)
    assert np.array_equal(np.concatenate([l for _, l in chunks]), lens.astype(np.int32))
    chunks = list(ds.get_chunked_data())
    assert torch.equal(torch.cat([c for c, _, _ in chunks]), dense)
    assert sum(yc.shape[0] for _, yc, _ in chunks) == n


def test_plan_function_needs_no_gpu():
    ok = ext.conv_token_rows_ok
    assert ok(9 * 21, 21, 21) == 1
    assert ok(9 * 21, 256, 18) == 0 and ok(9 * 18, 256, 18) == 1      # a window must be whole positions; the table cap is 4608 floats
    assert ok(2 * 3, 256, 3) == 1 and ok(1024, 4, 1) == 1 and ok(21, 21, 21) == 1
    assert ok(100 * 21, 21, 21) == 0 and ok(1025, 4, 1) == 0          # windows beyond 1024 elements
    assert ok(9 * 21, 256, 21) == 0 and ok(57, 81, 57) == 0           # tables over the cap (5376, 4617 floats)
    assert ok(9 * 21, 0, 21) == 0 and ok(9 * 21, 257, 21) == 0
    assert ok(0, 21, 21) == 0 and ok(21, 21, 0) == 0
    assert ext.cudaConvTokenRows is ext.hipConvTokenRows and ext.cudaConvTokenGradRows is ext.hipConvTokenGradRows


# sequences: n = 4, L = 12, V = 21, C = 8, conv_width 3 -> windows of 24 elements, padded 32
def tok(tokens=A, table=A, zc=A, radem=A, chi=A, sh=SEQLEN, sd=A, n=4, L=12, V=21, Cc=8, m=128, F=64, R=64, nseq=4, cw=3, sc=0,
        icpt=0, ws=A, wb=BIG):
    return "xgpr_conv_token_rows_f32", (tokens, table, zc, radem, chi, sh.ctypes.data, sd, n, L, V, Cc, m, F, R, nseq, cw, sc, icpt,
                                        ws, wb, None)


def tokg(tokens=A, table=A, z=A, g=A, radem=A, chi=A, sh=SEQLEN, sd=A, n=4, L=12, V=21, Cc=8, m=128, F=64, R=64, nseq=4, sigma=1.3,
         cw=3, sc=0, icpt=0, ws=A, wb=BIG):
    return "xgpr_conv_token_grad_rows_f32", (tokens, table, z, g, radem, chi, sh.ctypes.data, sd, n, L, V, Cc, m, F, R, nseq, sigma,
                                             cw, sc, icpt, ws, wb, None)


UNSERVED = "token input serves windows of up to 1024 elements and tables of up to 4608 floats (see xgpr_conv_token_rows_ok)"
CASES = {}
for label, mk in (("rows", tok), ("grad rows", tokg)):
    CASES.update({
        f"{label}: vocab 0": (mk(V=0), (-8, "token table: vocab must be 1 .. 256 (uint8 tokens)")),
        f"{label}: vocab 257": (mk(V=257), (-8, "token table: vocab must be 1 .. 256 (uint8 tokens)")),
        f"{label}: C < 1": (mk(Cc=0), (-8, "token table: needs at least one column")),
        f"{label}: n == 0": (mk(n=0, nseq=0), (-1, "no datapoints")),
        f"{label}: odd num_rffs": (mk(m=127), (-2, "last dim of output must be even number")),
        f"{label}: num_rffs != 2 * num_freqs": (mk(m=126), (-3, "incorrect number of rffs and or freqs.")),
        f"{label}: nseq != n": (mk(nseq=3), (-5, "wrong array sizes")),
        f"{label}: conv_width > L": (mk(cw=13, R=128), (-6, "invalid conv_width")),
        f"{label}: conv_width 0": (mk(cw=0), (-6, "invalid conv_width")),
        f"{label}: R not a multiple of the padded window": (mk(R=80, F=40, m=80), (-3, "incorrect number of rffs and or freqs.")),
        f"{label}: a sequence shorter than conv_width": (mk(sh=SEQLEN_SHORT), (-7, "All sequence lengths must be >= conv width and < array size.")),
        f"{label}: no device lengths": (mk(sd=None), (-21, "seqlen_dev (device copy of the sequence lengths) is required")),
        f"{label}: null tokens": (mk(tokens=None), (-21, "tokens and table are required")),
        f"{label}: null table": (mk(table=None), (-21, "tokens and table are required")),
        f"{label}: a window beyond 1024 elements": (mk(L=300, cw=5, Cc=250, V=4, R=2048, F=64), (-20, UNSERVED)),
        f"{label}: a table over the cap": (mk(V=256, Cc=19, R=64), (-20, UNSERVED)),
        f"{label}: no workspace": (mk(ws=None, wb=0), (-21, "workspace too small (see xgpr_conv_feature_rows_workspace_bytes)")),
        f"{label}: workspace below the sign masks": (mk(wb=16), (-21, "workspace too small (see xgpr_conv_feature_rows_workspace_bytes)")),
        # order: the shape checks come before the pointers, the plan before the workspace
        f"{label}: vocab 0 and n == 0": (mk(V=0, n=0, nseq=0), (-8, "token table: vocab must be 1 .. 256 (uint8 tokens)")),
        f"{label}: null tokens and an unserved table": (mk(tokens=None, V=256, Cc=19), (-21, "tokens and table are required")),
        f"{label}: an unserved table and no workspace": (mk(V=256, Cc=19, ws=None, wb=0), (-20, UNSERVED)),
    })
CASES.update({
    "rows: null rows": (tok(zc=None), (-21, "feature rows pointer must be 8-byte aligned")),
    "rows: rows 4 bytes off": (tok(zc=A + 4), (-21, "feature rows pointer must be 8-byte aligned")),
    "grad rows: null feature rows": (tokg(z=None), (-21, "feature rows pointer must be 8-byte aligned")),
    "grad rows: null gradient rows": (tokg(g=None), (-21, "gradient rows pointer must be 8-byte aligned")),
    "grad rows: gradient rows 4 bytes off": (tokg(g=A + 4), (-21, "gradient rows pointer must be 8-byte aligned")),
})


@pytest.mark.parametrize("name", sorted(CASES))
def test_token_entry_points_validate_before_any_launch(name):
    (fn, args), expected = CASES[name]
    lib = _lib.load()
    rc = getattr(lib, fn)(*args)
    assert int(rc) != -100                                 # XGPR_ERR_HIP: the row went past validation
    assert (int(rc), _lib.last_error()) == expected


def test_header_declares_the_token_entries_and_the_workspaces_are_the_siblings():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "xgpr_hip.h")).read()
    for decl in ("int xgpr_conv_token_rows_f32(const uint8_t *tokens, const float *table,",
                 "int xgpr_conv_token_grad_rows_f32(const uint8_t *tokens, const float *table,",
                 "int xgpr_conv_token_rows_ok(long width, long vocab, long C);"):
        assert decl in header
    assert set(("xgpr_conv_token_rows_f32", "xgpr_conv_token_grad_rows_f32", "xgpr_conv_token_rows_ok")) <= set(_lib.SIGNATURES)
