"""The max-pool operator over token input (hipConvTokenMaxpool, xgpr_conv_token_maxpool_f32 of include/xgpr_hip_pool.h).  The
yardstick needs no tolerance: after the window fetch the token kernel runs the code of wave_conv_kernel<LG, CONV_MAXPOOL>, so its
output must be ``torch.equal`` to what hipConv1dMaxpool leaves for the expanded array ``table[tokens]``.

Shapes.  n = 37 sequences (no multiple of the four waves of a workgroup) of L = 60 positions, lengths conv_width, L and ragged ones
in between; token positions past a sequence's length hold 255 -- outside every vocabulary below 256 -- and are never read.  The
windows cover every tile layout of the k-mer loop and both table limits; 70 / 96 / 1100 features are a ragged tile, a whole number
of 32-element transforms, and two tiles per sequence."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
N, L = 37, 60
GRID = [(1, 4, 4),          # P = 4, graph-like
        (3, 8, 21),         # P = 32, rows-only layout
        (5, 21, 21),        # P = 128
        (9, 21, 21),        # P = 256
        (9, 40, 100),       # P = 512, packed index registers
        (48, 21, 21),       # P = 1024
        (3, 18, 256),       # the 4608-float table limit
        (3, 8, 1)]          # one-row table
FEATURES = [70, 96, 1100]


@pytest.fixture(scope="module")
def ext():
    from xgpr_amd import xgpr_hip_rfgen_ext as e
    return e


def padded(width):
    return 1 << max(1, int(np.ceil(np.log2(width))))


def operands(cw, C, V, num_features, n=N, seed=0):
    """tokens with 255 behind every sequence's length, the same tokens with 0 there (what the dense expansion indexes), table,
    radem, chi, host lengths."""
    rng = np.random.default_rng([cw, C, V, num_features, n, seed])
    lens = rng.integers(cw, L + 1, size=n).astype(np.int32)
    lens[0], lens[1], lens[-1] = cw, L, cw
    valid = rng.integers(0, V, size=(n, L)).astype(np.uint8)
    valid[:, 0], valid[:, cw - 1] = 0, V - 1                                        # both ends of the vocabulary inside every sequence
    tokens = valid.copy()
    for i, n_i in enumerate(lens):
        tokens[i, n_i:] = 255
        valid[i, n_i:] = 0
    table = rng.standard_normal((V, C)).astype(np.float32)
    P = padded(cw * C)
    radem = rng.choice(np.asarray([-1, 1], dtype=np.int8), size=(3, 1, -(-num_features // P) * P))
    chi = (0.2 + rng.random(num_features)).astype(np.float32)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return to(tokens), to(valid), to(table), to(radem), to(chi), lens


@pytest.mark.parametrize("num_features", FEATURES)
@pytest.mark.parametrize("cw,C,V", GRID)
def test_token_maxpool_equals_the_dense_operator_bit_for_bit(ext, cw, C, V, num_features):
    tokens, valid, table, radem, chi, lens = operands(cw, C, V, num_features)
    assert ext.conv_token_rows_ok(cw * C, V, C) == 1
    assert int(lens.min()) == cw and int(lens.max()) == L and len(set(lens.tolist())) > 2
    if V < 256:
        assert int(tokens.max()) == 255
    dense = table[valid.long()].contiguous()
    for prefill in (0.0, 0.25):
        ref = torch.full((N, num_features), prefill, dtype=torch.float32, device=DEV)
        ext.hipConv1dMaxpool(dense, ref, radem, chi, lens, cw)
        out = torch.full_like(ref, prefill)
        ext.hipConvTokenMaxpool(tokens, table, out, radem, chi, lens, cw)
        assert torch.equal(out, ref), prefill
        # the operator takes the max with what is there: nothing below the pre-fill, and the filters did raise entries above it
        assert bool(torch.isfinite(out).all()) and float(out.min()) >= prefill and float(out.max()) > prefill
        again = torch.full_like(ref, prefill)
        ext.hipConvTokenMaxpool(tokens, table, again, radem, chi, lens, cw)
        assert torch.equal(again, out), prefill                                    # same bits twice
    # the output is read: a pre-fill above every filter response stays
    high = torch.full((N, num_features), 1e30, dtype=torch.float32, device=DEV)
    ext.hipConvTokenMaxpool(tokens, table, high, radem, chi, lens, cw)
    assert bool((high == 1e30).all())


def test_a_larger_batch_takes_the_longest_first_order(ext):
    """n >= 64 sequences: the launcher sorts them longest first (conv_order_kernel), as for the dense operator."""
    cw, C, V, F, n = 9, 21, 21, 1100, 150
    tokens, valid, table, radem, chi, lens = operands(cw, C, V, F, n=n, seed=5)
    ref = torch.zeros((n, F), dtype=torch.float32, device=DEV)
    out = torch.zeros_like(ref)
    ext.hipConv1dMaxpool(table[valid.long()].contiguous(), ref, radem, chi, lens, cw)
    ext.hipConvTokenMaxpool(tokens, table, out, radem, chi, lens, cw)
    assert torch.equal(out, ref)


def test_wrapper_errors(ext):
    cw, C, V, F = 3, 19, 256, 70                                                    # a table of 4864 floats
    tokens, valid, table, radem, chi, lens = operands(cw, C, V, F)
    assert ext.conv_token_rows_ok(cw * C, V, C) == 0
    out = torch.full((N, F), float("nan"), dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="xgpr_conv_token_rows_ok"):
        ext.hipConvTokenMaxpool(valid, table, out, radem, chi, lens, cw)
    assert bool(torch.isnan(out).all())                                            # nothing was launched
    tokens, valid, table, radem, chi, lens = operands(3, 8, 21, F)
    out = torch.zeros((N, F), dtype=torch.float32, device=DEV)
    with pytest.raises(TypeError, match="table"):
        ext.hipConvTokenMaxpool(tokens, table.to(torch.float64), out, radem, chi, lens, 3)
    with pytest.raises(TypeError, match="tokens"):
        ext.hipConvTokenMaxpool(tokens.to(torch.int32), table, out, radem, chi, lens, 3)
    with pytest.raises(TypeError, match="outputArr"):
        ext.hipConvTokenMaxpool(tokens, table, out.to(torch.float64), radem, chi, lens, 3)
    with pytest.raises(TypeError, match="seqlengths"):
        ext.hipConvTokenMaxpool(tokens, table, out, radem, chi, torch.from_numpy(lens).to(DEV), 3)
    with pytest.raises(RuntimeError, match="incorrect number of rffs"):           # radem_shape2 != reps * P
        ext.hipConvTokenMaxpool(tokens, table, out, torch.cat([radem, radem], dim=2).contiguous(), chi, lens, 3)
    assert bool((out == 0).all())
    assert ext.cudaConvTokenMaxpool is ext.hipConvTokenMaxpool
