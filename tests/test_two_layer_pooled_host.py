"""The pooled first layer of the two-layer kernel, the parts that need no GPU: the argument validation of
xgpr_conv_token_maxpool_f32 through the C ABI (dummy device pointers that are never dereferenced, as in
test_token_rows_host.py: no row reaches a launch), what the compiler made of the ten new kernel instantiations, and the host
logic -- the second-layer view of a CPU-device kernel and the rule by which the models hand the solver passes their pair."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from xgpr_amd import _lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tools"))

A = 0x100000                     # a dummy 4096-byte-aligned address
BIG = 1 << 30
SEQLEN = np.asarray([5, 12, 7, 9], dtype=np.int32)            # valid for L = 12, conv_width <= 5
SEQLEN_SHORT = np.asarray([5, 12, 2, 9], dtype=np.int32)


# sequences: n = 4, L = 12, V = 21, C = 8, conv_width 3 -> windows of 24 elements, padded 32; 64 features = two transforms
def pool(tokens=A, table=A, out=A, radem=A, chi=A, sh=SEQLEN, sd=A, n=4, L=12, V=21, Cc=8, rows=4, m=64, F=64, R=64, nseq=4, cw=3,
         ws=A, wb=BIG):
    return (tokens, table, out, radem, chi, sh.ctypes.data, sd, n, L, V, Cc, rows, m, F, R, nseq, cw, ws, wb, None)


UNSERVED = "token input serves windows of up to 1024 elements and tables of up to 4608 floats (see xgpr_conv_token_rows_ok)"
REQUIRED = "tokens, table and out are required"
RANGE = "All sequence lengths must be >= conv width and < array size."
CASES = {
    "vocab 0": (pool(V=0), (-8, "token table: vocab must be 1 .. 256 (uint8 tokens)")),
    "vocab 257": (pool(V=257), (-8, "token table: vocab must be 1 .. 256 (uint8 tokens)")),
    "C = 0": (pool(Cc=0), (-8, "token table: needs at least one column")),
    "null tokens": (pool(tokens=None), (-21, REQUIRED)),
    "null table": (pool(table=None), (-21, REQUIRED)),
    "null out": (pool(out=None), (-21, REQUIRED)),
    "a window of 1025 elements": (pool(L=300, cw=5, Cc=205, V=4, R=2048), (-20, UNSERVED)),
    "a table of 4609 floats": (pool(cw=1, Cc=419, V=11, R=512), (-20, UNSERVED)),
    "radem_shape2 != reps * P": (pool(R=128), (-3, "incorrect number of rffs and or freqs.")),
    "radem_shape2 no multiple of P": (pool(R=80), (-3, "incorrect number of rffs and or freqs.")),
    "num_freqs != num_rffs": (pool(F=32), (-3, "incorrect number of rffs and or freqs.")),
    "a sequence shorter than conv_width": (pool(sh=SEQLEN_SHORT), (-7, RANGE)),
    "a sequence longer than L": (pool(L=11), (-7, RANGE)),
    "no host lengths": (pool(sh=np.zeros(0, dtype=np.int32)), None),      # (replaced below: a NULL pointer)
    "no device lengths": (pool(sd=None), (-21, "seqlen_dev (device copy of the sequence lengths) is required")),
    "no workspace": (pool(ws=None, wb=0), (-21, "workspace too small (see xgpr_conv_workspace_bytes)")),
    "workspace below the sign masks": (pool(wb=16), (-21, "workspace too small (see xgpr_conv_workspace_bytes)")),
    "n == 0": (pool(n=0, rows=0, nseq=0), (-1, "no datapoints")),
    "out_rows != n": (pool(rows=3), (-1, "no datapoints")),
    "odd num_rffs": (pool(m=63, F=63), (-2, "last dim of output must be even number")),
    "nseq != n": (pool(nseq=3), (-5, "wrong array sizes")),
    "conv_width > L": (pool(cw=13, R=128), (-6, "invalid conv_width")),
    "conv_width 0": (pool(cw=0), (-6, "invalid conv_width")),
    # order: the shape checks come before the pointers, the plan before the workspace
    "vocab 0 and n == 0": (pool(V=0, n=0, rows=0, nseq=0), (-8, "token table: vocab must be 1 .. 256 (uint8 tokens)")),
    "null out and an unserved table": (pool(out=None, cw=1, Cc=419, V=11, R=512), (-21, REQUIRED)),
    "an unserved table and no workspace": (pool(cw=1, Cc=419, V=11, R=512, ws=None, wb=0), (-20, UNSERVED)),
}
_args = list(pool())
_args[5] = None
CASES["no host lengths"] = (tuple(_args), (-7, "seqlen_host is required (sequence lengths are validated on the host)"))


@pytest.mark.parametrize("name", sorted(CASES))
def test_token_maxpool_validates_before_any_launch(name):
    args, expected = CASES[name]
    lib = _lib.load()
    rc = lib.xgpr_conv_token_maxpool_f32(*args)
    assert int(rc) != -100                                 # XGPR_ERR_HIP: the row went past validation
    assert (int(rc), _lib.last_error()) == expected


def test_workspace_is_the_dense_operators():
    """The wrapper asks xgpr_conv_workspace_bytes for (radem_shape2, conv_width * C, 4, nseq): masks, then the order."""
    lib = _lib.load()
    assert lib.xgpr_conv_workspace_bytes(256, 189, 4, 700) >= lib.xgpr_sorf_workspace_bytes(256, 189, 4) + 4 * 700


def test_compiler_evidence_for_the_token_maxpool_instantiations():
    """Exactly the ten instantiations wave_conv_tok_kernel<1..10, 1>: no scratch, no spilled VGPR or SGPR, and register-limited
    occupancy not below the row-writer token sibling wave_conv_tok_kernel<LG, 3> of the same compile."""
    import resource_usage
    rows = {r["name"]: r for r in resource_usage.collect()}
    new = [n for n in rows if re.fullmatch(r"wave_conv_tok_kernel<\d+, 1>", n)]
    assert sorted(new) == sorted(f"wave_conv_tok_kernel<{lg}, 1>" for lg in range(1, 11))
    for name in new:
        r = rows[name]
        assert r["ScratchSize"] == 0 and r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, (name, r)
        sibling = re.sub(r", 1>$", ", 3>", name)
        assert sibling in rows and sibling != name
        assert r["Occupancy"] >= rows[sibling]["Occupancy"], (name, r["Occupancy"], rows[sibling]["Occupancy"])


# ------------------------------------------------------------------------------------------------------------ host logic
SETTINGS = {"conv_width": 3, "init_rffs": 64, "intercept": True}


def _two_layer(device="cpu", rffs=256):
    from xgpr_amd.kernels import make_kernel
    return make_kernel("Conv1dTwoLayer", (10, 12, 8), rffs, 123, device, dict(SETTINGS))


def test_second_layer_is_one_sorf_view_that_shares_the_draws():
    from xgpr_amd.kernels import SORFKernel
    k = _two_layer()
    s = k.second_layer()
    assert isinstance(s, SORFKernel) and s is k.second_layer() and s is k.second_layer()
    assert s.radem_diag is k.radem_diag and s.chi_arr is k.chi_arr                      # the same tensors: nothing was redrawn
    assert s.kernel_choice == "RBF" and s._xdim == (10, 64)
    assert s.fit_intercept is k.fit_intercept and s.num_rffs == k.num_rffs == 256 and s.num_freqs == 128
    assert s.get_num_rffs() == 256 and s.device == k.device and s.random_seed == k.random_seed
    assert _two_layer().second_layer() is not s                                         # one view per kernel object
    # what the fixed-vector machinery asks of a SORFKernel
    assert s.supports_fused and s.fused_ok() and s.rows_ok() and s.cache_ok() and s.block_ok()
    from xgpr_amd.kernels import make_kernel
    off = make_kernel("Conv1dTwoLayer", (10, 12, 8), 256, 123, "cpu", dict(SETTINGS, intercept=False))
    assert off.second_layer().fit_intercept is False


def test_hyperparameters_set_on_either_side_are_read_on_both():
    k = _two_layer()
    s = k.second_layer()
    assert np.array_equal(s.get_hyperparams(logspace=False), k.get_hyperparams(logspace=False))
    s.set_hyperparams(np.log(np.array([0.3, 1.7])), logspace=True)
    assert np.allclose(k.get_hyperparams(logspace=False), [0.3, 1.7]) and k.hyperparams is s.hyperparams
    assert float(k.get_lambda()) == float(s.get_lambda()) == pytest.approx(0.3)
    k.set_hyperparams(np.array([0.5, 0.7312]), logspace=False)
    assert np.array_equal(s.get_hyperparams(logspace=False), [0.5, 0.7312]) and float(s.hyperparams[1]) == 0.7312
    assert np.array_equal(s.get_hyperparams(), np.log([0.5, 0.7312]))
    twin = s.sibling(128)                                                               # the rank check's smaller twin
    assert twin.num_rffs == 128 and twin.owner is not k and np.array_equal(twin.hyperparams, k.hyperparams)
    assert torch.equal(twin.owner.radem_diag1, k.radem_diag1) and torch.equal(twin.owner.chi_arr1, k.chi_arr1)


def test_the_two_layer_kernel_gains_no_row_writer_attributes():
    import inspect
    from xgpr_amd.kernels import Conv1dTwoLayerKernel
    k = _two_layer()
    for attr in ("fill_feature_rows", "seq_rows_ok", "rows_ok"):
        assert not hasattr(k, attr), attr
    assert list(inspect.signature(Conv1dTwoLayerKernel.fill_grad_rows).parameters) == ["self", "x_unscaled", "zrows", "grows",
                                                                                       "sequence_length"]
    assert callable(k.pool) and callable(k.second_layer)


class _Pooling:
    """A dataset with ``pooled``: records the kernel it was asked with."""
    def __init__(self):
        self.asked = []

    def get_xdim(self):
        return (10, 12, 8)

    def pooled(self, kernel):
        self.asked.append(kernel)
        return "pooled dataset"


class _Chunked:
    """A dataset class without a resident shard: no ``pooled``."""
    def get_xdim(self):
        return (10, 12, 8)


def _model(kernel_choice, device, xdim_dataset, settings=None, cls=None):
    from xgpr_amd.models import xGPRegression
    model = (cls or xGPRegression)(num_rffs=256, kernel_choice=kernel_choice, device=device, kernel_settings=settings, verbose=False)
    model._initialize_kernel(xdim_dataset)
    return model


def test_solver_pair_rule(monkeypatch):
    from xgpr_amd.models import _ModelBase, xGPClassification, xGPRegression
    assert _ModelBase.pool_first_layer is True
    settings = dict(SETTINGS, matern_nu=2.5, averaging="none")
    # the route: a two-layer kernel on a HIP device over a dataset with ``pooled``
    for cls in (xGPRegression, xGPClassification):
        ds = _Pooling()
        model = _model("Conv1dTwoLayer", "cpu", ds, settings, cls)
        assert model._solver_pair(ds) == (model.kernel, ds) and ds.asked == []          # a CPU device: as it is
        monkeypatch.setattr(model.kernel, "device", "cuda")                             # the device check as on a HIP device
        assert model._solver_pair(ds) == (model.kernel.second_layer(), "pooled dataset") and ds.asked == [model.kernel]
        plain = _Chunked()
        assert model._solver_pair(plain) == (model.kernel, plain)                       # a dataset without ``pooled``
        model.pool_first_layer = False
        assert model._solver_pair(ds) == (model.kernel, ds) and ds.asked == [model.kernel]
        assert cls.pool_first_layer is True                                             # (the instance's switch only)
    # other kernels, whatever the device says
    class _Fixed(_Pooling):
        def get_xdim(self):
            return (10, 9)
    for name, ds in (("RBF", _Fixed()), ("Conv1dRBF", _Pooling()), ("GraphRBF", _Pooling())):
        model = _model(name, "cpu", ds, settings)
        monkeypatch.setattr(model.kernel, "device", "cuda")
        assert model._solver_pair(ds) == (model.kernel, ds) and ds.asked == []


def test_device_dataset_has_pooled_and_caches_by_kernel_object():
    """``DeviceDataset.pooled`` on host tensors with a stub in place of the first layer (the real one needs a device): the pooled
    dataset shares everything but x, is cached by kernel OBJECT and survives set_hyperparams; an empty shard pools nothing."""
    from xgpr_amd.dataset import DeviceDataset

    class Stub:
        init_rffs, device = 6, "cpu"

        def __init__(self):
            self.calls = 0
            self.hyperparams = np.ones(2)

        def pool(self, x, sl):
            self.calls += 1
            assert sl is not None and len(sl) == x.shape[0]
            return torch.full((x.shape[0], self.init_rffs), 2.0, dtype=torch.float32)

    x = torch.zeros((5, 12, 8), dtype=torch.float32)
    y = torch.arange(5, dtype=torch.float64)
    lens = np.full(5, 12, dtype=np.int32)
    ds = DeviceDataset(x, y, lens, chunk_size=3, trainy_mean=2.0, trainy_std=1.5, ndatapoints=11, device="cpu", max_class=None)
    k = Stub()
    p = ds.pooled(k)
    assert isinstance(p, DeviceDataset) and p is ds.pooled(k) and k.calls == 1
    k.hyperparams = np.array([0.3, 1.7])
    assert ds.pooled(k) is p and k.calls == 1
    assert tuple(p.get_xdata().shape) == (5, 6) and p.get_xdata().dtype == torch.float32
    assert p.get_sequence_lengths() is None and p.get_xdim() == (11, 6) and p.get_ndatapoints() == 11
    assert p._ydata is ds._ydata and p.comm is ds.comm and p.get_chunk_size() == 3 and p.get_n_classes() is None
    assert (p.get_ymean(), p.get_ystd()) == (2.0, 1.5)
    assert tuple(p.scaled_x(0.5).shape) == (5, 8) and float(p.scaled_x(0.5)[0, 0]) == 1.0      # rows padded to four floats
    other = Stub()
    assert ds.pooled(other) is not p and other.calls == 1                               # another kernel object: pooled again
    empty = DeviceDataset(x[:0], y[:0], lens[:0], chunk_size=3, ndatapoints=11, device="cpu")
    k2 = Stub()
    pe = empty.pooled(k2)
    assert k2.calls == 0 and tuple(pe.get_xdata().shape) == (0, 6) and pe.get_xdata().dtype == torch.float32
    assert pe.get_ndatapoints() == 11
