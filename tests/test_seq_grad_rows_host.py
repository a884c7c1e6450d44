"""CPU-only checks of the exact NMLL gradient's float32-rows route for the sequence, graph and two-layer kernels: the exported
symbols and their argument types, which kernel classes carry the predicate, the route's rule over shards, and what the compiler
made of the new kernel instantiations (no device needed for any of it)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SEQ = ["Conv1dRBF", "Conv1dMatern", "Conv1dCauchy", "GraphRBF", "GraphMatern", "GraphCauchy", "Conv1dTwoLayer"]


def _make(name, rffs=256, device="cpu"):
    from xgpr_amd.kernels import make_kernel
    return make_kernel(name, (10, 12, 8), rffs, 123, device, {"conv_width": 3, "matern_nu": 2.5, "init_rffs": 64})


def test_symbols_are_exported_with_the_declared_argument_types():
    from xgpr_amd import _lib
    from xgpr_amd import xgpr_hip_rfgen_ext as ext
    lib = _lib.load()
    vp, lg, it, db, sz = C.c_void_p, C.c_long, C.c_int, C.c_double, C.c_size_t
    fn = lib.xgpr_conv_grad_rows_f32
    # x, zrows, grows, radem, chi, seqlen_host, seqlen_dev | n, L, C, num_rffs, num_freqs, radem_shape2, nseq | sigma |
    # conv_width, scaling_type, fit_intercept | workspace, workspace_bytes, stream
    assert list(fn.argtypes) == [vp] * 7 + [lg] * 7 + [db] + [it] * 3 + [vp, sz, vp] and fn.restype is C.c_int
    fn = lib.xgpr_conv_grad_rows_workspace_bytes
    assert list(fn.argtypes) == [lg] * 4 and fn.restype is sz
    assert callable(ext.hipConvGradRows)
    header = open(os.path.join(ROOT, "include", "xgpr_hip.h")).read()
    assert "int xgpr_conv_grad_rows_f32(" in header and "size_t xgpr_conv_grad_rows_workspace_bytes(" in header


def test_workspace_covers_the_feature_rows_layout_and_two_staging_arrays():
    """Up to windows of 1024 elements: masks + order, as the feature rows.  Staged shapes: two float64 arrays of the same number
    of rows, together within the 256 MiB the feature-rows staging is bounded by."""
    from xgpr_amd import _lib
    lib = _lib.load()
    for width in (21, 189, 1000):
        assert lib.xgpr_conv_grad_rows_workspace_bytes(4096, width, 256, 70) == lib.xgpr_conv_feature_rows_workspace_bytes(4096, width, 256, 70)
    base = lib.xgpr_conv_feature_rows_workspace_bytes(8192, 5000, 256, 0)          # no sequences: no staging, no order
    got = lib.xgpr_conv_grad_rows_workspace_bytes(8192, 5000, 256, 37)
    assert got == base + 256 + 2 * 37 * 256 * 8                                   # (256: the order of 37 sequences, rounded up)
    big = lib.xgpr_conv_grad_rows_workspace_bytes(8192, 5000, 8192, 1 << 20)
    assert big - lib.xgpr_conv_feature_rows_workspace_bytes(8192, 5000, 8192, 0) - (4 << 20) <= 256 << 20


@pytest.mark.parametrize("name", SEQ)
def test_sequence_kernels_carry_the_gradient_rows_predicate(name, monkeypatch):
    k = _make(name)
    assert callable(k.grad_rows_ok) and callable(k.fill_grad_rows)
    assert k.grad_rows_ok() is False                # a CPU-device kernel never takes the route
    monkeypatch.setattr(k, "device", "cuda")        # the device check as on a HIP device; the arrays stay on the host
    assert k.grad_rows_ok() is True                 # M = 256: whole 128 x 128 tiles
    k = _make(name, rffs=320)
    monkeypatch.setattr(k, "device", "cuda")
    assert k.grad_rows_ok() is False


def test_fixed_vector_signature_and_the_kernels_without_a_route_are_unchanged():
    import inspect
    from xgpr_amd.kernels import SORFKernel, ConvSORFKernel, Conv1dTwoLayerKernel, make_kernel
    assert list(inspect.signature(SORFKernel.fill_grad_rows).parameters) == ["self", "x_unscaled", "zrows", "grows"]
    for cls in (ConvSORFKernel, Conv1dTwoLayerKernel):
        assert list(inspect.signature(cls.fill_grad_rows).parameters) == ["self", "x_unscaled", "zrows", "grows", "sequence_length"]
    for name, parms in (("MiniARD", {"split_points": [3]}), ("Linear", {})):
        assert not hasattr(make_kernel(name, (10, 8), 128, 123, "cpu", parms), "grad_rows_ok")


class _OnDevice(torch.Tensor):
    """A host tensor that answers ``is_cuda`` as a resident shard does (the route only asks; it reads nothing here)."""
    is_cuda = property(lambda self: True)


class _Shard:
    def __init__(self, x, lens):
        self._x, self._lens = x, lens

    def get_xdata(self):
        return self._x

    def get_sequence_lengths(self):
        return self._lens


class _Chunks:                                      # a dataset class without a resident shard
    def get_sequence_lengths(self):
        raise AssertionError("the route must not be probed further")


@pytest.mark.parametrize("name", ["Conv1dRBF", "GraphMatern", "Conv1dTwoLayer"])
def test_route_over_shards(name, monkeypatch):
    from xgpr_amd import nmll
    k = _make(name)
    lens = np.full(10, 12, dtype=np.int32)
    x32 = torch.zeros((10, 12, 8), dtype=torch.float32).as_subclass(_OnDevice)
    assert not nmll._grad_rows_route(_Shard(x32, lens), k)                 # the kernel's own predicate says no (CPU device)
    monkeypatch.setattr(type(k), "grad_rows_ok", lambda self: True)
    assert nmll._grad_rows_route(_Shard(x32, lens), k)
    assert not nmll._grad_rows_route(_Shard(x32, None), k)                 # no lengths
    assert not nmll._grad_rows_route(_Shard(x32.double().as_subclass(_OnDevice), lens), k)
    assert not nmll._grad_rows_route(_Shard(torch.zeros((10, 12, 8)), lens), k)      # a host tensor
    assert not nmll._grad_rows_route(_Shard(x32.transpose(1, 2), lens), k)           # not contiguous
    assert not nmll._grad_rows_route(_Shard(torch.zeros((10, 96)).as_subclass(_OnDevice), lens), k)     # 2-d: not this kernel's shard
    assert not nmll._grad_rows_route(_Chunks(), k)


def test_fixed_vector_route_keeps_its_rule(monkeypatch):
    from xgpr_amd import nmll
    from xgpr_amd.kernels import make_kernel
    k = make_kernel("RBF", (10, 9), 256, 123, "cpu", {})
    monkeypatch.setattr(type(k), "grad_rows_ok", lambda self: True)
    x2 = torch.zeros((10, 9), dtype=torch.float32).as_subclass(_OnDevice)
    assert nmll._grad_rows_route(_Shard(x2, None), k)
    assert not nmll._grad_rows_route(_Shard(x2.double().as_subclass(_OnDevice), None), k)
    assert not nmll._grad_rows_route(_Shard(torch.zeros((10, 3, 3), dtype=torch.float32).as_subclass(_OnDevice), np.ones(10, np.int32)), k)


def test_rows_route_hands_every_window_its_lengths(monkeypatch):
    """_gradient_terms_rows pairs each window of sequences with the matching slice of the host lengths (windows of 4 over 10
    sequences: 4, 4, 2); the four accumulations are stubbed out -- they need a device."""
    from xgpr_amd import nmll
    from xgpr_amd import xgpr_hip_rfgen_ext as ext
    k = _make("Conv1dRBF")
    lens = (np.arange(10, dtype=np.int32) % 7) + 3
    x = torch.arange(10 * 12 * 8, dtype=torch.float32).reshape(10, 12, 8)
    seen = []

    class DS(_Shard):
        def normalized_y(self):
            return torch.arange(10, dtype=torch.float64)
    monkeypatch.setattr(type(k), "fill_grad_rows", lambda self, xw, zr, gr, sl: seen.append((xw.clone(), zr.shape, gr.shape, sl.copy())))
    monkeypatch.setattr(nmll, "_grad_window_rows", lambda m: 4)
    for nm in ("hipZtZGram", "hipCrossGram", "hipZCacheBlockBackproject"):
        monkeypatch.setattr(ext, nm, lambda *a, **kw: None)
    monkeypatch.setattr(ext, "zcache_block_workspace_bytes", lambda *a: 16)
    f64 = dict(dtype=torch.float64)
    yty = torch.zeros(1, **f64)
    nmll._gradient_terms_rows(DS(x, lens), k, torch.zeros((256, 256), **f64), torch.zeros(256, **f64), torch.zeros((256, 1), **f64),
                              torch.zeros((256, 256, 1), **f64), yty)
    assert [s[0].shape[0] for s in seen] == [4, 4, 2]
    for (xw, zs, gs, sl), lo in zip(seen, (0, 4, 8)):
        assert torch.equal(xw, x[lo:lo + 4]) and np.array_equal(sl, lens[lo:lo + 4]) and zs == gs == (xw.shape[0], 256)
    assert float(yty) == float(sum(i * i for i in range(10)))


def test_compiler_evidence_for_the_gradient_rows_instantiations():
    """Every instantiation added for the writer: no scratch, no spilled VGPR, no spilled SGPR, and register-limited occupancy not
    below its float64-output gradient sibling at the same window width in the same compile -- wave_conv_kernel<LG, 4> against
    wave_conv_kernel<LG, 2>, wave_tile_conv_kernel<float, LG, 7> against <float, LG, 3>."""
    import resource_usage
    rows = {r["name"]: r for r in resource_usage.collect()}
    new = [n for n in rows if re.fullmatch(r"wave_conv_kernel<\d+, 4>", n) or re.fullmatch(r"wave_tile_conv_kernel<float, \d+, 7>", n)]
    assert sorted(new) == sorted([f"wave_conv_kernel<{lg}, 4>" for lg in range(1, 11)]
                                 + [f"wave_tile_conv_kernel<float, {lg}, 7>" for lg in (11, 12)])
    for name in new:
        r = rows[name]
        assert r["ScratchSize"] == 0 and r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, (name, r)
        sibling = re.sub(r", 4>$", ", 2>", name) if name.startswith("wave_conv_kernel") else re.sub(r", 7>$", ", 3>", name)
        assert sibling in rows and sibling != name
        assert rows[name]["Occupancy"] >= rows[sibling]["Occupancy"], (name, rows[name]["Occupancy"], rows[sibling]["Occupancy"])
