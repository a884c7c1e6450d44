"""CPU-only checks of the float32 feature rows of the sequence kernels (Conv1d* / Graph* RBF, Matern, Cauchy): which kernel
classes carry the new predicate, what the compiler made of the new kernel instantiations, and the window bookkeeping of the
solver passes (no device needed for any of it)."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _make(name, xdim, parms=None, rffs=512):
    from xgpr_amd.kernels import make_kernel
    return make_kernel(name, xdim, rffs, 123, "cpu", parms or {})


@pytest.mark.parametrize("name", ["Conv1dRBF", "Conv1dMatern", "Conv1dCauchy", "GraphRBF", "GraphMatern", "GraphCauchy"])
def test_sequence_kernels_carry_the_rows_predicate(name):
    parms = {"conv_width": 3, "matern_nu": 2.5}
    k = _make(name, (10, 12, 8), parms)
    assert callable(k.fill_feature_rows) and callable(k.seq_rows_ok)
    assert not hasattr(k, "rows_ok") and not k.fused_ok()
    assert k.seq_rows_ok() is False                 # a CPU-device kernel: there is no operator to write the rows
    assert k.cache_ok() and k.block_ok()
    assert not _make(name, (10, 12, 8), parms, rffs=510).block_ok()
    assert not _make(name, (10, 12, 8), parms, rffs=2 * 16385).cache_ok()
    from xgpr_amd import cg
    assert not cg.seq_rows_ok(k) and not cg.any_rows_ok(k) and not cg.rows_matvec_ok(k)


def test_other_kernels_have_neither_attribute():
    two = _make("Conv1dTwoLayer", (10, 12, 8), {"conv_width": 3, "init_rffs": 64})
    ard = _make("MiniARD", (10, 16), {"split_points": [8]})
    lin = _make("Linear", (10, 16))
    for k in (two, ard, lin):
        assert not hasattr(k, "fill_feature_rows") and not hasattr(k, "seq_rows_ok")
    from xgpr_amd import cg
    assert not cg.seq_rows_ok(two) and not cg.seq_rows_ok(ard) and not cg.seq_rows_ok(lin)


def test_a_dataset_without_a_resident_shard_keeps_its_chunk_loops(monkeypatch):
    from xgpr_amd import cg
    k = _make("GraphRBF", (10, 12, 8))
    monkeypatch.setattr(type(k), "seq_rows_ok", lambda self: True)       # as on a HIP device

    class Chunks:                                                       # no scaled_x, no get_sequence_lengths
        pass

    class Shard:
        def scaled_x(self, sigma):
            raise AssertionError

        def get_sequence_lengths(self):
            return None
    assert cg.seq_rows_ok(k) and cg.seq_rows_ok(k, Shard()) and not cg.seq_rows_ok(k, Chunks())
    assert cg.rows_matvec_ok(k, Shard()) and not cg.rows_matvec_ok(k, Chunks())


@pytest.mark.parametrize("n,win", [(10, 4), (10, 5), (3, 8), (1, 1), (4097, 1024), (0, 16)])
def test_sequence_windows_cover_the_shard_with_their_lengths(n, win):
    """Contiguous, non-overlapping ranges in order that cover range(n), each with the matching slice of the host lengths: a
    ragged last window, an exact fit, a shard smaller than one window, an empty shard."""
    from xgpr_amd.cg import window_ranges
    lens = (np.arange(n, dtype=np.int32) * 7) % 13 + 1
    got = list(window_ranges(n, win, lens))
    assert len(got) == -(-n // win)
    nxt = 0
    for lo, hi, sl in got:
        assert lo == nxt and lo < hi <= n and hi - lo <= win
        assert sl.dtype == np.int32 and np.array_equal(sl, lens[lo:hi])
        nxt = hi
    assert nxt == n
    assert all(hi - lo == win for lo, hi, _ in got[:-1])
    assert [(lo, hi) for lo, hi, _ in window_ranges(n, win)] == [(lo, hi) for lo, hi, _ in got]
    assert all(sl is None for _, _, sl in window_ranges(n, win))


def test_compiler_evidence_for_the_rows_instantiations():
    """Every instantiation added for the operator: no scratch, no spilled VGPR, no spilled SGPR, and register-limited occupancy
    not below its float64-output sibling at the same window width in the same compile -- wave_conv_kernel<LG, 3> against
    wave_conv_kernel<LG, 0>, wave_tile_conv_kernel<float, LG, 6> against <float, LG, 2>."""
    import resource_usage
    rows = {r["name"]: r for r in resource_usage.collect()}
    new = [n for n in rows if re.fullmatch(r"wave_conv_kernel<\d+, 3>", n) or re.fullmatch(r"wave_tile_conv_kernel<float, \d+, 6>", n)]
    assert sorted(new) == sorted([f"wave_conv_kernel<{lg}, 3>" for lg in range(1, 11)]
                                 + [f"wave_tile_conv_kernel<float, {lg}, 6>" for lg in (11, 12)])
    assert "round_rows_kernel" in rows
    for name in new + ["round_rows_kernel"]:
        r = rows[name]
        assert r["ScratchSize"] == 0 and r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, (name, r)
    for name in new:
        sibling = re.sub(r", 3>$", ", 0>", name) if name.startswith("wave_conv_kernel") else re.sub(r", 6>$", ", 2>", name)
        assert sibling in rows and sibling != name
        assert rows[name]["Occupancy"] >= rows[sibling]["Occupancy"], (name, rows[name]["Occupancy"], rows[sibling]["Occupancy"])
