"""CPU-only checks of the float32-rows predicate (SORFKernel.rows_ok): beyond padded width 4096, where no fused
regenerate-and-reduce kernel runs, the fixed-vector kernels still write float32 feature rows, so the resident cache and
the block operators are available there; at and below 4096 every predicate answers as before."""
import pytest

from xgpr_amd.kernels import make_kernel, SORFKernel


@pytest.mark.parametrize("d", [5000, 9000, 40000])
def test_wide_inputs_have_rows_cache_and_block_but_no_fused_kernel(d):
    k = make_kernel("RBF", (1, d), 8192, device="cpu")
    assert k.rows_ok() and k.cache_ok() and k.block_ok()
    assert not k.fused_ok()


@pytest.mark.parametrize("name,parms", [("Matern", {"matern_nu": 5 / 2}), ("Cauchy", {})])
def test_wide_rows_for_every_fixed_vector_kernel(name, parms):
    k = make_kernel(name, (1, 5000), 4096, device="cpu", kernel_spec_parms=parms)
    assert k.rows_ok() and k.cache_ok() and k.block_ok() and not k.fused_ok()


def test_wide_rows_envelope():
    # beyond 16384 frequencies the cache is applied through the block contractions (num_rffs % 4 == 0)
    k = make_kernel("RBF", (1, 5000), 2 * 20001, device="cpu")
    assert k.rows_ok() and not k.block_ok() and not k.cache_ok()
    k = make_kernel("RBF", (1, 5000), 2 * 20002, device="cpu")
    assert k.rows_ok() and k.block_ok() and k.cache_ok()
    # the solver's k = 1 rows route needs what the cached matvec needs (cache_ok), not rows alone
    from xgpr_amd.cg import rows_matvec_ok
    assert not rows_matvec_ok(make_kernel("RBF", (1, 5000), 2 * 20001, device="cpu"))
    assert rows_matvec_ok(make_kernel("RBF", (1, 5000), 2 * 20002, device="cpu"))
    assert rows_matvec_ok(make_kernel("RBF", (1, 5000), 8194, device="cpu"))
    # the launcher's frequency limit
    k = make_kernel("RBF", (1, 5000), 2 * 65538, device="cpu")
    assert not k.rows_ok() and not k.cache_ok() and not k.block_ok()


def test_narrow_inputs_keep_their_predicates():
    k = make_kernel("RBF", (1, 1500), 8192, device="cpu")
    assert k.fused_ok() and k.rows_ok() and k.cache_ok() and k.block_ok()
    k = make_kernel("RBF", (1, 1500), 8194, device="cpu")          # num_rffs % 4 != 0: no block operators
    assert k.fused_ok() and k.rows_ok() and k.cache_ok() and not k.block_ok()


def test_switching_off_the_fused_kernels_switches_off_the_cache_at_narrow_width(monkeypatch):
    k = make_kernel("RBF", (1, 1500), 8192, device="cpu")
    monkeypatch.setattr(SORFKernel, "fused_ok", lambda self: False)
    assert not k.rows_ok() and not k.cache_ok()


def test_convolution_and_mini_ard_kernels_are_unchanged():
    conv = make_kernel("Conv1dRBF", (1, 60, 21), 2048, device="cpu", kernel_spec_parms={"conv_width": 5})
    assert not hasattr(conv, "rows_ok")
    assert not conv.fused_ok() and conv.cache_ok() and conv.block_ok()
    wide = make_kernel("Conv1dRBF", (1, 600, 21), 2048, device="cpu", kernel_spec_parms={"conv_width": 300})
    assert not hasattr(wide, "rows_ok") and not wide.fused_ok()
    ard = make_kernel("MiniARD", (1, 40), 1024, device="cpu", kernel_spec_parms={"split_points": [20]})
    assert not hasattr(ard, "rows_ok")
    assert not ard.fused_ok()
