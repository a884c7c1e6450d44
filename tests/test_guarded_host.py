"""The guarded arena of tests/guarded.py on host tensors: the checker passes a clean "operator", reports each kind of violation
and names the array, keeps its alignment promises -- shown here, without a GPU, so that a green tests/test_gpu_memory_contract.py
means something.  Also: the table of that file names every entry point of include/xgpr_hip.h that writes device memory."""
import os
import re
import types

import pytest
import torch

import guarded
from guarded import Arena, Plain, patched_workspaces

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _clean_operator(x, w, out, ws):
    """out = x @ w through a workspace it fills before it reads it."""
    tmp = ws[:x.numel() * 8].view(torch.float64).reshape(x.shape)
    tmp.copy_(x)
    out.copy_(tmp @ w)


def _arrays(arena):
    x = arena.inp(torch.arange(12, dtype=torch.float64).reshape(3, 4), name="x")
    w = arena.inp(torch.ones(4, 5, dtype=torch.float64), name="w")
    out = arena.out((3, 5), torch.float64, name="out")
    ws = arena.workspace(96, name="ws")
    return x, w, out, ws


def test_a_clean_operator_passes_and_matches_the_plain_run():
    arena = Arena("cpu")
    x, w, out, ws = _arrays(arena)
    _clean_operator(x, w, out, ws)
    arena.verify()
    assert arena.violations() == []
    plain = Plain("cpu")
    po = plain.out((3, 5), torch.float64)
    _clean_operator(plain.inp(x), plain.inp(w), po, plain.workspace(96))
    assert guarded.same_bits(out, po)
    assert not guarded.same_bits(torch.zeros(1), -torch.zeros(1))              # -0 counts


def _past(t, elems):
    """A view of ``elems`` elements starting at the first element behind (elems > 0) or in front of (elems < 0) ``t``'s payload."""
    off = t.storage_offset() + (t.numel() if elems > 0 else elems)
    return torch.as_strided(t, (abs(elems),), (1,), off)


@pytest.mark.parametrize("what", ["past", "before", "workspace", "input"])
def test_each_violation_is_reported_and_names_the_array(what):
    arena = Arena("cpu")
    x, w, out, ws = _arrays(arena)
    _clean_operator(x, w, out, ws)
    arena.verify()
    if what == "past":
        _past(out.reshape(-1), 1).fill_(1.5)
        name, where = "out", "rear guard changed, bytes +0 .. +7"
    elif what == "before":
        _past(out.reshape(-1), -1).fill_(1.5)
        name, where = "out", f"front guard changed, bytes {-8 - 120} .. {-1 - 120}"
    elif what == "workspace":
        _past(ws, 1).fill_(0)
        name, where = "ws", "rear guard changed, bytes +0 .. +0"
    else:
        guarded.bits(x)[-8:].bitwise_xor_(0xFF)                                  # the last element, every byte
        name, where = "x", "input modified, bytes -8 .. -1"
    msgs = arena.violations()
    assert len(msgs) == 1 and msgs[0].startswith(name + " ") and where in msgs[0], msgs
    with pytest.raises(AssertionError, match="memory contract violated"):
        arena.verify()


def test_a_write_far_behind_the_payload_is_still_inside_the_guard():
    """The safety condition: the rear guard is at least as long as the payload (and at least 1 MiB)."""
    arena = Arena("cpu")
    out = arena.out((300000,), torch.float64, name="big")
    rec = arena.records[-1]
    assert rec.buf.numel() - rec.end >= max(1 << 20, out.numel() * 8)
    assert guarded.rear_guard_bytes(5) == 1 << 20 and guarded.rear_guard_bytes(3 << 20) == 3 << 20
    assert guarded.rear_guard_bytes(1 << 30) == 64 << 20 and guarded.FRONT_GUARD == 4096
    _past(out, out.numel())[-1] = 0.0                                            # the last element of an overrun by the payload's own size
    msgs = arena.violations()
    assert len(msgs) == 1 and msgs[0].startswith("big ") and f"+{2400000 - 8} .. +{2400000 - 1}" in msgs[0]


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32, torch.float64, torch.int8, torch.int32, torch.int64, torch.uint8])
def test_alignment_offsets_fills_and_guard_patterns(dtype):
    arena = Arena("cpu")
    item = torch.empty((), dtype=dtype).element_size()
    for off in (0, 1, 3):
        o = arena.out((5, 7), dtype, fill=3, offset_elems=off)
        assert o.data_ptr() % 256 == (off * item) % 256 and o.is_contiguous() and o.shape == (5, 7) and bool((o == 3).all())
        src = torch.arange(35).reshape(5, 7).to(dtype)
        i = arena.inp(src, offset_elems=off)
        assert i.data_ptr() % 256 == (off * item) % 256 and i.is_contiguous() and torch.equal(i, src)
        # what a read one element past the end / before the start meets
        for beyond in (_past(i.reshape(-1), 1), _past(i.reshape(-1), -1)):
            if dtype.is_floating_point:
                assert bool(torch.isnan(beyond).all())
            else:
                assert int(beyond[0]) == 0
        if dtype.is_floating_point:
            z = arena.inp(src, guard="zero")
            assert float(_past(z.reshape(-1), 1)[0]) == 0.0
    p = arena.out((4,), dtype)                                                   # no fill: 0xFF bytes
    assert bool((guarded.bits(p) == 0xFF).all())
    init = torch.arange(4).to(dtype)
    q = arena.out((2, 2), dtype, init=init.reshape(2, 2))
    assert torch.equal(q.reshape(-1), init)
    arena.verify()


def test_workspaces_are_exact_aligned_and_poisoned_also_at_zero_bytes():
    arena = Arena("cpu")
    for nbytes in (1, 96, 1000, 4097):
        ws = arena.workspace(nbytes)
        assert ws.dtype == torch.uint8 and ws.numel() == nbytes and ws.data_ptr() % 256 == 0 and bool((ws == 0xFF).all())
    stub = arena.workspace(0, name="empty")
    assert stub.numel() == 16 and stub.data_ptr() != 0 and stub.data_ptr() % 16 == 0
    arena.verify()
    stub[15] = 0                                                                 # the whole stub is guard
    msgs = arena.violations()
    assert len(msgs) == 1 and msgs[0].startswith("empty ") and "+15 .. +15" in msgs[0]


def test_the_workspace_seam_hands_out_exactly_what_was_asked_for(monkeypatch):
    ext = types.SimpleNamespace(_workspace=None)
    arena = Arena("cpu")
    patched_workspaces(monkeypatch, ext, arena)
    ws, ptr, size = ext._workspace(1000, "cpu")
    assert size.value == 1000 and ptr.value == ws.data_ptr() and ws.numel() == 1000 and ptr.value % 256 == 0
    ws, ptr, size = ext._workspace(0, "cpu")
    assert size.value == 0 and ptr.value % 16 == 0 and ptr.value != 0
    _past(arena.records[0].buf[arena.records[0].start:arena.records[0].end], 1).fill_(7)
    assert len(arena.violations()) == 1 and "internal workspace" in arena.violations()[0]


def test_the_seam_also_guards_the_device_copy_of_the_sequence_lengths(monkeypatch):
    lens = torch.tensor([3, 5, 4], dtype=torch.int32)
    ext = types.SimpleNamespace(_workspace=None, _seqlens=lambda seqlengths, device: (seqlengths.numpy(), seqlengths.clone()))
    arena = Arena("cpu")
    patched_workspaces(monkeypatch, ext, arena)
    host, dev = ext._seqlens(lens, "cpu")
    assert list(host) == [3, 5, 4] and torch.equal(dev, lens) and int(_past(dev, 1)[0]) == 0 and dev.data_ptr() % 256 == 0
    arena.verify()
    dev[1] = 9
    assert len(arena.violations()) == 1 and arena.violations()[0].startswith("device sequence lengths")


# ---------------------------------------------------------------------------------------------- the table covers the header
def _declared():
    hdr = open(os.path.join(ROOT, "include", "xgpr_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(xgpr_[a-z0-9_]+)\s*\(", hdr)))                # the expression of tests/test_cabi.py


# declared in the header, write no device memory of the caller's (host-side queries) -- or are exempt: the RCCL wrappers, the lane self test
NOT_IN_THE_TABLE = {"xgpr_last_error", "xgpr_build_arch", "xgpr_build_id", "xgpr_ztz_matvec_plan", "xgpr_conv_token_rows_ok",
                    "xgpr_rccl_load", "xgpr_rccl_unique_id", "xgpr_rccl_comm_init", "xgpr_allreduce_sum_f64", "xgpr_rccl_comm_destroy",
                    "xgpr_selftest_lane_xor"}


def test_every_entry_point_that_writes_device_memory_has_a_row():
    import test_gpu_memory_contract as table
    writers = {n for n in _declared() if not n.endswith("_workspace_bytes")} - NOT_IN_THE_TABLE
    assert len(writers) >= 45
    covered = table.covered_entry_points()
    assert covered == writers, (sorted(writers - covered), sorted(covered - writers))
    assert NOT_IN_THE_TABLE <= set(_declared())
