"""The memory contract of the two writers of include/xgpr_hip_indel_scan.h, in the pattern of
tests/test_gpu_subst_scan_memory_contract.py: each runs once the plain way and once with every array it sees -- tokens, table, w, radem,
chi, the device copy of the lengths, the scores, the outputs and the workspace, exactly the bytes xgpr_rbf_workspace_bytes advertises,
0xFF-poisoned -- inside the guarded arena of tests/guarded.py.  No guard band may change (no write outside an output), no input may be
modified (the scan reads the scores as a guarded input), and both runs must agree bit for bit (the workspace's contents do not
enter).  The tokens past a sequence's length are 255, a row the table does not have: one that was read would gather from beyond the
table.  A full-length sequence's append gap sits at the array's end: the byte behind it is the guard band."""
import numpy as np
import pytest
import torch

import dense_indel_scan as dis
from guarded import Arena, Plain, patched_workspaces, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64

COVERED = {"xgpr_conv_token_window_scores_f32", "xgpr_conv_token_indel_scan_f32"}
SHAPES = ["w16_c4_cw3", "w128_c21_cw6", "w1024_c21_cw48", "graph_cw1", "vocab256_c18"]


def covered_entry_points():
    return set(COVERED)


@pytest.fixture(scope="module")
def ext():
    from xgpr_amd import xgpr_hip_rfgen_ext as e
    return e


def _inputs(A, c):
    return {k: A.inp(torch.from_numpy(c[k]), name=k) for k in ("tokens", "table", "w", "radem", "chi")}


def window_scores(ext, A, name):
    c, cw, _, icpt = dis.case(name)
    scores = A.out(c["tokens"].shape, F64, name="scores")
    need = int(ext._LIB.xgpr_rbf_workspace_bytes(c["radem"].shape[2]))
    ws = A.workspace(need, name="internal workspace")
    dev = _inputs(A, c)
    ext.hipConvTokenWindowScores(dev["tokens"], dev["table"], dev["w"], scores, dev["radem"], dev["chi"], c["seqlen"], cw, icpt, workspace=ws)
    return scores, need


def indel_scan(ext, A, name, scores):
    c, cw, scaling, icpt = dis.case(name)
    n, L = c["tokens"].shape
    dele = A.out((n, L), F64, name="del")
    ins = A.out((n, L + 1, c["table"].shape[0]), F64, name="ins")
    need = int(ext._LIB.xgpr_rbf_workspace_bytes(c["radem"].shape[2]))
    ws = A.workspace(need, name="internal workspace")
    dev = _inputs(A, c)
    sc = A.inp(scores, name="scores")
    ext.hipConvTokenIndelScan(dev["tokens"], dev["table"], dev["w"], sc, dele, ins, dev["radem"], dev["chi"], c["seqlen"], cw, scaling, icpt,
                              workspace=ws)
    return dele, ins, need


INPUTS = {"internal workspace", "tokens", "table", "w", "radem", "chi", "device sequence lengths"}


def _workspace_is_exact(arena, need):
    ws = next(r for r in arena.records if r.name.split("#")[0] == "internal workspace")
    assert ws.end - ws.start == need > 0                                   # exactly what is advertised


@pytest.mark.parametrize("name", SHAPES)
def test_memory_contract_of_the_window_scores(ext, name, monkeypatch):
    plain, _ = window_scores(ext, Plain(DEV), name)
    arena = Arena(DEV)
    patched_workspaces(monkeypatch, ext, arena)              # (the device copy of the lengths becomes a guarded input)
    guarded, need = window_scores(ext, arena, name)
    arena.verify()
    assert {r.name.split("#")[0] for r in arena.records} == INPUTS | {"scores"}
    _workspace_is_exact(arena, need)
    assert same_bits(plain, guarded), "the guarded run differs from the plain run"
    assert bool(torch.isfinite(plain).all()) and float(plain.abs().max()) > 0


@pytest.mark.parametrize("name", SHAPES)
def test_memory_contract_of_the_scan(ext, name, monkeypatch):
    scores, _ = window_scores(ext, Plain(DEV), name)
    pd, pi, _ = indel_scan(ext, Plain(DEV), name, scores)
    arena = Arena(DEV)
    patched_workspaces(monkeypatch, ext, arena)
    gd, gi, need = indel_scan(ext, arena, name, scores)
    arena.verify()
    assert {r.name.split("#")[0] for r in arena.records} == INPUTS | {"scores", "del", "ins"}
    _workspace_is_exact(arena, need)
    assert same_bits(pd, gd) and same_bits(pi, gi), "the guarded run differs from the plain run"
    c, cw, _, _ = dis.case(name)
    nan = torch.from_numpy((np.arange(c["tokens"].shape[1])[None, :] < c["seqlen"][:, None]) & (c["seqlen"][:, None] == cw)).to(DEV)
    assert bool((torch.isnan(pd) == nan).all()) and bool(torch.isfinite(pi).all()) and float(pi.abs().max()) > 0


def test_a_workspace_one_byte_short_is_refused(ext):
    c, cw, scaling, icpt = dis.case("w16_c4_cw3")
    n, L = c["tokens"].shape
    need = int(ext._LIB.xgpr_rbf_workspace_bytes(c["radem"].shape[2]))
    scores = torch.zeros((n, L), dtype=F64, device=DEV)
    dele = torch.zeros((n, L), dtype=F64, device=DEV)
    ins = torch.zeros((n, L + 1, c["table"].shape[0]), dtype=F64, device=DEV)
    short = torch.empty(need - 1, dtype=torch.uint8, device=DEV)
    dev = {k: torch.from_numpy(c[k]).to(DEV) for k in ("tokens", "table", "w", "radem", "chi")}
    with pytest.raises(RuntimeError, match="workspace too small"):
        ext.hipConvTokenWindowScores(dev["tokens"], dev["table"], dev["w"], scores, dev["radem"], dev["chi"], c["seqlen"], cw, icpt,
                                     workspace=short)
    with pytest.raises(RuntimeError, match="workspace too small"):
        ext.hipConvTokenIndelScan(dev["tokens"], dev["table"], dev["w"], scores, dele, ins, dev["radem"], dev["chi"], c["seqlen"], cw,
                                  scaling, icpt, workspace=short)
    assert float(scores.abs().max()) == 0.0 and float(dele.abs().max()) == 0.0 and float(ins.abs().max()) == 0.0
