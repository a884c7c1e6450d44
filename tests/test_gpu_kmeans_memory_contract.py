"""The memory contract of the entry points of include/xgpr_hip_cluster.h, in the pattern of
tests/test_gpu_pool_input_grad_memory_contract.py: each writer runs once the plain way and once with every array it sees -- rows,
centers / labels, the outputs and the workspace, exactly the bytes its *_workspace_bytes function advertises, 0xFF-poisoned -- inside
the guarded arena of tests/guarded.py.  No guard band may change, no input may be modified, and both runs must agree bit for bit (the
workspace's contents do not enter).  One ``update`` case carries labels outside [0, K): that is where a stray write would land."""
import numpy as np
import pytest
import torch

import dense_cluster as dc
from guarded import Arena, Plain, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"

COVERED = {"xgpr_kmeans_assign_f32", "xgpr_kmeans_update_f32"}
#           n     M    K
SHAPES = [(5, 4, 1),                 # one ragged row tile, one float4 per row, one centre
          (257, 36, 17),             # a ragged feature chunk, two column tiles, a second ragged workgroup
          (3001, 128, 33),           # four column tiles, several row ranges
          (300, 1324, 256)]          # sixteen column tiles, the 128 KiB accumulator, a ragged column slab


def covered_entry_points():
    return set(COVERED)


@pytest.fixture(scope="module")
def ext():
    from xgpr_amd import xgpr_hip_rfgen_ext as e
    return e


def run_assign(ext, A, n, M, K):
    rows, centers = dc.make_case(n, M, K, seed=31)
    labels = A.out((n,), torch.int32, name="labels")
    dist2 = A.out((n,), torch.float64, name="dist2")
    need = int(ext._LIB.xgpr_kmeans_assign_workspace_bytes(n, M, K))
    ws = A.workspace(need, name="workspace")
    ext.hipKMeansAssign(A.inp(torch.from_numpy(rows), name="rows"), A.inp(torch.from_numpy(centers), name="centers"), labels, dist2,
                        workspace=ws)
    return labels, dist2, need


def run_update(ext, A, n, M, K, stray):
    rows, _ = dc.make_case(n, M, K, seed=32)
    rng = np.random.default_rng([n, M, K])
    lab = rng.integers(0, K, size=n).astype(np.int32)
    if stray:
        lab[::3] = np.asarray([-1, K, K + 1000, -(2 ** 31), 2 ** 31 - 1], dtype=np.int32)[np.arange(len(lab[::3])) % 5]
    sums = A.out((K, M), torch.float64, name="sums")
    counts = A.out((K,), torch.int64, name="counts")
    need = int(ext._LIB.xgpr_kmeans_update_workspace_bytes(n, M, K))
    ws = A.workspace(need, name="workspace")
    ext.hipKMeansUpdate(A.inp(torch.from_numpy(rows), name="rows"), A.inp(torch.from_numpy(lab), name="labels"), sums, counts,
                        workspace=ws)
    return sums, counts, need, lab


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_assign_memory_contract(ext, shape):
    plain_l, plain_d, _ = run_assign(ext, Plain(DEV), *shape)
    arena = Arena(DEV)
    lab, d2, need = run_assign(ext, arena, *shape)
    arena.verify()
    assert {r.name for r in arena.records} == {"labels", "dist2", "workspace", "rows", "centers"}
    ws = next(r for r in arena.records if r.name == "workspace")
    assert ws.end - ws.start == need > 0                                   # exactly what is advertised
    assert same_bits(plain_l, lab) and same_bits(plain_d, d2), "the guarded run differs from the plain run"
    assert int(lab.min()) >= 0 and int(lab.max()) < shape[2] and bool(torch.isfinite(d2).all())


@pytest.mark.parametrize("stray", [False, True], ids=["in-range", "stray-labels"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_update_memory_contract(ext, shape, stray):
    plain_s, plain_c, _, _ = run_update(ext, Plain(DEV), *shape, stray)
    arena = Arena(DEV)
    sums, counts, need, lab = run_update(ext, arena, *shape, stray)
    arena.verify()
    assert {r.name for r in arena.records} == {"sums", "counts", "workspace", "rows", "labels"}
    ws = next(r for r in arena.records if r.name == "workspace")
    assert ws.end - ws.start == need > 0
    assert same_bits(plain_s, sums) and same_bits(plain_c, counts), "the guarded run differs from the plain run"
    inside = (lab >= 0) & (lab < shape[2])
    assert int(counts.sum()) == int(inside.sum()) and bool(torch.isfinite(sums).all())
    assert stray == bool((~inside).any())


@pytest.mark.parametrize("which", ["assign", "update"])
def test_a_workspace_one_byte_short_is_refused(ext, which):
    n, M, K = 300, 36, 5
    rows, centers = dc.make_case(n, M, K, seed=33)
    rd = torch.from_numpy(rows).to(DEV)
    labels = torch.zeros(n, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="workspace too small"):
        if which == "assign":
            need = int(ext._LIB.xgpr_kmeans_assign_workspace_bytes(n, M, K))
            ext.hipKMeansAssign(rd, torch.from_numpy(centers).to(DEV), labels, workspace=torch.empty(need - 1, dtype=torch.uint8, device=DEV))
        else:
            need = int(ext._LIB.xgpr_kmeans_update_workspace_bytes(n, M, K))
            sums = torch.zeros((K, M), dtype=torch.float64, device=DEV)
            counts = torch.zeros(K, dtype=torch.int64, device=DEV)
            ext.hipKMeansUpdate(rd, labels, sums, counts, workspace=torch.empty(need - 1, dtype=torch.uint8, device=DEV))
            assert float(sums.abs().max()) == 0.0
    assert int(labels.abs().max()) == 0
