"""hipKMeansAssign and hipKMeansUpdate (include/xgpr_hip_cluster.h) against the long-double reference of tests/dense_cluster.py, through
the comparisons tests/test_cluster_host.py shows to catch every planted mistake, at the smallest shapes where the kernels can go wrong:
every number of column tiles (K = 1, 7, 16 | 17 | 33 | 256 -> 1, 2, 4, 16 tiles; 128 -> 8), one float4 per row (M = 4), a ragged feature
chunk (36, 1324), ragged row tiles and workgroups (n = 1, 5, 257, 3001), a ragged column slab of the update (36, 1324), every accumulator
size of the update (K <= 16, 32, 64, 128, 256) and more than one row range (n = 3001)."""
import numpy as np
import pytest
import torch

import dense_cluster as dc

pytestmark = pytest.mark.gpu
DEV = "cuda"

#          n     M     K
SHAPES = [(1, 4, 1), (5, 4, 7), (257, 4, 256), (5, 36, 16), (257, 36, 17), (3001, 36, 33), (257, 128, 7), (3001, 128, 17),
          (257, 128, 128), (5, 1324, 33), (257, 1324, 256), (3001, 1324, 16), (3001, 128, 256)]
IDS = ["-".join(map(str, s)) for s in SHAPES]


@pytest.fixture(scope="module")
def ext():
    from xgpr_amd import xgpr_hip_rfgen_ext as e
    return e


def gpu_assign(ext, rows, centers, want_dist2=True):
    n = rows.shape[0]
    labels = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    dist2 = torch.full((n,), float("nan"), dtype=torch.float64, device=DEV) if want_dist2 else None
    ext.hipKMeansAssign(torch.from_numpy(rows).to(DEV), torch.from_numpy(centers).to(DEV), labels, dist2)
    return labels.cpu().numpy(), (dist2.cpu().numpy() if want_dist2 else None)


def gpu_update(ext, rows, labels, K, sums=None, counts=None, accumulate=False):
    M = rows.shape[1]
    sums = torch.full((K, M), float("nan"), dtype=torch.float64, device=DEV) if sums is None else sums
    counts = torch.full((K,), -7, dtype=torch.int64, device=DEV) if counts is None else counts
    ext.hipKMeansUpdate(torch.from_numpy(rows).to(DEV), torch.from_numpy(labels).to(DEV), sums, counts, accumulate=accumulate)
    return sums, counts


@pytest.mark.parametrize("n,M,K", SHAPES, ids=IDS)
def test_assign_against_the_dense_reference(ext, n, M, K):
    rows, centers = dc.make_case(n, M, K, seed=41)
    ref = dc.Assign(rows, centers)
    assert int(ref.excused().sum()) == 0          # a property of the seeded inputs: no row's runner-up lies within twice the cap
    labels, dist2 = gpu_assign(ext, rows, centers)
    assert dc.compare_assign(ref, labels, dist2) == []
    assert (labels == ref.labels).all()
    again, dist2_again = gpu_assign(ext, rows, centers)
    assert (again == labels).all() and dist2_again.tobytes() == dist2.tobytes()          # bit-identical from run to run
    only_labels, _ = gpu_assign(ext, rows, centers, want_dist2=False)                     # dist2 may be left out
    assert (only_labels == labels).all()


@pytest.mark.parametrize("n,M,K,dup", [(257, 36, 7, (1, 5)), (257, 128, 33, (2, 31)), (300, 64, 256, (17, 200))],
                         ids=["one-tile", "across-tiles", "sixteen-tiles"])
def test_identical_centres_go_to_the_lower_index(ext, n, M, K, dup):
    rows, centers = dc.make_case(n, M, K, seed=42, duplicate=dup)
    rows[: n // 3] = (centers[dup[0]] + 0.01 * rows[: n // 3]).astype(np.float32)          # a third of the rows sit at the duplicated centre
    ref = dc.Assign(rows, centers)
    assert (ref.labels == dup[0]).sum() >= n // 3 and int(ref.excused().sum()) == 0
    labels, dist2 = gpu_assign(ext, rows, centers)
    assert dc.compare_assign(ref, labels, dist2) == []
    assert not (labels == dup[1]).any() and (labels == ref.labels).all()


def test_assign_above_any_short_launch_split(ext):
    n, M, K = 66000, 64, 5
    rows, centers = dc.make_case(n, M, K, seed=43)
    z = rows.astype(np.float64)
    s = (centers * centers).sum(axis=1)[None, :] - 2 * z @ centers.T
    want = np.argmin(s, axis=1).astype(np.int32)
    part = np.partition(s, 1, axis=1)
    # numpy's float64 scores are themselves within the cap of the exact ones: a row is decided when its two best scores are further
    # apart than four caps (two for each operator); asserted for these inputs: every row is
    cap = float(dc.gamma(M + 2)) * ((centers * centers).sum(axis=1).max() + 2 * (np.abs(z) @ np.abs(centers).T).max())
    assert ((part[:, 1] - part[:, 0]) > 4 * cap).all()
    labels, dist2 = gpu_assign(ext, rows, centers)
    assert (labels == want).all()
    d = np.maximum(0, (z * z).sum(axis=1) + s[np.arange(n), want])
    cap_d = float(dc.gamma(M + 3)) * ((z * z).sum(axis=1) + (centers * centers).sum(axis=1).max() + 2 * (np.abs(z) @ np.abs(centers).T).max(axis=1))
    assert (np.abs(dist2 - d) <= 2 * cap_d).all()                                         # (one cap for each side)


def labels_for(n, K, seed, stray=False, empty=None):
    rng = np.random.default_rng([n, K, seed])
    lab = rng.integers(0, K, size=n).astype(np.int32)
    if empty is not None:
        lab[lab == empty] = (empty + 1) % K
    if stray:
        lab[::5] = -1
        lab[2::7] = K
    return lab


@pytest.mark.parametrize("n,M,K", SHAPES, ids=IDS)
def test_update_against_the_dense_reference(ext, n, M, K):
    rows, _ = dc.make_case(n, M, K, seed=44)
    lab = labels_for(n, K, 44, stray=n > 1)
    ref = dc.Update(rows, lab, K)
    sums, counts = gpu_update(ext, rows, lab, K)
    assert dc.compare_update(ref, sums.cpu().numpy(), counts.cpu().numpy()) == []
    sums2, counts2 = gpu_update(ext, rows, lab, K)
    assert torch.equal(sums.view(torch.int64), sums2.view(torch.int64)) and torch.equal(counts, counts2)


@pytest.mark.parametrize("n,M,K", [(257, 36, 7), (3001, 128, 33), (300, 1324, 256)])
def test_an_empty_cluster_gives_exact_zeros(ext, n, M, K):
    rows, _ = dc.make_case(n, M, K, seed=45)
    lab = labels_for(n, K, 45, empty=K // 2)
    ref = dc.Update(rows, lab, K)
    assert ref.counts[K // 2] == 0
    sums, counts = gpu_update(ext, rows, lab, K)
    assert dc.compare_update(ref, sums.cpu().numpy(), counts.cpu().numpy()) == []
    assert int(counts[K // 2]) == 0 and bool((sums[K // 2] == 0).all())


@pytest.mark.parametrize("n,M,K", [(257, 36, 7), (3001, 128, 33), (3001, 1324, 256)])
def test_accumulate_over_two_halves(ext, n, M, K):
    """Two calls add one more rounding per element than one call: the cap grows by u |sum| (u = 2^-53)."""
    rows, _ = dc.make_case(n, M, K, seed=46)
    lab = labels_for(n, K, 46, stray=True)
    ref = dc.Update(rows, lab, K)
    h = n // 2 + 1
    sums, counts = gpu_update(ext, rows[:h], lab[:h], K)
    gpu_update(ext, rows[h:], lab[h:], K, sums=sums, counts=counts, accumulate=True)
    extra = dc.U * (np.abs(ref.sums) + ref.cap)
    assert dc.compare_update(ref, sums.cpu().numpy(), counts.cpu().numpy(), extra_cap=extra) == []
    one, _ = gpu_update(ext, rows, lab, K)
    assert float((one - sums).abs().max()) <= float((2 * ref.cap + extra).max())


def test_no_rows(ext):
    K, M = 5, 36
    sums = torch.full((K, M), float("nan"), dtype=torch.float64, device=DEV)
    counts = torch.full((K,), -7, dtype=torch.int64, device=DEV)
    empty_rows = torch.empty((0, M), dtype=torch.float32, device=DEV)
    empty_labels = torch.empty(0, dtype=torch.int32, device=DEV)
    ext.hipKMeansUpdate(empty_rows, empty_labels, sums, counts)
    assert bool((sums == 0).all()) and bool((counts == 0).all())
    sums.fill_(1.5)
    ext.hipKMeansUpdate(empty_rows, empty_labels, sums, counts, accumulate=True)
    assert bool((sums == 1.5).all())
    ext.hipKMeansAssign(empty_rows, torch.zeros((K, M), dtype=torch.float64, device=DEV), empty_labels)


def test_refusals_launch_nothing(ext):
    rows = torch.zeros((8, 66), dtype=torch.float32, device=DEV)
    labels = torch.full((8,), -7, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ext.hipKMeansAssign(rows, torch.zeros((3, 66), dtype=torch.float64, device=DEV), labels)
    rows = torch.zeros((8, 64), dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="256 centres"):
        ext.hipKMeansAssign(rows, torch.zeros((257, 64), dtype=torch.float64, device=DEV), labels)
    sums = torch.full((257, 64), 2.0, dtype=torch.float64, device=DEV)
    with pytest.raises(RuntimeError, match="256 centres"):
        ext.hipKMeansUpdate(rows, labels, sums, torch.zeros(257, dtype=torch.int64, device=DEV))
    assert bool((labels == -7).all()) and bool((sums == 2.0).all())
