"""The k-means operators without a GPU: the dense reference of tests/dense_cluster.py catches every planted mistake through the
comparison the GPU tests use (and passes it unplanted); the sixth public header, include/xgpr_hip_cluster.h, held to what
tests/test_pool_input_grad_host.py holds the fifth; the launchers' argument validation through the C ABI (nothing reaches a HIP
call: device pointers are dummy integers); the workspace sizes and the shape predicate on the host; and a Lloyd loop over the dense
helper on three blobs -- the GPU tests' comparison target, itself under test."""
import ctypes
import os
import re
import shutil

import numpy as np
import pytest

import dense_cluster as dc
from test_cabi import _build_module

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "include", "xgpr_hip_cluster.h")
NAMES = ["xgpr_kmeans_assign_f32", "xgpr_kmeans_assign_workspace_bytes", "xgpr_kmeans_ok", "xgpr_kmeans_update_f32",
         "xgpr_kmeans_update_workspace_bytes"]


# ------------------------------------------------------------------------------------------------ 1. the plants
def test_the_unplanted_reference_passes_its_own_comparison():
    rows, centers = dc.make_case(257, 36, 17, seed=1)
    ref = dc.Assign(rows, centers)
    assert int(ref.excused().sum()) == 0
    assert dc.compare_assign(ref, ref.labels, ref.dist2.astype(np.float64)) == []
    labels = ref.labels.copy()
    labels[::7] = -1
    labels[3::11] = 17
    up = dc.Update(rows, labels, 17)
    assert dc.compare_update(up, up.sums.astype(np.float64), up.counts) == []


@pytest.mark.parametrize("mistake", ["no_center_norm", "plus_sign"])
def test_a_wrong_score_is_caught(mistake):
    rows, centers = dc.make_case(257, 36, 17, seed=1)
    ref = dc.Assign(rows, centers)
    bad = dc.Assign(rows, centers, mistake=mistake)
    problems = dc.compare_assign(ref, bad.labels, bad.dist2.astype(np.float64))
    assert problems, mistake
    print(mistake, problems)


def test_the_last_index_among_tied_centres_is_caught():
    rows, centers = dc.make_case(257, 36, 7, seed=2, duplicate=(1, 5))
    ref = dc.Assign(rows, centers)
    assert ((ref.labels == 1).sum() > 0) and not (ref.labels == 5).any()      # some rows choose the duplicated centre: the lower index
    assert int(ref.excused().sum()) == 0                                       # (the gap is taken to the next DISTINCT score)
    bad = dc.Assign(rows, centers, mistake="last_tie")
    assert (bad.labels == 5).any()
    assert dc.compare_assign(ref, bad.labels, bad.dist2.astype(np.float64))
    assert dc.compare_assign(ref, ref.labels, ref.dist2.astype(np.float64)) == []


@pytest.mark.parametrize("mistake", ["sum_all_rows", "count_out_of_range"])
def test_a_wrong_update_is_caught(mistake):
    rows, _ = dc.make_case(257, 36, 7, seed=3)
    labels = np.random.default_rng(3).integers(-1, 8, size=257).astype(np.int32)       # -1 and 7 = K are out of range
    assert (labels == -1).any() and (labels == 7).any()
    ref = dc.Update(rows, labels, 7)
    bad = dc.Update(rows, labels, 7, mistake=mistake)
    assert dc.compare_update(ref, bad.sums.astype(np.float64), bad.counts), mistake


def test_every_mistake_has_a_test():
    assert set(dc.MISTAKES) == {"last_tie", "no_center_norm", "plus_sign", "sum_all_rows", "count_out_of_range"}


def test_the_cap_is_far_below_the_scores():
    rows, centers = dc.make_case(64, 1324, 33, seed=4)
    ref = dc.Assign(rows, centers)
    assert 0 < float(ref.cap_s.max()) < 1e-9 * float(np.abs(ref.s).max())
    assert float(ref.gap.min()) > 2 * float(ref.cap_s.max())


# ------------------------------------------------------------------------------------------------ 2. the sixth header
def _declared():
    hdr = open(HEADER).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(xgpr_[a-z0-9_]+)\s*\(", hdr)))                # the expression of tests/test_cabi.py


def test_the_header_declares_its_five_entry_points_and_nothing_of_the_other_headers():
    import test_cabi
    import test_input_grad_host
    import test_pool_header_host
    import test_pool_input_grad_host
    import test_seq_input_grad_host
    assert _declared() == NAMES
    assert not set(_declared()) & (set(test_cabi._declared()) | set(test_pool_header_host._declared())
                                   | set(test_input_grad_host._declared()) | set(test_seq_input_grad_host._declared())
                                   | set(test_pool_input_grad_host._declared()))


def test_library_exports_every_declared_name():
    bm = _build_module()
    bm.build_extension()
    lib = ctypes.CDLL(bm.LIB)
    for n in _declared():
        assert hasattr(lib, n), f"{n} declared in include/xgpr_hip_cluster.h but not exported"


def test_ctypes_table_matches_the_header():
    from xgpr_amd import _lib
    assert set(_lib.CLUSTER_SIGNATURES) == set(_declared())
    assert not set(_lib.CLUSTER_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.SIZE_FUNCS) | set(_lib.STRING_FUNCS)
                                               | set(_lib.POOL_SIGNATURES) | set(_lib.INPUT_GRAD_SIGNATURES)
                                               | set(_lib.SEQ_INPUT_GRAD_SIGNATURES) | set(_lib.POOL_INPUT_GRAD_SIGNATURES))
    lib = _lib.load()
    for name, args in _lib.CLUSTER_SIGNATURES.items():                               # load() applied the table
        fn = getattr(lib, name)
        assert fn.argtypes == args
        assert fn.restype is (ctypes.c_size_t if name.endswith("_workspace_bytes") else ctypes.c_int), name
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, args in _lib.CLUSTER_SIGNATURES.items():                               # the tables' lengths are the parameter counts
        decl = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)", hdr)
        assert len(decl.group(2).split(",")) == len(args), name
        assert (decl.group(1) == "size_t") == name.endswith("_workspace_bytes"), name


def test_every_writer_has_a_memory_contract_row():
    import test_gpu_kmeans_memory_contract as table
    writers = {n for n in _declared() if n.endswith("_f32")}                         # (_ok, _workspace_bytes: no device memory)
    assert writers == {"xgpr_kmeans_assign_f32", "xgpr_kmeans_update_f32"}
    covered = table.covered_entry_points()
    assert covered == writers, (sorted(writers - covered), sorted(covered - writers))


def test_source_id_covers_the_header(tmp_path, monkeypatch):
    bm = _build_module()
    assert os.path.samefile(bm.CLUSTER_HDR, HEADER) and bm.CLUSTER_HDR in bm.sources()
    assert any(os.path.basename(p) == "cluster.inc" for p in bm.sources())
    before = bm.source_id()
    copy = tmp_path / "xgpr_hip_cluster.h"
    shutil.copyfile(HEADER, copy)
    monkeypatch.setattr(bm, "CLUSTER_HDR", str(copy))
    assert bm.source_id() == before                                                  # name and contents, not the path
    with open(copy, "a") as f:
        f.write("/* changed */\n")
    assert bm.source_id() != before


# ------------------------------------------------------------------------------------------------ 3. launcher validation
A = 0x100000                     # a dummy 4096-byte-aligned address, never dereferenced on these paths
BIG = 1 << 40
UNSUPPORTED, WORKSPACE, ARRAY_DIMS = -20, -21, -8
DIMS = "incorrect array dims passed"
REFUSED = "k-means serves num_rffs a multiple of 4 and 1 .. 256 centres (see xgpr_kmeans_ok)"
NULL = "NULL array pointer"


def assign(rows=A, centers=A, labels=A, dist2=A, n=100, M=64, k=5, ws=A, wb=BIG):
    from xgpr_amd import _lib
    rc = _lib.load().xgpr_kmeans_assign_f32(rows, centers, labels, dist2, n, M, k, ws, wb, None)
    return int(rc), _lib.last_error()


def update(rows=A, labels=A, sums=A, counts=A, n=100, M=64, k=5, acc=0, ws=A, wb=BIG):
    from xgpr_amd import _lib
    rc = _lib.load().xgpr_kmeans_update_f32(rows, labels, sums, counts, n, M, k, acc, ws, wb, None)
    return int(rc), _lib.last_error()


BOTH = {
    "n < 0": (dict(n=-1), ARRAY_DIMS, DIMS),
    "no columns": (dict(M=0), ARRAY_DIMS, DIMS),
    "no centres": (dict(k=0), ARRAY_DIMS, DIMS),
    "negative k": (dict(k=-3), ARRAY_DIMS, DIMS),
    "num_rffs not a multiple of 4": (dict(M=66), UNSUPPORTED, REFUSED),
    "num_rffs 2": (dict(M=2), UNSUPPORTED, REFUSED),
    "257 centres": (dict(k=257), UNSUPPORTED, REFUSED),
    "NULL rows": (dict(rows=None), WORKSPACE, NULL),
    "NULL labels": (dict(labels=None), WORKSPACE, NULL),
    "misaligned rows": (dict(rows=A + 4), WORKSPACE, None),
    "no workspace": (dict(ws=None), WORKSPACE, None),
    "misaligned workspace": (dict(ws=A + 8), WORKSPACE, None),
    "short workspace": (dict(wb=8), WORKSPACE, None),
    # two failing checks at once: the first in the documented order is the one reported
    "n < 0 and 257 centres": (dict(n=-1, k=257), ARRAY_DIMS, DIMS),
    "257 centres and NULL rows": (dict(k=257, rows=None), UNSUPPORTED, REFUSED),
    "NULL rows and short workspace": (dict(rows=None, wb=8), WORKSPACE, NULL),
}


@pytest.mark.parametrize("name", sorted(BOTH))
def test_validation_outcome(name):
    kw, code, msg = BOTH[name]
    for fn, which in ((assign, "assign"), (update, "update")):
        rc, err = fn(**kw)
        assert rc == code, (which, rc, err)
        if msg is not None:
            assert err == msg
        elif "workspace" in name:
            assert err == f"workspace too small (see xgpr_kmeans_{which}_workspace_bytes)"


def test_the_operators_own_arrays():
    assert assign(centers=None) == (WORKSPACE, NULL)
    assert assign(centers=A + 8)[0] == WORKSPACE
    assert update(sums=None) == (WORKSPACE, NULL) and update(counts=None) == (WORKSPACE, NULL)
    assert update(sums=A + 8)[0] == WORKSPACE
    assert update(sums=None, n=0) == (WORKSPACE, NULL)                    # update writes its zeros for n == 0 too


def test_no_datapoints():
    assert assign(n=0, rows=None, centers=None, labels=None, dist2=None, ws=None, wb=0)[0] == 0      # nothing to do
    assert assign(n=0, k=257)[0] == UNSUPPORTED                                                       # ... but the shape is still checked
    assert update(n=0, acc=1, rows=None, labels=None, ws=None, wb=0)[0] == 0                          # adds nothing: nothing launched
    assert update(n=0, M=66)[0] == UNSUPPORTED


def test_ok_predicate_and_workspace_sizes():
    from xgpr_amd import _lib
    lib = _lib.load()
    ok = lambda m, k: int(lib.xgpr_kmeans_ok(m, k))
    assert [ok(4, 1), ok(64, 256), ok(1324, 33), ok(8192, 7)] == [1, 1, 1, 1]
    assert [ok(2, 1), ok(0, 1), ok(66, 3), ok(64, 0), ok(64, 257), ok(-4, 3)] == [0] * 6
    aw, uw = lib.xgpr_kmeans_assign_workspace_bytes, lib.xgpr_kmeans_update_workspace_bytes
    assert int(aw(0, 64, 5)) == 0 and int(uw(0, 64, 5)) == 0 and int(uw(100, 64, 300)) == 0
    assert int(aw(100, 64, 5)) >= 5 * 8 and int(aw(10 ** 6, 2048, 256)) >= 256 * 8
    for n, m, k in ((1, 4, 1), (257, 36, 17), (3001, 1324, 256), (10 ** 6, 2048, 256)):
        need = int(uw(n, m, k))
        assert need > 0 and need % (k * m * 8) == 0                       # whole [k, num_rffs] float64 slabs, one per row range
        assert need // (k * m * 8) <= max(1, -(-n // 256))                # ... of at least 256 rows
        assert update(n=n, M=m, k=k, wb=need - 1)[0] == WORKSPACE         # the bound the launcher checks is the advertised size
    need = int(aw(257, 36, 17))
    assert assign(n=257, M=36, k=17, wb=need - 1)[0] == WORKSPACE


def test_python_wrappers_refuse_what_the_predicate_refuses():
    from xgpr_amd import xgpr_hip_rfgen_ext as ext
    assert ext.kmeans_ok(64, 5) == 1 and ext.kmeans_ok(66, 5) == 0 and ext.kmeans_ok(64, 257) == 0
    assert callable(ext.hipKMeansAssign) and callable(ext.hipKMeansUpdate)


# ------------------------------------------------------------------------------------------------ 4. the Lloyd loop
def blobs(n=600, d=5, seed=0, sep=6.0):
    rng = np.random.default_rng(seed)
    means = sep * rng.standard_normal((3, d))
    truth = rng.integers(0, 3, size=n)
    return means[truth] + rng.standard_normal((n, d)), truth, means


def test_lloyd_converges_on_three_blobs():
    x, truth, means = blobs()
    init = x[[np.argmax(truth == k) for k in range(3)]]                   # one point of each blob
    labels, centers, history, n_iter, counts = dc.lloyd(x, init)
    assert (labels == truth).all() and 1 <= n_iter < 20
    assert np.abs(centers - np.stack([x[truth == k].mean(axis=0) for k in range(3)])).max() < 1e-12
    assert all(b <= a * (1 + 1e-12) for a, b in zip(history, history[1:]))
    assert (counts == np.bincount(truth, minlength=3)).all()
    # the same loop over the long-double operators of the helper
    z32 = x.astype(np.float32)

    def assign(c):
        ref = dc.Assign(z32, c)
        return ref.labels, ref.dist2.astype(np.float64)

    def update(lab):
        up = dc.Update(z32, lab, 3)
        return up.sums.astype(np.float64), up.counts

    l2, c2, h2, it2, n2 = dc.lloyd(z32.astype(np.float64), init, assign=assign, update=update)
    assert (l2 == truth).all() and it2 == n_iter and np.abs(c2 - centers).max() < 1e-5


def test_lloyd_keeps_the_centre_of_an_empty_cluster():
    x, truth, _ = blobs(n=200)
    far = np.full((1, x.shape[1]), 1e3)
    init = np.concatenate([x[[np.argmax(truth == k) for k in range(3)]], far])
    labels, centers, _, _, counts = dc.lloyd(x, init)
    assert counts[3] == 0 and (centers[3] == far[0]).all() and (labels < 3).all()
