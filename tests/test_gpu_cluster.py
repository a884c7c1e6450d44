"""xgpr_amd.cluster on the device: KernelKMeans against the numpy Lloyd loop of tests/dense_cluster.py run on ``KernelFGen.predict``
features (the loop tests/test_cluster_host.py checks on its own), and KernelPCA against numpy's eigendecomposition of the same
float64 features."""
import numpy as np
import pytest
import torch

import dense_cluster as dc
from test_cluster_host import blobs

pytestmark = pytest.mark.gpu
DEV = "cuda"
HP = np.asarray([-1.5])              # log sigma: blobs 6 apart and of unit spread are far apart, their own points close, in kernel terms
M, K, D = 64, 3, 5


@pytest.fixture(scope="module")
def cluster():
    from xgpr_amd import cluster as c
    return c


def fgen(num_rffs=M, hp=HP, d=D, kernel="RBF", settings=None):
    from xgpr_amd.models import KernelFGen
    return KernelFGen(num_rffs, hp, d, kernel_choice=kernel, device=DEV, kernel_settings=settings, verbose=False)


@pytest.fixture(scope="module")
def case():
    """The three blobs, their float64 features, one point of each blob as the initial centres, and numpy's Lloyd result."""
    x, truth, _ = blobs(n=600, d=D, seed=0)
    feats = fgen().predict(x)
    init = feats[[int(np.argmax(truth == k)) for k in range(K)]].copy()
    want = dc.lloyd(feats, init)
    assert (want[0] == truth).all()                                       # (the target itself finds the blobs)
    return x, truth, feats, init, want


def kmeans(cluster, init, n_clusters=K, **kw):
    return cluster.KernelKMeans(n_clusters, kw.pop("num_rffs", M), kw.pop("hp", HP), kw.pop("d", D), device=DEV, init=init, verbose=False,
                                **kw)


def test_kmeans_equals_the_numpy_lloyd_loop(cluster, case):
    x, truth, feats, init, (labels, centers, history, n_iter, counts) = case
    km = kmeans(cluster, init).fit(x)
    assert km.labels_.dtype == np.int32 and (km.labels_ == labels).all() and km.n_iter_ == n_iter
    assert km.cluster_centers_.dtype == np.float64 and km.cluster_centers_.shape == (K, M)
    assert np.abs(km.cluster_centers_ - centers).max() < 1e-9
    assert (km.counts_ == counts).all() and km.counts_.dtype == np.int64
    assert len(km.inertia_history_) == len(history) and km.inertia_ == km.inertia_history_[-1]
    assert np.allclose(km.inertia_history_, history, rtol=1e-9, atol=0)
    # non-increasing: each inertia is a sum of n squared distances, each within gamma_{M+3} (|z|^2 + |c|^2 + 2 |z||c|) <= 4 gamma_{M+3}
    # max(|z|^2, |c|^2) of the exact one, and |z|^2 = 1 for these features (cos^2 + sin^2 over the frequencies), |c|^2 <= 1
    cap = 600 * 4 * float(dc.gamma(M + 3))
    assert all(b <= a + 2 * cap for a, b in zip(km.inertia_history_, km.inertia_history_[1:]))
    assert (km.fit_predict(x) == labels).all()


def test_predict_is_the_argmin_over_dense_features(cluster, case):
    x, truth, feats, init, want = case
    km = kmeans(cluster, init).fit(x)
    xnew = blobs(n=300, d=D, seed=0)[2][np.random.default_rng(5).integers(0, 3, size=300)] + np.random.default_rng(6).standard_normal((300, D))
    fnew = fgen().predict(xnew)
    c = km.cluster_centers_
    s = (c * c).sum(axis=1)[None, :] - 2 * fnew @ c.T
    part = np.partition(s, 1, axis=1)
    assert ((part[:, 1] - part[:, 0]) > 1e-9).all()                       # (decided rows only: asserted for these inputs)
    got = km.predict(xnew, chunk_size=128)
    assert got.dtype == np.int32 and (got == np.argmin(s, axis=1)).all()
    assert (km.predict(x) == km.labels_).all()


def test_kmeans_plus_plus_is_reproducible(cluster, case):
    x, truth = case[0], case[1]
    a = kmeans(cluster, "k-means++", random_seed=7).fit(x)
    b = kmeans(cluster, "k-means++", random_seed=7).fit(x)
    assert a.cluster_centers_.tobytes() == b.cluster_centers_.tobytes() and (a.labels_ == b.labels_).all()
    # separated blobs: distance-proportional seeding lands one centre in each
    assert sorted(np.bincount(a.labels_, minlength=K).tolist()) == sorted(np.bincount(truth, minlength=K).tolist())


def test_cached_rows_against_regenerated_windows(cluster, monkeypatch):
    x, truth, _ = blobs(n=2500, d=D, seed=1)
    feats = fgen().predict(x)
    init = feats[[int(np.argmax(truth == k)) for k in range(K)]].copy()
    cached = kmeans(cluster, init).fit(x, cache_rows=True)
    monkeypatch.setattr(cluster, "WINDOW_BYTES", 1)                       # windows of 1024 rows: three of them
    windows = []
    real = cluster.RowSource.windows

    def counting(self):
        for w in real(self):
            windows.append(w[:2])
            yield w
    monkeypatch.setattr(cluster.RowSource, "windows", counting)
    regen = kmeans(cluster, init).fit(x, cache_rows=False)
    assert windows[:3] == [(0, 1024), (1024, 2048), (2048, 2500)]
    assert (regen.labels_ == cached.labels_).all() and regen.n_iter_ == cached.n_iter_
    assert np.abs(regen.cluster_centers_ - cached.cluster_centers_).max() <= 1e-12 * np.abs(cached.cluster_centers_).max()
    auto = kmeans(cluster, init).fit(x)                                   # "auto": 2500 x 64 floats fit the budget, one window
    assert auto.cluster_centers_.tobytes() == cached.cluster_centers_.tobytes()


def test_conv_kernel_from_tokens_and_from_the_dense_array(cluster):
    n, L, C, cw, m = 40, 12, 21, 9, 128
    rng = np.random.default_rng(8)
    motif = rng.integers(0, C, size=(2, L))
    truth = rng.integers(0, 2, size=n)
    tokens = motif[truth].copy()
    flip = rng.random((n, L)) < 0.1
    tokens[flip] = rng.integers(0, C, size=int(flip.sum()))
    tokens = tokens.astype(np.uint8)
    table = np.eye(C, dtype=np.float32)
    lens = rng.integers(cw, L + 1, size=n).astype(np.int32)
    settings = {"conv_width": cw, "intercept": True, "matern_nu": 5 / 2, "averaging": "none"}
    feats = fgen(m, np.asarray([0.0]), C, "Conv1dRBF", settings).predict(table[tokens], lens)
    init = feats[[int(np.argmax(truth == k)) for k in range(2)]].copy()
    kw = dict(n_clusters=2, num_rffs=m, hp=np.asarray([0.0]), d=C, kernel_choice="Conv1dRBF", kernel_settings=settings)
    dense = kmeans(cluster, init, **dict(kw)).fit(table[tokens], lens)
    tok = kmeans(cluster, init, **dict(kw)).fit(tokens, lens, token_table=table)
    assert (dense.labels_ == tok.labels_).all() and dense.cluster_centers_.tobytes() == tok.cluster_centers_.tobytes()
    want = dc.lloyd(feats, init)
    assert (dense.labels_ == want[0]).all() and np.abs(dense.cluster_centers_ - want[1]).max() < 1e-6      # (float32 rows of float64 sums)
    assert (tok.predict(tokens, lens, token_table=table) == tok.labels_).all()


def test_a_kernel_without_float32_rows(cluster, case):
    x, truth = case[0], case[1]
    settings = {"split_points": [2], "intercept": True}
    hp = np.asarray([-1.5, -1.5])
    feats = fgen(M, hp, D, "MiniARD", settings).predict(x)
    init = feats[[int(np.argmax(truth == k)) for k in range(K)]].copy()
    km = kmeans(cluster, init, hp=hp, kernel_choice="MiniARD", kernel_settings=settings).fit(x)
    want = dc.lloyd(feats, init)
    assert (km.labels_ == want[0]).all() and (km.labels_ == truth).all()
    assert np.abs(km.cluster_centers_ - want[1]).max() < 1e-6             # the rows are the float64 features rounded to float32


def test_an_empty_cluster_keeps_its_centre(cluster, case):
    x, truth, feats, init, want = case
    far = np.full((1, M), 10.0)
    km = kmeans(cluster, np.concatenate([init, far]), n_clusters=4).fit(x)
    assert km.counts_[3] == 0 and (km.labels_ == want[0]).all()
    assert np.allclose(km.cluster_centers_[3], far[0], rtol=1e-14, atol=0)
    assert np.abs(km.cluster_centers_[:3] - want[1]).max() < 1e-9


def test_refusals(cluster, case):
    with pytest.raises(RuntimeError, match="multiple of 4"):
        kmeans(cluster, "k-means++", num_rffs=66)
    with pytest.raises(RuntimeError, match="n_clusters = 257"):
        kmeans(cluster, "k-means++", n_clusters=257)
    with pytest.raises(RuntimeError, match="init must be"):
        kmeans(cluster, np.zeros((2, M))).fit(case[0])
    with pytest.raises(RuntimeError, match="multiple of 128"):
        cluster.KernelPCA(4, 64, HP, D, device=DEV, verbose=False)
    with pytest.raises(RuntimeError, match="components"):
        cluster.KernelPCA(33, 128, HP, D, device=DEV, verbose=False)


def test_kernel_pca_against_numpy(cluster):
    n, m, nc = 500, 128, 4
    rng = np.random.default_rng(9)
    x = rng.standard_normal((n, D)) * np.asarray([3.0, 2.0, 1.3, 0.8, 0.5])
    hp = np.asarray([-2.0])
    feats = fgen(m, hp).predict(x)
    mu = feats.mean(axis=0)
    cov = feats.T @ feats / n - np.outer(mu, mu)
    evals, evecs = np.linalg.eigh(cov)
    evals, evecs = evals[::-1], evecs[:, ::-1]
    print("kernel PCA reference eigenvalues:", evals[:nc + 1])
    assert (evals[:nc] - evals[1:nc + 1] > 1e-3 * evals[0]).all()         # a property of the inputs: the leading components are separated
    pca = cluster.KernelPCA(nc, m, hp, D, device=DEV, verbose=False).fit(x)
    assert np.abs(pca.explained_variance_ - evals[:nc]).max() <= 1e-8 * evals[0]
    assert np.abs(pca.mean_ - mu).max() < 1e-9
    big = np.abs(pca.components_).argmax(axis=1)
    assert (pca.components_[np.arange(nc), big] > 0).all()
    assert np.abs(pca.components_ @ pca.components_.T - np.eye(nc)).max() < 1e-12
    t = pca.transform(x, chunk_size=200)
    tref = (feats - mu) @ evecs[:, :nc]
    assert t.shape == (n, nc)
    assert np.abs(t @ t.T - tref @ tref.T).max() <= 1e-8 * np.abs(tref @ tref.T).max()
    assert np.abs(pca.fit_transform(x) - t).max() <= 1e-12 * np.abs(t).max()       # (another chunking: another split of the contraction)
