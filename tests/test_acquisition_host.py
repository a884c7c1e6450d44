"""xgpr_amd/acquisition.py on CPU tensors (no GPU, no library: the module imports torch alone): the joint posterior over a
single-edit neighbourhood -- covariances, draws and the greedy GP-BUCB batch -- against brute-force Gaussian conditioning on the
dense E x E covariance in numpy float64."""
import importlib.util
import os

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _load():
    # by path: importing the package needs the built library and a HIP runtime, this module needs neither
    spec = importlib.util.spec_from_file_location("xgpr_acquisition", os.path.join(ROOT, "xgpr_amd", "acquisition.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


acq = _load()
L, V, K = 6, 5, 9                       # E = 30 + 6 + 35 = 71
E = L * V + L + (L + 1) * V


def make(seed=0, length=5, noise=0.3, lowrank=False):
    rng = np.random.default_rng(seed)
    factor = rng.normal(size=(E, K)) * rng.uniform(0.2, 1.5, size=(E, 1))
    if lowrank:
        factor[:, 3:] = 0                                    # near-duplicates: many edits share three directions
    mean = rng.normal(size=E)
    own = rng.integers(0, V, size=L)
    pos = np.arange(L + 1)
    sub = (pos[:L, None] < length) & (np.arange(V)[None, :] != own[:, None])
    dele = pos[:L] < length
    ins = np.broadcast_to(pos[:, None] <= length, (L + 1, V))
    valid = np.concatenate([sub.reshape(-1), dele, ins.reshape(-1)])
    return acq.SingleEditPosterior(torch.from_numpy(mean), torch.from_numpy(factor), noise, torch.from_numpy(valid), L, V), valid


def test_order_and_unravel():
    nb, _ = make()
    assert len(nb) == E
    assert nb.unravel(0) == ("substitution", 0, 0)
    assert nb.unravel(L * V - 1) == ("substitution", L - 1, V - 1)
    assert nb.unravel(L * V) == ("deletion", 0, None)
    assert nb.unravel(L * V + L - 1) == ("deletion", L - 1, None)
    assert nb.unravel(L * V + L) == ("insertion", 0, 0)
    assert nb.unravel(E - 1) == ("insertion", L, V - 1)
    seen = {nb.unravel(i) for i in range(E)}
    assert len(seen) == E
    with pytest.raises(IndexError):
        nb.unravel(E)
    with pytest.raises(RuntimeError):
        acq.SingleEditPosterior(nb.mean[:-1], nb.factor, 0.1, nb.valid, L, V)


def test_covariance_and_variance_are_factor_factor_t():
    nb, _ = make(1)
    f = nb.factor.numpy()
    dense = f @ f.T
    np.testing.assert_allclose(nb.variance().numpy(), np.diag(dense), rtol=1e-13, atol=0)
    a, b = torch.tensor([0, 7, 33, 70]), torch.tensor([2, 33, 50])
    np.testing.assert_allclose(nb.covariance(a, b).numpy(), dense[np.ix_(a.numpy(), b.numpy())], rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(nb.covariance(a).numpy(), dense[np.ix_(a.numpy(), a.numpy())], rtol=1e-13, atol=1e-15)


def test_sample_is_reproducible_and_is_mean_plus_factor_eps():
    nb, _ = make(2)
    one, two, other = nb.sample(7, random_seed=5), nb.sample(7, random_seed=5), nb.sample(7, random_seed=6)
    assert one.shape == (E, 7)
    assert torch.equal(one, two) and not torch.equal(one, other)
    eps = acq.standard_normal(K, 7, 5)
    np.testing.assert_allclose(one.numpy(), nb.mean.numpy()[:, None] + nb.factor.numpy() @ eps.numpy(), rtol=1e-13, atol=1e-14)
    # one epsilon per draw for every edit: the draws' deviations lie in the factor's column space
    dev = (one - nb.mean[:, None]).numpy()
    coef = np.linalg.lstsq(nb.factor.numpy(), dev, rcond=None)[0]
    np.testing.assert_allclose(coef, eps.numpy(), rtol=1e-9, atol=1e-10)


def brute_force(mean, factor, noise, valid, batch, beta, maximize):
    """Greedy BUCB by conditioning the dense covariance, one noisy observation per pick -> [(index or None where the margin
    over the runner-up is within 1e-9 of the score range, sd vector at pick time, chosen index)]."""
    cov = factor @ factor.T
    free = valid.copy()
    out = []
    for _ in range(batch):
        sd = np.sqrt(np.maximum(np.diag(cov), 0) + noise)
        score = (mean if maximize else -mean) + beta * sd
        score = np.where(free, score, -np.inf)
        order = np.argsort(-score)
        j = int(order[0])
        spread = score[free].max() - score[free].min()
        clear = free.sum() < 2 or score[order[0]] - score[order[1]] > 1e-9 * spread
        out.append((j, clear, sd.copy(), np.diag(cov).copy()))
        free[j] = False
        c = cov[:, j].copy()
        cov = cov - np.outer(c, c) / (cov[j, j] + noise)
    return out


@pytest.mark.parametrize("seed,beta,maximize,lowrank", [(3, 2.0, True, False), (4, 2.0, False, False), (5, 0.7, True, True),
                                                        (6, 5.0, True, True)])
def test_select_batch_against_dense_conditioning(seed, beta, maximize, lowrank):
    nb, valid = make(seed, lowrank=lowrank)
    batch = 12
    picks = nb.select_batch(batch, beta=beta, maximize=maximize)
    ref = brute_force(nb.mean.numpy(), nb.factor.numpy(), nb.noise, valid, batch, beta, maximize)
    assert len(picks) == batch
    assert len({p["index"] for p in picks}) == batch
    for p, (j, clear, sd, _) in zip(picks, ref):
        assert valid[p["index"]], "an invalid row was picked"
        assert (p["kind"], p["position"], p["token"]) == nb.unravel(p["index"])
        if not clear:
            break                                            # a tie: the two routes may part ways from here on
        assert p["index"] == j
        assert p["mean"] == float(nb.mean[j])
        assert abs(p["sd"] - sd[j]) <= 1e-10 * sd[j]


def test_a_pick_drops_its_own_latent_variance_by_noise_over_noise_plus_v():
    nb, valid = make(7)
    first = nb.select_batch(1)[0]
    two = nb.select_batch(2)
    assert two[0] == first
    # the conditional latent variance of every row after the first pick, through a third pick's sd is not visible: recompute
    f = nb.factor.numpy()
    j = first["index"]
    v = float(f[j] @ f[j])
    ref = brute_force(nb.mean.numpy(), f, nb.noise, valid, 2, 2.0, True)
    after = ref[1][3]
    np.testing.assert_allclose(after[j], v * nb.noise / (nb.noise + v), rtol=1e-12)
    # and the class's own sd of the second pick is the conditional one
    k = two[1]["index"]
    np.testing.assert_allclose(two[1]["sd"] ** 2 - nb.noise, after[k], rtol=1e-10, atol=1e-14)
    # the picked row itself, seen through a run that may pick it again: beta large, a single valid row besides
    only = torch.zeros(E, dtype=torch.bool)
    only[j] = True
    solo = acq.SingleEditPosterior(nb.mean, nb.factor, nb.noise, only, L, V)
    assert [p["index"] for p in solo.select_batch(3)] == [j]          # never taken twice; the batch is shorter


def test_conditioned_sds_of_every_row_match_dense_conditioning():
    nb, valid = make(8, lowrank=True)
    f, noise = nb.factor.numpy(), nb.noise
    picks = nb.select_batch(6, beta=3.0)
    cov = f @ f.T
    for p in picks:
        j = p["index"]
        sd = np.sqrt(max(cov[j, j], 0) + noise)
        assert abs(p["sd"] - sd) <= 1e-10 * sd
        c = cov[:, j].copy()
        cov = cov - np.outer(c, c) / (cov[j, j] + noise)


def test_beta_zero_is_a_plain_top_b_of_the_means():
    for maximize in (True, False):
        nb, valid = make(9)
        picks = nb.select_batch(10, beta=0.0, maximize=maximize)
        m = nb.mean.numpy()
        order = [i for i in np.argsort(-m if maximize else m) if valid[i]][:10]
        assert [p["index"] for p in picks] == order


def test_invalid_rows_with_nan_never_enter():
    nb, valid = make(10)
    mean, factor = nb.mean.clone(), nb.factor.clone()
    bad = np.flatnonzero(~valid)
    mean[bad[0]] = float("nan")
    factor[bad[1]] = float("nan")
    nan_nb = acq.SingleEditPosterior(mean, factor, nb.noise, nb.valid, L, V)
    assert [p["index"] for p in nan_nb.select_batch(8)] == [p["index"] for p in nb.select_batch(8)]
    assert all(np.isfinite(p["sd"]) and np.isfinite(p["mean"]) for p in nan_nb.select_batch(8))
