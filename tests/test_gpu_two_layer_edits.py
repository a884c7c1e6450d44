"""xGPRegression.predict_single_edits at the model level: for a fitted Conv1dTwoLayer model, the predicted mean and variance of
EVERY single substitution, deletion and insertion against ``predict`` of the written-out mutant (written out here, with numpy).

The cap is derived, not tuned.  The mutants' pooled rows are those of the written-out route (tests/test_gpu_pool_edits.py), so what
is left between the two routes is the order of two float64 sums: a sum of n terms carries at most (n - 1) eps sum |terms| whatever
its order, and twice (n + 2) eps covers two orders, the products and the few operations around them.
    mean        2 (M + 2) 2^-53 std sum_k |z_k w_k|                          for each of the two means involved (mutant, sequence)
    variance    2 (nvar^2 + nvar + 2) 2^-53 lambda^2 std^2 sum_kl |z_k| |var_kl| |z_l|
both evaluated from the mutant's (and the sequence's) own features.  Every comparison prints one line with the measured error,
the cap and their ratio; no element is excused, and the cap is asserted to lie below 1e-6 of the case's largest output."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
NTRAIN, L, V, CW, M, NVAR, INIT = 60, 24, 8, 3, 128, 32, 64
NAMES = ("substitutions", "deletions", "insertions")
EPS = 2.0 ** -53


@functools.lru_cache(maxsize=None)
def _data():
    rng = np.random.default_rng(31)
    tokens = rng.integers(0, V, size=(NTRAIN, L)).astype(np.int64)
    sl = rng.integers(CW, L + 1, size=NTRAIN).astype(np.int32)
    table = np.eye(V, dtype=np.float32)
    y = np.sin(0.7 * tokens[:, :4].sum(axis=1)) + 0.1 * rng.standard_normal(NTRAIN)
    scan = rng.integers(0, V, size=(3, L)).astype(np.int64)
    scan_sl = np.asarray([CW, L, 11], dtype=np.int32)
    return tokens, table, sl, y, scan, scan_sl


@functools.lru_cache(maxsize=None)
def _model(kernel_choice="Conv1dTwoLayer"):
    from xgpr_amd.dataset import build_regression_dataset
    from xgpr_amd.models import xGPRegression
    tokens, table, sl, y, _, _ = _data()
    ds = build_regression_dataset(tokens, y, sl, chunk_size=256, device=DEV, token_table=table)
    settings = {"conv_width": CW, "intercept": True, "averaging": "none"}
    if kernel_choice == "Conv1dTwoLayer":
        settings["init_rffs"] = INIT
    model = xGPRegression(num_rffs=M, variance_rffs=NVAR, kernel_choice=kernel_choice, device=DEV, kernel_settings=settings, verbose=False)
    model.set_hyperparams(np.log(np.array([0.5, 0.6])), ds)
    model.fit(ds, mode="exact")
    return model


@functools.lru_cache(maxsize=None)
def _edits():
    _, table, _, _, scan, scan_sl = _data()
    return _model().predict_single_edits(scan, scan_sl, token_table=table, get_var=True)


def _mutants(name):
    """-> (token rows [n, slots, values, L + 1], lengths [n, slots, values], valid [n, slots]): every mutant written out."""
    _, _, _, _, scan, scan_sl = _data()
    n = scan.shape[0]
    slots, per = (L + 1 if name == "insertions" else L), (1 if name == "deletions" else V)
    rows = np.zeros((n, slots, per, L + 1), dtype=np.int64)
    lens = np.full((n, slots, per), CW, dtype=np.int32)
    valid = np.zeros((n, slots), dtype=bool)
    for i in range(n):
        s = int(scan_sl[i])
        seq = scan[i, :s]
        for site in range(slots):
            inside = site <= s if name == "insertions" else site < s
            valid[i, site] = inside and not (name == "deletions" and s == CW)
            for v in range(per):
                if not valid[i, site]:
                    mut = seq
                elif name == "substitutions":
                    mut = seq.copy()
                    mut[site] = v
                elif name == "deletions":
                    mut = np.delete(seq, site)
                else:
                    mut = np.insert(seq, site, v)
                rows[i, site, v, :len(mut)] = mut
                lens[i, site, v] = len(mut)
    return rows, lens, valid


@pytest.mark.parametrize("name", NAMES)
def test_every_single_edit_against_predict_of_the_written_out_mutant(name):
    from xgpr_amd.dataset import token_batch
    model = _model()
    _, table, _, _, scan, scan_sl = _data()
    edits = _edits()
    rows, lens, valid = _mutants(name)
    shape = lens.shape
    flat_rows, flat_lens = rows.reshape(-1, L + 1), lens.reshape(-1)
    want_mean, want_var = model.predict(flat_rows, flat_lens, get_var=True, token_table=table)
    base = model.predict(scan, scan_sl, token_table=table)
    got_mean = (base[:, None, None] + edits[name].reshape(shape)).reshape(-1)
    got_var = edits[name + "_var"].reshape(-1)
    # the caps, from the mutants' own features
    w, var = model.weights, model.var
    lam, std = float(model.kernel.get_lambda()), float(model.trainy_std)
    z = model.kernel.transform_x(token_batch(torch.from_numpy(flat_rows), table).to(DEV), flat_lens)
    z0 = model.kernel.transform_x(token_batch(torch.from_numpy(scan), table).to(DEV), scan_sl)
    s_mut = (z * w[None, :]).abs().sum(dim=1).cpu().numpy()
    s_own = np.repeat((z0 * w[None, :]).abs().sum(dim=1).cpu().numpy(), shape[1] * shape[2])
    cap_mean = 2 * (M + 2) * EPS * std * (s_mut + s_own)
    zv = z[:, :NVAR].abs()
    cap_var = 2 * (NVAR * NVAR + NVAR + 2) * EPS * lam ** 2 * std ** 2 * ((zv @ var.abs()) * zv).sum(dim=1).cpu().numpy()
    keep = np.repeat(valid.reshape(-1), shape[2])
    assert keep.sum() > 0.5 * keep.size / 3
    for what, got, want, cap in (("mean", got_mean, want_mean, cap_mean), ("variance", got_var, want_var, cap_var)):
        err = np.abs(got - want)[keep]
        c = cap[keep]
        worst = int(np.argmax(err / c))
        print(f"TWO_LAYER_EDITS {name} {what}: {int(keep.sum())} mutants, largest error {err.max():.3e}, cap there {c[worst]:.3e}, "
              f"largest error / cap {float((err / c).max()):.3e}")
        assert np.isfinite(got[keep]).all() and np.isfinite(want[keep]).all()
        assert (err <= c).all(), (what, float((err / c).max()))                      # no element is excused
        assert c.max() < 1e-6 * np.abs(want[keep]).max()                             # the cap separates something
    # the scan is not trivially flat: edits move the mean by far more than the cap
    assert np.abs(edits[name].reshape(-1)[keep]).max() > 1e6 * cap_mean[keep].max()


def test_zeros_and_nans_of_the_contract():
    _, _, _, _, scan, scan_sl = _data()
    edits = _edits()
    assert edits["substitutions"].shape == (3, L, V) and edits["deletions"].shape == (3, L) and edits["insertions"].shape == (3, L + 1, V)
    for i in range(3):
        s = int(scan_sl[i])
        assert (edits["substitutions"][i, np.arange(s), scan[i, :s]] == 0).all()                # the own token, by definition
        for name, first in (("substitutions", s), ("deletions", s), ("insertions", s + 1)):
            assert (edits[name][i, first:] == 0).all() and (edits[name + "_var"][i, first:] == 0).all()
    assert np.isnan(edits["deletions"][0, :CW]).all() and np.isnan(edits["deletions_var"][0, :CW]).all()     # a sequence of one window
    assert not np.isnan(edits["deletions"][1:]).any() and not np.isnan(edits["substitutions"]).any() and not np.isnan(edits["insertions"]).any()
    other = edits["substitutions"][1].copy()
    other[np.arange(L), scan[1]] = 1.0
    assert (other != 0).all()                                                        # every other substitution moves the mean
    assert (edits["substitutions_var"][1] > 0).all() and (edits["insertions_var"][1] > 0).all()


def test_a_token_batch_gives_the_same_arrays_and_get_var_is_optional():
    from xgpr_amd.dataset import token_batch
    model = _model()
    _, table, _, _, scan, scan_sl = _data()
    edits = _edits()
    # (the same chunks: the quadratic form is a matrix product, whose summation order may follow the number of rows it is given)
    again = model.predict_single_edits(token_batch(torch.from_numpy(scan), table), scan_sl, get_var=True)
    assert set(again) == set(edits) == set(NAMES) | {n + "_var" for n in NAMES}
    for k in edits:
        assert np.array_equal(again[k], edits[k], equal_nan=True), k
    means = model.predict_single_edits(scan, scan_sl, token_table=table)
    assert set(means) == set(NAMES)
    for k in NAMES:
        assert np.array_equal(means[k], edits[k], equal_nan=True), k


def test_the_composed_rows_give_the_same_scan():
    """Both row sources feed one function with the same slab boundaries: the same bits."""
    from xgpr_amd.dataset import token_batch
    model = _model()
    _, table, _, _, scan, scan_sl = _data()
    batch = token_batch(torch.from_numpy(scan), table).to(DEV)
    for name in NAMES:
        a = model.kernel.edit_scan(batch, scan_sl, model.weights, name, var=model.var)
        b = model.kernel.edit_scan(batch, scan_sl, model.weights, name, var=model.var, composed=True)
        for x, y in zip(a, b):
            assert torch.equal(torch.nan_to_num(x, nan=7.0), torch.nan_to_num(y, nan=7.0)), name


def test_sequence_kernels_return_their_own_scans():
    model = _model("Conv1dRBF")
    _, table, _, _, scan, scan_sl = _data()
    edits = model.predict_single_edits(scan, scan_sl, token_table=table, get_var=True)
    sub, sub_var = model.predict_substitutions(scan, scan_sl, token_table=table, get_var=True)
    dele, ins, dele_var, ins_var = model.predict_indels(scan, scan_sl, token_table=table, get_var=True)
    for k, want in (("substitutions", sub), ("deletions", dele), ("insertions", ins), ("substitutions_var", sub_var),
                    ("deletions_var", dele_var), ("insertions_var", ins_var)):
        assert np.array_equal(edits[k], want, equal_nan=True), k
    means = model.predict_single_edits(scan, scan_sl, token_table=table)
    assert set(means) == set(NAMES) and np.array_equal(means["insertions"], ins)


def test_refusals():
    from xgpr_amd.dataset import build_regression_dataset
    from xgpr_amd.models import xGPRegression
    model = _model()
    tokens, table, sl, y, scan, scan_sl = _data()
    with pytest.raises(RuntimeError, match="sequence_lengths is required"):
        model.predict_single_edits(scan, token_table=table)
    with pytest.raises(RuntimeError, match="needs token input"):
        model.predict_single_edits(table[scan], scan_sl)
    with pytest.raises(RuntimeError, match="shape\\[0\\] of sequence_lengths"):
        model.predict_single_edits(scan, scan_sl[:2], token_table=table)
    fresh = xGPRegression(num_rffs=M, variance_rffs=NVAR, kernel_choice="Conv1dTwoLayer", device=DEV,
                          kernel_settings={"conv_width": CW, "init_rffs": INIT}, verbose=False)
    with pytest.raises(RuntimeError, match="not yet been successfully fitted"):
        fresh.predict_single_edits(scan, scan_sl, token_table=table)
    rng = np.random.default_rng(3)
    x = rng.standard_normal((40, 6)).astype(np.float32)
    ds = build_regression_dataset(x, x[:, 0], chunk_size=64, device=DEV)
    rbf = xGPRegression(num_rffs=64, variance_rffs=16, kernel_choice="RBF", device=DEV, verbose=False)
    rbf.set_hyperparams(np.log(np.array([0.5, 0.6])), ds)
    rbf.fit(ds, mode="exact")
    with pytest.raises(RuntimeError, match="predict_single_edits is available for .* Conv1dTwoLayer .*'RBF'"):
        rbf.predict_single_edits(scan, scan_sl, token_table=table)
    # the three existing scans still refuse the two-layer kernel, in their own words
    for call in (model.predict_substitutions, model.predict_indels, model.predict_substitution_pairs):
        with pytest.raises(RuntimeError, match="Conv1dTwoLayer, the fixed-vector kernels, Linear and MiniARD are not supported"):
            call(scan, scan_sl, token_table=table)
