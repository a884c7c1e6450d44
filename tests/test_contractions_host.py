"""tests/dense_contractions.py on the host: the exact leg's float64 reference against an int64 evaluation, the longdouble
reference against numpy float64 under the derived caps, every planted mistake against the committed shape tables, and the
arm coverage of those tables for a 256-CU part.  No GPU."""
import functools

import numpy as np
import pytest

import dense_contractions as dc

INT64_MACS = 2e7                  # the int64 product (no BLAS) is evaluated on a strided subset of the output columns beyond this


def _int64_equal(a, b, ref):
    """ref == a^T b evaluated in int64 over the operands' quanta (a [K, I], b [K, J]); on a column subset when large."""
    qa, qb = dc._quantum(a), dc._quantum(b)
    step = max(1, int(np.ceil(a.shape[0] * a.shape[1] * b.shape[1] / INT64_MACS)))
    cols = np.arange(0, b.shape[1], step)
    got = dc.as_int64(a, qa).T @ dc.as_int64(b[:, cols], qb)
    assert np.abs(got).max(initial=0) < 2 ** 53
    return np.array_equal(got.astype(np.float64) * (qa * qb), ref[:, cols])


def _block_sample():
    """Every fifth case of the three tables (the stride is coprime to the tables' periods: every k, n, M and both intercept
    settings occur), the long-range shapes and the by-size shape."""
    cases = [c for rt in (1, 2, 4) for c in dc.block_cases(rt)[::5]]
    return cases + [c for c in dc.block_cases(1) if c.n >= 40000 and c not in cases]


@pytest.mark.parametrize("mode", ["matvec", "project", "backproject"])
def test_exact_block_reference_equals_int64(mode):
    for case in _block_sample():
        zc, op, scale, _ = dc.make_block(case, mode, True)              # (asserts the bit budget)
        z = dc.features(zc, scale, case.icpt)
        ref = dc.ref_block(mode, zc, op, case, scale)
        if mode == "project":
            assert _int64_equal(z.T, op, ref), case
        elif mode == "backproject":
            assert _int64_equal(z, op, ref), case
        else:
            t = z @ op
            assert _int64_equal(z.T, op, t) and _int64_equal(z, t, ref), case


def test_exact_sketch_gram_and_cross_references_equal_int64():
    for case in dc.SKETCH_CASES:
        zc, a, scale = dc.make_sketch(case, True)
        z = dc.features(zc, scale, case.icpt)
        ref = dc.ref_sketch(a, zc, case, False, scale)
        j = case.n if case.bt else case.m
        assert _int64_equal(a[:, :case.r], z.T if case.bt else z, ref[:, :j]), case
        assert np.all(ref[:, j:] == dc.SENTINEL)
        assert np.array_equal(dc.ref_sketch(a, zc, case, True, scale)[:, :case.r], ref[:, :j].T), case
    for case in dc.GRAM_CASES:
        zc, scale = dc.make_gram(case, True)
        z = dc.features(zc, scale, case.icpt)[:, :case.msub]
        assert _int64_equal(z, z, dc.ref_gram(zc, case, scale)[:, :case.msub]), case
    for case in dc.CROSS_CASES:
        a, b = dc.make_cross(case, True)
        a64, b64 = a.astype(np.float64), b.astype(np.float64)
        ref = dc.ref_cross(a, b, case)[:, :case.M]
        step = max(1, int(np.ceil(case.n * case.M * case.M / INT64_MACS)))
        cols = np.arange(0, case.M, step)
        ai, bi = dc.as_int64(a64, 2.0 ** -11), dc.as_int64(b64, 2.0 ** -11)
        got = ai.T @ bi[:, cols] + bi.T @ ai[:, cols]
        assert np.array_equal(got.astype(np.float64) * 2.0 ** -22, ref[:, cols]), case


def test_budget_refuses_a_shape_outside_the_exact_regime():
    rng = np.random.default_rng(3)
    a = dc.exact_operand(rng, (4096, 2), 30)
    z = dc.exact_rows(rng, (4096, 2), 23).astype(np.float64)
    assert dc.budget(a, z) >= 2.0 ** 53
    with pytest.raises(AssertionError):
        dc.assert_budget(dc.budget(a, z), "an over-long contraction")
    assert dc._quantum(np.array([0.75, -2.5, 0.0])) == 0.25


# ------------------------------------------------------------------------------------------------ the rounded leg
def _within(ref_ld, got64, cap):
    return dc.worst_ratio(ref_ld, got64, cap)


@functools.lru_cache(maxsize=None)
def _block_ref(case, mode):
    zc, op, scale, _ = dc.make_block(case, mode, False)
    return zc, op, scale, dc.ref_block(mode, zc, op, case, scale, dtype=dc.LD), dc.cap_block(mode, zc, op, case, scale)


def _rounded_block(case, mode, mistake=None):
    zc, op, scale, ref, cap = _block_ref(case, mode)
    return _within(ref, dc.ref_block(mode, zc, op, case, scale, mistake=mistake), cap)


@functools.lru_cache(maxsize=None)
def _sketch_ref(case, trans):
    zc, a, scale = dc.make_sketch(case, False)
    return zc, a, scale, dc.ref_sketch(a, zc, case, trans, scale, dtype=dc.LD), dc.cap_sketch(a, zc, case, trans, scale)


def _rounded_sketch(case, trans, mistake=None):
    zc, a, scale, ref, cap = _sketch_ref(case, trans)
    return _within(ref, dc.ref_sketch(a, zc, case, trans, scale, mistake=mistake), cap)


@functools.lru_cache(maxsize=None)
def _gram_ref(case):
    zc, scale = dc.make_gram(case, False)
    return zc, scale, dc.ref_gram(zc, case, scale, dtype=dc.LD), dc.cap_gram(zc, case, scale)


def _rounded_gram(case, mistake=None):
    zc, scale, ref, cap = _gram_ref(case)
    return _within(ref, dc.ref_gram(zc, case, scale, mistake=mistake), cap)


@functools.lru_cache(maxsize=None)
def _cross_ref(case):
    a, b = dc.make_cross(case, False)
    return a, b, dc.ref_cross(a, b, case, dtype=dc.LD), dc.cap_cross(a, b, case)


def _rounded_cross(case, mistake=None):
    a, b, ref, cap = _cross_ref(case)
    return _within(ref, dc.ref_cross(a, b, case, mistake=mistake), cap)


def _sketch(name):
    return next(c for c in dc.SKETCH_CASES if c.name == name)


def test_longdouble_reference_against_float64_is_inside_the_cap():
    for case in dc.BLOCK_ROUNDED + dc.BLOCK_ROUNDED_FORCED:
        for mode in ("matvec", "project", "backproject"):
            assert _rounded_block(case, mode) <= 1.0, (case, mode)
    for name in dc.SKETCH_ROUNDED:
        for trans in (False, True):
            assert _rounded_sketch(_sketch(name), trans) <= 1.0, name
    for case in dc.GRAM_ROUNDED:
        assert _rounded_gram(case) <= 1.0, case
    for case in dc.CROSS_ROUNDED:
        assert _rounded_cross(case) <= 1.0, case


# ------------------------------------------------------------------------------------------------ planted mistakes
GRAM_ONLY = ("mirror_wrong_triangle", "diagonal_unmirrored", "no_bta")
NOT_BLOCK = GRAM_ONLY + ("intercept_every_range", "write_padding")       # (the block outputs are [rows, k]: no padding columns)


def _exact_changes(mistake):
    """Where the mistake changes a bit of the exact-leg result (payload, padding or accumulate start) at a table shape."""
    for case in (() if mistake in NOT_BLOCK else _block_sample()):
        for mode in ("matvec", "project", "backproject"):
            zc, op, scale, c0 = dc.make_block(case, mode, True)
            for acc in ((False, True) if mode != "project" else (False,)):
                kw = dict(c0=c0 if acc else None, accumulate=acc)
                if not np.array_equal(dc.ref_block(mode, zc, op, case, scale, **kw),
                                      dc.ref_block(mode, zc, op, case, scale, mistake=mistake, **kw)):
                    return f"block {mode} {case}"
    for case in (() if mistake in GRAM_ONLY else dc.SKETCH_CASES):
        if case.n * case.m * case.r > 3e8:
            continue
        zc, a, scale = dc.make_sketch(case, True)
        for trans in (False, True):
            for acc in (False, True):
                kw = dict(c0=dc.sketch_start(case, trans) if acc else None, accumulate=acc)
                if not np.array_equal(dc.ref_sketch(a, zc, case, trans, scale, **kw),
                                      dc.ref_sketch(a, zc, case, trans, scale, mistake=mistake, **kw)):
                    return f"sketch {case}"
    for case in dc.GRAM_CASES:
        if case.n > 1000:
            continue
        zc, scale = dc.make_gram(case, True)
        if not np.array_equal(dc.ref_gram(zc, case, scale), dc.ref_gram(zc, case, scale, mistake=mistake)):
            return f"gram {case}"
    for case in dc.CROSS_CASES:
        if case.n > 1000:
            continue
        a, b = dc.make_cross(case, True)
        if not np.array_equal(dc.ref_cross(a, b, case), dc.ref_cross(a, b, case, mistake=mistake)):
            return f"cross {case}"
    return None


def _rounded_worst(mistake):
    worst = 0.0
    for case in (() if mistake in NOT_BLOCK else dc.BLOCK_ROUNDED + dc.BLOCK_ROUNDED_FORCED):
        for mode in ("matvec", "project", "backproject"):
            worst = max(worst, _rounded_block(case, mode, mistake))
    for name in (() if mistake in GRAM_ONLY else dc.SKETCH_ROUNDED):
        for trans in (False, True):
            worst = max(worst, _rounded_sketch(_sketch(name), trans, mistake))
    for case in dc.GRAM_ROUNDED:
        worst = max(worst, _rounded_gram(case, mistake))
    for case in dc.CROSS_ROUNDED:
        worst = max(worst, _rounded_cross(case, mistake))
    return worst


@pytest.mark.parametrize("mistake", dc.MISTAKES)
def test_every_planted_mistake_is_caught(mistake):
    where = _exact_changes(mistake)
    assert where is not None, f"{mistake}: no shape of the tables changes a bit of the exact leg -- the table is missing a shape"
    worst = _rounded_worst(mistake)
    assert worst >= 100.0, f"{mistake}: at most {worst:.3g} x the cap on the rounded-leg shapes -- the table is missing a shape"


# ------------------------------------------------------------------------------------------------ coverage
def test_tables_cover_every_arm_at_256_cus():
    covered, want = dc.covered_arms(256), dc.all_arms()
    assert covered - dc.ARMS_ELSEWHERE == want, (f"arms never launched: {sorted(map(str, want - covered))}; "
                                                 f"arms the model does not list: {sorted(map(str, covered - dc.ARMS_ELSEWHERE - want))}")


def test_tables_hold_the_required_shapes():
    for rt in (1, 2, 4):
        cases = dc.block_cases(rt)
        for k in dc.BLOCK_K:
            assert {(c.n, c.M) for c in cases if c.k == k} >= {(n, M) for n in dc.block_n(rt) for M in dc.BLOCK_M_ALL}
        assert {c.M for c in cases} >= set(dc.BLOCK_M) and all(c.rt == (0 if rt == 1 else rt) for c in cases)
    assert {(c.n, c.M, c.k) for c in dc.block_cases(1)} >= set(dc.BLOCK_LONG) | {dc.BLOCK_BY_SIZE}
    assert dc.zb_model(*dc.BLOCK_BY_SIZE, 256)["rt"] == 2 and dc.BLOCK_BY_SIZE[0] % 256 != 0
    shapes = {(c.n, c.m, c.r, bool(c.bt)) for c in dc.SKETCH_CASES}
    assert shapes >= {(8300, 16, 512, True), (66000, 16, 5, True), (70, 3202, 1030, False), (23, 256, 128, False),
                      (1031, 384, 129, False), (1, 256, 129, True)}
    for name, (ti, tmb, tj) in {"bt_map_ragged_tiles_i4": (4, 64, 65), "bt_map_ragged_tiles_i1": (1, 256, 516),
                                "map_ragged_tiles_i9": (9, 24, 26)}.items():
        c = _sketch(name)
        g = dc.sk_model(c.n, c.m, c.r, c.pad, c.bt, True, dc.sketch_ldc(c, True), 256)
        assert (g["tiles_i"], g["tmb"], g["tiles_j"]) == (ti, tmb, tj), name
    assert {(c.msub, c.n) for c in dc.GRAM_CASES} >= {(ms, n) for ms in (128, 256, 384) for n in dc.GRAM_N}
    assert {(c.M, c.n) for c in dc.CROSS_CASES} >= {(ms, n) for ms in (128, 256, 384) for n in dc.GRAM_N}
    assert dc.gram_model(384, 20000, 256)["starts_inside"] and dc.gram_model(384, 20000, 256, cross=True)["starts_inside"]
