"""Dense references, derived error caps, planted mistakes and an arm model for the float64 matrix-core contractions over
float32 feature rows: the block kernels (zblock.inc), the three sketch_gemm kernels, gram.inc and cross_gram.inc.  numpy
only -- independent of xgpr_amd, of the oracle and of torch (tests/dense_solver_steps.py is the precedent).

Two legs.

EXACT.  Feature rows are integers x 2^-b (exact in float32), the float64 operand integers x 2^-c, the explicit scale a power
of two, the intercept column 1.  ``budget`` computes, from the actual data, the sum of the absolute values of the terms of
every output in units of the common quantum and ``make_*`` asserts it below 2^53: every product and every partial sum, in
any order, fused or not, is then an integer multiple of the quantum below 2^53 -- representable --, so a correct kernel
returns the numpy float64 product BIT FOR BIT.  The magnitudes (11-bit rows x 20-bit operands, 6-bit rows x 10-bit vectors
for the two-stage matvec) make the sums need more than 24 bits: float32 accumulation would change bits.

ROUNDED.  Uniform rows in (-1, 1), a normal operand, the library's default (float32-rounded) scale, against a np.longdouble
product entry by entry under |err_ij| <= gamma_{K + c} sum_k |a_ki| |b_kj|: K - 1 additions in any order of ranges, chunks
and matrix-core steps, and c = EXTRA roundings for what surrounds them (the product with the scale inside or outside the
sum, 1 / scale for the intercept column of the block kernels and its product with the scale, the two scale factors of the
gram store, s * s).  Each cap is evaluated at 2^-53 and at the longdouble roundoff and the two are added (``_both``): the
reference's own error is inside the cap, nothing is fitted.

``mistake=`` plants one structural error into the reference (tests/test_contractions_host.py shows that the committed shape
tables catch every one of them); the ``*_model`` functions restate the launchers' geometry for a CU count -- they exist to
prove coverage and are themselves checked against the workspace sizes the library reports (tests/test_gpu_contractions.py)."""
import functools
from collections import namedtuple

import numpy as np

LD = np.longdouble
U64 = 2.0 ** -53
ULD = float(np.finfo(LD).eps) / 2
EXTRA = 8                        # roundings per output beside the K - 1 additions (see above): at most 6 are ever spent
SENTINEL = -7.25                 # what every output, padding and guard holds before a call
GUARD = 256                      # float64 elements in front of and behind every output

MISTAKES = ("drop_k_tail", "drop_range", "overwrite", "swap_even_odd", "shift_compaction", "scale_intercept", "scale_twice",
            "scale_once_matvec", "intercept_every_range", "mirror_wrong_triangle", "diagonal_unmirrored", "no_bta",
            "write_padding")


def gamma(n, u=U64):
    n = float(n)
    return n * u / (1.0 - n * u) if n * u < 1.0 else np.inf


def _both(fn):
    """A cap: the bound for float64 arithmetic plus the bound for this file's own longdouble evaluation."""
    return fn(U64) + fn(ULD)


def default_scale(num_rffs, icpt):
    """The library's RBF-family scale: sqrt(1 / (F - 0.5)) or sqrt(1 / F), F = num_rffs / 2, rounded to float32."""
    f = num_rffs // 2
    return float(np.float32(np.sqrt(1.0 / (f - 0.5 if icpt else f))))


# ------------------------------------------------------------------------------------------------------------ the cases
BlockCase = namedtuple("BlockCase", "n M k icpt rt")                    # rt: the forced row-tile count, 0 = by size
SketchCase = namedtuple("SketchCase", "name n m r pad bt icpt")
GramCase = namedtuple("GramCase", "n m msub ldpad icpt")
CrossCase = namedtuple("CrossCase", "n M ldpad")

BLOCK_K = (1, 16, 17, 20, 21, 24, 25, 28, 29, 32)                       # both ends of every column arm
BLOCK_M = (4, 36, 64, 96, 132, 516, 1024, 1540)
BLOCK_M_ALL = (36, 132, 1540)                                           # every (column arm, RT) pair meets these at every n
BLOCK_LONG = ((40000, 512, 17), (100000, 64, 26))                       # 3 and 7 chunks of 32 rows per W range
BLOCK_BY_SIZE = (131072 + 129, 64, 22)                                  # RT = 2 by size on 256 CUs, ragged last tile
SCALE_EXACT = 2.0 ** -3


def block_n(r):
    return (1, 128 * r - 1, 128 * r + 1, 3 * 128 * r + 17)


@functools.lru_cache(maxsize=None)
def block_cases(rt):
    """The block-kernel table of one row-tile count (rt = 1: not forced, every n is below the size thresholds)."""
    r, forced = rt, (0 if rt == 1 else rt)
    out, i = [], 0
    for k in BLOCK_K:
        for n in block_n(r):
            for M in BLOCK_M_ALL:
                out.append(BlockCase(n, M, k, i % 2 == 0, forced))
                i += 1
    for M in BLOCK_M:
        if M in BLOCK_M_ALL:
            continue
        for j, k in enumerate(BLOCK_K):
            out.append(BlockCase(block_n(r)[(j + i) % 4], M, k, i % 2 == 1, forced))
            i += 1
    if rt == 1:
        out += [BlockCase(n, M, k, True, 0) for n, M, k in BLOCK_LONG]
        out.append(BlockCase(*BLOCK_BY_SIZE, False, 0))
    return tuple(out)


BLOCK_ROUNDED = (BlockCase(401, 1540, 22, True, 0), BlockCase(129, 132, 32, False, 0), BlockCase(127, 36, 17, True, 0),
                 BlockCase(1000, 516, 26, True, 0), BlockCase(385, 1024, 1, False, 0))
BLOCK_ROUNDED_FORCED = (BlockCase(1553, 132, 22, True, 4), BlockCase(513, 1540, 29, False, 4),
                        BlockCase(785, 1540, 22, True, 2), BlockCase(257, 36, 16, False, 2))

SKETCH_CASES = (
    SketchCase("one_chunk_k16", 16, 256, 128, 128, False, True),
    SketchCase("odd_chunks_k48", 48, 256, 128, 128, False, False),
    SketchCase("k_tail_several_ranges", 1031, 384, 129, 128, False, True),
    SketchCase("r129_pad128", 300, 128, 129, 128, False, False),
    SketchCase("direct_r37_pad64", 1000, 516, 37, 64, False, False),
    SketchCase("direct_r5_pad64", 70, 128, 5, 64, False, True),
    SketchCase("bt_one_chunk_k16", 16, 16, 128, 128, True, True),
    SketchCase("bt_odd_chunks_k48", 130, 48, 128, 128, True, False),
    SketchCase("bt_one_datapoint", 1, 256, 129, 128, True, True),
    SketchCase("bt_many_ranges", 130, 4096, 128, 128, True, True),
    SketchCase("bt_direct_r37_pad64", 1001, 516, 37, 64, True, False),
    SketchCase("bt_direct_r5_pad64", 65, 128, 5, 64, True, True),
    # tile maps of more than one block, the last one ragged (256 CUs: tmb 64 x 65 column tiles, 256 x 516, 24 x 26)
    SketchCase("bt_map_ragged_tiles_i4", 8300, 16, 512, 128, True, True),
    SketchCase("bt_map_ragged_tiles_i1", 66000, 16, 5, 128, True, False),
    SketchCase("map_ragged_tiles_i9", 70, 3202, 1030, 128, False, True),
    SketchCase("bt_map_whole_blocks", 16384, 16, 512, 128, True, False),
    # one range through the LDS kernel + a K % 16 tail: the recursion forces accumulate for a caller who did not ask
    SketchCase("one_range_k_tail", 23, 256, 128, 128, False, True),
    # 17 ranges of 256, the last one 5 (4) contraction indices: an EMPTY last range for the LDS kernel + the tail recursion
    SketchCase("last_range_lt16_lds", 4101, 256, 128, 128, False, True),
    SketchCase("last_range_lt16_direct", 4101, 132, 37, 64, False, False),
    SketchCase("bt_last_range_lt16_direct", 65, 4100, 128, 128, True, True),
)
SKETCH_ROUNDED = ("k_tail_several_ranges", "direct_r37_pad64", "bt_many_ranges", "bt_direct_r37_pad64", "one_range_k_tail",
                  "bt_map_ragged_tiles_i4", "last_range_lt16_lds", "bt_one_datapoint")

GRAM_N = (9, 16, 37, 133, 20000)
GRAM_CASES = tuple(GramCase(n, msub, msub, 6 if (i + j) % 2 else 0, (i + j) % 2 == 0)
                   for i, msub in enumerate((128, 256, 384)) for j, n in enumerate(GRAM_N)) + (
    GramCase(37, 512, 256, 0, True), GramCase(133, 384, 128, 6, False))              # msub < num_rffs
GRAM_ROUNDED = (GramCase(133, 256, 256, 6, True), GramCase(9, 128, 128, 0, True), GramCase(1000, 384, 384, 0, False),
                GramCase(37, 512, 256, 0, True))
CROSS_CASES = tuple(CrossCase(n, M, 6 if (i + j) % 2 else 0) for i, M in enumerate((128, 256, 384)) for j, n in enumerate(GRAM_N))
CROSS_ROUNDED = (CrossCase(133, 256, 6), CrossCase(9, 128, 0), CrossCase(1000, 384, 0))


# ------------------------------------------------------------------------------------------------------------ the inputs
def _rng(*key):
    return np.random.default_rng([abs(int(x)) for x in key])


def _ints(rng, shape, bits):
    lim = 2 ** bits - 1
    return rng.integers(-lim, lim + 1, size=shape).astype(np.float64)


def exact_rows(rng, shape, bits):
    """float32 rows of integers x 2^-bits (|value| < 1)."""
    return (_ints(rng, shape, bits) * 2.0 ** -bits).astype(np.float32)


def exact_operand(rng, shape, bits):
    return _ints(rng, shape, bits) * 2.0 ** -bits


def rounded_rows(rng, shape):
    return rng.uniform(-1.0, 1.0, size=shape).astype(np.float32)


def features(zc, scale, icpt, dtype=np.float64, mistake=None):
    """Z = scale * rows with Z[:, 0] = 1 under the intercept."""
    s = dtype(scale)
    if mistake == "scale_twice":
        s = s * s
    z = zc.astype(dtype) * s
    if icpt:
        z[:, 0] = dtype(scale) if mistake == "scale_intercept" else dtype(1)
    return z


QUANTUM_FLOOR = 2.0 ** -40       # every exact-leg value is a multiple of it, below 2^22


def _quantum(x):
    """The largest power of two that divides every entry of x (1 for an all-zero array)."""
    xs = np.asarray(x, dtype=np.float64).ravel() / QUANTUM_FLOOR
    xi = xs.astype(np.int64)
    assert np.abs(xs).max(initial=0.0) < 2.0 ** 62 and np.array_equal(xi.astype(np.float64), xs), "not on the 2^-40 grid"
    low = int(np.bitwise_or.reduce(xi)) if xi.size else 0
    return float(low & -low) * QUANTUM_FLOOR if low else 1.0


def budget(a, b):
    """max over outputs of sum_k |a_ki| |b_kj| in units of quantum(a) quantum(b), for a [K, I], b [K, J].  The float64 product
    of the absolute values is itself exact below 2^53 and monotone above, so comparing IT with 2^53 decides the budget."""
    q = _quantum(a) * _quantum(b)
    s = np.abs(a).T @ np.abs(b)
    return float(s.max()) / q if s.size else 0.0


def assert_budget(units, what):
    assert units < 2.0 ** 53, f"{what}: {units:.3e} quanta -- outside the exact regime (2^53 = {2.0 ** 53:.3e})"


def as_int64(x, q):
    xi = np.asarray(x, dtype=np.float64) / q
    assert np.array_equal(xi, np.rint(xi)) and np.abs(xi).max(initial=0) < 2.0 ** 62
    return xi.astype(np.int64)


# ------------------------------------------------------------------------------------------------------------ arm models
ZB_ROWS, ZB_WFEATS, ZB_FEATS, ZB_RING = 32, 512, 32, 4
SK_TI = 128
COLUMN_ARMS = ("kp16", "nb4_1", "nb4_2", "nb4_3", "ct2")


def _cdiv(a, b):
    return -(-a // b)


def column_arm(k):
    return "kp16" if k <= 16 else "ct2" if k > 28 else f"nb4_{(k - 16 + 3) // 4}"


def zb_model(n, M, k, cus, force_rt=0):
    """zb_geometry of launchers.inc."""
    g = {"kp": 16 if k <= 16 else 32, "col": column_arm(k), "mblk": _cdiv(M, ZB_WFEATS)}
    target = max(1, min(_cdiv(2 * cus, g["mblk"]), _cdiv(n, ZB_ROWS)))
    g["rows_per_range"] = _cdiv(_cdiv(n, target), ZB_ROWS) * ZB_ROWS
    g["nrb"] = _cdiv(n, g["rows_per_range"])
    g["t_bytes"] = _cdiv(n * g["kp"] * 8, 256) * 256
    g["slab_bytes"] = g["nrb"] * M * g["kp"] * 8
    rt = 4 if n >= 2 * cus * 512 else 2 if n >= 2 * cus * 256 else 1
    g["rt"] = force_rt if force_rt in (1, 2, 4) else rt
    tiles = _cdiv(n, 128 * g["rt"])
    want = _cdiv(2 * cus, tiles) if g["rt"] == 1 else 1
    want = min(want, max(M // 512, 1), 64)
    g["msplit"], g["feats_per_split"] = 1, M
    if want > 1:
        fps = _cdiv(_cdiv(M, want), 128) * 128
        ms = _cdiv(M, fps)
        if ms > 1:
            g["msplit"], g["feats_per_split"] = ms, fps
    g["tpart_bytes"] = g["msplit"] * n * g["kp"] * 8 if g["msplit"] > 1 else 0
    g["tiles"] = tiles
    g["project_ws_bytes"] = g["tpart_bytes"]
    g["block_ws_bytes"] = g["t_bytes"] + g["slab_bytes"] + g["tpart_bytes"]
    return g


def zb_arms(case, cus):
    g = zb_model(case.n, case.M, case.k, cus, case.rt)
    arms = {("zb_t", g["col"], g["rt"]), ("zb_w", g["col"])}
    if g["msplit"] == 1:
        arms.add(("zb_t_split", "none"))
    else:
        arms.add(("zb_t_split", "short_last" if case.M % g["feats_per_split"] else "whole"))
        arms.add(("zb_project_workspace", "none_unsplit"))           # the same call once more without a workspace
    arms.add(("zb_t_tiles", g["rt"], ("one" if g["tiles"] == 1 else "many") + ("_ragged" if case.n % (128 * g["rt"]) else "_whole")))
    tch = _cdiv(g["feats_per_split"], ZB_FEATS)
    arms.add(("zb_t_chunks", "lt_ring" if tch < ZB_RING else "ge_ring_odd" if tch % 2 else "ge_ring_even"))
    arms.add(("zb_t_tail_chunk", case.M % ZB_FEATS != 0))
    arms.add(("zb_w_groups", "one" if g["mblk"] == 1 else "many_ragged" if case.M % ZB_WFEATS else "many_whole"))
    wch = g["rows_per_range"] // ZB_ROWS
    arms.add(("zb_w_chunks_per_range", "one" if wch == 1 else "lt_ring" if wch < ZB_RING else "gt_ring_odd" if wch % 2 else "gt_ring_even"))
    arms.add(("zb_w_ranges", "one" if g["nrb"] == 1 else "many_ragged" if case.n % g["rows_per_range"] else "many_whole"))
    return arms


def sk_model(n, m, r, pad, bt, trans_out, ldc, cus):
    """sk_geometry and the kernel choice of sketch_gemm_impl (first call; ``tail``: what the K % 16 recursion contracts)."""
    I, J, K = r, (n if bt else m), (m if bt else n)
    lda = _cdiv(r, pad) * pad
    g = {"tiles_i": _cdiv(I, SK_TI), "tiles_j": _cdiv(J, 128)}
    g["tmb"] = max(8, cus // g["tiles_i"] // 8 * 8)
    g["blocks"] = _cdiv(g["tiles_j"], g["tmb"])
    tiles = g["tiles_i"] * g["tiles_j"]
    nsplit = _cdiv(2 * cus, tiles) if tiles < 2 * cus else 1
    slab = (J if trans_out else I) * ldc * 8
    nsplit = max(nsplit, min(K // 8192, max((1 << 30) // slab, 1)))
    nsplit = max(1, min(nsplit, _cdiv(K, 256)))
    g["k_per_split"] = _cdiv(_cdiv(K, nsplit), 16) * 16
    g["nsplit"] = _cdiv(K, g["k_per_split"])
    g["ws_bytes"] = g["nsplit"] * (J if trans_out else I) * ldc * 8
    lds_ok = (not bt) and J % 128 == 0 and lda % 128 == 0 and m % 4 == 0 and (g["nsplit"] > 1 or K >= 16)
    lds_bt_ok = bool(bt) and lda % 128 == 0 and K % 16 == 0
    g["kernel"] = "lds" if lds_ok else "lds_bt" if lds_bt_ok else "direct"
    g["tail"] = K % 16 if lds_ok else 0
    g["last_range"] = K - (g["nsplit"] - 1) * g["k_per_split"]
    return g


def sk_arms(case, trans_out, cus):
    ldc = sketch_ldc(case, trans_out)
    g = sk_model(case.n, case.m, case.r, case.pad, case.bt, trans_out, ldc, cus)
    arms = {("sk_kernel", g["kernel"], bool(case.bt), bool(trans_out)),
            ("sk_ranges", g["kernel"], "one" if g["nsplit"] == 1 else "many"),
            ("sk_map", "one_block" if g["blocks"] == 1 else "ragged_last_block" if g["tiles_j"] % g["tmb"] else "whole_blocks")}
    if g["nsplit"] > 1:
        arms.add(("sk_last_range", "lt16" if g["last_range"] < 16 else "short" if g["last_range"] < g["k_per_split"] else "full"))
    if g["tail"]:
        arms.add(("sk_tail_recursion", "one_range" if g["nsplit"] == 1 else "many_ranges"))
    return arms


def gram_model(msub, n, cus, cross=False):
    """gram_workgroups / cross_gram_workgroups and the stream-K cut of gram_impl / cross_gram_impl."""
    T = msub // 128
    ntiles = T * (T + 1) // 2
    per_tile = (2 if cross else 1) * (n // 16)
    total = ntiles * per_tile
    g = {"workgroups": max(1, min(2 * cus, total)), "tail": n % 16, "nchunks": n // 16, "ntiles": ntiles}
    g["ws_bytes"] = g["workgroups"] * 128 * 128 * 8
    g["units_per_wg"], g["launched"], g["starts_inside"] = 0, 0, False
    if total:
        g["units_per_wg"] = _cdiv(total, g["workgroups"])
        g["launched"] = _cdiv(total, g["units_per_wg"])
        g["starts_inside"] = any((b * g["units_per_wg"]) % per_tile for b in range(g["launched"]))
    return g


def gram_arms(case, cus):
    cross = isinstance(case, CrossCase)
    fam = "cross" if cross else "gram"
    msub = case.M if cross else case.msub
    g = gram_model(msub, case.n, cus, cross)
    arms = {(fam, "tiles", "one" if g["ntiles"] == 1 else "off_diagonal"),
            (fam, "rows", "tail_only" if g["nchunks"] == 0 else "chunks_and_tail" if g["tail"] else "chunks_only"),
            (fam, "ldc", "padded" if case.ldpad else "tight")}
    if g["nchunks"]:
        arms.add((fam, "stream_k", "starts_inside_a_tile" if g["starts_inside"] else
                  "several_tiles_per_workgroup" if g["units_per_wg"] > (2 if cross else 1) * g["nchunks"] else "whole_tiles"))
    if not cross:
        arms.add((fam, "msub", "leading_block" if case.msub < case.m else "all"))
    return arms


def all_arms():
    """Every arm the model knows (the universe of the coverage set equality)."""
    arms = set()
    for col in COLUMN_ARMS:
        arms.add(("zb_w", col))
        for rt in (1, 2, 4):
            arms.add(("zb_t", col, rt))
    arms |= {("zb_t_split", x) for x in ("none", "whole", "short_last")} | {("zb_project_workspace", "none_unsplit")}
    arms |= {("zb_t_tiles", rt, x) for rt in (1, 2, 4) for x in ("one_ragged", "many_ragged")}
    arms |= {("zb_t_chunks", x) for x in ("lt_ring", "ge_ring_odd", "ge_ring_even")}
    arms |= {("zb_t_tail_chunk", x) for x in (False, True)}
    arms |= {("zb_w_groups", x) for x in ("one", "many_ragged", "many_whole")}
    arms |= {("zb_w_chunks_per_range", x) for x in ("one", "lt_ring", "gt_ring_odd")}
    arms |= {("zb_w_ranges", x) for x in ("one", "many_ragged")}
    for tr in (False, True):
        arms |= {("sk_kernel", "direct", False, tr), ("sk_kernel", "direct", True, tr), ("sk_kernel", "lds", False, tr),
                 ("sk_kernel", "lds_bt", True, tr)}
    arms |= {("sk_ranges", kern, x) for kern in ("direct", "lds", "lds_bt") for x in ("one", "many")}
    arms |= {("sk_map", x) for x in ("one_block", "ragged_last_block", "whole_blocks")}
    arms |= {("sk_last_range", x) for x in ("lt16", "short", "full")}
    arms |= {("sk_tail_recursion", x) for x in ("one_range", "many_ranges")}
    for fam in ("gram", "cross"):
        arms |= {(fam, "tiles", x) for x in ("one", "off_diagonal")}
        arms |= {(fam, "rows", x) for x in ("tail_only", "chunks_and_tail", "chunks_only")}
        arms |= {(fam, "ldc", x) for x in ("padded", "tight")}
        arms.add((fam, "stream_k", "starts_inside_a_tile"))
    arms.add(("gram", "stream_k", "whole_tiles"))         # (cross gram: a tile is two runs of chunks, one unit each below 2 CUs units)
    arms |= {("gram", "msub", x) for x in ("leading_block", "all")}
    return arms


# Arms that exist but that no small shape reaches, with the test that holds them: a row count that is a multiple of every tile
# (tests/test_gpu_fullsize.py: 262144 rows), whole W ranges and an even chunk count beyond the ring (the same shape), a gram
# workgroup that owns several whole tiles (more tiles than workgroups: msub >= 4096, tests/test_gpu_nmll.py).
ARMS_ELSEWHERE = ({("zb_t_tiles", rt, x) for rt in (1, 2, 4) for x in ("one_whole", "many_whole")} |
                  {("zb_w_chunks_per_range", "gt_ring_even"), ("zb_w_ranges", "many_whole"),
                   ("gram", "stream_k", "several_tiles_per_workgroup"), ("cross", "stream_k", "several_tiles_per_workgroup")})


def covered_arms(cus):
    """The arms the committed tables launch on a part with ``cus`` compute units."""
    arms = set()
    for rt in (1, 2, 4):
        for case in block_cases(rt):
            arms |= zb_arms(case, cus)
    for case in SKETCH_CASES:
        for tr in (False, True):
            arms |= sk_arms(case, tr, cus)
    for case in GRAM_CASES + CROSS_CASES:
        arms |= gram_arms(case, cus)
    return arms


# ------------------------------------------------------------------------------------------------------------ references
def _keep(K, ranges, mistake):
    """The contraction indices a (mistaken) kernel sums: a boolean mask over K.  ``ranges`` = (count, length)."""
    keep = np.ones(K, dtype=bool)
    nr, per = ranges
    if mistake == "drop_k_tail":
        keep[K // 16 * 16:] = False
    elif mistake == "drop_range" and nr > 1:
        keep[(nr - 1) * per:] = False
    elif mistake == "overwrite" and nr > 1:
        keep[:(nr - 1) * per] = False                      # the last range's store replaces the others
    return keep


def _swap_even_odd(c):
    """Rows 2 t and 2 t + 1 of every 32-row group exchanged (whole pairs only)."""
    out = c.copy()
    pairs = c.shape[0] // 2
    out[0:2 * pairs:2], out[1:2 * pairs:2] = c[1:2 * pairs:2], c[0:2 * pairs:2]
    return out


def _place(payload, rows, ld, c0, accumulate, mistake):
    """The [rows, ld] result array: payload (+ c0 under accumulate) in the leading columns, the padding as it was."""
    full = np.array(c0, dtype=payload.dtype, copy=True)
    assert full.shape == (rows, ld)
    ncols = payload.shape[1]
    add = accumulate and mistake != "overwrite"
    full[:, :ncols] = (full[:, :ncols] + payload) if add else payload
    if mistake == "write_padding":
        full[:, ncols:] = 0
    return full


def block_ranges(case, mode, cus):
    g = zb_model(case.n, case.M, case.k, cus, case.rt)
    if mode == "backproject":
        return g["nrb"], g["rows_per_range"]
    return g["msplit"], g["feats_per_split"]


def ref_block(mode, zc, op, case, scale, c0=None, accumulate=False, dtype=np.float64, mistake=None, cus=256):
    """matvec: s^2 Zc^T (Zc V); project: Z V [n, k]; backproject: Z^T R [M, k] -- Z as ``features``.  op: V [M, k] or R [n, k]."""
    n, M, k = case.n, case.M, case.k
    z = features(zc, scale, case.icpt, dtype, mistake if mode != "matvec" or mistake != "scale_twice" else None)
    if mode == "matvec" and mistake == "scale_once_matvec":
        z1 = features(zc, 1.0, False, dtype)
        if case.icpt:
            z1[:, 0] = dtype(1) / dtype(scale)
        z_first = z1                                       # the first stage un-scaled and no s^2 at the end, only s
    else:
        z_first = z
    opd = op.astype(dtype)
    if mode == "backproject":
        keep = _keep(n, block_ranges(case, mode, cus), mistake)
        res = z[keep].T @ opd[keep]
    else:
        keep = _keep(M, block_ranges(case, mode, cus), mistake)
        t = z_first[:, keep] @ opd[keep]
        if mode == "project":
            res = t
        else:
            keep2 = _keep(n, block_ranges(case, "backproject", cus), mistake if mistake != "drop_k_tail" else None)
            res = z[keep2].T @ t[keep2]
    if mistake == "shift_compaction" and mode != "project":
        res = np.concatenate([res[:, 1:], np.zeros_like(res[:, :1])], axis=1)
    if mistake == "swap_even_odd":
        res = _swap_even_odd(res)
    rows = n if mode == "project" else M
    if c0 is None:
        c0 = np.full((rows, k), SENTINEL, dtype=dtype)
    return _place(res, rows, k, np.asarray(c0, dtype=dtype), accumulate and mode != "project", mistake)


def sketch_ldc(case, trans_out):
    lda = _cdiv(case.r, case.pad) * case.pad
    if trans_out:
        return lda                                         # [J, lda]: the padded operand of the next product
    j = case.n if case.bt else case.m
    return (j + 1) // 2 * 2 + 2


def ref_sketch(a, zc, case, trans_out, scale, c0=None, accumulate=False, dtype=np.float64, mistake=None, cus=256):
    """C[r, J] (+)= A[:, :r]^T Z (bt False, a [n, lda]) or A[:, :r]^T Z^T (bt True, a [m, lda]); the transposed store gives [J, r]."""
    z = features(zc, scale, case.icpt, dtype, mistake)
    ad = a[:, :case.r].astype(dtype)
    b = z.T if case.bt else z                              # [K, J]
    K = b.shape[0]
    ldc = sketch_ldc(case, trans_out)
    g = sk_model(case.n, case.m, case.r, case.pad, case.bt, trans_out, ldc, cus)
    keep = _keep(K, (g["nsplit"], g["k_per_split"]), mistake)
    res = ad[keep].T @ b[keep]
    if mistake == "intercept_every_range" and case.bt and case.icpt:
        res = res + (g["nsplit"] - 1) * ad[0][:, None]
    if mistake == "swap_even_odd":
        res = _swap_even_odd(res)
    if trans_out:
        res = np.ascontiguousarray(res.T)
    rows = res.shape[0]
    if c0 is None:
        c0 = np.full((rows, ldc), SENTINEL, dtype=dtype)
    return _place(res, rows, ldc, np.asarray(c0, dtype=dtype), accumulate, mistake)


def _tile_mask(msub, which):
    """Boolean [msub, msub]: "upper_tiles" = 128 x 128 tiles strictly above the diagonal; "diag_lower" = the strictly lower
    part of the diagonal tiles."""
    i, j = np.indices((msub, msub))
    if which == "upper_tiles":
        return j // 128 > i // 128
    return (i // 128 == j // 128) & (i > j)


def _gram_finish(res, msub, ldpad, c0, accumulate, dtype, mistake):
    ld = msub + ldpad
    if c0 is None:
        c0 = np.full((msub, ld), SENTINEL, dtype=dtype)
    c0 = np.asarray(c0, dtype=dtype)
    if mistake == "swap_even_odd":
        res = _swap_even_odd(res)
    full = _place(res, msub, ld, c0, accumulate, mistake)
    if mistake == "mirror_wrong_triangle":                 # the (never computed) lower tiles copied over the computed ones
        mask = _tile_mask(msub, "upper_tiles")
        full[:, :msub][mask] = c0[:, :msub].T[mask]
    elif mistake == "diagonal_unmirrored":
        mask = _tile_mask(msub, "diag_lower")
        full[:, :msub][mask] = c0[:, :msub][mask]
    return full


def ref_gram(zc, case, scale, c0=None, accumulate=False, dtype=np.float64, mistake=None, cus=256):
    z = features(zc, scale, case.icpt, dtype, mistake)[:, :case.msub]
    keep = _keep(case.n, (1, case.n), mistake)
    res = z[keep].T @ z[keep]
    return _gram_finish(res, case.msub, case.ldpad, c0, accumulate, dtype, mistake)


def ref_cross(a, b, case, c0=None, accumulate=False, dtype=np.float64, mistake=None, cus=256):
    keep = _keep(case.n, (1, case.n), mistake)
    ad, bd = a.astype(dtype)[keep], b.astype(dtype)[keep]
    atb = ad.T @ bd
    res = atb if mistake == "no_bta" else atb + atb.T
    return _gram_finish(res, case.M, case.ldpad, c0, accumulate, dtype, mistake)


# ------------------------------------------------------------------------------------------------------------ the caps
def cap_single(a_abs, b_abs, K):
    """gamma_{K + EXTRA} |A|^T |B| for a [K, I], b [K, J] (absolute values, the scale inside b), float64 and longdouble."""
    s = a_abs.T @ b_abs
    s = s * (1.0 + gamma(K + EXTRA))                        # s itself is a float64 sum of non-negative terms
    return _both(lambda u: gamma(K + EXTRA, u)) * s


def cap_block(mode, zc, op, case, scale):
    za = np.abs(features(zc, scale, case.icpt))
    oa = np.abs(op)
    if mode == "project":
        return cap_single(za.T, oa, case.M)
    if mode == "backproject":
        return cap_single(za, oa, case.n)
    # matvec: the first stage's error gamma_{M + c} |Z| |V| propagates through |Z|^T; the second adds gamma_{n + c} |Z|^T |T^|
    q = za.T @ (za @ oa) * (1.0 + gamma(case.n + case.M + EXTRA))
    return _both(lambda u: (gamma(case.n + EXTRA, u) + gamma(case.M + EXTRA, u)) * (1.0 + gamma(case.M + EXTRA, u))) * q


def cap_sketch(a, zc, case, trans_out, scale):
    za = np.abs(features(zc, scale, case.icpt))
    b = za.T if case.bt else za
    cap = cap_single(np.abs(a[:, :case.r]), b, b.shape[0])
    return np.ascontiguousarray(cap.T) if trans_out else cap


def cap_gram(zc, case, scale):
    za = np.abs(features(zc, scale, case.icpt))[:, :case.msub]
    return cap_single(za, za, case.n)


def cap_cross(a, b, case):
    aa, ba = np.abs(a.astype(np.float64)), np.abs(b.astype(np.float64))
    s = aa.T @ ba
    return _both(lambda u: gamma(2 * case.n + EXTRA, u)) * (s + s.T) * (1.0 + gamma(2 * case.n + EXTRA))


def worst_ratio(ref_ld, got, cap):
    """max |ref - got| / cap over the whole array, the padding included: ``cap`` covers the leading columns, everything
    beside them has cap 0 (it must hold what it held -- any difference there counts as infinite)."""
    err = np.abs(np.asarray(ref_ld, dtype=LD) - np.asarray(got).astype(LD)).astype(np.float64)
    full = np.zeros(err.shape)
    full[:, :cap.shape[1]] = cap
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0.0, 0.0, err / full)
    return float(ratio.max()) if ratio.size else 0.0


# ------------------------------------------------------------------------------------------------------------ case data
def block_bits(mode):
    return (6, 10) if mode == "matvec" else (11, 20)


def make_block(case, mode, exact):
    """-> (rows float32 [n, M], operand float64, scale, start values of the output for the accumulate call)."""
    rng = _rng(case.n, case.M, case.k, case.rt, ("matvec", "project", "backproject").index(mode), int(exact))
    oshape = (case.n, case.k) if mode == "backproject" else (case.M, case.k)
    if not exact:
        return rounded_rows(rng, (case.n, case.M)), rng.standard_normal(oshape), default_scale(case.M, case.icpt), None
    rb, ob = block_bits(mode)
    zc, op = exact_rows(rng, (case.n, case.M), rb), exact_operand(rng, oshape, ob)
    z = features(zc, SCALE_EXACT, case.icpt)
    if mode == "project":
        assert_budget(budget(z.T, op), f"project {case}")
    elif mode == "backproject":
        assert_budget(budget(z, op), f"backproject {case}")
    else:
        t_abs = np.abs(z) @ np.abs(op)                     # sum |z| |v| per row and column, exact while below 2^53
        q = _quantum(z) ** 2 * _quantum(op)
        assert_budget(float((np.abs(z).T @ t_abs).max()) / q, f"matvec {case}")
    rows = case.n if mode == "project" else case.M
    return zc, op, SCALE_EXACT, exact_operand(rng, (rows, case.k), 8)


def make_sketch(case, exact):
    rng = _rng(case.n, case.m, case.r, int(case.bt), int(exact))
    lda = _cdiv(case.r, case.pad) * case.pad
    a = np.zeros((case.m if case.bt else case.n, lda))
    if not exact:
        a[:, :case.r] = rng.standard_normal((a.shape[0], case.r))
        return rounded_rows(rng, (case.n, case.m)), a, default_scale(case.m, case.icpt)
    zc = exact_rows(rng, (case.n, case.m), 11)
    a[:, :case.r] = exact_operand(rng, (a.shape[0], case.r), 20)
    z = features(zc, SCALE_EXACT, case.icpt)
    assert_budget(budget(a[:, :case.r], z.T if case.bt else z), f"sketch {case}")
    return zc, a, SCALE_EXACT


def sketch_start(case, trans_out):
    """Exact start values of C for the accumulate call, padding = SENTINEL."""
    rng = _rng(case.n, case.m, case.r, 77, int(trans_out))
    j = case.n if case.bt else case.m
    rows, cols = (j, case.r) if trans_out else (case.r, j)
    c0 = np.full((rows, sketch_ldc(case, trans_out)), SENTINEL)
    c0[:, :cols] = exact_operand(rng, (rows, cols), 8)
    return c0


def make_gram(case, exact):
    rng = _rng(case.n, case.m, case.msub, int(exact))
    if not exact:
        return rounded_rows(rng, (case.n, case.m)), default_scale(case.m, case.icpt)
    zc = exact_rows(rng, (case.n, case.m), 11)
    z = features(zc, SCALE_EXACT, case.icpt)[:, :case.msub]
    assert_budget(budget(z, z), f"gram {case}")
    return zc, SCALE_EXACT


def make_cross(case, exact):
    rng = _rng(case.n, case.M, 5, int(exact))
    if not exact:
        return rounded_rows(rng, (case.n, case.M)), (0.5 * rng.standard_normal((case.n, case.M))).astype(np.float32)
    a, b = exact_rows(rng, (case.n, case.M), 11), exact_rows(rng, (case.n, case.M), 11)
    assert_budget(2 * budget(a.astype(np.float64), b.astype(np.float64)), f"cross gram {case}")
    return a, b


def gram_start(msub, ldpad, seed):
    c0 = np.full((msub, msub + ldpad), SENTINEL)
    c0[:, :msub] = exact_operand(_rng(msub, ldpad, seed), (msub, msub), 8)
    return c0
