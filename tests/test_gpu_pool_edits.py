"""The two-layer kernel's single-edit pool on the device (hipConvTokenMaxpoolTables / hipConvTokenMaxpoolEdits,
include/xgpr_hip/pool_edits.h; Conv1dTwoLayerKernel.pool_edits).  No tolerance anywhere: the yardstick is hipConvTokenMaxpool on the
written-out mutants (written out HERE, with numpy, not by the code under test), every value must equal it, and wherever no table
row is zero -- every case but the last -- the bits must be the same too.

Shapes.  n = 5 sequences of L = 40 positions with lengths conv_width (one window: the deletions are NaN), conv_width + 1, L and two
ragged ones; token positions past a length hold 255 and are never read.  The windows cover every tile layout (P = 4, 32, 256, 512
with packed index registers, 1024) and the 4608-float table; 70 / 1100 filters are a ragged tile and two tiles."""
import numpy as np
import pytest
import torch

from guarded import same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda"
N, L = 5, 40
GRID = [(1, 4, 4), (3, 8, 21), (9, 21, 21), (9, 40, 100), (30, 21, 21), (3, 18, 256)]
FILTERS = [70, 1100]
MODES = ("substitutions", "deletions", "insertions")


@pytest.fixture(scope="module")
def ext():
    from xgpr_amd import xgpr_hip_rfgen_ext as e
    return e


def padded(width):
    return 1 << max(1, int(np.ceil(np.log2(width))))


def operands(cw, C, V, F, seed=0, zero_row=False):
    rng = np.random.default_rng([cw, C, V, F, seed])
    lens = np.asarray([cw, cw + 1, L, int(rng.integers(cw + 2, L)), int(rng.integers(cw + 2, L))], dtype=np.int32)
    tokens = rng.integers(0, V, size=(N, L)).astype(np.uint8)
    table = rng.standard_normal((V, C)).astype(np.float32)
    if zero_row:                                         # a padding token: an all-zero row, and runs of it longer than a window
        table[0] = 0.0
        tokens[2, 5:5 + 2 * cw + 1] = 0
        tokens[3, :cw + 1] = 0
    for i, s in enumerate(lens):
        tokens[i, s:] = 255
    P = padded(cw * C)
    radem = rng.choice(np.asarray([-1, 1], dtype=np.int8), size=(3, 1, -(-F // P) * P))
    chi = (0.2 + rng.random(F)).astype(np.float32)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return dict(tokens=tokens, lens=lens, table=table, cw=cw, F=F, V=V,
                dev=dict(tokens=to(tokens), table=to(table), radem=to(radem), chi=to(chi)))


def pool_written_out(ext, c, rows, lens):
    """hipConvTokenMaxpool of token rows [m, width] (numpy uint8) with host lengths -> float32 [m, F] in zeroed rows."""
    d = c["dev"]
    out = torch.zeros((rows.shape[0], c["F"]), dtype=torch.float32, device=DEV)
    ext.hipConvTokenMaxpool(torch.from_numpy(np.ascontiguousarray(rows)).to(DEV), d["table"], out, d["radem"], d["chi"],
                            np.ascontiguousarray(lens, dtype=np.int32), c["cw"])
    return out


def geometry(V, mode):
    return (L + 1 if mode == "insertions" else L), (1 if mode == "deletions" else V)


def reference(ext, c, mode):
    """[N, slots, values, F] (+ the NaN mask [N, slots]): every mutant written out with numpy and pooled by the existing operator."""
    tokens, lens, cw, V, F = c["tokens"], c["lens"], c["cw"], c["V"], c["F"]
    slots, per = geometry(V, mode)
    width = L + 1
    rows = np.full((N, slots, per, width), 255, dtype=np.uint8)
    mlen = np.zeros((N, slots, per), dtype=np.int32)
    live = np.zeros((N, slots), dtype=bool)
    nan = np.zeros((N, slots), dtype=bool)
    for i in range(N):
        s = int(lens[i])
        seq = tokens[i, :s]
        for site in range(slots):
            inside = site <= s if mode == "insertions" else site < s
            if inside and mode == "deletions" and s == cw:
                nan[i, site] = True
            live[i, site] = inside and not nan[i, site]
            for v in range(per):
                if not live[i, site]:
                    mut = seq                                # (a placeholder: the result is not used)
                elif mode == "substitutions":
                    mut = seq.copy()
                    mut[site] = v
                elif mode == "deletions":
                    mut = np.delete(seq, site)
                else:
                    mut = np.insert(seq, site, v)
                rows[i, site, v, :len(mut)] = mut
                mlen[i, site, v] = len(mut)
    ref = pool_written_out(ext, c, rows.reshape(-1, width), mlen.reshape(-1)).view(N, slots, per, F)
    ref = ref * torch.from_numpy(live).to(DEV)[:, :, None, None]                    # slots past the sequence: zero rows
    ref = ref.masked_fill(torch.from_numpy(nan).to(DEV)[:, :, None, None], float("nan"))
    return ref, torch.from_numpy(nan).to(DEV), torch.from_numpy(live).to(DEV)


def tables(ext, c):
    d = c["dev"]
    shape = (N, L - c["cw"] + 2, c["F"])
    pm = torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)            # (overwritten as a whole: no NaN may stay)
    sm = torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)
    ext.hipConvTokenMaxpoolTables(d["tokens"], d["table"], pm, sm, d["radem"], d["chi"], c["lens"], c["cw"])
    return pm, sm


def edits(ext, c, pm, sm, mode, lo=0, cnt=None):
    d = c["dev"]
    slots, per = geometry(c["V"], mode)
    cnt = N * slots - lo if cnt is None else cnt
    out = torch.full((cnt, c["F"]) if mode == "deletions" else (cnt, per, c["F"]), float("nan"), dtype=torch.float32, device=DEV)
    ext.hipConvTokenMaxpoolEdits(d["tokens"], d["table"], pm, sm, out, d["radem"], d["chi"], c["lens"], c["cw"], mode, lo, cnt)
    return out


@pytest.fixture(scope="module")
def case_cache():
    return {}


def get_case(ext, cache, cw, C, V, F):
    """Operands, tables and the three references of a shape: computed once, shared by the tests, never modified."""
    key = (cw, C, V, F)
    if key not in cache:
        c = operands(cw, C, V, F)
        assert ext.conv_token_maxpool_edits_ok(cw * C, V, C, F) == 1
        c["pm"], c["sm"] = tables(ext, c)
        c["ref"] = {mode: reference(ext, c, mode) for mode in MODES}
        cache[key] = c
    return cache[key]


@pytest.mark.parametrize("F", FILTERS)
@pytest.mark.parametrize("cw,C,V", GRID)
def test_tables_are_the_operator_on_prefixes_and_suffixes(ext, case_cache, cw, C, V, F):
    c = get_case(ext, case_cache, cw, C, V, F)
    pm, sm, tokens, lens = c["pm"], c["sm"], c["tokens"], c["lens"]
    nkmax = L - cw + 1
    assert not bool(torch.isnan(pm).any()) and not bool(torch.isnan(sm).any())
    pre_rows, pre_len, pre_at, suf_rows, suf_len, suf_at = [], [], [], [], [], []
    for i in range(N):
        nk = int(lens[i]) - cw + 1
        assert bool((pm[i, 0] == 0).all()) and bool((sm[i, nk:] == 0).all()) and bool((pm[i, nk + 1:] == 0).all())
        for j in range(1, nk + 1):                       # PM[i, j]: the sequence cut to its first j windows
            pre_rows.append(tokens[i])
            pre_len.append(j + cw - 1)
            pre_at.append((i, j))
        for j in range(nk):                              # SM[i, j]: the sequence from token j on
            row = np.full(L, 255, dtype=np.uint8)
            row[:L - j] = tokens[i, j:]
            suf_rows.append(row)
            suf_len.append(int(lens[i]) - j)
            suf_at.append((i, j))
    for table, rows, lengths, at in ((pm, pre_rows, pre_len, pre_at), (sm, suf_rows, suf_len, suf_at)):
        ref = pool_written_out(ext, c, np.stack(rows), np.asarray(lengths))
        idx = torch.tensor(at, device=DEV)
        got = table[idx[:, 0], idx[:, 1]]
        assert bool((got == ref).all())
        assert torch.equal(got, ref) and same_bits(got, ref)                        # (no zero table row: the zeros' signs agree too)
    assert nkmax + 1 == pm.shape[1]
    pm2, sm2 = tables(ext, c)
    assert same_bits(pm2, pm) and same_bits(sm2, sm)                                # the same bits twice


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("F", FILTERS)
@pytest.mark.parametrize("cw,C,V", GRID)
def test_edits_equal_the_operator_on_written_out_mutants(ext, case_cache, cw, C, V, F, mode):
    c = get_case(ext, case_cache, cw, C, V, F)
    ref, nan, live = c["ref"][mode]
    slots, per = geometry(V, mode)
    out = edits(ext, c, c["pm"], c["sm"], mode).view(N, slots, per, F)
    assert bool(((out == ref) | nan[:, :, None, None]).all())
    assert bool((torch.isnan(out) == nan[:, :, None, None].expand_as(out)).all())   # NaN: the deletions at one window, only those
    assert bool(nan.any()) == (mode == "deletions")
    keep = ~nan
    assert torch.equal(out[keep], ref[keep]) and same_bits(out[keep], ref[keep])
    assert bool((out[~live & keep] == 0).all()) and bool((~live).any())              # slots past the length: zero rows
    assert float(out[keep].max()) > 0
    if mode == "substitutions":                          # the own token gives the sequence's own pooled row
        own = pool_written_out(ext, c, c["tokens"], c["lens"])
        for i in range(N):
            s = int(c["lens"][i])
            pos = torch.arange(s, device=DEV)
            got = out[i, pos, torch.from_numpy(c["tokens"][i, :s].astype(np.int64)).to(DEV)]
            assert bool((got == own[i][None, :]).all())
    again = edits(ext, c, c["pm"], c["sm"], mode).view(N, slots, per, F)
    assert same_bits(again, out)                                                     # the same bits twice
    # a slab that starts and ends inside a sequence is that slice of the whole
    lo, cnt = slots + 3, slots + slots // 2
    part = edits(ext, c, c["pm"], c["sm"], mode, lo, cnt).view(cnt, per, F)
    assert same_bits(part, out.view(N * slots, per, F)[lo:lo + cnt])


@pytest.mark.parametrize("mode", MODES)
def test_a_zero_table_row_changes_at_most_the_sign_of_a_zero(ext, mode):
    """Token 0 is an all-zero row and runs of it fill whole windows: their products are +-0.0, and which sign survives depends on
    the order of the windows.  Equal as real numbers; the signs of the zeros are not compared."""
    cw, C, V, F = 3, 8, 21, 70
    c = operands(cw, C, V, F, seed=1, zero_row=True)
    pm, sm = tables(ext, c)
    ref, nan, _ = reference(ext, c, mode)
    slots, per = geometry(V, mode)
    out = edits(ext, c, pm, sm, mode).view(N, slots, per, F)
    assert bool(((out == ref) | nan[:, :, None, None]).all())
    assert bool((torch.isnan(out) == nan[:, :, None, None].expand_as(out)).all())
    nz = (ref != 0) & ~torch.isnan(ref)
    assert same_bits(out[nz], ref[nz]) and bool(nz.any())


# ------------------------------------------------------------------------------------------------ the kernel object's two routes
@pytest.mark.parametrize("cw,C,V,F", [(3, 8, 21, 70), (9, 21, 21, 1100)])
@pytest.mark.parametrize("mode", MODES)
def test_pool_edits_equals_pool_edits_composed(ext, monkeypatch, cw, C, V, F, mode):
    from xgpr_amd.dataset import TokenBatch
    from xgpr_amd.kernels import Conv1dTwoLayerKernel
    c = operands(cw, C, V, F, seed=2)
    kernel = Conv1dTwoLayerKernel((N, L, C), 64, device=DEV, kernel_spec_parms={"conv_width": cw, "init_rffs": F})
    slots, per = geometry(V, mode)
    kernel.POOL_EDITS_ELEMS = 7 * per * F                # slabs of 7 slots: they end inside sequences
    batch = TokenBatch(c["dev"]["tokens"], c["dev"]["table"])

    def gather(gen):
        lows, rows = zip(*[(lo, r.reshape(-1, per, F)) for lo, r in gen])
        assert list(lows) == list(range(0, N * slots, 7))
        return torch.cat(rows)

    calls = []
    real = ext.hipConvTokenMaxpoolEdits
    monkeypatch.setattr(ext, "hipConvTokenMaxpoolEdits", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    fast = gather(kernel.pool_edits(batch, c["lens"], mode))
    assert len(calls) == -(-N * slots // 7)                                          # the operator route was the one taken
    slow = gather(kernel.pool_edits_composed(batch, c["lens"], mode))
    assert len(calls) == -(-N * slots // 7)
    nan = torch.isnan(slow)
    assert bool(((fast == slow) | nan).all()) and bool((torch.isnan(fast) == nan).all())
    assert same_bits(fast[~nan], slow[~nan])
    monkeypatch.setattr(ext, "conv_token_maxpool_edits_ok", lambda *a: 0)            # the fallback, forced
    forced = gather(kernel.pool_edits(batch, c["lens"], mode))
    assert len(calls) == -(-N * slots // 7)
    assert same_bits(forced, slow)
    with pytest.raises(RuntimeError, match="TokenBatch"):
        next(kernel.pool_edits(c["dev"]["table"][c["dev"]["tokens"].clamp(max=V - 1).long()], c["lens"], mode))
    with pytest.raises(RuntimeError, match="edit must be one of"):
        next(kernel.pool_edits(batch, c["lens"], "swaps"))


def test_wrapper_errors(ext):
    c = operands(3, 8, 21, 70)
    d = c["dev"]
    pm, sm = tables(ext, c)
    out = torch.full((L, 21, 70), float("nan"), dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="mode must be one of"):
        ext.hipConvTokenMaxpoolEdits(d["tokens"], d["table"], pm, sm, out, d["radem"], d["chi"], c["lens"], 3, "swaps", 0, L)
    with pytest.raises(RuntimeError, match="Wrong array sizes"):
        ext.hipConvTokenMaxpoolEdits(d["tokens"], d["table"], pm, sm, out, d["radem"], d["chi"], c["lens"], 3, "deletions", 0, L)
    with pytest.raises(RuntimeError, match="Wrong array sizes"):
        ext.hipConvTokenMaxpoolEdits(d["tokens"], d["table"], pm[:, 1:].contiguous(), sm, out, d["radem"], d["chi"], c["lens"], 3,
                                     "substitutions", 0, L)
    with pytest.raises(RuntimeError, match="slot range"):
        ext.hipConvTokenMaxpoolEdits(d["tokens"], d["table"], pm, sm, out, d["radem"], d["chi"], c["lens"], 3, "substitutions",
                                     N * L - L + 1, L)
    with pytest.raises(TypeError, match="pm"):
        ext.hipConvTokenMaxpoolEdits(d["tokens"], d["table"], pm.double(), sm, out, d["radem"], d["chi"], c["lens"], 3,
                                     "substitutions", 0, L)
    assert bool(torch.isnan(out).all())                                              # nothing was launched
    table = torch.zeros((243, 19), dtype=torch.float32, device=DEV)                  # 4617 floats
    chi, radem = d["chi"][:64].contiguous(), d["radem"][:, :, :64].contiguous()
    pm = torch.zeros((N, L - 1, 64), dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="xgpr_conv_token_maxpool_edits_ok"):
        ext.hipConvTokenMaxpoolTables(d["tokens"], table, pm, pm.clone(), radem, chi, c["lens"], 3)
