"""CPU-only table of argument validation through the C ABI: every entry point whose implementation lives in
xgpr_amd/csrc/launchers.inc is called with arguments that fail a check BEFORE anything touches the device, and the code and
message (xgpr_last_error) are compared with literals recorded once from the build that preceded the launcher refactor.

What the table pins: the code and text of every host-side check, and -- through rows in which two checks fail at once -- the ORDER
of the checks inside each entry point (the first failing one is the one reported).  No row reaches a HIP call or the device
query: pointers are dummy integers (16-byte aligned, or 4 / 8 bytes off) that are never dereferenced on these paths; the sequence
entry points get a real host array of lengths, which their validation does read."""
import ctypes as C

import numpy as np
import pytest

A = 0x100000                     # a dummy 4096-byte-aligned address
BIG = 1 << 30                    # a workspace size no shape of this table exceeds

SEQLEN = np.asarray([5, 12, 7, 9], dtype=np.int32)            # valid for L = 12, conv_width <= 5
SEQLEN_SHORT = np.asarray([5, 12, 2, 9], dtype=np.int32)      # one sequence below conv_width 3
SEQLEN_LONG = np.asarray([5, 13, 7, 9], dtype=np.int32)       # one sequence beyond L = 12
SL, SL_SHORT, SL_LONG = (a.ctypes.data for a in (SEQLEN, SEQLEN_SHORT, SEQLEN_LONG))


def fht(s="f32", x=A, n=4, dim1=2, dim2=64):
    return f"xgpr_fht_{s}", (x, n, dim1, dim2, None)


def srht(s="f32", x=A, radem=A, n=4, dim=64, rlen=64):
    return f"xgpr_srht_{s}", (x, radem, n, dim, rlen, None)


def rbf(s="f32", x=A, out=A, radem=A, chi=A, n=4, d=60, out_rows=4, m=128, F=64, R=64, icpt=0, ws=A, wb=BIG):
    return f"xgpr_rbf_feature_gen_{s}", (x, out, radem, chi, n, d, out_rows, m, F, R, icpt, ws, wb, None)


def rbfg(s="f32", x=A, out=A, grad=A, radem=A, chi=A, n=4, d=60, out_rows=4, m=128, gr=4, gc=128, F=64, R=64, sigma=1.3, icpt=0,
         ws=A, wb=BIG):
    return f"xgpr_rbf_grad_{s}", (x, out, grad, radem, chi, n, d, out_rows, m, gr, gc, F, R, sigma, icpt, ws, wb, None)


def rbfgr(x=A, z=A, g=A, radem=A, chi=A, n=4, d=60, m=128, F=64, R=64, sigma=1.3, icpt=0, ws=A, wb=BIG):
    return "xgpr_rbf_grad_rows_f32", (x, z, g, radem, chi, n, d, m, F, R, sigma, icpt, ws, wb, None)


def cache(x=A, zc=A, radem=A, chi=A, n=4, d=60, m=128, F=64, R=64, ws=A, wb=BIG):
    return "xgpr_rbf_feature_cache_f32", (x, zc, radem, chi, n, d, m, F, R, ws, wb, None)


def ztz(fn="xgpr_ztz_matvec_f32", x=A, radem=A, chi=A, v=A, w=A, n=4, d=60, m=128, F=64, R=64, icpt=0, ws=A, wb=BIG):
    return fn, (x, radem, chi, v, w, n, d, m, F, R, icpt, ws, wb, None)


def zty(**kw):
    return ztz(fn="xgpr_zty_f32", **kw)


# sequences: n = 4, L = 12, C = 8, conv_width 3 -> windows of 24 elements, padded 32
def conv(s="f32", x=A, out=A, radem=A, chi=A, sh=SL, sd=A, n=4, L=12, Cc=8, out_rows=4, m=128, F=64, R=64, nseq=4, cw=3, sc=0,
         ws=A, wb=BIG):
    return f"xgpr_conv1d_fgen_{s}", (x, out, radem, chi, sh, sd, n, L, Cc, out_rows, m, F, R, nseq, cw, sc, ws, wb, None)


def convg(s="f32", x=A, out=A, grad=A, radem=A, chi=A, sh=SL, sd=A, n=4, L=12, Cc=8, out_rows=4, m=128, gr=4, gc=128, F=64, R=64,
          nseq=4, sigma=1.3, cw=3, sc=0, ws=A, wb=BIG):
    return f"xgpr_conv_grad_{s}", (x, out, grad, radem, chi, sh, sd, n, L, Cc, out_rows, m, gr, gc, F, R, nseq, sigma, cw, sc, ws,
                                   wb, None)


def convr(x=A, zc=A, radem=A, chi=A, sh=SL, sd=A, n=4, L=12, Cc=8, m=128, F=64, R=64, nseq=4, cw=3, sc=0, icpt=0, ws=A, wb=BIG):
    return "xgpr_conv_feature_rows_f32", (x, zc, radem, chi, sh, sd, n, L, Cc, m, F, R, nseq, cw, sc, icpt, ws, wb, None)


def convgr(x=A, z=A, g=A, radem=A, chi=A, sh=SL, sd=A, n=4, L=12, Cc=8, m=128, F=64, R=64, nseq=4, sigma=1.3, cw=3, sc=0, icpt=0,
           ws=A, wb=BIG):
    return "xgpr_conv_grad_rows_f32", (x, z, g, radem, chi, sh, sd, n, L, Cc, m, F, R, nseq, sigma, cw, sc, icpt, ws, wb, None)


def pool(s="f32", x=A, out=A, radem=A, chi=A, sh=SL, sd=A, n=4, L=12, Cc=8, out_rows=4, m=64, F=64, R=64, nseq=4, cw=3, ws=A, wb=BIG):
    return f"xgpr_conv1d_maxpool_{s}", (x, out, radem, chi, sh, sd, n, L, Cc, out_rows, m, F, R, nseq, cw, ws, wb, None)


def zmv(zc=A, v=A, w=A, n=4, m=128, icpt=0, ws=A, wb=BIG):
    return "xgpr_zcache_matvec_f32", (zc, v, w, n, m, icpt, ws, wb, None)


def zmvs(zc=A, v=A, w=A, n=4, m=128, scale=0.1, ws=A, wb=BIG):
    return "xgpr_zcache_matvec_scaled_f32", (zc, v, w, n, m, scale, ws, wb, None)


def zzty(zc=A, y=A, out=A, n=4, m=128, icpt=0, scale=0.0, ws=A, wb=BIG):
    return "xgpr_zcache_zty_f32", (zc, y, out, n, m, icpt, scale, ws, wb, None)


def zblock(which="matvec", zc=A, v=A, out=A, n=4, m=128, k=4, icpt=0, scale=0.0, acc=0, ws=A, wb=BIG):
    if which == "project":
        return "xgpr_zcache_block_project_f32", (zc, v, out, n, m, k, icpt, scale, ws, wb, None)
    return f"xgpr_zcache_block_{which}_f32", (zc, v, out, n, m, k, icpt, scale, acc, ws, wb, None)


def ard(s="f32", n=4, d=8, out_rows=4, m=128, F=64, w_cols=8, map_len=8, sig_len=8, gr=4, gc=128, nls=2, icpt=0):
    return f"xgpr_mini_ard_grad_{s}", (A, A, A, A, A, A, n, d, out_rows, m, F, w_cols, map_len, sig_len, gr, gc, nls, icpt, None)


def sample(s="f64", y=None, zty_out=None, n=4, m=64, P=64, ncols=8, ldo=8, ws=A, wb=BIG):
    return f"xgpr_srht_sample_{s}", (A, A, A, A, y, zty_out, n, m, P, ncols, ldo, ws, wb, None)


def samplerows(y=None, zty_out=None, n=4, m=64, P=64, ncols=8, ldo=8, scale=0.0, icpt=0, ws=A, wb=BIG):
    return "xgpr_srht_sample_rows_f32", (A, A, A, A, y, zty_out, n, m, P, ncols, ldo, scale, icpt, ws, wb, None)


def skg(a=A, lda=64, zc=A, n=32, m=128, c=A, ldc=128, I=8, bt=0, trans=0, scale=0.0, icpt=0, acc=0, ws=A, wb=BIG):
    return "xgpr_sketch_gemm_f64", (a, lda, zc, n, m, c, ldc, I, bt, trans, scale, icpt, acc, ws, wb, None)


def gram(zc=A, n=32, m=128, c=A, ldc=128, msub=128, scale=0.0, icpt=0, acc=0, ws=A, wb=BIG):
    return "xgpr_ztz_gram_f64", (zc, n, m, c, ldc, msub, scale, icpt, acc, ws, wb, None)


def xgram(a=A, b=A, n=32, m=128, c=A, ldc=128, acc=0, ws=A, wb=BIG):
    return "xgpr_cross_gram_f64", (a, b, n, m, c, ldc, acc, ws, wb, None)


# the four checks the five SORF entry points share, one at a time and two at a time (the first of the pair is reported)
def _shared(tag, call):
    return {
        f"{tag}: n == 0": call(n=0),
        f"{tag}: odd num_rffs": call(m=127),
        f"{tag}: num_rffs < 2": call(m=0, F=0),
        f"{tag}: 2 num_freqs != num_rffs": call(F=63),
        f"{tag}: num_freqs > R": call(m=256, F=128),
        f"{tag}: R % P": call(R=96),
        f"{tag}: n == 0 and odd num_rffs": call(n=0, m=127),
        f"{tag}: odd num_rffs and bad num_freqs": call(m=127, F=63),
        f"{tag}: bad num_freqs and R % P": call(F=63, R=96),
    }


CASES = {
    "fht: n == 0": fht(n=0),
    "fht: dim2 < 2": fht(dim2=1),
    "fht: dim2 not a power of 2": fht(dim2=48),
    "fht: dim1 < 1": fht(dim1=0),
    "fht f64: n == 0 and dim2 < 2": fht("f64", n=0, dim2=1),
    "fht f64: dim2 not a power of 2 and dim1 < 1": fht("f64", dim2=48, dim1=0),
    "srht: n == 0": srht(n=0),
    "srht: radem length": srht(rlen=32),
    "srht: dim < 2": srht(dim=1, rlen=1),
    "srht: dim not a power of 2": srht(dim=48, rlen=48),
    "srht f64: n == 0 and radem length": srht("f64", n=0, rlen=32),
    "srht f64: radem length and not a power of 2": srht("f64", dim=48, rlen=32),

    **_shared("rbf f32", rbf),
    **_shared("rbf f64", lambda **kw: rbf("f64", **kw)),
    "rbf f32: out_rows != n": rbf(out_rows=3),
    "rbf f32: R % P and misaligned out": rbf(R=96, out=A + 8),
    "rbf f32: misaligned out": rbf(out=A + 8),
    "rbf f64: misaligned out": rbf("f64", out=A + 8),
    "rbf f32: misaligned out and no workspace": rbf(out=A + 8, ws=None, wb=0),
    "rbf f32: no workspace": rbf(ws=None, wb=0),
    "rbf f32: workspace too small": rbf(wb=16),
    "rbf f32: padded width 65536 without the global scratch": rbf(d=40000, R=65536, ws=None, wb=0),
    **_shared("rbfgrad f32", rbfg),
    **_shared("rbfgrad f64", lambda **kw: rbfg("f64", **kw)),
    "rbfgrad f32: out_rows != n": rbfg(out_rows=3, gr=3),
    "rbfgrad f32: grad_rows": rbfg(gr=3),
    "rbfgrad f32: grad_cols": rbfg(gc=126),
    "rbfgrad f64: grad_cols": rbfg("f64", gc=126),
    "rbfgrad f32: bad num_freqs and grad_rows": rbfg(F=63, gr=3),
    "rbfgrad f32: grad_rows and R % P": rbfg(gr=3, R=96),
    "rbfgrad f64: grad_cols and R % P": rbfg("f64", gc=126, R=96),
    "rbfgrad f32: R % P and misaligned out": rbfg(R=96, out=A + 8),
    "rbfgrad f32: misaligned out and no workspace": rbfg(out=A + 8, ws=None, wb=0),
    "rbfgrad f32: no workspace and misaligned grad": rbfg(ws=None, wb=0, grad=A + 8),
    "rbfgrad f32: misaligned grad": rbfg(grad=A + 8),

    **_shared("gradrows", rbfgr),
    "gradrows: padded width > 8192": rbfgr(d=9000, R=16384),
    "gradrows: R % P and padded width > 8192": rbfgr(d=9000, R=8192),
    "gradrows: padded width > 8192 and misaligned rows": rbfgr(d=9000, R=16384, z=A + 4),
    "gradrows: zrows 4-byte aligned": rbfgr(z=A + 4),
    "gradrows: grows 4-byte aligned": rbfgr(g=A + 4),
    "gradrows: zrows NULL": rbfgr(z=None),
    "gradrows: R % P and misaligned rows": rbfgr(R=96, g=A + 4),
    "gradrows: misaligned rows and no workspace": rbfgr(g=A + 4, ws=None, wb=0),
    "gradrows: no workspace": rbfgr(ws=None, wb=0),
    "gradrows: workspace too small": rbfgr(wb=16),
    "gradrows: too many datapoints": rbfgr(n=1 << 34),
    "gradrows: no workspace and too many datapoints": rbfgr(n=1 << 34, ws=None, wb=0),
    "gradrows: wide rows, radem 8 bytes off": rbfgr(d=2000, R=2048, radem=A + 8),
    "gradrows: wide rows, misaligned rows and radem": rbfgr(d=2000, R=2048, radem=A + 8, z=A + 4),

    **_shared("cache", cache),
    "cache: no workspace": cache(ws=None, wb=0),
    "cache: workspace too small": cache(wb=16),
    "cache: zc 4-byte aligned": cache(zc=A + 4),
    "cache: R % P and no workspace": cache(R=96, ws=None, wb=0),
    "cache: no workspace and misaligned zc": cache(ws=None, wb=0, zc=A + 4),
    "cache: input width beyond 2^31 - 1": cache(d=(1 << 31) + 5, R=1 << 32, wb=1 << 40),
    "cache: misaligned zc and input width beyond 2^31 - 1": cache(d=(1 << 31) + 5, R=1 << 32, wb=1 << 40, zc=A + 4),

    **_shared("ztz", ztz),
    **_shared("zty", zty),
    "ztz: padded width > 4096": ztz(d=5000, R=8192),
    "ztz: R % P and padded width > 4096": ztz(d=5000, R=4096),
    "ztz: num_freqs > 65536": ztz(m=2 * 65600, F=65600, R=65664),
    "ztz: padded width > 4096 and num_freqs > 65536": ztz(d=5000, m=2 * 65600, F=65600, R=73728),
    "ztz: misaligned v": ztz(v=A + 8),
    "ztz: misaligned w": ztz(w=A + 8),
    "zty: y only 8-byte aligned passes, w does not": zty(v=A + 8, w=A + 8),
    "zty: y only 8-byte aligned, no workspace": zty(v=A + 8, ws=None, wb=0),
    "ztz: num_freqs > 65536 and misaligned w": ztz(m=2 * 65600, F=65600, R=65664, w=A + 8),
    "ztz: misaligned w and no workspace": ztz(w=A + 8, ws=None, wb=0),
    "ztz: no workspace": ztz(ws=None, wb=0),
    "ztz: workspace too small": ztz(wb=4096),
    "ztz: workspace 8 bytes off": ztz(ws=A + 8),
    "zty: workspace too small": zty(wb=4096),

    # ---- sequences
    "conv f32: n == 0": conv(n=0, out_rows=0, nseq=0),
    "conv f32: out_rows != n": conv(out_rows=3),
    "conv f64: odd num_rffs": conv("f64", m=127),
    "conv f32: 2 num_freqs != num_rffs": conv(F=63),
    "conv f32: num_freqs > R": conv(m=256, F=128),
    "conv f32: nseq != n": conv(nseq=3),
    "conv f32: L < conv_width": conv(cw=13),
    "conv f32: conv_width 0": conv(cw=0),
    "conv f32: R % P": conv(R=80),
    "conv f64: R % P": conv("f64", R=80),
    "conv f32: seqlen_host NULL": conv(sh=None),
    "conv f32: a sequence shorter than conv_width": conv(sh=SL_SHORT),
    "conv f64: a sequence longer than L": conv("f64", sh=SL_LONG),
    "conv f32: seqlen_dev NULL": conv(sd=None),
    "conv f32: misaligned out": conv(out=A + 8),
    "conv f32: no workspace": conv(ws=None, wb=0),
    "conv f32: n == 0 and odd num_rffs": conv(n=0, out_rows=0, nseq=0, m=127),
    "conv f32: odd num_rffs and bad num_freqs": conv(m=127, F=63),
    "conv f32: bad num_freqs and nseq": conv(F=63, nseq=3),
    "conv f32: nseq and conv_width": conv(nseq=3, cw=13),
    "conv f32: conv_width and R % P": conv(cw=0, R=80),
    "conv f32: R % P and a short sequence": conv(R=80, sh=SL_SHORT),
    "conv f32: a short sequence and seqlen_dev NULL": conv(sh=SL_SHORT, sd=None),
    "conv f32: seqlen_dev NULL and misaligned out": conv(sd=None, out=A + 8),
    "conv f32: misaligned out and no workspace": conv(out=A + 8, ws=None, wb=0),
    "convgrad f32: grad_rows": convg(gr=3),
    "convgrad f64: grad_cols": convg("f64", gc=126),
    "convgrad f32: bad num_freqs and grad_cols": convg(F=63, gc=126),
    "convgrad f32: grad_cols and nseq": convg(gc=126, nseq=3),
    "convgrad f32: grad_cols and R % P": convg(gc=126, R=80),
    "convgrad f32: misaligned out and grad": convg(out=A + 8, grad=A + 8),
    "convgrad f32: misaligned grad": convg(grad=A + 8),
    "convgrad f32: misaligned grad and no workspace": convg(grad=A + 8, ws=None, wb=0),
    "convgrad f32: a long sequence": convg(sh=SL_LONG),
    "convrows: n == 0": convr(n=0, nseq=0),
    "convrows: odd num_rffs": convr(m=127),
    "convrows: bad num_freqs": convr(F=63),
    "convrows: R % P": convr(R=80),
    "convrows: rows NULL": convr(zc=None),
    "convrows: rows 4-byte aligned": convr(zc=A + 4),
    "convrows: rows 8-byte aligned, no workspace": convr(zc=A + 8, ws=None, wb=0),
    "convrows: seqlen_dev NULL and misaligned rows": convr(sd=None, zc=A + 4),
    "convrows: a short sequence and misaligned rows": convr(sh=SL_SHORT, zc=A + 4),
    "convrows: misaligned rows and no workspace": convr(zc=A + 4, ws=None, wb=0),
    "convrows: staged (windows of 8192) without a workspace": convr(Cc=2500, cw=2, R=8192, ws=None, wb=0),
    "convrows: staged, workspace without room for one row": convr(Cc=2500, cw=2, R=8192, wb=4096),
    "convgradrows: n == 0": convgr(n=0, nseq=0),
    "convgradrows: bad num_freqs": convgr(F=63),
    "convgradrows: R % P": convgr(R=80),
    "convgradrows: zrows 4-byte aligned": convgr(z=A + 4),
    "convgradrows: grows NULL": convgr(g=None),
    "convgradrows: grows 4-byte aligned": convgr(g=A + 4),
    "convgradrows: both rows misaligned": convgr(z=A + 4, g=A + 4),
    "convgradrows: misaligned grows and no workspace": convgr(g=A + 4, ws=None, wb=0),
    "convgradrows: no workspace": convgr(ws=None, wb=0),
    "convgradrows: staged (windows of 8192) without a workspace": convgr(Cc=2500, cw=2, R=8192, ws=None, wb=0),
    "convgradrows: staged, workspace without room for two rows": convgr(Cc=2500, cw=2, R=8192, wb=4096),
    "convgradrows: staged, workspace 8 bytes off": convgr(Cc=2500, cw=2, R=8192, ws=A + 8),
    "maxpool f32: n == 0": pool(n=0, out_rows=0, nseq=0),
    "maxpool f32: odd num_rffs": pool(m=63, F=63),
    "maxpool f32: num_freqs != num_rffs": pool(F=32),
    "maxpool f64: num_freqs > R": pool("f64", m=128, F=128),
    "maxpool f32: R % P": pool(R=80),
    "maxpool f32: R beyond the repetitions": pool(R=96),
    "maxpool f64: R beyond the repetitions": pool("f64", R=128),
    "maxpool f32: odd num_rffs and num_freqs": pool(m=63, F=32),
    "maxpool f32: num_freqs and nseq": pool(F=32, nseq=3),
    "maxpool f32: R beyond the repetitions and a short sequence": pool(R=96, sh=SL_SHORT),
    "maxpool f32: seqlen_dev NULL": pool(sd=None),
    "maxpool f32: no workspace": pool(ws=None, wb=0),

    # ---- float32 feature rows
    "zmatvec: n == 0": zmv(n=0),
    "zmatvec: odd num_rffs": zmv(m=127),
    "zmatvec: num_freqs > 16384": zmv(m=2 * 16386),
    "zmatvec: misaligned v": zmv(v=A + 8),
    "zmatvec: misaligned zc": zmv(zc=A + 8),
    "zmatvec: no workspace": zmv(ws=None, wb=0),
    "zmatvec: workspace too small": zmv(wb=4096),
    "zmatvec: n == 0 and odd num_rffs": zmv(n=0, m=127),
    "zmatvec: num_freqs > 16384 and misaligned w": zmv(m=2 * 16386, w=A + 8),
    "zmatvec: misaligned w and no workspace": zmv(w=A + 8, ws=None, wb=0),
    "zmatvec scaled: scale 0": zmvs(scale=0.0),
    "zmatvec scaled: scale 0 and n == 0": zmvs(scale=0.0, n=0),
    "zmatvec scaled: n == 0": zmvs(n=0),
    "zcache zty: n == 0": zzty(n=0),
    "zcache zty: odd num_rffs": zzty(m=127),
    "zcache zty: y 4-byte aligned": zzty(y=A + 4),
    "zcache zty: 8-byte aligned pointers, no workspace": zzty(zc=A + 8, y=A + 8, out=A + 8, ws=None, wb=0),
    "zcache zty: workspace too small": zzty(wb=4096),
    "zcache zty: workspace 8 bytes off": zzty(ws=A + 8),
    "zcache zty: odd num_rffs and misaligned out": zzty(m=127, out=A + 4),
    **{f"zblock {w}: {what}": zblock(w, **kw) for w in ("matvec", "project", "backproject") for what, kw in (
        ("n == 0", dict(n=0)), ("num_rffs no multiple of 4", dict(m=126)), ("k == 0", dict(k=0)), ("k == 33", dict(k=33)),
        ("zc 8 bytes off", dict(zc=A + 8)), ("n == 0 and k == 33", dict(n=0, k=33)), ("num_rffs and k", dict(m=126, k=33)),
        ("k == 33 and misaligned zc", dict(k=33, zc=A + 8)))},

    **{f"ard {s}: {what}": ard(s, **kw) for s in ("f32", "f64") for what, kw in (
        ("n == 0", dict(n=0, out_rows=0, gr=0)), ("out_rows != n", dict(out_rows=3)), ("grad_rows", dict(gr=3)),
        ("grad_cols", dict(gc=126)), ("w_cols != d", dict(w_cols=7)), ("num_rffs != 2 num_freqs", dict(F=63)),
        ("map_len != w_cols", dict(map_len=7)), ("sig_len != map_len", dict(sig_len=7)), ("no lengthscales", dict(nls=0)),
        ("nine lengthscales", dict(nls=9)), ("too many datapoints", dict(n=4 * 65536, out_rows=4 * 65536, gr=4 * 65536)),
        ("n == 0 and grad_cols", dict(n=0, out_rows=0, gr=0, gc=126)), ("sig_len and nine lengthscales", dict(sig_len=7, nls=9)),
        ("nine lengthscales and too many datapoints", dict(nls=9, n=4 * 65536, out_rows=4 * 65536, gr=4 * 65536)))},

    **{f"sample {s}: {what}": sample(s, **kw) for s in ("f32", "f64") for what, kw in (
        ("n == 0", dict(n=0)), ("m == 0", dict(m=0)), ("P not a power of 2", dict(P=96)), ("m > P", dict(m=128)),
        ("ncols == 0", dict(ncols=0)), ("ncols > P", dict(ncols=65, ldo=65)), ("ldo < ncols", dict(ldo=7)),
        ("row beyond LDS", dict(P=65536)), ("n == 0 and P", dict(n=0, P=96)), ("P and ncols", dict(P=96, ncols=0)),
        ("ncols and row beyond LDS", dict(P=65536, ncols=0)))},
    **{f"samplerows: {what}": samplerows(**kw) for what, kw in (
        ("n == 0", dict(n=0)), ("m == 0", dict(m=0)), ("P not a power of 2", dict(P=96)), ("m > P", dict(m=128)),
        ("ncols == 0", dict(ncols=0)), ("ldo < ncols", dict(ldo=7)), ("more than 4 blocks", dict(P=65536)),
        ("blocks x columns beyond LDS", dict(P=16384, ncols=4097, ldo=4097)),
        ("blocks with z^T y, m % 4", dict(P=16384, m=130, y=A, zty_out=A)),
        ("n == 0 and P", dict(n=0, P=96)), ("P and ncols", dict(P=96, ncols=0)), ("ncols and blocks", dict(P=65536, ncols=0)),
        ("blocks and m % 4", dict(P=65536, m=130, y=A, zty_out=A)))},

    **{f"sketch gemm: {what}": skg(**kw) for what, kw in (
        ("n == 0", dict(n=0)), ("num_rffs < 2", dict(m=0)), ("I < 1", dict(I=0)), ("odd num_rffs", dict(m=127)),
        ("lda < I", dict(I=65)), ("lda no multiple of 64", dict(lda=96)), ("bt, num_rffs % 4", dict(bt=1, m=126, ldc=32)),
        ("ldc < J", dict(ldc=126)), ("ldc < I, transposed", dict(trans=1, ldc=6)), ("odd ldc", dict(ldc=129)),
        ("A 8 bytes off", dict(a=A + 8)), ("zc 8 bytes off", dict(zc=A + 8)), ("C 8 bytes off", dict(c=A + 8)),
        ("n == 0 and odd num_rffs", dict(n=0, m=127)), ("odd num_rffs and lda", dict(m=127, lda=96)),
        ("lda and bt", dict(lda=96, bt=1, m=126)), ("bt and ldc", dict(bt=1, m=126, ldc=6)), ("ldc and alignment", dict(ldc=126, c=A + 8)))},
    **{f"gram: {what}": gram(**kw) for what, kw in (
        ("n == 0", dict(n=0)), ("msub < 1", dict(msub=0)), ("msub > num_rffs", dict(msub=256)), ("odd num_rffs", dict(m=129)),
        ("msub % 128", dict(msub=64)), ("num_rffs % 4", dict(m=130)), ("ldc < msub", dict(ldc=126)), ("odd ldc", dict(ldc=129)),
        ("zc 8 bytes off", dict(zc=A + 8)), ("C 8 bytes off", dict(c=A + 8)), ("n == 0 and odd num_rffs", dict(n=0, m=129)),
        ("odd num_rffs and msub", dict(m=129, msub=64)), ("msub and ldc", dict(msub=64, ldc=62)), ("ldc and alignment", dict(ldc=126, c=A + 8)))},
    **{f"cross gram: {what}": xgram(**kw) for what, kw in (
        ("n == 0", dict(n=0)), ("num_rffs < 2", dict(m=0)), ("num_rffs % 128", dict(m=192)), ("ldc < num_rffs", dict(ldc=126)),
        ("odd ldc", dict(ldc=129)), ("A NULL", dict(a=None)), ("B 8 bytes off", dict(b=A + 8)), ("C 8 bytes off", dict(c=A + 8)),
        ("n == 0 and num_rffs % 128", dict(n=0, m=192)), ("num_rffs % 128 and ldc", dict(m=192, ldc=190)),
        ("ldc and alignment", dict(ldc=126, b=A + 8)))},
}

# (code, xgpr_last_error()) of every row, recorded from the build BEFORE the launchers were refactored -- literals, never regenerated
EXPECTED = {
    'fht: n == 0': (-1, 'no datapoints'),
    'fht: dim2 < 2': (-9, 'last dim not power of 2 > 1'),
    'fht: dim2 not a power of 2': (-9, 'last dim not power of 2'),
    'fht: dim1 < 1': (-8, 'incorrect array dims passed'),
    'fht f64: n == 0 and dim2 < 2': (-1, 'no datapoints'),
    'fht f64: dim2 not a power of 2 and dim1 < 1': (-9, 'last dim not power of 2'),
    'srht: n == 0': (-1, 'no datapoints'),
    'srht: radem length': (-8, 'incorrect array dims passed'),
    'srht: dim < 2': (-9, 'last dim not power of 2 > 1'),
    'srht: dim not a power of 2': (-9, 'last dim not power of 2'),
    'srht f64: n == 0 and radem length': (-1, 'no datapoints'),
    'srht f64: radem length and not a power of 2': (-8, 'incorrect array dims passed'),
    'rbf f32: n == 0': (-1, 'no datapoints'),
    'rbf f32: odd num_rffs': (-2, 'last dim of output must be even number'),
    'rbf f32: num_rffs < 2': (-2, 'last dim of output must be even number'),
    'rbf f32: 2 num_freqs != num_rffs': (-3, 'incorrect number of rffs and or freqs.'),
    'rbf f32: num_freqs > R': (-3, 'incorrect number of rffs and or freqs.'),
    'rbf f32: R % P': (-3, 'incorrect number of rffs and or freqs.'),
    'rbf f32: n == 0 and odd num_rffs': (-1, 'no datapoints'),
    'rbf f32: odd num_rffs and bad num_freqs': (-2, 'last dim of output must be even number'),
    'rbf f32: bad num_freqs and R % P': (-3, 'incorrect number of rffs and or freqs.'),
    'rbf f64: n == 0': (-1, 'no datapoints'),
    'rbf f64: odd num_rffs': (-2, 'last dim of output must be even number'),
    'rbf f64: num_rffs < 2': (-2, 'last dim of output must be even number'),
    'rbf f64: 2 num_freqs != num_rffs': (-3, 'incorrect number of rffs and or freqs.'),
    'rbf f64: num_freqs > R': (-3, 'incorrect number of rffs and or freqs.'),
    'rbf f64: R % P': (-3, 'incorrect number of rffs and or freqs.'),
    'rbf f64: n == 0 and odd num_rffs': (-1, 'no datapoints'),
    'rbf f64: odd num_rffs and bad num_freqs': (-2, 'last dim of output must be even number'),
    'rbf f64: bad num_freqs and R % P': (-3, 'incorrect number of rffs and or freqs.'),
    'rbf f32: out_rows != n': (-1, 'no datapoints'),
    'rbf f32: R % P and misaligned out': (-3, 'incorrect number of rffs and or freqs.'),
    'rbf f32: misaligned out': (-21, 'output pointer must be 16-byte aligned'),
    'rbf f64: misaligned out': (-21, 'output pointer must be 16-byte aligned'),
    'rbf f32: misaligned out and no workspace': (-21, 'output pointer must be 16-byte aligned'),
    'rbf f32: no workspace': (-21, 'workspace too small (see xgpr_rbf_workspace_bytes)'),
    'rbf f32: workspace too small': (-21, 'workspace too small (see xgpr_rbf_workspace_bytes)'),
    'rbf f32: padded width 65536 without the global scratch': (-21, 'workspace too small (see xgpr_sorf_workspace_bytes)'),
    'rbfgrad f32: n == 0': (-1, 'no datapoints'),
    'rbfgrad f32: odd num_rffs': (-2, 'last dim of output must be even number'),
    'rbfgrad f32: num_rffs < 2': (-2, 'last dim of output must be even number'),
    'rbfgrad f32: 2 num_freqs != num_rffs': (-3, 'incorrect number of rffs and or freqs.'),
    'rbfgrad f32: num_freqs > R': (-3, 'incorrect number of rffs and or freqs.'),
    'rbfgrad f32: R % P': (-3, 'incorrect number of rffs and or freqs.'),
    'rbfgrad f32: n == 0 and odd num_rffs': (-1, 'no datapoints'),
    'rbfgrad f32: odd num_rffs and bad num_freqs': (-2, 'last dim of output must be even number'),
    'rbfgrad f32: bad num_freqs and R % P': (-3, 'incorrect number of rffs and or freqs.'),
    'rbfgrad f64: n == 0': (-1, 'no datapoints'),
    'rbfgrad f64: odd num_rffs': (-2, 'last dim of output must be even number'),
    'rbfgrad f64: num_rffs < 2': (-2, 'last dim of output must be even number'),
    'rbfgrad f64: 2 num_freqs != num_rffs': (-3, 'incorrect number of rffs and or freqs.'),
    'rbfgrad f64: num_freqs > R': (-3, 'incorrect number of rffs and or freqs.'),
    'rbfgrad f64: R % P': (-3, 'incorrect number of rffs and or freqs.'),
    'rbfgrad f64: n == 0 and odd num_rffs': (-1, 'no datapoints'),
    'rbfgrad f64: odd num_rffs and bad num_freqs': (-2, 'last dim of output must be even number'),
    'rbfgrad f64: bad num_freqs and R % P': (-3, 'incorrect number of rffs and or freqs.'),
    'rbfgrad f32: out_rows != n': (-1, 'no datapoints'),
    'rbfgrad f32: grad_rows': (-4, 'Wrong array sizes.'),
    'rbfgrad f32: grad_cols': (-4, 'Wrong array sizes.'),
    'rbfgrad f64: grad_cols': (-4, 'Wrong array sizes.'),
    'rbfgrad f32: bad num_freqs and grad_rows': (-3, 'incorrect number of rffs and or freqs.'),
    'rbfgrad f32: grad_rows and R % P': (-4, 'Wrong array sizes.'),
    'rbfgrad f64: grad_cols and R % P': (-4, 'Wrong array sizes.'),
    'rbfgrad f32: R % P and misaligned out': (-3, 'incorrect number of rffs and or freqs.'),
    'rbfgrad f32: misaligned out and no workspace': (-21, 'output pointer must be 16-byte aligned'),
    'rbfgrad f32: no workspace and misaligned grad': (-21, 'workspace too small (see xgpr_rbf_workspace_bytes)'),
    'rbfgrad f32: misaligned grad': (-21, 'gradient pointer must be 16-byte aligned'),
    'gradrows: n == 0': (-1, 'no datapoints'),
    'gradrows: odd num_rffs': (-2, 'last dim of output must be even number'),
    'gradrows: num_rffs < 2': (-2, 'last dim of output must be even number'),
    'gradrows: 2 num_freqs != num_rffs': (-3, 'incorrect number of rffs and or freqs.'),
    'gradrows: num_freqs > R': (-3, 'incorrect number of rffs and or freqs.'),
    'gradrows: R % P': (-3, 'incorrect number of rffs and or freqs.'),
    'gradrows: n == 0 and odd num_rffs': (-1, 'no datapoints'),
    'gradrows: odd num_rffs and bad num_freqs': (-2, 'last dim of output must be even number'),
    'gradrows: bad num_freqs and R % P': (-3, 'incorrect number of rffs and or freqs.'),
    'gradrows: padded width > 8192': (-20, 'the gradient rows: no plan at padded width > 8192'),
    'gradrows: R % P and padded width > 8192': (-3, 'incorrect number of rffs and or freqs.'),
    'gradrows: padded width > 8192 and misaligned rows': (-20, 'the gradient rows: no plan at padded width > 8192'),
    'gradrows: zrows 4-byte aligned': (-21, 'row pointers must be 8-byte aligned'),
    'gradrows: grows 4-byte aligned': (-21, 'row pointers must be 8-byte aligned'),
    'gradrows: zrows NULL': (-21, 'row pointers must be 8-byte aligned'),
    'gradrows: R % P and misaligned rows': (-3, 'incorrect number of rffs and or freqs.'),
    'gradrows: misaligned rows and no workspace': (-21, 'row pointers must be 8-byte aligned'),
    'gradrows: no workspace': (-21, 'workspace too small (see xgpr_rbf_workspace_bytes)'),
    'gradrows: workspace too small': (-21, 'workspace too small (see xgpr_rbf_workspace_bytes)'),
    'gradrows: too many datapoints': (-20, 'too many datapoints for one launch'),
    'gradrows: no workspace and too many datapoints': (-21, 'workspace too small (see xgpr_rbf_workspace_bytes)'),
    'gradrows: wide rows, radem 8 bytes off': (-20, 'the gradient rows: the wave tiles read the Rademacher array 16 bytes at a time'),
    'gradrows: wide rows, misaligned rows and radem': (-21, 'row pointers must be 8-byte aligned'),
    'cache: n == 0': (-1, 'no datapoints'),
    'cache: odd num_rffs': (-2, 'last dim of output must be even number'),
    'cache: num_rffs < 2': (-2, 'last dim of output must be even number'),
    'cache: 2 num_freqs != num_rffs': (-3, 'incorrect number of rffs and or freqs.'),
    'cache: num_freqs > R': (-3, 'incorrect number of rffs and or freqs.'),
    'cache: R % P': (-3, 'incorrect number of rffs and or freqs.'),
    'cache: n == 0 and odd num_rffs': (-1, 'no datapoints'),
    'cache: odd num_rffs and bad num_freqs': (-2, 'last dim of output must be even number'),
    'cache: bad num_freqs and R % P': (-3, 'incorrect number of rffs and or freqs.'),
    'cache: no workspace': (-21, 'workspace too small (see xgpr_rbf_workspace_bytes)'),
    'cache: workspace too small': (-21, 'workspace too small (see xgpr_rbf_workspace_bytes)'),
    'cache: zc 4-byte aligned': (-21, 'cache pointer must be 8-byte aligned'),
    'cache: R % P and no workspace': (-3, 'incorrect number of rffs and or freqs.'),
    'cache: no workspace and misaligned zc': (-21, 'workspace too small (see xgpr_rbf_workspace_bytes)'),
    'cache: input width beyond 2^31 - 1': (-20, 'the feature cache: input width beyond 2^31 - 1'),
    'cache: misaligned zc and input width beyond 2^31 - 1': (-21, 'cache pointer must be 8-byte aligned'),
    'ztz: n == 0': (-1, 'no datapoints'),
    'ztz: odd num_rffs': (-2, 'last dim of output must be even number'),
    'ztz: num_rffs < 2': (-2, 'last dim of output must be even number'),
    'ztz: 2 num_freqs != num_rffs': (-3, 'incorrect number of rffs and or freqs.'),
    'ztz: num_freqs > R': (-3, 'incorrect number of rffs and or freqs.'),
    'ztz: R % P': (-3, 'incorrect number of rffs and or freqs.'),
    'ztz: n == 0 and odd num_rffs': (-1, 'no datapoints'),
    'ztz: odd num_rffs and bad num_freqs': (-2, 'last dim of output must be even number'),
    'ztz: bad num_freqs and R % P': (-3, 'incorrect number of rffs and or freqs.'),
    'zty: n == 0': (-1, 'no datapoints'),
    'zty: odd num_rffs': (-2, 'last dim of output must be even number'),
    'zty: num_rffs < 2': (-2, 'last dim of output must be even number'),
    'zty: 2 num_freqs != num_rffs': (-3, 'incorrect number of rffs and or freqs.'),
    'zty: num_freqs > R': (-3, 'incorrect number of rffs and or freqs.'),
    'zty: R % P': (-3, 'incorrect number of rffs and or freqs.'),
    'zty: n == 0 and odd num_rffs': (-1, 'no datapoints'),
    'zty: odd num_rffs and bad num_freqs': (-2, 'last dim of output must be even number'),
    'zty: bad num_freqs and R % P': (-3, 'incorrect number of rffs and or freqs.'),
    'ztz: padded width > 4096': (-20, 'fused matvec supports padded width <= 4096'),
    'ztz: R % P and padded width > 4096': (-3, 'incorrect number of rffs and or freqs.'),
    'ztz: num_freqs > 65536': (-20, 'fused matvec supports num_freqs <= 65536'),
    'ztz: padded width > 4096 and num_freqs > 65536': (-20, 'fused matvec supports padded width <= 4096'),
    'ztz: misaligned v': (-21, 'vector pointers must be 16-byte aligned'),
    'ztz: misaligned w': (-21, 'vector pointers must be 16-byte aligned'),
    'zty: y only 8-byte aligned passes, w does not': (-21, 'vector pointers must be 16-byte aligned'),
    'zty: y only 8-byte aligned, no workspace': (-21, 'workspace too small (see xgpr_ztz_matvec_workspace_bytes)'),
    'ztz: num_freqs > 65536 and misaligned w': (-20, 'fused matvec supports num_freqs <= 65536'),
    'ztz: misaligned w and no workspace': (-21, 'vector pointers must be 16-byte aligned'),
    'ztz: no workspace': (-21, 'workspace too small (see xgpr_ztz_matvec_workspace_bytes)'),
    'ztz: workspace too small': (-21, 'workspace too small (see xgpr_ztz_matvec_workspace_bytes)'),
    'ztz: workspace 8 bytes off': (-21, 'workspace too small (see xgpr_ztz_matvec_workspace_bytes)'),
    'zty: workspace too small': (-21, 'workspace too small (see xgpr_ztz_matvec_workspace_bytes)'),
    'conv f32: n == 0': (-1, 'no datapoints'),
    'conv f32: out_rows != n': (-1, 'no datapoints'),
    'conv f64: odd num_rffs': (-2, 'last dim of output must be even number'),
    'conv f32: 2 num_freqs != num_rffs': (-3, 'incorrect number of rffs and or freqs.'),
    'conv f32: num_freqs > R': (-3, 'incorrect number of rffs and or freqs.'),
    'conv f32: nseq != n': (-5, 'wrong array sizes'),
    'conv f32: L < conv_width': (-6, 'invalid conv_width'),
    'conv f32: conv_width 0': (-6, 'invalid conv_width'),
    'conv f32: R % P': (-3, 'incorrect number of rffs and or freqs.'),
    'conv f64: R % P': (-3, 'incorrect number of rffs and or freqs.'),
    'conv f32: seqlen_host NULL': (-7, 'seqlen_host is required (sequence lengths are validated on the host)'),
    'conv f32: a sequence shorter than conv_width': (-7, 'All sequence lengths must be >= conv width and < array size.'),
    'conv f64: a sequence longer than L': (-7, 'All sequence lengths must be >= conv width and < array size.'),
    'conv f32: seqlen_dev NULL': (-21, 'seqlen_dev (device copy of the sequence lengths) is required'),
    'conv f32: misaligned out': (-21, 'output pointer must be 16-byte aligned'),
    'conv f32: no workspace': (-21, 'workspace too small (see xgpr_rbf_workspace_bytes)'),
    'conv f32: n == 0 and odd num_rffs': (-1, 'no datapoints'),
    'conv f32: odd num_rffs and bad num_freqs': (-2, 'last dim of output must be even number'),
    'conv f32: bad num_freqs and nseq': (-3, 'incorrect number of rffs and or freqs.'),
    'conv f32: nseq and conv_width': (-5, 'wrong array sizes'),
    'conv f32: conv_width and R % P': (-6, 'invalid conv_width'),
    'conv f32: R % P and a short sequence': (-3, 'incorrect number of rffs and or freqs.'),
    'conv f32: a short sequence and seqlen_dev NULL': (-7, 'All sequence lengths must be >= conv width and < array size.'),
    'conv f32: seqlen_dev NULL and misaligned out': (-21, 'seqlen_dev (device copy of the sequence lengths) is required'),
    'conv f32: misaligned out and no workspace': (-21, 'output pointer must be 16-byte aligned'),
    'convgrad f32: grad_rows': (-4, 'Wrong array sizes.'),
    'convgrad f64: grad_cols': (-4, 'Wrong array sizes.'),
    'convgrad f32: bad num_freqs and grad_cols': (-3, 'incorrect number of rffs and or freqs.'),
    'convgrad f32: grad_cols and nseq': (-4, 'Wrong array sizes.'),
    'convgrad f32: grad_cols and R % P': (-4, 'Wrong array sizes.'),
    'convgrad f32: misaligned out and grad': (-21, 'output pointer must be 16-byte aligned'),
    'convgrad f32: misaligned grad': (-21, 'gradient pointer must be 16-byte aligned'),
    'convgrad f32: misaligned grad and no workspace': (-21, 'gradient pointer must be 16-byte aligned'),
    'convgrad f32: a long sequence': (-7, 'All sequence lengths must be >= conv width and < array size.'),
    'convrows: n == 0': (-1, 'no datapoints'),
    'convrows: odd num_rffs': (-2, 'last dim of output must be even number'),
    'convrows: bad num_freqs': (-3, 'incorrect number of rffs and or freqs.'),
    'convrows: R % P': (-3, 'incorrect number of rffs and or freqs.'),
    'convrows: rows NULL': (-21, 'feature rows pointer must be 8-byte aligned'),
    'convrows: rows 4-byte aligned': (-21, 'feature rows pointer must be 8-byte aligned'),
    'convrows: rows 8-byte aligned, no workspace': (-21, 'workspace too small (see xgpr_rbf_workspace_bytes)'),
    'convrows: seqlen_dev NULL and misaligned rows': (-21, 'seqlen_dev (device copy of the sequence lengths) is required'),
    'convrows: a short sequence and misaligned rows': (-7, 'All sequence lengths must be >= conv width and < array size.'),
    'convrows: misaligned rows and no workspace': (-21, 'feature rows pointer must be 8-byte aligned'),
    'convrows: staged (windows of 8192) without a workspace': (-21, 'workspace too small (see xgpr_conv_feature_rows_workspace_bytes)'),
    'convrows: staged, workspace without room for one row': (-21, 'workspace too small (see xgpr_conv_feature_rows_workspace_bytes)'),
    'convgradrows: n == 0': (-1, 'no datapoints'),
    'convgradrows: bad num_freqs': (-3, 'incorrect number of rffs and or freqs.'),
    'convgradrows: R % P': (-3, 'incorrect number of rffs and or freqs.'),
    'convgradrows: zrows 4-byte aligned': (-21, 'feature rows pointer must be 8-byte aligned'),
    'convgradrows: grows NULL': (-21, 'gradient rows pointer must be 8-byte aligned'),
    'convgradrows: grows 4-byte aligned': (-21, 'gradient rows pointer must be 8-byte aligned'),
    'convgradrows: both rows misaligned': (-21, 'feature rows pointer must be 8-byte aligned'),
    'convgradrows: misaligned grows and no workspace': (-21, 'gradient rows pointer must be 8-byte aligned'),
    'convgradrows: no workspace': (-21, 'workspace too small (see xgpr_rbf_workspace_bytes)'),
    'convgradrows: staged (windows of 8192) without a workspace': (-21, 'workspace too small (see xgpr_conv_grad_rows_workspace_bytes)'),
    'convgradrows: staged, workspace without room for two rows': (-21, 'workspace too small (see xgpr_conv_grad_rows_workspace_bytes)'),
    'convgradrows: staged, workspace 8 bytes off': (-21, 'workspace too small (see xgpr_conv_grad_rows_workspace_bytes)'),
    'maxpool f32: n == 0': (-1, 'no datapoints'),
    'maxpool f32: odd num_rffs': (-2, 'last dim of output must be even number'),
    'maxpool f32: num_freqs != num_rffs': (-3, 'incorrect number of rffs and or freqs.'),
    'maxpool f64: num_freqs > R': (-3, 'incorrect number of rffs and or freqs.'),
    'maxpool f32: R % P': (-3, 'incorrect number of rffs and or freqs.'),
    'maxpool f32: R beyond the repetitions': (-3, 'incorrect number of rffs and or freqs.'),
    'maxpool f64: R beyond the repetitions': (-3, 'incorrect number of rffs and or freqs.'),
    'maxpool f32: odd num_rffs and num_freqs': (-2, 'last dim of output must be even number'),
    'maxpool f32: num_freqs and nseq': (-3, 'incorrect number of rffs and or freqs.'),
    'maxpool f32: R beyond the repetitions and a short sequence': (-3, 'incorrect number of rffs and or freqs.'),
    'maxpool f32: seqlen_dev NULL': (-21, 'seqlen_dev (device copy of the sequence lengths) is required'),
    'maxpool f32: no workspace': (-21, 'workspace too small (see xgpr_rbf_workspace_bytes)'),
    'zmatvec: n == 0': (-1, 'no datapoints'),
    'zmatvec: odd num_rffs': (-2, 'last dim of output must be even number'),
    'zmatvec: num_freqs > 16384': (-20, 'cached matvec supports num_freqs <= 16384'),
    'zmatvec: misaligned v': (-21, 'pointers must be 16-byte aligned'),
    'zmatvec: misaligned zc': (-21, 'pointers must be 16-byte aligned'),
    'zmatvec: no workspace': (-21, 'workspace too small (see xgpr_ztz_matvec_workspace_bytes)'),
    'zmatvec: workspace too small': (-21, 'workspace too small (see xgpr_ztz_matvec_workspace_bytes)'),
    'zmatvec: n == 0 and odd num_rffs': (-1, 'no datapoints'),
    'zmatvec: num_freqs > 16384 and misaligned w': (-20, 'cached matvec supports num_freqs <= 16384'),
    'zmatvec: misaligned w and no workspace': (-21, 'pointers must be 16-byte aligned'),
    'zmatvec scaled: scale 0': (-8, 'scale must be positive'),
    'zmatvec scaled: scale 0 and n == 0': (-8, 'scale must be positive'),
    'zmatvec scaled: n == 0': (-1, 'no datapoints'),
    'zcache zty: n == 0': (-1, 'no datapoints'),
    'zcache zty: odd num_rffs': (-2, 'last dim of output must be even number'),
    'zcache zty: y 4-byte aligned': (-21, 'cache, y and output pointers must be 8-byte aligned'),
    'zcache zty: 8-byte aligned pointers, no workspace': (-21, 'workspace too small (see xgpr_ztz_matvec_workspace_bytes)'),
    'zcache zty: workspace too small': (-21, 'workspace too small (see xgpr_ztz_matvec_workspace_bytes)'),
    'zcache zty: workspace 8 bytes off': (-21, 'workspace too small (see xgpr_ztz_matvec_workspace_bytes)'),
    'zcache zty: odd num_rffs and misaligned out': (-2, 'last dim of output must be even number'),
    'zblock matvec: n == 0': (-1, 'no datapoints'),
    'zblock matvec: num_rffs no multiple of 4': (-20, 'block matvec needs num_rffs to be a multiple of 4'),
    'zblock matvec: k == 0': (-20, 'block matvec takes 1..32 right-hand sides per call'),
    'zblock matvec: k == 33': (-20, 'block matvec takes 1..32 right-hand sides per call'),
    'zblock matvec: zc 8 bytes off': (-21, 'cache pointer must be 16-byte aligned'),
    'zblock matvec: n == 0 and k == 33': (-1, 'no datapoints'),
    'zblock matvec: num_rffs and k': (-20, 'block matvec needs num_rffs to be a multiple of 4'),
    'zblock matvec: k == 33 and misaligned zc': (-20, 'block matvec takes 1..32 right-hand sides per call'),
    'zblock project: n == 0': (-1, 'no datapoints'),
    'zblock project: num_rffs no multiple of 4': (-20, 'block matvec needs num_rffs to be a multiple of 4'),
    'zblock project: k == 0': (-20, 'block matvec takes 1..32 right-hand sides per call'),
    'zblock project: k == 33': (-20, 'block matvec takes 1..32 right-hand sides per call'),
    'zblock project: zc 8 bytes off': (-21, 'cache pointer must be 16-byte aligned'),
    'zblock project: n == 0 and k == 33': (-1, 'no datapoints'),
    'zblock project: num_rffs and k': (-20, 'block matvec needs num_rffs to be a multiple of 4'),
    'zblock project: k == 33 and misaligned zc': (-20, 'block matvec takes 1..32 right-hand sides per call'),
    'zblock backproject: n == 0': (-1, 'no datapoints'),
    'zblock backproject: num_rffs no multiple of 4': (-20, 'block matvec needs num_rffs to be a multiple of 4'),
    'zblock backproject: k == 0': (-20, 'block matvec takes 1..32 right-hand sides per call'),
    'zblock backproject: k == 33': (-20, 'block matvec takes 1..32 right-hand sides per call'),
    'zblock backproject: zc 8 bytes off': (-21, 'cache pointer must be 16-byte aligned'),
    'zblock backproject: n == 0 and k == 33': (-1, 'no datapoints'),
    'zblock backproject: num_rffs and k': (-20, 'block matvec needs num_rffs to be a multiple of 4'),
    'zblock backproject: k == 33 and misaligned zc': (-20, 'block matvec takes 1..32 right-hand sides per call'),
    'ard f32: n == 0': (-1, 'no datapoints'),
    'ard f32: out_rows != n': (-1, 'no datapoints'),
    'ard f32: grad_rows': (-4, 'Wrong array sizes.'),
    'ard f32: grad_cols': (-4, 'Wrong array sizes.'),
    'ard f32: w_cols != d': (-4, 'Wrong array sizes.'),
    'ard f32: num_rffs != 2 num_freqs': (-4, 'Wrong array sizes.'),
    'ard f32: map_len != w_cols': (-4, 'Wrong array sizes.'),
    'ard f32: sig_len != map_len': (-4, 'Wrong array sizes.'),
    'ard f32: no lengthscales': (-20, 'MiniARD gradient supports up to 8 lengthscale groups'),
    'ard f32: nine lengthscales': (-20, 'MiniARD gradient supports up to 8 lengthscale groups'),
    'ard f32: too many datapoints': (-20, 'too many datapoints for one launch (chunk the input)'),
    'ard f32: n == 0 and grad_cols': (-1, 'no datapoints'),
    'ard f32: sig_len and nine lengthscales': (-4, 'Wrong array sizes.'),
    'ard f32: nine lengthscales and too many datapoints': (-20, 'MiniARD gradient supports up to 8 lengthscale groups'),
    'ard f64: n == 0': (-1, 'no datapoints'),
    'ard f64: out_rows != n': (-1, 'no datapoints'),
    'ard f64: grad_rows': (-4, 'Wrong array sizes.'),
    'ard f64: grad_cols': (-4, 'Wrong array sizes.'),
    'ard f64: w_cols != d': (-4, 'Wrong array sizes.'),
    'ard f64: num_rffs != 2 num_freqs': (-4, 'Wrong array sizes.'),
    'ard f64: map_len != w_cols': (-4, 'Wrong array sizes.'),
    'ard f64: sig_len != map_len': (-4, 'Wrong array sizes.'),
    'ard f64: no lengthscales': (-20, 'MiniARD gradient supports up to 8 lengthscale groups'),
    'ard f64: nine lengthscales': (-20, 'MiniARD gradient supports up to 8 lengthscale groups'),
    'ard f64: too many datapoints': (-20, 'too many datapoints for one launch (chunk the input)'),
    'ard f64: n == 0 and grad_cols': (-1, 'no datapoints'),
    'ard f64: sig_len and nine lengthscales': (-4, 'Wrong array sizes.'),
    'ard f64: nine lengthscales and too many datapoints': (-20, 'MiniARD gradient supports up to 8 lengthscale groups'),
    'sample f32: n == 0': (-8, 'incorrect array dims passed'),
    'sample f32: m == 0': (-8, 'incorrect array dims passed'),
    'sample f32: P not a power of 2': (-9, 'last dim not power of 2 > 1'),
    'sample f32: m > P': (-9, 'last dim not power of 2 > 1'),
    'sample f32: ncols == 0': (-8, 'incorrect array dims passed'),
    'sample f32: ncols > P': (-8, 'incorrect array dims passed'),
    'sample f32: ldo < ncols': (-8, 'incorrect array dims passed'),
    'sample f32: row beyond LDS': (-20, 'fused SRHT + sample needs the padded row to fit in LDS'),
    'sample f32: n == 0 and P': (-8, 'incorrect array dims passed'),
    'sample f32: P and ncols': (-9, 'last dim not power of 2 > 1'),
    'sample f32: ncols and row beyond LDS': (-8, 'incorrect array dims passed'),
    'sample f64: n == 0': (-8, 'incorrect array dims passed'),
    'sample f64: m == 0': (-8, 'incorrect array dims passed'),
    'sample f64: P not a power of 2': (-9, 'last dim not power of 2 > 1'),
    'sample f64: m > P': (-9, 'last dim not power of 2 > 1'),
    'sample f64: ncols == 0': (-8, 'incorrect array dims passed'),
    'sample f64: ncols > P': (-8, 'incorrect array dims passed'),
    'sample f64: ldo < ncols': (-8, 'incorrect array dims passed'),
    'sample f64: row beyond LDS': (-20, 'fused SRHT + sample needs the padded row to fit in LDS'),
    'sample f64: n == 0 and P': (-8, 'incorrect array dims passed'),
    'sample f64: P and ncols': (-9, 'last dim not power of 2 > 1'),
    'sample f64: ncols and row beyond LDS': (-8, 'incorrect array dims passed'),
    'samplerows: n == 0': (-8, 'incorrect array dims passed'),
    'samplerows: m == 0': (-8, 'incorrect array dims passed'),
    'samplerows: P not a power of 2': (-9, 'last dim not power of 2 > 1'),
    'samplerows: m > P': (-9, 'last dim not power of 2 > 1'),
    'samplerows: ncols == 0': (-8, 'incorrect array dims passed'),
    'samplerows: ldo < ncols': (-8, 'incorrect array dims passed'),
    'samplerows: more than 4 blocks': (-20, 'fused SRHT + sample: padded width x sampled columns beyond the LDS budget'),
    'samplerows: blocks x columns beyond LDS': (-20, 'fused SRHT + sample: padded width x sampled columns beyond the LDS budget'),
    'samplerows: blocks with z^T y, m % 4': (-20, 'fused SRHT + sample with z^T y: num_rffs must be a multiple of 4'),
    'samplerows: n == 0 and P': (-8, 'incorrect array dims passed'),
    'samplerows: P and ncols': (-9, 'last dim not power of 2 > 1'),
    'samplerows: ncols and blocks': (-8, 'incorrect array dims passed'),
    'samplerows: blocks and m % 4': (-20, 'fused SRHT + sample: padded width x sampled columns beyond the LDS budget'),
    'sketch gemm: n == 0': (-8, 'incorrect array dims passed'),
    'sketch gemm: num_rffs < 2': (-8, 'incorrect array dims passed'),
    'sketch gemm: I < 1': (-8, 'incorrect array dims passed'),
    'sketch gemm: odd num_rffs': (-2, 'last dim of output must be even number'),
    'sketch gemm: lda < I': (-8, 'sketch gemm: lda must be a multiple of 64 >= I'),
    'sketch gemm: lda no multiple of 64': (-8, 'sketch gemm: lda must be a multiple of 64 >= I'),
    'sketch gemm: bt, num_rffs % 4': (-20, 'sketch gemm (bt): num_rffs must be a multiple of 4'),
    'sketch gemm: ldc < J': (-8, 'sketch gemm: ldc too small (or odd for a row-major result)'),
    'sketch gemm: ldc < I, transposed': (-8, 'sketch gemm: ldc too small (or odd for a row-major result)'),
    'sketch gemm: odd ldc': (-8, 'sketch gemm: ldc too small (or odd for a row-major result)'),
    'sketch gemm: A 8 bytes off': (-21, 'pointers must be 16-byte aligned'),
    'sketch gemm: zc 8 bytes off': (-21, 'pointers must be 16-byte aligned'),
    'sketch gemm: C 8 bytes off': (-21, 'pointers must be 16-byte aligned'),
    'sketch gemm: n == 0 and odd num_rffs': (-8, 'incorrect array dims passed'),
    'sketch gemm: odd num_rffs and lda': (-2, 'last dim of output must be even number'),
    'sketch gemm: lda and bt': (-8, 'sketch gemm: lda must be a multiple of 64 >= I'),
    'sketch gemm: bt and ldc': (-20, 'sketch gemm (bt): num_rffs must be a multiple of 4'),
    'sketch gemm: ldc and alignment': (-8, 'sketch gemm: ldc too small (or odd for a row-major result)'),
    'gram: n == 0': (-8, 'incorrect array dims passed'),
    'gram: msub < 1': (-8, 'incorrect array dims passed'),
    'gram: msub > num_rffs': (-8, 'incorrect array dims passed'),
    'gram: odd num_rffs': (-2, 'last dim of output must be even number'),
    'gram: msub % 128': (-20, 'gram: msub must be a multiple of 128 and num_rffs of 4'),
    'gram: num_rffs % 4': (-20, 'gram: msub must be a multiple of 128 and num_rffs of 4'),
    'gram: ldc < msub': (-8, 'gram: ldc must be even and >= msub'),
    'gram: odd ldc': (-8, 'gram: ldc must be even and >= msub'),
    'gram: zc 8 bytes off': (-21, 'pointers must be 16-byte aligned'),
    'gram: C 8 bytes off': (-21, 'pointers must be 16-byte aligned'),
    'gram: n == 0 and odd num_rffs': (-8, 'incorrect array dims passed'),
    'gram: odd num_rffs and msub': (-2, 'last dim of output must be even number'),
    'gram: msub and ldc': (-20, 'gram: msub must be a multiple of 128 and num_rffs of 4'),
    'gram: ldc and alignment': (-8, 'gram: ldc must be even and >= msub'),
    'cross gram: n == 0': (-8, 'incorrect array dims passed'),
    'cross gram: num_rffs < 2': (-8, 'incorrect array dims passed'),
    'cross gram: num_rffs % 128': (-20, 'cross gram: num_rffs must be a multiple of 128'),
    'cross gram: ldc < num_rffs': (-8, 'cross gram: ldc must be even and >= num_rffs'),
    'cross gram: odd ldc': (-8, 'cross gram: ldc must be even and >= num_rffs'),
    'cross gram: A NULL': (-21, 'pointers must be 16-byte aligned'),
    'cross gram: B 8 bytes off': (-21, 'pointers must be 16-byte aligned'),
    'cross gram: C 8 bytes off': (-21, 'pointers must be 16-byte aligned'),
    'cross gram: n == 0 and num_rffs % 128': (-8, 'incorrect array dims passed'),
    'cross gram: num_rffs % 128 and ldc': (-20, 'cross gram: num_rffs must be a multiple of 128'),
    'cross gram: ldc and alignment': (-8, 'cross gram: ldc must be even and >= num_rffs'),
}


def run(fn, args):
    from xgpr_amd import _lib
    lib = _lib.load()
    rc = getattr(lib, fn)(*args)
    return int(rc), _lib.last_error()


def test_every_row_has_a_recorded_outcome_and_none_reached_the_device():
    assert sorted(CASES) == sorted(EXPECTED)
    for name, (code, msg) in EXPECTED.items():
        assert code < 0 and code != -100, (name, code, msg)          # XGPR_ERR_HIP: the row went past validation
        assert msg


def test_the_table_covers_every_entry_point_of_the_launchers():
    called = {fn for fn, _ in CASES.values()}
    assert called == {
        "xgpr_fht_f32", "xgpr_fht_f64", "xgpr_srht_f32", "xgpr_srht_f64", "xgpr_rbf_feature_gen_f32", "xgpr_rbf_feature_gen_f64",
        "xgpr_rbf_grad_f32", "xgpr_rbf_grad_f64", "xgpr_rbf_grad_rows_f32", "xgpr_rbf_feature_cache_f32", "xgpr_ztz_matvec_f32",
        "xgpr_zty_f32", "xgpr_conv1d_fgen_f32", "xgpr_conv1d_fgen_f64", "xgpr_conv_grad_f32", "xgpr_conv_grad_f64",
        "xgpr_conv_feature_rows_f32", "xgpr_conv_grad_rows_f32", "xgpr_conv1d_maxpool_f32", "xgpr_conv1d_maxpool_f64",
        "xgpr_zcache_matvec_f32", "xgpr_zcache_matvec_scaled_f32", "xgpr_zcache_zty_f32", "xgpr_zcache_block_matvec_f32",
        "xgpr_zcache_block_project_f32", "xgpr_zcache_block_backproject_f32", "xgpr_mini_ard_grad_f32", "xgpr_mini_ard_grad_f64",
        "xgpr_srht_sample_f32", "xgpr_srht_sample_f64", "xgpr_srht_sample_rows_f32", "xgpr_sketch_gemm_f64", "xgpr_ztz_gram_f64",
        "xgpr_cross_gram_f64"}


@pytest.mark.parametrize("name", sorted(CASES))
def test_validation_outcome(name):
    fn, args = CASES[name]
    assert run(fn, args) == EXPECTED[name], (name, fn)
