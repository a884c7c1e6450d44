#!/usr/bin/env python3
"""The two-layer kernel (Conv1dTwoLayer) with its first layer pooled once (``pool_first_layer`` True: ``DeviceDataset.pooled`` +
``Conv1dTwoLayerKernel.second_layer``, the fixed-vector solver path) against the route without it (False: every pass on the
two-layer kernel and the original dataset), at BASELINE configs[3]'s sequence shape -- one-hot protein-like sequences, L 64..512,
21 channels, conv_width 9 -- with init_rffs = 1024 and M = 8192 random features.

    python tools/bench_two_layer.py [--nseq 8192] [--reps 5] [--steps pool,cache,matvec,grad] [--out profiles/two_layer_pooled.json]

Needs a GPU (no fallback).  The driver itself never touches the GPU: every step runs in a process of its own under
``timeout -k 10 <limit>``, the steps are chained -- the first one that fails, faults or runs into its limit ends the run and no
later step is started -- and the parts the finished steps wrote are merged into the output file.

    pool     the first layer over the shard from the dense float32 array (hipConv1dMaxpool) and from tokens (hipConvTokenMaxpool),
             alternating after a warm-up of both; outputs compared bit for bit; peak device memory of one call of each
    cache    the resident feature cache at a new sigma: second layer over the pooled rows (hipRBFFeatureCache) against the two-layer
             kernel's own (float64 transform_x chunks rounded to float32), alternating over a list of sigmas
    matvec   one CG matvec Z^T (Z v): the pooled pair without a cache (the fused kernel, hipZtZMatvec) and with the resident cache,
             the two-layer kernel with its resident cache and without one
    grad     one exact_nmll_gradient evaluation at M = 2048, a new sigma every time: the pooled pair (the first evaluation pools)
             against the two-layer route

Timing: device events around each call in one process per step, the two routes alternating after a warm-up of both; medians and
min .. max are recorded -- a difference is read against the spread of the baseline's own rounds."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP_LIMITS_S = {"pool": 240, "cache": 300, "matvec": 300, "grad": 420}
L, C, CW, INIT_RFFS = 512, 21, 9, 1024
SIGMAS = (0.6, 0.7, 0.8, 0.9, 1.0, 1.1, 1.2)


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return out, e0.elapsed_time(e1)


def stats(ms):
    import numpy as np
    return {"ms": ms, "median_ms": float(np.median(ms)), "min_ms": min(ms), "max_ms": max(ms)}


def problem(nseq, m, tokens_too=True):
    import numpy as np
    from xgpr_amd.dataset import build_regression_dataset
    from xgpr_amd.kernels import make_kernel
    rng = np.random.default_rng(3)
    tokens = rng.integers(0, C, size=(nseq, L))
    lens = rng.integers(64, L + 1, size=nseq).astype(np.int32)
    y = rng.standard_normal(nseq)
    table = np.eye(C, dtype=np.float32)
    ds_dense = build_regression_dataset(table[tokens], y, lens, chunk_size=1024, device="cuda")
    ds_token = build_regression_dataset(tokens, y, lens, chunk_size=1024, device="cuda", token_table=table) if tokens_too else None
    kern = make_kernel("Conv1dTwoLayer", (nseq, L, C), m, 123, "cuda", {"conv_width": CW, "init_rffs": INIT_RFFS, "intercept": True})
    kern.set_hyperparams(np.array([1.0, 0.8]), logspace=False)
    return ds_dense, ds_token, kern, lens


def step_pool(args):
    import torch
    ds_dense, ds_token, kern, lens = problem(args.nseq, 8192)
    xd, xt = ds_dense.get_xdata(), ds_token.get_xdata()

    def one(x):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out, ms = timed(lambda: kern.pool(x, lens))
        return out, ms, torch.cuda.max_memory_allocated() - base

    pd, _, peak_dense = one(xd)
    pt, _, peak_token = one(xt)
    identical = bool(torch.equal(pd, pt))
    del pd, pt
    t_dense, t_token = [], []
    for _ in range(args.reps):
        t_dense.append(one(xd)[1])
        t_token.append(one(xt)[1])
    sd, st = stats(t_dense), stats(t_token)
    return {"what": "Conv1dTwoLayerKernel.pool over the shard: hipConv1dMaxpool on the dense float32 array, hipConvTokenMaxpool on tokens",
            "dense": sd, "token": st, "token_over_dense": st["median_ms"] / sd["median_ms"],
            "dense_spread_rel": (sd["max_ms"] - sd["min_ms"]) / sd["median_ms"], "bit_identical": identical,
            "kmers": int((lens.astype("int64") - CW + 1).sum()),
            "peak_bytes_during_call": {"dense": int(peak_dense), "token": int(peak_token), "pooled_rows": args.nseq * INIT_RFFS * 4},
            "input_bytes_resident": {"dense_x": args.nseq * L * C * 4, "tokens": args.nseq * L}}


def _set_sigma(kern, sigma):
    import numpy as np
    kern.set_hyperparams(np.array([1.0, sigma]), logspace=False)


def step_cache(args):
    ds, _, kern, _ = problem(args.nseq, 8192, tokens_too=False)
    second = kern.second_layer()
    pooled, pool_ms = timed(lambda: ds.pooled(kern))
    t_new, t_old = [], []
    for i, sigma in enumerate(SIGMAS[:args.reps + 1]):
        _set_sigma(kern, sigma)
        new_ms = timed(lambda: pooled.feature_cache(second))[1]
        old_ms = timed(lambda: ds.feature_cache(kern))[1]
        if i > 0:                                     # the first sigma is the warm-up of both
            t_new.append(new_ms)
            t_old.append(old_ms)
    sn, so = stats(t_new), stats(t_old)
    return {"what": "feature_cache at a new sigma, %d x 8192 float32 rows" % args.nseq, "first_layer_once_ms": pool_ms,
            "pooled_pair": sn, "two_layer": so, "pooled_over_two_layer": sn["median_ms"] / so["median_ms"],
            "two_layer_spread_rel": (so["max_ms"] - so["min_ms"]) / so["median_ms"],
            "pooled_bytes": {"rows": args.nseq * INIT_RFFS * 4, "sigma_scaled_copy": args.nseq * INIT_RFFS * 4}}


def step_matvec(args):
    import torch
    from xgpr_amd.cg import ConjugateGrad, rows_matvec_ok
    ds, _, kern, _ = problem(args.nseq, 8192, tokens_too=False)
    second, pooled = kern.second_layer(), ds.pooled(kern)
    m = kern.get_num_rffs()
    v = torch.randn(m, generator=torch.Generator(device="cuda").manual_seed(5), device="cuda", dtype=torch.float64)
    routes = {"pooled_pair_fused_no_cache": (ConjugateGrad(ds.comm, False), pooled, second),
              "pooled_pair_resident_cache": (ConjugateGrad(ds.comm, True), pooled, second),
              "two_layer_resident_cache": (ConjugateGrad(ds.comm, True), ds, kern),
              "two_layer_no_cache": (ConjugateGrad(ds.comm, False), ds, kern)}

    def apply(op, d, k, out):
        """Z^T (Z v) without the ridge term, by the entry ConjugateGrad.fit takes for this kernel and cache mode."""
        if k.fused_ok() or rows_matvec_ok(k, d) or op._use_cache(k, d):
            op._ztz(d, k, v, out)
        else:
            col = out[:, None]
            op._matvec(d, k, v[:, None].contiguous(), col, add_ridge=False)

    outs, times = {}, {name: [] for name in routes}
    for name, (op, d, k) in routes.items():           # warm-up: builds the caches, packs the masks
        outs[name] = torch.empty_like(v)
        apply(op, d, k, outs[name])
    for _ in range(args.reps):
        for name, (op, d, k) in routes.items():
            times[name].append(timed(lambda: apply(op, d, k, outs[name]))[1])
    ref = outs["two_layer_no_cache"]
    res = {name: dict(stats(t), rel_diff_to_two_layer_no_cache=float((outs[name] - ref).abs().max() / ref.abs().max()))
           for name, t in times.items()}
    res["what"] = "one CG matvec Z^T (Z v), %d sequences, M = 8192, init_rffs = %d" % (args.nseq, INIT_RFFS)
    return res


def step_grad(args):
    from xgpr_amd import nmll
    ds, _, kern, _ = problem(args.nseq, 2048, tokens_too=False)
    second = kern.second_layer()
    t_new, t_old, scores = [], [], []
    first_new = None
    for i, sigma in enumerate(SIGMAS[:args.reps + 1]):
        _set_sigma(kern, sigma)
        (s_new, _), new_ms = timed(lambda: nmll.exact_nmll_gradient(second, ds.pooled(kern)))
        (s_old, _), old_ms = timed(lambda: nmll.exact_nmll_gradient(kern, ds))
        scores.append((s_new, s_old))
        if i == 0:
            first_new = new_ms                        # includes the one pass of the first layer
        else:
            t_new.append(new_ms)
            t_old.append(old_ms)
    sn, so = stats(t_new), stats(t_old)
    return {"what": "one exact_nmll_gradient evaluation at a new sigma, %d sequences, M = 2048" % args.nseq,
            "pooled_pair": sn, "pooled_pair_first_evaluation_ms": first_new, "two_layer": so,
            "pooled_over_two_layer": sn["median_ms"] / so["median_ms"],
            "two_layer_spread_rel": (so["max_ms"] - so["min_ms"]) / so["median_ms"],
            "max_rel_score_diff": max(abs(a - b) / abs(b) for a, b in scores)}


STEPS = {"pool": step_pool, "cache": step_cache, "matvec": step_matvec, "grad": step_grad}


def run_step(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_two_layer.py needs a GPU")
    out = STEPS[args.step](args)
    out["device"] = torch.cuda.get_device_name(0)
    with open(args.part, "w") as f:
        json.dump(out, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nseq", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", default="pool,cache,matvec,grad")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "two_layer_pooled.json"))
    ap.add_argument("--step", choices=sorted(STEPS), help="(internal) run one step in this process")
    ap.add_argument("--part", help="(internal) where the step writes its figures")
    args = ap.parse_args()
    if args.reps < 1 or args.reps + 1 > len(SIGMAS):
        raise SystemExit("--reps must be 1 .. %d" % (len(SIGMAS) - 1))
    if args.step:
        return run_step(args)
    out = {"workload": "Conv1dTwoLayer at BASELINE configs[3]'s sequence shape: %d sequences (L 64..512, one-hot 21 channels, "
                       "conv_width 9), init_rffs %d; pool_first_layer True (pooled pair) against False (two-layer route)"
                       % (args.nseq, INIT_RFFS),
           "reps": args.reps,
           "timing": "device events around each call, one process per step, the routes alternating after a warm-up of each",
           "steps": {}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        for name in args.steps.split(","):
            part = os.path.join(tmp, name + ".json")
            cmd = ["timeout", "-k", "10", str(STEP_LIMITS_S[name]), sys.executable, os.path.abspath(__file__), "--step", name,
                   "--part", part, "--nseq", str(args.nseq), "--reps", str(args.reps)]
            rc = subprocess.run(cmd).returncode
            if rc != 0:                               # a failure, a fault or the time limit: nothing more is started on the GPU
                out["stopped_at"] = {"step": name, "exit_status": rc}
                break
            with open(part) as f:
                out["steps"][name] = json.load(f)
            with open(args.out, "w") as f:            # after every step: a later step's failure keeps the earlier figures
                json.dump(out, f, indent=1)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    return 1 if "stopped_at" in out else 0


if __name__ == "__main__":
    sys.exit(main())
