#!/usr/bin/env python3
"""The feature-cache build (ConvSORFKernel.build_feature_cache) at BASELINE configs[3]'s shape -- one-hot protein-like sequences,
L 64..512, 21 channels, conv_width 9, 16384 RFFs, 'sqrt' averaging -- from a dense float32 dataset and from a token dataset.

    python tools/bench_token_rows.py [--nseq 8192] [--reps 5] [--out profiles/token_rows.json]

Needs a GPU (no fallback).  The two inputs alternate inside one process: warm-up of both, then `reps` rounds of
(dense, token), each build timed with device events around the whole call (table scaling or shard scaling, ordering kernel,
feature kernel; the scaled dense shard is dropped before every dense build so that it is rebuilt as in a first fit).  The
margin a difference is read against is the spread of the dense builds themselves (min .. max over the rounds); both are
recorded.  The caches are compared bit for bit.  Peak device memory of one build of each kind is recorded as well: the
footprint is what token input is for."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nseq", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rffs", type=int, default=16384)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "token_rows.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_token_rows.py needs a GPU")
    from xgpr_amd.dataset import build_regression_dataset
    from xgpr_amd.kernels import make_kernel
    dev, L, C, w = "cuda", 512, 21, 9
    rng = np.random.default_rng(3)
    tokens = rng.integers(0, C, size=(args.nseq, L))
    lens = rng.integers(64, L + 1, size=args.nseq).astype(np.int32)
    y = rng.standard_normal(args.nseq)
    table = np.eye(C, dtype=np.float32)
    ds_dense = build_regression_dataset(table[tokens], y, lens, chunk_size=1024, device=dev)
    ds_token = build_regression_dataset(tokens, y, lens, chunk_size=1024, device=dev, token_table=table)
    kern = make_kernel("Conv1dRBF", (args.nseq, L, C), args.rffs, 123, dev, {"conv_width": w, "averaging": "sqrt"})
    kern.set_hyperparams(np.array([1.0, 0.8]), logspace=False)

    def build(ds):
        ds._scaled = {}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        e0.record()
        zc = kern.build_feature_cache(ds)
        e1.record()
        e1.synchronize()
        return zc, e0.elapsed_time(e1), torch.cuda.max_memory_allocated() - base

    zd, _, peak_dense = build(ds_dense)
    zt, _, peak_token = build(ds_token)
    identical = bool(torch.equal(zd, zt))
    del zd, zt
    t_dense, t_token = [], []
    for _ in range(args.reps):
        z, ms, _ = build(ds_dense)
        t_dense.append(ms)
        del z
        z, ms, _ = build(ds_token)
        t_token.append(ms)
        del z
    kmers = int((lens.astype(np.int64) - w + 1).sum())
    med = lambda v: float(np.median(v))
    out = {
        "workload": "BASELINE configs[3] shape: Conv1dRBF, %d sequences (L 64..512, one-hot 21 channels, conv_width 9), %d RFFs, "
                    "build_feature_cache" % (args.nseq, args.rffs),
        "device": torch.cuda.get_device_name(0), "reps": args.reps, "kmers": kmers,
        "dense_ms": t_dense, "token_ms": t_token,
        "dense_median_ms": med(t_dense), "token_median_ms": med(t_token),
        "dense_spread_ms": [min(t_dense), max(t_dense)],
        "token_over_dense": med(t_token) / med(t_dense),
        "dense_spread_rel": (max(t_dense) - min(t_dense)) / med(t_dense),
        "caches_bit_identical": identical,
        "peak_bytes_during_build": {"dense": int(peak_dense), "token": int(peak_token), "cache": args.nseq * args.rffs * 4},
        "input_bytes_resident": {"dense_x": args.nseq * L * C * 4, "tokens": args.nseq * L},
        "timing": "device events around build_feature_cache, dense and token builds alternating in one process after a warm-up of both",
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
