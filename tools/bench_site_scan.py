#!/usr/bin/env python3
"""Times the combinatorial site scan (xgpr_conv_token_site_scan_f32 through ConvSORFKernel.site_scan and SiteLibrary) against the
composed route that writes every variant out (ConvSORFKernel.site_scan_composed), and writes profiles/site_scan.json.

    python tools/bench_site_scan.py [--out profiles/site_scan.json] [--rounds 3] [--reps 3] [--composed-reps 1]

One sequence of 56 tokens (the length of GB1), one-hot tokens over V = 20 rows (C = 20 channels), conv_width 9, averaging "sqrt",
M = 16384 features (8192 frequencies, 8 tiles), one weight vector:
  * gb1      sites (38, 39, 40, 53): the whole library of 20^4 = 160 000 variants as a dense array.
             operator: site_scan, then SiteLibrary.dense();  composed: site_scan_composed (one table over all four sites).
  * two_by_3 sites (10, 11, 12, 38, 39, 40): two components of three sites, 20^6 = 6.4e7 variants, the 100 best.
             operator: site_scan, then SiteLibrary.topk(100);  composed: site_scan_composed of each component (8000 variants
             each), all 6.4e7 sums formed on the device and torch.topk of them -- the whole library is beyond what the composed
             route writes out in one piece.
The arms alternate inside every round (one process, one device); each timing is a device-event window around ``reps`` back-to-back
calls (``composed-reps`` for the composed route) after a warm-up of every arm; the median and the minimum over the rounds are
recorded, in milliseconds per call.  Peak device memory is torch's max_memory_allocated over one call, less what was allocated
before it.  Beside the measured ratio of times stands the ratio of tile transforms (one window through one 1024-frequency tile)
the two routes perform.  Needs a HIP device: there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_subst_scan import peak_bytes, timed     # noqa: E402

L, V, CONV_WIDTH, M = 56, 20, 9, 16384
TILES = (M // 2 + 1023) // 1024
CASES = [("gb1", (38, 39, 40, 53)), ("two_by_3", (10, 11, 12, 38, 39, 40))]
TOP = 100


def tile_transforms(sites, components):
    """(operator, composed): the operator transforms, for every run, V^g variants of each of its windows; the composed route every
    window of every written-out variant of every component it is called for, and of the sequence itself."""
    from xgpr_amd.acquisition import site_runs
    nk = L - CONV_WIDTH + 1
    op = sum((jhi - jlo + 1) * V ** g for jlo, jhi, _, g in site_runs(list(sites), L, CONV_WIDTH))
    comp = sum((V ** len(c) + 1) * nk for c in components)
    return op * TILES, comp * TILES


def run(name, sites, k, args, rng):
    from xgpr_amd.dataset import TokenBatch
    dev = "cuda"
    lengths = np.asarray([L], dtype=np.int32)
    tokens = torch.from_numpy(rng.integers(0, V, size=(1, L)).astype(np.uint8)).to(dev)
    raw = TokenBatch(tokens, torch.eye(V, dtype=torch.float32, device=dev))
    w = torch.from_numpy(rng.standard_normal(M)).to(dev)
    K = len(sites)
    whole = name == "gb1"
    comps = [tuple(range(K))] if whole else [c for c in k.site_scan(raw, lengths, w, sites).components()]
    keep = {}

    def operator():
        lib = k.site_scan(raw, lengths, w, sites)
        keep["operator"] = lib.dense().reshape(1, -1) if whole else lib.topk(TOP)

    def composed():
        parts = [k.site_scan_composed(raw, lengths, w, [sites[j] for j in c]).tables[0].reshape(-1) for c in comps]
        if whole:
            keep["composed"] = parts[0][None, :]
        else:
            sums = (parts[0][:, None] + parts[1][None, :]).reshape(-1)
            vals, flat = torch.topk(sums, TOP)
            keep["composed"] = (vals[None, :], flat)

    arms = {"operator": operator, "composed": composed}
    reps = {"operator": args.reps, "composed": args.composed_reps}
    for fn in arms.values():                             # warm-up: code objects, allocator
        fn()
    torch.cuda.synchronize()
    a, b = (keep["operator"], keep["composed"]) if whole else (keep["operator"][0], keep["composed"][0])
    diff, big = float((a - b).abs().max()), float(a.abs().max())
    same_picks = None
    if not whole:                                        # the 100 picks themselves: flat indices over (component 0, component 1)
        assign = keep["operator"][1][0]
        flat = torch.zeros(TOP, dtype=torch.long, device=dev)
        for j in range(K):
            flat = flat * V + assign[:, j]
        same_picks = int((flat == keep["composed"][1]).sum())
    keep.clear()
    torch.cuda.empty_cache()
    peaks = {nm: peak_bytes(fn) for nm, fn in arms.items()}
    keep.clear()
    times = {nm: [] for nm in arms}
    for _ in range(args.rounds):
        for nm, fn in arms.items():
            times[nm].append(timed(fn, reps[nm]))
    keep.clear()
    med = {nm: float(np.median(t)) for nm, t in times.items()}
    op, comp = tile_transforms(sites, comps)
    time_ratio, count_ratio = med["composed"] / med["operator"], comp / op
    return {"workload": {"name": name, "n": 1, "L": L, "sites": list(sites), "components": [list(c) for c in comps], "V": V, "C": V,
                         "conv_width": CONV_WIDTH, "averaging": "sqrt", "num_rffs": M, "variants": V ** K,
                         "result": "dense library" if whole else f"top {TOP}"},
            "reps_per_window": reps, "ms_median": med, "ms_min": {nm: float(np.min(t)) for nm, t in times.items()},
            "composed_over_operator_time": time_ratio,
            "tile_transforms": {"operator": op, "composed": comp}, "composed_over_operator_tile_transforms": count_ratio,
            "time_ratio_over_count_ratio": time_ratio / count_ratio,
            "operator_is_faster": bool(med["operator"] < med["composed"]),
            "peak_device_bytes_over_the_operands": peaks,
            "max_abs_diff_operator_composed": diff, "max_abs_output": big, "same_picks_of_100": same_picks}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "site_scan.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--composed-reps", type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_site_scan.py needs a HIP device")
    from xgpr_amd.kernels import ConvSORFKernel
    rng = np.random.default_rng(6)
    k = ConvSORFKernel("Conv1dRBF", (1, L, V), M, 123, "cuda", {"intercept": True, "conv_width": CONV_WIDTH, "averaging": "sqrt"})
    k.set_hyperparams(np.asarray([1.0, 2.1 / np.sqrt(CONV_WIDTH)]), logspace=False)
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "unit": "milliseconds per call (device events)",
              "note": "both arms include the host side of their route: the layout, the slicing and SiteLibrary's dense() or topk(); "
                      "the composed arm's windows hold composed-reps calls each",
              "shapes": [run(name, sites, k, args, rng) for name, sites in CASES]}
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
