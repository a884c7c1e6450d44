#!/usr/bin/env python3
"""Times the single-edit scan of the two-layer kernel (Conv1dTwoLayerKernel.pool_edits / edit_scan) on the device and
writes profiles/two_layer_edits.json.

    python tools/bench_two_layer_edits.py [--out profiles/two_layer_edits.json] [--rounds 3] [--shapes 1,64]

Workload: protein-like token sequences at BASELINE configs[3]'s sequence shape -- one-hot over V = 21 letters, conv_width 9, an
array of L = 300 positions; one sequence of 300 tokens, and 64 sequences with lengths uniform in 200 .. 300 --, init_rffs = 1024
filters, num_rffs = 16384 second-layer features.
Arms per shape and edit (substitutions, deletions, insertions), on the same tree and the same operands:
  * tables          hipConvTokenMaxpoolTables (once per call of pool_edits, whatever the edit);
  * edits           the slabs of hipConvTokenMaxpoolEdits, each written into one reused buffer;
  * composed_pool   the slabs of pool_edits_composed: every mutant written out as a token row and pooled by hipConvTokenMaxpool;
  * second_layer    _edit_rows_results -- the ONE function both row sources feed, with the same slab boundaries -- on the first slab
                    of the operator route.  It costs the same for both routes by construction, so it is timed on that slab and
                    scaled to the edit's rows (stated as such in the output: an extrapolation, not a measurement of the whole).
The first-layer arms alternate inside every round (one process, one device) after a warm-up of each; every timing is a device-event
window around one pass over all slabs; medians and minima over the rounds, in milliseconds.  Window-transform counts of both routes
are exact counts from the lengths.  Peak device memory is torch's max_memory_allocated over one pass, less what was allocated before.
Needs a HIP device: there is no fallback.  Reads nothing outside the repository."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L, V, CONV_WIDTH, INIT_RFFS, M, NVAR = 300, 21, 9, 1024, 16384, 512
MIN_LEN = 200
EDITS = ("substitutions", "deletions", "insertions")


def timed(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)                       # milliseconds


def peak_bytes(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def transform_counts(lengths, edit):
    """Exact window transforms of the first layer: (operator route incl. the tables, written-out route)."""
    cw = CONV_WIDTH
    op = comp = 0
    for s in (int(x) for x in lengths):
        nk = s - cw + 1
        op += nk                                         # the tables: every window of the sequence once
        if edit == "substitutions":
            op += V * sum(min(l, nk - 1) - max(0, l - cw + 1) + 1 for l in range(s))
            comp += s * V * nk
        elif edit == "deletions":
            op += sum(max(0, min(p - 1, nk - 2) - max(0, p - cw + 1) + 1) for p in range(s))
            comp += s * (nk - 1)
        else:
            op += V * sum(min(g, nk) - max(0, g - cw + 1) + 1 for g in range(s + 1))
            comp += (s + 1) * V * (nk + 1)
    return op, comp


def bench_shape(n, rounds, rng):
    from xgpr_amd import xgpr_hip_rfgen_ext as ext
    from xgpr_amd.dataset import TokenBatch
    from xgpr_amd.kernels import Conv1dTwoLayerKernel
    dev = "cuda"
    k = Conv1dTwoLayerKernel((n, L, V), M, 123, dev, {"intercept": True, "conv_width": CONV_WIDTH, "init_rffs": INIT_RFFS})
    k.set_hyperparams(np.array([0.5, 0.05]), logspace=False)
    lengths = (np.full(1, L) if n == 1 else rng.integers(MIN_LEN, L + 1, size=n)).astype(np.int32)
    tokens = rng.integers(0, V, size=(n, L)).astype(np.uint8)
    for i, s in enumerate(lengths):
        tokens[i, s:] = 255
    batch = TokenBatch(torch.from_numpy(tokens).to(dev), torch.eye(V, dtype=torch.float32, device=dev))
    w = torch.from_numpy(rng.standard_normal(M)).to(dev)
    a = rng.standard_normal((NVAR, NVAR))
    var = torch.from_numpy(a @ a.T / NVAR).to(dev)
    pm = torch.empty((n, L - CONV_WIDTH + 2, INIT_RFFS), dtype=torch.float32, device=dev)
    sm = torch.empty_like(pm)
    tail = (k.radem_diag1, k.chi_arr1, lengths, CONV_WIDTH)

    def tables():
        ext.hipConvTokenMaxpoolTables(batch.tokens, batch.table, pm, sm, *tail)

    result = {"n": n, "lengths": "300" if n == 1 else f"uniform {MIN_LEN} .. {L}", "k-mers": int((lengths - CONV_WIDTH + 1).sum()), "edits": {}}
    tables()
    torch.cuda.synchronize()
    for edit in EDITS:
        slots, per, step = k._edit_geometry(batch, edit)
        total = n * slots
        buf = torch.empty((min(step, total), INIT_RFFS) if edit == "deletions" else (min(step, total), per, INIT_RFFS),
                          dtype=torch.float32, device=dev)

        def edits():
            for lo in range(0, total, step):
                cnt = min(step, total - lo)
                ext.hipConvTokenMaxpoolEdits(batch.tokens, batch.table, pm, sm, buf[:cnt], *tail, edit, lo, cnt)

        def composed():
            for _ in k.pool_edits_composed(batch, lengths, edit):
                pass

        first = next(iter(k.pool_edits(batch, lengths, edit)))[1].reshape(-1, INIT_RFFS)
        if edit == "deletions":
            first = torch.nan_to_num(first, nan=0.0)

        def second():
            k._edit_rows_results(first, w, var)

        arms = {"tables": tables, "edits": edits, "composed_pool": composed}
        for fn in arms.values():                         # warm-up: code objects, allocator
            fn()
        second()
        torch.cuda.synchronize()
        # the two routes give the same rows (one slab compared; the tests compare all of them)
        ref = next(iter(k.pool_edits_composed(batch, lengths, edit)))[1].reshape(-1, INIT_RFFS)
        got = next(iter(k.pool_edits(batch, lengths, edit)))[1].reshape(-1, INIT_RFFS)
        same = bool(((got == ref) | (torch.isnan(got) & torch.isnan(ref))).all())
        del ref, got
        torch.cuda.empty_cache()
        peaks = {"operator (tables + one pass of edits)": peak_bytes(lambda: (tables(), edits())), "composed_pool": peak_bytes(composed)}
        times = {name: [] for name in arms}
        for _ in range(rounds):
            for name, fn in arms.items():
                times[name].append(timed(fn))
        t_second = [timed(second) for _ in range(max(2, rounds))]
        med = {name: float(np.median(t)) for name, t in times.items()}
        rows = total * per
        second_ms = float(np.median(t_second)) * rows / first.shape[0]
        op_first, comp_first = med["tables"] + med["edits"], med["composed_pool"]
        ops, comps = transform_counts(lengths, edit)
        result["edits"][edit] = {
            "mutant_rows": rows, "slabs": -(-total // step), "ms_median": med, "ms_min": {name: float(np.min(t)) for name, t in times.items()},
            "second_layer_ms_first_slab": float(np.median(t_second)), "second_layer_rows_first_slab": int(first.shape[0]),
            "second_layer_ms_scaled_to_all_rows": second_ms,
            "first_layer_ms": {"operator": op_first, "composed": comp_first}, "first_layer_speedup": comp_first / op_first,
            "total_ms": {"operator": op_first + second_ms, "composed": comp_first + second_ms},
            "total_speedup": (comp_first + second_ms) / (op_first + second_ms),
            "window_transforms": {"operator": ops, "composed": comps, "ratio": comps / ops},
            "speedup_over_transform_ratio": (comp_first / op_first) / (comps / ops),
            "peak_device_bytes_over_the_operands": peaks, "table_bytes": int(2 * pm.numel() * 4), "slab_bytes": int(buf.numel() * 4),
            "rows_equal_on_the_first_slab": same}
        del buf, first
        torch.cuda.empty_cache()
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "two_layer_edits.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default="1,64")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_two_layer_edits.py needs a HIP device")
    rng = np.random.default_rng(5)
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "unit": "milliseconds per pass over all slabs (device events)",
              "workload": {"L": L, "V": V, "table": "one-hot", "conv_width": CONV_WIDTH, "init_rffs": INIT_RFFS, "num_rffs": M, "nvar": NVAR},
              "note": "second_layer: timed on the operator route's first slab and scaled to the edit's rows -- both routes feed the same "
                      "function with the same slab boundaries, so it is the same for both; the totals contain that extrapolation",
              "shapes": []}
    for n in (int(x) for x in args.shapes.split(",")):
        result["shapes"].append(bench_shape(n, args.rounds, rng))
        print(json.dumps(result["shapes"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
