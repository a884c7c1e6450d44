#!/usr/bin/env python3
"""Times the backward of the two-layer kernel's first layer (xgpr_conv_maxpool_input_grad_f32 /
xgpr_conv_token_maxpool_input_grad_f32) on the device and writes profiles/two_layer_input_grad.json.

    python tools/bench_two_layer_input_grad.py [--out profiles/two_layer_input_grad.json] [--rounds 5] [--reps 5] [--composed-reps 1]

Workload: 1024 protein-like sequences at BASELINE configs[3]'s shape -- lengths uniform in 64 .. 512 in an array of L = 512, one-hot
over 21 channels, conv_width 9 --, init_rffs = 1024 filters, one g vector for all sequences.
Arms, on the same tree and the same operands:
  * operator        hipConvMaxpoolInputGrad on the dense float32 array;
  * operator_tokens hipConvTokenMaxpoolInputGrad on the uint8 tokens and the [21, 21] table;
  * composed        Conv1dTwoLayerKernel.first_layer_gradient_composed, the unfold route from existing operators;
  * maxpool         hipConv1dMaxpool on the same sequences into zero-filled rows: the forward half alone (the zero fill is inside
                    the timed window: the operator needs it).
The arms alternate inside every round (one process, one device); each timing is a device-event window around ``reps`` back-to-back
calls (``composed-reps`` for the composed route: a SHORT window, stated in the output) after a warm-up of every arm; the median and
the minimum over the rounds are recorded, in milliseconds per call.  Peak device memory of the operator and of the composed route is
torch's max_memory_allocated over one call, less what was allocated before it.
Needs a HIP device: there is no fallback.  Reads nothing outside the repository."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, L, C, CONV_WIDTH, INIT_RFFS, M = 1024, 512, 21, 9, 1024, 2048
MIN_LEN = 64


def timed(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / reps                # milliseconds per call


def peak_bytes(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "two_layer_input_grad.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--composed-reps", type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_two_layer_input_grad.py needs a HIP device")
    from xgpr_amd import xgpr_hip_rfgen_ext as ext
    from xgpr_amd.kernels import Conv1dTwoLayerKernel
    dev = "cuda"
    rng = np.random.default_rng(3)
    k = Conv1dTwoLayerKernel((N, L, C), M, 123, dev, {"intercept": True, "conv_width": CONV_WIDTH, "init_rffs": INIT_RFFS})
    lengths = rng.integers(MIN_LEN, L + 1, size=N).astype(np.int32)
    tokens = torch.from_numpy(rng.integers(0, C, size=(N, L)).astype(np.uint8)).to(dev)
    table = torch.eye(C, dtype=torch.float32, device=dev)
    x = table[tokens.long()].contiguous()
    g = torch.from_numpy(rng.standard_normal(INIT_RFFS)).to(dev)
    out = torch.empty((N, L, C), dtype=torch.float64, device=dev)
    out_tok = torch.empty_like(out)
    arg = torch.empty((N, INIT_RFFS), dtype=torch.int32, device=dev)
    arg_tok = torch.empty_like(arg)
    pooled = torch.empty((N, INIT_RFFS), dtype=torch.float32, device=dev)
    tail = (k.radem_diag1, k.chi_arr1, lengths, CONV_WIDTH)
    composed_out = []

    def maxpool():
        pooled.zero_()
        ext.hipConv1dMaxpool(x, pooled, *tail)

    arms = {
        "operator": lambda: ext.hipConvMaxpoolInputGrad(x, g, out, arg, *tail),
        "operator_tokens": lambda: ext.hipConvTokenMaxpoolInputGrad(tokens, table, g, out_tok, arg_tok, *tail),
        "composed": lambda: composed_out.__setitem__(slice(None), [k.first_layer_gradient_composed(x, lengths, g)]),
        "maxpool": maxpool,
    }
    reps = {name: args.composed_reps if name == "composed" else args.reps for name in arms}
    for fn in arms.values():                             # warm-up: code objects, allocator
        fn()
    torch.cuda.synchronize()
    diff = float((out - composed_out[0][0]).abs().max())
    argmax_equal = bool(torch.equal(arg, composed_out[0][1]))
    tokens_equal = bool(torch.equal(out.view(torch.int64), out_tok.view(torch.int64)) and torch.equal(arg, arg_tok))
    active_equal = bool(torch.equal(arg >= 0, pooled > 0))
    composed_out.clear()
    torch.cuda.empty_cache()
    peaks = {name: peak_bytes(arms[name]) for name in ("operator", "operator_tokens", "composed")}
    composed_out.clear()
    times = {name: [] for name in arms}
    for _ in range(args.rounds):
        for name, fn in arms.items():
            times[name].append(timed(fn, reps[name]))
    med = {name: float(np.median(t)) for name, t in times.items()}
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "reps_per_window": reps,
              "note": "the composed arm's windows hold composed-reps calls each: short windows",
              "unit": "milliseconds per call (device events)",
              "workload": {"n": N, "L": L, "min_length": MIN_LEN, "k-mers": int((lengths - CONV_WIDTH + 1).sum()), "C": C,
                           "conv_width": CONV_WIDTH, "init_rffs": INIT_RFFS, "g": "shared"},
              "ms_median": med, "ms_min": {name: float(np.min(t)) for name, t in times.items()},
              "operator_over_composed": med["operator"] / med["composed"],
              "operator_over_maxpool": med["operator"] / med["maxpool"],
              "operator_tokens_over_operator": med["operator_tokens"] / med["operator"],
              "peak_device_bytes_over_the_operands": peaks,
              "peak_note": "the operators write into preallocated outputs (n L C float64 and n F int32, not counted); the composed "
                           "route allocates its own, counted",
              "output_bytes": int(out.numel() * 8 + arg.numel() * 4),
              "max_abs_diff_operator_composed": diff, "argmax_equal_operator_composed": argmax_equal,
              "token_form_bit_identical": tokens_equal, "argmax_active_where_maxpool_positive": active_equal}
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
