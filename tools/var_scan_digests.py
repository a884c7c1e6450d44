#!/usr/bin/env python3
"""sha256 digests of what the two variance scans write -- the bitwise contracts of DESIGN.md 3.22 and 3.23, pinned.

    python tools/var_scan_digests.py [--op subst|indel] [--out FILE] [--commit HASH]     record (needs a HIP device)
    python tools/var_scan_digests.py [--op subst|indel] --check FILE                     compare with a recorded file; exit status 1 on
                                                                                         the first difference

``--op subst`` (the default): for every case of tests/dense_subst_var_scan.py the operator runs through the public
``ext.hipConvTokenSubstVarScan`` alone, on the case's operands with the exact u, q rounded to float64 and Vm strided where the case says
so (as tests/test_gpu_subst_var_scan.py calls it).  ``--op indel``: every case of tests/dense_indel_var_scan.py through
``ext.hipConvTokenIndelVarScan``, both outputs from ONE call, on u_del, q_del, u_ins, q_ins rounded to float64 and the same strided Vm
(``run_operator`` of tests/test_gpu_indel_var_scan.py).  So the same file runs on any tree that has the operators.  Recorded per case:
the sha256 of the raw bytes of each output (NaN payloads included) and of every input array.  ``--check`` reports a mismatch of input
digests as "operands differ" (numpy built other operands: nothing is said about the kernels).  tests/test_gpu_subst_var_scan_bits.py
holds the tree to tests/golden/subst_var_scan_digests.json and tests/golden/indel_var_scan_digests.json."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import dense_indel_var_scan as div     # noqa: E402
import dense_subst_var_scan as dv      # noqa: E402

NAMES = [c[0] for c in dv.CASES]
ARRAYS = ("tokens", "table", "seqlen", "radem", "chi")
DERIVED = ("vm", "u64", "q64")
INDEL_NAMES = [c[0] for c in div.CASES]
INDEL_DERIVED = ("vm", "u_del", "q_del", "u_ins", "q_ins")
INDEL_OUTPUTS = ("del", "ins")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _inputs(k, derived):
    out = {key: sha(k["c"][key]) for key in ARRAYS}
    out.update({key: sha(np.asarray(k[key], dtype=np.float64)) for key in derived})
    return out


def input_digests(name):
    """{array: sha256} of the operands of the substitution case (Vm, u and q included); no device."""
    return _inputs(dv.case(name), DERIVED)


def indel_input_digests(name):
    """{array: sha256} of the operands of the indel case (Vm and the two pairs u~, q~ included); no device."""
    return _inputs(div.case(name), INDEL_DERIVED)


def _device_operands(k):
    """(tokens, table, radem, chi, Vm) of a case on the device; Vm's rows strided where the case says so (NaN behind every row)."""
    import torch
    full = np.full((k["nvar"], k["nvar"] + k["pad"]), np.nan)
    full[:, :k["nvar"]] = k["vm"]
    return [torch.from_numpy(k["c"][key]).to("cuda") for key in ("tokens", "table", "radem", "chi")] + [torch.from_numpy(full).to("cuda")[:, :k["nvar"]]]


def output_digest(ext, name):
    """sha256 of what the substitution operator writes for the case, on the current HIP device."""
    import torch
    k = dv.case(name)
    c = k["c"]
    tokens, table, radem, chi, vm = _device_operands(k)
    n, L = c["tokens"].shape
    out = torch.full((n, L, c["table"].shape[0]), float("nan"), dtype=torch.float64, device="cuda")
    ext.hipConvTokenSubstVarScan(tokens, table, vm, torch.from_numpy(k["u64"]).to("cuda"), torch.from_numpy(k["q64"]).to("cuda"), out,
                                 radem, chi, c["seqlen"], k["cw"], k["scaling"], k["icpt"])
    return sha(out.cpu().numpy())


def indel_output_digests(ext, name):
    """{"del", "ins": sha256} of what ONE call of the indel operator writes for the case, on the current HIP device."""
    import torch
    k = div.case(name)
    c = k["c"]
    tokens, table, radem, chi, vm = _device_operands(k)
    n, L = c["tokens"].shape
    up = lambda key: torch.from_numpy(k[key]).to("cuda")
    od = torch.full((n, L), float("nan"), dtype=torch.float64, device="cuda")
    oi = torch.full((n, L + 1, c["table"].shape[0]), float("nan"), dtype=torch.float64, device="cuda")
    ext.hipConvTokenIndelVarScan(tokens, table, vm, up("u_del"), up("q_del"), up("u_ins"), up("q_ins"), od, oi, radem, chi, c["seqlen"],
                                 k["cw"], k["scaling"], k["icpt"])
    return {"del": sha(od.cpu().numpy()), "ins": sha(oi.cpu().numpy())}


def _operands_differ(want, mine, name):
    for key in mine:
        if mine[key] != want["inputs"][key]:
            return f"{name}: operands differ ({key}): the recorded digests say nothing about this run"
    return None


def first_difference(recorded, name, output=None):
    """None, or one line that says how the substitution case differs from ``recorded`` (the loaded file): its operands first, then
    ``output``."""
    want = recorded["cases"][name]
    diff = _operands_differ(want, input_digests(name), name)
    if diff is None and output is not None and output != want["output"]:
        diff = f"{name}: the output differs from the recorded bits"
    return diff


def indel_first_difference(recorded, name, outputs=None):
    """The same for the indel case; ``outputs``: what indel_output_digests returned, compared in the order of INDEL_OUTPUTS."""
    want = recorded["cases"][name]
    diff = _operands_differ(want, indel_input_digests(name), name)
    if diff is None and outputs is not None:
        for o in INDEL_OUTPUTS:
            if outputs[o] != want["outputs"][o]:
                return f"{name}: output {o} differs from the recorded bits"
    return diff


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--op", default="subst", choices=("subst", "indel"), help="the operator (default: the substitution variance scan)")
    ap.add_argument("--out", default=None, help="write the digests here (default: print them)")
    ap.add_argument("--commit", default=None, help="the commit the digests are recorded from, noted in the file")
    ap.add_argument("--check", default=None, metavar="FILE")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("var_scan_digests.py needs a HIP device")
    from xgpr_amd import xgpr_hip_rfgen_ext as ext
    names, inputs, outputs, differ, key = ((NAMES, input_digests, output_digest, first_difference, "output") if args.op == "subst" else
                                           (INDEL_NAMES, indel_input_digests, indel_output_digests, indel_first_difference, "outputs"))
    if args.check:
        with open(args.check) as f:
            recorded = json.load(f)
        for name in names:
            diff = differ(recorded, name, outputs(ext, name))
            if diff:
                print(diff)
                return 1
        print(f"{len(names)} cases equal {args.check}")
        return 0
    result = {"commit": args.commit, "device": torch.cuda.get_device_name(0),
              "cases": {name: {"inputs": inputs(name), key: outputs(ext, name)} for name in names}}
    text = json.dumps(result, indent=1) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
        print("wrote", args.out)
    else:
        print(text, end="")
    return 0


if __name__ == "__main__":
    sys.exit(main())
