#!/usr/bin/env python3
"""sha256 digests of what the substitution variance scan writes -- the bitwise contract of DESIGN.md 3.22, pinned.

    python tools/var_scan_digests.py [--out FILE] [--commit HASH]     record (needs a HIP device)
    python tools/var_scan_digests.py --check FILE                     compare with a recorded file; exit status 1 on the first difference

For every case of tests/dense_subst_var_scan.py the operator runs through the public ``ext.hipConvTokenSubstVarScan`` alone, on the
case's operands with the exact u, q rounded to float64 and Vm strided where the case says so (as tests/test_gpu_subst_var_scan.py
calls it), so the same file runs on any tree that has the operator.  Recorded per case: the sha256 of the raw bytes of the output and
of every input array.  ``--check`` reports a mismatch of input digests as "operands differ" (numpy built other operands: nothing is
said about the kernels).  tests/test_gpu_subst_var_scan_bits.py holds the tree to tests/golden/subst_var_scan_digests.json."""
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

import dense_subst_var_scan as dv      # noqa: E402

NAMES = [c[0] for c in dv.CASES]
ARRAYS = ("tokens", "table", "seqlen", "radem", "chi")
DERIVED = ("vm", "u64", "q64")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def input_digests(name):
    """{array: sha256} of the operands of the case (Vm, u and q included); no device."""
    k = dv.case(name)
    out = {key: sha(k["c"][key]) for key in ARRAYS}
    out.update({key: sha(np.asarray(k[key], dtype=np.float64)) for key in DERIVED})
    return out


def output_digest(ext, name):
    """sha256 of what the operator writes for the case, on the current HIP device."""
    import torch
    k = dv.case(name)
    c = k["c"]
    full = np.full((k["nvar"], k["nvar"] + k["pad"]), np.nan)
    full[:, :k["nvar"]] = k["vm"]
    vm = torch.from_numpy(full).to("cuda")[:, :k["nvar"]]
    n, L = c["tokens"].shape
    out = torch.full((n, L, c["table"].shape[0]), float("nan"), dtype=torch.float64, device="cuda")
    tokens, table, radem, chi = (torch.from_numpy(c[key]).to("cuda") for key in ("tokens", "table", "radem", "chi"))
    ext.hipConvTokenSubstVarScan(tokens, table, vm, torch.from_numpy(k["u64"]).to("cuda"), torch.from_numpy(k["q64"]).to("cuda"), out,
                                 radem, chi, c["seqlen"], k["cw"], k["scaling"], k["icpt"])
    return sha(out.cpu().numpy())


def first_difference(recorded, name, output=None):
    """None, or one line that says how the case differs from ``recorded`` (the loaded file): its operands first, then ``output``."""
    want = recorded["cases"][name]
    mine = input_digests(name)
    for key in ARRAYS + DERIVED:
        if mine[key] != want["inputs"][key]:
            return f"{name}: operands differ ({key}): the recorded digests say nothing about this run"
    if output is not None and output != want["output"]:
        return f"{name}: the output differs from the recorded bits"
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the digests here (default: print them)")
    ap.add_argument("--commit", default=None, help="the commit the digests are recorded from, noted in the file")
    ap.add_argument("--check", default=None, metavar="FILE")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("var_scan_digests.py needs a HIP device")
    from xgpr_amd import xgpr_hip_rfgen_ext as ext
    if args.check:
        with open(args.check) as f:
            recorded = json.load(f)
        for name in NAMES:
            diff = first_difference(recorded, name, output_digest(ext, name))
            if diff:
                print(diff)
                return 1
        print(f"{len(NAMES)} cases equal {args.check}")
        return 0
    result = {"commit": args.commit, "device": torch.cuda.get_device_name(0),
              "cases": {name: {"inputs": input_digests(name), "output": output_digest(ext, name)} for name in NAMES}}
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
