#!/usr/bin/env python3
"""Developer aid: measures the bounds tests/test_gpu_fringe.py holds the fringe fit to, on the GPU, with that module's own
cases -- the largest |gpu - float64| of delay and rate in grid cells and of snr (relative) over the parity cases, and the
coherence ratio fitted / injected truth of the closure cases -- and writes them where the tests read them:

    python tools/fringe_measure.py [--out profiles/fringe]        # parity.json, closure.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fringe"))
    args = ap.parse_args()
    import torch
    import test_gpu_fringe as t
    from effex_amd import plan as plan_mod
    os.makedirs(args.out, exist_ok=True)
    cases = []
    for n_ant, nchan in t.PARITY:
        for f in t.parity_case(plan_mod, torch, n_ant, nchan):
            print(json.dumps(f), flush=True)
            cases.append(f)
    parity = {key: max(f[key] for f in cases) for key in ("delay_cells", "rate_cells", "snr_rel")}
    parity["device"] = torch.cuda.get_device_name(0)
    parity["cases"] = len(cases)
    parity["worst_by_pad"] = {str(pad): {key: max(f[key] for f in cases if f["pad"] == pad) for key in ("delay_cells", "rate_cells", "snr_rel")}
                              for pad in (1, 2, 4)}
    with open(os.path.join(args.out, "parity.json"), "w") as fh:
        json.dump(parity, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(parity), flush=True)
    closure = {name: t.closure_case(plan_mod, torch, name) for name in sorted(t.CLOSURE)}
    with open(os.path.join(args.out, "closure.json"), "w") as fh:
        json.dump(closure, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(closure), flush=True)


if __name__ == "__main__":
    main()
