#!/usr/bin/env python3
"""Developer aid: measures the bounds tests/test_gpu_fringe_weighted.py holds the weighted fringe fit to, on the GPU, with that
module's own cases -- the largest |gpu - float64| of the baselines' delays and rates in grid cells and of their snr (relative),
the largest difference in cells between the library's antenna solution and the restatement's from the library's own baselines,
and the coherence ratio fitted / injected truth of the closure case -- and writes them where the tests read them:

    python tools/fringe_weighted_measure.py [--bounds tests/golden/fringe_weighted_bounds.json]
                                            [--closure profiles/fringe_weighted/closure.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KEYS = ("delay_cells", "rate_cells", "snr_rel", "antenna_cells")


def write(path, obj):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(obj, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(obj), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bounds", default=os.path.join(ROOT, "tests", "golden", "fringe_weighted_bounds.json"))
    ap.add_argument("--closure", default=os.path.join(ROOT, "profiles", "fringe_weighted", "closure.json"))
    args = ap.parse_args()
    import torch
    import test_gpu_fringe_weighted as t
    from effex_amd import plan as plan_mod
    cases = []
    for name in sorted(t.ALL_CASES):
        for f in t.all_case(plan_mod, torch, name)[0]:
            print(json.dumps(f), flush=True)
            cases.append(f)
    bounds = {key: max(f[key] for f in cases) for key in KEYS}
    bounds["device"] = torch.cuda.get_device_name(0)
    bounds["cases"] = len(cases)
    bounds["worst_by_case"] = {name: {key: max(f[key] for f in cases if f["case"] == name) for key in KEYS} for name in sorted(t.ALL_CASES)}
    write(args.bounds, bounds)
    write(args.closure, t.closure_case(plan_mod, torch))


if __name__ == "__main__":
    main()
