#!/usr/bin/env python3
"""Developer aid: measures the figures of the weighted gain solve's tests, with the test modules' own cases, and writes them where
the tests and DESIGN.md §3g read them.

    python tools/gains_weighted_measure.py --bounds              # no GPU: tests/golden/gains_weighted_bounds.json (the bound B of
                                                                 # the damaged-samples tests: three times the restatement's
                                                                 # largest error on the oracle's rows)
    python tools/gains_weighted_measure.py [--out profiles/gains_weighted]
                                                                 # on the GPU: parity.json (largest |gpu - float64| of gains and
                                                                 # step over the parity cases) and closure.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)


def write(path, obj):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(obj, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(path, json.dumps(obj), flush=True)


def bounds():
    import gains_ref
    import gains_weighted_ref as wref
    import test_gains_weighted_host as t
    errors = t.damage_errors()
    observed = max(err for err, _ in errors.values())
    write(t.BOUNDS, {"observed": observed, "bound": 3.0 * observed, "n_ant": wref.DAMAGE_ANT, "nchan": gains_ref.SAMPLE_NCHAN,
                     "spectra_per_chunk": gains_ref.SAMPLE_SPECTRA, "n_chunks": gains_ref.SAMPLE_CHUNKS,
                     "receiver_noise": gains_ref.SAMPLE_NOISE, "iters": gains_ref.SAMPLE_ITERS, "seeds": list(wref.DAMAGE_SEEDS),
                     "refs": list(wref.DAMAGE_REFS), "unweighted_smallest": min(plain for _, plain in errors.values()),
                     "errors": {"seed %d ref %d" % k: {"weighted": v[0], "unweighted": v[1]} for k, v in sorted(errors.items())}})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gains_weighted"))
    ap.add_argument("--bounds", action="store_true")
    args = ap.parse_args()
    if args.bounds:
        return bounds()
    import torch
    import test_gpu_gains_weighted as t
    from effex_amd import plan as plan_mod
    cases = []
    for n_ant, nchan in t.PARITY:
        for f in t.parity_case(plan_mod, torch, n_ant, nchan):
            print(json.dumps(f), flush=True)
            cases.append(f)
    keys = ("gain_rel", "step_abs")
    parity = {key: max(f[key] for f in cases) for key in keys}
    parity["device"] = torch.cuda.get_device_name(0)
    parity["cases"] = len(cases)
    parity["worst_by_antennas"] = {str(n): {key: max(f[key] for f in cases if f["n_ant"] == n) for key in keys}
                                   for n in sorted({f["n_ant"] for f in cases})}
    write(os.path.join(args.out, "parity.json"), parity)
    closure = {"device": torch.cuda.get_device_name(0), "bound": t.damage_bound(),
               "cases": [t.damage_case(plan_mod, torch, seed) for seed in t.DAMAGE_SEEDS]}
    write(os.path.join(args.out, "closure.json"), closure)


if __name__ == "__main__":
    main()
