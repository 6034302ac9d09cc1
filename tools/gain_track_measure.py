#!/usr/bin/env python3
"""Developer aid: the closure figure of the gain track (include/fxcorr.h fxc_set_track_gains) -- track, rows, solve per interval,
gains under the track, rows again; max |mean over each interval of the rows - 1| -- with the test modules' own case.

    python tools/gain_track_measure.py --bounds                  # no GPU: tests/golden/gain_track_bounds.json (the bound of the
                                                                 # closure test: three times the CPU restatement's figure)
    python tools/gain_track_measure.py [--out profiles/gain_track]   # on the GPU: closure.json, the library's measured figure
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


def shape():
    import gain_track_ref as r
    import gains_ref
    return {"n_ant": r.CLOSURE_ANT, "nchan": gains_ref.SAMPLE_NCHAN, "spectra_per_chunk": gains_ref.SAMPLE_SPECTRA,
            "n_chunks": 2 * r.CLOSURE_INTERVAL, "interval": r.CLOSURE_INTERVAL, "receiver_noise": gains_ref.SAMPLE_NOISE,
            "iters": gains_ref.SAMPLE_ITERS, "seeds": list(r.CLOSURE_SEEDS), "frequency": r.CLOSURE_F, "rate_per_antenna": r.CLOSURE_RHO}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gain_track"))
    ap.add_argument("--bounds", action="store_true")
    args = ap.parse_args()
    import gain_track_ref
    if args.bounds:
        f = gain_track_ref.closure_cpu()
        rec = dict(shape(), observed=f["flat"], bound=3.0 * f["flat"], cpu=f)
        return write(os.path.join(ROOT, "tests", "golden", "gain_track_bounds.json"), rec)
    import torch
    import test_gpu_gain_track as t
    from effex_amd import plan as plan_mod
    f = t.closure_case(plan_mod, torch)
    f.update(shape())
    f["device"] = torch.cuda.get_device_name(0)
    f["bound"] = json.load(open(t.BOUNDS))["bound"]
    write(os.path.join(args.out, "closure.json"), f)


if __name__ == "__main__":
    main()
