#!/usr/bin/env python3
"""Developer aid, CPU only: the coherent gain of the beamformer's restatement (tests/beam_ref.py) on the project's calibrator
samples (tests/gains_ref.py samples: x_a = c_a s + n_a), written where tests/test_beam_host.py, tests/test_gpu_beamform.py and
DESIGN.md §3j read it.  The bound is three times the restatement's largest deviation: the library is never the yardstick.

    python tools/beam_measure.py --bounds                              # tests/golden/beam_bounds.json
    python tools/beam_measure.py --parity profiles/beamform/parity.json  # on the GPU: the largest |gpu - float64| of every shape of
                                                                       # tests/test_gpu_beamform.py, of max P and of max |y|
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)


def parity(path):
    import torch
    import test_gpu_beamform as g
    from effex_amd import plan as plan_mod
    assert torch.cuda.is_available(), "--parity measures on the GPU only"
    shapes = {"x".join(map(str, shape)): g.shape_errors(plan_mod, torch, shape) for shape in g.SHAPES}
    power = max(v for errs in shapes.values() for k, v in errs.items() if k != "voltage")
    voltage = max(errs["voltage"] for errs in shapes.values())
    rec = {"device": torch.cuda.get_device_name(0), "shape": "n_ant x nchan x ntaps x n_pts x n_chunks x n_beam", "shapes": shapes,
           "power_of_max_P": power, "power_ceiling": g.TOL_BEAM_POWER.ceiling, "voltage_of_max_abs_y": voltage,
           "voltage_ceiling": g.TOL_BEAM_VOLTAGE.ceiling}
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", path, "power", power, "voltage", voltage)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bounds", action="store_true", help="write tests/golden/beam_bounds.json")
    ap.add_argument("--parity", default=None, metavar="JSON", help="on the GPU: write the observed errors of the GPU test's shapes")
    args = ap.parse_args()
    if args.parity:
        return parity(args.parity)
    import beam_ref
    import gains_ref
    import test_beam_host as t
    dev = {str(seed): t.coherent_gain_deviation(seed) for seed in beam_ref.GAIN_SEEDS}
    observed = max(dev.values())
    rec = {"n_ant": beam_ref.GAIN_ANT, "nchan": gains_ref.SAMPLE_NCHAN, "spectra": gains_ref.SAMPLE_SPECTRA,
           "n_chunks": beam_ref.GAIN_CHUNKS, "noise": gains_ref.SAMPLE_NOISE, "seeds": list(beam_ref.GAIN_SEEDS),
           "quantity": "| R_beam (1 / n_ant^2) sum_a 1 / R_a - 1 |, R = source power / noise power of a beam",
           "deviation": dev, "observed": observed, "bound": 3.0 * observed}
    print(json.dumps(rec, indent=1, sort_keys=True))
    if args.bounds:
        os.makedirs(os.path.dirname(t.BOUNDS), exist_ok=True)
        with open(t.BOUNDS, "w") as fh:
            json.dump(rec, fh, indent=1, sort_keys=True)
            fh.write("\n")
        print("wrote", t.BOUNDS)


if __name__ == "__main__":
    main()
