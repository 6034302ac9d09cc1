#!/usr/bin/env python3
"""Developer aid: the figures tests/test_beam_mask_host.py, tests/test_gpu_beam_mask.py and DESIGN.md §3n read.  The library is
never the yardstick of the interference scenario: its level and its bound come from the restatement (tests/beam_mask_ref.py) alone.

    python tools/beam_mask_measure.py --bounds                                # no GPU: the scenario of beam_mask_ref (a pulsed tone
                                                                              # in one antenna) over seeds 0 - 7 -> the tone's level
                                                                              # and the bound, tests/golden/beam_mask_bounds.json
    python tools/beam_mask_measure.py --parity profiles/beam_mask/parity.json # on the GPU: the largest |gpu - float64| of every shape
                                                                              # of tests/test_gpu_beam_mask.py under a random mask
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
BOUNDS = os.path.join(ROOT, "tests", "golden", "beam_mask_bounds.json")


def bounds(write):
    import beam_mask_ref as r
    import beam_ref
    import gains_ref
    chosen, figures = None, None
    for level in r.RFI_LEVELS:
        figures = {str(seed): r.rfi_restatement(seed, level) for seed in r.RFI_SEEDS}
        ok = all(f["flagged"] and f["factor"] >= r.RFI_FACTOR for f in figures.values())
        print("level", level, "flagged", [f["flagged"] for f in figures.values()], "smallest factor",
              min(f["factor"] for f in figures.values()))
        if ok:
            chosen = level
            break
    assert chosen is not None, "no level of RFI_LEVELS flags every affected cell and lifts the beam by the factor"
    observed = max(f["deviation"] for f in figures.values())
    rec = {"n_ant": beam_ref.GAIN_ANT, "nchan": gains_ref.SAMPLE_NCHAN, "spectra": gains_ref.SAMPLE_SPECTRA, "n_chunks": beam_ref.GAIN_CHUNKS,
           "noise": gains_ref.SAMPLE_NOISE, "seeds": list(r.RFI_SEEDS), "antenna": r.RFI_ANT, "bin": r.RFI_BIN, "frames_on": list(r.RFI_ON),
           "tint": r.RFI_TINT, "level": chosen,
           "level_is": "the tone's power in its bin over the bin's mean clean power in that antenna, while on: the smallest of "
                       "2^4 .. 2^19 that holds for every seed",
           "factor_required": r.RFI_FACTOR, "factor": min(f["factor"] for f in figures.values()),
           "quantity": "max over the cells that keep an antenna of | P_masked (n_ant / count)^2 - P_clean | / P_clean, float64",
           "figures": figures, "observed": observed, "margin": r.RFI_MARGIN, "bound": r.RFI_MARGIN * observed}
    print(json.dumps(rec, indent=1, sort_keys=True))
    if write:
        os.makedirs(os.path.dirname(BOUNDS), exist_ok=True)
        with open(BOUNDS, "w") as fh:
            json.dump(rec, fh, indent=1, sort_keys=True)
            fh.write("\n")
        print("wrote", BOUNDS)


def parity(path):
    import torch
    import test_gpu_beam_mask as g
    from effex_amd import plan as plan_mod
    assert torch.cuda.is_available(), "--parity measures on the GPU only"
    shapes = {"x".join(map(str, shape)): g.shape_errors(plan_mod, torch, shape) for shape in g.SHAPES}
    worst = {kind: max(v for errs in shapes.values() for k, v in errs.items() if k.startswith(kind)) for kind in ("power", "incoherent", "voltage")}
    rec = {"device": torch.cuda.get_device_name(0), "shape": "n_ant x nchan x ntaps x n_pts x n_chunks x n_beam",
           "keys": "mode, mask_tint, tint", "shapes": shapes, "power_of_max_P": worst["power"], "incoherent_of_max_P": worst["incoherent"],
           "power_ceiling": g.TOL_BEAM_POWER.ceiling, "voltage_of_max_abs_y": worst["voltage"], "voltage_ceiling": g.TOL_BEAM_VOLTAGE.ceiling}
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", path, worst)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bounds", action="store_true", help="write tests/golden/beam_mask_bounds.json (without it: print only)")
    ap.add_argument("--parity", default=None, metavar="JSON", help="on the GPU: write the observed errors of the GPU test's shapes")
    args = ap.parse_args()
    if args.parity:
        return parity(args.parity)
    bounds(args.bounds)


if __name__ == "__main__":
    main()
