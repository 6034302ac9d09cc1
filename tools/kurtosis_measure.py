#!/usr/bin/env python3
"""Developer aid: the figures tests/test_kurtosis_host.py, tests/test_gpu_kurtosis.py and DESIGN.md §3m read from
tests/golden/kurtosis_bounds.json.  The library is never the yardstick of the statistics: they come from the restatement
(tests/kurtosis_ref.py) alone.

    python tools/kurtosis_measure.py --bounds                               # no GPU: the estimator on clean noise, seeds 0 - 7:
                                                                            # |mean - 1|, |var / mu2 - 1| (bounds: 3 x the largest)
                                                                            # and the share outside sk_thresholds(64)
    python tools/kurtosis_measure.py --parity profiles/kurtosis/parity.json # on the GPU: the largest |gpu - float64| of every shape
                                                                            # of tests/test_gpu_kurtosis.py; the parity bounds
                                                                            # (2 x the largest) go into the golden file
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
BOUNDS = os.path.join(ROOT, "tests", "golden", "kurtosis_bounds.json")


def read_bounds():
    try:
        with open(BOUNDS) as fh:
            return json.load(fh)
    except (OSError, ValueError):
        return {}


def write_json(path, rec):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", path)


def bounds(write):
    import kurtosis_ref as kr
    stats = {str(seed): kr.noise_statistics(seed) for seed in kr.STAT_SEEDS}
    mean_dev = {s: v[0] for s, v in stats.items()}
    var_dev = {s: v[1] for s, v in stats.items()}
    alarm = {s: v[2] for s, v in stats.items()}
    rec = read_bounds()
    rec["statistics"] = {
        "shape": "n_ant x nchan x ntaps x n_pts x n_chunks = " + " x ".join(map(str, kr.STAT_SHAPE)), "seeds": list(kr.STAT_SEEDS),
        "mu2": kr.mu2(kr.STAT_SHAPE[3]), "mean_deviation": mean_dev, "variance_deviation": var_dev,
        "quantities": "| mean sk - 1 |, | var sk / mu2(64) - 1 | over all elements of a seed; share of elements outside 1 -/+ 3 sqrt(mu2)",
        "mean_bound": 3.0 * max(mean_dev.values()), "variance_bound": 3.0 * max(var_dev.values()),
        "false_alarm_share": alarm, "false_alarm_share_mean": sum(alarm.values()) / len(alarm)}
    print(json.dumps(rec["statistics"], indent=1, sort_keys=True))
    if write:
        write_json(BOUNDS, rec)


def parity(path):
    import torch
    import test_gpu_kurtosis as g
    from effex_amd import plan as plan_mod
    assert torch.cuda.is_available(), "--parity measures on the GPU only"
    shapes = {"x".join(map(str, shape)): g.shape_errors(plan_mod, torch, shape, tints) for shape, tints in g.SHAPES}
    sk = max(v for errs in shapes.values() for k, v in errs.items() if k.startswith("sk"))
    power = max(v for errs in shapes.values() for k, v in errs.items() if k.startswith("power"))
    write_json(path, {"device": torch.cuda.get_device_name(0), "shape": "n_ant x nchan x ntaps x n_pts x n_chunks", "shapes": shapes,
                      "sk_abs": sk, "power_of_max": power})
    rec = read_bounds()
    rec["parity"] = {"device": torch.cuda.get_device_name(0), "sk_observed": sk, "power_observed": power, "sk_bound": 2.0 * sk,
                     "power_bound": 2.0 * power, "largest_M": g.LARGEST_M,
                     "quantities": "largest | sk - float64 sk |; largest | power - float64 power | / max power, over every element of every shape"}
    write_json(BOUNDS, rec)
    print("sk", sk, "power", power)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bounds", action="store_true", help="write the statistics to tests/golden/kurtosis_bounds.json")
    ap.add_argument("--parity", default=None, metavar="JSON", help="on the GPU: write the observed errors and the parity bounds")
    args = ap.parse_args()
    if args.parity:
        return parity(args.parity)
    bounds(args.bounds)


if __name__ == "__main__":
    main()
