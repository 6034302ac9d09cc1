#!/usr/bin/env python3
"""Developer aid, CPU only: the figures of the averager's restatement (tests/average_ref.py) on the project's damaged samples
under the detector's and the truth's weights, with the test module's own cases, written where tests/test_average_host.py,
tests/test_gpu_average.py and DESIGN.md §3i read them.  The bound is three times the restatement's largest error: the library
is never the yardstick.

    python tools/average_measure.py              # tests/golden/average_bounds.json
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)


def main():
    import gains_ref
    import gains_weighted_ref as wref
    import test_average_host as t
    fig = t.closure_figures()
    observed = max(v[2] for v in fig.values())
    rec = {"n_ant": wref.DAMAGE_ANT, "nchan": gains_ref.SAMPLE_NCHAN, "n_chunks": gains_ref.SAMPLE_CHUNKS,
           "seeds": list(wref.DAMAGE_SEEDS), "time_bin": 0, "freq_bin": 1,
           "cells": {str(seed): v[0] for seed, v in sorted(fig.items())}, "cells_all": next(iter(fig.values()))[1],
           "detector_weighted": {str(seed): v[2] for seed, v in sorted(fig.items())},
           "plain": {str(seed): v[3] for seed, v in sorted(fig.items())},
           "tone_weight": {str(seed): v[4] for seed, v in sorted(fig.items())},
           "observed": observed, "bound": 3.0 * observed}
    os.makedirs(os.path.dirname(t.BOUNDS), exist_ok=True)
    with open(t.BOUNDS, "w") as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(t.BOUNDS, json.dumps(rec))


if __name__ == "__main__":
    main()
