#!/usr/bin/env python3
"""Developer aid, CPU only: the figures of the detector's restatement (tests/flag_ref.py) on the project's damaged and clean
samples, with the test module's own cases, written where tests/test_flag_host.py and DESIGN.md §3h read them.

    python tools/flag_measure.py              # tests/golden/flag_bounds.json
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
    import test_flag_host as t
    fig = t.detection_figures()
    shares = t.clean_shares()
    rec = {"n_ant": wref.DAMAGE_ANT, "nchan": gains_ref.SAMPLE_NCHAN, "n_chunks": gains_ref.SAMPLE_CHUNKS,
           "seeds": list(wref.DAMAGE_SEEDS), "refs": list(wref.DAMAGE_REFS),
           "parameters": {"window": 0, "time_threshold": 20.0, "freq_threshold": 8.0, "half_width": 8, "iters": 2},
           "caught": {str(seed): v for seed, v in sorted(fig["caught"].items())},
           "caught_smallest": min(fig["caught"].values()),
           "tone_bin_all_flagged": all(fig["tone"].values()),
           "closure": {"seed %d ref %d" % k: {"detector": v[0], "unweighted": v[1]} for k, v in sorted(fig["errors"].items())},
           "closure_worst": max(err for err, _ in fig["errors"].values()),
           "clean_share": {str(seed): v for seed, v in sorted(shares.items())}}
    os.makedirs(os.path.dirname(t.BOUNDS), exist_ok=True)
    with open(t.BOUNDS, "w") as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(t.BOUNDS, json.dumps(rec))


if __name__ == "__main__":
    main()
