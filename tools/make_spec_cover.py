#!/usr/bin/env python3
"""tests/golden/spec_cover.json: the channel counts whose kernels, between them, run every butterfly x stage position and every layout
feature (tests/spec_cover.py::features) that the measured table effex_amd/csrc/spec_tuned.h and a sample of the cost model's choices
use -- per build variant a greedy minimum cover, ties to the smaller channel count.  Needs no GPU: every shape is asked of the
library's own search (fxc_spec_probe compiles through hiprtc), in up to 16 worker processes, with the code objects kept in a scratch
cache so that a second run is fast.

    python tools/make_spec_cover.py [--cache build/spec_cover_cache] [--jobs 16]

Prints what the pull request that regenerates the file should state: the (radix, position) pairs the tests named in EXISTING reach,
the table entries the search does not take, and how much of the cost model's range was sampled.
"""
import argparse
import json
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import spec_cover  # noqa: E402

NTAPS = 4
VARIANTS = (0, 2, 3)

# (channels, taps, frames per step forced through the developer library or 0) of the tests that ran these kernels before the cover:
# tests/test_gpu_parity.py and tests/test_emul.py
EXISTING = {
    0: [(n, t, 0) for n, t in ((1000, 4), (96, 4), (1536, 4), (720, 3), (250, 2), (12, 4), (2000, 4), (1001, 4), (600, 1), (20, 4), (7, 1), (3000, 4),
                               (4000, 4), (2560, 3), (2400, 4), (3072, 2), (1020, 4), (34, 4), (1140, 3), (460, 4), (1900, 4), (2040, 4))] +
       [(n, t, u) for u in (1, 2) for n, t in ((1000, 4), (96, 4), (12, 4), (6, 2), (7, 1), (250, 4), (720, 3), (1001, 4), (1536, 4), (4, 4), (3000, 4),
                                               (4000, 4), (2560, 3), (2400, 4), (340, 4), (38, 2), (1700, 4))],
    2: [(n, t, 0) for n, t in ((1000, 4), (96, 4), (720, 3), (250, 1), (2000, 4), (96, 2), (3000, 4), (2400, 4), (4000, 4), (5000, 4), (6000, 3), (8000, 4),
                               (7168, 4), (6000, 4), (4500, 2), (6561, 4), (7000, 3), (250, 2), (7, 1), (12, 4), (3584, 2), (6000, 2))],
    3: [(n, t, 0) for n, t in ((6000, 4), (5000, 4), (4500, 2), (6561, 4), (7000, 3))],
}

# Channel counts the cost model serves (not in the table), four taps.  There is no cheap way to list every count whose kernel gets a
# radix outside {2 ... 11, 13, 16, 20, 25}: whether a count is eligible and which list it gets depends on the registers of the compiled
# candidates, so each costs a search.  Sampled instead: counts with the prime factors 17, 19 and 23 (which must run those butterflies),
# multiples of 32 that could take the 32-point butterfly, and a spread of other smooth counts.
SAMPLE = {
    0: [34, 68, 102, 170, 340, 510, 1020, 1700, 2040, 38, 76, 190, 380, 1140, 1900, 46, 92, 230, 460, 1380, 1840,
        480, 672, 1056, 1440, 2016, 2880, 3360, 6, 10, 22, 26, 33, 39, 44, 52, 55, 65, 66, 78, 88, 104, 132, 143, 156, 1001, 1716, 2002, 3003, 4004],
    2: [34, 68, 170, 340, 1020, 1700, 2040, 38, 190, 1140, 1900, 46, 230, 460, 1840, 480, 672, 1440, 2016, 3360, 6, 10, 22, 26, 33, 39, 143, 1001,
        4160, 4400, 4620, 5040, 6144, 6400, 7680, 8008, 8100],
    3: [4160, 4200, 4400, 4608, 4620, 5040, 5120, 5632, 6144, 6400, 6656, 7168, 7680, 8000, 8008, 8100],
}


def _probe(job):
    variant, nchan, ntaps, u = job
    if u:
        os.environ["FXC_RTC_U"] = str(u)
    else:
        os.environ.pop("FXC_RTC_U", None)
    try:
        return job, spec_cover.probe(nchan, ntaps, variant)
    finally:
        os.environ.pop("FXC_RTC_U", None)


def smooth23(n):
    for p in (2, 3, 5, 7, 11, 13, 17, 19, 23):
        while n % p == 0:
            n //= p
    return n == 1


def greedy(cands, universe):
    """cands {nchan: feature set} -> [(nchan, the features it was chosen for)]: most new features first, ties to the smaller count"""
    left, chosen = set(universe), []
    while left:
        gain, n = max(((len(f & left), -n) for n, f in cands.items()), default=(0, 0))
        if gain == 0:
            break
        n = -n
        chosen.append((n, cands[n] & left))
        left -= cands[n]
    return sorted(chosen), left


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cache", default=os.path.join(ROOT, "build", "spec_cover_cache"))
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--out", default=spec_cover.COVER_PATH)
    args = ap.parse_args()
    os.makedirs(args.cache, exist_ok=True)
    os.environ["FXC_RTC_CACHE"] = args.cache
    tables = spec_cover.parse_tuned()
    jobs = set()
    for v in VARIANTS:
        in_table = {e["n"] for e in tables[v]}
        jobs |= {(v, e["n"], NTAPS, 0) for e in tables[v]}
        jobs |= {(v, n, t, u) for n, t, u in EXISTING[v]}
        jobs |= {(v, n, NTAPS, 0) for n, t, u in EXISTING[v]}
        jobs |= {(v, n, NTAPS, 0) for n in SAMPLE[v] if n not in in_table}
    jobs = sorted(jobs)
    # the second pass needs antenna 0's F-only build beside it; a first-stage feature of F + X is also run from bytes (variant 1)
    with multiprocessing.Pool(min(16, max(1, args.jobs))) as pool:
        reports = dict(pool.imap_unordered(_probe, jobs, chunksize=1))
        out = {"ntaps": NTAPS, "cover": {}, "probed": {}, "not_eligible": {}, "universe": {}, "table_entries_not_taken": {}, "uncovered": {}}
        summary = {}
        extra_jobs = []
        for v in VARIANTS:
            in_table = {e["n"]: e for e in tables[v]}
            four = {n: rep for (vv, n, t, u), rep in reports.items() if vv == v and t == NTAPS and u == 0}
            cands = {n: spec_cover.features(v, rep) for n, rep in four.items() if rep is not None}
            universe = set().union(*cands.values())
            chosen, left = greedy(cands, universe)
            dead = []
            for n, e in sorted(in_table.items()):
                rep = four.get(n)
                if rep is None or rep["stages"] != e["radix"] or rep["frames_per_step"] != e["u"]:
                    dead.append({"nchan": n, "table": {"stages": e["radix"], "u": e["u"]},
                                 "search": None if rep is None else {"stages": rep["stages"], "u": rep["frames_per_step"]}})
            static = set().union(*[spec_cover.static_features(v, e) for e in tables[v]])
            pairs = {f for f in static if f[1] == "radix"}
            before = set()
            for (vv, n, t, u), rep in reports.items():
                if vv == v and rep is not None and (n, t, u) in set(EXISTING[v]):
                    before |= spec_cover.features(v, rep)
            limit = 4096 if v == 0 else 8192
            lo = 4097 if v == 3 else 2
            model_range = [n for n in range(lo, limit + 1) if smooth23(n) and n & (n - 1) and n not in in_table]
            sampled = sorted(n for n in four if n not in in_table)
            out["cover"][str(v)] = [dict(nchan=n, report=spec_cover.recorded(four[n]), chosen_for=sorted(list(f) for f in why)) for n, why in chosen]
            out["probed"][str(v)] = sorted(n for n, rep in four.items() if rep is not None)
            out["not_eligible"][str(v)] = sorted(n for n, rep in four.items() if rep is None)
            out["universe"][str(v)] = sorted(list(f) for f in universe)
            out["table_entries_not_taken"][str(v)] = dead
            out["uncovered"][str(v)] = sorted(list(f) for f in left)
            summary[v] = dict(table_entries=len(in_table), table_pairs=len(pairs), pairs_reached_before=len(pairs & before), pairs_in_universe=len(pairs & universe),
                              static_missing=sorted(static - universe), not_taken=len(dead), cover=[n for n, _ in chosen], universe=len(universe),
                              universe_reached_before=len(universe & before), sampled=len(sampled), sampled_eligible=len([n for n in sampled if four[n] is not None]),
                              smooth_counts_outside_table=len(model_range))
            if v == 3:
                extra_jobs += [(2, n, NTAPS, 0) for n, _ in chosen]
        extra = dict(pool.imap_unordered(_probe, [j for j in extra_jobs if j not in reports], chunksize=1))
    reports.update(extra)
    for e in out["cover"]["3"]:      # antenna 0's pass of the same channel count (the F-only build), for the emulation of both passes
        e["f_report"] = spec_cover.recorded(reports[(2, e["nchan"], NTAPS, 0)])
    out["sample"] = {"counts": {str(v): SAMPLE[v] for v in VARIANTS},
                     "exhaustive": False,
                     "why": "No cheap enumeration of the counts that get a radix outside {2 ... 11, 13, 16, 20, 25}: eligibility and the list taken depend on "
                            "the registers of the compiled candidates, so each count costs a search.  Sampled: counts with the prime factors 17, 19, 23, "
                            "multiples of 32, and a spread of other 23-smooth counts outside the table.  Every other count the cost model serves is NOT covered."}
    out["summary"] = {str(v): summary[v] for v in VARIANTS}
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    for v in VARIANTS:
        s = summary[v]
        print("variant %d (%s): %d table entries, %d (radix, position) pairs of which %d reached by the earlier tests and %d in the cover's universe; "
              "%d features in all (%d reached before); %d table entries not taken by the search; cost model: %d counts sampled (%d eligible) of %d "
              "23-smooth counts outside the table; cover: %s" % (v, spec_cover.VARIANT_TAG[v], s["table_entries"], s["table_pairs"], s["pairs_reached_before"],
                                                                 s["pairs_in_universe"], s["universe"], s["universe_reached_before"], s["not_taken"], s["sampled"],
                                                                 s["sampled_eligible"], s["smooth_counts_outside_table"], s["cover"]))
        if s["static_missing"]:
            print("  table features NO probed build has:", s["static_missing"])
        for d in out["table_entries_not_taken"][str(v)]:
            print("  not taken:", json.dumps(d))


if __name__ == "__main__":
    main()
