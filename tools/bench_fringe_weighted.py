#!/usr/bin/env python3
"""Developer aid: what the weighted fringe fit (include/fxcorr.h fxc_fringe_fit_weighted) costs beside the plain one, and all
baselines beside the baselines to ref.  Device rows and device weights (random 0/1, density 0.9), device events after a warm-up,
median of `reps`, the three fits alternated in one process; one JSON line per case (8 antennas x 4096 channels x 256 chunks,
64 x 4096 x 64; pad 2), in ms and in ms per fitted baseline.

    python tools/bench_fringe_weighted.py [--reps 10] [--out profiles/fringe_weighted/bench.jsonl] [--quick]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = [(8, 4096, 256), (64, 4096, 64)]      # n_ant, nchan, n_chunks
BW, FREQ, PAD = 2.4e6, 1.4204e9, 2


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="a quarter of the chunks (a smoke run of the tool)")
    args = ap.parse_args()
    import torch
    from effex_amd.plan import FxPlan
    lines = []
    for n_ant, nchan, n_chunks in CASES:
        if args.quick:
            n_chunks //= 4
        gen = torch.Generator(device="cuda").manual_seed(4321)
        with FxPlan(n_ant, nchan, 4, nchan * 8) as plan:
            n_base = plan.n_baselines
            # a common fringe on every baseline over unit noise: every fit has a peak to find
            t = torch.arange(n_chunks, device="cuda", dtype=torch.float32)[:, None, None]
            k = torch.arange(nchan, device="cuda", dtype=torch.float32)[None, None, :]
            rows = torch.randn((n_chunks, plan.n_rows, nchan), generator=gen, device="cuda", dtype=torch.complex64)
            rows += torch.polar(torch.ones_like(rows.real), 6.2831853 * (0.11 * k + 0.07 * t))
            weights = (torch.rand((n_chunks, n_base, nchan), generator=gen, device="cuda") < 0.9).to(torch.float32)
            calls = {"plain_ref": dict(), "weighted_ref": dict(weights=weights), "weighted_all": dict(weights=weights, baselines="all")}
            times = {name: [] for name in calls}
            for rep in range(args.warmup + args.reps):
                for name, kw in calls.items():
                    plan.timer_start()
                    plan.fringe_fit(rows, BW, FREQ, pad=PAD, **kw)
                    ms = plan.timer_stop()
                    if rep >= args.warmup:
                        times[name].append(ms)
            fits = {"plain_ref": n_ant - 1, "weighted_ref": n_ant - 1, "weighted_all": n_base}
            line = {"kind": "fringe_fit_weighted", "n_ant": n_ant, "nchan": nchan, "n_chunks": n_chunks, "pad": PAD, "reps": args.reps,
                    "device": torch.cuda.get_device_name(0)}
            for name in calls:
                line[name + "_ms"] = round(median(times[name]), 4)
                line[name + "_ms_per_baseline"] = round(median(times[name]) / fits[name], 4)
                line[name + "_fits"] = fits[name]
                line[name + "_ms_all"] = [round(v, 4) for v in times[name]]
        print(json.dumps(line), flush=True)
        lines.append(line)
        del rows, weights
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
