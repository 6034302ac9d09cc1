#!/usr/bin/env python3
"""Developer aid: what whole-sample delays cost (include/fxcorr.h fxc_set_sample_delays), on device-resident synthetic chunks.

    python tools/bench_align.py [--reps 8] [--out profiles/align/bench_align.json]

Per shape (2 antennas x 262144 samples x 1024 chunk pairs, 8 x 262144 x 256):
  align_*     the alignment pass alone: fxc_kernel_time of fx_rows with shifts minus fxc_kernel_time of fx_rows without (the F+X
              launches of the two calls are the same kernels on the same number of chunks; the alignment is one more timed launch),
              for even shifts (16-byte aligned source pairs) and odd shifts (8-byte aligned) separately;
  remove_dc   the yardstick: fxc_remove_dc over the same streams, between the plan's stream events (fxc_timer_*).  It reads every
              sample twice (the sum, then the subtraction) and writes it once, 24 bytes a sample against the alignment's 16;
  rows_*      fx_rows end to end at the shape with and without shifts, between the same events.
Medians over --reps, with the spread (min .. max) beside them."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stats(v):
    v = sorted(v)
    return {"median_ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)}


def measure(n_ant, nchan, num_samp, n_chunks, reps):
    import numpy as np
    import torch
    from effex_amd.plan import FxPlan, synth_fill
    x = torch.empty((n_chunks, n_ant, num_samp), dtype=torch.complex64, device="cuda")
    synth_fill(x, 1234)
    out = torch.empty_like(x)
    res = {"n_ant": n_ant, "nchan": nchan, "num_samp": num_samp, "n_chunks": n_chunks, "sample_GB": round(x.numel() * 8 / 1e9, 3)}
    with FxPlan(n_ant, nchan, 4, num_samp) as plan:
        res["path"] = plan.path

        def kernel_ms():
            plan.kernel_time(reset=True)
            plan.fx_rows(x)
            return plan.kernel_time(reset=True)[0]

        def wall_ms(fn):
            plan.timer_start()
            fn()
            return plan.timer_stop()

        shifts = {"none": None, "even": 2 * (np.arange(n_ant) % 3 + 1), "odd": 2 * (np.arange(n_ant) % 3) + 1}
        kern, wall = {}, {}
        for name, s in shifts.items():
            plan.set_sample_delays(s)
            plan.fx_rows(x)          # warm: buffers grown
            plan.sync()
            wall[name] = [wall_ms(lambda: plan.fx_rows(x)) for _ in range(reps)]
            plan.kernel_profiling(True)
            kern[name] = [kernel_ms() for _ in range(reps)]
            plan.kernel_profiling(False)
        plan.set_sample_delays(None)
        plan.remove_dc(x, out=out)
        plan.sync()
        dc = [wall_ms(lambda: plan.remove_dc(x, out=out)) for _ in range(reps)]
    base = sorted(kern["none"])[reps // 2]
    res["fx_kernels_none"] = stats(kern["none"])
    for name in ("even", "odd"):
        a = stats([k - base for k in kern[name]])
        a["GBps_16B_per_sample"] = round(2 * x.numel() * 8 / 1e6 / a["median_ms"], 1) if a["median_ms"] > 0 else None
        res["align_" + name] = a
        res["rows_" + name] = stats(wall[name])
    res["rows_none"] = stats(wall["none"])
    res["remove_dc"] = stats(dc)
    res["remove_dc"]["GBps_24B_per_sample"] = round(3 * x.numel() * 8 / 1e6 / res["remove_dc"]["median_ms"], 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--scale", type=int, default=1, help="divide the chunk counts by this (a quick look)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    results = [measure(2, 4096, 262144, 1024 // args.scale, args.reps), measure(8, 4096, 262144, 256 // args.scale, args.reps)]
    text = json.dumps({"tool": "tools/bench_align.py", "reps": args.reps, "results": results}, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
