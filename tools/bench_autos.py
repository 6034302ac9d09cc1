#!/usr/bin/env python3
"""Developer aid: what the autocorrelation products (include/fxcorr.h fxc_products) cost.  One JSON line per shape:
fx_accumulate of a cross-only plan and of a plan with autos on the same device-resident samples, in one process, timed with the
plans' device events (fxc_timer_*), alternated, after a warm-up, median of `reps`; their ratio; Msamples/s and the fraction of
8 TB/s on the sample bytes; and, for comparison, today's workaround -- fxc_channelize of every antenna into HBM plus a torch
|.|^2 mean over the frames -- timed with torch events.

    python tools/bench_autos.py [--reps 10] [--out profiles/autos/bench_autos.jsonl] [--quick]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# n_ant, nchan, ntaps, num_samp, n_chunks: the headline shape first (2 antennas, 2 048 chunk pairs of 2^18 samples), then a
# few of the other routes
SHAPES = [(2, 4096, 4, 2 ** 18, 2048), (2, 1000, 4, 2 ** 18, 512), (2, 2048, 4, 2 ** 18, 512), (2, 8192, 4, 2 ** 18, 512),
          (2, 1, 4, 2 ** 18, 512), (8, 4096, 4, 2 ** 18, 256)]


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def timed_accumulate(plan, x):
    plan.timer_start()
    plan.fx_accumulate(x)
    ms = plan.timer_stop()
    plan.finalize()
    return ms


def workaround_ms(torch, plan, x):
    """fxc_channelize of all n_chunks * n_ant streams (in slices that fit a few GB) + |.|^2 mean over frames and chunks."""
    n_chunks, n_ant, num_samp = x.shape
    per = max(1, int(4e9 // (n_ant * plan.n_pts * plan.nchan * 8)))
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    acc = torch.zeros((n_ant, plan.nchan), dtype=torch.float64, device=x.device)
    for c0 in range(0, n_chunks, per):
        xs = x[c0:c0 + per].reshape(-1, num_samp)
        spec = plan.channelize(xs).reshape(-1, n_ant, plan.n_pts, plan.nchan)
        acc += (spec.abs() ** 2).sum(dim=(0, 2), dtype=torch.float64)
    acc /= n_chunks * plan.n_pts
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="a quarter of the chunks (a smoke run of the tool)")
    args = ap.parse_args()
    import torch
    from effex_amd.plan import FxPlan, synth_fill
    lines = []
    for n_ant, nchan, ntaps, num_samp, n_chunks in SHAPES:
        if args.quick:
            n_chunks = max(4, n_chunks // 4)
        x = torch.empty((n_chunks, n_ant, num_samp), dtype=torch.complex64, device="cuda")
        synth_fill(x, 1234)
        with FxPlan(n_ant, nchan, ntaps, num_samp) as cross, FxPlan(n_ant, nchan, ntaps, num_samp, autos=True) as autos:
            for _ in range(args.warmup):
                timed_accumulate(cross, x)
                timed_accumulate(autos, x)
            t_cross, t_autos = [], []
            for _ in range(args.reps):
                t_cross.append(timed_accumulate(cross, x))
                t_autos.append(timed_accumulate(autos, x))
            workaround_ms(torch, cross, x)
            t_work = [workaround_ms(torch, cross, x) for _ in range(max(3, args.reps // 3))]
            mc, ma, mw = median(t_cross), median(t_autos), median(t_work)
            samples = n_chunks * n_ant * num_samp
            line = {"n_ant": n_ant, "nchan": nchan, "ntaps": ntaps, "num_samp": num_samp, "n_chunks": n_chunks, "path": cross.path,
                    "n_rows": autos.n_rows, "reps": args.reps, "cross_ms": round(mc, 4), "autos_ms": round(ma, 4),
                    "autos_over_cross": round(ma / mc, 4),
                    "cross_msamples_per_s": round(samples / mc / 1e3, 1), "autos_msamples_per_s": round(samples / ma / 1e3, 1),
                    "cross_frac_of_8TBs": round(samples * 8 / (mc * 1e-3) / 8e12, 4),
                    "autos_frac_of_8TBs": round(samples * 8 / (ma * 1e-3) / 8e12, 4),
                    "workaround_ms": round(mw, 4), "workaround_over_autos": round(mw / ma, 4),
                    "cross_ms_all": [round(v, 4) for v in t_cross], "autos_ms_all": [round(v, 4) for v in t_autos]}
        del x
        torch.cuda.empty_cache()
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
