#!/usr/bin/env python3
"""Developer aid: what per-antenna delay correction and one-call delay calibration (include/fxcorr.h fxc_set_rot_ant,
fxc_estimate_delays) cost.  Every time is taken with the plan's device events (fxc_timer_*, HIP events on the plan's stream),
after a warm-up, median of `reps`; one JSON line per measurement:

  kind "calibration": fxc_estimate_delays of n_ant device-resident streams of n samples against the n_ant - 1 pairwise
                      fxc_estimate_delay calls that give the same delays (8 and 64 antennas, n = 262144);
  kind "finish":      fx_rows (SPECTRUM) and finalize (SPECTRUM, an accumulator with nothing pending: the finishing kernel alone)
                      with the shared rot table against per-antenna tables (8 and 64 antennas, 4096 channels).

    python tools/bench_delays.py [--reps 10] [--out profiles/delays/bench_delays.jsonl] [--quick]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CALIBRATION = [(8, 262144), (64, 262144)]            # n_ant, n
FINISH = [(8, 4096, 4096 * 64, 16), (64, 4096, 4096 * 16, 4)]   # n_ant, nchan, num_samp, n_chunks
RATE, BW, FREQ = 2.4e6, 2.4e6, 1.4204e9


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def timed(plan, fn, reps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        plan.timer_start()
        fn()
        out.append(plan.timer_stop())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="fewer samples and chunks (a smoke run of the tool)")
    args = ap.parse_args()
    import numpy as np
    import torch
    from effex_amd.plan import FxPlan, synth_fill
    lines = []

    def emit(line):
        print(json.dumps(line), flush=True)
        lines.append(line)

    for n_ant, n in CALIBRATION:
        if args.quick:
            n //= 16
        x = torch.empty((1, n_ant, n), dtype=torch.complex64, device="cuda")
        synth_fill(x, 99, delays=[(5 * a) % 41 for a in range(n_ant)])
        x = x[0]
        with FxPlan(n_ant, 512, 4, 4096) as plan:
            batched = timed(plan, lambda: plan.estimate_delays(x, RATE), args.reps, args.warmup)
            pairwise = timed(plan, lambda: [plan.estimate_delay(x[0], x[a], RATE) for a in range(1, n_ant)], args.reps, args.warmup)
            same = bool(np.array_equal(plan.estimate_delays(x, RATE)[1:],
                                       np.array([plan.estimate_delay(x[0], x[a], RATE) for a in range(1, n_ant)])))
        mb, mp = median(batched), median(pairwise)
        emit({"kind": "calibration", "n_ant": n_ant, "n": n, "reps": args.reps, "estimate_delays_ms": round(mb, 4),
              "pairwise_ms": round(mp, 4), "pairwise_over_batched": round(mp / mb, 3), "bit_identical": same,
              "estimate_delays_ms_all": [round(v, 4) for v in batched], "pairwise_ms_all": [round(v, 4) for v in pairwise]})
        del x
        torch.cuda.empty_cache()

    for n_ant, nchan, num_samp, n_chunks in FINISH:
        if args.quick:
            n_chunks = max(2, n_chunks // 4)
        x = torch.empty((n_chunks, n_ant, num_samp), dtype=torch.complex64, device="cuda")
        synth_fill(x, 1234, delays=[a % 8 for a in range(n_ant)])
        tau = np.arange(n_ant) * 1.3e-7
        with FxPlan(n_ant, nchan, 4, num_samp) as plan:
            out = torch.empty((n_chunks, plan.n_baselines, nchan), dtype=torch.complex64, device="cuda")
            res = {}
            for name in ("shared", "per_antenna"):
                if name == "shared":
                    plan.set_delay(BW, FREQ, tau[1])
                else:
                    plan.set_delays(tau, BW, FREQ)
                res[name + "_rows"] = timed(plan, lambda: plan.fx_rows(x, "SPECTRUM", out=out), args.reps, args.warmup)
                plan.fx_accumulate(x)
                plan.finalize("SPECTRUM", reset=False)          # the fold of the pending rows: not part of what is timed
                res[name + "_finalize"] = timed(plan, lambda: plan.finalize("SPECTRUM", reset=False), args.reps, args.warmup)
                plan.acc_reset()
        line = {"kind": "finish", "n_ant": n_ant, "nchan": nchan, "num_samp": num_samp, "n_chunks": n_chunks, "path": plan.path,
                "reps": args.reps}
        for k, v in res.items():
            line[k + "_ms"] = round(median(v), 4)
        line["rows_ratio"] = round(median(res["per_antenna_rows"]) / median(res["shared_rows"]), 4)
        line["finalize_ratio"] = round(median(res["per_antenna_finalize"]) / median(res["shared_finalize"]), 4)
        for k, v in res.items():
            line[k + "_ms_all"] = [round(t, 4) for t in v]
        emit(line)
        del x, out
        torch.cuda.empty_cache()

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
