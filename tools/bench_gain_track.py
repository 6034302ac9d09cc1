#!/usr/bin/env python3
"""Developer aid: what a gain track (include/fxcorr.h fxc_set_track_gains) costs on top of a delay track.  Every time is taken
with the plan's device events (fxc_timer_*, HIP events on the plan's stream), after a warm-up, median of `reps`, the plain track
and the track with gains alternated in one process; one JSON line per shape and kind:

  kind "rows":       tracked fx_rows (SPECTRUM) without and with a gain track of 4 solutions;
  kind "integrate":  tracked fx_accumulate + finalize without and with it.

The shapes are those of tools/bench_tracking.py's rows: 2 antennas x 4096 channels with 512 chunks of 262144 samples, 8 x 4096
with 16 chunks, 64 x 4096 with 4 chunks.  The comparison column is the plain track on the same build: without a gain track that
build launches track_tables_kernel as before.

    python tools/bench_gain_track.py [--reps 10] [--out profiles/gain_track/bench_gain_track.jsonl] [--quick]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(2, 4096, 262144, 512), (8, 4096, 4096 * 64, 16), (64, 4096, 4096 * 16, 4)]     # n_ant, nchan, num_samp, n_chunks
N_SOLUTIONS = 4
BW, FREQ = 2.4e6, 1.42e9


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="fewer chunks (a smoke run of the tool)")
    args = ap.parse_args()
    import numpy as np
    import torch
    from effex_amd.plan import FxPlan, synth_fill
    lines = []

    def track_of(n_ant):
        a = np.arange(n_ant)
        return 1e-6 * ((3 * a * a) % 17) / 17.0, 1e-10 * ((5 * a) % 7 - 2.5)

    for n_ant, nchan, num_samp, n_chunks in SHAPES:
        if args.quick:
            n_chunks = max(2, n_chunks // 16)
        x = torch.empty((n_chunks, n_ant, num_samp), dtype=torch.complex64, device="cuda")
        synth_fill(x, 7, delays=[a % 5 for a in range(n_ant)])
        tau0, rate = track_of(n_ant)
        rng = np.random.default_rng(n_ant)
        gains = rng.uniform(0.5, 2.0, (N_SOLUTIONS, n_ant, nchan)) * np.exp(1j * rng.uniform(-np.pi, np.pi, (N_SOLUTIONS, n_ant, nchan)))
        interval = max(1, n_chunks // N_SOLUTIONS)
        with FxPlan(n_ant, nchan, 4, num_samp) as plan:
            out = plan.fx_rows(x, "SPECTRUM")
            plan.set_delay_track(tau0, rate, BW, FREQ)

            def plain():
                plan.set_track_gains(None)
                plan.track_seek(0)

            def with_gains():
                plan.set_track_gains(gains, interval=interval)
                plan.track_seek(0)

            def rows():
                plan.fx_rows(x, "SPECTRUM", out=out)

            def integrate():
                plan.fx_accumulate(x)
                plan.finalize_async("SPECTRUM")
                plan.finalize_wait()

            for kind, fn in (("rows", rows), ("integrate", integrate)):
                times = {"track": [], "track_gains": []}
                for rep in range(args.warmup + args.reps):
                    for name, setup in (("track", plain), ("track_gains", with_gains)):
                        setup()                     # (outside the timed region: it synchronises and uploads)
                        plan.timer_start()
                        fn()
                        ms = plan.timer_stop()
                        if rep >= args.warmup:
                            times[name].append(ms)
                ms = {name: median(v) for name, v in times.items()}
                line = {"kind": kind, "n_ant": n_ant, "nchan": nchan, "num_samp": num_samp, "n_chunks": n_chunks, "path": plan.path,
                        "n_solutions": N_SOLUTIONS, "interval": interval, "reps": args.reps, "ms": ms,
                        "msamples_per_s": {k: n_chunks * num_samp / v / 1e3 for k, v in ms.items()},
                        "gains_over_track": ms["track_gains"] / ms["track"], "device": torch.cuda.get_device_name(0)}
                print(json.dumps(line), flush=True)
                lines.append(line)
        del x, out

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
