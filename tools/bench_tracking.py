#!/usr/bin/env python3
"""Developer aid: what a delay track (include/fxcorr.h fxc_set_delay_track) costs.  Every time is taken with the plan's device
events (fxc_timer_*, HIP events on the plan's stream), after a warm-up, median of `reps`, tracked and static alternated in one
process; one JSON line per measurement:

  kind "rows":       fx_rows (SPECTRUM) with a static table (2 antennas: fxc_set_rot; more: fxc_set_rot_ant) against the same
                     call under a track (2 antennas x 4096 channels, 8 and 64 antennas x 4096);
  kind "integrate":  fx_accumulate + finalize under a track against (a) the static fx_accumulate + finalize and (b) the static
                     fx_rows of the same chunks -- the route the tracked integration runs (headline shape with 2048 resident
                     chunk pairs; 8 antennas);
  kind "dropin":     Correlator(mode='TEST') over an in-memory source, batch=1 against batch=64 with device_sweep=True, rows/s
                     (host clock around the whole run: the drop-in's own loop is what is compared).

    python tools/bench_tracking.py [--reps 10] [--out profiles/tracking/bench_tracking.jsonl] [--quick]
"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROWS = [(2, 4096, 262144, 512), (8, 4096, 4096 * 64, 16), (64, 4096, 4096 * 16, 4)]     # n_ant, nchan, num_samp, n_chunks
INTEGRATE = [(2, 4096, 262144, 2048), (8, 4096, 4096 * 64, 64)]
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
    from effex_amd.plan import FxPlan, rot_tables, synth_fill
    lines = []

    def emit(line):
        print(json.dumps(line), flush=True)
        lines.append(line)

    def alternate(plan, cases):
        """cases: name -> (setup, fn); every rep runs each case once, in turn"""
        times = {name: [] for name in cases}
        for rep in range(args.warmup + args.reps):
            for name, (setup, fn) in cases.items():
                setup()
                plan.timer_start()
                fn()
                ms = plan.timer_stop()
                if rep >= args.warmup:
                    times[name].append(ms)
        return {name: median(v) for name, v in times.items()}

    def track_of(n_ant):
        a = np.arange(n_ant)
        return 1e-6 * ((3 * a * a) % 17) / 17.0, 1e-10 * ((5 * a) % 7 - 2.5)

    for kind, shapes in (("rows", ROWS), ("integrate", INTEGRATE)):
        for n_ant, nchan, num_samp, n_chunks in shapes:
            if args.quick:
                n_chunks = max(2, n_chunks // 16)
            x = torch.empty((n_chunks, n_ant, num_samp), dtype=torch.complex64, device="cuda")
            synth_fill(x, 7, delays=[a % 5 for a in range(n_ant)])
            tau0, rate = track_of(n_ant)
            with FxPlan(n_ant, nchan, 4, num_samp) as plan:
                out = plan.fx_rows(x, "SPECTRUM")

                def static():
                    plan.set_rot_ant(rot_tables(nchan, BW, FREQ, tau0))

                def tracked():
                    plan.set_delay_track(tau0, rate, BW, FREQ)

                def rows():
                    plan.fx_rows(x, "SPECTRUM", out=out)

                def integrate():
                    plan.fx_accumulate(x)
                    plan.finalize_async("SPECTRUM")
                    plan.finalize_wait()

                if kind == "rows":
                    ms = alternate(plan, {"static": (static, rows), "tracked": (tracked, rows)})
                else:
                    ms = alternate(plan, {"static_accumulate": (static, integrate), "static_rows": (static, rows),
                                          "tracked_accumulate": (tracked, integrate)})
                line = {"kind": kind, "n_ant": n_ant, "nchan": nchan, "num_samp": num_samp, "n_chunks": n_chunks, "path": plan.path,
                        "reps": args.reps, "ms": ms, "msamples_per_s": {k: n_chunks * num_samp / v / 1e3 for k, v in ms.items()}}
                if kind == "rows":
                    line["tracked_over_static"] = ms["tracked"] / ms["static"]
                else:
                    line["tracked_over_static_accumulate"] = ms["tracked_accumulate"] / ms["static_accumulate"]
                    line["tracked_over_static_rows"] = ms["tracked_accumulate"] / ms["static_rows"]
                emit(line)
            del x, out

    from effex_amd import synth
    from effex_amd.correlator import ArraySource, Correlator
    num_samp, n_pairs = 4096 * 16, (66 if args.quick else 1025)
    chunks = synth.synth_iq(3, n_pairs, 2, num_samp)
    with tempfile.TemporaryDirectory() as tmp:
        rate = {}
        for name, kw in (("batch1", dict(batch=1)), ("batch64_device_sweep", dict(batch=64, device_sweep=True))):
            best = []
            for rep in range(3):
                cor = Correlator(num_samp=num_samp, nbins=4096, source=ArraySource(chunks), mode='TEST',
                                 output_file=os.path.join(tmp, "%s_%d.csv" % (name, rep)), loglevel='WARNING', **kw)
                t0 = time.perf_counter()
                n_rows = cor.run_state_machine()
                best.append(n_rows / (time.perf_counter() - t0))
            rate[name] = max(best)
        emit({"kind": "dropin", "mode": "TEST", "num_samp": num_samp, "nbins": 4096, "rows": n_pairs - 1, "rows_per_s": rate,
              "speedup": rate["batch64_device_sweep"] / rate["batch1"]})

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
