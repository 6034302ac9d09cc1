#!/usr/bin/env python3
"""Developer aid: what a gain solve (include/fxcorr.h fxc_solve_gains) costs on device rows, beside the same computation in
torch on the device: a float64 mean over the chunks, then the same `iters` iterations with batched tensor ops.  Device events,
after a warm-up, median of `reps`, the two forms alternated in one process; one JSON line per case (8 antennas x 4096 channels
x 256 chunks, 64 x 4096 x 64).  The rows are model rows g_a conj(g_b) + noise made on the device.

    python tools/bench_gains.py [--reps 10] [--out profiles/gains/bench_gains.jsonl] [--quick]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/bench_gains.py --reps 3 --no-torch
    python tools/bench_gains.py --merge plain.jsonl --kernel-stats case0.csv --kernel-stats case1.csv --out ...
                                        # no GPU: adds the kernels' times and gains_average_kernel's bytes per second to the lines
"""
import argparse
import csv
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = [(8, 4096, 256), (64, 4096, 64)]      # n_ant, nchan, n_chunks
ITERS = 50
READ_STREAM_TBS = [6.1, 6.5]                  # what a read-only stream reaches on this chip (docs/history.md §4.3)


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def kernel_times(path):
    """{kernel name fragment: [calls, average ns]} of the two gain kernels from a rocprofv3 --stats csv"""
    out = {}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            for name in ("gains_average_kernel", "gains_solve_kernel"):
                if name in row["Name"]:
                    out[name] = [int(row["Calls"]), float(row["AverageNs"]), float(row["MinNs"]), float(row["MaxNs"])]
    return out


def add_kernel_figures(line, stats_csv):
    for name, (calls, avg, lo, hi) in kernel_times(stats_csv).items():
        line[name + "_us"] = round(avg / 1e3, 2)
        line[name + "_us_min_max"] = [round(lo / 1e3, 2), round(hi / 1e3, 2)]
        line[name + "_calls"] = calls
    if "gains_average_kernel_us" in line:
        line["gains_average_kernel_TBs"] = round(line["row_bytes"] / (line["gains_average_kernel_us"] * 1e-6) / 1e12, 3)
        line["read_stream_TBs_recorded"] = READ_STREAM_TBS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="a quarter of the chunks (a smoke run of the tool)")
    ap.add_argument("--no-torch", action="store_true", help="the library's solve alone (for a profiler run)")
    ap.add_argument("--case", type=int, default=None, help="only this case (a profiler run per case gives per-case kernel times)")
    ap.add_argument("--merge", default=None, help="lines of an earlier run to add --kernel-stats to (no GPU)")
    ap.add_argument("--kernel-stats", action="append", default=[], help="rocprofv3 --stats csv of a --no-torch --case run, one per case in order")
    args = ap.parse_args()
    if args.merge:
        lines = [json.loads(ln) for ln in open(args.merge) if ln.strip()]
        for line, stats in zip(lines, args.kernel_stats):
            add_kernel_figures(line, stats)
            print(json.dumps(line), flush=True)
        with open(args.out, "w") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")
        return
    import numpy as np
    import torch
    from effex_amd.plan import FxPlan
    lines = []
    for index, (n_ant, nchan, n_chunks) in enumerate(CASES):
        if args.case is not None and index != args.case:
            continue
        if args.quick:
            n_chunks //= 4
        n_base = n_ant * (n_ant - 1) // 2
        gen = torch.Generator(device="cuda").manual_seed(4321 + n_ant)
        amp = 0.5 + 1.5 * torch.rand((n_ant, nchan), generator=gen, device="cuda", dtype=torch.float64)
        ph = (2.0 * torch.rand((n_ant, nchan), generator=gen, device="cuda", dtype=torch.float64) - 1.0) * np.pi
        g_true = torch.polar(amp, ph)
        ia, ib = torch.triu_indices(n_ant, n_ant, offset=1, device="cuda")
        model = (g_true[ia] * g_true[ib].conj()).to(torch.complex64)
        rows = torch.empty((n_chunks, n_base, nchan), dtype=torch.complex64, device="cuda")
        for c in range(n_chunks):
            noise = torch.randn((n_base, nchan, 2), generator=gen, device="cuda", dtype=torch.float32)
            rows[c] = model + 0.1 * torch.view_as_complex(noise)
        del noise
        off = (1.0 - torch.eye(n_ant, device="cuda", dtype=torch.float64)).to(torch.complex128)

        def torch_solve():
            v = torch.mean(rows, dim=0, dtype=torch.complex128)                       # [n_base, nchan]
            m = torch.zeros((nchan, n_ant, n_ant), dtype=torch.complex128, device="cuda")
            m[:, ia, ib] = v.T
            m[:, ib, ia] = v.T.conj()
            s = m[:, 1:, 0].abs().mean(dim=1)
            g = m[:, :, 0] / torch.sqrt(s)[:, None]
            g[:, 0] = torch.sqrt(s)
            step = None
            for it in range(1, ITERS + 1):
                n = torch.bmm(m, g[:, :, None])[:, :, 0]
                d = torch.matmul((g.abs() ** 2).to(torch.complex128), off)
                new = n / d
                if it % 2 == 0:
                    new = (new + g) / 2.0
                if it == ITERS:
                    step = torch.sqrt(((new - g).abs() ** 2).sum(dim=1) / (new.abs() ** 2).sum(dim=1))
                g = new
            u = g[:, 0].conj() / g[:, 0].abs()
            return (g * u[:, None]).T.contiguous(), step

        with FxPlan(n_ant, nchan, 4, nchan * 8) as plan:
            t_lib, t_torch = [], []
            for rep in range(args.warmup + args.reps):
                plan.timer_start()
                g, step = plan.solve_gains(rows, iters=ITERS)
                ms_lib = plan.timer_stop()
                if args.no_torch:
                    ms_torch = float("nan")
                else:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    tg, tstep = torch_solve()
                    e1.record()
                    e1.synchronize()
                    ms_torch = e0.elapsed_time(e1)
                if rep >= args.warmup:
                    t_lib.append(ms_lib)
                    t_torch.append(ms_torch)
        row_bytes = n_chunks * n_base * nchan * 8
        line = {"kind": "solve_gains", "n_ant": n_ant, "nchan": nchan, "n_chunks": n_chunks, "iters": ITERS, "reps": args.reps,
                "row_bytes": row_bytes, "solve_gains_ms": round(median(t_lib), 4),
                "step_max": float(step.max()), "truth_rel": float(np.abs(g[0] - (g_true * (g_true[0].conj() / g_true[0].abs())[None]).cpu().numpy()).max()),
                "solve_gains_ms_all": [round(v, 4) for v in t_lib]}
        if not args.no_torch:
            tg = tg.cpu().numpy()
            line.update({"torch_ms": round(median(t_torch), 4), "torch_over_solve_gains": round(median(t_torch) / median(t_lib), 3),
                         "torch_agrees_rel": float(np.abs(tg - g[0]).max() / np.abs(g[0]).max()),
                         "torch_ms_all": [round(v, 4) for v in t_torch]})
        print(json.dumps(line), flush=True)
        lines.append(line)
        del rows, model
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if args.case is not None else "w") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
