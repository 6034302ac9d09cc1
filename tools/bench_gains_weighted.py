#!/usr/bin/env python3
"""Developer aid: what the weighted gain solve (include/fxcorr.h fxc_solve_gains_weighted) costs beside the unweighted one on the
same device rows.  Plan device events, after a warm-up, medians of `reps`, the two calls alternated in one process; one JSON line
per case (8 antennas x 4096 channels x 256 chunks, 64 x 4096 x 64) with the bytes each call reads (rows 8 B an element, weights
4 B, the model once) and its time.  The weighted call runs with weights and one model.  The times are those of whole calls: both
kernels, the copy of the result to the host and the synchronisation.

    python tools/bench_gains_weighted.py [--reps 10] [--out profiles/gains_weighted/bench.jsonl] [--quick]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = [(8, 4096, 256), (64, 4096, 64)]      # n_ant, nchan, n_chunks
ITERS = 50


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
    import numpy as np
    import torch
    from effex_amd.plan import FxPlan
    lines = []
    for n_ant, nchan, n_chunks in CASES:
        if args.quick:
            n_chunks //= 4
        n_base = n_ant * (n_ant - 1) // 2
        gen = torch.Generator(device="cuda").manual_seed(4321 + n_ant)
        amp = 0.5 + 1.5 * torch.rand((n_ant, nchan), generator=gen, device="cuda", dtype=torch.float64)
        ph = (2.0 * torch.rand((n_ant, nchan), generator=gen, device="cuda", dtype=torch.float64) - 1.0) * np.pi
        g_true = torch.polar(amp, ph)
        ia, ib = torch.triu_indices(n_ant, n_ant, offset=1, device="cuda")
        vis = (g_true[ia] * g_true[ib].conj()).to(torch.complex64)
        rows = torch.empty((n_chunks, n_base, nchan), dtype=torch.complex64, device="cuda")
        weights = torch.empty((n_chunks, n_base, nchan), dtype=torch.float32, device="cuda")
        for c in range(n_chunks):
            noise = torch.randn((n_base, nchan, 2), generator=gen, device="cuda", dtype=torch.float32)
            rows[c] = vis + 0.1 * torch.view_as_complex(noise)
            w = 0.25 + 3.75 * torch.rand((n_base, nchan), generator=gen, device="cuda", dtype=torch.float32)
            w[torch.rand((n_base, nchan), generator=gen, device="cuda") < 0.2] = 0
            weights[c] = w
        del noise, w
        model = np.ones((n_base, nchan), np.complex64)
        with FxPlan(n_ant, nchan, 4, nchan * 8) as plan:
            t_plain, t_weighted = [], []
            for rep in range(args.warmup + args.reps):
                plan.timer_start()
                g0, step0 = plan.solve_gains(rows, iters=ITERS)
                ms_plain = plan.timer_stop()
                plan.timer_start()
                g1, step1 = plan.solve_gains(rows, iters=ITERS, weights=weights, model=model)
                ms_weighted = plan.timer_stop()
                if rep >= args.warmup:
                    t_plain.append(ms_plain)
                    t_weighted.append(ms_weighted)
        elems = n_chunks * n_base * nchan
        truth = (g_true * (g_true[0].conj() / g_true[0].abs())[None]).cpu().numpy()
        line = {"kind": "solve_gains_weighted", "device": torch.cuda.get_device_name(0), "n_ant": n_ant, "nchan": nchan,
                "n_chunks": n_chunks, "iters": ITERS, "reps": args.reps,
                "unweighted_bytes_read": elems * 8, "weighted_bytes_read": elems * 12 + n_base * nchan * 8,
                "unweighted_ms": round(median(t_plain), 4), "weighted_ms": round(median(t_weighted), 4),
                "weighted_over_unweighted": round(median(t_weighted) / median(t_plain), 3),
                "unweighted_truth_rel": float(np.abs(g0[0] - truth).max()), "weighted_truth_rel": float(np.abs(g1[0] - truth).max()),
                "unweighted_ms_all": [round(v, 4) for v in t_plain], "weighted_ms_all": [round(v, 4) for v in t_weighted]}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del rows, weights, vis
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
