#!/usr/bin/env python3
"""Developer aid: what a fringe fit (include/fxcorr.h fxc_fringe_fit) costs, beside the fx_rows call that made its rows and beside
the same fit done with torch.fft.fft2 + argmax on the device (which writes the padded 2-D spectrum to HBM and reads it back: the
alternative to the fused time-axis kernel of k_fringe.h).  Device events, after a warm-up, median of `reps`, the two fits
alternated in one process; one JSON line per case (8 antennas x 4096 channels x 256 chunks, 64 x 4096 x 64; pad 2).

    python tools/bench_fringe.py [--reps 10] [--out profiles/fringe/bench_fringe.jsonl] [--quick]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = [(8, 4096, 4096 * 8, 256), (64, 4096, 4096 * 8, 64)]      # n_ant, nchan, num_samp, n_chunks
BW, FREQ, PAD = 2.4e6, 1.4204e9, 2


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def pow2(n):
    p = 1
    while p < n:
        p *= 2
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="a quarter of the chunks (a smoke run of the tool)")
    args = ap.parse_args()
    import numpy as np
    import torch
    from effex_amd.plan import FxPlan, synth_fill
    lines = []
    for n_ant, nchan, num_samp, n_chunks in CASES:
        if args.quick:
            n_chunks //= 4
        x = torch.empty((n_chunks, n_ant, num_samp), dtype=torch.complex64, device="cuda")
        synth_fill(x, 4321, delays=[(3 * a) % 17 for a in range(n_ant)])
        lk, lt = pow2(PAD * nchan), pow2(PAD * n_chunks)
        with FxPlan(n_ant, nchan, 4, num_samp) as plan:
            rows = torch.empty((n_chunks, plan.n_rows, nchan), dtype=torch.complex64, device="cuda")
            t_rows, t_fit, t_torch = [], [], []

            def torch_fit():
                # baselines (0, b) are the first n_ant - 1 rows; the whole padded spectrum goes through HBM
                spec = torch.fft.fft2(rows[:, :n_ant - 1], s=(lt, lk), dim=(0, 2))
                return torch.argmax(spec.abs().permute(1, 0, 2).reshape(n_ant - 1, -1), dim=1)

            for rep in range(args.warmup + args.reps):
                plan.timer_start()
                plan.fx_rows(x, "SPECTRUM", out=rows)
                ms_rows = plan.timer_stop()
                plan.timer_start()
                d, r, s = plan.fringe_fit(rows, BW, FREQ, pad=PAD)
                ms_fit = plan.timer_stop()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                peak = torch_fit()
                e1.record()
                e1.synchronize()
                if rep >= args.warmup:
                    t_rows.append(ms_rows)
                    t_fit.append(ms_fit)
                    t_torch.append(e0.elapsed_time(e1))
            peak = peak.cpu().numpy()
            q0, m0 = peak // lk, peak % lk
            m_fit = np.rint(d[1:] * lk * BW / nchan).astype(np.int64) % lk
            q_fit = np.rint(r[1:] * lt * FREQ).astype(np.int64) % lt
            line = {"kind": "fringe_fit", "n_ant": n_ant, "nchan": nchan, "num_samp": num_samp, "n_chunks": n_chunks, "pad": PAD,
                    "Lk": lk, "Lt": lt, "path": plan.path, "reps": args.reps,
                    "fx_rows_ms": round(median(t_rows), 4), "fringe_fit_ms": round(median(t_fit), 4),
                    "torch_fft2_argmax_ms": round(median(t_torch), 4),
                    "torch_over_fringe_fit": round(median(t_torch) / median(t_fit), 3),
                    "fringe_fit_over_fx_rows": round(median(t_fit) / median(t_rows), 3),
                    # cells within one of torch's float32 peak (the sub-cell offset rounds either way at half a cell)
                    "peaks_agree": bool(np.all(np.minimum((m_fit - m0) % lk, (m0 - m_fit) % lk) <= 1)
                                        and np.all(np.minimum((q_fit - q0) % lt, (q0 - q_fit) % lt) <= 1)),
                    "snr_min": round(float(s[1:].min()), 3),
                    "fx_rows_ms_all": [round(v, 4) for v in t_rows], "fringe_fit_ms_all": [round(v, 4) for v in t_fit],
                    "torch_fft2_argmax_ms_all": [round(v, 4) for v in t_torch]}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del x, rows
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
