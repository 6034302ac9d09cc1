#!/usr/bin/env python3
"""Developer aid: what the dedispersion (include/fxcorr.h fxc_dedisperse) costs on device power, beside the same sums in torch: per
trial and series the shifted slices gathered -- ``ts.gather(0, t[:, None] + shifts[d][None, :])`` -- and summed over the channels.
A host clock around whole calls that end in a device synchronisation, after a warm-up, medians of `reps`, the two alternated in
one process; one JSON line per case: random power of 4 series x 4096 channels at n_t 65 536 and of 1 series x 1024 channels at n_t
262 144, with 16, 64 and 256 trials from ``dm_shifts`` for a band (400 MHz at 600 MHz) whose sweep at the last trial is 512
samples.  Each line carries the derived bound of DESIGN.md §3o -- the larger of ceil(n_dm / D) reads of the input from HBM and
n_dm reads of every sample from LDS -- and the share of it the call reaches.  torch adds in another order, so the line says how
far its result is from the library's, not whether the bits agree.

    python tools/bench_dedisperse.py [--reps 5] [--out profiles/dedisperse/bench.jsonl] [--quick]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = [(4, 4096, 65536), (1, 1024, 262144)]      # n_series, nchan, n_t
TRIALS = (16, 64, 256)
SWEEP = 512                                          # samples between the band's edges at the last trial
BW, FC, DM_TOP = 400e6, 600e6, 100.0
D = 8                                                # kDedD: the trials of a tile
HBM_BPS, LDS_B32_BPS = 6.3e12, 75e12                 # achievable HBM rate; ds_read_b32 with every CU streaming


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def torch_dedisperse(torch, power, shifts_dev, n_out):
    """power [n_series, n_t, nchan], shifts_dev int64 [n_dm, nchan] -> float32 [n_series, n_dm, n_out]"""
    n_series, _, nchan = power.shape
    n_dm = shifts_dev.shape[0]
    out = torch.empty((n_series, n_dm, n_out), dtype=torch.float32, device=power.device)
    t = torch.arange(n_out, device=power.device)[:, None]
    for d in range(n_dm):
        idx = t + shifts_dev[d][None, :]
        for s in range(n_series):
            out[s, d] = power[s].gather(0, idx).sum(dim=1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="a sixteenth of the times (a smoke run of the tool)")
    args = ap.parse_args()
    import numpy as np
    import torch
    from effex_amd.plan import FxPlan, dm_shifts
    assert torch.cuda.is_available(), "bench_dedisperse.py measures on the GPU only"
    lines = []
    for n_series, nchan, n_t in CASES:
        if args.quick:
            n_t //= 16
        gen = torch.Generator(device="cuda").manual_seed(2024 + nchan)
        power = torch.rand((n_series, n_t, nchan), generator=gen, device="cuda", dtype=torch.float32) + 0.5
        f = (np.fft.fftshift(np.fft.fftfreq(nchan, d=1.0 / BW)) + FC) / 1e6
        tsamp = 4.148808e3 * DM_TOP * (f.min() ** -2.0 - f.max() ** -2.0) / SWEEP
        with FxPlan(2, nchan, 4, nchan * 8) as plan:
            for n_dm in TRIALS:
                shifts = dm_shifts(nchan, BW, FC, np.linspace(0.0, DM_TOP, n_dm), tsamp)
                assert shifts.max() == SWEEP
                shifts_dev = torch.from_numpy(shifts.astype(np.int64)).cuda()
                n_out = n_t - SWEEP
                t_lib, t_torch = [], []
                for rep in range(args.warmup + args.reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    got, info = plan.dedisperse(power, shifts, return_info=True)
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    want = torch_dedisperse(torch, power, shifts_dev, n_out)
                    torch.cuda.synchronize()
                    t2 = time.perf_counter()
                    if rep >= args.warmup:
                        t_lib.append((t1 - t0) * 1e3)
                        t_torch.append((t2 - t1) * 1e3)
                in_bytes = n_series * n_t * nchan * 4
                hbm_ms = -(-n_dm // D) * in_bytes / HBM_BPS * 1e3
                lds_ms = n_dm * in_bytes / LDS_B32_BPS * 1e3
                bound_ms = max(hbm_ms, lds_ms)
                line = {"kind": "dedisperse", "device": torch.cuda.get_device_name(0), "n_series": n_series, "nchan": nchan, "n_t": n_t,
                        "n_dm": n_dm, "sweep": SWEEP, "reps": args.reps, "trials_tiled": info[0], "trials_direct": info[1],
                        "input_bytes": in_bytes, "dedisperse_ms": round(median(t_lib), 4), "torch_ms": round(median(t_torch), 4),
                        "torch_over_dedisperse": round(median(t_torch) / median(t_lib), 3), "bound_hbm_ms": round(hbm_ms, 4),
                        "bound_lds_ms": round(lds_ms, 4), "bound_over_dedisperse": round(bound_ms / median(t_lib), 3),
                        "adds_per_s": round(n_dm * n_series * n_out * nchan / median(t_lib) * 1e3, 1),
                        "torch_diff_rel": float(((got - want).abs() / want.abs().clamp(min=1e-30)).max()),
                        "dedisperse_ms_all": [round(v, 4) for v in t_lib], "torch_ms_all": [round(v, 4) for v in t_torch]}
                print(json.dumps(line), flush=True)
                lines.append(line)
                del got, want, shifts_dev
        del power
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
