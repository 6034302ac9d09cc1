#!/usr/bin/env python3
"""Developer aid: what the averager (include/fxcorr.h fxc_average_rows) costs on device rows, beside the same computation in torch
(float64 sums over the chunks with flagged samples set to zero, a reshape and a sum over the bins of an output bin, one division).
A host clock around whole calls that end in a device synchronisation, after a warm-up, medians of `reps`, the two alternated in
one process; one JSON line per case (8 antennas x 4096 channels x 256 chunks and 64 x 4096 x 64, at freq_bin 1 and 8, with and
without weights) with the bytes the call has to move (rows 8 B a sample in, weights 4 B where there are any, 12 B per output cell
out), its time and the rate the two give.  That rate is of the whole call -- the kernel, the allocation of the two results and the
synchronisation -- not of the kernel; DESIGN.md §3e has `gains_average_kernel`'s rate on rows of the same shapes.  torch adds in
another order, so the line says how far its result is from the library's, not whether the bits agree.

    python tools/bench_average.py [--reps 10] [--out profiles/average/bench.jsonl] [--quick]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = [(8, 4096, 256), (64, 4096, 64)]      # n_ant, nchan, n_chunks
FREQ_BINS = (1, 8)
BLOCK = 64                                    # baselines per torch pass: bounds its float64 temporaries


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def torch_average(torch, rows, weights, freq_bin):
    """the definition at time_bin 0 in torch (nchan a multiple of freq_bin): -> vis complex64, wsum float32 [1, nb, n_out]"""
    n, nb, nchan = rows.shape
    n_out = nchan // freq_bin
    vis = torch.empty((1, nb, n_out), dtype=torch.complex64, device=rows.device)
    wsum = torch.empty((1, nb, n_out), dtype=torch.float32, device=rows.device)
    for b0 in range(0, nb, BLOCK):
        part = rows[:, b0:b0 + BLOCK]
        if weights is None:
            s = part.to(torch.complex128).sum(dim=0)
            w = torch.full(s.shape, float(n), dtype=torch.float64, device=rows.device)
        else:
            wp = weights[:, b0:b0 + BLOCK]
            ok = wp > 0
            wd = torch.where(ok, wp, 0.0).double()
            s = torch.complex((wd * torch.where(ok, part.real, 0.0).double()).sum(dim=0), (wd * torch.where(ok, part.imag, 0.0).double()).sum(dim=0))
            w = wd.sum(dim=0)
        s = s.reshape(s.shape[0], n_out, freq_bin).sum(dim=2)
        w = w.reshape(w.shape[0], n_out, freq_bin).sum(dim=2)
        live = w > 0
        div = torch.where(live, w, 1.0)
        vis[0, b0:b0 + BLOCK] = torch.where(live, s / div, 0.0).to(torch.complex64)
        wsum[0, b0:b0 + BLOCK] = w.float()
    return vis, wsum


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="a quarter of the channels (a smoke run of the tool)")
    args = ap.parse_args()
    import torch
    from effex_amd.plan import FxPlan
    assert torch.cuda.is_available(), "bench_average.py measures on the GPU only"
    lines = []
    for n_ant, nchan, n_chunks in CASES:
        if args.quick:
            nchan //= 4
        n_base = n_ant * (n_ant - 1) // 2
        gen = torch.Generator(device="cuda").manual_seed(1987 + n_ant)
        centre = torch.view_as_complex(2.0 * torch.randn((n_base, nchan, 2), generator=gen, device="cuda", dtype=torch.float32))
        rows = torch.empty((n_chunks, n_base, nchan), dtype=torch.complex64, device="cuda")
        weights = torch.empty((n_chunks, n_base, nchan), dtype=torch.float32, device="cuda")
        for c in range(n_chunks):
            noise = torch.view_as_complex(torch.randn((n_base, nchan, 2), generator=gen, device="cuda", dtype=torch.float32))
            rows[c] = centre + 0.3 * noise
            w = 0.25 + 3.75 * torch.rand((n_base, nchan), generator=gen, device="cuda")
            weights[c] = torch.where(torch.rand((n_base, nchan), generator=gen, device="cuda") < 0.2, 0.0, w)
        del noise, w
        with FxPlan(n_ant, nchan, 4, nchan * 8) as plan:
            for freq_bin in FREQ_BINS:
                for weighted in (False, True):
                    wts = weights if weighted else None
                    t_lib, t_torch = [], []
                    for rep in range(args.warmup + args.reps):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        vis, wsum = plan.average_rows(rows, weights=wts, freq_bin=freq_bin)
                        torch.cuda.synchronize()
                        t1 = time.perf_counter()
                        vis_t, wsum_t = torch_average(torch, rows, wts, freq_bin)
                        torch.cuda.synchronize()
                        t2 = time.perf_counter()
                        if rep >= args.warmup:
                            t_lib.append((t1 - t0) * 1e3)
                            t_torch.append((t2 - t1) * 1e3)
                    scale = float(vis.abs().max())
                    samples = n_chunks * n_base * nchan
                    moved = samples * (12 if weighted else 8) + n_base * (nchan // freq_bin) * 12
                    line = {"kind": "average_rows", "device": torch.cuda.get_device_name(0), "n_ant": n_ant, "nchan": nchan,
                            "n_chunks": n_chunks, "time_bin": 0, "freq_bin": freq_bin, "weights": weighted, "reps": args.reps,
                            "bytes_moved": moved, "average_rows_ms": round(median(t_lib), 4),
                            "average_rows_call_gbps": round(moved / median(t_lib) / 1e6, 1), "torch_ms": round(median(t_torch), 4),
                            "torch_over_average_rows": round(median(t_torch) / median(t_lib), 3),
                            "torch_vis_diff_rel": float((vis - vis_t).abs().max()) / scale,
                            "torch_wsum_diff_rel": float(((wsum - wsum_t).abs() / wsum.clamp(min=1e-30)).max()),
                            "average_rows_ms_all": [round(v, 4) for v in t_lib], "torch_ms_all": [round(v, 4) for v in t_torch]}
                    print(json.dumps(line), flush=True)
                    lines.append(line)
                    del vis, wsum, vis_t, wsum_t
        del rows, weights
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
