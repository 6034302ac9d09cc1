#!/usr/bin/env python3
"""Developer aid: what the detector (include/fxcorr.h fxc_flag_rows) costs on device rows, beside the same computation in torch
(`torch.nanmedian` is the lower median over the values that are not NaN).  A host clock around whole calls that end in a device
synchronisation, after a warm-up, medians of `reps`, the two alternated in one process; one JSON line per case (8 antennas x 4096
channels x 256 chunks, 64 x 4096 x 64) with the bytes the call has to move (rows 8 B a sample in, weights 4 B out), its time and
the rate the two give.  That rate is of the whole call -- both kernels, the allocation of the result and the copy of the counts --
not of a kernel; DESIGN.md §3e has `gains_average_kernel`'s rate on rows of the same shapes.  The line also says whether torch's
weights equal the library's.

    python tools/bench_flag.py [--reps 10] [--out profiles/flag/bench.jsonl] [--quick]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = [(8, 4096, 256), (64, 4096, 64)]      # n_ant, nchan, n_chunks
TIME_THRESHOLD, FREQ_THRESHOLD, HALF_WIDTH, ITERS = 20.0, 8.0, 8, 2
BLOCK = 128                                   # baselines per torch pass: bounds its temporaries


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def torch_flag(torch, rows):
    """the definition with defaults, one window, no prior, in torch: -> weights float32 [n_chunks, n_baselines, nchan]"""
    nan = float("nan")
    out = torch.empty(rows.shape, dtype=torch.float32, device=rows.device)
    for b0 in range(0, rows.shape[1], BLOCK):
        part = rows[:, b0:b0 + BLOCK]
        x, y = part.real, part.imag
        live = torch.isfinite(x) & torch.isfinite(y) & ~((x == 0) & (y == 0))
        for it in range(ITERS + 1):
            mx = torch.nanmedian(torch.where(live, x, nan), dim=0).values
            my = torch.nanmedian(torch.where(live, y, nan), dim=0).values
            dx, dy = (x - mx).double(), (y - my).double()
            e = (dx * dx + dy * dy).float()
            d = torch.nanmedian(torch.where(live, e, nan), dim=0).values
            if it < ITERS:
                live &= ~((d > 0) & (e > TIME_THRESHOLD * d))
        defined = live.any(dim=0)
        level = (mx.double() * mx.double() + my.double() * my.double()).float()
        outlier = torch.zeros_like(defined)
        for plane, two_sided in ((level, True), (d, False)):
            padded = torch.nn.functional.pad(torch.where(defined, plane, nan), (HALF_WIDTH, HALF_WIDTH), value=nan)
            win = padded.unfold(-1, 2 * HALF_WIDTH + 1, 1)
            r = torch.nanmedian(win, dim=-1).values
            s = torch.nanmedian((win - r[..., None]).abs(), dim=-1).values
            diff = plane - r
            if two_sided:
                diff = diff.abs()
            outlier |= defined & (s > 0) & (diff > FREQ_THRESHOLD * s)
        live &= ~outlier
        out[:, b0:b0 + BLOCK] = live.float()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="a quarter of the channels (a smoke run of the tool)")
    args = ap.parse_args()
    import torch
    from effex_amd.plan import FxPlan
    assert torch.cuda.is_available(), "bench_flag.py measures on the GPU only"
    lines = []
    for n_ant, nchan, n_chunks in CASES:
        if args.quick:
            nchan //= 4
        n_base = n_ant * (n_ant - 1) // 2
        gen = torch.Generator(device="cuda").manual_seed(987 + n_ant)
        centre = torch.view_as_complex(2.0 * torch.randn((n_base, nchan, 2), generator=gen, device="cuda", dtype=torch.float32))
        rows = torch.empty((n_chunks, n_base, nchan), dtype=torch.complex64, device="cuda")
        for c in range(n_chunks):
            noise = torch.view_as_complex(torch.randn((n_base, nchan, 2), generator=gen, device="cuda", dtype=torch.float32))
            far = torch.rand((n_base, nchan), generator=gen, device="cuda") < 0.1
            rows[c] = centre + 0.1 * noise * torch.where(far, 30.0, 1.0)
        rows[:, :, nchan // 3] *= 40.0                      # a tone
        del noise, far
        with FxPlan(n_ant, nchan, 4, nchan * 8) as plan:
            t_lib, t_torch = [], []
            for rep in range(args.warmup + args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                w = plan.flag_rows(rows)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                w_torch = torch_flag(torch, rows)
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                if rep >= args.warmup:
                    t_lib.append((t1 - t0) * 1e3)
                    t_torch.append((t2 - t1) * 1e3)
            equal = bool(torch.equal(w, w_torch))
            flagged = float((w == 0).float().mean())
        samples = n_chunks * n_base * nchan
        moved = samples * 12
        line = {"kind": "flag_rows", "device": torch.cuda.get_device_name(0), "n_ant": n_ant, "nchan": nchan, "n_chunks": n_chunks,
                "reps": args.reps, "bytes_moved": moved, "flag_rows_ms": round(median(t_lib), 4),
                "flag_rows_call_gbps": round(moved / median(t_lib) / 1e6, 1), "torch_ms": round(median(t_torch), 4),
                "torch_over_flag_rows": round(median(t_torch) / median(t_lib), 3), "torch_equal": equal, "flagged_share": round(flagged, 5),
                "flag_rows_ms_all": [round(v, 4) for v in t_lib], "torch_ms_all": [round(v, 4) for v in t_torch]}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del rows, w, w_torch
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
