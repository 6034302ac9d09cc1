#!/usr/bin/env python3
"""Developer aid: what the single-pulse search (include/fxcorr.h fxc_boxcar_search) costs on device series, beside the same
computation in torch: per row a clipped mean and standard deviation, per width ``avg_pool1d`` with stride 1 scaled to S/N, and a
maximum per block with its width and time.  A host clock around whole calls that end in a device synchronisation, after a
warm-up, medians of `reps`, the two alternated in one process; one JSON line per case: random series of 4 x 256 x 65 536 and of
1 x 256 x 262 144 samples, widths (0, 8) and (0, 12), blocks of 64, 0 and 2 clipping rounds.  Each line carries the derived bound of
DESIGN.md §3p -- the larger of the HBM traffic (2 (R + 1) sweeps of the input, one read of every tile with its halo) and the
filter's LDS traffic (a tile's words written once and, per level, two reads and a write of every word the level keeps) -- and the
share of it the call reaches.  torch adds in another order and takes the first of equal maxima over another candidate order, so
the line says how far its S/N map is from the library's, not whether the bits agree.

    python tools/bench_boxcar.py [--reps 5] [--out profiles/boxcar/bench.jsonl] [--quick]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = [(4, 256, 65536), (1, 256, 262144)]          # n_series, n_dm, n_t
WIDTHS = ((0, 8), (0, 12))
BLOCK = 64
ROUNDS = (0, 2)
CLIP = 3.0
T = 4096                                             # kBoxT: the starts of a filter tile
HBM_BPS, LDS_B32_BPS = 6.3e12, 75e12                 # achievable HBM rate; ds_read_b32 with every CU streaming


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def torch_search(torch, ts, widths, block, clip, rounds):
    """ts [n_rows, n_t] -> (snr, width index, time) [n_rows, n_blk]"""
    n_rows, n_t = ts.shape
    x = ts.double()
    mask = torch.ones_like(x, dtype=torch.bool)
    for r in range(rounds + 1):
        n = mask.sum(dim=1, keepdim=True)
        m = (x * mask).sum(dim=1, keepdim=True) / n
        e = x - m
        v = (e * e * mask).sum(dim=1, keepdim=True) / (n - 1)
        if r < rounds:
            mask = e * e <= clip * clip * v
    y = (x - m).float()[:, None, :]
    std = v.sqrt().float()
    n_starts = n_t - (1 << widths[0]) + 1
    n_blk = -(-n_starts // block)
    best = best_j = best_t = None
    for j in range(widths[0], widths[1] + 1):
        w = 1 << j
        if w > n_t:
            break
        snr = torch.nn.functional.avg_pool1d(y, w, stride=1)[:, 0, :n_starts] * (float(w) ** 0.5) / std
        snr = torch.nn.functional.pad(snr, (0, n_blk * block - snr.shape[1]), value=float("-inf")).view(n_rows, n_blk, block)
        top, at = snr.max(dim=2)
        if best is None:
            best, best_j, best_t = top, torch.full_like(at, j), at
        else:
            better = top > best
            best = torch.where(better, top, best)
            best_j = torch.where(better, torch.full_like(at, j), best_j)
            best_t = torch.where(better, at, best_t)
    return best, best_j, best_t + torch.arange(n_blk, device=ts.device)[None, :] * block


def bound_ms(n_rows, n_t, widths, rounds):
    """-> (HBM ms, LDS ms) of DESIGN.md §3p"""
    j_hi = widths[1]
    halo = (1 << j_hi) - 1
    tiles = -(-(n_t - (1 << widths[0]) + 1) // T)
    hbm = n_rows * 4.0 * (2 * (rounds + 1) * n_t + tiles * (T + halo))
    words = (T + halo) + sum(3 * (T + halo + 1 - (1 << j)) for j in range(1, j_hi + 1)) + 4 * T      # load, levels, bests out and in
    lds = n_rows * tiles * 4.0 * words
    return hbm / HBM_BPS * 1e3, lds / LDS_B32_BPS * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="a sixteenth of the times (a smoke run of the tool)")
    args = ap.parse_args()
    import torch
    from effex_amd.plan import FxPlan
    assert torch.cuda.is_available(), "bench_boxcar.py measures on the GPU only"
    lines = []
    with FxPlan(2, 64, 4, 64 * 8) as plan:
        for n_series, n_dm, n_t in CASES:
            if args.quick:
                n_t //= 16
            gen = torch.Generator(device="cuda").manual_seed(2024 + n_t)
            ts = torch.randn((n_series, n_dm, n_t), generator=gen, device="cuda", dtype=torch.float32) * 2.0 + 64.0
            ts[:, :, n_t // 3:n_t // 3 + 8] += 6.0                  # a pulse of 8 samples in every row: the clipping has something to do
            rows = ts.view(n_series * n_dm, n_t)
            for widths in WIDTHS:
                for rounds in ROUNDS:
                    t_lib, t_torch = [], []
                    for rep in range(args.warmup + args.reps):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        got = plan.boxcar_search(ts, widths, BLOCK, CLIP, rounds)
                        torch.cuda.synchronize()
                        t1 = time.perf_counter()
                        want = torch_search(torch, rows, widths, BLOCK, CLIP, rounds)
                        torch.cuda.synchronize()
                        t2 = time.perf_counter()
                        if rep >= args.warmup:
                            t_lib.append((t1 - t0) * 1e3)
                            t_torch.append((t2 - t1) * 1e3)
                    hbm_ms, lds_ms = bound_ms(n_series * n_dm, n_t, widths, rounds)
                    bound = max(hbm_ms, lds_ms)
                    snr = got[0].view(n_series * n_dm, -1)
                    line = {"kind": "boxcar_search", "device": torch.cuda.get_device_name(0), "n_series": n_series, "n_dm": n_dm, "n_t": n_t,
                            "widths": list(widths), "block": BLOCK, "clip": CLIP, "clip_iters": rounds, "reps": args.reps,
                            "input_bytes": n_series * n_dm * n_t * 4, "boxcar_ms": round(median(t_lib), 4),
                            "torch_ms": round(median(t_torch), 4), "torch_over_boxcar": round(median(t_torch) / median(t_lib), 3),
                            "bound_hbm_ms": round(hbm_ms, 4), "bound_lds_ms": round(lds_ms, 4),
                            "bound_over_boxcar": round(bound / median(t_lib), 3),
                            "torch_snr_diff": float((snr - want[0]).abs().max()),
                            "torch_width_agree": float((got[1].view(snr.shape) == want[1]).float().mean()),
                            "boxcar_ms_all": [round(v, 4) for v in t_lib], "torch_ms_all": [round(v, 4) for v in t_torch]}
                    print(json.dumps(line), flush=True)
                    lines.append(line)
                    del got, want
            del ts, rows
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
