#!/usr/bin/env python3
"""Developer aid: what the spectral kurtosis pass (include/fxcorr.h fxc_kurtosis, k_kurtosis.h) costs beside the 1-beam pass of the
beamformer over the same resident spectra, and beside the same statistic in torch.  8 antennas x 4096 channels x 4 taps, num_samp
262144 (64 frames a chunk), 64 chunks: 1 GiB of spectra.  One plan, after a warm-up, medians of `reps`, the three alternated in
one process.

The library's own events (fxc_kernel_profiling / fxc_kernel_time) go round the F stage and round the pass that reads the
spectra; a pass's time is its call's kernel time minus the F stage's, taken from the channelize call of the same rep:
  f_ms            the F stage alone
  sk_pass_ms      kurtosis_kernel over the pass's spectra (tint 0 and tint 8, sk and power written)
  beam_pass_ms    the yardstick: beam_kernel<1, POWER>, one beam
  torch_ms        channelize, abs() ** 2, two means and the formula in torch, minus the F stage: torch_minus_f_ms

    python tools/bench_kurtosis.py [--reps 7] [--out profiles/kurtosis/times.json] [--quick]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_ANT, NCHAN, NTAPS, NUM_SAMP, N_CHUNKS = 8, 4096, 4, 262144, 64
TINTS = (0, 8)


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="8 chunks (a smoke run of the tool)")
    ap.add_argument("--no-torch", action="store_true", help="the library alone (for a profiler run)")
    args = ap.parse_args()
    import torch
    import numpy as np
    from effex_amd.plan import FxPlan, synth_fill
    assert torch.cuda.is_available(), "bench_kurtosis.py measures on the GPU only"
    n_chunks = 8 if args.quick else N_CHUNKS
    n_pts = NUM_SAMP // NCHAN
    x = torch.empty((n_chunks, N_ANT, NUM_SAMP), dtype=torch.complex64, device="cuda")
    synth_fill(x, 2024, delays=np.arange(N_ANT) % 5)
    gen = torch.Generator(device="cuda").manual_seed(7)
    w = torch.view_as_complex(torch.randn((1, N_ANT, NCHAN, 2), generator=gen, device="cuda") / 2.0 ** 0.5)
    beam = torch.empty((n_chunks, 1, 1, NCHAN), dtype=torch.float32, device="cuda")
    t = {"f": [], "beam_pass": [], "torch": [], "torch_minus_f": []}
    diff = None
    with FxPlan(N_ANT, NCHAN, NTAPS, NUM_SAMP) as plan:
        plan.kernel_profiling(True)
        outs = {tint: (torch.empty((n_chunks, N_ANT, -(-n_pts // (tint or n_pts)), NCHAN), dtype=torch.float32, device="cuda"),
                       torch.empty((n_chunks, N_ANT, -(-n_pts // (tint or n_pts)), NCHAN), dtype=torch.float32, device="cuda"))
                for tint in TINTS}
        for rep in range(args.warmup + args.reps):
            keep = rep >= args.warmup
            plan.kernel_time()
            spec = plan.channelize(x.view(-1, NUM_SAMP))
            torch.cuda.synchronize()
            f_ms = plan.kernel_time()[0]
            del spec
            plan.beamform(x, w, out=beam)
            torch.cuda.synchronize()
            beam_ms = plan.kernel_time()[0] - f_ms
            sk_ms = {}
            for tint in TINTS:
                plan.kurtosis(x, tint=tint, return_power=True, out=outs[tint])
                torch.cuda.synchronize()
                sk_ms[tint] = plan.kernel_time()[0] - f_ms
            torch_ms = None
            if not args.no_torch:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                p = plan.channelize(x.view(-1, NUM_SAMP)).view(n_chunks, N_ANT, n_pts, NCHAN).abs() ** 2
                s1, s2 = p.mean(dim=2), (p * p).mean(dim=2)
                sk_t = torch.fft.fftshift((n_pts + 1.0) / (n_pts - 1.0) * (s2 / (s1 * s1) - 1.0), dim=-1)
                e1.record()
                torch.cuda.synchronize()
                torch_ms = e0.elapsed_time(e1)
                plan.kernel_time()
                diff = float((sk_t - outs[0][0][:, :, 0]).abs().max())
                del p, s1, s2, sk_t
            if keep:
                t["f"].append(f_ms)
                t["beam_pass"].append(beam_ms)
                for tint in TINTS:
                    t.setdefault("sk_pass_tint%d" % tint, []).append(sk_ms[tint])
                if torch_ms is not None:
                    t["torch"].append(torch_ms)
                    t["torch_minus_f"].append(torch_ms - f_ms)
    spectra_bytes = n_chunks * N_ANT * n_pts * NCHAN * 8
    line = {"kind": "kurtosis", "device": torch.cuda.get_device_name(0), "n_ant": N_ANT, "nchan": NCHAN, "ntaps": NTAPS,
            "num_samp": NUM_SAMP, "n_chunks": n_chunks, "reps": args.reps, "spectra_bytes": spectra_bytes,
            "clock": "the library's events round the F stage and round the pass; pass = call - F stage of the same rep"}
    for key, v in t.items():
        if v:
            line[key + "_ms"] = round(median(v), 4)
            line[key + "_ms_all"] = [round(q, 4) for q in v]
    for tint in TINTS:
        ms = line["sk_pass_tint%d_ms" % tint]
        line["sk_pass_tint%d_over_beam_pass" % tint] = round(ms / line["beam_pass_ms"], 3)
        line["sk_pass_tint%d_TBs" % tint] = round(spectra_bytes / (ms * 1e-3) / 1e12, 3)
    line["beam_pass_TBs"] = round(spectra_bytes / (line["beam_pass_ms"] * 1e-3) / 1e12, 3)
    if t["torch"]:
        line["torch_minus_f_over_sk_pass_tint0"] = round(line["torch_minus_f_ms"] / line["sk_pass_tint0_ms"], 2)
        line["torch_sk_diff_abs"] = diff
    print(json.dumps(line, indent=1, sort_keys=True), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(line, fh, indent=1, sort_keys=True)
            fh.write("\n")


if __name__ == "__main__":
    main()
