#!/usr/bin/env python3
"""Developer aid: what the beam pass of the beamformer (include/fxcorr.h fxc_beamform, k_beam.h) costs beside the X-engine pass of the
same plan over the same chunks, and beside the same computation in torch.  8 antennas x 4096 channels x 4 taps, num_samp 262144
(64 frames a chunk), 64 resident chunks, power mode, tint 0; 1, 4, 8 and 16 beams.  One plan with autos, after a warm-up, medians
of `reps`, everything alternated in one process; one JSON line per beam count.

What the library's own clocks give (fxc_kernel_profiling / fxc_kernel_time put events round the F stage and round the beam pass;
fxc_timer_* round a whole call):
  f_ms            the F stage alone (a channelize call's kernel time)
  beam_pass_ms    a beamform call's kernel time minus the F stage's inside it, taken from the channelize call of the same rep
  x_pass_ms       the yardstick: an fx_rows call (events round the call) minus the F stage inside it (its kernel time).  What is left
                  is xengine_kernel<8, true> AND the rows kernel that finishes its 36 raw rows a chunk (75 MB read and written
                  beside the 1 GiB of spectra): the yardstick is that much too long, so the ratio that much too kind.
The kernels' own durations come from a profiler run of this tool and are merged into the lines:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/bench_beamform.py --reps 3 --no-torch
    python tools/bench_beamform.py --merge lines.jsonl --kernel-stats DIR/.../t_kernel_stats.csv --out profiles/beamform/times.json
With 4 beams the beam pass reads the bytes of the X-engine pass and issues its 128 fused multiply-adds per channel and frame (4 x 8
complex multiply-adds against 28 cross products and 8 autos); the expectation is beam pass <= 1.15 x X-engine pass.

    python tools/bench_beamform.py [--reps 10] [--out profiles/beamform/times.json] [--quick]

Masks and incoherent beams (fxc_beamform_ex; mask_main below): the masked and the incoherent passes beside the
unmasked beam_kernel pass of the same run, 1, 4 and 8 beams:
    python tools/bench_beamform.py --mask-tint 8 --mask-tint 64 [--mode INCOHERENT] [--reps 7] --out profiles/beam_mask/times.json
"""
import argparse
import csv
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_ANT, NCHAN, NTAPS, NUM_SAMP, N_CHUNKS = 8, 4096, 4, 262144, 64
BEAMS = (1, 4, 8, 16)
KERNELS = ("beam_kernel", "xengine_kernel", "rows_spectrum_kernel", "beam_weights_kernel")


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def kernel_stats(path):
    """{kernel name: [calls, average us, min us, max us]} of the beam, X-engine and rows kernels from a rocprofv3 --stats csv"""
    out = {}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            if any(k in row["Name"] for k in KERNELS):
                out[row["Name"]] = [int(row["Calls"]), round(float(row["AverageNs"]) / 1e3, 2), round(float(row["MinNs"]) / 1e3, 2),
                                    round(float(row["MaxNs"]) / 1e3, 2)]
    return out


def merge(args):
    lines = json.load(open(args.merge))["lines"] if args.merge.endswith(".json") else [json.loads(ln) for ln in open(args.merge) if ln.strip()]
    stats = {}
    for path in args.kernel_stats:
        stats.update(kernel_stats(path))
    rec = {"lines": lines, "kernel_stats_us": stats, "kernel_stats_columns": ["calls", "average", "min", "max"]}
    x = [v[1] for k, v in stats.items() if "xengine_kernel" in k]
    if x:
        rec["xengine_kernel_us"] = x[0]
        for k, v in stats.items():
            if "beam_kernel" in k:
                rec.setdefault("beam_kernel_over_xengine_kernel", {})[k] = round(v[1] / x[0], 3)
    write(args.out, rec)


def write(path, rec):
    print(json.dumps(rec, indent=1, sort_keys=True))
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            json.dump(rec, fh, indent=1, sort_keys=True)
            fh.write("\n")


def mask_main(args):
    """--mask-tint / --mode INCOHERENT (fxc_beamform_ex): in one run, per beam count (1, 4, 8) and mask_tint, the
    beam pass -- a call's kernel time minus the F stage's of the same rep -- of beam_kernel (no mask), of the masked kernel and of the
    incoherent kernel with and without the mask, tint 0, and each one's ratio to the unmasked pass of the same run.  The derived
    traffic ratio of a masked pass is 1 + 1 / (2 mask_tint) (4 mask bytes per mask_tint frames beside 8 sample bytes a frame); what
    exceeds it is instruction issue.  No time is a pass / fail condition."""
    import torch
    import numpy as np
    from effex_amd.plan import FxPlan, synth_fill
    assert torch.cuda.is_available(), "bench_beamform.py measures on the GPU only"
    n_chunks = 8 if args.quick else N_CHUNKS
    n_pts = NUM_SAMP // NCHAN
    mask_tints = args.mask_tint or [8, 64]
    x = torch.empty((n_chunks, N_ANT, NUM_SAMP), dtype=torch.complex64, device="cuda")
    synth_fill(x, 2024, delays=np.arange(N_ANT) % 5)
    gen = torch.Generator(device="cuda").manual_seed(7)
    lines = []
    with FxPlan(N_ANT, NCHAN, NTAPS, NUM_SAMP) as plan:
        plan.kernel_profiling(True)
        for n_beam in (1, 4, 8):
            w = torch.view_as_complex(torch.randn((n_beam, N_ANT, NCHAN, 2), generator=gen, device="cuda") / 2.0 ** 0.5)
            out = torch.empty((n_chunks, n_beam, 1, NCHAN), dtype=torch.float32, device="cuda")
            for mt in mask_tints:
                n_mbin = -(-n_pts // mt)
                mask = (torch.rand((n_chunks, N_ANT, n_mbin, NCHAN), generator=gen, device="cuda") >= 0.3).to(torch.float32)
                runs = {"unmasked": lambda: plan.beamform(x, w, out=out),
                        "masked": lambda: plan.beamform(x, w, out=out, mask=mask, mask_tint=mt),
                        "incoherent": lambda: plan.beamform_incoherent(x, w, out=out),
                        "incoherent_masked": lambda: plan.beamform_incoherent(x, w, out=out, mask=mask, mask_tint=mt)}
                if args.mode == "INCOHERENT":
                    runs = {k: v for k, v in runs.items() if k != "masked"}
                t = {k: [] for k in runs}
                t["f"] = []
                for rep in range(args.warmup + args.reps):
                    plan.kernel_time()
                    spec = plan.channelize(x.view(-1, NUM_SAMP))
                    torch.cuda.synchronize()
                    f_ms = plan.kernel_time()[0]
                    del spec
                    got = {}
                    for name, fn in runs.items():
                        fn()
                        torch.cuda.synchronize()
                        got[name] = plan.kernel_time()[0] - f_ms
                    if rep >= args.warmup:
                        t["f"].append(f_ms)
                        for name, v in got.items():
                            t[name].append(v)
                spectra_bytes = n_chunks * N_ANT * n_pts * NCHAN * 8
                line = {"kind": "beam_mask", "device": torch.cuda.get_device_name(0), "n_ant": N_ANT, "nchan": NCHAN, "ntaps": NTAPS,
                        "num_samp": NUM_SAMP, "n_chunks": n_chunks, "n_beam": n_beam, "tint": 0, "mask_tint": mt, "reps": args.reps,
                        "spectra_bytes": spectra_bytes, "mask_bytes": int(mask.numel()) * 4,
                        "derived_traffic_ratio": round(1.0 + 1.0 / (2.0 * mt), 4)}
                for key, v in t.items():
                    line[key + "_pass_ms" if key != "f" else "f_ms"] = round(median(v), 4)
                    line[(key + "_pass_ms" if key != "f" else "f_ms") + "_all"] = [round(q, 4) for q in v]
                for key in runs:
                    if key != "unmasked":
                        line[key + "_over_unmasked"] = round(line[key + "_pass_ms"] / line["unmasked_pass_ms"], 3)
                    line[key + "_TBs"] = round(spectra_bytes / (line[key + "_pass_ms"] * 1e-3) / 1e12, 3)
                print(json.dumps(line), flush=True)
                lines.append(line)
                del mask
            del w, out
    if args.out:
        write(args.out, {"lines": lines})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mask-tint", type=int, action="append", default=[], metavar="N",
                    help="time the masked and incoherent passes at N frames a mask bin beside the unmasked pass (repeatable; with "
                         "--mode INCOHERENT alone: 8 and 64); --out profiles/beam_mask/times.json")
    ap.add_argument("--mode", default="POWER", choices=["POWER", "INCOHERENT"], help="INCOHERENT: the incoherent passes (and the unmasked one) only")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="8 chunks (a smoke run of the tool)")
    ap.add_argument("--no-torch", action="store_true", help="the library alone (for a profiler run)")
    ap.add_argument("--merge", default=None, help="lines of an earlier run to add --kernel-stats to (no GPU)")
    ap.add_argument("--kernel-stats", action="append", default=[], help="rocprofv3 --stats csv of a --no-torch run")
    args = ap.parse_args()
    if args.merge:
        return merge(args)
    if args.mask_tint or args.mode == "INCOHERENT":
        return mask_main(args)
    import torch
    import numpy as np
    from effex_amd.plan import FxPlan, synth_fill
    assert torch.cuda.is_available(), "bench_beamform.py measures on the GPU only"
    n_chunks = 8 if args.quick else N_CHUNKS
    n_pts = NUM_SAMP // NCHAN
    x = torch.empty((n_chunks, N_ANT, NUM_SAMP), dtype=torch.complex64, device="cuda")
    synth_fill(x, 2024, delays=np.arange(N_ANT) % 5)
    gen = torch.Generator(device="cuda").manual_seed(7)
    lines = []
    with FxPlan(N_ANT, NCHAN, NTAPS, NUM_SAMP, autos=True) as plan:
        plan.kernel_profiling(True)
        rows = torch.empty((n_chunks, plan.n_rows, NCHAN), dtype=torch.complex64, device="cuda")
        for n_beam in BEAMS:
            w = torch.view_as_complex(torch.randn((n_beam, N_ANT, NCHAN, 2), generator=gen, device="cuda") / 2.0 ** 0.5)
            out = torch.empty((n_chunks, n_beam, 1, NCHAN), dtype=torch.float32, device="cuda")
            t = {"f": [], "f_in_rows": [], "rows_call": [], "x_pass": [], "beam_kernels": [], "beam_pass": [], "beam_call": [], "torch": [],
                 "torch_minus_f": []}
            for rep in range(args.warmup + args.reps):
                plan.kernel_time()
                spec = plan.channelize(x.view(-1, NUM_SAMP))
                torch.cuda.synchronize()
                f_ms = plan.kernel_time()[0]
                del spec
                plan.timer_start()
                plan.fx_rows(x, out=rows)
                rows_ms = plan.timer_stop()
                f_rows = plan.kernel_time()[0]
                plan.timer_start()
                plan.beamform(x, w, out=out)
                beam_call = plan.timer_stop()
                both = plan.kernel_time()[0]
                torch_ms = None
                if not args.no_torch:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    spec = plan.channelize(x.view(-1, NUM_SAMP)).view(n_chunks, N_ANT, n_pts, NCHAN)
                    y = torch.einsum("bak,caik->cbik", w, spec)
                    p_t = torch.fft.fftshift((y.abs() ** 2).mean(dim=2), dim=-1)
                    e1.record()
                    torch.cuda.synchronize()
                    torch_ms = e0.elapsed_time(e1)
                    plan.kernel_time()
                    diff = float((p_t - out[:, :, 0]).abs().max() / p_t.abs().max())
                    del spec, y, p_t
                if rep >= args.warmup:
                    for key, v in (("f", f_ms), ("f_in_rows", f_rows), ("rows_call", rows_ms), ("x_pass", rows_ms - f_rows),
                                   ("beam_kernels", both), ("beam_pass", both - f_ms), ("beam_call", beam_call)):
                        t[key].append(v)
                    if torch_ms is not None:
                        t["torch"].append(torch_ms)
                        t["torch_minus_f"].append(torch_ms - f_ms)
            spectra_bytes = n_chunks * N_ANT * n_pts * NCHAN * 8
            line = {"kind": "beamform", "device": torch.cuda.get_device_name(0), "n_ant": N_ANT, "nchan": NCHAN, "ntaps": NTAPS,
                    "num_samp": NUM_SAMP, "n_chunks": n_chunks, "n_beam": n_beam, "mode": "POWER", "tint": 0, "reps": args.reps,
                    "spectra_bytes": spectra_bytes, "spectra_reads": (n_beam + 7) // 8}
            for key, v in t.items():
                if v:
                    line[key + "_ms"] = round(median(v), 4)
                    line[key + "_ms_all"] = [round(q, 4) for q in v]
            line["beam_pass_over_x_pass"] = round(line["beam_pass_ms"] / line["x_pass_ms"], 3)
            line["beam_pass_TBs"] = round(spectra_bytes * line["spectra_reads"] / (line["beam_pass_ms"] * 1e-3) / 1e12, 3)
            if t["torch"]:
                line["torch_minus_f_over_beam_pass"] = round(line["torch_minus_f_ms"] / line["beam_pass_ms"], 2)
                line["torch_diff_rel"] = diff
            print(json.dumps(line), flush=True)
            lines.append(line)
            del w, out
    if args.out:
        if args.out.endswith(".jsonl"):
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                for line in lines:
                    fh.write(json.dumps(line) + "\n")
        else:
            write(args.out, {"lines": lines})


if __name__ == "__main__":
    main()
