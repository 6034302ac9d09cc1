#!/usr/bin/env python
"""Two builds of libfxcorr against each other, for a change that must leave results and host cost alone.

    FXCORR_LIB=<build> python tools/compare_builds.py dump OUT.npz     one small shape per route and row modifier -> every output
    python tools/compare_builds.py compare A.npz B.npz                  the two dumps bit for bit (exit status 1 if any differs)
    FXCORR_LIB=<build> python tools/compare_builds.py loop [--calls N]  wall time of N back-to-back fx_rows calls of one chunk on a
                                                                        small plan (device memory, no synchronisation inside):
                                                                        the per-call host path; one JSON line

`dump` takes its inputs from seeded generators, so two processes on two builds see the same samples.  A library under
<dir>/libfxcorr.so finds its pre-built per-channel-count kernels under <dir>/rtc_prebuilt/.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BW, FC = 2.4e6, 1.4204e9

# name, n_ant, nchan, ntaps, num_samp, n_chunks, expected plan.path
ROUTES = [
    ("fused 2x4096", 2, 4096, 4, 4096 * 16, 3, "fused"),
    ("tiled 2x1024", 2, 1024, 4, 1024 * 32, 5, "tiled"),
    ("prefilter 2x512x8", 2, 512, 8, 512 * 64 + 3, 5, "tiled"),
    ("small 2x64", 2, 64, 4, 64 * 200, 7, "tiled"),
    ("stream 2x1", 2, 1, 4, 20000, 6, "stream"),
    ("per-channel-count 2x1000", 2, 1000, 4, 1000 * 33 + 7, 4, "generic"),
    ("two-pass 2x5000", 2, 5000, 4, 5000 * 12 + 1, 3, "generic"),
    ("8 antennas x4096", 8, 4096, 4, 4096 * 16, 3, "fused"),
    ("12 antennas x1024", 12, 1024, 4, 1024 * 20, 3, None),
]


def samples(seed, n_chunks, n_ant, num_samp):
    rng = np.random.default_rng(seed)
    shape = (n_chunks, n_ant, num_samp)
    return (rng.standard_normal(shape, dtype=np.float32) + 1j * rng.standard_normal(shape, dtype=np.float32)).astype(np.complex64)


def dump(path):
    import torch
    from effex_amd import _lib
    from effex_amd.plan import FxPlan, FxPipeline
    out, routes = {}, {}

    def keep(name, v):
        v = v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)
        assert np.isfinite(v).all() and np.abs(v).max() > 0, name
        out[name] = v

    for k, (name, n_ant, nchan, ntaps, num_samp, n_chunks, want_path) in enumerate(ROUTES):
        x = samples(100 + k, n_chunks, n_ant, num_samp)
        xd = torch.from_numpy(x).cuda()
        with FxPlan(n_ant, nchan, ntaps, num_samp, device=0) as p:
            assert want_path is None or p.path == want_path, (name, p.path)
            keep(name + ": rows", p.fx_rows(xd, "SPECTRUM"))
            keep(name + ": continuum rows", p.fx_rows(xd, "CONTINUUM", bandwidth=BW))
            p.fx_accumulate(xd)
            keep(name + ": integration", p.finalize("SPECTRUM"))
            keep(name + ": host rows", p.fx_rows(x, "SPECTRUM"))
            info = p.info
            routes[name] = [p.path, info["specialised"], info["spec_source"], info["grid"], info["block"], info["lds_bytes"], info["workspace_bytes"]]
    # the row modifiers, on a 3-antenna plan (per-antenna tables) and on the headline shape
    for name, n_ant, nchan, num_samp in (("3x256", 3, 256, 256 * 300), ("2x4096", 2, 4096, 4096 * 16)):
        n_chunks = 6
        x = samples(200 + n_ant, n_chunks, n_ant, num_samp)
        xd = torch.from_numpy(x).cuda()
        rng = np.random.default_rng(300 + n_ant)
        u8 = torch.from_numpy(rng.integers(0, 256, (n_chunks, n_ant, num_samp, 2), dtype=np.uint8)).cuda()
        delays = [0.0, 3.2e-6, -1.7e-6][:n_ant]
        rates = [0.0, 2e-9, -1e-9][:n_ant]
        gains = (1.0 + 0.1 * rng.standard_normal((3, n_ant, nchan))) * np.exp(2j * np.pi * rng.random((3, n_ant, nchan)))
        with FxPlan(n_ant, nchan, 4, num_samp, device=0) as p:
            for aligned in (False, True):
                tag = "%s %s track" % (name, "aligned" if aligned else "delay")
                p.set_delay_track(delays, rates, BW, FC, whole_samples=aligned)
                keep(tag + ": rows", p.fx_rows(xd, "SPECTRUM"))
                p.fx_accumulate(xd)
                keep(tag + ": tracked integration", p.finalize("SPECTRUM"))
                keep(tag + ": tables", p.track_tables(4))
                p.set_track_gains(gains, interval=2)
                keep(tag + " + gain track: rows", p.fx_rows(xd, "SPECTRUM"))
                p.fx_accumulate_u8(u8, remove_dc=True)
                keep(tag + " + gain track: bytes integrated, continuum", p.finalize("CONTINUUM", bandwidth=BW))
            p.set_rot(np.exp(2j * np.pi * rng.random(nchan)))
            if n_ant > 2:
                p.set_rot_ant(np.exp(2j * np.pi * rng.random((n_ant, nchan))))
                keep(name + " per-antenna rot: rows", p.fx_rows(xd, "SPECTRUM"))
            p.set_sample_delays([0, 5, -3][:n_ant])
            keep(name + " sample delays: rows", p.fx_rows(xd, "SPECTRUM"))
            p.set_sample_delays([0] * n_ant)
            p.set_autos(True)
            keep(name + " autos: rows", p.fx_rows(xd, "SPECTRUM"))
            p.fx_accumulate(xd)
            keep(name + " autos: integration", p.finalize("SPECTRUM"))
            p.set_autos(False)
            with FxPipeline(p, 2, depth=2) as pipe:
                pipe.push(x[0:2])
                pipe.push(x[2:4])
                keep(name + " pipe: batch 0", pipe.pop())
                pipe.push(x[4:6])
                keep(name + " pipe: batch 1", pipe.pop())
                keep(name + " pipe: batch 2", pipe.pop())
    np.savez(path, **out)
    with open(os.path.splitext(path)[0] + ".routes.json", "w") as fh:
        json.dump(routes, fh, indent=1)
    print("%d arrays from %s -> %s" % (len(out), _lib.LIB_PATH, path))


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    ra, rb = (json.load(open(os.path.splitext(p)[0] + ".routes.json")) for p in (a_path, b_path))
    bad = sorted(set(a.files) ^ set(b.files))
    for name in sorted(set(a.files) & set(b.files)):
        same = a[name].dtype == b[name].dtype and a[name].shape == b[name].shape and a[name].tobytes() == b[name].tobytes()
        print("%-70s %-18s %s" % (name, "x".join(map(str, a[name].shape)), "identical" if same else "DIFFERS"))
        if not same:
            bad.append(name)
    for name in sorted(ra):
        print("route %-40s %s %s" % (name, ra[name], "same" if ra[name] == rb.get(name) else "DIFFERS: %s" % rb.get(name)))
        if ra[name] != rb.get(name):
            bad.append("route " + name)
    print("%d arrays compared, %d differ" % (len(a.files), len(bad)))
    return 1 if bad else 0


def loop(calls):
    import torch
    from effex_amd import _lib
    from effex_amd.plan import FxPlan
    n_ant, nchan, num_samp = 2, 1024, 1024 * 32
    xd = torch.from_numpy(samples(7, 1, n_ant, num_samp)).cuda()
    out = torch.empty((1, 1, nchan), dtype=torch.complex64, device="cuda")
    with FxPlan(n_ant, nchan, 4, num_samp, device=0) as p:
        for _ in range(200):
            p.fx_rows(xd, "SPECTRUM", out=out)
        torch.cuda.synchronize()
        walls = []
        for _ in range(5):
            t0 = time.perf_counter()
            for _ in range(calls):
                p.fx_rows(xd, "SPECTRUM", out=out)
            t1 = time.perf_counter()      # (the host's time to issue the calls: nothing inside the loop waits for the device)
            torch.cuda.synchronize()
            walls.append((t1 - t0) * 1e3)
    print(json.dumps({"tool": "compare_builds loop", "lib": _lib.LIB_PATH, "calls": calls, "wall_ms_median": round(float(np.median(walls)), 3),
                      "us_per_call": round(float(np.median(walls)) / calls * 1e3, 3), "wall_ms_all": [round(w, 3) for w in walls]}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("dump", "compare", "loop"))
    ap.add_argument("paths", nargs="*")
    ap.add_argument("--calls", type=int, default=2000)
    args = ap.parse_args()
    if args.what == "dump":
        dump(args.paths[0])
    elif args.what == "compare":
        sys.exit(compare(args.paths[0], args.paths[1]))
    else:
        loop(args.calls)
