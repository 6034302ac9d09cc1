"""Chunks of more than 1024 frames on the device, under every row modifier (tests/long_chunk_cases.py).

Such a chunk is cut into frame ranges by the X-engines (k_finish.h::x_range), one raw row per range, range-major, and the rows
kernels and the tracked fold read the ranges as their splits.  Each case names a route, asserts it from ``plan.path`` /
``plan.info``, and compares fx_rows (SPECTRUM, CONTINUUM) and fx_accumulate + finalize (SPECTRUM, CONTINUUM) with the float64
oracle, per group of rows (cross, autos): TOL_VIS / TOL_CONT of the group's largest value.  tests/test_long_chunks_host.py shows
that every wrong reading of the ranges, the chunk's tables or the auto rows misses these bounds by a factor of ten or more.
Tracked cases: the counter advances by the call's chunks, and the integration is within 1e-6 of the float64 mean of the plan's own
tracked rows (the bound of test_gpu_tracking.py).  Auto rows: imaginary part 0, real part >= 0.  The passes cases run in a child
process with a workspace target of 1 MiB (FXC_WS_MB is read once per process), as test_gpu_route_passes.py does."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import long_chunk_cases as lc
from tolerances import TOL_CONT, TOL_VIS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IN_PROCESS = [c for c in lc.CASES if not c.env]
IN_CHILD = [c for c in lc.CASES if c.env]


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def plan_mod(torch):
    from effex_amd import plan
    return plan


def r256(b):
    return (int(b) + 255) // 256 * 256


def check(case, out):
    """every comparison of a case's device outputs (long_chunk_cases.device_outputs) with the oracle"""
    seen = json.loads(str(out["route"][0]))
    print("%s: %s" % (case.id, {k: seen[k] for k in ("path", "block", "lds_bytes", "specialised", "workspace_bytes")}))
    assert {k: seen[k] for k in case.expect} == case.expect, (case.id, seen)
    # the frame ranges: the workspace the first fx_rows took holds a pass's spectra and one raw row per product and range
    cb, spec, raw = lc.passes(case, int(case.env["FXC_WS_MB"]) << 20) if case.env else lc.passes(case)
    assert int(out["info"][0]) == r256(spec) + r256(raw), (case.id, int(out["info"][0]), cb, lc.n_ranges(case))
    ref = lc.oracle(case)
    n, nb = case.n_chunks, len(lc.pairs(case.n_ant))
    rows, rows_c, integ, integ_c = out["rows"], out["rows_c"], out["integ"], out["integ_c"]
    assert rows.shape == ref.shape and rows.dtype == np.complex64
    assert rows_c.shape == ref.shape[:2] and integ.shape == ref.shape[1:] and integ_c.shape == ref.shape[1:2]
    ref_i = ref.mean(axis=0)
    errs = {}
    for name, g in lc.groups(case):
        errs[name, "rows SPECTRUM"] = lc.rel_err(rows[:, g], ref[:, g])
        errs[name, "rows CONTINUUM"] = lc.rel_err(rows_c[:, g], lc.continuum(ref[:, g]))
        errs[name, "integration SPECTRUM"] = lc.rel_err(integ[g], ref_i[g])
        errs[name, "integration CONTINUUM"] = lc.rel_err(integ_c[g], lc.continuum(ref_i[g]))
    own = lc.rel_err(integ, rows.astype(np.complex128).mean(axis=0))
    print("%s: %s; integration against the mean of the plan's rows: %.3g"
          % (case.id, ", ".join("%s %s %.3g" % (k + (v,)) for k, v in errs.items()), own))
    for (name, what), err in errs.items():
        assert err < (TOL_CONT if what.endswith("CONTINUUM") else TOL_VIS), (case.id, name, what, err)
    if lc.tracked(case):
        assert out["track"].tolist() == [lc.T0 + n] * 3, out["track"]
        assert own < 1e-6, (case.id, own)
    else:
        assert out["track"].size == 0
    if case.autos:
        for what, v in (("rows", rows[:, nb:]), ("integration", integ[nb:])):
            assert (v.imag == 0).all() and (v.real >= 0).all(), (case.id, what)


@pytest.mark.parametrize("case", IN_PROCESS, ids=lambda c: c.id)
def test_long_chunks_match_the_oracle(plan_mod, torch, case):
    xd = torch.from_numpy(lc.samples(case).copy()).cuda()
    check(case, lc.device_outputs(plan_mod, xd, case))


CHILD = r'''
import sys
import numpy as np, torch
for p in sys.argv[1:4]:
    sys.path.insert(0, p)
import long_chunk_cases as lc
from effex_amd import plan as plan_mod
case = lc.BY_ID[sys.argv[4]]
np.savez(sys.argv[5], **lc.device_outputs(plan_mod, torch.from_numpy(lc.samples(case).copy()).cuda(), case))
'''


@pytest.mark.parametrize("case", IN_CHILD, ids=lambda c: c.id)
def test_long_chunks_in_several_passes_match_the_oracle(torch, case):
    """5 chunks of 1027 frames in passes of 2, 2 and 1 chunks: every pass writes its own range-major rows, and the last, shorter
    pass has another split stride"""
    with tempfile.TemporaryDirectory() as tmp:
        res = os.path.join(tmp, "r.npz")
        proc = subprocess.run([sys.executable, "-c", CHILD, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), ROOT, case.id, res],
                              env=dict(os.environ, **case.env), capture_output=True, text=True, timeout=300)
        assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-2000:]
        out = dict(np.load(res))
    check(case, out)
    # the passes: the chunk arithmetic of h_run.h::autos_pass, which the workspace the first fx_rows took confirms
    cb, spec, raw = lc.passes(case, 1 << 20)
    ws, cu = (int(v) for v in out["info"])
    print("workspace %d bytes, %d CUs, %d chunks a pass" % (ws, cu, cb))
    assert ws == r256(spec) + r256(raw) and cb == 2, (ws, cb)
    assert [min(cb, case.n_chunks - c0) for c0 in range(0, case.n_chunks, cb)] == [2, 2, 1]


def test_long_tracked_rows_do_not_depend_on_batching(plan_mod, torch):
    """3 antennas, chunks of two frame ranges, under a track: one call, one call per chunk and a split at chunk 1 give the same
    bits, rows and exported sums alike (the BATCHING cases of test_gpu_tracking.py have no long chunk with more than two antennas)"""
    case = lc.BY_ID["wave-3x64x1027-track"]
    n = case.n_chunks
    x = torch.from_numpy(lc.samples(case).copy()).cuda()
    with plan_mod.FxPlan(case.n_ant, case.nchan, lc.NTAPS, lc.num_samp(case), window=lc.window(case)) as plan:
        lc.apply_modifier(plan, case)

        def rows_of(pieces):
            plan.track_seek(lc.T0)
            got = np.concatenate([lc.host(plan.fx_rows(x[lo:hi], "SPECTRUM")) for lo, hi in pieces])
            assert plan.track_chunk == lc.T0 + n
            return got

        def sums_of(pieces):
            plan.track_seek(lc.T0)
            for lo, hi in pieces:
                plan.fx_accumulate(x[lo:hi])
            assert plan.track_chunk == lc.T0 + n
            return lc.exported(plan)

        whole, each, split = [(0, n)], [(c, c + 1) for c in range(n)], [(0, 1), (1, n)]
        rows, sums = rows_of(whole), sums_of(whole)
        assert np.abs(rows).min() > 0 and not np.array_equal(rows[0], rows[1])
        assert lc.rel_err(rows, lc.oracle(case)) < TOL_VIS
        for name, pieces in (("one call per chunk", each), ("a split at chunk 1", split)):
            got_rows, got_sums = rows_of(pieces), sums_of(pieces)
            print("%s against one call: rows %.3g, sums %.3g" % (name, lc.rel_err(got_rows, rows), lc.rel_err(got_sums, sums)))
            assert np.array_equal(got_rows, rows), name
            assert np.array_equal(got_sums, sums), name
