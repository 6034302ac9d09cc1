"""Integrations whose X-engine workgroups sum several chunks into a raw row (tests/chunk_group_cases.py), on the device.

Every case takes its chunk count from the device's CU count so that the second of its two fx_accumulate calls has chunk groups
of three chunks at least and a shorter last group, whatever the kernel's occupancy is (tests/test_chunk_groups_host.py proves
that from the model).  The integration over both calls is compared with the float64 oracle (fx_oracle.fx_integrate; its
arithmetic on a subset of the baselines from 49 antennas on, and with the autos beside) baseline by baseline, each against its
own largest value, through TOL_VIS, and with the float64 mean of the plan's own fx_rows -- one chunk per raw row always -- at
2e-6.  Auto rows: imaginary part 0, real part >= 0.  The workspace the long call took shows its passes.  The passes cases and the
developer library's xengine_block_kernel run in a child process (FXC_WS_MB and FXC_XENGINE are read once per process), as
test_gpu_route_passes.py does."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import chunk_group_cases as cg
from tolerances import TOL_VIS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IN_PROCESS = [c for c in cg.CASES if not c.passes and c.kernel != "block"]
PASSES = [c for c in cg.CASES if c.passes]
BLOCK = [c for c in cg.CASES if c.kernel == "block"]
OWN_ROWS = 2e-6      # an integration against the float64 mean of the plan's own rows: the bound of test_gpu_parity.py


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def plan_mod(torch):
    from effex_amd import plan
    return plan


@pytest.fixture(scope="module")
def cu_count(plan_mod):
    with plan_mod.FxPlan(2, 64, 4, 64 * 8) as p:
        return int(p.info["cu_count"])


def check(case, cu, out, cb=None):
    """every comparison of a case's device outputs (chunk_group_cases.device_outputs) with the oracle; cb: chunks per pass"""
    n_long = cg.call_chunks(case, cu)
    integ, rows_mean = out["integ"], out["rows_mean"]
    ws, cu_seen = (int(v) for v in out["info"])
    nb = case.n_ant * (case.n_ant - 1) // 2
    assert str(out["path"][0]) == case.path and cu_seen == cu, (case.id, out["path"], cu_seen)
    assert integ.shape == rows_mean.shape == (cg.n_prod(case), case.nchan) and np.isfinite(integ).all()
    # the long call's passes: the workspace holds a pass's spectra, its raw rows and the fold's partial sums
    assert ws == cg.workspace_bytes(case, n_long if cb is None else cb), (case.id, ws, n_long, cb)
    cross, autos = cg.oracle(case, cu)
    which = cg.oracle_pairs(case)
    allp = cg.pairs(case.n_ant)
    idx = list(range(nb)) if len(which) == nb else [allp.index(p) for p in which]
    err, row = cg.worst_row(integ[idx], cross)
    own = cg.rel_err(integ, rows_mean)
    print("%s: %d + %d chunks, cg >= %d; %d of %d baselines against the oracle: %.3g at %s; against the mean of the plan's rows: %.3g"
          % (case.id, cg.SHORT, n_long, min(cg.cg_min(case, cu, nc) for nc in cg.pass_lengths(case, cu)), len(which), nb, err, which[row], own))
    assert err < TOL_VIS, (case.id, "baseline", which[row], err)
    assert own < OWN_ROWS, (case.id, own)
    if case.autos:
        a_err, ant = cg.worst_row(integ[nb:], autos)
        print("%s: autos against the oracle: %.3g at antenna %d" % (case.id, a_err, ant))
        assert a_err < TOL_VIS, (case.id, "antenna", ant, a_err)
        assert (integ[nb:].imag == 0).all() and (integ[nb:].real >= 0).all(), case.id


@pytest.mark.parametrize("case", IN_PROCESS, ids=lambda c: c.id)
def test_chunk_groups_match_the_oracle(plan_mod, torch, cu_count, case):
    xd = torch.from_numpy(cg.samples(case, cu_count).copy()).cuda()
    check(case, cu_count, cg.device_outputs(plan_mod, torch, xd, case))


CHILD = r'''
import sys
import numpy as np, torch
for p in sys.argv[1:4]:
    sys.path.insert(0, p)
import chunk_group_cases as cg
from effex_amd import plan as plan_mod
case = cg.BY_ID[sys.argv[4]]
xd = torch.from_numpy(np.load(sys.argv[6])).cuda()
np.savez(sys.argv[7], **cg.device_outputs(plan_mod, torch, xd, case, dev=sys.argv[5] == "dev"))
'''


def in_child(case, x, env, dev=False):
    with tempfile.TemporaryDirectory() as tmp:
        src, res = os.path.join(tmp, "x.npy"), os.path.join(tmp, "r.npz")
        np.save(src, x)
        proc = subprocess.run([sys.executable, "-c", CHILD, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), ROOT, case.id,
                               "dev" if dev else "shipped", src, res], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
        assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-2000:]
        return dict(np.load(res))


@pytest.mark.parametrize("case", PASSES, ids=lambda c: c.id)
def test_chunk_groups_in_several_passes_match_the_oracle(plan_mod, torch, cu_count, case):
    """the long call in passes of cb, cb and fewer chunks (a workspace target of a few MiB): every pass groups its own chunks and
    ends in a shorter group of its own.  Against the oracle, and against the same integration in one pass (the default workspace)
    to 2e-6 of its largest value -- the groups differ, so the bits may"""
    mb, cb, n_long = cg.pass_plan(case, cu_count)
    x = cg.samples(case, cu_count)
    whole = cg.device_outputs(plan_mod, torch, torch.from_numpy(x.copy()).cuda(), case)
    check(case, cu_count, whole)
    out = in_child(case, x, {"FXC_WS_MB": str(mb)})
    lengths = cg.pass_lengths(case, cu_count)
    print("%s: FXC_WS_MB=%d, passes of %s chunks" % (case.id, mb, lengths))
    assert len(lengths) >= 3 and lengths[0] == cb
    check(case, cu_count, out, cb=cb)
    diff = cg.rel_err(out["integ"], whole["integ"])
    print("%s: passes against one pass: %.3g" % (case.id, diff))
    assert diff < 2e-6, (case.id, diff)


def dev_kernels():
    """the developer library is there and reports its kernels (fxc_dev_kernels): xengine_block_kernel behind FXC_XENGINE=block"""
    from effex_amd import _lib
    try:
        return _lib.load(dev=True).fxc_dev_kernels() == 1
    except (ImportError, OSError):
        return False


@pytest.mark.parametrize("case", BLOCK, ids=lambda c: c.id)
def test_block_kernel_chunk_groups_match_the_oracle(plan_mod, torch, cu_count, case):
    """xengine_block_kernel, the vector X-engine over blocks of 8 antennas the matrix-core one replaced: its chunk loop with
    several trips, against the oracle and against the matrix-core kernel's integration of the same samples"""
    if not dev_kernels():
        pytest.skip("release build: no developer kernels (fxc_dev_kernels() == 0), so no xengine_block_kernel to run")
    x = cg.samples(case, cu_count)
    out = in_child(case, x, {"FXC_XENGINE": "block"}, dev=True)
    check(case, cu_count, out)
    mfma = cg.device_outputs(plan_mod, torch, torch.from_numpy(x.copy()).cuda(), case._replace(kernel="mfma"))
    diff = cg.rel_err(out["integ"], mfma["integ"])
    print("%s: block kernel against the matrix-core kernel: %.3g" % (case.id, diff))
    assert diff < 2e-6, (case.id, diff)
    # (another summation order: the same bits would mean the knob did not take)
    assert not np.array_equal(out["integ"], mfma["integ"]), case.id
