"""Per-antenna delay correction and one-call delay calibration on the GPU (include/fxcorr.h fxc_set_rot_ant, fxc_estimate_delays).

Oracle of cross row (a, b): fftshift(mean_i f_a[i, k] r_a[k] conj(f_b[i, k] r_b[k])) over the spectra of
fx_oracle.spectrometer_poly, with r_a = fx_oracle.rot_table(tau_a); CONTINUUM: its mean over the bins / bandwidth
(effex.py:523-524).  With r_0 = 1 and r_1 = rot that is the reference's f0 conj(f1 rot) (effex.py:516-521).  Bounds: TOL_VIS
of the largest magnitude.  Delays: fxc_estimate_delays against the pairwise fxc_estimate_delay, bit for bit."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import fx_oracle
from effex_amd import synth
from effex_amd.window import design_window

pytestmark = pytest.mark.gpu

from tolerances import TOL_VIS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BW = 2.4e6
FREQ = 1.4204e9


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def plan_mod(torch):
    from effex_amd import plan
    return plan


def rel_err(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def taus(n_ant):
    """distinct per-antenna delays, antenna 0 included, with distinct differences between neighbours"""
    return np.array([1e-7 * ((3 * a * a) % 17 + 0.25 * a) for a in range(n_ant)]) - 0.2e-6


def tables(n_ant, nchan, tau):
    return np.stack([fx_oracle.rot_table(nchan, BW, FREQ, t) for t in tau])


def oracle(x, nchan, window, rots):
    """x [n_chunks, A, num_samp], rots [A, nchan] -> per-chunk cross rows [C, NB, nchan] and their mean over the chunks"""
    n_chunks, n_ant, _ = x.shape
    ntaps = len(window) // nchan
    pairs = [(a, b) for a in range(n_ant) for b in range(a + 1, n_ant)]
    cross = np.zeros((n_chunks, len(pairs), nchan), np.complex128)
    for c in range(n_chunks):
        specs = [fx_oracle.spectrometer_poly(x[c, a], ntaps, nchan, window) * rots[a] for a in range(n_ant)]
        for p, (a, b) in enumerate(pairs):
            cross[c, p] = np.fft.fftshift((specs[a] * np.conj(specs[b])).mean(axis=0))
    return cross, cross.mean(axis=0)


# every route of 3 and more antennas: tiled, small, the F stage built per channel count, the F-only fused kernel +
# xengine_kernel<8>, 8192 channels, the MFMA X-engine (12 and 16 antennas)
ROUTES = [  # n_ant, nchan, num_samp, n_chunks, path
    (3, 64, 64 * 20, 5, "tiled"), (4, 128, 128 * 20, 5, "tiled"), (3, 1000, 1000 * 8 + 3, 4, None),
    (8, 4096, 4096 * 4, 3, "fused"), (3, 8192, 8192 * 5, 3, None), (12, 256, 256 * 20, 3, None),
    (16, 4096, 4096 * 4, 2, None)]


@pytest.mark.parametrize("n_ant,nchan,num_samp,n_chunks,path", ROUTES)
def test_per_antenna_rot_matches_the_oracle(plan_mod, torch, n_ant, nchan, num_samp, n_chunks, path):
    """fx_rows, fx_accumulate + finalize, finalize_async and acc_export + finalize_sums, SPECTRUM and CONTINUUM, with one table
    per antenna; a shared set_rot of the same data puts a baseline without antenna 0 elsewhere."""
    x_np = synth.synth_iq(3, n_chunks, n_ant, num_samp, delays=np.arange(n_ant) % 5)
    x = torch.from_numpy(x_np).cuda()
    window = design_window(4, nchan)
    tau = taus(n_ant)
    rots = tables(n_ant, nchan, tau)
    cross, cross_i = oracle(x_np, nchan, window, rots)
    nb = n_ant * (n_ant - 1) // 2
    with plan_mod.FxPlan(n_ant, nchan, 4, num_samp, window=window, path=path) as plan:
        plan.set_delays(tau, BW, FREQ)
        rows = host(plan.fx_rows(x, "SPECTRUM"))
        assert rows.shape == (n_chunks, nb, nchan)
        assert rel_err(rows, cross) < TOL_VIS
        cont = host(plan.fx_rows(x, "CONTINUUM", BW))
        assert rel_err(cont, cross.mean(axis=-1) / BW) < TOL_VIS
        plan.fx_accumulate(x)
        integ = plan.finalize("SPECTRUM", reset=False)
        assert rel_err(integ, cross_i) < TOL_VIS
        assert rel_err(plan.finalize("SPECTRUM", reset=False), cross_i) < TOL_VIS      # nothing pending: acc_finish_kernel<true>
        integ_c = plan.finalize("CONTINUUM", BW)
        assert rel_err(integ_c, cross_i.mean(axis=-1) / BW) < TOL_VIS
        plan.fx_accumulate(x)
        plan.finalize_async("SPECTRUM")
        assert rel_err(plan.finalize_wait(), cross_i) < TOL_VIS
        plan.fx_accumulate(x)
        sums = plan.new_sums()
        plan.acc_export(sums)
        plan.acc_reset()
        assert rel_err(plan.finalize_sums(sums, "SPECTRUM"), cross_i) < TOL_VIS
        assert rel_err(plan.finalize_sums(sums, "CONTINUUM", BW), cross_i.mean(axis=-1) / BW) < TOL_VIS
        # one shared table (antenna 1's, as in the 2-antenna reference): baseline (1, 2) comes out with another phase
        plan.set_rot(rots[1] * np.conj(rots[0]))
        shared = host(plan.fx_rows(x, "SPECTRUM"))
        p12 = n_ant - 1
        assert np.abs(shared[:, p12] - cross[:, p12]).max() > 1e-3 * np.abs(cross).max()


TWO_ANT = [(4096, 4096 * 5, 3, "fused"), (2048, 2048 * 9 + 5, 4, "tiled"), (1000, 1000 * 8 + 3, 4, None),
           (8192, 8192 * 5, 3, "tiled")]


@pytest.mark.parametrize("nchan,num_samp,n_chunks,path", TWO_ANT)
def test_two_antennas_tables_are_set_rot(plan_mod, torch, nchan, num_samp, n_chunks, path):
    """set_rot_ant([ones, rot]) is set_rot(rot), bit for bit, on the 2-antenna routes (fused, tiled, per channel count, 8192)."""
    x = torch.from_numpy(synth.synth_iq(5, n_chunks, 2, num_samp)).cuda()
    rot = fx_oracle.rot_table(nchan, BW, FREQ, 7.3e-7)
    out = []
    for use_tables in (False, True):
        with plan_mod.FxPlan(2, nchan, 4, num_samp, path=path) as plan:
            if use_tables:
                plan.set_rot_ant(np.stack([np.ones(nchan, np.complex128), rot]))
            else:
                plan.set_rot(rot)
            rows = host(plan.fx_rows(x, "SPECTRUM"))
            cont = host(plan.fx_rows(x, "CONTINUUM", BW))
            plan.fx_accumulate(x)
            integ = plan.finalize("SPECTRUM", reset=False)
            out.append((rows, cont, integ, plan.finalize("CONTINUUM", BW)))
    for a, b in zip(*out):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("n_ant,nchan,num_samp,n_chunks,path", [ROUTES[0], ROUTES[2], ROUTES[3], ROUTES[5]])
def test_unit_tables_and_set_rot_after_tables(plan_mod, torch, n_ant, nchan, num_samp, n_chunks, path):
    """All-ones tables give what a fresh plan gives, bit for bit; set_rot after set_rot_ant gives what a plan that only ever had
    set_rot gives."""
    x = torch.from_numpy(synth.synth_iq(7, n_chunks, n_ant, num_samp, delays=np.arange(n_ant) % 5)).cuda()
    rot = fx_oracle.rot_table(nchan, BW, FREQ, 4.1e-7)

    def run(plan):
        rows = host(plan.fx_rows(x, "SPECTRUM"))
        cont = host(plan.fx_rows(x, "CONTINUUM", BW))
        plan.fx_accumulate(x)
        integ = plan.finalize("SPECTRUM", reset=False)
        return rows, cont, integ, plan.finalize("CONTINUUM", BW)

    with plan_mod.FxPlan(n_ant, nchan, 4, num_samp, path=path) as plan:
        fresh = run(plan)
    with plan_mod.FxPlan(n_ant, nchan, 4, num_samp, path=path) as plan:
        plan.set_rot_ant(np.ones((n_ant, nchan), np.complex128))
        unit = run(plan)
        plan.set_rot_ant(tables(n_ant, nchan, taus(n_ant)))
        plan.set_rot(rot)
        after = run(plan)
    with plan_mod.FxPlan(n_ant, nchan, 4, num_samp, path=path) as plan:
        plan.set_rot(rot)
        only = run(plan)
    for a, b in zip(fresh, unit):
        assert np.array_equal(a, b)
    for a, b in zip(after, only):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("n_ant,nchan,num_samp,path", [(3, 64, 64 * 20, "tiled"), (4, 4096, 4096 * 4, "fused"),
                                                       (3, 1000, 1000 * 8 + 3, None)])
def test_tables_leave_the_autos_alone(plan_mod, torch, n_ant, nchan, num_samp, path):
    n_chunks = 3
    x_np = synth.synth_iq(9, n_chunks, n_ant, num_samp, delays=np.arange(n_ant) % 5)
    x = torch.from_numpy(x_np).cuda()
    window = design_window(4, nchan)
    tau = taus(n_ant)
    cross, cross_i = oracle(x_np, nchan, window, tables(n_ant, nchan, tau))
    nb = n_ant * (n_ant - 1) // 2
    with plan_mod.FxPlan(n_ant, nchan, 4, num_samp, window=window, path=path, autos=True) as plan:
        plain = host(plan.fx_rows(x, "SPECTRUM"))
        plan.fx_accumulate(x)
        plain_i = plan.finalize("SPECTRUM")
        plan.set_delays(tau, BW, FREQ)
        rows = host(plan.fx_rows(x, "SPECTRUM"))
        plan.fx_accumulate(x)
        integ = plan.finalize("SPECTRUM", reset=False)
        integ_c = plan.finalize("CONTINUUM", BW)
    assert rel_err(rows[:, :nb], cross) < TOL_VIS and rel_err(integ[:nb], cross_i) < TOL_VIS
    assert np.array_equal(rows[:, nb:], plain[:, nb:]) and np.array_equal(integ[nb:], plain_i[nb:])
    assert np.all(rows[:, nb:].imag == 0.0) and np.all(integ[nb:].imag == 0.0) and np.all(integ_c[nb:].imag == 0.0)


def test_pipeline_batch_takes_the_tables(plan_mod, torch):
    n_ant, nchan, num_samp = 8, 4096, 4096 * 4
    x = synth.synth_iq(11, 5, n_ant, num_samp)
    with plan_mod.FxPlan(n_ant, nchan, 4, num_samp) as plan:
        plan.set_delays(taus(n_ant), BW, FREQ)
        want = host(plan.fx_rows(torch.from_numpy(x).cuda(), "SPECTRUM"))
        with plan_mod.FxPipeline(plan, 5, depth=2, mode="SPECTRUM") as pipe:
            pipe.push(x)
            got = pipe.pop()
    assert np.array_equal(got, want)


# -- calibration ------------------------------------------------------------------------------------------------------------
RATE = 2.4e6


def shifted_streams(n_ant, n, seed):
    """n_ant noisy copies of one stream, shifted by a few samples each (not at all for the shortest streams, whose peak would
    otherwise fall on the last lag for some pairs)"""
    rng = np.random.default_rng(seed)
    base = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    out = np.empty((n_ant, n), np.complex64)
    for a in range(n_ant):
        shift = 0 if n < 8 else (3 * a) % 11
        out[a] = np.roll(base, shift) + 0.05 * (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    return out


def pairwise(plan, x, ref):
    d = np.array([plan.estimate_delay(x[ref], x[a], RATE) for a in range(len(x))])
    d[ref] = 0.0
    return d


@pytest.mark.parametrize("n_ant", [3, 8, 16])
@pytest.mark.parametrize("n", [3, 4099, 262144])
def test_estimate_delays_is_the_pairwise_call(plan_mod, torch, n_ant, n):
    x = shifted_streams(n_ant, n, n_ant * 1000 + n)
    xd = torch.from_numpy(x).cuda()
    with plan_mod.FxPlan(n_ant, 512, 4, 4096) as plan:
        for ref in (0, n_ant - 2):
            want = pairwise(plan, x, ref)
            for data in (x, xd):
                got = plan.estimate_delays(data, RATE, ref=ref)
                assert got.dtype == np.float64 and got.shape == (n_ant,)
                assert got[ref] == 0.0
                assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (ref, got, want)


def test_estimate_delays_in_groups(plan_mod, torch):
    """A small workspace target (FXC_WS_MB, read once per process: a child) makes the streams go through in several groups
    against the reference's one spectrum: the delays stay those of the pairwise call, host and device input alike."""
    n_ant, n = 16, 262144
    x = shifted_streams(n_ant, n, 77)
    with plan_mod.FxPlan(n_ant, 512, 4, 4096) as plan:
        want = {ref: pairwise(plan, x, ref) for ref in (0, 5)}
    code = ("import numpy as np, torch, sys; sys.path.insert(0, %r); from effex_amd import plan\n"
            "x = np.load(sys.argv[1]); xd = torch.from_numpy(x).cuda(); out = {}\n"
            "with plan.FxPlan(x.shape[0], 512, 4, 4096) as p:\n"
            "    for ref in (0, 5):\n"
            "        out['h%%d' %% ref] = p.estimate_delays(x, 2.4e6, ref=ref); out['d%%d' %% ref] = p.estimate_delays(xd, 2.4e6, ref=ref)\n"
            "np.savez(sys.argv[2], **out)\n" % ROOT)
    with tempfile.TemporaryDirectory() as tmp:
        np.save(os.path.join(tmp, "x.npy"), x)
        subprocess.run([sys.executable, "-c", code, os.path.join(tmp, "x.npy"), os.path.join(tmp, "r.npz")], check=True,
                       env=dict(os.environ, FXC_WS_MB="30"), timeout=600)
        got = np.load(os.path.join(tmp, "r.npz"))
        for ref in (0, 5):
            for kind in "hd":
                assert np.array_equal(got["%s%d" % (kind, ref)].view(np.uint64), want[ref].view(np.uint64)), (kind, ref)


def test_estimate_delays_argument_checks(plan_mod, torch):
    from effex_amd import _lib
    x = shifted_streams(3, 64, 1)
    with plan_mod.FxPlan(3, 64, 4, 64 * 20) as plan:
        for ref in (-1, 3):
            with pytest.raises(ValueError):
                plan.estimate_delays(x, RATE, ref=ref)
        out = np.zeros(3)
        lib = plan._lib
        assert lib.fxc_estimate_delays(plan._h, x.ctypes.data, 1, _lib.FXC_MEM_HOST, RATE, 0, out.ctypes.data) == _lib.FXC_ERR_ARG
        assert lib.fxc_estimate_delays(plan._h, x.ctypes.data, 64, _lib.FXC_MEM_HOST, 0.0, 0, out.ctypes.data) == _lib.FXC_ERR_ARG
        assert lib.fxc_estimate_delays(plan._h, None, 64, _lib.FXC_MEM_HOST, RATE, 0, out.ctypes.data) == _lib.FXC_ERR_ARG
        assert lib.fxc_set_rot_ant(plan._h, None) == _lib.FXC_ERR_ARG
        with pytest.raises(ValueError):
            plan.set_rot_ant(np.ones((2, 64), np.complex128))


def coherence(spec):
    """|mean_k X| / mean_k |X| of each row"""
    return np.abs(spec.mean(axis=-1)) / np.abs(spec).mean(axis=-1)


def test_array_calibration_end_to_end(plan_mod, torch):
    """synth_iq's integer per-antenna delays: estimate_delays finds them, set_delays phases every baseline of the array."""
    n_ant, nchan, num_samp, n_chunks = 8, 4096, 4096 * 64, 2
    d = np.array(synth.DEFAULT_DELAYS[:n_ant])
    x = torch.from_numpy(synth.synth_iq(21, n_chunks, n_ant, num_samp)).cuda()
    pairs = [(a, b) for a in range(n_ant) for b in range(a + 1, n_ant)]
    with plan_mod.FxPlan(n_ant, nchan, 4, num_samp) as plan:
        tau = plan.estimate_delays(x[0], RATE)
        assert tau[0] == 0.0
        assert np.all(np.abs(tau * RATE - (d - d[0])) < 0.5), tau * RATE
        plan.fx_accumulate(x)
        raw = plan.finalize("SPECTRUM")
        plan.set_delays(tau, RATE, 0.0)
        plan.fx_accumulate(x)
        phased = plan.finalize("SPECTRUM")
    c_raw, c_phased = coherence(raw), coherence(phased)
    assert np.all(c_phased > 0.9), c_phased
    for p, (a, b) in enumerate(pairs):
        if d[a] != d[b]:
            assert c_raw[p] < 0.5, (a, b, c_raw[p])
