"""Whole-sample delays on the GPU (include/fxcorr.h fxc_set_sample_delays, fxc_set_delay_track_aligned): antenna a's samples
are read s_a later, zeros where the chunk has none, ahead of the F stage; the tables keep the remainder.

The alignment is a copy of bits, so rows of a plan with shifts are compared BIT FOR BIT with the rows a plan without shifts
makes of tests/align_ref.py::align(x, s) under the same tables, route by route (the routes of tests/test_gpu_tracking.py).
What has no bit-exact twin (complex128 input, the aligned track) is compared with the float64 oracle under TOL_VIS / TOL_CONT;
the aligned track's tables have a derived bound of their own."""
import numpy as np
import pytest

import align_ref
import fx_oracle
from effex_amd import _lib, synth
from effex_amd.window import design_window
from tolerances import TOL_CONT, TOL_VIS

pytestmark = pytest.mark.gpu

BW = 2.4e6
FREQ = 1.42e9


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


def same_bits(a, b):
    a, b = np.ascontiguousarray(host(a)), np.ascontiguousarray(host(b))
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def make_plan(plan_mod, n_ant, nchan, num_samp, path=None, autos=False):
    window = design_window(4, nchan)
    return plan_mod.FxPlan(n_ant, nchan, 4, num_samp, window=window, path=path, autos=autos), window


def shift_sets(n_ant, nchan, num_samp):
    """a zero, an odd positive, an even negative, one larger than nchan and +-(num_samp - 1), dealt over the antennas"""
    vals = [0, 3, -4, nchan + 5, num_samp - 1, -(num_samp - 1)]
    n_sets = max(1, -(-len(vals) // n_ant))
    return [np.array([vals[(i * n_ant + a) % len(vals)] for a in range(n_ant)], dtype=np.int64) for i in range(n_sets)]


ROUTES = [  # n_ant, nchan, num_samp, n_chunks, path asked for, path taken, autos
    (2, 4096, 4096 * 6, 4, "fused", "fused", False), (2, 1024, 1024 * 9 + 5, 4, "tiled", "tiled", False),
    (2, 64, 64 * 20, 5, "tiled", "tiled", False), (2, 1000, 1000 * 8 + 3, 3, None, "generic", False),
    (2, 8192, 8192 * 5, 3, None, "tiled", False), (2, 1, 4096, 4, None, "stream", False),
    (3, 1024, 1024 * 8, 3, None, "tiled", False), (3, 1024, 1024 * 8, 3, None, "tiled", True),
    (8, 4096, 4096 * 4, 3, "fused", "fused", False), (12, 1024, 1024 * 6, 3, None, "tiled", False)]


# -- 1. bit-for-bit rows ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ant,nchan,num_samp,n_chunks,path,taken,autos", ROUTES)
def test_rows_are_those_of_the_aligned_samples(plan_mod, torch, n_ant, nchan, num_samp, n_chunks, path, taken, autos):
    x_np = synth.synth_iq(21, n_chunks, n_ant, num_samp, delays=np.arange(n_ant) % 5)
    x = torch.from_numpy(x_np).cuda()
    tables = plan_mod.rot_tables(nchan, BW, FREQ, 1e-6 * np.arange(n_ant))
    plan, _ = make_plan(plan_mod, n_ant, nchan, num_samp, path, autos)
    fresh, _ = make_plan(plan_mod, n_ant, nchan, num_samp, path, autos)
    with plan, fresh:
        assert plan.path == taken and fresh.path == taken
        for key in ("path", "grid", "block", "lds_bytes"):
            assert plan.info[key] == fresh.info[key]
        plan.set_rot_ant(tables)
        fresh.set_rot_ant(tables)
        assert not plan.sample_delays().any()
        for i, s in enumerate(shift_sets(n_ant, nchan, num_samp)):
            plan.set_sample_delays(s)
            assert np.array_equal(plan.sample_delays(), s) and np.array_equal(plan.sample_delays(7), s)
            xa = torch.from_numpy(align_ref.align(x_np, s)).cuda()
            for mode in ("SPECTRUM", "CONTINUUM"):
                got = plan.fx_rows(x, mode, BW)
                assert same_bits(got, fresh.fx_rows(xa, mode, BW)), (mode, s)
                if i == 0:      # host input: the same bits
                    assert same_bits(plan.fx_rows(x_np, mode, BW), got), mode
            plan.fx_accumulate(x)
            fresh.fx_accumulate(xa)
            for mode, reset in (("SPECTRUM", False), ("CONTINUUM", True)):
                assert same_bits(plan.finalize(mode, BW, reset=reset), fresh.finalize(mode, BW, reset=reset)), (mode, s)
            if i == 0:
                plan.fx_accumulate(x_np)
                fresh.fx_accumulate(xa)
                assert same_bits(plan.finalize("SPECTRUM"), fresh.finalize("SPECTRUM"))


# -- 2. formats -------------------------------------------------------------------------------------------------------------
FORMAT_ROUTES = [(2, 4096, 4096 * 6, 3, "fused"), (2, 1024, 1024 * 9 + 5, 3, "tiled"), (3, 1000, 1000 * 8 + 3, 3, None)]


@pytest.mark.parametrize("n_ant,nchan,num_samp,n_chunks,path", FORMAT_ROUTES)
def test_conditioned_formats_are_conditioned_then_aligned(plan_mod, torch, n_ant, nchan, num_samp, n_chunks, path):
    """Bytes with and without DC removal and complex64 with DC removal: the bits of the plain plan on the aligned output of
    convert_u8 / remove_dc (the mean is that of the delivered samples, the fill exact zeros).  complex128 with DC removal: host
    and device input give the same bits, within TOL_VIS of the float64 oracle."""
    rng = np.random.default_rng(8)
    u8 = rng.integers(0, 256, size=(n_chunks, n_ant, num_samp, 2), dtype=np.uint8)
    u8[..., 0] //= 2          # a mean well away from 127.5
    x8 = torch.from_numpy(u8).cuda()
    x_np = synth.synth_iq(4, n_chunks, n_ant, num_samp, delays=np.arange(n_ant)) + np.complex64(0.25 - 0.125j)
    x = torch.from_numpy(x_np).cuda()
    s = np.array([3, -4, nchan + 5][:n_ant], dtype=np.int64)
    tables = plan_mod.rot_tables(nchan, BW, FREQ, 1e-6 * np.arange(n_ant))
    plan, window = make_plan(plan_mod, n_ant, nchan, num_samp, path)
    fresh, _ = make_plan(plan_mod, n_ant, nchan, num_samp, path)
    with plan, fresh:
        plan.set_rot_ant(tables)
        fresh.set_rot_ant(tables)
        plan.set_sample_delays(s)
        for dc in (True, False):
            conv = host(fresh.convert_u8(x8, dc))
            want = fresh.fx_rows(torch.from_numpy(align_ref.align(conv, s)).cuda(), "SPECTRUM")
            assert same_bits(plan.fx_rows_u8(x8, "SPECTRUM", remove_dc=dc), want), dc
            assert same_bits(plan.fx_rows_u8(u8, "SPECTRUM", remove_dc=dc), want), dc
        dem = host(fresh.remove_dc(x, out=torch.empty_like(x)))
        want = fresh.fx_rows(torch.from_numpy(align_ref.align(dem, s)).cuda(), "SPECTRUM")
        assert same_bits(plan.fx_rows(x, "SPECTRUM", remove_dc=True), want)
        assert same_bits(plan.fx_rows(x_np, "SPECTRUM", remove_dc=True), want)
        assert same_bits(x, x_np)          # the caller's device buffer is never written
        x128_np = x_np.astype(np.complex128) * (1.0 + 2.0 ** -30)
        x128 = torch.from_numpy(x128_np).cuda()
        got = plan.fx_rows(x128, "SPECTRUM", remove_dc=True, c128=True)
        assert same_bits(plan.fx_rows(x128_np, "SPECTRUM", remove_dc=True, c128=True), got)
        dem128 = np.stack([np.stack([fx_oracle.remove_dc(x128_np[c, a]) for a in range(n_ant)]) for c in range(n_chunks)])
        ref = align_ref.rows(align_ref.align(dem128, s), nchan, window, tables)
        err = rel_err(host(got), ref)
        print("complex128 with DC removal, aligned, against the oracle: %.3g" % err)
        assert err < TOL_VIS


# -- 3. the pipe ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["c64", "u8"])
def test_pipe_batches_give_the_bits_of_fx_rows(plan_mod, torch, fmt):
    n_ant, nchan, num_samp, K = 2, 4096, 4096 * 6, 2
    if fmt == "u8":
        batches = np.random.default_rng(5).integers(0, 256, size=(2, K, n_ant, num_samp, 2), dtype=np.uint8)
    else:
        batches = synth.synth_iq(9, 2 * K, n_ant, num_samp).reshape(2, K, n_ant, num_samp)
    plan, _ = make_plan(plan_mod, n_ant, nchan, num_samp)
    with plan:
        plan.set_delays([0.0, 7.3 / BW], BW, FREQ, whole_samples=True)
        assert plan.sample_delays().tolist() == [0, 7]
        rows = lambda b: plan.fx_rows_u8(b, "SPECTRUM") if fmt == "u8" else plan.fx_rows(b, "SPECTRUM")
        want = [host(rows(b)) for b in batches]
        with plan_mod.FxPipeline(plan, K, depth=2, mode="SPECTRUM", fmt=fmt) as pipe:
            for b in batches:
                pipe.push(b)
            for w in want:
                assert same_bits(pipe.pop(), w)
            # like set_rot_ant, the shifts may change while a pipe uses the plan: they apply to the next batch
            plan.set_sample_delays([0, -2])
            pipe.push(batches[0])
            assert same_bits(pipe.pop(), rows(batches[0]))


# -- 4. clearing ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ant,nchan,num_samp,path", [(2, 4096, 4096 * 6, "fused"), (3, 1024, 1024 * 8, None)])
def test_cleared_shifts_leave_the_plan_as_it_was(plan_mod, torch, n_ant, nchan, num_samp, path):
    """set_sample_delays(None) and all-zero shifts: the rows of a plan that never had shifts and its launch count -- the
    alignment pass is gone, not run with zeros."""
    x = torch.from_numpy(synth.synth_iq(2, 3, n_ant, num_samp)).cuda()
    plan, _ = make_plan(plan_mod, n_ant, nchan, num_samp, path)
    fresh, _ = make_plan(plan_mod, n_ant, nchan, num_samp, path)

    def launches(p):
        p.kernel_profiling(True)
        p.kernel_time()
        out = p.fx_rows(x, "SPECTRUM")
        n = p.kernel_time()[1]
        p.kernel_profiling(False)
        return host(out), n

    with plan, fresh:
        want, n_plain = launches(fresh)
        plan.set_sample_delays(np.arange(n_ant) + 1)
        shifted, n_shifted = launches(plan)
        assert n_shifted == n_plain + 1 and not same_bits(shifted, want)
        for clear in (None, np.zeros(n_ant, dtype=np.int64)):
            plan.set_sample_delays(np.arange(n_ant) + 1)
            plan.set_sample_delays(clear)
            assert not plan.sample_delays().any()
            got, n = launches(plan)
            assert same_bits(got, want) and n == n_plain


# -- 5. the aligned track ---------------------------------------------------------------------------------------------------
TRACK_ROUTES = [(3, 1024, 1024 * 8, 4, None, False), (2, 4096, 4096 * 6, 4, "fused", False), (2, 1000, 1000 * 8 + 3, 4, None, False),
                (3, 1024, 1024 * 8, 4, None, True)]
T0 = 37


def aligned_track_of(n_ant):
    """delays in samples at chunk T0 + c: antenna 0 stays at 5.2 (never steps), antenna 1 is 10.4 + 0.3 c (10, 11, 11, 11:
    one step up), antenna 2 is -7.4 - 0.3 c (-7, -8, -8, -8: one step down); two antennas: 0 stays, 1 steps down"""
    at_t0 = np.array([5.2, 10.4, -7.4])
    slope = np.array([0.0, 0.3, -0.3])
    if n_ant == 2:
        at_t0, slope = at_t0[[0, 2]], slope[[0, 2]]
    rate = slope / BW
    return at_t0 / BW - T0 * rate, rate


def track_reference(plan_mod, x_np, nchan, window, tau0, rate, n_chunks, autos=False, gains=None):
    shifts = np.stack([align_ref.track_shifts(tau0, rate, BW, T0 + c) for c in range(n_chunks)])
    if gains is None:
        tabs = np.stack([align_ref.tables(nchan, BW, FREQ, tau0 + float(T0 + c) * rate, shifts[c]) for c in range(n_chunks)])
    else:
        tabs = np.stack([plan_mod.gain_track_tables(gains, 2, T0, T0 + c, tau0, rate, BW, FREQ, whole_samples=True) for c in range(n_chunks)])
    return shifts, tabs, align_ref.rows(align_ref.align(x_np, shifts), nchan, window, tabs, autos)


@pytest.mark.parametrize("n_ant,nchan,num_samp,n_chunks,path,autos", TRACK_ROUTES)
def test_aligned_track(plan_mod, torch, n_ant, nchan, num_samp, n_chunks, path, autos):
    x_np = synth.synth_iq(21, n_chunks, n_ant, num_samp, delays=(5, 10, 0)[:n_ant])
    x = torch.from_numpy(x_np).cuda()
    tau0, rate = aligned_track_of(n_ant)
    plan, window = make_plan(plan_mod, n_ant, nchan, num_samp, path, autos)
    shifts, tabs, ref = track_reference(plan_mod, x_np, nchan, window, tau0, rate, n_chunks, autos)
    steps = np.diff(shifts, axis=0)
    assert (steps == 0).all(axis=0).any() and (np.abs(steps) <= 1).all()
    assert (steps == -1).any() and ((steps == 1).any() or n_ant == 2)
    freqs = np.fft.fftfreq(nchan, d=1.0 / BW) + FREQ
    with plan:
        plan.set_sample_delays(np.arange(n_ant) + 2)
        plan.set_delay_track(tau0, rate, BW, FREQ, first_chunk=T0, whole_samples=True)
        assert plan.track_chunk == T0
        # the shifts, exactly; the tables under the bound of test_gpu_tracking.py::test_track_tables, its constant term doubled
        for c in range(n_chunks):
            assert np.array_equal(plan.sample_delays(T0 + c), shifts[c])
            got = plan.track_tables(T0 + c)
            tau = tau0 + float(T0 + c) * rate
            bound = 4 * np.pi * np.abs(freqs[None, :] * tau[:, None]) * 2.0 ** -52 + 16 * 2.0 ** -52
            assert (np.abs(got.real - tabs[c].real) <= bound).all() and (np.abs(got.imag - tabs[c].imag) <= bound).all()
        assert plan.track_chunk == T0
        rows = host(plan.fx_rows(x, "SPECTRUM"))
        assert plan.track_chunk == T0 + n_chunks
        err = rel_err(rows, ref)
        print("aligned track rows against the oracle: %.3g" % err)
        assert err < TOL_VIS
        plan.track_seek(T0)
        cont = host(plan.fx_rows(x, "CONTINUUM", BW))
        assert rel_err(cont, ref.mean(axis=-1) / BW) < TOL_CONT
        # one by one, and after a seek: the same bits
        plan.track_seek(T0)
        one = np.concatenate([host(plan.fx_rows(x[c:c + 1], "SPECTRUM")) for c in range(n_chunks)])
        assert same_bits(one, rows)
        plan.track_seek(T0 + 2)
        assert same_bits(plan.fx_rows(x[2:], "SPECTRUM"), rows[2:])
        # the tracked integration
        plan.track_seek(T0)
        plan.fx_accumulate(x)
        assert plan.track_chunk == T0 + n_chunks
        integ = plan.finalize("SPECTRUM", reset=False)
        assert rel_err(integ, ref.mean(axis=0)) < TOL_VIS
        assert rel_err(plan.finalize("CONTINUUM", BW), ref.mean(axis=0).mean(axis=-1) / BW) < TOL_CONT
        # a gain track on top: unit gains are the aligned track's bits, other gains the oracle's rows
        plan.set_track_gains(np.ones((n_ant, nchan), dtype=np.complex128))
        plan.track_seek(T0)
        assert same_bits(plan.fx_rows(x, "SPECTRUM"), rows)
        rng = np.random.default_rng(11)
        gains = (1.0 + 0.2 * rng.standard_normal((2, n_ant, nchan))) * np.exp(2j * np.pi * rng.random((2, n_ant, nchan)))
        plan.set_track_gains(gains, interval=2, first_chunk=T0)
        _, gtabs, gref = track_reference(plan_mod, x_np, nchan, window, tau0, rate, n_chunks, autos, gains)
        # (the phasor's bound above on either component, times |q|, and the product's own roundings)
        got, tau = plan.track_tables(T0 + 3), tau0 + float(T0 + 3) * rate
        bound = 4 * np.pi * np.abs(freqs[None, :] * tau[:, None]) * 2.0 ** -52 + 16 * 2.0 ** -52
        assert (np.abs(got - gtabs[3]) <= 2 * (bound + 4 * 2.0 ** -52) * np.maximum(np.abs(gtabs[3]), 1e-300)).all()
        plan.track_seek(T0)
        assert rel_err(host(plan.fx_rows(x, "SPECTRUM")), gref) < TOL_VIS
        # a plain track ends the aligned behaviour and keeps a track
        plan.set_delay_track(tau0, rate, BW, FREQ, first_chunk=T0)
        assert not plan.sample_delays(T0).any()


def test_aligned_track_of_shifts_past_the_chunk_is_zeros_not_an_error(plan_mod, torch):
    n_ant, nchan, num_samp = 2, 64, 64 * 20
    x = torch.from_numpy(synth.synth_iq(3, 2, n_ant, num_samp)).cuda()
    plan, _ = make_plan(plan_mod, n_ant, nchan, num_samp)
    with plan:
        plan.set_delay_track([0.0, (num_samp + 3) / BW], [0.0, 0.0], BW, FREQ, whole_samples=True)
        assert plan.sample_delays(0).tolist() == [0, num_samp + 3]
        assert not host(plan.fx_rows(x, "SPECTRUM")).any()


def test_aligned_rows_do_not_depend_on_the_passes(torch):
    """FXC_WS_MB small enough that a call goes in several alignment passes, each in several workspace passes (a process of its
    own: the target is read once): the shifts of a pass are written at its first chunk and read by the tables of every
    workspace pass inside it.  Complex64 (one staging buffer) and bytes (two: a chunk per pass)."""
    import os
    import subprocess
    import sys
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r"""
import sys, numpy as np, torch
sys.path.insert(0, %r)
from effex_amd import plan as plan_mod, synth
n_ant, nchan, num_samp, n, bw = 3, 1024, 1024 * 64, 12, 2.4e6
x = torch.from_numpy(synth.synth_iq(41, n, n_ant, num_samp)).cuda()
u8 = torch.from_numpy(np.random.default_rng(2).integers(0, 256, size=(n, n_ant, num_samp, 2), dtype=np.uint8)).cuda()
with plan_mod.FxPlan(n_ant, nchan, 4, num_samp) as plan:
    plan.set_delay_track([5.2 / bw, 10.4 / bw, -7.4 / bw], [0.0, 0.3 / bw, -0.3 / bw], bw, 1.42e9, first_chunk=9, whole_samples=True)
    assert len({tuple(plan.sample_delays(9 + c)) for c in range(n)}) >= 4
    rows = plan.fx_rows(x, "SPECTRUM").cpu().numpy()
    assert plan.track_chunk == 9 + n
    plan.track_seek(9)
    rows8 = plan.fx_rows_u8(u8, "SPECTRUM").cpu().numpy()
    plan.track_seek(9)
    plan.fx_accumulate(x)
    sums = plan.new_sums()
    plan.acc_export(sums)
    np.save(sys.argv[1], rows)
    np.save(sys.argv[2], rows8)
    np.save(sys.argv[3], sums.cpu().numpy())
""" % root
    got = {}
    with tempfile.TemporaryDirectory() as tmp:
        for ws in ("0", "3"):
            env = dict(os.environ, FXC_WS_MB=ws)
            paths = [os.path.join(tmp, "%s_%s.npy" % (k, ws)) for k in ("rows", "rows8", "sums")]
            subprocess.run([sys.executable, "-c", code] + paths, check=True, env=env, timeout=300)
            got[ws] = [np.load(p) for p in paths]
    for a, b in zip(got["0"], got["3"]):
        assert same_bits(a, b)


# -- 6. end to end ----------------------------------------------------------------------------------------------------------
def test_estimate_then_align_recovers_the_amplitude(plan_mod, torch):
    """Device synth_fill with delays (0, 42) at 64 channels: estimate_delays, then set_delays(.., whole_samples=True).  The ratios
    of tests/test_align_host.py hold on the device (aligned >= 0.95, phase-only <= 0.6 of the undelayed source's amplitude)
    and the rows are the oracle's."""
    nchan, num_samp, d = 64, 4096, 42
    xd = torch.empty((1, 2, num_samp), dtype=torch.complex64, device="cuda")
    x0 = torch.empty_like(xd)
    plan_mod.synth_fill(xd, 5, delays=(0, d))
    plan_mod.synth_fill(x0, 5, delays=(0, 0))
    plan, window = make_plan(plan_mod, 2, nchan, num_samp)
    with plan:
        base = abs(host(plan.fx_rows(x0, "SPECTRUM"))[0, 0].astype(np.complex128).mean())
        tau = plan.estimate_delays(xd[0], BW)
        shifts, _ = plan_mod.split_delays(tau, BW)
        assert shifts.tolist() == [0, d]
        plan.set_delays(tau, BW, FREQ)
        phase_only = abs(host(plan.fx_rows(xd, "SPECTRUM"))[0, 0].astype(np.complex128).mean()) / base
        plan.set_delays(tau, BW, FREQ, whole_samples=True)
        assert plan.sample_delays().tolist() == [0, d]
        rows = host(plan.fx_rows(xd, "SPECTRUM"))
        aligned = abs(rows[0, 0].astype(np.complex128).mean()) / base
        print("device: phase-only %.3f aligned %.3f" % (phase_only, aligned))
        assert aligned >= 0.95 and phase_only <= 0.6
        ref = align_ref.rows(align_ref.align(host(xd), shifts), nchan, window, align_ref.tables(nchan, BW, FREQ, tau, shifts))
        assert rel_err(rows, ref) < TOL_VIS
        # set_gains in the same way: unit gains are set_delays' tables and shifts
        plan.set_sample_delays(None)
        plan.set_gains(np.ones((2, nchan), dtype=np.complex128), tau, BW, FREQ, whole_samples=True)
        assert plan.sample_delays().tolist() == [0, d]
        assert rel_err(host(plan.fx_rows(xd, "SPECTRUM")), ref) < TOL_VIS


# -- 7. state rules ---------------------------------------------------------------------------------------------------------
def test_state_rules(plan_mod, torch):
    n_ant, nchan, num_samp = 3, 1024, 1024 * 8
    x = torch.from_numpy(synth.synth_iq(6, 2, n_ant, num_samp)).cuda()
    weights = plan_mod.beam_weights(n_ant, nchan, BW, FREQ)
    tau0, rate = aligned_track_of(n_ant)
    plan, _ = make_plan(plan_mod, n_ant, nchan, num_samp)
    with plan:
        lib, h = plan._lib, plan._h
        beams = host(plan.beamform(x, weights))
        assert lib.fxc_set_sample_delays(None, None) == _lib.FXC_ERR_ARG
        out = np.zeros(n_ant, dtype=np.int64)
        assert lib.fxc_sample_delays(h, 0, None) == _lib.FXC_ERR_ARG and lib.fxc_sample_delays(h, -1, out.ctypes.data) == _lib.FXC_ERR_ARG
        for bad in ([0, num_samp, 0], [0, 0, -num_samp]):
            with pytest.raises(ValueError):          # (FXC_ERR_ARG, as effex_amd/_lib.py maps it)
                plan.set_sample_delays(bad)
        with pytest.raises(ValueError):
            plan.set_sample_delays([1, 2])
        assert not plan.sample_delays().any()
        s = np.array([2, -3, num_samp - 1])
        plan.set_sample_delays(s)
        # independent of the tables: the shifts survive set_rot, set_rot_ant and a plain track
        plan.set_rot(np.ones(nchan, dtype=np.complex128))
        assert np.array_equal(plan.sample_delays(), s)
        plan.set_rot_ant(np.ones((n_ant, nchan), dtype=np.complex128))
        assert np.array_equal(plan.sample_delays(), s)
        plan.set_delay_track(tau0, rate, BW, FREQ)
        assert np.array_equal(plan.sample_delays(5), s)
        # the beamformer refuses, and says why; cleared, it runs again
        with pytest.raises(NotImplementedError) as e:
            plan.beamform(x, weights)
        assert "whole-sample" in str(e.value)
        plan.set_sample_delays(None)
        plan.beamform(x, weights)
        # an aligned track clears static shifts, refuses non-zero ones while it is in force and takes zeros
        plan.set_sample_delays(s)
        plan.set_delay_track(tau0, rate, BW, FREQ, first_chunk=T0, whole_samples=True)
        assert np.array_equal(plan.sample_delays(T0), align_ref.track_shifts(tau0, rate, BW, T0))
        with pytest.raises(_lib.FxcError) as e:
            plan.set_sample_delays(s)
        assert e.value.status == _lib.FXC_ERR_STATE
        plan.set_sample_delays(None)
        plan.set_sample_delays(np.zeros(n_ant, dtype=np.int64))
        with pytest.raises(NotImplementedError):
            plan.beamform(x, weights)
        # its arguments are the plain track's
        for bad in ((np.full(n_ant, np.nan), rate, BW, FREQ, 0), (tau0, rate, 0.0, FREQ, 0), (tau0, rate, BW, np.inf, 0), (tau0, rate, BW, FREQ, -1)):
            with pytest.raises(ValueError):
                plan.set_delay_track(*bad, whole_samples=True)
        assert lib.fxc_set_delay_track_aligned(h, None, None, BW, FREQ, 0) == _lib.FXC_ERR_ARG
        with plan_mod.FxPipeline(plan, 1, depth=2, mode="SPECTRUM"):
            with pytest.raises(_lib.FxcError) as e:
                plan.set_delay_track(tau0, rate, BW, FREQ, whole_samples=True)
            assert e.value.status == _lib.FXC_ERR_STATE
        # whatever ends a track ends it: the static tables, and no shifts are left behind
        plan.set_rot_ant(np.ones((n_ant, nchan), dtype=np.complex128))
        assert not plan.sample_delays(T0).any()
        assert same_bits(plan.beamform(x, weights), beams)


# -- 8. the drop-in ---------------------------------------------------------------------------------------------------------
def test_dropin_whole_samples(tmp_path, torch):
    """Correlator(whole_samples=True) on a source whose second stream is 42 samples late, 64 bins, CONTINUUM: at least 1.6 x the
    magnitude of the run without it (the oracle's ratio is 2.0: tests/test_align_host.py; the margin covers the noise of one
    chunk pair).  The default writes the bytes of a Correlator constructed without the argument."""
    from effex_amd.correlator import ArraySource, Correlator
    num_samp, nbins, n_pairs = 4096, 64, 4
    x = synth.synth_iq(5, n_pairs, 2, num_samp, delays=(0, 42))
    got = {}
    for name, kw in (("absent", {}), ("off", dict(whole_samples=False)), ("on", dict(whole_samples=True))):
        path = str(tmp_path / (name + ".csv"))
        cor = Correlator(num_samp=num_samp, nbins=nbins, source=ArraySource(x), output_file=path, mode='CONTINUUM', **kw)
        assert cor.run_state_machine() >= 2
        assert abs(cor.calibrated_delay * cor.bandwidth - 42) < 0.5
        got[name] = (open(path, "rb").read(), np.abs(np.loadtxt(path, dtype=np.complex128, delimiter=',', skiprows=1)))
    assert got["off"][0] == got["absent"][0]
    ratio = got["on"][1].mean() / got["off"][1].mean()
    print("whole_samples on / off: %.3f (row by row: %s)" % (ratio, got["on"][1] / got["off"][1]))
    assert ratio >= 1.6
