"""Delay tracking on the GPU (include/fxcorr.h fxc_set_delay_track): chunk t is phased with the per-antenna tables of
tau_a(t) = tau0[a] + t rate[a].

Oracle of chunk t: two antennas, fx_oracle.pfb_xcorr with calibrated_delay = tau_1(t) - tau_0(t) ... when tau_0 = 0, and for any
antenna count the per-antenna oracle of tests/test_gpu_delays.py (spectrometer_poly(x[c, a]) * rots[a]) with chunk t's tables.
Bounds: TOL_VIS / TOL_CONT of the largest magnitude; the tables have a derived bound of their own (test_track_tables)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fx_oracle
from effex_amd import _lib, synth
from effex_amd.window import design_window

pytestmark = pytest.mark.gpu

from tolerances import TOL_CONT, TOL_VIS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


def track_of(n_ant):
    """distinct delays up to 2e-5 s and distinct rates, antenna 0 included"""
    a = np.arange(n_ant)
    tau0 = 2e-5 * ((3 * a * a) % 17 + 0.25 * a) / 17.0 - 3e-6
    rate = 1e-9 * ((5 * a) % 7 - 2.5)
    return tau0, rate


def oracle(x, nchan, window, tau0, rate, t0, autos=False):
    """x [n_chunks, A, num_samp] -> rows [C, n_rows, nchan] complex128 of chunks t0 .., each with its own tables"""
    n_chunks, n_ant, _ = x.shape
    ntaps = len(window) // nchan
    pairs = [(a, b) for a in range(n_ant) for b in range(a + 1, n_ant)]
    out = np.zeros((n_chunks, len(pairs) + (n_ant if autos else 0), nchan), np.complex128)
    for c in range(n_chunks):
        tau = tau0 + (t0 + c) * rate
        spec = [fx_oracle.spectrometer_poly(x[c, a], ntaps, nchan, window) for a in range(n_ant)]
        rot = [fx_oracle.rot_table(nchan, BW, FREQ, t) for t in tau]
        for p, (a, b) in enumerate(pairs):
            out[c, p] = np.fft.fftshift((spec[a] * rot[a] * np.conj(spec[b] * rot[b])).mean(axis=0))
        if autos:
            for a in range(n_ant):
                out[c, len(pairs) + a] = np.fft.fftshift((np.abs(spec[a]) ** 2).mean(axis=0))
    return out


# -- 1. the tables ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ant,nchan", [(2, 4096), (3, 1000), (12, 256), (2, 1)])
def test_track_tables(plan_mod, torch, n_ant, nchan):
    """track_tables(t) against rot_tables(tau0 + t rate) of numpy.  Both sides round f_k tau once in float64 (numpy rounds
    2 pi f_k first and the product after, the same size of error), so the bound is derived:
    |diff| <= 4 pi |f_k tau| 2^-52 + 8 * 2^-52 per component (8e-11 at 1.42 GHz x 2e-5 s)."""
    tau0, rate = track_of(n_ant)
    tau0, rate = 0.5 * tau0, 2.5e-3 * rate         # |tau0| <= 7.4e-6 s, |rate| x 1e6 chunks <= 1.13e-5 s: within 2e-5 s
    freqs = np.fft.fftfreq(nchan, d=1.0 / BW) + FREQ
    with plan_mod.FxPlan(n_ant, nchan, 4, max(nchan, 16) * 8) as plan:
        plan.set_delay_track(tau0, rate, BW, FREQ)
        for t in (0, 1, 7, 1000, 999999, 1000000):
            got = plan.track_tables(t)
            tau = tau0 + t * rate
            assert np.abs(tau).max() <= 2e-5
            want = plan_mod.rot_tables(nchan, BW, FREQ, tau)
            bound = 4 * np.pi * np.abs(freqs[None, :] * tau[:, None]) * 2.0 ** -52 + 8 * 2.0 ** -52
            worst = max(np.abs(got.real - want.real).max(), np.abs(got.imag - want.imag).max())
            ratio = np.maximum(np.abs(got.real - want.real), np.abs(got.imag - want.imag)) / bound
            a_w, k_w = np.unravel_index(np.argmax(ratio), ratio.shape)
            print("tables n_ant %d nchan %d t %d: worst component error %.3g (bound %.3g); largest error / bound %.3f at antenna %d "
                  "bin %d, tau %.17g" % (n_ant, nchan, t, worst, bound.max(), ratio.max(), a_w, k_w, tau[a_w]))
            assert (np.abs(got.real - want.real) <= bound).all() and (np.abs(got.imag - want.imag) <= bound).all()
        assert plan.track_chunk == 0           # reading tables does not move the counter


# -- 2. rows against the oracle ----------------------------------------------------------------------------------------------
ROUTES = [  # n_ant, nchan, num_samp, n_chunks, path, first_chunk, autos
    (2, 4096, 4096 * 6, 4, "fused", 0, False), (2, 1024, 1024 * 9 + 5, 4, "tiled", 37, False),
    (2, 64, 64 * 20, 5, "tiled", 0, False), (2, 1000, 1000 * 8 + 3, 3, None, 5, False),
    (2, 8192, 8192 * 5, 3, None, 2, False), (2, 1, 4096, 4, None, 11, False),
    (3, 1024, 1024 * 8, 3, None, 0, False), (8, 4096, 4096 * 4, 3, "fused", 1000, False),
    (12, 1024, 1024 * 6, 2, None, 3, False), (3, 1024, 1024 * 8, 3, None, 9, True), (2, 4096, 4096 * 6, 3, "fused", 4, True)]


def make_plan(plan_mod, n_ant, nchan, num_samp, path, autos=False):
    ntaps = 4
    window = design_window(ntaps, nchan)
    return plan_mod.FxPlan(n_ant, nchan, ntaps, num_samp, window=window, path=path, autos=autos), window


@pytest.mark.parametrize("n_ant,nchan,num_samp,n_chunks,path,t0,autos", ROUTES)
def test_tracked_rows_and_integration_match_the_oracle(plan_mod, torch, n_ant, nchan, num_samp, n_chunks, path, t0, autos):
    """Tracked fx_rows (SPECTRUM, CONTINUUM) against the per-chunk oracle; tracked fx_accumulate + finalize, and acc_export +
    finalize_sums, against the float64 mean of the tracked rows (1e-6 of max|vis|) and against the oracle."""
    x_np = synth.synth_iq(21, n_chunks, n_ant, num_samp, delays=np.arange(n_ant) % 5)
    x = torch.from_numpy(x_np).cuda()
    tau0, rate = track_of(n_ant)
    plan, window = make_plan(plan_mod, n_ant, nchan, num_samp, path, autos)
    ref = oracle(x_np, nchan, window, tau0, rate, t0, autos)
    with plan:
        plan.set_delay_track(tau0, rate, BW, FREQ, first_chunk=t0)
        rows = host(plan.fx_rows(x, "SPECTRUM"))
        assert plan.track_chunk == t0 + n_chunks
        assert rows.shape == ref.shape
        assert rel_err(rows, ref) < TOL_VIS
        cont = host(plan.fx_rows(x, "CONTINUUM", BW))
        assert plan.track_chunk == t0 + 2 * n_chunks
        plan.track_seek(t0)
        cont = host(plan.fx_rows(x, "CONTINUUM", BW))
        assert rel_err(cont, ref.mean(axis=-1) / BW) < TOL_CONT
        if n_ant == 2 and not autos:       # the reference's own formula, chunk by chunk (effex.py:516-521)
            plan.set_delay_track(0.0, rate[1], BW, FREQ, first_chunk=t0)
            rows2 = host(plan.fx_rows(x, "SPECTRUM"))
            for c in range(n_chunks):
                want = fx_oracle.pfb_xcorr(x_np[c, 0], x_np[c, 1], 4, nchan, window, BW, FREQ, (t0 + c) * rate[1], "SPECTRUM")
                assert rel_err(rows2[c, 0], want) < TOL_VIS
            plan.set_delay_track(tau0, rate, BW, FREQ, first_chunk=t0)
        # integration
        plan.track_seek(t0)
        plan.fx_accumulate(x)
        assert plan.track_chunk == t0 + n_chunks
        mean_rows = rows.astype(np.complex128).mean(axis=0)
        integ = plan.finalize("SPECTRUM", reset=False)
        err = rel_err(integ, mean_rows)
        print("tracked integration against the mean of the tracked rows: %.3g" % err)
        assert err < 1e-6
        assert rel_err(integ, ref.mean(axis=0)) < TOL_VIS
        integ_c = plan.finalize("CONTINUUM", BW, reset=False)
        assert rel_err(integ_c, ref.mean(axis=0).mean(axis=-1) / BW) < TOL_CONT
        sums = plan.new_sums()
        plan.acc_export(sums)
        plan.acc_reset()
        via = plan.finalize_sums(sums, "SPECTRUM")
        assert rel_err(via, mean_rows) < 1e-6
        if autos:
            assert (np.asarray(integ)[-n_ant:].imag == 0).all()


def test_tracked_rows_from_bytes(plan_mod, torch):
    nchan, num_samp, n_chunks, t0 = 4096, 4096 * 6, 3, 6
    rng = np.random.default_rng(8)
    u8 = rng.integers(0, 256, size=(n_chunks, 2, num_samp, 2), dtype=np.uint8)
    x_np = fx_oracle.u8_to_complex(u8).astype(np.complex64)
    tau0, rate = track_of(2)
    plan, window = make_plan(plan_mod, 2, nchan, num_samp, None)
    ref = oracle(x_np, nchan, window, tau0, rate, t0)
    with plan:
        plan.set_delay_track(tau0, rate, BW, FREQ, first_chunk=t0)
        rows = host(plan.fx_rows_u8(torch.from_numpy(u8).cuda(), "SPECTRUM", remove_dc=False))
        assert plan.track_chunk == t0 + n_chunks
        assert rel_err(rows, ref) < TOL_VIS


def test_headline_sized_tracked_integration(plan_mod, torch):
    """262 144 samples per chunk at 4096 channels, more chunks than the fused kernel has workgroups and not a multiple of them
    (full rounds, then a launch for the rest)."""
    nchan, num_samp, n_chunks, t0 = 4096, 262144, 300, 123456
    x = torch.empty((n_chunks, 2, num_samp), dtype=torch.complex64, device="cuda")
    plan_mod.synth_fill(x, 5)
    tau0, rate = np.array([0.0, 1.1e-6]), np.array([0.0, 2.0e-13])      # (0.085 turns over the run: the mean of the rows stays coherent)
    with plan_mod.FxPlan(2, nchan, 4, num_samp) as plan:
        plan.set_delay_track(tau0, rate, BW, FREQ, first_chunk=t0)
        rows = host(plan.fx_rows(x, "SPECTRUM")).astype(np.complex128)
        assert plan.track_chunk == t0 + n_chunks
        plan.track_seek(t0)
        plan.fx_accumulate(x)
        assert plan.track_chunk == t0 + n_chunks
        integ = plan.finalize("SPECTRUM")
        err = rel_err(integ, rows.mean(axis=0))
        print("headline-sized tracked integration against the mean of its rows: %.3g" % err)
        assert err < 1e-6
        # three chunks of it against the oracle
        xs = host(x[:3])
        window = design_window(4, nchan)
        ref = oracle(xs, nchan, window, tau0, rate, t0)
        assert rel_err(rows[:3], ref) < TOL_VIS


# -- 3. independence of batching, bit for bit ------------------------------------------------------------------------------
# (the 300-chunk case: more chunks than the fused kernel has workgroups; 1024 x 600 frames: a shape whose untracked calls cut a
# chunk into more frame runs the fewer chunks they bring)
BATCHING = [(2, 4096, 4096 * 6, 7, "fused"), (2, 4096, 4096 * 4, 300, "fused"), (2, 1024, 1024 * 9 + 5, 6, "tiled"),
            (2, 1024, 1024 * 600, 4, "tiled"), (2, 1000, 1000 * 8 + 3, 5, None), (2, 1000, 1000 * 400, 4, None),
            (2, 8192, 8192 * 5, 5, None), (2, 64, 64 * 200, 5, "tiled"), (8, 4096, 4096 * 4, 5, "fused"), (3, 1024, 1024 * 8, 5, None)]


@pytest.mark.parametrize("n_ant,nchan,num_samp,n_chunks,path", BATCHING)
def test_rows_do_not_depend_on_batching(plan_mod, torch, n_ant, nchan, num_samp, n_chunks, path):
    """One call, one call per chunk, a split, a pipe: the same bits, and the counter ends at t0 + n."""
    t0 = 50
    x_np = synth.synth_iq(31, n_chunks, n_ant, num_samp)
    x = torch.from_numpy(x_np).cuda()
    tau0, rate = track_of(n_ant)
    plan, _ = make_plan(plan_mod, n_ant, nchan, num_samp, path)
    with plan:
        plan.set_delay_track(tau0, rate, BW, FREQ, first_chunk=t0)
        whole = host(plan.fx_rows(x, "SPECTRUM"))
        assert plan.track_chunk == t0 + n_chunks
        plan.track_seek(t0)
        single = np.concatenate([host(plan.fx_rows(x[c:c + 1], "SPECTRUM")) for c in range(n_chunks)])
        assert plan.track_chunk == t0 + n_chunks
        for cut in (1, n_chunks // 2, n_chunks - 1):
            plan.track_seek(t0)
            split = np.concatenate([host(plan.fx_rows(x[:cut], "SPECTRUM")), host(plan.fx_rows(x[cut:], "SPECTRUM"))])
            print("split at %d against one call: largest difference %.3g of max|vis|" % (cut, rel_err(split, whole)))
            assert np.array_equal(split, whole), cut
        print("one call per chunk against one call: largest difference %.3g of max|vis|" % rel_err(single, whole))
        assert np.array_equal(single, whole)
        plan.track_seek(t0)
        with plan_mod.FxPipeline(plan, 1, depth=2, mode="SPECTRUM") as pipe:
            piped = []
            for c in range(n_chunks):
                pipe.push(x_np[c:c + 1])
                piped.append(pipe.pop())
        assert plan.track_chunk == t0 + n_chunks
        assert np.array_equal(np.concatenate(piped), whole)
        # the accumulator: one call and pieces
        plan.track_seek(t0)
        plan.fx_accumulate(x)
        a = plan.new_sums()
        plan.acc_export(a)
        plan.acc_reset()
        plan.track_seek(t0)
        plan.fx_accumulate(x[:2])
        plan.fx_accumulate(x[2:3])
        plan.fx_accumulate(x[3:])
        assert plan.track_chunk == t0 + n_chunks
        b = plan.new_sums()
        plan.acc_export(b)
        plan.acc_reset()
        assert np.array_equal(host(a), host(b))


def test_rows_do_not_depend_on_the_workspace_passes(torch):
    """FXC_WS_MB small enough for several passes (a process of its own: the target is read once)."""
    code = r"""
import sys, numpy as np, torch
sys.path.insert(0, %r)
from effex_amd import plan as plan_mod, synth
n_ant, nchan, num_samp, n = 3, 1024, 1024 * 64, 12
x = torch.from_numpy(synth.synth_iq(41, n, n_ant, num_samp)).cuda()
with plan_mod.FxPlan(n_ant, nchan, 4, num_samp) as plan:
    plan.set_delay_track([1e-6, 2e-6, -3e-6], [1e-9, -2e-9, 3e-9], 2.4e6, 1.42e9, first_chunk=9)
    rows = plan.fx_rows(x, "SPECTRUM").cpu().numpy()
    assert plan.track_chunk == 9 + n
    plan.track_seek(9)
    plan.fx_accumulate(x)
    sums = plan.new_sums()
    plan.acc_export(sums)
    np.save(sys.argv[1], rows)
    np.save(sys.argv[2], sums.cpu().numpy() if hasattr(sums, "cpu") else np.asarray(sums))
""" % ROOT
    import tempfile
    got = {}
    with tempfile.TemporaryDirectory() as tmp:
        for ws in ("0", "3"):
            env = dict(os.environ, FXC_WS_MB=ws)
            paths = [os.path.join(tmp, "%s_%s.npy" % (k, ws)) for k in ("rows", "sums")]
            subprocess.run([sys.executable, "-c", code] + paths, check=True, env=env, timeout=300)
            got[ws] = [np.load(p) for p in paths]
    assert np.array_equal(got["0"][0], got["3"][0])
    assert np.array_equal(got["0"][1], got["3"][1])


# -- 4. rate zero is the static plan -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ant,nchan,num_samp,n_chunks,path", [(2, 4096, 4096 * 6, 4, "fused"), (3, 1024, 1024 * 8, 3, None)])
def test_rate_zero_is_the_static_plan(plan_mod, torch, n_ant, nchan, num_samp, n_chunks, path):
    x_np = synth.synth_iq(51, n_chunks, n_ant, num_samp)
    x = torch.from_numpy(x_np).cuda()
    tau0, _ = track_of(n_ant)
    plan, window = make_plan(plan_mod, n_ant, nchan, num_samp, path)
    ref = oracle(x_np, nchan, window, tau0, np.zeros(n_ant), 0)
    with plan:
        plan.set_delays(tau0, BW, FREQ)
        rows_s = host(plan.fx_rows(x, "SPECTRUM"))
        plan.fx_accumulate(x)
        int_s = plan.finalize("SPECTRUM")
        plan.set_delay_track(tau0, np.zeros(n_ant), BW, FREQ, first_chunk=77)
        rows_t = host(plan.fx_rows(x, "SPECTRUM"))
        plan.fx_accumulate(x)
        int_t = plan.finalize("SPECTRUM")
    for got in (rows_s, rows_t):
        assert rel_err(got, ref) < TOL_VIS
    for got in (int_s, int_t):
        assert rel_err(got, ref.mean(axis=0)) < TOL_VIS
    print("rate 0 against the static plan: rows %.3g, integration %.3g of max|vis|" % (rel_err(rows_t, rows_s), rel_err(int_t, int_s)))
    assert rel_err(rows_t, rows_s) < TOL_VIS and rel_err(int_t, int_s) < TOL_VIS


# -- 5. two ranks on one GPU -------------------------------------------------------------------------------------------------
def test_two_ranks_with_seek_add_up_to_the_single_plan(plan_mod, torch):
    n_ant, nchan, num_samp, n_chunks = 3, 1024, 1024 * 8, 6
    x = torch.from_numpy(synth.synth_iq(61, n_chunks, n_ant, num_samp)).cuda()
    tau0, rate = track_of(n_ant)
    sums = []
    for lo, hi in ((0, n_chunks), (0, 2), (2, n_chunks)):
        plan, _ = make_plan(plan_mod, n_ant, nchan, num_samp, None)
        with plan:
            plan.set_delay_track(tau0, rate, BW, FREQ)
            plan.track_seek(lo)
            plan.fx_accumulate(x[lo:hi])
            s = plan.new_sums()
            plan.acc_export(s)
            sums.append(host(s).copy())
    plan, _ = make_plan(plan_mod, n_ant, nchan, num_samp, None)
    with plan:
        plan.set_delay_track(tau0, rate, BW, FREQ)
        single = plan.finalize_sums(torch.from_numpy(sums[0]).cuda(), "SPECTRUM")
        both = plan.finalize_sums(torch.from_numpy(sums[1] + sums[2]).cuda(), "SPECTRUM")
    assert rel_err(both, single) < 1e-12


# -- 6. it stops fringes -----------------------------------------------------------------------------------------------------
def test_tracking_stops_fringes(plan_mod, torch):
    """The inter-antenna delay grows by one sample per chunk; frequency 0, bandwidth 1, so one sample is a delay of 1.  The
    static table of chunk 0 lets the noise part of the synthetic sky average exp(i theta d) over the band and d = 0 .. 15;
    the track follows it.  Oracle ratio tracked / static, computed here on the CPU first: it must be above 4 (the synthetic
    tone does not decorrelate, so it is far from 16)."""
    nchan, num_samp, n_chunks = 1024, 1024 * 32, 16
    x_np = np.concatenate([synth.synth_iq(71, 1, 2, num_samp, first_chunk=c, delays=(0, c)) for c in range(n_chunks)])
    window = design_window(4, nchan)

    def oracle_cont(rate):
        return np.mean([fx_oracle.pfb_xcorr(x_np[c, 0], x_np[c, 1], 4, nchan, window, 1.0, 0.0, c * rate, "CONTINUUM")
                        for c in range(n_chunks)])
    want_static, want_track = oracle_cont(0.0), oracle_cont(1.0)
    ratio = abs(want_track) / abs(want_static)
    print("fringe stopping, oracle: |tracked| / |static| = %.3g" % ratio)
    assert ratio > 4
    x = torch.from_numpy(x_np).cuda()
    with plan_mod.FxPlan(2, nchan, 4, num_samp, window=window) as plan:
        plan.set_delay(1.0, 0.0, 0.0)
        plan.fx_accumulate(x)
        got_static = plan.finalize("CONTINUUM", 1.0)[0]
        plan.set_delay_track(0.0, 1.0, 1.0, 0.0)
        plan.fx_accumulate(x)
        got_track = plan.finalize("CONTINUUM", 1.0)[0]
    scale = abs(want_track)
    assert abs(got_track - want_track) / scale < TOL_CONT
    assert abs(got_static - want_static) / scale < TOL_CONT
    assert abs(got_track) > 2 * abs(got_static)


# -- 7. state rules ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ant,nchan,num_samp", [(2, 4096, 4096 * 6), (3, 1024, 1024 * 8)])
def test_state_rules(plan_mod, torch, n_ant, nchan, num_samp):
    x = torch.from_numpy(synth.synth_iq(81, 3, n_ant, num_samp)).cuda()
    tau0, rate = track_of(n_ant)
    static = plan_mod.rot_tables(nchan, BW, FREQ, tau0)
    plain, _ = make_plan(plan_mod, n_ant, nchan, num_samp, None)
    with plain:
        plain.set_rot_ant(static)
        want_ant = host(plain.fx_rows(x, "SPECTRUM"))
        plain.set_rot(static[1])
        want_rot = host(plain.fx_rows(x, "SPECTRUM"))
    plan, _ = make_plan(plan_mod, n_ant, nchan, num_samp, None)
    with plan:
        with pytest.raises(_lib.FxcError) as e:
            plan.track_chunk
        assert e.value.status == _lib.FXC_ERR_STATE
        with pytest.raises(_lib.FxcError):
            plan.track_seek(3)
        with pytest.raises(_lib.FxcError):
            plan.track_tables(0)
        plan.set_delay_track(tau0, rate, BW, FREQ)
        plan.fx_rows(x, "SPECTRUM")
        plan.set_rot_ant(static)                       # ends the track
        with pytest.raises(_lib.FxcError):
            plan.track_chunk
        assert np.array_equal(host(plan.fx_rows(x, "SPECTRUM")), want_ant)
        plan.set_delay_track(tau0, rate, BW, FREQ)
        plan.set_rot(static[1])
        assert np.array_equal(host(plan.fx_rows(x, "SPECTRUM")), want_rot)
        # tracked and untracked chunks do not mix in one integration
        plan.fx_accumulate(x)
        with pytest.raises(_lib.FxcError) as e:
            plan.set_delay_track(tau0, rate, BW, FREQ)
        assert e.value.status == _lib.FXC_ERR_STATE
        plan.acc_reset()
        plan.set_delay_track(tau0, rate, BW, FREQ)
        plan.fx_accumulate(x)
        for setter, arg in ((plan.set_rot, static[1]), (plan.set_rot_ant, static)):
            with pytest.raises(_lib.FxcError) as e:
                setter(arg)
            assert e.value.status == _lib.FXC_ERR_STATE
        plan.set_delay_track(tau0, rate, BW, FREQ, first_chunk=3)      # a new ephemeris inside a tracked integration is fine
        plan.finalize("SPECTRUM")                                     # (resets)
        plan.set_rot(static[1])
        # argument checks
        for bad in ((np.full(n_ant, np.nan), rate, BW, FREQ, 0), (tau0, rate, 0.0, FREQ, 0), (tau0, rate, BW, np.inf, 0),
                    (tau0, rate, BW, FREQ, -1)):
            with pytest.raises(ValueError):          # (FXC_ERR_ARG, as effex_amd/_lib.py maps it)
                plan.set_delay_track(*bad)
        # an open pipe
        with plan_mod.FxPipeline(plan, 1, depth=2, mode="SPECTRUM"):
            with pytest.raises(_lib.FxcError) as e:
                plan.set_delay_track(tau0, rate, BW, FREQ)
            assert e.value.status == _lib.FXC_ERR_STATE


# -- 8. the drop-in ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pairs", [9, 8])
def test_dropin_test_mode_device_sweep(tmp_path, torch, n_pairs):
    """mode='TEST' with batch=4 and device_sweep=True writes the rows batch=1 writes and leaves the same calibrated_delay;
    9 pairs: calibration + 2 full batches, 8: the stream ends inside a batch."""
    from effex_amd.correlator import ArraySource, Correlator
    num_samp, nbins = 4096 * 6, 4096
    x = synth.synth_iq(91, n_pairs, 2, num_samp)
    got = {}
    for name, kw in (("pairwise", dict(batch=1)), ("sweep", dict(batch=4, device_sweep=True))):
        path = str(tmp_path / (name + ".csv"))
        cor = Correlator(num_samp=num_samp, nbins=nbins, source=ArraySource(x), output_file=path, mode='TEST', **kw)
        assert cor.run_state_machine() == n_pairs - 1
        got[name] = (np.loadtxt(path, dtype=np.complex128, delimiter=',', skiprows=1), cor.calibrated_delay)
    assert got["sweep"][0].shape == got["pairwise"][0].shape == (n_pairs - 1,)
    assert rel_err(got["sweep"][0], got["pairwise"][0]) < TOL_CONT
    assert got["sweep"][1] == got["pairwise"][1]
