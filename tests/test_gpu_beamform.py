"""The beamformer on the GPU (include/fxcorr.h fxc_beamform, FxPlan.beamform) against the float64 restatement of its definition
(beam_ref.py).  Inputs: seeded standard-normal noise per antenna plus a common source at amplitude 0.5 and random unit-scale
complex weights, so no beam cancels to nothing.  Every case runs on host and on device input and both must give the same bits.
Bounds, the project's two ceilings (tests/tolerances.py): beam power 1e-5 of max P, beam voltage 2e-6 of max |y|;
tools/beam_measure.py --parity writes the observed errors to profiles/beamform/parity.json.  Also: the expansion of the beam power in
the plan's own fx_rows, the delay and gain tracks, workspace batching, the untouched accumulator, the argument errors and the
coherent gain."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import beam_ref
import gains_ref
from effex_amd import _lib
from effex_amd.window import design_window
from tolerances import Bound

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_BEAM_POWER = Bound("TOL_BEAM_POWER", 1e-5)        # of max P: the visibilities' ceiling
TOL_BEAM_VOLTAGE = Bound("TOL_BEAM_VOLTAGE", 2e-6)    # of max |y|: the F-stage spectra's ceiling
BW, FC = 2.4e6, 1.4204e9


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def plan_mod(torch):
    from effex_amd import plan
    return plan


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype in (np.float32, np.complex64) else np.uint64)


def rel_err(got, want):
    return float(np.abs(np.asarray(got) - want).max() / np.abs(want).max())


def both_inputs(plan, torch, x, w, **kw):
    """beamform on host and on device input (numpy weights with the host samples, a CUDA tensor or numpy with the device
    samples); the bits must agree; -> numpy"""
    host = plan.beamform(x, w, **kw)
    assert isinstance(host, np.ndarray)
    dev = plan.beamform(torch.from_numpy(x).cuda(), torch.from_numpy(np.ascontiguousarray(w)).cuda(), **kw)
    assert dev.is_cuda and dev.dtype == (torch.float32 if kw.get("mode", "POWER") == "POWER" else torch.complex64)
    dev = dev.cpu().numpy()
    assert host.shape == dev.shape and host.dtype == dev.dtype
    assert np.array_equal(bits(host), bits(dev)), "host and device input differ"
    return host


# -- shapes -----------------------------------------------------------------------------------------------------------------------
# (n_ant, nchan, ntaps, n_pts, n_chunks, n_beam): the small case; part of a wave and a partial beam tile; a full beam tile; a second
# beam tile and more than 8 antennas (an odd count: the one-antenna tail trip); 64 antennas and 16 beams; the kernel per channel
# count (F only, prebuilt); an odd channel count (the fftshift); the fused F-only route; the ring F route; the pre-filter pass in
# front of the F stage (its buffer and the workspace carve)
SHAPES = [(2, 64, 4, 8, 3, 1), (3, 16, 4, 8, 2, 3), (8, 64, 4, 16, 3, 8), (9, 64, 4, 8, 2, 9), (64, 64, 4, 8, 1, 16),
          (5, 1000, 4, 8, 2, 4), (3, 63, 4, 8, 2, 2), (4, 4096, 4, 8, 2, 2), (2, 8192, 4, 8, 1, 2), (3, 64, 8, 8, 2, 2)]
# ... and more frames than a frame range (h_tools.h::launch_beam: ranges of fpr frames ride in grid.y, beam_kernel walks a range in
# tiles of 8 frames): 37 frames are VOLTAGE ranges of 32 + 5 and ranges of 30 + 7 at 3 or 5 frames a bin, every range's last tile
# partial, the chunk's last bin too (37 = 12 x 3 + 1 = 7 x 5 + 2); 70 frames are 32 + 32 + 6, with two beam tiles (8 + 1) and part of
# a wave; the one-antenna tail trip at an odd channel count with three beams of the tile idle; two beams.  Between them every beam
# tile -- 4, 8 and 1, 8, 2 -- meets a second range and a partial tile (tests/test_beam_host.py restates the ranges, tiles and bins)
# Their window is window_cases.rough_window (beam_ref.py says why)
SHAPES += beam_ref.LONG_SHAPES


shape_case = beam_ref.shape_case


def shape_errors(plan_mod, torch, shape, log=print):
    """-> {"power tint": error of max P, .., "voltage": error of max |y|} of one shape, host and device bits compared"""
    n_ant, nchan, ntaps, n_pts, n_chunks, n_beam = shape
    x, w, window = shape_case(shape)
    y = beam_ref.voltages(beam_ref.spectra(x, nchan, window), w)          # the float64 reference, once per shape
    errs = {}
    with plan_mod.FxPlan(n_ant, nchan, ntaps, nchan * n_pts, window=window) as plan:
        for tint in beam_ref.tints_of(n_pts):
            want = beam_ref.power(y, tint)
            got = both_inputs(plan, torch, x, w, tint=tint)
            assert got.shape == want.shape == (n_chunks, n_beam, -(-n_pts // (tint or n_pts)), nchan) and got.dtype == np.float32
            errs["power %d" % tint] = rel_err(got, want)
        got = both_inputs(plan, torch, x, w, mode="VOLTAGE")
        assert got.shape == y.shape == (n_chunks, n_beam, n_pts, nchan) and got.dtype == np.complex64
        errs["voltage"] = rel_err(got, y)
        if n_beam == 1:      # [n_ant, nchan] weights mean one beam
            assert np.array_equal(bits(plan.beamform(x, w[0], mode="VOLTAGE")), bits(got))
    log(shape, json.dumps(errs))
    return errs


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_beams_match_the_restatement(plan_mod, torch, shape):
    errs = shape_errors(plan_mod, torch, shape)
    for name, err in errs.items():
        assert err < (TOL_BEAM_VOLTAGE if name == "voltage" else TOL_BEAM_POWER), (name, err)


# -- the expansion in the plan's own visibilities -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ant", [2, 3, 8])
def test_power_equals_the_expansion_of_the_plans_own_rows(plan_mod, torch, n_ant):
    """beamform(.., tint=0) against sum_a |w_a|^2 A_a + 2 Re sum_{a<b'} w_a conj(w_b') V_ab' from fx_rows of the same plan (autos,
    no rot), chunk by chunk: 1e-5 of max P"""
    nchan, n_pts, n_chunks, n_beam = 64, 16, 3, 3
    x = beam_ref.noise_and_source(50 + n_ant, n_chunks, n_ant, nchan * n_pts)
    w = beam_ref.random_weights(60 + n_ant, n_beam, n_ant, nchan)
    nb = n_ant * (n_ant - 1) // 2
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * n_pts, autos=True) as plan:
        rows = plan.fx_rows(x).astype(np.complex128)
        want = beam_ref.expansion(w, rows[:, nb:], rows[:, :nb])          # [n_chunks, n_beam, nchan]
        got = both_inputs(plan, torch, x, w, tint=0)[:, :, 0]
    err = rel_err(got, want)
    print(n_ant, "expansion", err)
    assert err < TOL_BEAM_POWER


# -- tracks -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gains", [False, True], ids=["delay track", "delay and gain track"])
def test_tracks_fold_the_chunks_tables_into_the_weights(plan_mod, torch, gains):
    """8 frames, and 37: two frame ranges -- 30 + 7 frames at 3 a bin, 32 + 5 voltages -- under each chunk's effective weights"""
    for n_pts in (8, 37):
        tracks_case(plan_mod, torch, gains, n_pts)


def tracks_case(plan_mod, torch, gains, n_pts):
    n_ant, nchan, n_chunks, n_beam, first = 4, 64, 5, 3, 5
    x = beam_ref.noise_and_source(77, n_chunks, n_ant, nchan * n_pts)
    w = beam_ref.random_weights(78, n_beam, n_ant, nchan)
    window = design_window(4, nchan)
    rng = np.random.default_rng(79)
    tau, rate = rng.uniform(-2e-7, 2e-7, n_ant), rng.uniform(-3e-9, 3e-9, n_ant)
    f = beam_ref.spectra(x, nchan, window)
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * n_pts, window=window) as plan:
        plan.set_delay_track(tau, rate, BW, FC, first_chunk=first)
        if gains:
            plan.set_track_gains(np.stack([gains_ref.draw_gains(n_ant, nchan, rng) for _ in range(2)]), interval=3, first_chunk=first)
        tables = np.stack([plan.track_tables(first + c) for c in range(n_chunks)])
        assert np.abs(tables[0] - tables[-1]).max() > 1e-3                # the tables move
        y = beam_ref.voltages(f, w, tables)
        assert plan.track_chunk == first
        got = plan.beamform(x, w, tint=3)
        assert plan.track_chunk == first + n_chunks
        assert rel_err(got, beam_ref.power(y, 3)) < TOL_BEAM_POWER
        plan.track_seek(first)
        volt = plan.beamform(torch.from_numpy(x).cuda(), w, mode="VOLTAGE").cpu().numpy()      # numpy weights move to the device
        assert plan.track_chunk == first + n_chunks
        assert rel_err(volt, y) < TOL_BEAM_VOLTAGE
        # without the tables the answer is another one: the track is applied
        assert rel_err(volt, beam_ref.voltages(f, w)) > 1e-2
        # two calls of 2 and 3 chunks: the bits of one call of 5, on host and on device input
        for put in (lambda a: a, lambda a: torch.from_numpy(a).cuda()):
            plan.track_seek(first)
            parts = [plan.beamform(put(x[:2]), w, tint=3), plan.beamform(put(x[2:]), w, tint=3)]
            assert plan.track_chunk == first + n_chunks
            parts = np.concatenate([p if isinstance(p, np.ndarray) else p.cpu().numpy() for p in parts])
            assert np.array_equal(bits(parts), bits(got))
        # a failing call leaves the counter where it was
        plan.track_seek(first + 1)
        with pytest.raises(NotImplementedError):
            plan.beamform(x, beam_ref.random_weights(1, 17, n_ant, nchan))
        assert plan.track_chunk == first + 1


# -- workspace batching -----------------------------------------------------------------------------------------------------------
def test_outputs_do_not_depend_on_the_workspace_target(plan_mod, torch):
    """A workspace target of 1 MiB (passes of 15 and 9 chunks; 10, 10 and 4 under a track) and of 3 MiB (FXC_WS_MB is read once per
    process: a child for each setting) against the default: the same bits, host and device input, with and without a track"""
    n_ant, nchan, n_pts, n_chunks, n_beam = 8, 64, 16, 24, 8
    x = beam_ref.noise_and_source(5, n_chunks, n_ant, nchan * n_pts)
    w = beam_ref.random_weights(6, n_beam, n_ant, nchan)
    tau, rate = np.linspace(0.0, 1e-7, n_ant), np.linspace(1e-9, -1e-9, n_ant)
    code = ("import numpy as np, torch, sys; sys.path.insert(0, %r); from effex_amd import plan\n"
            "d = np.load(sys.argv[1]); x, w = d['x'], d['w']; out = {}\n"
            "xd, wd = torch.from_numpy(x).cuda(), torch.from_numpy(w).cuda()\n"
            "with plan.FxPlan(%d, %d, 4, %d) as p:\n"
            "    for track in (0, 1):\n"
            "        if track: p.set_delay_track(d['tau'], d['rate'], %r, %r)\n"
            "        for kind, xx, ww in (('h', x, w), ('d', xd, wd)):\n"
            "            for mode, tint in (('POWER', 0), ('POWER', 3), ('VOLTAGE', 0)):\n"
            "                if track: p.track_seek(2)\n"
            "                v = p.beamform(xx, ww, tint=tint, mode=mode)\n"
            "                out['%%d%%s%%s%%d' %% (track, kind, mode, tint)] = v if kind == 'h' else v.cpu().numpy()\n"
            "np.savez(sys.argv[2], **out)\n" % (ROOT, n_ant, nchan, nchan * n_pts, BW, FC))
    with tempfile.TemporaryDirectory() as tmp:
        np.savez(os.path.join(tmp, "in.npz"), x=x, w=w, tau=tau, rate=rate)
        got = {}
        for label, ws_mb in (("one", "1"), ("three", "3")):
            res = os.path.join(tmp, label + ".npz")
            subprocess.run([sys.executable, "-c", code, os.path.join(tmp, "in.npz"), res], check=True,
                           env=dict(os.environ, FXC_WS_MB=ws_mb), timeout=600)
            got[label] = dict(np.load(res))
    assert len(got["one"]) == len(got["three"]) == 12
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * n_pts) as plan:
        for track in (0, 1):
            if track:
                plan.set_delay_track(tau, rate, BW, FC)
            for mode, tint in (("POWER", 0), ("POWER", 3), ("VOLTAGE", 0)):
                if track:
                    plan.track_seek(2)
                want = plan.beamform(x, w, tint=tint, mode=mode)
                for label in ("one", "three"):
                    for kind in "hd":
                        assert np.array_equal(bits(got[label]["%d%s%s%d" % (track, kind, mode, tint)]), bits(want)), (label, kind, mode, tint)


# -- the accumulator ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ant,nchan,path", [(2, 4096, "fused"), (4, 64, None)])
def test_the_accumulator_is_untouched(plan_mod, torch, n_ant, nchan, path):
    """fx_accumulate, beamform, finalize equals fx_accumulate, finalize bit for bit: the call launches the pending fold (whose rows
    live in the workspace) before it writes the workspace, and adds nothing"""
    n_pts, n_chunks = 8, 6
    x = beam_ref.noise_and_source(31 + n_ant, n_chunks, n_ant, nchan * n_pts)
    w = beam_ref.random_weights(32, 2, n_ant, nchan)
    xd = torch.from_numpy(x).cuda()
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * n_pts, path=path) as plan:
        plan.fx_accumulate(xd)
        want = plan.finalize("SPECTRUM")
        ref = plan.beamform(xd, w).cpu().numpy()
        plan.fx_accumulate(xd)
        got_beam = plan.beamform(xd, w).cpu().numpy()
        got = plan.finalize("SPECTRUM")
        assert np.array_equal(bits(got), bits(want)) and np.abs(want).max() > 0
        assert np.array_equal(bits(got_beam), bits(ref))
        plan.fx_accumulate(x)                                             # host input: the staging path
        assert np.array_equal(bits(plan.beamform(x, w)), bits(ref))
        assert np.array_equal(bits(plan.finalize("SPECTRUM")), bits(want))


# -- argument errors ----------------------------------------------------------------------------------------------------------------
def test_argument_errors(plan_mod, torch):
    n_ant, nchan, n_pts = 3, 16, 8
    x = beam_ref.noise_and_source(1, 2, n_ant, nchan * n_pts)
    w = beam_ref.random_weights(2, 2, n_ant, nchan)
    w17 = beam_ref.random_weights(3, 17, n_ant, nchan)
    out = np.full((2, 2, 1, nchan), -7.0, np.float32)
    H, D, P, V = _lib.FXC_MEM_HOST, _lib.FXC_MEM_DEVICE, _lib.FXC_BEAM_POWER, _lib.FXC_BEAM_VOLTAGE
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * n_pts) as plan:
        call = plan._lib.fxc_beamform
        xp, wp, op = x.ctypes.data, w.ctypes.data, out.ctypes.data
        assert call(None, xp, wp, 2, op, 2, H, P, 0) == _lib.FXC_ERR_ARG
        for args in ((None, wp, 2, op, 2, H, P, 0), (xp, None, 2, op, 2, H, P, 0), (xp, wp, 2, None, 2, H, P, 0),      # NULL
                     (xp, wp, 0, op, 2, H, P, 0), (xp, wp, -1, op, 2, H, P, 0),                                       # n_beam < 1
                     (xp, wp, 2, op, -1, H, P, 0),                                                                    # n_chunks < 0
                     (xp, wp, 2, op, 2, H, 2, 0), (xp, wp, 2, op, 2, H, -1, 0),                                        # mode
                     (xp, wp, 2, op, 2, 3, P, 0), (xp, wp, 2, op, 2, _lib.FXC_MEM_DEVICE_TO_PINNED, P, 0),             # mem_kind
                     (xp, wp, 2, op, 2, H, P, -1), (xp, wp, 2, op, 2, H, P, n_pts + 1), (xp, wp, 2, op, 2, H, V, n_pts + 1)):   # tint
            assert call(plan._h, *args) == _lib.FXC_ERR_ARG, args
        assert call(plan._h, xp, w17.ctypes.data, 17, op, 2, H, P, 0) == _lib.FXC_ERR_UNSUPPORTED
        assert call(plan._h, xp, wp, 2, op, 0, H, P, 0) == _lib.FXC_OK and call(plan._h, None, None, 2, None, 0, D, V, 0) == _lib.FXC_OK
        assert (out == -7.0).all()                                        # nothing was written
        assert call(plan._h, xp, wp, 2, op, 2, H, P, n_pts) == _lib.FXC_OK and (out != -7.0).all()
        # the Python layer
        with pytest.raises(NotImplementedError):
            plan.beamform(x, w17)
        for bad in (dict(tint=-1), dict(tint=n_pts + 1)):
            with pytest.raises(ValueError):
                plan.beamform(x, w, **bad)
        with pytest.raises(KeyError):
            plan.beamform(x, w, mode="INCOHERENT")
        for bad_w in (w[:, :2], w[:, :, :8], w[0, 0], np.zeros((0, n_ant, nchan), np.complex64)):
            with pytest.raises(ValueError):
                plan.beamform(x, bad_w)
        with pytest.raises(ValueError):
            plan.beamform(x, torch.from_numpy(w).cuda())                  # device weights with host samples
        with pytest.raises(ValueError):
            plan.beamform(x[:, :2], w)
        xd = torch.from_numpy(x).cuda()
        good = plan.beamform(x, w, tint=3)
        for bad_out in (np.empty((2, 2, 2, nchan), np.float32), np.empty((2, 2, 3, nchan), np.complex64),
                        np.empty((2, 2, 3, nchan), np.float64), torch.empty((2, 2, 3, nchan), dtype=torch.float32, device="cuda")):
            with pytest.raises(ValueError):
                plan.beamform(x, w, tint=3, out=bad_out)
        for bad_out in (torch.empty((2, 2, 3, nchan + 1), dtype=torch.float32, device="cuda"),
                        torch.empty((2, 2, 3, nchan), dtype=torch.complex64, device="cuda"), np.empty((2, 2, 3, nchan), np.float32)):
            with pytest.raises(ValueError):
                plan.beamform(xd, w, tint=3, out=bad_out)
        with pytest.raises(ValueError):
            plan.beamform(x, w, mode="VOLTAGE", out=np.empty((2, 2, n_pts, nchan), np.float32))
        # a right `out` receives the result
        o = np.empty((2, 2, 3, nchan), np.float32)
        assert plan.beamform(x, w, tint=3, out=o) is o and np.array_equal(bits(o), bits(good))
        od = torch.empty((2, 2, n_pts, nchan), dtype=torch.complex64, device="cuda")
        assert plan.beamform(xd, w, mode="VOLTAGE", out=od) is od
        assert np.array_equal(bits(od.cpu().numpy()), bits(plan.beamform(x, w, mode="VOLTAGE")))


def test_a_pipe_on_a_tracked_plan_is_a_state_error(plan_mod, torch):
    n_ant, nchan, n_pts = 3, 16, 8
    x = beam_ref.noise_and_source(1, 2, n_ant, nchan * n_pts)
    w = beam_ref.random_weights(2, 2, n_ant, nchan)
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * n_pts) as plan:
        want = plan.beamform(x, w)
        plan.set_delay_track(np.zeros(n_ant), np.zeros(n_ant), BW, FC)
        tracked = plan.beamform(x, w)
        assert rel_err(tracked, want.astype(np.float64)) < 1e-6          # a track of zero delays: rho = 1
        with plan_mod.FxPipeline(plan, 2) as pipe:
            with pytest.raises(RuntimeError):
                plan.beamform(x, w)
            assert plan.track_chunk == 2
        assert np.array_equal(bits(plan.beamform(x, w)), bits(tracked))


# -- coherent gain ------------------------------------------------------------------------------------------------------------------
def test_coherent_gain_on_the_device(plan_mod, torch):
    """the on-source beam's source-to-noise ratio against n_ant times the antennas' (beam_ref.gain_deviation), seed 0, within the
    bound the restatement alone set"""
    from test_beam_host import BOUNDS, coherent_gain_deviation
    with open(BOUNDS) as fh:
        rec = json.load(fh)
    nchan = gains_ref.SAMPLE_NCHAN
    with plan_mod.FxPlan(beam_ref.GAIN_ANT, nchan, 4, nchan * gains_ref.SAMPLE_SPECTRA) as plan:
        dev = coherent_gain_deviation(0, lambda part, w: plan.beamform(part.astype(np.complex64), w.astype(np.complex64)).astype(np.float64))
    print("deviation", dev, "restatement", rec["deviation"]["0"], "bound", rec["bound"])
    assert dev <= rec["bound"]
    assert dev == pytest.approx(rec["deviation"]["0"], abs=1e-4)
