"""Antenna masks, incoherent beams and aligned passes of the beamformer on the GPU (include/fxcorr.h fxc_beamform_ex,
fxc_kurtosis_antenna_mask; FxPlan.beamform(mask=, mask_tint=, whole_samples=), FxPlan.beamform_incoherent, FxPlan.kurtosis_mask)
against the float64 restatement (beam_mask_ref.py) and against the unmasked beamformer's own bits.  Bounds, the project's two
ceilings as tests/test_gpu_beamform.py has them: beam power and incoherent power 1e-5 of max P, beam voltage 2e-6 of max |y|;
tools/beam_mask_measure.py --parity writes the observed errors to profiles/beam_mask/parity.json.  The interference scenario's
level and bound are the restatement's (tests/golden/beam_mask_bounds.json).

Observed on an MI355X (profiles/beam_mask/parity.json), the worst over the seven shapes: power 8.7e-7 and incoherent power 7.9e-7 of
max P, voltage 4.7e-7 of max |y|; the scenario at seed 0: factor 15.1, deviation 0.0175 under the bound 0.097."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import align_ref
import beam_mask_ref as r
import beam_ref
import gains_ref
from effex_amd import _lib
from effex_amd.window import design_window
from tolerances import Bound

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_BEAM_POWER = Bound("TOL_BEAM_POWER", 1e-5)        # of max P: tests/test_gpu_beamform.py's ceiling
TOL_BEAM_VOLTAGE = Bound("TOL_BEAM_VOLTAGE", 2e-6)    # of max |y|
BW, FC = 2.4e6, 1.4204e9

# (n_ant, nchan, ntaps, n_pts, n_chunks, n_beam): the small case; part of a wave and an odd antenna count (the one-antenna trip); the
# full tile; a second tile and an odd count above 8; an odd channel count (the fftshift's wrap inside the mask's index), ranges of
# 32 + 5 frames and a rough window; 70 frames and two tiles; the kernel per channel count; the two-beam tile with the one-antenna
# tail trip; tiles of 8 + 2 beams over a second frame range, partial tiles and a partial last bin
SHAPES = [(2, 64, 4, 8, 3, 1), (3, 16, 4, 8, 2, 3), (8, 64, 4, 16, 3, 8), (9, 64, 4, 8, 2, 9), (3, 63, 4, 37, 2, 5), (2, 16, 4, 70, 2, 9),
          (5, 1000, 4, 8, 2, 4), (3, 16, 4, 8, 2, 2), (2, 16, 4, 37, 1, 10)]
ROUGH = {(3, 63, 4, 37, 2, 5), (2, 16, 4, 70, 2, 9)}
ids = lambda s: "x".join(map(str, s))      # noqa: E731


def mask_tints_of(n_pts):
    """the whole chunk, single frames, bins inside a tile of 8 frames (2, 5: tiles that straddle bins), the tile itself, 33 and
    n_pts - 1 (one full bin and a bin of one frame)"""
    return sorted({0, n_pts - 1} | {t for t in (1, 2, 5, 8, 33) if t <= n_pts})


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


def host(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def shape_case(shape):
    import window_cases
    n_ant, nchan, ntaps, n_pts, n_chunks, n_beam = shape
    x = beam_ref.noise_and_source(1000 * n_ant + nchan + n_beam, n_chunks, n_ant, nchan * n_pts)
    w = beam_ref.random_weights(17 * n_ant + n_beam, n_beam, n_ant, nchan)
    window = window_cases.rough_window(ntaps, nchan) if tuple(shape) in ROUGH else design_window(ntaps, nchan)
    return x, w, window


def run(plan, mode, x, w, **kw):
    return plan.beamform_incoherent(x, w, **kw) if mode == "INCOHERENT" else plan.beamform(x, w, mode=mode, **kw)


def both_inputs(plan, torch, mode, x, w, mask=None, **kw):
    """host and device input (a CUDA mask, or a numpy mask that is moved); the bits must agree; -> numpy"""
    got = run(plan, mode, x, w, mask=mask, **kw)
    assert isinstance(got, np.ndarray)
    dmask = None if mask is None else (torch.from_numpy(mask).cuda() if kw.get("tint", 0) % 2 == 0 else mask)
    dev = run(plan, mode, torch.from_numpy(x).cuda(), torch.from_numpy(np.ascontiguousarray(w)).cuda(), mask=dmask, **kw)
    assert dev.is_cuda
    dev = dev.cpu().numpy()
    assert got.shape == dev.shape and got.dtype == dev.dtype
    assert np.array_equal(bits(got), bits(dev)), "host and device input differ"
    return got


# -- 1: a mask of ones, and no mask, are the unmasked beamformer bit for bit ------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_all_ones_and_no_mask_are_the_unmasked_bits(plan_mod, torch, shape):
    n_ant, nchan, ntaps, n_pts, n_chunks, n_beam = shape
    x, w, window = shape_case(shape)
    xd, wd = torch.from_numpy(x).cuda(), torch.from_numpy(w).cuda()
    with plan_mod.FxPlan(n_ant, nchan, ntaps, nchan * n_pts, window=window) as plan:
        want = {("VOLTAGE", 0): plan.beamform(x, w, mode="VOLTAGE")}
        for tint in beam_ref.tints_of(n_pts):
            want["POWER", tint] = plan.beamform(x, w, tint=tint)
        for (mode, tint), ref in want.items():
            bw = bits(ref)
            # no mask, through fxc_beamform_ex (whole_samples on a plan without shifts: no alignment, no other bit)
            assert np.array_equal(bits(plan.beamform(x, w, tint=tint, mode=mode, whole_samples=True)), bw), (mode, tint)
            out = np.empty_like(ref)
            rc = plan._lib.fxc_beamform_ex(plan._h, x.ctypes.data, w.ctypes.data, n_beam, None, 0, out.ctypes.data, n_chunks, _lib.FXC_MEM_HOST,
                                           plan_mod.BEAM_MODES[mode], tint, 0)
            assert rc == _lib.FXC_OK and np.array_equal(bits(out), bw), (mode, tint)
        for mt in mask_tints_of(n_pts):
            ones = np.ones((n_chunks, n_ant, r.n_mbin(n_pts, mt), nchan), np.float32)
            ones[0, 0, 0, 0], ones[-1, -1, -1, -1] = 0.25, np.inf          # > 0 counts, whatever the value
            od = torch.from_numpy(ones).cuda()
            for (mode, tint), ref in want.items():
                bw = bits(ref)
                assert np.array_equal(bits(plan.beamform(x, w, tint=tint, mode=mode, mask=ones, mask_tint=mt)), bw), (mode, tint, mt)
                assert np.array_equal(bits(host(plan.beamform(xd, wd, tint=tint, mode=mode, mask=od, mask_tint=mt))), bw), (mode, tint, mt)


# -- 2: a random mask against the restatement ---------------------------------------------------------------------------------------
def shape_errors(plan_mod, torch, shape, log=print):
    """-> {"power <mask_tint> <tint>": error of max P, "incoherent ..": the same, "voltage <mask_tint>": error of max |y|} of one
    shape under beam_mask_ref.random_mask; host and device bits compared, the cell with every antenna out exactly 0"""
    n_ant, nchan, ntaps, n_pts, n_chunks, n_beam = shape
    x, w, window = shape_case(shape)
    f = beam_ref.spectra(x, nchan, window)                               # the float64 reference, once per shape
    errs = {}
    with plan_mod.FxPlan(n_ant, nchan, ntaps, nchan * n_pts, window=window) as plan:
        for mt in mask_tints_of(n_pts):
            mask = r.random_mask(100 + mt, n_chunks, n_ant, n_pts, nchan, mt)
            none = r.special_cells(n_chunks, mask.shape[2], nchan)["none"]
            span = mt or n_pts
            i0, i1 = none[1] * span, min((none[1] + 1) * span, n_pts)                     # the frames of the empty cell
            k_nat = (none[2] - nchan // 2) % nchan
            y = r.voltages(f, w, mask, mt)
            got = both_inputs(plan, torch, "VOLTAGE", x, w, mask, mask_tint=mt)
            assert got.shape == y.shape and got.dtype == np.complex64
            assert not got[none[0], :, i0:i1, k_nat].any() and not y[none[0], :, i0:i1, k_nat].any()
            errs["voltage %d" % mt] = rel_err(got, y)
            for tint in beam_ref.tints_of(n_pts):
                for mode, want in (("POWER", beam_ref.power(y, tint)), ("INCOHERENT", r.incoherent(f, w, tint, mask, mt))):
                    got = both_inputs(plan, torch, mode, x, w, mask, mask_tint=mt, tint=tint)
                    assert got.shape == want.shape and got.dtype == np.float32
                    assert np.array_equal(got == 0, want == 0), (mode, mt, tint)           # the empty cells, and only they, exactly 0
                    errs["%s %d %d" % (mode.lower(), mt, tint)] = rel_err(got, want)
                    if tint == mt:                                                         # a time bin that is the empty cell
                        assert not got[none[0], :, none[1], none[2]].any(), (mode, mt)
        # the incoherent beams without a mask
        got = both_inputs(plan, torch, "INCOHERENT", x, w, tint=3)
        errs["incoherent none 3"] = rel_err(got, r.incoherent(f, w, 3))
    log(shape, json.dumps({k: errs[k] for k in sorted(errs, key=errs.get)[-3:]}))
    return errs


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_random_mask_matches_the_restatement(plan_mod, torch, shape):
    for name, err in shape_errors(plan_mod, torch, shape).items():
        assert err < (TOL_BEAM_VOLTAGE if name.startswith("voltage") else TOL_BEAM_POWER), (name, err)


# -- 3: one antenna out everywhere --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 16, 4, 8, 2, 3), (9, 64, 4, 8, 2, 9), (3, 63, 4, 37, 2, 5)], ids=ids)
def test_one_antenna_out_is_its_weights_zeroed_and_its_samples_never_read(plan_mod, torch, shape):
    n_ant, nchan, ntaps, n_pts, n_chunks, n_beam = shape
    x, w, window = shape_case(shape)
    out_ant = n_ant - 1                                                  # an odd count: the antenna of the one-antenna trip
    w0 = w.copy()
    w0[:, out_ant] = 0
    bad = x.copy()
    bad[0, out_ant, 5] = np.nan
    bad[0, out_ant, nchan * n_pts // 2] = np.inf
    bad[1, out_ant, :] = complex(np.nan, -np.inf)
    bad[1, out_ant, 3::7] = 1e30                                         # a tone of sorts
    with plan_mod.FxPlan(n_ant, nchan, ntaps, nchan * n_pts, window=window) as plan:
        for mt in (0, 5, 8):
            if mt > n_pts:
                continue
            mask = np.ones((n_chunks, n_ant, r.n_mbin(n_pts, mt), nchan), np.float32)
            mask[:, out_ant] = 0.0
            for mode, tint in (("POWER", 0), ("POWER", 3), ("VOLTAGE", 0), ("INCOHERENT", 0), ("INCOHERENT", 3)):
                want = run(plan, mode, x, w0, tint=tint)
                got = both_inputs(plan, torch, mode, x, w, mask, mask_tint=mt, tint=tint)
                assert np.array_equal(got, want), (mode, tint, mt)       # numerically: a sum may end in -0 where the other has +0
                assert np.abs(got).max() > 0
                poisoned = both_inputs(plan, torch, mode, bad, w, mask, mask_tint=mt, tint=tint)
                assert np.array_equal(bits(poisoned), bits(got)), (mode, tint, mt)
                assert not np.isfinite(run(plan, mode, bad, w, tint=tint)).all()           # unmasked, the samples do reach the beam


# -- 4: an incoherent beam of one antenna is that antenna's power -------------------------------------------------------------------
def test_incoherent_beam_of_one_antenna_is_the_kurtosis_calls_power(plan_mod, torch):
    n_ant, nchan, n_pts, n_chunks = 3, 64, 37, 2
    x = beam_ref.noise_and_source(9, n_chunks, n_ant, nchan * n_pts)
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * n_pts) as plan:
        for a in range(n_ant):
            w = np.zeros((1, n_ant, nchan), np.complex64)
            w[0, a] = 1.0
            for tint in (0, 3, 5, 36):
                _, power = plan.kurtosis(x, tint=tint, return_power=True)
                got = plan.beamform_incoherent(x, w, tint=tint)
                assert got.shape == (n_chunks, 1, power.shape[2], nchan)
                assert rel_err(got[:, 0], power[:, a].astype(np.float64)) < TOL_BEAM_POWER


# -- 5: workspace batching ----------------------------------------------------------------------------------------------------------
def test_outputs_do_not_depend_on_the_workspace_target(plan_mod, torch):
    """A workspace target of 1 MiB (FXC_WS_MB is read once per process: a child) on a plan with static shifts, whole_samples=True:
    192 KiB of spectra and 192 KiB of aligned samples a chunk, so 5 chunks go in passes of 2, 2 and 1 -- under a mask (staged pass by
    pass from host memory), host and device input, the three modes: the bits of the default target"""
    n_ant, nchan, n_pts, n_chunks, n_beam, mt = 4, 64, 96, 5, 3, 5
    x = beam_ref.noise_and_source(5, n_chunks, n_ant, nchan * n_pts)
    w = beam_ref.random_weights(6, n_beam, n_ant, nchan)
    mask = r.random_mask(7, n_chunks, n_ant, n_pts, nchan, mt)
    shifts = np.array([0, 3, -2, 8])
    code = ("import numpy as np, torch, sys; sys.path.insert(0, %r); from effex_amd import plan\n"
            "d = np.load(sys.argv[1]); x, w, m = d['x'], d['w'], d['m']; out = {}\n"
            "xd, wd, md = torch.from_numpy(x).cuda(), torch.from_numpy(w).cuda(), torch.from_numpy(m).cuda()\n"
            "with plan.FxPlan(%d, %d, 4, %d) as p:\n"
            "    p.set_sample_delays(d['s'])\n"
            "    for kind, xx, ww, mm in (('h', x, w, m), ('d', xd, wd, md)):\n"
            "        for mode in ('POWER', 'VOLTAGE', 'INCOHERENT'):\n"
            "            kw = dict(tint=3, mask=mm, mask_tint=%d, whole_samples=True)\n"
            "            v = p.beamform_incoherent(xx, ww, **kw) if mode == 'INCOHERENT' else p.beamform(xx, ww, mode=mode, **kw)\n"
            "            out[kind + mode] = v if kind == 'h' else v.cpu().numpy()\n"
            "np.savez(sys.argv[2], **out)\n" % (ROOT, n_ant, nchan, nchan * n_pts, mt))
    with tempfile.TemporaryDirectory() as tmp:
        np.savez(os.path.join(tmp, "in.npz"), x=x, w=w, m=mask, s=shifts)
        res = os.path.join(tmp, "one.npz")
        subprocess.run([sys.executable, "-c", code, os.path.join(tmp, "in.npz"), res], check=True, env=dict(os.environ, FXC_WS_MB="1"),
                       timeout=600)
        got = dict(np.load(res))
    assert len(got) == 6
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * n_pts) as plan:
        plan.set_sample_delays(shifts)
        for mode in ("POWER", "VOLTAGE", "INCOHERENT"):
            want = run(plan, mode, x, w, tint=3, mask=mask, mask_tint=mt, whole_samples=True)
            assert np.abs(want).max() > 0
            for kind in "hd":
                assert np.array_equal(bits(got[kind + mode]), bits(want)), (kind, mode)


# -- 6: tracks ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gains", [False, True], ids=["delay track", "delay and gain track"])
def test_tracks_under_a_mask(plan_mod, torch, gains):
    n_ant, nchan, n_pts, n_chunks, n_beam, first, mt = 4, 64, 37, 5, 3, 5, 5
    x = beam_ref.noise_and_source(77, n_chunks, n_ant, nchan * n_pts)
    w = beam_ref.random_weights(78, n_beam, n_ant, nchan)
    mask = r.random_mask(80, n_chunks, n_ant, n_pts, nchan, mt)
    window = design_window(4, nchan)
    rng = np.random.default_rng(79)
    tau, rate = rng.uniform(-2e-7, 2e-7, n_ant), rng.uniform(-3e-9, 3e-9, n_ant)
    f = beam_ref.spectra(x, nchan, window)
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * n_pts, window=window) as plan:
        plain_inc = plan.beamform_incoherent(x, w, tint=3, mask=mask, mask_tint=mt)
        plan.set_delay_track(tau, rate, BW, FC, first_chunk=first)
        if gains:
            plan.set_track_gains(np.stack([gains_ref.draw_gains(n_ant, nchan, rng) for _ in range(2)]), interval=3, first_chunk=first)
        tables = np.stack([plan.track_tables(first + c) for c in range(n_chunks)])
        assert np.abs(tables[0] - tables[-1]).max() > 1e-3               # the tables move
        for mode, want, tol in (("POWER", r.power(f, w, 3, mask, mt, tables), TOL_BEAM_POWER),
                                ("INCOHERENT", r.incoherent(f, w, 3, mask, mt, tables), TOL_BEAM_POWER),
                                ("VOLTAGE", r.voltages(f, w, mask, mt, tables), TOL_BEAM_VOLTAGE)):
            plan.track_seek(first)
            got = run(plan, mode, x, w, mask=mask, mask_tint=mt, tint=3)
            assert plan.track_chunk == first + n_chunks
            plan.track_seek(first)
            dev = run(plan, mode, torch.from_numpy(x).cuda(), w, mask=mask, mask_tint=mt, tint=3)      # numpy weights and mask move
            assert plan.track_chunk == first + n_chunks and np.array_equal(bits(host(dev)), bits(got))
            assert rel_err(got, want) < tol, mode
            if mode == "INCOHERENT":
                # a plain delay track (|rho| = 1) changes nothing but the roundings of w rho; a gain track scales the antennas
                assert (rel_err(got, plain_inc.astype(np.float64)) < 1e-5) == (not gains)
        # a failing call puts the counter back
        plan.track_seek(first + 1)
        with pytest.raises(ValueError):
            plan.beamform(x, w, mask=mask[:, :, :1], mask_tint=n_pts + 1)
        bad = np.ones((n_chunks, n_ant, 1, nchan), np.float32)
        out = np.empty((n_chunks, n_beam, 1, nchan), np.float32)
        assert plan._lib.fxc_beamform_ex(plan._h, x.ctypes.data, w.ctypes.data, n_beam, bad.ctypes.data, n_pts + 1, out.ctypes.data, n_chunks,
                                         _lib.FXC_MEM_HOST, _lib.FXC_BEAM_POWER, 0, 0) == _lib.FXC_ERR_ARG
        assert plan.track_chunk == first + 1


# -- 7: aligned passes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shifts", [(0, 3, -2), (4, -7, 1), (-1, 0, 64 + 5)], ids=str)
def test_whole_samples_on_static_shifts_equals_a_plain_plan_on_aligned_samples(plan_mod, torch, shifts):
    n_ant, nchan, n_pts, n_chunks, n_beam, mt = 3, 64, 37, 3, 3, 5
    x = beam_ref.noise_and_source(21, n_chunks, n_ant, nchan * n_pts)
    w = beam_ref.random_weights(22, n_beam, n_ant, nchan)
    mask = r.random_mask(23, n_chunks, n_ant, n_pts, nchan, mt)
    xa = align_ref.align(x, shifts)
    assert np.abs(xa - x).max() > 0
    cases = [("POWER", 3, None), ("POWER", 0, mask), ("VOLTAGE", 0, None), ("VOLTAGE", 0, mask), ("INCOHERENT", 3, mask)]
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * n_pts) as fresh, plan_mod.FxPlan(n_ant, nchan, 4, nchan * n_pts) as plan:
        plan.set_sample_delays(shifts)
        for mode, tint, m in cases:
            kw = dict(tint=tint, mask=m, mask_tint=mt if m is not None else 0)
            want = run(fresh, mode, xa, w, **kw)
            got = both_inputs(plan, torch, mode, x, w, whole_samples=True, **kw)
            assert np.array_equal(bits(got), bits(want)), (mode, tint)
            # on the plan without shifts whole_samples changes no bit
            assert np.array_equal(bits(run(fresh, mode, xa, w, whole_samples=True, **kw)), bits(want))
            with pytest.raises(NotImplementedError, match="whole-sample"):
                run(plan, mode, x, w, whole_samples=False, **kw)
        plan.set_sample_delays(None)
        assert np.array_equal(bits(plan.beamform(xa, w, tint=3)), bits(fresh.beamform(xa, w, tint=3)))


def test_whole_samples_under_an_aligned_track(plan_mod, torch):
    """set_delay_track(.., whole_samples=True): the shifts step inside the call.  Chunk by chunk the bits are those of a plan without
    shifts or track fed align_ref.align(x, shifts of the chunk) under the weights w rho -- rho the chunk's aligned table, rounded
    once to complex64, the product in float32 with every operation rounded on its own, as fxcorr.h defines weff; the shifts are
    align_ref.track_shifts', the tables align_ref.tables' (the bound of tests/test_gpu_align.py); and the float64 restatement holds"""
    n_ant, nchan, n_pts, n_chunks, n_beam, t0, mt = 3, 64, 37, 4, 3, 37, 8
    x = beam_ref.noise_and_source(31, n_chunks, n_ant, nchan * n_pts)
    w = beam_ref.random_weights(32, n_beam, n_ant, nchan)
    mask = r.random_mask(33, n_chunks, n_ant, n_pts, nchan, mt)
    window = design_window(4, nchan)
    slope = np.array([0.0, 0.3, -0.3]) / BW
    tau0 = np.array([5.2, 10.4, -7.4]) / BW - t0 * slope
    shifts = np.stack([align_ref.track_shifts(tau0, slope, BW, t0 + c) for c in range(n_chunks)])
    assert (np.diff(shifts, axis=0) != 0).any() and shifts.any(axis=0).all()
    tabs = np.stack([align_ref.tables(nchan, BW, FC, tau0 + float(t0 + c) * slope, shifts[c]) for c in range(n_chunks)])
    xa = align_ref.align(x, shifts)
    f = beam_ref.spectra(xa, nchan, window)
    freqs = np.fft.fftfreq(nchan, d=1.0 / BW) + FC
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * n_pts, window=window) as fresh, \
            plan_mod.FxPlan(n_ant, nchan, 4, nchan * n_pts, window=window) as plan:
        plan.set_delay_track(tau0, slope, BW, FC, first_chunk=t0, whole_samples=True)
        weff = []
        for c in range(n_chunks):
            assert np.array_equal(plan.sample_delays(t0 + c), shifts[c])
            rho = plan.track_tables(t0 + c)
            tau = tau0 + float(t0 + c) * slope
            bound = 4 * np.pi * np.abs(freqs[None, :] * tau[:, None]) * 2.0 ** -52 + 16 * 2.0 ** -52
            assert (np.abs(rho.real - tabs[c].real) <= bound).all() and (np.abs(rho.imag - tabs[c].imag) <= bound).all()
            rx, ry = rho.real.astype(np.float32)[None], rho.imag.astype(np.float32)[None]
            vx, vy = w.real.copy(), w.imag.copy()
            re, im = vx * rx, vx * ry                                    # float32 arrays: every operation rounded on its own
            re -= vy * ry
            im += vy * rx
            weff.append((re + 1j * im).astype(np.complex64))
        for mode, tint, m, want64, tol in (("POWER", 3, mask, r.power(f, w, 3, mask, mt, tabs), TOL_BEAM_POWER),
                                           ("VOLTAGE", 0, None, r.voltages(f, w, None, 0, tabs), TOL_BEAM_VOLTAGE),
                                           ("INCOHERENT", 0, mask, r.incoherent(f, w, 0, mask, mt, tabs), TOL_BEAM_POWER)):
            kw = dict(tint=tint, mask=m, mask_tint=mt if m is not None else 0)
            plan.track_seek(t0)
            got = run(plan, mode, x, w, whole_samples=True, **kw)
            assert plan.track_chunk == t0 + n_chunks
            assert rel_err(got, want64) < tol, mode
            plan.track_seek(t0)
            dev = run(plan, mode, torch.from_numpy(x).cuda(), w, whole_samples=True, **kw)
            assert np.array_equal(bits(host(dev)), bits(got))
            for c in range(n_chunks):
                kc = dict(kw, mask=None if m is None else m[c:c + 1])
                want = run(fresh, mode, xa[c:c + 1], weff[c], **kc)
                assert np.array_equal(bits(got[c:c + 1]), bits(want)), (mode, c)
                plan.track_seek(t0 + c)                                 # one by one, after a seek: the same bits
                assert np.array_equal(bits(run(plan, mode, x[c:c + 1], w, whole_samples=True, **kc)), bits(want)), (mode, c)
            plan.track_seek(t0)
            with pytest.raises(NotImplementedError, match="whole-sample"):
                run(plan, mode, x, w, **kw)
            assert plan.track_chunk == t0


# -- 8: the antenna mask ------------------------------------------------------------------------------------------------------------
def test_kurtosis_mask_is_the_numpy_rule(plan_mod, torch):
    n_ant, nchan, n_pts, n_chunks = 3, 63, 37, 2
    x = beam_ref.noise_and_source(41, n_chunks, n_ant, nchan * n_pts)
    x[1, 2, 11 * nchan + 3] = np.nan                                     # a damaged sample: its bins' sk is NaN
    x[0, 1] += 3.0                                                       # and something to flag: a steady carrier in bin 0
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * n_pts) as plan:
        for tint in (5, 0, 36, 2):
            sk = plan.kurtosis(x, tint=tint)
            th = r.mask_thresholds(n_pts, tint)
            want = r.antenna_mask(sk, n_pts, tint, *th)
            got = plan.kurtosis_mask(sk, tint=tint)
            assert got.dtype == np.float32 and got.shape == sk.shape
            assert np.array_equal(bits(got), bits(want)), tint
            dev = plan.kurtosis_mask(torch.from_numpy(sk).cuda(), tint=tint)
            assert dev.is_cuda and np.array_equal(bits(host(dev)), bits(want)), tint
            if tint == 5:
                assert np.isnan(sk).any() and (want[np.isnan(sk)] == 0).all() and 0 < want.mean() < 1
                assert (want[0, 1] == 0).any() and sk.shape[2] == 8
                # given thresholds serve the full bins; the partial last bin keeps those of its own count
                tight = plan.kurtosis_mask(sk, lo=0.9, hi=1.1, tint=tint)
                assert np.array_equal(bits(tight), bits(r.antenna_mask(sk, n_pts, tint, 0.9, 1.1, th[2], th[3])))
                assert tight.sum() < want.sum()
            if tint == 36:                                               # a last bin of one frame: sk is exactly 1 and it counts
                assert (sk[:, :, 1][np.isfinite(sk[:, :, 1])] == 1).all() and th[2:] == (-np.inf, np.inf)
        # the mask feeds the beamformer as it is
        w = beam_ref.random_weights(42, 2, n_ant, nchan)
        m = plan.kurtosis_mask(plan.kurtosis(x, tint=5), tint=5)
        assert np.isfinite(plan.beamform(x, w, tint=5, mask=m, mask_tint=5)).all()
        assert not np.isfinite(plan.beamform(x, w, tint=5)).all()


# -- 9: argument errors -------------------------------------------------------------------------------------------------------------
def test_argument_errors(plan_mod, torch):
    n_ant, nchan, n_pts = 3, 16, 8
    x = beam_ref.noise_and_source(1, 2, n_ant, nchan * n_pts)
    w = beam_ref.random_weights(2, 2, n_ant, nchan)
    w17 = beam_ref.random_weights(3, 17, n_ant, nchan)
    mask = np.ones((2, n_ant, 2, nchan), np.float32)
    out = np.full((2, 2, 1, nchan), -7.0, np.float32)
    sk = np.ones((2, n_ant, 2, nchan), np.float32)
    mout = np.full(sk.shape, -7.0, np.float32)
    H, D, P, V, I = _lib.FXC_MEM_HOST, _lib.FXC_MEM_DEVICE, _lib.FXC_BEAM_POWER, _lib.FXC_BEAM_VOLTAGE, _lib.FXC_BEAM_INCOHERENT
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * n_pts) as plan:
        call = plan._lib.fxc_beamform_ex
        xp, wp, mp, op = x.ctypes.data, w.ctypes.data, mask.ctypes.data, out.ctypes.data
        assert call(None, xp, wp, 2, mp, 4, op, 2, H, P, 0, 0) == _lib.FXC_ERR_ARG
        for args in ((None, wp, 2, mp, 4, op, 2, H, P, 0, 0), (xp, None, 2, mp, 4, op, 2, H, P, 0, 0), (xp, wp, 2, mp, 4, None, 2, H, P, 0, 0),   # NULL
                     (xp, wp, 0, mp, 4, op, 2, H, P, 0, 0), (xp, wp, 2, mp, 4, op, -1, H, P, 0, 0),                        # n_beam, n_chunks
                     (xp, wp, 2, mp, 4, op, 2, H, 3, 0, 0), (xp, wp, 2, mp, 4, op, 2, H, -1, 0, 0),                         # mode
                     (xp, wp, 2, mp, 4, op, 2, 3, P, 0, 0), (xp, wp, 2, mp, 4, op, 2, _lib.FXC_MEM_DEVICE_TO_PINNED, I, 0, 0),   # mem_kind
                     (xp, wp, 2, mp, 4, op, 2, H, P, -1, 0), (xp, wp, 2, mp, 4, op, 2, H, I, n_pts + 1, 0),                  # tint
                     (xp, wp, 2, mp, -1, op, 2, H, P, 0, 0), (xp, wp, 2, mp, n_pts + 1, op, 2, H, V, 0, 0),                  # mask_tint
                     (xp, wp, 2, None, n_pts + 1, op, 2, H, P, 0, 0),                                                     # ... without a mask
                     (xp, wp, 2, mp, 4, op, 2, H, P, 0, 2), (xp, wp, 2, mp, 4, op, 2, H, P, 0, -1)):                        # align
            assert call(plan._h, *args) == _lib.FXC_ERR_ARG, args
        assert call(plan._h, xp, w17.ctypes.data, 17, mp, 4, op, 2, H, I, 0, 0) == _lib.FXC_ERR_UNSUPPORTED
        assert call(plan._h, xp, wp, 2, mp, 4, op, 0, H, P, 0, 0) == _lib.FXC_OK and call(plan._h, None, None, 2, None, 0, None, 0, D, I, 0, 1) == _lib.FXC_OK
        assert (out == -7.0).all()                                        # nothing was written
        for mode in (P, I):
            out[:] = -7.0
            assert call(plan._h, xp, wp, 2, mp, 4, op, 2, H, mode, n_pts, 1) == _lib.FXC_OK and (out != -7.0).all()
        # fxc_beamform itself does not know the incoherent mode
        assert plan._lib.fxc_beamform(plan._h, xp, wp, 2, op, 2, H, I, 0) == _lib.FXC_ERR_ARG
        # the antenna mask
        km = plan._lib.fxc_kurtosis_antenna_mask
        sp, kp = sk.ctypes.data, mout.ctypes.data
        assert km(None, sp, 2, 4, 0.5, 1.5, 0.5, 1.5, kp, H) == _lib.FXC_ERR_ARG
        for args in ((None, 2, 4, 0.5, 1.5, 0.5, 1.5, kp, H), (sp, 2, 4, 0.5, 1.5, 0.5, 1.5, None, H), (sp, -1, 4, 0.5, 1.5, 0.5, 1.5, kp, H),
                     (sp, 2, -1, 0.5, 1.5, 0.5, 1.5, kp, H), (sp, 2, 1, 0.5, 1.5, 0.5, 1.5, kp, H), (sp, 2, n_pts + 1, 0.5, 1.5, 0.5, 1.5, kp, H),
                     (sp, 2, 4, 0.5, 1.5, 0.5, 1.5, kp, 3), (sp, 2, 4, 1.5, 0.5, 0.5, 1.5, kp, H), (sp, 2, 4, 0.5, 1.5, 1.5, 0.5, kp, H),
                     (sp, 2, 4, float("nan"), 1.5, 0.5, 1.5, kp, H), (sp, 2, 4, 0.5, 1.5, 0.5, float("nan"), kp, H)):
            assert km(plan._h, *args) == _lib.FXC_ERR_ARG, args
        assert km(plan._h, sp, 0, 4, 0.5, 1.5, 0.5, 1.5, kp, H) == _lib.FXC_OK and (mout == -7.0).all()
        assert km(plan._h, sp, 2, 4, 0.5, 1.5, -np.inf, np.inf, kp, H) == _lib.FXC_OK and (mout == 1.0).all()
        # the Python layer
        with pytest.raises(NotImplementedError):
            plan.beamform_incoherent(x, w17)
        for bad in (dict(mask=mask, mask_tint=-1), dict(mask=mask[:, :, :1], mask_tint=n_pts + 1), dict(mask_tint=n_pts + 1), dict(mask_tint=-1)):
            with pytest.raises(ValueError):
                plan.beamform(x, w, **bad)
        for bad_m in (mask[:1], mask[:, :2], mask[:, :, :1], mask[..., :8], mask[0]):
            with pytest.raises(ValueError):
                plan.beamform(x, w, mask=bad_m, mask_tint=4)
        with pytest.raises(ValueError):
            plan.beamform(x, w, mask=torch.from_numpy(mask).cuda(), mask_tint=4)        # a device mask with host samples
        with pytest.raises(ValueError):
            plan.beamform(torch.from_numpy(x).cuda(), w, mask=torch.from_numpy(mask.astype(np.float64)).cuda(), mask_tint=4)
        with pytest.raises(ValueError):
            plan.beamform_incoherent(x, w, out=np.empty((2, 2, 1, nchan), np.complex64))
        o = np.empty((2, 2, 2, nchan), np.float32)
        assert plan.beamform_incoherent(x, w, tint=4, out=o, mask=mask, mask_tint=4) is o
        for bad_sk in (sk[:, :2], sk[:, :, :1], sk[0]):
            with pytest.raises(ValueError):
                plan.kurtosis_mask(bad_sk, tint=4)
        with pytest.raises(ValueError):
            plan.kurtosis_mask(sk, tint=1)
        with pytest.raises(ValueError):
            plan.kurtosis_mask(sk, lo=2.0, hi=1.0, tint=4)


# -- 10: the interference scenario --------------------------------------------------------------------------------------------------
def test_a_pulsed_tone_in_one_antenna_is_flagged_and_masked_out_of_the_beam(plan_mod, torch):
    """kurtosis -> kurtosis_mask -> beamform(mask=) on the scenario of beam_mask_ref (seed 0, the recorded level): the antenna is
    flagged in every affected cell, the unmasked beam there is 10 x the clean beam or more, and the masked beam, rescaled by
    (n_ant / count)^2, is within the recorded bound of the float64 clean beam in every cell that keeps an antenna"""
    with open(os.path.join(ROOT, "tests", "golden", "beam_mask_bounds.json")) as fh:
        rec = json.load(fh)
    nchan, tint = gains_ref.SAMPLE_NCHAN, r.RFI_TINT
    x, w, tone, window = r.rfi_case(0)
    dirty = r.rfi_dirty(x, tone, r.rfi_amplitude(rec["level"], x, window))
    p_clean = r.power(beam_ref.spectra(x, nchan, window), w, tint)       # float64: the yardstick
    w = w.astype(np.complex64)
    with plan_mod.FxPlan(beam_ref.GAIN_ANT, nchan, 4, nchan * gains_ref.SAMPLE_SPECTRA, window=window) as plan:
        sk = plan.kurtosis(dirty, tint=tint)
        mask = plan.kurtosis_mask(sk, tint=tint)
        p_dirty = plan.beamform(dirty, w, tint=tint).astype(np.float64)
        p_masked = plan.beamform(dirty, w, tint=tint, mask=mask, mask_tint=tint).astype(np.float64)
    fig = r.rfi_figures(p_clean, p_dirty, p_masked, mask)
    print("gpu", json.dumps(fig), "restatement", json.dumps(rec["figures"]["0"]), "bound", rec["bound"])
    assert fig["flagged"]
    assert fig["factor"] >= rec["factor_required"]
    assert fig["deviation"] <= rec["bound"]
