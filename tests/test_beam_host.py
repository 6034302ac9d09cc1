"""The beamformer's definition without a GPU (include/fxcorr.h fxc_beamform): the float64 restatement (beam_ref.py) against the
expansion of the beam power in the array's own visibilities, beam_weights against the tables it is made of, a partial last time
bin written out by hand, the coherent gain of the on-source beam under the bound of tests/golden/beam_bounds.json
(tools/beam_measure.py: three times the restatement's own largest deviation) and the ABI's
argument check that needs no device.  (tests/test_isa_hazards.py holds the new kernels, like every kernel, to no scratch, no flat
instruction and 256 registers.)"""
import json
import os

import numpy as np
import pytest

import beam_ref
import fx_oracle
import gains_ref
from effex_amd import _lib
from effex_amd.window import design_window

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS = os.path.join(ROOT, "tests", "golden", "beam_bounds.json")
BW, FC = 2.4e6, 1.4204e9


def plan_module():
    from effex_amd import plan
    return plan


# -- the restatement against the expansion ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ant,nchan,n_beam", [(2, 16, 1), (3, 15, 2), (5, 32, 3)])
def test_restatement_equals_the_expansion_in_visibilities(n_ant, nchan, n_beam):
    """P_b = sum_a |w_a|^2 A_a + 2 Re sum_{a<b'} w_a conj(w_b') V_ab' to 1e-12 of max P, whole call as one time bin"""
    n_chunks, num_samp = 3, nchan * 6
    window = design_window(4, nchan)
    x = beam_ref.noise_and_source(n_ant * 100 + nchan, n_chunks, n_ant, num_samp)
    w = beam_ref.random_weights(7 + n_ant, n_beam, n_ant, nchan)
    per_chunk = beam_ref.beamform(x, w, nchan, window, tint=0)          # [n_chunks, n_beam, 1, nchan]
    assert per_chunk.shape == (n_chunks, n_beam, 1, nchan)
    got = per_chunk[:, :, 0].mean(axis=0)                               # equal frame counts: the mean over the call
    cross = fx_oracle.fx_integrate(x, nchan, window)
    autos = beam_ref.autos_of(x, nchan, window)
    want = beam_ref.expansion(w, autos, cross)
    assert want.shape == (n_beam, nchan)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


# -- beam_weights -----------------------------------------------------------------------------------------------------------------
def test_beam_weights_are_the_tables_times_the_taper():
    plan = plan_module()
    n_ant, nchan = 4, 12
    rng = np.random.default_rng(3)
    delays = rng.uniform(-1e-6, 1e-6, n_ant)
    offsets = rng.uniform(-1e-7, 1e-7, (3, n_ant))
    gains = gains_ref.draw_gains(n_ant, nchan, rng)
    gains[1, 5] = 0.0                                                   # a dead channel stays zero
    taper = rng.uniform(0.1, 1.0, n_ant)
    w = plan.beam_weights(n_ant, nchan, BW, FC, delays_s=delays, beam_delays_s=offsets, gains=gains, taper=taper)
    assert w.shape == (3, n_ant, nchan) and w.dtype == np.complex64
    for b in range(3):
        want = plan.gain_tables(gains, n_ant, nchan, delays + offsets[b], BW, FC) * taper[:, None]
        assert np.array_equal(w[b], want.astype(np.complex64))
    dead = int(np.flatnonzero(np.fft.ifftshift(np.arange(nchan)) == 5)[0])      # rows' bin 5 in natural order
    assert (w[:, 1, dead] == 0).all() and np.count_nonzero(w == 0) == 3
    w = plan.beam_weights(n_ant, nchan, BW, FC, delays_s=delays, beam_delays_s=offsets)
    for b in range(3):
        want = plan.rot_tables(nchan, BW, FC, delays + offsets[b]) / n_ant
        assert np.array_equal(w[b], want.astype(np.complex64))
    # no delays, no offsets: one beam at the phase centre, the plain mean of the antennas
    w = plan.beam_weights(n_ant, nchan, BW, FC)
    assert w.shape == (1, n_ant, nchan) and np.array_equal(w, np.full((1, n_ant, nchan), 1.0 / n_ant, np.complex64))
    # under a delay track: the offsets alone
    w = plan.beam_weights(n_ant, nchan, BW, FC, beam_delays_s=offsets[:2])
    assert np.array_equal(w[1], (plan.rot_tables(nchan, BW, FC, offsets[1]) / n_ant).astype(np.complex64))
    for bad in (dict(delays_s=np.zeros(n_ant + 1)), dict(beam_delays_s=np.zeros((2, n_ant + 1))), dict(taper=np.ones(n_ant - 1)),
                dict(gains=np.ones((n_ant, nchan + 1)))):
        with pytest.raises(ValueError):
            plan.beam_weights(n_ant, nchan, BW, FC, **bad)


# -- time bins --------------------------------------------------------------------------------------------------------------------
def test_partial_last_time_bin_by_hand():
    """7 frames at tint 3: bins of 3, 3 and 1 frames, the last divided by 1; and the fftshift of an odd channel count"""
    nchan, n_pts = 5, 7
    rng = np.random.default_rng(11)
    y = rng.standard_normal((1, 1, n_pts, nchan)) + 1j * rng.standard_normal((1, 1, n_pts, nchan))
    assert beam_ref.time_bins(n_pts, 3) == [(0, 3), (3, 6), (6, 7)]
    assert beam_ref.time_bins(n_pts, 0) == [(0, 7)] and beam_ref.time_bins(n_pts, 7) == [(0, 7)]
    assert beam_ref.time_bins(n_pts, 1) == [(i, i + 1) for i in range(n_pts)]
    got = beam_ref.power(y, 3)
    assert got.shape == (1, 1, 3, nchan)
    p = (y.real ** 2 + y.imag ** 2)[0, 0]
    order = [3, 4, 0, 1, 2]                                             # numpy's fftshift of five bins
    want = np.stack([(p[0] + p[1] + p[2]) / 3.0, (p[3] + p[4] + p[5]) / 3.0, p[6]])[:, order]
    assert np.allclose(got[0, 0], want, rtol=1e-15, atol=0)
    # the device's index: natural bin k lands at (k + nchan // 2) % nchan
    for n in (4, 5, 63, 64):
        k = np.arange(n)
        shifted = np.fft.fftshift(k)
        assert np.array_equal(shifted[(k + n // 2) % n], k)


# -- coherent gain ----------------------------------------------------------------------------------------------------------------
def coherent_gain_deviation(seed, beamform=None):
    """the deviation of beam_ref.gain_deviation for one seed; beamform(x, w) -> power [n_chunks, n_beam, 1, nchan] (default: the
    restatement)"""
    nchan = gains_ref.SAMPLE_NCHAN
    window = design_window(4, nchan)
    x, src, noise, c = beam_ref.gain_parts(beam_ref.GAIN_ANT, seed)
    assert np.array_equal(x, gains_ref.samples(beam_ref.GAIN_ANT, seed, n_chunks=beam_ref.GAIN_CHUNKS)[0])
    w = beam_ref.gain_weights(c, nchan)
    if beamform is None:
        def beamform(part, wts):
            return beam_ref.beamform(part, wts, nchan, window, tint=0)
    return beam_ref.gain_deviation(beamform(src, w), beamform(noise, w))


def test_coherent_gain_is_n_ant_times_one_antennas():
    with open(BOUNDS) as fh:
        rec = json.load(fh)
    assert rec["n_ant"] == beam_ref.GAIN_ANT and rec["seeds"] == list(beam_ref.GAIN_SEEDS) and rec["n_chunks"] == beam_ref.GAIN_CHUNKS
    assert rec["bound"] == 3.0 * rec["observed"] == 3.0 * max(rec["deviation"].values())
    assert 0.0 < rec["bound"] < 0.1                                     # cross terms of 8 x 32768 samples: a per cent or so
    for seed in beam_ref.GAIN_SEEDS:
        dev = coherent_gain_deviation(seed)
        print("seed", seed, "deviation", dev, "recorded", rec["deviation"][str(seed)], "bound", rec["bound"])
        assert dev == pytest.approx(rec["deviation"][str(seed)], rel=1e-6)
        assert dev <= rec["bound"]


# -- ABI --------------------------------------------------------------------------------------------------------------------------
def test_beamform_is_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "fxcorr.h")).read()
    assert "int fxc_beamform(fxc_plan* plan, const void* x, const void* weights, int n_beam, void* out" in text
    assert "enum fxc_beam_mode { FXC_BEAM_POWER = 0, FXC_BEAM_VOLTAGE = 1 };" in text
    assert (_lib.FXC_BEAM_POWER, _lib.FXC_BEAM_VOLTAGE) == (0, 1)
    lib = _lib.load()
    assert lib.fxc_beamform.argtypes == _lib.SIGNATURES["fxc_beamform"][1] and len(lib.fxc_beamform.argtypes) == 9
    # a NULL plan is an argument error before any device work
    assert lib.fxc_beamform(None, None, None, 1, None, 1, _lib.FXC_MEM_HOST, _lib.FXC_BEAM_POWER, 0) == _lib.FXC_ERR_ARG
