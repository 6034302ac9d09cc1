"""Whole-sample delays on the host (no GPU): why they are needed, from the float64 oracle, and the numpy half of the interface
(effex_amd.plan.split_delays / aligned_rot_tables) against tests/align_ref.py.

A phase slope after the FFT is the fractional-sample half of a delay correction.  For a delay of d samples two antennas' frames
overlap only partly and the correlated amplitude falls roughly as 1 - d / nchan whatever the slope does; reading the late
antenna's samples d later and keeping only the remainder in the table puts it back."""
import numpy as np
import pytest

import align_ref
from effex_amd import plan as fx_plan
from effex_amd import synth
from effex_amd.window import design_window
from tolerances import TOL_VIS

BW = 2.4e6
FREQ = 1.42e9
# nchan, num_samp, d: the lines of the table in DESIGN.md (whole-sample delays)
LINES = [(64, 4096, 42), (64, 4096, 12), (256, 8192, 42), (1024, 16384, 300)]

_cache = {}


def case(nchan, num_samp, d):
    """Everything a line's tests share, computed once: the streams, the window, the rows of the three corrections."""
    key = (nchan, num_samp, d)
    if key not in _cache:
        window = design_window(4, nchan)
        x0 = synth.synth_iq(5, 1, 2, num_samp, delays=(0, 0))
        xd = synth.synth_iq(5, 1, 2, num_samp, delays=(0, d))
        tau = np.array([0.0, d / BW])
        shifts, _ = fx_plan.split_delays(tau, BW)
        assert shifts.tolist() == [0, d]
        ones = np.ones((2, nchan), dtype=np.complex128)
        base = align_ref.rows(x0, nchan, window, ones)[0, 0]
        phase_only = align_ref.rows(xd, nchan, window, fx_plan.rot_tables(nchan, BW, FREQ, tau))[0, 0]
        tables = fx_plan.aligned_rot_tables(nchan, BW, FREQ, tau, shifts)          # what set_delays(.., whole_samples=True) sends
        aligned = align_ref.rows(align_ref.align(xd, shifts), nchan, window, tables)[0, 0]
        _cache[key] = dict(window=window, xd=xd, tau=tau, shifts=shifts, base=base, phase_only=phase_only, tables=tables, aligned=aligned)
    return _cache[key]


@pytest.mark.parametrize("nchan,num_samp,d", LINES)
def test_alignment_recovers_the_amplitude_a_phase_slope_loses(nchan, num_samp, d):
    """|mean over the bins of the row| relative to the same source with delays (0, 0): aligned >= 0.95 (measured 1.000 - 1.009),
    and at 64 channels and 42 samples the phase-only correction keeps at most 0.6 (measured 0.500); on every line the
    phase-only ratio is below the aligned one by about d / nchan."""
    c = case(nchan, num_samp, d)
    base = abs(c["base"].mean())
    r_phase, r_aligned = abs(c["phase_only"].mean()) / base, abs(c["aligned"].mean()) / base
    print("nchan %d num_samp %d d %d: phase-only %.3f aligned %.3f" % (nchan, num_samp, d, r_phase, r_aligned))
    assert r_aligned >= 0.95
    if (nchan, d) == (64, 42):
        assert r_phase <= 0.6
    # frames that overlap only partly can only lose: 0.956 at 64 / 12, 0.964 at 256 / 42, 0.871 at 1024 / 300
    assert r_phase < r_aligned and r_phase < 1.0


@pytest.mark.parametrize("nchan,num_samp,d", LINES)
def test_mutations_move_the_aligned_row(nchan, num_samp, d):
    """The shift with the wrong sign, the shift one sample off and the table's slope term with the wrong sign each move the
    oracle's aligned row by at least ten TOL_VIS ceilings of its maximum (measured: 0.28 to 1.9 of the maximum), so a comparison
    within TOL_VIS tells them apart."""
    c = case(nchan, num_samp, d)
    good, scale = c["aligned"], np.abs(c["aligned"]).max()
    mutants = {
        "sign of the shift": align_ref.rows(align_ref.align(c["xd"], -c["shifts"]), nchan, c["window"], c["tables"])[0, 0],
        "one sample off": align_ref.rows(align_ref.align(c["xd"], c["shifts"] + np.array([0, 1])), nchan, c["window"], c["tables"])[0, 0],
        "sign of the slope term": align_ref.rows(align_ref.align(c["xd"], c["shifts"]), nchan, c["window"],
                                                 align_ref.tables(nchan, BW, FREQ, c["tau"], c["shifts"], slope_sign=-1))[0, 0],
    }
    for name, row in mutants.items():
        moved = np.abs(row - good).max() / scale
        print("nchan %d d %d, %s: moved by %.3g of the maximum" % (nchan, d, name, moved))
        assert moved >= 10 * TOL_VIS.ceiling, name


def test_align_ref_is_a_zero_filled_shift():
    x = (np.arange(2 * 3 * 5).reshape(2, 3, 5) + 1).astype(np.complex64)
    shifts, _ = fx_plan.split_delays([0.0, 2.2 / BW, -1.4 / BW], BW)
    assert shifts.tolist() == [0, 2, -1]
    out = align_ref.align(x, shifts)
    assert np.array_equal(out[:, 0], x[:, 0])
    assert np.array_equal(out[1, 1], np.array([x[1, 1, 2], x[1, 1, 3], x[1, 1, 4], 0, 0]))
    assert np.array_equal(out[0, 2], np.array([0, x[0, 2, 0], x[0, 2, 1], x[0, 2, 2], x[0, 2, 3]]))
    per_chunk = align_ref.align(x, [[0, 5, -5], [4, -4, 1]])
    assert not per_chunk[0, 1:].any() and np.array_equal(per_chunk[1, 0], np.array([x[1, 0, 4], 0, 0, 0, 0]))
    assert np.array_equal(per_chunk[1, 1], np.array([0, 0, 0, 0, x[1, 1, 0]]))


def test_split_delays_round_trip_and_ties():
    rng = np.random.default_rng(3)
    tau = rng.uniform(-2e-3, 2e-3, size=64)
    shifts, rem = fx_plan.split_delays(tau, BW)
    assert shifts.dtype == np.int64 and rem.dtype == np.float64
    assert np.array_equal(shifts, np.rint(tau * BW).astype(np.int64))
    assert (np.abs(rem) * BW <= 0.5 + 1e-9).all()
    # tau = shifts / bw + remainder up to the rounding of the two operations (|tau| <= 2e-3: 2^-9 2^-52 each)
    assert np.abs(shifts / BW + rem - tau).max() <= 2 * 2.0 ** -61
    # ties go to even: bandwidth 2 makes tau * bandwidth exact
    shifts, rem = fx_plan.split_delays([0.25, 0.75, 1.25, -0.25, -0.75, 3.0], 2.0)
    assert shifts.tolist() == [0, 2, 2, 0, -2, 6]
    assert rem.tolist() == [0.25, -0.25, 0.25, -0.25, 0.25, 0.0]


@pytest.mark.parametrize("nchan", [1, 64, 1000, 4096])
def test_aligned_rot_tables(nchan):
    """aligned_rot_tables is tests/align_ref.py's table (the definition of include/fxcorr.h) and, with shifts 0, rot_tables
    within the bound of tests/test_gpu_tracking.py::test_track_tables with its constant term doubled for the two added
    operations: |diff| <= 4 pi |f_k tau| 2^-52 + 16 * 2^-52 per component."""
    tau = np.array([0.0, 42.3 / BW, -1234.5 / BW, 7.4e-6])
    shifts, _ = fx_plan.split_delays(tau, BW)
    got = fx_plan.aligned_rot_tables(nchan, BW, FREQ, tau, shifts)
    want = align_ref.tables(nchan, BW, FREQ, tau, shifts)
    assert got.shape == (4, nchan) and got.dtype == np.complex128
    assert np.abs(got - want).max() <= 8 * 2.0 ** -52          # the same v; exp against cos / sin of it
    freqs = np.fft.fftfreq(nchan, d=1.0 / BW) + FREQ
    bound = 4 * np.pi * np.abs(freqs[None, :] * tau[:, None]) * 2.0 ** -52 + 16 * 2.0 ** -52
    zero = fx_plan.aligned_rot_tables(nchan, BW, FREQ, tau, np.zeros(4, dtype=np.int64))
    plain = fx_plan.rot_tables(nchan, BW, FREQ, tau)
    assert (np.abs(zero.real - plain.real) <= bound).all() and (np.abs(zero.imag - plain.imag) <= bound).all()
    # what the table leaves out is exactly the baseband slope of the shift: r_aligned = r_full exp(-2 pi i kk s / nchan)
    kk = np.rint(np.fft.fftfreq(nchan) * nchan)
    slope = np.exp(-2j * np.pi * kk[None, :] * shifts[:, None] / nchan)
    assert (np.abs(got - plain * slope) <= 2 * bound).all()          # (the same bound: the full table's phase rounds at f_k tau)
