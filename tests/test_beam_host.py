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


# -- frame ranges, tiles and the bin flush of beam_kernel ---------------------------------------------------------------------------
K_BEAM_FRAMES = 8        # k_beam.h::kBeamFrames
K_GRID_MAX = 65535       # h_plan.h::kGridMax
LONG_FRAMES = (37, 70)   # the frame counts of beam_ref.LONG_SHAPES


def frames_per_range(n_pts, tint, power=True):
    """h_tools.h::launch_beam: whole time bins (VOLTAGE: whole tiles), 32 frames or more where a bin is shorter, and no more ranges
    than gridDim.y holds"""
    unit = (tint or n_pts) if power else K_BEAM_FRAMES
    fpr = unit * max(1, 32 // unit)
    return max(fpr, ((n_pts + K_GRID_MAX - 1) // K_GRID_MAX + unit - 1) // unit * unit)


def walk(n_pts, tint, power=True):
    """beam_kernel's loops over one (column, chunk): -> ranges [(i0, i1)], tiles [(range, frames read)], and -- POWER -- the flushes
    [(bin, frames added since the last flush, count the sum is divided by)]; VOLTAGE: [(frame stored, [frame read], 1)]"""
    tint = tint or n_pts
    fpr = frames_per_range(n_pts, tint, power)
    ranges, tiles, flushes = [], [], []
    for y in range(-(-n_pts // fpr)):
        i0 = y * fpr
        i1 = i0 + fpr if i0 + fpr < n_pts else n_pts
        ranges.append((i0, i1))
        added, cnt = [], 0
        for i in range(i0, i1, K_BEAM_FRAMES):
            read = [i + f if i + f < i1 else i1 - 1 for f in range(K_BEAM_FRAMES)]
            tiles.append((y, read))
            for f in range(K_BEAM_FRAMES):
                frame = i + f
                if frame >= i1:
                    break
                if not power:
                    flushes.append((frame, [read[f]], 1))
                    continue
                added.append(read[f])
                cnt += 1
                if cnt == tint or frame == n_pts - 1:
                    flushes.append((frame // tint, added, cnt))
                    added, cnt = [], 0
        assert not added, "a range ends inside a time bin"
    return ranges, tiles, flushes


def test_frame_ranges_are_the_ones_the_shapes_claim():
    assert [walk(37, t)[0] for t in (3, 5)] == [[(0, 30), (30, 37)]] * 2
    assert walk(37, 0, power=False)[0] == [(0, 32), (32, 37)] and walk(70, 0, power=False)[0] == [(0, 32), (32, 64), (64, 70)]
    assert walk(37, 36)[0] == [(0, 36), (36, 37)] and walk(70, 69)[0] == [(0, 69), (69, 70)] and walk(70, 33)[0] == [(0, 33), (33, 66), (66, 70)]
    assert walk(37, 1)[0] == [(0, 32), (32, 37)] and walk(37, 0)[0] == walk(37, 37)[0] == [(0, 37)]
    assert walk(8, 3)[0] == [(0, 8)] and walk(16, 1, power=False)[0] == [(0, 16)]          # the earlier shapes: one range, full tiles
    for n_pts in LONG_FRAMES:
        for tint, power in [(t, True) for t in beam_ref.tints_of(n_pts)] + [(0, False)]:
            ranges, tiles, _ = walk(n_pts, tint, power)
            assert ranges[0][0] == 0 and ranges[-1][1] == n_pts and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
            for y, read in tiles:                                        # every read stays inside its range
                assert all(ranges[y][0] <= i < ranges[y][1] for i in read)
            if tint not in (0, n_pts):
                assert len(ranges) > 1, (n_pts, tint)
            # the last range's last tile is partial; at 37 frames every range's is, but for the ranges of 32 (single frames, voltages)
            last = [[r for yy, r in tiles if yy == y][-1] for y in range(len(ranges))]
            partial = [len(set(r)) < K_BEAM_FRAMES for r in last]
            assert partial[-1] and (n_pts != 37 or tint == 1 or not power or all(partial)), (n_pts, tint, partial)


def beam_tiles(n_beam):
    """the kernel instantiations (beams per thread) of a call's beam tiles: h_tools.h::launch_beam"""
    out = []
    for b0 in range(0, n_beam, 8):
        left = n_beam - b0
        out.append(8 if left > 4 else 4 if left > 2 else 2 if left > 1 else 1)
    return out


def test_every_beam_tile_meets_a_second_range_and_a_partial_tile():
    """every shape of beam_ref.LONG_SHAPES has both in every mode (above), and between them they launch every instantiation"""
    assert [beam_tiles(s[5]) for s in beam_ref.LONG_SHAPES] == [[4], [8, 1], [8], [2]]
    assert [beam_tiles(n) for n in (1, 2, 3, 4, 5, 8, 9, 10, 16)] == [[1], [2], [4], [4], [8], [8], [8, 1], [8, 2], [8, 8]]


@pytest.mark.parametrize("n_pts", LONG_FRAMES)
def test_every_frame_lands_in_exactly_one_bin_with_its_count(n_pts):
    assert beam_ref.tints_of(37) == [0, 1, 3, 5, 33, 36, 37] and beam_ref.tints_of(70) == [0, 1, 3, 5, 33, 69, 70]
    assert beam_ref.tints_of(8) == [0, 1, 3, 5, 7, 8] and beam_ref.tints_of(16) == [0, 1, 3, 5, 15, 16]
    for tint in beam_ref.tints_of(n_pts):
        bins = beam_ref.time_bins(n_pts, tint)
        _, _, flushes = walk(n_pts, tint)
        assert [j for j, _, _ in flushes] == list(range(len(bins))), tint          # every bin stored once, no other
        for j, added, cnt in flushes:
            i0, i1 = bins[j]
            assert added == list(range(i0, i1)) and cnt == i1 - i0, (tint, j)      # its frames in order, the divisor power() uses
        assert sorted(i for _, added, _ in flushes for i in added) == list(range(n_pts))
    _, _, stored = walk(n_pts, 0, power=False)
    assert [(frame, read) for frame, read, _ in stored] == [(i, [i]) for i in range(n_pts)]


@pytest.mark.parametrize("shape", beam_ref.LONG_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_a_range_boundary_frame_lost_or_doubled_moves_the_power_ten_ceilings(shape):
    """what test_gpu_beamform.py would see, on its own inputs, of a range that drops its last frame or adds its first one twice
    (the bin keeps its divisor)"""
    assert sorted({s[3] for s in beam_ref.LONG_SHAPES}) == list(LONG_FRAMES)
    n_ant, nchan, ntaps, n_pts, n_chunks, n_beam = shape
    ceiling = 1e-5                                                           # (TOL_BEAM_POWER's)
    x, w, window = beam_ref.shape_case(shape)
    y = beam_ref.voltages(beam_ref.spectra(x, nchan, window), w)
    assert y.shape == (n_chunks, n_beam, n_pts, nchan)
    for tint in beam_ref.tints_of(n_pts):
        want = beam_ref.power(y, tint)
        for i0, i1 in walk(n_pts, tint)[0]:
            for frame, factor, what in ((i1 - 1, 0.0, "dropped"), (i0, np.sqrt(2.0), "counted twice")):
                bad = y.copy()
                bad[:, :, frame] *= factor
                err = np.abs(beam_ref.power(bad, tint) - want).max() / np.abs(want).max()
                assert err >= 10.0 * ceiling, (tint, frame, what, err)


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
