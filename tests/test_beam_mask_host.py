"""Masked and incoherent beams without a GPU (include/fxcorr.h fxc_beamform_ex): the float64 restatement (beam_mask_ref.py)
against the expansion of the beam power in the array's visibilities with the masked antennas' autos and baselines removed, the
coherent minus the incoherent power against the expansion's cross terms, the mask bin of every frame, the antenna-mask rule, and
the interference scenario under the figures of tests/golden/beam_mask_bounds.json (tools/beam_mask_measure.py --bounds: the tone's
level chosen and the bound set by the restatement alone)."""
import json
import os

import numpy as np
import pytest

import beam_mask_ref as r
import beam_ref
import fx_oracle
from effex_amd.window import design_window

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS = os.path.join(ROOT, "tests", "golden", "beam_mask_bounds.json")


def visibilities(f):
    """autos [n_ant, nchan] and cross [n_baselines, nchan] of the spectra f [n_chunks, n_ant, n_pts, nchan] over the whole call,
    in the rows' fftshifted order, with V_ab = <f_a conj(f_b)>"""
    n_ant = f.shape[1]
    autos = np.fft.fftshift((np.abs(f) ** 2).mean(axis=(0, 2)), axes=-1)
    cross = np.stack([np.fft.fftshift((f[:, a] * np.conj(f[:, b])).mean(axis=(0, 1)), axes=-1) for a, b in beam_ref.pairs(n_ant)])
    return autos, cross


@pytest.mark.parametrize("n_ant,nchan,n_beam,out", [(3, 16, 2, (1,)), (5, 15, 3, (0, 3)), (4, 32, 1, (0, 1, 2, 3))])
def test_masked_power_is_the_expansion_without_the_masked_antennas(n_ant, nchan, n_beam, out):
    """the antennas `out` masked in every cell: P_b equals beam_ref.expansion with their autos and baselines removed, 1e-12"""
    n_chunks, n_pts = 3, 6
    window = design_window(4, nchan)
    x = beam_ref.noise_and_source(n_ant * 100 + nchan, n_chunks, n_ant, nchan * n_pts)
    w = beam_ref.random_weights(7 + n_ant, n_beam, n_ant, nchan)
    f = beam_ref.spectra(x, nchan, window)
    assert np.allclose(visibilities(f)[1], fx_oracle.fx_integrate(x, nchan, window), rtol=0, atol=1e-12 * np.abs(f).max() ** 2)
    mask = np.ones((n_chunks, n_ant, 1, nchan), np.float32)
    mask[:, list(out)] = 0.0
    got = r.power(f, w, 0, mask, 0)[:, :, 0].mean(axis=0)
    autos, cross = visibilities(f)
    autos[list(out)] = 0.0
    for i, (a, b) in enumerate(beam_ref.pairs(n_ant)):
        if a in out or b in out:
            cross[i] = 0.0
    want = beam_ref.expansion(w, autos, cross)
    scale = np.abs(beam_ref.expansion(w, *visibilities(f))).max()
    assert np.abs(got - want).max() <= 1e-12 * scale
    if len(out) == n_ant:
        assert not got.any()


@pytest.mark.parametrize("n_ant,nchan,n_beam", [(2, 16, 1), (3, 15, 2), (5, 32, 3)])
def test_coherent_minus_incoherent_is_the_cross_terms(n_ant, nchan, n_beam):
    """P_coh - P_inc = 2 Re sum_{a<b} w_a conj(w_b) V_ab: the expansion with the autos at zero, within 1e-12 of max P; and the
    incoherent power alone is the expansion with the cross rows at zero -- with and without a mask that changes from cell to cell"""
    n_chunks, n_pts = 2, 7
    window = design_window(4, nchan)
    x = beam_ref.noise_and_source(n_ant * 10 + nchan, n_chunks, n_ant, nchan * n_pts)
    w = beam_ref.random_weights(3 + n_ant, n_beam, n_ant, nchan)
    f = beam_ref.spectra(x, nchan, window)
    for mask, mt in ((None, 0), (r.random_mask(5, n_chunks, n_ant, n_pts, nchan, 3), 3)):
        fs = r.select(f, mask, mt)                                       # a masked sample is a sample of 0: the identity holds on fs
        autos, cross = visibilities(fs)
        coh = r.power(f, w, 0, mask, mt)[:, :, 0].mean(axis=0)
        inc = r.incoherent(f, w, 0, mask, mt)[:, :, 0].mean(axis=0)
        scale = np.abs(coh).max()
        assert np.abs(coh - inc - beam_ref.expansion(w, np.zeros_like(autos), cross)).max() <= 1e-12 * scale
        assert np.abs(inc - beam_ref.expansion(w, autos, np.zeros_like(cross))).max() <= 1e-12 * scale


@pytest.mark.parametrize("n_pts", [37, 70])
def test_mask_bin_of_every_frame(n_pts):
    """frame i is under mask bin i // mask_tint (0: the chunk), written out by hand -- and the walk the kernel makes (k_beam.h
    MaskWalk: a running bin and a count inside it, by tiles of 8 frames inside ranges of fpr frames) gives the same bins"""
    for mt in (2, 5, 8, 33, 0):
        span = mt or n_pts
        want = [i // span for i in range(n_pts)]
        assert r.mask_bin_of_frames(n_pts, mt).tolist() == want
        assert r.n_mbin(n_pts, mt) == -(-n_pts // span) == want[-1] + 1
        for fpr in (30, 32, 35, 8):
            got = [None] * n_pts
            for i0 in range(0, n_pts, fpr):
                i1 = min(i0 + fpr, n_pts)
                j, rem = divmod(i0, span)
                for i in range(i0, i1, 8):
                    tile = []
                    for fr in range(8):
                        tile.append(j)
                        if i + fr + 1 < i1:
                            rem += 1
                            if rem == span:
                                rem, j = 0, j + 1
                    for fr in range(8):
                        if i + fr < i1:
                            got[i + fr] = tile[fr]
                        else:
                            assert tile[fr] == tile[i1 - 1 - i]               # past the range: the last frame's bin again
            assert got == want, (mt, fpr)


def test_antenna_mask_rule():
    n_pts, tint = 37, 5
    rng = np.random.default_rng(1)
    sk = rng.uniform(0.0, 2.0, (2, 3, 8, 6)).astype(np.float32)
    sk[0, 1, 2, 3] = np.nan
    sk[1, 0, 7, 0] = 1.0
    lo, hi, lo_last, hi_last = r.mask_thresholds(n_pts, tint)
    assert lo < 1 < hi and lo_last < lo and hi_last > hi               # two frames: wider than five
    m = r.antenna_mask(sk, n_pts, tint, lo, hi, lo_last, hi_last)
    assert m.dtype == np.float32 and m.shape == sk.shape and m[0, 1, 2, 3] == 0 and m[1, 0, 7, 0] == 1
    s = sk.astype(np.float64)
    for j in range(8):
        a, b = (lo_last, hi_last) if j == 7 else (lo, hi)
        with np.errstate(invalid="ignore"):
            assert np.array_equal(m[:, :, j], ((a <= s[:, :, j]) & (s[:, :, j] <= b)).astype(np.float32))
    assert r.mask_thresholds(36, 5)[2:] == (-np.inf, np.inf)           # a last bin of one frame: sk is exactly 1
    assert r.mask_thresholds(35, 5)[2:] == (-np.inf, np.inf)           # no partial bin: never used
    one = r.antenna_mask(sk[:, :, :1], 37, 0, lo, hi, 5.0, 6.0)         # the chunk's only bin: (lo, hi)
    assert np.array_equal(one, r.antenna_mask(sk[:, :, :1], 37, 0, lo, hi, lo, hi))


def test_random_mask_has_its_three_cells():
    m = r.random_mask(3, 2, 3, 37, 63, 5)
    cells = r.special_cells(2, 8, 63)
    with np.errstate(invalid="ignore"):
        on = m > 0
    assert not on[0, :, 7, 31].any() and on[0, :, 0, 30].all() and not on[1, 1].any() and cells["none"] == (0, 7, 31)
    assert 0.25 < 1.0 - on.mean() < 0.45                               # about 30 % zeros, and the antenna that is out


def test_interference_scenario_in_float64():
    """A pulsed tone in one antenna, flagged by the spectral kurtosis and masked out of the beam (beam_mask_ref.rfi_restatement),
    every seed: writes nothing, and finds the recorded figures again"""
    with open(BOUNDS) as fh:
        rec = json.load(fh)
    assert rec["level"] in r.RFI_LEVELS and rec["factor_required"] == r.RFI_FACTOR and rec["margin"] == r.RFI_MARGIN
    assert rec["seeds"] == list(r.RFI_SEEDS)
    worst = 0.0
    for seed in r.RFI_SEEDS:
        fig = r.rfi_restatement(seed, rec["level"])
        assert fig["flagged"] and fig["factor"] >= r.RFI_FACTOR, (seed, fig)
        assert fig["deviation"] == pytest.approx(rec["figures"][str(seed)]["deviation"], rel=1e-9)
        assert fig["factor"] == pytest.approx(rec["figures"][str(seed)]["factor"], rel=1e-9)
        assert fig["deviation"] <= rec["bound"]
        worst = max(worst, fig["deviation"])
    assert rec["observed"] == pytest.approx(worst, rel=1e-9) and rec["bound"] == pytest.approx(r.RFI_MARGIN * worst, rel=1e-9)
    # the level below the chosen one misses one of the two conditions for some seed: the choice is the smallest
    lower = r.RFI_LEVELS[r.RFI_LEVELS.index(rec["level"]) - 1]
    figs = [r.rfi_restatement(seed, lower) for seed in r.RFI_SEEDS]
    assert not all(f["flagged"] and f["factor"] >= r.RFI_FACTOR for f in figs)
