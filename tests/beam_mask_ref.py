"""Float64 restatement of the masked and the incoherent beams (include/fxcorr.h fxc_beamform_ex) and of the antenna mask
(fxc_kurtosis_antenna_mask) on beam_ref.spectra: what tests/test_beam_mask_host.py checks on its own and
tests/test_gpu_beam_mask.py holds the library to.  The mask, the bins and the sums are written as the header defines them; it
shares no code with the library or effex_amd/plan.py."""
import numpy as np

import beam_ref


# -- the definition ---------------------------------------------------------------------------------------------------------------
def mask_bin_of_frames(n_pts, mask_tint):
    """the mask bin of every frame: i // mask_tint, mask_tint 0 = the whole chunk"""
    span = n_pts if mask_tint == 0 else mask_tint
    return np.arange(n_pts) // span


def counted(mask, n_pts, mask_tint):
    """mask [n_chunks, n_ant, n_mbin, nchan] in the rows' fftshifted channel order -> bool [n_chunks, n_ant, n_pts, nchan] in
    NATURAL order: antenna a counts in a cell iff its value is > 0 (a NaN does not)"""
    mask = np.asarray(mask)
    bins = mask_bin_of_frames(n_pts, mask_tint)
    assert mask.shape[2] == bins[-1] + 1, (mask.shape, n_pts, mask_tint)
    with np.errstate(invalid="ignore"):
        on = np.fft.ifftshift(mask > 0, axes=-1)          # natural[k] = stored[(k + nchan // 2) % nchan]
    return on[:, :, bins]


def select(f, mask, mask_tint):
    """the spectra with every sample that does not count replaced by 0 -- a selection: what the sample held does not matter"""
    if mask is None:
        return np.asarray(f)
    return np.where(counted(mask, f.shape[2], mask_tint), f, 0.0)


def voltages(f, w, mask=None, mask_tint=0, tables=None):
    """y[c, b, i, k] = sum_{a counted} w[b, a, k] rho[c, a, k] f[c, a, i, k]"""
    return beam_ref.voltages(select(f, mask, mask_tint), w, tables)


def power(f, w, tint=0, mask=None, mask_tint=0, tables=None):
    return beam_ref.power(voltages(f, w, mask, mask_tint, tables), tint)


def incoherent(f, w, tint=0, mask=None, mask_tint=0, tables=None):
    """[n_chunks, n_beam, n_tbin, nchan] float64: fftshift_k of the mean over each time bin of sum_{a counted} |w rho|^2 |f|^2"""
    w = beam_ref.weights_3d(w)
    rho = np.ones((f.shape[0],) + w.shape[1:], np.complex128) if tables is None else np.asarray(tables, dtype=np.complex128)
    g2 = np.abs(w[None] * rho[:, None]) ** 2                                              # [c, b, a, k]
    q = np.einsum("cbak,caik->cbik", g2, np.abs(select(f, mask, mask_tint)) ** 2)
    out = np.stack([q[:, :, i0:i1].sum(axis=2) / float(i1 - i0) for i0, i1 in beam_ref.time_bins(f.shape[2], tint)], axis=2)
    return np.fft.fftshift(out, axes=-1)


def antenna_mask(sk, n_pts, tint, lo, hi, lo_last, hi_last):
    """sk [n_chunks, n_ant, n_tbin, nchan] (compared as float64) -> float32 of the same shape: 1 iff lo_j <= sk <= hi_j, with
    (lo_last, hi_last) for a partial last bin that is not the chunk's only bin -- comparisons, so a NaN gives 0"""
    s = np.asarray(sk).astype(np.float64)
    bins = beam_ref.time_bins(n_pts, tint)
    lo_j = np.full(len(bins), float(lo))
    hi_j = np.full(len(bins), float(hi))
    if len(bins) > 1 and bins[-1][1] - bins[-1][0] != bins[0][1] - bins[0][0]:
        lo_j[-1], hi_j[-1] = float(lo_last), float(hi_last)
    with np.errstate(invalid="ignore"):
        return ((lo_j[None, None, :, None] <= s) & (s <= hi_j[None, None, :, None])).astype(np.float32)


def mask_thresholds(n_pts, tint, sigma=3.0):
    """(lo, hi, lo_last, hi_last) as FxPlan.kurtosis_mask forms them when none is given: 1 -/+ sigma sqrt(mu2(M)) of a full bin
    and of the partial last bin's own count; (-inf, inf) below 2 frames"""
    import kurtosis_ref
    span = n_pts if tint == 0 else tint
    half = sigma * np.sqrt(kurtosis_ref.mu2(span))
    last = n_pts % span
    if last >= 2:
        h = sigma * np.sqrt(kurtosis_ref.mu2(last))
        return 1.0 - half, 1.0 + half, 1.0 - h, 1.0 + h
    return 1.0 - half, 1.0 + half, -np.inf, np.inf


# -- masks of the GPU tests -------------------------------------------------------------------------------------------------------
def n_mbin(n_pts, mask_tint):
    return int(mask_bin_of_frames(n_pts, mask_tint)[-1]) + 1


def random_mask(seed, n_chunks, n_ant, n_pts, nchan, mask_tint):
    """float32 [n_chunks, n_ant, n_mbin, nchan]: about 30 % zeros, the rest 1 -- with a few values that count (0.25, 7) and a few
    that do not (-1, NaN) --, plus one cell with every antenna out, one with all in, and one antenna out for a whole chunk (with a
    single chunk: for all of it but the all-in cell)"""
    rng = np.random.default_rng(seed)
    nb = n_mbin(n_pts, mask_tint)
    m = (rng.random((n_chunks, n_ant, nb, nchan)) >= 0.3).astype(np.float32)
    m[m > 0] = rng.choice(np.array([1.0, 1.0, 1.0, 0.25, 7.0], np.float32), size=int((m > 0).sum()))
    zeros = np.argwhere(m == 0)
    for row, v in zip(zeros[rng.choice(len(zeros), size=min(4, len(zeros)), replace=False)], (-1.0, np.nan, -0.0, -np.inf)):
        m[tuple(row)] = v
    cells = special_cells(n_chunks, nb, nchan)
    m[cells["none"][0], :, cells["none"][1], cells["none"][2]] = 0.0
    m[cells["chunk_out"][0], cells["chunk_out"][1] % n_ant] = 0.0
    m[cells["all"][0], :, cells["all"][1], cells["all"][2]] = 1.0           # (last: with one chunk the cell lies in the antenna's chunk)
    with np.errstate(invalid="ignore"):
        on = m > 0
    assert not on[cells["none"][0], :, cells["none"][1], cells["none"][2]].any()
    assert on[cells["all"][0], :, cells["all"][1], cells["all"][2]].all()
    out = on[cells["chunk_out"][0], cells["chunk_out"][1] % n_ant].copy()
    if cells["chunk_out"][0] == cells["all"][0]:
        out[cells["all"][1], cells["all"][2]] = False
    assert not out.any()
    expected = 0.3 + 0.7 / (n_chunks * n_ant)                              # the drawn zeros, and the antenna that is out for a chunk
    assert abs(1.0 - on.mean() - expected) < 0.15 or on.size < 64
    return m


def special_cells(n_chunks, nb, nchan):
    """(chunk, mask bin, stored channel) of the cell with every antenna out and of the cell with all in (the last bin, and on
    either side of the fftshift's wrap), and (chunk, antenna) of the antenna that is out for a whole chunk: the last chunk, so
    two chunks or more keep it off the two cells (with one chunk random_mask lets the all-in cell stand)"""
    return {"none": (0, nb - 1, nchan // 2), "all": (0, 0, max(nchan // 2 - 1, 0)), "chunk_out": (n_chunks - 1, 1)}


# -- the interference scenario ------------------------------------------------------------------------------------------------------
# beam_ref.gain_parts' samples (gains_ref.samples: x_a = c_a s + sigma n_a), 8 antennas x 64 channels x 128 frames x 4 chunks.
# Antenna RFI_ANT carries a tone centred on natural bin RFI_BIN that is on for the frames RFI_ON of every chunk: an eighth of the
# chunk, all inside the chunk's first time bin of RFI_TINT frames.  On-source weights (beam_ref.gain_weights, beam 0); time bins
# and mask bins of RFI_TINT frames.  The tone's level (its power in the bin over the bin's mean clean power in that antenna, while
# on) is chosen by tools/beam_mask_measure.py --bounds from RFI_LEVELS: the smallest that, for every seed of RFI_SEEDS, makes the
# spectral kurtosis of the restatement flag every affected cell and lifts the unmasked beam's power there to 10 x the clean beam's.
RFI_ANT, RFI_BIN, RFI_ON, RFI_TINT = 3, 21, (8, 24), 64
RFI_SEEDS = tuple(range(8))
RFI_LEVELS = tuple(float(2 ** k) for k in range(4, 20))
RFI_FACTOR = 10.0
RFI_MARGIN = 3.0          # beam_bounds.json's margin: eight seeds do not show the worst case


def rfi_window():
    import gains_ref
    from effex_amd.window import design_window
    return design_window(4, gains_ref.SAMPLE_NCHAN)


def rfi_case(seed):
    """-> clean x (complex64, the very samples of beam_ref.gain_parts), w [1, n_ant, nchan] on source, the unit tone [num_samp]
    (0 while off), window"""
    import gains_ref
    x, _, _, c = beam_ref.gain_parts(beam_ref.GAIN_ANT, seed)
    nchan, n_pts = gains_ref.SAMPLE_NCHAN, gains_ref.SAMPLE_SPECTRA
    n = np.arange(nchan * n_pts)
    frame = n // nchan
    tone = np.where((frame >= RFI_ON[0]) & (frame < RFI_ON[1]), np.exp(2j * np.pi * RFI_BIN * n / nchan), 0.0)
    return x, beam_ref.gain_weights(c, nchan)[:1], tone, rfi_window()


def rfi_amplitude(level, x, window):
    """the tone's amplitude for `level`: a tone of amplitude A centred on a bin reaches it as A sum(window)"""
    import gains_ref
    nchan = gains_ref.SAMPLE_NCHAN
    clean = (np.abs(beam_ref.spectra(x[:, RFI_ANT:RFI_ANT + 1], nchan, window)[:, 0, :, RFI_BIN]) ** 2).mean()
    return float(np.sqrt(level * clean) / abs(np.asarray(window, dtype=np.float64).sum()))


def rfi_dirty(x, tone, amplitude):
    out = np.array(x, dtype=np.complex128)
    out[:, RFI_ANT] += amplitude * tone
    return out.astype(np.complex64)


def rfi_cell():
    """(time bin, stored channel) of the affected cell of every chunk"""
    import gains_ref
    return RFI_ON[0] // RFI_TINT, (RFI_BIN + gains_ref.SAMPLE_NCHAN // 2) % gains_ref.SAMPLE_NCHAN


def rfi_figures(p_clean, p_dirty, p_masked, mask):
    """The scenario's three figures from beam powers [n_chunks, 1, n_tbin, nchan] and the mask [n_chunks, n_ant, n_tbin, nchan]:
    flagged = RFI_ANT is out in the affected cell of every chunk; factor = the smallest dirty / clean power over the affected
    cells; deviation = the largest |masked (n_ant / count)^2 - clean| / clean over ALL cells that keep an antenna (count > 0)"""
    j, k = rfi_cell()
    with np.errstate(invalid="ignore"):
        on = np.asarray(mask) > 0
    count = on.sum(axis=1).astype(np.float64)                                            # [n_chunks, n_tbin, nchan]
    flagged = bool((~on[:, RFI_ANT, j, k]).all())
    factor = float((p_dirty[:, 0, j, k] / p_clean[:, 0, j, k]).min())
    keep = count > 0
    scaled = p_masked[:, 0] * (on.shape[1] / np.where(keep, count, 1.0)) ** 2
    deviation = float((np.abs(scaled - p_clean[:, 0]) / p_clean[:, 0])[keep].max())
    return {"flagged": flagged, "factor": factor, "deviation": deviation, "cells_without_antennas": int((~keep).sum()),
            "count_in_cell": [int(v) for v in count[:, j, k]]}


def rfi_restatement(seed, level):
    """the scenario in float64 alone -> rfi_figures"""
    import gains_ref
    import kurtosis_ref
    nchan = gains_ref.SAMPLE_NCHAN
    x, w, tone, window = rfi_case(seed)
    dirty = rfi_dirty(x, tone, rfi_amplitude(level, x, window))
    f_clean, f_dirty = beam_ref.spectra(x, nchan, window), beam_ref.spectra(dirty, nchan, window)
    sk, _ = kurtosis_ref.kurtosis_of_spectra(f_dirty, RFI_TINT)
    mask = antenna_mask(sk, f_dirty.shape[2], RFI_TINT, *mask_thresholds(f_dirty.shape[2], RFI_TINT))
    return rfi_figures(power(f_clean, w, RFI_TINT), power(f_dirty, w, RFI_TINT), power(f_dirty, w, RFI_TINT, mask, RFI_TINT), mask)
