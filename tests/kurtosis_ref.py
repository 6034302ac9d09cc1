"""Float64 restatement of the spectral kurtosis estimator's definition (include/fxcorr.h fxc_kurtosis, fxc_kurtosis_weights): what
tests/test_kurtosis_host.py checks on its own and tests/test_gpu_kurtosis.py holds the library to.  Spectra come from
fx_oracle.spectrometer_poly per antenna and chunk; the time bins, the estimator, its special cases, the fftshift and the weights
rule are written as the header defines them."""
import numpy as np

import fx_oracle


def mu2(M):
    """the estimator's variance over M spectra of Gaussian noise (Nita & Gary 2010)"""
    M = float(M)
    return 4.0 * M * M / ((M - 1.0) * (M + 2.0) * (M + 3.0))


def pairs(n_ant):
    return [(a, b) for a in range(n_ant) for b in range(a + 1, n_ant)]


def time_bins(n_pts, tint):
    """[(first frame, end frame)]: tint frames a bin, 0 = the whole chunk; the last bin may be partial"""
    span = n_pts if tint == 0 else tint
    return [(i, min(i + span, n_pts)) for i in range(0, n_pts, span)]


def spectra(x, nchan, window):
    """x [n_chunks, n_ant, num_samp] -> f [n_chunks, n_ant, n_pts, nchan] complex128, natural bin order"""
    x = np.asarray(x)
    ntaps = len(window) // nchan
    return np.stack([np.stack([fx_oracle.spectrometer_poly(x[c, a], ntaps, nchan, window) for a in range(x.shape[1])])
                     for c in range(x.shape[0])])


def kurtosis_of_spectra(f, tint=0):
    """f [n_chunks, n_ant, n_pts, nchan] -> (sk, power) float64 [n_chunks, n_ant, n_tbin, nchan], bins fftshifted.  In this order:
    a bin of fewer than 2 frames has sk 1; sums that are not finite give NaN; S1 == 0 gives 0"""
    p = np.abs(np.asarray(f)) ** 2
    sk, power = [], []
    with np.errstate(all="ignore"):
        for i0, i1 in time_bins(p.shape[2], tint):
            m = float(i1 - i0)
            s1, s2 = p[:, :, i0:i1].sum(axis=2), (p[:, :, i0:i1] ** 2).sum(axis=2)
            power.append(s1 / m)
            if i1 - i0 < 2:
                sk.append(np.ones_like(s1))
                continue
            v = (m + 1.0) / (m - 1.0) * (m * s2 / np.where(s1 == 0, 1.0, s1) ** 2 - 1.0)
            v = np.where(s1 == 0, 0.0, v)
            sk.append(np.where(np.isfinite(s1) & np.isfinite(s2), v, np.nan))
    return np.fft.fftshift(np.stack(sk, axis=2), axes=-1), np.fft.fftshift(np.stack(power, axis=2), axes=-1)


def kurtosis(x, nchan, window, tint=0):
    return kurtosis_of_spectra(spectra(x, nchan, window), tint)


def counted_bins(n_pts, tint):
    """the bins the weights rule looks at: all but a partial last bin that is not the only bin of its chunk"""
    bins = time_bins(n_pts, tint)
    full = bins[0][1] - bins[0][0]
    if len(bins) > 1 and bins[-1][1] - bins[-1][0] != full:
        return len(bins) - 1
    return len(bins)


def weights(sk, n_pts, tint, lo, hi):
    """sk [n_chunks, n_ant, n_tbin, nchan] (any float type; compared as float64) -> float32 [n_chunks, n_baselines, nchan]: 1 iff
    lo <= sk <= hi in every counted bin of both antennas -- comparisons, so a NaN gives 0"""
    s = np.asarray(sk).astype(np.float64)[:, :, :counted_bins(n_pts, tint)]
    with np.errstate(invalid="ignore"):
        good = ((float(lo) <= s) & (s <= float(hi))).all(axis=2)          # [n_chunks, n_ant, nchan]
    n_ant = s.shape[1]
    out = np.zeros((s.shape[0], len(pairs(n_ant)), s.shape[3]), np.float32)
    for i, (a, b) in enumerate(pairs(n_ant)):
        out[:, i] = (good[:, a] & good[:, b]).astype(np.float32)
    return out


# -- inputs ---------------------------------------------------------------------------------------------------------------------
HIT_ANT = 1           # the antenna the interference is in
TONE_LEVEL = 30.0     # the tones' power in their bin over the bin's noise power, while they are on
PULSE = (4, 12)       # the second tone is on for the samples of frames [4, 12) of every 64


def noise(seed, n_chunks, n_ant, num_samp):
    """complex Gaussian noise of unit variance, complex128: a flat spectrum"""
    rng = np.random.default_rng(seed)
    shape = (n_chunks, n_ant, num_samp)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)


def tone_bins(nchan):
    """natural-order bins of the steady and of the pulsed tone"""
    return nchan // 4, nchan // 2 + nchan // 8


def shifted(k, nchan):
    """where natural bin k is stored"""
    return (k + nchan // 2) % nchan


def tones(window, nchan, n_chunks, num_samp, level=TONE_LEVEL):
    """[n_chunks, num_samp] complex128: a steady tone centred on bin tone_bins()[0] and one on bin tone_bins()[1] that is on for
    8 frames of every 64, each `level` times the bin's noise power (unit-variance noise: sum w^2) in the bin while on (a tone of
    amplitude A centred on a bin reaches it as A sum w)"""
    window = np.asarray(window, dtype=np.float64)
    amp = np.sqrt(level * (window ** 2).sum()) / abs(window.sum())
    n = np.arange(num_samp)
    k1, k2 = tone_bins(nchan)
    frame = (n // nchan) % 64
    on = (frame >= PULSE[0]) & (frame < PULSE[1])
    t = amp * np.exp(2j * np.pi * k1 * n / nchan) + amp * on * np.exp(2j * np.pi * k2 * n / nchan)
    return np.broadcast_to(t, (n_chunks, num_samp))


def case(seed, n_ant, nchan, ntaps, n_pts, n_chunks, with_tones=True):
    """-> x [n_chunks, n_ant, num_samp] complex128 (noise, the tones in antenna HIT_ANT), window"""
    from effex_amd.window import design_window
    window = design_window(ntaps, nchan)
    x = noise(seed, n_chunks, n_ant, nchan * n_pts)
    if with_tones:
        x[:, min(HIT_ANT, n_ant - 1)] += tones(window, nchan, n_chunks, nchan * n_pts)
    return x, window


# the statistical input of the issue: 2 antennas x 64 channels x 4 taps, M = 64 frames
STAT_SHAPE = (2, 64, 4, 64, 4)      # n_ant, nchan, ntaps, n_pts, n_chunks
STAT_SEEDS = tuple(range(8))


def noise_statistics(seed):
    """-> (|mean sk - 1|, |var sk / mu2(64) - 1|, share outside the default thresholds) of clean noise, one seed"""
    n_ant, nchan, ntaps, n_pts, n_chunks = STAT_SHAPE
    x, window = case(seed, n_ant, nchan, ntaps, n_pts, n_chunks, with_tones=False)
    sk, _ = kurtosis(x, nchan, window)
    half = 3.0 * np.sqrt(mu2(n_pts))
    return (float(abs(sk.mean() - 1.0)), float(abs(sk.var() / mu2(n_pts) - 1.0)),
            float(((sk < 1.0 - half) | (sk > 1.0 + half)).mean()))
