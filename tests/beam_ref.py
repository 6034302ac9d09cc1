"""Float64 restatement of the beamformer's definition (include/fxcorr.h fxc_beamform): what tests/test_beam_host.py checks on its
own and tests/test_gpu_beamform.py holds the library to.  Spectra come from fx_oracle.spectrometer_poly per antenna and chunk;
the sum over antennas, the time bins and the fftshift are written as the header defines them."""
import numpy as np

import fx_oracle


def pairs(n_ant):
    return [(a, b) for a in range(n_ant) for b in range(a + 1, n_ant)]


def spectra(x, nchan, window):
    """x [n_chunks, n_ant, num_samp] -> f [n_chunks, n_ant, n_pts, nchan] complex128, natural bin order"""
    x = np.asarray(x)
    ntaps = len(window) // nchan
    return np.stack([np.stack([fx_oracle.spectrometer_poly(x[c, a], ntaps, nchan, window) for a in range(x.shape[1])])
                     for c in range(x.shape[0])])


def weights_3d(w):
    w = np.asarray(w, dtype=np.complex128)
    return w[None] if w.ndim == 2 else w


def voltages(f, w, tables=None):
    """y[c, b, i, k] = sum_a w[b, a, k] rho[c, a, k] f[c, a, i, k]; tables = rho [n_chunks, n_ant, nchan] or None (1)"""
    w = weights_3d(w)
    rho = np.ones((f.shape[0],) + w.shape[1:], np.complex128) if tables is None else np.asarray(tables, dtype=np.complex128)
    return np.einsum("bak,cak,caik->cbik", w, rho, f)


def time_bins(n_pts, tint):
    """[(first frame, end frame)]: tint frames a bin, 0 = the whole chunk; the last bin may be partial"""
    span = n_pts if tint == 0 else tint
    return [(i, min(i + span, n_pts)) for i in range(0, n_pts, span)]


def power(y, tint=0):
    """y [n_chunks, n_beam, n_pts, nchan] -> [n_chunks, n_beam, n_tbin, nchan] float64: fftshift_k of the mean of |y|^2 over each
    time bin, every bin divided by its own count"""
    p = np.abs(y) ** 2
    out = np.stack([p[:, :, i0:i1].sum(axis=2) / float(i1 - i0) for i0, i1 in time_bins(y.shape[2], tint)], axis=2)
    return np.fft.fftshift(out, axes=-1)


def beamform(x, w, nchan, window, tint=0, mode="POWER", tables=None):
    y = voltages(spectra(x, nchan, window), w, tables)
    return power(y, tint) if mode.upper() == "POWER" else y


def autos_of(x, nchan, window):
    """The autos restatement of tests/test_gpu_autos.py over all chunks: A[a] = fftshift(mean over chunks and frames of |f_a|^2)"""
    f = spectra(x, nchan, window)
    return np.fft.fftshift((np.abs(f) ** 2).mean(axis=(0, 2)), axes=-1)


def expansion(w, autos, cross):
    """The beam power from the visibilities, every operand in the rows' fftshifted order: w [n_beam, n_ant, nchan] NATURAL order
    (shifted here), autos A [.., n_ant, nchan], cross V [.., n_baselines, nchan] with V_ab = <f_a conj(f_b)> ->
    P_b = sum_a |w_a|^2 A_a + 2 Re sum_{a < b'} w_a conj(w_b') V_ab'   as [.., n_beam, nchan]"""
    ws = np.fft.fftshift(weights_3d(w), axes=-1)
    autos, cross = np.asarray(autos), np.asarray(cross)
    n_ant = ws.shape[1]
    out = []
    for wb in ws:
        p = sum((np.abs(wb[a]) ** 2) * autos[..., a, :].real for a in range(n_ant))
        for i, (a, b) in enumerate(pairs(n_ant)):
            p = p + 2.0 * (wb[a] * np.conj(wb[b]) * cross[..., i, :]).real
        out.append(p)
    return np.stack(out, axis=-2)


# -- inputs of the GPU tests ----------------------------------------------------------------------------------------------------
def noise_and_source(seed, n_chunks, n_ant, num_samp, amplitude=0.5):
    """standard-normal noise per antenna plus a common source at `amplitude`: no beam of random weights cancels to nothing"""
    rng = np.random.default_rng(seed)
    shape = (n_chunks, n_ant, num_samp)
    n = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)
    s = (rng.standard_normal((n_chunks, 1, num_samp)) + 1j * rng.standard_normal((n_chunks, 1, num_samp))) / np.sqrt(2.0)
    return (n + amplitude * s).astype(np.complex64)


def random_weights(seed, n_beam, n_ant, nchan):
    """unit-scale complex weights, complex64"""
    rng = np.random.default_rng(seed)
    shape = (n_beam, n_ant, nchan)
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)).astype(np.complex64)


# more frames than a frame range of the kernel, (n_ant, nchan, ntaps, n_pts, n_chunks, n_beam) -- tests/test_gpu_beamform.py says what
# each is for.  Their window is window_cases.rough_window: a chunk's first frame meets data through the window's last taps alone, the
# designed window's smallest, and a first frame lost or doubled would hide under the bounds; with independent taps it counts
LONG_SHAPES = [(3, 64, 4, 37, 2, 3), (2, 16, 4, 70, 2, 9), (9, 63, 4, 37, 2, 5), (4, 32, 4, 37, 2, 2)]


def shape_case(shape):
    """-> x, w, window of a shape of the GPU test"""
    import window_cases
    from effex_amd.window import design_window
    n_ant, nchan, ntaps, n_pts, n_chunks, n_beam = shape
    x = noise_and_source(1000 * n_ant + nchan + n_beam, n_chunks, n_ant, nchan * n_pts)
    w = random_weights(17 * n_ant + n_beam, n_beam, n_ant, nchan)
    window = window_cases.rough_window(ntaps, nchan) if tuple(shape) in LONG_SHAPES else design_window(ntaps, nchan)
    return x, w, window


def tints_of(n_pts):
    """frames per time bin that the GPU test gives a shape: the whole chunk (0 and n_pts), single frames, 3; 5 and 33 where the chunk
    has as many; and n_pts - 1, one full bin and a bin of one frame, each a frame range of its own"""
    return sorted({0, 1, 3, n_pts, n_pts - 1} | {t for t in (5, 33) if t <= n_pts})


# -- coherent gain ----------------------------------------------------------------------------------------------------------------
# gains_ref.samples: x_a = c_a s + sigma n_a.  The beamformer is linear in x, so the source's and the noise's shares of a beam are
# the beams of the two parts alone.  With w_a = conj(c_a) / |c_a|^2 / n_ant the on-source beam is s + (sigma / n_ant) sum_a n_a /
# c_a: its source-to-noise power ratio R obeys 1 / R = (1 / n_ant^2) sum_a 1 / R_a with R_a = |c_a|^2 / sigma^2 antenna a's own
# ratio (the beam of w = conj(c_a) / |c_a|^2 on antenna a alone) -- n_ant times one antenna's where the antennas are alike, n_ant
# times their harmonic mean in general -- up to the noise's cross terms, which average away.
GAIN_ANT = 8
GAIN_CHUNKS = 4
GAIN_SEEDS = tuple(range(8))


def gain_parts(n_ant, seed, n_chunks=GAIN_CHUNKS):
    """gains_ref.samples' draws again, kept apart: -> x (the very samples), source part, noise part, c"""
    import gains_ref
    rng = np.random.default_rng(seed)
    c = gains_ref.draw_scalars(n_ant, rng)
    n = gains_ref.SAMPLE_NCHAN * gains_ref.SAMPLE_SPECTRA
    s = (rng.standard_normal((n_chunks, 1, n)) + 1j * rng.standard_normal((n_chunks, 1, n))) / np.sqrt(2.0)
    w = (rng.standard_normal((n_chunks, n_ant, n)) + 1j * rng.standard_normal((n_chunks, n_ant, n))) / np.sqrt(2.0)
    src, noise = c[None, :, None] * s, gains_ref.SAMPLE_NOISE * w
    return (src + noise).astype(np.complex64), src, noise, c


def gain_weights(c, nchan):
    """-> [1 + n_ant, n_ant, nchan] complex128: the on-source beam, then antenna a alone with w = conj(c_a) / |c_a|^2"""
    n_ant = len(c)
    inv = np.conj(c) / np.abs(c) ** 2
    w = np.zeros((1 + n_ant, n_ant, nchan), np.complex128)
    w[0] = (inv / n_ant)[:, None]
    for a in range(n_ant):
        w[1 + a, a] = inv[a]
    return w


def gain_deviation(p_src, p_noise):
    """p_src, p_noise [n_chunks, 1 + n_ant, n_tbin, nchan]: the beams of gain_weights on the two parts ->
    | R_0 (1 / n_ant^2) sum_a 1 / R_a - 1 | with R = mean source power / mean noise power of a beam"""
    r = p_src.mean(axis=(0, 2, 3)) / p_noise.mean(axis=(0, 2, 3))
    n_ant = len(r) - 1
    return float(abs(r[0] * (1.0 / r[1:]).sum() / n_ant ** 2 - 1.0))
