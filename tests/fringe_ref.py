"""Float64 restatement of the fringe fit's definition (include/fxcorr.h fxc_fringe_fit) and the model rows the fringe tests
fit: what tests/test_fringe_host.py checks on its own and tests/test_gpu_fringe.py holds the library to."""
import numpy as np

BW = 2.4e6
FC = 1.4204e9


def next_pow2(n):
    p = 1
    while p < n:
        p *= 2
    return p


def grid(nchan, n_chunks, pad):
    return next_pow2(pad * nchan), next_pow2(pad * n_chunks)


def cells(nchan, n_chunks, pad, bandwidth=BW, frequency=FC):
    """one grid cell in seconds of delay and in seconds per chunk of rate"""
    lk, lt = grid(nchan, n_chunks, pad)
    return nchan / (lk * bandwidth), 1.0 / (lt * frequency)


def _sub(a, b, c):
    la, lb, lc = np.log(a), np.log(b), np.log(c)
    return 0.5 * (la - lc) / (la - 2.0 * lb + lc)


def fit_baseline(R, bandwidth, frequency, pad):
    """R [n_chunks, nchan] of one baseline -> delay_s, rate_s_per_chunk, snr, (q0, m0)"""
    R = np.asarray(R, dtype=np.complex128)
    n_chunks, nchan = R.shape
    lk, lt = grid(nchan, n_chunks, pad)
    A = np.abs(np.fft.fft(np.fft.fft(R, lk, axis=1), lt, axis=0))
    q0, m0 = np.unravel_index(np.argmax(A), A.shape)
    dm = _sub(A[q0, (m0 - 1) % lk], A[q0, m0], A[q0, (m0 + 1) % lk])
    dq = _sub(A[(q0 - 1) % lt, m0], A[q0, m0], A[(q0 + 1) % lt, m0])
    m = m0 - lk if m0 >= lk // 2 else m0
    q = q0 - lt if q0 >= lt // 2 else q0
    snr = A[q0, m0] / np.sqrt((np.abs(R) ** 2).sum())
    return (m + dm) * nchan / (lk * bandwidth), (q + dq) / (lt * frequency), snr, (int(q0), int(m0))


def pairs(n_ant):
    return [(a, b) for a in range(n_ant) for b in range(a + 1, n_ant)]


def fit_rows(rows, n_ant, bandwidth, frequency, ref=0, pad=2):
    """rows [n_chunks, n_rows, nchan] -> delays [n_ant], rates [n_ant], snr [n_ant], peaks {b: (q0, m0)}"""
    index = {ab: i for i, ab in enumerate(pairs(n_ant))}
    delays, rates, snr, peaks = np.zeros(n_ant), np.zeros(n_ant), np.zeros(n_ant), {}
    for b in range(n_ant):
        if b == ref:
            continue
        R = rows[:, index[(ref, b)]] if ref < b else np.conj(rows[:, index[(b, ref)]])
        delays[b], rates[b], snr[b], peaks[b] = fit_baseline(R, bandwidth, frequency, pad)
    return delays, rates, snr, peaks


def bin_frequencies(nchan, bandwidth=BW, frequency=FC):
    return np.fft.fftshift(np.fft.fftfreq(nchan, 1.0 / bandwidth)) + frequency


def model_baseline(n_chunks, nchan, delay, rate, snr_in, rng, bandwidth=BW, frequency=FC):
    """snr_in exp(2 pi i f_j (delay + t rate)) + unit complex noise, [n_chunks, nchan] complex128"""
    f = bin_frequencies(nchan, bandwidth, frequency)
    t = np.arange(n_chunks)[:, None]
    ph = f[None, :] * (delay + t * rate)
    noise = (rng.standard_normal(ph.shape) + 1j * rng.standard_normal(ph.shape)) / np.sqrt(2.0)
    return snr_in * np.exp(2j * np.pi * (ph - np.rint(ph))) + noise


def model_rows(n_chunks, n_ant, nchan, delays, rates, snr_in, rng, bandwidth=BW, frequency=FC):
    """cross rows [n_chunks, n_base, nchan] complex64 of antennas with residual delays D_a(t) = delays[a] + t rates[a]:
    row (a, b) = snr_in exp(+2 pi i f_j (D_b(t) - D_a(t))) + noise"""
    pr = pairs(n_ant)
    out = np.empty((n_chunks, len(pr), nchan), np.complex64)
    for i, (a, b) in enumerate(pr):
        out[:, i] = model_baseline(n_chunks, nchan, delays[b] - delays[a], rates[b] - rates[a], snr_in, rng, bandwidth, frequency)
    return out


def draw_antennas(n_ant, nchan, rng, span=0.4, bandwidth=BW, frequency=FC):
    """per-antenna residuals whose differences stay within `span` of the unambiguous ranges"""
    delays = rng.uniform(-0.5 * span, 0.5 * span, n_ant) * nchan / bandwidth
    rates = rng.uniform(-0.5 * span, 0.5 * span, n_ant) / frequency
    return delays, rates
