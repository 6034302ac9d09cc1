"""Whole-sample delays in numpy: the restatement the tests of tests/test_align_host.py and tests/test_gpu_align.py compare
with (include/fxcorr.h fxc_set_sample_delays / fxc_set_delay_track_aligned).  It shares no code with effex_amd/plan.py."""
import numpy as np

import fx_oracle


def align(x, shifts):
    """out[c, a, n] = x[c, a, n + s] when 0 <= n + s < num_samp, exactly 0 otherwise; every chunk on its own.  ``shifts`` is
    [n_ant] or [n_chunks, n_ant]."""
    x = np.asarray(x)
    n_chunks, n_ant, num_samp = x.shape
    shifts = np.broadcast_to(np.asarray(shifts, dtype=np.int64), (n_chunks, n_ant))
    out = np.zeros_like(x)
    for c in range(n_chunks):
        for a in range(n_ant):
            s = int(shifts[c, a])
            if s >= num_samp or s <= -num_samp:
                continue
            if s >= 0:
                out[c, a, :num_samp - s] = x[c, a, s:]
            else:
                out[c, a, -s:] = x[c, a, :num_samp + s]
    return out


def tables(nchan, bandwidth, frequency, delays_s, shifts, slope_sign=1):
    """[n_ant, nchan] complex128, natural bin order: kk the integer bin index of np.fft.fftfreq, f_k = kk df + frequency,
    u = f_k tau - rint(f_k tau), m = (kk s) mod nchan (non-negative, exact in integers), v = u - m / nchan,
    r[k] = exp(2 pi i (v - rint(v))).  ``slope_sign`` -1: the mutation of tests/test_align_host.py."""
    tau = np.asarray(delays_s, dtype=np.float64).reshape(-1)
    shifts = np.asarray(shifts, dtype=np.int64).reshape(-1)
    df = 1.0 / (nchan * (1.0 / bandwidth))
    out = np.empty((len(tau), nchan), dtype=np.complex128)
    for a in range(len(tau)):
        for k in range(nchan):
            kk = k if k < (nchan + 1) // 2 else k - nchan
            f = kk * df + frequency
            turns = f * tau[a]
            u = turns - np.rint(turns)
            m = (kk * int(shifts[a])) % nchan          # Python integers: exact, non-negative
            v = u - slope_sign * (m / nchan)
            w = v - np.rint(v)
            out[a, k] = complex(np.cos(2 * np.pi * w), np.sin(2 * np.pi * w))
    return out


def track_shifts(tau0, rate, bandwidth, t):
    """s_a(t) = rint((tau0[a] + t rate[a]) bandwidth): ties to even, every operation rounded on its own."""
    tau = np.asarray(tau0, dtype=np.float64) + float(int(t)) * np.asarray(rate, dtype=np.float64)
    return np.rint(tau * float(bandwidth)).astype(np.int64)


def rows(x, nchan, window, rots, autos=False):
    """The float64 oracle's rows of samples that are already aligned: x [n_chunks, n_ant, num_samp], rots [n_ant, nchan] or
    [n_chunks, n_ant, nchan] -> [n_chunks, n_rows, nchan] complex128, row (a, b) = fftshift(mean(spec_a r_a conj(spec_b r_b)))."""
    x = np.asarray(x)
    n_chunks, n_ant, _ = x.shape
    rots = np.broadcast_to(np.asarray(rots), (n_chunks, n_ant, nchan))
    ntaps = len(window) // nchan
    pairs = [(a, b) for a in range(n_ant) for b in range(a + 1, n_ant)]
    out = np.zeros((n_chunks, len(pairs) + (n_ant if autos else 0), nchan), np.complex128)
    for c in range(n_chunks):
        spec = [fx_oracle.spectrometer_poly(x[c, a], ntaps, nchan, window) for a in range(n_ant)]
        for p, (a, b) in enumerate(pairs):
            out[c, p] = np.fft.fftshift((spec[a] * rots[c, a] * np.conj(spec[b] * rots[c, b])).mean(axis=0))
        if autos:
            for a in range(n_ant):
                out[c, len(pairs) + a] = np.fft.fftshift((np.abs(spec[a]) ** 2).mean(axis=0))
    return out
