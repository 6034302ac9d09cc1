"""numpy restatement of the dedispersion (include/fxcorr.h fxc_dedisperse) with exactly its order of additions, a
float64 truth, and the pulse case both test modules use.  Nothing here imports the library."""
import numpy as np

SEGMENT = 64                     # channels of a float32 segment sum
DM_CONSTANT_S = 4.148808e3       # s per unit DM at 1 MHz

# the wide band of the issue's prototype: 64 channels, 400 MHz at 600 MHz, 1 ms samples, trials 0, 2.5, .., 20 (shifts up to 387)
WIDE_NCHAN, WIDE_BW, WIDE_FC, WIDE_TSAMP = 64, 400e6, 600e6, 1e-3
WIDE_DMS = np.arange(9) * 2.5
PULSE_SEEDS = tuple(range(8))
PULSE_CHUNKS, PULSE_SERIES, PULSE_TBIN = 8, 2, 128
PULSE_DM_INDEX, PULSE_T0, PULSE_SERIES_AT = 4, 300, 1      # DM 10, in series 1 only


def freqs(nchan, bandwidth, frequency):
    return np.fft.fftshift(np.fft.fftfreq(nchan, d=1.0 / bandwidth)) + frequency


def shifts_formula(nchan, bandwidth, frequency, dms, tsamp):
    """dm_shifts from its definition, channel by channel"""
    f = freqs(nchan, bandwidth, frequency) / 1e6
    out = np.zeros((len(dms), nchan), np.int32)
    for d, dm in enumerate(dms):
        for k in range(nchan):
            out[d, k] = int(np.rint(DM_CONSTANT_S * float(dm) * (f[k] ** -2.0 - f.max() ** -2.0) / tsamp))
    return out


def series(power):
    """[n_chunks, n_series, n_tbin, nchan] (or 3-D / 2-D: one chunk) -> the time series [n_series, n_t, nchan]"""
    power = np.asarray(power)
    if power.ndim == 2:
        power = power[None]
    if power.ndim == 3:
        return power
    n_chunks, n_series, n_tbin, nchan = power.shape
    return power.transpose(1, 0, 2, 3).reshape(n_series, n_chunks * n_tbin, nchan)


def counted_channels(nchan, chan_weights):
    if chan_weights is None:
        return np.ones(nchan, bool)
    with np.errstate(invalid="ignore"):
        return np.asarray(chan_weights) > 0          # a NaN does not count


def column(ts, k, shift, n_out):
    """the samples channel k contributes to the outputs 0 .. n_out - 1 at this shift, [n_series, n_out]"""
    return ts[:, shift:shift + n_out, k]


def dedisperse(power, shifts, chan_weights=None, column=column, counted=None):
    """-> float32 [n_series, n_dm, n_t - shifts.max()]: per segment of 64 channels a float32 sum from +0 over the counted channels in
    ascending order, the segments' sums added in float64 in segment order, one rounding.  ``column`` and ``counted`` are the hooks of
    the mutations in tests/test_dedisperse_host.py."""
    ts = series(power)
    assert ts.dtype == np.float32
    shifts = np.asarray(shifts)
    n_series, n_t, nchan = ts.shape
    n_dm = shifts.shape[0]
    assert shifts.shape == (n_dm, nchan) and shifts.min() >= 0
    n_out = n_t - int(shifts.max())
    assert n_out >= 1
    if counted is None:
        counted = counted_channels(nchan, chan_weights)
    out = np.zeros((n_series, n_dm, n_out), np.float32)
    with np.errstate(all="ignore"):
        for d in range(n_dm):
            total = np.zeros((n_series, n_out), np.float64)
            for k0 in range(0, nchan, SEGMENT):
                acc = np.zeros((n_series, n_out), np.float32)
                for k in range(k0, min(nchan, k0 + SEGMENT)):
                    if counted[k]:
                        acc = acc + column(ts, k, int(shifts[d, k]), n_out)
                        assert acc.dtype == np.float32
                total = total + acc.astype(np.float64)
            out[:, d] = total.astype(np.float32)
    return out


def truth(power, shifts, chan_weights=None):
    """-> (the sums in float64, sum |P| per cell), both [n_series, n_dm, n_out]"""
    ts = series(power).astype(np.float64)
    shifts = np.asarray(shifts)
    n_series, n_t, nchan = ts.shape
    n_out = n_t - int(shifts.max())
    counted = counted_channels(nchan, chan_weights)
    val = np.zeros((n_series, shifts.shape[0], n_out))
    mag = np.zeros_like(val)
    for d in range(shifts.shape[0]):
        for k in np.nonzero(counted)[0]:
            col = ts[:, shifts[d, k]:shifts[d, k] + n_out, k]
            val[:, d] += col
            mag[:, d] += np.abs(col)
    return val, mag


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def wide_shifts(dms=WIDE_DMS, nchan=WIDE_NCHAN, tsamp=WIDE_TSAMP):
    return shifts_formula(nchan, WIDE_BW, WIDE_FC, dms, tsamp)


def pulse_case(seed):
    """chi-square noise of 32 degrees of freedom with unit mean, 8 chunks x 2 series x 128 bins x 64 channels, plus a pulse of
    height 1 in every channel of series 1 along the DM 10 sweep from t0 -> (power, shifts)"""
    rng = np.random.default_rng(seed)
    shifts = wide_shifts()
    power = (rng.chisquare(32, (PULSE_CHUNKS, PULSE_SERIES, PULSE_TBIN, WIDE_NCHAN)) / 32.0).astype(np.float32)
    for k in range(WIDE_NCHAN):
        t = PULSE_T0 + int(shifts[PULSE_DM_INDEX, k])
        power[t // PULSE_TBIN, PULSE_SERIES_AT, t % PULSE_TBIN, k] += np.float32(1.0)
    return power, shifts


def pulse_figures(out, n_counted=WIDE_NCHAN):
    """-> (argmax cell, the excess over the expected sum at the true cell / the best excess of the DM 0 series)"""
    cell = tuple(int(i) for i in np.unravel_index(np.argmax(out), out.shape))
    excess = out.astype(np.float64) - n_counted
    return cell, excess[PULSE_SERIES_AT, PULSE_DM_INDEX, PULSE_T0] / excess[:, 0].max()


def loud_power(rng, shape):
    """a loud asymmetric input: every series, chunk and channel on a scale of its own, every sample distinct"""
    n = int(np.prod(shape))
    ramp = (1.0 + np.arange(n, dtype=np.float64).reshape(shape) / n)
    scale = 1.0 + 3.0 * rng.random(shape[:-2] + (1, shape[-1])) if len(shape) > 2 else 1.0
    return (ramp * scale * (0.5 + rng.random(shape))).astype(np.float32)
