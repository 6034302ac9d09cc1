"""Numpy restatement of the detector's definition (include/fxcorr.h fxc_flag_rows), term for term, with the float32 / float64
casts where the definition has them: what tests/test_flag_host.py checks on its own and tests/test_gpu_flag.py holds the library
to, bit for bit.  A lower median is an element of its set, so sorting here and selecting on the device give the same bits."""
import numpy as np

F32 = np.float32


def windows(n_chunks, window):
    """[(first chunk, end chunk)] of the windows; window 0 is one over all chunks"""
    span = n_chunks if window == 0 else window
    return [(c, min(c + span, n_chunks)) for c in range(0, n_chunks, span)]


def lower_median(values, valid, axis):
    """the element at index (m - 1) // 2 of the ascending order of the m valid values along ``axis`` (garbage where m == 0).
    The values that are not valid are replaced before anything looks at them; a valid NaN (inf - inf in the frequency stage)
    sorts last, as its bit pattern does on the device."""
    v = np.where(valid, values, F32(np.nan)).astype(F32)
    v = np.sort(np.moveaxis(v, axis, -1), axis=-1)
    m = np.moveaxis(valid, axis, -1).sum(axis=-1)
    idx = np.where(m > 0, (m - 1) // 2, 0)
    return np.take_along_axis(v, idx[..., None], axis=-1)[..., 0]


def deviations(x, y, live):
    """-> mx, my [nb, nchan] and e [n, nb, nchan] float32 of the live samples (0 where not live)"""
    mx, my = lower_median(x, live, 0), lower_median(y, live, 0)
    with np.errstate(over="ignore", invalid="ignore"):
        dx = np.where(live, x, F32(0)) - np.where(live, mx[None], F32(0))          # ONE float32 subtraction each
        dy = np.where(live, y, F32(0)) - np.where(live, my[None], F32(0))
        dx64, dy64 = dx.astype(np.float64), dy.astype(np.float64)
        e = (dx64 * dx64 + dy64 * dy64).astype(F32)                                  # exact products, one rounding
    return mx, my, e


def sliding(values, defined, half_width):
    """values, defined [nb, nchan] -> (window values, window validity) [nb, nchan, 2 h + 1]: bin k's window holds the bins j with
    |j - k| <= half_width inside the band"""
    h = min(int(half_width), values.shape[1] - 1)       # a wider window holds the same bins
    pv = np.pad(np.where(defined, values, F32(0)).astype(F32), ((0, 0), (h, h)))
    pd = np.pad(defined, ((0, 0), (h, h)))
    view = np.lib.stride_tricks.sliding_window_view
    return view(pv, 2 * h + 1, axis=1), view(pd, 2 * h + 1, axis=1)


def frequency_outliers(level, scatter, defined, freq_threshold, half_width):
    """-> outlier [nb, nchan] bool, every decision from the planes as the time stage left them"""
    thr = F32(freq_threshold)
    out = np.zeros(level.shape, bool)
    for plane, two_sided in ((level, True), (scatter, False)):
        win, valid = sliding(plane, defined, half_width)
        r = lower_median(win, valid, -1)
        with np.errstate(invalid="ignore", over="ignore"):
            dev = np.abs((win - r[..., None]).astype(F32))
            s = lower_median(dev, valid, -1)
            diff = (np.where(defined, plane, F32(0)) - r).astype(F32)
            if two_sided:
                diff = np.abs(diff)
            out |= defined & (s > 0) & (diff > thr * s)
    return out


def flag_window(rows, prior, time_threshold, freq_threshold, half_width, iters):
    """rows [n, nb, nchan] complex64 and prior [n, nb, nchan] float32 (or None) of one window -> weights [n, nb, nchan] float32,
    counts [nb, 3] int64"""
    x, y = np.ascontiguousarray(rows.real, F32), np.ascontiguousarray(rows.imag, F32)
    live = np.isfinite(x) & np.isfinite(y) & ~((x == 0) & (y == 0))
    if prior is not None:
        with np.errstate(invalid="ignore"):
            live &= prior > 0
    counts = np.zeros((rows.shape[1], 3), np.int64)
    counts[:, 0] = (~live).sum(axis=(0, 2))
    thr = F32(time_threshold)
    for _ in range(iters):
        _, _, e = deviations(x, y, live)
        d = lower_median(e, live, 0)
        with np.errstate(invalid="ignore", over="ignore"):
            flagged = live & (d > 0)[None] & (e > (thr * d)[None])                  # one float32 multiply and a comparison
        counts[:, 1] += flagged.sum(axis=(0, 2))
        live &= ~flagged
    defined = live.any(axis=0)
    mx, my, e = deviations(x, y, live)
    with np.errstate(over="ignore", invalid="ignore"):
        mx64, my64 = mx.astype(np.float64), my.astype(np.float64)
        level = np.where(defined, (mx64 * mx64 + my64 * my64).astype(F32), F32(0))
    scatter = np.where(defined, lower_median(e, live, 0), F32(0))
    out = frequency_outliers(level, scatter, defined, freq_threshold, half_width)
    cleared = live & out[None]
    counts[:, 2] = cleared.sum(axis=(0, 2))
    live &= ~cleared
    weights = np.where(live, F32(1) if prior is None else prior, F32(0)).astype(F32)
    return weights, counts


def flag_rows(rows, n_baselines=None, window=0, time_threshold=20.0, freq_threshold=8.0, half_width=8, iters=2, prior=None,
              return_counts=False):
    """rows [n_chunks, n_rows, nchan] complex64 (or [n_rows, nchan]: one chunk; only the first n_baselines rows of a chunk are
    read, default all of them), prior [n_chunks, n_baselines, nchan] float32 or None -> weights [n_chunks, n_baselines, nchan]
    float32 and, with return_counts, counts [n_win, n_baselines, 3] int64"""
    rows = np.asarray(rows)
    one = rows.ndim == 2
    if one:
        rows = rows[None]
        prior = None if prior is None else np.asarray(prior)[None]
    nb = rows.shape[1] if n_baselines is None else n_baselines
    rows = rows[:, :nb].astype(np.complex64)
    if prior is not None:
        prior = np.asarray(prior, F32)
    weights = np.zeros(rows.shape, F32)
    counts = []
    for c0, c1 in windows(rows.shape[0], int(window)):
        w, n = flag_window(rows[c0:c1], None if prior is None else prior[c0:c1], time_threshold, freq_threshold, half_width, iters)
        weights[c0:c1] = w
        counts.append(n)
    if one:
        weights = weights[0]
    return (weights, np.stack(counts)) if return_counts else weights
