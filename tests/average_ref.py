"""Numpy restatement of the averager's definition (include/fxcorr.h fxc_average_rows), term for term, with the float32 / float64
casts where the definition has them: what tests/test_average_host.py checks on its own and tests/test_gpu_average.py holds the
library to, bit for bit.  Every sum is a loop of plain float64 adds in the definition's order; nothing is handed to numpy's own
(pairwise) summation."""
import numpy as np

F32 = np.float32


def intervals(n_chunks, time_bin):
    """[(first chunk, end chunk)] of the intervals; time_bin 0, or one beyond the chunks, is one interval over all of them"""
    span = n_chunks if time_bin == 0 else min(time_bin, n_chunks)
    return [(c, min(c + span, n_chunks)) for c in range(0, n_chunks, span)]


def sums(rows, weights):
    """rows [n, nb, nchan] complex64 and weights [n, nb, nchan] float32 (or None: every weight 1) of one interval -> Sx, Sy, W
    [nb, nchan] float64: chunk after chunk from 0.  A sample counts iff its weight is > 0; the value of one that does not is
    replaced before anything looks at it."""
    n, nb, nchan = rows.shape
    sx, sy, w_sum = (np.zeros((nb, nchan), np.float64) for _ in range(3))
    for c in range(n):
        x, y = rows[c].real.astype(F32), rows[c].imag.astype(F32)
        if weights is None:
            w, ok = np.ones((nb, nchan), F32), np.ones((nb, nchan), bool)
        else:
            w = np.asarray(weights[c], F32)
            with np.errstate(invalid="ignore"):
                ok = w > 0
        wd = np.where(ok, w, F32(0)).astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            sx += wd * np.where(ok, x, F32(0)).astype(np.float64)          # float32 x float32 is exact in float64
            sy += wd * np.where(ok, y, F32(0)).astype(np.float64)
            w_sum += wd
    return sx, sy, w_sum


def average_rows(rows, weights=None, time_bin=0, freq_bin=1, n_baselines=None):
    """rows [n_chunks, n_rows, nchan] complex64 (or [n_rows, nchan]: one chunk), of which the first n_baselines rows of a chunk
    are read (None: all), weights [n_chunks, n_baselines, nchan] float32 or None -> (out_rows [n_int, n_baselines, n_out]
    complex64, out_weights [n_int, n_baselines, n_out] float32)"""
    rows = np.asarray(rows)
    if rows.ndim == 2:
        rows = rows[None]
        weights = None if weights is None else np.asarray(weights)[None]
    nb = rows.shape[1] if n_baselines is None else int(n_baselines)
    rows = rows[:, :nb].astype(np.complex64)
    n_chunks, _, nchan = rows.shape
    if weights is not None:
        weights = np.asarray(weights, F32)
        assert weights.shape == rows.shape, (weights.shape, rows.shape)
    f = int(freq_bin)
    n_out = -(-nchan // f)
    spans = intervals(n_chunks, int(time_bin))
    out_rows = np.zeros((len(spans), nb, n_out), np.complex64)
    out_weights = np.zeros((len(spans), nb, n_out), F32)
    for s, (c0, c1) in enumerate(spans):
        sx, sy, w_sum = sums(rows[c0:c1], None if weights is None else weights[c0:c1])
        tx, ty, wm = (np.zeros((nb, n_out), np.float64) for _ in range(3))
        for i in range(f):                                                  # input bin m f + i of every output bin m, i ascending
            j = np.arange(n_out) * f + i
            m = np.nonzero(j < nchan)[0]                                    # the last bin may be partial
            with np.errstate(invalid="ignore", over="ignore"):
                tx[:, m] += sx[:, j[m]]
                ty[:, m] += sy[:, j[m]]
                wm[:, m] += w_sum[:, j[m]]
        with np.errstate(invalid="ignore"):
            live = wm > 0
        div = np.where(live, wm, 1.0)
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            re = np.where(live, (tx / div).astype(F32), F32(0))
            im = np.where(live, (ty / div).astype(F32), F32(0))
            out_weights[s] = wm.astype(F32)
        out_rows[s].real = re
        out_rows[s].imag = im
    return out_rows, out_weights
