"""Float64 restatement of the weighted fringe fit's definition (include/fxcorr.h fxc_fringe_fit_weighted) on top of fringe_ref.py,
and the damaged rows its tests fit: what tests/test_fringe_weighted_host.py checks on its own and
tests/test_gpu_fringe_weighted.py holds the library to."""
import numpy as np

import fringe_ref
from fringe_ref import BW, FC


def weighted(R, w):
    """Rw = w > 0 ? (w x, w y) : 0, the products rounded to float32 once each; complex64 in, complex128 out"""
    R = np.asarray(R, dtype=np.complex64)
    w = np.asarray(w, dtype=np.float32)
    live = w > 0                                      # False for 0, negative and NaN weights
    wl = np.where(live, w, np.float32(0))
    re = wl * np.where(live, R.real, np.float32(0))   # float32 products; what a flagged sample holds never meets an operation
    im = wl * np.where(live, R.imag, np.float32(0))
    return re.astype(np.float64) + 1j * im.astype(np.float64)


def fit_baseline_weighted(R, w, bandwidth, frequency, pad):
    """R [n_chunks, nchan] complex64 of one baseline, w its weights (None: all 1) -> delay_s, rate_s_per_chunk, snr, (q0, m0);
    all 0 and no peak where nothing counts"""
    Rw = np.asarray(R, dtype=np.complex64).astype(np.complex128) if w is None else weighted(R, w)
    if (np.abs(Rw) ** 2).sum() == 0.0:
        return 0.0, 0.0, 0.0, None
    if w is not None:
        # the magnitudes of the log-parabolas are those of weights / 2^e, e = floor(log2 of the largest counted weight): an exact
        # scaling of everything before the logarithms (snr, a ratio, does not see it); e = 0 for weights of 1
        w = np.asarray(w, dtype=np.float32)
        shift = 1 - int(np.frexp(w[w > 0].max())[1])
        Rw = np.ldexp(Rw.real, shift) + 1j * np.ldexp(Rw.imag, shift)
    return fringe_ref.fit_baseline(Rw, bandwidth, frequency, pad)


def threshold(nchan, n_chunks, pad, min_snr=0):
    lk, lt = fringe_ref.grid(nchan, n_chunks, pad)
    return min_snr if min_snr > 0 else np.sqrt(np.log(lk * lt) + np.log(1000.0))


def _solve_axis(x, s, used, reached, x0, pr, ref, period):
    n_ant = len(reached)
    slot = {a: k for k, a in enumerate(a for a in range(n_ant) if reached[a] and a != ref)}
    out = np.zeros(n_ant)
    if not slot:
        return out
    N = np.zeros((len(slot), len(slot)))
    y = np.zeros(len(slot))
    for i, (a, b) in enumerate(pr):
        if not (used[i] and reached[a] and reached[b]):
            continue
        d = x[i] + period * np.rint((x0[b] - x0[a] - x[i]) / period)
        wt = s[i] * s[i]
        for ant, sign in ((a, -1.0), (b, 1.0)):
            if ant in slot:
                N[slot[ant], slot[ant]] += wt
                y[slot[ant]] += sign * wt * d
        if a in slot and b in slot:
            N[slot[a], slot[b]] -= wt
            N[slot[b], slot[a]] -= wt
    L = np.linalg.cholesky(N)
    sol = np.linalg.solve(L.T, np.linalg.solve(L, y))
    for a, k in slot.items():
        out[a] = sol[k] - period * np.rint(sol[k] / period)
    return out


def solve_antennas(base, n_ant, ref, nchan, n_chunks, pad, bandwidth, frequency, min_snr=0):
    """base [n_base, 3] = (delay, rate, snr) of every cross row, the estimates of D_b - D_a -> delays [n_ant], rates [n_ant],
    snr [n_ant], used [n_base] bool: used, tree, unwrap, solve and wrap of the definition"""
    base = np.asarray(base, dtype=np.float64)
    pr = fringe_ref.pairs(n_ant)
    d, r, s = base[:, 0], base[:, 1], base[:, 2]
    used = s >= threshold(nchan, n_chunks, pad, min_snr)
    reached = np.zeros(n_ant, bool)
    reached[ref] = True
    d0, r0 = np.zeros(n_ant), np.zeros(n_ant)
    while True:
        pick = -1
        for i, (a, b) in enumerate(pr):
            if used[i] and reached[a] != reached[b] and (pick < 0 or s[i] > s[pick]):
                pick = i
        if pick < 0:
            break
        a, b = pr[pick]
        if reached[a]:
            d0[b], r0[b], reached[b] = d0[a] + d[pick], r0[a] + r[pick], True
        else:
            d0[a], r0[a], reached[a] = d0[b] - d[pick], r0[b] - r[pick], True
    delays = _solve_axis(d, s, used, reached, d0, pr, ref, nchan / bandwidth)
    rates = _solve_axis(r, s, used, reached, r0, pr, ref, 1.0 / frequency)
    snr = np.zeros(n_ant)
    for i, (a, b) in enumerate(pr):
        if used[i] and reached[a] and reached[b]:
            snr[a] += s[i] * s[i]
            snr[b] += s[i] * s[i]
    snr = np.sqrt(snr)
    snr[ref] = 0.0
    return delays, rates, snr, used


def fit_rows_weighted(rows, weights, n_ant, bandwidth, frequency, ref=0, pad=2, baselines="ref", min_snr=0):
    """rows [n_chunks, n_rows, nchan], weights [n_chunks, n_base, nchan] or None -> delays, rates, snr [n_ant], base [n_base, 3],
    peaks {row index: (q0, m0) or None}; base as row (lo, hi) reads in both modes"""
    pr = fringe_ref.pairs(n_ant)
    n_chunks, _, nchan = rows.shape
    base, peaks = np.zeros((len(pr), 3)), {}
    delays, rates, snr = np.zeros(n_ant), np.zeros(n_ant), np.zeros(n_ant)
    for i, (a, b) in enumerate(pr):
        if baselines == "ref" and ref not in (a, b):
            continue
        w = None if weights is None else weights[:, i]
        if baselines == "ref" and b == ref:          # antenna a against ref = b: the conjugated row
            dl, rt, sn, peaks[i] = fit_baseline_weighted(np.conj(rows[:, i]), w, bandwidth, frequency, pad)
            delays[a], rates[a], snr[a] = dl, rt, sn
            base[i] = (-dl, -rt, sn)
        else:
            dl, rt, sn, peaks[i] = fit_baseline_weighted(rows[:, i], w, bandwidth, frequency, pad)
            base[i] = (dl, rt, sn)
            if baselines == "ref":
                delays[b], rates[b], snr[b] = dl, rt, sn
    if baselines == "all":
        delays, rates, snr, _ = solve_antennas(base, n_ant, ref, nchan, n_chunks, pad, bandwidth, frequency, min_snr)
    return delays, rates, snr, base, peaks


# -- the damaged fixture -------------------------------------------------------------------------------------------------------
DAMAGED = dict(n_ant=6, nchan=64, n_chunks=32, pad=2, dead=4, lost=(0, 3), chunks=(5, 9), tone=17)
DAMAGED_D = np.array([0.0, 0.35, -0.35, 0.2, 0.05, -0.1]) * DAMAGED["nchan"] / BW
DAMAGED_R = np.array([0.0, -0.3, 0.1, 0.4, 0.0, -0.2]) / FC


def damaged_rows():
    """-> rows [32, 15, 64] complex64, weights [32, 15, 64] float32: six antennas at snr_in 1, antenna 4 dead (its rows are noise);
    chunks 5 to 8 dropped (NaN, weight 0), a tone of 1e30 in bin 17 (weight 0), baseline (0, 3) lost (Inf, weight 0)"""
    c = DAMAGED
    rng = np.random.default_rng(5)
    rows = fringe_ref.model_rows(c["n_chunks"], c["n_ant"], c["nchan"], DAMAGED_D, DAMAGED_R, 1.0, rng)
    pr = fringe_ref.pairs(c["n_ant"])
    for i, (a, b) in enumerate(pr):
        if c["dead"] in (a, b):
            shape = (c["n_chunks"], c["nchan"])
            rows[:, i] = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)
    weights = np.ones((c["n_chunks"], len(pr), c["nchan"]), np.float32)
    lo, hi = c["chunks"]
    weights[lo:hi] = 0
    rows[lo:hi] = np.nan + 1j * np.nan
    weights[:, :, c["tone"]] = 0
    rows[:, :, c["tone"]] = 1e30
    lost = pr.index(c["lost"])
    weights[:, lost] = 0
    rows[:, lost] = np.inf
    return rows, weights


def zeroed(rows, weights):
    """the same rows with zeros wherever the weight does not count"""
    out = rows.copy()
    out[~(weights > 0)] = 0
    return out
