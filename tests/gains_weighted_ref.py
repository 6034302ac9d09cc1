"""Float64 restatement of the weighted gain solve's definition (include/fxcorr.h fxc_solve_gains_weighted) and the inputs its
tests solve: what tests/test_gains_weighted_host.py checks on its own and tests/test_gpu_gains_weighted.py holds the library to.
With weights and model None it is gains_ref.solve_rows operation for operation."""
import numpy as np

import gains_ref


def average(rows, weights, n_ant, model=None):
    """rows [n, n_rows, nchan] and weights [n, n_baselines, nchan] (or None: ones) of one interval, model [n_baselines, nchan] (or
    None: ones) -> U [nchan, n_ant, n_ant] complex128 and D [nchan, n_ant, n_ant] float64, both with a zero diagonal.  A sample
    counts iff its weight is > 0; the value of one that does not is never touched."""
    rows = np.asarray(rows)
    pr = gains_ref.pairs(n_ant)
    nb, nchan, n = len(pr), rows.shape[2], rows.shape[0]
    s_re, s_im, s_w = (np.zeros((nb, nchan), np.float64) for _ in range(3))
    for c in range(n):
        v = rows[c, :nb]
        if weights is None:
            s_re += v.real.astype(np.float64)
            s_im += v.imag.astype(np.float64)
            s_w += 1.0
            continue
        w = np.asarray(weights[c], np.float32)
        with np.errstate(invalid="ignore"):
            ok = w > 0
        wd = np.where(ok, w, np.float32(0)).astype(np.float64)
        s_re += wd * np.where(ok, v.real, np.float32(0)).astype(np.float64)
        s_im += wd * np.where(ok, v.imag, np.float32(0)).astype(np.float64)
        s_w += wd
    a_re, a_im, wbar = s_re / float(n), s_im / float(n), s_w / float(n)
    if model is None:
        u, d = a_re + 1j * a_im, wbar
    else:
        mx, my = np.asarray(model).real.astype(np.float64), np.asarray(model).imag.astype(np.float64)
        u = (a_re * mx + a_im * my) + 1j * (a_im * mx - a_re * my)
        d = wbar * (mx * mx + my * my)
    um = np.zeros((nchan, n_ant, n_ant), np.complex128)
    dm = np.zeros((nchan, n_ant, n_ant), np.float64)
    for i, (a, b) in enumerate(pr):
        um[:, a, b] = u[i]
        um[:, b, a] = np.conj(u[i])
        dm[:, a, b] = d[i]
        dm[:, b, a] = d[i]
    return um, dm


def solve_matrix(um, dm, ref, iters):
    """U, D [nchan, n_ant, n_ant] (zero diagonals) -> gains [n_ant, nchan] complex128, step [nchan]"""
    nchan, n_ant, _ = um.shape
    has = dm[:, :, ref] != 0                                                     # [nchan, n_ant]; False at ref (the diagonal)
    div = np.where(has, dm[:, :, ref], 1.0)
    vhat = np.where(has, um[:, :, ref].real / div + 1j * (um[:, :, ref].imag / div), 0.0)
    count = has.sum(axis=1)
    s = np.abs(np.delete(vhat, ref, axis=1)).sum(axis=1) / np.where(count > 0, count, 1).astype(np.float64)
    live = (s != 0) & (count > 0)
    root = np.sqrt(np.where(live, s, 1.0))
    g = np.where(live[:, None], vhat / root[:, None], 0.0)
    g[:, ref] = np.where(live, root, 0.0)
    step = np.zeros(nchan)
    for it in range(1, iters + 1):
        n = np.matmul(um, g[:, :, None])[:, :, 0]
        d = np.matmul(dm, (np.abs(g) ** 2)[:, :, None])[:, :, 0]
        new = np.where(d != 0, n / np.where(d != 0, d, 1.0), 0.0)
        if it % 2 == 0:
            new = (new + g) / 2.0
        num, den = (np.abs(new - g) ** 2).sum(axis=1), (np.abs(new) ** 2).sum(axis=1)
        step = np.where(den != 0, np.sqrt(num / np.where(den != 0, den, 1.0)), 0.0)
        g = new
    mag = np.abs(g[:, ref])
    u = np.where(mag != 0, np.conj(g[:, ref]) / np.where(mag != 0, mag, 1.0), 1.0)
    g = g * u[:, None]
    g[:, ref] = np.where(mag != 0, mag, g[:, ref])
    return g.T.copy(), step


def solve_rows(rows, n_ant, interval=0, ref=0, iters=50, weights=None, model=None):
    """rows [n_chunks, n_rows, nchan] (or [n_rows, nchan]: one chunk), weights [n_chunks, n_baselines, nchan] float32 or None,
    model [n_baselines, nchan] or [n_int, n_baselines, nchan] or None -> gains [n_int, n_ant, nchan], step [n_int, nchan]"""
    rows = np.asarray(rows)
    if rows.ndim == 2:
        rows = rows[None]
        weights = None if weights is None else np.asarray(weights)[None]
    if model is not None:
        model = np.asarray(model).astype(np.complex64)
    out = []
    for s, (c0, c1) in enumerate(gains_ref.intervals(rows.shape[0], interval)):
        m = None if model is None else (model if model.ndim == 2 else model[s])
        um, dm = average(rows[c0:c1], None if weights is None else weights[c0:c1], n_ant, m)
        out.append(solve_matrix(um, dm, ref, iters))
    return np.stack([g for g, _ in out]), np.stack([s for _, s in out])


# -- model rows with damage (host test 4, GPU test 1) -------------------------------------------------------------------------------
DEAD_ANT = 1
DEAD_BIN = 5
FLAG_VALUE = np.complex64(1e6 + 1e6j)


def draw_model(n_ant, nchan, rng, n_model=None):
    """amplitudes uniform in 0.5 .. 1.5, random phases: [n_baselines, nchan] complex64, or [n_model, ..]"""
    nb = n_ant * (n_ant - 1) // 2
    shape = (nb, nchan) if n_model is None else (n_model, nb, nchan)
    return (rng.uniform(0.5, 1.5, shape) * np.exp(1j * rng.uniform(-np.pi, np.pi, shape))).astype(np.complex64)


def damaged_case(n_ant, nchan, n_chunks, rng, sigma=0.0, with_model=True):
    """-> g [n_ant, nchan], model [n_baselines, nchan] complex64 (None without), rows [n_chunks, n_baselines, nchan] complex64 =
    g_a conj(g_b) M_ab (+ noise), weights float32 uniform in 0.25 .. 4 with 20 % of the samples, antenna DEAD_ANT's baselines and
    bin DEAD_BIN flagged (weight 0) and every flagged sample overwritten with FLAG_VALUE"""
    g = gains_ref.draw_gains(n_ant, nchan, rng)
    model = draw_model(n_ant, nchan, rng) if with_model else None
    rows = gains_ref.model_rows(g, n_chunks, rng, sigma=sigma, dtype=np.complex128)
    if with_model:
        rows = rows * model.astype(np.complex128)[None]
    rows = rows.astype(np.complex64)
    weights = rng.uniform(0.25, 4.0, rows.shape).astype(np.float32)
    flagged = rng.uniform(size=rows.shape) < 0.2
    for i, (a, b) in enumerate(gains_ref.pairs(n_ant)):
        if DEAD_ANT in (a, b):
            flagged[:, i] = True
    flagged[:, :, DEAD_BIN] = True
    weights[flagged] = 0
    rows[flagged] = FLAG_VALUE
    return g, model, rows, weights


# -- samples with damage (host test 6, GPU test 4) ------------------------------------------------------------------------------------
DAMAGE_ANT = 8
DAMAGE_SEEDS = (0, 1, 2, 3)
DAMAGE_REFS = (0, 2)
DAMAGE_BAD_ANT = 3
DAMAGE_BAD_CHUNKS = (8, 16)
DAMAGE_TONE_BIN = 20
DAMAGE_TONE_ANTS = (1, 5)


def damaged_samples(seed):
    """gains_ref.samples(8, seed) with antenna 3's samples of chunks 8 .. 15 replaced by complex noise of standard deviation 5
    and a tone of amplitude 0.3 that lands in bin 20 of the rows added to antennas 1 and 5 -> x, c, weights [n_chunks,
    n_baselines, nchan] float32: 0 on antenna 3's baselines in those chunks and on bins 19 .. 21, 1 elsewhere"""
    x, c = gains_ref.samples(DAMAGE_ANT, seed)
    x = x.copy()
    nchan, n = gains_ref.SAMPLE_NCHAN, x.shape[2]
    rng = np.random.default_rng(1000 + seed)
    c0, c1 = DAMAGE_BAD_CHUNKS
    junk = (rng.standard_normal((c1 - c0, n)) + 1j * rng.standard_normal((c1 - c0, n))) / np.sqrt(2.0)
    x[c0:c1, DAMAGE_BAD_ANT] = (5.0 * junk).astype(np.complex64)
    t = np.arange(n, dtype=np.float64)
    tone = 0.3 * np.exp(2j * np.pi * (DAMAGE_TONE_BIN - nchan / 2) * t / nchan)
    x[:, DAMAGE_TONE_ANTS[0]] += tone.astype(np.complex64)
    x[:, DAMAGE_TONE_ANTS[1]] += (tone * np.exp(0.7j)).astype(np.complex64)
    pr = gains_ref.pairs(DAMAGE_ANT)
    weights = np.ones((x.shape[0], len(pr), nchan), np.float32)
    for i, (a, b) in enumerate(pr):
        if DAMAGE_BAD_ANT in (a, b):
            weights[c0:c1, i] = 0
    weights[:, :, DAMAGE_TONE_BIN - 1:DAMAGE_TONE_BIN + 2] = 0
    return x, c, weights


def scalar_ratios(gains, ref):
    """gains_ref.scalar_ratios with the unsolved bins (zero gain) left out of the inner half band"""
    g = np.asarray(gains)
    nchan = g.shape[1]
    keep = np.zeros(nchan, bool)
    keep[nchan // 4:nchan - nchan // 4] = True
    keep &= (g != 0).all(axis=0)
    g = g[:, keep]
    v = (g * (np.conj(g[ref]) / np.abs(g[ref]))[None, :]).mean(axis=1)
    return v / v[ref]
