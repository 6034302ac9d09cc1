"""Float64 restatement of the gain solve's definition (include/fxcorr.h fxc_solve_gains) and the model rows and samples the gain
tests solve: what tests/test_gains_host.py checks on its own and tests/test_gpu_gains.py holds the library to."""
import numpy as np


def pairs(n_ant):
    return [(a, b) for a in range(n_ant) for b in range(a + 1, n_ant)]


def intervals(n_chunks, interval):
    """[(first chunk, end chunk)] of the solution intervals; interval 0 is one over all chunks"""
    span = n_chunks if interval == 0 else min(interval, n_chunks)
    return [(c, min(c + span, n_chunks)) for c in range(0, n_chunks, span)]


def average(rows, n_ant):
    """rows [n, n_rows, nchan] of one interval -> the Hermitian matrices [nchan, n_ant, n_ant] complex128 with a zero diagonal:
    the first n_baselines rows added in float64 chunk after chunk, then divided by their number"""
    rows = np.asarray(rows)
    pr = pairs(n_ant)
    acc_re = np.zeros((len(pr), rows.shape[2]), np.float64)
    acc_im = np.zeros((len(pr), rows.shape[2]), np.float64)
    for c in range(rows.shape[0]):
        acc_re += rows[c, :len(pr)].real.astype(np.float64)
        acc_im += rows[c, :len(pr)].imag.astype(np.float64)
    v = acc_re / float(rows.shape[0]) + 1j * (acc_im / float(rows.shape[0]))
    m = np.zeros((rows.shape[2], n_ant, n_ant), np.complex128)
    for i, (a, b) in enumerate(pr):
        m[:, a, b] = v[i]
        m[:, b, a] = np.conj(v[i])
    return m


def solve_matrix(m, ref, iters):
    """m [nchan, n_ant, n_ant] (zero diagonal) -> gains [n_ant, nchan] complex128, step [nchan]"""
    nchan, n_ant, _ = m.shape
    off = 1.0 - np.eye(n_ant)
    s = np.abs(np.delete(m[:, :, ref], ref, axis=1)).sum(axis=1) / (n_ant - 1)
    live = s != 0
    root = np.sqrt(np.where(live, s, 1.0))
    g = np.where(live[:, None], m[:, :, ref] / root[:, None], 0.0)
    g[:, ref] = np.where(live, root, 0.0)
    step = np.zeros(nchan)
    for it in range(1, iters + 1):
        n = np.matmul(m, g[:, :, None])[:, :, 0]
        d = np.matmul(off[None], (np.abs(g) ** 2)[:, :, None])[:, :, 0]
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


def solve_rows(rows, n_ant, interval=0, ref=0, iters=50):
    """rows [n_chunks, n_rows, nchan] (or [n_rows, nchan]: one chunk) -> gains [n_int, n_ant, nchan], step [n_int, nchan]"""
    rows = np.asarray(rows)
    if rows.ndim == 2:
        rows = rows[None]
    out = [solve_matrix(average(rows[c0:c1], n_ant), ref, iters) for c0, c1 in intervals(rows.shape[0], interval)]
    return np.stack([g for g, _ in out]), np.stack([s for _, s in out])


def rotate_to_ref(g, ref):
    """gains [n_ant, nchan] with antenna ref made real and non-negative: what a solve can know of the truth"""
    g = np.asarray(g, np.complex128)
    return g * (np.conj(g[ref]) / np.abs(g[ref]))[None, :]


def draw_gains(n_ant, nchan, rng):
    """amplitudes uniform in 0.5 .. 2, phases uniform in +-pi"""
    return rng.uniform(0.5, 2.0, (n_ant, nchan)) * np.exp(1j * rng.uniform(-np.pi, np.pi, (n_ant, nchan)))


def model_rows(g, n_chunks, rng=None, sigma=0.0, dtype=np.complex64):
    """cross rows [n_chunks, n_base, nchan] of gains g [n_ant, nchan]: row (a, b) = g_a conj(g_b), plus complex noise of
    standard deviation sigma per chunk"""
    pr = pairs(g.shape[0])
    one = np.stack([g[a] * np.conj(g[b]) for a, b in pr])
    out = np.repeat(one[None], n_chunks, axis=0)
    if sigma:
        out = out + sigma * (rng.standard_normal(out.shape) + 1j * rng.standard_normal(out.shape)) / np.sqrt(2.0)
    return out.astype(dtype)


def apply_tables(rows, tables, n_ant):
    """what fxc_set_rot_ant does to cross rows in the rows' fftshifted order: row (a, b) times r_a conj(r_b), tables [n_ant,
    nchan] in natural bin order"""
    r = np.fft.fftshift(np.asarray(tables), axes=-1)
    out = np.array(rows, dtype=np.complex128)
    for i, (a, b) in enumerate(pairs(n_ant)):
        out[..., i, :] *= r[a] * np.conj(r[b])
    return out


# -- samples ------------------------------------------------------------------------------------------------------------------
# x_a = c_a s + n_a: one noise source s of unit power seen by every antenna through a complex scalar c_a, and receiver noise of
# standard deviation SAMPLE_NOISE beside it -- a strong calibrator.  The cross spectra are then c_a conj(c_b) |S|^2 plus cross
# terms that average away, the gains c_a sqrt(<|S|^2>) up to the reference's phase.
SAMPLE_NCHAN = 64
SAMPLE_SPECTRA = 128            # spectra per chunk
SAMPLE_CHUNKS = 32
SAMPLE_NOISE = 0.02
SAMPLE_ITERS = 60


def draw_scalars(n_ant, rng):
    """amplitudes uniform in 0.8 .. 1.25, phases uniform in +-pi"""
    return rng.uniform(0.8, 1.25, n_ant) * np.exp(1j * rng.uniform(-np.pi, np.pi, n_ant))


def samples(n_ant, seed, nchan=SAMPLE_NCHAN, n_spec=SAMPLE_SPECTRA, n_chunks=SAMPLE_CHUNKS, noise=SAMPLE_NOISE):
    """-> x [n_chunks, n_ant, nchan n_spec] complex64, c [n_ant]"""
    rng = np.random.default_rng(seed)
    c = draw_scalars(n_ant, rng)
    n = nchan * n_spec
    s = (rng.standard_normal((n_chunks, 1, n)) + 1j * rng.standard_normal((n_chunks, 1, n))) / np.sqrt(2.0)
    w = (rng.standard_normal((n_chunks, n_ant, n)) + 1j * rng.standard_normal((n_chunks, n_ant, n))) / np.sqrt(2.0)
    return (c[None, :, None] * s + noise * w).astype(np.complex64), c


def scalar_ratios(gains, ref):
    """gains [n_ant, nchan] of one solution -> the estimate of c_a conj(c_ref) / |c_ref|^2: g_a conj(g_ref) / |g_ref| averaged over
    the inner half of the band, normalised by antenna ref's value"""
    g = np.asarray(gains)
    nchan = g.shape[1]
    inner = slice(nchan // 4, nchan - nchan // 4)
    v = (g * (np.conj(g[ref]) / np.abs(g[ref]))[None, :])[:, inner].mean(axis=1)
    return v / v[ref]


def true_ratios(c, ref):
    return c * np.conj(c[ref]) / np.abs(c[ref]) ** 2
