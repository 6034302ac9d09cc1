"""Float64 numpy restatement of the gain track's definition (include/fxcorr.h fxc_set_track_gains): the solution a chunk takes,
the correction q = 1 / g in natural bin order, the tables of a chunk, and the oracle of tracked rows with gains -- what
tests/test_gain_track_host.py checks on its own and tests/test_gpu_gain_track.py holds the library to."""
import numpy as np

import fx_oracle


def solution_index(t, n_solutions, interval, first_chunk):
    """s(t) = clamp(floor((t - first_chunk) / interval), 0, n_solutions - 1); interval 0 is allowed with one solution only"""
    if n_solutions == 1:
        return 0
    assert interval >= 1
    return min(max((t - first_chunk) // interval, 0), n_solutions - 1)       # (// is floor division)


def inverse(g):
    """q[a][k] = 1 / g[a][(k + nchan // 2) % nchan], g [n_ant, nchan] in the rows' fftshifted order: (x / d, -y / d) with
    d = x x + y y, each operation rounded on its own, and 0 where g is 0"""
    g = np.asarray(g, np.complex128)
    nchan = g.shape[-1]
    g = g[..., (np.arange(nchan) + nchan // 2) % nchan]
    x, y = g.real, g.imag
    d = x * x + y * y
    live = d != 0
    safe = np.where(live, d, 1.0)
    return np.where(live, x / safe, 0.0) + 1j * np.where(live, -y / safe, 0.0)


def phasor(nchan, bandwidth, frequency, tau):
    """the delay track's tables [n_ant, nchan] for the delays tau [n_ant] (fxc_set_delay_track)"""
    freqs = np.fft.fftfreq(nchan, d=1.0 / bandwidth) + frequency
    return np.exp(2j * np.pi * freqs[None, :] * np.asarray(tau, np.float64)[:, None])


def tables(gains, interval, first_chunk, t, tau0, rate, bandwidth, frequency):
    """r_a[k](t) = phasor_a[k](t) * q[s(t)][a][k], the product (c qx - s qy, c qy + s qx); gains [n_solutions, n_ant, nchan]"""
    gains = np.asarray(gains, np.complex128)
    q = inverse(gains[solution_index(t, gains.shape[0], interval, first_chunk)])
    p = phasor(gains.shape[2], bandwidth, frequency, np.asarray(tau0) + t * np.asarray(rate))
    c, s, qx, qy = p.real, p.imag, q.real, q.imag
    return (c * qx - s * qy) + 1j * (c * qy + s * qx)


def spectra(x, nchan, window):
    """x [n_chunks, A, num_samp] -> the oracle's F stage, [n_chunks][A] arrays [n_pts, nchan]"""
    ntaps = len(window) // nchan
    return [[fx_oracle.spectrometer_poly(x[c, a], ntaps, nchan, window) for a in range(x.shape[1])] for c in range(x.shape[0])]


def rows_of(spec, nchan, tau0, rate, t0, bandwidth, frequency, gains=None, interval=0, first_chunk=0, autos=False):
    """the X stage of chunks t0 .. on spectra(x, ..), each chunk with its own tables -> rows [C, n_rows, nchan] complex128"""
    n_chunks, n_ant = len(spec), len(spec[0])
    pairs = [(a, b) for a in range(n_ant) for b in range(a + 1, n_ant)]
    out = np.zeros((n_chunks, len(pairs) + (n_ant if autos else 0), nchan), np.complex128)
    for c in range(n_chunks):
        t = t0 + c
        tau = tau0 + t * rate
        rot = [fx_oracle.rot_table(nchan, bandwidth, frequency, d) for d in tau]
        if gains is not None:
            q = inverse(gains[solution_index(t, gains.shape[0], interval, first_chunk)])
            rot = [rot[a] * q[a] for a in range(n_ant)]
        for p, (a, b) in enumerate(pairs):
            out[c, p] = np.fft.fftshift((spec[c][a] * rot[a] * np.conj(spec[c][b] * rot[b])).mean(axis=0))
        if autos:
            for a in range(n_ant):
                out[c, len(pairs) + a] = np.fft.fftshift((np.abs(spec[c][a]) ** 2).mean(axis=0))
    return out


def oracle(x, nchan, window, tau0, rate, t0, bandwidth, frequency, gains=None, interval=0, first_chunk=0, autos=False):
    """x [n_chunks, A, num_samp] -> rows [C, n_rows, nchan] complex128 of chunks t0 .., each with its own tables: the oracle of
    tests/test_gpu_tracking.py with rot[a] * q[s(t)][a] in place of rot[a] (gains None: rot[a] alone)"""
    return rows_of(spectra(x, nchan, window), nchan, tau0, rate, t0, bandwidth, frequency, gains, interval, first_chunk, autos)


# -- closure from samples -----------------------------------------------------------------------------------------------------
# gains_ref.samples of two seeds (different scalars c_a), 16 chunks each, every antenna's chunk t turned by a fringe rotation
# that the track (tau0 = 0, rate = RHO a, bandwidth 1, frequency F) stops: the loop of the issue -- track, rows, solve per 16
# chunks, gains under the track, rows again -- must give rows of 1.
CLOSURE_ANT = 8
CLOSURE_SEEDS = (200, 201)
CLOSURE_INTERVAL = 16
CLOSURE_F = 1e5
CLOSURE_RHO = 1e-6          # samples (bandwidth 1: seconds) per chunk and antenna index


def closure_samples():
    """-> x [32, 8, n] complex64.  The track's table of antenna a at chunk t is exp(+2 pi i f_k RHO a t) with f_k = F + the
    bin's offset (|offset| <= 1/2): multiplying the samples by exp(-2 pi i F RHO a t) is what it stops, up to the band slope
    2 pi (1/2) RHO a t <= 7e-4 rad that the rotation does not carry."""
    import gains_ref
    x = np.concatenate([gains_ref.samples(CLOSURE_ANT, seed, n_chunks=CLOSURE_INTERVAL)[0] for seed in CLOSURE_SEEDS])
    t = np.arange(x.shape[0], dtype=np.float64)[:, None, None]
    a = np.arange(CLOSURE_ANT, dtype=np.float64)[None, :, None]
    return (x * np.exp(-2j * np.pi * CLOSURE_F * CLOSURE_RHO * a * t)).astype(np.complex64)


def closure_track():
    return np.zeros(CLOSURE_ANT), CLOSURE_RHO * np.arange(CLOSURE_ANT, dtype=np.float64)


def interval_figure(rows, n_base):
    """max |mean over each interval of the cross rows - 1|"""
    rows = np.asarray(rows)[:, :n_base].astype(np.complex128)
    return float(max(np.abs(rows[c:c + CLOSURE_INTERVAL].mean(axis=0) - 1.0).max() for c in range(0, rows.shape[0], CLOSURE_INTERVAL)))


def closure_cpu():
    """The loop on the CPU: oracle rows under the track -> gains_ref.solve_rows -> tables applied.  -> figures"""
    import gains_ref
    from effex_amd.window import design_window
    nchan = gains_ref.SAMPLE_NCHAN
    window = design_window(4, nchan)
    x = closure_samples()
    tau0, rate = closure_track()
    n_base = CLOSURE_ANT * (CLOSURE_ANT - 1) // 2
    spec = spectra(x, nchan, window)
    untracked = rows_of(spec, nchan, tau0, 0.0 * rate, 0, 1.0, CLOSURE_F)
    rows = rows_of(spec, nchan, tau0, rate, 0, 1.0, CLOSURE_F)
    g, step = gains_ref.solve_rows(rows.astype(np.complex64), CLOSURE_ANT, interval=CLOSURE_INTERVAL, iters=gains_ref.SAMPLE_ITERS)
    flat = rows_of(spec, nchan, tau0, rate, 0, 1.0, CLOSURE_F, gains=g, interval=CLOSURE_INTERVAL)
    first_only = rows_of(spec, nchan, tau0, rate, 0, 1.0, CLOSURE_F, gains=g[:1])
    row_0_7 = CLOSURE_ANT - 2             # baselines in the order (0,1), (0,2) .. (0,7), (1,2) ..
    return {"untracked_mean_0_7": float(max(np.abs(untracked[c:c + CLOSURE_INTERVAL, row_0_7].mean(axis=0)).max()
                                            for c in range(0, x.shape[0], CLOSURE_INTERVAL))),
            "no_gains": interval_figure(rows, n_base), "flat": interval_figure(flat, n_base),
            "first_solution_only": interval_figure(first_only, n_base), "step": float(step.max())}
