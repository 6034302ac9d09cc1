"""FxPlan — thin Python handle on an ``fxc_plan`` (include/fxcorr.h).

Buffers are either device-resident ``torch`` complex64 tensors (passed by ``data_ptr()``; PyTorch is
only the allocator / stream / collective plumbing) or host numpy complex64 arrays (the library stages
them itself).  Outputs come back in the same kind as the input.
"""
import ctypes

import numpy as np

from . import _lib
from .window import design_window

MODES = {"SPECTRUM": _lib.FXC_MODE_SPECTRUM, "CONTINUUM": _lib.FXC_MODE_CONTINUUM, "TEST": _lib.FXC_MODE_CONTINUUM}
PATHS = {None: -1, "auto": -1, "generic": _lib.FXC_PATH_GENERIC, "fused": _lib.FXC_PATH_FUSED,
         "stream": _lib.FXC_PATH_STREAM, "tiled": _lib.FXC_PATH_TILED}
PATH_NAMES = {_lib.FXC_PATH_GENERIC: "generic", _lib.FXC_PATH_FUSED: "fused", _lib.FXC_PATH_STREAM: "stream",
              _lib.FXC_PATH_TILED: "tiled"}


def _current_torch_stream(device):
    """torch's current HIP stream on ``device`` (0 = the default stream) or 0 without torch/GPU."""
    try:
        import torch
        if torch.cuda.is_available():
            return int(torch.cuda.current_stream(device).cuda_stream)
    except ImportError:
        pass
    return 0


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _torch_dtype(dtype):
    """the torch type of a numpy ``dtype`` (they share their names)"""
    import torch
    return getattr(torch, np.dtype(dtype).name)


BEAM_MODES = {"POWER": _lib.FXC_BEAM_POWER, "VOLTAGE": _lib.FXC_BEAM_VOLTAGE}
IQ_FORMATS = {"c64": _lib.FXC_IQ_C64, "u8": _lib.FXC_IQ_U8, "c128": _lib.FXC_IQ_C128}
_IQ_DTYPES = {"c64": np.complex64, "u8": np.uint8, "c128": np.complex128}


def pinned_empty(shape, dtype):
    """A numpy array in pinned host memory from ``fxc_host_alloc`` -- the counterpart of the reference's
    ``cusignal.get_shared_mem`` staging buffers (effex.py:109-110): host-buffer calls copy from it by direct DMA, and
    visibility rows asked for into such an array are written by the device itself.  Freed when the last view dies."""
    import weakref
    lib = _lib.load()
    shape = tuple(int(v) for v in (shape if np.ndim(shape) else (shape,)))
    dtype = np.dtype(dtype)
    n_bytes = max(1, int(np.prod(shape)) * dtype.itemsize)
    ptr = ctypes.c_void_p()
    _lib.check(lib.fxc_host_alloc(ctypes.byref(ptr), n_bytes), None)
    buf = (ctypes.c_char * n_bytes).from_address(ptr.value)
    fin = weakref.finalize(buf, lib.fxc_host_free, ctypes.c_void_p(ptr.value))
    fin.atexit = False          # at interpreter exit the HIP runtime may already be gone; the OS takes the pages back
    return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)


def rot_table(nbins, bandwidth, frequency, calibrated_delay):
    """rot[k] = exp(+2 pi i f_k tau), natural bin order, complex128 — effex/effex.py:516,519.

    Formed in float64 on the host: the phase is ~9e3 rad for tau = 1 us.
    """
    freqs = np.fft.fftfreq(nbins, d=1.0 / bandwidth) + frequency
    return np.exp(2j * np.pi * freqs * calibrated_delay)


def rot_tables(nbins, bandwidth, frequency, delays):
    """Per-antenna rot tables [n_ant, nbins] complex128 for ``FxPlan.set_rot_ant``: row a is ``rot_table(..., delays[a])``."""
    return np.stack([rot_table(nbins, bandwidth, frequency, d) for d in np.asarray(delays, dtype=np.float64).reshape(-1)])


def split_delays(delays_s, bandwidth):
    """A delay's two halves: ``(shifts int64 [n], remainder_s float64 [n])`` with ``shifts = rint(tau * bandwidth)`` (ties to
    even) whole samples for ``FxPlan.set_sample_delays`` and ``remainder = tau - shifts / bandwidth`` seconds, at most half a
    sample, which a phase slope corrects without loss."""
    tau = np.asarray(delays_s, dtype=np.float64).reshape(-1)
    shifts = np.rint(tau * float(bandwidth)).astype(np.int64)
    return shifts, tau - shifts / float(bandwidth)


def aligned_rot_tables(nchan, bandwidth, frequency, delays_s, shifts):
    """Per-antenna tables [n_ant, nchan] complex128 for streams that ``FxPlan.set_sample_delays(shifts)`` has already moved by
    whole samples (fxcorr.h fxc_set_sample_delays): the full table of ``delays_s`` without the baseband slope ``kk s / nchan``
    turns the shift has undone, the carrier term ``frequency * tau`` kept.  With kk the integer bin index of ``np.fft.fftfreq``
    and f_k = kk df + frequency: u = f_k tau - rint(f_k tau), m = (kk s) mod nchan in integers, v = u - m / nchan,
    r[k] = exp(2 pi i (v - rint(v)))."""
    nchan = int(nchan)
    tau = np.asarray(delays_s, dtype=np.float64).reshape(-1)
    shifts = np.asarray(shifts, dtype=np.int64).reshape(-1)
    if shifts.shape != tau.shape:
        raise ValueError("delays_s and shifts must have the same number of entries")
    freqs = np.fft.fftfreq(nchan, d=1.0 / bandwidth) + frequency
    kk = np.arange(nchan, dtype=np.int64)
    kk = np.where(kk < (nchan + 1) // 2, kk, kk - nchan)
    turns = freqs[None, :] * tau[:, None]
    u = turns - np.rint(turns)
    m = np.mod(kk[None, :] * shifts[:, None], nchan)
    v = u - m.astype(np.float64) / float(nchan)
    return np.exp(2j * np.pi * (v - np.rint(v)))


def gain_tables(gains, n_ant, nchan, delays_s=None, bandwidth=None, frequency=None, shifts=None):
    """Per-antenna tables [n_ant, nchan] complex128 for ``FxPlan.set_rot_ant`` that undo the gains ``gains`` [n_ant, nchan] of
    ``FxPlan.solve_gains`` (bins in the rows' fftshifted order): ``ifftshift(1 / g_a)``, 0 where g_a is 0, times the rot table
    of ``delays_s[a]`` when delays are given (``shifts``: the ``aligned_rot_tables`` of streams moved by those whole samples)."""
    gains = np.asarray(gains, dtype=np.complex128)
    if gains.shape != (n_ant, nchan):
        raise ValueError("gains must have shape ({}, {})".format(n_ant, nchan))
    inv = np.zeros_like(gains)
    np.divide(1.0, gains, out=inv, where=gains != 0)
    tables = np.fft.ifftshift(inv, axes=1)
    if delays_s is not None:
        if bandwidth is None or frequency is None:
            raise ValueError("delays_s needs bandwidth and frequency")
        delays = np.asarray(delays_s, dtype=np.float64).reshape(-1)
        if delays.shape != (n_ant,):
            raise ValueError("delays_s must have {} entries".format(n_ant))
        if shifts is None:
            tables = tables * rot_tables(nchan, bandwidth, frequency, delays)
        else:
            tables = tables * aligned_rot_tables(nchan, bandwidth, frequency, delays, shifts)
    return tables


def offset_source_model(n_ant, nchan, bandwidth, frequency, delays_s, flux=1.0):
    """Model visibilities [n_baselines, nchan] complex64 for ``FxPlan.solve_gains(.., model=)``, bins in the rows' fftshifted
    order, baselines in the rows' order: a point source of flux ``flux`` whose signal reaches antenna a ``delays_s[a]`` later than
    the phase centre's would.  With r = ``rot_tables(nchan, bandwidth, frequency, delays_s)`` row (a, b) is
    ``flux * fftshift(conj(r_a) r_b)``: the phase slopes the rows of such a source carry (row (a, b) is x_a conj(x_b))."""
    delays = np.asarray(delays_s, dtype=np.float64).reshape(-1)
    if delays.shape != (n_ant,):
        raise ValueError("delays_s must have {} entries".format(n_ant))
    rot = np.fft.fftshift(rot_tables(nchan, bandwidth, frequency, delays), axes=1)
    out = [float(flux) * np.conj(rot[a]) * rot[b] for a in range(n_ant) for b in range(a + 1, n_ant)]
    return np.stack(out).astype(np.complex64)


def beam_weights(n_ant, nchan, bandwidth, frequency, delays_s=None, beam_delays_s=None, gains=None, taper=None):
    """Weights [n_beam, n_ant, nchan] complex64 for ``FxPlan.beamform``, natural bin order: beam b's row of antenna a is the
    table that phases the antenna for ``delays_s[a] + beam_delays_s[b, a]`` -- ``rot_tables(..)``, or with ``gains`` [n_ant, nchan]
    (one solution of ``solve_gains``, bins in the rows' order) ``gain_tables(gains, .., delays)``, which also undoes the gains --
    times ``taper[a]`` (default 1 / n_ant: the beam is the mean of the phased antennas).  ``beam_delays_s`` is [n_beam, n_ant]
    seconds; None is one beam at the phase centre.  ``delays_s`` None is 0: under a delay track the track carries the delays
    (and ``set_track_gains`` the gains).  Formed in float64 and rounded once."""
    n_ant, nchan = int(n_ant), int(nchan)
    base = np.zeros(n_ant) if delays_s is None else np.asarray(delays_s, dtype=np.float64).reshape(-1)
    if base.shape != (n_ant,):
        raise ValueError("delays_s must have {} entries".format(n_ant))
    offsets = np.zeros((1, n_ant)) if beam_delays_s is None else np.asarray(beam_delays_s, dtype=np.float64)
    if offsets.ndim == 1:
        offsets = offsets[None]
    if offsets.ndim != 2 or offsets.shape[0] < 1 or offsets.shape[1] != n_ant:
        raise ValueError("beam_delays_s must have shape (n_beam, {})".format(n_ant))
    taper = np.full(n_ant, 1.0 / n_ant) if taper is None else np.asarray(taper, dtype=np.float64).reshape(-1)
    if taper.shape != (n_ant,):
        raise ValueError("taper must have {} entries".format(n_ant))
    out = []
    for off in offsets:
        if gains is not None:
            tables = gain_tables(gains, n_ant, nchan, base + off, bandwidth, frequency)
        else:
            tables = rot_tables(nchan, bandwidth, frequency, base + off)
        out.append(tables * taper[:, None])
    return np.stack(out).astype(np.complex64)


def averaged_freqs(nchan, bandwidth, frequency, freq_bin=1):
    """The mean frequency of each output bin of ``FxPlan.average_rows(.., freq_bin=)``, float64 [ceil(nchan / freq_bin)]: the
    rows' bins in their fftshifted order have the frequencies ``frequency + fftshift(fftfreq(nchan, 1 / bandwidth))``; output bin
    m is the mean over the input bins [m freq_bin, min((m + 1) freq_bin, nchan)) -- the last one may hold fewer."""
    nchan, freq_bin = int(nchan), int(freq_bin)
    if nchan < 1 or freq_bin < 1:
        raise ValueError("nchan and freq_bin must be 1 or more")
    freqs = np.fft.fftshift(np.fft.fftfreq(nchan, d=1.0 / bandwidth)) + frequency
    return np.array([freqs[k:k + freq_bin].mean() for k in range(0, nchan, freq_bin)])


DM_CONSTANT_S = 4.148808e3      # seconds of delay per unit DM (pc cm^-3) at 1 MHz, against infinite frequency


def dm_shifts(nchan, bandwidth, frequency, dms, tsamp):
    """The shift table of ``FxPlan.dedisperse``, int32 [n_dm, nchan]: channel k of the rows' fftshifted order has the frequency
    ``f = frequency + fftshift(fftfreq(nchan, 1 / bandwidth))[k]`` (the axis of ``averaged_freqs``), lags the top of the band by
    ``4.148808e3 s * DM * ((f / MHz)^-2 - (f_max / MHz)^-2)`` at dispersion measure DM, and its shift is that delay over ``tsamp``
    seconds rounded to the nearest sample, formed in float64.  The top channel's shift is 0.  A beam's ``tsamp`` is ``tint * nchan /
    bandwidth``."""
    nchan = int(nchan)
    dms = np.atleast_1d(np.asarray(dms, dtype=np.float64))
    if nchan < 1 or dms.ndim != 1 or dms.size < 1:
        raise ValueError("nchan must be 1 or more and dms a list of one or more trials")
    if not tsamp > 0 or not bandwidth > 0:
        raise ValueError("tsamp and bandwidth must be > 0")
    if not (np.isfinite(dms).all() and (dms >= 0).all()):
        raise ValueError("the trial dispersion measures must be finite and >= 0")
    f_mhz = (np.fft.fftshift(np.fft.fftfreq(nchan, d=1.0 / bandwidth)) + frequency) / 1e6
    if not (f_mhz > 0).all():
        raise ValueError("the band reaches 0 Hz or below")
    delay = DM_CONSTANT_S * dms[:, None] * (f_mhz ** -2.0 - f_mhz.max() ** -2.0)[None, :]
    steps = np.rint(delay / float(tsamp))
    if steps.max() >= 2.0 ** 31:
        raise ValueError("a shift does not fit 31 bits")
    return steps.astype(np.int32)


BOXCAR_MAX_J = 12      # kBoxMaxJ of csrc/k_boxcar.h


def boxcar_widths(j_lo, j_hi):
    """The widths of ``FxPlan.boxcar_search(.., widths=(j_lo, j_hi))`` in samples: ``1 << arange(j_lo, j_hi + 1)``; the ``width``
    map holds the index j."""
    j_lo, j_hi = int(j_lo), int(j_hi)
    if not 0 <= j_lo <= j_hi <= BOXCAR_MAX_J:
        raise ValueError("widths must satisfy 0 <= j_lo <= j_hi <= {}, got ({}, {})".format(BOXCAR_MAX_J, j_lo, j_hi))
    return 1 << np.arange(j_lo, j_hi + 1)


SIFT_DTYPE = np.dtype([("series", np.int64), ("dm_index", np.int64), ("time", np.int64), ("width", np.int64), ("snr", np.float32),
                       ("n_cells", np.int64)])


def sift_pulses(snr, width, time, threshold=6.0):
    """Candidates from the maps of ``FxPlan.boxcar_search`` (host numpy; tensors are moved to the host): ``snr``, ``width``, ``time``
    of one shape [n_series, n_dm, n_blk] ([n_dm, n_blk] and [n_blk] are one series / one trial).  Per series the cells with ``snr >
    threshold`` are joined over the (trial, block) grid with 8-neighbour connectivity, and each cluster is reduced to its largest
    cell -- ties to the smallest trial, then the smallest block.  -> a structured array with the fields ``series, dm_index, time``
    (the start, samples), ``width`` (samples, ``1 << j``), ``snr, n_cells``, sorted by descending snr, then by (series, dm_index,
    time)."""
    maps = []
    for a in (snr, width, time):
        if _is_torch(a):
            a = a.detach().cpu().numpy()
        maps.append(np.asarray(a))
    snr, width, time = maps
    if not (snr.shape == width.shape == time.shape) or snr.ndim not in (1, 2, 3):
        raise ValueError("snr, width and time must share one shape of 1 to 3 axes, got {} {} {}".format(snr.shape, width.shape, time.shape))
    snr, width, time = (a.reshape((1,) * (3 - a.ndim) + a.shape) for a in (snr, width, time))
    n_series, n_dm, n_blk = snr.shape
    found = []
    with np.errstate(invalid="ignore"):
        above = snr > threshold
    for s in range(n_series):
        label = np.full((n_dm, n_blk), -1, np.int64)
        for d0, b0 in zip(*np.nonzero(above[s])):          # ascending trial, then block: a cluster's first cell is its seed
            if label[d0, b0] >= 0:
                continue
            label[d0, b0] = len(found)
            stack, cells = [(int(d0), int(b0))], []
            while stack:
                d, b = stack.pop()
                cells.append((d, b))
                for dd in range(max(0, d - 1), min(n_dm, d + 2)):
                    for bb in range(max(0, b - 1), min(n_blk, b + 2)):
                        if above[s, dd, bb] and label[dd, bb] < 0:
                            label[dd, bb] = len(found)
                            stack.append((dd, bb))
            best = min(cells, key=lambda c: (-float(snr[s][c]), c[0], c[1]))
            found.append((s, best[0], int(time[s][best]), 1 << int(width[s][best]), snr[s][best], len(cells)))
    out = np.array(found, dtype=SIFT_DTYPE) if found else np.zeros(0, SIFT_DTYPE)
    order = np.lexsort((out["time"], out["dm_index"], out["series"], -out["snr"].astype(np.float64)))
    return out[order]


def sk_thresholds(M, sigma=3.0):
    """(lo, hi) = 1 -/+ sigma sqrt(mu2) for ``FxPlan.kurtosis_weights``, with mu2 = 4 M^2 / ((M - 1)(M + 2)(M + 3)) the variance
    of the spectral kurtosis estimator over ``M`` spectra of Gaussian noise (Nita & Gary 2010).  A symmetric approximation of a
    skewed distribution: the false-alarm share on clean noise is a measured figure (tests/golden/kurtosis_bounds.json), not the
    Gaussian tail of ``sigma``."""
    M = int(M)
    if M < 2:
        raise ValueError("M={}: the estimator needs 2 or more spectra".format(M))
    if not sigma > 0:
        raise ValueError("sigma must be > 0")
    half = float(sigma) * float(np.sqrt(4.0 * M * M / ((M - 1.0) * (M + 2.0) * (M + 3.0))))
    return 1.0 - half, 1.0 + half


def gain_track_solution(chunk, n_solutions, interval, first_chunk):
    """The solution chunk ``chunk`` takes under a gain track (fxcorr.h fxc_set_track_gains):
    ``clamp(floor((chunk - first_chunk) / interval), 0, n_solutions - 1)``; interval 0 (one solution) is solution 0."""
    if int(interval) < 1:
        return 0
    return min(max((int(chunk) - int(first_chunk)) // int(interval), 0), int(n_solutions) - 1)


def gain_track_tables(gains, interval, first_chunk, chunk, delays, rates, bandwidth, frequency, whole_samples=False):
    """The numpy form of one chunk's tables under a delay track with a gain track (fxcorr.h fxc_set_track_gains): [n_ant, nchan]
    complex128, ``rot_tables(nchan, bandwidth, frequency, delays + chunk * rates)`` times ``ifftshift(1 / g)`` of the chunk's
    solution.  ``gains`` is [n_ant, nchan] or [n_solutions, n_ant, nchan] as ``FxPlan.solve_gains`` returns them (bins in the
    rows' fftshifted order).  The inverse is (x / d, -y / d) with d = x x + y y, 0 where g is 0, and the product
    (c qx - s qy, c qy + s qx), each operation rounded on its own, as the device forms them.  ``whole_samples``: the tables of
    an aligned track (``FxPlan.set_delay_track(.., whole_samples=True)``), ``aligned_rot_tables`` with the chunk's shifts
    ``rint(tau * bandwidth)``."""
    gains = np.asarray(gains, dtype=np.complex128)
    if gains.ndim == 2:
        gains = gains[None]
    if gains.ndim != 3 or gains.shape[0] < 1:
        raise ValueError("gains must have shape (n_ant, nchan) or (n_solutions, n_ant, nchan)")
    n_sol, n_ant, nchan = gains.shape
    if n_sol > 1 and int(interval) < 1:
        raise ValueError("{} solutions need an interval of 1 chunk or more".format(n_sol))
    delays = np.asarray(delays, dtype=np.float64).reshape(-1)
    rates = np.asarray(rates, dtype=np.float64).reshape(-1)
    if delays.shape != (n_ant,) or rates.shape != (n_ant,):
        raise ValueError("delays and rates must have {} entries".format(n_ant))
    g = np.fft.ifftshift(gains[gain_track_solution(chunk, n_sol, interval, first_chunk)], axes=1)
    x, y = g.real, g.imag
    d = x * x + y * y
    live = d != 0
    safe = np.where(live, d, 1.0)
    qx, qy = np.where(live, x / safe, 0.0), np.where(live, -y / safe, 0.0)
    tau = delays + float(int(chunk)) * rates
    if whole_samples:
        rot = aligned_rot_tables(nchan, bandwidth, frequency, tau, np.rint(tau * float(bandwidth)).astype(np.int64))
    else:
        rot = rot_tables(nchan, bandwidth, frequency, tau)
    c, s = rot.real, rot.imag
    return (c * qx - s * qy) + 1j * (c * qy + s * qx)


class FxPlan(object):
    def __init__(self, n_ant, nchan, ntaps, num_samp, window=None, device=0, stream=None, path=None, dev=False, autos=False):
        self._lib = _lib.load(dev=dev)          # dev: the developer build with the reference kernels (tests, tools/soak.py)
        self._h = ctypes.c_void_p()
        if window is None:
            window = design_window(ntaps, nchan)
        window = np.ascontiguousarray(window, dtype=np.float64)
        if window.shape != (int(ntaps) * int(nchan),):
            raise ValueError("window must have ntaps*nchan = {} taps, got {}".format(ntaps * nchan, window.shape))
        self.window = window
        self._pipes = []                                  # weak references to FxPipeline objects on this plan
        self._queued = []                                 # modes of the finalize results queued and not yet collected
        # Work is issued on the caller's stream so it is ordered with torch's own copies / kernels.  stream=None
        # follows torch's *current* stream call by call (``_follow``): under ``with torch.cuda.stream(s)`` the plan moves
        # to ``s`` (fxc_set_stream orders the two streams with an event), so inputs, kernels and outputs stay ordered.
        self._follow = stream is None
        if stream is None:
            stream = _current_torch_stream(int(device))
        elif stream == "owned":
            stream = -1                                   # FXC_STREAM_OWNED
        self._stream = int(stream)
        stream_ptr = ctypes.c_void_p(int(stream) & 0xFFFFFFFFFFFFFFFF) if stream else None
        rc = self._lib.fxc_plan_create(ctypes.byref(self._h), int(device), int(n_ant), int(nchan), int(ntaps),
                                       int(num_samp), window.ctypes.data, stream_ptr, PATHS[path])
        _lib.check(rc, None, self._lib)
        info = _lib.FxcInfo()
        self._check(self._lib.fxc_plan_get_info(self._h, ctypes.byref(info)))
        self.n_ant, self.n_baselines, self.nchan, self.ntaps = info.n_ant, info.n_baselines, info.nchan, info.ntaps
        self.num_samp, self.n_pts = info.num_samp, info.n_pts
        self.device = info.device
        self.path = PATH_NAMES[info.path]
        self.autos, self.n_rows = False, self.n_baselines
        self.tracked = False                              # a delay track is set (set_delay_track)
        if autos:
            self.set_autos(True)

    def set_autos(self, autos):
        """``fxc_set_products``: results of ``n_rows = n_baselines + n_ant`` rows -- the cross rows, then each antenna's
        autocorrelation (no rot, imaginary part 0) -- or back to the cross rows alone.  Only while nothing is accumulated,
        no finalize result is outstanding and no pipe uses the plan."""
        self._sync_stream()
        want = _lib.FXC_PRODUCTS_CROSS_AUTO if autos else _lib.FXC_PRODUCTS_CROSS
        self._check(self._lib.fxc_set_products(self._h, want))
        products, n_rows = ctypes.c_int(), ctypes.c_int()
        self._check(self._lib.fxc_plan_products(self._h, ctypes.byref(products), ctypes.byref(n_rows)))
        self.autos, self.n_rows = products.value == _lib.FXC_PRODUCTS_CROSS_AUTO, n_rows.value

    # -- plumbing ---------------------------------------------------------------------------
    def _check(self, rc):
        _lib.check(rc, self._h, self._lib)

    def close(self):
        if getattr(self, "_abandoned", False):      # a pipe of this plan was abandoned with a thread still writing into its
            self._h = ctypes.c_void_p()             # slots (FxPipeline.abandon): the plan stays, for the process's life
            return
        if getattr(self, "_h", None) is not None and self._h:
            for ref in list(getattr(self, "_pipes", ())):     # pipes hold a pointer to the plan: they go first
                pipe = ref()
                if pipe is not None:
                    pipe.close()
            self._pipes = []
            # FXC_ERR_STATE: a pipe made behind this object's back still uses the plan -- keep the handle (the plan and
            # its device buffers stay valid for that pipe) and say so instead of leaking silently
            self._check(self._lib.fxc_plan_destroy(self._h))
            self._h = ctypes.c_void_p()

    def _sync_stream(self):
        """Plans created with stream=None issue every call on torch's current stream of their device."""
        if not self._follow:
            return
        cur = _current_torch_stream(self.device)
        if cur != self._stream:
            self._check(self._lib.fxc_set_stream(self._h, ctypes.c_void_p(cur) if cur else None))
            self._stream = cur

    def set_stream(self, stream):
        """Issue the plan's work on ``stream`` (a raw hipStream_t / ``torch.cuda.Stream.cuda_stream``) from now on and
        stop following torch's current stream."""
        self._follow = False
        stream = int(stream)
        self._check(self._lib.fxc_set_stream(self._h, ctypes.c_void_p(stream) if stream else None))
        self._stream = stream

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def info(self):
        info = _lib.FxcInfo()
        self._check(self._lib.fxc_plan_get_info(self._h, ctypes.byref(info)))
        return {name: getattr(info, name) for name, _ in _lib.FxcInfo._fields_}

    def _in(self, x, shape_tail, c128=False):
        """-> (pointer, mem_kind, leading count, keepalive).  ``c128``: complex128 input is handed over as it is
        (``self._fmt`` = FXC_IQ_C128) instead of being narrowed on the host."""
        self._sync_stream()
        self._fmt = _lib.FXC_IQ_C64
        if _is_torch(x):
            import torch
            if c128 and x.dtype == torch.complex128:
                self._fmt = _lib.FXC_IQ_C128
            elif x.dtype != torch.complex64:
                raise ValueError("device input must be a contiguous complex64 CUDA tensor")
            if not x.is_cuda or not x.is_contiguous():
                raise ValueError("device input must be a contiguous complex64 CUDA tensor")
            if x.device.index != self.device:
                raise ValueError("tensor is on device {} but the plan is on {}".format(x.device.index, self.device))
            shape = tuple(x.shape)
            ptr, kind, keep = x.data_ptr(), _lib.FXC_MEM_DEVICE, x
        else:
            if c128 and getattr(x, "dtype", None) == np.complex128:
                self._fmt = _lib.FXC_IQ_C128
                keep = np.ascontiguousarray(x)
            else:
                keep = np.ascontiguousarray(x, dtype=np.complex64)
            shape = keep.shape
            ptr, kind = keep.ctypes.data, _lib.FXC_MEM_HOST
        if len(shape) == len(shape_tail):
            shape = (1,) + shape
        if len(shape) != len(shape_tail) + 1 or tuple(shape[1:]) != tuple(shape_tail):
            raise ValueError("expected shape [n, {}], got {}".format(", ".join(map(str, shape_tail)), shape))
        return ptr, kind, shape[0], keep

    def _out(self, like, shape, dtype, out=None):
        self._to_pinned = False
        if out is not None:
            if _is_torch(like) and not _is_torch(out):
                # device-resident samples, rows into pinned host memory (``pinned_empty``): the finishing kernel writes them
                # there across PCIe, asynchronously -- the caller orders its reads with ``sync()`` or an event on the stream
                if out.dtype != dtype or out.shape != tuple(shape) or not out.flags.c_contiguous or not out.flags.writeable:
                    raise ValueError("out must be a writable C-contiguous {} array of shape {}".format(np.dtype(dtype).name, tuple(shape)))
                self._to_pinned = True
                return out, out.ctypes.data
            if _is_torch(like) != _is_torch(out):
                raise ValueError("out must be of the same kind (host array / CUDA tensor) as the input")
            if _is_torch(out):
                import torch
                tdt = torch.complex64 if dtype == np.complex64 else torch.complex128
                if out.dtype != tdt or tuple(out.shape) != tuple(shape) or not out.is_contiguous() or not out.is_cuda:
                    raise ValueError("out must be a contiguous CUDA tensor of shape {}".format(tuple(shape)))
                return out, out.data_ptr()
            if out.dtype != dtype or out.shape != tuple(shape) or not out.flags.c_contiguous or not out.flags.writeable:
                raise ValueError("out must be a writable C-contiguous {} array of shape {}".format(np.dtype(dtype).name, tuple(shape)))
            return out, out.ctypes.data
        if _is_torch(like):
            import torch
            tdt = torch.complex64 if dtype == np.complex64 else torch.complex128
            out = torch.empty(shape, dtype=tdt, device=like.device)
            return out, out.data_ptr()
        out = np.empty(shape, dtype=dtype)
        return out, out.ctypes.data

    # -- configuration ----------------------------------------------------------------------
    def set_rot(self, rot):
        rot = np.ascontiguousarray(rot, dtype=np.complex128)
        if rot.shape != (self.nchan,):
            raise ValueError("rot must have shape ({},)".format(self.nchan))
        self._check(self._lib.fxc_set_rot(self._h, rot.ctypes.data))
        self.tracked = False

    def set_delay(self, bandwidth, frequency, calibrated_delay):
        self.set_rot(rot_table(self.nchan, bandwidth, frequency, calibrated_delay))

    def set_rot_ant(self, tables):
        """Per-antenna rot: ``tables`` [n_ant, nchan] complex128; cross row (a, b) is then multiplied by r_a conj(r_b)
        (fxcorr.h fxc_set_rot_ant).  Replaces the shared table of ``set_rot`` until the next ``set_rot``."""
        tables = np.ascontiguousarray(tables, dtype=np.complex128)
        if tables.shape != (self.n_ant, self.nchan):
            raise ValueError("tables must have shape ({}, {})".format(self.n_ant, self.nchan))
        self._check(self._lib.fxc_set_rot_ant(self._h, tables.ctypes.data))
        self.tracked = False

    def set_delays(self, delays_s, bandwidth, frequency, whole_samples=False):
        """Phase every baseline for the per-antenna delays ``delays_s`` [n_ant] (seconds, e.g. from ``estimate_delays``).
        ``whole_samples``: split every delay (``split_delays``): the whole samples move the antenna's stream
        (``set_sample_delays``), the tables (``aligned_rot_tables``) keep the rest -- a phase slope alone loses about
        ``d / nchan`` of the amplitude for a delay of d samples."""
        if not whole_samples:
            self.set_rot_ant(rot_tables(self.nchan, bandwidth, frequency, delays_s))
            return
        shifts, _ = split_delays(delays_s, bandwidth)
        self.set_rot_ant(aligned_rot_tables(self.nchan, bandwidth, frequency, delays_s, shifts))
        self.set_sample_delays(shifts)

    def set_sample_delays(self, shifts):
        """Whole-sample delays (fxcorr.h fxc_set_sample_delays): antenna a's samples are read ``shifts[a]`` later, zeros where
        a chunk has none.  ``None`` or all zeros removes them.  Independent of ``set_rot*``; an aligned track sets its own."""
        if shifts is None:
            self._check(self._lib.fxc_set_sample_delays(self._h, None))
            return
        shifts = np.ascontiguousarray(np.asarray(shifts).reshape(-1), dtype=np.int64)
        if shifts.shape != (self.n_ant,):
            raise ValueError("shifts must have {} entries".format(self.n_ant))
        self._check(self._lib.fxc_set_sample_delays(self._h, shifts.ctypes.data))

    def sample_delays(self, chunk=0):
        """The whole-sample shifts [n_ant] int64 chunk ``chunk`` gets: the static ones, an aligned track's, or zeros."""
        out = np.zeros(self.n_ant, dtype=np.int64)
        self._check(self._lib.fxc_sample_delays(self._h, int(chunk), out.ctypes.data))
        return out

    def _per_antenna(self, v, name):
        v = np.asarray(v, dtype=np.float64)
        if v.ndim == 0 and self.n_ant == 2:
            v = np.array([0.0, float(v)])          # a scalar: antenna 1 against antenna 0, as set_delay
        v = np.ascontiguousarray(v.reshape(-1))
        if v.shape != (self.n_ant,):
            raise ValueError("{} must have {} entries".format(name, self.n_ant))
        return v

    def set_delay_track(self, delays_s, rates_s_per_chunk, bandwidth, frequency, first_chunk=0, whole_samples=False):
        """Delays that move: chunk t is phased for ``delays_s[a] + t * rates_s_per_chunk[a]`` (fxcorr.h fxc_set_delay_track).
        Every ``fx_rows`` / ``fx_accumulate`` call and every pipe batch takes the next chunk indices, from ``first_chunk`` on.
        A scalar delay / rate on a two-antenna plan means antenna 1 against antenna 0.  Ends at the next ``set_rot*``.
        A new track drops the gains of ``set_track_gains``: they were solved on rows made under the earlier one, so solve or
        send them again.  ``whole_samples``: the aligned track (fxcorr.h fxc_set_delay_track_aligned): chunk t's streams are also
        moved by ``rint(tau_a(t) * bandwidth)`` whole samples and its tables keep the rest; ``track_tables`` returns those."""
        tau0 = self._per_antenna(delays_s, "delays_s")
        rate = self._per_antenna(rates_s_per_chunk, "rates_s_per_chunk")
        fn = self._lib.fxc_set_delay_track_aligned if whole_samples else self._lib.fxc_set_delay_track
        self._check(fn(self._h, tau0.ctypes.data, rate.ctypes.data, float(bandwidth), float(frequency), int(first_chunk)))
        self.tracked = True

    @property
    def track_chunk(self):
        """The chunk index the next chunk takes under the delay track."""
        t = ctypes.c_int64()
        self._check(self._lib.fxc_delay_track_chunk(self._h, ctypes.byref(t)))
        return t.value

    def track_seek(self, chunk):
        self._check(self._lib.fxc_delay_track_seek(self._h, int(chunk)))

    def track_tables(self, chunk):
        """The per-antenna tables [n_ant, nchan] complex128 the device applies to chunk ``chunk``, the gains of
        ``set_track_gains`` included."""
        out = np.empty((self.n_ant, self.nchan), dtype=np.complex128)
        self._check(self._lib.fxc_delay_track_tables(self._h, int(chunk), out.ctypes.data))
        return out

    def set_track_gains(self, gains, interval=0, first_chunk=0):
        """Gains under the delay track (fxcorr.h fxc_set_track_gains): ``gains`` [n_ant, nchan] or [n_solutions, n_ant, nchan]
        complex128, ``solve_gains``' output as it is; chunk t takes solution
        ``clamp((t - first_chunk) // interval, 0, n_solutions - 1)`` and antenna a's table of that chunk is multiplied by
        ``ifftshift(1 / g_a)`` (0 where g_a is 0), on the device.  ``interval`` may be 0 for one solution.  ``None`` removes
        the gains and keeps the track.  Needs a delay track, an empty accumulator and no open pipe."""
        if gains is None:
            self._check(self._lib.fxc_set_track_gains(self._h, None, 0, 0, 0))
            return
        gains = np.asarray(gains, dtype=np.complex128)
        if gains.ndim == 2:
            gains = gains[None]
        if gains.ndim != 3 or gains.shape[0] < 1 or gains.shape[1:] != (self.n_ant, self.nchan):
            raise ValueError("gains must have shape ({0}, {1}) or (n_solutions, {0}, {1})".format(self.n_ant, self.nchan))
        gains = np.ascontiguousarray(gains)
        self._check(self._lib.fxc_set_track_gains(self._h, gains.ctypes.data, int(gains.shape[0]), int(interval), int(first_chunk)))

    def track_gains_info(self):
        """(n_solutions, interval, first_chunk) of the gain track; zeros when the delay track carries none."""
        n, interval, first = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        self._check(self._lib.fxc_track_gains_info(self._h, ctypes.byref(n), ctypes.byref(interval), ctypes.byref(first)))
        return n.value, interval.value, first.value

    # -- F stage ----------------------------------------------------------------------------
    def channelize(self, x):
        """x: [n_streams, num_samp] (or [num_samp]) complex64 -> [n_streams, n_pts, nchan] complex64."""
        ptr, kind, n, keep = self._in(x, (self.num_samp,))
        out, optr = self._out(x, (n, self.n_pts, self.nchan), np.complex64)
        self._check(self._lib.fxc_channelize(self._h, ptr, optr, n, kind))
        return out

    def beamform(self, x, weights, tint=0, mode="POWER", out=None, *, mask=None, mask_tint=0, whole_samples=False):
        """Tied-array beams: phased sums of the antennas' spectra (fxcorr.h fxc_beamform).  ``x`` = [n_chunks, n_ant, num_samp]
        complex64 (numpy, or a CUDA tensor on the plan's device), ``weights`` = [n_beam, n_ant, nchan] complex64 in natural bin
        order (``beam_weights``; [n_ant, nchan] is one beam; numpy weights with a CUDA ``x`` are moved to the device).  Under a
        delay track every chunk's tables (gains included) multiply the weights and the track's counter advances; the tables of
        ``set_rot`` / ``set_rot_ant`` are not applied.  mode "POWER" -> [n_chunks, n_beam, n_tbin, nchan] float32, the mean of
        |y|^2 over time bins of ``tint`` frames (0: the whole chunk; the last may be partial), bins in the rows' fftshifted
        order; "VOLTAGE" -> [n_chunks, n_beam, n_pts, nchan] complex64, natural bin order.  numpy in, numpy out; CUDA tensor in,
        CUDA tensor out.  ``out``: an array / tensor of the result's shape and dtype to receive it.  At most 16 beams.

        ``mask``, ``mask_tint`` and ``whole_samples`` (fxcorr.h fxc_beamform_ex; with all three at their defaults the call is
        fxc_beamform as it was): ``mask`` = float32 [n_chunks, n_ant, n_mbin, nchan] in the memory of ``x`` (a numpy mask with a
        CUDA ``x`` is moved to the device), channels in the rows' fftshifted order, n_mbin = ceil(n_pts / mask_tint) bins of
        ``mask_tint`` frames (0: the whole chunk) -- what ``kurtosis_mask(kurtosis(x, tint=mask_tint), tint=mask_tint)`` returns.
        An antenna counts in a cell iff its value is > 0; a sample that does not count is selected away, so a NaN or a tone in it
        changes no bit.  Nothing is normalised: ``(mask > 0).sum(axis=1)`` is the count of antennas, and ``(n_ant / count) ** 2``
        rescales a point source's power (``tint == mask_tint`` keeps one count a bin).  ``whole_samples=True`` aligns every pass
        on a plan with whole-sample delays (``set_sample_delays``, ``set_delays(.., whole_samples=True)``, an aligned track);
        without it such a plan is refused (NotImplementedError).  The loop::

            sk = plan.kurtosis(x, tint=64)
            m = plan.kurtosis_mask(sk, tint=64)
            P = plan.beamform(x, w, tint=64, mask=m, mask_tint=64, whole_samples=True)
        """
        return self._beamform(x, weights, tint, BEAM_MODES[mode.upper()], out, mask, mask_tint, whole_samples)

    def beamform_incoherent(self, x, weights, tint=0, out=None, *, mask=None, mask_tint=0, whole_samples=False):
        """Incoherent beams (fxcorr.h fxc_beamform_ex, FXC_BEAM_INCOHERENT): the mean over time bins of
        ``sum_a |weff[b, a, k]|^2 |f_a|^2`` over the counted antennas -> float32 [n_chunks, n_beam, n_tbin, nchan], every
        argument, the bins and the order of the channels as ``beamform(.., mode="POWER")``.  The robust, wide-field companion
        of a tied-array beam: ``beamform(..) - beamform_incoherent(..)`` is the beam's cross-only power.  A gain track scales
        the antennas, a plain delay track changes nothing."""
        return self._beamform(x, weights, tint, _lib.FXC_BEAM_INCOHERENT, out, mask, mask_tint, whole_samples)

    def _beamform(self, x, weights, tint, m, out, mask, mask_tint, whole_samples):
        ptr, kind, n, keep = self._in(x, (self.n_ant, self.num_samp))
        device = kind == _lib.FXC_MEM_DEVICE
        move_to = keep.device if device else None      # numpy weights and a numpy mask with a CUDA x are moved to the device
        w_keep, w_ptr = self._like(weights, "weights", device, np.complex64, move_to, ("x: numpy weights for host samples", None))
        w_shape = tuple(w_keep.shape)
        if len(w_shape) == 2:
            w_shape = (1,) + w_shape
        if len(w_shape) != 3 or w_shape[0] < 1 or w_shape[1:] != (self.n_ant, self.nchan):
            raise ValueError("weights must have shape (n_beam, {}, {}), got {}".format(self.n_ant, self.nchan, tuple(w_keep.shape)))
        n_beam, tint = int(w_shape[0]), int(tint)
        if m != _lib.FXC_BEAM_VOLTAGE:
            shape, dtype = (n, n_beam, self._time_bins(tint)[1], self.nchan), np.float32
        else:
            shape, dtype = (n, n_beam, self.n_pts, self.nchan), np.complex64
        mask_tint, m_keep, m_ptr = int(mask_tint), None, None
        if mask is not None:
            m_keep, m_ptr = self._like(mask, "mask", device, np.float32, move_to, ("x: a numpy mask for host samples", "a device mask"))
            want = (n, self.n_ant, self._time_bins(mask_tint)[1], self.nchan)
            if tuple(m_keep.shape) != want:
                raise ValueError("mask must have shape {}, got {}".format(want, tuple(m_keep.shape)))
        out, o_ptr = self._out_like_x(out, shape, device, keep, dtype=dtype)
        if device and not self._follow:      # a stream of the plan's own: torch's may still be filling the moved weights
            import torch
            torch.cuda.current_stream(keep.device).synchronize()
        self._beam_keep = (keep, w_keep, m_keep)     # until the next call: the queued kernels read them
        if mask is None and mask_tint == 0 and not whole_samples and m != _lib.FXC_BEAM_INCOHERENT:
            self._check(self._lib.fxc_beamform(self._h, ptr, w_ptr, n_beam, o_ptr, n, kind, m, tint))
        else:
            self._check(self._lib.fxc_beamform_ex(self._h, ptr, w_ptr, n_beam, m_ptr, mask_tint, o_ptr, n, kind, m, tint,
                                                  int(bool(whole_samples))))
        return out

    def kurtosis_mask(self, sk, lo=None, hi=None, tint=0, sigma=3.0):
        """The antenna mask from ``kurtosis``'s sk (fxcorr.h fxc_kurtosis_antenna_mask): ``sk`` = float32 [n_chunks, n_ant, n_tbin,
        nchan] as ``kurtosis(x, tint=tint)`` returned it -> float32 of the same shape in the memory of sk, the ``mask`` of
        ``beamform(.., mask_tint=tint)``: 1 where ``lo <= sk <= hi``, else 0 (a NaN gives 0).  Thresholds that are not given come
        from ``sk_thresholds(M, sigma)`` with M the frames of a full bin; a partial last bin that is not the chunk's only bin gets
        ``sk_thresholds(M_last, sigma)`` of its own count whatever ``lo`` and ``hi`` are, and (-inf, inf) below 2 frames, where sk
        is exactly 1."""
        tint = int(tint)
        keep, ptr, kind, shape, span = self._sk_in(sk, tint)
        if lo is None or hi is None:
            t_lo, t_hi = sk_thresholds(span, sigma)
            lo, hi = (t_lo if lo is None else lo), (t_hi if hi is None else hi)
        m_last = self.n_pts % span if span else 0
        lo_last, hi_last = sk_thresholds(m_last, sigma) if m_last >= 2 else (-np.inf, np.inf)
        mask, m_ptr = self._out_like_rows(shape, np.float32, keep, _is_torch(keep))
        self._sk_keep = keep
        self._check(self._lib.fxc_kurtosis_antenna_mask(self._h, ptr, int(shape[0]), tint, float(lo), float(hi), float(lo_last),
                                                        float(hi_last), m_ptr, kind))
        return mask

    def _out_like_x(self, out, shape, device, like, name="out", dtype=np.float32):
        """a result of ``shape`` and ``dtype`` in the memory of the samples: ``out`` checked, or a new array / tensor -> (array, ptr)"""
        kind = np.dtype(dtype).name
        if out is not None:
            if _is_torch(out) != device:
                raise ValueError("{} must be of the same kind (host array / CUDA tensor) as x".format(name))
            if device:
                if out.dtype != _torch_dtype(dtype) or tuple(out.shape) != shape or not out.is_contiguous() or not out.is_cuda or \
                        out.device.index != self.device:
                    raise ValueError("{} must be a contiguous {} CUDA tensor of shape {}".format(name, kind, shape))
            elif out.dtype != dtype or out.shape != shape or not out.flags.c_contiguous or not out.flags.writeable:
                raise ValueError("{} must be a writable C-contiguous {} array of shape {}".format(name, kind, shape))
        elif device:
            import torch
            out = torch.empty(shape, dtype=_torch_dtype(dtype), device=like.device)
        else:
            out = np.empty(shape, dtype=dtype)
        return out, (out.data_ptr() if device else out.ctypes.data)

    def _time_bins(self, tint):
        """time bins of ``tint`` frames, 0: the whole chunk (h_tools.h time_bins) -> (frames of a full bin, bins a chunk).  A ``tint``
        out of range gives the shape of one bin, and the C call answers"""
        span = tint if 0 < tint <= self.n_pts else self.n_pts
        return span, (-(-self.n_pts // span) if span else 1)

    def _sk_in(self, sk, tint):
        """sk as ``kurtosis(x, tint=tint)`` returned it, numpy or a CUDA tensor on the plan's device -> (keep, ptr, mem_kind, shape,
        frames of a full bin)"""
        self._sync_stream()
        device = _is_torch(sk)
        keep, ptr = self._like(sk, "sk", device)
        span, n_tbin = self._time_bins(tint)
        shape = tuple(keep.shape)
        if len(shape) != 4 or shape[1:] != (self.n_ant, n_tbin, self.nchan):
            raise ValueError("sk must have shape (n_chunks, {}, {}, {}), got {}".format(self.n_ant, n_tbin, self.nchan, shape))
        return keep, ptr, (_lib.FXC_MEM_DEVICE if device else _lib.FXC_MEM_HOST), shape, span

    def kurtosis(self, x, tint=0, return_power=False, out=None):
        """Spectral kurtosis of every antenna's spectra (fxcorr.h fxc_kurtosis): ``x`` = [n_chunks, n_ant, num_samp] complex64
        (numpy, or a CUDA tensor on the plan's device) -> sk float32 [n_chunks, n_ant, n_tbin, nchan] over time bins of ``tint``
        frames (0: the whole chunk; 1 is refused; the last may be partial), bins in the rows' fftshifted order: 1 for Gaussian
        noise whatever its power, 0 for a steady carrier, about 1 / d - 1 at duty cycle d.  With ``return_power`` -> (sk, power),
        power = the mean of |f|^2 over the same bins.  The samples are taken as delivered: no shifts, tables, track or gains, and
        the track's counter stays.  numpy in, numpy out; CUDA tensor in, CUDA tensor out.  ``out``: an array / tensor of the
        result's shape to receive sk -- with ``return_power`` a pair (sk, power).  The loop with the detectors::

            w = plan.kurtosis_weights(plan.kurtosis(x))
            rows = plan.fx_rows(x)
            w = plan.flag_rows(rows, prior=w)
            vis, wsum = plan.average_rows(rows, weights=w)
        """
        ptr, kind, n, keep = self._in(x, (self.n_ant, self.num_samp))
        device = kind == _lib.FXC_MEM_DEVICE
        tint = int(tint)
        shape = (n, self.n_ant, self._time_bins(tint)[1], self.nchan)
        if return_power:
            if out is not None and (not isinstance(out, (tuple, list)) or len(out) != 2):
                raise ValueError("with return_power, out must be a pair (sk, power)")
            o_sk, o_pw = out if out is not None else (None, None)
        else:
            if isinstance(out, (tuple, list)):
                raise ValueError("out is a pair only with return_power")
            o_sk, o_pw = out, None
        sk, s_ptr = self._out_like_x(o_sk, shape, device, keep)
        power, p_ptr = self._out_like_x(o_pw, shape, device, keep, "out's power") if return_power else (None, None)
        if device and not self._follow:      # a stream of the plan's own: torch's may still be using the blocks it handed out
            import torch
            torch.cuda.current_stream(keep.device).synchronize()
        self._sk_keep = keep                 # until the next call: the queued kernels read it
        self._check(self._lib.fxc_kurtosis(self._h, ptr, s_ptr, p_ptr, n, kind, tint))
        return (sk, power) if return_power else sk

    def kurtosis_weights(self, sk, lo=None, hi=None, tint=0, sigma=3.0):
        """The row weights from ``kurtosis``'s sk (fxcorr.h fxc_kurtosis_weights): ``sk`` = float32 [n_chunks, n_ant, n_tbin, nchan]
        as ``kurtosis(x, tint=tint)`` returned it -> float32 [n_chunks, n_baselines, nchan] in the memory of sk, the array
        ``flag_rows(prior=)``, ``solve_gains(weights=)``, ``fringe_fit(weights=)`` and ``average_rows(weights=)`` take: 1 where
        ``lo <= sk <= hi`` in every counted bin of both antennas of the baseline, else 0 (a NaN gives 0).  A partial last bin is
        not counted unless it is the chunk's only bin.  Thresholds that are not given come from ``sk_thresholds(M, sigma)``
        with M the frames of a full bin."""
        tint = int(tint)
        keep, ptr, kind, shape, span = self._sk_in(sk, tint)
        if lo is None or hi is None:
            t_lo, t_hi = sk_thresholds(span, sigma)
            lo, hi = (t_lo if lo is None else lo), (t_hi if hi is None else hi)
        weights, w_ptr = self._out_like_rows((shape[0], self.n_baselines, self.nchan), np.float32, keep, _is_torch(keep))
        self._sk_keep = keep
        self._check(self._lib.fxc_kurtosis_weights(self._h, ptr, int(shape[0]), tint, float(lo), float(hi), w_ptr, kind))
        return weights

    # -- F + X ------------------------------------------------------------------------------
    def fx_accumulate(self, x, remove_dc=False, c128=False):
        """x: [n_chunks, n_ant, num_samp] complex64; adds into the plan's accumulator (async).  ``remove_dc`` / ``c128``
        as for ``fx_rows``."""
        ptr, kind, n, keep = self._in(x, (self.n_ant, self.num_samp), c128)
        if remove_dc or self._fmt != _lib.FXC_IQ_C64:
            self._check(self._lib.fxc_fx_accumulate_iq(self._h, ptr, n, kind, self._fmt, int(bool(remove_dc))))
        else:
            self._check(self._lib.fxc_fx_accumulate(self._h, ptr, n, kind))
        return n

    def fx_rows(self, x, mode="SPECTRUM", bandwidth=1.0, remove_dc=False, out=None, c128=False):
        """One visibility row per chunk (the reference's ``_run_task`` result, effex.py:490-527).

        SPECTRUM -> [n_chunks, n_rows, nchan] complex64; CONTINUUM/TEST -> [n_chunks, n_rows]
        complex128.  ``remove_dc``: the per-chunk, per-antenna mean is removed on the device first (effex.py:394-395;
        ``fxc_fx_rows_iq``).  ``c128``: complex128 input crosses to the device as it is and is narrowed there (after the
        DC removal) instead of on the host.  ``out``: an array / tensor of the result's shape to receive the rows -- a
        ``pinned_empty`` array is written by the device itself.
        """
        m = MODES[mode.upper()]
        ptr, kind, n, keep = self._in(x, (self.n_ant, self.num_samp), c128)
        if m == _lib.FXC_MODE_SPECTRUM:
            out, optr = self._out(x, (n, self.n_rows, self.nchan), np.complex64, out)
        else:
            out, optr = self._out(x, (n, self.n_rows), np.complex128, out)
        if self._to_pinned:
            kind = _lib.FXC_MEM_DEVICE_TO_PINNED
        if remove_dc or self._fmt != _lib.FXC_IQ_C64:
            self._check(self._lib.fxc_fx_rows_iq(self._h, ptr, optr, n, kind, m, float(bandwidth), self._fmt,
                                                 int(bool(remove_dc))))
        else:
            self._check(self._lib.fxc_fx_rows(self._h, ptr, optr, n, kind, m, float(bandwidth)))
        return out

    def acc_reset(self):
        self._sync_stream()
        self._check(self._lib.fxc_acc_reset(self._h))

    def acc_export(self, sums):
        """sums: CUDA complex128 tensor [n_rows*nchan + 1] (raw sums + {spectra count})."""
        import torch
        if sums.dtype != torch.complex128 or sums.numel() != self.n_rows * self.nchan + 1 \
                or not sums.is_contiguous() or not sums.is_cuda:
            raise ValueError("sums must be a contiguous CUDA complex128 tensor of n_rows*nchan + 1 elements")
        self._sync_stream()
        self._check(self._lib.fxc_acc_export(self._h, sums.data_ptr()))
        return sums

    def new_sums(self):
        import torch
        return torch.empty(self.n_rows * self.nchan + 1, dtype=torch.complex128,
                           device=torch.device("cuda", self.device))

    def finalize_sums(self, sums=None, mode="SPECTRUM", bandwidth=1.0):
        """Visibilities from exported (and reduced) sums; ``sums=None``: the plan's own copy, as ``reduce`` leaves it."""
        m = MODES[mode.upper()]
        shape = (self.n_rows, self.nchan) if m == _lib.FXC_MODE_SPECTRUM else (self.n_rows,)
        out = np.empty(shape, dtype=np.complex128)
        self._sync_stream()
        ptr = sums.data_ptr() if sums is not None else None
        self._check(self._lib.fxc_finalize_sums(self._h, ptr, out.ctypes.data, m, float(bandwidth)))
        return out

    def reduce(self, comm=None, root=0):
        """``fxc_reduce``: export the accumulator into the plan and sum it over the ranks of ``comm`` (an ``RcclComm``;
        None = single rank) on the plan's stream — ncclReduce to ``root``, ncclAllReduce if ``root`` is None."""
        self._sync_stream()
        handle = comm.handle if comm is not None else None
        self._check(self._lib.fxc_reduce(self._h, handle, -1 if root is None else int(root)))

    def finalize(self, mode="SPECTRUM", bandwidth=1.0, reset=True):
        """Mean over everything accumulated, times conj(rot), fft-shifted -> numpy complex128."""
        self._sync_stream()
        m = MODES[mode.upper()]
        shape = (self.n_rows, self.nchan) if m == _lib.FXC_MODE_SPECTRUM else (self.n_rows,)
        out = np.empty(shape, dtype=np.complex128)
        self._check(self._lib.fxc_finalize(self._h, out.ctypes.data, m, float(bandwidth), int(bool(reset))))
        return out

    def _result(self, mode_code):
        shape = (self.n_rows, self.nchan) if mode_code == _lib.FXC_MODE_SPECTRUM else (self.n_rows,)
        return np.empty(shape, dtype=np.complex128)

    def finalize_async(self, mode="SPECTRUM", bandwidth=1.0, reset=True, out=None):
        """Queue ``finalize`` on the plan's stream and return at once (``fxc_finalize_async``): on the 2-antenna fast
        paths the fold of the last ``fx_accumulate``'s partial sums, the finalize, the reset and the write into pinned
        host memory are one kernel.  Collect with ``finalize_wait()``; up to two results may be outstanding, so the
        next integration can be queued before the host waits for this one.  ``out``: a complex128 array of the result's
        shape (best: ``pinned_empty``) the device delivers the result into (``fxc_finalize_async_to``);
        ``finalize_wait()`` then returns that array without copying anything."""
        self._sync_stream()
        m = MODES[mode.upper()]
        if out is not None:
            want = self._result(m).shape
            if out.dtype != np.complex128 or out.shape != want or not out.flags.c_contiguous or not out.flags.writeable:
                raise ValueError("out must be a writable C-contiguous complex128 array of shape {}".format(want))
            self._check(self._lib.fxc_finalize_async_to(self._h, out.ctypes.data, m, float(bandwidth), int(bool(reset))))
            self._queued.append((m, out))
            return
        self._check(self._lib.fxc_finalize_async(self._h, m, float(bandwidth), int(bool(reset))))
        self._queued.append(m)

    def finalize_sums_async(self, sums=None, mode="SPECTRUM", bandwidth=1.0):
        """``finalize_sums`` without the wait (``fxc_finalize_sums_async``); collect with ``finalize_wait()``."""
        self._sync_stream()
        m = MODES[mode.upper()]
        ptr = sums.data_ptr() if sums is not None else None
        self._check(self._lib.fxc_finalize_sums_async(self._h, ptr, m, float(bandwidth)))
        self._queued.append(m)

    def finalize_wait(self):
        """The oldest queued finalize result as numpy complex128 (blocks on that result's event only)."""
        if not self._queued:
            raise _lib.FxcError(_lib.FXC_ERR_STATE, "no finalize result outstanding")
        head = self._queued[0]
        out = head[1] if isinstance(head, tuple) else self._result(head)
        self._check(self._lib.fxc_finalize_wait(self._h, out.ctypes.data))
        self._queued.pop(0)
        return out

    def warm_bytes(self):
        """Have the byte-ingest build of the kernel for this channel count ready before the first byte call: a plan builds it
        lazily, inside that call -- up to seconds of hiprtc in the middle of a live stream when the shape is neither pre-built nor
        cached.  ``fxc_spec_probe`` runs the same search now and leaves the code object in the run-time cache (a file read later).
        No effect on shapes without such a kernel; returns True if one is there."""
        if not (self.info["specialised"] & 1):
            return False
        return self._lib.fxc_spec_probe(int(self.nchan), int(self.ntaps), 1, None, None, 0) == 0

    @property
    def finalize_pending(self):
        return int(self._lib.fxc_finalize_pending(self._h))

    def sync(self):
        self._check(self._lib.fxc_sync(self._h))

    # -- input conditioning (device resident) -----------------------------------------------
    def remove_dc(self, x, out=None):
        """Per-stream DC removal (effex.py:394-395) of a CUDA complex64 tensor [..., num_samp]; in place
        unless ``out`` is given."""
        import torch
        if x.dtype != torch.complex64 or not x.is_cuda or not x.is_contiguous() or x.shape[-1] != self.num_samp:
            raise ValueError("x must be a contiguous CUDA complex64 tensor [..., num_samp]")
        out = x if out is None else out
        self._sync_stream()
        self._check(self._lib.fxc_remove_dc(self._h, x.data_ptr(), out.data_ptr(), x.numel() // self.num_samp))
        return out

    def convert_u8(self, iq_u8, remove_dc=True):
        """RTL-SDR interleaved uint8 I,Q [..., num_samp, 2] (CUDA) -> complex64 [..., num_samp]."""
        import torch
        if iq_u8.dtype != torch.uint8 or not iq_u8.is_cuda or not iq_u8.is_contiguous() \
                or tuple(iq_u8.shape[-2:]) != (self.num_samp, 2):
            raise ValueError("iq_u8 must be a contiguous CUDA uint8 tensor [..., num_samp, 2]")
        self._sync_stream()
        out = torch.empty(iq_u8.shape[:-1], dtype=torch.complex64, device=iq_u8.device)
        self._check(self._lib.fxc_convert_u8(self._h, iq_u8.data_ptr(), out.data_ptr(), out.numel() // self.num_samp,
                                             int(bool(remove_dc))))
        return out

    def _in_u8(self, iq_u8):
        """uint8 I,Q [n_chunks, n_ant, num_samp, 2] (CUDA tensor or host array) -> (pointer, mem_kind, n, keepalive)."""
        tail = (self.n_ant, self.num_samp, 2)
        self._sync_stream()
        if _is_torch(iq_u8):
            import torch
            if iq_u8.dtype != torch.uint8 or not iq_u8.is_cuda or not iq_u8.is_contiguous():
                raise ValueError("device input must be a contiguous uint8 CUDA tensor")
            shape, ptr, kind, keep = tuple(iq_u8.shape), iq_u8.data_ptr(), _lib.FXC_MEM_DEVICE, iq_u8
        else:
            keep = np.ascontiguousarray(iq_u8, dtype=np.uint8)
            shape, ptr, kind = keep.shape, keep.ctypes.data, _lib.FXC_MEM_HOST
        if len(shape) == 3:
            shape = (1,) + shape
        if len(shape) != 4 or tuple(shape[1:]) != tail:
            raise ValueError("expected shape [n, {}, {}, 2], got {}".format(self.n_ant, self.num_samp, shape))
        return ptr, kind, shape[0], keep

    def fx_rows_u8(self, iq_u8, mode="SPECTRUM", bandwidth=1.0, remove_dc=True, out=None):
        """``fx_rows`` straight from RTL-SDR bytes: uint8 I,Q [n_chunks, n_ant, num_samp, 2], converted as pyrtlsdr does
        (effex.py:652) with the per-stream mean removed (effex.py:394-395) unless ``remove_dc`` is false.  On fused
        plans the F+X kernel reads the bytes itself."""
        m = MODES[mode.upper()]
        ptr, kind, n, keep = self._in_u8(iq_u8)
        if m == _lib.FXC_MODE_SPECTRUM:
            out, optr = self._out(iq_u8, (n, self.n_rows, self.nchan), np.complex64, out)
        else:
            out, optr = self._out(iq_u8, (n, self.n_rows), np.complex128, out)
        if self._to_pinned:
            kind = _lib.FXC_MEM_DEVICE_TO_PINNED
        self._check(self._lib.fxc_fx_rows_u8(self._h, ptr, optr, n, kind, m, float(bandwidth), int(bool(remove_dc))))
        return out

    def fx_accumulate_u8(self, iq_u8, remove_dc=True):
        """``fx_accumulate`` straight from RTL-SDR bytes (see ``fx_rows_u8``)."""
        ptr, kind, n, keep = self._in_u8(iq_u8)
        self._check(self._lib.fxc_fx_accumulate_u8(self._h, ptr, n, kind, int(bool(remove_dc))))
        return n

    # -- delay calibration ------------------------------------------------------------------
    def estimate_delay(self, iq_0, iq_1, rate):
        """Sub-sample delay between two equal-length streams in seconds (effex.py:583-627)."""
        if len(iq_0) != len(iq_1):
            raise AssertionError('Algorithm assumes input complex timeseries are of equal length.')
        n = int(len(iq_0))
        self._sync_stream()
        if _is_torch(iq_0) or _is_torch(iq_1):
            import torch
            for t in (iq_0, iq_1):
                if not _is_torch(t) or t.dtype != torch.complex64 or not t.is_cuda or t.dim() != 1 \
                        or t.device.index != self.device:
                    raise ValueError("device inputs must both be 1-D complex64 CUDA tensors on device {}".format(self.device))
            a, b, kind = iq_0.contiguous(), iq_1.contiguous(), _lib.FXC_MEM_DEVICE
            pa, pb = a.data_ptr(), b.data_ptr()
        else:
            a = np.ascontiguousarray(iq_0, dtype=np.complex64)
            b = np.ascontiguousarray(iq_1, dtype=np.complex64)
            kind, pa, pb = _lib.FXC_MEM_HOST, a.ctypes.data, b.ctypes.data
        out = ctypes.c_double()
        self._check(self._lib.fxc_estimate_delay(self._h, pa, pb, n, kind, float(rate), ctypes.byref(out)))
        return out.value

    def estimate_delays(self, x, rate, ref=0):
        """Delays of every antenna against antenna ``ref`` in one call: x = [n_ant, n] complex64 (numpy, or a CUDA tensor on
        the plan's device) -> float64 [n_ant]; entry a is ``estimate_delay(x[ref], x[a], rate)`` bit for bit, entry ref 0."""
        self._sync_stream()
        if _is_torch(x):
            import torch
            if x.dtype != torch.complex64 or not x.is_cuda or x.dim() != 2 or x.device.index != self.device:
                raise ValueError("device input must be a 2-D complex64 CUDA tensor on device {}".format(self.device))
            keep = x.contiguous()
            ptr, kind = keep.data_ptr(), _lib.FXC_MEM_DEVICE
        else:
            keep = np.ascontiguousarray(x, dtype=np.complex64)
            if keep.ndim != 2:
                raise ValueError("x must have shape (n_ant, n)")
            ptr, kind = keep.ctypes.data, _lib.FXC_MEM_HOST
        if tuple(keep.shape)[0] != self.n_ant:
            raise ValueError("x must have shape ({}, n), got {}".format(self.n_ant, tuple(keep.shape)))
        out = np.zeros(self.n_ant, dtype=np.float64)
        self._check(self._lib.fxc_estimate_delays(self._h, ptr, int(keep.shape[1]), kind, float(rate), int(ref), out.ctypes.data))
        return out

    def _rows_in(self, rows, allow_2d):
        """SPECTRUM rows as a call takes them -> (keep, ptr, mem_kind, shape): ``keep`` = the contiguous complex64 array ``ptr``
        points into, ``shape`` = its (n_chunks, n_rows, nchan); with ``allow_2d`` a 2-D [n_rows, nchan] array is one chunk."""
        if _is_torch(rows):
            import torch
            if rows.dtype != torch.complex64 or not rows.is_cuda or rows.device.index != self.device:
                raise ValueError("device input must be a complex64 CUDA tensor on device {}".format(self.device))
            keep = rows.contiguous()
            ptr, kind = keep.data_ptr(), _lib.FXC_MEM_DEVICE
        else:
            keep = np.ascontiguousarray(rows, dtype=np.complex64)
            ptr, kind = keep.ctypes.data, _lib.FXC_MEM_HOST
        shape = tuple(keep.shape)
        if allow_2d and len(shape) == 2:
            shape = (1,) + shape
        if len(shape) != 3 or (allow_2d and shape[0] < 1) or shape[1:] != (self.n_rows, self.nchan):
            raise ValueError("rows must have shape (n_chunks, {}, {}), got {}".format(self.n_rows, self.nchan, tuple(keep.shape)))
        return keep, ptr, kind, shape

    def _like(self, x, name, device, dtype=np.float32, move_to=None, says=("rows: a CUDA tensor for device rows, numpy for host rows", None)):
        """``x`` of ``dtype`` (``weights``, ``prior``, ``mask``, ``sk``) in the memory of the rows, or of the samples x -> (keep, ptr).
        ``move_to``: the torch device a numpy ``x`` is moved to when the samples are on the device; ``says``: what the messages
        call that memory, and the operand on the device where it is not "device <name>" """
        if device and move_to is not None and not _is_torch(x):
            import torch
            x = torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).to(move_to)
        if _is_torch(x) != device:
            raise ValueError("{} must be in the memory of {}".format(name, says[0]))
        if device:
            import torch
            if x.dtype != _torch_dtype(dtype) or not x.is_cuda or x.device.index != self.device:
                raise ValueError("{} must be a {} CUDA tensor on device {}".format(says[1] or "device " + name, np.dtype(dtype).name,
                                                                                   self.device))
            keep = x.contiguous()
            return keep, keep.data_ptr()
        keep = np.ascontiguousarray(x, dtype=dtype)
        return keep, keep.ctypes.data

    def _weights_in(self, x, name, keep_rows, n_chunks, either=False):
        """``_like`` of ``x`` shaped [n_chunks, n_baselines, nchan], 2-D for 2-D rows (``either``: or 3-D, the shape the message names)"""
        keep, ptr = self._like(x, name, _is_torch(keep_rows))
        full = (n_chunks, self.n_baselines, self.nchan)
        want = full[1:] if keep_rows.ndim == 2 else full
        got = tuple(keep.shape)
        if got != want and not (either and got == full):
            raise ValueError("{} must have shape {}, got {}".format(name, full if either else want, got))
        return keep, ptr

    @staticmethod
    def _n_spans(n_chunks, span):
        """intervals (windows) of ``span`` chunks in ``n_chunks``; 0 or beyond the chunks means all of them in one"""
        return -(-n_chunks // (min(span, n_chunks) if span > 0 else n_chunks))

    def _out_like_rows(self, shape, dtype, keep, device):
        """an output of a call in the memory of the rows ``keep`` -> (array, ptr); ``dtype`` = the numpy type"""
        if device:
            import torch
            out = torch.empty(shape, dtype=_torch_dtype(dtype), device=keep.device)      # the call writes every element
            if not self._follow:      # a stream of the plan's own: torch's may still be using the block it handed out
                torch.cuda.current_stream(keep.device).synchronize()
            return out, out.data_ptr()
        out = np.zeros(shape, dtype=dtype)
        return out, out.ctypes.data

    def fringe_fit(self, rows, bandwidth, frequency, ref=0, pad=2, weights=None, baselines="ref", min_snr=None,
                   return_baselines=False):
        """Residual delay and delay rate of every antenna against antenna ``ref`` from SPECTRUM rows (fxcorr.h fxc_fringe_fit):
        ``rows`` = [n_chunks, n_rows, nchan] complex64 as ``fx_rows(x)`` returns them (numpy, or a CUDA tensor on the plan's
        device) -> (delays_s, rates_s_per_chunk, snr), float64 [n_ant] each, entry ``ref`` 0.  Added to what
        ``set_delay_track`` was given they stop the fringes.

        ``weights``, ``baselines``, ``min_snr`` and ``return_baselines`` (fxcorr.h fxc_fringe_fit_weighted; with all four at
        their defaults the call is fxc_fringe_fit as it was): ``weights`` = float32 [n_chunks, n_baselines, nchan], numpy for
        host rows or a CUDA tensor on the plan's device for device rows, for instance from ``flag_rows``; a sample counts iff
        its weight is > 0, and what a sample that does not count holds (NaN, a tone) is never used.  ``baselines`` = "ref": the
        baselines to ``ref`` alone; "all": every baseline is fitted, those of snr >= ``min_snr`` (None: the threshold of a 1e-3
        false-alarm probability on the padded grid) are kept, and the antennas are solved for by least squares over them -- an
        antenna whose baseline to ``ref`` is flagged is still measured, one that no kept baseline reaches gets 0 with snr 0.
        With ``return_baselines`` a fourth result, float64 [n_baselines, 3] = (delay, rate, snr) per fitted baseline (b minus
        a of row (a, b)), is returned.  The loop with the detector::

            w = plan.flag_rows(rows)
            d, r, s = plan.fringe_fit(rows, bw, fc, weights=w, baselines="all")
        """
        self._sync_stream()
        keep, ptr, kind, shape = self._rows_in(rows, allow_2d=False)
        if baselines not in ("ref", "all"):
            raise ValueError("baselines must be 'ref' or 'all', got {!r}".format(baselines))
        delays = np.zeros(self.n_ant, dtype=np.float64)
        rates = np.zeros(self.n_ant, dtype=np.float64)
        snr = np.zeros(self.n_ant, dtype=np.float64)
        if weights is None and baselines == "ref" and min_snr is None and not return_baselines:
            self._check(self._lib.fxc_fringe_fit(self._h, ptr, int(shape[0]), kind, float(bandwidth), float(frequency), int(ref),
                                                 int(pad), delays.ctypes.data, rates.ctypes.data, snr.ctypes.data))
            return delays, rates, snr
        w_keep, w_ptr = None, None
        if weights is not None:
            w_keep, w_ptr = self._weights_in(weights, "weights", keep, shape[0])
        base = np.zeros((self.n_baselines, 3), dtype=np.float64)
        mode = _lib.FXC_FRINGE_ALL if baselines == "all" else _lib.FXC_FRINGE_REF
        self._check(self._lib.fxc_fringe_fit_weighted(self._h, ptr, w_ptr, int(shape[0]), kind, float(bandwidth), float(frequency),
                                                      int(ref), int(pad), mode, 0.0 if min_snr is None else float(min_snr),
                                                      delays.ctypes.data, rates.ctypes.data, snr.ctypes.data,
                                                      base.ctypes.data if return_baselines else None))
        return (delays, rates, snr, base) if return_baselines else (delays, rates, snr)

    def solve_gains(self, rows, interval=0, ref=0, iters=50, weights=None, model=None):
        """Every antenna's complex gain per bin from SPECTRUM rows of a calibrator (fxcorr.h fxc_solve_gains): ``rows`` =
        [n_chunks, n_rows, nchan] complex64 as ``fx_rows(x)`` returns them (numpy, or a CUDA tensor on the plan's device; a 2-D
        [n_rows, nchan] array such as an integration from ``finalize`` is one chunk) -> (gains [n_int, n_ant, nchan]
        complex128, step [n_int, nchan] float64), one solution per ``interval`` chunks (0: one over all), bins in the rows'
        order, antenna ``ref`` real.  ``set_gains(gains[s])`` applies a solution; under a delay track ``set_track_gains(gains,
        interval)`` applies all of them.

        ``weights`` and ``model`` (fxcorr.h fxc_solve_gains_weighted; with both None the call is fxc_solve_gains as it was):
        ``weights`` = float32 [n_chunks, n_baselines, nchan] ([n_baselines, nchan] for 2-D rows), numpy for host rows or a
        CUDA tensor on the plan's device for device rows; a sample counts iff its weight is > 0.  ``model`` = the model
        visibilities, anything numpy casts to complex64, [n_baselines, nchan] or [n_int, n_baselines, nchan] (for instance
        ``offset_source_model``)."""
        self._sync_stream()
        keep, ptr, kind, shape = self._rows_in(rows, allow_2d=True)
        interval = int(interval)
        n_int = self._n_spans(shape[0], interval)
        gains = np.zeros((n_int, self.n_ant, self.nchan), dtype=np.complex128)
        step = np.zeros((n_int, self.nchan), dtype=np.float64)
        if weights is None and model is None:
            self._check(self._lib.fxc_solve_gains(self._h, ptr, int(shape[0]), kind, interval, int(ref), int(iters), gains.ctypes.data,
                                                  step.ctypes.data))
            return gains, step
        w_keep, w_ptr = None, None
        if weights is not None:
            w_keep, w_ptr = self._weights_in(weights, "weights", keep, shape[0], either=True)
        m_keep, m_ptr, n_model = None, None, 0
        if model is not None:
            m_keep = np.ascontiguousarray(np.asarray(model).astype(np.complex64))
            if m_keep.ndim == 2:
                m_keep = m_keep[None]
            if m_keep.ndim != 3 or m_keep.shape[0] not in (1, n_int) or m_keep.shape[1:] != (self.n_baselines, self.nchan):
                raise ValueError("model must have shape ({1}, {2}) or ({0}, {1}, {2}), got {3}".format(
                    n_int, self.n_baselines, self.nchan, tuple(np.shape(model))))
            m_ptr, n_model = m_keep.ctypes.data, int(m_keep.shape[0])
        self._check(self._lib.fxc_solve_gains_weighted(self._h, ptr, w_ptr, int(shape[0]), kind, m_ptr, n_model, interval, int(ref),
                                                       int(iters), gains.ctypes.data, step.ctypes.data))
        return gains, step

    def flag_rows(self, rows, window=0, time_threshold=20.0, freq_threshold=8.0, half_width=8, iters=2, prior=None,
                  return_counts=False):
        """The weights ``solve_gains(weights=)`` takes, from the rows alone (fxcorr.h fxc_flag_rows): ``rows`` = [n_chunks,
        n_rows, nchan] complex64 as ``fx_rows(x)`` returns them, fringes stopped (numpy, or a CUDA tensor on the plan's device;
        a 2-D [n_rows, nchan] array is one chunk) -> float32 [n_chunks, n_baselines, nchan] in the memory of rows: numpy for
        host rows, a CUDA tensor for device rows, which goes into ``solve_gains`` without touching the host.  Per ``window``
        chunks (0: all) a sample further than ``time_threshold`` median deviations from its (baseline, bin) column's complex
        median gets weight 0 (``iters`` rounds), then a bin whose level or scatter stands ``freq_threshold`` median deviations
        out of the bins within ``half_width`` loses its column.  The thresholds are multiples of the median deviation, not
        sigmas.  ``prior`` = float32 weights in the memory of rows: a sample whose prior is not > 0 is ignored, a surviving one
        keeps its prior.  With ``return_counts`` -> (weights, counts [n_win, n_baselines, 3] int64: not live at the start,
        flagged in time, flagged in frequency)."""
        self._sync_stream()
        keep, ptr, kind, shape = self._rows_in(rows, allow_2d=True)
        device = kind == _lib.FXC_MEM_DEVICE
        p_keep, p_ptr = None, None
        if prior is not None:
            p_keep, p_ptr = self._weights_in(prior, "prior", keep, shape[0])
        window = int(window)
        counts = np.zeros((self._n_spans(shape[0], window), self.n_baselines, 3), dtype=np.int64)
        weights, w_ptr = self._out_like_rows((shape[0], self.n_baselines, self.nchan), np.float32, keep, device)
        self._check(self._lib.fxc_flag_rows(self._h, ptr, p_ptr, int(shape[0]), kind, window, float(time_threshold),
                                            float(freq_threshold), int(half_width), int(iters), w_ptr, counts.ctypes.data))
        if keep.ndim == 2:
            weights = weights[0]
        return (weights, counts) if return_counts else weights

    def average_rows(self, rows, weights=None, time_bin=0, freq_bin=1):
        """The weighted mean of SPECTRUM rows over intervals of chunks and bins of channels (fxcorr.h fxc_average_rows): ``rows``
        = [n_chunks, n_rows, nchan] complex64 as ``fx_rows(x)`` returns them (numpy, or a CUDA tensor on the plan's device; a 2-D
        [n_rows, nchan] array is one chunk), ``weights`` = float32 [n_chunks, n_baselines, nchan] in the memory of rows, for
        instance from ``flag_rows`` (None: every weight 1); a sample counts iff its weight is > 0, and what a sample that does
        not count holds is never used.  -> (vis [n_int, n_baselines, n_out] complex64, wsum [n_int, n_baselines, n_out] float32)
        in the memory of rows: one interval per ``time_bin`` chunks (0: one over all), one output bin per ``freq_bin`` input bins
        (256 at most; the last may be partial, ``averaged_freqs`` gives the bins' frequencies); a cell without a counted sample
        is 0 with weight 0.  At ``freq_bin`` 1 the pair goes straight into ``solve_gains(vis, weights=wsum)``, ``flag_rows(vis,
        prior=wsum)`` or ``fringe_fit(vis, ..)``."""
        self._sync_stream()
        keep, ptr, kind, shape = self._rows_in(rows, allow_2d=True)
        device = kind == _lib.FXC_MEM_DEVICE
        w_keep, w_ptr = None, None
        if weights is not None:
            w_keep, w_ptr = self._weights_in(weights, "weights", keep, shape[0])
        time_bin, freq_bin = int(time_bin), int(freq_bin)
        out_shape = (self._n_spans(shape[0], time_bin), self.n_baselines, -(-self.nchan // max(freq_bin, 1)))
        vis, v_ptr = self._out_like_rows(out_shape, np.complex64, keep, device)
        wsum, s_ptr = self._out_like_rows(out_shape, np.float32, keep, device)
        self._check(self._lib.fxc_average_rows(self._h, ptr, w_ptr, int(shape[0]), kind, time_bin, freq_bin, v_ptr, s_ptr))
        return vis, wsum

    def dedisperse(self, power, shifts, chan_weights=None, out=None, return_info=False):
        """Incoherent dedispersion of power at full time resolution (fxcorr.h fxc_dedisperse): ``power`` = float32 [n_chunks,
        n_series, n_tbin, nchan] as ``beamform(.., mode="POWER")``, ``beamform_incoherent`` or ``kurtosis(.., return_power=True)``
        return it (numpy, or a CUDA tensor on the plan's device); [n_series, n_t, nchan] and [n_t, nchan] are one chunk.
        ``shifts`` = int32 [n_dm, nchan] from ``dm_shifts`` and ``chan_weights`` = float32 [nchan] or None are numpy, or are moved to
        the host; a channel counts iff its weight is > 0 (None: all do), and what an uncounted channel holds is never used.
        -> float32 [n_series, n_dm, n_t - shifts.max()] in the memory of power ([n_dm, ..] for 2-D power): the sum over the counted
        channels of ``power[t + shifts[d, k], k]``, not normalised.  Every time bin must hold the same number of frames (``tint``
        divides ``n_pts``).  ``out``: an array / tensor of the result's shape to receive it.  ``return_info`` -> (result, (trials
        on the tiled kernel, trials on the direct kernel)).  The loop it closes::

            P = plan.beamform(x, w, tint=16, mask=m, mask_tint=16)
            sh = dm_shifts(nchan, bw, fc, dms, 16 * nchan / bw)
            ts = plan.dedisperse(P, sh, chan_weights=band_ok)      # [n_beam, n_dm, n_t - sh.max()]
        """
        self._sync_stream()
        device = _is_torch(power)
        if device:
            import torch
            if power.dtype != torch.float32 or not power.is_cuda or power.device.index != self.device:
                raise ValueError("device power must be a float32 CUDA tensor on device {}".format(self.device))
            keep = power.contiguous()
            ptr, kind = keep.data_ptr(), _lib.FXC_MEM_DEVICE
        else:
            if not isinstance(power, np.ndarray) or power.dtype != np.float32:
                raise ValueError("power must be a float32 array or CUDA tensor")
            keep = np.ascontiguousarray(power)
            ptr, kind = keep.ctypes.data, _lib.FXC_MEM_HOST
        shape = tuple(keep.shape)
        if len(shape) not in (2, 3, 4) or shape[-1] != self.nchan or min(shape) < 1:
            raise ValueError("power must have shape (n_chunks, n_series, n_tbin, {0}), (n_series, n_t, {0}) or (n_t, {0}), got {1}".format(
                self.nchan, shape))
        n_chunks, n_series, n_tbin = shape[:3] if len(shape) == 4 else ((1,) + shape[:2] if len(shape) == 3 else (1, 1, shape[0]))
        if _is_torch(shifts):
            shifts = shifts.cpu().numpy()
        shifts = np.asarray(shifts)
        if shifts.ndim != 2 or shifts.shape[1] != self.nchan or shifts.shape[0] < 1 or shifts.dtype.kind not in "iu":
            raise ValueError("shifts must be an integer array of shape (n_dm, {}), got {} {}".format(self.nchan, shifts.dtype,
                                                                                                      shifts.shape))
        n_t = n_chunks * n_tbin
        if shifts.min() < 0:
            raise ValueError("shifts must be >= 0")
        s_max = int(shifts.max())
        if s_max >= n_t:
            raise ValueError("the largest shift {} leaves no output: n_t is {}".format(s_max, n_t))
        shifts = np.ascontiguousarray(shifts, dtype=np.int32)
        w_ptr = None
        if chan_weights is not None:
            if _is_torch(chan_weights):
                chan_weights = chan_weights.cpu().numpy()
            chan_weights = np.asarray(chan_weights)
            if chan_weights.shape != (self.nchan,) or chan_weights.dtype.kind != "f":
                raise ValueError("chan_weights must be a float array of shape ({},)".format(self.nchan))
            chan_weights = np.ascontiguousarray(chan_weights, dtype=np.float32)
            w_ptr = chan_weights.ctypes.data
        n_dm = int(shifts.shape[0])
        want = (n_series, n_dm, n_t - s_max) if len(shape) != 2 else (n_dm, n_t - s_max)
        res, o_ptr = self._out_like_x(out, want, device, keep)
        if device and not self._follow:      # a stream of the plan's own: torch's may still be using the blocks it handed out
            import torch
            torch.cuda.current_stream(keep.device).synchronize()
        info = np.zeros(2, dtype=np.int64)
        self._check(self._lib.fxc_dedisperse(self._h, ptr, n_chunks, n_series, n_tbin, kind, shifts.ctypes.data, n_dm, w_ptr, o_ptr,
                                             info.ctypes.data))
        return (res, (int(info[0]), int(info[1]))) if return_info else res

    def boxcar_search(self, ts, widths=(0, 8), block=64, clip=3.0, clip_iters=2, out=None, return_stats=False):
        """Single-pulse search on dedispersed series (fxcorr.h fxc_boxcar_search): ``ts`` = float32 [..., n_t] with 1 to 3 axes, as
        ``dedisperse`` returns it (numpy, or a CUDA tensor on the plan's device).  Every row is normalised by its mean and standard
        deviation after ``clip_iters`` rounds of clipping at ``clip`` standard deviations (``clip=0``: none), matched-filtered with
        boxcars of the widths ``boxcar_widths(*widths)`` = 2^j_lo .. 2^j_hi samples, and reduced per block of ``block`` starts.
        -> (snr float32, width int32 -- the index j --, time int32 -- the absolute start) of shape ``ts.shape[:-1] + (n_blk,)``,
        ``n_blk = ceil((n_t - 2^j_lo + 1) / block)``, in the memory of ``ts``; ties go to the narrowest width, then the earliest
        start.  ``out``: three arrays / tensors of that shape to receive them.  ``return_stats`` adds a float64 numpy array [..., 3]
        of (mean, std, counted samples) per row; std = 0 marks a degenerate row, whose cells hold snr 0.  The loop it closes::

            ts = plan.dedisperse(P, sh)
            snr, w, t = plan.boxcar_search(ts)
            cands = sift_pulses(snr, w, t)
        """
        self._sync_stream()
        device = _is_torch(ts)
        if device:
            import torch
            if ts.dtype != torch.float32 or not ts.is_cuda or ts.device.index != self.device:
                raise ValueError("device series must be a float32 CUDA tensor on device {}".format(self.device))
            keep = ts.contiguous()
            ptr, kind = keep.data_ptr(), _lib.FXC_MEM_DEVICE
        else:
            if not isinstance(ts, np.ndarray) or ts.dtype != np.float32:
                raise ValueError("ts must be a float32 array or CUDA tensor")
            keep = np.ascontiguousarray(ts)
            ptr, kind = keep.ctypes.data, _lib.FXC_MEM_HOST
        shape = tuple(keep.shape)
        if len(shape) not in (1, 2, 3) or min(shape) < 1:
            raise ValueError("ts must have shape (n_series, n_dm, n_t), (n_dm, n_t) or (n_t,), got {}".format(shape))
        try:
            j_lo, j_hi = (int(j) for j in widths)
        except (TypeError, ValueError):
            raise ValueError("widths must be a pair (j_lo, j_hi)")
        n_t = shape[-1]
        if not 0 <= j_lo <= j_hi <= BOXCAR_MAX_J or (1 << j_lo) > n_t:
            raise ValueError("widths must satisfy 0 <= j_lo <= j_hi <= {} and 2^j_lo <= n_t = {}, got {}".format(BOXCAR_MAX_J, n_t,
                                                                                                              (j_lo, j_hi)))
        block, clip_iters = int(block), int(clip_iters)
        if block < 1 or not clip >= 0 or not 0 <= clip_iters <= 4:
            raise ValueError("block must be 1 or more, clip 0 or more and clip_iters within 0 .. 4")
        n_rows = int(np.prod(shape[:-1], dtype=np.int64))
        n_blk = -(-(n_t - (1 << j_lo) + 1) // block)
        want = shape[:-1] + (n_blk,)
        if out is not None and (not isinstance(out, (tuple, list)) or len(out) != 3):
            raise ValueError("out must be three arrays / tensors (snr, width, time)")
        res, ptrs = [], []
        for i, (name, dtype) in enumerate((("out[0] (snr)", np.float32), ("out[1] (width)", np.int32), ("out[2] (time)", np.int32))):
            a, a_ptr = self._out_like_x(None if out is None else out[i], want, device, keep, name=name, dtype=dtype)
            res.append(a)
            ptrs.append(a_ptr)
        if device and not self._follow:      # a stream of the plan's own: torch's may still be using the blocks it handed out
            import torch
            torch.cuda.current_stream(keep.device).synchronize()
        stats = np.zeros(shape[:-1] + (3,), dtype=np.float64) if return_stats else None
        self._check(self._lib.fxc_boxcar_search(self._h, ptr, n_rows, n_t, kind, j_lo, j_hi, block, float(clip), clip_iters, ptrs[0],
                                                ptrs[1], ptrs[2], None if stats is None else stats.ctypes.data))
        return tuple(res) + ((stats,) if return_stats else ())

    def set_gains(self, gains, delays_s=None, bandwidth=None, frequency=None, whole_samples=False):
        """Correct the rows for the per-antenna gains ``gains`` [n_ant, nchan] (one solution of ``solve_gains``, bins in the
        rows' order): antenna a's table is ``ifftshift(1 / g_a)``, 0 where g_a is 0 so that a dead channel stays zero, times
        ``rot_tables(nchan, bandwidth, frequency, delays_s)[a]`` when delays are given, handed to ``set_rot_ant``.
        ``whole_samples`` (needs delays): the delays are split as in ``set_delays(.., whole_samples=True)``."""
        if not whole_samples:
            self.set_rot_ant(gain_tables(gains, self.n_ant, self.nchan, delays_s, bandwidth, frequency))
            return
        if delays_s is None or bandwidth is None or frequency is None:
            raise ValueError("whole_samples needs delays_s, bandwidth and frequency")
        shifts, _ = split_delays(delays_s, bandwidth)
        self.set_rot_ant(gain_tables(gains, self.n_ant, self.nchan, delays_s, bandwidth, frequency, shifts=shifts))
        self.set_sample_delays(shifts)

    # -- measurement ------------------------------------------------------------------------
    def timer_start(self):
        self._check(self._lib.fxc_timer_start(self._h))

    def timer_stop(self):
        ms = ctypes.c_double()
        self._check(self._lib.fxc_timer_stop(self._h, ctypes.byref(ms)))
        return ms.value

    def kernel_profiling(self, enable):
        self._check(self._lib.fxc_kernel_profiling(self._h, int(bool(enable))))

    def kernel_time(self, reset=True):
        ms, n = ctypes.c_double(), ctypes.c_int64()
        self._check(self._lib.fxc_kernel_time(self._h, ctypes.byref(ms), ctypes.byref(n), int(bool(reset))))
        return ms.value, n.value


class FxPipeline(object):
    """Host-fed, double-buffered front end on a plan (include/fxcorr.h ``fxc_pipe_*``): push batches of host
    chunks, pop their visibility rows; H2D, compute and D2H of successive batches overlap."""

    def __init__(self, plan, chunks_per_batch, depth=2, mode="SPECTRUM", bandwidth=1.0, u8=False, remove_dc=None, fmt=None):
        """``fmt``: sample format of the batches -- 'c64' (default), 'u8' (the receivers' bytes, uint8
        [chunks, n_ant, num_samp, 2]; ``u8=True`` is the same) or 'c128'.  ``remove_dc``: the per-chunk mean is removed
        on the device (effex.py:394-395); default: on for bytes, off otherwise (``fxc_pipe_create_iq``)."""
        self.plan = plan
        self.chunks = int(chunks_per_batch)
        self.mode = MODES[mode.upper()]
        fmt = fmt or ("u8" if u8 else "c64")
        if fmt not in IQ_FORMATS:
            raise ValueError("fmt must be one of {}".format(sorted(IQ_FORMATS)))
        self.fmt = fmt
        self.u8 = fmt == "u8"
        if remove_dc is None:
            remove_dc = self.u8
        self._shape = (self.chunks, plan.n_ant, plan.num_samp) + ((2,) if self.u8 else ())
        self._dtype = _IQ_DTYPES[fmt]
        self._h = ctypes.c_void_p()
        plan._check(plan._lib.fxc_pipe_create_iq(ctypes.byref(self._h), plan._h, self.chunks, int(depth), self.mode,
                                                 float(bandwidth), IQ_FORMATS[fmt], int(bool(remove_dc))))
        import weakref
        plan._pipes.append(weakref.ref(self))      # FxPlan.close() closes its pipes first

    def push(self, x):
        x = np.ascontiguousarray(x, dtype=self._dtype)
        if x.shape != self._shape:
            raise ValueError("expected a batch of shape {}".format(self._shape))
        self.plan._check(self.plan._lib.fxc_pipe_push(self._h, x.ctypes.data))

    def acquire(self):
        """Pinned input buffer of the next free slot as a numpy view (the batch shape) to fill in place."""
        ptr = ctypes.c_void_p()
        self.plan._check(self.plan._lib.fxc_pipe_acquire(self._h, ctypes.byref(ptr)))
        n_bytes = int(np.prod(self._shape)) * np.dtype(self._dtype).itemsize
        buf = (ctypes.c_uint8 * n_bytes).from_address(ptr.value)
        return np.frombuffer(buf, dtype=self._dtype).reshape(self._shape)

    def submit(self):
        self.plan._check(self.plan._lib.fxc_pipe_submit(self._h))

    def pop(self, out=None):
        """The oldest batch's rows.  ``out``: a C-contiguous array of the batch's shape and dtype to receive them in place --
        e.g. a window of a memory-mapped row file (``effex_amd.rowsink.BinSink.reserve``): the rows then go from the pinned
        result slot straight into the page cache."""
        if self.mode == _lib.FXC_MODE_SPECTRUM:
            shape, dtype = (self.chunks, self.plan.n_rows, self.plan.nchan), np.complex64
        else:
            shape, dtype = (self.chunks, self.plan.n_rows), np.complex128
        if out is None:
            out = np.empty(shape, dtype=dtype)
        elif out.dtype != dtype or out.size != int(np.prod(shape)) or not out.flags.c_contiguous or not out.flags.writeable:
            raise ValueError("out must be a writable C-contiguous {} array of {} elements".format(np.dtype(dtype).name, int(np.prod(shape))))
        self.plan._check(self.plan._lib.fxc_pipe_pop(self._h, out.ctypes.data))
        return out

    @property
    def in_flight(self):
        return self.plan._lib.fxc_pipe_in_flight(self._h)

    def close(self):
        if self._h:
            self.plan._lib.fxc_pipe_destroy(self._h)
            self._h = ctypes.c_void_p()

    def abandon(self):
        """Give the pipe up WITHOUT freeing it: for the error path of a caller whose producer thread may still be writing
        into a pinned slot (a read that did not notice its source being closed).  The slots, and the plan they belong to,
        stay allocated for the life of the process -- a leak instead of a write into freed memory."""
        self._h = ctypes.c_void_p()
        self.plan._abandoned = True

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class RcclComm(object):
    """One rank of an RCCL communicator made by libfxcorr (``fxc_comm_*``) for ``FxPlan.reduce``.

    ``unique_id()`` on rank 0 gives the 128 bytes every rank needs; how they travel is the caller's business
    (``effex_amd.sharding.make_comm`` broadcasts them through ``torch.distributed``).  Creation is collective."""

    def __init__(self, device, rank, world_size, unique_id):
        self._lib = _lib.load()
        self.handle = ctypes.c_void_p()
        if len(unique_id) != _lib.FXC_COMM_ID_BYTES:
            raise ValueError("unique_id must be {} bytes".format(_lib.FXC_COMM_ID_BYTES))
        buf = (ctypes.c_char * _lib.FXC_COMM_ID_BYTES).from_buffer_copy(bytes(unique_id))
        _lib.check(self._lib.fxc_comm_create(ctypes.byref(self.handle), int(device), int(rank), int(world_size),
                                             ctypes.cast(buf, ctypes.c_void_p)), None)
        self.rank, self.world_size, self.device = int(rank), int(world_size), int(device)

    @staticmethod
    def unique_id():
        lib = _lib.load()
        buf = (ctypes.c_char * _lib.FXC_COMM_ID_BYTES)()
        _lib.check(lib.fxc_comm_unique_id(ctypes.cast(buf, ctypes.c_void_p)), None)
        return bytes(buf.raw)

    def info(self):
        """What the live communicator says about itself (``fxc_comm_info``): ``ranks_seen`` / ``rank_seen`` /
        ``device_seen`` are asked of the ncclComm_t (None where the bound RCCL lacks the query), ``*_given`` are what this
        object was made with; ``rccl_version``, ``async_error`` (0 = ncclSuccess), ``reduces`` queued through it."""
        d = _lib.FxcCommDesc()
        _lib.check(self._lib.fxc_comm_info(self.handle, ctypes.byref(d)), None)
        out = {name: int(getattr(d, name)) for name, _ in d._fields_}
        for key in ("ranks_seen", "rank_seen", "device_seen", "async_error"):
            if out[key] < 0:
                out[key] = None
        return out

    def probe(self):
        """Collective, blocking: every rank contributes 1.0 to one ncclAllReduce; returns the count RCCL added up."""
        n = ctypes.c_int64(0)
        _lib.check(self._lib.fxc_comm_probe(self.handle, ctypes.byref(n)), None)
        return int(n.value)

    @staticmethod
    def library():
        """(version, path) of the librccl bound at run time; raises FxcError(FXC_ERR_COMM) if none could be."""
        lib = _lib.load()
        v = ctypes.c_int(0)
        buf = ctypes.create_string_buffer(1024)
        _lib.check(lib.fxc_rccl_version(ctypes.byref(v), buf, len(buf)), None)
        return int(v.value), buf.value.decode("utf-8", "replace")

    def close(self):
        if getattr(self, "handle", None):
            self._lib.fxc_comm_destroy(self.handle)
            self.handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def synth_fill(x, seed, first_chunk=0, delays=None, stream=None):
    """Fill a CUDA complex64 tensor [n_chunks, n_ant, num_samp] with the synthetic stream of
    ``effex_amd.synth`` (bit-identical), generated on the device."""
    import torch
    from . import synth
    lib = _lib.load()
    if x.dtype != torch.complex64 or not x.is_cuda or not x.is_contiguous() or x.dim() != 3:
        raise ValueError("x must be a contiguous CUDA complex64 tensor [n_chunks, n_ant, num_samp]")
    n_chunks, n_ant, num_samp = x.shape
    if delays is None:
        delays = synth.DEFAULT_DELAYS
    d = np.ascontiguousarray(delays[:n_ant], dtype=np.int32)
    if len(d) < n_ant:
        raise ValueError("not enough delays for n_ant")
    tone = synth.tone_table()
    if stream is None:
        stream = torch.cuda.current_stream(x.device).cuda_stream
    rc = lib.fxc_synth_fill(x.device.index, ctypes.c_void_p(int(stream)), x.data_ptr(), int(seed), int(first_chunk),
                            n_chunks, n_ant, num_samp, d.ctypes.data, tone.ctypes.data, len(tone))
    _lib.check(rc, None)
    return x
