"""Chunks of more than 1024 frames under every row modifier.

A chunk of more than ``kRowSpectra`` = 1024 spectra (h_launch.h) is no single float32 raw row.  With 3 and more antennas, and on
every plan with autos, the X-engines cut it into frame ranges (k_finish.h::x_range), write one raw row per range, range-major
(``row = range * n_groups + group``), and the rows kernels and the tracked fold read the ranges as their splits.  ``CASES`` has one
line per (route, modifier) that meets such a chunk; ``test_gpu_long_chunks.py`` runs them on the device against the float64
oracle below and ``test_long_chunks_host.py`` shows, in the oracle alone, that every wrong reading of those index rules moves a
result by ten ceilings or more.  A new route or a new row modifier adds a line to ``CASES``.

Sizes: ``n_chunks`` >= 3 (with one chunk range-major and group-major rows coincide); ``n_pts`` = 1027 is two ranges of 514 and
513 frames -- the second one odd, starting at frame 514 -- and 2051 three of 684, 684 and 683; ``ntaps`` = 4,
``num_samp = nchan * n_pts``.  The X-engine route off the powers of two (``mixed_xeng``) takes its ranges from x_geometry: runs
of 64 frames, 17 ranges of 61 and 51 frames at 1027.

Modifiers: ``rot`` one shared table (set_rot); ``ant`` per-antenna tables (set_delays); ``track`` a delay track from chunk
``T0`` on whose rates turn every baseline by a tenth of a turn or more per chunk; ``gains`` the track with two gain solutions
of two chunks each, so that the call's chunks take both.

Input (``samples``): per antenna standard-normal noise at a level of its own plus a common component, no tone -- the suite's
metric divides by the largest value of a group of rows and one loud bin would hide the others.  The sample blocks on both sides
of every range boundary and the chunk's first and last blocks are three times as loud, so that a frame lost or counted twice there
is large.  The window is ``window_cases.rough_window``: a chunk's first frame has no history and meets data through the window's last
taps alone, which the designed window makes its smallest -- with independent taps that frame has a quarter of a later frame's power
and counts, and every bin still has the same expected power (white input: the sum of the squared taps).

Oracle: per chunk the spectra of ``fx_oracle.spectrometer_poly`` (``gain_track_ref.spectra``), summed range by range
(``range_sums``), and the chunk's tables -- ``fx_oracle.rot_table``, times ``gain_track_ref.inverse`` of the chunk's solution
under gains -- put on the sums (``rows_from``).  The sum over the ranges is the mean over the chunk's frames:
``test_long_chunks_host.py`` holds ``oracle`` to ``gain_track_ref.oracle`` (the oracle of test_gpu_tracking.py) for every case;
the range sums are kept apart because the wrong readings are statements about ranges.
"""
import collections
import functools
import json

import numpy as np

import window_cases as wc

Case = collections.namedtuple("Case", "id n_ant nchan n_pts n_chunks route autos mod expect env")

NTAPS = 4
BW = 2.4e6
FREQ = 1.42e9
K_ROW_SPECTRA = 1024        # h_launch.h::kRowSpectra
TAU_ROT = 7.3e-7            # the shared table's delay
T0 = 9                      # first chunk of the tracked calls
G_INTERVAL, G_FIRST = 2, 9  # two solutions: chunks 9, 10 take solution 0, 11 and later solution 1
LOUD = 3.0                  # the factor of the sample blocks at the range boundaries
SOURCE = 0.5                # the common component's amplitude

MODS = ("rot", "ant", "track", "gains")


def _case(n_ant, nchan, n_pts, mod, autos, route, expect, n_chunks=3, env=None, tag=""):
    assert mod in MODS
    name = "%s-%dx%dx%d-%s%s%s" % (route, n_ant, nchan, n_pts, mod, "+autos" if autos else "", tag)
    return Case(name, n_ant, nchan, n_pts, n_chunks, route, autos, mod, expect, dict(env or {}))


def _wave3(n_pts):
    sh = (3, 64, n_pts)
    return [_case(*sh, mod, autos, "wave", wc._small(64)) for mod, autos in
            (("ant", False), ("track", False), ("gains", False), ("rot", True), ("ant", True), ("track", True), ("gains", True))]


_PASSES = {"FXC_WS_MB": "1"}
# the generic path at 1000 channels, 3 antennas: the F stage built for the channel count (2) and none that takes F and X in one pass (1)
_MIXED_XENG = {"path": "generic", "block": 256, "lds_bytes": 1000 * 8, "specialised": 2}

# what plan.path / plan.info show of a route (window_cases.py): the wave-local kernels' plans (16 ... 256 channels, the X-engine
# by the antenna count: xengine_kernel<3 ... 8>, the matrix cores from 9 on, one tile per 16 antennas), the tiled ring kernel's,
# the fused kernel's, the generic path's.  The workspace a fresh plan's first fx_rows takes shows the ranges (``passes``).
CASES = _wave3(1027) + _wave3(2051) + [
    # two antennas with autos: xengine_kernel<2, true>
    _case(2, 64, 1027, "rot", True, "wave", wc._small(64)),
    _case(2, 64, 1027, "track", True, "wave", wc._small(64)),
    # part of a wave
    _case(3, 16, 1027, "track", True, "wave", wc._small(16)),
    # xengine_kernel<8>, two columns of 64 channels
    _case(8, 128, 1027, "ant", True, "wave", wc._small(128)),
    _case(8, 128, 1027, "track", False, "wave", wc._small(128)),
    # the tiled F-only kernel + X-engine, raw layout 0
    _case(3, 512, 1027, "ant", False, "tiled", wc._tiled(512)),
    _case(3, 512, 1027, "track", True, "tiled", wc._tiled(512)),
    # the fused F-only kernel + xengine_kernel, raw layout 2 (specpos_of_bin) under the split stride; with autos the plan's F stage
    _case(4, 4096, 1027, "ant", False, "fused", wc._fused()),
    _case(4, 4096, 1027, "track", True, "fused", wc._fused()),
    # the X-engine route off the powers of two: 17 ranges
    _case(3, 1000, 1027, "track", False, "mixed_xeng", _MIXED_XENG),
    _case(3, 1000, 1027, "gains", False, "mixed_xeng", _MIXED_XENG),
    # the matrix-core X-engine, 1 ... 4 tiles of 16 antennas
    _case(9, 64, 1027, "ant", False, "mfma1", wc._small(64)),
    _case(9, 64, 1027, "track", False, "mfma1", wc._small(64)),
    _case(17, 64, 1027, "ant", False, "mfma2", wc._small(64)),
    _case(33, 64, 1027, "track", False, "mfma3", wc._small(64)),
    _case(49, 64, 1027, "ant", False, "mfma4", wc._small(64)),
    # several workspace passes of range-major rows, the last one shorter (a child process with a workspace target of 1 MiB)
    _case(3, 16, 1027, "track", True, "wave", wc._small(16), n_chunks=5, env=_PASSES, tag="-passes"),
    _case(3, 16, 1027, "ant", True, "wave", wc._small(16), n_chunks=5, env=_PASSES, tag="-passes"),
]
BY_ID = {c.id: c for c in CASES}


def num_samp(case):
    return case.nchan * case.n_pts


def pairs(n_ant):
    return [(a, b) for a in range(n_ant) for b in range(a + 1, n_ant)]


def window(case):
    return wc.rough_window(NTAPS, case.nchan)


# ---- the ranges: k_finish.h::x_range and the launchers' range counts, restated ---------------------------------------------------
def n_ranges(case):
    """frame ranges of a chunk in a call for rows: h_launch.h::frame_ranges, or -- the X-engine route off the powers of two
    without autos -- x_geometry's splits (runs of 256 / kx * 64 frames, 256 at the most)"""
    if case.route == "mixed_xeng" and not case.autos:
        kx = 1
        while kx < 256 and kx < case.nchan:
            kx <<= 1
        run = 256 // kx * 64
        return min(max(-(-case.n_pts // run), 1), 256)
    return min(-(-case.n_pts // K_ROW_SPECTRA), 4096)


def x_range(n_pts, n, rg):
    """(i0, i1) of range rg of n: x_range's arithmetic"""
    per = (n_pts + n - 1) // n
    i0 = rg * per if rg * per < n_pts else n_pts
    i1 = i0 + per if i0 + per < n_pts else n_pts
    return i0, i1


def ranges(case):
    n = n_ranges(case)
    return [x_range(case.n_pts, n, rg) for rg in range(n)]


def passes(case, workspace=12 << 30):
    """(chunks per pass, bytes of a pass's spectra, bytes of its raw rows) of a call for rows under a workspace target (the
    library's own: 12 GiB): the sizing of h_run.h::autos_pass, h_launch.h::fused_chunks_per_pass and generic_chunks_per_pass, which agree for three
    and more antennas and for plans with autos -- every antenna's spectra, and one raw row per product and frame range"""
    n_prod = len(pairs(case.n_ant)) + (case.n_ant if case.autos else 0)
    spec = case.n_ant * case.n_pts * case.nchan * 8
    raw = n_prod * case.nchan * 8 * n_ranges(case)
    cb = max(1, min(workspace // (spec + raw), case.n_chunks))
    return cb, cb * spec, cb * raw


# ---- input -------------------------------------------------------------------------------------------------------------------
def loud_blocks(case):
    """the sample blocks (frames' worth of samples) made LOUD: both sides of every range boundary, the chunk's first and last"""
    out = {0, case.n_pts - 1}
    for i0, _ in ranges(case)[1:]:
        out |= {i0 - 1, i0}
    return sorted(out)


def noise_level(n_ant):
    """antenna a's noise amplitude: 1 ... 1.5, every antenna its own (the auto rows differ by more than their noise)"""
    return 1.0 + 0.5 * np.arange(n_ant) / max(n_ant - 1, 1)


@functools.lru_cache(maxsize=2)
def _samples(n_ant, nchan, n_pts, n_chunks, loud):
    n = nchan * n_pts
    x = np.empty((n_chunks, n_ant, n), np.complex64)
    level = noise_level(n_ant)[:, None].astype(np.float32)
    def draw(rng, rows):             # unit-variance complex noise, drawn as float32: the samples are complex64
        v = rng.standard_normal((rows, n, 2), dtype=np.float32) * np.float32(np.sqrt(0.5))
        return v.view(np.complex64)[..., 0]

    for c in range(n_chunks):        # (chunk by chunk; beam_ref.noise_and_source's pattern)
        rng = np.random.default_rng([1000 * n_ant + nchan, n_pts, c])
        v = (level * draw(rng, n_ant) + np.float32(SOURCE) * draw(rng, 1)).reshape(n_ant, n_pts, nchan)
        v[:, list(loud)] *= np.float32(LOUD)
        x[c] = v.reshape(n_ant, n)
    x.setflags(write=False)
    return x


def samples(case):
    """x [n_chunks, n_ant, num_samp] complex64, seeded by the shape (read-only: shared by the cases of a shape)"""
    return _samples(case.n_ant, case.nchan, case.n_pts, case.n_chunks, tuple(loud_blocks(case)))


# ---- tables ------------------------------------------------------------------------------------------------------------------
def track_of(n_ant):
    """delays up to 2.3e-6 s (5.5 turns over the band) and rates in steps of 1 / (2 n_ant) turns per chunk at the centre frequency
    from antenna to antenna, antenna 0 included: baseline (a, b) turns by (b - a) / (2 n_ant) of a turn from chunk to chunk, less
    than half a turn and no baseline's table stands still"""
    a = np.arange(n_ant)
    tau0 = 2e-6 * ((3 * a * a) % 17 + 0.25 * a) / 17.0 - 3e-7
    rate = (a - (n_ant - 1) / 2.0) / (2.0 * n_ant * FREQ)
    return tau0, rate


def gains_of(case):
    """[2, n_ant, nchan] complex128, the rows' fftshifted order: gains_ref.draw_gains twice"""
    import gains_ref
    rng = np.random.default_rng(77 + 1000 * case.n_ant + case.nchan)
    return np.stack([gains_ref.draw_gains(case.n_ant, case.nchan, rng) for _ in range(2)])


def solution(case, c, flip=False):
    import gain_track_ref
    s = gain_track_ref.solution_index(T0 + c, 2, G_INTERVAL, G_FIRST)
    return 1 - s if flip else s


def tables(case, shift=0, flip=False):
    """rho [n_chunks, n_ant, nchan] complex128, natural bin order: the tables of the modifier's chunks (``rot``: None).
    shift: chunk t + shift's delays in place of chunk t's; flip: the other solution's gains"""
    import fx_oracle
    import gain_track_ref
    if case.mod == "rot":
        return None
    tau0, rate = track_of(case.n_ant)
    if case.mod == "ant":
        rate = 0.0 * rate
    out = np.empty((case.n_chunks, case.n_ant, case.nchan), np.complex128)
    g = gains_of(case) if case.mod == "gains" else None
    for c in range(case.n_chunks):
        tau = tau0 + (T0 + c + shift) * rate
        out[c] = [fx_oracle.rot_table(case.nchan, BW, FREQ, d) for d in tau]
        if g is not None:
            out[c] *= gain_track_ref.inverse(g[solution(case, c, flip)])
    return out


def factors(case, rho=None):
    """[n_chunks, n_baselines, nchan]: what the cross sums of chunk c, baseline (a, b) are multiplied by -- rho_a conj(rho_b), or
    conj(rot) of the shared table"""
    import fx_oracle
    pr = pairs(case.n_ant)
    if case.mod == "rot":
        rot = fx_oracle.rot_table(case.nchan, BW, FREQ, TAU_ROT)
        return np.broadcast_to(np.conj(rot), (case.n_chunks, len(pr), case.nchan)).copy()
    rho = tables(case) if rho is None else rho
    ia, ib = [a for a, _ in pr], [b for _, b in pr]
    return rho[:, ia] * np.conj(rho[:, ib])


def apply_modifier(plan, case):
    """the modifier on an FxPlan"""
    tau0, rate = track_of(case.n_ant)
    if case.mod == "rot":
        plan.set_delay(BW, FREQ, TAU_ROT)
    elif case.mod == "ant":
        plan.set_delays(tau0, BW, FREQ)
    else:
        plan.set_delay_track(tau0, rate, BW, FREQ, first_chunk=T0)
        if case.mod == "gains":
            plan.set_track_gains(gains_of(case), interval=G_INTERVAL, first_chunk=G_FIRST)


def tracked(case):
    return case.mod in ("track", "gains")


# ---- the oracle --------------------------------------------------------------------------------------------------------------
Sums = collections.namedtuple("Sums", "cross autos first_cross first_autos last_cross last_autos")


def _products(f):
    """f [n_ant, n, nchan] -> sum over the n frames of f_a conj(f_b) [n_baselines, nchan] and of |f_a|^2 [n_ant, nchan]"""
    g = np.ascontiguousarray(f.transpose(2, 0, 1))                    # [nchan, n_ant, n]
    v = np.matmul(g, np.conj(g).transpose(0, 2, 1))                   # [nchan, a, b]
    pr = pairs(f.shape[0])
    cross = v[:, [a for a, _ in pr], [b for _, b in pr]].T
    autos = (np.abs(f) ** 2).sum(axis=1)
    return cross, autos


def _range_sums(case, x):
    import gain_track_ref
    rg = ranges(case)
    nb = len(pairs(case.n_ant))
    shape_c, shape_a = (case.n_chunks, len(rg), nb, case.nchan), (case.n_chunks, len(rg), case.n_ant, case.nchan)
    s = Sums(*(np.zeros(shape, np.complex128 if i % 2 == 0 else np.float64) for i, shape in enumerate((shape_c, shape_a) * 3)))
    win = window(case)
    for c in range(case.n_chunks):
        f = np.stack(gain_track_ref.spectra(x[c:c + 1], case.nchan, win)[0])       # [n_ant, n_pts, nchan]
        assert f.shape == (case.n_ant, case.n_pts, case.nchan)
        for r, (i0, i1) in enumerate(rg):
            s.cross[c, r], s.autos[c, r] = _products(f[:, i0:i1])
            s.first_cross[c, r], s.first_autos[c, r] = _products(f[:, i0:i0 + 1])
            s.last_cross[c, r], s.last_autos[c, r] = _products(f[:, i1 - 1:i1])
    for a in s:
        a.setflags(write=False)
    return s


_kept = collections.OrderedDict()      # the range sums of the last two shapes: the cases of a shape stand side by side in CASES


def range_sums(case, x=None):
    """Sums over the frames of every range, natural bin order, no table and no division: cross [n_chunks, n_ranges, n_baselines,
    nchan] of f_a conj(f_b), autos [.., n_ant, nchan] of |f_a|^2, and the same products of each range's first and last frame
    alone.  x None: the case's samples (kept per shape: the cases of a shape differ in their tables only)"""
    if x is not None:
        return _range_sums(case, x)
    key = (case.n_ant, case.nchan, case.n_pts, case.n_chunks, n_ranges(case))
    if key not in _kept:
        while len(_kept) >= 2:
            _kept.popitem(last=False)
        _kept[key] = _range_sums(case, samples(case))
    return _kept[key]


def rows_from(case, cross, autos, fac, auto_fac=None):
    """cross [n_chunks, n_ranges', n_baselines, nchan], autos [.., n_ant, nchan] -> rows [n_chunks, n_rows, nchan] complex128:
    fftshift((sum over the ranges) / n_pts * fac), the auto rows -- plans with autos -- after the cross rows, times auto_fac
    where one is given (no correct reading does)"""
    rows = cross.sum(axis=1) / case.n_pts * fac
    if case.autos:
        au = autos.sum(axis=1) / case.n_pts + 0j
        rows = np.concatenate([rows, au if auto_fac is None else au * auto_fac], axis=1)
    return np.fft.fftshift(rows, axes=-1)


def oracle(case, x=None):
    """rows [n_chunks, n_rows, nchan] complex128: cross rows fftshift(mean_i f_a rho_a conj(f_b rho_b)) of every chunk with its
    own tables, then -- plans with autos -- the auto rows fftshift(mean_i |f_a|^2)"""
    s = range_sums(case, x)
    return rows_from(case, s.cross, s.autos, factors(case))


def restated_elsewhere(case, x):
    """The same rows from gain_track_ref.oracle -- the oracle of test_gpu_tracking.py, with gains where the case has them -- for
    the per-antenna modifiers, and from test_gpu_autos.py's statement (the shared table on the cross rows only) for ``rot``"""
    import fx_oracle
    import gain_track_ref
    tau0, rate = track_of(case.n_ant)
    kw = {}
    if case.mod == "gains":
        kw = dict(gains=gains_of(case), interval=G_INTERVAL, first_chunk=G_FIRST)
    if case.mod in ("rot", "ant"):
        tau0, rate = (0.0 * tau0 if case.mod == "rot" else tau0), 0.0 * rate
    rows = gain_track_ref.oracle(x, case.nchan, window(case), tau0, rate, T0, BW, FREQ, autos=case.autos, **kw)
    if case.mod == "rot":
        nb = len(pairs(case.n_ant))
        rows[:, :nb] *= np.fft.fftshift(np.conj(fx_oracle.rot_table(case.nchan, BW, FREQ, TAU_ROT)))
    return rows


# ---- the wrong readings ------------------------------------------------------------------------------------------------------
def wrong_readings(case, s=None):
    """(name, groups it must move, rows) for every way of misreading the ranges, the chunk's tables or the auto rows that the case
    can show: groups is a subset of ("cross", "autos")"""
    s = range_sums(case) if s is None else s
    fac = factors(case)
    both = ("cross", "autos") if case.autos else ("cross",)
    n_r, n_c = s.cross.shape[1], case.n_chunks

    def rows(cross=s.cross, autos=s.autos, f=fac, af=None):
        return rows_from(case, cross, autos, f, af)

    for r in range(n_r):
        pick = np.zeros((1, n_r, 1, 1))
        pick[0, r] = 1.0
        yield "last frame of range %d dropped" % r, both, rows(s.cross - pick * s.last_cross, s.autos - pick * s.last_autos)
        yield "first frame of range %d counted twice" % r, both, rows(s.cross + pick * s.first_cross, s.autos + pick * s.first_autos)
    yield "last range left out", both, rows(s.cross[:, :-1], s.autos[:, :-1])
    # the device writes raw row range * n_chunks + chunk; read group-major, split s of chunk c is raw row c * n_ranges + s
    at = np.arange(n_c)[:, None] * n_r + np.arange(n_r)[None, :]
    rg, grp = at // n_c, at % n_c
    yield "group-major rows", both, rows(s.cross[grp, rg], s.autos[grp, rg])
    if tracked(case):
        for shift in (-1, 1):
            yield "tables of chunk t %+d" % shift, ("cross",), rows(f=factors(case, tables(case, shift=shift)))
    if case.mod == "gains":
        yield "the neighbouring solution's gains", ("cross",), rows(f=factors(case, tables(case, flip=True)))
    if case.mod == "ant":
        for shift in (-1, 1):
            yield "tables of baseline p %+d" % shift, ("cross",), rows(f=np.roll(fac, shift, axis=1))
    if case.autos:
        # (the shared table, or a baseline's: row n_baselines + a read as a cross row)
        af = fac[:, [0] * case.n_ant] if case.mod == "rot" else fac[:, [min(a, len(pairs(case.n_ant)) - 1) for a in range(case.n_ant)]]
        yield "auto rows given a rot", ("autos",), rows(af=af)
        for shift in (-1, 1):
            yield "auto row of antenna a %+d" % shift, ("autos",), rows(autos=np.roll(s.autos, shift, axis=2))


# ---- comparisons -------------------------------------------------------------------------------------------------------------
def rel_err(a, b):
    """The suite's metric: max|a - b| / max|b|."""
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


def groups(case):
    nb = len(pairs(case.n_ant))
    return [("cross", slice(0, nb))] + ([("autos", slice(nb, None))] if case.autos else [])


def continuum(rows):
    """CONTINUUM values of SPECTRUM rows: the mean over the bins / bandwidth"""
    return np.asarray(rows).mean(axis=-1) / BW


def row_checks(case, got, ref):
    """(group, "SPECTRUM" | "CONTINUUM", error) of rows [n_chunks, n_rows, nchan] against the oracle's, CONTINUUM from the rows"""
    out = []
    for name, g in groups(case):
        out.append((name, "SPECTRUM", rel_err(got[:, g], ref[:, g])))
        out.append((name, "CONTINUUM", rel_err(continuum(got[:, g]), continuum(ref[:, g]))))
    return out


# ---- the device side, in the test's process or in a child ----------------------------------------------------------------------
def host(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


def exported(plan):
    sums = plan.new_sums()
    plan.acc_export(sums)
    plan.acc_reset()
    return host(sums).copy()


def device_outputs(plan_mod, xd, case):
    """Every output the device test compares, as numpy arrays: fx_rows SPECTRUM / CONTINUUM, fx_accumulate + finalize SPECTRUM /
    CONTINUUM; "track": the plan's chunk counter after each of the three calls (tracked cases); "info": workspace bytes and CUs after
    the first call; "route": what plan.path and plan.info show"""
    out = {}
    counters = []
    with plan_mod.FxPlan(case.n_ant, case.nchan, NTAPS, num_samp(case), window=window(case), autos=case.autos) as p:
        apply_modifier(p, case)

        def rewind():
            if tracked(case):
                counters.append(p.track_chunk)
                p.track_seek(T0)

        out["rows"] = host(p.fx_rows(xd, "SPECTRUM"))
        info = p.info
        out["info"] = np.array([info["workspace_bytes"], info["cu_count"]])
        out["route"] = np.array([json.dumps(dict(info, path=p.path))])
        rewind()
        out["rows_c"] = host(p.fx_rows(xd, "CONTINUUM", BW))
        rewind()
        p.fx_accumulate(xd)
        rewind()
        out["integ"] = host(p.finalize("SPECTRUM", reset=False))
        out["integ_c"] = host(p.finalize("CONTINUUM", BW))
    out["track"] = np.array(counters, np.int64)
    return out
