"""The averager (include/fxcorr.h fxc_average_rows, FxPlan.average_rows), the parts that need no GPU: the declaration, the exported
and bound symbol, the call without a plan, the compiled kernel's resources, and the numpy restatement of the definition
(average_ref.py) -- the reference tests/test_gpu_average.py holds the library to, bit for bit, has to ignore what uncounted
samples hold, commute with a power of two on the weights, reduce to the gain solve's average, handle partial intervals and bins as
defined, and bring the detector-weighted average of the project's damaged samples to the truth-weighted one where the plain
average does not."""
import json
import os
import re

import numpy as np
import pytest

import average_ref
import flag_ref
import gains_ref
import gains_weighted_ref as wref
from effex_amd import _lib
from test_gains_weighted_host import damage_rows
from test_isa_hazards import asm_listing, kernel_resources, needs_hipcc  # noqa: F401  (the module's listing fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fxcorr.h")
BOUNDS = os.path.join(ROOT, "tests", "golden", "average_bounds.json")
CELL_FLOOR = 0.94            # share of the cells to which both the detector's and the truth's weights leave weight


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.complex64 else np.uint32)


def same(got, want):
    """both outputs bit for bit (so +0.0f is not -0.0f, and a NaN equals the same NaN)"""
    return (got[0].dtype == np.complex64 and got[1].dtype == np.float32 and got[0].shape == want[0].shape and got[1].shape == want[1].shape
            and np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1])))


# -- declaration and binding ----------------------------------------------------------------------------------------------------
def test_header_declares_average_rows():
    text = open(HEADER).read()
    assert re.search(r"int fxc_average_rows\(fxc_plan\* plan, const void\* rows, const void\* weights, int64_t n_chunks, int mem_kind, "
                     r"int64_t time_bin,\s+int freq_bin,\s+"
                     r"void\* out_rows\s+/\* \[n_int\]\[n_baselines\]\[n_out\] complex64, in the memory kind of rows \*/,\s+"
                     r"void\* out_weights\s+/\* \[n_int\]\[n_baselines\]\[n_out\] float32, in the memory kind of rows, may be NULL \*/\);",
                     text)
    assert "#define FXC_VERSION 106" in text
    for phrase in ("A sample counts iff w > 0", "Wm > 0 ?", "power of two changes no bit of out_rows", "freq_bin > 256",
                   "the V that fxc_solve_gains averages", "The outputs are written on FXC_OK only"):
        assert phrase in text, phrase


def test_average_rows_is_exported_and_bound():
    handle = _lib.load()
    assert "fxc_average_rows" in _lib.SIGNATURES
    assert handle.fxc_average_rows is not None
    assert handle.fxc_version() == 106


def test_call_without_a_plan_is_an_argument_error():
    handle = _lib.load()
    rows = np.ones((4, 3, 64), dtype=np.complex64)
    vis = np.full((1, 3, 64), -7.0 - 7.0j, dtype=np.complex64)
    wsum = np.full((1, 3, 64), -7.0, dtype=np.float32)
    rc = handle.fxc_average_rows(None, rows.ctypes.data, None, 4, _lib.FXC_MEM_HOST, 0, 1, vis.ctypes.data, wsum.ctypes.data)
    assert rc == _lib.FXC_ERR_ARG
    assert (vis == -7.0 - 7.0j).all() and (wsum == -7.0).all()


@needs_hipcc
def test_average_kernel_compiles_without_scratch(asm_listing):  # noqa: F811
    res = kernel_resources(asm_listing)
    kernel = "rows_average_kernel"
    hits = {name: r for name, r in res.items() if re.search(r"{}{}".format(len(kernel), kernel), name)}
    assert len(hits) == 1, (kernel, sorted(hits))
    vgprs, _, _, scratch, lds = next(iter(hits.values()))
    print(kernel, "VGPRs", vgprs, "scratch", scratch, "LDS", lds)
    assert scratch == 0 and vgprs <= 128, (kernel, vgprs, scratch)
    assert lds == 3 * 768 * 8          # three planes of doubles: 512 bins and a word of padding per output bin of an even freq_bin


def test_averaged_freqs():
    from effex_amd.plan import averaged_freqs
    bw, fc = 2.4e6, 1.4204e9
    freqs = fc + np.fft.fftshift(np.fft.fftfreq(10, 1.0 / bw))
    assert np.array_equal(averaged_freqs(10, bw, fc), freqs) and np.array_equal(averaged_freqs(10, bw, fc, 1), freqs)
    got = averaged_freqs(10, bw, fc, 4)
    assert got.shape == (3,) and got.dtype == np.float64
    assert np.allclose(got, [freqs[0:4].mean(), freqs[4:8].mean(), freqs[8:10].mean()], rtol=1e-15, atol=0)
    assert (np.diff(got) > 0).all()
    assert averaged_freqs(1, bw, fc, 8).tolist() == [fc]
    with pytest.raises(ValueError):
        averaged_freqs(10, bw, fc, 0)


# -- properties of the restatement, each bit for bit ----------------------------------------------------------------------------
def noisy_rows(rng, n_chunks, nb, nchan):
    """a value per (baseline, bin) plus complex noise, complex64"""
    centre = (rng.standard_normal((1, nb, nchan)) + 1j * rng.standard_normal((1, nb, nchan))) * 2.0
    return (centre + 0.3 * (rng.standard_normal((n_chunks, nb, nchan)) + 1j * rng.standard_normal((n_chunks, nb, nchan)))).astype(np.complex64)


def flagged_case(rng, n_chunks, nb, nchan, share=0.2, dead_baseline=None, dead_bin=None):
    """-> rows, weights float32 uniform in 0.25 .. 4, the mask of the flagged samples: `share` of them, a dead baseline and a dead
    bin where asked for; a flagged sample has weight 0, -1 or NaN and its value overwritten with NaN, Inf or 1e30"""
    rows = noisy_rows(rng, n_chunks, nb, nchan)
    weights = rng.uniform(0.25, 4.0, rows.shape).astype(np.float32)
    off = rng.uniform(size=rows.shape) < share
    if dead_baseline is not None:
        off[:, dead_baseline] = True
    if dead_bin is not None:
        off[:, :, dead_bin] = True
    n_off = int(off.sum())
    weights[off] = rng.choice(np.array([0.0, -1.0, np.nan], np.float32), n_off)
    junk = rng.choice(np.array([np.nan, np.inf, 1e30], np.float32), n_off)
    rows.real[off] = junk
    rows.imag[off] = -junk
    return rows, weights, off


def test_uncounted_values_change_nothing():
    rng = np.random.default_rng(9100)
    rows = noisy_rows(rng, 19, 3, 24)
    weights = rng.uniform(0.25, 4.0, rows.shape).astype(np.float32)
    off = rng.uniform(size=rows.shape) < 0.2
    weights[off] = 0
    want = average_ref.average_rows(rows, weights, time_bin=8, freq_bin=3)
    assert np.isfinite(want[0]).all() and (want[1] > 0).all()
    for value in (np.nan, np.inf, 1e30):
        other = rows.copy()
        other[off] = np.complex64(complex(value, -value))
        assert same(average_ref.average_rows(other, weights, time_bin=8, freq_bin=3), want), value
    for value in (-1.0, np.nan, -np.inf):
        other = weights.copy()
        other[off] = value
        assert same(average_ref.average_rows(rows, other, time_bin=8, freq_bin=3), want), value
    # a counted sample's value is used as it is: a NaN under a positive weight, or under no weights at all, propagates
    bad = rows.copy()
    bad[2, 1, 4] = np.complex64(complex(np.nan, 1.0))
    got = average_ref.average_rows(bad, None, time_bin=8, freq_bin=3)
    assert np.isnan(got[0][0, 1, 1].real) and np.isfinite(got[0][0, 1, 1].imag) and np.isfinite(got[0][1:]).all()


def test_weights_times_four():
    rng = np.random.default_rng(9101)
    rows, weights, _ = flagged_case(rng, 21, 3, 30, dead_baseline=1, dead_bin=7)
    for time_bin, freq_bin in ((0, 1), (5, 4), (8, 7)):
        want = average_ref.average_rows(rows, weights, time_bin, freq_bin)
        got = average_ref.average_rows(rows, weights * np.float32(4), time_bin, freq_bin)
        assert np.array_equal(bits(got[0]), bits(want[0]))
        assert np.array_equal(bits(got[1]), bits(want[1] * np.float32(4)))


def test_a_cell_without_a_live_sample_is_plus_zero():
    rng = np.random.default_rng(9102)
    rows, weights, _ = flagged_case(rng, 12, 3, 24, dead_baseline=2, dead_bin=5)
    vis, wsum = average_ref.average_rows(rows, weights, time_bin=5, freq_bin=1)
    assert vis.shape == (3, 3, 24) and wsum.shape == (3, 3, 24)
    for cell in (np.s_[:, 2, :], np.s_[:, :, 5]):
        assert (bits(vis[cell]) == 0).all() and (bits(wsum[cell]) == 0).all()          # +0.0, not -0.0
    assert (wsum[:, :2, :5] > 0).all() and np.isfinite(vis).all()
    # a dead bin inside a wider output bin only takes its share out
    vis4, wsum4 = average_ref.average_rows(rows, weights, time_bin=5, freq_bin=4)
    assert (wsum4[:, :2] > 0).all() and (bits(vis4[:, 2]) == 0).all()


@pytest.mark.parametrize("n_ant", [3, 8])
def test_unit_weights_and_one_bin_are_the_gain_solves_average(n_ant):
    """F = 1 and NULL weights: the complex64 rounding of gains_ref.average's V, interval by interval; weights of ones give the same"""
    rng = np.random.default_rng(9103 + n_ant)
    pr = gains_ref.pairs(n_ant)
    rows = noisy_rows(rng, 13, len(pr) + n_ant, 20)                                      # auto rows behind the cross rows
    for time_bin in (0, 5, 13, 40):
        vis, wsum = average_ref.average_rows(rows, None, time_bin, 1, n_baselines=len(pr))
        spans = gains_ref.intervals(13, time_bin)
        assert vis.shape == (len(spans), len(pr), 20)
        for s, (c0, c1) in enumerate(spans):
            m = gains_ref.average(rows[c0:c1], n_ant)
            v = np.stack([m[:, a, b] for a, b in pr])
            assert np.array_equal(bits(vis[s]), bits(v.astype(np.complex64)))
            assert (wsum[s] == c1 - c0).all()
        ones = np.ones((13, len(pr), 20), np.float32)
        assert same(average_ref.average_rows(rows, ones, time_bin, 1, n_baselines=len(pr)), (vis, wsum))


def test_partial_last_interval_and_bin():
    rng = np.random.default_rng(9104)
    rows, weights, _ = flagged_case(rng, 19, 2, 30, share=0.1)
    vis, wsum = average_ref.average_rows(rows, weights, time_bin=8, freq_bin=4)
    assert vis.shape == (3, 2, 8)                                                        # 8 + 8 + 3 chunks, 7 x 4 + 2 bins
    # the last interval and the last bin, written out: chunks 16 .. 18, bins 28 and 29
    with np.errstate(invalid="ignore"):
        ok = weights > 0
    w64 = np.where(ok, weights, 0).astype(np.float64)
    x64 = np.where(ok, rows.real, 0).astype(np.float64)
    y64 = np.where(ok, rows.imag, 0).astype(np.float64)
    for b in range(2):
        s = np.zeros((3, 2))
        for j in (28, 29):
            for c in (16, 17, 18):
                s[0, j - 28] += w64[c, b, j] * x64[c, b, j]
                s[1, j - 28] += w64[c, b, j] * y64[c, b, j]
                s[2, j - 28] += w64[c, b, j]
        t = (0.0 + s[:, 0]) + s[:, 1]
        assert t[2] > 0
        assert vis[2, b, 7] == np.complex64(complex(np.float32(t[0] / t[2]), np.float32(t[1] / t[2])))
        assert wsum[2, b, 7] == np.float32(t[2])
    # the first seven bins of an interval are those of the band cut to 28 channels, an interval those of its chunks alone
    head = average_ref.average_rows(rows[:, :, :28], weights[:, :, :28], time_bin=8, freq_bin=4)
    assert np.array_equal(bits(vis[:, :, :7]), bits(head[0])) and np.array_equal(bits(wsum[:, :, :7]), bits(head[1]))
    tail = average_ref.average_rows(rows[16:], weights[16:], time_bin=0, freq_bin=4)
    assert same((vis[2:], wsum[2:]), tail)
    # one chunk as 2-D rows, a freq_bin beyond the band, a time_bin beyond the chunks
    one = average_ref.average_rows(rows[3], weights[3], freq_bin=256)
    assert one[0].shape == (1, 2, 1) and same(one, average_ref.average_rows(rows[3:4], weights[3:4], time_bin=99, freq_bin=30))


# -- closure on the project's damaged samples -----------------------------------------------------------------------------------
def closure_figures():
    """per seed of wref.damaged_samples through the oracle, time_bin 0 and freq_bin 1: with the cells = those to which both the
    detector's default weights and the truth's weights leave weight, and every error relative to the largest cell of the
    truth-weighted average -> {seed: (cells, all cells, error of the detector-weighted average on the cells, error of the plain
    average on the cells, the detector's summed weight in the tone's cell)}"""
    out = {}
    tone = gains_ref.pairs(wref.DAMAGE_ANT).index(wref.DAMAGE_TONE_ANTS)
    for seed in wref.DAMAGE_SEEDS:
        rows, _, w_truth = damage_rows(seed)
        out[seed] = closure_of(rows, flag_ref.flag_rows(rows), w_truth, average_ref.average_rows, tone)
    return out


def closure_of(rows, w_det, w_truth, average, tone):
    """the figures of closure_figures for one set of rows, with ``average(rows, weights)`` -> numpy (vis, wsum)"""
    truth, truth_w = average(rows, w_truth)
    det, det_w = average(rows, w_det)
    plain, _ = average(rows, None)
    both = (truth_w[0] > 0) & (det_w[0] > 0)
    scale = float(np.abs(truth[0]).max())
    return (int(both.sum()), int(both.size), float(np.abs(det[0] - truth[0])[both].max()) / scale,
            float(np.abs(plain[0] - truth[0])[both].max()) / scale, float(det_w[0, tone, wref.DAMAGE_TONE_BIN]))


def test_the_detectors_weights_bring_the_average_to_the_truth_weighted_one():
    """Antenna 3 replaced by noise in chunks 8 .. 15 and a tone in bin 20 of antennas 1 and 5, seeds 0 - 3, time_bin 0, freq_bin 1:
    on the cells to which both sets of weights leave weight -- at least 94 % of the 1792 (1688 - 1707 in a run; the truth's weights
    alone leave out 84) -- the detector-weighted average lies within B of the truth-weighted one, the plain average misses by 2 B
    or more (0.23 - 0.32 in a run), and the tone's cell has no weight.  B (tests/golden/average_bounds.json, written by
    tools/average_measure.py) is three times the restatement's largest error over the four seeds (0.0248 in a run: what the
    detector leaves of antenna 3's noise and takes from the clean samples)."""
    rec = json.load(open(BOUNDS))
    assert rec["bound"] == pytest.approx(3.0 * rec["observed"])
    fig = closure_figures()
    for seed, (cells, total, err, plain, tone_w) in sorted(fig.items()):
        print("seed %d: %d of %d cells, detector-weighted %.4g, plain %.4g (B %.4g), tone weight %g" % (seed, cells, total, err, plain,
                                                                                                        rec["bound"], tone_w))
        assert total == 1792 and cells >= CELL_FLOOR * total
        assert err <= rec["bound"]
        assert plain >= 2.0 * rec["bound"]
        assert tone_w == 0
    assert max(v[2] for v in fig.values()) == pytest.approx(rec["observed"], rel=0.05)      # the recorded figure is of this computation
