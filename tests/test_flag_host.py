"""The detector (include/fxcorr.h fxc_flag_rows, FxPlan.flag_rows), the parts that need no GPU: the declaration, the exported and
bound symbol, the call without a plan, the compiled kernels' resources, and the numpy restatement of the definition (flag_ref.py)
-- the reference tests/test_gpu_flag.py holds the library to, bit for bit, has to ignore what non-live samples hold, commute with
chunk permutations and powers of two, pass a prior through, find the damage of gains_weighted_ref.damaged_samples without being
told where it is, and leave clean samples mostly alone."""
import json
import os
import re

import numpy as np
import pytest

import flag_ref
import gains_ref
import gains_weighted_ref as wref
from effex_amd import _lib
from test_gains_weighted_host import damage_rows
from test_gains_host import oracle_rows
from test_isa_hazards import asm_listing, kernel_resources, needs_hipcc  # noqa: F401  (the module's listing fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fxcorr.h")
BOUNDS = os.path.join(ROOT, "tests", "golden", "flag_bounds.json")
WEIGHTED_BOUNDS = os.path.join(ROOT, "tests", "golden", "gains_weighted_bounds.json")
CLEAN_SEEDS = (0, 1, 2, 3)
CLEAN_CAP = 0.05
DETECTION_FLOOR = 0.95


# -- declaration and binding ----------------------------------------------------------------------------------------------------
def test_header_declares_flag_rows():
    text = open(HEADER).read()
    assert re.search(r"int fxc_flag_rows\(fxc_plan\* plan, const void\* rows, const void\* prior, int64_t n_chunks, int mem_kind, "
                     r"int64_t window,\s+float time_threshold, float freq_threshold, int half_width, int iters,\s+"
                     r"void\* weights\s+/\* \[n_chunks\]\[n_baselines\]\[nchan\] float32, in the memory kind of rows \*/,\s+"
                     r"int64_t\* counts\s+/\* \[n_win\]\[n_baselines\]\[3\], host, may be NULL \*/\);", text)
    assert "Lower median" in text and "more than 1024 chunks in a window" in text


def test_flag_rows_is_exported_and_bound():
    handle = _lib.load()
    assert "fxc_flag_rows" in _lib.SIGNATURES
    assert handle.fxc_flag_rows is not None


def test_call_without_a_plan_is_an_argument_error():
    handle = _lib.load()
    rows = np.ones((4, 3, 64), dtype=np.complex64)
    weights = np.full((4, 3, 64), -7.0, dtype=np.float32)
    counts = np.full((1, 3, 3), -7, dtype=np.int64)
    rc = handle.fxc_flag_rows(None, rows.ctypes.data, None, 4, _lib.FXC_MEM_HOST, 0, 20.0, 8.0, 8, 2, weights.ctypes.data,
                              counts.ctypes.data)
    assert rc == _lib.FXC_ERR_ARG
    assert (weights == -7.0).all() and (counts == -7).all()


@needs_hipcc
def test_flag_kernels_compile_without_scratch(asm_listing):  # noqa: F811
    res = kernel_resources(asm_listing)
    for kernel in ("flag_time_kernel", "flag_freq_kernel"):
        hits = {name: r for name, r in res.items() if re.search(r"{}{}".format(len(kernel), kernel), name)}
        assert len(hits) == 1, (kernel, sorted(hits))
        vgprs, _, _, scratch, _ = next(iter(hits.values()))
        print(kernel, "VGPRs", vgprs, "scratch", scratch)
        assert scratch == 0 and vgprs <= 128, (kernel, vgprs, scratch)


# -- invariances of the restatement, each bit for bit -----------------------------------------------------------------------------
def noisy_rows(rng, n_chunks, nb, nchan, outliers=0.15):
    """a constant per (baseline, bin) plus complex noise, `outliers` of the samples far off, a loud bin and a noisy bin"""
    centre = (rng.standard_normal((1, nb, nchan)) + 1j * rng.standard_normal((1, nb, nchan))) * 2.0
    rows = centre + 0.1 * (rng.standard_normal((n_chunks, nb, nchan)) + 1j * rng.standard_normal((n_chunks, nb, nchan)))
    bad = rng.uniform(size=rows.shape) < outliers
    rows[bad] += 3.0 * (rng.standard_normal(int(bad.sum())) + 1j * rng.standard_normal(int(bad.sum())))
    if nchan > 12:
        rows[:, :, 5] *= 40.0                                                    # a tone: the level test
        rows[:, :, 11] += 2.0 * (rng.standard_normal((n_chunks, nb)) + 1j * rng.standard_normal((n_chunks, nb)))  # scatter
    return rows.astype(np.complex64)


def with_dead(rng, rows, share=0.1):
    """rows with `share` of the samples, one column and one bin exactly zero (dropped); -> rows, the mask of those samples"""
    rows = rows.copy()
    dead = rng.uniform(size=rows.shape) < share
    dead[:, 0, 3] = True
    dead[:, :, 7] = True
    rows[dead] = 0
    return rows, dead


def test_non_live_values_change_nothing():
    rng = np.random.default_rng(9000)
    rows, dead = with_dead(rng, noisy_rows(rng, 19, 3, 24))
    prior = rng.uniform(0.5, 2.0, rows.shape).astype(np.float32)
    off = rng.uniform(size=rows.shape) < 0.1
    prior[off] = 0
    want = flag_ref.flag_rows(rows, window=8, prior=prior, return_counts=True)
    assert (want[0][dead | off] == 0).all() and (want[0] > 0).any() and want[1][:, :, 1].sum() > 0 and want[1][:, :, 2].sum() > 0
    for value in (np.nan, np.inf, 1e30):
        other = rows.copy()
        other[off] = np.complex64(complex(value, -value))                 # flagged by the prior: the value is never used
        got = flag_ref.flag_rows(other, window=8, prior=prior, return_counts=True)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), value
    for value in (np.nan, np.inf):
        other = rows.copy()
        other[dead] = np.complex64(complex(value, 1.0))                   # not finite instead of zero: as dead as before
        got = flag_ref.flag_rows(other, window=8, prior=prior, return_counts=True)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), value
    for value in (-1.0, np.nan):
        other = prior.copy()
        other[off] = value
        got = flag_ref.flag_rows(rows, window=8, prior=other, return_counts=True)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), value


def test_a_power_of_two_changes_nothing():
    rng = np.random.default_rng(9001)
    rows, _ = with_dead(rng, noisy_rows(rng, 16, 3, 24))
    want = flag_ref.flag_rows(rows, return_counts=True)
    got = flag_ref.flag_rows(rows * np.float32(2.0 ** -7), return_counts=True)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert 0 < (want[0] == 0).mean() < 0.6


def test_a_chunk_permutation_permutes_the_weights():
    rng = np.random.default_rng(9002)
    rows, _ = with_dead(rng, noisy_rows(rng, 12, 3, 24))
    want = flag_ref.flag_rows(rows, window=6, return_counts=True)
    perm = np.concatenate([rng.permutation(6), 6 + rng.permutation(6)])      # within each window
    got = flag_ref.flag_rows(rows[perm], window=6, return_counts=True)
    assert np.array_equal(got[0], want[0][perm]) and np.array_equal(got[1], want[1])
    assert not np.array_equal(want[0], want[0][perm])


def test_a_prior_passes_through():
    rng = np.random.default_rng(9003)
    rows, _ = with_dead(rng, noisy_rows(rng, 16, 3, 24))
    want = flag_ref.flag_rows(rows, return_counts=True)
    ones = flag_ref.flag_rows(rows, prior=np.ones(rows.shape, np.float32), return_counts=True)
    assert np.array_equal(ones[0], want[0]) and np.array_equal(ones[1], want[1])
    prior = rng.uniform(0.25, 4.0, rows.shape).astype(np.float32)
    got = flag_ref.flag_rows(rows, prior=prior, return_counts=True)
    assert np.array_equal(got[0], np.where(want[0] > 0, prior, np.float32(0))) and np.array_equal(got[1], want[1])
    assert not np.signbit(got[0][got[0] == 0]).any()                     # +0.0f


def test_one_channel_and_one_chunk():
    rng = np.random.default_rng(9004)
    rows = noisy_rows(rng, 40, 1, 1)
    w, counts = flag_ref.flag_rows(rows, return_counts=True)
    assert counts[0, 0, 2] == 0 and counts[0, 0, 1] > 0                   # the frequency stage never fires at nchan 1
    w1 = flag_ref.flag_rows(rows[0])                                       # 2-D rows: one chunk, its own median, d == 0
    assert w1.shape == (1, 1) and (w1 == 1).all()


# -- detection on the project's damaged samples -------------------------------------------------------------------------------------
def detection_figures():
    """the detector's weights (defaults) on wref.damaged_samples through the oracle: per seed the share of antenna 3's baselines'
    samples in chunks 8 .. 15 that are flagged and whether every sample of baseline (1, 5) in bin 20 is; per (seed, ref) the
    error of the ratios solved with those weights and of the unweighted restatement"""
    pr = gains_ref.pairs(wref.DAMAGE_ANT)
    bad = [i for i, (a, b) in enumerate(pr) if wref.DAMAGE_BAD_ANT in (a, b)]
    tone = pr.index(wref.DAMAGE_TONE_ANTS)
    c0, c1 = wref.DAMAGE_BAD_CHUNKS
    out = {"caught": {}, "tone": {}, "errors": {}}
    for seed in wref.DAMAGE_SEEDS:
        rows, c, _ = damage_rows(seed)
        w = flag_ref.flag_rows(rows)
        out["caught"][seed] = float((w[c0:c1, bad] == 0).mean())
        out["tone"][seed] = bool((w[:, tone, wref.DAMAGE_TONE_BIN] == 0).all())
        for ref in wref.DAMAGE_REFS:
            truth = gains_ref.true_ratios(c, ref)
            g, _ = wref.solve_rows(rows, wref.DAMAGE_ANT, ref=ref, iters=gains_ref.SAMPLE_ITERS, weights=w)
            plain, _ = gains_ref.solve_rows(rows, wref.DAMAGE_ANT, ref=ref, iters=gains_ref.SAMPLE_ITERS)
            out["errors"][(seed, ref)] = (float(np.abs(wref.scalar_ratios(g[0], ref) - truth).max()),
                                          float(np.abs(wref.scalar_ratios(plain[0], ref) - truth).max()))
    return out


def clean_shares():
    """{seed: share of the samples of the undamaged gains_ref.samples(8, seed) that the detector flags}"""
    return {seed: float((flag_ref.flag_rows(oracle_rows(gains_ref.samples(wref.DAMAGE_ANT, seed)[0], gains_ref.SAMPLE_NCHAN)) == 0).mean())
            for seed in CLEAN_SEEDS}


def test_the_detector_finds_the_damage_and_the_solve_closes():
    """Antenna 3 replaced by noise in chunks 8 .. 15, a tone in bin 20 of antennas 1 and 5, the detector's weights alone (defaults):
    at least 95 % of antenna 3's baselines' samples in those chunks are flagged, every sample of baseline (1, 5) in bin 20 is, the
    weighted restatement returns the ratios within the project's own bound (tests/golden/gains_weighted_bounds.json) and the
    unweighted one stays above ten times it.  The figures recorded in tests/golden/flag_bounds.json (tools/flag_measure.py) are of
    this computation."""
    rec = json.load(open(BOUNDS))
    bound = json.load(open(WEIGHTED_BOUNDS))["bound"]
    fig = detection_figures()
    for seed in wref.DAMAGE_SEEDS:
        print("seed %d: caught %.4f, tone %s" % (seed, fig["caught"][seed], fig["tone"][seed]))
        assert fig["caught"][seed] >= DETECTION_FLOOR
        assert fig["tone"][seed]
    for key, (err, plain) in sorted(fig["errors"].items()):
        print("seed %d ref %d: detector's weights %.3g, unweighted %.3g (B %.3g)" % (key + (err, plain, bound)))
    worst = max(err for err, _ in fig["errors"].values())
    assert worst <= bound
    assert min(plain for _, plain in fig["errors"].values()) > 10.0 * bound
    assert worst == pytest.approx(rec["closure_worst"], rel=0.05)
    assert min(fig["caught"].values()) == pytest.approx(rec["caught_smallest"], rel=1e-3)


def test_clean_samples_are_mostly_left_alone():
    """on the undamaged samples at most 5 % are flagged (a cap; the restatement gives 1.2 - 2.2 %)"""
    rec = json.load(open(BOUNDS))
    shares = clean_shares()
    for seed, share in sorted(shares.items()):
        print("seed %d: %.4f flagged" % (seed, share))
        assert share <= CLEAN_CAP
        assert share == pytest.approx(rec["clean_share"][str(seed)], rel=0.02)
