"""Weighted fringe fit (include/fxcorr.h fxc_fringe_fit_weighted), the parts that need no GPU: the declaration, the exported and
bound symbol, the call without a plan, the compiled gather of k_fringe.h, and the float64 restatement of the definition
(fringe_weighted_ref.py) -- the reference tests/test_gpu_fringe_weighted.py holds the library to has to ignore what is flagged,
unwrap the baselines and find the injected delays and rates itself."""
import os
import re

import numpy as np
import pytest

import fringe_ref
import fringe_weighted_ref as fw
from effex_amd import _lib
from fringe_ref import BW, FC
from test_isa_hazards import asm_listing, kernel_resources, needs_hipcc  # noqa: F401  (the module's listing fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fxcorr.h")


def test_header_declares_the_weighted_fit():
    text = open(HEADER).read()
    assert re.search(r"int fxc_fringe_fit_weighted\(fxc_plan\* plan, const void\* rows, const void\* weights, int64_t n_chunks, "
                     r"int mem_kind,\s+double bandwidth, double frequency, int ref, int pad, int baselines, double min_snr,\s+"
                     r"double\* delay_s, double\* rate_s_per_chunk, double\* snr, double\* base_out\);", text)
    assert re.search(r"^#define FXC_FRINGE_REF 0$", text, re.M) and re.search(r"^#define FXC_FRINGE_ALL 1$", text, re.M)
    assert (_lib.FXC_FRINGE_REF, _lib.FXC_FRINGE_ALL) == (0, 1)


def test_weighted_fit_is_exported_and_bound():
    handle = _lib.load()
    assert "fxc_fringe_fit_weighted" in _lib.SIGNATURES
    assert handle.fxc_fringe_fit_weighted is not None


def test_call_without_a_plan_is_an_argument_error():
    handle = _lib.load()
    rows = np.zeros((4, 1, 64), dtype=np.complex64)
    out = [np.full(2, -7.0), np.full(2, -7.0), np.full(2, -7.0), np.full((1, 3), -7.0)]
    rc = handle.fxc_fringe_fit_weighted(None, rows.ctypes.data, None, 4, _lib.FXC_MEM_HOST, BW, FC, 0, 2, _lib.FXC_FRINGE_ALL, 0.0,
                                        *[o.ctypes.data for o in out])
    assert rc == _lib.FXC_ERR_ARG
    assert all((o == -7.0).all() for o in out)


@needs_hipcc
def test_weighted_gather_compiles_without_scratch(asm_listing):  # noqa: F811
    res = kernel_resources(asm_listing)
    kernel = "fringe_gather_weighted_kernel"
    hits = {name: r for name, r in res.items() if re.search(r"{}{}".format(len(kernel), kernel), name)}
    assert len(hits) == 1, sorted(hits)
    vgprs, _, _, scratch, _ = next(iter(hits.values()))
    assert scratch == 0 and vgprs <= 128, (vgprs, scratch)


# -- the restatement -----------------------------------------------------------------------------------------------------------
def bits(*arrays):
    return [np.ascontiguousarray(a, dtype=np.float64).view(np.uint64) for a in arrays]


def same_bits(got, want):
    return all(np.array_equal(g, w) for g, w in zip(bits(*got), bits(*want)))


@pytest.mark.parametrize("ref", [0, 2])
def test_unit_weights_reproduce_the_plain_restatement(ref):
    n_ant, nchan, n_chunks = 4, 64, 48
    rng = np.random.default_rng(11)
    delays, rates = fringe_ref.draw_antennas(n_ant, nchan, rng)
    rows = fringe_ref.model_rows(n_chunks, n_ant, nchan, delays, rates, 1.0, rng)
    want = fringe_ref.fit_rows(rows, n_ant, BW, FC, ref=ref, pad=2)
    ones = np.ones((n_chunks, 6, nchan), np.float32)
    for w in (ones, None):
        got = fw.fit_rows_weighted(rows, w, n_ant, BW, FC, ref=ref, pad=2, baselines="ref")
        assert same_bits(got[:3], want[:3])
        index = {ab: i for i, ab in enumerate(fringe_ref.pairs(n_ant))}
        for b, peak in want[3].items():
            i = index[(min(ref, b), max(ref, b))]
            assert got[4][i] == peak
            sign = -1.0 if b < ref else 1.0          # base is as the row reads: D_hi - D_lo
            assert got[3][i, 0] == sign * want[0][b] and got[3][i, 1] == sign * want[1][b] and got[3][i, 2] == want[2][b]
        untouched = [i for ab, i in index.items() if ref not in ab]
        assert (got[3][untouched] == 0).all()


@pytest.mark.parametrize("baselines", ["ref", "all"])
def test_flagged_values_and_the_scale_of_the_weights_change_no_bit(baselines):
    rows, weights = fw.damaged_rows()
    assert np.isnan(rows).any() and np.isinf(rows.real).any() and (np.abs(rows.real) == np.float32(1e30)).any()
    want = fw.fit_rows_weighted(fw.zeroed(rows, weights), weights, 6, BW, FC, baselines=baselines)
    assert all(np.isfinite(a).all() for a in want[:4])
    assert same_bits(fw.fit_rows_weighted(rows, weights, 6, BW, FC, baselines=baselines)[:4], want[:4])
    assert same_bits(fw.fit_rows_weighted(rows, 4.0 * weights, 6, BW, FC, baselines=baselines)[:4], want[:4])
    # negative and NaN weights leave a sample out like 0
    odd = weights.copy()
    odd[5:7] = -1.0
    odd[7:9] = np.nan
    assert same_bits(fw.fit_rows_weighted(rows, odd, 6, BW, FC, baselines=baselines)[:4], want[:4])


def on_grid_base(n_ant, nchan, n_chunks, pad, md, qr, drop=()):
    """noiseless baselines of antennas at the grid cells md, qr: (delay, rate, snr) of every row, measured modulo the periods"""
    cd, cr = fringe_ref.cells(nchan, n_chunks, pad)
    pd, pr = nchan / BW, 1.0 / FC
    base = []
    for a, b in fringe_ref.pairs(n_ant):
        d, r = (md[b] - md[a]) * cd, (qr[b] - qr[a]) * cr
        d, r = d - pd * np.rint(d / pd), r - pr * np.rint(r / pr)          # what a baseline can see
        base.append((d, r, 0.0 if (a, b) in drop else np.sqrt(nchan * n_chunks)))
    return np.array(base)


@pytest.mark.parametrize("wraps", [False, True])
def test_solve_antennas_returns_on_grid_delays(wraps):
    """noiseless, on-grid: the antenna solution is the injected one to 1e-9 cell, also where differences leave the principal range
    (Lk = 128: antennas at -40 and +45 cells are 85 apart, seen as -43)"""
    n_ant, nchan, n_chunks, pad = 5, 64, 32, 2
    cd, cr = fringe_ref.cells(nchan, n_chunks, pad)
    md = np.array([0, 45, -40, 20, -7]) if wraps else np.array([0, 12, -9, 20, -7])
    qr = np.array([0, -25, 22, 3, 30]) if wraps else np.array([0, -5, 8, 3, 11])
    base = on_grid_base(n_ant, nchan, n_chunks, pad, md, qr)
    lk, lt = fringe_ref.grid(nchan, n_chunks, pad)
    assert any(abs(md[b] - md[a]) > lk // 2 for a, b in fringe_ref.pairs(n_ant)) == wraps
    d, r, s, used = fw.solve_antennas(base, n_ant, 0, nchan, n_chunks, pad, BW, FC)
    assert used.all()
    assert np.abs(d / cd - md).max() < 1e-9 and np.abs(r / cr - qr).max() < 1e-9
    assert s[0] == 0.0 and np.allclose(s[1:], np.sqrt(4 * nchan * n_chunks))
    # another reference: the differences to it
    d, r, s, _ = fw.solve_antennas(base, n_ant, 3, nchan, n_chunks, pad, BW, FC)
    want_d, want_r = md - md[3], qr - qr[3]
    want_d, want_r = (want_d + lk // 2) % lk - lk // 2, (want_r + lt // 2) % lt - lt // 2
    assert np.abs(d / cd - want_d).max() < 1e-9 and np.abs(r / cr - want_r).max() < 1e-9 and s[3] == 0.0


def test_an_antenna_without_a_used_baseline_gets_zeros():
    n_ant, nchan, n_chunks, pad = 5, 64, 32, 2
    cd, cr = fringe_ref.cells(nchan, n_chunks, pad)
    md, qr = np.array([0, 12, -9, 20, -7]), np.array([0, -5, 8, 3, 11])
    cut = [(a, b) for a, b in fringe_ref.pairs(n_ant) if 2 in (a, b)]
    base = on_grid_base(n_ant, nchan, n_chunks, pad, md, qr, drop=cut + [(0, 3)])
    d, r, s, used = fw.solve_antennas(base, n_ant, 0, nchan, n_chunks, pad, BW, FC)
    assert used.sum() == 10 - 4 - 1
    assert d[2] == 0.0 and r[2] == 0.0 and s[2] == 0.0
    keep = [1, 3, 4]                                  # antenna 3 has lost its baseline to ref and is still measured
    assert np.abs(d[keep] / cd - md[keep]).max() < 1e-9 and np.abs(r[keep] / cr - qr[keep]).max() < 1e-9
    assert np.allclose(s[3], np.sqrt(2 * nchan * n_chunks))
    # a threshold of one's own: nothing passes, every antenna gets zeros
    d, r, s, used = fw.solve_antennas(base, n_ant, 0, nchan, n_chunks, pad, BW, FC, min_snr=100.0)
    assert not used.any() and not d.any() and not r.any() and not s.any()


def test_threshold_is_the_false_alarm_level_of_the_grid():
    assert abs(fw.threshold(64, 32, 2) - 3.99) < 0.005              # Lk 128, Lt 64
    assert fw.threshold(64, 32, 2, min_snr=6.5) == 6.5


def test_the_damaged_fixture():
    c = fw.DAMAGED
    n_ant, nchan, n_chunks, pad = c["n_ant"], c["nchan"], c["n_chunks"], c["pad"]
    rows, weights = fw.damaged_rows()
    pairs = fringe_ref.pairs(n_ant)
    cd, cr = fringe_ref.cells(nchan, n_chunks, pad)
    pd, pr = nchan / BW, 1.0 / FC
    # the plain definition is lost on these rows: every antenna NaN
    with np.errstate(all="ignore"):
        plain = fringe_ref.fit_rows(rows, n_ant, BW, FC)
    assert np.isnan(plain[0][1:]).all()
    d, r, s, base, _ = fw.fit_rows_weighted(rows, weights, n_ant, BW, FC, baselines="all")
    _, _, _, used = fw.solve_antennas(base, n_ant, 0, nchan, n_chunks, pad, BW, FC)
    good = [i for i, (a, b) in enumerate(pairs) if 4 not in (a, b) and (a, b) != (0, 3)]
    noise = [i for i, (a, b) in enumerate(pairs) if 4 in (a, b)]
    assert len(good) == 9 and sorted(np.flatnonzero(used)) == good
    assert base[good, 2].min() > 25.0 and base[good, 2].max() < 30.0
    assert base[noise, 2].max() <= 3.5 < fw.threshold(nchan, n_chunks, pad)
    assert (base[pairs.index((0, 3))] == 0).all()
    i12 = pairs.index((1, 2))                         # the truth is -0.70 Pd: seen as +0.30
    assert abs(base[i12, 0] / pd - 0.30) < 0.01 and abs((fw.DAMAGED_D[2] - fw.DAMAGED_D[1]) / pd + 0.70) < 1e-12
    ed, er = d - fw.DAMAGED_D, r - fw.DAMAGED_R
    ed, er = (ed - pd * np.rint(ed / pd)) / cd, (er - pr * np.rint(er / pr)) / cr
    live = [1, 2, 3, 5]
    assert np.abs(ed[live]).max() < 0.03 and np.abs(er[live]).max() < 0.03, (ed, er)
    assert d[4] == 0.0 and r[4] == 0.0 and s[4] == 0.0 and s[0] == 0.0 and (s[live] > 40.0).all()
    d, r, s, base, _ = fw.fit_rows_weighted(rows, weights, n_ant, BW, FC, baselines="ref")
    assert d[3] == 0.0 and r[3] == 0.0 and s[3] == 0.0
    assert abs(s[4] - 2.9) < 0.1                      # a noise peak, reported as if it were a delay
