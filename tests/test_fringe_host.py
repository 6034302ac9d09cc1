"""Fringe fit (include/fxcorr.h fxc_fringe_fit), the parts that need no GPU: the declaration, the exported and bound symbol, the
call without a plan, the compiled kernels of k_fringe.h, and the float64 restatement of the definition (fringe_ref.py) on model
rows -- the reference tests/test_gpu_fringe.py holds the library to has to find the injected delay and rate itself."""
import os
import re

import numpy as np
import pytest

import fringe_ref
from effex_amd import _lib
from fringe_ref import BW, FC
from test_isa_hazards import asm_listing, kernel_resources, needs_hipcc  # noqa: F401  (the module's listing fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fxcorr.h")


def test_header_declares_fringe_fit():
    text = open(HEADER).read()
    assert re.search(r"int fxc_fringe_fit\(fxc_plan\* plan, const void\* rows, int64_t n_chunks, int mem_kind, double bandwidth, "
                     r"double frequency,\s+int ref, int pad, double\* delay_s, double\* rate_s_per_chunk, double\* snr\);", text)
    assert "#define FXC_VERSION 106" in text           # fxc_info does not grow: the version stays


def test_fringe_fit_is_exported_and_bound():
    handle = _lib.load()
    assert "fxc_fringe_fit" in _lib.SIGNATURES
    assert handle.fxc_fringe_fit is not None


def test_call_without_a_plan_is_an_argument_error():
    handle = _lib.load()
    rows = np.zeros((4, 1, 64), dtype=np.complex64)
    d, r, s = np.full(2, -7.0), np.full(2, -7.0), np.full(2, -7.0)
    rc = handle.fxc_fringe_fit(None, rows.ctypes.data, 4, _lib.FXC_MEM_HOST, BW, FC, 0, 2, d.ctypes.data, r.ctypes.data, s.ctypes.data)
    assert rc == _lib.FXC_ERR_ARG
    assert (d == -7.0).all() and (r == -7.0).all() and (s == -7.0).all()


@needs_hipcc
def test_fringe_kernels_compile_without_scratch(asm_listing):  # noqa: F811
    res = kernel_resources(asm_listing)
    for kernel in ("fringe_gather_kernel", "fringe_time_peak_kernel", "fringe_stencil_kernel"):
        hits = {name: r for name, r in res.items() if re.search(r"{}{}".format(len(kernel), kernel), name)}
        assert len(hits) == 1, (kernel, sorted(hits))
        vgprs, _, _, scratch, _ = next(iter(hits.values()))
        assert scratch == 0 and vgprs <= 128, (kernel, vgprs, scratch)


def test_grid_is_the_next_power_of_two():
    assert fringe_ref.grid(64, 48, 1) == (64, 64)
    assert fringe_ref.grid(1000, 48, 2) == (2048, 128)
    assert fringe_ref.grid(4096, 128, 4) == (16384, 512)


def test_restatement_on_a_noiseless_fringe_is_exact_at_a_cell():
    """a fringe that sits on a grid cell comes back as that cell; negative delay and rate map to signed indices"""
    nchan, n_chunks, pad = 64, 32, 2
    cd, cr = fringe_ref.cells(nchan, n_chunks, pad)
    f = fringe_ref.bin_frequencies(nchan)
    t = np.arange(n_chunks)[:, None]
    # the time term of the definition takes f_k = FC: build the rows the same way so that the cell is exact
    for m, q in ((5, 3), (-7, -11), (0, 0)):
        R = np.exp(2j * np.pi * ((f - f[0])[None, :] * (m * cd) + t * q * cr * FC))
        d, r, snr, peak = fringe_ref.fit_baseline(R, BW, FC, pad)
        assert peak == (q % 64, m % 128)
        # the two neighbours of the peak along an axis are equal in exact arithmetic: offsets vanish to rounding
        assert abs(d - m * cd) < 1e-6 * cd and abs(r - q * cr) < 1e-6 * cr
        assert abs(snr - np.sqrt(nchan * n_chunks)) < 1e-9 * snr


@pytest.mark.parametrize("pad", [1, 2, 4])
@pytest.mark.parametrize("nchan,n_chunks", [(256, 64), (1000, 48), (4096, 128)])
def test_restatement_finds_the_injected_fringe(nchan, n_chunks, pad):
    """40 seeded draws, snr_in 0.2, delay and rate within 0.4 nchan / bandwidth and 0.4 / frequency: every fit within half a
    grid cell of the truth -- a condition (the right peak), not a measurement."""
    rng = np.random.default_rng(1000 * nchan + 10 * n_chunks + pad)
    cd, cr = fringe_ref.cells(nchan, n_chunks, pad)
    worst = [0.0, 0.0]
    for draw in range(40):
        delay = rng.uniform(-0.4, 0.4) * nchan / BW
        rate = rng.uniform(-0.4, 0.4) / FC
        R = fringe_ref.model_baseline(n_chunks, nchan, delay, rate, 0.2, rng)
        d, r, snr, _ = fringe_ref.fit_baseline(R, BW, FC, pad)
        ed, er = abs(d - delay) / cd, abs(r - rate) / cr
        worst = [max(worst[0], ed), max(worst[1], er)]
        assert ed < 0.5 and er < 0.5, (draw, ed, er, snr)
    print("nchan %d chunks %d pad %d: worst error in cells, delay %.3f rate %.3f" % (nchan, n_chunks, pad, worst[0], worst[1]))


def test_fit_rows_conjugates_below_the_reference():
    """antenna residuals D_a: with any ref the fit of antenna b is D_b - D_ref, from row (ref, b) or the conjugate of (b, ref)"""
    n_ant, nchan, n_chunks = 4, 64, 48
    rng = np.random.default_rng(5)
    delays, rates = fringe_ref.draw_antennas(n_ant, nchan, rng)
    rows = fringe_ref.model_rows(n_chunks, n_ant, nchan, delays, rates, 1.0, rng)
    cd, cr = fringe_ref.cells(nchan, n_chunks, 2)
    for ref in (0, 2, 3):
        d, r, snr, _ = fringe_ref.fit_rows(rows, n_ant, BW, FC, ref=ref, pad=2)
        assert d[ref] == 0.0 and r[ref] == 0.0 and snr[ref] == 0.0
        for b in range(n_ant):
            if b != ref:
                assert abs(d[b] - (delays[b] - delays[ref])) < 0.5 * cd and abs(r[b] - (rates[b] - rates[ref])) < 0.5 * cr
