"""Per-antenna delay correction and batched delay calibration (include/fxcorr.h fxc_set_rot_ant, fxc_estimate_delays), the parts
that need no GPU: the declarations, the exported and bound symbols, the argument checks that answer before any device is
touched, the host-side tables, and the compiled ANT finish kernels (k_finish.h) -- no scratch, beside the shared-rot ones."""
import ctypes
import os
import re

import numpy as np
import pytest

from effex_amd import _lib
from effex_amd.plan import rot_table, rot_tables
from test_isa_hazards import asm_listing, kernel_resources, needs_hipcc  # noqa: F401  (the module's listing fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fxcorr.h")


def test_header_declares_the_per_antenna_api():
    text = open(HEADER).read()
    assert re.search(r"int fxc_set_rot_ant\(fxc_plan\* plan, const double\* rot_ant_re_im\);", text)
    assert re.search(r"int fxc_estimate_delays\(fxc_plan\* plan, const void\* x, int64_t n, int mem_kind, double rate, int ref, "
                     r"double\* delays_s\);", text)
    assert "#define FXC_VERSION 106" in text           # fxc_info does not grow: the version stays


def test_per_antenna_symbols_are_exported_and_bound():
    handle = _lib.load()
    for name in ("fxc_set_rot_ant", "fxc_estimate_delays"):
        assert name in _lib.SIGNATURES
        assert getattr(handle, name) is not None


def test_calls_without_a_plan_are_argument_errors():
    handle = _lib.load()
    tables = np.ones((3, 16), dtype=np.complex128)
    assert handle.fxc_set_rot_ant(None, tables.ctypes.data) == _lib.FXC_ERR_ARG
    x = np.zeros((3, 64), dtype=np.complex64)
    out = np.full(3, -7.0)
    assert handle.fxc_estimate_delays(None, x.ctypes.data, 64, _lib.FXC_MEM_HOST, 1.0, 0, out.ctypes.data) == _lib.FXC_ERR_ARG
    assert (out == -7.0).all()


def test_rot_tables_rows_are_the_rot_tables_of_each_delay():
    nbins, bw, f0 = 1000, 2.048e6, 1.4204e9
    delays = np.array([0.0, 1.3e-6, -4.7e-7, 2.5e-9])
    tabs = rot_tables(nbins, bw, f0, delays)
    assert tabs.shape == (4, nbins) and tabs.dtype == np.complex128
    for a, d in enumerate(delays):
        assert np.array_equal(tabs[a], rot_table(nbins, bw, f0, d))
    assert np.array_equal(tabs[0], np.ones(nbins, dtype=np.complex128))


def test_two_antenna_combination_with_tau0_zero_is_the_shared_table():
    """fxc_set_rot_ant folds a 2-antenna plan's tables into w = r_1 conj(r_0), formed in float64 as below; with tau_0 = 0 that is
    r_1 itself, bit for bit -- the table fxc_set_rot(r_1) would upload."""
    tabs = rot_tables(4096, 2.048e6, 1.4204e9, [0.0, 3.3e-6])
    ra, rb = tabs[0], tabs[1]
    w_re = rb.real * ra.real + rb.imag * ra.imag
    w_im = rb.imag * ra.real - rb.real * ra.imag
    assert np.array_equal(w_re.view(np.uint64), rb.real.view(np.uint64))
    assert np.array_equal(w_im.view(np.uint64), rb.imag.view(np.uint64))


def _by_pattern(res, pattern):
    return {name: r for name, r in res.items() if re.search(pattern, name)}


@needs_hipcc
def test_per_antenna_finish_kernels_compile_without_scratch(asm_listing):  # noqa: F811
    res = kernel_resources(asm_listing)
    for kernel in ("rows_spectrum_kernel", "rows_continuum_kernel", "rows_continuum_part_kernel", "acc_finish_kernel",
                   "finalize_spectrum_kernel", "finalize_continuum_kernel"):
        for flag in ("1", "0"):
            # (the rows kernels: <ANT, TRACK>, the untracked forms here -- test_tracking_host.py has the tracked ones)
            hits = _by_pattern(res, r"{}{}ILb{}E{}".format(len(kernel), kernel, flag, "Lb0E" if kernel.startswith("rows_") else ""))
            assert len(hits) == 1, (kernel, flag, sorted(hits))
            vgprs, _, _, scratch, _ = next(iter(hits.values()))
            assert scratch == 0 and vgprs <= 128, (kernel, flag, vgprs, scratch)
    for row in ("N3fxc2cfE", "N3fxc2cdE"):
        hits = _by_pattern(res, r"18fold_finish_kernelI{}Lb1E".format(row))
        assert len(hits) == 1, (row, sorted(hits))
        assert next(iter(hits.values()))[3] == 0
    pad = _by_pattern(res, r"16delay_pad_kernel")
    assert len(pad) == 1 and next(iter(pad.values()))[3] == 0
