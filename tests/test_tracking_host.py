"""Delay tracking (include/fxcorr.h fxc_set_delay_track and the three calls beside it), the parts that need no GPU: the
declarations, the exported and bound symbols, the argument checks that answer before any device is touched, and the compiled
tracked kernels (k_finish.h, k_track.h) -- no scratch."""
import ctypes
import os
import re

import numpy as np
import pytest

from effex_amd import _lib
from test_isa_hazards import asm_listing, kernel_resources, needs_hipcc  # noqa: F401  (the module's listing fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fxcorr.h")
NAMES = ("fxc_set_delay_track", "fxc_delay_track_chunk", "fxc_delay_track_seek", "fxc_delay_track_tables")


def test_header_declares_the_tracking_api():
    text = re.sub(r"\s+", " ", open(HEADER).read())
    assert ("int fxc_set_delay_track(fxc_plan* plan, const double* tau0_s, const double* rate_s_per_chunk, double bandwidth, "
            "double frequency, int64_t first_chunk);") in text
    assert "int fxc_delay_track_chunk(const fxc_plan* plan, int64_t* next_chunk);" in text
    assert "int fxc_delay_track_seek(fxc_plan* plan, int64_t chunk);" in text
    assert "int fxc_delay_track_tables(fxc_plan* plan, int64_t chunk, double* out_re_im);" in text
    assert "#define FXC_VERSION 106" in text           # fxc_info does not grow: the version stays


def test_tracking_symbols_are_exported_and_bound():
    handle = _lib.load()
    assert handle.fxc_version() == 106
    for name in NAMES:
        assert name in _lib.SIGNATURES
        assert getattr(handle, name) is not None


def test_calls_without_a_plan_are_argument_errors():
    handle = _lib.load()
    tau = np.zeros(2)
    assert handle.fxc_set_delay_track(None, tau.ctypes.data, tau.ctypes.data, 2.4e6, 1.42e9, 0) == _lib.FXC_ERR_ARG
    t = ctypes.c_int64(-7)
    assert handle.fxc_delay_track_chunk(None, ctypes.byref(t)) == _lib.FXC_ERR_ARG and t.value == -7
    assert handle.fxc_delay_track_seek(None, 3) == _lib.FXC_ERR_ARG
    out = np.full((2, 16), -7.0 + 0j)
    assert handle.fxc_delay_track_tables(None, 0, out.ctypes.data) == _lib.FXC_ERR_ARG
    assert (out == -7.0).all()


def test_plan_methods_exist():
    from effex_amd.plan import FxPlan
    for name in ("set_delay_track", "track_chunk", "track_seek", "track_tables"):
        assert hasattr(FxPlan, name)
    assert isinstance(FxPlan.track_chunk, property)


@needs_hipcc
def test_tracked_kernels_compile_without_scratch(asm_listing):  # noqa: F811
    res = kernel_resources(asm_listing)
    for kernel in ("rows_spectrum_kernel", "rows_continuum_kernel", "rows_continuum_part_kernel"):
        for ant in ("0", "1"):
            for trk in ("0", "1"):
                hits = {n: r for n, r in res.items() if re.search(r"{}{}ILb{}ELb{}E".format(len(kernel), kernel, ant, trk), n)}
                assert len(hits) == 1, (kernel, ant, trk, sorted(hits))
                vgprs, _, _, scratch, _ = next(iter(hits.values()))
                assert scratch == 0 and vgprs <= 128, (kernel, ant, trk, vgprs, scratch)
    for kernel in ("track_tables_kernel", "track_fold_kernel"):
        for flag in ("0", "1"):
            hits = {n: r for n, r in res.items() if re.search(r"{}{}ILb{}E".format(len(kernel), kernel, flag), n)}
            assert len(hits) == 1, (kernel, flag, sorted(hits))
            vgprs, _, _, scratch, _ = next(iter(hits.values()))
            assert scratch == 0 and vgprs <= 128, (kernel, flag, vgprs, scratch)


@needs_hipcc
def test_rows_kernels_are_one_template(asm_listing):  # noqa: F811
    """The rows kernels are one text over <ANT, TRACK>: three stems x four instantiations, and no kernel named *_track_kernel
    (the tracked forms' names before they were template arguments)."""
    assert "_track_kernel" not in asm_listing
    names = list(kernel_resources(asm_listing))
    rows = [n for n in names if re.search(r"\d+rows_(spectrum|continuum|continuum_part)_kernelI", n)]
    assert len(rows) == 12 and len(set(rows)) == 12, sorted(rows)
