"""Autocorrelation products (include/fxcorr.h fxc_products), the parts that need no GPU: the declarations, the exported and
bound symbols, the argument checks that answer before any device is touched, and the compiled X-engine that sums the autos
(k_finish.h::xengine_kernel<A, true>) -- no scratch, within the two-waves-per-SIMD register budget -- beside the untouched
headline kernel."""
import ctypes
import os
import re

import pytest

from effex_amd import _lib
from test_isa_hazards import asm_listing, kernel_resources, needs_hipcc  # noqa: F401  (the module's listing fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fxcorr.h")


def test_header_declares_the_products_api():
    text = open(HEADER).read()
    assert re.search(r"enum fxc_products\s*\{\s*FXC_PRODUCTS_CROSS\s*=\s*0\s*,\s*FXC_PRODUCTS_CROSS_AUTO\s*=\s*1\s*\}", text)
    assert re.search(r"int fxc_set_products\(fxc_plan\* plan, int products\);", text)
    assert re.search(r"int fxc_plan_products\(const fxc_plan\* plan, int\* products, int\* n_rows\);", text)
    assert "#define FXC_VERSION 106" in text           # fxc_info does not grow: the version stays
    assert _lib.FXC_PRODUCTS_CROSS == 0 and _lib.FXC_PRODUCTS_CROSS_AUTO == 1


def test_products_symbols_are_exported_and_bound():
    handle = _lib.load()
    for name in ("fxc_set_products", "fxc_plan_products"):
        assert name in _lib.SIGNATURES
        assert getattr(handle, name) is not None


def test_set_products_without_a_plan_is_an_argument_error():
    handle = _lib.load()
    assert handle.fxc_set_products(None, _lib.FXC_PRODUCTS_CROSS_AUTO) == _lib.FXC_ERR_ARG
    assert handle.fxc_set_products(None, _lib.FXC_PRODUCTS_CROSS) == _lib.FXC_ERR_ARG
    products, n_rows = ctypes.c_int(-5), ctypes.c_int(-5)
    assert handle.fxc_plan_products(None, ctypes.byref(products), ctypes.byref(n_rows)) == _lib.FXC_ERR_ARG
    assert (products.value, n_rows.value) == (-5, -5)


def _by_pattern(res, pattern):
    return {name: r for name, r in res.items() if re.search(pattern, name)}


@needs_hipcc
def test_autos_xengine_compiles_without_scratch(asm_listing):  # noqa: F811
    res = kernel_resources(asm_listing)
    for a in range(2, 9):
        hits = _by_pattern(res, r"xengine_kernelILi{}ELb1E".format(a))
        assert len(hits) == 1, (a, sorted(hits))
        vgprs, _, _, scratch, _ = next(iter(hits.values()))
        assert scratch == 0 and vgprs <= 256, (a, vgprs, scratch)
    # the cross-only X-engines are still there, as the multi-antenna routes launch them
    for a in range(3, 9):
        assert len(_by_pattern(res, r"xengine_kernelILi{}ELb0E".format(a))) == 1, a


@needs_hipcc
def test_fused_autos_variant_fits_two_waves_per_simd(asm_listing):  # noqa: F811
    """The 2-antenna 4096-channel F+X kernel with the autos in the same pass (fx_fused4096_kernel AUTOS) exists, has no scratch
    and stays within the 256 VGPRs of two waves per SIMD; the default instantiation keeps its 248 VGPRs."""
    res = kernel_resources(asm_listing)
    autos = _by_pattern(res, r"fx_fused4096_kernelILb0ELb0ELb0ELb1EEEv")
    assert len(autos) == 1, sorted(autos)
    vgprs, _, _, scratch, _ = next(iter(autos.values()))
    assert scratch == 0 and vgprs <= 256, (vgprs, scratch)
    default = _by_pattern(res, r"fx_fused4096_kernelILb0ELb0ELb0ELb0EEEv")
    assert len(default) == 1, sorted(default)
    vgprs, _, _, scratch, _ = next(iter(default.values()))
    assert (vgprs, scratch) == (248, 0)
