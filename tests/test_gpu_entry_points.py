"""Every spelling of one call gives the same bits.

The six entry points that take samples (fxc_fx_rows / fxc_fx_accumulate and their _u8 and _iq forms) and the pipe go through one
front end (effex_amd/csrc/h_ingest.h): rows of a device tensor, of a host array, written straight into pinned host memory
(FXC_MEM_DEVICE_TO_PINNED) and popped from a depth-2 pipe are the same launches on the same chunks, so they are compared with
``np.array_equal`` -- accuracy against the oracle is held by the rest of the suite.  Host and pipe inputs land in 256-byte
aligned library buffers and 4 chunks never reach the two rounds of chunks the in-kernel byte sums (DCK) need, so nothing here
depends on where a buffer happens to lie."""
import numpy as np
import pytest

from effex_amd import _lib

pytestmark = pytest.mark.gpu

BW = 2.4e6
FREQ = 1.42e9
N_CHUNKS = 4
FRAMES = 8

# the smallest shapes that reach each ingest branch: (antennas, channels, autos)
SHAPES = {
    "wave_local": (2, 64, False),        # bytes read in the wave-local kernel
    "per_count": (2, 1000, False),       # per-channel-count kernel from the pre-built code object, bytes in the kernel
    "staged": (3, 256, False),           # no in-kernel ingest: conversion into the staging buffer
    "autos": (2, 64, True),              # 2 antennas, yet no in-kernel ingest
}
FORMATS = [("u8", True), ("u8", False), ("c64", True), ("c128", True), ("c128", False)]


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def plans(torch):
    """one plan per shape for the whole module"""
    from effex_amd.plan import FxPlan
    made = {}

    def get(shape):
        if shape not in made:
            n_ant, nchan, autos = SHAPES[shape]
            made[shape] = FxPlan(n_ant, nchan, 4, nchan * FRAMES, device=0, autos=autos)
        return made[shape]

    yield get
    for plan in made.values():
        plan.close()


def samples(shape, fmt):
    """seeded, with a mean worth removing"""
    n_ant, nchan, _ = SHAPES[shape]
    rng = np.random.default_rng(sorted(SHAPES).index(shape) * 10 + len(fmt))
    dims = (N_CHUNKS, n_ant, nchan * FRAMES)
    if fmt == "u8":
        return rng.integers(0, 256, size=dims + (2,), dtype=np.uint8)
    x = rng.standard_normal(dims) + 1j * rng.standard_normal(dims) + (0.3 - 0.2j)
    return x.astype(np.complex64 if fmt == "c64" else np.complex128)


def check_spellings(torch, plan, shape, fmt, remove_dc, mode, tracked):
    from effex_amd.plan import FxPipeline, pinned_empty
    x = samples(shape, fmt)
    xd = torch.from_numpy(x).cuda()

    def rewind():
        if tracked:
            plan.track_seek(0)

    def rows(src, out=None):
        rewind()
        if fmt == "u8":
            return plan.fx_rows_u8(src, mode, BW, remove_dc=remove_dc, out=out)
        return plan.fx_rows(src, mode, BW, remove_dc=remove_dc, out=out, c128=fmt == "c128")

    def integrate(src):
        rewind()
        if fmt == "u8":
            plan.fx_accumulate_u8(src, remove_dc=remove_dc)
        else:
            plan.fx_accumulate(src, remove_dc=remove_dc, c128=fmt == "c128")
        return plan.finalize(mode, BW)

    want = rows(xd).cpu().numpy()
    assert np.isfinite(want.view(want.real.dtype)).all() and np.abs(want).max() > 0
    assert np.array_equal(rows(x), want), "host array against device tensor"

    pinned = pinned_empty(want.shape, want.dtype)
    pinned[...] = 0
    rows(xd, out=pinned)
    plan.sync()
    assert np.array_equal(pinned, want), "FXC_MEM_DEVICE_TO_PINNED against device tensor"

    if fmt == "u8":
        rewind()
        out = torch.empty(want.shape, dtype=torch.complex64 if want.dtype == np.complex64 else torch.complex128, device=xd.device)
        plan._check(plan._lib.fxc_fx_rows_iq(plan._h, xd.data_ptr(), out.data_ptr(), N_CHUNKS, _lib.FXC_MEM_DEVICE,
                                             _lib.FXC_MODE_SPECTRUM if mode == "SPECTRUM" else _lib.FXC_MODE_CONTINUUM, BW,
                                             _lib.FXC_IQ_U8, int(remove_dc)))
        assert np.array_equal(out.cpu().numpy(), want), "fxc_fx_rows_iq(FXC_IQ_U8) against fxc_fx_rows_u8"

    # a depth-2 pipe: two batches in flight, then a slot's second use
    with FxPipeline(plan, N_CHUNKS, depth=2, mode=mode, bandwidth=BW, fmt=fmt, remove_dc=remove_dc) as pipe:
        rewind()
        pipe.push(x)
        rewind()
        pipe.push(x)
        popped = [pipe.pop(), pipe.pop()]
        rewind()
        pipe.push(x)
        popped.append(pipe.pop())
    for k, got in enumerate(popped):
        assert np.array_equal(got, want), "pipe batch %d against device tensor" % k

    assert np.array_equal(integrate(x), integrate(xd)), "accumulate + finalize: host array against device tensor"


@pytest.mark.parametrize("mode", ["SPECTRUM", "CONTINUUM"])
@pytest.mark.parametrize("fmt,remove_dc", FORMATS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_spellings_agree(torch, plans, shape, fmt, remove_dc, mode):
    plan = plans(shape)
    plan.set_delay(BW, FREQ, 1e-6)
    check_spellings(torch, plan, shape, fmt, remove_dc, mode, tracked=False)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_spellings_agree_under_a_delay_track(torch, plans, shape):
    """Bytes with DC removal under a delay track with a non-zero rate: every spelling rewinds the track to chunk 0 first."""
    plan = plans(shape)
    n_ant = SHAPES[shape][0]
    plan.set_delay_track(2e-6 * np.arange(n_ant), 1e-9 * (np.arange(n_ant) + 1.0), BW, FREQ)
    try:
        check_spellings(torch, plan, shape, "u8", True, "SPECTRUM", tracked=True)
    finally:
        plan.set_delay(BW, FREQ, 1e-6)
