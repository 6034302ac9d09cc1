"""Every butterfly x stage position and layout feature of the kernels compiled per channel count, on the device: one case per entry of
the cover list (tests/golden/spec_cover.json, tests/spec_cover.py) -- the channel counts whose builds, between them, run everything the
measured table effex_amd/csrc/spec_tuned.h and a sample of the cost model's choices use -- against the float64 oracle.

Four taps and design_window(4, nchan) throughout (the table applies to four taps).  Shapes: 7 frames (odd: a build that carries two
frames a step ends on a single one; more than 2 * taps - 1), 41 frames up to 64 channels (several slots and splits get runs of
different lengths), a tail of min(3, nchan - 1) samples that is dropped, 3 chunks.  Bounds: the ceilings of tests/tolerances.py
(TOL_VIS, TOL_SPEC_ANY: 1e-5) and the suite's 2e-6 for an integration against the float64 mean of its rows."""
import numpy as np
import pytest

import fx_oracle
import golden_inputs as gi
import spec_cover
from effex_amd import synth
from effex_amd.window import design_window

pytestmark = pytest.mark.gpu

from tolerances import TOL_SPEC_ANY, TOL_VIS

NTAPS, N_CHUNKS, DELAY = 4, 3, 3e-7
ENTRIES = spec_cover.cover_entries()


def _cases(variant):
    return [pytest.param(n, e, id="%s-%d" % (spec_cover.VARIANT_TAG[variant], n)) for v, n, e in ENTRIES if v == variant]


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def plan_mod(torch):
    from effex_amd import plan
    return plan


def rel_err(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


def shape_of(nchan):
    frames = 41 if nchan <= 64 else 7
    return frames, nchan * frames + min(3, nchan - 1)


def two_antenna_checks(p, torch, x, nchan, window):
    """rows of every chunk against the oracle, the same bits from a second call, the integration against the float64 mean of the rows"""
    xd = torch.from_numpy(x).cuda()
    p.set_delay(gi.BANDWIDTH, gi.FREQUENCY, DELAY)
    rows = p.fx_rows(xd, "SPECTRUM").cpu().numpy()
    for c in range(x.shape[0]):
        ref = fx_oracle.pfb_xcorr(x[c, 0], x[c, 1], NTAPS, nchan, window, gi.BANDWIDTH, gi.FREQUENCY, DELAY, "SPECTRUM")
        err = rel_err(rows[c, 0], ref)
        print("nchan %d chunk %d rows err %.3g" % (nchan, c, err))
        assert err < TOL_VIS, c
    np.testing.assert_array_equal(p.fx_rows(xd, "SPECTRUM").cpu().numpy(), rows)
    p.fx_accumulate(xd)
    err = rel_err(p.finalize("SPECTRUM"), rows.astype(np.complex128).mean(axis=0))
    print("nchan %d integration against the mean of the rows %.3g" % (nchan, err))
    assert err < 2e-6


@pytest.mark.parametrize("nchan,entry", _cases(0))
def test_fx_cover_entry_on_the_device(plan_mod, torch, nchan, entry):
    """F + X in one pass (variant 0): the plan runs the recorded build (threads, LDS); where the entry stands for a first-stage (or
    only-stage) feature also the byte ingest (variant 1), whose first stage converts as it fills the ring."""
    rep = entry["report"]
    frames, num_samp = shape_of(nchan)
    window = design_window(NTAPS, nchan)
    x = synth.synth_iq(7000 + nchan, N_CHUNKS, 2, num_samp)
    with plan_mod.FxPlan(2, nchan, NTAPS, num_samp, window=window) as p:
        info = p.info
        assert info["specialised"] & 1, info
        assert info["block"] == rep["tpr"] * rep["slots"] and info["lds_bytes"] == rep["lds_bytes"], (info, rep)
        two_antenna_checks(p, torch, x, nchan, window)
        if any("first" in f or "only" in f for f in entry["chosen_for"]):
            u8 = np.random.default_rng(7000 + nchan).integers(0, 256, size=(N_CHUNKS, 2, num_samp, 2), dtype=np.uint8)
            by = p.fx_rows_u8(torch.from_numpy(u8).cuda(), "SPECTRUM", remove_dc=False).cpu().numpy()
            xc = fx_oracle.u8_to_complex(u8)
            for c in range(N_CHUNKS):
                ref = fx_oracle.pfb_xcorr(xc[c, 0], xc[c, 1], NTAPS, nchan, window, gi.BANDWIDTH, gi.FREQUENCY, DELAY, "SPECTRUM")
                err = rel_err(by[c, 0], ref)
                print("nchan %d chunk %d rows from bytes err %.3g" % (nchan, c, err))
                assert err < TOL_VIS, c


@pytest.mark.parametrize("nchan,entry", _cases(2))
def test_f_cover_entry_on_the_device(plan_mod, torch, nchan, entry):
    """The F stage alone (variant 2) under three antennas: nine streams (odd: the last pair is half empty) against the oracle's spectra,
    and the first chunk's rows, which read the antenna-interleaved spectra this build stores."""
    frames, num_samp = shape_of(nchan)
    window = design_window(NTAPS, nchan)
    x = synth.synth_iq(7000 + nchan, N_CHUNKS, 3, num_samp)
    xd = torch.from_numpy(x).cuda()
    flat = x.reshape(-1, num_samp)
    with plan_mod.FxPlan(3, nchan, NTAPS, num_samp, window=window) as p:
        spec = p.channelize(xd.reshape(-1, num_samp)).cpu().numpy()
        assert p.info["specialised"] & 2, p.info
        for s_ in (0, 4, 8):
            err = rel_err(spec[s_], fx_oracle.spectrometer_poly(flat[s_], NTAPS, nchan, window))
            print("nchan %d stream %d spectra err %.3g" % (nchan, s_, err))
            assert err < TOL_SPEC_ANY, s_
        err = rel_err(p.fx_rows(xd).cpu().numpy()[0], fx_oracle.fx_integrate(x[:1], nchan, window))
        print("nchan %d rows of chunk 0 err %.3g" % (nchan, err))
        assert err < TOL_VIS


@pytest.mark.parametrize("nchan,entry", _cases(3))
def test_second_pass_cover_entry_on_the_device(plan_mod, torch, nchan, entry):
    """Two antennas above 4096 channels (variant 3): antenna 0 through the F-only build, antenna 1 through the second-pass build whose last
    butterfly multiplies with antenna 0's spectra."""
    frames, num_samp = shape_of(nchan)
    window = design_window(NTAPS, nchan)
    x = synth.synth_iq(7000 + nchan, N_CHUNKS, 2, num_samp)
    with plan_mod.FxPlan(2, nchan, NTAPS, num_samp, window=window) as p:
        two_antenna_checks(p, torch, x, nchan, window)
        assert p.info["specialised"] & 4, p.info
