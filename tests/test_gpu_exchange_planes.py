"""The fused 4096-channel kernel with lane-addressed exchange stores (fx_fused4096.h "exchanges"), every instantiation on the
device: 4096 channels, 4 taps, a rough asymmetric window (tests/window_cases.py) and every chunk's row against the float64 oracle.
Every (branch, tap) has a weight of its own, so a value that reaches the wrong lane -- the thread <-> branch map of phase 1 in
the loads, the twiddles or the window columns, a stripe of either exchange -- shows in specific bins of every row.

Cases (the path each exercises):
  complex64-3x5            every workgroup on the frame-range tail
  complex64-3x6            ... with ranges that start inside a chunk (ring prologue from the chunk's earlier frames)
  complex64-259x2-ragged   whole-chunk rounds on one workgroup per CU, then a tail; 100 samples beyond the last frame
  bytes-dc-259x2           byte ingest with DC removal
  bytes-dc-515x2           ... with two rounds of chunks: the kernel sums the bytes of a workgroup's next chunk itself
  autos-3x5                the variant with autocorrelations (lean twiddles)
  four-antennas-3x5        spectra out, into the X-engine
Bounds: the fused route's own (tests/tolerances.py TOL_VIS)."""
import numpy as np
import pytest

import fx_oracle
import window_cases as wc
from effex_amd import synth
from tolerances import TOL_VIS

pytestmark = pytest.mark.gpu

NCHAN, NTAPS = 4096, 4
CASES = [  # id, n_ant, n_chunks, frames, extra samples, bytes, autos
    ("complex64-3x5", 2, 3, 5, 0, False, False),
    ("complex64-3x6", 2, 3, 6, 0, False, False),
    ("complex64-259x2-ragged", 2, 259, 2, 100, False, False),
    ("bytes-dc-259x2", 2, 259, 2, 0, True, False),
    ("bytes-dc-515x2", 2, 515, 2, 0, True, False),
    ("autos-3x5", 2, 3, 5, 0, False, True),
    ("four-antennas-3x5", 4, 3, 5, 0, False, False),
]


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def reference(x, window, autos):
    """x [n_chunks, A, num_samp] (float64 oracle input) -> rows [n_chunks, n_rows, nchan]: baselines, then autos."""
    n_chunks, n_ant, _ = x.shape
    pairs = [(a, b) for a in range(n_ant) for b in range(a + 1, n_ant)]
    rows = np.zeros((n_chunks, len(pairs) + (n_ant if autos else 0), NCHAN), np.complex128)
    for c in range(n_chunks):
        specs = [fx_oracle.spectrometer_poly(x[c, a], NTAPS, NCHAN, window) for a in range(n_ant)]
        for p, (a, b) in enumerate(pairs):
            rows[c, p] = np.fft.fftshift((specs[a] * np.conj(specs[b])).mean(axis=0))
        if autos:
            for a in range(n_ant):
                rows[c, len(pairs) + a] = np.fft.fftshift((np.abs(specs[a]) ** 2).mean(axis=0))
    return rows


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_rows_match_the_oracle(torch, case):
    from effex_amd.plan import FxPlan
    name, n_ant, n_chunks, frames, extra, u8, autos = case
    num_samp = NCHAN * frames + extra
    window = wc.rough_window(NTAPS, NCHAN)
    if u8:
        raw = np.random.default_rng(n_chunks).integers(0, 256, size=(n_chunks, n_ant, num_samp, 2), dtype=np.uint8)
        a = fx_oracle.u8_to_complex(raw)
        x = np.stack([np.stack([fx_oracle.remove_dc(a[c, s]) for s in range(n_ant)]) for c in range(n_chunks)])
    else:
        raw = x = synth.synth_iq(17 + n_chunks, n_chunks, n_ant, num_samp, delays=np.arange(n_ant) % 5)
    ref = reference(x, window, autos)
    xd = torch.from_numpy(raw).cuda()
    with FxPlan(n_ant, NCHAN, NTAPS, num_samp, window=window, path="fused", autos=autos) as plan:
        assert plan.path == "fused" and plan.info["block"] == 512
        if n_chunks > 256:
            assert plan.info["grid"] == 256      # (the cases are cut for one workgroup on each of 256 CUs)
        rows = (plan.fx_rows_u8(xd, "SPECTRUM", remove_dc=True) if u8 else plan.fx_rows(xd, "SPECTRUM")).cpu().numpy()
        if u8:
            plan.fx_accumulate_u8(xd, remove_dc=True)
        else:
            plan.fx_accumulate(xd)
        integ = plan.finalize("SPECTRUM")
    assert rows.shape == ref.shape
    nb = n_ant * (n_ant - 1) // 2
    groups = [("cross", slice(0, nb))] + ([("autos", slice(nb, nb + n_ant))] if autos else [])
    for label, sl in groups:
        errs = [wc.rel_err(rows[c, sl], ref[c, sl]) for c in range(n_chunks)]
        worst = int(np.argmax(errs))
        print("%s: %s rows: largest error %.3g (chunk %d)" % (name, label, errs[worst], worst))
        assert errs[worst] < TOL_VIS, (name, label, worst)
        err = wc.rel_err(integ[sl], ref[:, sl].mean(axis=0))
        print("%s: %s integration: %.3g" % (name, label, err))
        assert err < TOL_VIS, (name, label)
