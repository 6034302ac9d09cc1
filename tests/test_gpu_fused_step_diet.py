"""The fused 4096-channel kernel's step after its diet (k_fused4096.h: w256 twiddles of the default instantiation in registers,
two branch rows per scalar load offset, the prefetch's chunk base carried from step to step and moved by additions), on the
device: 4096 channels, 4 taps, the rough asymmetric window of tests/window_cases.py, every chunk's row and the integration
against the float64 oracle.  The shapes are the smallest at which the changed address and walk logic can go wrong:

  complex64-3x5, 3x6       unroll remainders 1 and 2; every workgroup on the frame-range tail, ranges that start inside chunks
                           (ring prologue from the chunk's earlier frames, the carried base starts inside a chunk)
  complex64-259x2          one round of whole chunks on 256 workgroups, then a 3-chunk tail: the base is set up again for the tail
  complex64-515x2          two rounds: every workgroup's prefetch jumps by seg_jump chunks at each chunk end -- the carried base's
                           addition; its integration runs with unit > 1 (rows of several chunks) against the float64 mean of the rows
  bytes-dc-515x2           byte ingest with DC removal, the kernel sums its next chunk's bytes (keeps the per-step base)
  autos-3x5                the variant with autocorrelations (LDS twiddle table, FIR group of 2)
  four-antennas-3x5        spectra out, into the X-engine
  second call              the 515-chunk plan called again with 259 chunks: nothing carried in scalar registers survives a launch
Bounds: the fused route's own (tests/tolerances.py TOL_VIS)."""
import numpy as np
import pytest

import fx_oracle
import window_cases as wc
from effex_amd import synth
from tolerances import TOL_VIS

pytestmark = pytest.mark.gpu

NCHAN, NTAPS = 4096, 4
CASES = [  # id, n_ant, n_chunks, frames, bytes, autos
    ("complex64-3x5", 2, 3, 5, False, False),
    ("complex64-3x6", 2, 3, 6, False, False),
    ("complex64-259x2", 2, 259, 2, False, False),
    ("complex64-515x2", 2, 515, 2, False, False),
    ("bytes-dc-515x2", 2, 515, 2, True, False),
    ("autos-3x5", 2, 3, 5, False, True),
    ("four-antennas-3x5", 4, 3, 5, False, False),
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


def check(name, rows, integ, ref, n_ant, autos):
    assert rows.shape == ref.shape
    n_chunks = ref.shape[0]
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


@pytest.fixture(scope="module")
def two_rounds():
    """515 x 2 frames of complex64 and their float64 rows, computed once: the 515-chunk case and the second-call test share them."""
    num_samp = NCHAN * 2
    window = wc.rough_window(NTAPS, NCHAN)
    x = synth.synth_iq(17 + 515, 515, 2, num_samp, delays=np.arange(2) % 5)
    ref = reference(x, window, False)
    ref.setflags(write=False)
    return x, window, ref


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_rows_and_integration_match_the_oracle(torch, case, two_rounds):
    from effex_amd.plan import FxPlan
    name, n_ant, n_chunks, frames, u8, autos = case
    num_samp = NCHAN * frames
    if name == "complex64-515x2":
        raw, window, ref = two_rounds
    else:
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
            plan.fx_accumulate(xd)      # (two antennas: raw rows of `unit` chunks, unit > 1 at 2 frames a chunk)
        integ = plan.finalize("SPECTRUM")
    check(name, rows, integ, ref, n_ant, autos)


def test_second_call_with_another_chunk_count(torch, two_rounds):
    """One plan, 515 chunks then the first 259 of them (two rounds, then one round and a tail), then 515 again."""
    from effex_amd.plan import FxPlan
    x, window, ref = two_rounds
    xd = torch.from_numpy(x).cuda()
    with FxPlan(2, NCHAN, NTAPS, NCHAN * 2, window=window, path="fused") as plan:
        for n in (515, 259, 515):
            rows = plan.fx_rows(xd[:n], "SPECTRUM").cpu().numpy()
            plan.fx_accumulate(xd[:n])
            integ = plan.finalize("SPECTRUM")
            check("second-call-%d" % n, rows, integ, ref[:n], 2, False)
