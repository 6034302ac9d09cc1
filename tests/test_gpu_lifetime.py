"""Closing a plan or a pipe gives the device memory back: cycles of create / use / close, free memory read before and after."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BW, FC = 2.4e6, 1.4204e9
# plan A: aligned delay track + gain track, host rows, bytes with DC removal, a continuum finalize, a pipe
A_ANT, A_NCHAN, A_TAPS, A_SAMP, A_CHUNKS = 3, 256, 4, 2 ** 20, 2
A_SOLUTIONS = 700
# plan B: the pre-filter route (more than 4 taps);  plan C: a result past the direct-write size (256 KiB), so the large-result path
B_ANT, B_NCHAN, B_TAPS, B_SAMP, B_CHUNKS = 2, 512, 8, 2 ** 20, 2
C_ANT, C_NCHAN, C_TAPS, C_SAMP = 8, 4096, 4, 4096 * 16
CF, CD = 8, 16      # bytes of a complex64 / complex128

# every buffer the cycle makes large on purpose, from the shapes (bytes)
LARGE = {
    "aligned samples (d_align), a pass of plan A": A_CHUNKS * A_ANT * A_SAMP * CF,
    "gain table (d_gain_q)": A_SOLUTIONS * A_ANT * A_NCHAN * CD,
    "host staging of the samples (d_stage[0])": A_CHUNKS * A_ANT * A_SAMP * CF,
    "converted bytes (d_stage[2])": A_ANT * A_SAMP * CF,
    "a pipe slot's device input": A_ANT * A_SAMP * CF,
    "pre-filtered streams (d_pre)": B_CHUNKS * B_ANT * B_SAMP * CF,
    # (acc_capacity: the cross rows and room for the autos of plans of up to 8 antennas)
    "large-result buffer (d_res_big), one of two": (C_ANT * (C_ANT - 1) // 2 + C_ANT) * C_NCHAN * CD,
}


def test_close_returns_device_memory():
    """12 cycles of three plans and a pipe, each used so that every lazily made buffer of a visible size is live at close():
    free device memory after cycle 12 against after cycle 2 must have fallen by less than the smallest buffer of LARGE
    (one such buffer leaked per cycle would cost ten times it), and every result equals cycle 1's bit for bit.

    What this cannot see: tables of a few KiB (d_one, d_shift, d_track_par, d_cont ...) -- below the grain of the allocator
    and of mem_get_info.  Those rest on the host test of the owners (tests/emul/emul_own.cpp) and on there being no list of
    buffers to free that a new one could be left off."""
    import torch
    from effex_amd.plan import FxPlan, FxPipeline

    assert LARGE["gain table (d_gain_q)"] >= 8 << 20
    assert LARGE["large-result buffer (d_res_big), one of two"] > 256 << 10
    bound = min(LARGE.values())

    rng = np.random.default_rng(61)

    def noise(*shape):
        return (rng.standard_normal(shape, dtype=np.float32) + 1j * rng.standard_normal(shape, dtype=np.float32)).astype(np.complex64)

    xa_host = noise(A_CHUNKS, A_ANT, A_SAMP)
    xa_u8 = torch.from_numpy(rng.integers(0, 256, (1, A_ANT, A_SAMP, 2), dtype=np.uint8)).cuda()
    xa_pipe = noise(1, A_ANT, A_SAMP)
    gains = (1.0 + 0.1 * rng.standard_normal((A_SOLUTIONS, A_ANT, A_NCHAN))) * np.exp(2j * np.pi * rng.random((A_SOLUTIONS, A_ANT, A_NCHAN)))
    delays, rates = [0.0, 3.2e-6, -1.7e-6], [0.0, 2e-9, -1e-9]
    xb = torch.from_numpy(noise(B_CHUNKS, B_ANT, B_SAMP)).cuda()
    out_b = torch.empty((B_CHUNKS, 1, B_NCHAN), dtype=torch.complex64, device="cuda")
    xc = torch.from_numpy(noise(1, C_ANT, C_SAMP)).cuda()

    def cycle():
        got = {}
        with FxPlan(A_ANT, A_NCHAN, A_TAPS, A_SAMP, device=0) as a:
            a.set_delay_track(delays, rates, BW, FC, whole_samples=True)
            a.set_track_gains(gains, interval=1)
            got["A rows"] = a.fx_rows(xa_host, "SPECTRUM")
            a.fx_accumulate_u8(xa_u8, remove_dc=True)
            got["A continuum"] = a.finalize("CONTINUUM", bandwidth=BW)
            pipe = FxPipeline(a, 1, depth=2)
            pipe.push(xa_pipe)
            got["A pipe rows"] = pipe.pop()
            pipe.close()
        with FxPlan(B_ANT, B_NCHAN, B_TAPS, B_SAMP, device=0) as b:
            b.fx_rows(xb, "SPECTRUM", out=out_b)
            got["B rows"] = out_b.cpu().numpy()
        with FxPlan(C_ANT, C_NCHAN, C_TAPS, C_SAMP, device=0) as c:
            c.fx_accumulate(xc)
            got["C spectrum"] = c.finalize("SPECTRUM")
        return got

    free = {}
    first = None
    for n in range(1, 13):
        got = cycle()
        if first is None:
            first = got
            for name, v in first.items():
                assert np.isfinite(v).all() and np.abs(v).max() > 0, name
        for name, v in got.items():
            assert torch.equal(torch.from_numpy(v), torch.from_numpy(first[name])), "%s of cycle %d differs from cycle 1's" % (name, n)
        if n in (2, 12):
            torch.cuda.synchronize()
            free[n] = torch.cuda.mem_get_info()[0]
    fell = free[2] - free[12]
    print("free device memory after cycle 2: %d B, after cycle 12: %d B, fell by %d B; smallest large buffer %d B" % (free[2], free[12], fell, bound))
    assert fell < bound, (fell, bound)
