"""The dedispersion on the GPU (include/fxcorr.h fxc_dedisperse, FxPlan.dedisperse) against the numpy restatement of its definition
(dedisperse_ref.py).  The output must EQUAL the restatement's bits on host and on device input: every add is a single IEEE
operation in a fixed order, so there is nothing to tolerate.  Seeded power goes straight into dedisperse; the closure test takes
it from the beamformer.  Bits: no output depends on which kernel served a trial, on the tiles, on host against device input, on
the alignment of a device tensor, on the workspace target, on what an uncounted channel holds or on a factor of four on the
channel weights; the call leaves its inputs and a delay track's counter alone."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import dedisperse_ref as ref
from dedisperse_ref import bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 8              # kDedD of effex_amd/csrc/k_dedisperse.h: the trials of a tile
TIME_TILE = 256    # kDedT: the output times of a tile
MAX_SPAN = 1023    # kDedMaxSpan: the spread of a group's shifts inside 32 channels the tiled kernel takes


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def plan_mod(torch):
    from effex_amd import plan
    return plan


def same(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(bits(got), bits(want))


def both_inputs(plan, torch, power, shifts, chan_weights=None):
    """dedisperse on host and on device input -> [(numpy result, info)] * 2; the device result must be a CUDA tensor"""
    host, h_info = plan.dedisperse(power, shifts, chan_weights=chan_weights, return_info=True)
    assert isinstance(host, np.ndarray) and host.dtype == np.float32
    dev, d_info = plan.dedisperse(torch.from_numpy(power).cuda(), shifts, chan_weights=chan_weights, return_info=True)
    assert dev.is_cuda and dev.dtype == torch.float32
    assert h_info == d_info and sum(h_info) == shifts.shape[0]
    return [(host, h_info), (dev.cpu().numpy(), d_info)]


def noise(rng, shape):
    return (rng.chisquare(32, shape) / 32.0).astype(np.float32)


def band_shifts(nchan, n_dm, top):
    """dm_shifts of the wide band (400 MHz at 600 MHz), the sample time chosen so that the last trial's largest shift is `top`"""
    from effex_amd.plan import dm_shifts
    dms = np.linspace(0.0, 20.0, n_dm) if n_dm > 1 else np.array([20.0])
    f = ref.freqs(nchan, ref.WIDE_BW, ref.WIDE_FC) / 1e6
    sweep = ref.DM_CONSTANT_S * 20.0 * (f.min() ** -2.0 - f.max() ** -2.0)
    sh = dm_shifts(nchan, ref.WIDE_BW, ref.WIDE_FC, dms, sweep / top if nchan > 1 and top > 0 else 1.0)
    assert sh.max() == (top if nchan > 1 else 0)
    return sh


def tables(rng, nchan, n_dm, n_t):
    last = rng.integers(0, n_t, (n_dm, nchan)).astype(np.int32)
    last[n_dm // 2, nchan // 3] = n_t - 1                      # n_out = 1
    return {"zeros": np.zeros((n_dm, nchan), np.int32), "band": band_shifts(nchan, n_dm, n_t // 2),
            "random": rng.integers(0, n_t // 2, (n_dm, nchan)).astype(np.int32), "one output": last}


# -- shapes -----------------------------------------------------------------------------------------------------------------------
# channels, chunks x series x bins: one step of 32 twice; an odd count with a partial segment and time crossing chunks with series
# in between; 15 segments plus one of 40; one channel.  Trials: 1, 5, D + 1, 2 D + 1.
SHAPES = [(64, (4, 1, 16)), (63, (3, 3, 37)), (1000, (2, 2, 64)), (1, (5, 2, 8))]
TRIALS = (1, 5, D + 1, 2 * D + 1)


@pytest.mark.parametrize("nchan,dims", SHAPES)
def test_outputs_equal_the_restatement(plan_mod, torch, nchan, dims):
    rng = np.random.default_rng(nchan + dims[2])
    power = noise(rng, dims + (nchan,))
    n_t = dims[0] * dims[2]
    with plan_mod.FxPlan(2, nchan, 4, nchan * 8) as plan:
        for n_dm in TRIALS:
            for name, shifts in tables(rng, nchan, n_dm, n_t).items():
                want = ref.dedisperse(power, shifts)
                assert want.shape == (dims[1], n_dm, n_t - int(shifts.max())) and (name != "one output" or want.shape[2] == 1)
                for got, info in both_inputs(plan, torch, power, shifts):
                    differ = int((bits(got) != bits(want)).sum()) if got.shape == want.shape else -1
                    print(nchan, dims, n_dm, name, "tiled / direct", info, "differ", differ)
                    assert same(got, want), (n_dm, name)


def test_one_output_more_than_a_time_tile(plan_mod, torch):
    """n_out = the time tile + 1: the second tile holds one output; 3-D and 2-D input are one chunk"""
    nchan = 64
    rng = np.random.default_rng(3)
    shifts = band_shifts(nchan, D + 1, 45)
    power = noise(rng, (2, TIME_TILE + 1 + 45, nchan))
    want = ref.dedisperse(power, shifts)
    assert want.shape == (2, D + 1, TIME_TILE + 1)
    with plan_mod.FxPlan(2, nchan, 4, nchan * 8) as plan:
        for got, info in both_inputs(plan, torch, power, shifts):
            assert same(got, want) and info == (D + 1, 0)
        one = plan.dedisperse(power[1], shifts)
        assert one.shape == (D + 1, TIME_TILE + 1) and same(one, want[1])
        out = torch.zeros((D + 1, TIME_TILE + 1), dtype=torch.float32, device="cuda")
        assert plan.dedisperse(torch.from_numpy(power[0]).cuda(), shifts, out=out) is out and same(out.cpu().numpy(), want[0])


# -- both kernels -------------------------------------------------------------------------------------------------------------------
def test_both_kernels_give_the_same_bits(plan_mod, torch):
    """64 channels, n_t 4096: shifts uniform in [0, n_t / 2) spread over more than 1023 samples in 32 channels -- the direct kernel;
    the band's table -- the tiled kernel; both kinds of trial in one call -- both; and a table served by the direct kernel alone
    gives the bits the tiled kernel gives for its trials"""
    nchan, dims = 64, (4, 1, 1024)
    n_t = 4096
    rng = np.random.default_rng(4)
    power = noise(rng, dims + (nchan,))
    wild = rng.integers(0, n_t // 2, (D, nchan)).astype(np.int32)
    for half in (wild[:, :32], wild[:, 32:]):
        assert half.max() - half.min() > MAX_SPAN
    band = band_shifts(nchan, D, 387)
    mixed = np.concatenate([band, wild, band[:3]])
    with plan_mod.FxPlan(2, nchan, 4, nchan * 8) as plan:
        for shifts, kernels in ((wild, (0, D)), (band, (D, 0)), (mixed, (D + 3, D))):
            want = ref.dedisperse(power, shifts)
            for got, info in both_inputs(plan, torch, power, shifts):
                assert info == kernels and same(got, want), kernels
        # the band's trials between wild ones: every group goes to the direct kernel, the band's bits stay
        spread = np.concatenate([band[:4], wild[:4], band[4:], wild[4:]])
        got, info = plan.dedisperse(power, spread, return_info=True)
        assert info == (0, 2 * D) and same(got, ref.dedisperse(power, spread))
        n_out = got.shape[2]
        assert np.array_equal(bits(got[:, :4]), bits(ref.dedisperse(power, band)[:, :4, :n_out]))
    # the direct kernel where time crosses chunks with series in between: 8 x 2 x 512
    power = noise(rng, (8, 2, 512, nchan))
    with plan_mod.FxPlan(2, nchan, 4, nchan * 8) as plan:
        for shifts, kernels in ((wild[:3], (0, 3)), (mixed, (D + 3, D))):
            want = ref.dedisperse(power, shifts)
            for got, info in both_inputs(plan, torch, power, shifts):
                assert info == kernels and same(got, want), kernels


# -- weights ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nchan,dims", [(63, (3, 3, 37)), (1000, (2, 2, 64))])
def test_uncounted_channels_are_selected_away(plan_mod, torch, nchan, dims):
    rng = np.random.default_rng(7 + nchan)
    power = noise(rng, dims + (nchan,))
    n_t = dims[0] * dims[2]
    shifts = tables(rng, nchan, D + 1, n_t)["random"]
    weights = (0.25 + 3.75 * rng.random(nchan)).astype(np.float32)
    off = rng.permutation(nchan)[:max(3, nchan // 5)]
    weights[off] = np.resize(np.array([0.0, -1.0, np.nan], np.float32), off.size)
    dirty = power.copy()
    for i, k in enumerate(off):
        dirty[..., k] = (np.nan, np.inf, 1e30)[i % 3]
    want = ref.dedisperse(power, shifts, weights)
    assert np.isfinite(want).all()
    with plan_mod.FxPlan(2, nchan, 4, nchan * 8) as plan:
        for p in (power, dirty):
            for got, _ in both_inputs(plan, torch, p, shifts, weights):
                assert same(got, want)
        for got, _ in both_inputs(plan, torch, power, shifts, weights * np.float32(4)):
            assert same(got, want)
        for got, _ in both_inputs(plan, torch, dirty, shifts, np.where(np.arange(nchan) % 2, 0.0, np.nan).astype(np.float32)):
            assert got.shape == want.shape and (bits(got) == 0).all()      # no channel counts: +0
        # a counted channel is used as it is
        got = plan.dedisperse(dirty, shifts)
        assert not np.isfinite(got).all()


# -- bits -------------------------------------------------------------------------------------------------------------------------
def test_a_device_tensor_off_16_bytes(plan_mod, torch):
    nchan, dims = 64, (3, 2, 50)
    rng = np.random.default_rng(8)
    power = noise(rng, dims + (nchan,))
    shifts = band_shifts(nchan, D + 1, 70)
    want = ref.dedisperse(power, shifts)
    flat = torch.empty(power.size + 1, dtype=torch.float32, device="cuda")
    view = flat[1:].view(power.shape)
    view.copy_(torch.from_numpy(power))
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 and flat.data_ptr() % 16 == 0
    with plan_mod.FxPlan(2, nchan, 4, nchan * 8) as plan:
        assert same(plan.dedisperse(view, shifts).cpu().numpy(), want)
        out = torch.zeros(want.size + 1, dtype=torch.float32, device="cuda")[1:].view(want.shape)
        assert out.data_ptr() % 16 == 4
        plan.dedisperse(view, shifts, out=out)
        assert same(out.cpu().numpy(), want)


def test_outputs_do_not_depend_on_the_slabs(plan_mod, torch):
    """A workspace target of 1 MiB (FXC_WS_MB is read once per process: a child) against the default here: 3 MB of host power go
    through in slabs of some 37 of the 64 chunks of a series with a halo of 300 samples -- the same bits, and the restatement's"""
    nchan, dims = 96, (64, 2, 64)
    rng = np.random.default_rng(9)
    power = noise(rng, dims + (nchan,))
    shifts = np.concatenate([band_shifts(nchan, D + 1, 300), rng.integers(0, 300, (2, nchan)).astype(np.int32)])
    weights = np.where(rng.random(nchan) < 0.2, 0.0, 1.0).astype(np.float32)
    want = ref.dedisperse(power, shifts, weights)
    code = ("import numpy as np, torch, sys; sys.path.insert(0, %r); from effex_amd import plan\n"
            "d = np.load(sys.argv[1]); out = {}\n"
            "with plan.FxPlan(2, %d, 4, %d) as p:\n"
            "    out['h'] = p.dedisperse(d['power'], d['shifts'], chan_weights=d['weights'])\n"
            "    out['d'] = p.dedisperse(torch.from_numpy(d['power']).cuda(), d['shifts'], chan_weights=d['weights']).cpu().numpy()\n"
            "np.savez(sys.argv[2], **out)\n" % (ROOT, nchan, nchan * 8))
    with tempfile.TemporaryDirectory() as tmp:
        np.savez(os.path.join(tmp, "in.npz"), power=power, shifts=shifts, weights=weights)
        res = os.path.join(tmp, "one.npz")
        subprocess.run([sys.executable, "-c", code, os.path.join(tmp, "in.npz"), res], check=True, env=dict(os.environ, FXC_WS_MB="1"),
                       timeout=600)
        small = dict(np.load(res))
    assert same(small["h"], want) and same(small["d"], want)
    with plan_mod.FxPlan(2, nchan, 4, nchan * 8) as plan:
        for got, _ in both_inputs(plan, torch, power, shifts, weights):
            assert same(got, want)


def test_inputs_and_the_track_are_left_alone(plan_mod, torch):
    nchan, dims = 64, (4, 2, 32)
    rng = np.random.default_rng(10)
    power = noise(rng, dims + (nchan,))
    shifts = band_shifts(nchan, 5, 40)
    weights = np.ones(nchan, np.float32)
    weights[5] = 0.0
    keep_p, keep_s, keep_w = power.copy(), shifts.copy(), weights.copy()
    want = ref.dedisperse(power, shifts, weights)
    with plan_mod.FxPlan(4, nchan, 4, nchan * 8) as plan:
        plan.set_delay_track(np.linspace(0.0, 1e-7, 4), np.zeros(4), 2.4e6, 1.4204e9)
        plan.track_seek(5)
        dev = torch.from_numpy(power).cuda()
        assert same(plan.dedisperse(power, shifts, chan_weights=weights), want)
        assert same(plan.dedisperse(dev, torch.from_numpy(shifts).cuda(), chan_weights=torch.from_numpy(weights).cuda()).cpu().numpy(), want)
        assert plan.track_chunk == 5
        assert np.array_equal(bits(dev.cpu().numpy()), bits(keep_p)) and np.array_equal(bits(power), bits(keep_p))
        assert np.array_equal(shifts, keep_s) and np.array_equal(bits(weights), bits(keep_w))


# -- closure on the device ----------------------------------------------------------------------------------------------------------
def test_a_dispersed_impulse_through_the_beamformer(plan_mod, torch):
    """2 antennas, 64 channels: noise plus an impulse dispersed on the host by a chirp in the frequency domain, beamform(POWER, tint=1)
    on the device, dedisperse on its output without leaving the device: the largest cell lies at the injected trial, and the result
    equals the restatement applied to the beamformer's own output"""
    from effex_amd.window import design_window
    n_ant, nchan, ntaps, n_chunks, n_pts = 2, 64, 4, 4, 64
    bw, fc = 16e6, 1.4e9          # 12 samples of sweep per unit DM: 73 at the injected trial, 91 at the last
    num_samp = nchan * n_pts
    n = n_chunks * num_samp
    dms = np.arange(6) * 1.5
    true = 4
    rng = np.random.default_rng(12)
    # H(f) = exp(2 pi i k_DM DM f^2 / (f0^2 (f0 + f))) at baseband offset f: the cold-plasma chirp
    f = np.fft.fftfreq(n, d=1.0 / bw)
    chirp = np.exp(2j * np.pi * ref.DM_CONSTANT_S * 1e12 * dms[true] * f * f / (fc * fc * (fc + f)))
    impulse = np.zeros(n, np.complex128)
    impulse[n // 6] = 40.0
    pulse = np.fft.ifft(np.fft.fft(impulse) * chirp)
    x = np.empty((n_chunks, n_ant, num_samp), np.complex64)
    for a in range(n_ant):
        noise_a = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.05
        x[:, a] = (pulse + noise_a).reshape(n_chunks, num_samp)
    weights = np.ones((1, n_ant, nchan), np.complex64)
    shifts = plan_mod.dm_shifts(nchan, bw, fc, dms, nchan / bw)
    assert shifts[true].max() > 8 and shifts.max() < n_chunks * n_pts // 2
    with plan_mod.FxPlan(n_ant, nchan, ntaps, num_samp, window=design_window(ntaps, nchan)) as plan:
        assert plan.n_pts == n_pts
        power = plan.beamform(torch.from_numpy(x).cuda(), torch.from_numpy(weights).cuda(), tint=1)
        assert power.is_cuda and tuple(power.shape) == (n_chunks, 1, n_pts, nchan)
        got, info = plan.dedisperse(power, shifts, return_info=True)
        assert got.is_cuda and info == (len(dms), 0)
        got = got.cpu().numpy()
        cell = np.unravel_index(np.argmax(got), got.shape)
        peaks = got[0].max(axis=1)
        print("peaks per trial", peaks, "largest cell", cell)
        assert cell[1] == true
        assert same(got, ref.dedisperse(power.cpu().numpy(), shifts))


# -- arguments ----------------------------------------------------------------------------------------------------------------------
def test_dedisperse_argument_checks(plan_mod, torch):
    from effex_amd import _lib
    nchan, dims = 64, (3, 2, 16)
    rng = np.random.default_rng(13)
    power = noise(rng, dims + (nchan,))
    shifts = rng.integers(0, 20, (5, nchan)).astype(np.int32)
    negative = shifts.copy()
    negative[3, 9] = -1
    late = shifts.copy()
    late[4, 63] = 48                                          # S_max = n_t

    def call(plan, power_ptr, n_chunks=3, n_series=2, n_tbin=16, kind=_lib.FXC_MEM_HOST, table=shifts, n_dm=5, out=True, plan_h=True):
        o, info = np.full((2, 5, 48), -7.0, np.float32), np.full(2, -7, np.int64)
        rc = plan._lib.fxc_dedisperse(plan._h if plan_h else None, power_ptr, n_chunks, n_series, n_tbin, kind,
                                      None if table is None else table.ctypes.data, n_dm, None, o.ctypes.data if out else None,
                                      info.ctypes.data)
        if rc != 0:
            assert (o == -7.0).all() and (info == -7).all(), "outputs written on an error"
        return rc

    with plan_mod.FxPlan(2, nchan, 4, nchan * 8) as plan:
        ptr = power.ctypes.data
        for change in (dict(power_ptr=None), dict(table=None), dict(out=False), dict(plan_h=False), dict(n_chunks=0), dict(n_chunks=-2),
                       dict(n_series=0), dict(n_tbin=0), dict(n_tbin=-1), dict(n_dm=0), dict(n_dm=-1), dict(kind=7),
                       dict(kind=_lib.FXC_MEM_DEVICE_TO_PINNED), dict(table=negative), dict(table=late)):
            args = dict(power_ptr=ptr)
            args.update(change)
            rc = call(plan, **args)
            assert rc == _lib.FXC_ERR_ARG, change
            if "plan_h" not in change:
                with pytest.raises(ValueError):
                    _lib.check(rc, plan._h)
        assert call(plan, ptr) == 0
        # n_t >= 2^31 through the arguments alone: nothing that large is allocated or read
        for n_chunks, n_tbin in ((1 << 20, 1 << 11), (1, 1 << 31), (1 << 40, 1 << 40)):
            rc = call(plan, ptr, n_chunks=n_chunks, n_tbin=n_tbin)
            assert rc == _lib.FXC_ERR_UNSUPPORTED
            with pytest.raises(NotImplementedError):
                _lib.check(rc, plan._h)
        assert call(plan, ptr, n_chunks=(1 << 20) - 1, n_tbin=1 << 11, table=negative) == _lib.FXC_ERR_ARG
        # the Python exceptions
        dev = torch.from_numpy(power).cuda()
        for bad in (dict(shifts=negative), dict(shifts=late), dict(shifts=shifts[:, :32]), dict(shifts=shifts.astype(np.float32)),
                    dict(shifts=shifts[0]), dict(chan_weights=np.ones(32, np.float32)), dict(chan_weights=np.ones(nchan, np.int32)),
                    dict(out=torch.zeros((2, 5, 29), dtype=torch.float32, device="cuda")), dict(out=np.zeros((2, 5, 28), np.float32)),
                    dict(out=np.zeros((2, 5, 29), np.float64))):
            args = dict(shifts=shifts)
            args.update(bad)
            with pytest.raises(ValueError):
                plan.dedisperse(power, **args)
        with pytest.raises(ValueError):
            plan.dedisperse(dev, shifts, out=np.zeros((2, 5, 29), np.float32))      # mixed host and device memory
        for bad_power in (power.astype(np.float64), power[..., :32], power[0, 0, 0], dev.double(), torch.from_numpy(power)):
            with pytest.raises(ValueError):
                plan.dedisperse(bad_power, shifts)
        assert int(shifts.max()) == 19 and plan.dedisperse(power, shifts).shape == (2, 5, 29)
