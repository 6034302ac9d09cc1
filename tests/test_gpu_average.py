"""The averager on the GPU (include/fxcorr.h fxc_average_rows, FxPlan.average_rows) against the numpy restatement of its definition
(average_ref.py).  Both outputs must EQUAL the restatement's: every product is exact in float64, every add and the division are
single IEEE operations in a fixed order, so there is nothing to tolerate.  Seeded random rows go straight into average_rows (no
F / X stage).  Bits: no output depends on host against device input, on the alignment of a device tensor, on the workspace
target, on auto rows behind the cross rows, on what an uncounted sample holds or on a factor of four on the weights, and the call
leaves a delay track's counter alone.  Downstream: the pair at freq_bin 1 goes into solve_gains(vis, weights=wsum).  Closure: the
damaged samples of tests/test_gains_weighted_host.py through fx_rows, flag_rows and average_rows without leaving the device, under
the bound of tests/golden/average_bounds.json."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import average_ref
import gains_ref
import gains_weighted_ref as wref
from effex_amd.window import design_window
from test_average_host import BOUNDS, CELL_FLOOR, bits, closure_of, flagged_case, noisy_rows, same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CEIL_PARITY = 1e-9          # the gain solve against its restatement
BW, FC = 2.4e6, 1.4204e9


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def plan_mod(torch):
    from effex_amd import plan
    return plan


def n_base(n_ant):
    return n_ant * (n_ant - 1) // 2


def to_numpy(pair):
    return tuple(a if isinstance(a, np.ndarray) else a.cpu().numpy() for a in pair)


def both_inputs(plan, torch, rows, weights=None, **kw):
    """average_rows on host and on device input, as numpy; the device result must be a pair of CUDA tensors"""
    host = plan.average_rows(rows, weights=weights, **kw)
    assert isinstance(host[0], np.ndarray) and isinstance(host[1], np.ndarray)
    dev = plan.average_rows(torch.from_numpy(rows).cuda(), weights=None if weights is None else torch.from_numpy(weights).cuda(), **kw)
    assert dev[0].is_cuda and dev[0].dtype == torch.complex64 and dev[1].is_cuda and dev[1].dtype == torch.float32
    return host, to_numpy(dev)


def cases(n_ant, nchan, n_chunks):
    """-> rows and the weight sets of a shape: none; 0.25 .. 4 with 20 % of the samples, a dead baseline (where there are two) and
    a dead bin (where there are four) flagged as 0, -1 or NaN and overwritten with NaN / Inf / 1e30"""
    rng = np.random.default_rng(1000 * n_ant + nchan + n_chunks)
    nb = n_base(n_ant)
    rows, weights, _ = flagged_case(rng, n_chunks, nb, nchan, dead_baseline=nb - 1 if nb > 1 else None, dead_bin=3 if nchan > 3 else None)
    clean = noisy_rows(rng, n_chunks, nb, nchan)
    return ((clean, None), (rows, weights))


# -- shapes -----------------------------------------------------------------------------------------------------------------------
# antennas x channels x chunks, time_bins, freq_bins: one baseline and every freq_bin; partial last intervals (19 = 3 x 5 + 4 = 16 +
# 3) and one interval of all; an odd channel count (narrow loads) with a partial last bin at freq_bin 4; a tile of 511 bins (odd:
# narrow loads) and of 512 with a partial second tile; 2016 baselines; nchan 1
SHAPES = [(2, 64, 32, (0,), (1, 2, 3, 8, 64, 256)), (3, 64, 19, (0, 5, 16, 19), (1, 8)), (5, 63, 32, (0, 7), (1, 3, 4)),
          (8, 1000, 32, (0,), (1, 7, 8, 256)), (64, 64, 8, (0, 3), (1, 8)), (2, 1, 40, (0, 16), (1, 8))]


@pytest.mark.parametrize("n_ant,nchan,n_chunks,time_bins,freq_bins", SHAPES)
def test_outputs_equal_the_restatement(plan_mod, torch, n_ant, nchan, n_chunks, time_bins, freq_bins):
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * 8) as plan:
        for rows, weights in cases(n_ant, nchan, n_chunks):
            for time_bin in time_bins:
                for freq_bin in freq_bins:
                    want = average_ref.average_rows(rows, weights, time_bin, freq_bin)
                    assert want[0].shape == (len(average_ref.intervals(n_chunks, time_bin)), n_base(n_ant), -(-nchan // freq_bin))
                    if weights is not None:
                        assert (want[1] > 0).any() and (freq_bin > 1 or nchan <= 3 or (want[1] == 0).any())      # the dead bin
                    for got in both_inputs(plan, torch, rows, weights, time_bin=time_bin, freq_bin=freq_bin):
                        differ = int((bits(got[0]) != bits(want[0])).sum()) if got[0].shape == want[0].shape else -1
                        print(n_ant, nchan, n_chunks, "weights" if weights is not None else "none", time_bin, freq_bin, "differ", differ)
                        assert same(got, want), (time_bin, freq_bin)


def test_a_freq_bin_of_257_is_unsupported(plan_mod, torch):
    from effex_amd import _lib
    rows = np.ones((4, 1, 600), np.complex64)
    vis = np.full((1, 1, 3), -7.0 - 7.0j, np.complex64)
    wsum = np.full((1, 1, 3), -7.0, np.float32)
    with plan_mod.FxPlan(2, 600, 4, 600 * 8) as plan:
        rc = plan._lib.fxc_average_rows(plan._h, rows.ctypes.data, None, 4, _lib.FXC_MEM_HOST, 0, 257, vis.ctypes.data, wsum.ctypes.data)
        assert rc == _lib.FXC_ERR_UNSUPPORTED
        assert (vis == -7.0 - 7.0j).all() and (wsum == -7.0).all()
        with pytest.raises(NotImplementedError):
            plan.average_rows(rows, freq_bin=257)
        got = plan.average_rows(rows, freq_bin=256)
        assert got[0].shape == (1, 1, 3) and same(got, average_ref.average_rows(rows, None, 0, 256))


# -- bits -------------------------------------------------------------------------------------------------------------------------
def test_a_device_tensor_off_16_bytes_takes_the_narrow_loads(plan_mod, torch):
    """rows 8 bytes and weights 4 bytes past a 16-byte boundary, apart and together: the same bits as the aligned tensors'"""
    n_ant, nchan, n_chunks = 4, 64, 21
    rows, weights = cases(n_ant, nchan, n_chunks)[1]

    def shifted(a):
        flat = torch.empty(a.size + 1, dtype=torch.from_numpy(a).dtype, device="cuda")
        view = flat[1:].view(a.shape)
        view.copy_(torch.from_numpy(a))
        assert view.is_contiguous() and view.data_ptr() % 16 != 0 and flat.data_ptr() % 16 == 0
        return view

    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * 8) as plan:
        for time_bin, freq_bin in ((0, 1), (8, 4)):
            want = average_ref.average_rows(rows, weights, time_bin, freq_bin)
            rd, wd = torch.from_numpy(rows).cuda(), torch.from_numpy(weights).cuda()
            assert rd.data_ptr() % 16 == 0 and wd.data_ptr() % 8 == 0
            for r, w in ((rd, wd), (shifted(rows), wd), (rd, shifted(weights)), (shifted(rows), shifted(weights))):
                assert same(to_numpy(plan.average_rows(r, weights=w, time_bin=time_bin, freq_bin=freq_bin)), want)
            clean = cases(n_ant, nchan, n_chunks)[0][0]
            assert same(to_numpy(plan.average_rows(shifted(clean), time_bin=time_bin, freq_bin=freq_bin)),
                        average_ref.average_rows(clean, None, time_bin, freq_bin))


def test_outputs_do_not_depend_on_the_slabs(plan_mod, torch):
    """A workspace target of 1 and of 3 MiB (FXC_WS_MB is read once per process: a child for each setting) against the default here:
    host rows go through in slabs of a few baselines (228 KB of rows and weights a baseline at time_bin 0) -- the same bits, and the
    restatement's."""
    n_ant, nchan, n_chunks = 8, 1000, 19
    rows, weights = cases(n_ant, nchan, n_chunks)[1]
    settings = ((0, 1), (5, 7), (0, 8))
    code = ("import numpy as np, torch, sys; sys.path.insert(0, %r); from effex_amd import plan\n"
            "d = np.load(sys.argv[1]); rows, weights = d['rows'], d['weights']; out = {}\n"
            "rd, wd = torch.from_numpy(rows).cuda(), torch.from_numpy(weights).cuda()\n"
            "with plan.FxPlan(%d, %d, 4, %d) as p:\n"
            "    for t, f in %r:\n"
            "        for kind, r, w in (('h', rows, weights), ('d', rd, wd)):\n"
            "            v, s = p.average_rows(r, weights=w, time_bin=t, freq_bin=f)\n"
            "            out['v%%s%%d_%%d' %% (kind, t, f)] = v if kind == 'h' else v.cpu().numpy()\n"
            "            out['s%%s%%d_%%d' %% (kind, t, f)] = s if kind == 'h' else s.cpu().numpy()\n"
            "np.savez(sys.argv[2], **out)\n" % (ROOT, n_ant, nchan, nchan * 8, settings))
    with tempfile.TemporaryDirectory() as tmp:
        np.savez(os.path.join(tmp, "in.npz"), rows=rows, weights=weights)
        got = {}
        for label, ws_mb in (("one", "1"), ("three", "3")):
            env = dict(os.environ, FXC_WS_MB=ws_mb)
            res = os.path.join(tmp, label + ".npz")
            subprocess.run([sys.executable, "-c", code, os.path.join(tmp, "in.npz"), res], check=True, env=env, timeout=600)
            got[label] = dict(np.load(res))
    got["default"] = {}
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * 8) as plan:
        for t, f in settings:
            for kind, (v, s) in zip("hd", both_inputs(plan, torch, rows, weights, time_bin=t, freq_bin=f)):
                got["default"]["v%s%d_%d" % (kind, t, f)], got["default"]["s%s%d_%d" % (kind, t, f)] = v, s
    for t, f in settings:
        want = average_ref.average_rows(rows, weights, t, f)
        for label in ("default", "one", "three"):
            for kind in "hd":
                assert same((got[label]["v%s%d_%d" % (kind, t, f)], got[label]["s%s%d_%d" % (kind, t, f)]), want), (label, kind, t, f)


P_ANT, P_CHAN, P_CHUNKS = 4, 64, 24


def test_autos_and_the_tracks_change_nothing(plan_mod, torch):
    rows, weights = cases(P_ANT, P_CHAN, P_CHUNKS)[1]
    rng = np.random.default_rng(91)
    autos = (rng.standard_normal((P_CHUNKS, P_ANT, P_CHAN)) * 50).astype(np.complex64)
    wide = np.ascontiguousarray(np.concatenate([rows, autos], axis=1))
    want = average_ref.average_rows(rows, weights, 10, 4)
    with plan_mod.FxPlan(P_ANT, P_CHAN, 4, P_CHAN * 8, autos=True) as plan:
        assert plan.n_rows == plan.n_baselines + P_ANT
        for got in both_inputs(plan, torch, wide, weights, time_bin=10, freq_bin=4):
            assert got[0].shape == (3, plan.n_baselines, 16) and same(got, want)
        one = plan.average_rows(wide[3], weights=weights[3], freq_bin=4)                # 2-D rows: one chunk
        assert same(one, average_ref.average_rows(rows[3], weights[3], 0, 4)) and one[0].shape == (1, plan.n_baselines, 16)
    with plan_mod.FxPlan(P_ANT, P_CHAN, 4, P_CHAN * 8) as plan:
        plan.set_delay_track(np.linspace(0.0, 1e-7, P_ANT), np.zeros(P_ANT), BW, FC)
        plan.set_track_gains(np.full((2, P_ANT, P_CHAN), 1.5 - 0.5j), interval=4)
        plan.track_seek(5)
        keep_r, keep_w = rows.copy(), weights.copy()
        dev_r, dev_w = torch.from_numpy(rows).cuda(), torch.from_numpy(weights).cuda()
        for got in (plan.average_rows(rows, weights=weights, time_bin=10, freq_bin=4),
                    plan.average_rows(dev_r, weights=dev_w, time_bin=10, freq_bin=4)):
            assert same(to_numpy(got), want)
        assert plan.track_chunk == 5
        # the call leaves its inputs alone
        assert np.array_equal(bits(dev_r.cpu().numpy()), bits(keep_r)) and np.array_equal(bits(rows), bits(keep_r))
        assert np.array_equal(bits(dev_w.cpu().numpy()), bits(keep_w)) and np.array_equal(bits(weights), bits(keep_w))
        for bad in (dict(weights=dev_w), dict(weights=weights[:, :2]), dict(weights=weights[0])):
            with pytest.raises(ValueError):
                plan.average_rows(rows, **bad)
        with pytest.raises(ValueError):
            plan.average_rows(dev_r, weights=weights)
        with pytest.raises(ValueError):
            plan.average_rows(rows[:, :2])


def test_weights_times_four(plan_mod, torch):
    n_ant, nchan, n_chunks = 5, 63, 32
    rows, weights = cases(n_ant, nchan, n_chunks)[1]
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * 8) as plan:
        for time_bin, freq_bin in ((0, 1), (7, 4), (16, 64)):
            base = both_inputs(plan, torch, rows, weights, time_bin=time_bin, freq_bin=freq_bin)
            four = both_inputs(plan, torch, rows, weights * np.float32(4), time_bin=time_bin, freq_bin=freq_bin)
            for got, ref in zip(four, base):
                assert np.array_equal(bits(got[0]), bits(ref[0])) and np.array_equal(bits(got[1]), bits(ref[1] * np.float32(4)))
            assert same(base[0], average_ref.average_rows(rows, weights, time_bin, freq_bin))


# -- downstream ---------------------------------------------------------------------------------------------------------------------
def test_the_averaged_pair_feeds_the_weighted_gain_solve(plan_mod, torch):
    """rows g_a conj(g_b) + noise with antenna 1 dead, bin 5 flagged and 20 % of the samples flagged, averaged 8 chunks at a time at
    freq_bin 1: solve_gains(vis, weights=wsum) on the pair as it comes back -- numpy from host rows, CUDA tensors from device rows --
    agrees with the restatement's solve of the same arrays within the gain solve's ceiling"""
    n_ant, nchan, n_chunks = 8, 64, 24
    rng = np.random.default_rng(92)
    _, _, rows, weights = wref.damaged_case(n_ant, nchan, n_chunks, rng, sigma=0.1, with_model=False)
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * 8) as plan:
        for r, w in ((rows, weights), (torch.from_numpy(rows).cuda(), torch.from_numpy(weights).cuda())):
            vis, wsum = plan.average_rows(r, weights=w, time_bin=8)
            vis_np, wsum_np = to_numpy((vis, wsum))
            assert same((vis_np, wsum_np), average_ref.average_rows(rows, weights, 8, 1)) and vis_np.shape == (3, 28, nchan)
            for interval in (0, 1):
                g, step = plan.solve_gains(vis, interval=interval, ref=2, iters=60, weights=wsum)
                want_g, want_s = wref.solve_rows(vis_np, n_ant, interval=interval, ref=2, iters=60, weights=wsum_np)
                rel, dstep = np.abs(g - want_g).max() / np.abs(want_g).max(), np.abs(step - want_s).max()
                print("interval %d: gains %.3g step %.3g" % (interval, rel, dstep))
                assert rel <= CEIL_PARITY and dstep <= CEIL_PARITY
                assert (g[:, wref.DEAD_ANT] == 0).all() and (g[:, :, wref.DEAD_BIN] == 0).all()


# -- closure on the device ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", wref.DAMAGE_SEEDS)
def test_the_loop_closes_on_damaged_samples_without_leaving_the_device(plan_mod, torch, seed):
    """wref.damaged_samples(seed) through fx_rows, flag_rows and average_rows on the device rows: the figures of
    tests/test_average_host.py's closure, under the same bound, with the library's average in the restatement's place -- and the
    library's outputs are the restatement's on the same rows and weights"""
    rec = json.load(open(BOUNDS))
    x_np, _, w_truth = wref.damaged_samples(seed)
    nchan = gains_ref.SAMPLE_NCHAN
    tone = gains_ref.pairs(wref.DAMAGE_ANT).index(wref.DAMAGE_TONE_ANTS)
    with plan_mod.FxPlan(wref.DAMAGE_ANT, nchan, 4, x_np.shape[2], window=design_window(4, nchan)) as plan:
        rows = plan.fx_rows(torch.from_numpy(x_np).cuda())
        w_det = plan.flag_rows(rows)
        assert rows.is_cuda and w_det.is_cuda

        def average(r, w):
            return to_numpy(plan.average_rows(r, weights=w))

        cells, total, err, plain, tone_w = closure_of(rows, w_det, torch.from_numpy(w_truth).cuda(), average, tone)
        print("seed %d: %d of %d cells, detector-weighted %.4g, plain %.4g (B %.4g), tone weight %g" % (seed, cells, total, err, plain,
                                                                                                        rec["bound"], tone_w))
        assert total == 1792 and cells >= CELL_FLOOR * total
        assert err <= rec["bound"]
        assert plain >= 2.0 * rec["bound"]
        assert tone_w == 0
        assert same(average(rows, w_det), average_ref.average_rows(rows.cpu().numpy(), w_det.cpu().numpy()))


# -- arguments ---------------------------------------------------------------------------------------------------------------------
def test_average_rows_argument_checks(plan_mod, torch):
    from effex_amd import _lib
    n_ant, nchan, n = 3, 64, 7
    rng = np.random.default_rng(93)
    rows = noisy_rows(rng, n, 3, nchan)

    def call(plan, rows_ptr, n_chunks=n, kind=_lib.FXC_MEM_HOST, time_bin=0, freq_bin=1, out=True, sums=True):
        v, s = np.full((n, 3, nchan), -7.0 - 7.0j, np.complex64), np.full((n, 3, nchan), -7.0, np.float32)
        rc = plan._lib.fxc_average_rows(plan._h, rows_ptr, None, n_chunks, kind, time_bin, freq_bin, v.ctypes.data if out else None,
                                        s.ctypes.data if sums else None)
        if rc != 0:
            assert (v == -7.0 - 7.0j).all() and (s == -7.0).all(), "outputs written on an error"
        return rc

    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * 8) as plan:
        ptr = rows.ctypes.data
        for change in (dict(rows_ptr=None), dict(out=False), dict(n_chunks=0), dict(n_chunks=-3), dict(time_bin=-1), dict(freq_bin=0),
                       dict(freq_bin=-4), dict(kind=7)):
            args = dict(rows_ptr=ptr)
            args.update(change)
            rc = call(plan, **args)
            assert rc == _lib.FXC_ERR_ARG, change
            with pytest.raises(ValueError):
                _lib.check(rc, plan._h)
        assert call(plan, ptr, freq_bin=257) == _lib.FXC_ERR_UNSUPPORTED
        assert call(plan, ptr, freq_bin=0, kind=7) == _lib.FXC_ERR_ARG and call(plan, ptr, freq_bin=300, kind=7) == _lib.FXC_ERR_ARG
        assert call(plan, ptr) == 0 and call(plan, ptr, time_bin=3, freq_bin=5) == 0 and call(plan, ptr, time_bin=100, freq_bin=256) == 0
        assert call(plan, ptr, sums=False) == 0                                        # out_weights NULL
        v = np.zeros((1, 3, nchan), np.complex64)
        assert plan._lib.fxc_average_rows(plan._h, ptr, None, n, _lib.FXC_MEM_HOST, 0, 1, v.ctypes.data, None) == 0
        assert np.array_equal(bits(v), bits(average_ref.average_rows(rows)[0]))
        dev = torch.from_numpy(rows).cuda()
        dv = torch.zeros((1, 3, nchan), dtype=torch.complex64, device="cuda")
        assert plan._lib.fxc_average_rows(plan._h, dev.data_ptr(), None, n, _lib.FXC_MEM_DEVICE, 0, 1, dv.data_ptr(), None) == 0
        assert np.array_equal(bits(dv.cpu().numpy()), bits(v))
        for kwargs in (dict(time_bin=-1), dict(freq_bin=0), dict(freq_bin=-2)):
            with pytest.raises(ValueError):
                plan.average_rows(rows, **kwargs)
        with pytest.raises(ValueError):
            plan.average_rows(rows[:, :, :32])
    with plan_mod.FxPlan(1, nchan, 4, nchan * 8) as plan:                               # one antenna: no baseline
        one = np.ones((n, max(plan.n_rows, 1), nchan), np.complex64)
        v, s = np.full((1, 1, nchan), -7.0 - 7.0j, np.complex64), np.full((1, 1, nchan), -7.0, np.float32)
        rc = plan._lib.fxc_average_rows(plan._h, one.ctypes.data, None, n, _lib.FXC_MEM_HOST, 0, 1, v.ctypes.data, s.ctypes.data)
        assert rc == _lib.FXC_ERR_ARG and (v == -7.0 - 7.0j).all() and (s == -7.0).all()
