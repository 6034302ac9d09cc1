"""The detector on the GPU (include/fxcorr.h fxc_flag_rows, FxPlan.flag_rows) against the numpy restatement of its definition
(flag_ref.py).  Weights and counts must EQUAL the restatement's: every median is an element of its set, every other operation of
the definition is one float32 or exact float64 operation, so there is nothing to tolerate.  Seeded random rows go straight into
flag_rows (no F / X stage), with 15 % of the samples far off, a loud bin and a noisy bin, so that both stages fire.
Bits: no output depends on host against device input, on the workspace target, on auto rows behind the cross rows, and the call
leaves a delay track's counter alone.  Closure: the damaged samples of tests/test_gains_weighted_host.py through fx_rows,
flag_rows and solve_gains(weights=) without the weights leaving the device."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import flag_ref
import gains_ref
import gains_weighted_ref as wref
from effex_amd.window import design_window
from test_flag_host import noisy_rows, with_dead

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHTED_BOUNDS = os.path.join(ROOT, "tests", "golden", "gains_weighted_bounds.json")
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


def same(got, want):
    """weights bit for bit (+0.0f, not -0.0f) and counts"""
    return (got[0].dtype == np.float32 and got[0].shape == want[0].shape
            and np.array_equal(np.ascontiguousarray(got[0]).view(np.uint32), np.ascontiguousarray(want[0]).view(np.uint32))
            and got[1].dtype == np.int64 and np.array_equal(got[1], want[1]))


def both_inputs(plan, torch, rows, prior=None, **kw):
    """flag_rows(return_counts=True) on host and on device input, as numpy; the device result must be a CUDA tensor"""
    host = plan.flag_rows(rows, prior=prior, return_counts=True, **kw)
    assert isinstance(host[0], np.ndarray)
    dev = plan.flag_rows(torch.from_numpy(rows).cuda(), prior=None if prior is None else torch.from_numpy(prior).cuda(),
                         return_counts=True, **kw)
    assert dev[0].is_cuda and dev[0].dtype == torch.float32
    return host, (dev[0].cpu().numpy(), dev[1])


def n_base(n_ant):
    return n_ant * (n_ant - 1) // 2


# -- shapes -----------------------------------------------------------------------------------------------------------------------
# antennas x channels x chunks, windows: one baseline; a partial last window, one of 1 chunk (19 = 3 x 6 + 1) and of 3 (16 + 3);
# narrow loads; a partial last bin tile; 2016 baselines; nchan 1; the largest window; and windows of 100 and 200 chunks, at which a
# wave holds 4 and 2 columns (16 up to 32 chunks, 8 up to 64, 2 from 129 on)
SHAPES = [(2, 64, 32, (0,)), (3, 64, 19, (0, 5, 6, 16)), (5, 63, 32, (0,)), (8, 1000, 32, (0,)), (64, 64, 8, (0,)), (2, 1, 40, (0,)),
          (2, 16, 1024, (0,)), (3, 40, 100, (0,)), (2, 32, 200, (0,))]


@pytest.mark.parametrize("n_ant,nchan,n_chunks,windows", SHAPES)
def test_weights_and_counts_equal_the_restatement(plan_mod, torch, n_ant, nchan, n_chunks, windows):
    rng = np.random.default_rng(1000 * n_ant + nchan + n_chunks)
    rows = noisy_rows(rng, n_chunks, n_base(n_ant), nchan)
    if nchan > 12:
        rows = with_dead(rng, rows, share=0.02)[0]
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * 8) as plan:
        for window in windows:
            want = flag_ref.flag_rows(rows, window=window, return_counts=True)
            assert want[1][:, :, 1].sum() > 0 and (nchan == 1 or want[1][:, :, 2].sum() > 0)      # both stages fire
            assert 0.1 < (want[0] > 0).mean() < 1.0
            for got in both_inputs(plan, torch, rows, window=window):
                print(n_ant, nchan, n_chunks, window, "counts", got[1].sum(axis=(0, 1)), "differ", int((got[0] != want[0]).sum()))
                assert same(got, want), window


def test_a_window_of_1025_chunks_is_unsupported(plan_mod, torch):
    from effex_amd import _lib
    rows = np.ones((1025, 1, 16), np.complex64)
    weights = np.full((1025, 1, 16), -7.0, np.float32)
    counts = np.full((1, 1, 3), -7, np.int64)
    with plan_mod.FxPlan(2, 16, 4, 16 * 8) as plan:
        rc = plan._lib.fxc_flag_rows(plan._h, rows.ctypes.data, None, 1025, _lib.FXC_MEM_HOST, 0, 20.0, 8.0, 8, 2, weights.ctypes.data,
                                     counts.ctypes.data)
        assert rc == _lib.FXC_ERR_UNSUPPORTED
        assert (weights == -7.0).all() and (counts == -7).all()
        with pytest.raises(NotImplementedError):
            plan.flag_rows(rows)
        assert plan.flag_rows(rows, window=1024).shape == (1025, 1, 16)      # 1024 + 1: two windows


# -- parameters and inputs ----------------------------------------------------------------------------------------------------------
P_ANT, P_CHAN, P_CHUNKS = 4, 64, 24


@pytest.fixture(scope="module")
def param_rows():
    rng = np.random.default_rng(77)
    return with_dead(rng, noisy_rows(rng, P_CHUNKS, n_base(P_ANT), P_CHAN), share=0.05)[0]


@pytest.mark.parametrize("kw", [dict(half_width=0), dict(half_width=1), dict(half_width=8), dict(half_width=P_CHAN),
                                dict(half_width=1000), dict(iters=1), dict(iters=3), dict(iters=8),
                                dict(time_threshold=6.0, freq_threshold=3.0), dict(time_threshold=50.0, freq_threshold=20.5, window=7)],
                         ids=str)
def test_parameters_equal_the_restatement(plan_mod, torch, param_rows, kw):
    want = flag_ref.flag_rows(param_rows, return_counts=True, **kw)
    with plan_mod.FxPlan(P_ANT, P_CHAN, 4, P_CHAN * 8) as plan:
        for got in both_inputs(plan, torch, param_rows, **kw):
            assert same(got, want)


def test_ties_dead_columns_and_samples_that_are_not_numbers(plan_mod, torch):
    """rows quantised to a handful of values (medians tie, d == 0 occurs), a column and two whole bins entirely non-live, samples
    of NaN, Inf and exact zero, and 2-D rows"""
    rng = np.random.default_rng(78)
    nb = n_base(P_ANT)
    coarse = (np.round(rng.standard_normal((P_CHUNKS, nb, P_CHAN)) * 1.2) + 1j * np.round(rng.standard_normal((P_CHUNKS, nb, P_CHAN)) * 1.2))
    coarse[:, :, :16] = 1.0 + 1.0j                                # constant columns: d == 0
    coarse[::5, :, :16] = 3.0 - 2.0j                              # .. with a minority off the median: still d == 0
    coarse = coarse.astype(np.complex64)
    want = flag_ref.flag_rows(coarse, return_counts=True)
    assert (want[0][:, :, :16] == 1).all()
    odd = noisy_rows(rng, P_CHUNKS, nb, P_CHAN)
    odd[:, 1, 9] = 0                                               # a column
    odd[:, :, 20] = np.complex64(complex(np.nan, 1.0))             # a bin of NaN
    odd[:, :, 30] = 0                                              # a bin of zeros
    pick = rng.uniform(size=odd.shape)
    odd[pick < 0.03] = np.complex64(complex(np.inf, 0.5))
    odd[(pick >= 0.03) & (pick < 0.06)] = np.complex64(complex(1.0, -np.inf))
    odd[(pick >= 0.06) & (pick < 0.09)] = np.complex64(complex(0.25, np.nan))
    odd[(pick >= 0.09) & (pick < 0.12)] = 0
    want_odd = flag_ref.flag_rows(odd, return_counts=True)
    assert (want_odd[0][:, :, 20] == 0).all() and (want_odd[0][:, :, 30] == 0).all() and (want_odd[0] > 0).any()
    with plan_mod.FxPlan(P_ANT, P_CHAN, 4, P_CHAN * 8) as plan:
        for got in both_inputs(plan, torch, coarse):
            assert same(got, want)
        for got in both_inputs(plan, torch, odd):
            assert same(got, want_odd)
        one = plan.flag_rows(odd[3], return_counts=True)
        assert same(one, flag_ref.flag_rows(odd[3], return_counts=True)) and one[0].shape == (nb, P_CHAN)
        assert plan.flag_rows(torch.from_numpy(odd[3]).cuda()).shape == (nb, P_CHAN)


def test_a_prior(plan_mod, torch, param_rows):
    rng = np.random.default_rng(79)
    prior = rng.uniform(0.25, 4.0, param_rows.shape).astype(np.float32)
    off = rng.uniform(size=prior.shape) < 0.1
    prior[off] = np.where(rng.uniform(size=int(off.sum())) < 0.5, 0.0, -1.0).astype(np.float32)
    prior[0, 0, 0] = np.nan
    poisoned = param_rows.copy()
    poisoned[off] = np.complex64(complex(np.nan, 1e30))            # what the prior flags is never looked at
    want = flag_ref.flag_rows(param_rows, prior=prior, window=10, return_counts=True)
    with plan_mod.FxPlan(P_ANT, P_CHAN, 4, P_CHAN * 8) as plan:
        for rows in (param_rows, poisoned):
            for got in both_inputs(plan, torch, rows, prior=prior, window=10):
                assert same(got, want)
        ones = plan.flag_rows(param_rows, prior=np.ones(param_rows.shape, np.float32), return_counts=True)
        assert same(ones, plan.flag_rows(param_rows, return_counts=True))
        for bad in (dict(prior=torch.from_numpy(prior).cuda()), dict(prior=prior[:, :2]), dict(prior=prior[0])):
            with pytest.raises(ValueError):
                plan.flag_rows(param_rows, **bad)
        with pytest.raises(ValueError):
            plan.flag_rows(torch.from_numpy(param_rows).cuda(), prior=prior)
        with pytest.raises(ValueError):
            plan.flag_rows(param_rows[:, :2])


# -- bits -------------------------------------------------------------------------------------------------------------------------
def test_outputs_do_not_depend_on_the_slabs(plan_mod, torch):
    """A workspace target of 1 and of 3 MiB (FXC_WS_MB is read once per process: a child for each setting) against the default here:
    host rows go through in slabs of a few baselines, device rows window by window -- the same bits, and the restatement's."""
    n_ant, nchan, n_chunks = 8, 1000, 19
    rng = np.random.default_rng(80)
    rows = noisy_rows(rng, n_chunks, n_base(n_ant), nchan)          # 152 KB of rows a baseline and window, 8 KB of planes
    prior = rng.uniform(0.5, 2.0, rows.shape).astype(np.float32)
    code = ("import numpy as np, torch, sys; sys.path.insert(0, %r); from effex_amd import plan\n"
            "d = np.load(sys.argv[1]); rows, prior = d['rows'], d['prior']; out = {}\n"
            "rd, pd = torch.from_numpy(rows).cuda(), torch.from_numpy(prior).cuda()\n"
            "with plan.FxPlan(%d, %d, 4, %d) as p:\n"
            "    for window in (0, 5):\n"
            "        for kind, r, q in (('h', rows, prior), ('d', rd, pd)):\n"
            "            w, c = p.flag_rows(r, window=window, prior=q, return_counts=True)\n"
            "            out['w%%s%%d' %% (kind, window)] = w if kind == 'h' else w.cpu().numpy(); out['c%%s%%d' %% (kind, window)] = c\n"
            "np.savez(sys.argv[2], **out)\n" % (ROOT, n_ant, nchan, nchan * 8))
    with tempfile.TemporaryDirectory() as tmp:
        np.savez(os.path.join(tmp, "in.npz"), rows=rows, prior=prior)
        got = {}
        for label, ws_mb in (("one", "1"), ("three", "3")):
            env = dict(os.environ, FXC_WS_MB=ws_mb)
            res = os.path.join(tmp, label + ".npz")
            subprocess.run([sys.executable, "-c", code, os.path.join(tmp, "in.npz"), res], check=True, env=env, timeout=600)
            got[label] = dict(np.load(res))
    got["default"] = {}
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * 8) as plan:
        for window in (0, 5):
            for kind, (w, c) in zip("hd", both_inputs(plan, torch, rows, prior=prior, window=window)):
                got["default"]["w%s%d" % (kind, window)], got["default"]["c%s%d" % (kind, window)] = w, c
    for window in (0, 5):
        want = flag_ref.flag_rows(rows, window=window, prior=prior, return_counts=True)
        for label in ("default", "one", "three"):
            for kind in "hd":
                assert same((got[label]["w%s%d" % (kind, window)], got[label]["c%s%d" % (kind, window)]), want), (label, kind, window)


def test_autos_and_a_delay_track_change_nothing(plan_mod, torch, param_rows):
    rng = np.random.default_rng(81)
    autos = (rng.standard_normal((P_CHUNKS, P_ANT, P_CHAN)) * 50).astype(np.complex64)
    wide = np.ascontiguousarray(np.concatenate([param_rows, autos], axis=1))
    want = flag_ref.flag_rows(param_rows, window=10, return_counts=True)
    with plan_mod.FxPlan(P_ANT, P_CHAN, 4, P_CHAN * 8, autos=True) as plan:
        assert plan.n_rows == plan.n_baselines + P_ANT
        for got in both_inputs(plan, torch, wide, window=10):
            assert same(got, want)
    with plan_mod.FxPlan(P_ANT, P_CHAN, 4, P_CHAN * 8) as plan:
        plan.set_delay_track(np.linspace(0.0, 1e-7, P_ANT), np.zeros(P_ANT), BW, FC)
        plan.track_seek(5)
        keep = param_rows.copy()
        dev = torch.from_numpy(param_rows).cuda()
        for got in (plan.flag_rows(param_rows, window=10, return_counts=True), plan.flag_rows(dev, window=10, return_counts=True)):
            got = (got[0] if isinstance(got[0], np.ndarray) else got[0].cpu().numpy(), got[1])
            assert same(got, want)
        assert plan.track_chunk == 5
        # the call leaves its inputs alone
        assert np.array_equal(dev.cpu().numpy().view(np.uint64), keep.view(np.uint64)) and np.array_equal(param_rows.view(np.uint64),
                                                                                                           keep.view(np.uint64))


# -- closure on the device ----------------------------------------------------------------------------------------------------------
def test_the_loop_closes_on_damaged_samples_without_leaving_the_device(plan_mod, torch):
    """wref.damaged_samples(0) through fx_rows, flag_rows on the device rows, solve_gains(weights=w) with w a CUDA tensor: the
    weights are the restatement's on the same rows and the ratios lie within the bound of the weighted solve's own test"""
    bound = json.load(open(WEIGHTED_BOUNDS))["bound"]
    x_np, c, _ = wref.damaged_samples(0)
    nchan = gains_ref.SAMPLE_NCHAN
    with plan_mod.FxPlan(wref.DAMAGE_ANT, nchan, 4, x_np.shape[2], window=design_window(4, nchan)) as plan:
        rows = plan.fx_rows(torch.from_numpy(x_np).cuda())
        w, counts = plan.flag_rows(rows, return_counts=True)
        assert w.is_cuda and w.dtype == torch.float32
        assert same((w.cpu().numpy(), counts), flag_ref.flag_rows(rows.cpu().numpy(), return_counts=True))
        for ref in wref.DAMAGE_REFS:
            g, _ = plan.solve_gains(rows, ref=ref, iters=gains_ref.SAMPLE_ITERS, weights=w)
            err = float(np.abs(wref.scalar_ratios(g[0], ref) - gains_ref.true_ratios(c, ref)).max())
            print("ref %d: %.3g (bound %.3g)" % (ref, err, bound))
            assert err <= bound


# -- arguments ---------------------------------------------------------------------------------------------------------------------
def test_flag_rows_argument_checks(plan_mod, torch):
    from effex_amd import _lib
    n_ant, nchan, n = 3, 64, 7
    rng = np.random.default_rng(82)
    rows = noisy_rows(rng, n, 3, nchan)

    def call(plan, rows_ptr, n_chunks=n, kind=_lib.FXC_MEM_HOST, window=0, tt=20.0, ft=8.0, half_width=8, iters=2, out=True):
        w, k = np.full((n, 3, nchan), -7.0, np.float32), np.full((n, 3, 3), -7, np.int64)
        rc = plan._lib.fxc_flag_rows(plan._h, rows_ptr, None, n_chunks, kind, window, tt, ft, half_width, iters,
                                     w.ctypes.data if out else None, k.ctypes.data)
        if rc != 0:
            assert (w == -7.0).all() and (k == -7).all(), "outputs written on an error"
        return rc

    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * 8) as plan:
        ptr = rows.ctypes.data
        for change in (dict(rows_ptr=None), dict(out=False), dict(n_chunks=0), dict(n_chunks=-3), dict(window=-1), dict(tt=0.0),
                       dict(tt=-1.0), dict(tt=float("nan")), dict(tt=float("inf")), dict(ft=0.0), dict(ft=-2.0), dict(ft=float("nan")),
                       dict(ft=float("inf")), dict(half_width=-1), dict(iters=0), dict(iters=-1), dict(iters=9), dict(kind=7)):
            args = dict(rows_ptr=ptr)
            args.update(change)
            rc = call(plan, **args)
            assert rc == _lib.FXC_ERR_ARG, change
            with pytest.raises(ValueError):
                _lib.check(rc, plan._h)
        assert call(plan, ptr) == 0 and call(plan, ptr, window=3, iters=8, half_width=0) == 0
        w = np.zeros((n, 3, nchan), np.float32)
        assert plan._lib.fxc_flag_rows(plan._h, ptr, None, n, _lib.FXC_MEM_HOST, 0, 20.0, 8.0, 8, 2, w.ctypes.data, None) == 0   # counts NULL
        assert np.array_equal(w, flag_ref.flag_rows(rows))
        for kwargs in (dict(iters=0), dict(window=-1), dict(time_threshold=0.0), dict(freq_threshold=float("nan")), dict(half_width=-1)):
            with pytest.raises(ValueError):
                plan.flag_rows(rows, **kwargs)
        with pytest.raises(ValueError):
            plan.flag_rows(rows[:, :, :32])
