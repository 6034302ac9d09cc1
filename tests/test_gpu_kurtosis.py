"""Spectral kurtosis on the GPU (include/fxcorr.h fxc_kurtosis, fxc_kurtosis_weights; FxPlan.kurtosis, FxPlan.kurtosis_weights)
against the float64 restatement of its definition (kurtosis_ref.py).  Inputs: seeded noise with a flat spectrum plus, in one
antenna, a steady tone and a pulsed one at 30 times their bin's noise power -- no bin is near-empty beside a loud one, because sk
is a ratio of a bin's own sums while the spectra's float32 error scales with the loudest bin.  Every element of
every case is compared; every case runs on host and on device input and both must give the same bits.  Bounds: twice the largest
error tools/kurtosis_measure.py --parity observed on the MI355X (tests/golden/kurtosis_bounds.json, the convention of
tests/tolerances.py).  Also: the bits across calls and workspace targets, the weights against the numpy rule bit for bit, the
plan's untouched state, the chain into the rows tools, and the argument errors."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import kurtosis_ref as kr
from effex_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS = os.path.join(ROOT, "tests", "golden", "kurtosis_bounds.json")
BW, FC = 2.4e6, 1.4204e9
# ((n_ant, nchan, ntaps, n_pts, n_chunks), tints or None = 0, 2, 3 and n_pts): the small case (tint 3: bins of 3, 3 and 2 frames);
# part of a wave; an odd count and the fftshift (tint 2: the last bin a single frame); more than 8 antennas; the kernel per channel
# count (F only); the fused F-only route; the ring F route; the pre-filter pass; bins longer than any segment (1027 = 16 x 64 + 3:
# 17 segments, five rounds of four waves, a partial segment; 515 = 8 x 64 + 3 with a partial last bin of 512; 64: bins of one
# segment, a partial last bin of 3); the statistical input
SHAPES = [((2, 64, 4, 8, 3), None), ((3, 16, 4, 8, 2), None), ((3, 63, 4, 9, 2), None), ((9, 64, 4, 8, 2), None),
          ((5, 1000, 4, 8, 2), None), ((4, 4096, 4, 8, 2), None), ((2, 8192, 4, 8, 1), None), ((3, 64, 8, 8, 2), None),
          ((2, 64, 4, 1027, 2), (0, 515, 64)), (kr.STAT_SHAPE, None)]
LARGEST_M = 1027
ROUTES = {(5, 1000, 4, 8, 2): "generic", (4, 4096, 4, 8, 2): "fused", (2, 8192, 4, 8, 1): "tiled", (3, 64, 8, 8, 2): "tiled"}


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def plan_mod(torch):
    from effex_amd import plan
    return plan


@pytest.fixture(scope="module")
def parity_bounds():
    with open(BOUNDS) as fh:
        rec = json.load(fh)
    assert "parity" in rec, "tools/kurtosis_measure.py --parity has not written the parity bounds"
    return rec["parity"]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def tints_of(n_pts, tints):
    return (0, 2, 3, n_pts) if tints is None else tints


def shape_input(shape):
    """-> x complex64, window of a shape"""
    n_ant, nchan, ntaps, n_pts, n_chunks = shape
    x, window = kr.case(1000 * n_ant + nchan + n_pts, n_ant, nchan, ntaps, n_pts, n_chunks)
    return x.astype(np.complex64), window


def both_inputs(plan, torch, x, tint):
    """kurtosis with power on host and on device input; the bits must agree, and sk alone is the same sk; -> numpy sk, power"""
    sk, power = plan.kurtosis(x, tint=tint, return_power=True)
    assert isinstance(sk, np.ndarray) and isinstance(power, np.ndarray) and sk.dtype == power.dtype == np.float32
    d_sk, d_power = plan.kurtosis(torch.from_numpy(x).cuda(), tint=tint, return_power=True)
    assert d_sk.is_cuda and d_power.is_cuda and d_sk.dtype == d_power.dtype == torch.float32
    assert same_bits(sk, d_sk.cpu().numpy()) and same_bits(power, d_power.cpu().numpy()), "host and device input differ"
    assert same_bits(plan.kurtosis(x, tint=tint), sk)
    return sk, power


def shape_errors(plan_mod, torch, shape, tints=None, log=print):
    """-> {"sk tint": largest |sk - float64 sk|, "power tint": largest |power - float64 power| / max power, ..} of one shape"""
    n_ant, nchan, ntaps, n_pts, n_chunks = shape
    x, window = shape_input(shape)
    f = kr.spectra(x, nchan, window)          # the float64 reference, once per shape
    errs = {}
    with plan_mod.FxPlan(n_ant, nchan, ntaps, nchan * n_pts, window=window) as plan:
        for tint in tints_of(n_pts, tints):
            want_sk, want_power = kr.kurtosis_of_spectra(f, tint)
            sk, power = both_inputs(plan, torch, x, tint)
            assert sk.shape == power.shape == want_sk.shape == (n_chunks, n_ant, -(-n_pts // (tint or n_pts)), nchan)
            assert np.isfinite(sk).all() and np.isfinite(power).all()
            errs["sk %d" % tint] = float(np.abs(sk - want_sk).max())
            errs["power %d" % tint] = float(np.abs(power - want_power).max() / want_power.max())
        if tuple(shape) in ROUTES:
            assert plan.path == ROUTES[tuple(shape)], plan.path
        if nchan == 1000:
            assert plan.info["specialised"] & 2          # the F stage ran the build for this channel count
    log(shape, json.dumps(errs))
    return errs


# -- parity -----------------------------------------------------------------------------------------------------------------------
def test_the_recorded_bound_moves_no_three_sigma_decision(parity_bounds):
    """The sk bound stays below 1 % of the estimator's own standard deviation at the largest M of the shape list: rounding moves
    no 3-sigma decision.  (Were it not so, the combine would have to widen -- never the bound.)"""
    assert parity_bounds["largest_M"] == LARGEST_M == max(s[3] for s, _ in SHAPES)
    assert parity_bounds["sk_bound"] == pytest.approx(2.0 * parity_bounds["sk_observed"])
    assert parity_bounds["power_bound"] == pytest.approx(2.0 * parity_bounds["power_observed"])
    assert parity_bounds["sk_bound"] < 0.01 * np.sqrt(kr.mu2(LARGEST_M))


@pytest.mark.parametrize("shape,tints", SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) and len(v) == 5 else "")
def test_sk_and_power_match_the_restatement(plan_mod, torch, parity_bounds, shape, tints):
    errs = shape_errors(plan_mod, torch, shape, tints)
    for name, err in errs.items():
        assert err <= parity_bounds["sk_bound" if name.startswith("sk") else "power_bound"], (name, err)


def test_the_special_cases(plan_mod, torch):
    """a dead stream has sk 0 and power 0; a non-finite sample makes its bin's sk NaN and no other bin's; a bin of one frame holds
    1 exactly with its power written"""
    n_ant, nchan, n_pts = 3, 16, 9
    x, window = kr.case(5, n_ant, nchan, 4, n_pts, 2, with_tones=False)
    x = x.astype(np.complex64)
    x[0, 2] = 0.0                                     # antenna 2 of chunk 0 is dead
    x[1, 0, 5 * nchan + 3] = np.nan                   # frames 5 .. 8 of antenna 0, chunk 1 see it: the bins from frame 4 on at tint 2
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * n_pts, window=window) as plan:
        sk, power = both_inputs(plan, torch, x, 2)
        assert (sk[0, 2, :4] == 0.0).all() and (power[0, 2] == 0.0).all()
        assert (sk[:, :, 4] == 1.0).all()             # the ninth frame alone: 1 exactly, a NaN or a dead stream included
        assert np.isnan(sk[1, 0, 2:4]).all() and np.isfinite(sk[1, 0, :2]).all()
        assert np.isfinite(sk[1, 1:]).all() and np.isfinite(sk[0]).all()
        assert np.isfinite(power[:, 1, 4]).all() and (power[:, 1, 4] > 0).all()
        w = both_weights(plan, torch, sk, 2, lo=1e-3, hi=10.0)      # (at M = 2 the 3-sigma pair is wider than sk's range)
        assert (w[1, 0] == 0.0).all() and (w[1, 1] == 0.0).all() and (w[0, 1] == 0.0).all() and (w[0, 2] == 0.0).all()


def test_the_tones_are_flagged_on_the_device_as_on_the_host(plan_mod, torch):
    n_ant, nchan, ntaps, n_pts, n_chunks = kr.STAT_SHAPE
    x, window = shape_input(kr.STAT_SHAPE)
    from effex_amd.plan import sk_thresholds
    lo, hi = sk_thresholds(n_pts)
    k1, k2 = (kr.shifted(k, nchan) for k in kr.tone_bins(nchan))
    want = kr.weights(kr.kurtosis(x, nchan, window)[0], n_pts, 0, lo, hi)
    with plan_mod.FxPlan(n_ant, nchan, ntaps, nchan * n_pts, window=window) as plan:
        sk = plan.kurtosis(x)
        assert (sk[:, kr.HIT_ANT, 0, k1] < lo).all() and (sk[:, kr.HIT_ANT, 0, k2] > hi).all()
        w = plan.kurtosis_weights(sk)
        assert (w[:, 0, [k1, k2]] == 0.0).all()
        # a decision differs from the float64 one only where sk is within the parity bound of a threshold: nowhere here
        assert np.array_equal(w, want)


# -- bits ---------------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_bits_of_one(plan_mod, torch):
    shape = (3, 64, 4, 70, 5)
    x, window = shape_input(shape)
    with plan_mod.FxPlan(3, 64, 4, 64 * 70, window=window) as plan:
        for tint in (0, 3, 66):
            whole = both_inputs(plan, torch, x, tint)
            for put in (lambda a: a, lambda a: torch.from_numpy(a).cuda()):
                parts = [plan.kurtosis(put(x[:2]), tint=tint, return_power=True), plan.kurtosis(put(x[2:]), tint=tint, return_power=True)]
                for q in (0, 1):
                    got = np.concatenate([p[q] if isinstance(p[q], np.ndarray) else p[q].cpu().numpy() for p in parts])
                    assert same_bits(got, whole[q]), (tint, q)


def test_outputs_do_not_depend_on_the_workspace_target(plan_mod, torch):
    """A workspace target of 1 MiB (passes of 16 and 8 chunks) and of 3 MiB (FXC_WS_MB is read once per process: a child for each
    setting) against the default: the same bits, host and device input"""
    n_ant, nchan, n_pts, n_chunks = 8, 64, 16, 24
    x = kr.case(7, n_ant, nchan, 4, n_pts, n_chunks)[0].astype(np.complex64)
    code = ("import numpy as np, torch, sys; sys.path.insert(0, %r); from effex_amd import plan\n"
            "x = np.load(sys.argv[1])['x']; out = {}\n"
            "xd = torch.from_numpy(x).cuda()\n"
            "with plan.FxPlan(%d, %d, 4, %d) as p:\n"
            "    for kind, xx in (('h', x), ('d', xd)):\n"
            "        for tint in (0, 3):\n"
            "            sk, pw = p.kurtosis(xx, tint=tint, return_power=True)\n"
            "            out['%%ss%%d' %% (kind, tint)] = sk if kind == 'h' else sk.cpu().numpy()\n"
            "            out['%%sp%%d' %% (kind, tint)] = pw if kind == 'h' else pw.cpu().numpy()\n"
            "np.savez(sys.argv[2], **out)\n" % (ROOT, n_ant, nchan, nchan * n_pts))
    with tempfile.TemporaryDirectory() as tmp:
        np.savez(os.path.join(tmp, "in.npz"), x=x)
        got = {}
        for label, ws_mb in (("one", "1"), ("three", "3")):
            res = os.path.join(tmp, label + ".npz")
            subprocess.run([sys.executable, "-c", code, os.path.join(tmp, "in.npz"), res], check=True,
                           env=dict(os.environ, FXC_WS_MB=ws_mb), timeout=600)
            got[label] = dict(np.load(res))
    assert len(got["one"]) == len(got["three"]) == 8
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * n_pts) as plan:
        for tint in (0, 3):
            sk, power = plan.kurtosis(x, tint=tint, return_power=True)
            for label in ("one", "three"):
                for kind in "hd":
                    assert same_bits(got[label]["%ss%d" % (kind, tint)], sk), (label, kind, tint)
                    assert same_bits(got[label]["%sp%d" % (kind, tint)], power), (label, kind, tint)


# -- weights ------------------------------------------------------------------------------------------------------------------------
def both_weights(plan, torch, sk, tint, **kw):
    """kurtosis_weights on host and on device memory; both equal the numpy rule on the same float32 array, bit for bit"""
    from effex_amd.plan import sk_thresholds
    t_lo, t_hi = sk_thresholds(tint or plan.n_pts, kw.get("sigma", 3.0))
    lo = t_lo if kw.get("lo") is None else kw["lo"]
    hi = t_hi if kw.get("hi") is None else kw["hi"]
    want = kr.weights(sk, plan.n_pts, tint, lo, hi)
    w = plan.kurtosis_weights(sk, tint=tint, **kw)
    assert isinstance(w, np.ndarray) and w.dtype == np.float32 and same_bits(w, want)
    wd = plan.kurtosis_weights(torch.from_numpy(sk).cuda(), tint=tint, **kw)
    assert wd.is_cuda and wd.dtype == torch.float32 and same_bits(wd.cpu().numpy(), want)
    return w


@pytest.mark.parametrize("n_ant,nchan,n_pts,tint", [(2, 64, 64, 0), (3, 63, 9, 2), (9, 16, 70, 3), (4, 64, 1027, 515)])
def test_weights_equal_the_numpy_rule_bit_for_bit(plan_mod, torch, n_ant, nchan, n_pts, tint):
    x, window = kr.case(11 + n_ant, n_ant, nchan, 4, n_pts, 3)
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * n_pts, window=window) as plan:
        sk = plan.kurtosis(x.astype(np.complex64), tint=tint)
        both_weights(plan, torch, sk, tint)                                       # the default thresholds
        both_weights(plan, torch, sk, tint, sigma=1.0)
        lo, hi = float(np.float32(np.median(sk))), float(sk.max())                # a threshold that is one of the values: counted
        w = both_weights(plan, torch, sk, tint, lo=lo, hi=hi)
        assert w.mean() < 1.0                                                     # (half of the values lie below the median)
        both_weights(plan, torch, sk, tint, lo=0.9)                               # one given, one default
        planted = sk.copy()
        planted[1, n_ant - 1, 0, 5] = np.nan
        w_nan = both_weights(plan, torch, planted, tint, lo=-1e30, hi=1e30)
        want = np.ones_like(w_nan)
        want[1, [i for i, ab in enumerate(kr.pairs(n_ant)) if n_ant - 1 in ab], 5] = 0.0
        assert np.array_equal(w_nan, want)                                        # the NaN alone is flagged


# -- state ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ant,nchan,path", [(2, 4096, "fused"), (4, 64, None)])
def test_the_accumulator_is_untouched(plan_mod, torch, n_ant, nchan, path):
    """fx_accumulate, kurtosis, finalize equals fx_accumulate, finalize bit for bit: the call launches the pending fold (whose rows
    live in the workspace) before it writes the workspace, and adds nothing"""
    n_pts, n_chunks = 8, 6
    x = kr.case(31 + n_ant, n_ant, nchan, 4, n_pts, n_chunks)[0].astype(np.complex64)
    xd = torch.from_numpy(x).cuda()
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * n_pts, path=path) as plan:
        plan.fx_accumulate(xd)
        want = plan.finalize("SPECTRUM")
        ref = plan.kurtosis(xd).cpu().numpy()
        plan.fx_accumulate(xd)
        got_sk = plan.kurtosis(xd).cpu().numpy()
        got = plan.finalize("SPECTRUM")
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)) and np.abs(want).max() > 0
        assert same_bits(got_sk, ref)
        plan.fx_accumulate(x)                                             # host input: the staging path
        assert same_bits(plan.kurtosis(x), ref)
        assert np.array_equal(plan.finalize("SPECTRUM").view(np.uint64), want.view(np.uint64))


def test_a_delay_track_is_neither_applied_nor_moved(plan_mod, torch):
    n_ant, nchan, n_pts, n_chunks = 3, 64, 8, 4
    x = kr.case(41, n_ant, nchan, 4, n_pts, n_chunks)[0].astype(np.complex64)
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * n_pts) as plan:
        want = plan.kurtosis(x, tint=2, return_power=True)
        plan.set_delay_track(np.linspace(0.0, 2e-7, n_ant), np.linspace(1e-9, -1e-9, n_ant), BW, FC, first_chunk=5)
        assert plan.track_chunk == 5
        got = plan.kurtosis(x, tint=2, return_power=True)
        assert plan.track_chunk == 5
        got_d = plan.kurtosis(torch.from_numpy(x).cuda(), tint=2, return_power=True)
        assert plan.track_chunk == 5
        for q in (0, 1):
            assert same_bits(got[q], want[q]) and same_bits(got_d[q].cpu().numpy(), want[q])
        rows = plan.fx_rows(x)                                            # the track goes on from where it was
        assert plan.track_chunk == 5 + n_chunks
        plan.track_seek(5)
        plan.kurtosis(x)
        assert same_bits(plan.fx_rows(x).view(np.float32), rows.view(np.float32))


def test_sample_delays_are_not_applied(plan_mod, torch):
    n_ant, nchan, n_pts, n_chunks = 3, 64, 8, 3
    x = kr.case(43, n_ant, nchan, 4, n_pts, n_chunks)[0].astype(np.complex64)
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * n_pts) as plain, plan_mod.FxPlan(n_ant, nchan, 4, nchan * n_pts) as shifted:
        want = plain.kurtosis(x, tint=3, return_power=True)
        shifted.set_sample_delays([0, 5, 130])
        rows = shifted.fx_rows(x)
        assert not np.array_equal(rows, plain.fx_rows(x))                 # the shifts are in force
        got = shifted.kurtosis(x, tint=3, return_power=True)
        got_d = shifted.kurtosis(torch.from_numpy(x).cuda(), tint=3, return_power=True)
        for q in (0, 1):
            assert same_bits(got[q], want[q]) and same_bits(got_d[q].cpu().numpy(), want[q])
        assert same_bits(shifted.fx_rows(x).view(np.float32), rows.view(np.float32))


# -- chain ----------------------------------------------------------------------------------------------------------------------------
def test_the_weights_go_into_the_rows_tools(plan_mod, torch):
    n_ant, nchan, ntaps, n_pts, n_chunks = 3, 64, 4, 64, 4
    x, window = kr.case(51, n_ant, nchan, ntaps, n_pts, n_chunks)
    x = x.astype(np.complex64)
    k1, k2 = (kr.shifted(k, nchan) for k in kr.tone_bins(nchan))
    hit = [i for i, ab in enumerate(kr.pairs(n_ant)) if kr.HIT_ANT in ab]
    with plan_mod.FxPlan(n_ant, nchan, ntaps, nchan * n_pts, window=window) as plan:
        for put in (lambda a: a, lambda a: torch.from_numpy(a).cuda()):
            get = lambda a: a if isinstance(a, np.ndarray) else a.cpu().numpy()
            xx = put(x)
            w = plan.kurtosis_weights(plan.kurtosis(xx, tint=0))
            rows = plan.fx_rows(xx)
            assert tuple(w.shape) == (n_chunks, plan.n_baselines, nchan)
            assert (get(w)[:, hit][:, :, [k1, k2]] == 0.0).all()
            flagged = plan.flag_rows(rows, prior=w)
            assert tuple(flagged.shape) == tuple(w.shape) and (get(flagged)[get(w) == 0.0] == 0.0).all()
            gains, step = plan.solve_gains(rows, weights=w)
            assert gains.shape == (1, n_ant, nchan) and np.isfinite(gains).all()
            vis, wsum = plan.average_rows(rows, weights=w)
            wsum = get(wsum)
            assert (wsum[0][hit][:, [k1, k2]] == 0.0).all()
            assert np.array_equal(wsum[0], get(w).sum(axis=0))
            assert wsum[0].max() == n_chunks


# -- argument errors ----------------------------------------------------------------------------------------------------------------
def test_argument_errors(plan_mod, torch):
    n_ant, nchan, n_pts = 3, 16, 8
    x = kr.case(1, n_ant, nchan, 4, n_pts, 2)[0].astype(np.complex64)
    sk = np.full((2, n_ant, 1, nchan), -7.0, np.float32)
    power = np.full((2, n_ant, 1, nchan), -7.0, np.float32)
    wout = np.full((2, 3, nchan), -7.0, np.float32)
    H, D, A, U = _lib.FXC_MEM_HOST, _lib.FXC_MEM_DEVICE, _lib.FXC_ERR_ARG, _lib.FXC_ERR_UNSUPPORTED
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * n_pts) as plan:
        call, wcall = plan._lib.fxc_kurtosis, plan._lib.fxc_kurtosis_weights
        xp, sp, pp, wp = x.ctypes.data, sk.ctypes.data, power.ctypes.data, wout.ctypes.data
        assert call(None, xp, sp, pp, 2, H, 0) == A
        for args in ((None, sp, pp, 2, H, 0), (xp, None, pp, 2, H, 0),                                      # NULL
                     (xp, sp, pp, -1, H, 0),                                                                  # n_chunks < 0
                     (xp, sp, pp, 2, H, -1), (xp, sp, pp, 2, H, 1), (xp, sp, pp, 2, H, n_pts + 1),               # tint
                     (xp, sp, pp, 2, 3, 0), (xp, sp, pp, 2, -1, 0), (xp, sp, pp, 2, _lib.FXC_MEM_DEVICE_TO_PINNED, 0)):   # mem_kind
            assert call(plan._h, *args) == A, args
        assert call(plan._h, xp, sp, pp, 0, H, 0) == _lib.FXC_OK and call(plan._h, None, None, None, 0, D, 2) == _lib.FXC_OK
        assert wcall(None, sp, 2, 0, 0.5, 1.5, wp, H) == A
        for args in ((None, 2, 0, 0.5, 1.5, wp, H), (sp, 2, 0, 0.5, 1.5, None, H),                          # NULL
                     (sp, -1, 0, 0.5, 1.5, wp, H),                                                          # n_chunks < 0
                     (sp, 2, -1, 0.5, 1.5, wp, H), (sp, 2, 1, 0.5, 1.5, wp, H), (sp, 2, n_pts + 1, 0.5, 1.5, wp, H),   # tint
                     (sp, 2, 0, 0.5, 1.5, wp, 3), (sp, 2, 0, 0.5, 1.5, wp, _lib.FXC_MEM_DEVICE_TO_PINNED),   # mem_kind
                     (sp, 2, 0, float("nan"), 1.5, wp, H), (sp, 2, 0, 0.5, float("inf"), wp, H),
                     (sp, 2, 0, float("-inf"), 1.5, wp, H), (sp, 2, 0, 1.5, 0.5, wp, H)):                      # thresholds
            assert wcall(plan._h, *args) == A, args
        assert wcall(plan._h, sp, 0, 0, 0.5, 1.5, wp, H) == _lib.FXC_OK and wcall(plan._h, None, 0, 0, 0.5, 1.5, None, D) == _lib.FXC_OK
        assert (sk == -7.0).all() and (power == -7.0).all() and (wout == -7.0).all()          # a refused call writes nothing
        # right calls write everything; power may be NULL; lo == hi is a pair
        assert call(plan._h, xp, sp, None, 2, H, 0) == _lib.FXC_OK and (sk != -7.0).all() and (power == -7.0).all()
        assert call(plan._h, xp, sp, pp, 2, H, n_pts) == _lib.FXC_OK and (power > 0.0).all()
        assert wcall(plan._h, sp, 2, 0, 1.0, 1.0, wp, H) == _lib.FXC_OK and (wout == 0.0).all()
        # the Python layer
        for bad in (dict(tint=-1), dict(tint=1), dict(tint=n_pts + 1)):
            with pytest.raises(ValueError):
                plan.kurtosis(x, **bad)
            with pytest.raises(ValueError):
                plan.kurtosis_weights(sk, **bad)
        for lo, hi in ((float("nan"), 1.5), (0.5, float("inf")), (1.5, 0.5)):
            with pytest.raises(ValueError):
                plan.kurtosis_weights(sk, lo=lo, hi=hi)
        with pytest.raises(ValueError):
            plan.kurtosis(x[:, :2])
        with pytest.raises(ValueError):
            plan.kurtosis(x.astype(np.complex128).view(np.float64))
        with pytest.raises(ValueError):
            plan.kurtosis(torch.from_numpy(x.astype(np.complex128)).cuda())      # complex64 only
        xd = torch.from_numpy(x).cuda()
        for bad_sk in (sk[:, :2], sk[..., :8], sk[0], np.zeros((2, n_ant, 2, nchan), np.float32)):
            with pytest.raises(ValueError):
                plan.kurtosis_weights(bad_sk)
        with pytest.raises(ValueError):
            plan.kurtosis_weights(torch.from_numpy(sk).cuda().double())
        good = plan.kurtosis(x, tint=3, return_power=True)
        shape = (2, n_ant, 3, nchan)
        for bad_out in (np.empty((2, n_ant, 2, nchan), np.float32), np.empty(shape, np.float64),
                        torch.empty(shape, dtype=torch.float32, device="cuda"), (np.empty(shape, np.float32),) * 2):
            with pytest.raises(ValueError):
                plan.kurtosis(x, tint=3, out=bad_out)
        for bad_out in (np.empty(shape, np.float32), torch.empty(shape, dtype=torch.float64, device="cuda")):
            with pytest.raises(ValueError):
                plan.kurtosis(xd, tint=3, out=bad_out)
        with pytest.raises(ValueError):
            plan.kurtosis(x, tint=3, return_power=True, out=np.empty(shape, np.float32))
        # a right `out` receives the result
        o = np.empty(shape, np.float32)
        assert plan.kurtosis(x, tint=3, out=o) is o and same_bits(o, good[0])
        pair = (torch.empty(shape, dtype=torch.float32, device="cuda"), torch.empty(shape, dtype=torch.float32, device="cuda"))
        got = plan.kurtosis(xd, tint=3, return_power=True, out=pair)
        assert got[0] is pair[0] and got[1] is pair[1]
        assert same_bits(pair[0].cpu().numpy(), good[0]) and same_bits(pair[1].cpu().numpy(), good[1])
    # a chunk of one frame: unsupported, whatever the channel count
    for nchan1 in (1, 16):
        with plan_mod.FxPlan(2, nchan1, 4, nchan1) as short:
            one = np.zeros((1, 2, nchan1), np.complex64)
            out1 = np.full((1, 2, 1, nchan1), -7.0, np.float32)
            assert short._lib.fxc_kurtosis(short._h, one.ctypes.data, out1.ctypes.data, None, 1, H, 0) == U
            assert short._lib.fxc_kurtosis_weights(short._h, out1.ctypes.data, 1, 0, 0.5, 1.5, wout.ctypes.data, H) == U
            assert (out1 == -7.0).all()
            with pytest.raises(NotImplementedError):
                short.kurtosis(one)
