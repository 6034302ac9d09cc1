"""Weighted fringe fit on the GPU (include/fxcorr.h fxc_fringe_fit_weighted, FxPlan.fringe_fit(weights=, baselines=)) against the
float64 restatement of its definition (fringe_weighted_ref.py) and against the plain call.

Same bits: with weights of 1, or none, the baselines-to-ref mode is fxc_fringe_fit.  Parity: every baseline's peak cell is the
restatement's, and the sub-cell parts differ by the float32 rounding of the transforms; tests/golden/fringe_weighted_bounds.json
holds the largest |gpu - float64| of the baselines' delays and rates in grid cells and of their snr (relative) over the cases of
this module on an MI355X, and the largest difference in cells between the library's antenna solution and the restatement's from
the library's own baselines (tools/fringe_weighted_measure.py writes it); the tests hold to twice those, under the ceilings 0.05
cell and 1e-5 (baselines) and 1e-6 cell (antennas).  Closure: samples with injected delays and rates and a run of lost chunks,
fitted over all baselines and fed back as a track, against the same samples under the injected truth;
profiles/fringe_weighted/closure.json holds the measured coherence ratio, the test holds to it less 0.01."""
import functools
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import fringe_ref
import fringe_weighted_ref as fw
from effex_amd.window import design_window
from fringe_ref import BW, FC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS = os.path.join(ROOT, "tests", "golden", "fringe_weighted_bounds.json")
CLOSURE_FILE = os.path.join(ROOT, "profiles", "fringe_weighted", "closure.json")
CEIL_CELL = 0.05        # beyond this the interpolation adds more error than the estimator has
CEIL_SNR = 1e-5         # TOL_VIS
CEIL_ANT = 1e-6         # the antenna solution is float64 on both sides


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def plan_mod(torch):
    from effex_amd import plan
    return plan


def recorded(path):
    with open(path) as f:
        return json.load(f)


def as_bits(arrays):
    return [np.ascontiguousarray(a, dtype=np.float64).view(np.uint64) for a in arrays]


def assert_same_bits(got, want, what):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(as_bits(got), as_bits(want))):
        assert np.array_equal(g, w), (what, k)


def model_rows(n_ant, nchan, n_chunks, seed):
    """the rows of test_gpu_fringe.py's parity cases: residuals within 0.4 of the ranges, snr_in 1"""
    rng = np.random.default_rng(seed)
    delays, rates = fringe_ref.draw_antennas(n_ant, nchan, rng)
    return fringe_ref.model_rows(n_chunks, n_ant, nchan, delays, rates, 1.0, rng)


# -- the same bits as the plain call -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nchan,n_chunks", [(64, 48), (1000, 40)])
def test_unit_weights_and_no_weights_are_the_plain_call(plan_mod, torch, nchan, n_chunks):
    n_ant = 3
    rows = model_rows(n_ant, nchan, n_chunks, 100 * n_ant + nchan)
    ones = np.ones((n_chunks, 3, nchan), np.float32)
    pairs = fringe_ref.pairs(n_ant)
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * 8) as plan:
        for ref in (0, 1):                            # ref 1: antenna 0 comes from the conjugate of row (0, 1)
            for kind in ("host", "device"):
                data, w = (rows, ones) if kind == "host" else (torch.from_numpy(rows).cuda(), torch.from_numpy(ones).cuda())
                want = plan.fringe_fit(data, BW, FC, ref=ref, pad=2)
                assert np.all(want[2][np.arange(n_ant) != ref] > 10.0)
                assert_same_bits(plan.fringe_fit(data, BW, FC, ref=ref, pad=2, weights=w), want, (ref, kind, "ones"))
                got = plan.fringe_fit(data, BW, FC, ref=ref, pad=2, weights=None, return_baselines=True)
                assert_same_bits(got[:3], want, (ref, kind, "none"))
                base = got[3]
                assert base.shape == (3, 3) and base.dtype == np.float64
                for i, (a, b) in enumerate(pairs):
                    if ref == a:
                        assert_same_bits([base[i]], [[want[0][b], want[1][b], want[2][b]]], (ref, kind, i))
                    elif ref == b:                    # as the row reads: D_b - D_a, the negative of antenna a against b
                        assert_same_bits([base[i]], [[-want[0][a], -want[1][a], want[2][a]]], (ref, kind, i))
                    else:
                        assert_same_bits([base[i]], [[0.0, 0.0, 0.0]], (ref, kind, i))


# -- parity of the baselines and the antenna solution, all baselines -------------------------------------------------------------
ALL_CASES = {"2x64": (2, 64, 48), "damaged": (6, 64, 32), "5x1000": (5, 1000, 40)}


@functools.lru_cache(maxsize=None)
def all_rows(name):
    """-> rows, weights (None: the call without weights)"""
    n_ant, nchan, n_chunks = ALL_CASES[name]
    if name == "damaged":
        return fw.damaged_rows()
    rows = model_rows(n_ant, nchan, n_chunks, 100 * n_ant + nchan)
    if name == "2x64":
        return rows, None
    rng = np.random.default_rng(77)
    weights = (rng.random((n_chunks, n_ant * (n_ant - 1) // 2, nchan)) < 0.8).astype(np.float32)
    rows[weights == 0] = np.nan + 1j * np.nan
    return rows, weights


@functools.lru_cache(maxsize=None)
def all_restated(name, pad):
    n_ant = ALL_CASES[name][0]
    rows, weights = all_rows(name)
    return fw.fit_rows_weighted(rows, weights, n_ant, BW, FC, ref=0, pad=pad, baselines="all")


def period_diff(x, y, period):
    e = np.asarray(x) - np.asarray(y)
    return e - period * np.rint(e / period)


def all_case(plan_mod, torch, name):
    """-> per pad: the peaks agree, host and device input give the same bits (both asserted here), and the figures: baselines
    against the restatement (delay, rate in cells, snr relative), antennas against the restatement's solve of the library's
    baselines (cells); the library's outputs of the last pad for further checks"""
    n_ant, nchan, n_chunks = ALL_CASES[name]
    rows, weights = all_rows(name)
    figures, got = [], None
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * 8) as plan:
        for pad in (1, 2):
            want_d, want_r, want_s, want_base, peaks = all_restated(name, pad)
            cd, cr = fringe_ref.cells(nchan, n_chunks, pad)
            lk, lt = fringe_ref.grid(nchan, n_chunks, pad)
            got = plan.fringe_fit(rows, BW, FC, pad=pad, weights=weights, baselines="all", return_baselines=True)
            dev = plan.fringe_fit(torch.from_numpy(rows).cuda(), BW, FC, pad=pad, baselines="all", return_baselines=True,
                                  weights=None if weights is None else torch.from_numpy(weights).cuda())
            assert_same_bits(dev, got, (name, pad, "host against device"))
            d, r, s, base = got
            assert base.shape == (n_ant * (n_ant - 1) // 2, 3) and d[0] == 0.0 and r[0] == 0.0 and s[0] == 0.0
            fitted = []
            for i, peak in peaks.items():
                if peak is None:                      # nothing counted
                    assert not base[i].any(), (name, pad, i)
                    continue
                q0, m0 = peak
                em = (base[i, 0] / cd - m0 + lk // 2) % lk - lk // 2
                eq = (base[i, 1] / cr - q0 + lt // 2) % lt - lt // 2
                assert abs(em) <= 0.5 + CEIL_CELL and abs(eq) <= 0.5 + CEIL_CELL, (name, pad, i, q0, m0, em, eq)
                fitted.append(i)
            sol_d, sol_r, sol_s, _ = fw.solve_antennas(base, n_ant, 0, nchan, n_chunks, pad, BW, FC)
            ant = max(np.abs(period_diff(d, sol_d, nchan / BW)).max() / cd, np.abs(period_diff(r, sol_r, 1.0 / FC)).max() / cr)
            assert np.array_equal(s == 0.0, sol_s == 0.0) and np.allclose(s, sol_s, rtol=1e-12, atol=0.0)
            figures.append({"case": name, "pad": pad,
                            "delay_cells": float(np.abs(base[fitted, 0] - want_base[fitted, 0]).max() / cd),
                            "rate_cells": float(np.abs(base[fitted, 1] - want_base[fitted, 1]).max() / cr),
                            "snr_rel": float(np.abs(base[fitted, 2] / want_base[fitted, 2] - 1.0).max()),
                            "antenna_cells": float(ant)})
    return figures, got


@pytest.mark.parametrize("name", sorted(ALL_CASES))
def test_all_baselines_match_the_restatement(plan_mod, torch, name):
    rec = recorded(BOUNDS)
    bound = {"delay_cells": min(2.0 * rec["delay_cells"], CEIL_CELL), "rate_cells": min(2.0 * rec["rate_cells"], CEIL_CELL),
             "snr_rel": min(2.0 * rec["snr_rel"], CEIL_SNR), "antenna_cells": min(2.0 * rec["antenna_cells"], CEIL_ANT)}
    figures, got = all_case(plan_mod, torch, name)
    for f in figures:
        print(json.dumps(f))
    for f in figures:
        for key, b in bound.items():
            assert f[key] <= b, (f, bound)
    if name != "damaged":
        return
    # the damaged fixture (pad 2): the four live antennas near the truth, the dead one exactly 0
    c = fw.DAMAGED
    d, r, s, base = got
    cd, cr = fringe_ref.cells(c["nchan"], c["n_chunks"], 2)
    live = [1, 2, 3, 5]
    ed = period_diff(d, fw.DAMAGED_D, c["nchan"] / BW) / cd
    er = period_diff(r, fw.DAMAGED_R, 1.0 / FC) / cr
    assert np.abs(ed[live]).max() < 0.1 and np.abs(er[live]).max() < 0.1, (ed, er)
    assert d[4] == 0.0 and r[4] == 0.0 and s[4] == 0.0 and (s[live] > 40.0).all()


def test_baselines_to_ref_lose_what_all_baselines_keep(plan_mod, torch):
    """the damaged fixture through the baselines to ref alone: antenna 3, whose baseline to ref is lost, cannot be measured"""
    rows, weights = fw.damaged_rows()
    with plan_mod.FxPlan(6, 64, 4, 64 * 8) as plan:
        d, r, s, base = plan.fringe_fit(rows, BW, FC, weights=weights, return_baselines=True)
    assert d[3] == 0.0 and r[3] == 0.0 and s[3] == 0.0 and not base[fringe_ref.pairs(6).index((0, 3))].any()
    assert np.isfinite(d).all() and np.isfinite(r).all() and (s[[1, 2, 5]] > 25.0).all() and 0.0 < s[4] < 4.0


# -- flagged values are never used ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("baselines", ["ref", "all"])
def test_flagged_values_and_the_scale_of_the_weights_change_no_bit(plan_mod, torch, baselines):
    rows, weights = fw.damaged_rows()
    clean = fw.zeroed(rows, weights)
    with plan_mod.FxPlan(6, 64, 4, 64 * 8) as plan:
        want = plan.fringe_fit(clean, BW, FC, weights=weights, baselines=baselines, return_baselines=True)
        assert all(np.isfinite(a).all() for a in want)
        for kind in ("host", "device"):
            data, w = (rows, weights) if kind == "host" else (torch.from_numpy(rows).cuda(), torch.from_numpy(weights).cuda())
            assert_same_bits(plan.fringe_fit(data, BW, FC, weights=w, baselines=baselines, return_baselines=True), want, (kind, "flagged"))
            assert_same_bits(plan.fringe_fit(data, BW, FC, weights=w * 4.0, baselines=baselines, return_baselines=True), want, (kind, "x 4"))
        odd = weights.copy()                          # negative and NaN weights leave a sample out like 0
        odd[5:7] = -1.0
        odd[7:9] = np.nan
        assert_same_bits(plan.fringe_fit(rows, BW, FC, weights=odd, baselines=baselines, return_baselines=True), want, "odd weights")


# -- batches --------------------------------------------------------------------------------------------------------------------
def test_a_second_batch_fits_its_rows_like_the_first(plan_mod, torch):
    """12 antennas are 66 baselines: a batch of the fixed 64 and one of 2.  A value depends on its baseline's rows alone, so row i
    of the 66 gives the bits it gives as the one baseline of a two-antenna plan."""
    n_ant, nchan, n_chunks = 12, 16, 16
    rows = model_rows(n_ant, nchan, n_chunks, 1216)
    rng = np.random.default_rng(12)
    weights = (rng.random((n_chunks, 66, nchan)) < 0.9).astype(np.float32) * 2.0
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * 8) as plan:
        host = plan.fringe_fit(rows, BW, FC, pad=2, weights=weights, baselines="all", return_baselines=True)
        dev = plan.fringe_fit(torch.from_numpy(rows).cuda(), BW, FC, pad=2, weights=torch.from_numpy(weights).cuda(), baselines="all",
                              return_baselines=True)
    assert_same_bits(dev, host, "host against device")
    assert host[3].shape == (66, 3) and (host[3][:, 2] > 0.0).all()
    with plan_mod.FxPlan(2, nchan, 4, nchan * 8) as one:
        for i in (0, 63, 64, 65):
            single = one.fringe_fit(np.ascontiguousarray(rows[:, i:i + 1]), BW, FC, pad=2, baselines="all", return_baselines=True,
                                    weights=np.ascontiguousarray(weights[:, i:i + 1]))
            assert_same_bits([single[3][0]], [host[3][i]], i)


def test_outputs_do_not_depend_on_the_batches(plan_mod, torch):
    """10 baselines of 40 chunks at Lk 2048 take 1.25 MiB of transform buffers each: this process, with the default workspace
    target, fits them in one batch; a child whose target of 4 MiB holds fewer than 10 (FXC_WS_MB is read once per process)
    takes several.  The same bits, host and device input, both modes."""
    n_ant, nchan, n_chunks = ALL_CASES["5x1000"]
    rows, weights = all_rows("5x1000")
    code = ("import numpy as np, torch, sys; sys.path.insert(0, %r); from effex_amd import plan\n"
            "rows, w = np.load(sys.argv[1]), np.load(sys.argv[2]); out = {}\n"
            "with plan.FxPlan(%d, %d, 4, %d) as p:\n"
            "    for mode in ('ref', 'all'):\n"
            "        for kind, data, wt in (('h', rows, w), ('d', torch.from_numpy(rows).cuda(), torch.from_numpy(w).cuda())):\n"
            "            res = p.fringe_fit(data, %r, %r, ref=2, pad=2, weights=wt, baselines=mode, return_baselines=True)\n"
            "            out[kind + mode] = np.concatenate([np.ravel(a) for a in res])\n"
            "np.savez(sys.argv[3], **out)\n" % (ROOT, n_ant, nchan, nchan * 8, BW, FC))
    want = {}
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * 8) as plan:
        for mode in ("ref", "all"):
            for kind, data, wt in (("h", rows, weights), ("d", torch.from_numpy(rows).cuda(), torch.from_numpy(weights).cuda())):
                res = plan.fringe_fit(data, BW, FC, ref=2, pad=2, weights=wt, baselines=mode, return_baselines=True)
                want[kind + mode] = np.concatenate([np.ravel(a) for a in res])
    with tempfile.TemporaryDirectory() as tmp:
        np.save(os.path.join(tmp, "rows.npy"), rows)
        np.save(os.path.join(tmp, "w.npy"), weights)
        res = os.path.join(tmp, "small.npz")
        subprocess.run([sys.executable, "-c", code, os.path.join(tmp, "rows.npy"), os.path.join(tmp, "w.npy"), res], check=True,
                       env=dict(os.environ, FXC_WS_MB="4"), timeout=600)
        small = dict(np.load(res))
    assert sorted(small) == sorted(want)
    for key, w in want.items():
        assert np.isfinite(w).all() and np.array_equal(small[key].view(np.uint64), w.view(np.uint64)), key


# -- arguments ------------------------------------------------------------------------------------------------------------------
def test_weighted_fit_argument_checks(plan_mod, torch):
    from effex_amd import _lib
    n_ant, nchan, n_chunks = 3, 64, 48
    rows = model_rows(n_ant, nchan, n_chunks, 364)
    ones = np.ones((n_chunks, 3, nchan), np.float32)
    nan, inf = float("nan"), float("inf")

    def call(plan, rows_ptr, n_chunks, bw, fc, ref, pad, mode=_lib.FXC_FRINGE_ALL, min_snr=0.0, d=True, r=True, kind=_lib.FXC_MEM_HOST):
        out = [np.full(plan.n_ant, -7.0) for _ in range(3)] + [np.full((plan.n_baselines, 3), -7.0)]
        rc = plan._lib.fxc_fringe_fit_weighted(plan._h, rows_ptr, ones.ctypes.data, n_chunks, kind, bw, fc, ref, pad, mode, min_snr,
                                               out[0].ctypes.data if d else None, out[1].ctypes.data if r else None,
                                               out[2].ctypes.data, out[3].ctypes.data)
        assert all((o == -7.0).all() for o in out), "outputs written on an error"
        return rc

    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * 8) as plan:
        ptr = rows.ctypes.data
        bad = [dict(rows_ptr=None), dict(d=False), dict(r=False), dict(ref=-1), dict(ref=3), dict(n_chunks=1), dict(n_chunks=0),
               dict(pad=0), dict(pad=3), dict(pad=16), dict(bw=0.0), dict(bw=-1.0), dict(bw=nan), dict(bw=inf), dict(fc=0.0),
               dict(fc=-2.0), dict(fc=nan), dict(fc=inf), dict(kind=7),
               dict(mode=2), dict(mode=-1), dict(min_snr=-1.0), dict(min_snr=nan), dict(min_snr=inf), dict(min_snr=-inf),
               dict(mode=_lib.FXC_FRINGE_REF, min_snr=5.0)]
        for change in bad:
            args = dict(rows_ptr=ptr, n_chunks=n_chunks, bw=BW, fc=FC, ref=0, pad=2)
            args.update(change)
            rc = call(plan, **args)
            assert rc == _lib.FXC_ERR_ARG, change
            with pytest.raises(ValueError):
                _lib.check(rc, plan._h)
        for chunks, pad in ((4097, 1), (2049, 2), (513, 8)):          # Lt = 8192: nothing reads the chunks rows does not hold
            rc = call(plan, ptr, chunks, BW, FC, 0, pad)
            assert rc == _lib.FXC_ERR_UNSUPPORTED, (chunks, pad)
            with pytest.raises(NotImplementedError, match="4096"):
                _lib.check(rc, plan._h)
        # snr and base_out may be NULL
        want = plan.fringe_fit(rows, BW, FC, weights=ones, baselines="all", min_snr=5.0)
        d, r = np.zeros(3), np.zeros(3)
        assert plan._lib.fxc_fringe_fit_weighted(plan._h, ptr, ones.ctypes.data, n_chunks, _lib.FXC_MEM_HOST, BW, FC, 0, 2,
                                                 _lib.FXC_FRINGE_ALL, 5.0, d.ctypes.data, r.ctypes.data, None, None) == 0
        assert np.array_equal(d, want[0]) and np.array_equal(r, want[1]) and (want[2][1:] > 10.0).all()
        # a threshold nothing passes: every antenna 0
        none = plan.fringe_fit(rows, BW, FC, weights=ones, baselines="all", min_snr=1e6, return_baselines=True)
        assert not none[0].any() and not none[1].any() and not none[2].any() and (none[3][:, 2] > 10.0).all()
        for word in ("ALL", "every", "", None, 1):
            with pytest.raises(ValueError):
                plan.fringe_fit(rows, BW, FC, baselines=word)
        for shape in ((n_chunks, 3, nchan - 1), (n_chunks, 2, nchan), (n_chunks - 1, 3, nchan), (3, nchan), (n_chunks, plan.n_rows + 1, nchan)):
            with pytest.raises(ValueError):
                plan.fringe_fit(rows, BW, FC, weights=np.ones(shape, np.float32))
        with pytest.raises(ValueError):                                # weights in the memory of rows
            plan.fringe_fit(rows, BW, FC, weights=torch.from_numpy(ones).cuda())
        with pytest.raises(ValueError):
            plan.fringe_fit(torch.from_numpy(rows).cuda(), BW, FC, weights=ones)
        with pytest.raises(ValueError):
            plan.fringe_fit(rows, BW, FC, baselines="ref", min_snr=5.0)
    with plan_mod.FxPlan(1, 64, 4, 64 * 8) as plan:                    # one antenna: no baseline
        out = [np.full(1, -7.0) for _ in range(3)]
        rc = plan._lib.fxc_fringe_fit_weighted(plan._h, rows.ctypes.data, None, n_chunks, _lib.FXC_MEM_HOST, BW, FC, 0, 2, _lib.FXC_FRINGE_ALL,
                                               0.0, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, None)
        assert rc == _lib.FXC_ERR_ARG and all((o == -7.0).all() for o in out)


# -- nothing else moved ---------------------------------------------------------------------------------------------------------
def test_weighted_fit_leaves_the_rows_alone(plan_mod, torch):
    from effex_amd import synth
    n_ant, nchan, n_spec, n_chunks = 3, 64, 20, 6
    x = torch.from_numpy(synth.synth_iq(31, n_chunks, n_ant, nchan * n_spec)).cuda()
    tau = np.arange(n_ant) * 1.7e-7
    rate = np.arange(n_ant) * 0.11 / FC
    ones = np.ones((n_chunks, 3, nchan), np.float32)
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * n_spec) as plan:
        before = plan.fx_rows(x).cpu().numpy()
        plan.fringe_fit(before, BW, FC, weights=ones, baselines="all")
        plan.fringe_fit(torch.from_numpy(before).cuda(), BW, FC, ref=n_ant - 1, pad=4, weights=torch.from_numpy(ones).cuda())
        assert np.array_equal(plan.fx_rows(x).cpu().numpy(), before)
        plan.set_delay_track(tau, rate, BW, FC)
        tracked = plan.fx_rows(x).cpu().numpy()
        assert plan.track_chunk == n_chunks
        plan.fringe_fit(tracked, BW, FC, weights=ones, baselines="all")
        assert plan.track_chunk == n_chunks          # the fit consumes no chunk
        plan.track_seek(0)
        assert np.array_equal(plan.fx_rows(x).cpu().numpy(), tracked)
        plan.fx_accumulate(x)                        # chunks 6 .. 11 of the track
        plan.fringe_fit(tracked, BW, FC, weights=ones, baselines="all")
        integ = plan.finalize("SPECTRUM")
        plan.track_seek(n_chunks)
        plan.fx_accumulate(x)
        assert np.array_equal(plan.finalize("SPECTRUM"), integ)


# -- closure from samples -------------------------------------------------------------------------------------------------------
CLOSURE = (4, 64, 32, 48)       # n_ant, nchan, spectra per chunk, chunks
LOST = (10, 15)                 # chunks 10 to 14 are lost


def closure_samples(n_ant, nchan, n_spec, n_chunks, seed):
    """test_gpu_fringe.py's construction with a fourth antenna: common noise delayed by tau_a(t) = tau0[a] + t rho[a], receiver
    noise of four times the source power on top.  Rates 0.21 and -0.33 / FC are 0.54 apart: baseline (1, 2) wraps."""
    rng = np.random.default_rng(seed)
    n = nchan * n_spec
    tau0 = np.array([0.0, 3.3, -7.6, 5.2][:n_ant]) / BW
    rho = np.array([0.0, 0.21, -0.33, 0.12][:n_ant]) / FC
    df = np.fft.fftfreq(n, 1.0 / BW)
    x = np.zeros((n_chunks, n_ant, n), np.complex64)
    for t in range(n_chunks):
        s = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)
        sf = np.fft.fft(s)
        for a in range(n_ant):
            tau = tau0[a] + t * rho[a]
            ph = FC * tau
            y = np.fft.ifft(sf * np.exp(-2j * np.pi * df * tau)) * np.exp(-2j * np.pi * (ph - np.rint(ph)))
            x[t, a] = y + 2.0 * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)
    return x, tau0, rho


def coherence_to_ref(rows, n_ant, keep, ref=0):
    """|sum R| / sum |R| over the chunks `keep` and the bins of every baseline to ref"""
    index = {ab: i for i, ab in enumerate(fringe_ref.pairs(n_ant))}
    out = []
    for b in range(n_ant):
        if b != ref:
            R = rows[keep, index[(min(ref, b), max(ref, b))]].astype(np.complex128)
            out.append(abs(R.sum()) / np.abs(R).sum())
    return np.array(out)


def closure_case(plan_mod, torch):
    n_ant, nchan, n_spec, n_chunks = CLOSURE
    x_np, tau0, rho = closure_samples(n_ant, nchan, n_spec, n_chunks, seed=3)
    x = torch.from_numpy(x_np).cuda()
    cd, cr = fringe_ref.cells(nchan, n_chunks, 2)
    pd, pr = nchan / BW, 1.0 / FC
    keep = np.ones(n_chunks, bool)
    keep[LOST[0]:LOST[1]] = False
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * n_spec, window=design_window(4, nchan)) as plan:
        raw = plan.fx_rows(x)
        w = torch.ones((n_chunks, plan.n_baselines, nchan), dtype=torch.float32, device=raw.device)
        raw[LOST[0]:LOST[1]] = complex(float("nan"), float("nan"))
        w[LOST[0]:LOST[1]] = 0.0
        d, r, s = plan.fringe_fit(raw, BW, FC, weights=w, baselines="all")
        plan.set_delay_track(d, r, BW, FC)
        fitted = plan.fx_rows(x)
        d2, r2, s2 = plan.fringe_fit(fitted, BW, FC, weights=w, baselines="all")
        plan.set_delay_track(tau0, rho, BW, FC)
        truth = plan.fx_rows(x).cpu().numpy()
    c_raw = coherence_to_ref(raw.cpu().numpy(), n_ant, keep)
    c_fit = coherence_to_ref(fitted.cpu().numpy(), n_ant, keep)
    c_truth = coherence_to_ref(truth, n_ant, keep)
    return {"coherence_raw": c_raw.tolist(), "coherence_fitted": c_fit.tolist(), "coherence_truth": c_truth.tolist(),
            "ratio": float((c_fit / c_truth).min()), "snr": s[1:].tolist(),
            "first_fit_cells": [float(np.abs(period_diff(d, tau0, pd)).max() / cd), float(np.abs(period_diff(r, rho, pr)).max() / cr)],
            "second_fit_cells": [float(np.abs(d2).max() / cd), float(np.abs(r2).max() / cr)]}


def test_fitted_track_stops_the_fringes_over_lost_chunks(plan_mod, torch):
    rec = recorded(CLOSURE_FILE)
    f = closure_case(plan_mod, torch)
    print(json.dumps(f))
    assert f["ratio"] >= rec["ratio"] - 0.01, (f, rec)
    assert max(f["coherence_raw"]) < 0.1                  # the uncorrected fringes average away: the closure is no accident
    assert max(f["second_fit_cells"]) < 0.5, f
