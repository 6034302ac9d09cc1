"""Fringe fit on the GPU (include/fxcorr.h fxc_fringe_fit, FxPlan.fringe_fit) against the float64 restatement of its definition
(fringe_ref.py).

Parity: the peak cell is the restatement's; the sub-cell parts differ by the float32 rounding of the frequency transform the
float64 stencil is summed from.  That bound is measured: profiles/fringe/parity.json holds the largest |gpu - float64| of the
delays and of the rates in grid cells, and the largest relative difference of snr, over the cases of this module on an MI355X
(tools/fringe_measure.py writes it); the tests hold to twice those, under the ceilings 0.05 cell and 1e-5.
Closure: samples with injected delays and rates, fitted from the rows and fed back as a track, against the same samples under
the injected truth; profiles/fringe/closure.json holds the measured coherence ratios, the test holds to them less 0.01."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import fringe_ref
from effex_amd.window import design_window
from fringe_ref import BW, FC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILES = os.path.join(ROOT, "profiles", "fringe")
CEIL_CELL = 0.05        # beyond this the interpolation adds more error than the estimator has
CEIL_SNR = 1e-5         # TOL_VIS


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def plan_mod(torch):
    from effex_amd import plan
    return plan


def recorded(name):
    with open(os.path.join(PROFILES, name)) as f:
        return json.load(f)


# -- parity -----------------------------------------------------------------------------------------------------------------
N_CHUNKS = {64: 48, 1000: 40, 4096: 32}
PARITY = [(n_ant, nchan) for n_ant in (2, 3, 8, 16) for nchan in (64, 1000, 4096)]
SNR_IN = 1.0


def parity_rows(n_ant, nchan):
    rng = np.random.default_rng(100 * n_ant + nchan)
    delays, rates = fringe_ref.draw_antennas(n_ant, nchan, rng)
    return fringe_ref.model_rows(N_CHUNKS[nchan], n_ant, nchan, delays, rates, SNR_IN, rng)


def parity_case(plan_mod, torch, n_ant, nchan):
    """-> per (ref, pad, input kind): the peaks agree (asserted here), and the figures (delay, rate in cells, snr relative)"""
    rows = parity_rows(n_ant, nchan)
    rows_dev = torch.from_numpy(rows).cuda()
    n_chunks = N_CHUNKS[nchan]
    figures = []
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * 8) as plan:
        for ref in sorted({0, n_ant // 2 if n_ant > 2 else 1}):
            for pad in (1, 2, 4):
                want_d, want_r, want_s, peaks = fringe_ref.fit_rows(rows, n_ant, BW, FC, ref=ref, pad=pad)
                cd, cr = fringe_ref.cells(nchan, n_chunks, pad)
                lk, lt = fringe_ref.grid(nchan, n_chunks, pad)
                for kind, data in (("host", rows), ("device", rows_dev)):
                    d, r, s = plan.fringe_fit(data, BW, FC, ref=ref, pad=pad)
                    for out in (d, r, s):
                        assert out.dtype == np.float64 and out.shape == (n_ant,) and out[ref] == 0.0
                    # the same peak cell: each result lies within its cell (the offsets are at most half a cell) of the
                    # restatement's (q0, m0); the measured bound below then leaves no room for a neighbouring cell
                    for b, (q0, m0) in peaks.items():
                        em = (d[b] / cd - m0 + lk // 2) % lk - lk // 2
                        eq = (r[b] / cr - q0 + lt // 2) % lt - lt // 2
                        assert abs(em) <= 0.5 + CEIL_CELL and abs(eq) <= 0.5 + CEIL_CELL, (ref, pad, kind, b, q0, m0, em, eq)
                    others = [b for b in range(n_ant) if b != ref]
                    figures.append({"n_ant": n_ant, "nchan": nchan, "ref": ref, "pad": pad, "input": kind,
                                    "delay_cells": float(np.abs(d - want_d).max() / cd),
                                    "rate_cells": float(np.abs(r - want_r).max() / cr),
                                    "snr_rel": float(np.abs(s[others] / want_s[others] - 1.0).max())})
    return figures


@pytest.mark.parametrize("n_ant,nchan", PARITY)
def test_fringe_fit_matches_the_restatement(plan_mod, torch, n_ant, nchan):
    rec = recorded("parity.json")
    bound_d = min(2.0 * rec["delay_cells"], CEIL_CELL)
    bound_r = min(2.0 * rec["rate_cells"], CEIL_CELL)
    bound_s = min(2.0 * rec["snr_rel"], CEIL_SNR)
    figures = parity_case(plan_mod, torch, n_ant, nchan)
    for f in figures:
        print(json.dumps(f))
    for f in figures:
        assert f["delay_cells"] <= bound_d and f["rate_cells"] <= bound_r and f["snr_rel"] <= bound_s, (f, bound_d, bound_r, bound_s)


def test_host_and_device_rows_give_the_same_bits(plan_mod, torch):
    rows = parity_rows(3, 1000)
    with plan_mod.FxPlan(3, 1000, 4, 8000) as plan:
        host = plan.fringe_fit(rows, BW, FC, ref=1, pad=2)
        dev = plan.fringe_fit(torch.from_numpy(rows).cuda(), BW, FC, ref=1, pad=2)
    for a, b in zip(host, dev):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


# -- arguments --------------------------------------------------------------------------------------------------------------
def test_fringe_fit_argument_checks(plan_mod, torch):
    from effex_amd import _lib
    rows = parity_rows(3, 64)
    nan, inf = float("nan"), float("inf")

    def call(plan, rows_ptr, n_chunks, bw, fc, ref, pad, d=True, r=True, kind=_lib.FXC_MEM_HOST):
        out = [np.full(plan.n_ant, -7.0) for _ in range(3)]
        rc = plan._lib.fxc_fringe_fit(plan._h, rows_ptr, n_chunks, kind, bw, fc, ref, pad, out[0].ctypes.data if d else None,
                                      out[1].ctypes.data if r else None, out[2].ctypes.data)
        assert all((o == -7.0).all() for o in out), "outputs written on an error"
        return rc

    with plan_mod.FxPlan(3, 64, 4, 64 * 8) as plan:
        ptr = rows.ctypes.data
        bad = [dict(rows_ptr=None), dict(d=False), dict(r=False), dict(ref=-1), dict(ref=3), dict(n_chunks=1), dict(n_chunks=0),
               dict(pad=0), dict(pad=3), dict(pad=16), dict(bw=0.0), dict(bw=-1.0), dict(bw=nan), dict(bw=inf), dict(fc=0.0),
               dict(fc=-2.0), dict(fc=nan), dict(fc=inf), dict(kind=7)]
        for change in bad:
            args = dict(rows_ptr=ptr, n_chunks=48, bw=BW, fc=FC, ref=0, pad=2)
            args.update(change)
            rc = call(plan, **args)
            assert rc == _lib.FXC_ERR_ARG, change
            with pytest.raises(ValueError):
                _lib.check(rc, plan._h)
        # Lt = 8192: more chunks than rows holds, and nothing reads them
        for n_chunks, pad in ((4097, 1), (2049, 2), (513, 8)):
            rc = call(plan, ptr, n_chunks, BW, FC, 0, pad)
            assert rc == _lib.FXC_ERR_UNSUPPORTED, (n_chunks, pad)
            with pytest.raises(NotImplementedError, match="4096"):
                _lib.check(rc, plan._h)
        for ref in (-1, 3):
            with pytest.raises(ValueError):
                plan.fringe_fit(rows, BW, FC, ref=ref)
        with pytest.raises(ValueError):
            plan.fringe_fit(rows[:, :2], BW, FC)
        with pytest.raises(ValueError):
            plan.fringe_fit(rows[:, :, :32], BW, FC)
        with pytest.raises(ValueError):
            plan.fringe_fit(rows[0], BW, FC)
        # snr may be NULL
        d, r = np.zeros(3), np.zeros(3)
        assert plan._lib.fxc_fringe_fit(plan._h, ptr, 48, _lib.FXC_MEM_HOST, BW, FC, 0, 2, d.ctypes.data, r.ctypes.data, None) == 0
        want = plan.fringe_fit(rows, BW, FC)
        assert np.array_equal(d, want[0]) and np.array_equal(r, want[1])
    with plan_mod.FxPlan(1, 64, 4, 64 * 8) as plan:                       # one antenna: no baseline
        assert call(plan, rows.ctypes.data, 48, BW, FC, 0, 2) == _lib.FXC_ERR_ARG
    with plan_mod.FxPlan(2, 16384, 1, 16384 * 2) as plan:                  # Lk = 131072
        rc = call(plan, rows.ctypes.data, 4, BW, FC, 0, 8)
        assert rc == _lib.FXC_ERR_UNSUPPORTED
        with pytest.raises(NotImplementedError, match="65536"):
            _lib.check(rc, plan._h)
    with plan_mod.FxPlan(2, 1, 4, 4096, window=np.array([0.4, 0.3, 0.2, 0.1])) as plan:   # no frequency axis
        rc = call(plan, rows.ctypes.data, 48, BW, FC, 0, 2)
        assert rc == _lib.FXC_ERR_UNSUPPORTED
        with pytest.raises(NotImplementedError):
            _lib.check(rc, plan._h)


# -- closure from samples -----------------------------------------------------------------------------------------------------
CLOSURE = {"3x64": (3, 64, 32, 48, None), "2x4096": (2, 4096, 8, 48, None)}     # n_ant, nchan, spectra per chunk, chunks, path


def closure_samples(n_ant, nchan, n_spec, n_chunks, seed):
    """common noise delayed by tau_a(t) = tau0[a] + t rho[a] (fractional delay in the frequency domain, fringe rotation of the
    carrier), receiver noise of four times the source power on top"""
    rng = np.random.default_rng(seed)
    n = nchan * n_spec
    tau0 = np.array([0.0, 3.3, -7.6][:n_ant]) / BW
    rho = np.array([0.0, 0.21, -0.33][:n_ant]) / FC
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


def coherence_to_ref(rows, n_ant, ref=0):
    """|sum R| / sum |R| over chunks and bins of every baseline to ref"""
    index = {ab: i for i, ab in enumerate(fringe_ref.pairs(n_ant))}
    out = []
    for b in range(n_ant):
        if b != ref:
            R = rows[:, index[(min(ref, b), max(ref, b))]].astype(np.complex128)
            out.append(abs(R.sum()) / np.abs(R).sum())
    return np.array(out)


def closure_case(plan_mod, torch, name):
    n_ant, nchan, n_spec, n_chunks, path = CLOSURE[name]
    x_np, tau0, rho = closure_samples(n_ant, nchan, n_spec, n_chunks, seed=3)
    x = torch.from_numpy(x_np).cuda()
    cd, cr = fringe_ref.cells(nchan, n_chunks, 2)
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * n_spec, window=design_window(4, nchan), path=path) as plan:
        raw = plan.fx_rows(x)
        d, r, s = plan.fringe_fit(raw, BW, FC)
        plan.set_delay_track(d, r, BW, FC)
        fitted = plan.fx_rows(x)
        d2, r2, s2 = plan.fringe_fit(fitted, BW, FC)
        plan.set_delay_track(tau0, rho, BW, FC)
        truth = plan.fx_rows(x).cpu().numpy()
    c_raw = coherence_to_ref(raw.cpu().numpy(), n_ant)
    c_fit = coherence_to_ref(fitted.cpu().numpy(), n_ant)
    c_truth = coherence_to_ref(truth, n_ant)
    return {"coherence_raw": c_raw.tolist(), "coherence_fitted": c_fit.tolist(), "coherence_truth": c_truth.tolist(),
            "ratio": float((c_fit / c_truth).min()), "snr": s[1:].tolist(),
            "first_fit_cells": [float(np.abs(d - tau0).max() / cd), float(np.abs(r - rho).max() / cr)],
            "second_fit_cells": [float(np.abs(d2).max() / cd), float(np.abs(r2).max() / cr)]}


@pytest.mark.parametrize("name", sorted(CLOSURE))
def test_fitted_track_stops_the_fringes(plan_mod, torch, name):
    rec = recorded("closure.json")[name]
    f = closure_case(plan_mod, torch, name)
    print(json.dumps(f))
    assert f["ratio"] >= rec["ratio"] - 0.01, (f, rec)
    assert max(f["coherence_raw"]) < 0.1                  # the uncorrected fringes average away: the closure is no accident
    assert max(f["second_fit_cells"]) < 0.5, f


# -- batches ------------------------------------------------------------------------------------------------------------------
def test_outputs_do_not_depend_on_the_batches(plan_mod, torch):
    """One baseline per batch (a workspace target below two baselines' buffers; FXC_WS_MB is read once per process: a child for
    each setting) against the default's one batch: the same bits, host and device input."""
    n_ant, nchan = 8, 4096
    rows = parity_rows(n_ant, nchan)               # 32 chunks, pad 4: Lk 16384, 8 MiB of transform buffers a baseline
    code = ("import numpy as np, torch, sys; sys.path.insert(0, %r); from effex_amd import plan\n"
            "rows = np.load(sys.argv[1]); dev = torch.from_numpy(rows).cuda(); out = {}\n"
            "with plan.FxPlan(%d, %d, 4, %d) as p:\n"
            "    for ref in (0, 3):\n"
            "        for kind, data in (('h', rows), ('d', dev)):\n"
            "            d, r, s = p.fringe_fit(data, %r, %r, ref=ref, pad=4)\n"
            "            out['%%s%%d' %% (kind, ref)] = np.stack([d, r, s])\n"
            "np.savez(sys.argv[2], **out)\n" % (ROOT, n_ant, nchan, nchan * 8, BW, FC))
    with tempfile.TemporaryDirectory() as tmp:
        np.save(os.path.join(tmp, "rows.npy"), rows)
        got = {}
        for label, ws_mb in (("default", None), ("single", "12")):
            env = {k: v for k, v in os.environ.items() if k != "FXC_WS_MB"}
            if ws_mb:
                env["FXC_WS_MB"] = ws_mb
            res = os.path.join(tmp, label + ".npz")
            subprocess.run([sys.executable, "-c", code, os.path.join(tmp, "rows.npy"), res], check=True, env=env, timeout=600)
            got[label] = dict(np.load(res))
    for key, want in got["default"].items():
        assert np.array_equal(got["single"][key].view(np.uint64), want.view(np.uint64)), key


def test_outputs_do_not_depend_on_the_split_of_the_lines(plan_mod, torch):
    """More lines in a batch than one launch of a frequency pass takes: 16 baselines of 4096 chunks are 65536 lines, passes of
    65535 and 1 (gridDim.y).  This process, with the default workspace target, against a child whose target of 1 MiB holds one
    baseline a batch (4096 lines, no split): the same bits."""
    n_ant, nchan, n_chunks, ref = 17, 16, 4096, 5
    rng = np.random.default_rng(17)
    delays, rates = fringe_ref.draw_antennas(n_ant, nchan, rng)
    rows = fringe_ref.model_rows(n_chunks, n_ant, nchan, delays, rates, SNR_IN, rng)
    code = ("import numpy as np, torch, sys; sys.path.insert(0, %r); from effex_amd import plan\n"
            "dev = torch.from_numpy(np.load(sys.argv[1])).cuda()\n"
            "with plan.FxPlan(%d, %d, 4, %d) as p:\n"
            "    np.save(sys.argv[2], np.stack(p.fringe_fit(dev, %r, %r, ref=%d, pad=1)))\n" % (ROOT, n_ant, nchan, nchan * 8, BW, FC, ref))
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * 8) as plan:
        split = np.stack(plan.fringe_fit(torch.from_numpy(rows).cuda(), BW, FC, ref=ref, pad=1))
    with tempfile.TemporaryDirectory() as tmp:
        np.save(os.path.join(tmp, "rows.npy"), rows)
        env = dict(os.environ, FXC_WS_MB="1")
        res = os.path.join(tmp, "single.npy")
        subprocess.run([sys.executable, "-c", code, os.path.join(tmp, "rows.npy"), res], check=True, env=env, timeout=600)
        single = np.load(res)
    assert split.shape == (3, n_ant) and np.all(split[2, np.arange(n_ant) != ref] > 0.0)
    assert np.array_equal(single.view(np.uint64), split.view(np.uint64))


# -- nothing else moved -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ant,nchan,n_spec", [(3, 64, 20), (2, 4096, 5)])
def test_fringe_fit_leaves_the_rows_alone(plan_mod, torch, n_ant, nchan, n_spec):
    from effex_amd import synth
    n_chunks = 6
    x = torch.from_numpy(synth.synth_iq(31, n_chunks, n_ant, nchan * n_spec)).cuda()
    tau = np.arange(n_ant) * 1.7e-7
    rate = np.arange(n_ant) * 0.11 / FC
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * n_spec) as plan:
        before = plan.fx_rows(x).cpu().numpy()
        plan.fringe_fit(before, BW, FC)
        plan.fringe_fit(torch.from_numpy(before).cuda(), BW, FC, ref=n_ant - 1, pad=4)
        assert np.array_equal(plan.fx_rows(x).cpu().numpy(), before)
        plan.set_delay_track(tau, rate, BW, FC)
        tracked = plan.fx_rows(x).cpu().numpy()
        assert plan.track_chunk == n_chunks
        plan.fringe_fit(tracked, BW, FC)
        assert plan.track_chunk == n_chunks          # the fit consumes no chunk
        plan.track_seek(0)
        assert np.array_equal(plan.fx_rows(x).cpu().numpy(), tracked)
        plan.fx_accumulate(x)                        # chunks 6 .. 11 of the track
        plan.fringe_fit(tracked, BW, FC)
        integ = plan.finalize("SPECTRUM")
        plan.track_seek(n_chunks)
        plan.fx_accumulate(x)
        assert np.array_equal(plan.finalize("SPECTRUM"), integ)
