"""Weighted gain solve on the GPU (include/fxcorr.h fxc_solve_gains_weighted, FxPlan.solve_gains(weights=, model=)) against the
float64 restatement of its definition (gains_weighted_ref.py).

Parity: both sides are float64 from the sums on, the sums S and Sw are exact products added in the same order, so only the order
of the sums over b and the contraction of multiply-adds differ.  The tests hold to the project's ceiling for this comparison,
1e-9 (CEIL_PARITY of tests/test_gpu_gains.py); reordering the restatement's own sums moves it by 1.3e-15 on these inputs.
tools/gains_weighted_measure.py writes the observed maxima to profiles/gains_weighted/parity.json.
Bits: no output bit depends on the workspace target, on host or device input, on auto rows behind the cross rows, on what a
flagged sample holds, on how a flag is written (0, -1, NaN) or on a common power-of-two factor of the weights.
Damage: the samples of tests/test_gains_weighted_host.py through the library's own F and X stages: the weighted solve is within
the bound of tests/golden/gains_weighted_bounds.json, the unweighted solve of the same rows more than ten bounds off."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import gains_ref
import gains_weighted_ref as wref
from effex_amd.window import design_window

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS = os.path.join(ROOT, "tests", "golden", "gains_weighted_bounds.json")
CEIL_PARITY = 1e-9
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


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


# -- parity -----------------------------------------------------------------------------------------------------------------
N_CHUNKS = 19           # one full block of 16 loads and a remainder of 2 + 1; intervals of 5 cut it 5 5 5 4, of 16 16 + 3
INTERVALS = (0, 5, 16)
PARITY = [(3, 64), (4, 64), (5, 63), (8, 1000), (16, 64), (17, 64), (33, 64), (55, 64), (64, 64)]
SIGMA = 0.1
_CASES = {}


def parity_inputs(n_ant, nchan):
    """-> rows, weights, model, models per interval {interval: [n_int, n_baselines, nchan]}, and (rows, weights) of the same
    kind made without a model; drawn once per shape.  Every solve below gets rows its model fits: rows g_a conj(g_b) M_ab with the
    model M or with (1 + s / 4) M for interval s, rows g_a conj(g_b) without a model.  Rows that carry M solved without it fit
    nothing, and at 3 and 4 live antennas the iteration then wanders (step of 2 to 3 after 60 iterations on an MI355X and in the
    restatement alike) and multiplies rounding differences to 6e-7: that compares two roundings, not two implementations."""
    if (n_ant, nchan) not in _CASES:
        rng = np.random.default_rng(100 * n_ant + nchan)
        _, model, rows, weights = wref.damaged_case(n_ant, nchan, N_CHUNKS, rng, sigma=SIGMA)
        per = {iv: np.stack([model * np.float32(1.0 + 0.25 * s) for s in range(len(gains_ref.intervals(N_CHUNKS, iv)))]) for iv in INTERVALS}
        _, _, rows_plain, weights_plain = wref.damaged_case(n_ant, nchan, N_CHUNKS, rng, sigma=SIGMA, with_model=False)
        _CASES[(n_ant, nchan)] = (rows, weights, model, per, (rows_plain, weights_plain))
    return _CASES[(n_ant, nchan)]


def parity_case(plan_mod, torch, n_ant, nchan):
    """-> per (interval, model kind, ref, iters, input kind): max|g_gpu - g_ref| / max|g_ref| and max|step_gpu - step_ref|; the
    exact zeros of the dead antenna and bin and the real reference gain are asserted on the way"""
    rows_m, weights_m, model, per, (rows_p, weights_p) = parity_inputs(n_ant, nchan)
    device = {id(a): torch.from_numpy(a).cuda() for a in (rows_m, weights_m, rows_p, weights_p)}
    figures = []
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * 8) as plan:
        for interval in INTERVALS:
            spans = gains_ref.intervals(N_CHUNKS, interval)
            for kind, mdl, rows, weights in (("none", None, rows_p, weights_p), ("one", model, rows_m, weights_m),
                                             ("each", per[interval], rows_m, weights_m)):
                mats = [wref.average(rows[c0:c1], weights[c0:c1], n_ant, None if mdl is None else (mdl if mdl.ndim == 2 else mdl[s]))
                        for s, (c0, c1) in enumerate(spans)]
                for ref in (0, n_ant // 2):
                    for iters in (10, 60):
                        want = [wref.solve_matrix(um, dm, ref, iters) for um, dm in mats]
                        want_g, want_s = np.stack([g for g, _ in want]), np.stack([s for _, s in want])
                        for source, data, w in (("host", rows, weights), ("device", device[id(rows)], device[id(weights)])):
                            g, s = plan.solve_gains(data, interval=interval, ref=ref, iters=iters, weights=w, model=mdl)
                            assert g.dtype == np.complex128 and g.shape == (len(spans), n_ant, nchan)
                            assert s.dtype == np.float64 and s.shape == (len(spans), nchan)
                            assert np.isfinite(g).all() and np.isfinite(s).all()
                            assert (g[:, ref].imag == 0).all() and (g[:, ref].real >= 0).all()
                            assert (g[:, wref.DEAD_ANT] == 0).all() and (g[:, :, wref.DEAD_BIN] == 0).all()
                            assert (s[:, wref.DEAD_BIN] == 0).all()
                            figures.append({"n_ant": n_ant, "nchan": nchan, "interval": interval, "model": kind, "ref": ref,
                                            "iters": iters, "input": source,
                                            # (3 antennas with ref 1, the dead one: nothing is solved, both sides are 0)
                                            "gain_rel": float(np.abs(g - want_g).max() / max(np.abs(want_g).max(), 1e-300)),
                                            "step_abs": float(np.abs(s - want_s).max()), "step_ref_max": float(want_s.max())})
    return figures


@pytest.mark.parametrize("n_ant,nchan", PARITY)
def test_weighted_solve_matches_the_restatement(plan_mod, torch, n_ant, nchan):
    figures = parity_case(plan_mod, torch, n_ant, nchan)
    print(json.dumps({"gain_rel": max(f["gain_rel"] for f in figures), "step_abs": max(f["step_abs"] for f in figures)}))
    for f in figures:
        assert f["gain_rel"] <= CEIL_PARITY and f["step_abs"] <= CEIL_PARITY, f


@pytest.mark.parametrize("n_ant,nchan", [(8, 1000), (64, 64)])
def test_unit_weights_and_a_unit_model_agree_with_solve_gains(plan_mod, torch, n_ant, nchan):
    rows = parity_inputs(n_ant, nchan)[4][0].copy()       # rows g_a conj(g_b) + noise: what a solve without a model fits
    rows[rows == wref.FLAG_VALUE] = 0.25 - 0.5j           # the unweighted solve reads every sample
    nb = n_ant * (n_ant - 1) // 2
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * 8) as plan:
        for interval in (0, 5):
            want_g, want_s = plan.solve_gains(rows, interval=interval, ref=1, iters=30)
            for kwargs in (dict(weights=np.ones((N_CHUNKS, nb, nchan), np.float32)), dict(model=np.ones((nb, nchan)))):
                g, s = plan.solve_gains(rows, interval=interval, ref=1, iters=30, **kwargs)
                assert np.abs(g - want_g).max() / np.abs(want_g).max() <= CEIL_PARITY, sorted(kwargs)
                assert np.abs(s - want_s).max() <= CEIL_PARITY, sorted(kwargs)


# -- bits ---------------------------------------------------------------------------------------------------------------------
BITS_SHAPE = (8, 1000)
BITS_INTERVALS = (0, 2, 5)


def bits_model(interval):
    """one model for intervals 0 and 5, a model per interval for 2 (10 of them: groups of intervals upload their own part)"""
    model = parity_inputs(*BITS_SHAPE)[2]
    if interval != 2:
        return model
    n_int = len(gains_ref.intervals(N_CHUNKS, 2))
    return np.stack([model * np.float32(1.0 + 0.25 * s) for s in range(n_int)])


def test_outputs_do_not_depend_on_the_batches(plan_mod, torch):
    """A workspace target of 1 and of 3 MiB (FXC_WS_MB is read once per process: a child for each setting) against the default:
    host rows and weights go through in batches of a chunk or a few, the intervals in groups with their part of the models --
    the same bits, host and device input."""
    n_ant, nchan = BITS_SHAPE
    rows, weights = parity_inputs(n_ant, nchan)[:2]       # 224 KB of cross rows and 112 KB of weights a chunk, 672 KB of U, D
    code = ("import numpy as np, torch, sys; sys.path.insert(0, %r); from effex_amd import plan\n"
            "d = np.load(sys.argv[1]); rows, weights = d['rows'], d['weights']; out = {}\n"
            "rd, wd = torch.from_numpy(rows).cuda(), torch.from_numpy(weights).cuda()\n"
            "with plan.FxPlan(%d, %d, 4, %d) as p:\n"
            "    for interval in (0, 2, 5):\n"
            "        for kind, r, w in (('h', rows, weights), ('d', rd, wd)):\n"
            "            g, s = p.solve_gains(r, interval=interval, ref=3, iters=20, weights=w, model=d['m%%d' %% interval])\n"
            "            out['g%%s%%d' %% (kind, interval)] = g; out['s%%s%%d' %% (kind, interval)] = s\n"
            "np.savez(sys.argv[2], **out)\n" % (ROOT, n_ant, nchan, nchan * 8))
    with tempfile.TemporaryDirectory() as tmp:
        np.savez(os.path.join(tmp, "in.npz"), rows=rows, weights=weights, **{"m%d" % iv: bits_model(iv) for iv in BITS_INTERVALS})
        got = {}
        for label, ws_mb in (("default", None), ("one", "1"), ("three", "3")):
            env = {k: v for k, v in os.environ.items() if k != "FXC_WS_MB"}
            if ws_mb:
                env["FXC_WS_MB"] = ws_mb
            res = os.path.join(tmp, label + ".npz")
            subprocess.run([sys.executable, "-c", code, os.path.join(tmp, "in.npz"), res], check=True, env=env, timeout=600)
            got[label] = dict(np.load(res))
    for key, want in got["default"].items():
        for label in ("one", "three"):
            assert same_bits(got[label][key], want), (label, key)
    for interval in BITS_INTERVALS:
        for name in ("g", "s"):
            assert same_bits(got["default"]["%sh%d" % (name, interval)], got["default"]["%sd%d" % (name, interval)]), (name, interval)
        want_g, want_s = wref.solve_rows(rows, n_ant, interval=interval, ref=3, iters=20, weights=weights, model=bits_model(interval))
        assert np.abs(got["default"]["gh%d" % interval] - want_g).max() / np.abs(want_g).max() <= CEIL_PARITY


def test_flags_autos_and_weight_scale_change_no_bit(plan_mod, torch):
    """against the plain call on the same inputs: a plan with autos (n_rows > n_baselines, weights still n_baselines rows), flagged
    values of NaN / Inf / 1e30, flags written as -1 or NaN, and all weights times 4"""
    n_ant, nchan = BITS_SHAPE
    rows, weights, model = parity_inputs(n_ant, nchan)[:3]
    flagged = weights == 0
    rng = np.random.default_rng(5)
    autos = (rng.standard_normal((N_CHUNKS, n_ant, nchan)) * 50).astype(np.complex64)
    kw = dict(interval=5, ref=1, iters=20)
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * 8) as plan:
        want = plan.solve_gains(rows, weights=weights, model=model, **kw)
        keep_rows, keep_weights = rows.copy(), weights.copy()
        for value in (np.nan, np.inf, 1e30):
            other = rows.copy()
            other[flagged] = np.complex64(complex(value, -value))
            for r, w in ((other, weights), (torch.from_numpy(other).cuda(), torch.from_numpy(weights).cuda())):
                got = plan.solve_gains(r, weights=w, model=model, **kw)
                assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]), value
        for value in (-1.0, np.nan):
            other = weights.copy()
            other[flagged] = value
            for r, w in ((rows, other), (torch.from_numpy(rows).cuda(), torch.from_numpy(other).cuda())):
                got = plan.solve_gains(r, weights=w, model=model, **kw)
                assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]), value
        got = plan.solve_gains(rows, weights=weights * np.float32(4), model=model, **kw)
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
        # the call leaves its inputs alone
        dev_r, dev_w = torch.from_numpy(rows).cuda(), torch.from_numpy(weights).cuda()
        plan.solve_gains(dev_r, weights=dev_w, model=model, **kw)
        assert np.array_equal(dev_r.cpu().numpy().view(np.uint64), keep_rows.view(np.uint64))
        assert np.array_equal(dev_w.cpu().numpy().view(np.uint32), keep_weights.view(np.uint32))
        assert np.array_equal(rows.view(np.uint64), keep_rows.view(np.uint64)) and np.array_equal(weights, keep_weights)
    wide = np.ascontiguousarray(np.concatenate([rows, autos], axis=1))
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * 8, autos=True) as plan:
        assert plan.n_rows == plan.n_baselines + n_ant
        for r, w in ((wide, weights), (torch.from_numpy(wide).cuda(), torch.from_numpy(weights).cuda())):
            got = plan.solve_gains(r, weights=w, model=model, **kw)
            assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
        with pytest.raises(ValueError):
            plan.solve_gains(wide, weights=np.ones(wide.shape, np.float32))       # weights have no auto rows


# -- samples with damage --------------------------------------------------------------------------------------------------------
DAMAGE_SEEDS = (0, 1)


def damage_bound():
    return json.load(open(BOUNDS))["bound"]


def damage_case(plan_mod, torch, seed):
    x_np, c, weights = wref.damaged_samples(seed)
    nchan = gains_ref.SAMPLE_NCHAN
    out = {"seed": seed}
    with plan_mod.FxPlan(wref.DAMAGE_ANT, nchan, 4, x_np.shape[2], window=design_window(4, nchan)) as plan:
        rows = plan.fx_rows(torch.from_numpy(x_np).cuda())
        w_dev = torch.from_numpy(weights).cuda()
        for ref in wref.DAMAGE_REFS:
            truth = gains_ref.true_ratios(c, ref)
            g, _ = plan.solve_gains(rows, ref=ref, iters=gains_ref.SAMPLE_ITERS, weights=w_dev)
            plain, _ = plan.solve_gains(rows, ref=ref, iters=gains_ref.SAMPLE_ITERS)
            out["weighted ref %d" % ref] = float(np.abs(wref.scalar_ratios(g[0], ref) - truth).max())
            out["unweighted ref %d" % ref] = float(np.abs(wref.scalar_ratios(plain[0], ref) - truth).max())
    return out


@pytest.mark.parametrize("seed", DAMAGE_SEEDS)
def test_weights_recover_the_scalars_from_damaged_samples(plan_mod, torch, seed):
    bound = damage_bound()
    f = damage_case(plan_mod, torch, seed)
    print(json.dumps(f), "bound", bound)
    for ref in wref.DAMAGE_REFS:
        assert f["weighted ref %d" % ref] <= bound, (f, bound)
        assert f["unweighted ref %d" % ref] > 10.0 * bound, (f, bound)


# -- into the gain track -----------------------------------------------------------------------------------------------------------
def test_a_dead_antenna_goes_into_the_gain_track_as_zero_rows(plan_mod, torch):
    """8 antennas x 64 channels under a zero-rate delay track: a weighted solve with antenna 2 dead; set_track_gains takes it, the
    rows of every baseline with antenna 2 are exactly 0 and the others are those under the same gains with g_2 = 1, bit for bit"""
    from effex_amd import synth
    n_ant, nchan, dead = 8, 64, 2
    x = torch.from_numpy(synth.synth_iq(41, 4, n_ant, nchan * 16)).cuda()
    pr = gains_ref.pairs(n_ant)
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * 16) as plan:
        plan.set_delay_track(np.linspace(0.0, 1e-7, n_ant), np.zeros(n_ant), BW, FC)
        rows = plan.fx_rows(x)
        weights = np.ones((4, len(pr), nchan), np.float32)
        for i, (a, b) in enumerate(pr):
            if dead in (a, b):
                weights[:, i] = 0
        g, step = plan.solve_gains(rows, iters=30, weights=torch.from_numpy(weights).cuda())
        assert np.isfinite(g).all() and (g[0, dead] == 0).all()
        live = [a for a in range(n_ant) if a != dead]
        assert (g[0, live] != 0).all()
        plan.track_seek(0)
        plan.set_track_gains(g)
        got = plan.fx_rows(x).cpu().numpy()
        patched = g.copy()
        patched[0, dead] = 1.0
        plan.track_seek(0)
        plan.set_track_gains(patched)
        want = plan.fx_rows(x).cpu().numpy()
    for i, (a, b) in enumerate(pr):
        if dead in (a, b):
            assert (got[:, i] == 0).all(), (a, b)
        else:
            assert np.array_equal(got[:, i].view(np.uint64), want[:, i].view(np.uint64)), (a, b)
            assert (got[:, i] != 0).any()


# -- arguments ---------------------------------------------------------------------------------------------------------------------
def test_weighted_solve_argument_checks(plan_mod, torch):
    from effex_amd import _lib
    n_ant, nchan, n = 3, 64, 7
    rng = np.random.default_rng(11)
    rows = gains_ref.model_rows(gains_ref.draw_gains(n_ant, nchan, rng), n, rng, sigma=0.1)
    weights = np.ones((n, 3, nchan), np.float32)
    model = np.ones((3, nchan), np.complex64)
    model4 = np.ones((2, 3, nchan), np.complex64)        # intervals of 4: two of them

    def call(plan, rows_ptr, w_ptr=None, n_chunks=n, kind=_lib.FXC_MEM_HOST, model_ptr=None, n_model=0, interval=0, ref=0, iters=10,
             gains=True):
        g, s = np.full((n, plan.n_ant, plan.nchan), -7.0 + 0j), np.full((n, plan.nchan), -7.0)
        rc = plan._lib.fxc_solve_gains_weighted(plan._h, rows_ptr, w_ptr, n_chunks, kind, model_ptr, n_model, interval, ref, iters,
                                                g.ctypes.data if gains else None, s.ctypes.data)
        if rc != 0:
            assert (g == -7.0).all() and (s == -7.0).all(), "outputs written on an error"
        return rc

    bad_model = model.copy()
    bad_model[1, 7] = np.complex64(complex(np.nan, 0.0))
    inf_model = model.copy()
    inf_model[2, 0] = np.complex64(complex(1.0, np.inf))
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * 8) as plan:
        ptr, wp, mp = rows.ctypes.data, weights.ctypes.data, model.ctypes.data
        for change in (dict(rows_ptr=None), dict(gains=False), dict(n_chunks=0), dict(n_chunks=-3), dict(interval=-1), dict(ref=-1),
                       dict(ref=3), dict(iters=0), dict(iters=-5), dict(iters=1001), dict(kind=7),
                       dict(model_ptr=mp, n_model=0), dict(model_ptr=None, n_model=1), dict(model_ptr=mp, n_model=2),
                       dict(model_ptr=mp, n_model=-1), dict(model_ptr=model4.ctypes.data, n_model=3, interval=4),
                       dict(model_ptr=bad_model.ctypes.data, n_model=1), dict(model_ptr=inf_model.ctypes.data, n_model=1)):
            args = dict(rows_ptr=ptr, w_ptr=wp)
            args.update(change)
            rc = call(plan, **args)
            assert rc == _lib.FXC_ERR_ARG, change
            with pytest.raises(ValueError):
                _lib.check(rc, plan._h)
        # the same calls made right succeed: NULL weights, a model per interval, a zero in the model, step NULL
        assert call(plan, ptr) == 0 and call(plan, ptr, wp, model_ptr=mp, n_model=1) == 0
        assert call(plan, ptr, wp, model_ptr=model4.ctypes.data, n_model=2, interval=4) == 0
        zero_model = model.copy()
        zero_model[0, 9] = 0
        g, s = plan.solve_gains(rows, weights=weights, model=zero_model)
        assert np.isfinite(g).all() and np.isfinite(s).all()
        only = np.zeros((1, n_ant, nchan), np.complex128)
        assert plan._lib.fxc_solve_gains_weighted(plan._h, ptr, wp, n, _lib.FXC_MEM_HOST, None, 0, 0, 0, 10, only.ctypes.data, None) == 0
        assert same_bits(only, plan.solve_gains(rows, iters=10, weights=weights)[0])
        # Python: shapes and host / device mixing
        for kwargs in (dict(weights=weights[:, :2]), dict(weights=weights[:5]), dict(weights=weights[:, :, :32]), dict(weights=weights[0]),
                       dict(model=model[:2]), dict(model=model[:, :32]), dict(model=model4), dict(model=np.ones((3, 3, nchan))),
                       dict(weights=torch.from_numpy(weights).cuda()), dict(weights=weights, iters=0), dict(model=model, ref=3)):
            with pytest.raises(ValueError):
                plan.solve_gains(rows, **kwargs)
        with pytest.raises(ValueError):
            plan.solve_gains(torch.from_numpy(rows).cuda(), weights=weights)
        with pytest.raises(ValueError):
            plan.solve_gains(torch.from_numpy(rows).cuda(), weights=torch.from_numpy(weights.astype(np.float64)).cuda())
        # 2-D rows take 2-D weights
        g2 = plan.solve_gains(rows[1], weights=weights[1], model=model)
        g3 = plan.solve_gains(rows[1:2], weights=weights[1:2], model=model)
        assert same_bits(g2[0], g3[0]) and same_bits(g2[1], g3[1])
    with plan_mod.FxPlan(2, nchan, 4, nchan * 8) as plan:                # two antennas: one baseline closes nothing
        rc = call(plan, rows.ctypes.data, weights.ctypes.data)
        assert rc == _lib.FXC_ERR_UNSUPPORTED
        with pytest.raises(NotImplementedError, match="3 or more antennas"):
            _lib.check(rc, plan._h)
        with pytest.raises(NotImplementedError):
            plan.solve_gains(rows[:, :1], weights=weights[:, :1])
