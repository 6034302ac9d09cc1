"""Gain solve on the GPU (include/fxcorr.h fxc_solve_gains, FxPlan.solve_gains / set_gains) against the float64 restatement of
its definition (gains_ref.py).

Parity: both sides are float64 from the sum on, so only the order of the sums over b and the contraction of multiply-adds
differ.  profiles/gains/parity.json holds the largest max|g_gpu - g_ref| / max|g_ref| and max|step_gpu - step_ref| over the
cases of this module on an MI355X (tools/gains_measure.py writes it); the tests hold to twice those, under the ceiling 1e-9.
Bits: no output bit depends on the workspace target, on host or device rows, or on auto rows behind the cross rows.
Closure: samples x_a = c_a s + n_a (gains_ref.samples), 8 antennas; the gains solved from their rows, applied with set_gains,
make the rows of the same samples solve to 1.  The second solve is the least-squares fit of rows divided by the first one's
model, so it is 1 exactly only for rows the model fits exactly; with receiver noise the weights |g_b|^2 of the two fits differ
and leave a term of (noise in V) x (spread of |g|^2), which the model's strong calibrator (receiver noise 0.02 of the source)
keeps small: measured on an MI355X max|g' - 1| = 1.6e-6 (the complex64 rounding of the rows alone would leave 6e-8), step
2.5e-16.  profiles/gains/closure.json holds the measured figure; the test holds to twice that under the ceiling 1e-4."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import gains_ref
from effex_amd.window import design_window

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILES = os.path.join(ROOT, "profiles", "gains")
BOUNDS = os.path.join(ROOT, "tests", "golden", "gains_bounds.json")
CEIL_PARITY = 1e-9
CEIL_CLOSURE = 1e-4


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


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


# -- parity -----------------------------------------------------------------------------------------------------------------
N_CHUNKS = 7            # 5 does not divide it: intervals of 5 and 2 chunks
PARITY = [(n_ant, nchan) for n_ant in (3, 4, 8, 16, 64) for nchan in (64, 1000, 4096)]
SIGMA = 0.1


def parity_rows(n_ant, nchan):
    rng = np.random.default_rng(100 * n_ant + nchan)
    return gains_ref.model_rows(gains_ref.draw_gains(n_ant, nchan, rng), N_CHUNKS, rng, sigma=SIGMA)


def parity_case(plan_mod, torch, n_ant, nchan):
    """-> per (interval, ref, iters, input kind): max|g_gpu - g_ref| / max|g_ref| and max|step_gpu - step_ref|"""
    rows = parity_rows(n_ant, nchan)
    rows_dev = torch.from_numpy(rows).cuda()
    figures = []
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * 8) as plan:
        for interval in (0, 5):
            mats = [gains_ref.average(rows[c0:c1], n_ant) for c0, c1 in gains_ref.intervals(N_CHUNKS, interval)]
            for ref in (0, n_ant // 2):
                for iters in (10, 60):
                    want = [gains_ref.solve_matrix(m, ref, iters) for m in mats]
                    want_g, want_s = np.stack([g for g, _ in want]), np.stack([s for _, s in want])
                    for kind, data in (("host", rows), ("device", rows_dev)):
                        g, s = plan.solve_gains(data, interval=interval, ref=ref, iters=iters)
                        assert g.dtype == np.complex128 and g.shape == (len(mats), n_ant, nchan)
                        assert s.dtype == np.float64 and s.shape == (len(mats), nchan)
                        assert (g[:, ref].imag == 0).all() and (g[:, ref].real >= 0).all()
                        figures.append({"n_ant": n_ant, "nchan": nchan, "interval": interval, "ref": ref, "iters": iters, "input": kind,
                                        "gain_rel": float(np.abs(g - want_g).max() / np.abs(want_g).max()),
                                        "step_abs": float(np.abs(s - want_s).max())})
    return figures


@pytest.mark.parametrize("n_ant,nchan", PARITY)
def test_solve_gains_matches_the_restatement(plan_mod, torch, n_ant, nchan):
    rec = recorded("parity.json")
    bound_g = min(2.0 * rec["gain_rel"], CEIL_PARITY)
    bound_s = min(2.0 * rec["step_abs"], CEIL_PARITY)
    figures = parity_case(plan_mod, torch, n_ant, nchan)
    for f in figures:
        print(json.dumps(f))
    for f in figures:
        assert f["gain_rel"] <= bound_g and f["step_abs"] <= bound_s, (f, bound_g, bound_s)


# antenna counts that are no power of two times a tile: tiles of 8, 4 and 4 bins, the workgroup's last wave partly idle
ODD_ANTENNAS = [(17, 64), (33, 64), (55, 64)]
# 31 chunks are every block of the average's walk: 16 + 8 + 4 + 2 + 1 with 16-byte loads (an even channel count; 1000 channels
# leave the last tile partial), 3 x 8 + 4 + 2 + 1 with 8-byte loads (an odd one)
LONG_CHUNKS = 31
LONG = [(8, 1000), (5, 63)]


def ceiling_case(plan_mod, torch, n_ant, nchan, n_chunks, refs, iters):
    """intervals 0 and 5, host and device rows against gains_ref.solve_rows under CEIL_PARITY, and the two against each other
    bit for bit"""
    rng = np.random.default_rng(1000 * n_chunks + 100 * n_ant + nchan)
    rows = gains_ref.model_rows(gains_ref.draw_gains(n_ant, nchan, rng), n_chunks, rng, sigma=SIGMA)
    rows_dev = torch.from_numpy(rows).cuda()
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * 8) as plan:
        for interval in (0, 5):
            for ref in refs:
                want_g, want_s = gains_ref.solve_rows(rows, n_ant, interval=interval, ref=ref, iters=iters)
                got = [plan.solve_gains(data, interval=interval, ref=ref, iters=iters) for data in (rows, rows_dev)]
                for kind, (g, s) in zip(("host", "device"), got):
                    assert g.shape == want_g.shape and s.shape == want_s.shape
                    gain_rel = float(np.abs(g - want_g).max() / np.abs(want_g).max())
                    step_abs = float(np.abs(s - want_s).max())
                    print(json.dumps({"n_ant": n_ant, "nchan": nchan, "n_chunks": n_chunks, "interval": interval, "ref": ref,
                                      "input": kind, "gain_rel": gain_rel, "step_abs": step_abs}))
                    assert gain_rel <= CEIL_PARITY and step_abs <= CEIL_PARITY, (kind, interval, ref, gain_rel, step_abs)
                assert same_bits(got[0][0], got[1][0]) and same_bits(got[0][1], got[1][1]), (interval, ref)


@pytest.mark.parametrize("n_ant,nchan", ODD_ANTENNAS)
def test_antenna_counts_that_leave_a_wave_partly_idle(plan_mod, torch, n_ant, nchan):
    ceiling_case(plan_mod, torch, n_ant, nchan, N_CHUNKS, (0, n_ant // 2), 30)


@pytest.mark.parametrize("n_ant,nchan", LONG)
def test_every_block_of_the_average_walk(plan_mod, torch, n_ant, nchan):
    ceiling_case(plan_mod, torch, n_ant, nchan, LONG_CHUNKS, (n_ant // 2,), 30)


def test_odd_channel_counts_and_one_chunk(plan_mod, torch):
    """an odd channel count takes the 8-byte loads; a 2-D array is one chunk; a zero bin gives zero gains and step"""
    n_ant, nchan = 5, 63
    rng = np.random.default_rng(17)
    rows = gains_ref.model_rows(gains_ref.draw_gains(n_ant, nchan, rng), 3, rng, sigma=SIGMA)
    rows[:, :, 11] = 0
    rec = recorded("parity.json")
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * 8) as plan:
        for data, ref_rows in ((rows, rows), (torch.from_numpy(rows).cuda(), rows), (rows[1], rows[1:2]),
                               (torch.from_numpy(rows[1]).cuda(), rows[1:2])):
            g, s = plan.solve_gains(data, ref=2, iters=30)
            want_g, want_s = gains_ref.solve_rows(ref_rows, n_ant, ref=2, iters=30)
            assert np.isfinite(g).all() and np.isfinite(s).all()
            assert (g[0, :, 11] == 0).all() and s[0, 11] == 0
            assert np.abs(g - want_g).max() / np.abs(want_g).max() <= min(2.0 * rec["gain_rel"], CEIL_PARITY)
            assert np.abs(s - want_s).max() <= min(2.0 * rec["step_abs"], CEIL_PARITY)


# -- bits ---------------------------------------------------------------------------------------------------------------------
def test_outputs_do_not_depend_on_the_batches(plan_mod, torch):
    """A workspace target of 1 and of 3 MiB (FXC_WS_MB is read once per process: a child for each setting) against the default:
    host rows go through in batches of a chunk or a few, the intervals in groups -- the same bits, host and device rows."""
    n_ant, nchan = 8, 1000
    rows = parity_rows(n_ant, nchan)               # 224 KB of cross rows a chunk, 448 KB of V an interval
    code = ("import numpy as np, torch, sys; sys.path.insert(0, %r); from effex_amd import plan\n"
            "rows = np.load(sys.argv[1]); dev = torch.from_numpy(rows).cuda(); out = {}\n"
            "with plan.FxPlan(%d, %d, 4, %d) as p:\n"
            "    for interval in (0, 2, 5):\n"
            "        for kind, data in (('h', rows), ('d', dev)):\n"
            "            g, s = p.solve_gains(data, interval=interval, ref=3, iters=20)\n"
            "            out['g%%s%%d' %% (kind, interval)] = g; out['s%%s%%d' %% (kind, interval)] = s\n"
            "np.savez(sys.argv[2], **out)\n" % (ROOT, n_ant, nchan, nchan * 8))
    with tempfile.TemporaryDirectory() as tmp:
        np.save(os.path.join(tmp, "rows.npy"), rows)
        got = {}
        for label, ws_mb in (("default", None), ("one", "1"), ("three", "3")):
            env = {k: v for k, v in os.environ.items() if k != "FXC_WS_MB"}
            if ws_mb:
                env["FXC_WS_MB"] = ws_mb
            res = os.path.join(tmp, label + ".npz")
            subprocess.run([sys.executable, "-c", code, os.path.join(tmp, "rows.npy"), res], check=True, env=env, timeout=600)
            got[label] = dict(np.load(res))
    for key, want in got["default"].items():
        for label in ("one", "three"):
            assert same_bits(got[label][key], want), (label, key)
    for interval in (0, 2, 5):
        for name in ("g", "s"):
            assert same_bits(got["default"]["%sh%d" % (name, interval)], got["default"]["%sd%d" % (name, interval)]), (name, interval)


def test_auto_rows_are_not_read(plan_mod, torch):
    """a plan with autos has n_rows = n_baselines + n_ant: the same cross rows give the bits of the plan without"""
    n_ant, nchan = 8, 1000
    rows = parity_rows(n_ant, nchan)
    rng = np.random.default_rng(5)
    autos = (rng.standard_normal((N_CHUNKS, n_ant, nchan)) * 50).astype(np.complex64)
    wide = np.ascontiguousarray(np.concatenate([rows, autos], axis=1))
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * 8) as plan:
        want = plan.solve_gains(rows, interval=5, ref=1, iters=20)
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * 8, autos=True) as plan:
        assert plan.n_rows == plan.n_baselines + n_ant
        for data in (wide, torch.from_numpy(wide).cuda()):
            got = plan.solve_gains(data, interval=5, ref=1, iters=20)
            assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
        with pytest.raises(ValueError):
            plan.solve_gains(rows)


# -- from samples -------------------------------------------------------------------------------------------------------------
def closure_case(plan_mod, torch, seed=100):
    n_ant, nchan, iters = 8, gains_ref.SAMPLE_NCHAN, gains_ref.SAMPLE_ITERS
    x_np, c = gains_ref.samples(n_ant, seed)
    x = torch.from_numpy(x_np).cuda()
    with plan_mod.FxPlan(n_ant, nchan, 4, x_np.shape[2], window=design_window(4, nchan)) as plan:
        raw = plan.fx_rows(x)
        g, step = plan.solve_gains(raw, iters=iters)
        plan.set_gains(g[0])
        flat = plan.fx_rows(x)
        g2, step2 = plan.solve_gains(flat, iters=iters)
    flat = flat.cpu().numpy()
    return {"closure": float(np.abs(g2 - 1.0).max()), "step_first": float(step.max()), "step_second": float(step2.max()),
            "rows_flat": float(np.abs(flat.mean(axis=0) - 1.0).max()),
            "ratio_error": float(np.abs(gains_ref.scalar_ratios(g[0], 0) - gains_ref.true_ratios(c, 0)).max())}


def test_solved_gains_flatten_the_rows_of_the_same_samples(plan_mod, torch):
    rec = recorded("closure.json")
    bound = json.load(open(BOUNDS))["bound"]
    f = closure_case(plan_mod, torch)
    print(json.dumps(f))
    assert f["closure"] <= min(2.0 * rec["closure"], CEIL_CLOSURE), (f, rec)
    assert f["step_second"] < 1e-12 and f["step_first"] < 1e-12            # float64 rounding: the iteration has converged
    assert f["ratio_error"] <= bound, (f, bound)


def test_scalars_from_samples_within_the_cpu_bound(plan_mod, torch):
    """the inputs of tests/test_gains_host.py's sample test through the library's own F, X and solve: within the same B"""
    import test_gains_host as host
    bound = json.load(open(BOUNDS))["bound"]
    nchan = gains_ref.SAMPLE_NCHAN
    for seed in host.SAMPLE_SEEDS:
        x_np, c = gains_ref.samples(host.SAMPLE_ANT, seed)
        with plan_mod.FxPlan(host.SAMPLE_ANT, nchan, 4, x_np.shape[2], window=design_window(4, nchan)) as plan:
            rows = plan.fx_rows(torch.from_numpy(x_np).cuda())
            for ref in host.SAMPLE_REFS:
                g, _ = plan.solve_gains(rows, ref=ref, iters=gains_ref.SAMPLE_ITERS)
                err = float(np.abs(gains_ref.scalar_ratios(g[0], ref) - gains_ref.true_ratios(c, ref)).max())
                print("seed %d ref %d: error %.3g (B %.3g)" % (seed, ref, err, bound))
                assert err <= bound, (seed, ref, err, bound)


def test_set_gains_with_delays(plan_mod, torch):
    """set_gains(g, tau, bw, fc) is set_rot_ant of the product tables: the rows equal those of the tables set by hand"""
    from effex_amd import synth
    n_ant, nchan, bw, fc = 4, 256, 2.4e6, 1.4204e9
    rng = np.random.default_rng(9)
    g = gains_ref.draw_gains(n_ant, nchan, rng)
    tau = rng.uniform(-1e-6, 1e-6, n_ant)
    x = torch.from_numpy(synth.synth_iq(77, 2, n_ant, nchan * 16)).cuda()
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * 16) as plan:
        plan.set_gains(g, tau, bw, fc)
        got = plan.fx_rows(x).cpu().numpy()
        plan.set_rot_ant(np.fft.ifftshift(1.0 / g, axes=1) * plan_mod.rot_tables(nchan, bw, fc, tau))
        assert np.array_equal(plan.fx_rows(x).cpu().numpy(), got)
        plan.set_delays(tau, bw, fc)
        plain = plan.fx_rows(x).cpu().numpy()
    want = gains_ref.apply_tables(plain, np.fft.ifftshift(1.0 / g, axes=1), n_ant)
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()          # TOL_VIS: complex64 rows


# -- errors -------------------------------------------------------------------------------------------------------------------
def test_solve_gains_argument_checks(plan_mod, torch):
    from effex_amd import _lib
    rows = parity_rows(3, 64)

    def call(plan, rows_ptr, n_chunks=N_CHUNKS, interval=0, ref=0, iters=10, gains=True, kind=_lib.FXC_MEM_HOST):
        g, s = np.full((N_CHUNKS, plan.n_ant, plan.nchan), -7.0 + 0j), np.full((N_CHUNKS, plan.nchan), -7.0)
        rc = plan._lib.fxc_solve_gains(plan._h, rows_ptr, n_chunks, kind, interval, ref, iters, g.ctypes.data if gains else None,
                                       s.ctypes.data)
        assert (g == -7.0).all() and (s == -7.0).all(), "outputs written on an error"
        return rc

    with plan_mod.FxPlan(3, 64, 4, 64 * 8) as plan:
        ptr = rows.ctypes.data
        for change in (dict(rows_ptr=None), dict(gains=False), dict(n_chunks=0), dict(n_chunks=-3), dict(interval=-1), dict(ref=-1),
                       dict(ref=3), dict(iters=0), dict(iters=-5), dict(iters=1001), dict(kind=7)):
            args = dict(rows_ptr=ptr)
            args.update(change)
            rc = call(plan, **args)
            assert rc == _lib.FXC_ERR_ARG, change
            with pytest.raises(ValueError):
                _lib.check(rc, plan._h)
        for kwargs in (dict(iters=0), dict(ref=3), dict(interval=-1)):
            with pytest.raises(ValueError):
                plan.solve_gains(rows, **kwargs)
        with pytest.raises(ValueError):
            plan.solve_gains(rows[:, :2])
        with pytest.raises(ValueError):
            plan.solve_gains(rows[:, :, :32])
        # step may be NULL; an interval beyond the chunks is one interval
        g = np.zeros((1, 3, 64), np.complex128)
        assert plan._lib.fxc_solve_gains(plan._h, ptr, N_CHUNKS, _lib.FXC_MEM_HOST, 0, 0, 10, g.ctypes.data, None) == 0
        want = plan.solve_gains(rows, iters=10)
        assert same_bits(g, want[0])
        far = plan.solve_gains(rows, interval=100, iters=10)
        assert same_bits(far[0], want[0]) and same_bits(far[1], want[1])
        with pytest.raises(ValueError):
            plan.set_gains(np.ones((3, 32)))
    with plan_mod.FxPlan(2, 64, 4, 64 * 8) as plan:                       # two antennas: one baseline closes nothing
        rc = call(plan, rows.ctypes.data)
        assert rc == _lib.FXC_ERR_UNSUPPORTED
        with pytest.raises(NotImplementedError, match="3 or more antennas"):
            _lib.check(rc, plan._h)
        with pytest.raises(NotImplementedError):
            plan.solve_gains(rows[:, :1])


def test_solve_gains_leaves_the_rows_alone(plan_mod, torch):
    from effex_amd import synth
    n_ant, nchan = 3, 64
    x = torch.from_numpy(synth.synth_iq(31, 6, n_ant, nchan * 20)).cuda()
    with plan_mod.FxPlan(n_ant, nchan, 4, nchan * 20) as plan:
        before = plan.fx_rows(x)
        keep = before.cpu().numpy()
        plan.solve_gains(before, interval=4)
        assert np.array_equal(before.cpu().numpy(), keep)
        assert np.array_equal(plan.fx_rows(x).cpu().numpy(), keep)
        plan.fx_accumulate(x)
        plan.solve_gains(keep)
        integ = plan.finalize("SPECTRUM")
        plan.fx_accumulate(x)
        assert np.array_equal(plan.finalize("SPECTRUM"), integ)
