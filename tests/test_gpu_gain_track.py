"""Gain track on the GPU (include/fxcorr.h fxc_set_track_gains): under a delay track chunk t takes the gains of solution
s(t) = clamp((t - first_chunk) // interval, 0, n_solutions - 1), and antenna a's table becomes phasor_a(t) * ifftshift(1 / g_a).

Oracle: gain_track_ref.py, the float64 restatement -- the oracle of tests/test_gpu_tracking.py with rot[a] * q[s(t)][a] in place
of rot[a].  Bounds: TOL_VIS / TOL_CONT of the largest magnitude, the ceilings the project states; the tables have a derived
bound (test_gain_track_tables); the closure test holds to three times the figure the CPU restatement reaches on the same samples
(tests/golden/gain_track_bounds.json, written by tools/gain_track_measure.py --bounds)."""
import json
import os

import numpy as np
import pytest

import gain_track_ref
import gains_ref
from effex_amd import _lib, synth
from effex_amd.window import design_window

pytestmark = pytest.mark.gpu

from tolerances import TOL_CONT, TOL_VIS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS = os.path.join(ROOT, "tests", "golden", "gain_track_bounds.json")
BW = 2.4e6
FREQ = 1.42e9


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def plan_mod(torch):
    from effex_amd import plan
    return plan


def rel_err(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def track_of(n_ant):
    """distinct delays up to 2e-5 s and distinct rates, antenna 0 included (tests/test_gpu_tracking.py)"""
    a = np.arange(n_ant)
    tau0 = 2e-5 * ((3 * a * a) % 17 + 0.25 * a) / 17.0 - 3e-6
    rate = 1e-9 * ((5 * a) % 7 - 2.5)
    return tau0, rate


def draw(n_solutions, n_ant, nchan, seed):
    rng = np.random.default_rng(seed)
    return np.stack([gains_ref.draw_gains(n_ant, nchan, rng) for _ in range(n_solutions)])


def make_plan(plan_mod, n_ant, nchan, num_samp, path, autos=False):
    ntaps = 4
    window = design_window(ntaps, nchan)
    return plan_mod.FxPlan(n_ant, nchan, ntaps, num_samp, window=window, path=path, autos=autos), window


def exported(plan):
    sums = plan.new_sums()
    plan.acc_export(sums)
    plan.acc_reset()
    return host(sums).copy()


# -- 1. the tables ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ant,nchan", [(2, 4096), (3, 1000), (12, 256), (3, 125), (2, 1)])
def test_gain_track_tables(plan_mod, torch, n_ant, nchan):
    """track_tables(t) against numpy's rot_tables(tau0 + t rate) * ifftshift(1 / g[s(t)]).  The phasor's components are within
    B = 4 pi |f_k tau| 2^-52 + 8 * 2^-52 of numpy's (test_track_tables); each component of the product is a sum of two products
    of a phasor component with a component of q, and |qx| + |qy| <= sqrt(2) |q|; the inverse's and the product's own roundings
    cost a few 2^-52 on each side, which 2^-48 covers: the bound per component is sqrt(2) |q| (B + 2^-48)."""
    tau0, rate = track_of(n_ant)
    tau0, rate = 0.5 * tau0, 2.5e-3 * rate         # |tau0| <= 7.4e-6 s, |rate| x 1e6 chunks <= 1.13e-5 s: within 2e-5 s
    freqs = np.fft.fftfreq(nchan, d=1.0 / BW) + FREQ
    g = draw(3, n_ant, nchan, 1000 * n_ant + nchan)
    times = (0, 9, 10, 11, 12, 15, 16, 1000, 999999)
    with plan_mod.FxPlan(n_ant, nchan, 4, max(nchan, 16) * 8) as plan:
        plan.set_delay_track(tau0, rate, BW, FREQ)
        plain = {t: plan.track_tables(t) for t in times}
        assert plan.track_gains_info() == (0, 0, 0)
        plan.set_track_gains(g, interval=2, first_chunk=10)
        assert plan.track_gains_info() == (3, 2, 10)
        for t in times:
            s = gain_track_ref.solution_index(t, 3, 2, 10)
            assert s == {0: 0, 9: 0, 10: 0, 11: 0, 12: 1, 15: 2, 16: 2, 1000: 2, 999999: 2}[t]
            got = plan.track_tables(t)
            tau = tau0 + t * rate
            assert np.abs(tau).max() <= 2e-5
            q = np.fft.ifftshift(1.0 / g[s], axes=1)
            want = plan_mod.rot_tables(nchan, BW, FREQ, tau) * q
            bound = np.sqrt(2.0) * np.abs(q) * (4 * np.pi * np.abs(freqs[None, :] * tau[:, None]) * 2.0 ** -52 + 8 * 2.0 ** -52 + 2.0 ** -48)
            err = np.maximum(np.abs(got.real - want.real), np.abs(got.imag - want.imag))
            print("tables n_ant %d nchan %d t %d solution %d: worst component error %.3g, largest error / bound %.3f"
                  % (n_ant, nchan, t, s, err.max(), (err / bound).max()))
            assert (err <= bound).all()
            # the package's numpy form states the same tables
            form = plan_mod.gain_track_tables(g, 2, 10, t, tau0, rate, BW, FREQ)
            assert (np.maximum(np.abs(got.real - form.real), np.abs(got.imag - form.imag)) <= bound).all()
        plan.set_track_gains(np.ones((3, n_ant, nchan)), interval=2, first_chunk=10)
        for t in times:
            assert np.array_equal(plan.track_tables(t), plain[t]), t
        plan.set_track_gains(np.ones((n_ant, nchan)))          # one solution, interval 0: every chunk
        assert plan.track_gains_info() == (1, 0, 0)
        for t in times:
            assert np.array_equal(plan.track_tables(t), plain[t]), t
        assert plan.track_chunk == 0           # reading tables does not move the counter


# -- 2. rows and integration against the oracle --------------------------------------------------------------------------------
ROUTES = [  # n_ant, nchan, num_samp, path, autos
    (2, 4096, 4096 * 6, "fused", False), (2, 1000, 1000 * 8 + 3, None, False), (2, 8192, 8192 * 5, None, False),
    (2, 1, 4096, None, False), (3, 1024, 1024 * 8, None, True), (8, 4096, 4096 * 4, "fused", False), (12, 1024, 1024 * 6, None, False)]
N_CHUNKS, T0, G_FIRST, G_INTERVAL = 6, 9, 10, 2     # chunk 9 clamped to solution 0, 10-11 on 0, 12-13 on 1, 14 clamped to 1


@pytest.mark.parametrize("n_ant,nchan,num_samp,path,autos", ROUTES)
def test_rows_and_integration_match_the_oracle(plan_mod, torch, n_ant, nchan, num_samp, path, autos):
    assert [gain_track_ref.solution_index(T0 + c, 2, G_INTERVAL, G_FIRST) for c in range(N_CHUNKS)] == [0, 0, 0, 1, 1, 1]
    x_np = synth.synth_iq(21, N_CHUNKS, n_ant, num_samp, delays=np.arange(n_ant) % 5)
    x = torch.from_numpy(x_np).cuda()
    tau0, rate = track_of(n_ant)
    g = draw(2, n_ant, nchan, 77 + n_ant)
    plan, window = make_plan(plan_mod, n_ant, nchan, num_samp, path, autos)
    ref = gain_track_ref.oracle(x_np, nchan, window, tau0, rate, T0, BW, FREQ, g, G_INTERVAL, G_FIRST, autos)
    with plan:
        plan.set_delay_track(tau0, rate, BW, FREQ, first_chunk=T0)
        plain = host(plan.fx_rows(x, "SPECTRUM"))
        plan.track_seek(T0)
        plan.set_track_gains(g, interval=G_INTERVAL, first_chunk=G_FIRST)
        assert plan.track_chunk == T0                   # the gains leave the counter alone
        rows = host(plan.fx_rows(x, "SPECTRUM"))
        assert plan.track_chunk == T0 + N_CHUNKS
        assert rows.shape == ref.shape
        err = rel_err(rows, ref)
        print("rows against the oracle: %.3g; against the rows without gains: %.3g" % (err, rel_err(rows, plain)))
        assert err < TOL_VIS
        plan.track_seek(T0)
        cont = host(plan.fx_rows(x, "CONTINUUM", BW))
        assert rel_err(cont, ref.mean(axis=-1) / BW) < TOL_CONT
        if autos:
            assert np.array_equal(rows[:, -n_ant:], plain[:, -n_ant:])
        # integration
        plan.track_seek(T0)
        plan.fx_accumulate(x)
        assert plan.track_chunk == T0 + N_CHUNKS
        mean_rows = rows.astype(np.complex128).mean(axis=0)
        integ = plan.finalize("SPECTRUM", reset=False)
        err = rel_err(integ, mean_rows)
        print("tracked integration against the mean of the tracked rows: %.3g" % err)
        assert err < 1e-6
        assert rel_err(integ, ref.mean(axis=0)) < TOL_VIS
        integ_c = plan.finalize("CONTINUUM", BW)
        assert rel_err(integ_c, ref.mean(axis=0).mean(axis=-1) / BW) < TOL_CONT
        if autos:
            assert (np.asarray(integ)[-n_ant:].imag == 0).all()


# -- 3. unit gains are the plain track ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ant,nchan,num_samp,path", [(2, 4096, 4096 * 6, "fused"), (3, 1024, 1024 * 8, None)])
def test_unit_gains_are_the_plain_track(plan_mod, torch, n_ant, nchan, num_samp, path):
    x = torch.from_numpy(synth.synth_iq(31, 4, n_ant, num_samp)).cuda()
    tau0, rate = track_of(n_ant)
    plan, _ = make_plan(plan_mod, n_ant, nchan, num_samp, path)
    with plan:
        plan.set_delay_track(tau0, rate, BW, FREQ, first_chunk=5)
        rows = host(plan.fx_rows(x, "SPECTRUM"))
        plan.track_seek(5)
        plan.fx_accumulate(x)
        sums = exported(plan)
        plan.set_track_gains(np.ones((2, n_ant, nchan)), interval=2, first_chunk=5)
        plan.track_seek(5)
        assert np.array_equal(host(plan.fx_rows(x, "SPECTRUM")), rows)
        plan.track_seek(5)
        plan.fx_accumulate(x)
        assert np.array_equal(exported(plan), sums)


# -- 4. batching is invisible ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ant,nchan,num_samp,path", [(2, 4096, 4096 * 6, "fused"), (3, 1024, 1024 * 8, None)])
def test_rows_do_not_depend_on_batching(plan_mod, torch, n_ant, nchan, num_samp, path):
    """6 chunks, 3 solutions of 2 chunks from the first chunk on: cuts 1, 3, 5 fall inside an interval, 2 and 4 on a boundary"""
    n_chunks, t0 = 6, 50
    x_np = synth.synth_iq(41, n_chunks, n_ant, num_samp)
    x = torch.from_numpy(x_np).cuda()
    tau0, rate = track_of(n_ant)
    g = draw(3, n_ant, nchan, 5)
    plan, _ = make_plan(plan_mod, n_ant, nchan, num_samp, path)
    with plan:
        plan.set_delay_track(tau0, rate, BW, FREQ, first_chunk=t0)
        plan.set_track_gains(g, interval=2, first_chunk=t0)
        whole = host(plan.fx_rows(x, "SPECTRUM"))
        assert not np.array_equal(whole[1], whole[2])
        for cut in range(1, n_chunks):
            plan.track_seek(t0)
            split = np.concatenate([host(plan.fx_rows(x[:cut], "SPECTRUM")), host(plan.fx_rows(x[cut:], "SPECTRUM"))])
            assert np.array_equal(split, whole), cut
        plan.track_seek(t0)
        single = np.concatenate([host(plan.fx_rows(x[c:c + 1], "SPECTRUM")) for c in range(n_chunks)])
        assert plan.track_chunk == t0 + n_chunks
        assert np.array_equal(single, whole)
        plan.track_seek(t0)
        with plan_mod.FxPipeline(plan, 2, depth=2, mode="SPECTRUM") as pipe:
            piped = []
            for c in range(0, n_chunks, 2):
                pipe.push(x_np[c:c + 2])
                piped.append(pipe.pop())
        assert plan.track_chunk == t0 + n_chunks
        assert np.array_equal(np.concatenate(piped), whole)
        # the accumulator: one call and pieces
        plan.track_seek(t0)
        plan.fx_accumulate(x)
        a = exported(plan)
        for pieces in ((1, 3), (2, 4), (3, 5)):
            plan.track_seek(t0)
            for lo, hi in zip((0,) + pieces, pieces + (n_chunks,)):
                plan.fx_accumulate(x[lo:hi])
            assert plan.track_chunk == t0 + n_chunks
            assert np.array_equal(exported(plan), a), pieces


# -- 5. rate 0 with one solution against the static plan ---------------------------------------------------------------------
def test_rate_zero_with_one_solution_is_set_gains(plan_mod, torch):
    """set_gains(g, tau, bw, fc) forms its tables with numpy, the track on the device: agreement within TOL_VIS, no bit claim"""
    n_ant, nchan, num_samp = 4, 256, 256 * 16
    x = torch.from_numpy(synth.synth_iq(51, 3, n_ant, num_samp)).cuda()
    tau0, _ = track_of(n_ant)
    g = draw(1, n_ant, nchan, 6)
    plan, _ = make_plan(plan_mod, n_ant, nchan, num_samp, None)
    with plan:
        plan.set_gains(g[0], tau0, BW, FREQ)
        rows_s = host(plan.fx_rows(x, "SPECTRUM"))
        plan.fx_accumulate(x)
        int_s = plan.finalize("SPECTRUM")
        plan.set_delay_track(tau0, np.zeros(n_ant), BW, FREQ, first_chunk=77)
        plan.set_track_gains(g[0])
        rows_t = host(plan.fx_rows(x, "SPECTRUM"))
        plan.fx_accumulate(x)
        int_t = plan.finalize("SPECTRUM")
    print("rate 0, one solution against set_gains: rows %.3g, integration %.3g of max|vis|" % (rel_err(rows_t, rows_s), rel_err(int_t, int_s)))
    assert rel_err(rows_t, rows_s) < TOL_VIS and rel_err(int_t, int_s) < TOL_VIS


# -- 6. two ranks on one GPU -------------------------------------------------------------------------------------------------
def test_two_ranks_with_seek_add_up_to_the_single_plan(plan_mod, torch):
    """the ranks' ranges 0-2 and 3-5 cut inside the interval of chunks 2-3"""
    n_ant, nchan, num_samp, n_chunks = 3, 1024, 1024 * 8, 6
    x = torch.from_numpy(synth.synth_iq(61, n_chunks, n_ant, num_samp)).cuda()
    tau0, rate = track_of(n_ant)
    g = draw(3, n_ant, nchan, 7)
    sums = []
    for lo, hi in ((0, n_chunks), (0, 3), (3, n_chunks)):
        plan, _ = make_plan(plan_mod, n_ant, nchan, num_samp, None)
        with plan:
            plan.set_delay_track(tau0, rate, BW, FREQ)
            plan.set_track_gains(g, interval=2)
            plan.track_seek(lo)
            plan.fx_accumulate(x[lo:hi])
            sums.append(exported(plan))
    plan, _ = make_plan(plan_mod, n_ant, nchan, num_samp, None)
    with plan:
        plan.set_delay_track(tau0, rate, BW, FREQ)
        single = plan.finalize_sums(torch.from_numpy(sums[0]).cuda(), "SPECTRUM")
        both = plan.finalize_sums(torch.from_numpy(sums[1] + sums[2]).cuda(), "SPECTRUM")
    assert rel_err(both, single) < 1e-12


# -- 7. a dead channel stays zero --------------------------------------------------------------------------------------------
def test_dead_channel(plan_mod, torch):
    n_ant, nchan, num_samp, n_chunks = 3, 1024, 1024 * 8, 4
    x = torch.from_numpy(synth.synth_iq(71, n_chunks, n_ant, num_samp)).cuda()
    tau0, rate = track_of(n_ant)
    g = draw(2, n_ant, nchan, 8)
    bins = np.array([0, 3, 511, 512, 1023])
    dead = g.copy()
    dead[1, 1, bins] = 0                          # solution 1, antenna 1
    plan, _ = make_plan(plan_mod, n_ant, nchan, num_samp, None)
    with plan:
        plan.set_delay_track(tau0, rate, BW, FREQ)
        plan.set_track_gains(g, interval=2)
        alive = host(plan.fx_rows(x, "SPECTRUM"))
        plan.set_track_gains(dead, interval=2)
        plan.track_seek(0)
        rows = host(plan.fx_rows(x, "SPECTRUM"))
    hit = np.zeros(rows.shape, bool)
    for row in (0, 2):                            # baselines (0,1) and (1,2); (0,2) is row 1
        hit[np.ix_([2, 3], [row], bins)] = True
    assert (alive[hit] != 0).all()
    assert (rows[hit] == 0).all()
    assert np.array_equal(rows[~hit], alive[~hit])


# -- 8. closure from samples ---------------------------------------------------------------------------------------------------
def closure_case(plan_mod, torch):
    """track -> rows -> solve per 16 chunks -> gains under the track -> rows again (gain_track_ref.closure_samples)"""
    n_ant, nchan, interval = gain_track_ref.CLOSURE_ANT, gains_ref.SAMPLE_NCHAN, gain_track_ref.CLOSURE_INTERVAL
    x_np = gain_track_ref.closure_samples()
    x = torch.from_numpy(x_np).cuda()
    tau0, rate = gain_track_ref.closure_track()
    with plan_mod.FxPlan(n_ant, nchan, 4, x_np.shape[2], window=design_window(4, nchan)) as plan:
        n_base = plan.n_baselines
        plan.set_delay_track(tau0, rate, 1.0, gain_track_ref.CLOSURE_F)
        rows = plan.fx_rows(x)
        g, step = plan.solve_gains(rows, interval=interval, iters=gains_ref.SAMPLE_ITERS)
        assert g.shape == (2, n_ant, nchan)
        plan.set_track_gains(g, interval=interval)
        plan.track_seek(0)
        flat = host(plan.fx_rows(x))
        plan.set_track_gains(g[0])
        plan.track_seek(0)
        first_only = host(plan.fx_rows(x))
    return {"flat": gain_track_ref.interval_figure(flat, n_base), "step": float(step.max()),
            "no_gains": gain_track_ref.interval_figure(host(rows), n_base),
            "first_solution_only": gain_track_ref.interval_figure(first_only, n_base)}


def test_closure_from_samples(plan_mod, torch):
    """Two calibrator scans with different gains under fringes that the track stops: the solved gains, applied interval by
    interval under the track, make the mean of every interval's rows 1 within three times the CPU restatement's figure."""
    cpu = gain_track_ref.closure_cpu()
    print("cpu", json.dumps(cpu))
    assert cpu["untracked_mean_0_7"] < 0.5 and cpu["no_gains"] > 0.1         # the test's conditions, on the CPU oracle
    rec = json.load(open(BOUNDS))
    assert rec["bound"] == pytest.approx(3.0 * rec["observed"]) and cpu["flat"] == pytest.approx(rec["observed"], rel=0.05)
    f = closure_case(plan_mod, torch)
    print("gpu", json.dumps(f), "bound", rec["bound"])
    assert f["flat"] <= rec["bound"], (f, rec["bound"])
    assert f["step"] < 1e-12
    assert f["first_solution_only"] > 0.1                                    # the second solution matters


# -- 9. state and argument rules ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ant,nchan,num_samp", [(3, 1024, 1024 * 8), (2, 4096, 4096 * 6)])
def test_state_and_argument_rules(plan_mod, torch, n_ant, nchan, num_samp):
    x = torch.from_numpy(synth.synth_iq(81, 3, n_ant, num_samp)).cuda()
    tau0, rate = track_of(n_ant)
    g = draw(2, n_ant, nchan, 9)
    static = plan_mod.rot_tables(nchan, BW, FREQ, tau0)
    plan, _ = make_plan(plan_mod, n_ant, nchan, num_samp, None)

    def raw(gains, n_solutions, interval, first_chunk):
        keep = None if gains is None else np.ascontiguousarray(gains, dtype=np.complex128)      # (alive until the call returns)
        return plan._lib.fxc_set_track_gains(plan._h, None if keep is None else keep.ctypes.data, n_solutions, interval, first_chunk)

    def rows_now(seek=0):
        plan.track_seek(seek)
        return host(plan.fx_rows(x, "SPECTRUM"))

    with plan:
        # no track
        assert raw(g, 2, 2, 0) == _lib.FXC_ERR_STATE
        assert raw(None, 0, 0, 0) == _lib.FXC_ERR_STATE
        with pytest.raises(_lib.FxcError) as e:
            plan.track_gains_info()
        assert e.value.status == _lib.FXC_ERR_STATE
        plan.set_rot_ant(static)
        want_static = host(plan.fx_rows(x, "SPECTRUM"))
        plan.set_delay_track(tau0, rate, BW, FREQ)
        assert plan.track_gains_info() == (0, 0, 0)
        plain = rows_now()
        plan.set_track_gains(g, interval=2, first_chunk=1)
        assert plan.track_gains_info() == (2, 2, 1)
        with_g = rows_now()
        assert not np.array_equal(with_g, plain)
        # every argument error; a failed call keeps the gain track
        bad = g.copy()
        bad[1, 0, 5] = np.nan
        inf = g.copy()
        inf[0, n_ant - 1, 0] = complex(0.0, np.inf)
        tiny, huge = g.copy(), g.copy()
        tiny[1, 1, 7] = 1e-151
        huge[1, 1, 7] = complex(0.0, -1e151)
        for args in ((None, 2, 2, 0), (g, -1, 2, 0), (g, 2, 0, 0), (g, 2, -1, 0), (g, 1, -1, 0), (g, 2, 2, -1), (bad, 2, 2, 0),
                     (inf, 2, 2, 0), (tiny, 2, 2, 0), (huge, 2, 2, 0)):
            rc = raw(*args)
            assert rc == _lib.FXC_ERR_ARG, args[1:]
            with pytest.raises(ValueError):          # (FXC_ERR_ARG, as effex_amd/_lib.py maps it)
                _lib.check(rc, plan._h)
            assert plan.track_gains_info() == (2, 2, 1)
        assert np.array_equal(rows_now(), with_g)
        for wrong in (g[:, :, :nchan // 2], g[:, :1], np.ones(nchan)):
            with pytest.raises(ValueError):
                plan.set_track_gains(wrong, interval=2)
        # the limits themselves and a zero gain are fine
        edge = g.copy()
        edge[0, 0, 0], edge[0, 0, 1], edge[0, 0, 2] = 1e-150, 1e150, 0.0
        assert raw(edge, 2, 2, 1) == _lib.FXC_OK
        plan.set_track_gains(g, interval=2, first_chunk=1)
        # chunks in the accumulator
        plan.track_seek(0)
        plan.fx_accumulate(x)
        assert raw(g[::-1], 2, 1, 0) == _lib.FXC_ERR_STATE
        assert raw(None, 0, 0, 0) == _lib.FXC_ERR_STATE
        assert plan.track_gains_info() == (2, 2, 1)
        plan.acc_reset()
        assert np.array_equal(rows_now(), with_g)
        # an open pipe
        with plan_mod.FxPipeline(plan, 1, depth=2, mode="SPECTRUM"):
            assert raw(g[::-1], 2, 1, 0) == _lib.FXC_ERR_STATE
            assert plan.track_gains_info() == (2, 2, 1)
        assert np.array_equal(rows_now(), with_g)
        # solve_gains and fringe_fit neither read nor change the gain track
        dev_rows = plan.fx_rows(x, "SPECTRUM")
        plan.fringe_fit(dev_rows, BW, FREQ)
        if n_ant > 2:
            plan.solve_gains(dev_rows, interval=2)
        assert plan.track_gains_info() == (2, 2, 1)
        assert np.array_equal(rows_now(), with_g)
        # None removes the gains and keeps the track
        plan.set_track_gains(None)
        assert plan.track_gains_info() == (0, 0, 0)
        assert np.array_equal(rows_now(), plain)
        # a new track drops the gains
        plan.set_track_gains(g, interval=2, first_chunk=1)
        plan.set_delay_track(tau0, rate, BW, FREQ)
        assert plan.track_gains_info() == (0, 0, 0)
        assert np.array_equal(rows_now(), plain)
        # set_rot_ant ends both; the gains do not come back with a new track
        plan.set_track_gains(g, interval=2, first_chunk=1)
        plan.set_rot_ant(static)
        with pytest.raises(_lib.FxcError) as e:
            plan.track_gains_info()
        assert e.value.status == _lib.FXC_ERR_STATE
        assert raw(g, 2, 2, 1) == _lib.FXC_ERR_STATE
        assert np.array_equal(host(plan.fx_rows(x, "SPECTRUM")), want_static)
        plan.set_delay_track(tau0, rate, BW, FREQ)
        assert plan.track_gains_info() == (0, 0, 0)
        assert np.array_equal(rows_now(), plain)
