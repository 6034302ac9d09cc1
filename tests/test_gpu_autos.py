"""Autocorrelation products on the GPU (include/fxcorr.h fxc_products): plans with autos against the float64 oracle on every
route, rot, byte / complex128 input, the integration plumbing, the state rules and the drop-in's files.

Oracle of an auto row: fftshift(mean_i |f_a[i, k]|^2) over the spectra of fx_oracle.spectrometer_poly; CONTINUUM: its mean
over the bins / bandwidth (the cross formula, effex.py:523-524).  Cross rows: fx_oracle.fx_integrate.  Bounds: TOL_VIS of
the largest magnitude of each group (cross rows, auto rows)."""
import numpy as np
import pytest

import fx_oracle
from effex_amd import _lib, synth
from effex_amd.window import design_window

pytestmark = pytest.mark.gpu

from tolerances import TOL_VIS

BW = 2.4e6


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


def oracle(x, nchan, window, rot=None):
    """x [n_chunks, A, num_samp] -> per-chunk cross [C, NB, nchan], autos [C, A, nchan]; integrated cross [NB, nchan],
    autos [A, nchan] (all fft-shifted SPECTRUM values, rot applied to the cross rows only)."""
    x = np.asarray(x)
    n_chunks, n_ant, _ = x.shape
    ntaps = len(window) // nchan
    pairs = [(a, b) for a in range(n_ant) for b in range(a + 1, n_ant)]
    rot = np.ones(nchan) if rot is None else rot
    cross = np.zeros((n_chunks, len(pairs), nchan), np.complex128)
    autos = np.zeros((n_chunks, n_ant, nchan), np.complex128)
    for c in range(n_chunks):
        specs = [fx_oracle.spectrometer_poly(x[c, a], ntaps, nchan, window) for a in range(n_ant)]
        for p, (a, b) in enumerate(pairs):
            cross[c, p] = np.fft.fftshift((specs[a] * np.conj(specs[b] * rot)).mean(axis=0))
        for a in range(n_ant):
            autos[c, a] = np.fft.fftshift((np.abs(specs[a]) ** 2).mean(axis=0))
    return cross, autos, cross.mean(axis=0), autos.mean(axis=0)


def assert_autos_exact(autos):
    autos = np.asarray(autos)
    assert np.all(autos.imag == 0.0)
    assert np.all(autos.real >= 0.0)


# 2 antennas at 4096 / 4 on the fused path take the fused kernel's AUTOS variant (one pass): 7 chunks are all frame ranges over the
# workgroups (leading-part rows), 300 whole chunks dealt round-robin plus a tail; every other shape the F stage + X-engine route
SHAPES = [  # n_ant, nchan, ntaps, num_samp, n_chunks, path
    (2, 4096, 4, 4096 * 6, 7, "fused"), (2, 4096, 4, 4096 * 3, 300, "fused"), (2, 4096, 4, 4096 * 5 + 17, 1, "fused"), (2, 2048, 4, 2048 * 9 + 5, 11, "tiled"),
    (2, 2048, 32, 2048 * 40, 3, "tiled"), (2, 8192, 4, 8192 * 5, 4, "tiled"), (2, 256, 4, 256 * 20, 5, "tiled"),
    (2, 16, 4, 16 * 70, 5, "tiled"), (2, 1, 4, 5000, 6, "stream"), (2, 1000, 4, 1000 * 8 + 3, 4, None),
    (2, 6000, 4, 6000 * 5, 3, None), (3, 8, 4, 8 * 20, 5, "generic"), (3, 4096, 4, 4096 * 4, 3, None),
    (4, 4096, 4, 4096 * 4, 3, "fused"), (8, 4096, 4, 4096 * 4, 3, "fused"), (3, 64, 4, 64 * 20, 5, "tiled")]


@pytest.mark.parametrize("n_ant,nchan,ntaps,num_samp,n_chunks,path", SHAPES)
def test_autos_match_the_oracle(plan_mod, torch, n_ant, nchan, ntaps, num_samp, n_chunks, path):
    """fx_rows and fx_accumulate + finalize of a plan with autos, SPECTRUM and CONTINUUM: cross and auto rows."""
    x_np = synth.synth_iq(5, n_chunks, n_ant, num_samp, delays=np.arange(n_ant) % 5)
    x = torch.from_numpy(x_np).cuda()
    window = design_window(ntaps, nchan)
    cross, autos, cross_i, autos_i = oracle(x_np, nchan, window)
    nb = n_ant * (n_ant - 1) // 2
    with plan_mod.FxPlan(n_ant, nchan, ntaps, num_samp, window=window, path=path, autos=True) as plan:
        assert plan.autos and plan.n_rows == nb + n_ant and plan.n_baselines == nb
        rows = host(plan.fx_rows(x, "SPECTRUM"))
        assert rows.shape == (n_chunks, nb + n_ant, nchan)
        assert rel_err(rows[:, :nb], cross) < TOL_VIS
        assert rel_err(rows[:, nb:], autos) < TOL_VIS
        assert_autos_exact(rows[:, nb:])
        cont = host(plan.fx_rows(x, "CONTINUUM", BW))
        assert cont.shape == (n_chunks, nb + n_ant)
        assert rel_err(cont[:, :nb], cross.mean(axis=-1) / BW) < TOL_VIS
        assert rel_err(cont[:, nb:], autos.mean(axis=-1) / BW) < TOL_VIS
        assert_autos_exact(cont[:, nb:])
        plan.fx_accumulate(x)
        integ = plan.finalize("SPECTRUM", reset=False)
        assert integ.shape == (nb + n_ant, nchan)
        assert rel_err(integ[:nb], cross_i) < TOL_VIS
        assert rel_err(integ[nb:], autos_i) < TOL_VIS
        assert_autos_exact(integ[nb:])
        integ_c = plan.finalize("CONTINUUM", BW)
        assert rel_err(integ_c[:nb], cross_i.mean(axis=-1) / BW) < TOL_VIS
        assert rel_err(integ_c[nb:], autos_i.mean(axis=-1) / BW) < TOL_VIS
        assert_autos_exact(integ_c[nb:])


@pytest.mark.parametrize("n_ant,nchan,num_samp,path", [(2, 4096, 4096 * 5, "fused"), (2, 1000, 1000 * 6, None),
                                                       (3, 64, 64 * 20, "tiled")])
def test_rot_leaves_the_autos_alone(plan_mod, torch, n_ant, nchan, num_samp, path):
    n_chunks = 3
    x_np = synth.synth_iq(9, n_chunks, n_ant, num_samp, delays=np.arange(n_ant) % 5)
    x = torch.from_numpy(x_np).cuda()
    window = design_window(4, nchan)
    rot = fx_oracle.rot_table(nchan, BW, 1.4204e9, 7.3e-7)
    cross, autos, cross_i, autos_i = oracle(x_np, nchan, window, rot)
    nb = n_ant * (n_ant - 1) // 2
    with plan_mod.FxPlan(n_ant, nchan, 4, num_samp, window=window, path=path, autos=True) as plan:
        unit_rows = host(plan.fx_rows(x, "SPECTRUM"))
        unit_cont = host(plan.fx_rows(x, "CONTINUUM", BW))
        plan.fx_accumulate(x)
        unit_integ = plan.finalize("SPECTRUM")
        plan.set_rot(rot)
        rows = host(plan.fx_rows(x, "SPECTRUM"))
        cont = host(plan.fx_rows(x, "CONTINUUM", BW))
        plan.fx_accumulate(x)
        integ = plan.finalize("SPECTRUM")
    assert rel_err(rows[:, :nb], cross) < TOL_VIS
    assert rel_err(integ[:nb], cross_i) < TOL_VIS
    assert rel_err(cont[:, :nb], cross.mean(axis=-1) / BW) < TOL_VIS
    assert rel_err(unit_rows[:, :nb], cross) > 1e-3          # the rot really turned the cross rows
    assert np.array_equal(rows[:, nb:], unit_rows[:, nb:])
    assert np.array_equal(cont[:, nb:], unit_cont[:, nb:])
    assert np.array_equal(integ[nb:], unit_integ[nb:])
    for a in (rows[:, nb:], cont[:, nb:], integ[nb:]):
        assert_autos_exact(a)


@pytest.mark.parametrize("nchan,num_samp,path", [(4096, 4096 * 5, "fused"), (1000, 1000 * 6, None), (256, 256 * 20, "tiled")])
def test_byte_and_complex128_input(plan_mod, torch, nchan, num_samp, path):
    """uint8 with and without the DC removal, complex128 with it: the oracle chain u8_to_complex -> remove_dc -> channelize."""
    n_chunks, n_ant = 3, 2
    rng = np.random.default_rng(3)
    u8 = rng.integers(0, 256, size=(n_chunks, n_ant, num_samp, 2), dtype=np.uint8)
    u8[:, 1, 3:] = u8[:, 0, :-3]                               # correlated: antenna 1 = antenna 0 delayed by 3
    u8[:, :, :, 0] = np.clip(u8[:, :, :, 0].astype(int) + 9, 0, 255).astype(np.uint8)      # and a DC offset
    window = design_window(4, nchan)
    nb = 1
    samples = fx_oracle.u8_to_complex(u8)
    with plan_mod.FxPlan(n_ant, nchan, 4, num_samp, window=window, path=path, autos=True) as plan:
        for dc in (False, True):
            ref_in = np.array([[fx_oracle.remove_dc(s) if dc else s for s in chunk] for chunk in samples])
            cross, autos, cross_i, autos_i = oracle(ref_in, nchan, window)
            rows = host(plan.fx_rows_u8(torch.from_numpy(u8).cuda(), "SPECTRUM", remove_dc=dc))
            assert rel_err(rows[:, :nb], cross) < TOL_VIS
            assert rel_err(rows[:, nb:], autos) < TOL_VIS
            plan.fx_accumulate_u8(torch.from_numpy(u8).cuda(), remove_dc=dc)
            integ = plan.finalize("SPECTRUM")
            assert rel_err(integ[:nb], cross_i) < TOL_VIS
            assert rel_err(integ[nb:], autos_i) < TOL_VIS
        x128 = synth.synth_iq(4, n_chunks, n_ant, num_samp).astype(np.complex128) + (0.3 - 0.2j)
        ref_in = np.array([[fx_oracle.remove_dc(s) for s in chunk] for chunk in x128])
        cross, autos, _, _ = oracle(ref_in, nchan, window)
        rows = host(plan.fx_rows(x128, "SPECTRUM", remove_dc=True, c128=True))
        assert rel_err(rows[:, :nb], cross) < TOL_VIS
        assert rel_err(rows[:, nb:], autos) < TOL_VIS
        assert_autos_exact(rows[:, nb:])


@pytest.mark.parametrize("n_ant,nchan,num_samp,path", [(2, 4096, 4096 * 4, "fused"), (4, 512, 512 * 10, "tiled")])
def test_integration_plumbing(plan_mod, torch, n_ant, nchan, num_samp, path):
    """finalize_async = finalize; acc_export -> finalize_sums = finalize; reduce on one rank = finalize; a pipe = fx_rows."""
    x = torch.from_numpy(synth.synth_iq(13, 5, n_ant, num_samp, delays=np.arange(n_ant) % 5)).cuda()
    window = design_window(4, nchan)
    with plan_mod.FxPlan(n_ant, nchan, 4, num_samp, window=window, path=path, autos=True) as plan:
        rows_n = plan.n_rows
        for mode in ("SPECTRUM", "CONTINUUM"):
            plan.fx_accumulate(x)
            blocking = plan.finalize(mode, BW)
            plan.fx_accumulate(x)
            plan.finalize_async(mode, BW)
            assert np.array_equal(plan.finalize_wait(), blocking)
            plan.fx_accumulate(x)
            sums = plan.new_sums()
            assert sums.numel() == rows_n * nchan + 1
            plan.acc_export(sums)
            assert np.array_equal(plan.finalize_sums(sums, mode, BW), blocking)
            plan.reduce(None)
            assert np.array_equal(plan.finalize_sums(None, mode, BW), blocking)
            plan.acc_reset()
        want = host(plan.fx_rows(x, "SPECTRUM"))
        with plan_mod.FxPipeline(plan, 5, depth=2, mode="SPECTRUM") as pipe:
            pipe.push(host(x))
            got = pipe.pop()
        assert got.shape == (5, rows_n, nchan)
        assert np.array_equal(got, want)


def test_set_products_state_rules(plan_mod, torch):
    num_samp, nchan = 4096 * 3, 4096
    x = torch.from_numpy(synth.synth_iq(17, 2, 2, num_samp)).cuda()
    with plan_mod.FxPlan(2, nchan, 4, num_samp) as plan:
        plain = host(plan.fx_rows(x, "SPECTRUM"))
        assert plain.shape == (2, 1, nchan)
        plan.fx_accumulate(x)
        with pytest.raises(_lib.FxcError) as e:
            plan.set_autos(True)
        assert e.value.status == _lib.FXC_ERR_STATE
        plan.finalize_async("SPECTRUM", reset=True)             # accumulator cleared, a result outstanding
        with pytest.raises(_lib.FxcError) as e:
            plan.set_autos(True)
        assert e.value.status == _lib.FXC_ERR_STATE
        plan.finalize_wait()
        with plan_mod.FxPipeline(plan, 2, depth=2) as pipe:
            with pytest.raises(_lib.FxcError) as e:
                plan.set_autos(True)
            assert e.value.status == _lib.FXC_ERR_STATE
            del pipe
        plan.set_autos(True)
        assert (plan.autos, plan.n_rows) == (True, 3)
        assert host(plan.fx_rows(x, "SPECTRUM")).shape == (2, 3, nchan)
        plan.fx_accumulate(x)
        assert plan.finalize("SPECTRUM").shape == (3, nchan)
        plan.set_autos(False)
        assert (plan.autos, plan.n_rows) == (False, 1)
        back = host(plan.fx_rows(x, "SPECTRUM"))
        assert back.shape == (2, 1, nchan) and np.array_equal(back, plain)
    with plan_mod.FxPlan(9, 64, 4, 64 * 20) as plan9:
        with pytest.raises(NotImplementedError):          # FXC_ERR_UNSUPPORTED (effex_amd._lib.check)
            plan9.set_autos(True)
        assert plan9._lib.fxc_set_products(plan9._h, _lib.FXC_PRODUCTS_CROSS_AUTO) == _lib.FXC_ERR_UNSUPPORTED
        assert (plan9.autos, plan9.n_rows) == (False, 36)


@pytest.mark.parametrize("mode,batch,fmt", [("SPECTRUM", 1, "csv"), ("SPECTRUM", 4, "bin"), ("TEST", 1, "csv"),
                                            ("CONTINUUM", 4, "csv"), ("TEST", 4, "bin")])
def test_dropin_writes_auto_files(tmp_path, torch, mode, batch, fmt):
    from effex_amd import rowsink
    from effex_amd.correlator import ArraySource, Correlator
    n_chunks, nbins, num_samp = 7, 256, 256 * 24
    x = synth.synth_iq(23, n_chunks, 2, num_samp)
    ext = ".csv" if fmt == "csv" else ".fxb"
    files = {}
    for autos in (False, True):
        path = str(tmp_path / ("vis_{}{}".format(int(autos), ext)))
        cor = Correlator(num_samp=num_samp, nbins=nbins, source=ArraySource(x), output_file=path, calibrate=False,
                         mode=mode, batch=batch, output_format=fmt, autos=autos)
        assert cor.run_state_machine() == n_chunks
        files[autos] = (path, cor)
    plain, with_autos = files[False][0], files[True][0]
    assert open(plain, "rb").read() == open(with_autos, "rb").read()
    window = design_window(4, nbins)
    ref_in = np.array([[fx_oracle.remove_dc(s) for s in chunk] for chunk in x])
    _, autos_ref, _, _ = oracle(ref_in, nbins, window)
    spectrum = mode == "SPECTRUM"
    for a in range(2):
        path = files[True][1].auto_file(a)
        if fmt == "bin":
            csv = path + ".csv"
            rowsink.to_csv(path, csv)
            path = csv
        if fmt == "csv":
            assert open(path).readline() == open(plain).readline()          # the same header line
        data = np.loadtxt(path, dtype=np.complex128, delimiter=",", skiprows=2 if spectrum else 1)
        ref = autos_ref[:, a] if spectrum else autos_ref[:, a].mean(axis=-1) / 2.4e6
        data = data.reshape(ref.shape)
        assert rel_err(data, ref) < TOL_VIS
        assert np.all(data.imag == 0.0)
    last = files[True][1].last_autos
    assert last.shape == ((2, nbins) if spectrum else (2,))


def test_dropin_run_task_and_integrate_expose_autos(torch):
    from effex_amd.correlator import ArraySource, Correlator
    nbins, num_samp = 512, 512 * 16
    x = synth.synth_iq(29, 3, 2, num_samp)
    window = design_window(4, nbins)
    cor = Correlator(num_samp=num_samp, nbins=nbins, source=ArraySource(x), calibrate=False, autos=True, remove_dc=False)
    cor._stage((x[0, 0], x[0, 1]))
    row = cor._run_task()
    assert row.shape == (nbins,)
    cross, autos, _, _ = oracle(x[:1], nbins, window)
    assert rel_err(row, cross[0, 0]) < TOL_VIS
    assert cor.last_autos.shape == (2, nbins)
    assert rel_err(cor.last_autos, autos[0]) < TOL_VIS
    integ = cor.integrate(torch.from_numpy(x).cuda())
    _, _, cross_i, autos_i = oracle(x, nbins, window)
    assert rel_err(integ, cross_i[0]) < TOL_VIS
    assert rel_err(cor.last_autos, autos_i) < TOL_VIS
    cor.close()


@pytest.mark.parametrize("batch", [1, 4])
def test_dropin_byte_source_writes_auto_files(tmp_path, torch, batch):
    """A receiver-byte source: the autos are those of the converted, de-meaned samples (u8_to_complex -> remove_dc)."""
    from effex_amd.correlator import ArraySource, Correlator
    n_chunks, nbins, num_samp = 6, 256, 256 * 24
    rng = np.random.default_rng(8)
    u8 = rng.integers(0, 256, size=(n_chunks, 2, num_samp, 2), dtype=np.uint8)
    u8[:, 1, 2:] = u8[:, 0, :-2]
    files = {}
    for autos in (False, True):
        path = str(tmp_path / "vis_{}.csv".format(int(autos)))
        cor = Correlator(num_samp=num_samp, nbins=nbins, source=ArraySource(u8), output_file=path, calibrate=False, batch=batch,
                         autos=autos)
        assert cor.run_state_machine() == n_chunks
        files[autos] = (path, cor)
    assert open(files[False][0], "rb").read() == open(files[True][0], "rb").read()
    ref_in = np.array([[fx_oracle.remove_dc(s) for s in chunk] for chunk in fx_oracle.u8_to_complex(u8)])
    _, autos_ref, _, _ = oracle(ref_in, nbins, design_window(4, nbins))
    for a in range(2):
        data = np.loadtxt(files[True][1].auto_file(a), dtype=np.complex128, delimiter=",", skiprows=2)
        assert rel_err(data, autos_ref[:, a]) < TOL_VIS
        assert np.all(data.imag == 0.0)
