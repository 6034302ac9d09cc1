"""Weighted gain solve (include/fxcorr.h fxc_solve_gains_weighted, FxPlan.solve_gains(weights=, model=)), the parts that need no
GPU: the declaration, the exported and bound symbol, the call without a plan, the compiled kernels' resources, and the float64
restatement of the definition (gains_weighted_ref.py) -- the reference tests/test_gpu_gains_weighted.py holds the library to has
to reduce to the unweighted restatement, recover injected gains under flags and a model, ignore what flagged samples hold, and
close on samples with damage, where the unweighted solve does not."""
import json
import os
import re

import numpy as np
import pytest

import gains_ref
import gains_weighted_ref as wref
from effex_amd import _lib
from effex_amd.plan import offset_source_model, rot_tables
from test_gains_host import oracle_rows
from test_isa_hazards import asm_listing, kernel_resources, needs_hipcc  # noqa: F401  (the module's listing fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fxcorr.h")
BOUNDS = os.path.join(ROOT, "tests", "golden", "gains_weighted_bounds.json")
BW, FC = 2.4e6, 1.4204e9


# -- declaration and binding ----------------------------------------------------------------------------------------------------
def test_header_declares_solve_gains_weighted():
    text = open(HEADER).read()
    assert re.search(r"int fxc_solve_gains_weighted\(fxc_plan\* plan, const void\* rows, const void\* weights, int64_t n_chunks, "
                     r"int mem_kind,\s+const void\* model, int64_t n_model, int64_t interval, int ref, int iters,\s+"
                     r"double\* gains_re_im /\* \[n_int\]\[n_ant\]\[nchan\] complex128[^/]*\*/,\s+"
                     r"double\* step\s+/\* \[n_int\]\[nchan\], may be NULL \*/\);", text)
    assert "#define FXC_VERSION 106" in text
    assert "weights or flags, two antennas" not in text      # fxc_solve_gains points at the new call instead
    assert "A sample counts iff" in text and "power of two changes no output bit" in text


def test_solve_gains_weighted_is_exported_and_bound():
    handle = _lib.load()
    assert "fxc_solve_gains_weighted" in _lib.SIGNATURES
    assert handle.fxc_solve_gains_weighted is not None
    assert handle.fxc_version() == 106


def test_call_without_a_plan_is_an_argument_error():
    handle = _lib.load()
    rows = np.zeros((4, 3, 64), dtype=np.complex64)
    weights = np.ones((4, 3, 64), dtype=np.float32)
    g, s = np.full((3, 64), -7.0 + 0j), np.full(64, -7.0)
    rc = handle.fxc_solve_gains_weighted(None, rows.ctypes.data, weights.ctypes.data, 4, _lib.FXC_MEM_HOST, None, 0, 0, 0, 10,
                                         g.ctypes.data, s.ctypes.data)
    assert rc == _lib.FXC_ERR_ARG
    assert (g == -7.0).all() and (s == -7.0).all()


@needs_hipcc
def test_weighted_gains_kernels_compile_without_scratch(asm_listing):  # noqa: F811
    res = kernel_resources(asm_listing)
    for kernel in ("gains_weighted_average_kernel", "gains_weighted_solve_kernel"):
        hits = {name: r for name, r in res.items() if re.search(r"{}{}".format(len(kernel), kernel), name)}
        assert len(hits) == 1, (kernel, sorted(hits))
        vgprs, _, _, scratch, _ = next(iter(hits.values()))
        print(kernel, "VGPRs", vgprs, "scratch", scratch)
        assert scratch == 0 and vgprs <= 128, (kernel, vgprs, scratch)


# -- the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ant", [3, 8, 17])
def test_restatement_reduces_to_the_unweighted_one(n_ant):
    """weights None and model None, and weights of ones with a model of ones: gains_ref.solve_rows' arrays bit for bit"""
    rng = np.random.default_rng(8000 + n_ant)
    nchan, n_chunks = 24, 7
    rows = gains_ref.model_rows(gains_ref.draw_gains(n_ant, nchan, rng), n_chunks, rng, sigma=0.1)
    rows[:, :, 3] = 0                                   # a dead bin stays dead in both
    nb = len(gains_ref.pairs(n_ant))
    for interval in (0, 5):
        for ref in (0, n_ant // 2):
            want_g, want_s = gains_ref.solve_rows(rows, n_ant, interval=interval, ref=ref, iters=21)
            n_int = want_g.shape[0]
            for weights, model in ((None, None), (np.ones((n_chunks, nb, nchan), np.float32), np.ones((nb, nchan), np.complex64)),
                                   (np.ones((n_chunks, nb, nchan), np.float32), None), (None, np.ones((n_int, nb, nchan)))):
                got_g, got_s = wref.solve_rows(rows, n_ant, interval=interval, ref=ref, iters=21, weights=weights, model=model)
                assert np.array_equal(got_g, want_g) and np.array_equal(got_s, want_s)
                assert (got_g[:, :, 3] == 0).all()


TRUTH_CHUNKS = 7
TRUTH_ITERS = 60


def truth_case(n_ant, nchan, ref, iters=TRUTH_ITERS, seed=None):
    rng = np.random.default_rng(8100 + n_ant if seed is None else seed)
    g, model, rows, weights = wref.damaged_case(n_ant, nchan, TRUTH_CHUNKS, rng)
    got, step = wref.solve_rows(rows, n_ant, ref=ref, iters=iters, weights=weights, model=model)
    return g, got[0], step[0]


@pytest.mark.parametrize("n_ant,nchan", [(16, 32), (64, 8)])
def test_restatement_recovers_the_truth_under_flags_and_a_model(n_ant, nchan):
    """Noiseless rows g_a conj(g_b) M_ab in complex64, weights 0.25 .. 4, 20 % of the samples flagged and overwritten with 1e6 (1 +
    i), antenna 1 dead, bin 5 flagged: every live gain within 1e-6 relative of the truth rotated to the reference (a run gave 3e-8
    and 1.3e-8, the complex64 rounding of rows and model), antenna 1 and bin 5 exactly 0, everything finite."""
    live_ant = [a for a in range(n_ant) if a != wref.DEAD_ANT]
    live_bin = [k for k in range(nchan) if k != wref.DEAD_BIN]
    for ref in (0, n_ant // 2):
        g, got, step = truth_case(n_ant, nchan, ref)
        assert np.isfinite(got).all() and np.isfinite(step).all()
        assert (got[wref.DEAD_ANT] == 0).all() and (got[:, wref.DEAD_BIN] == 0).all() and step[wref.DEAD_BIN] == 0
        want = gains_ref.rotate_to_ref(g, ref)
        sel = np.ix_(live_ant, live_bin)
        rel = (np.abs(got[sel] - want[sel]) / np.abs(want[sel])).max()
        print("n_ant %d ref %d: rel %.3g step %.3g" % (n_ant, ref, rel, step.max()))
        assert rel <= 1e-6
        assert (got[ref, live_bin].imag == 0).all() and (got[ref, live_bin].real > 0).all()
        if n_ant == 16:
            assert step.max() <= 1e-12


@pytest.mark.parametrize("n_ant", [3, 4, 5, 8])
def test_few_antennas_converge_slowly_but_converge(n_ant):
    """3 .. 8 antennas (antenna 1 dead): step after 60 iterations is below step after 10 (4 antennas 6.9e-3 -> 3.4e-4 in a run of
    this definition, 5 antennas 7.1e-3 -> 8.1e-5, 8 antennas 1.2e-3 -> 4.6e-10).  At 3 antennas the dead antenna leaves ONE
    baseline, whose start value is already the solution: step is 3.4e-16 after 10 iterations and after 60, rounding both times, so
    "below" cannot hold there.  Where the iteration has converged to rounding by iteration 10 the condition is therefore that it
    stays there (step after 60 not above step after 10, both <= 1e-12) and that the products g_a conj(g_b) of the live antennas are
    the truth's within 1e-6 (one baseline fixes the product, not the two gains)."""
    g, got10, step10 = truth_case(n_ant, 32, 0, iters=10)
    _, got60, step60 = truth_case(n_ant, 32, 0, iters=60)
    print("n_ant %d: step after 10 %.3g, after 60 %.3g" % (n_ant, step10.max(), step60.max()))
    assert np.isfinite(step60).all() and np.isfinite(got60).all()
    if step10.max() <= 1e-12:
        assert step60.max() <= step10.max()
        live_bin = [k for k in range(32) if k != wref.DEAD_BIN]
        for a, b in gains_ref.pairs(n_ant):
            if wref.DEAD_ANT not in (a, b):
                fit, truth = (got60[a] * np.conj(got60[b]))[live_bin], (g[a] * np.conj(g[b]))[live_bin]
                assert (np.abs(fit - truth) / np.abs(truth)).max() <= 1e-6, (a, b)
    else:
        assert step60.max() < step10.max()


def test_flagged_values_and_weight_scale_change_no_bit():
    n_ant, nchan = 8, 16
    rng = np.random.default_rng(8200)
    _, model, rows, weights = wref.damaged_case(n_ant, nchan, TRUTH_CHUNKS, rng, sigma=0.1)
    flagged = weights == 0
    assert flagged.any() and not flagged.all()
    want = wref.solve_rows(rows, n_ant, interval=5, ref=2, iters=20, weights=weights, model=model)
    for value in (np.nan, np.inf, 1e30):
        other = rows.copy()
        other[flagged] = np.complex64(complex(value, -value))
        got = wref.solve_rows(other, n_ant, interval=5, ref=2, iters=20, weights=weights, model=model)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), value
    for value in (-1.0, np.nan):
        other = weights.copy()
        other[flagged] = value
        got = wref.solve_rows(rows, n_ant, interval=5, ref=2, iters=20, weights=other, model=model)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), value
    got = wref.solve_rows(rows, n_ant, interval=5, ref=2, iters=20, weights=weights * np.float32(4), model=model)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# -- closure from samples with damage -------------------------------------------------------------------------------------------------
_DAMAGE = {}


def damage_rows(seed):
    """(rows through the oracle, c, weights) of wref.damaged_samples(seed), computed once per process"""
    if seed not in _DAMAGE:
        x, c, weights = wref.damaged_samples(seed)
        _DAMAGE[seed] = (oracle_rows(x, gains_ref.SAMPLE_NCHAN), c, weights)
    return _DAMAGE[seed]


def damage_errors():
    """{(seed, ref): (weighted error, unweighted error)}: max_a |estimate - c_a conj(c_ref) / |c_ref|^2| of the weighted restatement
    and of gains_ref.solve_rows on the same rows"""
    out = {}
    for seed in wref.DAMAGE_SEEDS:
        rows, c, weights = damage_rows(seed)
        for ref in wref.DAMAGE_REFS:
            truth = gains_ref.true_ratios(c, ref)
            g, _ = wref.solve_rows(rows, wref.DAMAGE_ANT, ref=ref, iters=gains_ref.SAMPLE_ITERS, weights=weights)
            plain, _ = gains_ref.solve_rows(rows, wref.DAMAGE_ANT, ref=ref, iters=gains_ref.SAMPLE_ITERS)
            out[(seed, ref)] = (float(np.abs(wref.scalar_ratios(g[0], ref) - truth).max()),
                                float(np.abs(wref.scalar_ratios(plain[0], ref) - truth).max()))
    return out


def test_weights_recover_the_scalars_from_damaged_samples():
    """gains_ref.samples at 8 antennas with antenna 3 replaced by noise in chunks 8 .. 15 and a tone in bin 20 of antennas 1 and 5,
    through the oracle's F and X stages; weights 0 on exactly that.  The ratios c_a / c_ref come back within B (tests/golden/
    gains_weighted_bounds.json, written by tools/gains_weighted_measure.py --bounds: three times the restatement's largest error
    over the 8 seeded draws; that error is the difference in source power between antenna 3's 24 chunks and the others' 32, not
    rounding), and the unweighted restatement on the same rows errs by more than 10 B in every draw."""
    rec = json.load(open(BOUNDS))
    assert rec["bound"] == pytest.approx(3.0 * rec["observed"])
    errors = damage_errors()
    for key, (err, plain) in sorted(errors.items()):
        print("seed %d ref %d: weighted %.3g, unweighted %.3g (B %.3g)" % (key + (err, plain, rec["bound"])))
    worst = max(err for err, _ in errors.values())
    assert worst <= rec["bound"]
    assert worst == pytest.approx(rec["observed"], rel=0.05)       # the recorded figure is of this computation
    assert min(plain for _, plain in errors.values()) > 10.0 * rec["bound"]


# -- the model of an offset source -----------------------------------------------------------------------------------------------
def test_offset_source_model_takes_the_slopes_out():
    """A noise-free common source, antennas 1 .. 3 delayed by 1, 2, 3 whole samples (4 antennas x 64 channels), rows through the
    oracle: solved with offset_source_model of those delays, the phase of g_a conj(g_ref) has no slope across the inner half
    band -- below 1 % of the slope the same solve shows without the model.  This fixes the model's sign."""
    n_ant, nchan, n_spec, n_chunks = 4, 64, 128, 2
    rng = np.random.default_rng(8300)
    n = nchan * n_spec
    s = (rng.standard_normal((n_chunks, n + 3)) + 1j * rng.standard_normal((n_chunks, n + 3))) / np.sqrt(2.0)
    lag = np.arange(n_ant)
    x = np.stack([s[:, 3 - k:3 - k + n] for k in lag], axis=1).astype(np.complex64)       # x_a[t] = s[t - a]
    rows = oracle_rows(x, nchan)
    delays = lag / BW
    model = offset_source_model(n_ant, nchan, BW, FC, delays)
    assert model.shape == (n_ant * (n_ant - 1) // 2, nchan) and model.dtype == np.complex64
    assert np.allclose(np.abs(model), 1.0, atol=1e-6)
    assert np.allclose(np.abs(offset_source_model(n_ant, nchan, BW, FC, delays, flux=2.5)), 2.5, atol=1e-5)
    rot = np.fft.fftshift(rot_tables(nchan, BW, FC, delays), axes=1)
    assert np.array_equal(model[2], (np.conj(rot[0]) * rot[3]).astype(np.complex64))      # baseline (0, 3)
    inner = np.arange(nchan // 4, nchan - nchan // 4)

    def slopes(gains):
        out = []
        for a in range(1, n_ant):
            phase = np.unwrap(np.angle(gains[a, inner] * np.conj(gains[0, inner])))
            out.append(np.polyfit(inner.astype(np.float64), phase, 1)[0])
        return np.array(out)

    bare = slopes(wref.solve_rows(rows, n_ant, iters=60)[0][0])
    with_model = slopes(wref.solve_rows(rows, n_ant, iters=60, model=model)[0][0])
    print("slopes without the model", bare, "with", with_model)
    assert np.allclose(np.abs(bare), 2.0 * np.pi * lag[1:] / nchan, rtol=0.05)
    assert (np.abs(with_model) < 0.01 * np.abs(bare)).all()
    with pytest.raises(ValueError):
        offset_source_model(n_ant, nchan, BW, FC, delays[:3])
