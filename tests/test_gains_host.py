"""Gain solve (include/fxcorr.h fxc_solve_gains, FxPlan.solve_gains / set_gains), the parts that need no GPU: the declaration,
the exported and bound symbol, the call without a plan, the compiled kernels of k_gains.h, and the float64 restatement of the
definition (gains_ref.py) -- the reference tests/test_gpu_gains.py holds the library to has to recover injected gains itself,
from model rows and from samples through the oracle."""
import json
import os
import re

import numpy as np
import pytest

import fx_oracle
import gains_ref
from effex_amd import _lib
from effex_amd.plan import gain_tables, rot_tables
from effex_amd.window import design_window
from test_isa_hazards import asm_listing, kernel_resources, needs_hipcc  # noqa: F401  (the module's listing fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fxcorr.h")
BOUNDS = os.path.join(ROOT, "tests", "golden", "gains_bounds.json")
BW, FC = 2.4e6, 1.4204e9


def test_header_declares_solve_gains():
    text = open(HEADER).read()
    assert re.search(r"int fxc_solve_gains\(fxc_plan\* plan, const void\* rows, int64_t n_chunks, int mem_kind, int64_t interval, "
                     r"int ref, int iters,\s+double\* gains_re_im /\* \[n_int\]\[n_ant\]\[nchan\] complex128[^/]*\*/,\s+"
                     r"double\* step\s+/\* \[n_int\]\[nchan\], may be NULL \*/\);", text)
    assert "#define FXC_VERSION 106" in text           # fxc_info does not grow: the version stays
    assert "need not have unit modulus" in text        # fxc_set_rot_ant says that 1 / g_a is a legitimate table


def test_solve_gains_is_exported_and_bound():
    handle = _lib.load()
    assert "fxc_solve_gains" in _lib.SIGNATURES
    assert handle.fxc_solve_gains is not None
    assert handle.fxc_version() == 106


def test_call_without_a_plan_is_an_argument_error():
    handle = _lib.load()
    rows = np.zeros((4, 3, 64), dtype=np.complex64)
    g, s = np.full((3, 64), -7.0 + 0j), np.full(64, -7.0)
    rc = handle.fxc_solve_gains(None, rows.ctypes.data, 4, _lib.FXC_MEM_HOST, 0, 0, 10, g.ctypes.data, s.ctypes.data)
    assert rc == _lib.FXC_ERR_ARG
    assert (g == -7.0).all() and (s == -7.0).all()


@needs_hipcc
def test_gains_kernels_compile_without_scratch(asm_listing):  # noqa: F811
    res = kernel_resources(asm_listing)
    for kernel in ("gains_average_kernel", "gains_solve_kernel"):
        hits = {name: r for name, r in res.items() if re.search(r"{}{}".format(len(kernel), kernel), name)}
        assert len(hits) == 1, (kernel, sorted(hits))
        vgprs, _, _, scratch, _ = next(iter(hits.values()))
        assert scratch == 0 and vgprs <= 128, (kernel, vgprs, scratch)


# -- the restatement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ant", [8, 16, 64])
def test_restatement_recovers_the_truth(n_ant):
    """Noiseless rows g_a conj(g_b): after 60 iterations every gain within 1e-9 relative of the truth rotated to the reference and
    step < 1e-9 -- a condition with room (a run of this definition gave at most 2.3e-12 / 5.5e-13 at 8 antennas, 1e-15 above)."""
    rng = np.random.default_rng(7000 + n_ant)
    nchan = 256 if n_ant < 64 else 32
    for draw in range(10 if n_ant < 64 else 2):
        g = gains_ref.draw_gains(n_ant, nchan, rng)
        rows = gains_ref.model_rows(g, 1, dtype=np.complex128)
        for ref in (0, n_ant // 2):
            got, step = gains_ref.solve_rows(rows, n_ant, ref=ref, iters=60)
            want = gains_ref.rotate_to_ref(g, ref)
            rel = (np.abs(got[0] - want) / np.abs(want)).max()
            print("n_ant %d draw %d ref %d: rel %.3g step %.3g" % (n_ant, draw, ref, rel, step.max()))
            assert got.shape == (1, n_ant, nchan) and step.shape == (1, nchan)
            assert rel < 1e-9 and step.max() < 1e-9
            assert (got[0, ref].imag == 0).all() and (got[0, ref].real > 0).all()


@pytest.mark.parametrize("n_ant", [3, 4, 5])
def test_few_antennas_converge_slowly_but_converge(n_ant):
    """3 .. 5 antennas: the same iteration is slow (1.2e-2 relative after 60 iterations at 3 antennas), so no truth recovery is
    asserted -- only that step after 60 iterations is below step after 10."""
    rng = np.random.default_rng(7100 + n_ant)
    g = gains_ref.draw_gains(n_ant, 256, rng)
    rows = gains_ref.model_rows(g, 1, dtype=np.complex128)
    step10 = gains_ref.solve_rows(rows, n_ant, iters=10)[1]
    step60 = gains_ref.solve_rows(rows, n_ant, iters=60)[1]
    print("n_ant %d: step after 10 %.3g, after 60 %.3g" % (n_ant, step10.max(), step60.max()))
    assert step60.max() < step10.max()


def test_an_all_zero_bin_gives_zero_gains():
    rng = np.random.default_rng(7200)
    rows = gains_ref.model_rows(gains_ref.draw_gains(8, 16, rng), 3, rng, sigma=0.1)
    rows[:, :, 5] = 0
    for iters in (1, 2, 60):
        g, step = gains_ref.solve_rows(rows, 8, ref=3, iters=iters)
        assert np.isfinite(g).all() and np.isfinite(step).all()
        assert (g[0, :, 5] == 0).all() and step[0, 5] == 0
        assert (g[0, :, 4] != 0).all()


def test_intervals():
    """10 chunks in intervals of 4: three solutions, the last over 2 chunks, each the solve of its own chunks alone"""
    assert gains_ref.intervals(10, 4) == [(0, 4), (4, 8), (8, 10)]
    assert gains_ref.intervals(10, 0) == [(0, 10)] and gains_ref.intervals(3, 7) == [(0, 3)]
    rng = np.random.default_rng(7300)
    rows = gains_ref.model_rows(gains_ref.draw_gains(8, 32, rng), 10, rng, sigma=0.2)
    g, step = gains_ref.solve_rows(rows, 8, interval=4, ref=1, iters=20)
    assert g.shape == (3, 8, 32) and step.shape == (3, 32)
    for s, (c0, c1) in enumerate([(0, 4), (4, 8), (8, 10)]):
        one_g, one_step = gains_ref.solve_rows(rows[c0:c1], 8, ref=1, iters=20)
        assert np.array_equal(g[s], one_g[0]) and np.array_equal(step[s], one_step[0])
    assert not np.array_equal(g[2], g[0])
    # auto rows behind the cross rows are not read; a 2-D array is one chunk
    with_autos = np.concatenate([rows, np.full((10, 8, 32), 9.0, np.complex64)], axis=1)
    assert np.array_equal(gains_ref.solve_rows(with_autos, 8, interval=4, ref=1, iters=20)[0], g)
    assert np.array_equal(gains_ref.solve_rows(rows[0], 8, iters=5)[0], gains_ref.solve_rows(rows[:1], 8, iters=5)[0])


def test_average_adds_in_chunk_order():
    """the sum is the plain float64 loop over the chunks: order matters in the last bit, and the restatement keeps it"""
    rng = np.random.default_rng(7400)
    rows = (rng.standard_normal((9, 3, 8)) + 1j * rng.standard_normal((9, 3, 8))).astype(np.complex64) * 10.0 ** rng.uniform(-3, 3, (9, 1, 1))
    m = gains_ref.average(rows, 3)
    acc = 0.0
    for c in range(9):
        acc = acc + float(rows[c, 1, 2].real)
    assert m[2, 0, 2].real == acc / 9.0 and m[2, 2, 0] == np.conj(m[2, 0, 2]) and m[2, 1, 1] == 0


def test_gain_tables_flatten_the_model_rows():
    """set_gains' table math: ifftshift(1 / g) times the rot tables; r_a conj(r_b) applied to the rows of the same gains (under
    the same delays) gives 1 for every baseline and bin"""
    n_ant, nchan = 6, 64
    rng = np.random.default_rng(7500)
    g = gains_ref.draw_gains(n_ant, nchan, rng)
    delays = rng.uniform(-2e-6, 2e-6, n_ant)
    plain = gain_tables(g, n_ant, nchan)
    assert plain.dtype == np.complex128 and plain.shape == (n_ant, nchan)
    assert np.array_equal(plain, np.fft.ifftshift(1.0 / g, axes=1))
    both = gain_tables(g, n_ant, nchan, delays, BW, FC)
    assert np.array_equal(both, np.fft.ifftshift(1.0 / g, axes=1) * rot_tables(nchan, BW, FC, delays))
    rows = gains_ref.model_rows(g, 2, dtype=np.complex128)
    flat = gains_ref.apply_tables(rows, plain, n_ant)
    assert np.abs(flat - 1.0).max() < 1e-12
    # rows still carrying the delays' phase slopes: the rot part of the tables takes them out
    rot = np.fft.fftshift(rot_tables(nchan, BW, FC, delays), axes=1)
    slopes = np.stack([np.conj(rot[a]) * rot[b] for a, b in gains_ref.pairs(n_ant)])
    assert np.abs(gains_ref.apply_tables(rows * slopes[None], both, n_ant) - 1.0).max() < 1e-12
    # a dead channel stays zero
    g[2, 7] = 0
    dead = gain_tables(g, n_ant, nchan)
    assert np.isfinite(dead).all() and np.fft.fftshift(dead, axes=1)[2, 7] == 0
    with pytest.raises(ValueError):
        gain_tables(g[:, :32], n_ant, nchan)
    with pytest.raises(ValueError):
        gain_tables(g, n_ant, nchan, delays)


# -- from samples -------------------------------------------------------------------------------------------------------------
SAMPLE_ANT = 4
SAMPLE_SEEDS = tuple(range(8))
SAMPLE_REFS = (0, 2)


def oracle_rows(x, nchan):
    """the cross rows of every chunk of x [n_chunks, n_ant, num_samp] as the correlator writes them (no rot), complex64"""
    window = design_window(4, nchan)
    return np.stack([fx_oracle.fx_integrate(x[c:c + 1], nchan, window) for c in range(x.shape[0])]).astype(np.complex64)


def sample_errors():
    """{(seed, ref): max_a |estimate - c_a conj(c_ref) / |c_ref|^2|} of the restatement on the seeded draws"""
    out = {}
    for seed in SAMPLE_SEEDS:
        x, c = gains_ref.samples(SAMPLE_ANT, seed)
        rows = oracle_rows(x, gains_ref.SAMPLE_NCHAN)
        for ref in SAMPLE_REFS:
            g, _ = gains_ref.solve_rows(rows, SAMPLE_ANT, ref=ref, iters=gains_ref.SAMPLE_ITERS)
            out[(seed, ref)] = float(np.abs(gains_ref.scalar_ratios(g[0], ref) - gains_ref.true_ratios(c, ref)).max())
    return out


def test_restatement_recovers_the_scalars_from_samples():
    """x_a = c_a s + n_a through the oracle's F and X stages, 4 antennas x 64 channels, 32 chunks of 128 spectra (4096 spectra
    per bin, 32 bins in the inner half: the estimate is determined to about 1e-4): the ratios c_a / c_ref come back within B.
    B (tests/golden/gains_bounds.json, written by tools/gains_measure.py --bounds) is three times the largest error the
    restatement showed over these 16 seeded draws; the GPU test holds the library to the same B on the same inputs."""
    rec = json.load(open(BOUNDS))
    assert rec["bound"] == pytest.approx(3.0 * rec["observed"])
    errors = sample_errors()
    for key, err in sorted(errors.items()):
        print("seed %d ref %d: error %.3g (B %.3g)" % (key + (err, rec["bound"])))
    assert max(errors.values()) <= rec["bound"]
    assert max(errors.values()) == pytest.approx(rec["observed"], rel=0.05)       # the recorded figure is of this computation
