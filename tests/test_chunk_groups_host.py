"""The cases of tests/chunk_group_cases.py claim what they should.  From the module's model of the group sizes alone, for devices
of 64, 128, 256 and 304 CUs: every pass of every case's long call has chunk groups of two chunks at least (three, in fact) even
if the device holds every workgroup the bound allows; its last group is shorter than the others for every group size the
device can choose; the input stays under 300 MB; in every matrix-core case a tile of kFT frames holds frames of two chunks, or --
one case, n_pts = kFT -- ends exactly where a chunk ends; the passes cases take three passes.  The constants the model restates
are the ones the sources state, the restated oracle is fx_oracle.fx_integrate, and a chunk left out of an integration moves the
oracle by ten ceilings of the device test's bound.  No GPU."""
import os
import re

import numpy as np
import pytest

import chunk_group_cases as cg
import fx_oracle
from effex_amd import synth
from tolerances import TOL_VIS

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "effex_amd", "csrc")
MFMA = [c for c in cg.CASES if c.kernel == "mfma"]


def source(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def test_the_cases_are_the_ones_the_issue_lists():
    ids = [c.id for c in cg.CASES]
    assert len(ids) == len(set(ids))
    plain = [c for c in cg.CASES if not c.passes]
    assert sorted(c.n_ant for c in plain if c.kernel == "mfma") == [9, 16, 17, 32, 33, 48, 49, 64]
    by_t = {}
    for c in MFMA:
        by_t.setdefault(cg.tiles(c), []).append(c)
    assert sorted(by_t) == [1, 2, 3, 4]
    # n_pts over {1, 3, kFT, kFT + 1, 2 kFT + 1}, every one of them taken
    kinds = set()
    for c in MFMA:
        ft = cg.k_ft(cg.tiles(c))
        names = {1: "1", 3: "3", ft: "kFT", ft + 1: "kFT+1", 2 * ft + 1: "2kFT+1"}
        assert c.n_pts in names, c.id
        kinds.add(names[c.n_pts])
    assert kinds == {"1", "3", "kFT", "kFT+1", "2kFT+1"}
    vec = [c for c in plain if c.kernel == "vector"]
    assert {c.n_ant for c in vec} >= {3, 5, 8} and {c.n_pts for c in vec} == {1, 3}
    assert [c.id for c in vec if c.path == "fused"] == ["vector-4x4096x3"] and cg.BY_ID["vector-4x4096x3"].ntaps == 4
    assert any(c.nchan == 32 for c in vec)
    autos = [c for c in plain if c.autos]
    assert sorted(c.n_ant for c in autos) == [2, 4] and all(c.kernel == "autos" for c in autos)
    assert (autos[0].nchan, autos[0].ntaps) != (4096, 4) or autos[0].n_ant != 2          # off the fused kernel
    assert sorted((c.kernel, c.n_ant) for c in cg.CASES if c.passes) == [("mfma", 9), ("vector", 3)]
    assert sorted(c.n_ant for c in cg.CASES if c.kernel == "block") == [9, 17]
    for c in cg.CASES:
        assert 2 <= c.ntaps <= 4 and c.n_pts <= 256 and cg.fused_unit(c) >= 4, c.id
        assert c.kernel in ("mfma", "vector", "autos", "block") and c.path in ("tiled", "fused"), c.id
        assert (c.kernel == "autos") == c.autos and (2 if c.autos else 3) <= c.n_ant <= (8 if c.kernel in ("vector", "autos") else 64), c.id
        assert c.kernel not in ("mfma", "block") or (c.n_ant > cg.X_BLOCK and c.nchan % cg.MFMA_COLUMN == 0), c.id
    assert any(c.tail for c in cg.CASES) and any(not c.tail for c in cg.CASES)
    with_rot = sum(bool(c.rot) for c in cg.CASES)
    assert abs(2 * with_rot - len(cg.CASES)) <= 3          # a rot table in about half of the cases


def test_the_models_constants_are_the_sources():
    finish, launch, build, xmfma, run = (source(n) for n in ("k_finish.h", "h_launch.h", "h_build.h", "k_xmfma.h", "h_run.h"))
    assert re.search(r"constexpr int kXThreads = %d;" % cg.X_THREADS, finish)
    assert re.search(r"constexpr int kXB = %d;" % cg.X_BLOCK, finish)
    assert re.search(r"kRowSpectra = %d\b" % cg.K_ROW_SPECTRA, launch)
    assert "std::min<int64_t>(kRowSpectra / std::max<int64_t>(1, p->n_pts), 64)" in launch          # fused_unit
    assert "std::max<int64_t>(1, std::min<int64_t>(unit, (nc + groups - 1) / groups))" in launch    # xengine_group
    assert "std::max<int64_t>(1, std::min<int64_t>(unit, (nc + groups - 1) / groups))" in run       # autos_group
    assert "per_cu = std::min(per_cu, 4 * std::min(8, 512 / regs));" in build and cg.ONE_WAVE_PER_CU == 4 * 8
    # the matrix-core kernel's tiles: frames per tile 8 / 4 / 4 / 4, rows of kCH + 1 = 17 complex, 34 KiB for the small tiles
    assert re.search(r"#define FXC_XMFMA_FT1 8\n#define FXC_XMFMA_FT2 4\n", xmfma)
    assert "kFT = T == 1 ? FXC_XMFMA_FT1 : (T == 2 ? FXC_XMFMA_FT2 : 4);" in xmfma
    assert "kPitch = kCH + 1;" in xmfma and "#define FXC_XMFMA_CH34 16" in xmfma
    assert "kLdsBytes = (2 * kTileCf > 256 * kPitch ? 2 * kTileCf : 256 * kPitch) * (int)sizeof(cf);" in xmfma
    assert "Small tiles: 34 KiB of LDS per workgroup" in xmfma
    assert [cg.k_ft(t) for t in (1, 2, 3, 4)] == [8, 4, 4, 4]
    assert [cg.mfma_lds_bytes(t) for t in (1, 2, 3, 4)] == [34 << 10, 34 << 10, 51 << 10, 68 << 10]
    assert [cg.LDS_PER_CU // cg.mfma_lds_bytes(t) for t in (1, 2, 3, 4)] == [4, 4, 3, 2]
    for c in cg.CASES:
        assert cg.per_cu_bound(c) == ({1: 4, 2: 4, 3: 3, 4: 2}[cg.tiles(c)] if c.kernel == "mfma" else 32), c.id
    c = cg.BY_ID
    assert [cg.cols(c[k]) for k in ("mfma-9x4096x3", "mfma-64x256x3", "vector-3x32x1", "vector-8x8192x1", "autos-2x2048x3",
                                    "block-9x2048x1", "block-17x1024x3")] == [256, 16, 1, 128, 32, 32 * 3, 16 * 6]
    assert [cg.fused_unit(c[k]) for k in ("mfma-16x512x17", "mfma-17x512x1", "vector-3x8192x3")] == [60, 64, 64]


@pytest.mark.parametrize("cu", cg.CU_COUNTS)
@pytest.mark.parametrize("case", cg.CASES, ids=lambda c: c.id)
def test_every_pass_has_groups_of_several_chunks_and_a_shorter_last_one(case, cu):
    unit = cg.fused_unit(case)
    lengths = cg.pass_lengths(case, cu)
    assert sum(lengths) == cg.call_chunks(case, cu) and cg.n_chunks(case, cu) == cg.SHORT + sum(lengths)
    assert len(lengths) >= 3 if case.passes else len(lengths) == 1, lengths
    for nc in lengths:
        assert nc >= 2 * cg.groups_max(case, cu) + 1 and nc > unit and nc < 65535, (nc, lengths)
        lo = cg.cg_min(case, cu, nc)
        assert 3 <= lo <= unit, (nc, lo)
        for cgs in range(lo, unit + 1):          # whatever the occupancy is: fewer resident workgroups, larger groups
            g = cg.group_lengths(nc, cgs)
            assert len(g) >= 2 and set(g[:-1]) == {cgs} and 0 < g[-1] < cgs and sum(g) == nc, (nc, cgs)
    # the first, short call groups differently: one chunk per row wherever a row's workgroups fit the device twice
    assert cg.SHORT < 3 <= min(cg.cg_min(case, cu, nc) for nc in lengths)
    assert cg.input_bytes(case, cu) < cg.INPUT_CAP and cg.input_bytes(case, cu) == cg.n_chunks(case, cu) * case.n_ant * cg.num_samp(case) * 8
    # a chunk left out moves the mean over the chunks by its share: five ceilings of the device test's bound at the least
    assert 1.0 / cg.n_chunks(case, cu) >= 5 * TOL_VIS.ceiling


@pytest.mark.parametrize("cu", cg.CU_COUNTS)
def test_a_tile_holds_frames_of_two_chunks_in_the_matrix_core_cases(cu):
    straddling = set()
    for case in MFMA:
        t = cg.tiles(case)
        ft = cg.k_ft(t)
        for nc in cg.pass_lengths(case, cu):
            for cgs in range(cg.cg_min(case, cu, nc), cg.fused_unit(case) + 1):
                fast, slow = cg.fast_and_slow(case, cgs)
                assert slow >= 1 and fast + slow == -(-case.n_pts * cgs // ft), (case.id, cgs)
                if case.n_pts % ft == 0:
                    # the one case whose chunks are whole tiles: every tile ends with its chunk, walk_i wraps at the tile's end
                    assert case.n_pts == ft and not cg.straddles(case, cgs) and fast == 0, case.id
                else:
                    assert cg.straddles(case, cgs), (case.id, cgs)
                    straddling.add(t)
                # 2 kFT + 1 frames a chunk: tiles at fixed strides between the ones that cross a boundary
                assert (fast > 0) == (case.n_pts > ft), (case.id, cgs, fast)
    assert straddling == {1, 2, 3, 4}
    assert [c.id for c in MFMA if c.n_pts % cg.k_ft(cg.tiles(c)) == 0] == ["mfma-32x512x4"]


def test_tile_walk_model_on_known_groups():
    c = cg.BY_ID
    assert cg.fast_and_slow(c["mfma-33x256x9"], 3) == (4, 3)        # 27 frames: per chunk two tiles inside, one across the boundary
    assert cg.fast_and_slow(c["mfma-17x512x1"], 5) == (0, 2)        # five chunks of one frame: four in the first tile
    assert cg.fast_and_slow(c["mfma-16x512x17"], 3) == (4, 3)       # 51 frames: tiles 2, 4 and 6 of seven cross a boundary or the end
    assert not cg.straddles(c["mfma-32x512x4"], 64) and cg.straddles(c["mfma-9x4096x3"], 2)
    assert cg.group_lengths(67, 17) == [17, 17, 17, 16] and cg.group_lengths(67, 3)[-1] == 1


@pytest.mark.parametrize("cu", cg.CU_COUNTS)
def test_passes_of_the_passes_cases(cu):
    for case in cg.CASES:
        if not case.passes:
            continue
        mb, cb, n = cg.pass_plan(case, cu)
        per = sum(cg.chunk_bytes(case))
        assert cb == (mb << 20) // per == cg.chunks_per_pass(case, mb << 20, n) and cg.is_prime(cb)
        lengths = cg.pass_lengths(case, cu)
        assert lengths == [cb, cb, n - 2 * cb] and cg.is_prime(lengths[-1]) and cg.pass_floor(case, cu) <= lengths[-1] < cb
        # the default workspace takes the same call in one pass, and a pass's workspace is the model's
        assert cg.chunks_per_pass(case, 12 << 30, n) == n
        spec, raw = cg.chunk_bytes(case)
        assert cg.workspace_bytes(case, cb) > cg.r256(cb * spec) + cg.r256(cb * raw)
    c = cg.BY_ID["vector-3x8192x1-passes"]
    assert cg.chunk_bytes(c) == (3 * 8192 * 8, 3 * 8192 * 8) and cg.pass_plan(c, 256) == (56, 149, 429)
    assert cg.workspace_bytes(c, 149) == 2 * 149 * 3 * 8192 * 8 + 32 * 3 * 8192 * 16


# ---- input and oracle ------------------------------------------------------------------------------------------------------------
def test_samples_are_synth_iq_chunks_with_a_delay_per_antenna():
    case = cg.BY_ID["vector-3x32x1"]
    x = cg._samples(case, 5)
    want = synth.synth_iq(cg.seed(case), 5, case.n_ant, cg.num_samp(case), delays=cg.delays(case.n_ant))
    assert x.dtype == np.complex64 and x.shape == (5, 3, 32) and not x.flags.writeable and np.array_equal(x, want)
    assert len(set(cg.delays(11))) == 11 and len(cg.delays(64)) == 64
    assert len({cg.seed(c) for c in cg.CASES}) == len(cg.CASES)
    for c0 in range(4):                     # chunks are distinct: a chunk read twice is another integration
        assert not np.array_equal(x[c0], x[c0 + 1])


def test_restated_oracle_is_fx_integrate():
    case = cg.BY_ID["mfma-17x512x1"]._replace(nchan=64, n_pts=5, tail=3)
    x = cg._samples(case, 4)
    win, rot = cg.window(case), cg.rot(case)
    assert rot is not None
    ref = fx_oracle.fx_integrate(x, case.nchan, win, rot=rot)
    allp = cg.pairs(case.n_ant)
    got, autos = cg.integrate_pairs(x, case.nchan, win, allp, rot, autos=True)
    assert cg.rel_err(got, ref) < 1e-13
    which = [(0, 16), (3, 4), (15, 16)]
    sub = cg.integrate_pairs(x, case.nchan, win, which, rot)
    assert cg.rel_err(sub, ref[[allp.index(p) for p in which]]) < 1e-13
    for a in (0, 16):                       # the autos as test_gpu_route_passes.py states them
        want = np.mean([np.fft.fftshift((np.abs(fx_oracle.spectrometer_poly(x[c, a], case.ntaps, case.nchan, win)) ** 2).mean(axis=0))
                        for c in range(4)], axis=0)
        assert cg.rel_err(autos[a], want) < 1e-13
    assert cg.oracle(cg.BY_ID["mfma-17x512x1"], 64)[1] is None


def test_oracle_subset_from_49_antennas():
    assert cg.oracle_pairs(cg.BY_ID["mfma-48x256x5"]) == cg.pairs(48)
    for name, n_ant in (("mfma-49x256x5", 49), ("mfma-64x256x3", 64)):
        sub = cg.oracle_pairs(cg.BY_ID[name])
        assert sub == sorted(set(sub)) and set(sub) <= set(cg.pairs(n_ant))
        for e in (0, 15, 16, 33, n_ant - 1):
            assert {(min(e, o), max(e, o)) for o in range(n_ant) if o != e} <= set(sub)
        assert {(a, b) for a, b in cg.pairs(n_ant) if a >= 48} <= set(sub)          # inside the last pair of tiles: (3, 3)
        assert {(a // 16, b // 16) for a, b in sub} == {(a // 16, b // 16) for a, b in cg.pairs(n_ant)}      # every pair of tiles
        assert len(sub) < len(cg.pairs(n_ant)) // 2


def test_a_lost_chunk_moves_the_oracle_ten_ceilings():
    """what the two mutations of the issue do, in float64: every group one chunk short, or the last (shorter) group's row not
    folded -- the sum over the remaining chunks still divided by all the frames"""
    case, cu = cg.BY_ID["mfma-17x512x1"], 64
    x = cg.samples(case, cu)
    n, nc = x.shape[0], cg.call_chunks(case, cu)
    win, which = cg.window(case), [(0, 1), (0, 16), (15, 16), (8, 12)]
    ref = cg.integrate_pairs(x, case.nchan, win, which, cg.rot(case))
    assert cg.rel_err(ref, cg.oracle(case, cu)[0][[cg.pairs(17).index(p) for p in which]]) < 1e-13
    cgs = cg.cg_min(case, cu, nc)
    groups = cg.group_lengths(nc, cgs)
    ends = np.cumsum(groups) + cg.SHORT
    for name, lost in (("a group's last chunk", [int(e) - 1 for e in ends if e - 1 >= cg.SHORT]), ("the last group", list(range(int(ends[-2]), n)))):
        keep = [c for c in range(n) if c not in lost]
        bad = cg.integrate_pairs(x[keep], case.nchan, win, which, cg.rot(case)) * (len(keep) / n)
        err, row = cg.worst_row(bad, ref)
        least = min(cg.worst_row(bad[r:r + 1], ref[r:r + 1])[0] for r in range(len(which)))
        assert least >= 10 * TOL_VIS.ceiling, (name, least, err, which[row])


def test_worst_row_scales_every_row_by_itself():
    ref = np.array([[1.0, 2.0], [100.0, 50.0]])
    got = ref + np.array([[0.0, 0.02], [0.5, 0.0]])
    err, row = cg.worst_row(got, ref)
    assert row == 0 and abs(err - 0.01) < 1e-12          # the global metric would say 0.5 / 100 of row 1
    assert np.isnan(cg.worst_row(np.array([[np.nan, 1.0]]), np.array([[1.0, 1.0]]))[0])
