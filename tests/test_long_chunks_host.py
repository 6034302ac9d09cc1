"""The device test of chunks of more than 1024 frames (test_gpu_long_chunks.py) can see what it is meant to see.  For every case
of ``long_chunk_cases.CASES`` and every wrong reading of the frame ranges, the chunk's tables and the auto rows -- a range's last
frame dropped, its first counted twice, the last range left out, the raw rows read group-major, a neighbouring chunk's tables, the
other solution's gains, a neighbouring baseline's tables, an auto row given a rot or taken from the antenna next to it -- the float64
oracle under the wrong reading differs from the oracle by at least ten times the ceiling the device test holds, in every group of
rows the reading touches (cross rows, auto rows), SPECTRUM and CONTINUUM, in the device test's own metric.  Also: the oracle is the
one gain_track_ref.py and test_gpu_tracking.py state, and the ranges are those of x_range.  No GPU."""
import numpy as np
import pytest

import gain_track_ref
import long_chunk_cases as lc
from tolerances import TOL_CONT, TOL_VIS

FACTOR = 10.0
CEILING = {"SPECTRUM": TOL_VIS.ceiling, "CONTINUUM": TOL_CONT.ceiling}


def test_ceilings_are_the_ones_the_issue_names():
    assert CEILING == {"SPECTRUM": 1e-5, "CONTINUUM": 1e-5}


def test_case_ids_are_unique_and_every_case_is_a_long_chunk():
    ids = [c.id for c in lc.CASES]
    assert len(ids) == len(set(ids))
    for c in lc.CASES:
        assert c.n_chunks >= 3 and c.n_pts > lc.K_ROW_SPECTRA and c.mod in lc.MODS, c
        assert c.n_ant > 2 or c.autos, c                     # two antennas without autos never reach the X-engines
        assert set(c.expect) <= {"path", "block", "lds_bytes", "specialised"} and "path" in c.expect, c
        assert set(c.env) <= {"FXC_WS_MB"}, c
    have = {(c.n_ant, c.nchan, c.n_pts, c.mod, c.autos) for c in lc.CASES if not c.env}
    for n_pts in (1027, 2051):
        for mod, autos in (("ant", False), ("track", False), ("gains", False), ("rot", True), ("ant", True), ("track", True), ("gains", True)):
            assert (3, 64, n_pts, mod, autos) in have
    for want in ((2, 64, 1027, "rot", True), (2, 64, 1027, "track", True), (3, 16, 1027, "track", True), (8, 128, 1027, "ant", True),
                 (8, 128, 1027, "track", False), (3, 512, 1027, "ant", False), (3, 512, 1027, "track", True), (4, 4096, 1027, "ant", False),
                 (4, 4096, 1027, "track", True), (3, 1000, 1027, "track", False), (3, 1000, 1027, "gains", False), (9, 64, 1027, "ant", False),
                 (9, 64, 1027, "track", False), (17, 64, 1027, "ant", False), (33, 64, 1027, "track", False), (49, 64, 1027, "ant", False)):
        assert want in have, want
    assert {(c.n_ant, c.nchan, c.n_pts, c.n_chunks, c.mod, c.autos) for c in lc.CASES if c.env} == \
        {(3, 16, 1027, 5, "track", True), (3, 16, 1027, 5, "ant", True)}


# ---- the ranges --------------------------------------------------------------------------------------------------------------
def x_range_as_the_kernel_states_it(n_pts, n_chunks, cg, n_ranges, block_y):
    """k_finish.h::x_range line by line -> (group, raw row, i0, i1)"""
    n_groups = (n_chunks + cg - 1) // cg
    grp = block_y // n_ranges
    rg = block_y - grp * n_ranges
    per = (n_pts + n_ranges - 1) // n_ranges
    i0 = rg * per if rg * per < n_pts else n_pts
    i1 = i0 + per if i0 + per < n_pts else n_pts
    return grp, rg * n_groups + grp, i0, i1


def test_range_lengths_are_the_ones_the_cases_claim():
    frame_ranges = lambda n_pts: min((n_pts + 1024 - 1) // 1024, 4096)          # h_launch.h::frame_ranges
    assert [frame_ranges(n) for n in (1024, 1025, 1027, 2048, 2049, 2051)] == [1, 2, 2, 2, 3, 3]
    for n_pts, want in ((1027, [(0, 514), (514, 1027)]), (2051, [(0, 684), (684, 1368), (1368, 2051)])):
        n = frame_ranges(n_pts)
        n_chunks = 3
        seen = [x_range_as_the_kernel_states_it(n_pts, n_chunks, 1, n, y) for y in range(n_chunks * n)]
        for y, (grp, row, i0, i1) in enumerate(seen):
            assert (grp, row) == (y // n, (y % n) * n_chunks + y // n)        # range-major rows
            assert (i0, i1) == want[y % n] == lc.x_range(n_pts, n, y % n)
        assert sorted(row for _, row, _, _ in seen) == list(range(n_chunks * n))
    assert [i1 - i0 for i0, i1 in lc.ranges(lc.BY_ID["wave-3x64x1027-ant"])] == [514, 513]
    assert [i1 - i0 for i0, i1 in lc.ranges(lc.BY_ID["wave-3x64x2051-ant"])] == [684, 684, 683]
    # the X-engine route off the powers of two: x_geometry's runs of 64 frames
    mixed = lc.BY_ID["mixed_xeng-3x1000x1027-track"]
    assert lc.n_ranges(mixed) == 17 and [i1 - i0 for i0, i1 in lc.ranges(mixed)] == [61] * 16 + [51]
    for c in lc.CASES:
        rg = lc.ranges(c)
        assert len(rg) > 1 and rg[0][0] == 0 and rg[-1][1] == c.n_pts and all(a[1] == b[0] for a, b in zip(rg, rg[1:])), c.id
        assert all(0 < i1 - i0 <= lc.K_ROW_SPECTRA for i0, i1 in rg), c.id
        assert any((i1 - i0) % 2 for i0, i1 in rg), c.id                       # an odd range: the one-spectrum tail of the kXU = 2 loop
        assert set(lc.loud_blocks(c)) == {0, c.n_pts - 1} | {i for i0, _ in rg[1:] for i in (i0 - 1, i0)}, c.id


def test_passes_of_the_passes_cases():
    for c in lc.CASES:
        if c.env:
            cb, spec, raw = lc.passes(c, 1 << 20)
            assert lc.passes(c) == (5, 5 * spec // 2, 5 * raw // 2)
            assert (cb, spec, raw) == (2, 2 * 3 * 1027 * 16 * 8, 2 * 6 * 16 * 8 * 2)
            assert [min(cb, c.n_chunks - c0) for c0 in range(0, c.n_chunks, cb)] == [2, 2, 1]


# ---- inputs and tables ---------------------------------------------------------------------------------------------------------
def test_samples_are_reproducible_loud_at_the_boundaries_and_have_no_tone():
    c = lc.BY_ID["wave-3x64x2051-track+autos"]
    x = lc.samples(c)
    assert x.dtype == np.complex64 and x.shape == (3, 3, 64 * 2051) and not x.flags.writeable
    lc._samples.cache_clear()
    assert np.array_equal(x, lc.samples(c))
    p = (np.abs(x.reshape(3, 3, c.n_pts, c.nchan).astype(np.complex128)) ** 2).mean(axis=(0, 3))      # [antenna, block]
    loud = np.zeros(c.n_pts, bool)
    loud[lc.loud_blocks(c)] = True
    want = lc.noise_level(3) ** 2 + lc.SOURCE ** 2
    assert np.allclose(p[:, ~loud].mean(axis=1), want, rtol=0.02)
    assert np.allclose(p[:, loud].mean(axis=1), lc.LOUD ** 2 * want, rtol=0.2)
    rows = np.abs(lc.oracle(c))
    nb = 3
    for g in (rows[:, :nb], rows[:, nb:]):          # no bin carries a group: the smallest value is within a factor of 4 of the largest
        assert g.min() > 0.25 * g.max()


def test_the_tables_move_and_the_chunks_take_both_solutions():
    for c in lc.CASES:
        if not lc.tracked(c):
            continue
        fac = lc.factors(c._replace(mod="track"))          # (the delays alone: a new solution moves a table anyway)
        step = np.abs(fac[1:] - fac[:-1]) / np.abs(fac[:-1])
        slowest = 2.0 * np.sin(np.pi / (2.0 * c.n_ant))      # the chord of 1 / (2 n_ant) of a turn: neighbouring antennas
        assert step.min() > 0.99 * slowest > 0.06, c.id      # every baseline, every bin, 6000 ceilings from chunk to chunk
        if c.mod == "gains":
            assert [lc.solution(c, k) for k in range(c.n_chunks)] == [0, 0, 1][:c.n_chunks]
            assert [lc.solution(c, k, flip=True) for k in range(c.n_chunks)] == [1, 1, 0][:c.n_chunks]
            assert [gain_track_ref.solution_index(lc.T0 + k, 2, lc.G_INTERVAL, lc.G_FIRST) for k in range(3)] == [0, 0, 1]


# ---- the oracle, and what a wrong reading does to it -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", lc.CASES, ids=lambda c: c.id)
def test_oracle_is_the_one_stated_elsewhere(case):
    """the sums over the ranges with the chunk's tables are gain_track_ref.oracle's rows (test_gpu_tracking.py's, with gains) --
    for ``rot`` test_gpu_autos.py's -- to 1e-12"""
    ref = lc.oracle(case)
    other = lc.restated_elsewhere(case, lc.samples(case))
    assert ref.shape == other.shape == (case.n_chunks, len(lc.pairs(case.n_ant)) + (case.n_ant if case.autos else 0), case.nchan)
    for name, g in lc.groups(case):
        assert lc.rel_err(ref[:, g], other[:, g]) < 1e-12, name


@pytest.mark.parametrize("case", lc.CASES, ids=lambda c: c.id)
def test_every_wrong_reading_moves_the_oracle_ten_ceilings(case):
    ref = lc.oracle(case)
    seen = []
    for name, touched, bad in lc.wrong_readings(case):
        seen.append(name)
        assert touched and set(touched) <= {g for g, _ in lc.groups(case)}
        for group, mode, err in lc.row_checks(case, bad, ref):
            if group not in touched:
                assert err == 0.0, (name, group)
                continue
            need = FACTOR * CEILING[mode]
            assert err >= need, "%s: %s moves the %s rows (%s) by %.3g, under %.3g" % (case.id, name, group, mode, err, need)
    n_r = lc.n_ranges(case)
    want = 2 * n_r + 2 + (2 if lc.tracked(case) else 0) + (1 if case.mod == "gains" else 0) + (2 if case.mod == "ant" else 0) + \
        (3 if case.autos else 0)
    assert len(seen) == want == len(set(seen)), seen
