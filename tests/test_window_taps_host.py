"""The device test of the window layouts (test_gpu_window_taps.py) can see what it is meant to see: for every case of
``window_cases.CASES`` and every mutation of its rough window -- two taps exchanged in the middle, at either end, one branch's tap
order reversed, the whole window reversed -- the float64 oracle under the wrong window differs from the oracle under the right one
by at least ten times the ceiling the device test holds, in every comparison the device test makes (its own metric, chunk by
chunk / stream by stream).  No GPU."""
import numpy as np
import pytest

import window_cases as wc
from tolerances import TOL_SPEC, TOL_SPEC_ANY, TOL_VIS

FACTOR = 10.0


def ceiling(case):
    """The ceiling the device test compares the case with (tests/tolerances.py)."""
    if case.entry != "channelize":
        return TOL_VIS.ceiling
    return (TOL_SPEC_ANY if case.nchan & (case.nchan - 1) else TOL_SPEC).ceiling


def test_case_ids_are_unique_and_cases_are_small():
    ids = [c.id for c in wc.CASES]
    assert len(ids) == len(set(ids))
    for c in wc.CASES:
        assert c.n_chunks == 2 and c.entry in ("fx", "fx_u8", "channelize"), c
        assert c.ntaps < c.frames <= 67, c          # every tap meets data; nothing takes long
        assert set(c.expect) <= {"path", "block", "lds_bytes", "specialised"} and "path" in c.expect, c
        assert c.dev or not (set(c.env) - {"FXC_RTC"}), c      # every other knob exists in the developer library only
    assert sum(1 for c in wc.CASES if c.extra) > len(wc.CASES) // 2      # ragged tails in most cases


def test_rough_window_is_reproducible_and_rough():
    for ntaps, nchan in ((4, 4096), (32, 16), (1, 128), (17, 8192)):
        w = wc.rough_window(ntaps, nchan)
        assert w.dtype == np.float64 and w.shape == (ntaps * nchan,)
        np.testing.assert_array_equal(w, wc.rough_window(ntaps, nchan))
        np.testing.assert_array_equal(w, np.random.default_rng(1000003 * ntaps + nchan).standard_normal(ntaps * nchan))
        assert np.all(w != 0.0)
        assert np.abs(w - w[::-1]).max() > 1.0          # no symmetry
    assert not np.array_equal(wc.rough_window(4, 4096)[:4096], wc.rough_window(2, 4096)[:4096])


def test_mutations_change_what_they_name():
    w = wc.rough_window(4, 64)
    got = dict(wc.mutations(w, 4, 64))
    assert list(got) == ["mid_adjacent_swapped", "last_two_swapped", "first_two_swapped", "one_branch_tap_order_reversed",
                         "whole_window_reversed"]
    assert np.flatnonzero(got["mid_adjacent_swapped"] != w).tolist() == [2 * 64 + 28, 2 * 64 + 29]
    assert np.flatnonzero(got["last_two_swapped"] != w).tolist() == [254, 255]
    assert np.flatnonzero(got["first_two_swapped"] != w).tolist() == [0, 1]
    assert np.flatnonzero(got["one_branch_tap_order_reversed"] != w).tolist() == [28, 64 + 28, 128 + 28, 192 + 28]
    np.testing.assert_array_equal(got["whole_window_reversed"], w[::-1])
    assert "one_branch_tap_order_reversed" not in dict(wc.mutations(wc.rough_window(1, 64), 1, 64))
    for name, wrong in got.items():
        np.testing.assert_array_equal(np.sort(wrong), np.sort(w), err_msg=name)      # a permutation of the same taps


@pytest.mark.parametrize("case", wc.CASES, ids=[c.id for c in wc.CASES])
def test_every_mutation_moves_the_oracle_ten_ceilings(case):
    window = wc.rough_window(case.ntaps, case.nchan)
    x, _ = wc.make_input(case)
    ref = wc.oracle(case, x, window)
    need = FACTOR * ceiling(case)
    for name, wrong in wc.mutations(window, case.ntaps, case.nchan):
        bad = wc.oracle(case, x, wrong)
        for label, err in wc.checks(case, bad, ref):
            assert err >= need, "%s: %s moves %s by %.3g, under %.3g" % (case.id, name, label, err, need)
