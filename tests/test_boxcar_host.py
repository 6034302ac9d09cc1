"""The single-pulse search's definition on the host (no GPU): the numpy restatement (boxcar_ref.py) against a float64 truth under
tests/golden/boxcar_bounds.json, the wide-pulse case, the mutations the restatement must notice, sift_pulses and the binding.
The bounds file is written by ``write_bounds()`` of this module (``python tests/test_boxcar_host.py``) and committed: a bound is
twice the largest error of the restatement observed over the shapes below (the rule of tests/tolerances.py) and never above its
derived ceiling.  The ceilings, for rows whose samples lie within 64 std of the mean:
  statistics, relative to std: the tree sum is three sequential float64 sums of at most 256, 256 and n_t / 65536 terms, so m and v
    carry at most some 1024 roundings of 2^-53 of mean |x| <= 64 std: 1024 * 64 * 2^-53 = 7.3e-12;
  snr, absolute: L_j is a tree of float32 adds j deep over 2^j samples that were each rounded once, so |L_j - exact| <=
    (j + 2) 2^-24 sum |y| <= (j + 2) 2^-24 2^j 64 std, over den_j = std 2^(j/2): (j + 2) 2^-24 2^(j/2) 64 = 3.4e-3 at j = 12."""
import json
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import boxcar_ref as ref             # noqa: E402
import dedisperse_ref                # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)         # (run as a script to write the bounds file)
BOUNDS = os.path.join(ROOT, "tests", "golden", "boxcar_bounds.json")
STATS_CEILING = 1024 * 64 * 2.0 ** -53
SNR_CEILING = 14 * 2.0 ** -24 * 64 * 64
TILE = 4096        # kBoxT of effex_amd/csrc/k_boxcar.h

# rows x n_t of tests/test_gpu_boxcar.py (the degenerate (3, 1) has no truth) and the widths compared at each
SHAPES = [(2, 2), (5, 255), (4, 257), (2, TILE + 1), (2, TILE + 4096), (3, 65836)]
WIDTHS = (0, 3, 12)


def restatement_errors():
    """-> (the largest |m - truth| / std and |std - truth| / std, the largest |snr - truth|) over the shapes"""
    stats_err, snr_err = 0.0, 0.0
    for n_rows, n_t in SHAPES:
        x = ref.loud_rows(np.random.default_rng(n_rows * 100003 + n_t), n_rows, n_t)
        for row in x:
            for j in WIDTHS:
                if (1 << j) > n_t:
                    continue
                snr, width, time, (m, std, n) = ref.search_row(row, j, j, 1)
                tm, tstd, tn, tsnr = ref.truth(row, j)
                assert n == tn and (width == j).all() and np.array_equal(time, np.arange(n_t - (1 << j) + 1))
                assert np.abs(row.astype(np.float64) - tm).max() <= 64 * tstd      # what the ceilings assume
                stats_err = max(stats_err, abs(m - tm) / tstd, abs(std - tstd) / tstd)
                snr_err = max(snr_err, float(np.abs(snr.astype(np.float64) - tsnr).max()))
    return stats_err, snr_err


def pulse_results():
    """per seed: the largest cell of the whole map (series, trial, j, t), sift_pulses' first candidate, and the figures"""
    from effex_amd.plan import sift_pulses
    out = []
    for seed in dedisperse_ref.PULSE_SEEDS:
        ts = ref.wide_pulse_case(seed)[2]
        assert ts.shape == (2, 9, 637)
        snr, width, time, stats = ref.search(ts, (0, 5), 1, 3.0, 2)
        s, d, b = (int(i) for i in np.unravel_index(np.argmax(snr), snr.shape))
        narrow = ref.search(ts, (0, 0), 1, 3.0, 2)[0]
        unclipped = ref.search(ts, (0, 5), 1, 3.0, 0)[3]
        at = (dedisperse_ref.PULSE_SERIES_AT, dedisperse_ref.PULSE_DM_INDEX)
        out.append({"cell": (s, d, int(width[s, d, b]), int(time[s, d, b])), "first": sift_pulses(snr, width, time, 6.0)[0],
                    "snr": float(snr[s, d, b]), "snr_width_1": float(narrow[at + (dedisperse_ref.PULSE_T0,)]),
                    "quiet_series_max": float(snr[0].max()), "std_clipped": float(stats[at + (1,)]),
                    "std_unclipped": float(unclipped[at + (1,)])})
    return out


def write_bounds():
    stats_err, snr_err = restatement_errors()
    pulses = pulse_results()
    rec = {"stats_observed": stats_err, "stats_bound": min(2.0 * stats_err, STATS_CEILING), "stats_ceiling": STATS_CEILING,
           "snr_observed": snr_err, "snr_bound": min(2.0 * snr_err, SNR_CEILING), "snr_ceiling": SNR_CEILING}
    for key in ("snr", "snr_width_1", "quiet_series_max", "std_clipped", "std_unclipped"):
        rec["pulse_" + key] = [min(p[key] for p in pulses), max(p[key] for p in pulses)]
    with open(BOUNDS, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    return rec


@pytest.fixture(scope="module")
def rec():
    return json.load(open(BOUNDS))


# -- the restatement ----------------------------------------------------------------------------------------------------------------
def test_the_bounds_file_is_what_the_module_writes(rec):
    assert rec["stats_ceiling"] == STATS_CEILING and rec["snr_ceiling"] == SNR_CEILING
    assert rec["stats_bound"] == pytest.approx(min(2.0 * rec["stats_observed"], STATS_CEILING)) and 0 < rec["stats_bound"] <= STATS_CEILING
    assert rec["snr_bound"] == pytest.approx(min(2.0 * rec["snr_observed"], SNR_CEILING)) and 0 < rec["snr_bound"] <= SNR_CEILING


def test_the_restatement_against_float64(rec):
    stats_err, snr_err = restatement_errors()
    print("statistics relative to std %.3g (bound %.3g, ceiling %.3g); snr %.3g (bound %.3g, ceiling %.3g)" % (
        stats_err, rec["stats_bound"], STATS_CEILING, snr_err, rec["snr_bound"], SNR_CEILING))
    assert stats_err <= rec["stats_bound"] and snr_err <= rec["snr_bound"]


def test_the_tree_sum_is_the_definitions():
    """segments of 256, groups of 256 segments, the groups in order: against plain loops on 256 * 256 + 300 terms"""
    rng = np.random.default_rng(1)
    terms = rng.standard_normal(65836) * 10.0 ** rng.integers(-3, 4, 65836)
    counted = rng.random(65836) < 0.7
    segs = []
    for a in range(0, terms.size, 256):
        s = 0.0
        for t in range(a, min(a + 256, terms.size)):
            if counted[t]:
                s = s + terms[t]
        segs.append(s)
    groups = []
    for a in range(0, len(segs), 256):
        s = 0.0
        for v in segs[a:a + 256]:
            s = s + v
        groups.append(s)
    total = 0.0
    for v in groups:
        total = total + v
    assert len(segs) == 258 and len(groups) == 2
    assert ref.tree_sum(terms, counted) == total


def test_degenerate_rows_and_widths_that_do_not_fit():
    snr, width, time, stats = ref.search(np.array([[3.0], [4.0]], np.float32), (0, 12), 1)
    assert (ref.bits(snr) == 0).all() and (width == 0).all() and (time == 0).all() and np.array_equal(stats[:, 1:], [[0, 1], [0, 1]])
    const = np.full((1, 300), 2.5, np.float32)
    snr, width, time, stats = ref.search(const, (2, 5), 37)
    assert snr.shape == (1, 9) and (ref.bits(snr) == 0).all() and (width == 2).all() and np.array_equal(time[0], np.arange(9) * 37)
    assert stats[0, 0] == 2.5 and stats[0, 1] == 0.0 and stats[0, 2] == 300
    # a clip so tight that a round counts fewer than 2 samples
    x = ref.loud_rows(np.random.default_rng(2), 1, 300)
    assert ref.row_stats(x[0], 1e-6, 2)[3] and ref.row_stats(x[0], 1e-6, 2)[2] < 2
    # a width that does not fit has no start: (0, 12) on 300 samples is (0, 8)
    for a, b in zip(ref.search(x, (0, 12), 37), ref.search(x, (0, 8), 37)):
        assert np.array_equal(a, b)


# -- the wide pulse -----------------------------------------------------------------------------------------------------------------
def test_the_wide_pulse_is_found_at_its_trial_width_and_time(rec):
    want = (dedisperse_ref.PULSE_SERIES_AT, dedisperse_ref.PULSE_DM_INDEX, ref.PULSE_J, dedisperse_ref.PULSE_T0)
    for seed, p in zip(dedisperse_ref.PULSE_SEEDS, pulse_results()):
        print("seed %d: largest cell %s, snr %.2f (width 1: %.2f), quiet series at most %.2f, std %.3f clipped / %.3f not" % (
            seed, p["cell"], p["snr"], p["snr_width_1"], p["quiet_series_max"], p["std_clipped"], p["std_unclipped"]))
        assert p["cell"] == want
        first = p["first"]
        assert (first["series"], first["dm_index"], first["time"], first["width"]) == (want[0], want[1], want[3], 1 << want[2])
        assert first["snr"] == np.float32(p["snr"])
        assert p["std_clipped"] < p["std_unclipped"]
        for key in ("snr", "snr_width_1", "quiet_series_max", "std_clipped", "std_unclipped"):
            assert rec["pulse_" + key][0] <= p[key] <= rec["pulse_" + key][1], key


# -- mutations ----------------------------------------------------------------------------------------------------------------------
def test_the_restatement_notices_every_mutation():
    """each wrong reading of the definition changes the output on a loud input (or, for the tie rules, on the row of exact ties)"""
    n_t = 37 * 19 + 1           # 704: 19 blocks of 37 over the starts of width 4, 20 over n_t
    x = ref.loud_rows(np.random.default_rng(11), 3, n_t)
    ties = ref.tie_row(n_t)[None]

    def changed(got, want):
        return any(a.shape != b.shape or not np.array_equal(ref.bits(a), ref.bits(b)) for a, b in zip(got[:3], want[:3]))

    def with_stats(**hooks):
        return np.stack([np.concatenate(ref.search_row(r, 0, 5, 37, stats=ref.row_stats(r, 3.0, 2, **hooks))[:3]) for r in x])

    want = ref.search(x, (0, 5), 37)
    want_rows = (np.stack([np.concatenate(ref.search_row(r, 0, 5, 37)[:3]) for r in x]),)
    want_ties = ref.search(ties, (0, 5), 37)
    assert not changed(ref.search(x, (0, 5), 37, tile=None), want) and not changed((with_stats(),), want_rows)
    # the tie row holds ties of both kinds: equal S/N at two widths, and at two starts of one width
    s0 = ref.search(ties, (0, 0), 1)[0][0]
    s2 = ref.search(ties, (2, 2), 1)[0][0]
    assert s0.max() == s2.max() and (s0 == s0.max()).sum() == 2
    mutations = {
        "the second child one sample late": changed(ref.search(x, (0, 5), 37, child=1), want),
        "the second child one sample early": changed(ref.search(x, (0, 5), 37, child=-1), want),
        "a level read after it was overwritten": changed(ref.search(x, (0, 5), 37, in_place=True), want),
        "zeros in place of the halo at a tile boundary": changed(ref.search(x, (0, 5), 37, tile=256), want),
        "the mean not subtracted": changed(ref.search(x, (0, 5), 37, subtract_mean=False), want),
        "r_j left out": changed(ref.search(x, (0, 5), 37, use_root=False), want),
        "the clip test against the previous round's m": changed((with_stats(clip_against="previous round"),), want_rows),
        "ties to the widest width": changed(ref.search(ties, (0, 5), 37, ties="widest width"), want_ties),
        "ties to the latest start": changed(ref.search(ties, (0, 5), 37, ties="latest start"), want_ties),
        "blocks counted over n_t": changed(ref.search(x, (2, 5), 37, starts_of_blocks="n_t"), ref.search(x, (2, 5), 37)),
    }
    # dropped samples multiplied by 0 instead of selected away, with a NaN under the clip: the NaN is a term that does not count
    terms = x[0].astype(np.float64)
    counted = np.ones(n_t, bool)
    terms[100], counted[100] = np.nan, False
    assert np.isfinite(ref.tree_sum(terms, counted))
    mutations["dropped samples multiplied by 0"] = not np.isfinite(ref.tree_sum(terms, counted, drop="multiply"))
    for name, moved in mutations.items():
        print("%-50s %s" % (name, "changes the output" if moved else "IS NOT NOTICED"))
    assert all(mutations.values()), [k for k, v in mutations.items() if not v]


# -- sift_pulses --------------------------------------------------------------------------------------------------------------------
def test_sift_pulses_clusters_order_and_ties():
    from effex_amd.plan import boxcar_widths, sift_pulses
    snr = np.zeros((2, 6, 8), np.float32)
    width = np.zeros((2, 6, 8), np.int32)
    time = (np.arange(8, dtype=np.int32) * 64)[None, None, :] + np.zeros((2, 6, 1), np.int32)
    snr[0, 1, 1], snr[0, 2, 2] = 7.0, 9.0            # touch diagonally: one cluster
    snr[0, 4, 4], snr[0, 4, 6] = 8.0, 8.0            # a cell apart: two clusters, equal snr
    snr[0, 0, 7] = 6.0                               # not above the threshold
    snr[1, 5, 0], snr[1, 5, 1], snr[1, 4, 1] = 12.0, 12.0, 12.0      # one cluster of equal cells: the smallest trial, then block
    width[0, 2, 2], width[1, 4, 1] = 3, 5
    time[0, 2, 2] += 17
    got = sift_pulses(snr, width, time, threshold=6.0)
    assert got.dtype.names == ("series", "dm_index", "time", "width", "snr", "n_cells")
    rows = [tuple(int(v) if k != "snr" else float(v) for k, v in zip(got.dtype.names, r)) for r in got]
    assert rows == [(1, 4, 64, 32, 12.0, 3), (0, 2, 128 + 17, 8, 9.0, 2), (0, 4, 256, 1, 8.0, 1), (0, 4, 384, 1, 8.0, 1)]
    assert len(sift_pulses(snr, width, time, threshold=12.0)) == 0
    assert len(sift_pulses(snr[0, 0], width[0, 0], time[0, 0], threshold=5.0)) == 1          # one row is one series, one trial
    one = sift_pulses(snr[1], width[1], time[1])
    assert len(one) == 1 and one[0]["series"] == 0 and one[0]["dm_index"] == 4
    with pytest.raises(ValueError):
        sift_pulses(snr, width[0], time)
    assert np.array_equal(boxcar_widths(0, 8), [1, 2, 4, 8, 16, 32, 64, 128, 256]) and np.array_equal(boxcar_widths(12, 12), [4096])
    for bad in ((-1, 3), (3, 2), (0, 13)):
        with pytest.raises(ValueError):
            boxcar_widths(*bad)


# -- the binding --------------------------------------------------------------------------------------------------------------------
def test_the_binding_matches_the_header():
    import ctypes
    from effex_amd import _lib
    restype, argtypes = _lib.SIGNATURES["fxc_boxcar_search"]
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fxcorr.h")).read(), flags=re.S)
    proto = re.search(r"\bint\s+fxc_boxcar_search\s*\((.*?)\)\s*;", text, re.S)
    assert proto, "include/fxcorr.h does not declare fxc_boxcar_search"
    params = [" ".join(a.split()) for a in proto.group(1).split(",")]
    kinds = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "double": ctypes.c_double}
    want = [ctypes.c_void_p if "*" in a else kinds[a.split()[-2]] for a in params]
    assert restype is ctypes.c_int and argtypes == want, (params, argtypes)
    assert [a.split()[-1].lstrip("*") for a in params] == ["plan", "series", "n_rows", "n_t", "mem_kind", "j_lo", "j_hi", "block", "clip",
                                                            "clip_iters", "snr_out", "width_out", "time_out", "stats_out"]
    header = open(os.path.join(ROOT, "include", "fxcorr.h")).read()
    assert "boxcar matched filtering and candidate" not in header


if __name__ == "__main__":
    print(write_bounds())
