"""The measured table of stage lists (effex_amd/csrc/spec_tuned.h) and the cover list drawn from it (tests/golden/spec_cover.json,
tests/spec_cover.py), without a GPU: the table is well formed, the cover reaches every butterfly x stage position and frames per step
the table uses, the library's search still gives every cover entry the build that was recorded, and each of those builds, run on the
host (tests/emul/emul_spec.cpp), gives the float64 oracle's answer.  A combination that fails here can be stepped through with gdb."""
import pytest

import spec_cover

NTAPS = 4
COVER = spec_cover.load_cover()
ENTRIES = spec_cover.cover_entries(COVER)
IDS = ["%s-%d" % (spec_cover.VARIANT_TAG[v], n) for v, n, _ in ENTRIES]
TABLES = spec_cover.parse_tuned()


def test_the_three_tables_are_read_whole():
    """parse_tuned drops nothing but the three {0, ...} sentinels: as many entries as the file has lines that open one"""
    import re
    lines = [ln for ln in open(spec_cover.TUNED_PATH) if re.match(r"\s*\{\s*\d", ln)]
    assert sum(len(TABLES[v]) for v in (0, 2, 3)) == len(lines) - 3 and all(len(TABLES[v]) > 0 for v in (0, 2, 3))


@pytest.mark.parametrize("variant", [0, 2, 3], ids=["xf", "f", "xm"])
def test_table_sanity(variant):
    """Every entry of spec_tuned.h by itself: channel counts strictly increasing (the lookup takes the first match), the stages multiply
    to the channel count, n_stages says how many there are and fits SpecTuned::radix, every radix has a butterfly (at most 32, no prime
    factor above 23), one or two frames per step and two only where there is an LDS trip to share, at most 8192 channels."""
    last = 0
    for e in TABLES[variant]:
        tag = "table sanity: %s entry %d" % (spec_cover.TABLE_OF_VARIANT[variant], e["n"])
        assert e["n"] > last, tag
        last = e["n"]
        prod = 1
        for r in e["radix"]:
            prod *= r
            m = r
            for p in (2, 3, 5, 7, 11, 13, 17, 19, 23):
                while m % p == 0:
                    m //= p
            assert 2 <= r <= 32 and m == 1, tag
        assert prod == e["n"], tag
        assert e["n_stages"] == len(e["radix"]) and 1 <= e["n_stages"] <= spec_cover.MAX_TABLE_STAGES, tag
        assert e["u"] in (1, 2) and (e["u"] == 1 or e["n_stages"] >= 2), tag
        assert e["n"] <= 8192, tag


def test_cover_is_complete():
    """Every (radix, position) pair and frames per step a table entry names is a feature of some cover entry's recorded build."""
    for variant in (0, 2, 3):
        have = set()
        for e in COVER["cover"][str(variant)]:
            have |= spec_cover.features(variant, e["report"])
        assert spec_cover.as_tuples(COVER["universe"][str(variant)]) <= have, "cover is complete: regenerate with tools/make_spec_cover.py"
        for e in TABLES[variant]:
            missing = spec_cover.static_features(variant, e) - have
            assert not missing, "cover is complete: %s entry %d uses %s, which no cover entry runs: regenerate with tools/make_spec_cover.py" % (
                spec_cover.TABLE_OF_VARIANT[variant], e["n"], sorted(missing))


@pytest.mark.parametrize("variant,nchan,entry", ENTRIES, ids=IDS)
def test_cover_is_current(variant, nchan, entry):
    """The library's search (spec_tuned.h, the cost model, the layout search of h_rtc.h) gives this channel count the build that the cover
    recorded: a change to any of them moves what the cover's tests run, and shows here."""
    fresh = spec_cover.probe(nchan, NTAPS, variant)
    assert fresh is not None and spec_cover.recorded(fresh) == entry["report"], (
        "cover is current: %s-%d now builds %s, recorded %s: regenerate with tools/make_spec_cover.py" % (
            spec_cover.VARIANT_TAG[variant], nchan, fresh and spec_cover.recorded(fresh), entry["report"]))
    assert spec_cover.as_tuples(entry["chosen_for"]) <= spec_cover.features(variant, fresh), "cover is current: regenerate with tools/make_spec_cover.py"
    if variant == 3:
        first = spec_cover.probe(nchan, NTAPS, 2)
        assert first is not None and spec_cover.recorded(first) == entry["f_report"], (
            "cover is current: the F pass of xm-%d changed: regenerate with tools/make_spec_cover.py" % nchan)


@pytest.mark.parametrize("variant,nchan,entry", ENTRIES, ids=IDS)
def test_cover_entry_matches_oracle_on_the_host(tmp_path, variant, nchan, entry):
    """The recorded build of every cover entry through the host emulation against the float64 oracle, with the bounds of
    tests/test_emul.py (1e-5 of the largest sum for F + X and the second pass, 2e-6 of the largest spectrum for the F stage): two chunks,
    five frames (seven where a step carries two: the last step has one), a dropped tail, two splits of a chunk where a workgroup has
    several slots.  The F stage: two chunks of three antennas, so stream pairs straddle a chunk and the store is antenna-interleaved."""
    rep = entry["report"]
    n_pts = 7 if rep["frames_per_step"] == 2 else 5
    wg_splits = 2 if rep["slots"] > 1 else 1
    if variant == 0:
        spec_cover.check_fx_emulation(tmp_path, nchan, NTAPS, n_pts, wg_splits, False, spec_cover.emul_flags(rep), rep["tpr"], rep["slots"])
    elif variant == 2:
        spec_cover.check_f_emulation(tmp_path, nchan, NTAPS, n_pts, wg_splits, 6, 3, spec_cover.emul_flags(rep, fonly=True), extra=min(3, nchan - 1))
    else:
        f_rep = entry["f_report"]
        spec_cover.check_two_pass_emulation(tmp_path, nchan, NTAPS, n_pts, wg_splits,
                                            (spec_cover.emul_flags(f_rep, fonly=True), f_rep["tpr"], f_rep["slots"]),
                                            (spec_cover.emul_flags(rep, xm=True), rep["tpr"], rep["slots"]), n_chunks=2, extra=min(3, nchan - 1))
