"""The dedispersion's definition on the host (no GPU): dm_shifts against its formula, the numpy restatement (dedisperse_ref.py)
against a float64 truth under tests/golden/dedisperse_bounds.json, the pulse case, the mutations the restatement must notice, and
the binding.  The bounds file is written by ``write_bounds()`` of this module (``python tests/test_dedisperse_host.py``) and
committed: the bound is twice the largest error of the restatement observed over the shapes below, relative to sum |P| of the
cell, and never above 64 * 2^-24 -- a sequential float32 sum of at most 64 terms plus one rounding; the pulse factor is half the
smallest ratio observed over the eight seeds."""
import json
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dedisperse_ref as ref      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS = os.path.join(ROOT, "tests", "golden", "dedisperse_bounds.json")
CEILING = 64 * 2.0 ** -24

# nchan, (n_chunks, n_series, n_tbin), trials: the shapes of tests/test_gpu_dedisperse.py and the pulse case's
SHAPES = [(64, (4, 1, 16), 5), (63, (3, 3, 37), 9), (1000, (2, 2, 64), 5), (1, (5, 2, 8), 5), (64, (8, 2, 128), 9)]


def random_shifts(rng, n_dm, nchan, below):
    return rng.integers(0, below, (n_dm, nchan)).astype(np.int32)


def noise(rng, shape):
    return (rng.chisquare(32, shape) / 32.0).astype(np.float32)


def restatement_errors():
    """-> the largest |restatement - truth| / sum |P| of every shape, with and without channel weights"""
    worst = []
    for nchan, dims, n_dm in SHAPES:
        rng = np.random.default_rng(nchan + dims[2])
        power = noise(rng, dims + (nchan,))
        shifts = random_shifts(rng, n_dm, nchan, max(1, dims[0] * dims[2] // 2))
        weights = np.where(rng.random(nchan) < 0.2, 0.0, 1.0).astype(np.float32)
        weights[0] = 1.0
        for w in (None, weights):
            val, mag = ref.truth(power, shifts, w)
            worst.append(float((np.abs(ref.dedisperse(power, shifts, w).astype(np.float64) - val) / mag).max()))
    return worst


def pulse_results():
    return [ref.pulse_figures(ref.dedisperse(*ref.pulse_case(seed))) for seed in ref.PULSE_SEEDS]


def write_bounds():
    observed = max(restatement_errors())
    ratios = [r for _, r in pulse_results()]
    rec = {"observed": observed, "bound": min(2.0 * observed, CEILING), "ceiling": CEILING, "pulse_ratio_smallest": min(ratios),
           "pulse_factor": 0.5 * min(ratios)}
    with open(BOUNDS, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    return rec


@pytest.fixture(scope="module")
def rec():
    return json.load(open(BOUNDS))


# -- dm_shifts --------------------------------------------------------------------------------------------------------------------
def test_dm_shifts_against_the_formula():
    from effex_amd.plan import averaged_freqs, dm_shifts
    for nchan, bw, fc, tsamp in ((64, 400e6, 600e6, 1e-3), (63, 2.4e6, 1.4204e9, 63 / 2.4e6), (1000, 200e6, 400e6, 2e-4), (1, 1e6, 1e9, 1e-6)):
        dms = np.array([0.0, 2.5, 10.0, 55.5])
        got = dm_shifts(nchan, bw, fc, dms, tsamp)
        assert got.dtype == np.int32 and got.shape == (4, nchan)
        assert np.array_equal(got, ref.shifts_formula(nchan, bw, fc, dms, tsamp))
        f = averaged_freqs(nchan, bw, fc)                      # the same axis
        assert np.array_equal(f, ref.freqs(nchan, bw, fc))
        assert (got[:, np.argmax(f)] == 0).all() and np.argmax(f) == nchan - 1 and (got >= 0).all()
        assert (np.diff(got.astype(np.int64), axis=1) <= 0).all()      # the rows' order ascends in frequency
        assert (got[0] == 0).all()
        # linear in DM before the rounding
        delay = ref.DM_CONSTANT_S * ((f / 1e6) ** -2.0 - (f.max() / 1e6) ** -2.0) / tsamp
        assert np.abs(got - dms[:, None] * delay[None, :]).max() <= 0.5 + 1e-9
    assert dm_shifts(64, 400e6, 600e6, ref.WIDE_DMS, 1e-3).max() == 387
    assert dm_shifts(64, 400e6, 600e6, 3.0, 1e-3).shape == (1, 64)
    for bad in (dict(dms=[-1.0]), dict(dms=[np.nan]), dict(tsamp=0.0), dict(nchan=0), dict(dms=[]), dict(frequency=100e6)):
        args = dict(nchan=64, bandwidth=400e6, frequency=600e6, dms=[1.0], tsamp=1e-3)
        args.update(bad)
        with pytest.raises(ValueError):
            dm_shifts(**args)


# -- the restatement ----------------------------------------------------------------------------------------------------------------
def test_the_bounds_file_is_what_the_module_writes(rec):
    assert rec["ceiling"] == CEILING and rec["bound"] == pytest.approx(min(2.0 * rec["observed"], CEILING))
    assert rec["pulse_factor"] == pytest.approx(0.5 * rec["pulse_ratio_smallest"])
    assert 0 < rec["bound"] <= CEILING


def test_the_restatement_against_float64(rec):
    worst = restatement_errors()
    print("restatement against float64, relative to sum |P|:", ["%.3g" % w for w in worst], "bound %.3g" % rec["bound"])
    assert max(worst) <= rec["bound"]


def test_the_pulse_is_found_at_its_trial_and_time(rec):
    for seed, (cell, ratio) in zip(ref.PULSE_SEEDS, pulse_results()):
        print("seed %d: largest cell %s, excess over the best of DM 0 x%.3g (factor %.3g)" % (seed, cell, ratio, rec["pulse_factor"]))
        assert cell == (ref.PULSE_SERIES_AT, ref.PULSE_DM_INDEX, ref.PULSE_T0)
        assert ratio >= rec["pulse_factor"]


def test_special_values():
    rng = np.random.default_rng(5)
    power = noise(rng, (2, 2, 16, 70))
    shifts = random_shifts(rng, 3, 70, 9)
    none = ref.dedisperse(power, shifts, np.zeros(70, np.float32))
    assert none.shape == (2, 3, 32 - int(shifts.max())) and (ref.bits(none) == 0).all()      # +0
    w = np.ones(70, np.float32)
    w[[3, 64, 69]] = (0.0, -1.0, np.nan)
    dirty = power.copy()
    dirty[..., 3], dirty[..., 64], dirty[..., 69] = np.nan, np.inf, 1e30
    assert np.array_equal(ref.bits(ref.dedisperse(dirty, shifts, w)), ref.bits(ref.dedisperse(power, shifts, w)))
    assert np.array_equal(ref.bits(ref.dedisperse(power, shifts, w * 4)), ref.bits(ref.dedisperse(power, shifts, w)))
    # 3-D and 2-D input are one chunk
    assert np.array_equal(ref.dedisperse(power[0], shifts), ref.dedisperse(power[:1], shifts))
    assert np.array_equal(ref.dedisperse(power[0, 1], shifts)[0], ref.dedisperse(power[:1], shifts)[1])


# -- mutations ----------------------------------------------------------------------------------------------------------------------
def test_the_restatement_notices_every_mutation(rec):
    """each wrong reading of the definition moves the restatement by ten bounds or more, relative to sum |P|, on a loud input"""
    rng = np.random.default_rng(11)
    dims, nchan = (3, 3, 37), 63
    power = ref.loud_power(rng, dims + (nchan,))
    shifts = np.minimum(ref.wide_shifts(np.arange(5) * 4.0, nchan=nchan, tsamp=8e-3), 50).astype(np.int32)
    shifts[:, 0] = 50                                        # S_max stays whatever the mutation does
    weights = np.ones(nchan, np.float32)
    weights[[7, 40]] = 0.0
    want = ref.dedisperse(power, shifts, weights).astype(np.float64)
    _, mag = ref.truth(power, shifts, weights)
    n_tbin = dims[2]

    def moved(got):
        return float((np.abs(got.astype(np.float64) - want) / mag).max())

    def stays_in_its_chunk(ts, k, shift, n_out):
        t = np.arange(n_out)
        return ts[:, (t // n_tbin) * n_tbin + (t % n_tbin + shift) % n_tbin, k]

    off_by_one = shifts.copy()
    off_by_one[2, 30] += 1
    assert off_by_one.max() == shifts.max()
    mutations = {
        "the table in natural channel order": ref.dedisperse(power, np.fft.ifftshift(shifts, axes=1), weights),
        "one channel's shift off by one": ref.dedisperse(power, off_by_one, weights),
        "the neighbouring series": ref.dedisperse(np.roll(power, 1, axis=1), shifts, weights),
        "a series stride of one bin less": ref.dedisperse(
            np.lib.stride_tricks.as_strided(power, power.shape, (power.strides[0], power.strides[1] - power.strides[2]) + power.strides[2:]).copy(),
            shifts, weights),
        "time not carried across a chunk": ref.dedisperse(power, shifts, weights, column=stays_in_its_chunk),
        "an uncounted channel added": ref.dedisperse(power, shifts, counted=np.arange(nchan) != 7),
    }
    for name, got in mutations.items():
        print("%-40s moves the result by %.3g of sum |P| (bound %.3g)" % (name, moved(got), rec["bound"]))
        assert moved(got) >= 10.0 * rec["bound"], name


# -- the binding --------------------------------------------------------------------------------------------------------------------
def test_the_binding_matches_the_header():
    import ctypes
    from effex_amd import _lib
    restype, argtypes = _lib.SIGNATURES["fxc_dedisperse"]
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fxcorr.h")).read(), flags=re.S)
    proto = re.search(r"\bint\s+fxc_dedisperse\s*\((.*?)\)\s*;", text, re.S)
    assert proto, "include/fxcorr.h does not declare fxc_dedisperse"
    params = [" ".join(a.split()) for a in proto.group(1).split(",")]
    kinds = {"int64_t": ctypes.c_int64, "int": ctypes.c_int}
    want = [ctypes.c_void_p if "*" in a else kinds[a.split()[-2]] for a in params]
    assert restype is ctypes.c_int and argtypes == want, (params, argtypes)
    assert [a.split()[-1].lstrip("*") for a in params] == ["plan", "power", "n_chunks", "n_series", "n_tbin", "mem_kind", "shifts", "n_dm",
                                                            "chan_weights", "out", "info_out"]


if __name__ == "__main__":
    print(write_bounds())
