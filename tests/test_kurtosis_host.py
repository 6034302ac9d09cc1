"""The spectral kurtosis estimator without a GPU: the restatement of its definition (kurtosis_ref.py) on the statistics the
estimator is used for, the weights rule by hand, and ``sk_thresholds`` against its formula.  The allowed deviations of the
noise statistics are three times what tools/kurtosis_measure.py --bounds measured on the restatement over seeds 0 - 7
(tests/golden/kurtosis_bounds.json): successive polyphase frames share input samples and a chunk's first frames see part of the
window only, so neither the mean nor the variance is exactly the paper's, and eight seeds do not show the worst case."""
import json
import os

import numpy as np
import pytest

import kurtosis_ref as kr
from effex_amd.plan import sk_thresholds

BOUNDS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kurtosis_bounds.json")
N_ANT, NCHAN, NTAPS, N_PTS, N_CHUNKS = kr.STAT_SHAPE


@pytest.fixture(scope="module")
def record():
    with open(BOUNDS) as fh:
        return json.load(fh)["statistics"]


def test_thresholds_follow_the_formula():
    for M in (2, 3, 64, 515, 4096):
        for sigma in (3.0, 4.5):
            mu2 = 4.0 * M * M / ((M - 1.0) * (M + 2.0) * (M + 3.0))
            lo, hi = sk_thresholds(M, sigma)
            assert lo == pytest.approx(1.0 - sigma * np.sqrt(mu2), rel=1e-15) and hi == pytest.approx(1.0 + sigma * np.sqrt(mu2), rel=1e-15)
            assert kr.mu2(M) == pytest.approx(mu2, rel=1e-15)
    assert sk_thresholds(64) == sk_thresholds(64, 3.0)
    for bad in (1, 0, -3):
        with pytest.raises(ValueError):
            sk_thresholds(bad)
    with pytest.raises(ValueError):
        sk_thresholds(64, 0.0)


@pytest.mark.parametrize("seed", kr.STAT_SEEDS)
def test_noise_has_mean_one_and_the_papers_variance(record, seed):
    mean_dev, var_dev, alarm = kr.noise_statistics(seed)
    print("seed", seed, "mean", mean_dev, "variance", var_dev, "false alarms", alarm)
    assert record["mu2"] == pytest.approx(kr.mu2(N_PTS))
    assert mean_dev <= record["mean_bound"]
    assert var_dev <= record["variance_bound"]
    # the record is this restatement's own: the tool wrote what this computes
    assert mean_dev == pytest.approx(record["mean_deviation"][str(seed)], abs=1e-9)
    assert var_dev == pytest.approx(record["variance_deviation"][str(seed)], abs=1e-9)
    assert alarm == pytest.approx(record["false_alarm_share"][str(seed)], abs=1e-12)


def test_the_recorded_bounds_are_three_times_the_largest_deviation(record):
    assert record["mean_bound"] == pytest.approx(3.0 * max(record["mean_deviation"].values()))
    assert record["variance_bound"] == pytest.approx(3.0 * max(record["variance_deviation"].values()))
    assert record["mean_bound"] < 0.5 and record["variance_bound"] < 1.0          # "near": the bounds still say something
    shares = record["false_alarm_share"].values()
    assert record["false_alarm_share_mean"] == pytest.approx(sum(shares) / len(shares))


@pytest.mark.parametrize("n_ant", [2, 3])
@pytest.mark.parametrize("seed", kr.STAT_SEEDS)
def test_both_tones_are_flagged_and_only_their_antenna(seed, n_ant):
    """a steady tone at 30 times the bin's noise power falls below lo, the same tone on for 8 frames of 64 rises above hi, in
    every chunk; both bins lose every baseline of the hit antenna and -- three antennas -- no other"""
    x, window = kr.case(seed, n_ant, NCHAN, NTAPS, N_PTS, N_CHUNKS)
    sk, power = kr.kurtosis(x, NCHAN, window)
    assert sk.shape == power.shape == (N_CHUNKS, n_ant, 1, NCHAN)
    lo, hi = sk_thresholds(N_PTS)
    k1, k2 = (kr.shifted(k, NCHAN) for k in kr.tone_bins(NCHAN))
    assert (sk[:, kr.HIT_ANT, 0, k1] < lo).all(), sk[:, kr.HIT_ANT, 0, k1]
    assert (sk[:, kr.HIT_ANT, 0, k2] > hi).all(), sk[:, kr.HIT_ANT, 0, k2]
    w = kr.weights(sk, N_PTS, 0, lo, hi)
    assert w.shape == (N_CHUNKS, len(kr.pairs(n_ant)), NCHAN) and w.dtype == np.float32
    for i, (a, b) in enumerate(kr.pairs(n_ant)):
        if kr.HIT_ANT in (a, b):
            assert (w[:, i, [k1, k2]] == 0.0).all()
    if n_ant == 3:
        # the baseline (0, 2) without the hit antenna keeps the weights the same noise has without the tones, their bins included
        clean = kr.case(seed, n_ant, NCHAN, NTAPS, N_PTS, N_CHUNKS, with_tones=False)[0]
        clean_w = kr.weights(kr.kurtosis(clean, NCHAN, window)[0], N_PTS, 0, lo, hi)
        assert np.array_equal(w[:, 1], clean_w[:, 1])
        assert w[:, 1].mean() > 0.9          # (clean noise: a few false alarms at most)


def test_scaling_the_samples_changes_nothing():
    x, window = kr.case(3, 2, NCHAN, NTAPS, N_PTS, 2)
    sk, power = kr.kurtosis(x, NCHAN, window, tint=16)
    for c in (1e-3, 1e3):
        sk_c, power_c = kr.kurtosis(c * x, NCHAN, window, tint=16)
        assert np.abs(sk_c - sk).max() < 1e-12
        assert np.abs(power_c / (c * c) - power).max() < 1e-12 * power.max()


def test_the_definition_on_a_case_small_enough_to_read():
    """4 frames of one channel pair, bins of 3: a full bin, then a single frame.  p = 1, 4, 9 | 16"""
    f = np.zeros((1, 1, 4, 2), np.complex128)
    f[0, 0, :, 0] = [1.0, 2.0j, -3.0, 4.0]                  # natural bin 0 is stored at 1
    sk, power = kr.kurtosis_of_spectra(f, tint=3)
    assert sk.shape == (1, 1, 2, 2)
    s1, s2 = 14.0, 98.0
    assert sk[0, 0, 0, 1] == pytest.approx(4.0 / 2.0 * (3.0 * s2 / s1 ** 2 - 1.0)) and power[0, 0, 0, 1] == pytest.approx(s1 / 3.0)
    assert sk[0, 0, 1, 1] == 1.0 and power[0, 0, 1, 1] == 16.0          # one frame is no evidence; the power is still there
    assert sk[0, 0, 0, 0] == 0.0 and power[0, 0, 0, 0] == 0.0           # the dead channel
    f[0, 0, 1, 0] = np.nan
    assert np.isnan(kr.kurtosis_of_spectra(f, tint=3)[0][0, 0, 0, 1])
    f[0, 0, 1, 0] = np.inf
    assert np.isnan(kr.kurtosis_of_spectra(f, tint=3)[0][0, 0, 0, 1])
    # a constant amplitude is 0, whatever the amplitude
    assert kr.kurtosis_of_spectra(np.full((1, 1, 8, 1), 3.0 - 1.0j), 0)[0][0, 0, 0, 0] == pytest.approx(0.0, abs=1e-12)
    # odd channel counts: numpy's fftshift
    g = np.zeros((1, 1, 2, 5), np.complex128)
    g[0, 0, :, 0] = 1.0
    assert kr.kurtosis_of_spectra(g)[1][0, 0, 0].tolist() == [0.0, 0.0, 1.0, 0.0, 0.0] and kr.shifted(0, 5) == 2


def test_the_weights_rule_by_hand():
    lo, hi = 0.5, 1.5
    # 3 antennas, 7 frames at 3 a bin: bins of 3, 3 and 1 frame -- the last is partial and not counted; 4 channels
    sk = np.ones((2, 3, 3, 4), np.float32)
    sk[0, 0, 0, 0] = np.nan            # a NaN: antenna 0, channel 0, chunk 0
    sk[0, 1, 1, 1] = lo                # equal to lo: counted as good
    sk[0, 2, 1, 2] = np.float32(1.6)   # above hi: antenna 2, channel 2
    sk[1, 1, 2, 3] = 9.0               # the partial last bin would flag: ignored
    w = kr.weights(sk, 7, 3, lo, hi)
    assert kr.counted_bins(7, 3) == 2 and kr.time_bins(7, 3) == [(0, 3), (3, 6), (6, 7)]
    want = np.ones((2, 3, 4), np.float32)          # baselines (0,1), (0,2), (1,2)
    want[0, [0, 1], 0] = 0.0
    want[0, [1, 2], 2] = 0.0
    assert np.array_equal(w, want)
    # the same partial bin as the only bin of its chunk is counted: 2 frames at tint 0
    only = np.ones((1, 2, 1, 4), np.float32)
    only[0, 1, 0, 3] = 9.0
    assert kr.counted_bins(2, 0) == 1
    assert kr.weights(only, 2, 0, lo, hi)[0, 0].tolist() == [1.0, 1.0, 1.0, 0.0]
    # a bin of a single frame holds 1 by definition: 3 frames at 2 a bin, counted or not it flags nothing
    f = np.zeros((1, 2, 3, 4), np.complex128)
    f[..., :] = [[1.0], [5.0], [2.0]]
    sk3, _ = kr.kurtosis_of_spectra(f, tint=2)
    assert (sk3[:, :, 1] == 1.0).all() and kr.counted_bins(3, 2) == 1
    # full bins only: all are counted
    assert kr.counted_bins(8, 2) == 4 and kr.counted_bins(8, 0) == 1 and kr.counted_bins(8, 8) == 1
    # float32 values are compared as they are, in float64: a threshold between two float32 neighbours
    edge = np.float32(0.7)
    one = np.full((1, 2, 1, 1), edge, np.float32)
    assert kr.weights(one, 2, 0, float(edge), 2.0)[0, 0, 0] == 1.0
    assert kr.weights(one, 2, 0, float(edge) + 1e-12, 2.0)[0, 0, 0] == 0.0
