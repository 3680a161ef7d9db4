"""The host side of the resampler (xvector_amd/resample.py) without a GPU: table geometry and output counts
against the numbers worked out by hand, every fp32 weight against an independent fp64 formula, what the filter does to a tone
in and above the pass band (the fp64 restatement of tests/resample_ref.py), and the utterance rules of --allow-downsample /
--allow-upsample."""
import logging
import math

import numpy as np
import pytest

import resample_ref as ref
from xvector_amd import mfcc, resample


@pytest.mark.parametrize("fi,fo,Ui,Uo,row", [(16000, 8000, 2, 1, 25), (8000, 16000, 1, 2, 13), (44100, 8000, 441, 80, 67),
                                             (48000, 8000, 6, 1, 73), (11025, 8000, 441, 320, 17)])
def test_table_geometry(fi, fo, Ui, Uo, row):
    ui, uo, first, ntaps, w = resample.tables(fi, fo)
    assert (ui, uo) == (Ui, Uo)
    assert first.dtype == np.int32 and ntaps.dtype == np.int32 and w.dtype == np.float32
    assert first.shape == ntaps.shape == (Uo,) and w.shape == (Uo, row) and int(ntaps.max()) == row
    f64, n64, _ = ref.weights64(fi, fo)
    assert first.tolist() == f64 and ntaps.tolist() == n64
    sums = w.astype(np.float64).sum(axis=1)
    assert 1.00003 <= sums.min() and sums.max() <= 1.0009
    assert resample.tables(fi, fo)[4] is w                    # cached per pair


def test_output_counts():
    assert resample.num_output_samples([0, 1, 2, 3, 4], 16000, 8000).tolist() == [0, 1, 1, 2, 2]
    assert resample.num_output_samples([0, 1, 2], 8000, 16000).tolist() == [0, 2, 4]
    assert resample.num_output_samples([0, 1, 5, 6, 441, 442], 44100, 8000).tolist() == [0, 1, 1, 2, 80, 81]
    # per-utterance rates in one call, and the plan's own counts
    assert resample.num_output_samples([4, 2, 442], [16000, 8000, 44100], [8000, 16000, 8000]).tolist() == [2, 4, 81]
    pl = resample.plan([4, 0, 442, 3000], [16000, 16000, 44100, 16000], 8000)
    assert pl.out_samples.tolist() == [2, 0, 81, 1500] and pl.pairs == [(16000, 8000), (44100, 8000)]
    assert pl.utt[0].tolist() == [0, 4, 4, 446] and pl.utt[2].tolist() == [0, 2, 2, 83] and pl.utt[4].tolist() == [0, 0, 1, 0]
    assert pl.tiles.tolist() == [[0, 0], [2, 0], [3, 0], [3, resample.OUT_TILE]]
    assert (pl.in_total, pl.out_total) == (3446, 1583)


def test_output_counts_beyond_int32():
    for fi, fo in ref.PAIRS:
        ns = [2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 33 + 12345, 2 ** 40 + 7]
        got = resample.num_output_samples(np.array(ns, np.int64), fi, fo)
        assert got.dtype == np.int64 and got.tolist() == [ref.num_output(n, fi, fo) for n in ns]
    assert int(resample.num_output_samples(2 ** 33, 8000, 16000)) == 2 ** 34


@pytest.mark.parametrize("fi,fo", ref.PAIRS)
def test_weights_against_the_fp64_formula(fi, fo):
    """Two fp32 roundings (filter and window, then product and quotient) plus the fp32 time argument: 4 ulp of the filter's peak
    value 2 cutoff / fi."""
    _, _, _, ntaps, w = resample.tables(fi, fo)
    _, _, rows = ref.weights64(fi, fo)
    tol = 4 * 2.0 ** -24 * (2 * ref.cutoff(fi, fo) / fi)
    worst = 0.0
    for p, row in enumerate(rows):
        assert len(row) == ntaps[p]
        worst = max(worst, float(np.abs(w[p, :len(row)].astype(np.float64) - np.array(row)).max()))
        assert not w[p, len(row):].any()
    print("%d -> %d: worst weight error %.3g of %.3g allowed" % (fi, fo, worst, tol))
    assert worst <= tol


def _tone(freq, fs, n=4000, amp=10000.0):
    return amp * np.sin(2 * math.pi * freq / fs * np.arange(n))


def _rms(v):
    return float(np.sqrt(np.mean(np.square(v))))


def test_pass_band_and_stop_band():
    """16 k -> 8 k on 4000 samples, middle half of the output: a 1 kHz tone keeps its rms, a 7 kHz tone (which would alias to
    1 kHz) is removed."""
    y, _, _ = ref.resample64(_tone(1000.0, 16000), 16000, 8000)
    assert len(y) == 2000
    mid = slice(len(y) // 4, 3 * len(y) // 4)
    rms_in = 10000.0 / math.sqrt(2.0)
    dev = abs(_rms(y[mid]) / rms_in - 1.0)
    print("1 kHz: rms deviation %.3g" % dev)
    assert dev <= 1e-3
    y7, _, _ = ref.resample64(_tone(7000.0, 16000), 16000, 8000)
    left = _rms(y7[mid]) / rms_in
    print("7 kHz: %.3g of the input rms left" % left)
    assert left <= 1e-3


def test_fmaf_chain_matches_fp64_on_exact_cases():
    """The ctypes fmaf chain is the fp32 arithmetic it claims to be: exact where every partial sum is representable (one tap per
    output), and within the recursive-sum bound of the fp64 sum elsewhere."""
    x = np.zeros(50, np.int16)
    x[20] = 16384
    y = ref.resample_chain(x, 16000, 8000)
    y64, mag, T = ref.resample64(x, 16000, 8000)
    assert np.array_equal(y.astype(np.float64), y64)
    rng = np.random.default_rng(0)
    x = rng.integers(-32768, 32768, 300).astype(np.int16)
    for fi, fo in ((16000, 8000), (8000, 16000)):
        y = ref.resample_chain(x, fi, fo)
        y64, mag, T = ref.resample64(x, fi, fo)
        assert np.all(np.abs(y.astype(np.float64) - y64) <= (T + 1) * 2.0 ** -24 * mag)


def test_check_takes_the_resampler_into_account():
    for kw in (dict(allow_downsample=True), dict(allow_upsample=True)):
        with pytest.raises(NotImplementedError):
            mfcc.MfccOptions(**kw).check()
        assert mfcc.MfccOptions(**kw).check(resample=True) is not None
    with pytest.raises(NotImplementedError):
        mfcc.MfccOptions(allow_downsample=True, htk_compat=True).check(resample=True)


def test_select_channel_outcomes(caplog):
    x = np.arange(2 * 8000, dtype=np.int16).reshape(2, 8000)
    base = dict(sample_frequency=8000.0, channel=0)
    with caplog.at_level(logging.WARNING, logger="mfcc"):
        # allowed: the channel, carrying its rate
        w = mfcc.select_channel("k", 16000, x, mfcc.MfccOptions(allow_downsample=True, **base))
        assert isinstance(w, mfcc.Wave) and w.rate == 16000 and np.array_equal(np.asarray(w), x[0]) and not caplog.records
        w = mfcc.select_channel("k", 4000, x, mfcc.MfccOptions(allow_upsample=True, **dict(base, channel=1)))
        assert w.rate == 4000 and np.array_equal(np.asarray(w), x[1]) and not caplog.records
        # a wave at the configured rate is a plain array whatever the options say
        w = mfcc.select_channel("k", 8000, x, mfcc.MfccOptions(allow_downsample=True, allow_upsample=True, **base))
        assert type(w) is np.ndarray and not caplog.records
        # the other direction only: Kaldi's message, a warning and a skip
        assert mfcc.select_channel("k", 4000, x, mfcc.MfccOptions(allow_downsample=True, **base)) is None
        assert "Waveform and config sample Frequency mismatch: 4000 .vs 8000" in caplog.text
        assert "(use --allow-upsample=true to allow upsampling)" in caplog.text and "--allow-downsample" not in caplog.text
        caplog.clear()
        assert mfcc.select_channel("k", 16000, x, mfcc.MfccOptions(allow_upsample=True, **base)) is None
        assert "Waveform and config sample Frequency mismatch: 16000 .vs 8000" in caplog.text
        assert "(use --allow-downsample=true to allow downsampling)" in caplog.text and "--allow-upsample" not in caplog.text
        caplog.clear()
        # both off: the warning and the skip of before
        assert mfcc.select_channel("k", 16000, x, mfcc.MfccOptions(**base)) is None
        assert "Sample frequency 16000 of key k differs from --sample-frequency=8000; skipping (no resampling)" in caplog.text
        caplog.clear()
        # --min-duration looks at the original length at the original rate: 8000 samples are 0.5 s at 16 kHz
        assert mfcc.select_channel("k", 16000, x, mfcc.MfccOptions(allow_downsample=True, min_duration=0.6, **base)) is None
        assert "too short (0.5 sec)" in caplog.text
        assert mfcc.select_channel("k", 16000, x, mfcc.MfccOptions(allow_downsample=True, min_duration=0.4, **base)) is not None
