"""Host side of the MFCC + VAD front-end (no GPU): the oracle's frame geometry, the mel-table support, every table (window, mel
bank, lifter x DCT, twiddles) against fp64 definitions written without the product, Philox against the Random123 known-answer
vectors, the --config parser, the WAV reader and the CLI's argument errors."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import mfcc_ref
from conftest import GOLDEN, TWIN
from xvector_amd import mfcc


def recipe():
    return mfcc.MfccOptions().update(mfcc.read_config(os.path.join(GOLDEN, "mfcc.conf")))


@pytest.mark.parametrize("snip", [True, False])
def test_frame_counts_and_starts(snip):
    o = recipe().update([("snip_edges", snip)])
    assert (o.frame_length_samples, o.frame_shift_samples, o.padded_length) == (200, 80, 256)
    Ns = [0, 1, 40, 199, 200, 201, 80001]
    want = [0, 0, 0, 0, 1, 1, 998] if snip else [0, 0, 1, 2, 3, 3, 1000]
    assert o.num_frames(Ns).tolist() == want
    assert o.first_sample([0, 1, 2]).tolist() == ([0, 80, 160] if snip else [-60, 20, 100])


def test_reflected_indices():
    o = recipe()
    idx = mfcc_ref.frame_indices(o, 40)                 # a 40-sample utterance gives one frame at 8 kHz
    assert idx.shape == (1, 200) and idx.min() >= 0 and idx.max() < 40
    # start -60: -60 -> 59 -> 2*40-1-59 = 20
    assert idx[0, 0] == 20 and idx[0, 59] == 0 and idx[0, 60] == 0 and idx[0, 99] == 39 and idx[0, 100] == 39
    idx = mfcc_ref.frame_indices(o.update([("snip_edges", False)]), 1000)
    assert idx[0, 59] == 0 and idx[0, 58] == 1 and idx[-1, -1] <= 999


def test_mel_support_pins():
    f, w, n = mfcc.mel_banks(recipe())
    assert f.tolist() == [1, 3, 5, 7, 9, 12, 14, 17, 20, 24, 27, 31, 35, 40, 44, 50, 55, 61, 68, 75, 82, 90, 99]
    assert (f + n - 1).tolist() == [4, 6, 8, 11, 13, 16, 19, 23, 26, 30, 34, 39, 43, 49, 54, 60, 67, 74, 81, 89, 98, 108, 118]
    o = mfcc.MfccOptions()
    assert o.padded_length == 512
    f, w, n = mfcc.mel_banks(o)
    assert f.tolist() == [1, 4, 6, 10, 13, 17, 21, 26, 31, 37, 43, 50, 58, 67, 77, 87, 99, 113, 127, 144, 162, 182, 204]
    assert (f + n - 1).tolist() == [5, 9, 12, 16, 20, 25, 30, 36, 42, 49, 57, 66, 76, 86, 98, 112, 126, 143, 161, 181, 203, 228, 255]
    assert (f + n).max() <= 256 and (w >= 0).all() and (w <= 1).all()


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32_10."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for c, k, want in kat:
        got = mfcc_ref.philox4x32_10(*c, *k)
        assert [int(x) for x in got] == list(want)


def test_dither_noise_statistics_and_key():
    g = mfcc_ref.gauss(mfcc.dither_key("spk1-utt1", 0), np.arange(400)[:, None], np.arange(200)[None, :])
    assert abs(g.mean()) < 0.01 and abs(g.std() - 1) < 0.01
    assert mfcc.fnv1a64("") == 0xCBF29CE484222325 and mfcc.fnv1a64("a") == 0xAF63DC4C8601EC8C
    assert mfcc.dither_key("a", 5) == 0xAF63DC4C8601EC8C ^ 5


def test_config_parser_on_the_recipe_files():
    o = recipe()
    assert (o.sample_frequency, o.frame_length, o.low_freq, o.high_freq, o.num_ceps, o.snip_edges) == (8000, 25, 20, 3700, 23, False)
    assert (o.dither, o.num_mel_bins, o.window_type) == (1.0, 23, "povey")            # Kaldi's defaults where the file is silent
    v = mfcc.VadOptions().update(mfcc.read_config(os.path.join(GOLDEN, "vad.conf")))
    assert (v.vad_energy_threshold, v.vad_energy_mean_scale, v.vad_proportion_threshold, v.vad_frames_context) == (5.5, 0.5, 0.12, 2)
    assert (mfcc.VadOptions().vad_energy_threshold, mfcc.MfccOptions().num_ceps, mfcc.MfccOptions().snip_edges) == (5.0, 13, True)


def test_config_parser_rules():
    p = mfcc.parse_config_lines(["# a comment", "--snip-edges   # bare flag", "--use-energy=f", "  --dither=0 # x", ""])
    o = mfcc.MfccOptions().update(p)
    assert o.snip_edges is True and o.use_energy is False and o.dither == 0.0
    for v, want in (("true", True), ("t", True), ("1", True), ("false", False), ("F", False), ("0", False)):
        assert mfcc.MfccOptions().update([("raw-energy", v)]).raw_energy is want
    with pytest.raises(ValueError):
        mfcc.MfccOptions().update(mfcc.parse_config_lines(["--no-such-option=1"]))
    with pytest.raises(ValueError):
        mfcc.MfccOptions().update([("raw-energy", "maybe")])
    with pytest.raises(ValueError):
        mfcc.parse_config_lines(["snip-edges=false"])
    for bad in (dict(round_to_power_of_two=False), dict(htk_compat=True), dict(vtln_warp=0.9), dict(allow_downsample=True)):
        with pytest.raises(NotImplementedError):
            mfcc.MfccOptions(**bad).check()


def test_tables():
    o = recipe()
    t = mfcc.MfccTables(o)
    assert t.window.dtype == np.float32 and t.window.shape == (200,) and t.window[0] == 0 and abs(t.window[100] - 1) < 1e-3
    assert t.lifter_dct.shape == (23, 23) and abs(t.lifter_dct[0, 0] - np.sqrt(1 / 23)) < 1e-7
    assert t.twiddle.shape == (128, 2) and t.twiddle[64, 0] == np.float32(np.cos(-np.pi / 2)) and t.twiddle[64, 1] == -1


# ------------------------------------------------------------------------------------------------
# the tables against definitions written without the product (mfcc_ref.window64 / mel_dense64 / lifter_dct64 / twiddle64)
# ------------------------------------------------------------------------------------------------
# (sample frequency, frame length in ms) -> (samples, padded): every padded length at every rate, with and without zero padding
GEOMETRY = {(8000, 10): (80, 128), (8000, 16): (128, 128), (8000, 25): (200, 256), (8000, 64): (512, 512), (8000, 100): (800, 1024),
            (16000, 8): (128, 128), (16000, 10): (160, 256), (16000, 25): (400, 512), (16000, 32): (512, 512), (16000, 64): (1024, 1024),
            (32000, 3): (96, 128), (32000, 8): (256, 256), (32000, 12): (384, 512), (32000, 25): (800, 1024), (32000, 32): (1024, 1024)}
WINDOWS = [(w, 0.42) for w in mfcc.WINDOW_TYPES] + [("blackman", 0.40)]
BINS = (10, 13, 23, 40, 65, 80, 128)
ABS0 = 1e-14            # entries that are exactly 0 in one statement and ~1e-15 in the other (cos pi/2)
# reference against scipy, both fp64: a cosine's argument of size x, formed by a few roundings, is off by a few x 2^-53, and the
# cosine moves by as much.  Windows: x <= 4 pi, amplitude <= 1.  DCT: the reference reduces its angle below 2 pi, amplitude
# sqrt(2/B) <= 0.45, and scipy's FFT-based transform of a unit vector is as exact; the same allowance serves.
WIN_TOL = 8 * 4 * np.pi * 2.0 ** -53
DCT_TOL = WIN_TOL


def _geometry(fs, ms, **kw):
    o = mfcc.MfccOptions(sample_frequency=fs, frame_length=ms, **kw)
    assert (o.frame_length_samples, o.padded_length) == GEOMETRY[(fs, ms)]
    return o


def _rounded_once(table, ref):
    """An fp32 table formed in fp64 and rounded once lies within half an fp32 ulp of the independent fp64 value."""
    assert table.dtype == np.float32 and table.shape == ref.shape
    err = np.abs(table.astype(np.float64) - ref)
    bound = mfcc_ref.half_ulp32(ref) + ABS0
    assert (err <= bound).all(), (float((err / bound).max()), np.unravel_index(np.argmax(err / bound), err.shape))


@pytest.mark.parametrize("window,coeff", WINDOWS)
@pytest.mark.parametrize("fs,ms", sorted(GEOMETRY))
def test_window_against_the_definition(fs, ms, window, coeff):
    o = _geometry(fs, ms, window_type=window, blackman_coeff=coeff)
    _rounded_once(mfcc.window_function(o), mfcc_ref.window64(window, o.frame_length_samples, coeff))


@pytest.mark.parametrize("Q", [0.0, 22.0, 30.0])
@pytest.mark.parametrize("B", BINS)
def test_lifter_dct_against_the_definition(B, Q):
    for C in sorted({1, 13, B}):
        if C > B:
            continue
        o = mfcc.MfccOptions(num_mel_bins=B, num_ceps=C, cepstral_lifter=Q)
        _rounded_once(mfcc.lifter_dct(o), mfcc_ref.lifter_dct64(B, C, Q))


@pytest.mark.parametrize("fs,ms", sorted(GEOMETRY))
def test_twiddles_against_the_definition(fs, ms):
    o = _geometry(fs, ms)
    _rounded_once(mfcc.twiddles(o), mfcc_ref.twiddle64(o.padded_length))


def test_tables_object_holds_the_builders_output():
    """``MfccTables`` (what is uploaded) is the builders' output, bit for bit."""
    o = _geometry(32000, 25, num_mel_bins=80, num_ceps=80, high_freq=-400.0, window_type="blackman", blackman_coeff=0.40)
    t = mfcc.MfccTables(o)
    f, w, n = mfcc.mel_banks(o)
    for got, want in ((t.window, mfcc.window_function(o)), (t.lifter_dct, mfcc.lifter_dct(o)), (t.twiddle, mfcc.twiddles(o)),
                      (t.mel_first, f), (t.mel_w, w), (t.mel_len, n)):
        assert got.dtype == want.dtype and np.array_equal(got, want)


def _mel_dense32(first, w, length, half):
    B = len(first)
    assert w.dtype == np.float32 and w.shape[0] == B and w.shape[1] == int(length.max())
    W = np.zeros((half, B), np.float64)
    inside = np.zeros((half, B), bool)
    for b in range(B):
        f, n = int(first[b]), int(length[b])
        assert n >= 1 and f >= 0 and f + n <= half, (b, f, n)
        assert not w[b, n:].any(), b                                  # nothing past the band's length
        W[f:f + n, b] = w[b, :n]
        inside[f:f + n, b] = True
    return W, inside


@pytest.mark.parametrize("fs,ms", sorted(GEOMETRY))
def test_mel_bank_against_the_definition(fs, ms):
    """The fp32 bank (Kaldi forms it in fp32) against the fp64 definition.  Bound: a mel value of size up to mel(high), rounded
    to fp32 (2^-24 relative), divided by the band's half-width delta, times 8 for the few operations involved, plus 2 roundings of
    the weight itself: 2^-24 (2 + 8 mel(high) / delta)."""
    N = GEOMETRY[(fs, ms)][1]
    accepted = refused = 0
    worst = 0.0
    for B in BINS:
        for low in (0.0, 20.0, 300.0):
            for high in (0.0, -400.0, 3700.0):
                o = _geometry(fs, ms, num_mel_bins=B, low_freq=low, high_freq=high)
                W64 = mfcc_ref.mel_dense64(fs, N, B, low, high)
                mlo, mhi = mfcc_ref.mel_range64(fs, low, high)
                bound = 2.0 ** -24 * (2.0 + 8.0 * mhi / ((mhi - mlo) / (B + 1)))
                what = (fs, N, B, low, high)
                try:
                    first, w, length = mfcc.mel_banks(o)
                except ValueError as e:
                    # a refusal is right only where the definition leaves some band without a bin too
                    assert "has no FFT bin" in str(e) and (W64.max(axis=0) <= bound).any(), what
                    refused += 1
                    continue
                accepted += 1
                W32, inside = _mel_dense32(first, w, length, N // 2)
                err = np.abs(W32 - W64)
                worst = max(worst, float(err.max() / bound))
                assert (err <= bound).all(), (what, float(err.max() / bound))
                assert (W32 >= 0).all() and (W32 <= 1).all(), what
                assert (W64[(W32 > 0) != (W64 > 0)] < bound).all(), what       # the supports differ only in negligible weights
                assert (W64[~inside] < bound).all(), what                      # and nothing of weight lies outside a stored row
                assert (W32.max(axis=0) > 0).all(), what
    print("mel bank fs %d N %d: worst error / bound %.3f, %d accepted, %d refused" % (fs, N, worst, accepted, refused))
    assert accepted >= 9                                                       # the grid is not refused away


def test_too_many_mel_bins_are_refused():
    with pytest.raises(ValueError, match=r"mel band \d+ has no FFT bin"):
        mfcc.mel_banks(mfcc.MfccOptions(num_mel_bins=128))
    with pytest.raises(ValueError, match=r"mel band \d+ has no FFT bin"):
        mfcc.MfccTables(mfcc.MfccOptions(num_mel_bins=128))


def test_reference_dct_against_scipy():
    fft = pytest.importorskip("scipy.fft")
    for B in BINS:
        for C in sorted({1, 13, B}):
            if C <= B:
                want = fft.dct(np.eye(B), type=2, norm="ortho", axis=0)[:C]
                assert np.abs(mfcc_ref.dct64(B, C) - want).max() <= DCT_TOL
                assert np.array_equal(mfcc_ref.lifter_dct64(B, C, 0.0), mfcc_ref.dct64(B, C))
    # the lifter: 1 at k = 0, 1 + Q/2 at k = Q/2, 1 again at k = Q
    assert mfcc_ref.lifter64(23, 22.0)[0] == 1.0 and mfcc_ref.lifter64(23, 22.0)[11] == 12.0
    assert abs(mfcc_ref.lifter64(23, 22.0)[22] - 1.0) <= 1e-14 and mfcc_ref.lifter64(31, 30.0)[15] == 16.0


def test_reference_windows_against_scipy():
    windows = pytest.importorskip("scipy.signal.windows")
    for L in sorted({v[0] for v in GEOMETRY.values()}):
        hann = windows.hann(L)                                                 # symmetric, as Kaldi's
        assert np.abs(mfcc_ref.window64("hanning", L) - hann).max() <= WIN_TOL
        assert np.abs(mfcc_ref.window64("hamming", L) - windows.hamming(L)).max() <= WIN_TOL
        assert np.abs(mfcc_ref.window64("blackman", L, 0.42) - windows.blackman(L)).max() <= WIN_TOL
        assert np.abs(mfcc_ref.window64("povey", L) - np.maximum(hann, 0.0) ** 0.85).max() <= WIN_TOL
        assert (mfcc_ref.window64("rectangular", L) == 1.0).all()
        sine = mfcc_ref.window64("sine", L)                                    # scipy's cosine window is another one
        assert np.abs(sine * sine - hann).max() <= WIN_TOL                       # sin^2(pi x) = 1/2 - 1/2 cos(2 pi x)


def test_wav_reader_formats():
    rng = np.random.default_rng(0)
    x = rng.integers(-32768, 32767, (2, 1001)).astype(np.int16)
    for kw in (dict(), dict(extensible=True), dict(streaming=True), dict(extra_chunks=[(b"LIST", b"abc"), (b"junk", b"12345678")])):
        rate, y = mfcc.read_wav(mfcc.wav_bytes(x, 8000, **kw))
        assert rate == 8000 and np.array_equal(y, x)
    b = mfcc.wav_bytes(x[0], 16000)
    b0 = b[:40] + struct.pack("<I", 0) + b[44:]                       # data size 0: read to the end
    assert np.array_equal(mfcc.read_wav(b0)[1][0], x[0])
    with pytest.raises(mfcc.WavError):
        mfcc.read_wav(b[:-10])                                       # truncated
    for bits in (8, 24):
        bad = bytearray(b)
        bad[34:36] = struct.pack("<H", bits)
        with pytest.raises(mfcc.WavError, match="%d-bit" % bits):
            mfcc.read_wav(bytes(bad), "k1")
    bad = bytearray(b)
    bad[20:22] = struct.pack("<H", 3)                                 # IEEE float
    with pytest.raises(mfcc.WavError, match="format tag"):
        mfcc.read_wav(bytes(bad))


def test_channel_duration_and_rate_rules():
    x = np.arange(16000, dtype=np.int16).reshape(2, 8000)
    o = recipe()
    assert np.array_equal(mfcc.select_channel("k", 8000, x, o), x[0])            # --channel=-1 on stereo: channel 0
    assert np.array_equal(mfcc.select_channel("k", 8000, x, o.update([("channel", 1)])), x[1])
    assert mfcc.select_channel("k", 8000, x, o.update([("channel", 2)])) is None
    assert mfcc.select_channel("k", 16000, x, recipe()) is None
    assert mfcc.select_channel("k", 8000, x, recipe().update([("min_duration", 1.5)])) is None


def test_wav_scp_paths_and_pipes(tmp_path):
    w = np.arange(500, dtype=np.int16)
    p = tmp_path / "a.wav"
    p.write_bytes(mfcc.wav_bytes(w, 8000))
    (tmp_path / "wav.scp").write_text("a %s\nb cat %s |\nc cat %s/missing.wav |\n" % (p, p, tmp_path))
    entries = list(mfcc.read_wav_scp(str(tmp_path / "wav.scp")))
    assert [k for k, _ in entries] == ["a", "b", "c"]
    for k, rx in entries[:2]:
        assert np.array_equal(mfcc.load_wav(k, rx)[1][0], w)
    with pytest.raises(mfcc.WavError, match="c: command"):
        mfcc.load_wav(*entries[2])


def _cli(args):
    return subprocess.run([sys.executable, os.path.join(TWIN, "mfcc_vad.py")] + args, stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, timeout=120)


def test_cli_errors_before_any_device_use(tmp_path):
    conf = tmp_path / "bad.conf"
    conf.write_text("--num-ceps=23\n--frobnicate=1 # no such option\n")
    (tmp_path / "wav.scp").write_text("")
    out = "ark,scp:%s/f.ark,%s/f.scp" % (tmp_path, tmp_path)
    p = _cli(["compute-mfcc-feats", "--config=%s" % conf, "scp:%s/wav.scp" % tmp_path, out])
    assert p.returncode != 0 and b"frobnicate" in p.stdout
    p = _cli(["compute-mfcc-feats", "--htk-compat=true", "scp:%s/wav.scp" % tmp_path, out])
    assert p.returncode != 0 and b"htk-compat" in p.stdout
    p = _cli(["compute-mfcc-feats", "scp:%s/wav.scp" % tmp_path, "ark,t,scp:x"])
    assert p.returncode != 0
    p = _cli(["compute-vad", "--vad-frames-context=x", "scp:nothing.scp", out])
    assert p.returncode != 0 and b"vad-frames-context" in p.stdout
    p = _cli(["compute-mfcc-feats", "ark:wav.scp", out])
    assert p.returncode != 0 and b"scp:wav.scp" in p.stdout
