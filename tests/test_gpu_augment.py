"""wav-reverberate on the GPU (csrc/xv_augment.hip, xvector_amd/augment.py) against the fp64 oracle (tests/augment_ref.py) under
the bound of DESIGN.md §8.7, the bitwise independence of an utterance from its batch, NaN canaries around the written rows, and
stage 2 end to end through compute-mfcc-feats, wav-to-duration and make_mfcc_mi355x.sh."""
import math
import os
import shlex
import subprocess
import sys

import numpy as np
import pytest

import augment_ref
from conftest import ROOT, TWIN

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -23
EPS64 = 2.0 ** -52
FS = 8000
WORST = {}


@pytest.fixture(scope="module")
def env():
    import torch
    from xvector_amd import augment, hiplib, mfcc, synthetic
    hiplib.require_gpu()
    yield dict(torch=torch, augment=augment, mfcc=mfcc, synthetic=synthetic)
    print("\nworst error / bound ratio: " + ", ".join("%s %.3e" % kv for kv in sorted(WORST.items())))


def _wav(env, path, x, fs=FS):
    with open(path, "wb") as f:
        f.write(env["mfcc"].wav_bytes(x, fs))
    return str(path)


def rir_like(L, seed, peak=None):
    """A room-like impulse response in int16: a direct-path peak, then exponentially decaying noise."""
    rng = np.random.default_rng(seed)
    peak = min(L - 1, L // 10) if peak is None else peak
    t = np.arange(L)
    h = rng.standard_normal(L) * 6000.0 * np.exp(-np.maximum(t - peak, 0) / max(L / 6.0, 1.0))
    h[:peak] *= 0.05
    h[peak] = 30000.0
    return np.clip(np.rint(h), -32767, 32767).astype(np.int16)


def speech(env, n, seed):
    return env["synthetic"].speech_like_wave(n, FS, seed)


def window_norm(x, L):
    """||x[n - L + 1 .. n]||_2 for n in [0, N + L - 1)."""
    c = np.concatenate([[0.0], np.cumsum(np.asarray(x, np.float64) ** 2)])
    n = np.arange(len(x) + L - 1)
    hi = np.minimum(n + 1, len(x))
    lo = np.maximum(n - L + 1, 0)
    return np.sqrt(np.maximum(c[hi] - c[lo], 0.0))


def check(env, tmp_path, name, x, rir=None, noises=(), snrs=(), times=(), **opts):
    """One evaluation through the real entry form; scalars, waveform and int16 output against the oracle."""
    augment = env["augment"]
    args = ["wav-reverberate"]
    for k, v in opts.items():
        args.append("--%s=%s" % (k.replace("_", "-"), str(v).lower() if isinstance(v, bool) else v))
    if rir is not None:
        args.append("--impulse-response=%s" % _wav(env, tmp_path / ("%s_rir.wav" % name), rir))
    if noises:
        paths = [_wav(env, tmp_path / ("%s_n%d.wav" % (name, i)), n) for i, n in enumerate(noises)]
        args += ["--additive-signals=" + ",".join(paths), "--snrs=" + ",".join(map(str, snrs)),
                 "--start-times=" + ",".join(map(str, times))]
    args += [_wav(env, tmp_path / ("%s_x.wav" % name), x), "-", "|"]
    node = augment.parse_rx(" ".join(args))
    waves, info, _ = augment.Augmenter().evaluate([(name, node)], debug=True)
    got, inf = waves[0], info[0]
    ref = augment_ref.reverberate(x, FS, rir, noises, [float(np.float32(s)) for s in snrs], times,
                                  shift_output=opts.get("shift_output", False), volume=opts.get("volume", 0.0),
                                  duration=opts.get("duration", 0.0), normalize_output=opts.get("normalize_output", True))
    for k in ("P0", "E", "P1", "level"):
        assert inf[k] == pytest.approx(ref[k], rel=1e-6), (name, k)
    np.testing.assert_allclose(inf["noise_power"], ref["noise_power"], rtol=1e-6)
    np.testing.assert_allclose(inf["noise_scale"], ref["noise_scale"], rtol=1e-6)
    # the waveform before the level: exact products, fp64 sums -> far inside the fp32 bound of the issue
    y, yr = inf["y"], ref["y"]
    assert y.shape == yr.shape
    bound = np.zeros_like(yr)
    if rir is not None:
        L = len(rir)
        hn = float(np.linalg.norm(np.asarray(rir, np.float64) / 32768.0))
        bound += 16 * EPS32 * math.ceil(math.log2(2 * L)) * hn * window_norm(x, L)
    for n, s, t in zip(noises, ref["noise_scale"], times):
        off = int(np.float32(t) * np.float32(FS))
        k = max(0, min(len(yr) - off, len(n)))
        bound[off:off + k] += 2 * EPS32 * abs(s) * np.abs(np.asarray(n[:k], np.float64))
    bound += 4 * EPS64 * (np.abs(yr) + 1.0)
    if rir is not None and len(x) * len(rir) > 5e7:              # the oracle's own fp64 FFT rounding
        hn = float(np.linalg.norm(np.asarray(rir, np.float64) / 32768.0))
        bound += 8 * EPS64 * math.log2(2 * (len(x) + len(rir))) * hn * float(np.linalg.norm(np.asarray(x, np.float64)))
    err = np.abs(y - yr)
    WORST["waveform"] = max(WORST.get("waveform", 0.0), float((err / bound).max()))
    assert (err <= bound).all(), (name, float((err / bound).max()))
    if rir is not None and not noises and len(x) * len(rir) <= 5e7:
        # reverberation alone, within the oracle's direct form: the convolution is exact (int16 taps / 32768, partial sums below
        # 2^53 on the 2^-15 grid), so the waveform equals the integer convolution bit for bit
        exact = np.convolve(np.asarray(x, np.int64), np.asarray(rir, np.int64)).astype(np.float64) * 2.0 ** -15
        assert np.array_equal(y, exact), (name, np.flatnonzero(y != exact)[:8])
    # int16: equal except where the oracle's value lies within the propagated bound of a truncation boundary
    assert got.dtype == np.int16 and got.shape == ref["out"].shape, name
    pre = ref["pre"]
    pb = ref["level"] * bound[ref["idx"]] + 2 * EPS32 * np.abs(pre)
    near = np.abs(pre - np.rint(pre)) <= pb
    diff = got.astype(np.int32) - ref["out"]
    assert (np.abs(diff) <= 1).all() and not diff[~near].any(), name
    assert np.count_nonzero(diff) <= 1e-4 * len(got), (name, np.count_nonzero(diff))
    assert inf["clipped"] == ref["clipped"] or np.count_nonzero(diff), name
    return got, inf, ref


@pytest.mark.parametrize("L", [1, 7, 409, 4097, 8000, 2 ** 15 + 3])
def test_reverb_long_input(env, tmp_path, L):
    x = speech(env, 5 * FS + 123, L)
    check(env, tmp_path, "long%d" % L, x, rir_like(L, L), shift_output=True)


@pytest.mark.parametrize("L", [409, 8000, 2 ** 15 + 3, 2 ** 20])
def test_reverb_input_shorter_than_rir(env, tmp_path, L):
    x = speech(env, min(L - 1, 3 * FS), 7 + L)
    check(env, tmp_path, "short%d" % L, x, rir_like(L, L + 1), shift_output=L % 2 == 1)


def test_reverb_without_shift(env, tmp_path):
    check(env, tmp_path, "noshift", speech(env, 2 * FS, 3), rir_like(4000, 3, peak=900), shift_output=False)


def test_noises_shorter_longer_and_past_the_end(env, tmp_path):
    x = speech(env, 3 * FS, 11)
    n1 = speech(env, FS // 2, 12)                    # shorter than y
    n2 = speech(env, 6 * FS, 13)                     # longer than y
    n3 = speech(env, FS, 14)                         # starts past the end
    check(env, tmp_path, "noises", x, rir_like(3000, 5), [n1, n2, n3], [10, 5, 0], [0.7, 0.0, 9.0], shift_output=True)


def test_noise_without_rir_and_volume(env, tmp_path):
    x = speech(env, 2 * FS, 21)
    check(env, tmp_path, "vol", x, None, [speech(env, FS, 22), speech(env, FS, 23)], [15, 3], [0.25, 1.5], volume=0.5)


def test_duration_repeat_and_trim(env, tmp_path):
    x = speech(env, FS + 77, 31)
    check(env, tmp_path, "rep", x, None, duration=3.7)
    check(env, tmp_path, "rep_rir", x, rir_like(2000, 6), duration=2.9, shift_output=True)
    check(env, tmp_path, "trim", x, rir_like(2000, 7), duration=0.3, shift_output=True)


def test_saturation(env, tmp_path):
    x = np.full(4000, 30000, np.int16)
    _, inf, ref = check(env, tmp_path, "sat", x, None, volume=1.5)
    assert ref["clipped"] == 4000 and inf["clipped"] == 4000


def test_exact_truncation_boundaries(env, tmp_path):
    """Samples that land exactly on +-32768, -32770, +-0.5 and +-1.5 before the write: the GPU output equals the oracle's."""
    for name, x, vol, want in (("b2", [16384, -16384, -16385, 16383, 3], 2.0, [32767, -32768, -32768, 32766, 6]),
                               ("b05", [1, -1, 3, -3, 32767], 0.5, [0, 0, 1, -1, 16383])):
        got, inf, ref = check(env, tmp_path, name, np.array(x, np.int16), None, volume=vol)
        assert list(got) == want == list(ref["out"]) and inf["clipped"] == ref["clipped"]


def test_empty_noise_keeps_the_noise_list_aligned(env, tmp_path):
    x = speech(env, 2 * FS, 71)
    empty = np.zeros(0, np.int16)
    _, inf, ref = check(env, tmp_path, "empty", x, rir_like(900, 8), [speech(env, FS, 72), empty, speech(env, FS, 73)],
                        [10, 5, 0], [0.1, 0.2, 0.3], shift_output=True)
    assert len(inf["noise_power"]) == len(inf["noise_scale"]) == 3
    assert inf["noise_power"][1] == 0 and inf["noise_scale"][1] == 0 and inf["noise_scale"][0] > 0 and inf["noise_scale"][2] > 0


def test_nested_duration_noises(env, tmp_path):
    """The background form: each noise a nested wav-reverberate --duration, evaluated in-process one level earlier."""
    augment = env["augment"]
    x = speech(env, 2 * FS + 5, 41)
    s1, s2 = speech(env, FS // 3, 42), speech(env, FS, 43)
    px, p1, p2 = (_wav(env, tmp_path / n, a) for n, a in (("x.wav", x), ("s1.wav", s1), ("s2.wav", s2)))
    rx = ("wav-reverberate --shift-output=true --additive-signals='wav-reverberate --duration=2.0 \"%s\" - |,"
          "wav-reverberate --duration=2.0 \"%s\" - |' --start-times='0,0' --snrs='19,13' %s - |" % (p1, p2, px))
    waves, info, _ = augment.Augmenter().evaluate([("bg", augment.parse_rx(rx))])
    M = int(np.float32(2.0) * np.float32(FS))
    n1 = augment_ref.reverberate(s1, FS, duration=2.0)["out"]
    n2 = augment_ref.reverberate(s2, FS, duration=2.0)["out"]
    assert len(n1) == M and (n1[:len(s1)] == s1).all() and (n1[len(s1):2 * len(s1)] == s1).all()
    ref = augment_ref.reverberate(x, FS, None, [n1, n2], [19.0, 13.0], [0.0, 0.0])
    np.testing.assert_allclose(info[0]["noise_power"], ref["noise_power"], rtol=1e-6)
    np.testing.assert_allclose(info[0]["noise_scale"], ref["noise_scale"], rtol=1e-6)
    diff = waves[0].astype(np.int32) - ref["out"]
    assert np.abs(diff).max() <= 1 and np.count_nonzero(diff) <= 1e-4 * len(diff)


def _entries(env, tmp_path):
    """A mixed batch in the recipe's forms: reverb with a piped RIR, pipe input, foreground noises, nested background noises."""
    d = tmp_path / "src"
    d.mkdir(exist_ok=True)
    x = [speech(env, int(FS * s), 50 + i) for i, s in enumerate((2.3, 4.1, 1.7, 3.3))]
    px = [_wav(env, d / ("u%d.wav" % i), a) for i, a in enumerate(x)]
    rir = _wav(env, d / "rir.wav", rir_like(3000, 9))
    noise = [_wav(env, d / ("n%d.wav" % i), speech(env, FS * (i + 1), 60 + i)) for i in range(2)]
    return [
        ("u0-reverb", "wav-reverberate --shift-output=true --impulse-response=\"cat %s |\" %s - |" % (rir, px[0])),
        ("u1-reverb", "cat %s | wav-reverberate --shift-output=true --impulse-response=\"cat %s |\" - - |" % (px[1], rir)),
        ("u2-noise", "wav-reverberate --shift-output=true --additive-signals='%s,%s' --start-times='0,0.51' --snrs='10,5' %s - |"
         % (noise[0], noise[1], px[2])),
        ("u3-babble", "wav-reverberate --shift-output=true --additive-signals='wav-reverberate --duration=3.3 \"%s\" - |,"
         "wav-reverberate --duration=3.3 \"%s\" - |' --start-times='0,0' --snrs='19,13' %s - |" % (noise[0], noise[1], px[3])),
    ]


def test_batch_independence_and_canaries(env, tmp_path):
    torch, augment = env["torch"], env["augment"]
    entries = _entries(env, tmp_path)
    aug = augment.Augmenter()
    alone = [aug.evaluate([(k, augment.parse_rx(rx))])[0][0] for k, rx in entries]
    plan = aug.plan([(k, augment.parse_rx(rx)) for k, rx in entries])
    lens = plan.lengths()
    gap = 1000
    offs = np.cumsum([gap] + [n + gap for n in lens])[:-1]
    out = torch.full((int(offs[-1] + lens[-1] + gap),), float("nan"), dtype=torch.float32, device="cuda")
    aug.run(plan, out, offs, sample_format=1)
    o = out.cpu().numpy()
    written = np.zeros(len(o), bool)
    for a, n, ref in zip(offs, lens, alone):
        seg = o[a:a + n]
        assert np.array_equal(seg, ref.astype(np.float32))            # bit for bit, alone or in a mixed batch, int16 or fp32
        written[a:a + n] = True
    assert np.isnan(o[~written]).all()


def _run(args, **kw):
    return subprocess.run([sys.executable] + args, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, **kw)


def test_cli_end_to_end(env, tmp_path):
    mfcc = env["mfcc"]
    entries = _entries(env, tmp_path)
    data = tmp_path / "data"
    data.mkdir()
    with open(data / "wav.scp", "w") as f:
        for k, rx in entries:
            f.write("%s %s\n" % (k, rx))
    # a wav-reverberate first on PATH that would leave a marker: it must never run
    stub = tmp_path / "bin"
    stub.mkdir()
    marker = tmp_path / "stub_ran"
    with open(stub / "wav-reverberate", "w") as f:
        f.write("#!/bin/sh\ntouch %s\nexit 1\n" % marker)
    os.chmod(stub / "wav-reverberate", 0o755)
    envv = dict(os.environ, PATH="%s:%s" % (stub, os.environ.get("PATH", "")))
    conf = os.path.join(ROOT, "tests", "golden", "mfcc.conf")
    tool = os.path.join(TWIN, "mfcc_vad.py")
    _run([tool, "compute-mfcc-feats", "--config=" + conf, "--write-num-frames=ark,t:%s" % (tmp_path / "nf"),
          "scp:%s" % (data / "wav.scp"), "ark:%s" % (tmp_path / "aug.ark")], env=envv)
    # the same entries through wav_reverberate.py into WAV files, then the clean path
    clean = tmp_path / "clean.scp"
    with open(clean, "w") as f:
        for k, rx in entries:
            stages = env["augment"].split_pipeline(rx.rstrip()[:-1])
            argv = shlex.split(stages[-1])[1:]
            wav = tmp_path / ("%s.wav" % k)
            if len(stages) > 1:                                   # pipe input: feed the earlier stages' WAV on stdin
                src = subprocess.run("|".join(stages[:-1]), shell=True, check=True, stdout=subprocess.PIPE).stdout
                _run([os.path.join(TWIN, "wav_reverberate.py")] + argv[:-1] + [str(wav)], input=src, env=envv)
            else:
                _run([os.path.join(TWIN, "wav_reverberate.py")] + argv[:-1] + [str(wav)], env=envv)
            f.write("%s %s\n" % (k, wav))
    _run([tool, "compute-mfcc-feats", "--config=" + conf, "scp:%s" % clean, "ark:%s" % (tmp_path / "clean.ark")], env=envv)
    assert not marker.exists()
    import kaldi_io
    a = dict(kaldi_io.read_mat_ark(str(tmp_path / "aug.ark")))
    b = dict(kaldi_io.read_mat_ark(str(tmp_path / "clean.ark")))
    assert sorted(a) == sorted(b) == sorted(k for k, _ in entries)
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k
    # wav-to-duration: the augmented entries' lengths without the GPU, equal to what the features were computed from
    _run([tool, "wav-to-duration", "--read-entire-file", "scp:%s" % (data / "wav.scp"), "ark,t:%s" % (tmp_path / "utt2dur")],
         env=envv)
    opts = mfcc.MfccOptions().update(mfcc.read_config(conf))
    nf = dict(l.split() for l in open(tmp_path / "nf"))
    for line in open(tmp_path / "utt2dur"):
        k, dur = line.split()
        rate, w = mfcc.read_wav(open(tmp_path / ("%s.wav" % k), "rb").read(), k)
        assert float(dur) == pytest.approx(w.shape[1] / rate, rel=1e-6)
        assert int(nf[k]) == int(opts.num_frames(w.shape[1])) == a[k].shape[0]
    assert not marker.exists()


def test_make_mfcc_leaves_vad(env, tmp_path):
    entries = _entries(env, tmp_path)
    data = tmp_path / "data_aug"
    data.mkdir()
    with open(data / "wav.scp", "w") as f:
        for k, rx in entries:
            f.write("%s %s\n" % (k, rx))
    vad = b"u0-reverb /somewhere/vad.ark:12\nu1-reverb /somewhere/vad.ark:99\n"
    with open(data / "vad.scp", "wb") as f:
        f.write(vad)
    conf = os.path.join(ROOT, "tests", "golden", "mfcc.conf")
    subprocess.run(["bash", os.path.join(TWIN, "make_mfcc_mi355x.sh"), str(data), conf, str(tmp_path / "mfcc")], check=True,
                   stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert open(data / "vad.scp", "rb").read() == vad
    feats = [l.split()[0] for l in open(data / "feats.scp")]
    assert feats == [k for k, _ in entries]
    assert [l.split()[0] for l in open(data / "utt2num_frames")] == feats


def test_cli_over_several_batches(env, tmp_path, monkeypatch):
    """compute-mfcc-feats with a window that splits the RIR entries into batches, the last one a single reverb entry: the same
    features, bit for bit, as in one batch."""
    import kaldi_io
    import mfcc_vad
    d = tmp_path / "src"
    d.mkdir()
    rir = _wav(env, d / "rir.wav", rir_like(2500, 17))
    lines = []
    for i, sec in enumerate((2.1, 2.4, 1.9, 2.2, 2.6)):
        x = _wav(env, d / ("u%d.wav" % i), speech(env, int(FS * sec), 80 + i))
        lines.append("u%d-reverb wav-reverberate --shift-output=true --impulse-response=%s %s - |\n" % (i, rir, x))
    scp = tmp_path / "wav.scp"
    scp.write_text("".join(lines))
    conf = os.path.join(ROOT, "tests", "golden", "mfcc.conf")
    opts = mfcc_vad.mfcc.MfccOptions().update(mfcc_vad.mfcc.read_config(conf))
    sizes = [len(ws) for _, ws in mfcc_vad._planned_batches(str(scp), opts, env["augment"].Augmenter(), 40000)]
    assert sizes == [2, 2, 1]
    assert mfcc_vad.main(["compute-mfcc-feats", "--config=" + conf, "scp:%s" % scp, "ark:%s" % (tmp_path / "one.ark")]) == 0
    monkeypatch.setattr(mfcc_vad, "WINDOW_SAMPLES", 40000)
    assert mfcc_vad.main(["compute-mfcc-feats", "--config=" + conf, "scp:%s" % scp, "ark:%s" % (tmp_path / "many.ark")]) == 0
    a = dict(kaldi_io.read_mat_ark(str(tmp_path / "one.ark")))
    b = dict(kaldi_io.read_mat_ark(str(tmp_path / "many.ark")))
    assert sorted(a) == sorted(b) == ["u%d-reverb" % i for i in range(5)]
    for k in a:
        assert a[k].shape[0] > 0 and np.array_equal(a[k], b[k]), k
