"""MFCC + energy VAD on the GPU (csrc/xv_mfcc.hip) against the fp64 oracle (tests/mfcc_ref.py) under the propagated fp32 bound
of DESIGN.md §8.6, the bitwise independence of a frame from its batch, exact VAD decisions, and the stage-1 CLI end to end.  The
oracle computes with the product's fp32 tables; tests/test_mfcc_cpu.py pins those against independent fp64 definitions."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import mfcc_ref

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -23
A = 64.0                      # the bound's constant, fixed before any measurement
WORST = {}                    # the worst observed error / bound ratio per quantity (printed at the end of the module)


@pytest.fixture(scope="module")
def env():
    import torch
    from xvector_amd import hiplib, mfcc, synthetic
    hiplib.require_gpu()
    yield dict(torch=torch, mfcc=mfcc, synthetic=synthetic, hiplib=hiplib)
    print("\nworst error / bound ratio: " + ", ".join("%s %.4f" % kv for kv in sorted(WORST.items())))


def recipe_opts(mfcc, **kw):
    here = os.path.dirname(os.path.abspath(__file__))
    o = mfcc.MfccOptions().update(mfcc.read_config(os.path.join(here, "golden", "mfcc.conf")))
    return o.update(kw.items())


def recipe_vad(mfcc):
    here = os.path.dirname(os.path.abspath(__file__))
    return mfcc.VadOptions().update(mfcc.read_config(os.path.join(here, "golden", "vad.conf")))


def signals(synthetic, fs, seed):
    """The signal set: speech-like audio, a pure tone, a full-scale clipped square wave, a large DC offset under a small signal,
    digital silence; lengths from 0 samples up."""
    rng = np.random.default_rng(seed)
    n = int(3.1 * fs)
    t = np.arange(n)
    out = [("speech", synthetic.speech_like_wave(n, fs, seed)),
           ("tone", np.rint(8000 * np.sin(2 * np.pi * 1000.0 / fs * t)).astype(np.int16)),
           ("square", np.where(np.sin(2 * np.pi * 330.0 / fs * t) >= 0, 32767, -32768).astype(np.int16)),
           ("dc", np.clip(20000 + np.rint(10 * rng.standard_normal(n)), -32768, 32767).astype(np.int16)),
           ("silence", np.zeros(n, np.int16))]
    sp = synthetic.speech_like_wave(fs, fs, seed + 1)
    for L in (0, 1, 40, 199, 200, 201, 399, 401, 1234):
        out.append(("len%d" % L, sp[:L]))
    return out


def check(env, opts, named, key_prefix="u", logmel=True):
    """Run the named waves in one launch and hold every frame to the bounds; returns the device results."""
    mfcc = env["mfcc"]
    keys = ["%s%03d-%s" % (key_prefix, i, n) for i, (n, _) in enumerate(named)]
    waves = [w for _, w in named]
    eng = mfcc.Mfcc(opts, with_logmel=logmel)
    feats, _, logmels = eng.compute(keys, waves)
    tb = eng.tables
    absd = np.abs(tb.lifter_dct.astype(np.float64))
    for k, w, f, lm in zip(keys, waves, feats, logmels):
        ref = mfcc_ref.mfcc(opts, tb, w, mfcc.dither_key(k, opts.seed))
        T = ref["feats"].shape[0]
        assert f.shape == (T, opts.num_ceps) and lm.shape == (T, opts.num_mel_bins), k
        if T == 0:
            continue
        assert np.isfinite(f).all() and np.isfinite(lm).all(), k
        e_ref = np.maximum(ref["power_sum"], opts.padded_length / 2 * ref["energy_raw"])[:, None]
        bound = A * EPS32 * (1 + np.sqrt(e_ref / np.maximum(ref["mel"], mfcc_ref.FLT_EPSILON)))
        err = np.abs(lm.astype(np.float64) - ref["logmel"])
        WORST["logmel"] = max(WORST.get("logmel", 0), float((err / bound).max()))
        assert (err <= bound).all(), (k, float((err / bound).max()))
        cb = bound @ absd.T + A * EPS32 * (np.abs(ref["logmel"]) @ absd.T)
        ferr = np.abs(f.astype(np.float64) - ref["feats"])
        j0 = 1 if opts.use_energy else 0
        WORST["cepstra"] = max(WORST.get("cepstra", 0), float((ferr[:, j0:] / cb[:, j0:]).max()))
        assert (ferr[:, j0:] <= cb[:, j0:]).all(), (k, float((ferr[:, j0:] / cb[:, j0:]).max()))
        if opts.use_energy:
            e_used = np.exp(ref["feats"][:, 0])
            b0 = A * EPS32 * (1 + np.sqrt(ref["energy_raw"] / np.maximum(e_used, mfcc_ref.FLT_EPSILON)))
            WORST["c0"] = max(WORST.get("c0", 0), float((ferr[:, 0] / b0).max()))
            assert (ferr[:, 0] <= b0).all(), (k, float((ferr[:, 0] / b0).max()))
    return keys, waves, feats, logmels


@pytest.mark.parametrize("dither", [0.0, 1.0])
@pytest.mark.parametrize("snip", [False, True])
def test_recipe_config_8k(env, dither, snip):
    opts = recipe_opts(env["mfcc"], dither=dither, snip_edges=snip, seed=7)
    check(env, opts, signals(env["synthetic"], 8000, 3))


@pytest.mark.parametrize("dither", [0.0, 1.0])
def test_kaldi_defaults_16k(env, dither):
    opts = env["mfcc"].MfccOptions(dither=dither)
    assert opts.padded_length == 512 and opts.num_ceps == 13
    check(env, opts, signals(env["synthetic"], 16000, 4))


@pytest.mark.parametrize("window", ["hamming", "hanning", "povey", "rectangular", "sine", "blackman"])
def test_every_window_and_raw_energy_false(env, window):
    named = signals(env["synthetic"], 8000, 5)[:4]
    check(env, recipe_opts(env["mfcc"], window_type=window), named)
    check(env, recipe_opts(env["mfcc"], window_type=window, raw_energy=False, energy_floor=1.0), named)


# The kernel's option space (xv_mfcc_f32 takes padded 128 .. 1024, up to 128 bins and cepstra): the smallest configurations that
# reach each branch the recipe and the 16 kHz defaults leave out.  (base, options, (frame length, shift, padded), what it reaches)
OPTION_CASES = {
    "pad128_full": ("kaldi", dict(sample_frequency=8000, frame_length=16, num_mel_bins=13, num_ceps=13, low_freq=20, high_freq=3700,
                                  snip_edges=False), (128, 80, 128)),           # H/2 = 32 butterflies, no zero padding, reflection
    "pad128_short": ("kaldi", dict(sample_frequency=8000, frame_length=10, frame_shift=10, num_mel_bins=10, num_ceps=7, low_freq=100),
                     (80, 80, 128)),                                            # a partial second lane trip; ceps < bins
    "pad1024": ("kaldi", dict(sample_frequency=32000, frame_length=25, num_mel_bins=80, num_ceps=80, high_freq=-400),
                (800, 320, 1024)),                                              # 16 v[] slots, two lane trips of mel and DCT
    "pad1024_full": ("kaldi", dict(sample_frequency=16000, frame_length=64, num_mel_bins=128, num_ceps=128, low_freq=0,
                                   snip_edges=False), (1024, 160, 1024)),       # the limits of all three constants at once
    "65x65": ("kaldi", dict(num_mel_bins=65, num_ceps=65), (400, 160, 512)),    # one lane in the second trip
    "flags_off": ("recipe", dict(remove_dc_offset=False, preemphasis_coefficient=0, use_energy=False, cepstral_lifter=0),
                  (200, 80, 256)),                                              # c0 is the DCT's row 0, held by the cepstra bound
    "floor": ("recipe", dict(energy_floor=1e6, raw_energy=True), (200, 80, 256)),
    "gaps_nosnip": ("kaldi", dict(sample_frequency=8000, frame_length=20, frame_shift=25, snip_edges=False), (160, 200, 256)),
    "gaps_snip": ("kaldi", dict(sample_frequency=8000, frame_length=20, frame_shift=25, snip_edges=True), (160, 200, 256)),
}
OPTION_RUNS = [(name, 0.0) for name in OPTION_CASES] + [("pad1024", 1.0), ("pad1024_full", 1.0)]


@pytest.mark.parametrize("name,dither", OPTION_RUNS, ids=["%s-dither%g" % r for r in OPTION_RUNS])
def test_option_space(env, name, dither):
    mfcc, syn = env["mfcc"], env["synthetic"]
    base, kw, geometry = OPTION_CASES[name]
    opts = (recipe_opts(mfcc) if base == "recipe" else mfcc.MfccOptions()).update(list(kw.items()) + [("dither", dither), ("seed", 5)])
    L = opts.frame_length_samples
    assert (L, opts.frame_shift_samples, opts.padded_length) == geometry
    fs = int(opts.sample_frequency)
    named = [(n, w[:int(0.6 * fs)]) for n, w in signals(syn, fs, 6)[:4]]
    sp = syn.speech_like_wave(2 * L, fs, 8)
    named += [("len%d" % n, sp[:n]) for n in (0, 1, L - 1, L, L + 1)]
    if name == "floor":
        named.append(("silence", np.zeros(int(0.6 * fs), np.int16)))
    _, _, feats, _ = check(env, opts, named)
    if name == "floor":
        c0 = feats[-1][:, 0]
        want = np.log(1e6)
        assert c0.shape[0] > 0 and (c0 == c0[0]).all() and abs(float(c0[0]) - want) <= float(np.spacing(np.float32(want)))
        assert feats[2][:, 0].min() > want + 1                   # the clipped square is far above the floor: both sides are met


def _direct(env, opts, x, ns, keys):
    """hiplib.mfcc on one sample buffer (int16 or float32): -> (feats [rows, C], logmel [rows, B], first rows, frame counts)."""
    torch, mfcc, hiplib = env["torch"], env["mfcc"], env["hiplib"]
    dev = mfcc.MfccTables(opts).to_device("cuda:0")
    ns = np.asarray(ns, np.int64)
    T = opts.num_frames(ns)
    row0 = np.concatenate([[0], np.cumsum(T)[:-1]]).astype(np.int64)
    rows = int(T.sum())
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    off = np.concatenate([[0], np.cumsum(ns)[:-1]]).astype(np.int64)
    keyv = np.array([mfcc.dither_key(k, opts.seed) for k in keys], np.uint64).view(np.int64)
    feats = torch.full((rows, opts.num_ceps), float("nan"), device="cuda")
    lm = torch.full((rows, opts.num_mel_bins), float("nan"), device="cuda")
    hiplib.mfcc(cuda(x), cuda(off), cuda(ns), cuda(row0), cuda(keyv), rows, dev, opts, feats, lm)
    return feats.cpu().numpy(), lm.cpu().numpy(), row0, T


def test_sample_formats(env):
    """The same integer samples as int16 and as fp32 give the same bits; fp32 non-integers stay within the bounds of the oracle
    fed the same fp32 values."""
    mfcc, syn = env["mfcc"], env["synthetic"]
    opts = recipe_opts(mfcc, dither=1.0, seed=13)
    waves = [syn.speech_like_wave(n, 8000, 40 + n) for n in (4000, 0, 199, 2501)]
    waves.append(np.where(np.arange(1000) % 24 < 12, 32767, -32768).astype(np.int16))
    x = np.concatenate(waves)
    ns, keys = [w.shape[0] for w in waves], ["fmt%d" % i for i in range(len(waves))]
    f16, l16, _, T = _direct(env, opts, x, ns, keys)
    f32, l32, _, _ = _direct(env, opts, x.astype(np.float32), ns, keys)
    assert f16.shape[0] == int(T.sum()) > 0 and np.isfinite(f16).all() and np.isfinite(l16).all()
    assert np.array_equal(f16.view(np.uint32), f32.view(np.uint32)) and np.array_equal(l16.view(np.uint32), l32.view(np.uint32))
    scaled = (waves[0].astype(np.float64) * 0.37).astype(np.float32)
    assert (scaled != np.rint(scaled)).any()
    check(env, opts, [("scaled", scaled), ("scaled-short", scaled[:201])])


def test_vad_through_a_strided_matrix(env):
    """xv_vad_energy_f32 on column 0 of a [rows, 23] matrix (row stride 23; compute_vad only ever feeds stride 1): three
    utterances at non-zero first rows, one of them empty; the other columns and the rows of no utterance are NaN."""
    torch, mfcc, hiplib = env["torch"], env["mfcc"], env["hiplib"]
    rng = np.random.default_rng(17)
    row0 = np.array([5, 102, 110], np.int64)
    T = np.array([97, 0, 300], np.int32)
    rows, canary = 410, 29
    m = np.full((rows + canary, 23), np.nan, np.float32)
    c0s = [(rng.standard_normal(int(t)) * 4 + 12).astype(np.float32) for t in T]
    for r, c in zip(row0, c0s):
        m[r:r + len(c), 0] = c
    d_m = torch.from_numpy(m).cuda()
    assert d_m.stride(0) == 23
    for v in (recipe_vad(mfcc), mfcc.VadOptions(vad_frames_context=5, vad_proportion_threshold=0.5)):
        out = torch.full((rows + canary,), float("nan"), device="cuda")
        hiplib.vad_energy(d_m, torch.from_numpy(row0).cuda(), torch.from_numpy(T).cuda(), v, out)
        got = out.cpu().numpy()
        written = np.zeros(rows + canary, bool)
        for r, c in zip(row0, c0s):
            assert np.array_equal(got[r:r + len(c)], mfcc_ref.vad(c, v))
            written[r:r + len(c)] = True
        assert np.isnan(got[~written]).all() and written.sum() == 397


BAD_ARG, UNSUPPORTED = -1, -2             # XV_ERR_BAD_ARG, XV_ERR_UNSUPPORTED of include/xvector_hip.h
POISON = 0x7FC0BEEF


def test_refused_mfcc_arguments_leave_the_output_alone(env):
    torch, mfcc, hiplib = env["torch"], env["mfcc"], env["hiplib"]
    lib = hiplib.load()
    opts = recipe_opts(mfcc, dither=0.0)
    tb = mfcc.MfccTables(opts).to_device("cuda:0")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    n = 2000
    rows = int(opts.num_frames(n))
    x = dev(env["synthetic"].speech_like_wave(n, 8000, 2))
    one = lambda v: dev(np.array([v], np.int64))  # noqa: E731
    # buffers wide enough for every refused shape, should a check be missing
    feats = dev(np.full((rows + 8, 256), POISON, np.uint32).view(np.float32))
    lm = dev(np.full((rows + 8, 256), POISON, np.uint32).view(np.float32))
    good = dict(samples=x, sample_format=0, utt_offset=one(0), utt_samples=one(n), utt_row0=one(0), utt_key=one(1), n_utts=1,
                total_rows=rows, window=tb["window"], mel_first=tb["mel_first"], mel_len=tb["mel_len"], mel_w=tb["mel_w"],
                num_bins=23, mel_ld=int(tb["mel_w"].shape[1]), lifter_dct=tb["lifter_dct"], num_ceps=23, twiddle=tb["twiddle"],
                frame_length=200, frame_shift=80, padded_length=256, snip_edges=0, dither=0.0, preemph_coeff=0.97, remove_dc=1,
                use_energy=1, raw_energy=1, energy_floor=0.0, feats=feats, ld_feats=256, logmel=lm, ld_logmel=256, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return lib.xv_mfcc_f32(*[ctypes.c_void_p(v.data_ptr()) if isinstance(v, torch.Tensor) else v for v in a.values()])

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t.cpu().numpy().view(np.uint32) == POISON).all()) for t in (feats, lm))

    refused = [(dict(padded_length=64, frame_length=50), UNSUPPORTED), (dict(padded_length=2048), UNSUPPORTED),
               (dict(padded_length=384), UNSUPPORTED), (dict(num_bins=129), UNSUPPORTED),
               (dict(num_ceps=24), BAD_ARG), (dict(frame_length=257), BAD_ARG), (dict(frame_length=0), BAD_ARG),
               (dict(frame_shift=0), BAD_ARG), (dict(ld_feats=22), BAD_ARG), (dict(ld_logmel=22), BAD_ARG),
               (dict(dither=-1.0), BAD_ARG), (dict(sample_format=2), BAD_ARG), (dict(n_utts=-1), BAD_ARG),
               (dict(total_rows=-1), BAD_ARG)]
    pointers = ("samples", "utt_offset", "utt_samples", "utt_row0", "utt_key", "window", "mel_first", "mel_len", "mel_w",
                "lifter_dct", "twiddle", "feats")
    refused += [({p: None}, BAD_ARG) for p in pointers]
    for kw, code in refused:
        assert call(**kw) == code, (kw, lib.xv_last_error())
        assert b"mfcc" in lib.xv_last_error(), kw
    assert untouched()
    # no rows: nothing to do, whatever the pointers
    assert call(total_rows=0, **{p: None for p in pointers}) == 0 and call(total_rows=0, n_utts=0) == 0
    assert untouched()
    # a narrow log-mel stride is fine without a log-mel buffer; and the call with nothing wrong writes exactly its rows
    assert call(logmel=None, ld_logmel=0) == 0 and call() == 0
    torch.cuda.synchronize()
    f, l = feats.cpu().numpy(), lm.cpu().numpy()
    assert np.isfinite(f[:rows, :23]).all() and np.isfinite(l[:rows, :23]).all()
    for a in (f, l):
        assert (a[rows:].view(np.uint32) == POISON).all() and (a[:, 23:].view(np.uint32) == POISON).all()


def test_refused_vad_arguments_leave_the_output_alone(env):
    torch, hiplib = env["torch"], env["hiplib"]
    lib = hiplib.load()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    c0 = np.linspace(0, 20, 60).astype(np.float32)
    good = dict(feats=dev(c0), ld=1, utt_row0=dev(np.array([0, 40], np.int64)), n_frames=dev(np.array([40, 20], np.int32)), n_utts=2,
                energy_threshold=5.0, energy_mean_scale=0.5, frames_context=2, proportion_threshold=0.6,
                out=dev(np.full(64, POISON, np.uint32).view(np.float32)), stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return lib.xv_vad_energy_f32(*[ctypes.c_void_p(v.data_ptr()) if isinstance(v, torch.Tensor) else v for v in a.values()])

    def poison_left():
        torch.cuda.synchronize()
        return int((good["out"].cpu().numpy().view(np.uint32) == POISON).sum())

    for kw in (dict(frames_context=-1), dict(ld=0), dict(n_utts=-1), dict(feats=None), dict(utt_row0=None), dict(n_frames=None),
               dict(out=None)):
        assert call(**kw) == BAD_ARG, (kw, lib.xv_last_error())
        assert b"vad_energy" in lib.xv_last_error(), kw
    assert call(n_utts=0) == 0 and call(n_utts=0, feats=None, out=None) == 0
    assert poison_left() == 64
    assert call() == 0
    assert poison_left() == 4
    vopts = env["mfcc"].VadOptions(vad_frames_context=2)
    got = good["out"].cpu().numpy()
    assert np.array_equal(got[:40], mfcc_ref.vad(c0[:40], vopts)) and np.array_equal(got[40:60], mfcc_ref.vad(c0[40:], vopts))


def test_silence_without_dither_is_the_floor(env):
    opts = recipe_opts(env["mfcc"], dither=0.0)
    eng = env["mfcc"].Mfcc(opts, with_logmel=True)
    f, _, lm = eng.compute(["z"], [np.zeros(8000, np.int16)])
    floor = np.log(mfcc_ref.FLT_EPSILON)                      # the device's logf: within one fp32 ulp of it, the same everywhere
    assert (lm[0] == lm[0][0, 0]).all() and (f[0][:, 0] == lm[0][0, 0]).all()
    assert abs(float(lm[0][0, 0]) - floor) <= abs(np.spacing(np.float32(floor)))


def test_ten_minutes_in_one_launch(env):
    """One 10-minute utterance (4.8 M samples, 60 k frames) beside short ones, dithered."""
    syn = env["synthetic"]
    named = [("long", syn.speech_like_wave(4800000, 8000, 9)), ("short", syn.speech_like_wave(3000, 8000, 10)), ("empty", np.zeros(0, np.int16))]
    keys, _, feats, _ = check(env, recipe_opts(env["mfcc"], seed=3), named)
    assert feats[0].shape == (60000, 23)


def test_nan_poisoned_outputs_and_canaries(env):
    torch, mfcc, hiplib = env["torch"], env["mfcc"], env["hiplib"]
    opts = recipe_opts(mfcc)
    tb = mfcc.MfccTables(opts)
    dev = tb.to_device("cuda:0")
    waves = [env["synthetic"].speech_like_wave(n, 8000, n) for n in (0, 1000, 40, 7777, 0)]
    ns = np.array([w.shape[0] for w in waves], np.int64)
    T = opts.num_frames(ns)
    row0 = np.concatenate([[0], np.cumsum(T)[:-1]]).astype(np.int64)
    rows = int(T.sum())
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    x = cuda(np.concatenate(waves))
    off = cuda(np.concatenate([[0], np.cumsum(ns)[:-1]]).astype(np.int64))
    keys = cuda(np.array([mfcc.dither_key("k%d" % i) for i in range(5)], np.uint64).view(np.int64))
    canary = 37
    feats = torch.full((rows + canary, 40), float("nan"), device="cuda")
    lm = torch.full((rows + canary, 30), float("nan"), device="cuda")
    hiplib.mfcc(x, off, cuda(ns), cuda(row0), keys, rows, dev, opts, feats[:, :23], lm[:, :23])
    f, l = feats.cpu().numpy(), lm.cpu().numpy()
    assert np.isfinite(f[:rows, :23]).all() and np.isfinite(l[:rows, :23]).all()
    assert np.isnan(f[:, 23:]).all() and np.isnan(l[:, 23:]).all() and np.isnan(f[rows:]).all() and np.isnan(l[rows:]).all()


@pytest.mark.parametrize("dither", [0.0, 1.0])
def test_bitwise_independence_of_the_batch(env, dither):
    """A frame's output is identical alone, in another batch, in another order, and split across launch windows."""
    mfcc, syn = env["mfcc"], env["synthetic"]
    opts = recipe_opts(mfcc, dither=dither, seed=11)
    rng = np.random.default_rng(5)
    keys = ["spk%d-utt%d" % (i % 3, i) for i in range(12)]
    waves = [syn.speech_like_wave(int(rng.integers(0, 30000)), 8000, i) for i in range(12)]
    base, _, _ = mfcc.Mfcc(opts).compute(keys, waves)
    eng = mfcc.Mfcc(opts)
    for i in (0, 5, 11):
        alone, _, _ = eng.compute([keys[i]], [waves[i]])
        assert np.array_equal(alone[0], base[i])
    rev, _, _ = eng.compute(keys[::-1], waves[::-1])
    assert all(np.array_equal(a, b) for a, b in zip(rev[::-1], base))
    other, _, _ = eng.compute(keys[3:7] + ["x-extra"], waves[3:7] + [syn.speech_like_wave(5000, 8000, 99)])
    assert all(np.array_equal(a, b) for a, b in zip(other[:4], base[3:7]))
    split, _, _ = mfcc.Mfcc(opts, window_samples=20000).compute(keys, waves)
    assert all(np.array_equal(a, b) for a, b in zip(split, base))
    if dither:
        other_key, _, _ = eng.compute(["another-id"], [waves[1]])
        assert waves[1].shape[0] < 200 or not np.array_equal(other_key[0], base[1])


def _vad_device(env, c0s, vopts):
    return list(env["mfcc"].compute_vad([np.asarray(c, np.float32)[:, None] for c in c0s], vopts))


def test_vad_on_oracle_c0_is_exact(env):
    mfcc = env["mfcc"]
    vopts = recipe_vad(mfcc)
    rng = np.random.default_rng(3)
    c0s = [(rng.standard_normal(T) * 4 + 12).astype(np.float32) for T in (1, 2, 3, 4, 5, 6, 97, 1000, 20000)]
    c0s.append(np.full(50, 11.0, np.float32))           # every frame exactly at thr = 5.5 + 0.5 * 11 = 11: none voiced (strict >)
    c0s.append(np.full(3, 11.0, np.float32))
    for ctx, prop in ((2, 0.12), (0, 0.6), (5, 0.5), (1, 1.0)):
        v = mfcc.VadOptions(vad_energy_threshold=5.5, vad_energy_mean_scale=0.5, vad_frames_context=ctx, vad_proportion_threshold=prop)
        got = _vad_device(env, c0s, v)
        for c, g in zip(c0s, got):
            assert np.array_equal(g, mfcc_ref.vad(c, v)), (len(c), ctx, prop)
    got = _vad_device(env, c0s[-2:], vopts)
    assert not got[0].any() and not got[1].any()
    assert mfcc_ref.threshold(c0s[-2], vopts) == 11.0


def _wav_dir(env, tmp_path, n=14):
    mfcc, syn = env["mfcc"], env["synthetic"]
    rng = np.random.default_rng(21)
    lines, waves = [], {}
    for i in range(n):
        key = "spk%d-utt%02d" % (i % 4, i)
        w = syn.speech_like_wave(int(rng.integers(8000, 8000 * 9)), 8000, 100 + i)
        path = str(tmp_path / (key + ".wav"))
        with open(path, "wb") as f:
            f.write(mfcc.wav_bytes(w, 8000, extensible=(i % 3 == 0), streaming=(i % 4 == 1)))
        waves[key] = w
        lines.append("%s %s" % (key, path) if i % 2 else "%s cat %s |" % (key, path))
    scp = tmp_path / "wav.scp"
    scp.write_text("\n".join(lines) + "\n")
    return str(scp), waves


def _run(args, **kw):
    here = os.path.dirname(os.path.abspath(__file__))
    cli = os.path.join(here, "..", "x-vector-kaldi-tf_amd", "local", "tf", "mfcc_vad.py")
    return subprocess.run([sys.executable, cli] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600, **kw)


def test_cli_end_to_end_to_xvectors(env, tmp_path):
    import kaldi_io
    import models
    import extract_embedding as ee
    mfcc, syn = env["mfcc"], env["synthetic"]
    here = os.path.dirname(os.path.abspath(__file__))
    conf, vconf = os.path.join(here, "golden", "mfcc.conf"), os.path.join(here, "golden", "vad.conf")
    wav_scp, waves = _wav_dir(env, tmp_path)
    d = tmp_path
    p = _run(["compute-mfcc-vad", "--config=" + conf, "--vad-config=" + vconf, "--write-num-frames=ark,t:%s/nf" % d,
              "scp:" + wav_scp, "ark,scp:%s/f.ark,%s/f.scp" % (d, d), "ark,scp:%s/v.ark,%s/v.scp" % (d, d)])
    assert p.returncode == 0, p.stdout.decode()
    feats = dict(kaldi_io.read_mat_scp(str(d / "f.scp")))
    vads = dict(kaldi_io.read_vec_flt_scp(str(d / "v.scp")))
    nf = dict(l.split() for l in open(str(d / "nf")))
    assert list(feats) == list(waves) == list(vads) == list(nf)
    opts, vopts = recipe_opts(mfcc), recipe_vad(mfcc)
    tb = mfcc.MfccTables(opts)
    near = total = 0
    for k, w in waves.items():
        ref = mfcc_ref.mfcc(opts, tb, w, mfcc.dither_key(k, opts.seed))
        f = feats[k]
        assert f.shape == ref["feats"].shape and int(nf[k]) == f.shape[0]
        assert np.abs(f[:, 0] - ref["feats"][:, 0]).max() < 1e-3
        rv = mfcc_ref.vad(ref["feats"][:, 0], vopts)
        thr = mfcc_ref.threshold(ref["feats"][:, 0], vopts)
        close = np.abs(ref["feats"][:, 0] - thr) < 1e-4
        ctx = vopts.vad_frames_context
        in_ctx = np.convolve(close.astype(int), np.ones(2 * ctx + 1, int), mode="same") > 0
        assert np.array_equal(vads[k][~in_ctx], rv[~in_ctx]), k
        near += int(in_ctx.sum())
        total += f.shape[0]
    assert near < 0.01 * total
    # two passes give byte-identical tables
    p = _run(["compute-mfcc-feats", "--config=" + conf, "scp:" + wav_scp, "ark,scp:%s/f2.ark,%s/f2.scp" % (d, d)])
    assert p.returncode == 0, p.stdout.decode()
    p = _run(["compute-vad", "--config=" + vconf, "scp:%s/f2.scp" % d, "ark,scp:%s/v2.ark,%s/v2.scp" % (d, d)])
    assert p.returncode == 0, p.stdout.decode()
    assert open(str(d / "f.ark"), "rb").read() == open(str(d / "f2.ark"), "rb").read()
    assert open(str(d / "v.ark"), "rb").read() == open(str(d / "v2.ark"), "rb").read()
    # into the extractor
    topo = syn.SMALL_TOPOLOGY
    w = syn.trained_like(topo, 23, num_classes=8, seed=12)
    mdir = str(tmp_path / "nnet")
    models.Model.save_model(dict(weights=w, topology=topo, model_class="Model", num_classes=8, feat_dim=23), mdir, None)
    xa, xs = str(d / "x.ark"), str(d / "x.scp")
    ee.main(["--min-chunk-size", "25", "--chunk-size", "300", "--feature-rspecifier", "scp:%s/f.scp" % d,
             "--vector-wspecifier", "ark,scp:%s,%s" % (xa, xs), "--model-dir", mdir, "--cmn-window", "300",
             "--vad-rspecifier", "scp:%s/v.scp" % d])
    vecs = dict(kaldi_io.read_vec_flt_scp(xs))
    assert set(vecs) == {k for k, v in vads.items() if v.sum() >= 25}
    assert all(v.shape == (topo["embedding_sizes"][0],) and np.isfinite(v).all() for v in vecs.values())


def test_data_dir_script(env, tmp_path):
    """make_mfcc_vad_mi355x.sh turns a wav.scp-only data dir into feats.scp / vad.scp / utt2num_frames; a segments file is refused."""
    here = os.path.dirname(os.path.abspath(__file__))
    script = os.path.join(here, "..", "x-vector-kaldi-tf_amd", "local", "tf", "make_mfcc_vad_mi355x.sh")
    conf, vconf = os.path.join(here, "golden", "mfcc.conf"), os.path.join(here, "golden", "vad.conf")
    data = tmp_path / "data"
    data.mkdir()
    wav_scp, waves = _wav_dir(env, data, n=5)
    env_vars = dict(os.environ, PATH=os.path.dirname(sys.executable) + os.pathsep + os.environ.get("PATH", ""))
    p = subprocess.run(["bash", script, str(data), conf, vconf, str(tmp_path / "mfcc")], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=600, env=env_vars)
    assert p.returncode == 0, p.stdout.decode()
    import kaldi_io
    assert [k for k, _ in kaldi_io.read_mat_scp(str(data / "feats.scp"))] == list(waves)
    assert [k for k, _ in kaldi_io.read_vec_flt_scp(str(data / "vad.scp"))] == list(waves)
    assert len(open(str(data / "utt2num_frames")).read().split("\n")) == 6
    (data / "segments").write_text("x y 0 1\n")
    p = subprocess.run(["bash", script, str(data), conf, vconf, str(tmp_path / "mfcc")], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=60, env=env_vars)
    assert p.returncode != 0 and b"segments" in p.stdout
