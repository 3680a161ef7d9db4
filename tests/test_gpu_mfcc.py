"""MFCC + energy VAD on the GPU (csrc/xv_mfcc.hip) against the fp64 oracle (tests/mfcc_ref.py) under the propagated fp32 bound
of DESIGN.md §8.6, the bitwise independence of a frame from its batch, exact VAD decisions, and the stage-1 CLI end to end."""
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
