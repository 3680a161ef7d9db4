"""The resampler on the GPU (csrc/xv_resample.hip): every rate pair and edge length in one launch against the
exact fmaf chain and the fp64 sum of tests/resample_ref.py, impulses that show any indexing error as an inequality, the bitwise
independence of an utterance from its batch, the refused arguments, and the feature engine and stage-1 CLI with
--allow-downsample / --allow-upsample."""
import ctypes
import logging
import os

import numpy as np
import pytest

import resample_ref as ref

pytestmark = pytest.mark.gpu

WORST = {}                    # the worst observed error / bound ratio per signal (printed at the end of the module)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def env():
    import torch
    from xvector_amd import hiplib, mfcc, resample, synthetic
    hiplib.require_gpu()
    yield dict(torch=torch, mfcc=mfcc, synthetic=synthetic, hiplib=hiplib, resample=resample)
    print("\nworst |y_gpu - y_fp64| / ((T + 1) 2^-24 sum |w x|): " + ", ".join("%s %.4f" % kv for kv in sorted(WORST.items())))


@pytest.fixture(scope="module")
def batch(env):
    """Every pair x every edge length of full-scale random int16, plus one speech-like wave per pair: one launch as int16, one as
    fp32, and the references, computed once."""
    rs, synthetic = env["resample"], env["synthetic"]
    rng = np.random.default_rng(11)
    waves, rates, kinds = [], [], []
    for fi, fo in ref.PAIRS:
        for n in ref.lengths(fi, fo, rs.OUT_TILE):
            waves.append(rng.integers(-32768, 32768, n).astype(np.int16))
            rates.append((fi, fo))
            kinds.append("random")
        waves.append(synthetic.speech_like_wave(ref.length_for_outputs(rs.OUT_TILE + 300, fi, fo), fi, seed=fi % 97))
        rates.append((fi, fo))
        kinds.append("speech")
    return dict(waves=waves, rates=rates, kinds=kinds)


def run_mixed(env, waves, rates, dtype=np.int16):
    """Waves of any (fi, fo) pairs in ONE launch: -> float32 arrays.  (resample_waves takes one output rate; the kernel does not
    care, so the layout is built here from the same pieces.)"""
    rs, torch, hiplib = env["resample"], env["torch"], env["hiplib"]
    pairs = []
    for r in rates:
        if r not in pairs:
            pairs.append(r)
    n_in = np.array([len(w) for w in waves], np.int64)
    n_out = np.array([ref.num_output(len(w), *r) for w, r in zip(waves, rates)], np.int64)
    utt = np.zeros((5, len(waves)), np.int64)
    utt[1], utt[3], utt[4] = n_in, n_out, [pairs.index(r) for r in rates]
    utt[0, 1:], utt[2, 1:] = np.cumsum(n_in[:-1]), np.cumsum(n_out[:-1])
    tab, first, ntaps, w = rs.pool(pairs)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")  # noqa: E731
    flat = np.concatenate([np.asarray(x).astype(dtype) for x in waves] + [np.zeros(1, dtype)])
    out = torch.full((int(n_out.sum()) + 64,), float("nan"), dtype=torch.float32, device="cuda:0")
    hiplib.resample(dev(flat), utt, tab, dev(first), dev(ntaps), dev(w), dev(rs.tile_list(n_out)), out)
    y = out.cpu().numpy()
    assert np.isnan(y[int(n_out.sum()):]).all()                   # nothing past the last utterance is written
    return [y[o:o + m] for o, m in zip(utt[2].tolist(), n_out.tolist())]


@pytest.fixture(scope="module")
def results(env, batch):
    y16 = run_mixed(env, batch["waves"], batch["rates"], np.int16)
    y32 = run_mixed(env, batch["waves"], batch["rates"], np.float32)
    chain = [ref.resample_chain(w, *r) for w, r in zip(batch["waves"], batch["rates"])]
    f64 = [ref.resample64(w, *r) for w, r in zip(batch["waves"], batch["rates"])]
    return dict(y16=y16, y32=y32, chain=chain, f64=f64)


def test_shapes_and_counts(env, batch, results):
    rs = env["resample"]
    assert len({r for r in batch["rates"]}) == 5
    for w, (fi, fo), y, z in zip(batch["waves"], batch["rates"], results["y16"], results["y32"]):
        m = ref.num_output(len(w), fi, fo)
        assert y.shape == z.shape == (m,) and y.dtype == np.float32
        assert m == int(rs.num_output_samples(len(w), fi, fo)) == env["hiplib"].resample_num_output(len(w), fi, fo)
        assert np.isfinite(y).all()
    assert env["hiplib"].resample_num_output(5, 8000, 8000) == -1 and env["hiplib"].resample_num_output(5, 0, 8000) == -1


def test_every_output_is_the_fmaf_chain(batch, results):
    """Bit for bit, int16 and fp32 input alike."""
    for i, (c, y, z) in enumerate(zip(results["chain"], results["y16"], results["y32"])):
        assert np.array_equal(bits(y), bits(c)), (i, batch["rates"][i], len(batch["waves"][i]))
        assert np.array_equal(bits(z), bits(c)), (i, batch["rates"][i], len(batch["waves"][i]))


def test_elementwise_bound_against_fp64(batch, results):
    """|y_gpu - y_fp64| <= (T + 1) 2^-24 sum_j |w_j x_j|, T the taps the output used: the bound of a length-T recursive fp32 sum
    (T roundings of the accumulator; the fused products add none) plus one unit of slack, derived, not measured."""
    for kind, rate, y, (y64, mag, T) in zip(batch["kinds"], batch["rates"], results["y16"], results["f64"]):
        if not len(y):
            continue
        bound = (T + 1) * 2.0 ** -24 * mag
        err = np.abs(y.astype(np.float64) - y64)
        nz = bound > 0
        assert np.all(err[~nz] == 0)
        if nz.any():
            WORST[kind] = max(WORST.get(kind, 0.0), float((err[nz] / bound[nz]).max()))
        assert np.all(err <= bound), (kind, rate, float((err[nz] / bound[nz]).max()))


@pytest.mark.parametrize("fi,fo", ref.PAIRS)
def test_impulses_exact(env, fi, fo):
    """x = 16384 delta[k]: every output is w[p][k - k0] * 16384 exactly (a power-of-two scale, the other taps add zeros or are
    skipped), or 0.0 where no tap meets k.  k: both ends of the wave and one index either side of the first input sample of the
    second tile."""
    rs = env["resample"]
    Ui, Uo, first, ntaps, w = rs.tables(fi, fo)
    n = ref.length_for_outputs(5 * rs.OUT_TILE // 2, fi, fo)
    b = int(first[rs.OUT_TILE % Uo]) + (rs.OUT_TILE // Uo) * Ui
    ks = [0, n - 1, b - 1, b, b + 1]
    assert 0 < b - 1 and b + 1 < n - 1
    waves = []
    for k in ks:
        x = np.zeros(n, np.int16)
        x[k] = 16384
        waves.append(x)
    ys = run_mixed(env, waves, [(fi, fo)] * len(ks))
    o = np.arange(ref.num_output(n, fi, fo))
    p = o % Uo
    k0 = first[p].astype(np.int64) + (o // Uo) * Ui
    for k, y in zip(ks, ys):
        j = k - k0
        hit = (j >= 0) & (j < ntaps[p])
        want = np.where(hit, w[p, np.clip(j, 0, w.shape[1] - 1)] * np.float32(16384), np.float32(0)).astype(np.float32) + np.float32(0)
        assert hit.any()
        assert np.array_equal(bits(y), bits(want)), (k, np.flatnonzero(bits(y) != bits(want))[:8])


def test_independent_of_the_batch(env, batch, results):
    """An utterance's bits alone, first and last in a batch, and beside utterances of other rate pairs."""
    waves, rates = batch["waves"], batch["rates"]
    pick = [i for i, (w, r) in enumerate(zip(waves, rates)) if batch["kinds"][i] == "speech" and r in ((16000, 8000), (44100, 8000))]
    assert len(pick) == 2
    for i in pick:
        alone = run_mixed(env, [waves[i]], [rates[i]])[0]
        others = [j for j in range(len(waves)) if rates[j] != rates[i] and 0 < len(waves[j]) < 3000][:4]
        front = run_mixed(env, [waves[i]] + [waves[j] for j in others], [rates[i]] + [rates[j] for j in others])[0]
        back = run_mixed(env, [waves[j] for j in others] + [waves[i]], [rates[j] for j in others] + [rates[i]])[-1]
        for y in (alone, front, back):
            assert np.array_equal(bits(y), bits(results["y16"][i]))


def test_zero_input_gives_exact_zeros(env):
    rs = env["resample"]
    waves = [np.zeros(ref.length_for_outputs(rs.OUT_TILE + 5, fi, fo), np.int16) for fi, fo in ref.PAIRS]
    for y in run_mixed(env, waves, list(ref.PAIRS)):
        assert len(y) and not bits(y).any()
    got = rs.resample_waves(waves[:1] + waves[2:4], [16000, 44100, 48000], 8000)
    assert [len(g) for g in got] == [ref.num_output(len(w), r, 8000) for w, r in zip(waves[:1] + waves[2:4], (16000, 44100, 48000))]
    assert all(not bits(g).any() for g in got)


def test_resample_waves_is_the_same_launch(env, batch, results):
    """The public entry point on the waves that share the output rate 8000 (it takes one output rate per call)."""
    idx = [i for i, r in enumerate(batch["rates"]) if r[1] == 8000 and batch["kinds"][i] == "speech"]
    got = env["resample"].resample_waves([batch["waves"][i] for i in idx], [batch["rates"][i][0] for i in idx], 8000)
    for i, g in zip(idx, got):
        assert np.array_equal(bits(g), bits(results["y16"][i]))
    with pytest.raises(ValueError):
        env["resample"].resample_waves([np.zeros(4, np.int16)], [8000], 8000)


def test_refused_arguments_leave_the_output_alone(env):
    rs, torch, hiplib = env["resample"], env["torch"], env["hiplib"]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")  # noqa: E731
    x = dev(np.full(4096, 1000, np.int16))
    poison = 0x7FC0BEEF
    out = dev(np.full(4096, poison, np.uint32).view(np.float32))
    tab, first, ntaps, w = rs.pool([(16000, 8000)])
    d_first, d_ntaps, d_tiles = dev(first), dev(ntaps), dev(np.zeros((1, 2), np.int64))

    def call(utt, tab, w=w, first=d_first, ntaps=d_ntaps):
        hiplib.resample(x, np.array(utt, np.int64).reshape(5, 1), tab, first, ntaps, dev(w), d_tiles, out)

    def untouched():
        torch.cuda.synchronize()
        return bool((out.cpu().numpy().view(np.uint32) == poison).all())

    # one output more than 2001 samples give
    with pytest.raises(hiplib.XvectorHipError, match=r"\(-1\)"):
        call([0, 2001, 0, 1002, 0], tab)
    assert untouched()
    # a tap row of 1025, 4097 phases, nine tables
    long_row = tab.copy()
    long_row[0, 2] = 1025
    with pytest.raises(hiplib.XvectorHipError, match=r"\(-2\)"):
        call([0, 2001, 0, 1001, 0], long_row, w=np.zeros(1025, np.float32))
    assert untouched()
    many = tab.copy()
    many[0, 1], many[0, 2] = 4097, 1
    z = dev(np.zeros(4097, np.int32))
    with pytest.raises(hiplib.XvectorHipError, match=r"\(-2\)"):
        call([0, 0, 0, 0, 0], many, w=np.zeros(4097, np.float32), first=z, ntaps=z)
    assert untouched()
    with pytest.raises(hiplib.XvectorHipError, match=r"\(-2\)"):
        call([0, 2001, 0, 1001, 0], np.repeat(tab, 9, axis=0))
    assert untouched()
    # a descriptor without phases, and the raw entry point: a null pointer, a negative count, an unknown sample format
    bad = tab.copy()
    bad[0, 1] = 0
    with pytest.raises(hiplib.XvectorHipError, match=r"\(-1\)"):
        call([0, 2001, 0, 1001, 0], bad)
    lib = hiplib.load()
    d_utt = dev(np.array([[0], [2001], [0], [1001], [0]], np.int64))
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    d_w = dev(w)

    def raw(inp=ptr(x), fmt=0, n_utts=1, n_tiles=1, outp=ptr(out)):
        return lib.xv_resample_f32(inp, fmt, ptr(d_utt[0]), ptr(d_utt[1]), ptr(d_utt[2]), ptr(d_utt[3]), ptr(d_utt[4]), n_utts,
                                   tab.ctypes.data_as(ctypes.c_void_p), 1, ptr(d_first), ptr(d_ntaps), ptr(d_w), ptr(d_tiles), n_tiles,
                                   outp, None)

    assert raw(inp=None) == -1 and raw(outp=None) == -1 and raw(fmt=2) == -1 and raw(n_utts=-1) == -1 and raw(n_tiles=-1) == -1
    assert untouched()
    # and the same call with nothing wrong writes exactly its 1001 outputs
    assert raw() == 0
    torch.cuda.synchronize()
    y = out.cpu().numpy()
    assert (y[1001:].view(np.uint32) == poison).all() and np.isfinite(y[:1001]).all()
    assert np.array_equal(bits(y[:1001]), bits(ref.resample_chain(np.full(2001, 1000, np.int16), 16000, 8000)))


def recipe_opts(mfcc, **kw):
    here = os.path.dirname(os.path.abspath(__file__))
    o = mfcc.MfccOptions().update(mfcc.read_config(os.path.join(here, "golden", "mfcc.conf")))
    return o.update(kw.items())


def test_engine_window_with_resampled_utterances(env):
    """One window of a 16 kHz, a 44.1 kHz and two 8 kHz utterances: the native ones do not notice the others, and a resampled
    one gets the features of its resampled wave."""
    mfcc, rs, synthetic = env["mfcc"], env["resample"], env["synthetic"]
    opts = recipe_opts(mfcc, allow_downsample=True, seed=5)
    assert opts.sample_frequency == 8000
    keys = ["nat-a", "wide-16k", "nat-b", "cd-44k"]
    waves = [synthetic.speech_like_wave(9000, 8000, 1), synthetic.speech_like_wave(17001, 16000, 2),
             synthetic.speech_like_wave(4321, 8000, 3), synthetic.speech_like_wave(30011, 44100, 4)]
    rates = [8000, 16000, None, 44100]
    eng = mfcc.Mfcc(opts, mfcc.VadOptions())
    feats, vads, _ = eng.compute(keys, waves, rates=rates)
    assert eng.stats["launches"] == 1 and eng.stats["resampled"] == 2
    nat, nat_vads, _ = eng.compute([keys[0], keys[2]], [waves[0], waves[2]])
    assert np.array_equal(bits(feats[0]), bits(nat[0])) and np.array_equal(bits(feats[2]), bits(nat[1]))
    assert np.array_equal(vads[0], nat_vads[0]) and np.array_equal(vads[2], nat_vads[1])
    res = rs.resample_waves([waves[1], waves[3]], [16000, 44100], 8000)
    assert [len(r) for r in res] == [ref.num_output(17001, 16000, 8000), ref.num_output(30011, 44100, 8000)]
    again, again_vads, _ = eng.compute([keys[1], keys[3]], res)
    for i, j in ((1, 0), (3, 1)):
        assert feats[i].shape == (int(opts.num_frames(len(res[j]))), opts.num_ceps) and feats[i].shape[0] > 50
        assert np.array_equal(bits(feats[i]), bits(again[j])) and np.array_equal(vads[i], again_vads[j])
    # the rate a Wave carries is read like an explicit one, and the options gate the direction
    w16 = mfcc.select_channel(keys[1], 16000, waves[1][None], opts)
    one, _, _ = eng.compute([keys[1]], [w16])
    assert np.array_equal(bits(one[0]), bits(feats[1]))
    with pytest.raises(ValueError, match="--allow-upsample"):
        eng.compute(["k"], [waves[2]], rates=[4000])
    # windows are cut by the samples on the device, outputs and inputs: three small windows give the same bits
    small = mfcc.Mfcc(opts, mfcc.VadOptions(), window_samples=30000)
    f2, v2, _ = small.compute(keys, waves, rates=rates)
    assert small.stats["launches"] == 3
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(f2, feats))


def _table(path):
    with open(path) as f:
        return dict(line.split(None, 1) for line in f if line.strip())


def test_cli_allow_downsample(env, tmp_path, caplog):
    """compute-mfcc-vad on one 16 kHz and one 8 kHz file.  (The warnings are the records of the 'mfcc' logger, whose handler the
    CLI points at stderr.)"""
    import mfcc_vad
    mfcc, synthetic = env["mfcc"], env["synthetic"]
    here = os.path.dirname(os.path.abspath(__file__))
    conf = os.path.join(here, "golden", "mfcc.conf")
    vconf = os.path.join(here, "golden", "vad.conf")
    n16, n8 = 24001, 9000
    (tmp_path / "a16.wav").write_bytes(mfcc.wav_bytes(synthetic.speech_like_wave(n16, 16000, 8), 16000))
    (tmp_path / "b8.wav").write_bytes(mfcc.wav_bytes(synthetic.speech_like_wave(n8, 8000, 9), 8000))
    scp = tmp_path / "wav.scp"
    scp.write_text("a16 %s\nb8 %s\n" % (tmp_path / "a16.wav", tmp_path / "b8.wav"))
    opts = recipe_opts(mfcc)

    def run(tag, *flags):
        d = tmp_path / tag
        d.mkdir()
        caplog.clear()
        with caplog.at_level(logging.WARNING, logger="mfcc"):
            rc = mfcc_vad.main(["compute-mfcc-vad", "--config=" + conf, "--vad-config=" + vconf] + list(flags) +
                               ["--write-num-frames=ark,t:%s" % (d / "utt2num_frames"), "scp:%s" % scp,
                                "ark,scp:%s,%s" % (d / "feats.ark", d / "feats.scp"), "ark,scp:%s,%s" % (d / "vad.ark", d / "vad.scp")])
        assert rc == 0
        return _table(d / "feats.scp"), _table(d / "vad.scp"), {k: int(v) for k, v in _table(d / "utt2num_frames").items()}, caplog.text

    feats, vad, nf, log = run("down", "--allow-downsample=true")
    assert sorted(feats) == sorted(vad) == sorted(nf) == ["a16", "b8"] and "skipping" not in log
    assert nf["a16"] == int(opts.num_frames(ref.num_output(n16, 16000, 8000))) and nf["b8"] == int(opts.num_frames(n8))
    import kaldi_io
    mats = dict(kaldi_io.read_mat_scp(str(tmp_path / "down" / "feats.scp")))
    assert mats["a16"].shape == (nf["a16"], opts.num_ceps) and mats["b8"].shape == (nf["b8"], opts.num_ceps)

    feats, vad, nf, log = run("plain")
    assert sorted(feats) == sorted(vad) == sorted(nf) == ["b8"]
    assert "Sample frequency 16000 of key a16 differs from --sample-frequency=8000; skipping (no resampling)" in log

    feats, vad, nf, log = run("up", "--sample-frequency=16000", "--allow-downsample=true")
    assert sorted(feats) == sorted(vad) == sorted(nf) == ["a16"]
    assert "Waveform and config sample Frequency mismatch: 8000 .vs 16000" in log and "--allow-upsample=true" in log
