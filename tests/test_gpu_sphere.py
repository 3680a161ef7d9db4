"""The SPHERE decoder on the GPU (csrc/xv_sphere.hip): every coding, channel layout, edge length and alignment in
one launch per sample format against the table-free formulas of tests/sphere_ref.py bit for bit, shared raw spans, the bitwise
independence of an utterance from its batch, the refused arguments, and the feature engine and the stage-1 CLI on coded
entries against the same audio decoded on the host."""
import ctypes
import os

import numpy as np
import pytest

import sphere_ref as ref

pytestmark = pytest.mark.gpu

TILE = 4096
LENGTHS = (0, 1, 2, 7, 8, 9, 15, 16, 17, TILE - 1, TILE, TILE + 1, 2 * TILE + TILE // 2 + 3)
LAYOUTS = [(coding, nch, ch) for coding in range(4) for nch in (1, 2) for ch in range(nch)]
POISON16, POISON32, RAW_POISON = 0x7B5D, 0x7FC0BEEF, 0xEE
GUARD = 37                     # elements before the first output: odd, so every output offset has its own alignment


@pytest.fixture(scope="module")
def env():
    import torch
    from xvector_amd import hiplib, mfcc, sphere, synthetic
    hiplib.require_gpu()
    assert sphere.DEC_TILE == TILE
    return dict(torch=torch, hiplib=hiplib, mfcc=mfcc, sphere=sphere, synthetic=synthetic)


def _region(rng, coding, nch, n):
    """The bytes of n frames: G.711 channels run through all 256 codes (up and down) and go on with random bytes; PCM is
    full-scale random and holds -32768 and 32767."""
    if coding in (ref.ULAW, ref.ALAW):
        chans = [np.concatenate([np.arange(256)[::1 - 2 * c], rng.integers(0, 256, max(n - 256, 0))])[:n] for c in range(nch)]
        return np.ascontiguousarray(np.stack(chans, axis=1).astype(np.uint8)).reshape(-1)
    x = rng.integers(-32768, 32768, (n, nch)).astype(np.int16)
    x.reshape(-1)[:2] = (-32768, 32767)[:x.size]
    return np.frombuffer(x.astype("<i2" if coding == ref.PCM16_LE else ">i2").tobytes(), np.uint8)


@pytest.fixture(scope="module")
def batch():
    """Every layout x every length; each utterance has a raw span of its own, begun at the next residue mod 16, poison between."""
    rng = np.random.default_rng(23)
    parts, utts, pos, k = [], [], 0, 0
    for coding, nch, ch in LAYOUTS:
        for n in LENGTHS:
            width = 2 if coding < 2 else 1
            pad = (k % 16 - pos) % 16 + 16
            parts.append(np.full(pad, RAW_POISON, np.uint8))
            pos += pad
            assert pos % 16 == k % 16
            reg = _region(rng, coding, nch, n)
            utts.append(dict(raw_off=pos, n=n, stride=width * nch, ch_off=width * ch, coding=coding))
            parts.append(reg)
            pos += len(reg)
            k += 1
    parts.append(np.full(5, RAW_POISON, np.uint8))          # the buffer ends 5 bytes after the last span: no whole 16 to read
    raw = np.concatenate(parts)
    assert {u["raw_off"] % 16 for u in utts} == set(range(16))
    want = [ref.decode(raw, u["coding"], u["stride"], u["ch_off"], u["n"], u["raw_off"]) for u in utts]
    return dict(raw=raw, utts=utts, want=want)


def _launch(env, raw, utts, fmt, guard=GUARD, tail=64):
    """One xv_wave_decode launch of ``utts`` packed back to back after ``guard`` poisoned elements: -> the outputs; asserts
    that the guards before the first and after the last output are untouched."""
    torch, hiplib, sphere = env["torch"], env["hiplib"], env["sphere"]
    ns = np.array([u["n"] for u in utts], np.int64)
    off = guard + np.concatenate([[0], np.cumsum(ns[:-1])]).astype(np.int64)
    total = guard + int(ns.sum()) + tail
    utt = np.zeros((len(utts), 8), np.int64)
    for i, u in enumerate(utts):
        utt[i, :6] = (u["raw_off"], u["n"], u["stride"], u["ch_off"], u["coding"], off[i])
    if fmt == 0:
        host = np.full(total, POISON16, np.int16)
    else:
        host = np.full(total, POISON32, np.uint32).view(np.float32)
    out = torch.from_numpy(host.copy()).to("cuda:0")
    # a device buffer padded to a multiple of 16 like any allocation, but raw_bytes says where the data end
    d_raw = torch.from_numpy(np.ascontiguousarray(raw)).to("cuda:0")
    hiplib.wave_decode(d_raw, utt, torch.from_numpy(sphere.tile_list(ns, off)).to("cuda:0"), out, fmt)
    torch.cuda.synchronize()
    y = out.cpu().numpy()
    bits = y if fmt == 0 else y.view(np.uint32)
    poison = POISON16 if fmt == 0 else POISON32
    assert (bits[:guard] == poison).all(), "the guard before the first output was written"
    assert (bits[guard + int(ns.sum()):] == poison).all(), "the guard after the last output was written"
    return [y[o:o + n] for o, n in zip(off.tolist(), ns.tolist())]


@pytest.fixture(scope="module")
def results(env, batch):
    return {fmt: _launch(env, batch["raw"], batch["utts"], fmt) for fmt in (0, 1)}


@pytest.mark.parametrize("fmt", [0, 1])
def test_every_layout_length_and_alignment_bit_for_bit(batch, results, fmt):
    assert len(batch["utts"]) == len(LAYOUTS) * len(LENGTHS) == 156
    bad = []
    for u, want, got in zip(batch["utts"], batch["want"], results[fmt]):
        assert got.dtype == (np.int16 if fmt == 0 else np.float32) and got.shape == want.shape
        if not np.array_equal(got, want if fmt == 0 else want.astype(np.float32)):
            i = int(np.flatnonzero(got != want)[0])
            bad.append("%r: first difference at sample %d: got %r, want %r" % (u, i, got[i], want[i]))
    assert not bad, "\n".join(bad[:10])


def test_reference_is_g711_by_an_independent_implementation():
    """The formulas the GPU is held to, against audioop (where this Python has it) for all 256 codes."""
    if ref.audioop is None:
        pytest.skip("no audioop in this Python")
    for coding in ("ulaw", "alaw"):
        assert np.array_equal(ref.formula_table(coding), ref.audioop_table(coding))


def test_shared_spans_and_independence_of_the_batch(env, batch, results):
    """-c 1 and -c 2 of one file read the same bytes; an utterance has the same bits alone, first and last in a batch."""
    utts, want = batch["utts"], batch["want"]
    long_ = [i for i, u in enumerate(utts) if u["n"] == LENGTHS[-1]]
    pairs = [(i, j) for i in long_ for j in long_ if utts[i]["coding"] == utts[j]["coding"] and utts[i]["stride"] == utts[j]["stride"]
             and utts[i]["ch_off"] == 0 and utts[j]["ch_off"] > 0]
    assert len(pairs) == 4
    for fmt in (0, 1):
        for i, j in pairs:
            left = dict(utts[i])
            right = dict(utts[i], ch_off=utts[j]["ch_off"])                   # the other channel of the SAME span
            a, b = _launch(env, batch["raw"], [left, right], fmt, guard=8)
            assert np.array_equal(a, want[i])
            assert np.array_equal(b, ref.decode(batch["raw"], right["coding"], right["stride"], right["ch_off"], right["n"], right["raw_off"]))
        for i in (long_[0], long_[5], long_[-1]):
            others = [utts[k] for k in (3, 40, 100, long_[2])]
            alone = _launch(env, batch["raw"], [utts[i]], fmt, guard=0)[0]
            first = _launch(env, batch["raw"], [utts[i]] + others, fmt, guard=3)[0]
            last = _launch(env, batch["raw"], others + [utts[i]], fmt, guard=13)[-1]
            for got in (alone, first, last, results[fmt][i]):
                assert np.array_equal(got.view(np.uint16 if fmt == 0 else np.uint32), alone.view(np.uint16 if fmt == 0 else np.uint32))
            assert np.array_equal(alone, want[i])


def test_refused_arguments_leave_the_output_alone(env):
    torch, hiplib, sphere = env["torch"], env["hiplib"], env["sphere"]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")  # noqa: E731
    raw_h = np.arange(4096, dtype=np.uint32).astype(np.uint8)
    raw = dev(raw_h)
    out = dev(np.full(4096, POISON16, np.int16))
    out32 = dev(np.full(4096, POISON32, np.uint32).view(np.float32))
    tiles = dev(np.zeros((1, 2), np.int64))

    def untouched():
        torch.cuda.synchronize()
        return bool((out.cpu().numpy() == POISON16).all()) and bool((out32.cpu().numpy().view(np.uint32) == POISON32).all())

    good = [16, 1000, 2, 1, ref.ULAW, 7, 0, 0]

    def call(o=out, fmt=0, **kw):
        d = list(good)
        for k, v in kw.items():
            d[dict(raw_off=0, n=1, stride=2, ch_off=3, coding=4, out_off=5, res=6)[k]] = v
        hiplib.wave_decode(raw, np.array([d], np.int64), tiles, o, fmt)

    for kw in (dict(coding=4), dict(coding=-1), dict(stride=3), dict(stride=0), dict(stride=8), dict(ch_off=2), dict(ch_off=-1),
               dict(coding=ref.PCM16_BE, ch_off=1),                          # a 16-bit sample that would straddle two frames
               dict(coding=ref.PCM16_LE, stride=1, ch_off=0),
               dict(n=-1), dict(raw_off=-1), dict(raw_off=4096 - 1999), dict(n=2049), dict(raw_off=1 << 40),
               dict(out_off=-1), dict(out_off=4096 - 999), dict(out_off=1 << 40), dict(n=1 << 62), dict(res=1)):
        with pytest.raises(hiplib.XvectorHipError, match=r"xv_wave_decode failed \(-1\)"):
            call(**kw)
        with pytest.raises(hiplib.XvectorHipError, match=r"\(-1\)"):
            call(o=out32, fmt=1, **kw)
    assert untouched()
    # the raw entry point: a null pointer, a negative count, an unknown sample format, a misaligned buffer
    lib = hiplib.load()
    d_utt = dev(np.array([good], np.int64))
    ptr = lambda t, add=0: ctypes.c_void_p(t.data_ptr() + add)  # noqa: E731

    def rawcall(r=ptr(raw), nbytes=4096, u=ptr(d_utt), n_utts=1, t=ptr(tiles), n_tiles=1, o=ptr(out), fmt=0):
        return lib.xv_wave_decode(r, nbytes, u, n_utts, t, n_tiles, o, fmt, None)

    assert rawcall(r=None) == -1 and rawcall(u=None) == -1 and rawcall(t=None) == -1 and rawcall(o=None) == -1
    assert rawcall(n_utts=-1) == -1 and rawcall(n_utts=0) == -1 and rawcall(n_tiles=-1) == -1 and rawcall(nbytes=-1) == -1
    assert rawcall(fmt=2) == -1 and rawcall(fmt=-1) == -1 and rawcall(r=ptr(raw, 4)) == -1 and rawcall(o=ptr(out, 2)) == -1
    assert b"wave_decode" in lib.xv_last_error()
    assert rawcall(n_tiles=0) == 0 and rawcall(n_tiles=0, r=None, o=None) == 0          # nothing to do is not an error
    assert untouched()
    # and the same call with nothing wrong writes exactly its 1000 samples
    assert rawcall() == 0
    torch.cuda.synchronize()
    y = out.cpu().numpy()
    assert (y[:7] == POISON16).all() and (y[1007:] == POISON16).all()
    assert np.array_equal(y[7:1007], ref.decode(raw_h, ref.ULAW, 2, 1, 1000, 16))
    assert sphere.tile_list([0, 1, TILE - 7, TILE - 6], [0, 7, 7, 7]).tolist() == [[1, 0], [2, 0], [3, 0], [3, TILE]]


# ------------------------------------------------------------------------------------------------
# the engine and the CLI
# ------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def recipe_opts(mfcc, **kw):
    here = os.path.dirname(os.path.abspath(__file__))
    o = mfcc.MfccOptions().update(mfcc.read_config(os.path.join(here, "golden", "mfcc.conf")))
    return o.update(kw.items())


@pytest.fixture(scope="module")
def corpus(env, tmp_path_factory):
    """A two-channel mu-law file, a big-endian one-channel PCM file, a one-channel A-law file (8 kHz, speech-like) and a plain
    WAV; for each entry the int16 wave a host decode gives."""
    mfcc, synthetic = env["mfcc"], env["synthetic"]
    d = tmp_path_factory.mktemp("sph")
    sp = lambda n, seed: synthetic.speech_like_wave(n, 8000, seed)  # noqa: E731
    codes = np.stack([ref.lin2ulaw(sp(12345, 1)), ref.lin2ulaw(sp(12345, 2))])
    (d / "conv.sph").write_bytes(ref.sph_bytes(codes, 8000, "ulaw"))
    be = sp(9001, 3)
    (d / "mic.sph").write_bytes(ref.sph_bytes(be, 8000, "pcm", "10", header=2048))
    acodes = np.arange(7000, dtype=np.int64) * 37 % 256                  # every A-law code, over and over
    (d / "a.sph").write_bytes(ref.sph_bytes(acodes.astype(np.uint8), 8000, "alaw", sample_count=False))
    plain = sp(8000, 4)
    (d / "p.wav").write_bytes(mfcc.wav_bytes(plain, 8000))
    u = ref.formula_table("ulaw").astype(np.int16)
    entries = [("conv-A", "sph2pipe -f wav -p -c 1 %s/conv.sph |" % d, u[codes[0]]),
               ("conv-B", "sph2pipe -f wav -p -c 2 %s/conv.sph |" % d, u[codes[1]]),
               ("mic", "sph2pipe -f wav -p -c 1 %s/mic.sph |" % d, be),
               ("alaw", "sph2pipe -f wav -p %s/a.sph |" % d, ref.formula_table("alaw").astype(np.int16)[acodes]),
               ("plain", "%s/p.wav" % d, plain)]
    return dict(dir=d, entries=entries)


def _coded(env, corpus, opts):
    mfcc, sphere = env["mfcc"], env["sphere"]
    out = {}
    for key, rx, wave in corpus["entries"]:
        c = sphere.recognise(key, rx)
        if c is not None:
            out[key] = mfcc.select_coded(key, c, opts)
            assert isinstance(out[key], mfcc.CodedWave) and out[key].shape == wave.shape
            assert np.array_equal(mfcc.load_wav(key, rx)[1][0], wave)                  # the host decode agrees with the formulas
    return out


def test_engine_coded_waves_give_the_bits_of_host_decoded_ones(env, corpus):
    mfcc, synthetic = env["mfcc"], env["synthetic"]
    opts = recipe_opts(mfcc, allow_downsample=True, seed=3)
    assert opts.sample_frequency == 8000
    coded = _coded(env, corpus, opts)
    host = {k: w for k, _, w in corpus["entries"]}
    keys = ["conv-A", "conv-B", "mic", "alaw"]
    ref_eng = mfcc.Mfcc(opts, mfcc.VadOptions())
    want, want_vad, _ = ref_eng.compute(keys + ["plain"], [host[k] for k in keys + ["plain"]])
    want = dict(zip(keys + ["plain"], want))
    want_vad = dict(zip(keys + ["plain"], want_vad))
    assert all(want[k].shape[0] > 80 for k in want)

    def check(eng, ks, waves, **kw):
        feats, vads, _ = eng.compute(ks, waves, **kw)
        for k, f, v in zip(ks, feats, vads):
            if k in want:
                assert np.array_equal(bits(f), bits(want[k])), k
                assert np.array_equal(v, want_vad[k]), k
        return feats

    # alone: int16 window, nothing but coded utterances; conv.sph goes up once for its two sides
    eng = mfcc.Mfcc(opts, mfcc.VadOptions())
    check(eng, keys, [coded[k] for k in keys])
    sizes = {"conv": 2 * 12345, "mic": 2 * 9001, "a": 7000}
    assert eng.stats["decoded"] == 4 and eng.stats["launches"] == 1 and eng.stats["resampled"] == 0
    assert eng.stats["raw_bytes"] == sum((s + 15) // 16 * 16 for s in sizes.values())
    # mixed with plain waves in one window, coded and plain alternating
    eng = mfcc.Mfcc(opts, mfcc.VadOptions())
    order = ["plain", "conv-B", "mic", "plain2", "conv-A"]
    waves = [host["plain"], coded["conv-B"], coded["mic"], host["mic"][:5000], coded["conv-A"]]
    check(eng, order, waves)
    assert eng.stats["decoded"] == 3 and eng.stats["launches"] == 1
    assert eng.stats["raw_bytes"] == sum((sizes[s] + 15) // 16 * 16 for s in ("conv", "mic"))
    # with a resampled wave: the fp32 window
    eng = mfcc.Mfcc(opts, mfcc.VadOptions())
    wide = synthetic.speech_like_wave(17001, 16000, 9)
    check(eng, ["conv-A", "wide", "plain", "alaw"], [coded["conv-A"], wide, host["plain"], coded["alaw"]], rates=[None, 16000, None, None])
    assert eng.stats["resampled"] == 1 and eng.stats["decoded"] == 2 and eng.stats["launches"] == 1
    # small windows cut between the two sides of one file: the file goes up once per window
    eng = mfcc.Mfcc(opts, mfcc.VadOptions(), window_samples=13000)
    check(eng, keys, [coded[k] for k in keys])
    assert eng.stats["launches"] == 4 and eng.stats["raw_bytes"] == sum((sizes[s] + 15) // 16 * 16 for s in ("conv", "conv", "mic", "a"))
    # compressed output: the payload bytes are those of the host-decoded waves
    packed_want, _, _ = ref_eng.compute(keys, [host[k] for k in keys], compress=True)
    packed, _, _ = mfcc.Mfcc(opts, mfcc.VadOptions()).compute(keys, [coded[k] for k in keys], compress=True)
    for k, a, b in zip(keys, packed, packed_want):
        assert (a.rows, a.cols) == (b.rows, b.cols) and a.rows > 80 and bytes(a.payload) == bytes(b.payload), k
    # a coded wave at another rate is the reader's to decode (select_coded); the engine refuses it
    with pytest.raises(NotImplementedError):
        mfcc.Mfcc(recipe_opts(mfcc, sample_frequency=16000, allow_upsample=True)).compute(["k"], [coded["mic"]])


def test_cli_sphere_entries_write_the_bytes_of_wav_entries(env, corpus, tmp_path, monkeypatch):
    """compute-mfcc-vad on both sides of the mu-law file, the big-endian PCM file and a WAV path, with no sph2pipe anywhere,
    against the same audio as WAV files: the same ark and scp bytes."""
    import mfcc_vad
    mfcc = env["mfcc"]
    here = os.path.dirname(os.path.abspath(__file__))
    conf, vconf = os.path.join(here, "golden", "mfcc.conf"), os.path.join(here, "golden", "vad.conf")
    empty = tmp_path / "emptybin"
    empty.mkdir()
    monkeypatch.setenv("PATH", str(empty))
    monkeypatch.delenv("XVECTOR_NATIVE_SPH", raising=False)
    entries = [e for e in corpus["entries"] if e[0] != "alaw"]
    outs = {}
    for tag in ("sph", "wav"):
        d = tmp_path / tag
        d.mkdir()
        lines = []
        for key, rx, wave in entries:
            if tag == "wav" and rx.endswith("|"):
                (d / (key + ".wav")).write_bytes(mfcc.wav_bytes(wave, 8000))
                rx = str(d / (key + ".wav"))
            lines.append("%s %s\n" % (key, rx))
        (d / "wav.scp").write_text("".join(lines))
        monkeypatch.chdir(d)                                  # relative outputs: the scp lines of the two runs can be equal
        for compress in ("false", "true"):
            assert mfcc_vad.main(["compute-mfcc-vad", "--config=" + conf, "--vad-config=" + vconf, "--compress=" + compress,
                                  "--write-num-frames=ark,t:nf_%s" % compress, "scp:wav.scp",
                                  "ark,scp:feats_%s.ark,feats_%s.scp" % (compress, compress),
                                  "ark,scp:vad_%s.ark,vad_%s.scp" % (compress, compress)]) == 0
        outs[tag] = {n: (d / n).read_bytes() for n in sorted(os.listdir(d)) if n.startswith(("feats_", "vad_", "nf_"))}
    assert sorted(outs["sph"]) == sorted(outs["wav"]) and len(outs["sph"]) == 10
    for n in outs["sph"]:
        assert outs["sph"][n] == outs["wav"][n], n
    assert outs["sph"]["nf_false"].decode().split() == ["conv-A", "154", "conv-B", "154", "mic", "113", "plain", "100"]
