"""Host side of the native SPHERE reader (xvector_amd/sphere.py; no GPU): the G.711 tables against the formulas
and ``audioop``, the header grammar, the recognised and refused sph2pipe command forms, ``mfcc.load_wav`` without any sph2pipe
program, the unchanged shell route for what is not native, augmented entries and wav-to-duration."""
import logging
import os
import stat

import numpy as np
import pytest

import sphere_ref as ref
from xvector_amd import augment, mfcc, sphere


@pytest.fixture
def no_sph2pipe(tmp_path, monkeypatch):
    """A PATH without any sph2pipe: an empty directory only (``sh -c`` itself needs no PATH)."""
    d = tmp_path / "emptybin"
    d.mkdir()
    monkeypatch.setenv("PATH", str(d))
    monkeypatch.delenv("XVECTOR_NATIVE_SPH", raising=False)


@pytest.fixture
def stereo_ulaw(tmp_path):
    rng = np.random.default_rng(3)
    codes = np.concatenate([np.stack([np.arange(256), np.arange(255, -1, -1)]), rng.integers(0, 256, (2, 745))], axis=1).astype(np.uint8)
    p = tmp_path / "two ch.sph"                                   # a space in the path: the entries quote it
    p.write_bytes(ref.sph_bytes(codes, 8000, "ulaw"))
    return p, codes


# ------------------------------------------------------------------------------------------------
# tables
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coding,table", [("ulaw", sphere.ULAW_TABLE), ("alaw", sphere.ALAW_TABLE)])
def test_tables_are_g711(coding, table):
    assert table.dtype == np.int16 and table.shape == (256,)
    assert np.array_equal(table.astype(np.int64), ref.formula_table(coding))
    if ref.audioop is None:
        pytest.skip("no audioop in this Python: the formula comparison above stands alone")
    assert np.array_equal(table.astype(np.int64), ref.audioop_table(coding))


def test_table_landmarks():
    """Values anyone can check against G.711 by hand: mu-law 0xFF / 0x7F are +0 / -0, 0x80 / 0x00 the extremes +-32124; A-law
    0xD5 / 0x55 are +-8, 0xAA / 0x2A the extremes +-32256."""
    u, a = sphere.ULAW_TABLE, sphere.ALAW_TABLE
    assert (u[0xFF], u[0x7F], u[0x80], u[0x00]) == (0, 0, 32124, -32124)
    assert (a[0xD5], a[0x55], a[0xAA], a[0x2A]) == (8, -8, 32256, -32256)


# ------------------------------------------------------------------------------------------------
# the header
# ------------------------------------------------------------------------------------------------
def test_header_fields_in_any_order_and_size():
    x = np.arange(40, dtype=np.int16).reshape(2, 20)
    for seed in range(4):
        for header in (1024, 2048):
            data = ref.sph_bytes(x, 16000, "pcm", "10", header=header, shuffle=seed)
            h = sphere.parse_header(data, "k")
            assert (h.size, h.rate, h.channels, h.n_bytes, h.byte_format, h.coding, h.shorten, h.sample_count) == \
                (header, 16000, 2, 2, "10", "pcm", False, 20)
            assert len(data) == header + 80


@pytest.mark.parametrize("name,want", [("ulaw", "ulaw"), ("mu-law", "ulaw"), ("pculaw", "ulaw"), ("alaw", "alaw"), ("", "pcm"),
                                       ("pcm", "pcm")])
def test_header_coding_names(name, want):
    pcm = want == "pcm"
    x = np.zeros((1, 8), np.int16 if pcm else np.uint8)
    h = sphere.parse_header(ref.sph_bytes(x, 8000, "pcm" if pcm else want, coding_name=name), "k")
    assert h.coding == want and not h.shorten and h.n_bytes == (2 if pcm else 1)


def test_header_errors_name_the_key():
    good = ref.sph_bytes(np.zeros((1, 8), np.int16), 8000)
    with pytest.raises(mfcc.WavError, match="utt7.*NIST_1A"):
        sphere.parse_header(b"RIFF" + good[4:], "utt7")
    with pytest.raises(mfcc.WavError, match="utt7.*end_head"):
        sphere.parse_header(good.replace(b"end_head", b"end_haed"), "utt7")
    with pytest.raises(mfcc.WavError, match="utt7.*sample_rate"):
        sphere.parse_header(ref.sph_bytes(np.zeros((1, 8), np.int16), 8000, fields={"sample_rate": None}), "utt7")
    with pytest.raises(mfcc.WavError, match="utt7.*header size"):
        sphere.parse_header(good.replace(b"   1024\n", b"   10x4\n"), "utt7")


def _cmd(path, channel=None, pcm=True):
    c = sphere.Command()
    c.path, c.channel, c.pcm = str(path), channel, pcm
    return c


def test_files_left_to_sph2pipe():
    """Three channels, shorten, 8-bit or 24-bit PCM and G.711 without -p are not native: ``describe`` says so naming the key."""
    def describe(data, **kw):
        h = sphere.parse_header(data, "k9")
        return sphere.describe("k9", _cmd("/d/x.sph", **kw), h, len(data))

    with pytest.raises(sphere.NotNative, match="k9.*channel_count 3.*not native"):
        describe(ref.sph_bytes(np.zeros((3, 8), np.uint8), 8000, "ulaw"))
    short = ref.sph_bytes(np.zeros((1, 8), np.uint8), 8000, "ulaw", coding_name="ulaw,embedded-shorten-v2.00")
    assert sphere.parse_header(short, "k9").shorten
    with pytest.raises(sphere.NotNative, match="k9.*shorten.*not native"):
        describe(short)
    with pytest.raises(sphere.NotNative, match="not native"):
        describe(ref.sph_bytes(np.zeros((1, 8), np.int16), 8000, "pcm", coding_name="pcm,embedded-shorten-v2.00"))
    with pytest.raises(sphere.NotNative, match="3-byte PCM"):
        describe(ref.sph_bytes(np.zeros((1, 8), np.int16), 8000, fields={"sample_n_bytes": 3}))
    with pytest.raises(sphere.NotNative, match="without -p"):
        describe(ref.sph_bytes(np.zeros((1, 8), np.uint8), 8000, "alaw"), pcm=False)
    assert issubclass(sphere.NotNative, mfcc.WavError)
    # 16-bit PCM needs no -p; -c beyond the file's channels is an error, not a fallback
    c = describe(ref.sph_bytes(np.zeros((2, 8), np.int16), 8000, "pcm", "10"), pcm=False, channel=1)
    assert (c.coding, c.stride, c.width, c.n, c.channel, c.data_off) == (sphere.PCM16_BE, 4, 2, 8, 1, 1024)
    with pytest.raises(mfcc.WavError, match="k9: -c 2"):
        describe(ref.sph_bytes(np.zeros((1, 8), np.int16), 8000), channel=1)


def test_sample_count_rule(tmp_path, caplog):
    """Whole frames present, capped by sample_count; a header that promises more is truncated with ONE warning per file."""
    codes = np.arange(2 * 50, dtype=np.uint8).reshape(2, 50)
    cases = {"exact": (ref.sph_bytes(codes, 8000, "ulaw"), 50),
             "nocount": (ref.sph_bytes(codes, 8000, "ulaw", sample_count=False), 50),
             "capped": (ref.sph_bytes(codes, 8000, "ulaw", sample_count=30), 30),
             "odd": (ref.sph_bytes(codes, 8000, "ulaw", sample_count=False) + b"\x00", 50),      # half a frame at the end
             "promised": (ref.sph_bytes(codes, 8000, "ulaw", sample_count=80)[:-1], 49)}
    for name, (data, want) in cases.items():
        p = tmp_path / (name + ".sph")
        p.write_bytes(data)
        rx = "sph2pipe -f wav -p %s |" % p
        caplog.clear()
        with caplog.at_level(logging.WARNING, logger="mfcc"):
            n = [sphere.recognise(name, rx).n for _ in range(3)]
        assert n == [want] * 3, name
        promises = [r for r in caplog.records if "promises 80 samples" in r.getMessage()]
        assert len(promises) == (1 if name == "promised" else 0), name
        rate, x = mfcc.load_wav(name, rx)
        assert rate == 8000 and x.shape == (2, want)
        assert np.array_equal(x[1], ref.decode(np.frombuffer(data, np.uint8), ref.ULAW, 2, 1, want, 1024))


# ------------------------------------------------------------------------------------------------
# the command
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rx,path,channel,pcm", [
    ("sph2pipe -f wav -p -c 1 /d/a.sph |", "/d/a.sph", 0, True),
    ("sph2pipe -f wav -p -c 2 /d/a.sph |", "/d/a.sph", 1, True),
    ("sph2pipe -f wav -p /d/a.sph |", "/d/a.sph", None, True),
    ("sph2pipe -f wav /d/a.sph |", "/d/a.sph", None, False),
    ("sph2pipe -f rif -c 1 -p /d/a.sph |", "/d/a.sph", 0, True),
    ("sph2pipe -c 2 /d/a.sph -p -f wav |", "/d/a.sph", 1, True),
    ("/opt/kaldi/tools/sph2pipe_v2.5/sph2pipe -f wav -p -c 1 /d/a.sph |", "/d/a.sph", 0, True),
    ("sph2pipe -f wav -p -c 1 '/d/with space/a.sph' |", "/d/with space/a.sph", 0, True),
    ('sph2pipe -f wav -p -c 1 "/d/with space/a.sph"|', "/d/with space/a.sph", 0, True),
    ("sph2pipe -f wav -p -c 1 /d/with\\ space/a.sph |", "/d/with space/a.sph", 0, True),
    ("  sph2pipe  -f  wav  -p  /d/a.sph  |  ", "/d/a.sph", None, True),
])
def test_recognised_commands(rx, path, channel, pcm):
    c = sphere.parse_command(rx)
    assert c is not None and (c.path, c.channel, c.pcm) == (path, channel, pcm)


@pytest.mark.parametrize("rx", [
    "sph2pipe -p -c 1 /d/a.sph |",                                # no -f: SPHERE out
    "sph2pipe -f sph -p /d/a.sph |", "sph2pipe -f raw -p /d/a.sph |", "sph2pipe -f au -p /d/a.sph |", "sph2pipe -f aif /d/a.sph |",
    "sph2pipe -f wav -p -t 0:10 /d/a.sph |", "sph2pipe -f wav -p -s 0:80000 /d/a.sph |",
    "sph2pipe -f wav -u /d/a.sph |", "sph2pipe -f wav -a /d/a.sph |",
    "sph2pipe -f wav -p /d/a.sph /d/out.wav |",                   # an output file
    "sph2pipe -f wav -p -c 1 /d/a.sph | sox -t wav - -r 8k -t wav - |",
    "sph2pipe -f wav -p -c 3 /d/a.sph |", "sph2pipe -f wav -p -c 0 /d/a.sph |", "sph2pipe -f wav -p -c /d/a.sph |",
    "sph2pipe -f wav -f wav -p /d/a.sph |", "sph2pipe -f wav -p -c 1 -c 2 /d/a.sph |",
    "sph2pipe -fwav -p /d/a.sph |", "sph2pipe -f wav -p |", "sph2pipe -f wav -p - |", "sph2pipe -f |",
    "sph2pipe -f wav -p /d/a.sph", "/d/a.sph", "cat /d/a.sph |", "mysph2pipe -f wav -p /d/a.sph |", "sph2pipe.sh -f wav -p /d/a.sph |",
    "sph2pipe -f wav -p '/d/a.sph |", "sph2pipe -f wav -p /d/a.sph > /tmp/x; cat /tmp/x |",
    "cd /d && sph2pipe -f wav -p a.sph |", "sph2pipe -f wav -p -x /d/a.sph |",
])
def test_refused_commands(rx):
    assert sphere.parse_command(rx) is None


def test_shell_syntax_is_left_to_the_shell():
    """What shlex would pass through but a shell would expand or redirect: such a stage is not 'exactly one sph2pipe command'."""
    for rx in ("sph2pipe -f wav -p /d/a.sph 2>/dev/null |", "sph2pipe -f wav -p $DIR/a.sph |", "sph2pipe -f wav -p /d/*.sph |",
               "sph2pipe -f wav -p `echo a.sph` |", "sph2pipe -f wav -p /d/a.sph & |", "sph2pipe -f wav -p ~/a.sph |"):
        assert sphere.parse_command(rx) is None, rx


# ------------------------------------------------------------------------------------------------
# load_wav: native, and the unchanged shell route
# ------------------------------------------------------------------------------------------------
def test_load_wav_native_without_any_sph2pipe(no_sph2pipe, stereo_ulaw):
    """THE test of the feature: with no sph2pipe on PATH the recipe's entries are read; before, the shell's status 127."""
    p, codes = stereo_ulaw
    want = ref.formula_table("ulaw")[codes].astype(np.int16)
    for flags, rows in (("-c 1", [0]), ("-c 2", [1]), ("", [0, 1])):
        rate, x = mfcc.load_wav("utt", "sph2pipe -f wav -p %s '%s' |" % (flags, p))
        assert rate == 8000 and x.dtype == np.int16 and x.shape == (len(rows), 1001)
        assert np.array_equal(x, want[rows])
    # the other codings through the same door
    rng = np.random.default_rng(5)
    pcm = rng.integers(-32768, 32768, (2, 333)).astype(np.int16)
    pcm[0, :2] = (-32768, 32767)
    acodes = rng.integers(0, 256, (1, 77)).astype(np.uint8)
    d = p.parent
    for name, data, want, flags in (("le.sph", ref.sph_bytes(pcm, 16000, "pcm", "01"), pcm[1:2], "-c 2"),
                                    ("be.sph", ref.sph_bytes(pcm, 16000, "pcm", "10", header=2048), pcm[0:1], "-c 1"),
                                    ("a.sph", ref.sph_bytes(acodes, 8000, "alaw"), ref.formula_table("alaw")[acodes], "-p")):
        (d / name).write_bytes(data)
        rate, x = mfcc.load_wav("k", "sph2pipe -f wav %s %s |" % (flags, d / name))
        assert np.array_equal(x, want) and x.dtype == np.int16
    # what is not native still goes to the shell, which has no such program here
    with pytest.raises(mfcc.WavError, match="utt: command .* exited with status 127"):
        mfcc.load_wav("utt", "sph2pipe -f wav -p -t 0:1 '%s' |" % p)
    with pytest.raises(mfcc.WavError, match="utt: cannot read"):
        mfcc.load_wav("utt", "sph2pipe -f wav -p %s/missing.sph |" % d)


def _fake_sph2pipe(tmp_path, monkeypatch, wav):
    """A program named sph2pipe that logs its arguments and writes ``wav``."""
    bindir = tmp_path / "bin"
    bindir.mkdir()
    (tmp_path / "fake.wav").write_bytes(wav)
    prog = bindir / "sph2pipe"
    prog.write_text("#!/bin/sh\necho \"$@\" >> '%s'\nexec cat '%s'\n" % (tmp_path / "calls.log", tmp_path / "fake.wav"))
    prog.chmod(prog.stat().st_mode | stat.S_IXUSR)
    monkeypatch.setenv("PATH", str(bindir) + os.pathsep + os.environ["PATH"])
    return tmp_path / "calls.log"


def test_fallback_is_the_unchanged_shell_route(tmp_path, monkeypatch, stereo_ulaw):
    p, codes = stereo_ulaw
    marker = np.arange(100, 164, dtype=np.int16)
    log = _fake_sph2pipe(tmp_path, monkeypatch, mfcc.wav_bytes(marker, 8000))
    monkeypatch.delenv("XVECTOR_NATIVE_SPH", raising=False)
    # native: the program is not started
    rate, x = mfcc.load_wav("k", "sph2pipe -f wav -p -c 1 '%s' |" % p)
    assert x.shape == (1, 1001) and not log.exists()
    # a shorten-labelled file: the program runs with the entry's own arguments
    sh = tmp_path / "short.sph"
    sh.write_bytes(ref.sph_bytes(codes, 8000, "ulaw", coding_name="ulaw,embedded-shorten-v2.00"))
    rate, x = mfcc.load_wav("k", "sph2pipe -f wav -p -c 1 %s |" % sh)
    assert rate == 8000 and np.array_equal(x, marker[None])
    assert log.read_text() == "-f wav -p -c 1 %s\n" % sh
    assert sphere.recognise("k", "sph2pipe -f wav -p -c 1 %s |" % sh) is None
    # XVECTOR_NATIVE_SPH=0: everything runs in the shell
    monkeypatch.setenv("XVECTOR_NATIVE_SPH", "0")
    rate, x = mfcc.load_wav("k", "sph2pipe -f wav -p -c 2 '%s' |" % p)
    assert np.array_equal(x, marker[None])
    assert log.read_text().splitlines()[1] == "-f wav -p -c 2 %s" % p
    assert augment.duration_samples("k", "sph2pipe -f wav -p -c 2 '%s' |" % p) == (64, 8000)


# ------------------------------------------------------------------------------------------------
# augmented entries, durations, the reader's rules
# ------------------------------------------------------------------------------------------------
def test_augmented_entry_reads_its_input_natively(no_sph2pipe, stereo_ulaw, tmp_path):
    p, codes = stereo_ulaw
    rir = tmp_path / "R.wav"
    h = np.zeros(40, np.int16)
    h[7] = 20000
    rir.write_bytes(mfcc.wav_bytes(h, 8000))
    rx = "sph2pipe -f wav -p -c 2 '%s' | wav-reverberate --shift-output=true --impulse-response=%s - - |" % (p, rir)
    node = augment.parse_rx(rx)
    assert isinstance(node, augment.Reverb) and node.input.rx == "sph2pipe -f wav -p -c 2 '%s' |" % p
    plan = augment.Augmenter().plan([("aug", node)])
    top = plan.top[0]
    assert (top.N, top.M, top.rate, top.shift) == (1001, 1001, 8000, 7)
    assert np.array_equal(top.x[3], ref.formula_table("ulaw")[codes[1]].astype(np.int16))
    assert augment.duration_samples("aug", rx) == (1001, 8000)


def test_wav_to_duration_reads_headers_only(no_sph2pipe, stereo_ulaw, tmp_path):
    import mfcc_vad
    p, _ = stereo_ulaw
    big = tmp_path / "big.sph"                       # sample_count below what the file holds: the header's count is the length
    big.write_bytes(ref.sph_bytes(np.zeros((1, 12345), np.int16), 16000, "pcm", "10", sample_count=12000))
    wav = tmp_path / "w.wav"
    wav.write_bytes(mfcc.wav_bytes(np.zeros(4000, np.int16), 8000))
    scp = tmp_path / "wav.scp"
    scp.write_text("a sph2pipe -f wav -p -c 1 '%s' |\nb sph2pipe -f wav -p -c 1 %s |\nc %s\n" % (p, big, wav))
    out = tmp_path / "utt2dur"
    assert mfcc_vad.main(["wav-to-duration", "--read-entire-file=true", "scp:%s" % scp, "ark,t:%s" % out]) == 0
    got = dict(line.split() for line in out.read_text().splitlines())
    assert got == {"a": "%.7g" % (np.float32(1001) / np.float32(8000)), "b": "0.75", "c": "0.5"}


def test_reader_rules_from_the_header_alone(no_sph2pipe, stereo_ulaw, tmp_path, caplog):
    """mfcc_vad._read_waves: CodedWaves for plain recognised entries, Kaldi's skip rules without reading a sample, a host-decoded
    Wave for an entry that is to be resampled."""
    import mfcc_vad
    p, codes = stereo_ulaw
    wide = tmp_path / "wide.sph"
    pcm = np.arange(-300, 300, dtype=np.int16)[None]
    wide.write_bytes(ref.sph_bytes(pcm, 16000, "pcm", "10"))
    scp = tmp_path / "wav.scp"
    scp.write_text("a sph2pipe -f wav -p -c 1 '%s' |\nb sph2pipe -f wav -p -c 2 '%s' |\nab sph2pipe -f wav -p '%s' |\n"
                   "w sph2pipe -f wav -p -c 1 %s |\n" % (p, p, p, wide))
    opts = mfcc.MfccOptions(sample_frequency=8000)
    with caplog.at_level(logging.WARNING, logger="mfcc"):
        got = dict(mfcc_vad._read_waves(str(scp), opts))
    assert sorted(got) == ["a", "ab", "b"] and "Sample frequency 16000 of key w" in caplog.text
    assert "Channel not specified but you have data with 2 channels; defaulting to zero (key ab)" in caplog.text
    assert all(isinstance(w, mfcc.CodedWave) and w.shape == (1001,) and w.rate == 8000 and w.channels == 2 for w in got.values())
    assert (got["a"].channel, got["b"].channel, got["ab"].channel) == (0, 1, 0)
    assert got["a"].ident == got["b"].ident and got["a"].coding == sphere.ULAW
    assert np.array_equal(got["a"].region(), np.ascontiguousarray(codes.T).reshape(-1))
    # --channel applies to what the command leaves: one channel after -c, two without
    got = dict(mfcc_vad._read_waves(str(scp), mfcc.MfccOptions(sample_frequency=8000, channel=1)))
    assert sorted(got) == ["ab"] and got["ab"].channel == 1
    assert dict(mfcc_vad._read_waves(str(scp), mfcc.MfccOptions(sample_frequency=8000, min_duration=0.2))) == {}
    # another rate, allowed: decoded here, resampled on the device like any other Wave
    got = dict(mfcc_vad._read_waves(str(scp), mfcc.MfccOptions(sample_frequency=8000, allow_downsample=True)))
    assert isinstance(got["w"], mfcc.Wave) and got["w"].rate == 16000 and np.array_equal(np.asarray(got["w"]), pcm[0])
    assert isinstance(got["a"], mfcc.CodedWave)
