"""The wav.scp -> x-vector route without a GPU: what the command line and the driver refuse before anything is launched, and the
reader thread's batching."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, TWIN

BASE = ["--vector-wspecifier", "ark,scp:/nonexistent/x.ark,/nonexistent/x.scp", "--model-dir", "/nonexistent/model"]


def _usage_error(argv, capsys):
    import extract_embedding as ee
    with pytest.raises(SystemExit) as e:
        ee.get_args(argv)
    assert e.value.code == 2                                  # argparse's usage error, before the model directory is looked at
    return capsys.readouterr().err


def test_wav_rspecifier_excludes_the_table_inputs(capsys):
    wav = ["--wav-rspecifier", "scp:wav.scp", "--cmn-window", "300"]
    assert "excludes" in _usage_error(BASE + wav + ["--feature-rspecifier", "scp:feats.scp"], capsys)
    assert "excludes" in _usage_error(BASE + wav + ["--vad-rspecifier", "scp:vad.scp"], capsys)
    assert "required" in _usage_error(BASE + ["--cmn-window", "300"], capsys)                # neither input
    assert "go with --wav-rspecifier" in _usage_error(BASE + ["--feature-rspecifier", "scp:f.scp", "--mfcc-config", "m.conf"], capsys)
    assert "scp:wav.scp" in _usage_error(BASE + ["--wav-rspecifier", "ark:wav.ark", "--cmn-window", "300"], capsys)


def test_wav_rspecifier_needs_a_cmn_window(capsys):
    assert "needs --cmn-window > 0" in _usage_error(BASE + ["--wav-rspecifier", "scp:wav.scp", "--cmn-window", "0"], capsys)
    assert "needs --cmn-window > 0" in _usage_error(BASE + ["--wav-rspecifier", "scp:wav.scp"], capsys)          # the default is 0


def test_wav_rspecifier_refuses_more_than_one_rank(capsys, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    err = _usage_error(BASE + ["--wav-rspecifier", "scp:wav.scp", "--cmn-window", "300"], capsys)
    assert "WORLD_SIZE=2" in err and "one process" in err


def test_accepted_wav_command_line_reaches_the_model_check(monkeypatch):
    """A well-formed --wav-rspecifier line passes the usage checks (and then fails on the missing model directory, as every
    command line does); the table-input line still parses as before."""
    import extract_embedding as ee
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for argv in (["--wav-rspecifier", "scp:wav.scp", "--cmn-window", "300", "--mfcc-config", "m.conf", "--vad-config", "v.conf"],
                 ["--feature-rspecifier", "scp:feats.scp"]):
        with pytest.raises(Exception, match="expects the input model"):
            ee.get_args(BASE + argv)


def test_shell_script_refuses_from_wav_on_several_gpus_before_python_starts(tmp_path):
    marker = tmp_path / "python-was-started"
    fake = tmp_path / "bin"
    fake.mkdir()
    (fake / "python").write_text("#!/bin/sh\ntouch '%s'\n" % marker)
    (fake / "python").chmod(0o755)
    env = dict(os.environ, PATH="%s:%s" % (fake, os.environ["PATH"]))
    script = os.path.join(TWIN, "extract_xvectors_mi355x.sh")
    r = subprocess.run(["bash", script, "--from-wav", "--ngpu", "2", str(tmp_path / "nnet"), str(tmp_path / "data"), str(tmp_path / "out")],
                       env=env, capture_output=True, text=True)
    assert r.returncode == 1 and "--from-wav" in r.stderr and "one GPU" in r.stderr
    assert not marker.exists() and not (tmp_path / "out").exists()
    # --from-wav on one GPU asks for wav.scp, not for feats.scp
    r = subprocess.run(["bash", script, "--from-wav", str(tmp_path / "nnet"), str(tmp_path / "data"), str(tmp_path / "out")],
                       env=env, capture_output=True, text=True)
    assert r.returncode == 1 and "wav.scp" in r.stderr and "feats.scp" not in r.stderr and not marker.exists()


def _options():
    from xvector_amd import mfcc
    opts, vopts = mfcc.MfccOptions(), mfcc.VadOptions()
    opts.update(mfcc.read_config(os.path.join(GOLDEN, "mfcc.conf")))
    vopts.update(mfcc.read_config(os.path.join(GOLDEN, "vad.conf")))
    return opts, vopts


def test_make_embedding_refuses_a_wave_table_with_a_vad_stream_or_without_cmn(tmp_path):
    import models
    from xvector_amd import extract_stream
    scp = tmp_path / "wav.scp"
    scp.write_text("")
    opts, vopts = _options()
    for kw in (dict(cmn_window=0), dict(cmn_window=300, vad_stream=iter(()))):
        table = extract_stream.WaveTable(str(scp), opts, vopts)
        with pytest.raises(ValueError, match="WaveTable"):
            models.Model().make_embedding(table, None, str(tmp_path / "no-model"), 25, 100, True, None, **kw)
        assert table._thread is None                          # refused before the reader thread was started


def test_wave_table_thread_deals_the_batches_of_compute_mfcc_vad(tmp_path):
    """The reader thread yields (keys, WaveBatch, None) per window: the batches mfcc_vad._planned_batches forms for the same
    budget, in order, with the interface make_embedding's loop uses on a window."""
    import mfcc_vad
    from xvector_amd import augment, extract_stream, mfcc
    opts, vopts = _options()
    rng = np.random.default_rng(0)
    lines = []
    for i, n in enumerate((8000, 12000, 9000, 30000, 4000)):
        path = tmp_path / ("u%d.wav" % i)
        path.write_bytes(mfcc.wav_bytes(rng.integers(-3000, 3000, n).astype(np.int16), 8000))
        lines.append("utt%d %s\n" % (i, path))
    scp = tmp_path / "wav.scp"
    scp.write_text("".join(lines))
    want = [(k, [np.asarray(w) for w in ws]) for k, ws in mfcc_vad._planned_batches(str(scp), opts, augment.Augmenter(), 25000)]
    assert len(want) >= 3
    table = extract_stream.WaveTable(str(scp), opts, vopts, 25000)
    got = list(table)
    table.close()
    assert [k for k, _, _ in got] == [k for k, _ in want] and all(v is None for _, _, v in got)
    for (keys, batch, _), (_, waves) in zip(got, want):
        assert isinstance(batch, extract_stream.WaveBatch) and batch.keys == keys and len(batch) == len(keys)
        assert batch.uniform_cols() is None and batch.addrs is None and list(batch.holders) == []
        assert all(np.array_equal(a, b) for a, b in zip(batch.waves, waves))


def test_end_to_end_audio_has_the_voiced_counts_it_is_built_for(tmp_path):
    """The constructions of tests/wav_direct_inputs.py through the fp64 restatement of MFCC + energy VAD (tests/mfcc_ref.py): the
    loud files are voiced throughout, the half-loud one in its loud half, the quiet one nowhere, the blip in fewer frames than the
    smallest chunk.  (The 16 kHz file is loud throughout; its resampling is the GPU test's.)  The route's reader admits all seven,
    the 16 kHz one as a wave that carries its rate."""
    import mfcc_ref
    import wav_direct_inputs as wdi
    from xvector_amd import extract_stream, mfcc
    opts, vopts = _options()
    opts.update([("allow_downsample", "true")])
    lines = []
    for key, rate, wave in wdi.waves():
        (tmp_path / (key + ".wav")).write_bytes(mfcc.wav_bytes(wave, rate))
        lines.append("%s %s\n" % (key, tmp_path / (key + ".wav")))
    (tmp_path / "wav.scp").write_text("".join(lines))
    table = extract_stream.WaveTable(str(tmp_path / "wav.scp"), opts, vopts)
    (keys, batch, _), = list(table)
    table.close()
    assert keys == [k for k, _, _ in wdi.waves()]
    assert [getattr(w, "rate", None) for w in batch.waves] == [None] * 6 + [16000]
    tables = mfcc.MfccTables(opts, resample=True)
    counts, frames = {}, {}
    for key, rate, wave in wdi.waves():
        if rate != wdi.FS:
            continue
        c0 = mfcc_ref.mfcc(opts, tables, wave, mfcc.dither_key(key, opts.seed))["feats"][:, 0]
        counts[key], frames[key] = int(mfcc_ref.vad(c0, vopts).sum()), len(c0)
    for key in ("loud-1s", "loud-2.5s", "loud-4s"):
        assert counts[key] == frames[key] >= 100, key
    assert frames["half-3s"] == 300 and 145 <= counts["half-3s"] <= 155
    assert counts["quiet-2s"] == 0 and frames["quiet-2s"] == 200
    assert 0 < counts["blip-2.2s"] < wdi.MIN_CHUNK
    assert sum(counts[k] >= wdi.MIN_CHUNK for k in counts) + 1 == len(wdi.EXPECTED_KEYS) >= 4
