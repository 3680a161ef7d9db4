"""The wav.scp -> x-vector route on the MI355X: Extractor.submit_device_raw against Extractor.submit_raw on
the same values, and extract_embedding.py --wav-rspecifier against compute-mfcc-vad + extract_embedding.py on the same audio.
Both routes run the same kernels on the same values, so every comparison is equality of bits / bytes."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

TS = [300, 40, 1, 0, 777, 25, 1300, 90, 260, 33]


@pytest.fixture(scope="module")
def window():
    """The utterances of test_device_front_end_path_equals_host_round_trip with a complete VAD vector each (one of them all
    zero), as host arrays and as the device tensors the direct route takes."""
    import torch
    from xvector_amd import hiplib
    hiplib.require_gpu()
    rng = np.random.default_rng(12)
    mats = [(rng.standard_normal((t, 23)) * 3 + 1.5).astype(np.float32) for t in TS]
    vads = [(rng.random(t) < 0.7).astype(np.float32) for t in TS]
    vads[1] = np.zeros(40, np.float32)              # nothing voiced -> dropped
    T = np.array(TS, np.int64)
    row0 = np.zeros(len(TS), np.int64)
    np.cumsum(T[:-1], out=row0[1:])

    def device(ms):
        return torch.from_numpy(np.concatenate(ms)).cuda()
    return dict(mats=mats, vads=vads, T=T, row0=row0, device=device, vad_d=torch.from_numpy(np.concatenate(vads)).cuda())


def _same(got, want, n):
    (g_vecs, g_lens, g_drop), (w_vecs, w_lens, w_drop) = got, want
    assert np.array_equal(g_lens, w_lens) and np.array_equal(g_drop, w_drop)
    assert len(g_vecs) == len(w_vecs) == n
    for a, b in zip(g_vecs, w_vecs):
        assert (a is None) == (b is None) and (a is None or np.array_equal(a, b))


@pytest.mark.parametrize("host_lib", [True, False])
def test_submit_device_raw_equals_submit_raw_bit_for_bit(window, monkeypatch, host_lib):
    """Chunking, small batches that split utterances, a VAD that drops an utterance, and a window without VAD; the same again
    with libxvector_host.so out of reach of the direct route (it calls nothing of it)."""
    from xvector_amd import engine, synthetic, topology
    if engine._host_lib() is None:
        pytest.skip("libxvector_host.so disabled: no submit_raw to compare with")
    topo = topology.get("ModelWithoutDropout")
    model = engine.DeviceModel(synthetic.trained_like(topo, 23, seed=3), topo, "cuda:0")
    w = window
    feats = w["device"](w["mats"])
    for with_vad, (mn, cs, rows) in ((True, (25, 200, 262144)), (True, (10, -1, 512)), (True, (25, 10000, 262144)), (False, (25, 300, 700))):
        ex = engine.Extractor(model, mn, cs, max_batch_rows=rows)
        handle, lens, dropped = ex.submit_raw(w["mats"], w["vads"] if with_vad else None, 300, True)
        want = (ex.finish(handle), lens, dropped)
        assert sum(v is not None for v in want[0]) >= 4
        ex2 = engine.Extractor(model, mn, cs, max_batch_rows=rows)
        with monkeypatch.context() as mp:
            if not host_lib:
                mp.setattr(engine, "_host_lib", lambda: None)
            handle, lens, dropped = ex2.submit_device_raw(feats, w["row0"], w["T"], w["vad_d"] if with_vad else None, 300, True)
            got = (ex2.finish(handle), lens, dropped)
        _same(got, want, len(TS))
        assert ex2.stats == ex.stats, (mn, cs, rows)          # the same batches, chunks, frames and rows
        assert dropped[1] == with_vad and (not with_vad or lens[1] == 0)


def test_device_route_redo_and_demotion_equal_bf16x3(window, monkeypatch):
    """Cases (b) and (c) of test_device_front_end_redo_and_demotion_equal_bf16x3 through submit_device_raw: a window with one
    utterance scaled by 1e6 raises the status word and is repeated on the bf16x3 twin from the same device tensors; a failed
    run-time probe demotes the extractor and the next window is routed to the twin.  Each equals submit_raw on a bf16x3 model."""
    from xvector_amd import engine, synthetic, topology
    if engine._host_lib() is None:
        pytest.skip("libxvector_host.so disabled: no submit_raw to compare with")
    topo = topology.get("ModelWithoutDropout")
    wts = synthetic.trained_like(topo, 23, seed=3)
    w = window
    loud = list(w["mats"])
    loud[6] = w["mats"][6] * np.float32(1e6)
    fast = engine.DeviceModel(wts, topo, "cuda:0", precision="f16bf8")
    exact = engine.DeviceModel(wts, topo, "cuda:0", precision="bf16x3")
    d_mats, d_loud = w["device"](w["mats"]), w["device"](loud)

    def ref_run(ex, ms):
        handle, lens, dropped = ex.submit_raw(ms, w["vads"], 300, True)
        return ex.finish(handle), lens, dropped

    def run(ex, feats):
        handle, lens, dropped = ex.submit_device_raw(feats, w["row0"], w["T"], w["vad_d"], 300, True)
        return (ex.finish(handle), lens, dropped), handle

    for rows in (262144, 700):
        ref_ex = engine.Extractor(exact, 25, 200, max_batch_rows=rows)
        ref, ref_loud = ref_run(ref_ex, w["mats"]), ref_run(ref_ex, loud)
        frames = ref_ex.stats["frames"] // 2
        # (b) out of range: the status word alone (no probe) has the window repeated on the twin
        ex = engine.Extractor(fast, 25, 200, max_batch_rows=rows, accuracy_probe=False)
        got, _ = run(ex, d_loud)
        assert ex.stats["fallback_windows"] == 1 and not ex.demoted
        _same(got, ref_loud, len(TS))
        # (c) demotion: the probed window is repeated, the next one is routed
        with monkeypatch.context() as mp:
            mp.setattr(engine, "DATA_PROBE_LIMIT", 0.0)
            ex = engine.Extractor(fast, 25, 200, max_batch_rows=rows)
            before, _ = run(ex, d_mats)
            assert ex.demoted and ex.stats["fallback_windows"] == 1 and ex.stats["frames"] == frames
            _same(before, ref, len(TS))
            after, handle = run(ex, d_mats)
            assert handle.get("owner") is ex._fallback_ex and handle.get("owner") is not None
            _same(after, ref, len(TS))
            assert ex.stats["fallback_windows"] == 1 and ex.stats["frames"] == 2 * frames


# ---------------------------------------------------------------------------------------------------------------------------------
# end to end: extract_embedding.py --wav-rspecifier against compute-mfcc-vad + extract_embedding.py
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_model(tmp_path_factory):
    import models
    from xvector_amd import synthetic
    topo = synthetic.SMALL_TOPOLOGY
    mdir = str(tmp_path_factory.mktemp("nnet"))
    models.Model.save_model(dict(weights=synthetic.trained_like(topo, 23, num_classes=8, seed=12), topology=topo, model_class="Model",
                                 num_classes=8, feat_dim=23), mdir, None)
    return mdir


def _configs(d):
    """The recipe's option files; the MFCC one also admits the 16 kHz entry."""
    conf = d / "mfcc.conf"
    conf.write_text(open(os.path.join(GOLDEN, "mfcc.conf")).read() + "--allow-downsample=true\n")
    return str(conf), os.path.join(GOLDEN, "vad.conf")


def _two_step(d, scp, conf, vconf, mdir, mn, cs):
    """Route A: plain float tables on disk, then the extractor's table mode.  -> (ark bytes, scp keys)."""
    import extract_embedding as ee
    import mfcc_vad
    a = d / "A"
    a.mkdir()
    assert mfcc_vad.main(["compute-mfcc-vad", "--config", conf, "--vad-config", vconf, "scp:%s" % scp,
                          "ark,scp:%s,%s" % (a / "feats.ark", a / "feats.scp"), "ark,scp:%s,%s" % (a / "vad.ark", a / "vad.scp")]) == 0
    ee.main(["--min-chunk-size", str(mn), "--chunk-size", str(cs), "--feature-rspecifier", "scp:%s" % (a / "feats.scp"),
             "--vad-rspecifier", "scp:%s" % (a / "vad.scp"), "--cmn-window", "300",
             "--vector-wspecifier", "ark,scp:%s,%s" % (a / "xvector.ark", a / "xvector.scp"), "--model-dir", mdir])
    return (a / "xvector.ark").read_bytes(), [ln.split()[0] for ln in open(a / "xvector.scp")]


def _direct(d, scp, conf, vconf, mdir, mn, cs):
    """Route B: the same wav.scp straight into the extractor.  -> (ark bytes, scp keys, files the route left behind)."""
    import extract_embedding as ee
    b = d / "B"
    b.mkdir()
    ee.main(["--min-chunk-size", str(mn), "--chunk-size", str(cs), "--wav-rspecifier", "scp:%s" % scp, "--mfcc-config", conf,
             "--vad-config", vconf, "--cmn-window", "300",
             "--vector-wspecifier", "ark,scp:%s,%s" % (b / "xvector.ark", b / "xvector.scp"), "--model-dir", mdir])
    return (b / "xvector.ark").read_bytes(), [ln.split()[0] for ln in open(b / "xvector.scp")], sorted(os.listdir(b))


@pytest.mark.parametrize("precision,budget", [(None, None), ("bf16x3", 40000)])
def test_wav_route_writes_the_bytes_of_the_two_step_route(small_model, tmp_path, monkeypatch, precision, budget):
    """Seven WAV files (tests/wav_direct_inputs.py): four loud or half-loud ones and a 16 kHz one give vectors, the quiet one is
    dropped for its VAD, the blip rejected for its length.  Once in the default arithmetic with one window, once in bf16x3 with a
    window budget that cuts the table into at least three windows."""
    import extract_embedding as ee
    import mfcc_vad
    import wav_direct_inputs as wdi
    from xvector_amd import augment, mfcc
    lines = []
    for key, rate, wave in wdi.waves():
        (tmp_path / (key + ".wav")).write_bytes(mfcc.wav_bytes(wave, rate))
        lines.append("%s %s\n" % (key, tmp_path / (key + ".wav")))
    scp = tmp_path / "wav.scp"
    scp.write_text("".join(lines))
    conf, vconf = _configs(tmp_path)
    if precision:
        monkeypatch.setenv("XVECTOR_PRECISION", precision)
    if budget:
        monkeypatch.setattr(ee, "WAV_WINDOW_SAMPLES", budget)
        opts = mfcc.MfccOptions().update(mfcc.read_config(conf))
        assert len(list(mfcc_vad._planned_batches(str(scp), opts, augment.Augmenter(), budget))) >= 3
    ark_a, keys_a = _two_step(tmp_path, scp, conf, vconf, small_model, wdi.MIN_CHUNK, 100)
    ark_b, keys_b, left = _direct(tmp_path, scp, conf, vconf, small_model, wdi.MIN_CHUNK, 100)
    assert keys_a == wdi.EXPECTED_KEYS and len(keys_a) >= 4
    assert keys_b == keys_a
    assert len(ark_a) > 0 and ark_b == ark_a
    assert left == ["xvector.ark", "xvector.scp"]             # no feature or VAD table anywhere


def test_reverberated_and_sphere_entries_equal_the_two_step_route(small_model, tmp_path):
    """A wav-reverberate entry (the samples are made on the GPU inside the MFCC engine's buffer), an sph2pipe entry (decoded
    there) and a plain one, through both routes."""
    import sphere_ref
    from test_gpu_augment import rir_like
    from xvector_amd import mfcc, synthetic
    sp = lambda n, seed: synthetic.speech_like_wave(n, 8000, seed)  # noqa: E731
    (tmp_path / "x.wav").write_bytes(mfcc.wav_bytes(sp(20000, 50), 8000))
    (tmp_path / "rir.wav").write_bytes(mfcc.wav_bytes(rir_like(2500, 9), 8000))
    (tmp_path / "p.wav").write_bytes(mfcc.wav_bytes(sp(16000, 4), 8000))
    codes = np.stack([sphere_ref.lin2ulaw(sp(18000, 1)), sphere_ref.lin2ulaw(sp(18000, 2))])
    (tmp_path / "conv.sph").write_bytes(sphere_ref.sph_bytes(codes, 8000, "ulaw"))
    scp = tmp_path / "wav.scp"
    scp.write_text("u0-reverb wav-reverberate --shift-output=true --impulse-response=%s %s - |\n" % (tmp_path / "rir.wav", tmp_path / "x.wav")
                   + "u1-conv-B sph2pipe -f wav -p -c 2 %s |\n" % (tmp_path / "conv.sph")
                   + "u2-plain %s\n" % (tmp_path / "p.wav"))
    conf, vconf = _configs(tmp_path)
    ark_a, keys_a = _two_step(tmp_path, scp, conf, vconf, small_model, 10, 100)
    ark_b, keys_b, _ = _direct(tmp_path, scp, conf, vconf, small_model, 10, 100)
    assert keys_a == ["u0-reverb", "u1-conv-B", "u2-plain"]
    assert keys_b == keys_a and ark_b == ark_a and len(ark_a) > 0
