"""Stage 2 on the host, no GPU: parsing Kaldi's wav-reverberate entries into evaluation trees, the refusals, the planning of
lengths (what wav-to-duration reports), and hand checks of the fp64 oracle (tests/augment_ref.py) against DESIGN.md §8.7."""
import os
import subprocess
import sys

import numpy as np
import pytest

import augment_ref
from conftest import TWIN
from xvector_amd import augment, mfcc

A = augment


def _wav(path, x, fs=8000):
    with open(path, "wb") as f:
        f.write(mfcc.wav_bytes(x, fs))
    return str(path)


# ------------------------------------------------------------------------------------------------
# parsing
# ------------------------------------------------------------------------------------------------
def test_split_pipeline_respects_quotes():
    cmd = "sph2pipe -f wav a.sph | wav-reverberate --impulse-response=\"sox r.wav -t wav - |\" --x='a|b' - - "
    st = A.split_pipeline(cmd)
    assert len(st) == 2 and "|".join(st) == cmd
    assert A.split_pipeline("a 'b|c' \"d|e\" f\\|g") == ["a 'b|c' \"d|e\" f\\|g"]


def test_parse_path_input_with_quoted_pipe_rir():
    n = A.parse_rx('wav-reverberate --shift-output=true --impulse-response="sox RIRS_NOISES/simulated_rirs/smallroom/Room001/'
                   'Room001-00001.wav -r 8000 -t wav - |" /d/u1.wav - |')
    assert isinstance(n, A.Reverb) and n.opts.shift_output
    assert isinstance(n.input, A.Source) and n.input.rx == "/d/u1.wav"
    assert isinstance(n.rir, A.Source) and n.rir.rx.startswith("sox RIRS_NOISES") and n.rir.rx.endswith("- |")
    assert n.noises == [] and n.opts.normalize_output and n.opts.volume == 0 and n.opts.duration == 0


def test_parse_pipe_input():
    rx = 'sph2pipe -f wav -p -c 1 /d/u2.sph | wav-reverberate --shift-output=true --impulse-response="sox r.wav -r 8000 -t wav - |" - - |'
    n = A.parse_rx(rx)
    assert n.input.rx == "sph2pipe -f wav -p -c 1 /d/u2.sph |"        # the earlier stages, byte for byte, run in the shell
    assert n.rir.rx == "sox r.wav -r 8000 -t wav - |"


def test_parse_foreground_noise():
    n = A.parse_rx("wav-reverberate --shift-output=true --additive-signals='/m/n1.wav,/m/n2.wav' --start-times='0,7.51' "
                   "--snrs='10,5' /d/u1.wav - |")
    assert [s.rx for s in n.noises] == ["/m/n1.wav", "/m/n2.wav"]
    assert n.snrs == [10.0, 5.0] and n.start_times == [0.0, float(np.float32(7.51))] and n.rir is None


def test_parse_nested_duration_noises():
    rx = ("wav-reverberate --shift-output=true --additive-signals='wav-reverberate --duration=12.3 \"/m/s1.wav\" - |,"
          "wav-reverberate --duration=12.3 \"/m/s2.wav\" - |' --start-times='0,0' --snrs='19,13' /d/u1.wav - |")
    n = A.parse_rx(rx)
    assert len(n.noises) == 2 and all(isinstance(c, A.Reverb) for c in n.noises)
    assert [c.input.rx for c in n.noises] == ["/m/s1.wav", "/m/s2.wav"]
    assert all(c.opts.duration == pytest.approx(12.3) and not c.opts.shift_output for c in n.noises)


def test_plain_entries_are_sources():
    for rx in ("/d/u1.wav", "sph2pipe -f wav -p -c 1 /d/u2.sph |", "sox a.wav -t wav - |"):
        assert isinstance(A.parse_rx(rx), A.Source) and A.parse_rx(rx).rx == rx
    assert not A.is_augmented("sox a.wav -t wav - |") and A.is_augmented("wav-reverberate a.wav - |")


@pytest.mark.parametrize("rx,msg", [
    ("wav-reverberate --additive-signals=a.wav,b.wav --snrs=1 --start-times=0,0 x.wav - |", "--snrs"),
    ("wav-reverberate --additive-signals=a.wav --snrs=1,2 --start-times=0 x.wav - |", "--snrs"),
    ("wav-reverberate --additive-signals=a.wav --snrs=1 --start-times=0,1 x.wav - |", "--start-times"),
    ("wav-reverberate --bogus=1 x.wav - |", "unknown option"),
    ("wav-reverberate --multi-channel-output=true x.wav - |", "multi-channel"),
    ("wav-reverberate x.wav - | sox -t wav - -t wav - |", "last stage"),
    ("wav-reverberate x.wav out.wav |", "output must be"),
    ("wav-reverberate - - |", "no pipeline stage"),
    ("cat y.wav | wav-reverberate x.wav - |", "earlier pipeline stages"),
    ("wav-reverberate --duration x.wav - |", "needs a value"),
    ("wav-reverberate --impulse-response='wav-reverberate a.wav - | sox - - |' x.wav - |", "last stage"),
])
def test_refusals(rx, msg):
    with pytest.raises(A.AugmentError, match=msg):
        A.parse_rx(rx)


def test_rate_mismatch_is_refused(tmp_path):
    x = _wav(tmp_path / "x.wav", np.ones(100, np.int16), 8000)
    r = _wav(tmp_path / "r.wav", np.ones(10, np.int16), 16000)
    n = _wav(tmp_path / "n.wav", np.ones(10, np.int16), 16000)
    with pytest.raises(A.AugmentError, match="k1.*impulse response's sample rate"):
        A.Augmenter().plan([("k1", A.parse_rx("wav-reverberate --impulse-response=%s %s - |" % (r, x)))])
    with pytest.raises(A.AugmentError, match="k2.*additive signal's sample rate"):
        A.Augmenter().plan([("k2", A.parse_rx("wav-reverberate --additive-signals=%s --snrs=0 --start-times=0 %s - |" % (n, x)))])


def test_plan_lengths_and_shared_decodes(tmp_path):
    x = _wav(tmp_path / "x.wav", np.arange(1000, dtype=np.int16))
    r = _wav(tmp_path / "r.wav", np.array([0, 5, 32000, 7, 32000], np.int16))
    nest = "wav-reverberate --duration=0.7 \"%s\" - |" % x
    e1 = A.parse_rx("wav-reverberate --shift-output=true --impulse-response=%s %s - |" % (r, x))
    e2 = A.parse_rx("wav-reverberate --duration=2.5 --additive-signals='%s' --snrs=3 --start-times=0 %s - |" % (nest, x))
    e3 = A.parse_rx("wav-reverberate --additive-signals='%s,%s' --snrs=3,4 --start-times=0,1 %s - |" % (nest, nest, x))
    plan = A.Augmenter().plan([("a", e1), ("b", e2), ("c", e3)])
    assert plan.lengths() == [1000, 20000, 1000] and plan.rates() == [8000, 8000, 8000]
    assert plan.top[0].shift == 2                                     # the first maximum
    assert len(plan.decoded) == 2                                     # x.wav and r.wav decoded once
    assert len(plan.nodes) == 4                                       # the nested evaluation once for the batch
    assert plan.top[1].level == 1 and plan.top[0].level == 0
    assert A.duration_samples("a", "%s" % x) == (1000, 8000)


def test_wav_to_duration_cli(tmp_path):
    x = _wav(tmp_path / "x.wav", np.arange(1234, dtype=np.int16))
    scp = tmp_path / "wav.scp"
    scp.write_text("a %s\nb wav-reverberate --duration=1.5 %s - |\nc wav-reverberate --impulse-response=%s %s - |\n" % (x, x, x, x))
    subprocess.run([sys.executable, os.path.join(TWIN, "mfcc_vad.py"), "wav-to-duration", "scp:%s" % scp,
                    "ark,t:%s" % (tmp_path / "d")], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    got = [l.split() for l in open(tmp_path / "d")]
    assert [k for k, _ in got] == ["a", "b", "c"]
    assert [float(v) for _, v in got] == pytest.approx([1234 / 8000.0, 1.5, 1234 / 8000.0])


# ------------------------------------------------------------------------------------------------
# the oracle by hand
# ------------------------------------------------------------------------------------------------
def test_identity_rir_reproduces_x():
    # [32768] in int16 units is h = [1.0] (the oracle takes the RIR in any integer type; a WAV cannot hold it)
    x = np.array([3, -7, 100, 12345, -32768, 0, 5], np.int16)
    r = augment_ref.reverberate(x, 8000, rir=np.array([32768], np.int64))
    assert (r["out"] == x).all() and r["shift"] == 0 and r["level"] == 1.0
    assert r["E"] == r["P0"] == r["P1"]


def test_delayed_delta_with_and_without_shift():
    x = np.array([1000, -2000, 3000, 4000], np.int16)
    h = np.zeros(6, np.int16)
    h[3] = 16384                                                       # 0.5, three samples late
    a = augment_ref.reverberate(x, 8000, rir=h, volume=2.0)
    assert (a["out"] == np.array([0, 0, 0, 1000], np.int16)).all()     # M = N samples from the start of y
    b = augment_ref.reverberate(x, 8000, rir=h, volume=2.0, shift_output=True)
    assert b["shift"] == 3 and (b["out"] == x).all()


def test_duration_repeat():
    x = np.array([1, 2, 3], np.int16)
    r = augment_ref.reverberate(x, 10, duration=0.8)
    assert (r["out"] == np.array([1, 2, 3, 1, 2, 3, 1, 2], np.int16)).all()
    r = augment_ref.reverberate(x, 10, duration=0.2)
    assert (r["out"] == np.array([1, 2], np.int16)).all()


def test_offset_truncation():
    x = np.full(10, 100, np.int16)
    n = np.full(4, 50, np.int16)
    # fp32(0.7) * fp32(10) rounds to 7.0 exactly in fp32: offset 7, the noise cut at the end of y, no wrap
    assert int(np.float32(0.7) * np.float32(10)) == 7
    r = augment_ref.reverberate(x, 10, noises=[n], snrs=[0.0], start_times=[0.7], normalize_output=False)
    s = r["noise_scale"][0]
    assert s == pytest.approx(2.0)
    assert (r["out"] == np.array([100] * 7 + [200] * 3, np.int16)).all()


def test_early_window_fp32_edge_at_16k():
    # fp32(0.001) * 16000 rounds to exactly 16.0f: peak 17 gives start 1, peak 16 gives 0 (the exact product would give 0
    # for peak 17); fp32(0.05) * 16000 = 800.0f
    assert augment_ref.window(17, 100000, 16000) == A.early_window(17, 100000, 16000.0) == (1, 817)
    assert augment_ref.window(16, 100000, 16000) == (0, 816)
    assert augment_ref.window(3, 50, 16000) == (0, 50)
    # at 8 kHz fp32(0.001) * 8000 = 8.0f
    assert A.early_window(20, 10000, 8000.0) == (12, 420)


def test_truncation_and_saturation():
    # through the oracle's own write step: volume 2 puts samples exactly on +32768 (clipped to 32767), -32768 (kept) and -32770
    # (clipped); volume 0.5 puts them on +-0.5 and +-1.5, which truncate toward zero
    r = augment_ref.reverberate(np.array([16384, -16384, -16385, 16383, 3], np.int16), 8000, volume=2.0)
    assert list(r["pre"]) == [32768.0, -32768.0, -32770.0, 32766.0, 6.0]
    assert (r["out"] == np.array([32767, -32768, -32768, 32766, 6], np.int16)).all() and r["clipped"] == 2
    r = augment_ref.reverberate(np.array([1, -1, 3, -3, 32767], np.int16), 8000, volume=0.5)
    assert list(r["pre"]) == [0.5, -0.5, 1.5, -1.5, 16383.5]
    assert (r["out"] == np.array([0, 0, 1, -1, 16383], np.int16)).all() and r["clipped"] == 0
    big = augment_ref.reverberate(np.array([30000, -30000, 100], np.int16), 8000, volume=1.2)
    assert (big["out"] == np.array([32767, -32768, 120], np.int16)).all() and big["clipped"] == 2


def test_batches_keep_the_plan_each_entry_was_planned_into(tmp_path):
    """The reader plans an entry before the batcher knows which batch takes it (the entry that overflows a batch is read before
    the batch is yielded): every augmented entry must come with the plan that holds its node and decoded sources, also when the
    last batch is that one overflowed entry."""
    import mfcc_vad
    rir = _wav(tmp_path / "rir.wav", np.array([0, 100, 32000, -500, 20], np.int16))
    lines = []
    for i in range(3):
        x = _wav(tmp_path / ("u%d.wav" % i), (np.arange(1000) % 50).astype(np.int16))
        lines.append("u%d-reverb wav-reverberate --shift-output=true --impulse-response=%s %s - |\n" % (i, rir, x))
    scp = tmp_path / "wav.scp"
    scp.write_text("".join(lines))
    opts = mfcc.MfccOptions(sample_frequency=8000)
    aug = A.Augmenter()
    batches = list(mfcc_vad._planned_batches(str(scp), opts, aug, 2000))
    assert [k for k, _ in batches] == [["u0-reverb", "u1-reverb"], ["u2-reverb"]]
    items = [w for _, ws in batches for w in ws]
    assert all(isinstance(w, A.Pending) and w.plan is not None and any(w.node is n for n in w.plan.top) for w in items)
    for w in items:                                   # what the device path does first with an entry's RIR: no GPU needed
        assert aug._rir(w.plan, w.node.rir).peak == 2
    assert items[0].plan is items[1].plan
