"""The segmentation of DESIGN.md §8.18 without a GPU: the NumPy twin against the per-frame loop (tests/segment_ref.py), the
options' refusals, the segments-file arithmetic, the ``vad-to-segments`` command and the new usage errors of extract_embedding.py."""
import os

import numpy as np
import pytest

import segment_ref

PARAMS = [(30, 50, 10, 1000), (30, 50, 10, 100), (0, 1, 0, 0), (0, 1, 0, 2), (7, 3, 3, 6), (5, 20, 2, 0), (2, 4, 1, 9)]     # (G, M, P, L)


def _twin(v, G, M, P, L):
    from xvector_amd import segment
    tab = segment.vad_segments_host(v, segment.SegmentOptions(G, M, P, L).check())
    assert tab.dtype == np.int32 and tab.ndim == 2 and tab.shape[1] == 2
    return [tuple(r) for r in tab.tolist()]


def _random_params(rng, i):
    M = int(rng.integers(1, 40))
    G = int(rng.integers(0, 40))
    P = int(rng.integers(0, G // 2 + 1))
    L = 0 if i % 3 == 0 else int(rng.integers(2 * M, 2 * M + 120))
    return G, M, P, L


def test_twin_equals_the_loop_on_random_bursty_inputs():
    rng = np.random.default_rng(818)
    n_split = n_closed = n_dropped = 0
    for i in range(2000):
        G, M, P, L = _random_params(rng, i)
        T = int(rng.integers(0, 401))
        v = segment_ref.bursty(rng, T, int(rng.integers(1, 80)), int(rng.integers(1, 60)))
        want = segment_ref.segments(v, G, M, P, L)
        assert _twin(v, G, M, P, L) == want, (i, G, M, P, L, v.tolist())
        segment_ref.check_properties(want, T, G, M, L)
        n_split += any(L and n < L and a + n == b for (a, n), (b, _) in zip(want, want[1:]))
        idx = np.flatnonzero(v)
        gaps = np.diff(idx) - 1
        n_closed += bool(((gaps > 0) & (gaps <= G)).any())
        n_dropped += len(want) == 0 and len(idx) > 0
    assert n_split > 50 and n_closed > 500 and n_dropped > 50          # the inputs reach every step of the rule


@pytest.mark.parametrize("params", PARAMS)
def test_twin_equals_the_loop_on_the_hand_cases(params):
    G, M, P, L = params
    for name, v in segment_ref.hand_cases(G, M, P, L):
        want = segment_ref.segments(v, G, M, P, L)
        assert _twin(v, G, M, P, L) == want, name
        segment_ref.check_properties(want, len(v), G, M, L)


def test_hand_cases_mean_what_their_names_say():
    G, M, P, L = 30, 50, 10, 100
    got = {name: segment_ref.segments(v, G, M, P, L) for name, v in segment_ref.hand_cases(G, M, P, L)}
    assert got["gap of exactly G"] == [(0, 65), (65, 65)]                  # one run of 130 frames, split evenly
    assert got["gap of G + 1"] == [(0, 60), (71, 60)]                      # two runs, padded towards each other, not touching
    assert got["run of M - 1"] == [] and got["run of M"] == [(0, 60)]
    assert got["unclosed gap at frame 0"] == [(20, 60)] and got["unclosed gap at T"] == [(0, 60)]
    assert got["all voiced"] == [(0, 75), (75, 76)] and got["all unvoiced"] == [] and got["T = 0"] == []
    assert got["padding clipped at 0"] == [(0, 69)] and got["padding clipped at T"] == [(3, 69)]
    assert got["a NaN decision"] == [(0, 58)]
    assert got["whole utterance of n = 100"] == [(0, 100)] and got["whole utterance of n = 101"] == [(0, 50), (50, 51)]
    assert got["whole utterance of n = 200"] == [(0, 100), (100, 100)]
    assert got["whole utterance of n = 201"] == [(0, 67), (67, 67), (134, 67)]


def test_capacity_host_function_and_abi():
    from xvector_amd import hiplib, segment
    new = {"xv_vad_segments_i32", "xv_vad_segments_workspace_bytes", "xv_vad_segments_capacity"}
    assert hiplib.ABI_VERSION >= 44 and new <= set(hiplib.SYMBOLS) and hiplib.SEG_TILE == 256
    rng = np.random.default_rng(5)
    for i in range(300):
        G, M, P, L = _random_params(rng, i)
        T = int(rng.integers(0, 200000))
        assert hiplib.vad_segments_capacity(T, G, M, L) == segment_ref.capacity(T, G, M, L) == segment.SegmentOptions(G, M, P, L).capacity(T)
    for bad in ((-1, 0, 1, 0), (10, -1, 1, 0), (10, 0, 0, 0), (10, 0, 5, 9), (10, 0, 5, -1)):
        with pytest.raises(ValueError):
            hiplib.vad_segments_capacity(*bad)
    assert hiplib.vad_segments_workspace_bytes(100000) >= 0


def test_segment_options_refusals():
    from xvector_amd.segment import SegmentOptions
    o = SegmentOptions()
    assert (o.max_gap, o.min_len, o.pad, o.max_len) == (30, 50, 10, 1000) and o.check() is o
    for ok in ((0, 1, 0, 0), (30, 50, 15, 100), (1, 1, 0, 2)):
        SegmentOptions(*ok).check()
    for bad, word in (((-1, 50, 0, 0), "max_gap"), ((30, 0, 10, 0), "min_len"), ((30, 50, -1, 0), "pad"), ((30, 50, 16, 0), "pad"),
                      ((30, 50, 10, 99), "max_len"), ((30, 50, 10, -5), "max_len")):
        with pytest.raises(ValueError) as e:
            SegmentOptions(*bad).check()
        assert word in str(e.value)


def test_frames_of_segments():
    from xvector_amd.segment import frames_of_segments
    T_of = {"r1": 1000, "r2": 300}
    lines = [("b", "r1", 1004, 2996),          # 100.4 -> 100, 299.6 -> 300
             ("a", "r1", 5, 995),              # 0.5 -> 1 (half rounds up), 99.5 -> 100: touches b, does not overlap
             ("c", "r1", 9000, 20000),         # clipped to T
             ("late", "r1", 10000, 11000),     # first >= T: skipped
             ("thin", "r1", 5001, 5003),       # end <= first after rounding: skipped
             ("x", "nobody", 0, 1000),         # unknown recording
             ("d", "r2", 0, 2996)]             # clipped to r2's T
    per, n_empty, n_unknown = frames_of_segments(lines, T_of, 10.0)
    assert (n_empty, n_unknown) == (2, 1) and sorted(per) == ["r1", "r2"]
    ids, tab = per["r1"]
    assert ids == ["a", "b", "c"] and tab.dtype == np.int32 and tab.tolist() == [[1, 99], [100, 200], [900, 100]]
    assert per["r2"][0] == ["d"] and per["r2"][1].tolist() == [[0, 300]]
    per, _, _ = frames_of_segments([("s", "r2", 125, 375)], T_of, 12.5)          # another frame shift: 10 -> 30
    assert per["r2"][1].tolist() == [[10, 20]]
    with pytest.raises(ValueError) as e:
        frames_of_segments([("p", "r1", 0, 1000), ("q", "r1", 990, 2000)], T_of, 10.0)
    assert "p" in str(e.value) and "q" in str(e.value)
    assert frames_of_segments([], T_of, 10.0) == ({}, 0, 0)


def test_read_segments_refusals_stand(tmp_path):
    import plda_backend
    f = tmp_path / "segments"
    f.write_text("s1 r1 2.0 1.0\n")
    with pytest.raises(SystemExit):
        plda_backend.read_segments(str(f))


def test_vad_to_segments_cli(tmp_path, monkeypatch):
    import kaldi_io
    import mfcc_vad
    G, M, P, L = 3, 4, 1, 12
    vads = [("recA", np.array([0, 1, 1, 1, 0, 0, 1, 1, 0, 0, 0, 0, 1, 0, 0], np.float32)),      # [1, 8) closed and padded; [12, 13) dropped
            ("recB", np.zeros(9, np.float32)),                                                  # no segment
            ("recC", np.ones(25, np.float32))]                                                  # split into 3
    ark = str(tmp_path / "vad.ark")
    with kaldi_io.TableWriter(ark, str(tmp_path / "vad.scp")) as fd:
        for k, v in vads:
            kaldi_io.write_vec_flt(fd, v, key=k)
    out = tmp_path / "segments"
    seen = {}
    real_rename = os.rename

    def rename(src, dst):
        seen[dst] = (src, os.path.exists(src), os.path.exists(dst))
        real_rename(src, dst)
    monkeypatch.setattr(os, "rename", rename)
    argv = ["vad-to-segments", "--max-gap", str(G), "--min-segment-length", str(M), "--pad", str(P), "--max-segment-length", str(L)]
    assert mfcc_vad.main(argv + ["scp:%s" % (tmp_path / "vad.scp"), str(out)]) == 0
    monkeypatch.undo()
    assert seen[str(out)] == (str(out) + ".tmp", True, False) and not os.path.exists(str(out) + ".tmp")
    assert out.read_text() == ("recA-00000000-00000009 recA 0.000 0.090\n"
                               "recC-00000000-00000008 recC 0.000 0.080\n"
                               "recC-00000008-00000016 recC 0.080 0.160\n"
                               "recC-00000016-00000025 recC 0.160 0.250\n")
    for k, v in vads:
        assert _twin(v, G, M, P, L) == segment_ref.segments(v, G, M, P, L)
    import plda_backend
    assert [(k, r) for k, r, _, _ in plda_backend.read_segments(str(out))][0] == ("recA-00000000-00000009", "recA")
    # the ark form, another frame shift, and a refused option set (exit through SystemExit with a message, nothing written)
    assert mfcc_vad.main(argv + ["--frame-shift", "12.5", "ark:" + ark, str(tmp_path / "s2")]) == 0
    assert (tmp_path / "s2").read_text().splitlines()[0] == "recA-00000000-00000009 recA 0.000 0.113"
    with pytest.raises(SystemExit) as e:
        mfcc_vad.main(["vad-to-segments", "--max-gap", "3", "--pad", "2", "ark:" + ark, str(tmp_path / "s3")])
    assert "pad" in str(e.value) and not os.path.exists(str(tmp_path / "s3")) and not os.path.exists(str(tmp_path / "s3.tmp"))


# ---- the command line of extract_embedding.py ------------------------------------------------------------------------------------
WAV = ["--vector-wspecifier", "ark,scp:/nonexistent/x.ark,/nonexistent/x.scp", "--model-dir", "/nonexistent/model",
       "--wav-rspecifier", "scp:/nonexistent/wav.scp", "--cmn-window", "300"]
TABLE = ["--vector-wspecifier", "ark,scp:/nonexistent/x.ark,/nonexistent/x.scp", "--model-dir", "/nonexistent/model",
         "--feature-rspecifier", "scp:/nonexistent/feats.scp"]


@pytest.mark.parametrize("argv, words", [
    (TABLE + ["--segment-by-vad"], ("--wav-rspecifier",)),
    (TABLE + ["--segments", "/nonexistent/segments"], ("--wav-rspecifier",)),
    (TABLE + ["--segment-max-gap", "20"], ("--wav-rspecifier",)),
    (TABLE + ["--vad-rspecifier", "scp:/nonexistent/vad.scp", "--cmn-window", "300", "--segment-pad", "5"], ("--wav-rspecifier",)),
    (WAV + ["--segment-by-vad", "--segments", "/nonexistent/segments"], ("--segments", "--segment-by-vad")),
    (WAV + ["--segment-max-gap", "20"], ("--segment-max-gap", "--segment-by-vad")),
    (WAV + ["--segment-pad", "5"], ("--segment-pad", "--segment-by-vad")),
    (WAV + ["--segment-max-length", "500"], ("--segment-max-length", "--segment-by-vad")),
    (WAV + ["--segments", "/nonexistent/segments", "--segment-max-length", "500"], ("--segment-max-length", "--segment-by-vad")),
    (WAV + ["--segment-by-vad", "--segment-max-gap", "-1"], ("max_gap",)),
    (WAV + ["--segment-by-vad", "--segment-pad", "16"], ("pad",)),
    (WAV + ["--segment-by-vad", "--segment-max-gap", "10"], ("pad",)),                       # the default pad of 10 needs a gap of 20
    (WAV + ["--segment-by-vad", "--segment-max-length", "150"], ("max_len",)),               # below twice --min-chunk-size (100)
    (WAV + ["--segment-by-vad", "--min-chunk-size", "0"], ("min_len",)),
])
def test_usage_errors_exit_2_before_the_model_directory_is_touched(argv, words, capsys, monkeypatch):
    import extract_embedding as ee
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        ee.get_args(argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert all(w in err for w in words), err


def test_accepted_command_lines(tmp_path, monkeypatch):
    import extract_embedding as ee
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    # a valid segmented command line gets past the usage checks: what stops it is the model directory (an Exception, not exit 2)
    with pytest.raises(Exception) as e:
        ee.get_args(WAV + ["--segment-by-vad"])
    assert not isinstance(e.value, SystemExit) and "/nonexistent/model" in str(e.value)
    (tmp_path / "model.meta").write_text("{}")
    common = ["--vector-wspecifier", "ark:x", "--model-dir", str(tmp_path), "--wav-rspecifier", "scp:wav.scp", "--cmn-window", "300"]
    a = ee.get_args(common)                                                                   # nothing given: today's behaviour
    assert (a.segment_by_vad, a.segments) == (False, "")
    a = ee.get_args(common + ["--segment-by-vad"])
    assert (a.segment_by_vad, a.segment_max_gap, a.segment_pad, a.segment_max_length) == (True, 30, 10, 1000)
    a = ee.get_args(common + ["--segment-by-vad", "--segment-max-gap", "50", "--segment-pad", "25", "--segment-max-length", "0",
                              "--window", "150", "--period", "75", "--subsegments-file", "S"])
    assert (a.segment_max_gap, a.segment_pad, a.segment_max_length, a.window) == (50, 25, 0, 150)
    a = ee.get_args(common + ["--segments", "/nonexistent/segments"])                         # the file is not read here
    assert a.segments == "/nonexistent/segments" and not a.segment_by_vad
