"""Extraction inside segments on the MI355X: extract_embedding.py --wav-rspecifier with --segment-by-vad (the
segments made on the device) against --segments (the file mfcc_vad.py vad-to-segments writes from the VAD table of
compute-mfcc-vad) and against the table route over the segments' rows cut out of the feature table."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FS = 8000
G, M, P, L = 30, 50, 10, 1000                     # the defaults of the command line; M is --min-chunk-size
WINDOW, PERIOD = 150, 75
# (kind, seconds[, seed]): bursts of synthetic.speech_like_wave (which pause inside, too) separated by zeros
RECORDINGS = {
    "recA": [("b", 2.6, 11), ("z", 0.22), ("b", 1.9, 12), ("z", 0.9), ("b", 0.25, 13), ("z", 0.7), ("b", 1.6, 14)],
    "recB": [("z", 0.3), ("b", 1.2, 21), ("z", 0.15), ("b", 1.4, 22), ("z", 0.25), ("b", 1.1, 23), ("z", 1.2), ("b", 0.3, 24), ("z", 0.6),
             ("b", 2.2, 25), ("z", 0.2)],
}


@pytest.fixture(scope="module")
def small_model(tmp_path_factory):
    import models
    from xvector_amd import synthetic
    topo = synthetic.SMALL_TOPOLOGY
    mdir = str(tmp_path_factory.mktemp("nnet"))
    models.Model.save_model(dict(weights=synthetic.trained_like(topo, 23, num_classes=8, seed=12), topology=topo, model_class="Model",
                                 num_classes=8, feat_dim=23), mdir, None)
    return mdir


def _extract(argv):
    import extract_embedding as ee
    ee.main(["--min-chunk-size", str(M), "--chunk-size", "100", "--cmn-window", "300"] + argv)


def _vectors(ark):
    import kaldi_io
    return [(k, np.asarray(v)) for k, v in kaldi_io.read_vec_flt_ark(str(ark))]


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """The two recordings, their compute-mfcc-vad tables, the segments file of vad-to-segments, and the checks that the
    segmentation is not a trivial one."""
    import kaldi_io
    import mfcc_vad
    import plda_backend
    from xvector_amd import hiplib, mfcc, segment, synthetic
    hiplib.require_gpu()
    d = tmp_path_factory.mktemp("segment_extract")
    lines = []
    for key, parts in RECORDINGS.items():
        wave = np.concatenate([synthetic.speech_like_wave(int(p[1] * FS), FS, p[2], level_db=(-14.0, -8.0)) if p[0] == "b"
                               else np.zeros(int(p[1] * FS), np.int16) for p in parts])
        (d / (key + ".wav")).write_bytes(mfcc.wav_bytes(wave, FS))
        lines.append("%s %s\n" % (key, d / (key + ".wav")))
    scp = d / "wav.scp"
    scp.write_text("".join(lines))
    conf, vconf = os.path.join(GOLDEN, "mfcc.conf"), os.path.join(GOLDEN, "vad.conf")
    assert mfcc_vad.main(["compute-mfcc-vad", "--config", conf, "--vad-config", vconf, "scp:%s" % scp,
                          "ark,scp:%s,%s" % (d / "feats.ark", d / "feats.scp"), "ark,scp:%s,%s" % (d / "vad.ark", d / "vad.scp")]) == 0
    assert mfcc_vad.main(["vad-to-segments", "--max-gap", str(G), "--min-segment-length", str(M), "--pad", str(P),
                          "--max-segment-length", str(L), "scp:%s" % (d / "vad.scp"), str(d / "segments")]) == 0
    vads = {k: np.asarray(v) for k, v in kaldi_io.read_vec_flt_scp(str(d / "vad.scp"))}
    segs = {}
    for key, v in vads.items():
        tab = segment.vad_segments_host(v, segment.SegmentOptions(G, M, P, L))
        segs[key] = [(a, a + n) for a, n in tab.tolist()]
        idx = np.flatnonzero(v != 0)
        gaps = np.diff(idx) - 1
        ends = np.flatnonzero(gaps > G)                                       # the closed runs, from the voiced frames
        a, b = idx[np.concatenate([[0], ends + 1])], idx[np.concatenate([ends, [len(idx) - 1]])] + 1
        assert len(tab) >= 2 and ((gaps > 0) & (gaps <= G)).any() and (b - a < M).any(), (key, tab.tolist())
    file_segs = plda_backend.read_segments(str(d / "segments"))
    assert [(k, r) for k, r, _, _ in file_segs] == [("%s-%08d-%08d" % (r, a, b), r) for r in RECORDINGS for a, b in segs[r]]
    return dict(dir=d, scp=scp, conf=conf, vconf=vconf, vads=vads, segs=segs, file_segs=file_segs)


def _wav_args(data, small_model, out, extra):
    return ["--wav-rspecifier", "scp:%s" % data["scp"], "--mfcc-config", data["conf"], "--vad-config", data["vconf"],
            "--vector-wspecifier", "ark,scp:%s,%s" % (out / "xvector.ark", out / "xvector.scp"), "--model-dir", small_model] + extra


@pytest.fixture(scope="module")
def sliding(data, small_model):
    """The sliding job through both segment sources: -> {source: directory}."""
    out = {}
    for name, source in (("device", ["--segment-by-vad"]), ("file", ["--segments", str(data["dir"] / "segments")])):
        o = data["dir"] / ("sliding-" + name)
        o.mkdir()
        _extract(_wav_args(data, small_model, o, source + ["--window", str(WINDOW), "--period", str(PERIOD),
                                                           "--subsegments-file", str(o / "subsegments")]))
        out[name] = o
    return out


def test_device_route_equals_the_file_route_byte_for_byte(sliding):
    dev, fil = sliding["device"], sliding["file"]
    for name in ("xvector.ark", "subsegments"):
        assert (dev / name).read_bytes() == (fil / name).read_bytes() and (dev / name).stat().st_size > 0, name
    # (the scp names its own ark: the same lines but for the directory)
    assert (dev / "xvector.scp").read_text().replace(str(dev), "D") == (fil / "xvector.scp").read_text().replace(str(fil), "D")
    assert sorted(os.listdir(dev)) == ["subsegments", "xvector.ark", "xvector.scp"]


def test_both_equal_the_table_route_over_the_cut_rows(data, sliding, small_model):
    """Each segment's rows cut out of the compute-mfcc-vad feature table into a table keyed by segment, through the table route
    (CMN over the segment's own rows, no VAD): the same vectors, bit for bit, under the keys moved by the segment's first frame."""
    import kaldi_io
    d = data["dir"]
    o = d / "table"
    o.mkdir()
    want_keys = []
    with kaldi_io.TableWriter(str(o / "cut.ark"), str(o / "cut.scp")) as fd:
        for reco, mat in kaldi_io.read_mat_scp(str(d / "feats.scp")):
            mat = np.asarray(mat, np.float32)
            for a, b in data["segs"][reco]:
                seg = "%s-%08d-%08d" % (reco, a, b)
                kaldi_io.write_mat(fd, np.ascontiguousarray(mat[a:b]), key=seg)
                want_keys.append((seg, reco, a))
    _extract(["--feature-rspecifier", "scp:%s" % (o / "cut.scp"), "--window", str(WINDOW), "--period", str(PERIOD),
              "--vector-wspecifier", "ark,scp:%s,%s" % (o / "xvector.ark", o / "xvector.scp"), "--model-dir", small_model])
    first_of = {seg: (reco, a) for seg, reco, a in want_keys}
    table = []
    for key, vec in _vectors(o / "xvector.ark"):
        seg, f, e = key.rsplit("-", 2)
        reco, a = first_of[seg]
        table.append(("%s-%08d-%08d" % (reco, a + int(f), a + int(e)), vec))
    got = _vectors(sliding["device"] / "xvector.ark")
    assert [k for k, _ in got] == [k for k, _ in table] and len(got) >= 8
    for (k, v), (_, w) in zip(got, table):
        assert v.dtype == w.dtype and v.tobytes() == w.tobytes(), k


def test_windows_stay_inside_segments_and_the_file_is_diarizable(data, sliding):
    import plda_backend
    sub = plda_backend.read_segments(str(sliding["device"] / "subsegments"))           # (d) what diarize reads
    assert sorted(set(r for _, r, _, _ in sub)) == sorted(RECORDINGS)
    keys = [k for k, _ in _vectors(sliding["device"] / "xvector.ark")]
    assert [k for k, _, _, _ in sub] == keys and len(set(keys)) == len(keys)
    covered = {r: set() for r in RECORDINGS}
    for key, reco, t0, t1 in sub:
        r, f, e = key.rsplit("-", 2)
        f, e = int(f), int(e)
        assert r == reco and (t0, t1) == (10 * f, 10 * e) and M <= e - f <= WINDOW
        inside = [(a, b) for a, b in data["segs"][reco] if a <= f and e <= b]
        assert len(inside) == 1, (key, data["segs"][reco])                            # (c) inside exactly one segment
        covered[reco].add(inside[0])
        v = data["vads"][reco][f:e] != 0
        idx = np.flatnonzero(v)
        assert len(idx) and (np.diff(idx) - 1 <= G).all() and idx[0] <= G and len(v) - 1 - idx[-1] <= G, key     # no pause above max_gap
    for reco in RECORDINGS:
        assert covered[reco] == set(data["segs"][reco])                                # every segment gave a window
        first = [int(k.rsplit("-", 2)[1]) for k, r, _, _ in sub if r == reco]
        assert first == sorted(first)


def test_one_vector_per_segment_without_window(data, small_model):
    """No --window: one vector per segment, averaged over --chunk-size chunks; under <reco>-<first>-<end> with --segment-by-vad,
    under the seg-id with --segments (here: other ids over the same times, so the vectors are the same bits)."""
    d = data["dir"]
    renamed = d / "segments.ids"
    renamed.write_text("".join("seg%03d %s %.3f %.3f\n" % (i, r, t0 / 1000.0, t1 / 1000.0) for i, (_, r, t0, t1) in enumerate(data["file_segs"])))
    got = {}
    for name, source in (("device", ["--segment-by-vad"]), ("file", ["--segments", str(renamed)])):
        o = d / ("whole-" + name)
        o.mkdir()
        _extract(_wav_args(data, small_model, o, source))
        got[name] = _vectors(o / "xvector.ark")
    assert [k for k, _ in got["device"]] == [k for k, _, _, _ in data["file_segs"]]
    assert [k for k, _ in got["file"]] == ["seg%03d" % i for i in range(len(data["file_segs"]))]
    for (k, v), (_, w) in zip(got["device"], got["file"]):
        assert v.tobytes() == w.tobytes() and np.isfinite(v).all(), k
