"""Host side of the egs builder (xvector_amd/egs.py, local/tf/make_egs.py) on the CPU: the allocation against what the reference's
create_egs.py wrote (tests/golden/egs_alloc.npz, made by tests/golden/make_golden_egs.py), stage 3's filters, and EgsWriter with a
NumPy stand-in for the device gather (tests/egs_ref.py) against examples_io.RangesDataLoader on a no-silence table."""
import os

import numpy as np
import pytest

import egs_ref


def _golden_tables(g):
    def rd(k):
        return [tuple(line.split()) for line in bytes(g[k]).decode().splitlines()]
    return rd("utt2len"), rd("utt2int")


def _kwargs(flags):
    kw = {}
    for f in flags:
        k, v = str(f)[2:].split("=")
        k = k.replace("-", "_")
        kw[k] = v if k == "prefix" else (v == "true") if k == "randomize_chunk_length" else int(v)
    return kw


def _files(d):
    names = sorted(os.path.relpath(os.path.join(dd, f), d) for dd, _, fs in os.walk(d) for f in fs)
    return dict((n, open(os.path.join(d, n), "rb").read()) for n in names)


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_allocate_writes_the_reference_files_byte_for_byte(golden, tmp_path, tag):
    from xvector_amd import egs
    g = golden("egs_alloc.npz")
    utt2len, utt2int = _golden_tables(g)
    kw = _kwargs(g[tag + "_args"])
    counts = egs.allocate(utt2len, utt2int, str(tmp_path / "egs"), **kw)
    got = _files(str(tmp_path / "egs"))
    names = [str(n) for n in g[tag + "_names"]]
    assert sorted(got) == names and len(names) >= 5
    for i, n in enumerate(names):
        assert got[n] == bytes(g["%s_%d" % (tag, i)]), n
    pre = kw.get("prefix", "") + "_" if kw.get("prefix") else ""
    assert [int(l.split()[1]) for l in got["temp/%sarchive_minibatch_count" % pre].decode().splitlines()] == counts
    assert int(g[tag + "_stdout_retries"]) > 0                         # the fixture does take the short-utterance redraw
    if tag == "b":                                                     # "Ran out of speakers": 12 draws per archive, 3 minibatches of 4
        assert counts == [3, 3, 3]
    # another seed deals other chunks
    egs.allocate(utt2len, utt2int, str(tmp_path / "other"), **dict(kw, seed=124))
    other = _files(str(tmp_path / "other"))
    assert sorted(other) == names and any(other[n] != got[n] for n in names if "ranges" in n)


def test_allocate_raises_where_the_reference_would_spin(tmp_path):
    from xvector_amd import egs
    utt2len = [("a1", 90), ("a2", 80), ("b1", 30), ("b2", 35)]
    utt2int = [("a1", 0), ("a2", 0), ("b1", 1), ("b2", 1)]
    with pytest.raises(egs.AllocationError, match="speaker 1"):
        egs.allocate(utt2len, utt2int, str(tmp_path), num_repeats=4, min_frames_per_chunk=40, max_frames_per_chunk=40, frames_per_iter=1000,
                     num_archives=1, num_jobs=1, minibatch_size=2)
    # the check costs no draw: with chunks every speaker can serve, the files are those of the plain run
    a = egs.allocate(utt2len, utt2int, str(tmp_path / "x"), num_repeats=4, min_frames_per_chunk=20, max_frames_per_chunk=30,
                     frames_per_iter=1000, num_archives=1, num_jobs=1, minibatch_size=2)
    assert a == [4]


def test_filter_utterances_strict_length_and_inclusive_count():
    from xvector_amd import egs
    utt2spk = [("s1-u%d" % i, "s1") for i in range(3)] + [("s2-u%d" % i, "s2") for i in range(3)] + [("s3-u0", "s3")]
    voiced = dict((u, (11, 20)) for u, _ in utt2spk)
    voiced["s1-u2"] = (10, 20)                         # == min_len: out (strict >), s1 keeps 2 utterances
    voiced["s2-u1"] = (10, 20)
    voiced["s2-u2"] = (0, 20)
    lengths = dict((u, (20, 23)) for u, _ in utt2spk)
    u2s, s2u, u2n = egs.filter_utterances(utt2spk, voiced, lengths, min_len=10, min_num_utts=2)
    assert s2u == [("s1", ["s1-u0", "s1-u1"])]          # s1 has exactly min_num_utts (>=), s2 one too few, s3 one
    assert u2s == [("s1-u0", "s1"), ("s1-u1", "s1")] and u2n == [("s1-u0", 11), ("s1-u1", 11)]
    u2s, s2u, _ = egs.filter_utterances(utt2spk, voiced, lengths, min_len=9, min_num_utts=2)
    assert [s for s, _ in s2u] == ["s1", "s2"] and len(u2s) == 5


def test_prepare_drops_what_select_voiced_frames_drops(tmp_path):
    import kaldi_io
    import make_egs
    data = str(tmp_path / "data")
    utts = egs_ref.make_data_dir(data, 2, 4, 60, 90, 5, seed=3, voiced_p=0.8)
    keys = list(utts)
    # rewrite the VAD table: one vector one frame short, one with nothing voiced
    with kaldi_io.TableWriter(os.path.join(data, "vad.ark"), os.path.join(data, "vad.scp")) as tv:
        for k in keys:
            v = utts[k][1]
            if k == keys[1]:
                v = v[:-1]
            if k == keys[5]:
                v = np.zeros_like(v)
            kaldi_io.write_vec_flt(tv, v, key=k)
    from xvector_amd import egs
    lens = egs.feat_lengths(os.path.join(data, "feats.scp"))
    assert [lens[k] for k in keys] == [(utts[k][0].shape[0], 5) for k in keys]
    vc = egs.voiced_counts(os.path.join(data, "vad.scp"))
    assert vc[keys[0]] == (int(np.count_nonzero(utts[keys[0]][1])), len(utts[keys[0]][1])) and vc[keys[5]][0] == 0
    make_egs.main(["prepare", "--data", data, "--out-dir", str(tmp_path / "ns"), "--min-len", "20", "--min-num-utts", "3"])
    kept = [l.split()[0] for l in open(str(tmp_path / "ns" / "utt2num_frames"))]
    assert kept == sorted(k for k in keys if k not in (keys[1], keys[5]))
    assert open(str(tmp_path / "ns" / "feat_dim")).read() == "5\n"
    want = dict((k, int(np.count_nonzero(utts[k][1]))) for k in kept)
    assert dict((l.split()[0], int(l.split()[1])) for l in open(str(tmp_path / "ns" / "utt2num_frames"))) == want
    (tmp_path / "data" / "segments").write_text("x\n")
    with pytest.raises(SystemExit):
        make_egs.main(["prepare", "--data", data, "--out-dir", str(tmp_path / "ns2")])


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    """One data directory -> allocation (2 archives, 1 job) -> EgsWriter with the NumPy gather."""
    from xvector_amd import egs
    root = tmp_path_factory.mktemp("egs_cpu")
    data, egs_dir = str(root / "data"), str(root / "egs")
    B, F = 4, 7
    utts = egs_ref.make_data_dir(data, 5, 4, 80, 150, F, seed=5, voiced_p=0.8)
    voiced = egs.voiced_counts(os.path.join(data, "vad.scp"))
    utt2len = [(k, voiced[k][0]) for k in utts]
    utt2int = [(k, int(k[3:k.index("-")])) for k in utts]
    counts = egs.allocate(utt2len, utt2int, egs_dir, num_repeats=8, min_frames_per_chunk=20, max_frames_per_chunk=40, frames_per_iter=1000,
                          num_archives=2, num_jobs=1, minibatch_size=B)
    os.makedirs(os.path.join(egs_dir, "info"))
    for name, v in (("feat_dim", F), ("num_archives", 2)):
        open(os.path.join(egs_dir, "info", name), "wt").write("%d\n" % v)
    gather = egs_ref.NumpyGather(300, True, 100)
    w = egs.EgsWriter(egs_dir, os.path.join(data, "feats.scp"), os.path.join(data, "vad.scp"), F, B, shuffle=True, random_seed=2468,
                      gather=gather, frame_budget=500)
    w.write_job(os.path.join(egs_dir, "temp", "outputs.1"))
    # the no-silence table stage 3 of the reference would have written, from the oracle (float32 of the float64 CMN)
    table = dict((k, egs_ref.cmn_f64(m)[egs_ref.voiced_rows(v)].astype(np.float32)) for k, (m, v) in utts.items())
    scp = egs_ref.write_table(str(root / "no_sil"), table)
    return dict(egs_dir=egs_dir, counts=counts, B=B, F=F, scp=scp, gather=gather, writer=w, data=data)


def test_writer_members_are_the_chunks_the_ranges_loader_cuts(written):
    egs_dir, B, F = written["egs_dir"], written["B"], written["F"]
    assert written["gather"].calls > 2                     # the frame budget cut the archives into several windows
    rs = np.random.RandomState(2468)                       # ONE seeded stream, one permutation per archive in outputs-file order
    for idx, count in enumerate(written["counts"], 1):
        perm = rs.permutation(np.arange(count))
        want, want_labels = egs_ref.served_by_ranges_loader(os.path.join(egs_dir, "temp", "ranges.%d" % idx), written["scp"], count, B, F)
        members, labels = egs_ref.read_tar(os.path.join(egs_dir, "egs.%d.tar" % idx))
        assert len(members) == count and labels.shape == (count, B)
        for i in range(count):
            assert members[i].dtype == np.float16 and members[i].shape == want[perm[i]].shape
            assert np.array_equal(members[i], want[perm[i]].astype(np.float16)), (idx, i)
            assert np.array_equal(labels[i], want_labels[perm[i]])
        assert not os.path.exists(os.path.join(egs_dir, "egs.%d.tar.tmp.tar" % idx))
        assert sorted(f for f in os.listdir(egs_dir) if f.startswith("egs.%d." % idx)) == ["egs.%d.npy" % idx, "egs.%d.tar" % idx]


def test_writer_output_is_what_the_trainer_reads(written):
    import examples_io
    import ze_utils
    num_archives, feat_dim, counts = ze_utils.verify_egs_dir(written["egs_dir"])
    assert num_archives == 2 and feat_dim == written["F"] and counts == dict(enumerate(written["counts"], 1))
    loader = examples_io.TarFileDataLoader(os.path.join(written["egs_dir"], "egs.1.tar"))
    assert loader.count == written["counts"][0]
    data, labels = loader.pop(timeout=10)
    loader.close()
    assert data.dtype == np.float16 and data.shape[0] == written["B"] and data.shape[2] == written["F"] and labels.shape == (written["B"],)


def test_writer_leaves_an_existing_archive_alone(written):
    from xvector_amd import egs
    egs_dir = written["egs_dir"]
    tar1 = os.path.join(egs_dir, "egs.1.tar")
    before2 = open(os.path.join(egs_dir, "egs.2.tar"), "rb").read()
    labels2 = open(os.path.join(egs_dir, "egs.2.npy"), "rb").read()
    keep = open(tar1, "rb").read()
    try:
        open(tar1, "wb").write(b"from before")
        os.remove(os.path.join(egs_dir, "egs.2.tar"))
        gather = egs_ref.NumpyGather(300, True, 100)
        w = egs.EgsWriter(egs_dir, os.path.join(written["data"], "feats.scp"), os.path.join(written["data"], "vad.scp"), written["F"],
                          written["B"], shuffle=True, random_seed=2468, gather=gather)
        w.write_job(os.path.join(egs_dir, "temp", "outputs.1"))
        assert open(tar1, "rb").read() == b"from before"
        # the second archive is rebuilt with the SECOND permutation of the stream although the first was skipped
        assert open(os.path.join(egs_dir, "egs.2.tar"), "rb").read() == before2
        assert open(os.path.join(egs_dir, "egs.2.npy"), "rb").read() == labels2
    finally:
        open(tar1, "wb").write(keep)


def test_writer_refuses_a_table_that_leaves_its_utterance(written):
    from xvector_amd import hiplib
    counts = np.array([10, 5], np.int32)
    ok = (np.array([0, 1]), np.array([0, 2]), np.array([10, 3]), np.array([0, 70], np.int64))
    hiplib.check_chunk_table(ok, counts, 7, 70 + 21)
    for bad in ((np.array([0]), np.array([1]), np.array([10]), np.array([0], np.int64)),          # past the voiced count
                (np.array([2]), np.array([0]), np.array([1]), np.array([0], np.int64)),           # no such utterance
                (np.array([1]), np.array([-1]), np.array([2]), np.array([0], np.int64)),
                (np.array([1]), np.array([0]), np.array([5]), np.array([60], np.int64))):          # past the destination
        with pytest.raises(ValueError):
            hiplib.check_chunk_table(bad, counts, 7, 91)


def test_cli_takes_the_command_lines_get_egs_sh_builds():
    import make_egs
    p = make_egs.get_parser()
    a = p.parse_args("allocate --num-repeats=10 --num-jobs=6 --minibatch-size=128 --min-frames-per-chunk=200 --max-frames-per-chunk=400 "
                     "--frames-per-iter=10000000 --num-archives=17 --utt2len-filename=e/temp/utt2num_frames.train "
                     "--utt2int-filename=e/temp/utt2int.train --egs-dir=e".split())
    assert (a.num_repeats, a.num_jobs, a.minibatch_size, a.randomize_chunk_length, a.seed, a.accepted_overlap, a.num_pdfs, a.prefix) == \
        (10, 6, 128, "true", 123, 0.2, -1, "")
    a = p.parse_args("allocate --prefix=valid --num-repeats=8 --num-jobs=1 --minibatch-size=128 --min-frames-per-chunk=200 "
                     "--max-frames-per-chunk=400 --randomize-chunk-length=false --frames-per-iter=100000 --num-archives=1 "
                     "--utt2len-filename=a --utt2int-filename=b --egs-dir=e".split())
    assert a.prefix == "valid" and a.randomize_chunk_length == "false"
    d = p.parse_args("allocate --utt2len-filename=a --utt2int-filename=b --egs-dir=e".split())
    assert (d.num_repeats, d.min_frames_per_chunk, d.max_frames_per_chunk, d.frames_per_iter, d.num_archives, d.num_jobs, d.minibatch_size) \
        == (10, 50, 300, 1000000, -1, -1, 128)
    w = p.parse_args("write --prefix=train_subset --random-seed=2468 --feature-dim=23 --minibatch-size=128 "
                     "--outputs-file=e/temp/train_subset_outputs.1 --shuffle=True --egs-dir=e --feats-scp d/feats.scp --vad-scp d/vad.scp".split())
    assert (w.prefix, w.random_seed, w.feature_dim, w.minibatch_size, w.shuffle, w.cmn_window, w.cmn_center, w.min_window) == \
        ("train_subset", 2468, 23, 128, True, 300, "yes", 100)
    with pytest.raises(SystemExit):
        p.parse_args("write --egs-dir=e --outputs-file=o --feats-scp f --vad-scp v".split())      # --feature-dim, --minibatch-size required
