"""The host pipeline of Model.make_embedding without a GPU: the VAD/feature key alignment (frontend.VadAligner) on its own, and
the reader -> driver -> writer pipeline (xvector_amd.extract_stream) around a stand-in extractor."""
import io
import itertools
import logging
import threading
import types

import numpy as np
import pytest

import kaldi_io
from xvector_amd import engine, frontend

LOG = logging.getLogger("extract-stream-cpu")
LOG.addHandler(logging.NullHandler())


# ---- VAD alignment -------------------------------------------------------------------------------------------------------------
N_KEYS = 70
KEYS = ["utt%03d" % i for i in range(N_KEYS)]
_rng = np.random.default_rng(21)
VADS = [_rng.random(int(_rng.integers(1, 40))).astype(np.float32) for _ in range(N_KEYS)]       # distinct, 1-39 frames
EXTRA = [("zzz%02d" % i, np.full(17, 2.0 + i, np.float32)) for i in range(5)]
MISSING = {KEYS[3], KEYS[40], KEYS[69]}


def _table(base, with_extra):
    order = {"in_order": range(N_KEYS), "missing": range(N_KEYS), "empty": (),
             "permuted": np.random.default_rng(5).permutation(N_KEYS).tolist()}[base]
    entries = [(KEYS[i], VADS[i]) for i in order if not (base == "missing" and KEYS[i] in MISSING)]
    if with_extra:              # entries the features do not have, in between and at both ends (as tests/test_gpu_frontend.py has them)
        entries = [("aaa", np.ones(9, np.float32))] + entries[:20] + EXTRA[:2] + entries[20:51] + EXTRA[2:] + entries[51:]
    return entries


class _BlockTable(object):
    """Serves (key, vector) entries the way kaldi_io.VecScp does: blocks of (keys, values back to back, offsets)."""

    def __init__(self, entries, sizes):
        self.entries, self.sizes = entries, sizes

    def blocks(self):
        at, sizes = 0, itertools.cycle(self.sizes)
        while at < len(self.entries):
            part = self.entries[at:at + next(sizes)]
            at += len(part)
            yield [k for k, _ in part], np.concatenate([v for _, v in part]), np.cumsum([0] + [len(v) for _, v in part]).astype(np.int64)


BLOCK_SIZES = {"one_block": (10 ** 6,), "blocks_of_7": (7,), "blocks_of_1": (1,), "blocks_16_3_9": (16, 3, 9)}
WINDOW_SIZES = {"all": (N_KEYS,), "11": (11,), "1": (1,), "5_23": (5, 23)}


@pytest.mark.parametrize("with_extra", [False, True], ids=["plain", "with_extra_entries"])
@pytest.mark.parametrize("base", ["in_order", "permuted", "missing", "empty"])
def test_vad_aligner_hands_every_key_its_own_vector(base, with_extra):
    """Every table (in feature order, permuted, three keys missing, empty; each also with entries the features lack before,
    between and after) x every way of serving it (block source in blocks of {all, 7, 1, 16/3/9 in turn}; (key, vector) iterator)
    x every window size ({all, 11, 1, 5/23 in turn} keys at a time): each window's VadRuns has one vector per key, the
    table's vector for that key, or an empty float32 vector where the table lacks the key."""
    entries = _table(base, with_extra)
    want = dict(entries)
    assert len(want) == len(entries)
    for (sname, sizes), (wname, wsizes) in itertools.product(list(BLOCK_SIZES.items()) + [("iterator", None)], WINDOW_SIZES.items()):
        aligner = frontend.VadAligner(iter(list(entries)) if sizes is None else _BlockTable(entries, sizes))
        at, take = 0, itertools.cycle(wsizes)
        while at < N_KEYS:
            bkeys = KEYS[at:at + next(take)]
            at += len(bkeys)
            runs = frontend.VadRuns()
            aligner.append(list(bkeys), runs)
            assert len(runs) == len(bkeys), (sname, wname, at)
            for key, got in zip(bkeys, runs):
                exp = want.get(key, np.zeros(0, np.float32))
                assert got.dtype == np.float32 and got.shape == exp.shape and np.array_equal(got, exp), (sname, wname, key)


def test_vad_aligner_reads_an_ark_stream():
    """The third kind of ``vad_stream``: the VAD ark itself."""
    buf = io.BytesIO()
    for k, v in zip(KEYS, VADS):
        kaldi_io.write_vec_flt(buf, v, key=k)
    aligner = frontend.VadAligner(io.BytesIO(buf.getvalue()))
    runs = frontend.VadRuns()
    aligner.append(list(KEYS), runs)
    assert len(runs) == N_KEYS and all(np.array_equal(a, b) for a, b in zip(runs, VADS))


# ---- reader -> driver -> writer around a stand-in extractor --------------------------------------------------------------------
LENS = [30, 5, 80, 12, 0, 200, 45, 9, 60, 33, 150, 10, 71]          # the ark of tests/test_dist_cpu.py
MIN_CHUNK = 10


def _utterances():
    rng = np.random.default_rng(2)
    return [("utt%02d" % i, rng.standard_normal((t, 5)).astype(np.float32)) for i, t in enumerate(LENS)]


def _ark():
    buf = io.BytesIO()
    for k, m in _utterances():
        kaldi_io.write_mat(buf, m, key=k)
    return buf.getvalue()


class FakeExtractor(object):          # stand-in for the GPU extractor: vector = f(utterance), None below min_chunk_size
    fail_on_submit = None

    def __init__(self, model, min_chunk_size, chunk_size, **kw):
        self.min = min_chunk_size
        self.stats = dict(batches=0, chunks=0, frames=0, rows=0)

    def submit(self, mats, addrs=None):
        if self.fail_on_submit is not None:
            raise self.fail_on_submit
        self.stats["frames"] += sum(m.shape[0] for m in mats)
        return [None if m.shape[0] < self.min else np.concatenate([m.mean(0), [m.shape[0]]]).astype(np.float32) for m in mats]

    def finish(self, h, as_array=False):
        valid = np.array([v is not None for v in h], bool)
        full = np.zeros((len(h), 6), np.float32)
        for i, v in enumerate(h):
            if v is not None:
                full[i] = v
        return (full, valid) if as_array else h


@pytest.fixture
def models_mod(monkeypatch):
    """local/tf/models.py with the stand-in extractor and loader and the settings that cut the ark into several windows."""
    import models

    def fake_load(self, sess, input_dir, logger):
        self.device_model = types.SimpleNamespace(device="cpu", embed_dim=6, feat_dim=5)
    monkeypatch.setattr(engine, "Extractor", FakeExtractor)
    monkeypatch.setattr(FakeExtractor, "fail_on_submit", None)
    monkeypatch.setattr(models.Model, "load_model", fake_load)
    monkeypatch.setattr(models.Model, "window_frames", 400)
    monkeypatch.setattr(models.Model, "arena_bytes", 4096)               # (in-place reader: one arena = one window)
    monkeypatch.setattr(models.Model, "first_arena_bytes", 4096)
    return models


def _reader(monkeypatch, reader):
    if reader == "in_place":
        monkeypatch.setattr(kaldi_io, "_HOST_LIB", False)                # (not tried yet)
        if kaldi_io._host_lib() is None:
            pytest.skip("libxvector_host.so is not built")
    else:
        monkeypatch.setattr(kaldi_io, "_HOST_LIB", None)                 # the generic block reader, with or without the library


def _source(kind, data):
    if kind == "bytesio":
        return io.BytesIO(data)
    if kind == "buffered":
        return io.BufferedReader(io.BytesIO(data))
    return iter(_utterances())


def _embed(models, source, out=None):
    out = io.BytesIO() if out is None else out
    models.Model().make_embedding(source, out, "unused", MIN_CHUNK, -1, True, LOG)
    return out.getvalue()


@pytest.mark.parametrize("reader,kind", [("generic", "bytesio"), ("generic", "buffered"), ("generic", "iterator"),
                                         ("in_place", "bytesio"), ("in_place", "buffered")])
def test_every_input_kind_writes_the_same_vectors(monkeypatch, models_mod, reader, kind):
    """The ark as a BytesIO, a BufferedReader and an iterator of (key, matrix), through the generic reader and (when the
    host library is built) the in-place one: the same bytes as the iterator through the generic reader writes, the keys with
    >= 10 rows in input order, each with its own vector."""
    _reader(monkeypatch, reader)
    got = _embed(models_mod, _source(kind, _ark()))
    monkeypatch.setattr(kaldi_io, "_HOST_LIB", None)
    assert got == _embed(models_mod, _source("iterator", None))
    vecs = list(kaldi_io.read_vec_flt_ark(io.BytesIO(got)))
    utts = [(k, m) for k, m in _utterances() if m.shape[0] >= MIN_CHUNK]
    assert [k for k, _ in vecs] == [k for k, _ in utts]
    for (_, v), (_, m) in zip(vecs, utts):
        assert v[-1] == m.shape[0] and np.allclose(v[:-1], m.mean(0), rtol=1e-6, atol=1e-6)


class _Boom(Exception):
    pass


class _FailingOutput(object):
    mode = "wb"

    def __init__(self, error):
        self.error = error

    def write(self, data):
        raise self.error

    def write_vectors(self, keys, vecs):
        raise self.error


@pytest.mark.parametrize("reader,kind", [("generic", "iterator"), ("generic", "bytesio"), ("in_place", "buffered")])
@pytest.mark.parametrize("failure", ["load_model", "submit", "output"])
def test_no_thread_outlives_a_failed_call(monkeypatch, models_mod, failure, reader, kind):
    """A load_model that raises, an extractor whose submit raises on the first window, an output that cannot be written: the
    same error comes out of make_embedding, and every thread the call started ends (the queues poll their cancel flag every
    0.2 s; 5 s leaves room for a loaded machine).  The iterator makes the two-window case: when the loader fails after the
    input has been read to its end -- as beside a real model load -- the reader has two windows queued and its end mark in
    hand, and a blocking put there held the thread and its arenas for good."""
    _reader(monkeypatch, reader)
    error, out, source = _Boom(failure), None, _source(kind, _ark())
    drained = threading.Event()
    if kind == "iterator":
        def until_drained(it):
            for item in it:
                yield item
            drained.set()
        source = until_drained(source)
    else:
        drained.set()
    if failure == "load_model":
        def failing_load(self, sess, input_dir, logger):
            drained.wait(5.0)
            raise error
        monkeypatch.setattr(models_mod.Model, "load_model", failing_load)
    elif failure == "submit":
        monkeypatch.setattr(FakeExtractor, "fail_on_submit", error)
    else:
        out = _FailingOutput(error)
    before = set(threading.enumerate())
    with pytest.raises(_Boom) as caught:
        _embed(models_mod, source, out)
    assert caught.value is error
    started = [t for t in threading.enumerate() if t not in before]
    for t in started:
        t.join(5.0)
    assert not [t.name for t in started if t.is_alive()]


@pytest.mark.parametrize("reader", ["generic", "in_place"])
def test_a_truncated_ark_raises_in_the_caller(monkeypatch, models_mod, reader):
    """The last 7 bytes cut, through a BufferedReader: the reader's error comes out of make_embedding (no hang)."""
    _reader(monkeypatch, reader)
    before = set(threading.enumerate())
    with pytest.raises(ValueError):
        _embed(models_mod, io.BufferedReader(io.BytesIO(_ark()[:-7])))
    for t in [t for t in threading.enumerate() if t not in before]:
        t.join(5.0)
        assert not t.is_alive()
