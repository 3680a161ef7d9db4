"""The host pipeline of ``Model.make_embedding`` (local/tf/models.py), stage by stage: ``WindowReader`` parses the input into
windows on a thread of its own (``WaveTable`` in its place when the input is a wav.scp), ``Extraction`` carries one call's windows through the front-end and the extractor, and
``VectorWriter`` serialises the finished vectors on a third thread.  The driver loop itself stays in ``make_embedding``."""
import functools
import queue
import threading
import time

import numpy as np

from . import engine, frontend


class _Cancelled(Exception):
    pass


def put_unless_cancelled(q, item, cancel):
    """``q.put(item)`` that gives up (-> False) once ``cancel`` is set: what EVERY producer thread here enqueues with, its
    end-of-stream mark and a forwarded exception included -- a consumer that has given up no longer reads the queue, and a
    plain ``put`` on a full queue would then hold the thread (and what it owns) for the life of the process."""
    while not cancel.is_set():
        try:
            q.put(item, timeout=0.2)
            return True
        except queue.Full:
            pass
    return False


def prefetched(blocks, cancel, depth=2):
    """``blocks`` read by a thread of its own, ``depth`` ahead (the VAD table beside the features: its reads release the
    interpreter lock, so the two files are read side by side)."""
    q, end = queue.Queue(maxsize=depth), object()

    def run():
        try:
            for b in blocks:
                if not put_unless_cancelled(q, b, cancel):
                    return
            put_unless_cancelled(q, end, cancel)
        except BaseException as e:      # noqa: B902 -- forwarded to the consumer
            put_unless_cancelled(q, e, cancel)
    threading.Thread(target=run, daemon=True).start()
    while True:
        try:
            b = q.get(timeout=0.2)
        except queue.Empty:
            if cancel.is_set():         # the thread above may have left without its end mark
                raise _Cancelled()
            continue
        if b is end:
            return
        if isinstance(b, BaseException):
            raise b
        yield b


class _Held(object):
    """Keeps a gathered block alive as the holder of an ``ArkMats`` piece and hands out its utterances as views."""

    def __init__(self, feats, offsets):
        self.buf, self.addr, self._feats, self._off = feats, feats.ctypes.data, feats, offsets


class WindowReader(object):
    """A reader thread parses the next window of the input while the GPU works on the current one (bounded queue: at most 2
    parsed windows in memory).  Iterating yields ``(keys, mats, vads)`` per window -- a kaldi_io.ArkMats and, with a
    ``vad_stream``, a frontend.VadRuns -- in input order; a parse error is re-raised in the consumer.

    The utterances are used IN PLACE: the stream is read (readinto) into a few long-lived arenas, the native scanner locates
    the matrices there, and the native packer copies them from the arena straight into the pinned staging sets -- one host
    copy between the ark bytes and the H2D DMA, no fresh pages per window (at GB/s the page faults of ever-new arrays and the
    extra gather copy cost more than the parsing).  The consumer hands a window's arenas back (``recycle``) once the window
    has been collected.  Without libxvector_host.so the generic (gathering) block reader is used.

    The thread starts with the object.  ``model`` is the Model instance: its ``window_frames``, ``first_window_frames``,
    ``arena_bytes``, ``first_arena_bytes``, ``arena_count`` and ``map_input`` are read as the thread goes."""

    def __init__(self, model, input_stream, vad_stream=None):
        import kaldi_io
        self.model, self.input_stream, self.vad_stream = model, input_stream, vad_stream
        self.in_place = kaldi_io._host_lib() is not None and (hasattr(input_stream, "read") or hasattr(input_stream, "windows"))
        self.arena_bytes = int(model.arena_bytes)
        self._cancel = threading.Event()              # set when the consumer gives up (e.g. the model failed to load)
        self._windows = queue.Queue(maxsize=2)
        self._pool = queue.Queue()
        self._mine = []                               # arenas this call took from the process-wide free list
        self._thread = threading.Thread(target=self._run, daemon=True)
        self._thread.start()

    def __iter__(self):
        return self

    def __next__(self):
        item = self._windows.get()
        if item is None:
            raise StopIteration
        if isinstance(item, BaseException):
            raise item
        return item

    def recycle(self, arenas):
        for a in arenas:
            self._pool.put(a)

    def cancel(self):
        self._cancel.set()

    def close(self):
        """The consumer is done (a no-op for the thread after a complete pass: it has already returned).  The arenas go back
        to the process-wide free list unless the thread is still inside one."""
        import kaldi_io
        self._cancel.set()
        if not self._thread.is_alive():
            for a in self._mine:
                kaldi_io.arena_release(a)
            self._mine = []

    def _take_arena(self):
        import kaldi_io
        if len(self._mine) < self.model.arena_count and self._pool.empty():
            self._mine.append(kaldi_io.arena_acquire(self.arena_bytes))
            return self._mine[-1]
        while True:
            try:
                return self._pool.get(timeout=0.2)
            except queue.Empty:
                if self._cancel.is_set():         # the consumer gave up: nobody will ever return an arena
                    raise _Cancelled()

    def _pieces(self):
        """(keys, addr[n], rows[n], cols, holder) -- utterances where they lie: whole arenas for ark streams and scp
        tables (first arena short, then doubling: the GPU starts after a fraction of a window), gathered blocks
        without the host library, one matrix at a time for (key, matrix) iterators."""
        import kaldi_io
        input_stream, take_arena, release = self.input_stream, self._take_arena, self._pool.put
        first = int(self.model.first_arena_bytes)
        if self.in_place:
            # an ark that already sits in memory (a BytesIO, a regular file through the page cache) is not read at
            # all: the scanner walks the mapping and the packer takes the rows from there
            mapped = kaldi_io.map_stream(input_stream) if (hasattr(input_stream, "read") and self.model.map_input) else None
            if mapped is not None:
                source = kaldi_io.scan_mat_ark_mapped(
                    mapped, self.arena_bytes, first,
                    fallback=lambda rest: kaldi_io.scan_mat_ark_windows(kaldi_io.MemStream(rest), take_arena, None, release))
            elif hasattr(input_stream, "read"):
                source = kaldi_io.scan_mat_ark_windows(input_stream, take_arena, first, release)
            else:
                source = input_stream.windows(take_arena, first, release)
            for item in source:
                yield item
        elif hasattr(input_stream, "read") or hasattr(input_stream, "blocks"):
            source = kaldi_io.read_mat_ark_blocks(input_stream) if hasattr(input_stream, "read") else input_stream.blocks()
            for bkeys, bfeats, off in source:
                row_bytes = bfeats.shape[1] * bfeats.itemsize if bfeats.ndim == 2 else 0
                yield bkeys, (bfeats.ctypes.data + off[:-1] * row_bytes).astype(np.uint64), np.diff(off).astype(np.int32), \
                    (bfeats.shape[1] if bfeats.ndim == 2 else 0), _Held(bfeats, off)
        else:
            for key, mat in input_stream:
                mat = np.ascontiguousarray(mat, dtype=np.float32)
                yield [key], np.array([mat.__array_interface__["data"][0]], np.uint64), \
                    np.array([mat.shape[0]], np.int32), (mat.shape[1] if mat.ndim == 2 else 0), mat

    def _put(self, item):
        if not put_unless_cancelled(self._windows, item, self._cancel):
            raise _Cancelled()

    def _run(self):
        import kaldi_io
        try:
            model, aligner = self.model, None
            if self.vad_stream is not None:
                aligner = frontend.VadAligner(self.vad_stream, functools.partial(prefetched, cancel=self._cancel))
            keys, mats, frames = [], kaldi_io.ArkMats(), 0
            vads = None if aligner is None else frontend.VadRuns()
            # a window closes at the first piece boundary past its frame limit (in place: one arena = one window)
            limit = min(model.window_frames, model.first_window_frames)
            for bkeys, addr, rows, cols, holder in self._pieces():
                keys.extend(bkeys)
                mats.add(addr, rows, cols, holder)
                if aligner is not None:
                    aligner.append(list(bkeys), vads)
                frames += int(np.sum(rows))
                if frames >= limit or self.in_place:
                    self._put((keys, mats, vads))
                    keys, mats, frames = [], kaldi_io.ArkMats(), 0
                    vads = None if aligner is None else frontend.VadRuns()
                    limit = min(model.window_frames, 2 * limit)
            if keys:
                self._put((keys, mats, vads))
            self._put(None)
        except _Cancelled:
            pass
        except BaseException as e:          # noqa: B902 -- forwarded to the consumer
            put_unless_cancelled(self._windows, e, self._cancel)


class WaveBatch(object):
    """One window of a ``WaveTable``: the keys and waves of a ``mfcc_vad._planned_batches`` batch, in the place of a window's
    matrices (it answers what ``make_embedding``'s loop asks of those: no uniform column count, no arenas to give back)."""
    holders = ()
    addrs = None

    def __init__(self, table, keys, waves):
        self.table, self.keys, self.waves = table, keys, waves

    def __len__(self):
        return len(self.keys)

    def uniform_cols(self):
        return None


class WaveTable(object):
    """A wav.scp as the ``input_stream`` of ``Model.make_embedding``: x-vectors straight from audio, the MFCC rows and the VAD
    decisions never leave the device.  The thread interface is ``WindowReader``'s.  The thread does host work
    only -- it reads the files and their headers, plans ``wav-reverberate`` entries and deals the entries into windows of at most
    ``window_samples`` samples, with ``mfcc_vad._planned_batches``, i.e. exactly the batches ``compute-mfcc-vad`` would launch --
    and yields ``(keys, WaveBatch, None)``; the consumer's thread runs ``compute`` (the MFCC engine's launches) and the submit.
    ``mfcc_opts`` / ``vad_opts``: ``mfcc.MfccOptions`` / ``mfcc.VadOptions``.  ``start`` starts the thread (``make_embedding``
    calls it once it has accepted its arguments).  ``segmenter`` (a ``segment.VadSegmenter`` or ``segment.FileSegmenter``; DESIGN.md
    §8.18): every recording is cut into segments and the extractor takes each segment as an utterance of its own."""

    def __init__(self, wav_scp, mfcc_opts, vad_opts, window_samples=1 << 26, segmenter=None):
        from . import augment
        self.path, self.opts, self.vad_opts, self.window_samples = wav_scp, mfcc_opts, vad_opts, int(window_samples)
        self.segmenter = segmenter
        self.opts.check(resample=True)                # (NotImplementedError / ValueError: before anything is read)
        self._augmenter = augment.Augmenter()
        self._engine = None
        self._cancel = threading.Event()
        self._windows = queue.Queue(maxsize=2)
        self._thread = None

    def start(self):
        if self._thread is None:
            self._thread = threading.Thread(target=self._run, daemon=True)
            self._thread.start()
        return self

    def __iter__(self):
        return self.start()

    def __next__(self):
        item = self._windows.get()
        if item is None:
            raise StopIteration
        if isinstance(item, BaseException):
            raise item
        return item

    def recycle(self, arenas):
        pass

    def cancel(self):
        self._cancel.set()

    def close(self):
        self._cancel.set()

    def _run(self):
        try:
            import mfcc_vad
            for keys, waves in mfcc_vad._planned_batches(self.path, self.opts, self._augmenter, self.window_samples):
                if not put_unless_cancelled(self._windows, (keys, WaveBatch(self, keys, waves), None), self._cancel):
                    return
            put_unless_cancelled(self._windows, None, self._cancel)
        except BaseException as e:          # noqa: B902 -- forwarded to the consumer (SystemExit of an unreadable entry included)
            put_unless_cancelled(self._windows, e, self._cancel)

    def compute(self, batch, device):
        """MFCC + VAD of one window on ``device``: ``mfcc.Mfcc.compute_device``'s result (through ``augment.mfcc_compute`` when the
        window holds ``wav-reverberate`` entries)."""
        from . import augment, mfcc
        if self._engine is None:
            self._engine = mfcc.Mfcc(self.opts, self.vad_opts, device=device, window_samples=self.window_samples)
            self._augmenter.device = device
        if any(isinstance(w, augment.Pending) for w in batch.waves):
            return augment.mfcc_compute(self._engine, self._augmenter, batch.keys, batch.waves, device=True)
        return self._engine.compute_device(batch.keys, batch.waves)

    def segments(self, batch, vad, row0, T, ready):
        """The segment tables of a computed window, one (seg-ids or None, int32 [n, 2] of (first frame, length)) per recording:
        the segmenter's, on the MFCC engine's stream behind ``ready``."""
        return self.segmenter.tables(batch.keys, vad, row0, T, self.opts.frame_shift, self._engine._stream, ready)


class SegmentKeys(list):
    """The keys of a window whose utterances are segments of recordings: beside each key, its recording (``reco``) and its first
    frame there (``first``, int64 array)."""

    def __init__(self, keys, reco, first):
        list.__init__(self, keys)
        self.reco, self.first = list(reco), np.asarray(first, np.int64).reshape(-1)


def subsegment_key(utt, first, end):
    """The key of the x-vector of frames [first, end) of ``utt`` (sliding mode): fixed-width numbers, so that the keys of an
    utterance sort in the order of their first frames."""
    return "%s-%08d-%08d" % (utt, first, end)


def subsegment_line(key, utt, first, end, frame_shift):
    """One line of the subsegments file, the layout of a Kaldi ``segments`` file: ``<key> <utt> <start s> <end s>``;
    ``frame_shift`` in milliseconds."""
    return "%s %s %.3f %.3f\n" % (key, utt, first * frame_shift / 1000.0, end * frame_shift / 1000.0)


class VectorWriter(object):
    """A writer thread serialises the records of finished windows (same bytes as write_vec_flt per key), in order, so that
    formatting ~50 k records per window does not sit between two kernel launches (bounded queue: 4 windows).  After an error
    it keeps draining, so that the producer never blocks; ``check`` re-raises the error in the caller."""

    def __init__(self, output_stream, subsegments=None, frame_shift=10.0):
        """subsegments (sliding mode): a text stream that gets one line per vector whose ``put`` names its sub-segment, in the
        layout of a Kaldi ``segments`` file; ``frame_shift`` in milliseconds turns frame indices into seconds."""
        self._out, self._q, self.error = output_stream, queue.Queue(maxsize=4), None
        self._sub, self._shift = subsegments, float(frame_shift)
        self._thread = threading.Thread(target=self._run, daemon=True)
        self._thread.start()

    def _run(self):
        import kaldi_io
        while True:
            item = self._q.get()
            if item is None:
                return
            if self.error is not None:
                continue
            try:
                kaldi_io.write_vec_flt_batch(self._out, item[0], item[1])
                if self._sub is not None and item[2] is not None:
                    self._sub.write("".join(subsegment_line(k, u, f, e, self._shift) for k, u, (f, e) in
                                            zip(item[0], item[2][0], item[2][1].tolist())))
            except BaseException as e:          # noqa: B902 -- forwarded to the caller
                self.error = e

    def put(self, keys, vecs, subsegments=None):
        """subsegments: None, or (utterance key per vector, spans int [n, 2]) for the subsegments file."""
        self._q.put((keys, vecs, subsegments))

    def check(self):
        if self.error is not None:
            raise self.error

    def close(self):
        self._q.put(None)
        self._thread.join()                     # the caller closes the output right after make_embedding returns


class Extraction(object):
    """One make_embedding call between its reader and its writer: what happens to a window (``submit``, later ``retire``) and
    the call's counters.  ``rank``/``world``: this process's place among those that share the input stream (0, 1: alone);
    then ``stash`` holds (keys, lens, shards, local vectors) per window until ``model._exchange_shards`` sends them."""

    def __init__(self, model, ex, front, writer, logger, min_chunk_size, chunk_size, rank=0, world=1):
        self.model, self.ex, self.front, self.writer, self.logger = model, ex, front, writer, logger
        self.min_chunk_size, self.chunk_size, self.rank, self.world = min_chunk_size, chunk_size, rank, world
        self.total_segments = self.num_fail = self.num_success = 0
        self.compute_time = 0.0
        self.stash = []
        # sliding mode (the extractor has a ``window``): one vector per sub-segment, keys expanded by ``emit_subsegments``
        self.sliding = getattr(ex, "window", None) is not None
        self.num_vectors = 0
        self.num_segments = 0                 # segments submitted as utterances (a WaveTable with a segmenter)

    def _finish_subsegments(self, handle, keep, voiced_rows):
        """Sliding mode: (vectors, spans, offsets) of the utterances ``keep`` (None: all) -- ``Extractor.finish(as_array=True)``.
        ``voiced_rows`` (the host front-end in front of the table route): per utterance None or its voiced frames, through
        which spans counted in selected rows become RAW frame indices, as on the raw routes."""
        vecs, spans, off = self.ex.finish(handle, as_array=True)
        if keep is not None:
            counts = np.diff(off)[keep]
            src = np.repeat(off[:-1][keep] - (np.cumsum(counts) - counts), counts) + np.arange(int(counts.sum()), dtype=np.int64)
            vecs, spans = vecs[src], spans[src]
            off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        if voiced_rows is not None:
            for i, rows in enumerate(voiced_rows):
                if rows is not None and off[i + 1] > off[i]:
                    sp = spans[off[i]:off[i + 1]]
                    spans[off[i]:off[i + 1]] = np.stack([rows[sp[:, 0]], rows[sp[:, 1] - 1] + 1], axis=1)
        return vecs, spans, off

    def _finish(self, handle, keep=None, shards=None, voiced_rows=None):
        """The vectors of a submitted window: (vectors, valid) of the utterances ``keep`` (None: all), or this rank's share."""
        if self.sliding:
            return self._finish_subsegments(handle, keep, voiced_rows)
        full, valid = self.ex.finish(handle, as_array=True)
        if shards is not None:
            return "shard", shards, full
        return (full, valid) if keep is None else (full[keep], valid[keep])

    def submit_window(self, mats, addrs):
        """-> a zero-argument function returning the vectors of the window (this rank's share of it when world > 1)."""
        if self.world == 1:
            # packed, copied and launched; results are collected later
            return functools.partial(self._finish, self.ex.submit(mats, addrs))
        from . import dist as xdist
        lens = mats.lengths if hasattr(mats, "lengths") else np.array([m.shape[0] for m in mats], np.int64)
        shards = xdist.partition_lpt(lens, self.world)
        mine = engine._Rows(mats, shards[self.rank], lens, addrs)         # (not materialised)
        return functools.partial(self._finish, self.ex.submit(mine, mine.addrs), shards=shards)

    def _segment_utterances(self, recos, tables, row0):
        """The segments of a window's recordings as utterances: (SegmentKeys, first feature row, length).  A segment's key is its id
        in the segments file, else ``subsegment_key(reco, first, end)``; a recording without a segment is warned about and fails."""
        keys, reco_of, first, length, start = [], [], [], [], []
        for reco, (ids, tab), r0 in zip(recos, tables, np.asarray(row0).tolist()):
            if not len(tab):
                self.logger.warning("No segment for recording: '%s'" % reco)
                self.num_fail += 1
                continue
            spans = tab.tolist()
            keys.extend(ids if ids is not None else [subsegment_key(reco, f, f + n) for f, n in spans])
            reco_of.extend([reco] * len(spans))
            first.extend(f for f, _ in spans)
            length.extend(n for _, n in spans)
            start.extend(r0 + f for f, _ in spans)
        self.num_segments += len(keys)
        return SegmentKeys(keys, reco_of, first), np.array(start, np.int64), np.array(length, np.int64)

    def _warn_unvoiced(self, key):
        self.logger.warning("No voiced frames (or VAD / feature length mismatch) for utterance: '%s'" % key)
        self.num_fail += 1

    def submit(self, keys, mats, vads=None, addrs=None):
        """Front-end (optional) + everything up to the kernel launches of one window; returns what ``collect`` needs:
        the keys that go on, their (selected) lengths and a function that yields the vectors."""
        t0 = time.time()
        front, ex = self.front, self.ex
        raw = None
        if isinstance(mats, WaveBatch):
            # a window of a WaveTable: MFCC + VAD on the device, and the extractor reads the rows where they lie
            feats, vad, row0, T, ready = mats.table.compute(mats, self.model.device_model.device)
            if mats.table.segmenter is not None:
                # every segment is an utterance of its own: a row range of its recording, every frame of it counted
                keys, row0, T = self._segment_utterances(keys, mats.table.segments(mats, vad, row0, T, ready), row0)
                vad = None
            raw = ex.submit_device_raw(feats, row0, T, vad, front.cmn_window, front.center, front.min_window, ready)
        elif front is not None and front.cmn_window > 0 and self.world == 1 and hasattr(ex, "submit_raw") and \
                engine._host_lib() is not None and (addrs is not None or engine.can_submit_raw(mats, self.model.device_model.feat_dim)):
            # CMN + voiced-frame selection on the device, scattered straight into the packed batches
            raw = ex.submit_raw(mats, vads, front.cmn_window, front.center, front.min_window, addrs)
        if raw is not None:
            handle, lens, dropped = raw
            keep = None
            if dropped.any():
                for i in np.flatnonzero(dropped).tolist():
                    self._warn_unvoiced(keys[i])
                keep = np.flatnonzero(~dropped)
                keys, lens = [keys[i] for i in keep.tolist()], lens[keep]          # (segments come without a VAD: none is dropped)
            result = functools.partial(self._finish, handle, keep)
        else:
            voiced_rows = None
            if front is not None:
                kept = []
                for i, (key, m) in enumerate(zip(keys, front.apply(mats, vads))):
                    if m is None:      # select-voiced-frames: VAD length mismatch or no voiced frame -> nothing written
                        self._warn_unvoiced(key)
                    else:
                        kept.append((key, m, i))
                if self.sliding and vads is not None:
                    # the spans of the table route count selected rows: the voiced frames they stand for (see _finish_subsegments)
                    voiced_rows = [None if vads[i] is None else np.flatnonzero(np.asarray(vads[i]).reshape(-1) != 0) for _, _, i in kept]
                keys, mats, addrs = [k for k, _, _ in kept], [m for _, m, _ in kept], None
            result = self.submit_window(mats, addrs)
            if voiced_rows is not None:
                result = functools.partial(result.func, *result.args, voiced_rows=voiced_rows)
            lens = mats.lengths if hasattr(mats, "lengths") else np.fromiter((m.shape[0] for m in mats), dtype=np.int64, count=len(mats))
        self.compute_time += time.time() - t0
        return keys, lens, result

    def retire(self, in_flight, reader):
        """Collect the window in flight (if any) and give its arenas back.  They stay out of the pool until the vectors are
        down: finish() may have to pack the window again (out-of-range f16bf8 window -> bf16x3 twin), and it does so from the
        raw addresses."""
        if in_flight is not None:
            self.collect(*in_flight[0])
            reader.recycle(in_flight[1])

    def collect(self, keys, lens, result):
        """Wait for a submitted window and write its vectors (input order)."""
        t0 = time.time()
        out = result()
        self.compute_time += time.time() - t0
        if self.sliding:
            return self.emit_subsegments(keys, lens, *out)
        if len(out) == 3:                     # multi-GPU: this rank's share of the window; exchanged once, at the end
            self.stash.append((keys, lens, out[1], out[2]))
            # XVECTOR_EXCHANGE_WINDOWS=N (default 0 = the single gather at the very end): exchange -- and let rank 0 write --
            # every N windows instead: bounds what a rank holds and what a late failure loses on an endless pipe, at the
            # price of N-th as many collectives.  Every rank sees the same windows, so the counts agree without talking.
            if self.model.exchange_windows > 0 and len(self.stash) >= self.model.exchange_windows:
                self.exchange()
            return
        self.emit(keys, lens, *out)

    def exchange(self):
        """Every rank's stashed vectors to rank 0, which emits them (Model._exchange_shards)."""
        from . import dist as xdist
        xdist.wait_process_group()
        self.model._exchange_shards(self.stash, self.rank, self.world, self.min_chunk_size, self.chunk_size, self.emit)
        del self.stash[:]

    def _warn_rejected(self, keys, lens, valid):
        for i in np.flatnonzero(~valid).tolist():
            if lens[i] == 0:
                self.logger.warning("Zero-length utterance: '%s'" % keys[i])
            else:
                self.logger.warning("Minimum chunk size of %d is greater than the number of rows in utterance: %s" %
                                    (self.min_chunk_size, keys[i]))
        self.num_fail += int((~valid).sum())

    def emit_subsegments(self, keys, lens, vecs, spans, offsets):
        """``emit`` in sliding mode: the same warnings; sub-segment k of ``<utt>`` goes out under ``subsegment_key(utt, first, end)``
        of its span (strictly increasing ``first`` within an utterance: unique and sorted), with its line of the subsegments file."""
        counts = np.diff(offsets)
        valid = counts > 0
        if not valid.all():
            self._warn_rejected(keys, lens, valid)
        if isinstance(keys, SegmentKeys):
            # a window's span counts frames of its segment: recording-relative by the segment's first frame, under the recording's key
            utts = [k for k, c in zip(keys.reco, counts.tolist()) for _ in range(c)]
            spans = spans + np.repeat(keys.first, counts).astype(spans.dtype)[:, None]
        else:
            utts = [k for k, c in zip(keys, counts.tolist()) for _ in range(c)]
        out_keys = [subsegment_key(u, f, e) for u, (f, e) in zip(utts, spans.tolist())]
        self.writer.put(out_keys, vecs, (utts, spans))
        self.num_success += int(valid.sum())
        self.num_vectors += len(out_keys)

    def emit(self, keys, lens, vecs, valid):
        """Warn about rejected utterances, hand the rest to the writer thread."""
        if not valid.all():
            self._warn_rejected(keys, lens, valid)
            keys = [k for k, ok in zip(keys, valid.tolist()) if ok]
            vecs = vecs[valid]
        self.writer.put(keys, vecs)             # written by the writer thread, in order
        self.num_success += len(keys)
