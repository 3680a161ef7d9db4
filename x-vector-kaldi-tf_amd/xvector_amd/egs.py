"""Training examples from raw features: stages 3-5 of the recipe without Kaldi binaries.

The reference builds the egs directory its trainer reads in three steps:

* ``run.sh`` stage 3 pipes every utterance through ``apply-cmvn-sliding | select-voiced-frames``, writes the result as a second copy
  of all features, and keeps utterances with more than 500 frames left and speakers with at least 8 such utterances
  (``run.sh:199-215``);
* ``local/tf/get_egs.sh`` calls ``create_egs.py``, which deals chunks of those utterances to minibatches and archives
  (``temp/ranges.<n>``, first frame and length in the numbering of the copy);
* ``create_tar_files.py`` cuts the chunks, casts them to float16 and writes ``egs.<n>.tar`` + ``egs.<n>.npy``.

Here the copy is never made.  ``voiced_counts`` / ``filter_utterances`` give the utterance lengths after silence removal from
``vad.scp`` alone; ``allocate`` restates the allocation the reference actually runs (``our_splitting_per_archive``) call for call on
Python's ``random`` stream, so the same inputs and seed give byte-identical files; ``EgsWriter`` reads the RAW rows and VAD vectors of
the utterances an archive names and has the device cut, normalise and cast its chunks (``xv_vad_compact_i32``,
``xv_egs_chunks_f16``) before one copy back and ``examples_io.write_egs_tar``.
"""
import math
import os
import random
import struct
from collections import OrderedDict

import numpy as np

from . import hiplib

__all__ = ["read_pairs", "feat_lengths", "voiced_counts", "filter_utterances", "allocate", "AllocationError", "parse_ranges",
           "DeviceGather", "EgsWriter"]


# ------------------------------------------------------------------------------------------------
# stage 3 without writing features
# ------------------------------------------------------------------------------------------------
def read_pairs(path):
    """``key value`` lines of a Kaldi text table (utt2spk, an scp, utt2num_frames) -> list of (key, value) in file order."""
    out = []
    with open(path, "rt") as fid:
        for line in fid:
            f = line.split(None, 1)
            if len(f) == 2:
                out.append((f[0], f[1].strip()))
    return out


def _dims_at(fd):
    """(rows, cols) of the binary matrix record at the stream position (FM / DM / CM / CM2 / CM3): the header only."""
    if fd.read(2) != b"\x00B":
        return None
    tag = fd.read(3)
    if tag in (b"FM ", b"DM "):
        _, rows, _, cols = struct.unpack("<bibi", fd.read(10))
        return rows, cols
    if tag[:2] == b"CM":
        if tag != b"CM ":
            fd.read(1)
        hdr = fd.read(16)
        rows, cols = struct.unpack("<ii", hdr[8:])
        return rows, cols
    return None


def feat_lengths(feats_scp):
    """key -> (frames, dim) for every entry of a feats.scp, from the record headers (no matrix is read unless an entry is a pipe
    or a text matrix)."""
    import kaldi_io
    out, handles = OrderedDict(), {}
    try:
        for key, rx in read_pairs(feats_scp):
            m = kaldi_io._RX_OFFSET.match(rx)
            dims = None
            if m is not None and not rx.endswith("|"):
                path = m.group(1)
                fd = handles.get(path)
                if fd is None:
                    if len(handles) >= 64:
                        handles.popitem()[1].close()
                    fd = handles[path] = open(path, "rb")
                fd.seek(int(m.group(2)))
                dims = _dims_at(fd)
            if dims is None:
                dims = kaldi_io.read_mat(rx).shape
            out[key] = (int(dims[0]), int(dims[1]))
    finally:
        for fd in handles.values():
            fd.close()
    return out


def voiced_counts(vad_scp):
    """key -> (voiced frames, frames) for every entry of a vad.scp, in its order: the utt2num_frames of the no-silence set."""
    import kaldi_io
    out = OrderedDict()
    for keys, vals, off in kaldi_io.VecScp(vad_scp).blocks():
        off = np.asarray(off, np.int64)
        nz = np.concatenate([[0], np.cumsum(np.asarray(vals).reshape(-1) != 0, dtype=np.int64)])
        cnt = nz[off[1:]] - nz[off[:-1]]
        for k, c, n in zip(keys, cnt.tolist(), np.diff(off).tolist()):
            out[k] = (int(c), int(n))
    return out


def filter_utterances(utt2spk, voiced, lengths=None, min_len=500, min_num_utts=8):
    """Stage 3's selection.  ``utt2spk``: list of (utt, spk); ``voiced``: utt -> (voiced frames, VAD length) (voiced_counts);
    ``lengths``: utt -> (frames, dim) of the features (feat_lengths), None = do not compare.  An utterance without a VAD, with a VAD
    whose length differs from its features or without a voiced frame has no no-silence features (select-voiced-frames writes
    nothing for it); of the others those with MORE than ``min_len`` voiced frames stay, then the speakers with AT LEAST
    ``min_num_utts`` of them (run.sh:199-215).  Returns (utt2spk, spk2utt, utt2num_frames) as sorted lists of (utt, spk),
    (spk, [utts]) and (utt, frames), the order fix_data_dir.sh leaves."""
    kept = {}
    for utt, spk in utt2spk:
        v = voiced.get(utt)
        if v is None or v[0] <= 0:
            continue
        if lengths is not None and (utt not in lengths or lengths[utt][0] != v[1]):
            continue
        if v[0] > min_len:
            kept[utt] = (spk, v[0])
    by_spk = {}
    for utt in sorted(kept):
        by_spk.setdefault(kept[utt][0], []).append(utt)
    spk2utt = [(spk, by_spk[spk]) for spk in sorted(by_spk) if len(by_spk[spk]) >= min_num_utts]
    utt2spk_out = sorted((utt, spk) for spk, utts in spk2utt for utt in utts)
    utt2num_frames = [(utt, kept[utt][1]) for utt, _ in utt2spk_out]
    return utt2spk_out, spk2utt, utt2num_frames


# ------------------------------------------------------------------------------------------------
# stage 4: allocation of chunks to minibatches and archives
# ------------------------------------------------------------------------------------------------
class AllocationError(ValueError):
    pass


def _offset_lists(utt2len):
    """One list of (offset, length) per utterance, SHARED between an utterance and the copies named <utterance>-<suffix> (its
    augmented versions) when the utterance itself is in the table: their chunks are kept apart as if they were one recording."""
    lists = {}
    for key in utt2len:
        cut = key.rfind("-")
        base = key[:cut] if cut > 0 and key[:cut] in utt2len else key
        if base not in lists:
            lists[base] = []
        lists[key] = lists[base]
    return lists


def _geometric_length(archive, num_archives, lo, hi):
    if hi == lo:
        return hi
    if num_archives == 1:
        return int(hi)
    return int(math.pow(float(hi) / lo, float(archive) / (num_archives - 1)) * lo + 0.5)


def allocate(utt2len, utt2int, egs_dir, prefix="", num_repeats=10, min_frames_per_chunk=50, max_frames_per_chunk=300,
             randomize_chunk_length=True, frames_per_iter=1000000, num_archives=-1, num_jobs=-1, seed=123, num_pdfs=-1,
             accepted_overlap=0.2, minibatch_size=128):
    """What the reference's create_egs.py runs.  ``utt2len`` / ``utt2int``: lists of (utt, frames) / (utt, speaker label) in file
    order (the order decides the draws).  Writes ``temp/<prefix_>ranges.<n>`` (one per archive; lines ``utt minibatch slot first
    frames label``, sorted), ``temp/<prefix_>archive_minibatch_count``, ``temp/<prefix_>outputs.<job>`` and ``<prefix_>pdf2num``;
    returns the minibatch count of every archive.

    Per archive: every speaker ``num_repeats`` times, shuffled; a minibatch draws its chunk length, then for each of its slots takes
    the next speaker, draws one of its utterances WITHOUT replacement (the speaker's list is refilled when one or none is left, the
    draw still being made from the old list), draws again while the utterance is shorter than the chunk, and draws an offset that
    overlaps the chunks already taken from the same recording by at most ``accepted_overlap``, giving up after
    ``len / chunk + 1`` retries (a float).  Same calls to ``random`` in the same order as the reference, hence the same files.

    One deviation: a speaker none of whose utterances is as long as the drawn chunk makes the reference draw for ever; here that
    raises AllocationError naming the speaker (checked without a draw)."""
    if num_repeats < 1:
        raise ValueError("--num-repeats should have a minimum value of 1")
    if min_frames_per_chunk <= 1:
        raise ValueError("--min-frames-per-chunk is invalid.")
    if max_frames_per_chunk < min_frames_per_chunk:
        raise ValueError("--max-frames-per-chunk is invalid.")
    if frames_per_iter < 1000:
        raise ValueError("--frames-per-iter is invalid.")
    if num_archives < 1:
        raise ValueError("--num-archives is invalid")
    if num_jobs > num_archives:
        raise ValueError("--num-jobs is invalid (must not exceed num-archives)")
    if num_jobs < 1:
        raise ValueError("--num-jobs is invalid")
    rng = random.Random(seed)                       # the stream random.seed(seed) + the module's functions would give
    utt2len = OrderedDict((k, int(v)) for k, v in utt2len)
    spk2utt, utt2spk = OrderedDict(), {}
    for utt, spk in utt2int:
        spk = int(spk)
        utt2spk[utt] = spk
        spk2utt.setdefault(spk, []).append(utt)
    if num_pdfs == -1:
        num_pdfs = max(spk2utt) + 1
    if prefix:
        prefix = prefix + "_"
    temp = os.path.join(egs_dir, "temp")
    os.makedirs(temp, exist_ok=True)
    longest = dict((spk, max(utt2len[u] for u in utts)) for spk, utts in spk2utt.items())
    left = dict((spk, list(utts)) for spk, utts in spk2utt.items())
    offsets = _offset_lists(utt2len)
    pdf2num, counts = {}, []

    def draw_utterance(spk):
        utts = left[spk]
        n = len(utts)
        if n <= 1:
            left[spk] = list(spk2utt[spk])
        return utts.pop(rng.randint(0, n - 1))

    def overlap_ok(offset, taken, length):
        for pre_offset, pre_length in taken:
            span = length if offset < pre_offset else pre_length
            if abs(pre_offset - offset) * 1.0 / span < (1 - accepted_overlap):
                return False
        return True

    with open(os.path.join(temp, prefix + "archive_minibatch_count"), "w") as info:
        for archive in range(num_archives):
            egs = []
            spkrs = num_repeats * list(spk2utt.keys())
            rng.shuffle(spkrs)
            for taken in offsets.values():
                del taken[:]
            total, minibatch = 0, 0
            while total < frames_per_iter:
                if len(spkrs) < minibatch_size:             # "Ran out of speakers"
                    break
                if randomize_chunk_length:
                    length = rng.randint(min_frames_per_chunk, max_frames_per_chunk)
                else:
                    length = _geometric_length(archive, num_archives, min_frames_per_chunk, max_frames_per_chunk)
                for slot in range(minibatch_size):
                    spk = spkrs.pop()
                    if longest[spk] < length:
                        raise AllocationError("speaker %d has no utterance of %d frames (its longest has %d): the reference would "
                                              "draw for ever; lower --max-frames-per-chunk or drop the speaker" % (spk, length, longest[spk]))
                    while True:
                        utt = draw_utterance(spk)
                        utt_len = utt2len[utt]
                        if utt_len >= length:
                            break
                    free = utt_len - length
                    tries = utt_len / length + 1
                    taken = offsets[utt]
                    offset = rng.randint(0, free)
                    while tries > 0 and not overlap_ok(offset, taken, length):
                        offset = rng.randint(0, free)
                        tries -= 1
                    taken.append((offset, length))
                    egs.append((utt, minibatch, slot, offset, length))
                    total += length
                minibatch += 1
            info.write("%d %d\n" % (archive + 1, minibatch))
            counts.append(minibatch)
            with open(os.path.join(temp, prefix + "ranges.%d" % (archive + 1)), "w") as f:
                for utt, mb, slot, offset, length in sorted(egs):
                    f.write("%s %d %d %d %d %d\n" % (utt, mb, slot, offset, length, utt2spk[utt]))
                    pdf2num[utt2spk[utt]] = pdf2num.get(utt2spk[utt], 0) + 1
    for job in range(num_jobs):
        with open(os.path.join(temp, prefix + "outputs.%d" % (job + 1)), "w") as f:
            f.write("\n".join("%segs.%d.tar" % (prefix, n + 1) for n in range(job, num_archives, num_jobs)) + "\n")
    with open(os.path.join(egs_dir, prefix + "pdf2num"), "w") as f:
        f.write(" ".join(str(pdf2num.get(k, 0)) for k in range(num_pdfs)) + "\n")
    return counts


# ------------------------------------------------------------------------------------------------
# stage 5: cutting the chunks
# ------------------------------------------------------------------------------------------------
def parse_ranges(ranges_file, minibatch_count, minibatch_size):
    """-> (chunks: utt -> [(minibatch, first, frames, label)] in file order, length of every minibatch).  The checks of
    examples_io.RangesDataLoader: one chunk length per minibatch, exactly ``minibatch_size`` chunks in each."""
    chunks, length, total = OrderedDict(), [None] * minibatch_count, [0] * minibatch_count
    with open(ranges_file, "rt") as fid:
        for line in fid:
            f = line.split()
            if not f:
                continue
            mb, first, n, label = int(f[1]), int(f[3]), int(f[4]), int(f[5])
            if not 0 <= mb < minibatch_count:
                raise ValueError("%s: minibatch %d outside [0, %d)" % (ranges_file, mb, minibatch_count))
            chunks.setdefault(f[0], []).append((mb, first, n, label))
            if length[mb] is None:
                length[mb] = n
            if length[mb] != n:
                raise ValueError("%s: minibatch %d mixes chunk lengths %d and %d" % (ranges_file, mb, length[mb], n))
            total[mb] += 1
    for mb in range(minibatch_count):
        if length[mb] is None or total[mb] != minibatch_size:
            raise ValueError("%s: minibatch %d holds %d chunks, expected %d" % (ranges_file, mb, total[mb], minibatch_size))
    return chunks, length


class DeviceGather(object):
    """The gather step of EgsWriter on the MI355X.  ``alloc(n)`` -> the archive's buffer of n halves on the device;
    ``gather(y, feats, vad, utt_start, utt_len, table)`` uploads one window of raw rows + VAD values, builds the voiced index
    (xv_vad_compact_i32), checks ``table`` against the counts and cuts its chunks into y (xv_egs_chunks_f16), returning the voiced
    counts; ``fetch(y)`` -> the buffer as a host float16 array (the one copy back)."""

    def __init__(self, device="cuda:0", cmn_window=300, center=True, min_window=100):
        import torch
        hiplib.require_gpu()
        self.torch, self.device = torch, torch.device(device)
        self.cmn_window, self.center, self.min_window = int(cmn_window), bool(center), int(min_window)

    def alloc(self, n):
        return self.torch.zeros(int(n), dtype=self.torch.float16, device=self.device)

    def __call__(self, y, feats, vad, utt_start, utt_len, table):
        torch = self.torch
        with torch.cuda.device(self.device):
            x = torch.from_numpy(np.ascontiguousarray(feats, np.float32)).to(self.device)
            v = torch.from_numpy(np.ascontiguousarray(vad, np.float32)).to(self.device)
            us = torch.from_numpy(np.ascontiguousarray(utt_start, np.int32)).to(self.device)
            ul = torch.from_numpy(np.ascontiguousarray(utt_len, np.int32)).to(self.device)
            count, rows = hiplib.vad_compact(v, us, ul)
            counts = count.cpu().numpy()
            hiplib.egs_chunks(x, us, ul, count, rows, table, counts, self.cmn_window, self.center, self.min_window, y)
        return counts

    def fetch(self, y):
        return y.cpu().numpy()


class EgsWriter(object):
    """create_tar_files.py for one job, from RAW features.  ``write_job(outputs_file)`` seeds NumPy's legacy stream once
    (``random_seed`` != 0) and, for every archive the file names, in file order, draws one ``permutation(arange(count))`` (drawn
    whether or not the archive already exists, as the reference does), writes ``<egs_dir>/<name>`` through ``<name>.tmp.tar`` + rename
    unless it exists, and ``<name minus .tar>.npy`` with the labels permuted alike.

    An archive: ``temp/<prefix_>ranges.<n>`` names utterances and chunks; the utterances are read from ``feats_scp`` (RAW rows) and
    ``vad_scp`` in feats.scp order, in windows of about ``frame_budget`` raw frames; ``gather`` (DeviceGather, or any object with its
    three calls) cuts each window's chunks into the archive's buffer, which comes back once.  Slot order inside a minibatch is
    RangesDataLoader's: utterances in scp order, within an utterance ranges-file order."""

    def __init__(self, egs_dir, feats_scp, vad_scp, feature_dim, minibatch_size, prefix="", shuffle=True, random_seed=0, gather=None,
                 cmn_window=300, center=True, min_window=100, frame_budget=4000000, logger=None):
        self.egs_dir, self.feature_dim, self.minibatch_size = egs_dir, int(feature_dim), int(minibatch_size)
        self.prefix = prefix + "_" if prefix else ""
        self.shuffle, self.random_seed, self.frame_budget, self.logger = bool(shuffle), int(random_seed), int(frame_budget), logger
        self.gather = gather if gather is not None else DeviceGather("cuda:0", cmn_window, center, min_window)
        self.feats = read_pairs(feats_scp)
        self.vads = dict(read_pairs(vad_scp))
        self.counts = {}
        with open(os.path.join(egs_dir, "temp", self.prefix + "archive_minibatch_count"), "rt") as fid:
            for f in (line.split() for line in fid):
                if f:
                    self.counts[int(f[0])] = int(f[1])
        self.stats = dict(archives=0, frames_in=0, frames_out=0)

    def _info(self, msg):
        if self.logger is not None:
            self.logger.info(msg)

    def write_job(self, outputs_file):
        from examples_io import write_egs_tar
        rs = np.random.RandomState(self.random_seed) if self.random_seed != 0 else np.random
        written = []
        with open(outputs_file, "rt") as fid:
            names = [line.strip() for line in fid if len(line.strip()) > 1]
        for name in names:
            tar_path = os.path.join(self.egs_dir, name)
            idx = int(tar_path.split(".")[-2])
            count = self.counts[idx]
            order = rs.permutation(np.arange(count)) if self.shuffle else np.arange(count)
            npy_path = tar_path[:-4] + ".npy"
            if os.path.exists(tar_path) and os.path.exists(npy_path):
                self._info("Output file {%s} exist from before." % tar_path)
                continue
            members, labels = self.cut_archive(idx)
            labels = labels[order]
            if not os.path.exists(tar_path):
                self._info("Processing file {%s}" % tar_path)
                tmp = tar_path + ".tmp.tar"
                write_egs_tar(tmp, [members[i] for i in order], labels)          # (writes <tmp minus .tar>.npy too)
                os.rename(tmp, tar_path)
                os.remove(tmp[:-4] + ".npy")
                written.append(tar_path)
            if not os.path.exists(npy_path):
                tmp = npy_path + ".tmp.npy"
                np.save(tmp, labels)
                os.rename(tmp, npy_path)
        return written

    def cut_archive(self, idx):
        """-> (members: list of float16 [B, T_i, F] in minibatch order, labels int32 [count, B]) of archive ``idx``."""
        import kaldi_io
        B, F, count = self.minibatch_size, self.feature_dim, self.counts[idx]
        chunks, length = parse_ranges(os.path.join(self.egs_dir, "temp", "%sranges.%d" % (self.prefix, idx)), count, B)
        sizes = np.array([B * n * F for n in length], np.int64)
        member_off = np.concatenate([[0], np.cumsum(sizes)])
        y = self.gather.alloc(int(member_off[-1]))
        labels = np.zeros((count, B), np.int32)
        filled = [0] * count
        lines = ["%s %s" % (k, rx) for k, rx in self.feats if k in chunks]
        missing = set(chunks) - set(k for k, _ in self.feats)
        if missing:
            raise ValueError("ranges.%d names %d utterances feats.scp does not list (e.g. %s)" % (idx, len(missing), sorted(missing)[0]))
        window, frames = [], 0

        def flush():
            keys = [k for ks, _, _ in window for k in ks]
            feats = window[0][1] if len(window) == 1 else np.concatenate([m for _, m, _ in window], axis=0)
            lens = np.concatenate([np.diff(np.asarray(o, np.int64)) for _, _, o in window])
            if feats.shape[1] != F:
                raise ValueError("feature dimension %d of %s differs from --feature-dim %d" % (feats.shape[1], keys[0], F))
            starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
            try:
                vlines = ["%s %s" % (k, self.vads[k]) for k in keys]
            except KeyError as e:
                raise ValueError("vad.scp has no entry for %s" % e.args[0])
            vparts, vlens = [], []
            for _, vals, off in kaldi_io.VecScp(vlines).blocks():
                vparts.append(np.asarray(vals, np.float32).reshape(-1))
                vlens.append(np.diff(np.asarray(off, np.int64)))
            vlens = np.concatenate(vlens)
            if len(vlens) != len(lens) or (vlens != lens).any():
                bad = keys[int(np.flatnonzero(vlens != lens)[0])] if len(vlens) == len(lens) else keys[0]
                raise ValueError("the VAD of %s does not have the length of its features" % bad)
            cu, cf, cl, cd = [], [], [], []
            for u, k in enumerate(keys):
                for mb, first, n, label in chunks[k]:
                    slot = filled[mb]
                    filled[mb] += 1
                    labels[mb, slot] = label
                    cu.append(u); cf.append(first); cl.append(n)
                    cd.append(int(member_off[mb]) + slot * n * F)
            table = (np.array(cu, np.int32), np.array(cf, np.int32), np.array(cl, np.int32), np.array(cd, np.int64))
            self.gather(y, feats, np.concatenate(vparts) if vparts else np.zeros(0, np.float32), starts, lens, table)
            self.stats["frames_in"] += int(lens.sum())
            del window[:]

        for keys, feats, off in kaldi_io.MatScp(lines).blocks():
            off = np.asarray(off, np.int64)
            i = 0
            while i < len(keys):                            # the reader's block, cut where the window reaches its budget
                j = int(np.searchsorted(off, off[i] + max(self.frame_budget - frames, 1), side="left"))
                j = min(max(j, i + 1), len(keys))
                window.append((list(keys[i:j]), np.array(feats[int(off[i]):int(off[j])], np.float32), off[i:j + 1] - off[i]))
                frames += int(off[j] - off[i])
                i = j
                if frames >= self.frame_budget:
                    flush()
                    frames = 0
        if window:
            flush()
        assert all(n == B for n in filled)
        host = self.gather.fetch(y)
        members = [host[int(member_off[mb]):int(member_off[mb + 1])].reshape(B, length[mb], F) for mb in range(count)]
        self.stats["archives"] += 1
        self.stats["frames_out"] += int(member_off[-1]) // F
        return members, labels
