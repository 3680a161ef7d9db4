"""Speech segments of a recording: from its VAD decisions -- on the host (``vad_segments_host``, what
``mfcc_vad.py vad-to-segments`` runs) or on the device where the decisions of the ``--wav-rspecifier`` route lie
(``segments_device``: xv_vad_segments_i32) -- or from a Kaldi ``segments`` file (``frames_of_segments``).  A segment is a row range
of its recording's feature rows (the semantics of Kaldi's utils/data/subsegment_data_dir.sh): the extractor takes it as an
utterance of its own, so windows, chunks and the sliding CMN stay inside it.

The rule (this project's own; include/xvector_hip.h holds the contract).  A frame is voiced iff its decision is != 0 (NaN counts as
voiced).  With max_gap G, min_len M, pad P and max_len L, all in frames:
  1. close  a maximal unvoiced run [a, b) with a > 0, b < T and b - a <= G becomes voiced;
  2. drop   of the maximal voiced runs of the result, those with b - a >= M are kept;
  3. pad    a kept run becomes [max(a - P, 0), min(b + P, T));
  4. split  a run of n > L frames (L > 0) becomes k = ceil(n / L) pieces [a + floor(i n / k), a + floor((i + 1) n / k)).
"""
import numpy as np


class SegmentOptions(object):
    """The parameters of the rule, in frames."""

    def __init__(self, max_gap=30, min_len=50, pad=10, max_len=1000):
        self.max_gap, self.min_len, self.pad, self.max_len = int(max_gap), int(min_len), int(pad), int(max_len)

    def check(self):
        """ValueError unless max_gap >= 0, min_len >= 1, pad >= 0 with 2 pad <= max_gap, and max_len is 0 or >= 2 min_len."""
        if self.max_gap < 0:
            raise ValueError("segment max_gap %d is negative" % self.max_gap)
        if self.min_len < 1:
            raise ValueError("segment min_len %d is not positive" % self.min_len)
        if self.pad < 0 or 2 * self.pad > self.max_gap:
            raise ValueError("segment pad %d must lie in [0, max_gap / 2] (max_gap %d): padded segments could touch" % (self.pad, self.max_gap))
        if self.max_len != 0 and self.max_len < 2 * self.min_len:
            raise ValueError("segment max_len %d must be 0 (no splitting) or at least twice min_len %d: a piece could fall below min_len"
                             % (self.max_len, self.min_len))
        return self

    def capacity(self, T):
        """The most segments an utterance of T frames can have: (T + G + 1) / (M + G + 1) + (L ? T / L : 0), integer division."""
        T = int(T)
        return (T + self.max_gap + 1) // (self.min_len + self.max_gap + 1) + (T // self.max_len if self.max_len else 0)


_EMPTY = np.zeros((0, 2), np.int32)


def vad_segments_host(v, opts):
    """The segments of one utterance with decisions ``v``: int32 [n, 2] of (first frame, length), in increasing order.  The NumPy
    twin of xv_vad_segments_i32, run over the voiced frames: a run ends where the next voiced frame is more than max_gap + 1 away."""
    v = np.asarray(v).reshape(-1)
    T = len(v)
    idx = np.flatnonzero(v != 0)
    if not len(idx):
        return _EMPTY.copy()
    brk = np.flatnonzero(np.diff(idx) - 1 > opts.max_gap)
    a = idx[np.concatenate([[0], brk + 1])]
    b = idx[np.concatenate([brk, [len(idx) - 1]])] + 1
    keep = b - a >= opts.min_len
    a, b = np.maximum(a[keep] - opts.pad, 0), np.minimum(b[keep] + opts.pad, T)
    n = (b - a).astype(np.int64)
    k = np.ones(len(n), np.int64)
    if opts.max_len > 0:
        k = np.where(n > opts.max_len, -(-n // opts.max_len), 1)
    run = np.repeat(np.arange(len(n)), k)
    i = np.arange(int(k.sum()), dtype=np.int64) - np.repeat(np.cumsum(k) - k, k)
    lo, hi = i * n[run] // k[run], (i + 1) * n[run] // k[run]
    return np.stack([a[run] + lo, hi - lo], axis=1).astype(np.int32)


_PINNED = []


def _pinned_i32(torch, n):
    """A pinned int32 host tensor of at least n elements, kept for the next call (the caller is done with it when it returns)."""
    if not _PINNED or _PINNED[0].numel() < n:
        size = 1024
        while size < n:
            size *= 2
        _PINNED[:] = [torch.empty(size, dtype=torch.int32).pin_memory()]
    return _PINNED[0]


def segments_device(vad, row0, T, opts, stream=None, ready=None):
    """The segments of the utterances at rows row0[u] .. row0[u] + T[u] - 1 of ``vad`` (cuda float32, e.g. ``Mfcc.compute_device``'s;
    row0 / T: host integer arrays), made where the decisions lie: one launch of xv_vad_segments_i32 with every utterance's table
    sized by ``hiplib.vad_segments_capacity``, then ONE download of the counts and the tables together through a pinned buffer.
    Both run on ``stream`` (None: the current one) behind the event ``ready``; the call returns when the table is down.
    -> one int32 [n, 2] array of (first frame, length) per utterance.  RuntimeError when a count exceeds its capacity."""
    import torch
    from . import hiplib
    opts.check()
    row0 = np.asarray(row0, np.int64).reshape(-1)
    T = np.asarray(T, np.int64).reshape(-1)
    n = len(T)
    if n == 0:
        return []
    assert len(row0) == n and int(T.max()) < 2 ** 31 and vad.numel() < 2 ** 31
    cap = np.array([hiplib.vad_segments_capacity(t, opts.max_gap, opts.min_len, opts.max_len) for t in T.tolist()], np.int64)
    off = np.zeros(n, np.int64)
    np.cumsum(cap[:-1], out=off[1:])
    slots = int(cap.sum())
    assert slots < 2 ** 31
    dev = vad.device
    with torch.cuda.device(dev), torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(dev)):
        s = torch.cuda.current_stream()
        if ready is not None:
            s.wait_event(ready)
        host = _pinned_i32(torch, max(4 * n, n + 2 * slots))
        up = host[:4 * n].view(4, n)
        up.numpy()[:] = np.stack([row0, T, off, cap])
        tab = up.to(dev, non_blocking=True)
        out = torch.empty(n + 2 * max(slots, 1), dtype=torch.int32, device=dev)
        count_d, first_d, len_d = out[:n], out[n:n + max(slots, 1)], out[n + max(slots, 1):]
        hiplib.vad_segments(vad, tab[0], tab[1], opts.max_gap, opts.min_len, opts.pad, opts.max_len, tab[2], tab[3],
                            count_d, first_d, len_d)
        down = host[:out.numel()]
        down.copy_(out, non_blocking=True)            # (behind the upload on the same stream: the pinned words are free again)
        done = torch.cuda.Event()
        done.record(s)
        done.synchronize()
        res = down.numpy().copy()
    count, first, length = res[:n], res[n:n + max(slots, 1)], res[n + max(slots, 1):]
    over = np.flatnonzero(count > cap)
    if len(over):
        u = int(over[0])
        raise RuntimeError("vad segments: utterance %d of %d frames has %d segments, above the capacity %d of its table"
                           % (u, T[u], count[u], cap[u]))
    return [np.stack([first[o:o + c], length[o:o + c]], axis=1) for o, c in zip(off.tolist(), count.tolist())]


def frames_of_segments(lines, T_of, shift_ms):
    """The segments of an external ``segments`` file in frames.  ``lines``: (seg-id, recording, start ms, end ms) tuples as
    ``plda_backend.read_segments`` returns them; ``T_of``: {recording: frames}; ``shift_ms``: milliseconds per frame.
    first = floor(start / shift + 0.5), end = min(floor(end / shift + 0.5), T).  A segment with first >= T or end <= first is skipped
    and counted, and so is a line whose recording ``T_of`` does not hold.  The segments of a recording are taken in (first, end)
    order; two that overlap in frames are a ValueError naming both.
    -> ({recording: (seg-ids, int32 [n, 2] of (first, length))}, number skipped as empty, number of unknown recording)."""
    shift = float(shift_ms)
    per, n_empty, n_unknown = {}, 0, 0
    for key, reco, t0, t1 in lines:
        if reco not in T_of:
            n_unknown += 1
            continue
        T = int(T_of[reco])
        first = int(np.floor(t0 / shift + 0.5))
        end = min(int(np.floor(t1 / shift + 0.5)), T)
        if first >= T or end <= first:
            n_empty += 1
            continue
        per.setdefault(reco, []).append((first, end, key))
    out = {}
    for reco, segs in per.items():
        segs.sort(key=lambda s: (s[0], s[1]))
        for (f0, e0, k0), (f1, e1, k1) in zip(segs, segs[1:]):
            if f1 < e0:
                raise ValueError("segments %s (frames [%d, %d)) and %s (frames [%d, %d)) of recording %s overlap"
                                 % (k0, f0, e0, k1, f1, e1, reco))
        out[reco] = ([k for _, _, k in segs], np.array([[f, e - f] for f, e, _ in segs], np.int32).reshape(-1, 2))
    return out, n_empty, n_unknown


class VadSegmenter(object):
    """The segmenter of ``--segment-by-vad`` (``extract_stream.WaveTable``): per window, ``segments_device`` of its decisions."""
    skipped = 0

    def __init__(self, opts):
        self.opts = opts.check()

    def tables(self, keys, vad, row0, T, shift_ms, stream, ready):
        """-> per recording (None, int32 [n, 2]): the segments carry no ids of their own."""
        return [(None, t) for t in segments_device(vad, row0, T, self.opts, stream, ready)]

    def unknown(self):
        return 0


class FileSegmenter(object):
    """The segmenter of ``--segments FILE``: the file's lines, grouped by recording; a window takes those of its recordings."""
    def __init__(self, lines):
        self.by_reco, self.skipped, self._seen = {}, 0, set()
        for ln in lines:
            self.by_reco.setdefault(ln[1], []).append(ln)

    def tables(self, keys, vad, row0, T, shift_ms, stream, ready):
        """-> per recording (seg-ids, int32 [n, 2]) from ``frames_of_segments`` (ValueError on an overlap)."""
        lines = [ln for k in keys for ln in self.by_reco.get(k, ())]
        self._seen.update(keys)
        per, n_empty, _ = frames_of_segments(lines, dict(zip(keys, np.asarray(T).tolist())), shift_ms)
        self.skipped += n_empty
        return [per.get(k, ([], _EMPTY)) for k in keys]

    def unknown(self):
        """Lines whose recording no window has brought (after the run: the recordings wav.scp does not hold)."""
        return sum(len(v) for k, v in self.by_reco.items() if k not in self._seen)
