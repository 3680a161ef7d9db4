"""NumPy restatement of the row-plan kernels (xv_voiced_rank_i32, xv_chunk_row_plan_i32 of csrc/xv_rowplan.hip), written from
include/xvector_hip.h: per utterance and per frame, no attempt at speed."""
import numpy as np


def _in_range(s, T, n_frames):
    return s >= 0 and T >= 0 and s + T <= n_frames


def voiced_rank(vad, utt_start, utt_len, n_frames, rank):
    """Writes ``rank`` (int32 [>= n_frames], the caller's initial values stay where nothing is listed) in place and returns the
    voiced counts.  vad: float array or None (every frame voiced)."""
    count = np.zeros(len(utt_start), np.int32)
    for u, (s, T) in enumerate(zip(np.asarray(utt_start, np.int64).tolist(), np.asarray(utt_len, np.int64).tolist())):
        if not _in_range(s, T, n_frames):
            continue
        if vad is None:
            rank[s:s + T] = np.arange(T)
            count[u] = T
            continue
        v = np.asarray(vad[s:s + T]) != 0
        before = np.cumsum(v) - v                           # voiced frames before each frame
        rank[s:s + T] = np.where(v, before, -1)
        count[u] = int(v.sum())
    return count


def chunk_row_plan(rank, utt_start, utt_len, chunk_size, chunks_kept, first_chunk, n_frames, b0, b1, row_start, dst_row):
    """Writes ``dst_row`` (int32 [>= n_frames]) in place for the listed utterances."""
    for i, (s, T) in enumerate(zip(np.asarray(utt_start, np.int64).tolist(), np.asarray(utt_len, np.int64).tolist())):
        if not _in_range(s, T, n_frames):
            continue
        size, kept, first = int(chunk_size[i]), int(chunks_kept[i]), int(first_chunk[i])
        v = np.asarray(rank[s:s + T], np.int64)
        if size <= 0 or T == 0:
            dst_row[s:s + T] = -1
            continue
        k, r = v // size, v % size
        cid = first + k
        ok = (v >= 0) & (k < kept) & (cid >= b0) & (cid < b1)
        row = np.asarray(row_start, np.int64)[np.where(ok, cid - b0, 0)] if ok.any() else 0
        dst_row[s:s + T] = np.where(ok, row + r, -1)
    return dst_row
