"""NumPy restatements for the sliding-window ("sub-segment") extraction mode, written from the documents and not from the code
under test: the plan from its rule and xv_cmn_sliding_gather_f32 from its header comment
(include/xvector_hip.h).  No GPU, no package import."""
import numpy as np


def plan_loop(n, min_chunk_size, window, period):
    """The sub-segments of an utterance of ``n`` frames, one candidate at a time: None for a rejected utterance."""
    if n == 0 or n < min_chunk_size:
        return None
    out = []
    k = 0
    while True:
        start = k * period
        if k >= 1:
            if not (k - 1) * period + window < n:          # the one before it already reached the end
                break
        length = min(window, n - start)
        if k >= 1 and length < min_chunk_size:             # a short last piece is dropped
            break
        out.append((start, length))
        k += 1
    return out


def cmn_window(t, T, window, center, min_window):
    """[ws, we) of Kaldi's SlidingWindowCmn around frame t of an utterance of T frames."""
    if center:
        ws = t - window // 2
        we = ws + window
    else:
        ws = t - window
        we = t + 1
    if ws < 0:
        we -= ws
        ws = 0
    if not center and we > t:
        we = max(t + 1, min_window)
    if we > T:
        ws -= we - T
        we = T
        if ws < 0:
            ws = 0
    return ws, we


def gather(x, feat_dim, utt_start, utt_len, voiced_count, voiced_row, chunk_utt, chunk_first, chunk_len, chunk_row, cmn_window_frames,
           center, min_window, y):
    """xv_cmn_sliding_gather_f32 on host arrays: x[x_rows, >= feat_dim] float32, y[y_rows, >= feat_dim] float32 is written in place
    (columns [0, feat_dim) of the addressed rows only).  voiced_count / voiced_row both None: every frame is voiced.  Rows the
    header says are skipped are skipped."""
    x64 = np.asarray(x, dtype=np.float64)[:, :feat_dim]
    x_rows, y_rows, n_utts = x.shape[0], y.shape[0], len(utt_start)
    for c in range(len(chunk_utt)):
        u = int(chunk_utt[c])
        if u < 0 or u >= n_utts:
            continue
        base, T = int(utt_start[u]), int(utt_len[u])
        if base < 0 or T <= 0 or base + T > x_rows:
            continue
        count = T if voiced_row is None else int(voiced_count[u])
        for j in range(int(chunk_len[c])):
            v = int(chunk_first[c]) + j
            row = int(chunk_row[c]) + j
            if v < 0 or v >= count or v >= T or row < 0 or row >= y_rows:
                continue
            t = v if voiced_row is None else int(voiced_row[base + v])
            if t < 0 or t >= T:
                continue
            ws, we = cmn_window(t, T, cmn_window_frames, center, min_window)
            mean = x64[base + ws:base + we].sum(axis=0) / float(we - ws)
            y[row, :feat_dim] = (x64[base + t] - mean).astype(np.float32)
    return y


def voiced_lists(vads, utt_start, utt_len, n_rows):
    """What xv_vad_compact_i32 makes of per-utterance VAD vectors: (voiced_count[n_utts], voiced_row[n_rows]) int32, the list of
    utterance u at voiced_row[utt_start[u]:], -1 elsewhere."""
    count = np.zeros(len(vads), np.int32)
    rows = np.full(n_rows, -1, np.int32)
    for u, v in enumerate(vads):
        idx = np.flatnonzero(np.asarray(v)[:utt_len[u]] != 0)
        count[u] = len(idx)
        rows[utt_start[u]:utt_start[u] + len(idx)] = idx
    return count, rows
