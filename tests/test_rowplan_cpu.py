"""The row plan of the wav.scp -> x-vector route without a GPU: the NumPy restatement of the two kernels (tests/rowplan_ref.py)
against the host function they replace (xv_raw_row_plan of libxvector_host.so), and the property the extractor relies on -- over
the batches of a window every row of every kept chunk receives exactly one frame."""
import numpy as np
import pytest

import rowplan_ref


def _scattered_spans(rng, T, slack=3):
    """Feature rows of utterances of T frames listed in shuffled order with gaps between them: (utt_start, n_frames)."""
    order = rng.permutation(len(T))
    start = np.zeros(len(T), np.int64)
    at = int(rng.integers(0, slack + 1))
    for u in order.tolist():
        start[u] = at
        at += int(T[u]) + int(rng.integers(0, slack + 1))
    return start, at


def test_restatement_equals_the_host_row_plan():
    """rank + chunk_row_plan, indexed by feature row, give what xv_raw_row_plan gives at the running offset of the same frame:
    random utterances with and without VAD, random chunk sizes, kept counts that drop tails, [b0, b1) cutting the chunk list."""
    from xvector_amd import engine, hiplib
    assert hiplib.ABI_VERSION >= 36 and {"xv_voiced_rank_i32", "xv_chunk_row_plan_i32"} <= set(hiplib.SYMBOLS)
    lib = engine._host_lib()
    if lib is None:
        pytest.skip("host library not built")
    rng = np.random.default_rng(36)
    for trial in range(60):
        nU = int(rng.integers(1, 40))
        T = rng.integers(0, 300, nU).astype(np.int64)
        with_vad = trial % 3 != 0
        off = np.zeros(nU, np.int64)                         # the running offset of the host function = the flags' offset
        np.cumsum(T[:-1], out=off[1:])
        total = int(T.sum())
        voiced = (rng.random(total) < rng.choice([0.0, 0.2, 0.8, 1.0])) if with_vad else None
        V = np.array([voiced[o:o + t].sum() for o, t in zip(off, T)], np.int64) if with_vad else T.copy()
        size = rng.integers(-1, 120, nU).astype(np.int64)                                # (<= 0: no chunk of the utterance exists)
        kept = np.minimum(rng.integers(0, 5, nU), -(-V // np.maximum(size, 1))).astype(np.int64)
        seg = np.zeros(nU, np.int64)
        np.cumsum(kept[:-1], out=seg[1:])
        nch = int(kept.sum())
        b0 = int(rng.integers(0, max(1, nch // 2 + 1)))
        b1 = int(rng.integers(b0, nch + 1))
        row_start = (np.arange(max(b1 - b0, 1)) * 137 + 5).astype(np.int32)
        want = np.full(total + 1, 12345, np.int32)
        fl = np.ascontiguousarray(voiced) if voiced is not None else None
        rc = lib.xv_raw_row_plan(nU, T.ctypes.data, fl.ctypes.data if fl is not None else None, off.ctypes.data, size.ctypes.data,
                                 kept.ctypes.data, seg.ctypes.data, b0, b1, row_start.ctypes.data, want.ctypes.data, total)
        assert rc == 0
        start, n_frames = _scattered_spans(rng, T)
        vad = None
        if with_vad:
            vad = np.full(n_frames, 9.0, np.float32)         # decisions outside the spans are never read as this utterance's
            for u in range(nU):
                vad[start[u]:start[u] + T[u]] = voiced[off[u]:off[u] + T[u]] * rng.choice([1.0, -2.5])
        rank = np.full(n_frames, -7, np.int32)
        count = rowplan_ref.voiced_rank(vad, start, T, n_frames, rank)
        assert np.array_equal(count, V), trial
        dst = np.full(n_frames, -7, np.int32)
        rowplan_ref.chunk_row_plan(rank, start, T, size, kept, seg, n_frames, b0, b1, row_start, dst)
        listed = np.zeros(n_frames, bool)
        for u in range(nU):
            assert np.array_equal(dst[start[u]:start[u] + T[u]], want[off[u]:off[u] + T[u]]), (trial, u)
            listed[start[u]:start[u] + T[u]] = True
        assert np.all(dst[~listed] == -7) and np.all(rank[~listed] == -7), trial


@pytest.mark.parametrize("mn,cs", [(25, 200), (10, -1), (25, 10000), (1, 1), (30, 64)])
def test_the_batches_of_a_window_fill_every_kept_chunk_row_once(mn, cs):
    """The extractor's own plan (engine.plan_chunk_table, BatchLayout) for the voiced counts of a window, its chunk list cut into
    batches: the non-negative dst_row of batch [b0, b1) are exactly the rows of its chunks, each once, and a frame that lands in
    a batch lands in no other."""
    from xvector_amd import engine
    rng = np.random.default_rng(mn * 1000 + cs + 7)
    T = np.array([300, 40, 1, 0, 777, 25, 1300, 90, 260, 33], np.int64)
    start, n_frames = _scattered_spans(rng, T)
    vad = (rng.random(n_frames) < 0.7).astype(np.float32)
    vad[start[1]:start[1] + T[1]] = 0                        # one utterance without a voiced frame
    rank = np.full(n_frames, -7, np.int32)
    V = rowplan_ref.voiced_rank(vad, start, T, n_frames, rank).astype(np.int64)
    order, _, _, c_len, seg = engine.plan_chunk_table(V, mn, cs)
    nch = len(c_len)
    assert nch > 0
    cuts = sorted(set([0, nch] + [nch // 3, nch // 3 + 1, 2 * nch // 3]))
    table = engine.device_plan_table(start, T, order, c_len, seg)          # the tables submit_device_raw uploads
    assert table.dtype == np.int32 and table.shape == (5, len(order))
    hits = np.zeros(n_frames, np.int64)                      # batches each feature row lands in
    for b0, b1 in zip(cuts[:-1], cuts[1:]):
        layout = engine.BatchLayout(c_len[b0:b1], 8, 8)
        dst = np.full(n_frames, -7, np.int32)
        rowplan_ref.chunk_row_plan(rank, *table, n_frames, b0, b1, layout.row_start, dst)
        got = np.sort(dst[dst >= 0])
        want = np.sort(np.concatenate([layout.row_start[j] + np.arange(c_len[b0 + j]) for j in range(b1 - b0)]))
        assert np.array_equal(got, want), (b0, b1)
        hits += dst >= 0
    assert hits.max() == 1 and int(hits.sum()) == int(c_len.sum())
