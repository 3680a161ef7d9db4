"""The row-plan kernels on the MI355X (csrc/xv_rowplan.hip) against their NumPy restatement (tests/rowplan_ref.py).  Integers
only: every comparison is exact."""
import ctypes

import numpy as np
import pytest

import rowplan_ref

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 5000)       # around the wave (64) and its tile of 4 steps (256)
SENTINEL = -7


@pytest.fixture(scope="module")
def env():
    import torch
    from xvector_amd import hiplib
    hiplib.require_gpu()
    return dict(torch=torch, hiplib=hiplib)


def _dev(torch, a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


@pytest.fixture(scope="module")
def problem():
    """Every length of LENGTHS under every VAD pattern (all voiced, none, alternating, 70 % random), listed in shuffled order with
    gaps between the spans, plus one span that leaves [0, n_frames); per-utterance chunk tables that cover chunk size 1, a size
    beyond the voiced count, sizes <= 0 and a kept count that drops the tail.  The restatement's answers are computed once."""
    rng = np.random.default_rng(20260)
    T, pattern = [], []
    for n in LENGTHS:
        for p in range(4):
            T.append(n)
            pattern.append(p)
    T = np.array(T + [100], np.int64)                        # the last one: its span leaves the buffer
    nU = len(T)
    start = np.zeros(nU, np.int64)
    at = 5
    for u in rng.permutation(nU - 1).tolist():
        start[u] = at
        at += int(T[u]) + int(rng.integers(0, 4))
    n_frames = at + 2
    start[-1] = n_frames - 40
    vad = (rng.random(n_frames) < 0.5).astype(np.float32) * 3.0          # the gaps hold decisions too: they belong to nobody
    for u in range(nU - 1):
        s, n = int(start[u]), int(T[u])
        vad[s:s + n] = [np.ones(n), np.zeros(n), np.arange(n) % 2, (rng.random(n) < 0.7) * -0.5][pattern[u]]
    rank = np.full(n_frames, SENTINEL, np.int32)
    count = rowplan_ref.voiced_rank(vad, start, T, n_frames, rank)
    rank_all = np.full(n_frames, SENTINEL, np.int32)
    count_all = rowplan_ref.voiced_rank(None, start, T, n_frames, rank_all)
    size = np.array([(1, 37, 100, 0, -3, 6000, 64, 250)[u % 8] for u in range(nU)], np.int64)
    size[np.flatnonzero(T == 5000)] = (37, 1, 100, 64)       # the long ones bring many chunks each
    nchunks = np.where(size > 0, -(-count.astype(np.int64) // np.maximum(size, 1)), 0)
    kept = np.where(np.arange(nU) % 3 == 0, np.maximum(nchunks - 1, 0), nchunks)          # every third drops its tail
    kept[np.flatnonzero(size <= 0)] = 2                      # (ignored: no chunk of such an utterance exists)
    first = np.zeros(nU, np.int64)
    np.cumsum(np.where(size > 0, kept, 0)[:-1], out=first[1:])
    nch = int(first[-1] + (kept[-1] if size[-1] > 0 else 0))
    return dict(T=T, start=start, n_frames=n_frames, vad=vad, rank=rank, count=count, rank_all=rank_all, count_all=count_all,
                size=size, kept=kept, first=first, nch=nch)


def test_voiced_rank_equals_the_restatement_and_leaves_the_rest_alone(env, problem):
    torch, hiplib, p = env["torch"], env["hiplib"], problem
    us, ul = _dev(torch, p["start"], np.int32), _dev(torch, p["T"], np.int32)
    vad = _dev(torch, p["vad"], np.float32)
    for v, want_rank, want_count in ((vad, p["rank"], p["count"]), (None, p["rank_all"], p["count_all"])):
        runs = []
        for _ in range(2):
            rank = torch.full((p["n_frames"],), SENTINEL, dtype=torch.int32, device="cuda")
            _, count = hiplib.voiced_rank(v, us, ul, p["n_frames"], rank=rank)
            runs.append((rank.cpu().numpy(), count.cpu().numpy()))
        assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
        assert np.array_equal(runs[0][1], want_count)
        assert np.array_equal(runs[0][0], want_rank)         # the gaps and the out-of-range span keep the sentinel
    assert p["count"][-1] == 0 and (p["rank"] == SENTINEL).any()
    compact = hiplib.vad_compact(vad, us, ul)[0].cpu().numpy()
    assert np.array_equal(compact, p["count"])
    # nothing to do / refused
    e = torch.zeros(0, dtype=torch.int32, device="cuda")
    r, c = hiplib.voiced_rank(vad, e, e, p["n_frames"])
    assert c.numel() == 0
    lib = hiplib.load()
    q = ctypes.c_void_p(torch.zeros(16, dtype=torch.int32, device="cuda").data_ptr())     # (one empty utterance, were it read)
    assert lib.xv_voiced_rank_i32(None, None, None, 0, 10, q, q, None) == 0
    for bad in ((None, q), (q, None)):
        assert lib.xv_voiced_rank_i32(None, q, q, 1, 10, bad[0], bad[1], None) != 0
    assert lib.xv_voiced_rank_i32(None, q, q, -1, 10, q, q, None) != 0 and lib.xv_voiced_rank_i32(None, q, q, 1, -1, q, q, None) != 0


def test_chunk_row_plan_equals_the_restatement_over_three_batches(env, problem):
    torch, hiplib, p = env["torch"], env["hiplib"], problem
    nch, n_frames = p["nch"], p["n_frames"]
    long_u = int(np.flatnonzero((p["T"] == 5000) & (p["size"] == 37))[0])                 # its chunks lie in all three batches
    f, k = int(p["first"][long_u]), int(p["kept"][long_u])
    cuts = [0, f + k // 3, f + 2 * k // 3, nch]
    assert k >= 3 and 0 < cuts[1] < cuts[2] < nch
    tabs = [_dev(torch, p[name], np.int32) for name in ("start", "T", "size", "kept", "first")]
    rank = _dev(torch, p["rank"], np.int32)
    seen = 0
    for b0, b1 in zip(cuts[:-1], cuts[1:]):
        row_start = (11 + 5003 * np.arange(b1 - b0)).astype(np.int32)
        want = np.full(n_frames, SENTINEL, np.int32)
        rowplan_ref.chunk_row_plan(p["rank"], p["start"], p["T"], p["size"], p["kept"], p["first"], n_frames, b0, b1, row_start, want)
        dst = torch.full((n_frames,), SENTINEL, dtype=torch.int32, device="cuda")
        hiplib.chunk_row_plan(rank, *tabs, n_frames, b0, b1, _dev(torch, row_start, np.int32), dst)
        got = dst.cpu().numpy()
        assert np.array_equal(got, want), (b0, b1)
        s = int(p["start"][long_u])
        assert (got[s:s + 5000] >= 0).any()
        seen += int((got >= 0).sum())
    assert (want == SENTINEL).any() and seen > 0
    lib = hiplib.load()
    q = ctypes.c_void_p(torch.zeros(16, dtype=torch.int32, device="cuda").data_ptr())     # (one empty utterance, were it read)
    assert lib.xv_chunk_row_plan_i32(None, None, None, None, None, None, 0, 10, 0, 0, None, q, None) == 0
    assert lib.xv_chunk_row_plan_i32(q, q, q, q, q, q, 1, 10, 0, 1, q, None, None) != 0
    assert lib.xv_chunk_row_plan_i32(q, q, q, q, q, q, -1, 10, 0, 1, q, q, None) != 0
    assert lib.xv_chunk_row_plan_i32(q, q, q, q, q, q, 1, -1, 0, 1, q, q, None) != 0


def test_seventy_thousand_short_utterances(env):
    """More utterances than one grid dimension of 65535 holds, each 0 .. 3 frames."""
    torch, hiplib = env["torch"], env["hiplib"]
    rng = np.random.default_rng(70000)
    nU = 70000
    T = rng.integers(0, 4, nU).astype(np.int64)
    start = np.zeros(nU, np.int64)
    np.cumsum(T[:-1], out=start[1:])
    n_frames = int(T.sum())
    vad = (rng.random(n_frames) < 0.7).astype(np.float32)
    utt = np.repeat(np.arange(nU), T)
    want_rank = np.full(n_frames, SENTINEL, np.int32)
    want_count = rowplan_ref.voiced_rank(vad, start, T, n_frames, want_rank)
    size = rng.integers(1, 4, nU).astype(np.int64)
    kept = -(-want_count.astype(np.int64) // size)
    first = np.zeros(nU, np.int64)
    np.cumsum(kept[:-1], out=first[1:])
    nch = int(kept.sum())
    b0, b1 = nch // 2, nch - 5
    row_start = (8 * np.arange(b1 - b0) + 8).astype(np.int32)
    want_dst = np.full(n_frames, SENTINEL, np.int32)
    rowplan_ref.chunk_row_plan(want_rank, start, T, size, kept, first, n_frames, b0, b1, row_start, want_dst)
    us, ul = _dev(torch, start, np.int32), _dev(torch, T, np.int32)
    rank, count = hiplib.voiced_rank(_dev(torch, vad, np.float32), us, ul, n_frames)
    assert np.array_equal(count.cpu().numpy(), want_count)
    assert np.array_equal(rank.cpu().numpy()[:n_frames], want_rank)
    dst = hiplib.chunk_row_plan(rank, us, ul, _dev(torch, size, np.int32), _dev(torch, kept, np.int32), _dev(torch, first, np.int32),
                                n_frames, b0, b1, _dev(torch, row_start, np.int32))
    assert np.array_equal(dst.cpu().numpy()[:n_frames], want_dst)
    assert (want_dst[utt >= 65535] >= 0).any()               # utterances past a grid dimension of 65535 are planned too
