"""xv_vad_segments_i32 on the MI355X (csrc/xv_segment.hip) against the per-frame loop of tests/segment_ref.py.  Integers only:
every comparison is exact.  One launch holds every utterance; the reference is computed once per parameter set."""
import ctypes

import numpy as np
import pytest

import segment_ref

pytestmark = pytest.mark.gpu

LENGTHS = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 5000)
PARAMS = [(30, 50, 10, 300), (0, 1, 0, 0), (4, 3, 2, 6)]        # (G, M, P, L): the recipe's shape with frequent splits; the rule's lower ends
SENTINEL = -7
SLACK = 2                                                        # sentinel slots behind every utterance's table


@pytest.fixture(scope="module")
def env():
    import torch
    from xvector_amd import hiplib
    hiplib.require_gpu()
    return dict(torch=torch, hiplib=hiplib)


def _dev(torch, a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _utterances(G, M, P, L, tile):
    """The decisions of every utterance of the launch (the last one is the one whose span leaves the buffer)."""
    rng = np.random.default_rng(8180 + G)
    utts = [v for _, v in segment_ref.hand_cases(G, M, P, L)]
    for n in LENGTHS:
        utts.append(segment_ref.bursty(rng, n, 40, 25))
    utts.append(np.ones(5000, np.float32))                                    # one run over 20 tiles
    # runs and gaps around the tile: bursts of about a tile, a tile and a half, and gaps on both sides of G that land anywhere
    for run, gap in ((tile, G + 1), (tile + tile // 2, max(G // 2, 1)), (3 * tile, tile), (tile // 2, G + 2), (17, G + 1)):
        utts.append(segment_ref.bursty(rng, 4 * tile + int(rng.integers(0, tile)), run, gap))
    # gaps of exactly G and G + 1 laid ACROSS tile boundaries, and a run that ends / starts exactly at one
    v = np.ones(6 * tile, np.float32)
    v[tile - G // 2 - 1:tile - G // 2 - 1 + G] = 0
    v[2 * tile - 1:2 * tile + G] = 0
    v[3 * tile:3 * tile + G + 1] = 0
    v[4 * tile - (G + 1):4 * tile] = 0
    v[5 * tile - 1] = 0
    utts.append(v)
    long = segment_ref.bursty(rng, 100000, 6000, 60, lead=3)                  # long runs: pieces across many tiles
    long[40000:40000 + G + 1] = 0
    utts.append(long)
    utts.append(segment_ref.bursty(rng, 100, 40, 5))                          # (its span will leave the buffer)
    return utts


@pytest.fixture(scope="module", params=PARAMS, ids=lambda p: "G%d-M%d-P%d-L%d" % p)
def problem(request):
    return build_problem(*request.param)


def build_problem(G, M, P, L):
    """The launch and the loop's answers for it (host only: the capacities come from the library's host function)."""
    from xvector_amd import hiplib
    utts = _utterances(G, M, P, L, hiplib.SEG_TILE)
    nU = len(utts)
    rng = np.random.default_rng(3)
    T = np.array([len(v) for v in utts], np.int64)
    start = np.zeros(nU, np.int64)
    at = 3
    for u in rng.permutation(nU - 1).tolist():                                # shuffled order, gaps between the spans
        start[u] = at
        at += int(T[u]) + int(rng.integers(0, 5))
    n_frames = at + 1
    start[-1] = n_frames - 40
    vad = np.ones(n_frames, np.float32)                                       # the gaps hold voiced decisions: they belong to nobody
    for u in range(nU - 1):
        vad[start[u]:start[u] + T[u]] = utts[u]
    want = [segment_ref.segments(v, G, M, P, L) for v in utts[:-1]] + [[]]
    for u in range(nU - 1):
        segment_ref.check_properties(want[u], int(T[u]), G, M, L)
    count = np.array([len(w) for w in want], np.int64)
    cap = np.array([hiplib.vad_segments_capacity(int(t), G, M, L) for t in T], np.int64)
    assert (count <= cap).all() and count.max() > 50 and (count == 0).sum() >= 3
    short = int(np.flatnonzero((count >= 3) & (T < 5000))[0])                 # this one's table is one entry short
    cap[short] = count[short] - 1
    cap[-1] = 5                                                               # (the span that leaves the buffer: nothing is written)
    room = np.maximum(cap, count) + SLACK
    off = np.zeros(nU, np.int64)
    order = rng.permutation(nU)                                               # the tables lie in another order than the utterances
    off[order] = np.concatenate([[0], np.cumsum(room[order])[:-1]])
    n_slots = int(room.sum())
    first = np.full(n_slots, SENTINEL, np.int32)
    length = np.full(n_slots, SENTINEL, np.int32)
    for u in range(nU):
        k = min(int(count[u]), int(cap[u]))
        if k:
            w = np.array(want[u][:k], np.int32)
            first[off[u]:off[u] + k], length[off[u]:off[u] + k] = w[:, 0], w[:, 1]
    return dict(params=(G, M, P, L), T=T, start=start, vad=vad, n_frames=n_frames, off=off, cap=cap, count=count, first=first,
                length=length, n_slots=n_slots, short=short)


def _launch(env, p, **over):
    torch, hiplib = env["torch"], env["hiplib"]
    G, M, P, L = p["params"]
    out = [torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda") for n in (len(p["T"]), p["n_slots"], p["n_slots"])]
    hiplib.vad_segments(_dev(torch, p["vad"], np.float32), _dev(torch, p["start"], np.int32), _dev(torch, p["T"], np.int32),
                        G, M, P, L, _dev(torch, over.get("off", p["off"]), np.int32), _dev(torch, p["cap"], np.int32), *out)
    return [t.cpu().numpy() for t in out]


def test_segments_equal_the_loop_and_repeat_bit_for_bit(env, problem):
    p = problem
    runs = [_launch(env, p) for _ in range(2)]
    assert all(np.array_equal(a, b) for a, b in zip(*runs))
    count, first, length = runs[0]
    assert np.array_equal(count, p["count"])                  # the full counts: also of the short table and of the span outside
    assert count[p["short"]] == p["cap"][p["short"]] + 1 and count[-1] == 0
    assert np.array_equal(first, p["first"])                  # every entry no segment names keeps the sentinel
    assert np.array_equal(length, p["length"])


def test_entries_outside_the_slots_are_not_written(env, problem):
    """Tables moved so that some begin before slot 0 and some end behind the last one: what lies inside is written, nothing else."""
    p = problem
    shift = np.where(np.arange(len(p["T"])) % 2 == 0, -40, 25)
    off = p["off"] + shift
    count, first, length = _launch(env, p, off=off)
    assert np.array_equal(count, p["count"])
    want_first = np.full(p["n_slots"], SENTINEL, np.int32)
    want_len = np.full(p["n_slots"], SENTINEL, np.int32)
    # (moved tables may overlap their neighbours' slack or entries: apply them in any order and compare only where exactly one writes)
    writers = np.zeros(p["n_slots"], np.int64)
    for u in range(len(p["T"])):
        k = min(int(p["count"][u]), int(p["cap"][u]))
        for i in range(k):
            s = int(off[u]) + i
            if 0 <= s < p["n_slots"]:
                writers[s] += 1
                want_first[s], want_len[s] = p["first"][p["off"][u] + i], p["length"][p["off"][u] + i]
    one = writers <= 1
    assert (writers == 0).sum() > 0 and np.array_equal(first[one], want_first[one]) and np.array_equal(length[one], want_len[one])


def test_bad_arguments_launch_nothing(env):
    torch, hiplib = env["torch"], env["hiplib"]
    lib = hiplib.require_gpu()
    n, slots = 2, 8
    vad = torch.ones(64, dtype=torch.float32, device="cuda")
    us, ul = _dev(torch, [0, 32], np.int32), _dev(torch, [32, 32], np.int32)
    off, cap = _dev(torch, [0, 4], np.int32), _dev(torch, [4, 4], np.int32)
    out = [torch.full((k,), SENTINEL, dtype=torch.int32, device="cuda") for k in (n, slots, slots)]
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())        # noqa: E731
    good = dict(vad=ptr(vad), us=ptr(us), ul=ptr(ul), n=n, frames=64, G=30, M=5, P=10, L=0, off=ptr(off), cap=ptr(cap), slots=slots,
                count=ptr(out[0]), first=ptr(out[1]), length=ptr(out[2]), ws=None, ws_bytes=0)

    def call(**over):
        a = dict(good, **over)
        return lib.xv_vad_segments_i32(a["vad"], a["us"], a["ul"], a["n"], a["frames"], a["G"], a["M"], a["P"], a["L"], a["off"], a["cap"],
                                       a["slots"], a["count"], a["first"], a["length"], a["ws"], a["ws_bytes"], None)
    bad = [dict(vad=None), dict(us=None), dict(ul=None), dict(off=None), dict(cap=None), dict(count=None), dict(first=None),
           dict(length=None), dict(n=-1), dict(frames=-1), dict(slots=-1), dict(G=-1), dict(M=0), dict(P=-1), dict(P=16), dict(L=9),
           dict(L=-1), dict(ws=None, ws_bytes=64)]
    for over in bad:
        assert call(**over) == -1, over                       # XV_ERR_BAD_ARG
        assert b"vad_segments" in lib.xv_last_error()
    torch.cuda.synchronize()
    assert all((t.cpu().numpy() == SENTINEL).all() for t in out)
    assert call(n=0) == 0                                      # no utterance: nothing launched
    torch.cuda.synchronize()
    assert all((t.cpu().numpy() == SENTINEL).all() for t in out)
    assert call() == 0                                         # and the good call runs: one segment of 32 frames each
    torch.cuda.synchronize()
    assert out[0].cpu().tolist() == [1, 1] and out[1].cpu().tolist()[::4] == [0, 0] and out[2].cpu().tolist()[::4] == [32, 32]


def test_segments_device_equals_the_twin(env, problem):
    """``segment.segments_device``: capacities from the library, one download, per-utterance tables; a wrong bound is an error."""
    from xvector_amd import segment
    torch, p = env["torch"], problem
    opts = segment.SegmentOptions(*p["params"])
    keep = np.arange(len(p["T"]) - 1)                          # (without the span that leaves the buffer)
    vad = _dev(torch, p["vad"], np.float32)
    got = segment.segments_device(vad, p["start"][keep], p["T"][keep], opts)
    for u in keep.tolist():
        want = segment.vad_segments_host(p["vad"][p["start"][u]:p["start"][u] + p["T"][u]], opts)
        assert got[u].dtype == np.int32 and np.array_equal(got[u], want), u
    assert segment.segments_device(vad, [], [], opts) == []
