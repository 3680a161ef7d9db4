"""Diarization on the MI355X: xv_score_blocks_f32 against xv_score_matrix_f32 and xv_ahc_average_batch_f64
against tests/ahc_ref.py AND the single-problem xv_ahc_average_f64, all bit for bit and on poisoned outputs; independence of a
group from its neighbours, its position, the workspace and what ran before; the argument policy on the host and on the device;
the routing of backend.ahc_batch; planted speakers through backend.diarize and through `plda_backend.py diarize`."""
import ctypes
import functools
import os

import numpy as np
import pytest

import ahc_ref
import backend_ref as ref
import diar_ref
import test_gpu_cluster as single

pytestmark = pytest.mark.gpu

NINF, PINF = -np.inf, np.inf
BAD, UNSUPPORTED = -1, -2
NT, STRIDE = 256, 512              # threads of a group's workgroup, slots one of its passes covers (AHC_BATCH_NT, NT * AHC_BATCH_U)
AHC_SIZES = (1, 2, 3, 5, 17, 63, 64, 65, 130, 257, NT - 1, NT, STRIDE - 1, STRIDE, STRIDE + 1)        # NT + 1 = 257 is there
CONFIGS = ((NINF, 1), (0.0, 1), (0.5, 1), (NINF, 5), (PINF, 1))


def _ld(n):
    return (n + 3) & ~3


@functools.lru_cache(maxsize=None)
def _full(n, kind):
    """The reference's full dendrogram of single._scores(n, kind), computed once; every stop rule is a cut of it."""
    out = ahc_ref.dendrogram(single._scores(n, kind))
    for a in out:
        a.setflags(write=False)
    return out


class Tables(object):
    """Host and device tables of a ragged batch, the score blocks ``gap`` elements apart."""

    def __init__(self, sizes, gap=0):
        import torch
        self.sizes = list(sizes)
        self.row0 = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int32)
        self.score0, at = [], gap
        for n in self.sizes:
            self.score0.append(at)
            at += n * _ld(n) + gap
        self.score0 = np.asarray(self.score0, np.int64)
        self.elems = at
        self.n_rows = int(self.row0[-1])
        self.row0_d = torch.from_numpy(self.row0).cuda()
        self.score0_d = torch.from_numpy(self.score0).cuda()
        self.status = torch.zeros(1, dtype=torch.int32, device="cuda")

    def block(self, packed, g):
        n, o = self.sizes[g], int(self.score0[g])
        return packed[o:o + n * _ld(n)].reshape(n, _ld(n))

    def pack(self, group_scores):
        """The device buffer: every group's strict upper triangle in its block, NaN everywhere else."""
        import torch
        host = np.full(self.elems, np.nan, np.float32)
        for g, s in enumerate(group_scores):
            n = self.sizes[g]
            iu = np.triu_indices(n, 1)
            self.block(host, g)[:, :n][iu] = s[iu]
        return torch.from_numpy(host).cuda()


# ------------------------------------------------------------------------------------------------
# score blocks
# ------------------------------------------------------------------------------------------------
BLOCK_SIZES = (1, 2, 3, 5, 31, 33, 127, 128, 129, 130, 257)


@pytest.mark.parametrize("kpad", [8, 304])
def test_score_blocks_equal_the_dense_scorer(kpad):
    import torch
    from xvector_amd import hiplib
    rng = np.random.default_rng(kpad)
    n_rows = sum(BLOCK_SIZES)
    E = torch.from_numpy(rng.standard_normal((n_rows, kpad)).astype(np.float32)).cuda()
    T = torch.from_numpy(rng.standard_normal((n_rows, kpad)).astype(np.float32)).cuda()
    r = torch.from_numpy(rng.standard_normal(n_rows).astype(np.float32)).cuda()
    tb = Tables(BLOCK_SIZES, gap=8)
    out = torch.full((tb.elems + 16,), float("nan"), dtype=torch.float32, device="cuda")
    hiplib.score_blocks(E, T, r, tb.row0_d, tb.score0_d, max(BLOCK_SIZES), out[:tb.elems], tb.status)
    got = out.cpu().numpy()
    assert tb.status.cpu().tolist() == [0]
    written = np.zeros(got.size, bool)
    want = []
    for g, n in enumerate(BLOCK_SIZES):
        r0 = int(tb.row0[g])
        dense = torch.full((n, _ld(n)), float("nan"), dtype=torch.float32, device="cuda")
        hiplib.score_matrix(E[r0:r0 + n], T[r0:r0 + n], r[r0:r0 + n], dense)
        want.append(dense.cpu().numpy())
        assert np.array_equal(tb.block(got, g).view(np.int32), want[g].view(np.int32)), "group %d of %d rows" % (g, n)   # padding: NaN both
        assert np.all(np.isfinite(want[g][:, :n])) and np.all(np.isnan(want[g][:, n:]))
        tb.block(written, g)[:, :n] = True
    assert np.all(np.isnan(got[~written])) and np.all(np.isfinite(got[written]))          # gaps, padding and the tail keep the poison
    # the groups in another order, no gaps: the same blocks
    perm = rng.permutation(len(BLOCK_SIZES))
    rows = np.concatenate([np.arange(tb.row0[g], tb.row0[g + 1]) for g in perm])
    idx = torch.from_numpy(rows).cuda()
    tp = Tables([BLOCK_SIZES[g] for g in perm])
    out2 = torch.full((tp.elems,), float("nan"), dtype=torch.float32, device="cuda")
    hiplib.score_blocks(E[idx].contiguous(), T[idx].contiguous(), r[idx].contiguous(), tp.row0_d, tp.score0_d, 257, out2, tp.status)
    got2 = out2.cpu().numpy()
    assert tp.status.cpu().tolist() == [0]
    for k, g in enumerate(perm.tolist()):
        assert np.array_equal(tp.block(got2, k).view(np.int32), want[g].view(np.int32)), "group %d at position %d" % (g, k)


# ------------------------------------------------------------------------------------------------
# batch clustering
# ------------------------------------------------------------------------------------------------
class BatchOutputs(object):
    """Poisoned outputs of a batch, longer than needed."""

    def __init__(self, n_rows, n_groups):
        import torch
        self.a = torch.full((n_rows + 7,), -1, dtype=torch.int32, device="cuda")
        self.b = torch.full((n_rows + 7,), -1, dtype=torch.int32, device="cuda")
        self.s = torch.full((n_rows + 7,), float("nan"), dtype=torch.float64, device="cuda")
        self.m = torch.full((n_groups + 4,), -1, dtype=torch.int32, device="cuda")
        self.lab = torch.full((n_rows + 5,), -1, dtype=torch.int32, device="cuda")
        self.n_rows = n_rows

    def host(self):
        return [t.cpu().numpy() for t in (self.a, self.b, self.s, self.m, self.lab)]

    def untouched(self):
        a, b, s, m, lab = self.host()
        return bool(np.all(a == -1) and np.all(b == -1) and np.all(np.isnan(s)) and np.all(m == -1) and np.all(lab == -1))


def _ws_tables(sizes):
    """(byte offsets int64 [G], total bytes) of the groups' workspace slices, back to back."""
    from xvector_amd import hiplib
    need = [hiplib.ahc_average_batch_workspace_bytes(n) for n in sizes]
    return np.concatenate([[0], np.cumsum(need)[:-1]]).astype(np.int64), int(sum(need))


def _run_batch(tb, packed, thresholds, min_clusters, ws=None, ws0=None, max_n=None):
    import torch
    from xvector_amd import hiplib
    offs, total = _ws_tables(tb.sizes)
    if ws0 is not None:
        offs = ws0
    if ws is None:
        ws = torch.empty(max(total, 8), dtype=torch.uint8, device="cuda")
    out = BatchOutputs(tb.n_rows, len(tb.sizes))
    hiplib.ahc_average_batch(packed, tb.row0_d, tb.score0_d, torch.from_numpy(np.asarray(offs, np.int64)).cuda(),
                             torch.from_numpy(np.asarray(thresholds, np.float64)).cuda(),
                             torch.from_numpy(np.asarray(min_clusters, np.int32)).cuda(), max(tb.sizes) if max_n is None else max_n,
                             out.a[:tb.n_rows], out.b[:tb.n_rows], out.s[:tb.n_rows], out.m[:len(tb.sizes)], out.lab[:tb.n_rows],
                             tb.status, ws)
    return out


def _check_group(host, tb, g, want, what):
    """Group g's outputs equal want = (a, b, score) and its labels; the rest of what it owns stays poisoned."""
    a, b, sc, m, lab = host
    wa, wb, ws = want
    n, r0, k = tb.sizes[g], int(tb.row0[g]), len(want[0])
    assert m[g] == k, what
    assert np.array_equal(a[r0:r0 + k], wa) and np.array_equal(b[r0:r0 + k], wb), what
    assert np.array_equal(sc[r0:r0 + k].view(np.int64), ws.view(np.int64)), what              # bit for bit
    assert np.array_equal(lab[r0:r0 + n], ahc_ref.labels(n, wa, wb)), what
    assert np.all(a[r0 + k:r0 + n] == -1) and np.all(b[r0 + k:r0 + n] == -1) and np.all(np.isnan(sc[r0 + k:r0 + n])), what


def _check_tails(host, tb):
    a, b, sc, m, lab = host
    assert np.all(a[tb.n_rows:] == -1) and np.all(b[tb.n_rows:] == -1) and np.all(np.isnan(sc[tb.n_rows:]))
    assert np.all(m[len(tb.sizes):] == -1) and np.all(lab[tb.n_rows:] == -1)


@pytest.mark.parametrize("kind", ["normal", "ties"])
def test_batch_exact(kind):
    """Every size under every stop rule, all in ONE call, the groups in a shuffled order."""
    from xvector_amd import hiplib
    groups = [(n, c) for n in AHC_SIZES for c in CONFIGS if c[1] <= n]
    order = np.random.default_rng(5).permutation(len(groups))
    groups = [groups[i] for i in order]
    sizes = [n for n, _ in groups]
    tb = Tables(sizes, gap=4)
    packed = tb.pack([single._scores(n, kind) for n in sizes])
    host = _run_batch(tb, packed, [c[0] for _, c in groups], [c[1] for _, c in groups]).host()
    assert tb.status.cpu().tolist() == [0]
    _check_tails(host, tb)
    fives = 0
    for g, (n, (threshold, min_clusters)) in enumerate(groups):
        what = "group %d: n %d %s threshold %r min_clusters %d" % (g, n, kind, threshold, min_clusters)
        want = ahc_ref.cut(n, _full(n, kind), threshold, min_clusters)
        _check_group(host, tb, g, want, what)
        # ... and the single-problem entry point on the same block
        one = single.Outputs(n)
        blk = tb.block(packed, g)[:, :n]
        hiplib.ahc_average(blk, threshold, min_clusters, one.a, one.b, one.s, one.m, one.lab)
        oa, ob, os_, om, olab = one.host()
        r0, k = int(tb.row0[g]), int(om[0])
        assert k == host[3][g], what
        assert oa[:k].tobytes() == host[0][r0:r0 + k].tobytes() and ob[:k].tobytes() == host[1][r0:r0 + k].tobytes(), what
        assert os_[:k].tobytes() == host[2][r0:r0 + k].tobytes() and olab[:n].tobytes() == host[4][r0:r0 + n].tobytes(), what
        if threshold == PINF:
            assert k == 0, what
        if (threshold, min_clusters) == (NINF, 5):
            assert k == n - 5 and len(set(host[4][r0:r0 + n].tolist())) == 5, what
            fives += 1
    assert fives == len([n for n in AHC_SIZES if n >= 5])


@pytest.mark.parametrize("kind", ["normal", "ties"])
def test_batch_independence(kind):
    """A 257-item group: alone, first, in the middle and last among others, over workspaces of every filling, and again on the
    workspace the first run left behind -- byte-equal outputs."""
    import torch
    n = 257
    s = single._scores(n, kind)
    others = [130, 5, 64, 300]
    runs = []
    for pos, fill in ((None, 0x00), (0, 0xFF), (2, 0x7F), (4, 0x00)):
        sizes = [n] if pos is None else others[:pos] + [n] + others[pos:]
        g = 0 if pos is None else pos
        tb = Tables(sizes, gap=4 * len(runs))
        packed = tb.pack([s if m == n else single._scores(m, "normal") for m in sizes])
        _, total = _ws_tables(sizes)
        ws = torch.full((total + 64,), fill, dtype=torch.uint8, device="cuda")
        for again in range(2):                                       # the second run finds the first one's state
            a, b, sc, m, lab = _run_batch(tb, packed, [0.0] * len(sizes), [1] * len(sizes), ws=ws).host()
            r0 = int(tb.row0[g])
            runs.append((a[r0:r0 + n], b[r0:r0 + n], sc[r0:r0 + n], m[g:g + 1], lab[r0:r0 + n]))
        assert tb.status.cpu().tolist() == [0]
    assert runs[0][3][0] > 0
    want = ahc_ref.cut(n, _full(n, kind), 0.0, 1)
    assert np.array_equal(runs[0][0][:len(want[0])], want[0])
    for r in runs[1:]:
        for x, y in zip(runs[0], r):
            assert x.tobytes() == y.tobytes()


def test_argument_policy_host():
    import torch
    from xvector_amd import hiplib
    lib = hiplib.require_gpu()
    sizes = [12, 7]
    tb = Tables(sizes)
    packed = tb.pack([single._scores(n, "normal") for n in sizes])
    offs, total = _ws_tables(sizes)
    ws = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
    ws0 = torch.from_numpy(offs).cuda()
    thr = torch.zeros(2, dtype=torch.float64, device="cuda")
    minc = torch.ones(2, dtype=torch.int32, device="cuda")
    out = BatchOutputs(tb.n_rows, 2)
    assert hiplib.ahc_average_batch_workspace_bytes(0) == 0 and hiplib.ahc_average_batch_workspace_bytes(12) == 8 * 144 + 24 * 12 + 64
    assert hiplib.ahc_average_batch_workspace_bytes(hiplib.AHC_BATCH_MAX_N + 1) == 0
    assert hiplib.ahc_average_batch_workspace_bytes(hiplib.AHC_BATCH_MAX_N) >= 8 * hiplib.AHC_BATCH_MAX_N ** 2
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)

    def call(**kw):
        a = dict(scores=P(packed), elems=tb.elems, row0=P(tb.row0_d), score0=P(tb.score0_d), ws0=P(ws0), thr=P(thr), minc=P(minc),
                 n_groups=2, max_n=12, n_rows=tb.n_rows, a=P(out.a), b=P(out.b), s=P(out.s), m=P(out.m), lab=P(out.lab),
                 status=P(tb.status), ws=P(ws), ws_bytes=total)
        a.update(kw)
        return lib.xv_ahc_average_batch_f64(a["scores"], a["elems"], a["row0"], a["score0"], a["ws0"], a["thr"], a["minc"], a["n_groups"],
                                            a["max_n"], a["n_rows"], a["a"], a["b"], a["s"], a["m"], a["lab"], a["status"], a["ws"],
                                            a["ws_bytes"], hiplib._stream())

    cases = [(k + " NULL", {k: None}, BAD) for k in ("scores", "row0", "score0", "ws0", "thr", "minc", "a", "b", "s", "m", "lab",
                                                      "status", "ws")]
    cases += [("misaligned scores", dict(scores=P(packed, 4)), BAD), ("misaligned score0", dict(score0=P(tb.score0_d, 4)), BAD),
              ("misaligned ws0", dict(ws0=P(ws0, 4)), BAD), ("misaligned thresholds", dict(thr=P(thr, 4)), BAD),
              ("misaligned merge_score", dict(s=P(out.s, 4)), BAD), ("misaligned labels", dict(lab=P(out.lab, 2)), BAD),
              ("misaligned workspace", dict(ws=P(ws, 4)), BAD), ("n_groups 0", dict(n_groups=0), BAD),
              ("n_groups < 0", dict(n_groups=-1), BAD), ("max_n 0", dict(max_n=0), BAD), ("workspace_bytes 0", dict(ws_bytes=0), BAD),
              ("max_n > XV_AHC_BATCH_MAX_N", dict(max_n=hiplib.AHC_BATCH_MAX_N + 1), UNSUPPORTED)]
    for what, kw, code in cases:
        assert call(**kw) == code, what
        assert lib.xv_last_error(), what
    torch.cuda.synchronize()
    assert out.untouched() and tb.status.cpu().tolist() == [0]
    assert call() == 0                                           # and the same call with nothing wrong runs
    host = out.host()
    for g, n in enumerate(sizes):
        _check_group(host, tb, g, ahc_ref.cut(n, ahc_ref.dendrogram(single._scores(n, "normal")), 0.0, 1), "group %d" % g)

    # xv_score_blocks_f32
    E = torch.ones((tb.n_rows, 16), dtype=torch.float32, device="cuda")
    r = torch.zeros(tb.n_rows, dtype=torch.float32, device="cuda")
    sc = torch.full((tb.elems,), float("nan"), dtype=torch.float32, device="cuda")

    def blocks(**kw):
        a = dict(e=P(E), t=P(E), ldk=16, kpad=16, n_rows=tb.n_rows, r=P(r), row0=P(tb.row0_d), score0=P(tb.score0_d), n_groups=2,
                 max_n=12, scores=P(sc), elems=tb.elems, status=P(tb.status))
        a.update(kw)
        return lib.xv_score_blocks_f32(a["e"], a["t"], a["ldk"], a["kpad"], a["n_rows"], a["r"], a["row0"], a["score0"], a["n_groups"],
                                       a["max_n"], a["scores"], a["elems"], a["status"], hiplib._stream())

    cases = [(k + " NULL", {k: None}, BAD) for k in ("e", "t", "row0", "score0", "scores", "status")]
    cases += [("n_groups 0", dict(n_groups=0), BAD), ("max_n 0", dict(max_n=0), BAD), ("kpad % 8", dict(kpad=12), BAD),
              ("ldk < kpad", dict(ldk=8), BAD), ("ldk % 4", dict(ldk=18), BAD), ("misaligned e", dict(e=P(E, 4)), BAD),
              ("misaligned scores", dict(scores=P(sc, 4)), BAD), ("kpad > 1024", dict(kpad=1032, ldk=1032), UNSUPPORTED)]
    for what, kw, code in cases:
        assert blocks(**kw) == code, what
        assert lib.xv_last_error(), what
    torch.cuda.synchronize()
    assert bool(torch.isnan(sc).all()) and tb.status.cpu().tolist() == [0]
    assert blocks() == 0
    got = sc.cpu().numpy()
    assert all(np.all(tb.block(got, g)[:, :n] == 16.0) for g, n in enumerate(sizes))


@pytest.mark.parametrize("broken", ["n_g = 0", "min_clusters = n_g + 1", "workspace slice past the end"])
def test_argument_policy_device(broken):
    """One group out of contract: status is set, that group's outputs stay poisoned, every other group is right."""
    import torch
    from xvector_amd import hiplib
    sizes = [17, 0, 33] if broken == "n_g = 0" else [17, 9, 33]
    tb = Tables(sizes)
    packed = tb.pack([single._scores(n, "normal") for n in sizes])
    offs, total = _ws_tables(sizes)
    minc = [1, 1, 1]
    if broken == "min_clusters = n_g + 1":
        minc[1] = sizes[1] + 1
    elif broken == "workspace slice past the end":
        offs = offs.copy()
        offs[1] = total - hiplib.ahc_average_batch_workspace_bytes(sizes[1]) + 8
    else:
        # score_blocks skips the same group: the others are written, nothing else is
        E = torch.ones((tb.n_rows, 8), dtype=torch.float32, device="cuda")
        sc = torch.full((tb.elems + 8,), float("nan"), dtype=torch.float32, device="cuda")
        hiplib.score_blocks(E, E, None, tb.row0_d, tb.score0_d, 33, sc[:tb.elems], tb.status)
        got = sc.cpu().numpy()
        assert tb.status.cpu().tolist() == [1]
        assert np.all(tb.block(got, 0)[:, :17] == 8.0) and np.all(tb.block(got, 2)[:, :33] == 8.0)
        assert np.all(np.isnan(tb.block(got, 0)[:, 17:])) and np.all(np.isnan(tb.block(got, 2)[:, 33:])) and np.all(np.isnan(got[tb.elems:]))
        tb.status.zero_()
    ws = torch.zeros(total, dtype=torch.uint8, device="cuda")
    host = _run_batch(tb, packed, [0.0] * 3, minc, ws=ws, ws0=offs, max_n=33).host()
    assert tb.status.cpu().tolist() == [1]
    a, b, sc, m, lab = host
    _check_tails(host, tb)
    assert m[1] == -1
    r0, n1 = int(tb.row0[1]), sizes[1]
    assert np.all(a[r0:r0 + n1] == -1) and np.all(b[r0:r0 + n1] == -1) and np.all(np.isnan(sc[r0:r0 + n1])) and np.all(lab[r0:r0 + n1] == -1)
    for g in (0, 2):
        want = ahc_ref.cut(sizes[g], ahc_ref.dendrogram(single._scores(sizes[g], "normal")), 0.0, 1)
        _check_group(host, tb, g, want, "%s: group %d" % (broken, g))


@pytest.mark.parametrize("case", ["route above max_batch_n", "cut under max_bytes"])
def test_routing_and_cutting(case):
    """backend.ahc_batch: groups above max_batch_n through the single-problem kernel, and calls cut by max_bytes, change nothing.
    (10, 64, 65, 130) cannot be cut into three calls -- whatever holds the 130 also holds the other three together -- so the
    cutting case puts a second 130 in front: [130], [10, 64, 65], [130] under a limit of one 130's workspace."""
    from xvector_amd import backend, hiplib
    sizes = [10, 64, 65, 130] if case == "route above max_batch_n" else [130, 10, 64, 65, 130]
    G = len(sizes)
    tables = backend.GroupTables(sizes, "cuda:0")
    tb = Tables(sizes)
    assert tb.score0.tolist() == tables.score0.tolist() and tb.elems == tables.scores_elems
    packed = tb.pack([single._scores(n, "normal") for n in sizes])
    thr, minc = ([0.0, NINF, 0.5, 0.0, NINF])[:G], ([1, 3, 1, 1, 7])[:G]
    base = backend.ahc_batch(packed, tables, thr, minc)
    for g, n in enumerate(sizes):
        wa, wb, ws = ahc_ref.cut(n, _full(n, "normal"), thr[g], minc[g])
        assert np.array_equal(base[1][g][0], wa) and np.array_equal(base[1][g][1], wb)
        assert np.array_equal(base[1][g][2].view(np.int64), ws.view(np.int64)) and np.array_equal(base[0][g], ahc_ref.labels(n, wa, wb))
    need130 = hiplib.ahc_average_batch_workspace_bytes(130)
    if case == "route above max_batch_n":
        assert backend.plan_ahc_batch(sizes, max_batch_n=64)[1] == [2, 3]
        variants = (dict(max_batch_n=64), dict(max_batch_n=9))                    # 65 and 130 routed; everything routed
    else:
        assert [c[:2] for c in backend.plan_ahc_batch(sizes, max_bytes=need130)[0]] == [(0, 1), (1, 4), (4, 5)]      # three calls
        variants = (dict(max_bytes=need130), dict(max_bytes=need130, max_batch_n=64))
    for kw in variants:
        labels, merges = backend.ahc_batch(packed, tables, thr, minc, **kw)
        for g in range(G):
            assert labels[g].tobytes() == base[0][g].tobytes() and labels[g].dtype == np.int32, (kw, g)
            assert all(x.tobytes() == y.tobytes() and x.dtype == y.dtype for x, y in zip(merges[g], base[1][g])), (kw, g)
    if case == "cut under max_bytes":
        return
    with pytest.raises(ValueError, match="max_bytes"):
        backend.ahc_batch(packed, tables, thr, minc, max_bytes=need130 - 1)
    with pytest.raises(ValueError):
        backend.ahc_batch(packed, tables, thr, [1, 3, 1, 131])
    with pytest.raises(ValueError):
        backend.ahc_batch(packed, tables, [0.0, float("nan"), 0.0, 0.0], minc)
    bad = packed.clone()
    bad[int(tb.score0[2]) + 1] = float("inf")                        # cell (0, 1) of group 2
    with pytest.raises(ValueError, match="not finite"):
        backend.ahc_batch(bad, tables, thr, minc)
    bad[int(tb.score0[2]) + 1] = 0.0
    bad[int(tb.score0[2]) + 65] = float("inf")                       # a padding column of its row 0: never looked at
    backend.ahc_batch(bad, tables, thr, minc)


# ------------------------------------------------------------------------------------------------
# planted speakers
# ------------------------------------------------------------------------------------------------
D, DIM, THRESHOLD = single.D, single.DIM, single.THRESHOLD
# (speakers, vectors per speaker, vectors dropped): 42 .. 117 vectors per recording, none a multiple of 4
RECORDINGS = ((2, 21, 0), (3, 15, 0), (4, 15, 1), (3, 23, 0), (2, 35, 0), (4, 25, 1), (3, 31, 0), (2, 53, 0), (3, 39, 0), (4, 19, 2),
              (2, 27, 0), (3, 19, 0))


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """An out-of-domain LDA + PLDA as test_gpu_cluster's, and 12 recordings of 2-4 planted speakers each, shuffled within."""
    from xvector_amd import backend
    rng = np.random.default_rng(23)
    mix = rng.standard_normal((D, D)) / np.sqrt(D)
    mu = rng.standard_normal(D)
    xo, lo = single._draw(rng, mix, mu, 60, 6)
    xo64 = xo.astype(np.float64)
    t = backend.fit_lda(xo64 - xo64.mean(axis=0), list(lo), DIM).astype(np.float32)
    plda = backend.fit_plda(ref.chain(xo64, xo64.mean(axis=0), t, True), [np.flatnonzero(lo == s) for s in range(60)])
    mu_in = mu + 0.5 * rng.standard_normal(D)
    xs, spk, sizes = [], [], []
    for n_spk, n_utt, drop in RECORDINGS:
        x, l = single._draw(rng, mix, mu_in, n_spk, n_utt)
        keep = rng.permutation(len(x))[:len(x) - drop]
        xs.append(x[keep]); spk.append(l[keep]); sizes.append(len(keep))
    x = np.concatenate(xs)
    assert all(40 <= n <= 120 and n % 4 for n in sizes)
    mean_in = x.astype(np.float64).mean(axis=0).astype(np.float32)
    return dict(t=t, plda=plda, x=x, spk=spk, sizes=sizes, mean_in=mean_in, p=str(tmp_path_factory.mktemp("diarize")))


def _scores64(world):
    """Every recording's float64 score matrix under the float64 reference chain."""
    plda, t, mean_in = world["plda"], world["t"], world["mean_in"]
    pl = (plda.mean, plda.transform, plda.psi)
    out, at = [], 0
    for n in world["sizes"]:
        x = world["x"][at:at + n]
        at += n
        ones = np.ones(n)
        rows, r = ref.side_rows_enrol(ref.chain(x, mean_in, t, True, pl, ones), ones, plda.psi)
        out.append(rows @ ref.side_rows_test(ref.chain(x, mean_in, t, True, pl, None)).T + r[:, None])
    return out


def _split(labels, sizes):
    return np.split(np.asarray(labels), np.cumsum(sizes)[:-1])


def test_planted_speakers(world):
    from xvector_amd import backend
    x, sizes, spk, t, plda, mean_in = (world[k] for k in ("x", "sizes", "spk", "t", "plda", "mean_in"))
    G = len(sizes)
    # the fixture, not the kernel, carries the condition: the float64 reference on float64 scores recovers every planted partition
    ref64 = diar_ref.cluster_groups(_scores64(world), [THRESHOLD] * G, [1] * G)
    for g in range(G):
        assert single._partition(ref64[g][0]) == single._partition(spk[g]), "recording %d" % g
    # the device: the planted partitions, and the reference's merges on the device's own fp32 blocks
    labels, merges = backend.diarize(x, sizes, plda, mean=mean_in, transform=t, threshold=THRESHOLD)
    assert labels.dtype == np.int32 and labels.shape == (len(x),) and len(merges) == G
    for g, lab in enumerate(_split(labels, sizes)):
        assert single._partition(lab) == single._partition(spk[g]), "recording %d" % g
    scores, tables = backend.score_blocks(x, sizes, plda, mean_in, t)
    s32 = diar_ref.blocks(scores.cpu().numpy(), sizes)
    assert tables.status.cpu().tolist() == [0]
    want = diar_ref.cluster_groups(s32, [THRESHOLD] * G, [1] * G)
    for g, lab in enumerate(_split(labels, sizes)):
        wl, (wa, wb, ws) = want[g]
        a, b, sc = merges[g]
        assert np.array_equal(a, wa) and np.array_equal(b, wb) and np.array_equal(sc.view(np.int64), ws.view(np.int64)), g
        assert np.array_equal(lab, wl) and a.dtype == np.int32 and sc.dtype == np.float64, g
    # a block is what the dense route gives that recording on its own
    one = backend.score_matrix_self(x[:sizes[0]], plda, mean_in, t)[:, :sizes[0]].cpu().numpy()
    assert np.array_equal(one.view(np.int32), np.ascontiguousarray(s32[0]).view(np.int32))
    # speaker counts for half of the recordings: exactly those counts, the other half as before
    num_spk = [(g % 5) + 1 if g % 2 else None for g in range(G)]
    lab2, merges2 = backend.diarize(x, sizes, plda, mean=mean_in, transform=t, threshold=THRESHOLD, num_spk=num_spk)
    thr, minc = diar_ref.stop_rules(sizes, THRESHOLD, num_spk)
    want2 = diar_ref.cluster_groups(s32, thr, minc)
    for g, lab in enumerate(_split(lab2, sizes)):
        if num_spk[g] is not None:
            assert len(set(lab.tolist())) == num_spk[g] and len(merges2[g][0]) == sizes[g] - num_spk[g], g
        assert np.array_equal(lab, want2[g][0]) and np.array_equal(merges2[g][0], want2[g][1][0]), g
        assert np.array_equal(merges2[g][2].view(np.int64), want2[g][1][2].view(np.int64)), g


def test_cli_route(world, caplog):
    """`plda_backend.py diarize` through its own entry point: labels and RTTM byte-equal to tests/diar_ref.py on the device's scores."""
    import kaldi_io
    import plda_backend
    from xvector_amd import backend
    p = world["p"]
    G = 4                                                            # the first four recordings
    sizes = world["sizes"][:G]
    n = sum(sizes)
    x = world["x"][:n]
    reco_of = np.repeat(np.arange(G), sizes)
    within = np.concatenate([np.arange(m) for m in sizes])
    # the file interleaves the recordings: sub-segment i of every recording, then i + 1, ...; 1.5 s spans every 0.75 s
    file_order = np.lexsort((reco_of, within))
    keys = ["reco%d-%04d" % (reco_of[i], within[i]) for i in range(n)]
    seg_lines = ["%s reco%d %.2f %.2f" % (keys[i], reco_of[i], 0.75 * within[i], 0.75 * within[i] + 1.5) for i in file_order]
    seg_lines.insert(5, "ghost-0000 reco1 0.00 1.50")                 # lines without a vector: skipped and counted
    seg_lines.append("ghost-0001 reco9 0.00 1.50")
    with open(p + "/segments", "w") as f:
        f.write("\n".join(seg_lines) + "\n")
    with kaldi_io.TableWriter(p + "/xvector.ark", p + "/xvector.scp") as w:
        kaldi_io.write_vec_flt_batch(w, keys, list(x))
    backend.write_transform(p + "/transform.mat", world["t"])
    backend.write_plda(p + "/plda", world["plda"])
    kaldi_io.write_vec_flt(p + "/mean.vec", world["mean_in"])
    with open(p + "/reco2num_spk", "w") as f:
        f.write("reco1 2\nreco3 500\nreco7 3\n")                      # 500 is clipped to the recording's vector count
    argv = ["diarize", "--mean", p + "/mean.vec", "--lda", p + "/transform.mat", "--threshold", str(THRESHOLD), "--reco2num-spk",
            p + "/reco2num_spk", "--rttm", p + "/out.rttm", "--rttm-channel", "1", p + "/plda", "scp:" + p + "/xvector.scp",
            p + "/segments", p + "/labels"]
    with caplog.at_level("INFO", logger="plda_backend"):
        plda_backend.main(argv)
    # the reference, from the device's own scores: recording g's vectors in file order are its vectors in their own order
    scores, _ = backend.score_blocks(x, sizes, world["plda"], world["mean_in"], world["t"])
    s32 = diar_ref.blocks(scores.cpu().numpy(), sizes)
    thr, minc = diar_ref.stop_rules(sizes, THRESHOLD, [None, 2, None, 500])
    clustered = diar_ref.cluster_groups(s32, thr, minc)
    label = {}
    recos = []
    row0 = np.concatenate([[0], np.cumsum(sizes)])
    for g in range(G):
        numbered = diar_ref.number_labels(clustered[g][0])
        segs = []
        for j, l in enumerate(numbered):
            label[keys[row0[g] + j]] = l
            segs.append((diar_ref.to_ms("%.2f" % (0.75 * j)), diar_ref.to_ms("%.2f" % (0.75 * j + 1.5)), keys[row0[g] + j], l))
        recos.append(("reco%d" % g, segs))
    n_speakers = sum(max(label[keys[i]] for i in range(row0[g], row0[g + 1])) for g in range(G))
    assert open(p + "/labels").read() == "".join("%s %d\n" % (keys[i], label[keys[i]]) for i in file_order)
    assert open(p + "/out.rttm").read() == diar_ref.rttm(recos, 1)
    assert not os.path.exists(p + "/labels.tmp") and not os.path.exists(p + "/out.rttm.tmp")
    assert len(set(label[k] for k in keys[row0[1]:row0[2]])) == 2 and len(set(label[k] for k in keys[row0[3]:row0[4]])) == sizes[3]
    for g in (0, 2):
        assert single._partition([label[k] for k in keys[row0[g]:row0[g + 1]]]) == single._partition(world["spk"][g])
    assert "Diarized %d recordings: %d vectors of dimension %d into %d speakers (2 segments without a vector skipped)" % (
        G, n, DIM, n_speakers) in caplog.text
    assert "2 segments" in caplog.text and "using %d" % sizes[3] in caplog.text
    # a vector without a line: a non-zero exit, nothing written
    with open(p + "/segments_short", "w") as f:
        f.write("\n".join(l for l in seg_lines if not l.startswith(keys[3] + " ")) + "\n")
    with pytest.raises(SystemExit) as ei:
        plda_backend.main(["diarize", "--rttm", p + "/no.rttm", p + "/plda", "scp:" + p + "/xvector.scp", p + "/segments_short",
                           p + "/no_labels"])
    assert ei.value.code not in (0, None) and keys[3] in str(ei.value)
    # a dimension mismatch, in the words of `cluster`
    backend.write_plda(p + "/plda17", backend.plda_from_covariances(np.zeros(DIM + 1), np.eye(DIM + 1) * 2.0, np.eye(DIM + 1)))
    with pytest.raises(SystemExit) as ei:
        plda_backend.main(["diarize", "--lda", p + "/transform.mat", p + "/plda17", "scp:" + p + "/xvector.scp", p + "/segments",
                           p + "/no_labels"])
    assert "dimension" in str(ei.value)
    assert not any(os.path.exists(p + "/" + f) for f in ("no.rttm", "no_labels", "no.rttm.tmp", "no_labels.tmp"))
