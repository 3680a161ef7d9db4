"""Host side of diarization, no GPU: the RTTM rule of `plda_backend.py diarize` on hand-written cases against
tests/diar_ref.py byte for byte, grouping by recording and label numbering, the usage errors, and the planning of
backend.ahc_batch / backend.diarize (size order, cutting calls under max_bytes, routing large groups) with the device calls
replaced."""
import numpy as np
import pytest

import diar_ref

L = "SPEAKER %s {} %7.3f %7.3f <NA> <NA> %s <NA> <NA>\n"

# name -> ([(reco, [(start s, end s, key, label)])], the expected lines as (reco, start s, duration s, label))
RTTM_CASES = {
    "disjoint": ([("r", [("0", "1.5", "a", 1), ("2.0", "3.5", "b", 1)])], [("r", 0.0, 1.5, 1), ("r", 2.0, 1.5, 1)]),
    "touching, same label": ([("r", [("0", "1.5", "a", 1), ("1.5", "3", "b", 1)])], [("r", 0.0, 3.0, 1)]),
    "overlapping, same label": ([("r", [("0.75", "2.25", "b", 2), ("0", "1.5", "a", 2)])], [("r", 0.0, 2.25, 2)]),
    # end 1500 > start 751: both move to (1500 + 751) // 2 = 1125
    "overlapping, different labels, odd overlap": ([("r", [("0", "1.5", "a", 1), ("0.751", "2", "b", 2)])],
                                                   [("r", 0.0, 1.125, 1), ("r", 1.125, 0.875, 2)]),
    # b is squeezed to [750, 750] by a and dropped; a and c were not consecutive when pieces merged, so they stay two lines
    "a piece squeezed to zero length": ([("r", [("0", "1", "a", 1), ("0.5", "0.75", "b", 2), ("0.75", "1.5", "c", 1)])],
                                        [("r", 0.0, 0.75, 1), ("r", 0.75, 0.75, 1)]),
    "three speakers interleaved": ([("r", [("0", "1.5", "k0", 1), ("0.75", "2.25", "k1", 2), ("1.5", "3", "k2", 3),
                                           ("2.25", "3.75", "k3", 1)])],
                                   [("r", 0.0, 1.125, 1), ("r", 1.125, 0.75, 2), ("r", 1.875, 0.75, 3), ("r", 2.625, 1.125, 1)]),
    "two recordings": ([("x", [("0", "1", "x0", 1), ("2", "3", "x1", 2)]), ("y", [("0.5", "1", "y0", 1)])],
                       [("x", 0.0, 1.0, 1), ("x", 2.0, 1.0, 2), ("y", 0.5, 0.5, 1)]),
}


@pytest.mark.parametrize("name", sorted(RTTM_CASES))
def test_rttm_rule(name):
    import plda_backend
    recos, want = RTTM_CASES[name]
    ms = [(r, [(plda_backend.parse_ms(a), plda_backend.parse_ms(b), k, l) for a, b, k, l in segs]) for r, segs in recos]
    assert ms == [(r, [(diar_ref.to_ms(a), diar_ref.to_ms(b), k, l) for a, b, k, l in segs]) for r, segs in recos]
    for channel in (0, 3):
        text = plda_backend.rttm_text(ms, channel)
        assert text == "".join(L.format(channel) % w for w in want)
        assert text == diar_ref.rttm(ms, channel)


SEGMENTS = """rA-0 rA 0.00 1.50
rB-0 rB 0.00 1.50
rA-1 rA 0.75 2.25

rB-1 rB 0.75 2.25
rC-0 rC 0 1.5
rA-2 rA 1.5 3.0
rB-2 rB 1.50 2.9996
"""


def test_grouping_and_label_numbering(tmp_path):
    import plda_backend
    p = str(tmp_path / "segments")
    open(p, "w").write(SEGMENTS)
    segs = plda_backend.read_segments(p)
    assert [s[0] for s in segs] == ["rA-0", "rB-0", "rA-1", "rB-1", "rC-0", "rA-2", "rB-2"]
    assert segs[2] == ("rA-1", "rA", 750, 2250) and segs[6] == ("rB-2", "rB", 1500, 3000)
    have = set(s[0] for s in segs) - {"rC-0", "rB-1"}           # rC loses its only vector and vanishes; rB keeps two
    recos, groups, missing = plda_backend.group_segments(segs, have)
    assert recos == ["rA", "rB"] and groups == [[0, 2, 5], [1, 6]] and missing == 2
    r_recos, r_members, r_skipped = diar_ref.group_by_reco(segs, have)
    assert r_recos == recos and [r_members[r] for r in recos] == groups and r_skipped == missing
    # clusters are numbered by their first member, whatever the slots are called
    for slots in ([0, 0, 0], [0, 1, 0], [0, 1, 2], [0, 1, 1], [5, 2, 5, 9, 2], [0]):
        assert plda_backend.number_labels(slots) == diar_ref.number_labels(slots)
    assert plda_backend.number_labels([0, 1, 0, 3, 1]) == [1, 2, 1, 3, 2]


def test_usage_errors_come_before_the_gpu(tmp_path, monkeypatch):
    import plda_backend
    from xvector_amd import hiplib

    class Reached(Exception):
        pass

    def no_gpu():
        raise Reached()

    monkeypatch.setattr(hiplib, "require_gpu", no_gpu)
    q = str(tmp_path)
    open(q + "/segments", "w").write(SEGMENTS)
    open(q + "/backwards", "w").write("k0 r 0.0 1.5\nk1 r 2.0 1.5\n")
    open(q + "/twice", "w").write("k0 r 0.0 1.5\nk0 r 2.0 2.5\n")
    open(q + "/short", "w").write("k0 r 0.0\n")
    open(q + "/counts0", "w").write("rA 2\nrB 0\n")
    open(q + "/counts", "w").write("rA 2\n")
    tail = [q + "/plda", "scp:" + q + "/xvector.scp"]               # neither exists: nothing may be read before the GPU is required
    out = [q + "/labels"]
    bad = [["--threshold", "nan"] + tail + [q + "/segments"] + out,
           ["--rttm-channel", "-1"] + tail + [q + "/segments"] + out,
           ["--reco2num-spk", q + "/counts0"] + tail + [q + "/segments"] + out,
           tail + [q + "/backwards"] + out,
           tail + [q + "/twice"] + out,
           tail + [q + "/short"] + out]
    for argv in bad:
        with pytest.raises(SystemExit) as ei:
            plda_backend.main(["diarize"] + argv)
        assert ei.value.code not in (0, None), argv
    # and a command line with nothing wrong gets as far as requiring the GPU
    with pytest.raises(Reached):
        plda_backend.main(["diarize", "--reco2num-spk", q + "/counts", "--rttm", q + "/rttm"] + tail + [q + "/segments"] + out)
    assert not (tmp_path / "labels").exists() and not (tmp_path / "rttm").exists()


def _ws_bytes(n):
    return 8 * n * n + 24 * n + 64


@pytest.fixture
def host_only(monkeypatch):
    from xvector_amd import hiplib
    monkeypatch.setattr(hiplib, "ahc_average_batch_workspace_bytes", _ws_bytes)
    monkeypatch.setattr(hiplib, "ahc_average_workspace_bytes", _ws_bytes)
    monkeypatch.setattr(hiplib, "require_gpu", lambda: None)


def test_size_order_and_its_inverse():
    from xvector_amd import backend
    sizes = [5, 130, 7, 130, 1, 64]
    order, inverse = backend.size_order(sizes)
    assert order.tolist() == [1, 3, 5, 2, 0, 4]                   # descending, equal sizes in their own order
    assert [sizes[g] for g in order] == [130, 130, 64, 7, 5, 1]
    assert order[inverse].tolist() == list(range(6)) and inverse[order].tolist() == list(range(6))


def test_plan_cuts_calls_under_max_bytes(host_only):
    from xvector_amd import backend
    sizes = [130, 65, 64, 10, 10, 3]
    need = [_ws_bytes(n) for n in sizes]
    calls, routed = backend.plan_ahc_batch(sizes)                  # everything fits one call
    assert routed == [] and len(calls) == 1
    lo, hi, ws0, total = calls[0]
    assert (lo, hi, total) == (0, 6, sum(need)) and ws0.tolist() == np.concatenate([[0], np.cumsum(need)[:-1]]).tolist()
    assert ws0.dtype == np.int64 and all(o % 8 == 0 for o in ws0.tolist())
    # room for the first group and a little more: [130], [65, 64 + small ones as they fit] ...
    limit = need[0] + 100
    calls, routed = backend.plan_ahc_batch(sizes, max_bytes=limit)
    assert routed == [] and [c[:2] for c in calls] == [(0, 1), (1, 6)]
    assert all(c[3] <= limit for c in calls) and calls[1][2][0] == 0
    limit = need[1] + need[2] - 1
    calls, _ = backend.plan_ahc_batch(sizes, max_bytes=need[0])
    assert [c[:2] for c in calls] == [(0, 1), (1, 6)]
    calls, _ = backend.plan_ahc_batch(sizes[1:], max_bytes=limit)
    assert [c[:2] for c in calls] == [(0, 1), (1, 5)] and all(c[3] <= limit for c in calls)
    covered = [g for lo, hi, _, _ in calls for g in range(lo, hi)]
    assert covered == list(range(5))                               # every group once, in order
    with pytest.raises(ValueError, match="max_bytes"):
        backend.plan_ahc_batch(sizes, max_bytes=need[0] - 1)


def test_plan_routes_large_groups(host_only):
    from xvector_amd import backend, hiplib
    sizes = [130, 65, 64, 10]
    calls, routed = backend.plan_ahc_batch(sizes, max_batch_n=64)
    assert routed == [0, 1] and [c[:2] for c in calls] == [(2, 4)]
    # a routed group in the middle splits the run: a call is a run of consecutive groups
    calls, routed = backend.plan_ahc_batch([10, 64, 65, 130, 7], max_batch_n=64)
    assert routed == [2, 3] and [c[:2] for c in calls] == [(0, 2), (4, 5)]
    assert calls[1][2].tolist() == [0]
    # the kernel's own limit caps whatever the caller asks for
    calls, routed = backend.plan_ahc_batch([hiplib.AHC_BATCH_MAX_N, hiplib.AHC_BATCH_MAX_N + 1], max_bytes=1 << 40, max_batch_n=1 << 20)
    assert routed == [1] and [c[:2] for c in calls] == [(0, 1)]


def test_stop_rules():
    from xvector_amd import backend
    thr, minc = backend.diarize_stop_rules([10, 3, 8], 0.25, [None, 5, 2])
    assert thr.tolist() == [0.25, -np.inf, -np.inf] and minc.tolist() == [1, 3, 2]
    r_thr, r_minc = diar_ref.stop_rules([10, 3, 8], 0.25, [None, 5, 2])
    assert thr.tolist() == r_thr and minc.tolist() == r_minc
    thr, minc = backend.diarize_stop_rules([4, 4], -1.0)
    assert thr.tolist() == [-1.0, -1.0] and minc.tolist() == [1, 1]
    for bad in (dict(threshold=float("nan")), dict(num_spk=[1]), dict(num_spk=[0, None])):
        with pytest.raises(ValueError):
            backend.diarize_stop_rules([4, 4], **bad)


def test_diarize_sorts_for_the_device_and_unsorts_the_results(host_only, monkeypatch):
    """backend.diarize with both device stages replaced: the device sees the recordings by size, descending, with their own stop
    rules, and every result comes back to the caller's rows and recordings."""
    from xvector_amd import backend, hiplib
    sizes = [3, 6, 2, 6, 1]
    n = sum(sizes)
    x = np.zeros((n, 4), np.float32)
    x[:, 0] = np.arange(n)                                          # a row's first element names it
    x[:, 1] = np.repeat(np.arange(len(sizes)), sizes)               # ... and its recording
    seen = {}

    def fake_score_blocks(xs, group_sizes, plda, mean=None, transform=None, device=None, target_energy=1.0,
                          pca_max_bytes=backend.PCA_MAX_BYTES, keep_plain=False):
        assert target_energy == 1.0 and pca_max_bytes == backend.PCA_MAX_BYTES and keep_plain is False
        seen["sizes"] = list(group_sizes)
        seen["x"] = np.array(xs)
        return "scores", backend.GroupTables(group_sizes)

    def fake_ahc_batch(scores, tables, thresholds, min_clusters, max_bytes=backend.AHC_MAX_BYTES, max_batch_n=hiplib.AHC_BATCH_MAX_N):
        assert max_bytes == backend.AHC_MAX_BYTES and max_batch_n == hiplib.AHC_BATCH_MAX_N
        assert scores == "scores"
        seen["thr"], seen["minc"] = list(thresholds), list(min_clusters)
        labels, merges, at = [], [], 0
        for g, m in enumerate(tables.sizes.tolist()):
            rows = seen["x"][at:at + m]
            at += m
            assert len(set(rows[:, 1].tolist())) == 1                # a group holds one recording's rows, in their order
            assert rows[:, 0].tolist() == sorted(rows[:, 0].tolist())
            labels.append(np.arange(m, dtype=np.int32) % 2)
            merges.append(("merges of recording", int(rows[0, 1])))
        return labels, merges

    monkeypatch.setattr(backend, "score_blocks", fake_score_blocks)
    monkeypatch.setattr(backend, "ahc_batch", fake_ahc_batch)
    labels, merges = backend.diarize(x, sizes, None, threshold=0.5, num_spk=[None, 2, None, 9, None])
    assert seen["sizes"] == [6, 6, 3, 2, 1]
    assert seen["x"][:, 1].tolist() == [1] * 6 + [3] * 6 + [0] * 3 + [2] * 2 + [4]
    assert seen["thr"] == [-np.inf, -np.inf, 0.5, 0.5, 0.5] and seen["minc"] == [2, 6, 1, 1, 1]
    assert labels.dtype == np.int32
    assert labels.tolist() == [i % 2 for m in sizes for i in range(m)]
    assert merges == [("merges of recording", g) for g in range(len(sizes))]
    with pytest.raises(ValueError):
        backend.diarize(x, [3, 6, 2, 6], None)
    with pytest.raises(ValueError):
        backend.diarize(x, [3, 6, 2, 6, 0, 1], None)


def test_group_tables():
    from xvector_amd import backend
    t = backend.GroupTables([1, 2, 5, 130])
    assert t.row0.tolist() == [0, 1, 3, 8, 138] and t.row0.dtype == np.int32
    assert t.ld.tolist() == [4, 4, 8, 132]
    assert t.score0.tolist() == [0, 4, 12, 52] and t.score0.dtype == np.int64 and t.scores_elems == 52 + 130 * 132
    assert t.max_n == 130 and t.n_rows == 138
    packed = np.arange(t.scores_elems, dtype=np.float32)
    assert t.block(packed, 2).shape == (5, 5) and t.block(packed, 2)[1, 0] == 12 + 8
    assert all(np.array_equal(a, b) for a, b in zip(diar_ref.blocks(packed, [1, 2, 5, 130]), [t.block(packed, g) for g in range(4)]))
    for bad in ([], [3, 0]):
        with pytest.raises(ValueError):
            backend.GroupTables(bad)
