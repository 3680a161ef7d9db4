"""Host side of VBx resegmentation, no GPU: backend.vbx_host (the linear form the kernel uses) against
tests/vbx_ref.py (the generic log-domain form) within the bound of vbx_ref.bound, the ELBO's monotony, the split-cluster case, the
edge cases T = 1, S = 1 and a pi that underflows to 0, the usage errors of `plda_backend.py diarize --vbx`, and the planning of
backend.diarize / backend.vbx_groups with the device calls replaced."""
import numpy as np
import pytest

import vbx_ref


def _host(case, **kw):
    from xvector_amd import backend
    y, lab, S, mdl = vbx_ref.make(case)
    return backend.vbx_host(y, lab, backend.Plda(*mdl), S, **kw)


@pytest.mark.parametrize("case", vbx_ref.CASES, ids=lambda c: "D%d-T%d-S%d" % (c[0], c[1], c[3]))
@pytest.mark.parametrize("iters", [1, 3, 10])
def test_host_twin_against_the_log_domain_reference(case, iters):
    ref, (dg, dp, de) = vbx_ref.reference(case, iters, -np.inf)
    got = _host(case, max_iters=iters, epsilon=-np.inf)
    assert got["info"] == 0 and got["iters"] == iters == ref["iters"]
    eg, ep = np.abs(got["gamma"] - ref["gamma"]).max(), np.abs(got["pi"] - ref["pi"]).max()
    ee = (np.abs(got["elbo"] - ref["elbo"]) / np.abs(ref["elbo"])).max()
    print("gamma %.2e (d %.2e)  pi %.2e (d %.2e)  elbo %.2e (d %.2e)" % (eg, dg, ep, dp, ee, de))
    assert eg <= vbx_ref.bound(dg) and ep <= vbx_ref.bound(dp) and ee <= vbx_ref.bound(de)
    assert ref["margin"] >= 0.5 and np.array_equal(got["labels"], ref["labels"])


@pytest.mark.parametrize("case", vbx_ref.CASES, ids=lambda c: "D%d-T%d-S%d" % (c[0], c[1], c[3]))
def test_elbo_does_not_decrease(case):
    """To rounding: a step may fall short by the rounding of a sum of T + S D terms of the ELBO's size."""
    for e in (_host(case, max_iters=10, epsilon=-np.inf)["elbo"], vbx_ref.reference(case, 10, -np.inf)[0]["elbo"]):
        assert np.all(np.diff(e) >= -1e-12 * np.abs(e[1:]) * (case[1] + case[3] * case[0]))


def test_stop_rule_counts_as_the_reference():
    for case in vbx_ref.CASES:
        ref, _ = vbx_ref.reference(case, 40, 1e-6)
        steps = np.diff(ref["elbo"])
        assert not np.any((steps >= 1e-6 / 1.5) & (steps <= 1.5e-6)), case      # no step near the threshold: the count is robust
        got = _host(case)
        assert got["iters"] == ref["iters"] and len(got["elbo"]) == ref["iters"], case


def test_split_cluster_is_dropped():
    """60 rows in 12 turns of 5, three true speakers, one of them split over two initial labels, three rows mislabelled."""
    y, lab, S, mdl = vbx_ref.make(vbx_ref.SPLIT_CASE)
    assert S == 4 and np.unique(lab).size == 4
    truth = vbx_ref.turns_case(*vbx_ref.SPLIT_CASE[:4], seed=vbx_ref.SPLIT_CASE[4], mdl=mdl)[2]
    assert (np.minimum(lab, 2) != truth).sum() == 3                  # slot 3 is the split half of speaker 2
    got = _host(vbx_ref.SPLIT_CASE)
    assert got["info"] == 0 and got["iters"] < 10
    assert np.unique(got["labels"]).size == 3 and np.sort(got["pi"])[0] < 1e-30
    assert np.array_equal(np.unique(got["labels"], return_inverse=True)[1], truth)    # the turns, exactly
    assert np.array_equal(got["labels"], vbx_ref.reference(vbx_ref.SPLIT_CASE, 40, 1e-6)[0]["labels"])


def test_one_row_and_one_speaker():
    from xvector_amd import backend
    rng = np.random.default_rng(3)
    mdl = vbx_ref.model(5, 1)
    plda = backend.Plda(*mdl)
    y = rng.standard_normal((1, 5)).astype(np.float32)
    for S in (1, 3):                                                # T = 1: gamma_0 = a_0, pi' = gamma_0
        got = backend.vbx_host(y, [S - 1], plda, S, max_iters=4, epsilon=-np.inf)
        ref = vbx_ref.vbx_ref(y, [S - 1], S, *mdl, max_iters=4, epsilon=-np.inf)
        assert got["info"] == 0 and got["gamma"].shape == (1, S) and abs(got["gamma"].sum() - 1) < 1e-15
        assert np.abs(got["gamma"] - ref["gamma"]).max() < 1e-12 and np.abs(got["pi"] - got["gamma"][0]).max() == 0
    y = rng.standard_normal((7, 5)).astype(np.float32)             # S = 1: everything belongs to the one speaker
    got = backend.vbx_host(y, np.zeros(7, int), plda, 1, max_iters=3, epsilon=-np.inf)
    ref = vbx_ref.vbx_ref(y, np.zeros(7, int), 1, *mdl, max_iters=3, epsilon=-np.inf)
    assert np.all(got["gamma"] == 1.0) and got["pi"].tolist() == [1.0] and not got["labels"].any()
    assert np.abs(got["elbo"] - ref["elbo"]).max() <= 1e-12 * np.abs(ref["elbo"]).max()


def test_pi_underflows_to_zero_and_stays_legal():
    """The dropped speaker's pi reaches exactly 0 after enough iterations: no logarithm of pi is taken, nothing turns NaN."""
    got = _host(vbx_ref.SPLIT_CASE, max_iters=60, epsilon=-np.inf)
    ref, (dg, dp, _) = vbx_ref.reference(vbx_ref.SPLIT_CASE, 60, -np.inf)
    assert got["info"] == 0 and got["iters"] == 60 and np.sort(got["pi"])[0] == 0.0 and np.sort(ref["pi"])[0] == 0.0
    assert np.all(np.isfinite(got["gamma"])) and np.all(np.isfinite(got["elbo"])) and np.all(np.isfinite(ref["gamma"]))
    assert np.abs(got["gamma"] - ref["gamma"]).max() <= vbx_ref.bound(dg) and np.abs(got["pi"] - ref["pi"]).max() <= vbx_ref.bound(dp)


def test_a_nan_row_falls_back_to_the_initial_labels():
    from xvector_amd import backend
    y, lab, S, mdl = vbx_ref.make(vbx_ref.SPLIT_CASE)
    y = y.copy()
    y[7, 2] = np.nan
    got = backend.vbx_host(y, lab, backend.Plda(*mdl), S)
    assert got["info"] == 2 and got["iters"] == 1 and np.array_equal(got["labels"], lab)


def test_parameter_ranges():
    from xvector_amd import backend
    assert backend.check_vbx_params() == backend.VBX_DEFAULTS
    assert backend.check_vbx_params(epsilon=-np.inf)["epsilon"] == -np.inf
    for bad in (dict(fa=0.0), dict(fa=np.inf), dict(fb=-1.0), dict(fb=np.nan), dict(loop_prob=1.0), dict(loop_prob=-0.1),
                dict(init_smoothing=-1.0), dict(init_smoothing=np.inf), dict(max_iters=0), dict(max_iters=101), dict(max_iters=2.5),
                dict(epsilon=np.nan)):
        with pytest.raises(ValueError):
            backend.check_vbx_params(**bad)


SEGMENTS = "rA-0 rA 0.00 1.50\nrA-1 rA 0.75 2.25\nrB-0 rB 0.00 1.50\n"


def test_cli_usage_errors_come_before_the_gpu(tmp_path, monkeypatch):
    import plda_backend
    from xvector_amd import hiplib

    class Reached(Exception):
        pass

    def no_gpu():
        raise Reached()

    monkeypatch.setattr(hiplib, "require_gpu", no_gpu)
    q = str(tmp_path)
    tail = [q + "/plda", "scp:" + q + "/xvector.scp", q + "/segments", q + "/labels"]       # none exists: nothing may be read
    for opt in (["--vbx-fa", "0"], ["--vbx-fb", "-3"], ["--vbx-fb", "nan"], ["--vbx-loop-prob", "1"], ["--vbx-max-iters", "0"],
                ["--vbx-max-iters", "101"], ["--vbx-epsilon", "nan"], ["--vbx-init-smoothing", "-1"]):
        with pytest.raises(SystemExit) as ei:
            plda_backend.main(["diarize", "--vbx"] + opt + tail)
        assert ei.value.code not in (0, None), opt
    open(q + "/segments", "w").write(SEGMENTS)
    with pytest.raises(Reached):
        plda_backend.main(["diarize", "--vbx", "--vbx-fa", "0.4", "--vbx-epsilon=-inf", "--rttm", q + "/rttm"] + tail)
    assert not (tmp_path / "labels").exists() and not (tmp_path / "rttm").exists()


@pytest.fixture
def host_only(monkeypatch):
    from xvector_amd import hiplib
    monkeypatch.setattr(hiplib, "require_gpu", lambda: None)


def _rows(sizes):
    n = sum(sizes)
    x = np.zeros((n, 4), np.float32)
    x[:, 0] = np.arange(n)                                          # a row's first element names it
    x[:, 1] = np.repeat(np.arange(len(sizes)), sizes)               # ... and its recording
    return x


def test_diarize_without_vbx_makes_the_calls_it_made(host_only, monkeypatch):
    """vbx=None and the default target energy: the default route asks its two stages for nothing beyond their defaults -- their
    first six (four) arguments are what they were before the PCA and VBx existed, the target energy is 1, keep_plain is False and
    every other parameter has its declared default -- and it touches nothing of the VBx stage."""
    import inspect
    from xvector_amd import backend
    sizes = [3, 6, 2]
    x = _rows(sizes)
    real = dict(score_blocks=backend.score_blocks, ahc_batch=backend.ahc_batch)
    calls = []

    def bound(name, first, a, k):
        """The call's arguments by name; asserts that all but the first ``first`` and those the caller checks hold their defaults."""
        sig = inspect.signature(real[name])
        b = sig.bind(*a, **k)
        b.apply_defaults()
        for p in list(sig.parameters.values())[first:]:
            if p.name not in ("target_energy", "keep_plain"):
                assert b.arguments[p.name] == p.default, (name, p.name)
        calls.append(name)
        return b.arguments

    def fake_score_blocks(*a, **k):
        v = bound("score_blocks", 6, a, k)
        assert np.array_equal(v["x"], x[[3, 4, 5, 6, 7, 8, 0, 1, 2, 9, 10]]) and list(v["group_sizes"]) == [6, 3, 2]
        assert v["plda"] is None and v["mean"] is None and v["transform"] is None and v["device"] == "cuda:0"
        assert backend.target_energy_is_one(v["target_energy"]) and v["keep_plain"] is False
        return "scores", backend.GroupTables(v["group_sizes"])

    def fake_ahc_batch(*a, **k):
        v = bound("ahc_batch", 4, a, k)
        assert v["scores"] == "scores" and v["tables"].sizes.tolist() == [6, 3, 2]
        assert list(v["thresholds"]) == [0.5] * 3 and list(v["min_clusters"]) == [1] * 3
        return [np.zeros(m, np.int32) for m in v["tables"].sizes.tolist()], ["m"] * v["tables"].sizes.size

    def never(*a, **k):
        raise AssertionError("the VBx stage ran")

    monkeypatch.setattr(backend, "score_blocks", fake_score_blocks)
    monkeypatch.setattr(backend, "ahc_batch", fake_ahc_batch)
    for name in ("vbx_groups", "_diarize_vbx", "prepare", "check_vbx_params"):
        monkeypatch.setattr(backend, name, never)
    labels, merges = backend.diarize(x, sizes, None, threshold=0.5)
    assert calls == ["score_blocks", "ahc_batch"]
    assert labels.tolist() == [0] * 11 and merges == ["m"] * 3


def test_diarize_with_vbx_hands_over_rows_labels_and_time_order(host_only, monkeypatch):
    """vbx={...}: the recordings that run are gathered from the PLAIN rows in the device's order with their compacted cluster
    labels, speaker counts and time order; kept recordings, recordings above the speaker cap and info-2 recordings keep their
    clustering; the report comes back in the caller's order."""
    import torch
    from xvector_amd import backend, hiplib
    sizes = [3, 70, 2, 6, 4]                                        # device order: 1, 3, 4, 0, 2
    x = _rows(sizes)
    n = x.shape[0]
    seen = {}

    def fake_score_blocks(xs, group_sizes, plda, mean=None, transform=None, device=None, target_energy=1.0,
                          pca_max_bytes=backend.PCA_MAX_BYTES, keep_plain=False):
        assert keep_plain and target_energy == 1.0 and pca_max_bytes == backend.PCA_MAX_BYTES
        t = backend.GroupTables(group_sizes)
        t.plain = torch.as_tensor(np.array(xs))
        return "scores", t

    def fake_ahc_batch(scores, tables, thresholds, min_clusters, max_bytes=backend.AHC_MAX_BYTES, max_batch_n=hiplib.AHC_BATCH_MAX_N):
        assert max_bytes == backend.AHC_MAX_BYTES and max_batch_n == hiplib.AHC_BATCH_MAX_N
        # recording 1 (70 rows): 70 clusters, above the cap; the others: slots 0 and 5 alternating
        return [np.arange(m, dtype=np.int32) if m == 70 else (np.arange(m, dtype=np.int32) % 2) * 5 for m in tables.sizes.tolist()], \
               [None] * tables.sizes.size

    def fake_vbx_groups(y_rows, tables, init_labels, plda, time_order=None, n_spk=None, max_bytes=None, **params):
        seen.update(y=y_rows.numpy().copy(), sizes=tables.sizes.tolist(), init=np.array(init_labels), order=np.array(time_order),
                    n_spk=np.array(n_spk), params=params, max_bytes=max_bytes)
        G = tables.sizes.size
        return dict(labels=np.full(tables.n_rows, 7, np.int32), iters=np.arange(1, G + 1, dtype=np.int32),
                    info=np.asarray([0, 2, 0][:G], np.int32))

    class FakePlda(object):
        dim = 4

    monkeypatch.setattr(backend, "score_blocks", fake_score_blocks)
    monkeypatch.setattr(backend, "ahc_batch", fake_ahc_batch)
    monkeypatch.setattr(backend, "vbx_groups", fake_vbx_groups)
    order = np.concatenate([np.arange(m)[::-1] for m in sizes])     # every recording backwards in time
    keep = np.asarray([False, False, True, False, False])
    rep = {}
    labels, _ = backend.diarize(x, sizes, FakePlda(), vbx=dict(fa=0.5, time_order=order, keep=keep, max_bytes=123), vbx_report=rep)
    # ran, in the device's order: recordings 3, 4, 0 (1 is above the cap, 2 is kept)
    assert seen["sizes"] == [6, 4, 3] and seen["y"][:, 1].tolist() == [3] * 6 + [4] * 4 + [0] * 3
    assert seen["y"][:, 0].tolist() == sorted(seen["y"][:6, 0].tolist()) + sorted(seen["y"][6:10, 0].tolist()) + sorted(seen["y"][10:, 0].tolist())
    assert seen["init"].tolist() == [0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0] and seen["n_spk"].tolist() == [2, 2, 2]
    assert seen["order"].tolist() == [5, 4, 3, 2, 1, 0, 3, 2, 1, 0, 2, 1, 0]
    assert seen["params"] == dict(backend.VBX_DEFAULTS, fa=0.5) and seen["max_bytes"] == 123
    row0 = np.concatenate([[0], np.cumsum(sizes)])
    per = [labels[row0[g]:row0[g + 1]].tolist() for g in range(5)]
    assert per[3] == [7] * 6 and per[0] == [7] * 3                  # VBx's labels
    assert per[4] == [0, 5, 0, 5]                                   # info 2: the clustering
    assert per[1] == list(range(70)) and per[2] == [0, 5]           # above the cap; kept
    assert rep["ran"].tolist() == [True, False, False, True, True] and rep["iters"].tolist() == [3, 0, 0, 1, 2]
    assert rep["info"].tolist() == [0, 0, 0, 0, 2] and rep["spk_before"].tolist() == [2, 70, 2, 2, 2]
    assert rep["spk_after"].tolist() == [1, 70, 2, 1, 2]
    assert hiplib.VBX_MAX_SPK == 64
    with pytest.raises(ValueError):
        backend.diarize(x, sizes, FakePlda(), vbx=dict(loop_prob=1.0))
    with pytest.raises(ValueError):
        backend.diarize(x, sizes, FakePlda(), vbx=dict(keep=keep[:3]))


def test_plan_cuts_calls_under_max_bytes(monkeypatch):
    from xvector_amd import backend, hiplib
    monkeypatch.setattr(hiplib, "vbx_groups_workspace_bytes", lambda n, g, d, s: 8 * (n * (d + 3 + 3 * s) + g * 2 * s * d))
    row0 = np.concatenate([[0], np.cumsum([100, 50, 50, 10])])
    per = lambda n, g: 8 * (n * (16 + 3 + 12) + g * 2 * 4 * 16)
    assert backend.plan_vbx_groups(row0, 16, 4) == [(0, 4)]
    assert backend.plan_vbx_groups(row0, 16, 4, max_bytes=per(100, 2)) == [(0, 1), (1, 3), (3, 4)]
    assert backend.plan_vbx_groups(row0, 16, 4, max_bytes=per(110, 3)) == [(0, 1), (1, 4)]
    with pytest.raises(ValueError, match="max_bytes"):
        backend.plan_vbx_groups(row0, 16, 4, max_bytes=per(100, 1) - 1)
    with pytest.raises(ValueError, match="max_bytes"):
        backend.plan_vbx_groups([0, 10, 110], 16, 4, max_bytes=per(50, 1))
