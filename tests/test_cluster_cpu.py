"""Host side of clustering-based PLDA adaptation, no GPU: the test reference of the clustering kernel against
scipy, labels_from_merges, interpolate_plda and the two subcommands of plda_backend.py."""
import os

import numpy as np
import pytest

import ahc_ref
import backend_ref as ref


def _sym_scores(rng, n):
    s = rng.standard_normal((n, n)).astype(np.float32)
    return np.triu(s, 1) + np.triu(s, 1).T


def _partition(labels):
    """A partition as a set of frozensets: independent of how the clusters are named."""
    out = {}
    for i, l in enumerate(np.asarray(labels).tolist()):
        out.setdefault(l, []).append(i)
    return set(frozenset(v) for v in out.values())


@pytest.mark.parametrize("n,seed", [(2, 0), (17, 1), (130, 2), (300, 3)])
def test_reference_against_scipy(n, seed):
    hierarchy = pytest.importorskip("scipy.cluster.hierarchy")
    rng = np.random.default_rng(seed)
    s = _sym_scores(rng, n)                                       # continuous draws: no ties
    big = float(np.abs(s).max())
    C = float(s.max()) + 1.0
    iu = np.triu_indices(n, 1)
    Z = hierarchy.linkage(C - s[iu].astype(np.float64), method="average")      # the condensed form is the row-major upper triangle
    a, b, sc = ahc_ref.dendrogram(s)
    # average linkage is linear in the similarities: height = C - average score
    got, want = np.sort(C - sc), np.sort(Z[:, 2])
    print("n %d: max |height - scipy| = %.3e (bound %.3e)" % (n, np.abs(got - want).max(), 1e-12 * big))
    assert np.abs(got - want).max() <= 1e-12 * big
    for thr in (0.5, 0.0, -0.3):
        lab, merges = ahc_ref.ahc(s, threshold=thr)
        if len(merges[0]) < n - 1 and min(abs(sc - thr)) > 1e-9:        # a cut that falls between two heights
            want_lab = hierarchy.fcluster(Z, C - thr, criterion="distance")
            assert _partition(lab) == _partition(want_lab)


@pytest.mark.parametrize("kind", ["normal", "ties"])
def test_reference_compaction_changes_nothing(kind):
    rng = np.random.default_rng(7)
    n = 150
    s = _sym_scores(rng, n) if kind == "normal" else rng.integers(-2, 3, (n, n)).astype(np.float32)
    p, q = ahc_ref.dendrogram(s, compact=True), ahc_ref.dendrogram(s, compact=False)
    assert all(np.array_equal(x, y) for x, y in zip(p, q))
    a, b, sc = p
    assert np.all(a < b)
    lab, (ca, cb, cs) = ahc_ref.ahc(s, threshold=-np.inf, min_clusters=5)
    assert len(ca) == n - 5 and len(set(lab.tolist())) == 5 and np.array_equal(ca, a[:n - 5])
    assert all(lab[i] == min(j for j in range(n) if lab[j] == lab[i]) for i in range(n))     # the slot is the smallest member


def test_reference_tie_rule_by_hand():
    # all scores equal: every step merges the lexicographically smallest live pair, (0, 1) then (0, 2) ...; averages stay 1
    a, b, sc = ahc_ref.dendrogram(np.ones((4, 4), np.float32))
    assert a.tolist() == [0, 0, 0] and b.tolist() == [1, 2, 3] and sc.tolist() == [1.0, 1.0, 1.0]
    # (1, 3) and (2, 3) tie at the top: (1, 3) is first; then {1, 3}-2 averages (0 + 5) / 2 against (0, 1) = (0, 2) = 1
    s = np.array([[0, 1, 1, 1], [0, 0, 0, 5], [0, 0, 0, 5], [0, 0, 0, 0]], np.float32)
    a, b, sc = ahc_ref.dendrogram(s)
    assert (a[0], b[0], sc[0]) == (1, 3, 5.0) and (a[1], b[1], sc[1]) == (1, 2, 2.5) and (a[2], b[2], sc[2]) == (0, 1, 1.0)
    lab, m = ahc_ref.ahc(s, threshold=2.0)
    assert lab.tolist() == [0, 1, 1, 1] and len(m[0]) == 2
    lab, m = ahc_ref.ahc(np.zeros((1, 1), np.float32))
    assert lab.tolist() == [0] and len(m[0]) == 0


def test_labels_from_merges():
    from xvector_amd import backend
    assert backend.labels_from_merges(5, [], []).tolist() == [0, 1, 2, 3, 4]
    assert backend.labels_from_merges(5, [3, 1, 0], [4, 3, 2]).tolist() == [0, 1, 0, 1, 1]
    assert backend.labels_from_merges(4, [2, 1, 0], [3, 2, 1]).tolist() == [0, 0, 0, 0]            # a chain
    assert backend.labels_from_merges(1, [], []).dtype == np.int32
    rng = np.random.default_rng(3)
    s = _sym_scores(rng, 60)
    lab, (a, b, _) = ahc_ref.ahc(s, threshold=0.2)
    assert np.array_equal(backend.labels_from_merges(60, a, b), lab)
    for bad in (([1], [1]), ([2], [1]), ([0, 0], [1, 1]), ([0, 1], [1, 2]), ([0], [5])):
        with pytest.raises(ValueError):
            backend.labels_from_merges(4, *bad)


def _model(d, seed):
    from xvector_amd import backend
    rng = np.random.default_rng(seed)
    a, b = rng.standard_normal((d, d)), rng.standard_normal((d, d))
    return backend.plda_from_covariances(rng.standard_normal(d), b @ b.T / d + 0.2 * np.eye(d), a @ a.T / d + 0.5 * np.eye(d))


def _llr_matrix(plda, x, y):
    """float64 LLR of every x (one-utterance enrolment) against every y, through tests/backend_ref.py."""
    pl = (plda.mean, plda.transform, plda.psi)
    n1 = np.ones(len(x))
    rows, r = ref.side_rows_enrol(ref.chain(x, None, None, False, pl, n1), n1, plda.psi)
    return rows @ ref.side_rows_test(ref.chain(y, None, None, False, pl, None)).T + r[:, None]


def test_interpolate_plda():
    from xvector_amd import backend
    d = 12
    p_out, p_in = _model(d, 1), _model(d, 2)
    rng = np.random.default_rng(0)
    x, y = rng.standard_normal((20, d)) * 2, rng.standard_normal((30, d)) * 2
    for alpha, want in ((0.0, p_out), (1.0, p_in)):
        got = backend.interpolate_plda(p_out, p_in, alpha)
        g, w = _llr_matrix(got, x, y), _llr_matrix(want, x, y)
        err = np.abs(g - w).max() / np.abs(w).max()
        print("alpha %g: max relative LLR difference %.3e" % (alpha, err))
        assert err <= 1e-9
    h1, h2 = backend.interpolate_plda(p_out, p_in, 0.5), backend.interpolate_plda(p_in, p_out, 0.5)
    g, w = _llr_matrix(h1, x, y), _llr_matrix(h2, x, y)
    assert np.abs(g - w).max() / np.abs(w).max() <= 1e-9
    assert np.all(np.diff(h1.psi) <= 0) and np.all(h1.psi >= 0)
    # the mix is linear in the covariances: W(0.25) = 0.75 W_out + 0.25 W_in
    q = backend.interpolate_plda(p_out, p_in, 0.25)
    cov = lambda p: np.linalg.inv(p.transform) @ np.linalg.inv(p.transform).T
    assert np.allclose(cov(q), 0.75 * cov(p_out) + 0.25 * cov(p_in), rtol=1e-10, atol=1e-12)
    assert np.allclose(q.mean, 0.75 * p_out.mean + 0.25 * p_in.mean, rtol=1e-12, atol=1e-14)
    for alpha in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            backend.interpolate_plda(p_out, p_in, alpha)
    with pytest.raises(ValueError):
        backend.interpolate_plda(p_out, _model(d + 1, 3), 0.5)


@pytest.mark.parametrize("binary", ["true", "false"])
def test_interpolate_plda_cli(tmp_path, binary):
    import plda_backend
    from xvector_amd import backend
    d = 8
    p_out, p_in = _model(d, 4), _model(d, 5)
    p = str(tmp_path)
    backend.write_plda(p + "/out", p_out)
    backend.write_plda(p + "/in", p_in, binary=False)
    plda_backend.main(["interpolate-plda", "--alpha", "0.25", "--binary", binary, p + "/out", p + "/in", p + "/mix"])
    got = backend.read_plda(p + "/mix")
    want = backend.interpolate_plda(backend.read_plda(p + "/out"), backend.read_plda(p + "/in"), 0.25)
    tol = dict(rtol=1e-6, atol=1e-6) if binary == "true" else dict(rtol=0, atol=0)       # the binary form stores float32
    assert np.allclose(got.mean, want.mean, **tol) and np.allclose(got.transform, want.transform, **tol)
    assert np.allclose(got.psi, want.psi, **tol)
    assert open(p + "/mix", "rb").read(2) == (b"\x00B" if binary == "true" else b"<P")
    for argv, word in ((["interpolate-plda", "--alpha", "1.5", p + "/out", p + "/in", p + "/bad1"], "alpha"),):
        with pytest.raises(SystemExit) as ei:
            plda_backend.main(argv)
        assert word in str(ei.value)
    backend.write_plda(p + "/other", _model(d + 1, 6))
    with pytest.raises(SystemExit) as ei:
        plda_backend.main(["interpolate-plda", p + "/out", p + "/other", p + "/bad2"])
    assert "dimensions" in str(ei.value)
    assert not os.path.exists(p + "/bad1") and not os.path.exists(p + "/bad2")


def test_subcommands_parse():
    import plda_backend
    for argv in (["cluster"], ["interpolate-plda", "a"], ["cluster", "--threshold", "x", "p", "ark:v", "o"]):
        with pytest.raises(SystemExit) as ei:
            plda_backend.main(argv)
        assert ei.value.code == 2                                          # argparse's usage error
    assert "cluster" in plda_backend.__doc__ and "interpolate-plda" in plda_backend.__doc__


def test_cluster_needs_a_gpu(tmp_path, monkeypatch):
    """Without a GPU `cluster` fails in require_gpu, before it reads anything, and writes no file."""
    import torch
    import plda_backend
    from xvector_amd import backend, hiplib
    monkeypatch.setattr(hiplib, "_GPU_SEEN", [])
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    out = str(tmp_path / "utt2cluster")
    with pytest.raises(hiplib.XvectorHipError):
        plda_backend.main(["cluster", str(tmp_path / "no_such_plda"), "ark:" + str(tmp_path / "no_such_ark"), out])
    assert not os.path.exists(out)
    with pytest.raises(hiplib.XvectorHipError):
        backend.cluster_vectors(np.ones((3, 4), np.float32), backend.Plda(np.zeros(4), np.eye(4), np.ones(4)))
    with pytest.raises(hiplib.XvectorHipError):
        backend.ahc(torch.zeros((3, 3)))
