"""The host side of the per-recording PCA, no GPU: backend.est_pca and Plda.apply_transform against
tests/pca_ref.py, the energy rule on hand-made spectra, the fallbacks, the emulated rotation order, the command line's usage
errors and the ABI."""
import numpy as np
import pytest

import pca_ref


def _rows(rng, d, n, n_spk=3):
    centers = rng.standard_normal((n_spk, d))
    y = centers[rng.integers(0, n_spk, n)] + 0.6 * rng.standard_normal((n, d))
    y *= np.sqrt(d) / np.linalg.norm(y, axis=1, keepdims=True)
    return y.astype(np.float32)


def _model(rng, d):
    from xvector_amd import backend
    g, h = rng.standard_normal((d, d)), rng.standard_normal((d, d))
    W = np.eye(d) + 0.3 * g @ g.T / d
    B = (h * (2.0 * 0.9 ** np.arange(d))) @ h.T / d + 0.05 * np.eye(d)
    return backend.plda_from_covariances(0.1 * rng.standard_normal(d), B, W), W, B


@pytest.mark.parametrize("d,n", [(7, 30), (16, 5), (40, 200), (128, 60)])
@pytest.mark.parametrize("target", [0.1, 0.5, 0.9])
def test_est_pca_and_apply_transform(d, n, target):
    from xvector_amd import backend
    rng = np.random.default_rng(d * 1000 + n)
    y = _rows(rng, d, n)
    plda, W, B = _model(rng, d)
    want = pca_ref.est_pca(y, target)
    assert want["margin"] >= 1e-9
    A, s = backend.est_pca(y, target)
    p = want["p"]
    assert A.shape == (p, d) and s.shape == (d,) and np.all(np.diff(s) <= 0)
    scale = d * 2.0 ** -52 * np.linalg.norm(want["C"], 2)
    assert np.abs(s - want["eigvals"]).max() <= 8 * scale
    assert np.abs(A @ A.T - np.eye(p)).max() <= 8 * d * 2.0 ** -52
    assert np.abs(A @ want["C"] @ A.T - np.diag(s[:p])).max() <= 8 * scale
    at = np.argmax(np.abs(A), axis=1)
    assert np.all(A[np.arange(p), at] > 0)
    # the model's covariances come back from its transform and psi
    W2, B2 = plda.covariances()
    assert np.abs(W2 - W).max() <= 1e-12 * np.abs(W).max() and np.abs(B2 - B).max() <= 1e-12 * np.abs(B).max()
    pg = plda.apply_transform(A)
    ref = pca_ref.project(plda.mean, plda.transform, plda.psi, A)
    assert pg.dim == p and np.all(pg.psi >= 0) and np.all(np.diff(pg.psi) <= 0)
    assert np.abs(pg.psi - ref["psi"]).max() <= 1e-11 * max(1.0, ref["psi"][0])
    Pg = pg.transform
    assert np.abs(Pg @ ref["W"] @ Pg.T - np.eye(p)).max() <= 1e-11
    assert np.abs(Pg @ ref["B"] @ Pg.T - np.diag(pg.psi)).max() <= 1e-11 * max(1.0, ref["psi"][0])
    assert np.array_equal(pg.mean, A @ plda.mean)
    # the score does not depend on the basis chosen inside the retained subspace
    q, _ = np.linalg.qr(rng.standard_normal((p, p)))
    rot = plda.apply_transform(q @ A)
    e1, r1, t1 = pca_ref.operand_rows(y, pg.transform @ A, -(pg.transform @ pg.mean), pg.psi)
    e2, r2, t2 = pca_ref.operand_rows(y, rot.transform @ q @ A, -(rot.transform @ rot.mean), rot.psi)
    s1, s2 = e1 @ t1.T + r1[:, None], e2 @ t2.T + r2[:, None]
    assert np.abs(s1 - s2).max() <= 1e-9 * max(1.0, np.abs(s1).max())
    tabs = backend.host_pca_tables(y, [n], plda, target)
    assert tabs["dim"].tolist() == [p] and tabs["info"].tolist() == [0]
    assert np.array_equal(tabs["map"][0, :p], pg.transform @ A) and np.all(tabs["map"][0, p:] == 0)


def test_energy_rule():
    from xvector_amd import backend
    s = np.array([4.0, 3.0, 2.0, 1.0])
    assert backend.energy_dim(s, 0.39) == 2                            # 0.4 > 0.39: k = 1, p = 2
    assert backend.energy_dim(s, 0.41) == 3                            # 0.7 > 0.41: k = 2, p = 3
    assert backend.energy_dim(s, 0.95) == 4                            # k = 4: capped at d
    assert backend.energy_dim(s, 0.8) == 4                             # k = 3, p = 4 = d
    assert backend.energy_dim(s, 1.0) == 4                             # no count exceeds 1
    assert backend.energy_dim(np.array([5.0]), 0.1) == 1
    assert backend.energy_dim(np.zeros(4), 0.5) is None and backend.energy_dim(np.array([np.nan, 1.0]), 0.5) is None
    assert backend.energy_dim(np.array([-1.0, -2.0]), 0.5) is None
    for t in (0.39, 0.41, 0.8, 0.95):
        assert pca_ref.energy_rule(s, t)[0] == backend.energy_dim(s, t)
    # ties keep the smaller original column in front; the sign makes the first component of largest magnitude positive
    u = np.array([[0.6, 0.0, -0.8], [0.0, -1.0, 0.0], [-0.8, 0.0, -0.6]])
    vals, rows = backend.order_eigenpairs(np.array([2.0, 3.0, 2.0]), u)
    assert vals.tolist() == [3.0, 2.0, 2.0]
    assert np.array_equal(rows, np.array([[0.0, 1.0, 0.0], [-0.6, 0.0, 0.8], [0.8, 0.0, 0.6]]))
    tie = np.array([[0.5, 0.5], [-0.5, -0.5]])                         # equal magnitudes: the first component decides
    assert np.array_equal(backend.order_eigenpairs(np.array([1.0, 1.0]), tie.T)[1], np.array([[0.5, 0.5], [0.5, 0.5]]))


def test_fallbacks_and_the_approximate_one():
    from xvector_amd import backend
    rng = np.random.default_rng(3)
    y = _rows(rng, 12, 4)
    assert backend.est_pca(y[:1], 0.5) is None                          # one vector: C = 0
    assert backend.est_pca(np.repeat(y[:1], 4, axis=0), 0.5) is None    # identical vectors: every sum is exact, C = 0
    bad = y.copy()
    bad[2, 3] = np.nan
    assert backend.est_pca(bad, 0.5) is None
    assert pca_ref.est_pca(y[:1], 0.5) is None
    plda, _, _ = _model(rng, 12)
    tabs = backend.host_pca_tables(np.concatenate([y, y[:1]]), [4, 1], plda, 0.5)
    assert tabs["info"].tolist() == [0, 1] and tabs["dim"][1] == 12 and np.array_equal(tabs["map"][1], plda.transform)
    assert np.array_equal(tabs["psi"][1], plda.psi)
    for t in (1.0, 0.9995, 1.001, 0.999001):
        assert backend.target_energy_is_one(t) and backend.check_target_energy(t) == t
    for t in (0.99, 0.5, 1e-9):
        assert not backend.target_energy_is_one(t) and backend.check_target_energy(t) == t
    for t in (0.0, -0.1, 1.01, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            backend.check_target_energy(t)
    with pytest.raises(ValueError):
        plda.apply_transform(np.zeros((3, 11)))


@pytest.mark.parametrize("d,n", [(2, 5), (7, 30), (8, 3), (33, 100)])
def test_emulated_rotation_order(d, n):
    """The round-robin tournament meets every pair once per sweep, and the emulated iteration agrees with eigh."""
    m = (d + 1) & ~1
    seen = set()
    for r in range(m - 1):
        p, q = pca_ref.round_robin_pairs(m, r)
        assert np.all(p < q) and len(set(p.tolist()) | set(q.tolist())) == m
        seen |= set(zip(p.tolist(), q.tolist()))
    assert len(seen) == m * (m - 1) // 2
    c = pca_ref.covariance(_rows(np.random.default_rng(d), d, n))
    eig, res_i, res_c, sweeps = pca_ref.emulation_ratios(c)
    assert max(eig, res_i, res_c) <= 8 and sweeps <= pca_ref.MAX_SWEEPS


def test_cli_usage_errors(tmp_path):
    """A bad --target-energy exits before the GPU is required and before any file is read: the files do not exist."""
    import plda_backend
    tail = [str(tmp_path / "plda"), "scp:" + str(tmp_path / "x.scp"), str(tmp_path / "segments"), str(tmp_path / "labels")]
    for bad in ("0", "-0.5", "1.5", "nan", "inf"):
        with pytest.raises(SystemExit) as ei:
            plda_backend.main(["diarize", "--target-energy", bad] + tail)
        assert "--target-energy" in str(ei.value), bad
    for good in ("1.0", "0.5", "0.9999"):
        with pytest.raises((SystemExit, OSError)) as ei:                # accepted: the next thing to fail is the missing file
            plda_backend.main(["diarize", "--target-energy", good] + tail)
        assert "--target-energy" not in str(ei.value), good
    with pytest.raises(SystemExit):
        plda_backend.main(["diarize", "--target-energy", "half"] + tail)
    assert not (tmp_path / "labels").exists()


def test_abi():
    from xvector_amd import hiplib
    new = {"xv_pca_plda_groups_f64", "xv_pca_plda_groups_workspace_bytes", "xv_backend_prepare_groups_f32"}
    assert hiplib.ABI_VERSION >= 40 and new <= set(hiplib.SYMBOLS)
    lib = hiplib.load()
    assert lib.xv_version() == hiplib.ABI_VERSION and all(getattr(lib, s) is not None for s in new)
    assert hiplib.PCA_MAX_DIM == 128 and hiplib.PCA_MAX_SWEEPS == pca_ref.MAX_SWEEPS
    assert hiplib.pca_plda_groups_workspace_bytes(3, 128) == 3 * 4 * 128 * 128 * 8
    assert hiplib.pca_plda_groups_workspace_bytes(3, 129) == 0 and hiplib.pca_plda_groups_workspace_bytes(0, 16) == 0
