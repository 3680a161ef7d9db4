"""The scoring back-end's host side: the LLR algebra against a direct two-Gaussian ratio, the PLDA EM and the LDA fit against
their defining properties (and sklearn), Kaldi <Plda> / transform.mat I/O, the EER against sklearn's ROC, and no silent CPU
fallback."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import backend_ref as ref
from conftest import ROOT, TWIN


@pytest.mark.parametrize("n", [1, 3, 8])
@pytest.mark.parametrize("d", [1, 7, 50])
def test_llr_closed_form_is_the_gaussian_ratio(n, d):
    from scipy.stats import multivariate_normal
    rng = np.random.default_rng(n * 100 + d)
    psi = rng.uniform(0.1, 4.0, d)
    Psi, I = np.diag(psi), np.eye(d)
    same = np.block([[Psi + I / n, Psi], [Psi, Psi + I]])
    diff = np.block([[Psi + I / n, np.zeros((d, d))], [np.zeros((d, d)), Psi + I]])
    zs = rng.standard_normal((6, d)) * 1.5
    ts = rng.standard_normal((6, d)) * 1.5
    for z, t in zip(zs, ts):
        x = np.concatenate([z, t])
        direct = multivariate_normal(np.zeros(2 * d), same).logpdf(x) - multivariate_normal(np.zeros(2 * d), diff).logpdf(x)
        closed = ref.llr(z, n, t, psi)
        assert abs(closed - direct) <= 1e-9 * max(1.0, abs(direct)), (closed, direct)
        rows, r = ref.side_rows_enrol(z[None], [n], psi)
        packed = rows[0] @ ref.side_rows_test(t[None])[0] + r[0]
        assert abs(packed - closed) <= 1e-10 * max(1.0, abs(closed))


def _two_cov_data(rng, n_spk, d):
    a = rng.standard_normal((d, d)) / np.sqrt(d)
    B = a @ a.T * 2.0 + 0.5 * np.eye(d)
    c = rng.standard_normal((d, d)) / np.sqrt(d)
    W = c @ c.T + 0.5 * np.eye(d)
    mu = rng.standard_normal(d)
    ys = rng.multivariate_normal(np.zeros(d), B, n_spk)
    xs, groups, i = [], [], 0
    for s in range(n_spk):
        n = int(rng.integers(2, 13))
        xs.append(mu + ys[s] + rng.multivariate_normal(np.zeros(d), W, n))
        groups.append(np.arange(i, i + n))
        i += n
    return np.vstack(xs), groups, mu, B, W


def _marginal_ll(x, groups, mu, B, W):
    """Exact log-likelihood of the two-covariance model: each speaker's stacked vectors ~ N(mu, I_n (x) W + 1 1^T (x) B)."""
    from scipy.stats import multivariate_normal
    by_n = {}
    for g in groups:
        by_n.setdefault(len(g), []).append(x[g].ravel())
    d = x.shape[1]
    total = 0.0
    for n, rows in by_n.items():
        cov = np.kron(np.eye(n), W) + np.kron(np.ones((n, n)), B)
        total += multivariate_normal(np.tile(mu, n), cov).logpdf(np.array(rows)).sum()
    return total


def test_plda_fit_properties():
    from xvector_amd import backend
    rng = np.random.default_rng(0)
    d = 20
    x, groups, mu, B, W = _two_cov_data(rng, 2000, d)
    plda, hist = backend.fit_plda(x, groups, num_em_iters=10, return_history=True)
    means = np.array([x[g].mean(axis=0) for g in groups])
    mu_hat = means.mean(axis=0)
    assert np.allclose(plda.mean, mu_hat)
    lls = [_marginal_ll(x, groups, mu_hat, np.eye(d), np.eye(d))] + [_marginal_ll(x, groups, mu_hat, b, w) for b, w in hist]
    steps = np.diff(lls)
    assert np.all(steps >= -1e-8 * abs(lls[-1])), steps
    Bh, Wh = hist[-1]
    print("PLDA fit: relative Frobenius error B %.3f, W %.3f" % (np.linalg.norm(Bh - B) / np.linalg.norm(B),
                                                                 np.linalg.norm(Wh - W) / np.linalg.norm(W)))
    assert np.linalg.norm(Bh - B) / np.linalg.norm(B) <= 0.10
    assert np.linalg.norm(Wh - W) / np.linalg.norm(W) <= 0.10
    P = plda.transform
    assert np.abs(P @ Wh @ P.T - np.eye(d)).max() <= 1e-10
    assert np.abs(P @ Bh @ P.T - np.diag(plda.psi)).max() <= 1e-10
    assert np.all(np.diff(plda.psi) <= 0)


def test_plda_skips_single_utterance_speakers(caplog):
    from xvector_amd import backend
    rng = np.random.default_rng(1)
    x, groups, _, _, _ = _two_cov_data(rng, 50, 4)
    extra = np.vstack([x, rng.standard_normal((3, 4))])
    with caplog.at_level("INFO", logger="plda_backend"):
        a = backend.fit_plda(extra, groups + [np.array([len(x)]), np.array([len(x) + 1]), np.array([len(x) + 2])])
    b = backend.fit_plda(x, groups)
    assert np.array_equal(a.transform, b.transform)
    assert "Skipping 3 speakers with only one utterance" in caplog.text
    assert "(3 with only one utterance, skipped)" in caplog.text


def test_lda_fit_properties():
    from scipy.linalg import subspace_angles
    from sklearn.discriminant_analysis import LinearDiscriminantAnalysis
    from xvector_amd import backend
    rng = np.random.default_rng(2)
    D, C, per, dim = 30, 25, 40, 10
    centres = rng.standard_normal((C, D)) * np.linspace(3.0, 0.2, D)
    mix = rng.standard_normal((D, D)) / np.sqrt(D) + np.eye(D)
    x = np.vstack([centres[c] + rng.standard_normal((per, D)) @ mix for c in range(C)])
    labels = np.repeat(np.arange(C), per)
    t = backend.fit_lda(x, labels, dim)
    A = t[:, :D]
    assert np.allclose(t[:, D], -A @ x.mean(axis=0))
    mean, sw, st = backend.scatter_matrices(x, labels)
    sb = st - sw
    assert np.abs(A @ sw @ A.T - np.eye(dim)).max() <= 1e-9
    proj = A @ sb @ A.T
    assert np.abs(proj - np.diag(np.diag(proj))).max() <= 1e-9 * np.abs(proj).max()
    assert np.all(np.diff(np.diag(proj)) <= 0)
    sk = LinearDiscriminantAnalysis(solver="eigen").fit(x, labels)
    angles = subspace_angles(A.T, sk.scalings_[:, :dim])
    assert angles.max() <= 1e-6, angles.max()


def test_plda_io_round_trips(tmp_path):
    from xvector_amd import backend
    rng = np.random.default_rng(4)
    d = 6
    plda = backend.Plda(rng.standard_normal(d), rng.standard_normal((d, d)), np.sort(rng.uniform(0, 3, d))[::-1])
    for binary in (True, False):
        p1, p2 = str(tmp_path / ("a%d" % binary)), str(tmp_path / ("b%d" % binary))
        backend.write_plda(p1, plda, binary=binary)
        back = backend.read_plda(p1)
        for a, b in ((plda.mean, back.mean), (plda.transform, back.transform), (plda.psi, back.psi)):
            assert np.array_equal(a, b)
        backend.write_plda(p2, back, binary=binary)
        assert open(p1, "rb").read() == open(p2, "rb").read()
    assert open(str(tmp_path / "a0"), "rb").read().startswith(b"<Plda>  [ ")
    m = rng.standard_normal((4, 7)).astype(np.float32)
    for binary in (True, False):
        p = str(tmp_path / ("t%d.mat" % binary))
        backend.write_transform(p, m, binary=binary)
        assert np.array_equal(backend.read_transform(p), m)


def test_plda_reads_hand_assembled_kaldi_bytes(tmp_path):
    """The documented binary layout: \\0B "<Plda> " DV-mean DM-transform DV-psi "</Plda> " (Kaldi Plda::Write)."""
    from xvector_amd import backend
    mean = [1.5, -2.0]
    tr = [[1.0, 2.0], [3.0, 4.0]]
    psi = [2.5, 0.5]
    blob = (b"\x00B<Plda> " + b"DV \x04" + struct.pack("<i", 2) + struct.pack("<2d", *mean) +
            b"DM \x04" + struct.pack("<i", 2) + b"\x04" + struct.pack("<i", 2) + struct.pack("<4d", 1.0, 2.0, 3.0, 4.0) +
            b"DV \x04" + struct.pack("<i", 2) + struct.pack("<2d", *psi) + b"</Plda> ")
    p = str(tmp_path / "plda")
    open(p, "wb").write(blob)
    got = backend.read_plda(p)
    assert got.mean.tolist() == mean and got.transform.tolist() == tr and got.psi.tolist() == psi
    backend.write_plda(str(tmp_path / "again"), got)
    assert open(str(tmp_path / "again"), "rb").read() == blob
    text = "<Plda>  [ 1.5 -2 ]\n [\n  1 2 \n  3 4 ]\n [ 2.5 0.5 ]\n</Plda> "
    open(p, "w").write(text)
    got = backend.read_plda(p)
    assert got.mean.tolist() == mean and got.transform.tolist() == tr and got.psi.tolist() == psi


def test_eer_agrees_with_roc():
    from sklearn.metrics import roc_curve
    from xvector_amd import backend
    rng = np.random.default_rng(6)
    for nt, nn, sep in ((100, 1000, 2.0), (537, 4000, 1.0), (2000, 2000, 3.0), (50, 20000, 0.5)):
        tgt = rng.standard_normal(nt) + sep
        non = rng.standard_normal(nn)
        e, _ = backend.eer(tgt, non)
        y = np.r_[np.ones(nt), np.zeros(nn)]
        fpr, tpr, _ = roc_curve(y, np.r_[tgt, non])
        fnr = 1 - tpr
        i = np.argmin(np.abs(fnr - fpr))
        assert abs(e - (fpr[i] + fnr[i]) / 2) <= 1.0 / min(nt, nn), (e, fpr[i], fnr[i])
    assert backend.eer([1.0, 2.0], [-1.0, 0.0])[0] == 0.0


def test_scoring_needs_a_gpu(tmp_path):
    import torch
    from xvector_amd import backend, hiplib
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    d = 4
    plda = backend.Plda(np.zeros(d), np.eye(d), np.ones(d))
    with pytest.raises(hiplib.XvectorHipError):
        backend.Scorer(np.ones((2, d), np.float32), np.ones((3, d), np.float32), plda)
    with pytest.raises(hiplib.XvectorHipError):
        backend.prepare(np.ones((2, d), np.float32), hiplib.SIDE_PLAIN)
    backend.write_plda(str(tmp_path / "plda"), plda)
    for f in ("enrol", "test", "trials", "scores"):
        open(str(tmp_path / f), "w").close()
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "x-vector-kaldi-tf_amd"), TWIN]))
    res = subprocess.run([sys.executable, os.path.join(TWIN, "plda_backend.py"), "score", str(tmp_path / "plda"),
                          "ark:" + str(tmp_path / "enrol"), "ark:" + str(tmp_path / "test"), str(tmp_path / "trials"),
                          str(tmp_path / "scores")], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode != 0 and "XvectorHipError" in res.stderr


def test_eer_cli(tmp_path):
    p = str(tmp_path / "in")
    open(p, "w").write("".join("%g %s\n" % (s, l) for s, l in ((3.0, "target"), (1.0, "target"), (2.0, "nontarget"),
                                                                 (0.0, "nontarget"))))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "x-vector-kaldi-tf_amd"), TWIN]))
    out = subprocess.run([sys.executable, os.path.join(TWIN, "plda_backend.py"), "compute-eer", p], env=env, capture_output=True,
                         text=True, timeout=300, check=True).stdout
    assert float(out.strip()) == 50.0
