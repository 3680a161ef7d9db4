"""PLDA domain adaptation end to end on the MI355X: `plda_backend.py adapt-plda --lda` against the float64
pipeline (the same chain in NumPy float64, then tests/adapt_ref.py), the moments kernel isolated from the chain, stage 10's
scores under the adapted model against float64 scores, and the CLI's refusals.

Data: a two-covariance model in D = 64 (the generator of test_gpu_backend.py), LDA to d = 20.  The out-of-domain model is fitted
on 100 speakers; the in-domain set is 3000 unlabelled vectors of a shifted model: another mean, and extra within-speaker variance
along 3 directions."""
import os
import subprocess
import sys

import numpy as np
import pytest

import adapt_ref
import backend_ref as ref
from conftest import ROOT, TWIN

pytestmark = pytest.mark.gpu

D, DIM = 64, 20
WS, BS = 0.75, 0.25                  # the recipe's scales
CLI = os.path.join(TWIN, "plda_backend.py")

# Fit: relative Frobenius distance of the CLI's adapted W, B and mean from the float64 pipeline's.  The difference is the fp32
# chain of xv_backend_prepare_f32 (mean subtraction, LDA on the exact-fp32 MFMA, length norm), which has no one-number bound
# here, so the bars are 4x what was measured on an MI355X (W 6.99e-8, B 6.70e-9, mean 1.96e-8 of the rows' length sqrt(d)):
# the factor 4 absorbs a box-to-box difference in the last bits of the fp32 chain.
FIT_BAR_W, FIT_BAR_B, FIT_BAR_MEAN = 2.8e-7, 2.7e-8, 7.9e-8


def _run(args, check=True):
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "x-vector-kaldi-tf_amd"), TWIN] + [env.get("PYTHONPATH", "")])
    return subprocess.run([sys.executable] + args, env=env, check=check, capture_output=True, text=True, timeout=600)


def _draw(rng, mu, B, W, n_spk, n_utt):
    spk = rng.multivariate_normal(np.zeros(D), B, n_spk) + mu
    x = spk[:, None, :] + rng.multivariate_normal(np.zeros(D), W, (n_spk, n_utt))
    return x.reshape(n_spk * n_utt, D).astype(np.float32), np.repeat(np.arange(n_spk), n_utt)


def _write_vectors(path, keys, x):
    import kaldi_io
    with kaldi_io.TableWriter(path + ".ark", path + ".scp") as w:
        kaldi_io.write_vec_flt_batch(w, list(keys), list(x))


def _chain64(x, transform):
    """Stage 8's chain in float64: subtract the set's own mean, transform-vec, ivector-normalize-length."""
    x = np.asarray(x, dtype=np.float64)
    return ref.chain(x, x.mean(axis=0), transform, True)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """Files of the out-of-domain model and of the in-domain data, the adapted model written by the CLI, and the float64
    pipeline's adapted covariances (computed once, shared, never modified)."""
    from xvector_amd import backend
    p = str(tmp_path_factory.mktemp("adapt"))
    rng = np.random.default_rng(5)
    B = np.diag(rng.uniform(0.5, 3.0, D))
    A = rng.standard_normal((D, D)) / np.sqrt(D)
    W = A @ A.T + 0.3 * np.eye(D)
    mu = rng.standard_normal(D)
    # out-of-domain training set and model (host, float64)
    xt, lt = _draw(rng, mu, B, W, 100, 6)
    t = backend.fit_lda(xt.astype(np.float64) - xt.astype(np.float64).mean(axis=0), list(lt), DIM).astype(np.float32)
    groups = [np.flatnonzero(lt == s) for s in range(100)]
    plda = backend.fit_plda(_chain64(xt, t), groups)
    backend.write_transform(p + "/transform.mat", t)
    backend.write_plda(p + "/plda", plda)
    # the in-domain model: shifted mean, more within-speaker variance along 3 directions
    q, _ = np.linalg.qr(rng.standard_normal((D, 3)))
    W_in = W + q @ np.diag([4.0, 3.0, 2.0]) @ q.T
    mu_in = mu + 0.8 * rng.standard_normal(D)
    xa, _ = _draw(rng, mu_in, B, W_in, 600, 5)                         # 3000 unlabelled vectors
    _write_vectors(p + "/major", ["major-%05d" % i for i in range(len(xa))], xa)
    res = _run([CLI, "adapt-plda", "--within-covar-scale", str(WS), "--between-covar-scale", str(BS), "--lda", p + "/transform.mat",
                p + "/plda", "scp:" + p + "/major.scp", p + "/plda_adapt"])
    # float64 pipeline on the same files
    plda_f = backend.read_plda(p + "/plda")
    t_f = backend.read_transform(p + "/transform.mat")
    y = _chain64(xa, t_f)
    W0, B0 = adapt_ref.covariances(plda_f.mean, plda_f.transform, plda_f.psi)
    m_ref, W_ref, B_ref = adapt_ref.adapt_from_moments(plda_f.mean, W0, B0, len(y), y.sum(axis=0), y.T @ y, WS, BS, 1.0)
    # evaluation set, in-domain: 80 speakers, 3 enrolment utterances and 3 tests each
    xe, le = _draw(rng, mu_in, B, W_in, 80, 6)
    return dict(p=p, log=res.stderr, plda=plda_f, t=t_f, xa=xa, ref=(m_ref, W_ref, B_ref), W0=W0, B0=B0, xe=xe, le=le,
                mean_in=xa.astype(np.float64).mean(axis=0).astype(np.float32))


def test_fit_matches_the_float64_pipeline(world):
    from xvector_amd import backend
    out = backend.read_plda(world["p"] + "/plda_adapt")
    Wg, Bg = adapt_ref.covariances(out.mean, out.transform, out.psi)
    m_ref, W_ref, B_ref = world["ref"]
    ew, eb = adapt_ref.rel_fro(Wg, W_ref), adapt_ref.rel_fro(Bg, B_ref)
    em = np.linalg.norm(out.mean - m_ref) / np.sqrt(DIM)        # against the rows' own length sqrt(d): the mean itself is near 0
    moved = adapt_ref.rel_fro(W_ref, world["W0"])
    print("adapt-plda vs float64 pipeline: rel Frobenius W %.3e, B %.3e, mean %.3e (the adaptation moved W by %.3e)" %
          (ew, eb, em, moved))
    assert "Read 3000 vectors of dimension %d" % DIM in world["log"] and "eigenvalues" in world["log"], world["log"]
    assert moved > 0.1                                                # the data does call for an adaptation
    assert ew <= FIT_BAR_W and eb <= FIT_BAR_B and em <= FIT_BAR_MEAN
    assert np.all(np.diff(out.psi) <= 0) and np.all(out.psi >= 0)


def test_moments_isolated_from_the_chain(world):
    """adapt_plda on the kernel's moments of the device-prepared rows against adapt_plda on NumPy-float64 moments of the same
    rows downloaded: the fp32 chain is common to both, what differs is the summation alone."""
    from xvector_amd import backend, hiplib
    xa = world["xa"]
    rows, _ = backend.prepare(xa, hiplib.SIDE_PLAIN, mean=world["mean_in"], transform=world["t"], length_norm=True)
    n, s1, s2 = backend.moment_stats(rows, DIM)
    y = rows[:, :DIM].cpu().numpy().astype(np.float64)
    a = backend.adapt_plda(world["plda"], n, s1, s2, WS, BS)
    b = backend.adapt_plda(world["plda"], len(y), y.sum(axis=0), y.T @ y, WS, BS)
    (Wa, Ba), (Wb, Bb) = (adapt_ref.covariances(o.mean, o.transform, o.psi) for o in (a, b))
    ew, eb = adapt_ref.rel_fro(Wa, Wb), adapt_ref.rel_fro(Ba, Bb)
    print("kernel moments vs NumPy moments of the same rows: rel Frobenius W %.3e, B %.3e" % (ew, eb))
    assert n == len(xa) and ew <= 1e-9 and eb <= 1e-9


def test_stage10_scores_under_the_adapted_model(world):
    from xvector_amd import backend
    p, xe, le = world["p"], world["xe"], world["le"]
    utt = np.tile(np.arange(6), 80)
    spk_keys = ["spk%03d" % s for s in range(80)]
    enrol = np.stack([xe[(le == s) & (utt < 3)].astype(np.float64).mean(axis=0) for s in range(80)]).astype(np.float32)
    tsel = np.flatnonzero(utt >= 3)
    test_keys = ["spk%03d-u%d" % (le[i], utt[i]) for i in tsel]
    xtest = xe[tsel]
    _write_vectors(p + "/spk", spk_keys, enrol)
    _write_vectors(p + "/test", test_keys, xtest)
    with open(p + "/num_utts.ark", "w") as f:
        f.writelines("%s 3\n" % s for s in spk_keys)
    import kaldi_io
    kaldi_io.write_vec_flt(p + "/mean.vec", world["mean_in"])
    trials = [(s, u) for s in spk_keys for u in test_keys]
    with open(p + "/trials", "w") as f:
        f.writelines("%s %s\n" % tr for tr in trials)
    _run([CLI, "score", "--num-utts=ark:" + p + "/num_utts.ark", "--mean", p + "/mean.vec", "--lda", p + "/transform.mat",
          p + "/plda_adapt", "scp:" + p + "/spk.scp", "scp:" + p + "/test.scp", p + "/trials", p + "/scores_adapt"])
    lines = open(p + "/scores_adapt").read().splitlines()
    assert len(lines) == len(trials) and all(tuple(l.split()[:2]) == tr for l, tr in zip(lines, trials))
    got = np.array([float(l.split()[2]) for l in lines]).reshape(80, len(test_keys))
    # float64 scores under the float64-adapted model
    m_ref, W_ref, B_ref = world["ref"]
    P_ref, psi_ref = adapt_ref.diagonalise(B_ref, W_ref)            # the reference's own diagonalisation (symmetric whitening)
    pl = (m_ref, P_ref, psi_ref)
    mean = world["mean_in"].astype(np.float64)
    nu = np.full(80, 3)
    z = ref.chain(enrol, mean, world["t"], True, pl, nu)
    tz = ref.chain(xtest, mean, world["t"], True, pl, None)
    e_rows, r = ref.side_rows_enrol(z, nu, psi_ref)
    want = e_rows @ ref.side_rows_test(tz).T + r[:, None]
    worst = np.abs(got - want).max()
    target = np.array([[u.startswith(s) for u in test_keys] for s in spk_keys])
    eer_adapt, _ = backend.eer(got[target], got[~target])
    # the unadapted model on the same trials (in process)
    sc = backend.Scorer(enrol, xtest, world["plda"], nu.astype(np.int32), world["mean_in"], world["t"])
    plain = sc.score_matrix().cpu().numpy()
    eer_plain, _ = backend.eer(plain[target], plain[~target])
    print("stage 10: max |score - float64| = %.3e over %d trials; EER adapted %.3f %%, unadapted %.3f %%" %
          (worst, got.size, 100 * eer_adapt, 100 * eer_plain))
    assert worst <= 1e-3
    assert np.isfinite(eer_adapt) and np.isfinite(eer_plain)


def test_cli_refusals(world, tmp_path):
    from xvector_amd import backend
    p, q = world["p"], str(tmp_path)
    other = backend.plda_from_covariances(np.zeros(DIM + 1), np.eye(DIM + 1) * 2.0, np.eye(DIM + 1))
    backend.write_plda(q + "/plda21", other)
    open(q + "/empty.ark", "wb").close()
    base = [CLI, "adapt-plda", "--lda", p + "/transform.mat"]
    for args, word in ((base + [q + "/plda21", "scp:" + p + "/major.scp", q + "/out1"], "dimension"),
                       (base + [p + "/plda", "ark:" + q + "/empty.ark", q + "/out2"], "no vectors"),
                       (base + ["--within-covar-scale", "-0.5", p + "/plda", "scp:" + p + "/major.scp", q + "/out3"], "within-covar-scale")):
        res = _run(args, check=False)
        assert res.returncode != 0 and word in res.stderr, (res.returncode, res.stderr)
    assert not any(os.path.exists(q + "/out%d" % i) for i in (1, 2, 3))
