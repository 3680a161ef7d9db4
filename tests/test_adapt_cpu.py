"""backend.adapt_plda (ivector-adapt-plda) on the host, against properties that follow from the definition and
against tests/adapt_ref.py, an independent float64 restatement.  Covariances are compared, never eigenvectors."""
import numpy as np
import pytest

import adapt_ref as ref

DIMS = [1, 3, 20]
WS, BS = 0.75, 0.25                  # the recipe's scales (run.sh, end of stage 8)


def _spd(rng, d, floor=0.5):
    a = rng.standard_normal((d, d + 2))
    return a @ a.T / (d + 2) + floor * np.eye(d)


def _model(d, seed=0):
    from xvector_amd import backend
    rng = np.random.default_rng(100 * d + seed)
    W, B, mu = _spd(rng, d), _spd(rng, d, 0.2) * 1.7, rng.standard_normal(d)
    plda = backend.plda_from_covariances(mu, B, W)
    W1, B1 = _cov(plda)                                    # the helper that recovers covariances is sound on the input model
    assert ref.rel_fro(W1, W) <= 1e-10 and ref.rel_fro(B1, B) <= 1e-10
    return rng, plda, mu, W, B


def _moments(m, V, n=1000):
    return n, n * m, n * (V + np.outer(m, m))


def _cov(plda):
    return ref.covariances(plda.mean, plda.transform, plda.psi)


def _psd_rank(rng, d, rank, scale):
    g = rng.standard_normal((d, min(rank, d)))
    return scale * g @ g.T


def _adapt(plda, m, V, **kw):
    from xvector_amd import backend
    return backend.adapt_plda(plda, *_moments(m, V), **kw)


@pytest.mark.parametrize("d", DIMS)
def test_identity(d):
    _, plda, mu, W, B = _model(d)
    out = _adapt(plda, mu, W + B, within_covar_scale=WS, between_covar_scale=BS)
    W1, B1 = _cov(out)
    assert ref.rel_fro(W1, W) <= 1e-10 and ref.rel_fro(B1, B) <= 1e-10
    assert np.linalg.norm(out.psi - plda.psi) <= 1e-10 * np.linalg.norm(plda.psi)
    assert np.linalg.norm(out.mean - mu) <= 1e-12 * max(np.linalg.norm(mu), 1.0)


@pytest.mark.parametrize("d", DIMS)
def test_known_excess(d):
    rng, plda, mu, W, B = _model(d)
    D = _psd_rank(rng, d, 2, 0.8)
    out = _adapt(plda, mu, W + B + D, within_covar_scale=WS, between_covar_scale=BS)
    W1, B1 = _cov(out)
    assert ref.rel_fro(W1, W + WS * D) <= 1e-9 and ref.rel_fro(B1, B + BS * D) <= 1e-9
    # the output is a diagonalised model of exactly those covariances
    P = out.transform
    Wn, Bn = W + WS * D, B + BS * D
    assert np.abs(P @ Wn @ P.T - np.eye(d)).max() <= 1e-9
    assert np.abs(P @ Bn @ P.T - np.diag(out.psi)).max() <= 1e-9 * max(out.psi.max(), 1.0)
    assert np.all(np.diff(out.psi) <= 0) and np.all(out.psi >= 0)


@pytest.mark.parametrize("d", DIMS)
def test_shrinkage_is_left_alone(d):
    rng, plda, mu, W, B = _model(d)
    T = W + B
    s, u = np.linalg.eigh(T)
    k = min(2, d)
    Dm = (u[:, :k] * (0.5 * s[:k])) @ u[:, :k].T           # halves the k smallest eigenvalues of T: T - Dm stays SPD
    assert np.linalg.eigvalsh(T - Dm).min() > 0
    out = _adapt(plda, mu, T - Dm, within_covar_scale=WS, between_covar_scale=BS)
    W1, B1 = _cov(out)
    assert ref.rel_fro(W1, W) <= 1e-10 and ref.rel_fro(B1, B) <= 1e-10


@pytest.mark.parametrize("d", DIMS)
def test_mean(d):
    rng, plda, mu, W, B = _model(d)
    m = mu + rng.standard_normal(d) * 1.5
    V = W + B + _psd_rank(rng, d, 2, 0.3)
    shift = np.outer(m - mu, m - mu)
    a = _adapt(plda, m, V, within_covar_scale=WS, between_covar_scale=BS, mean_diff_scale=1.0)
    b = _adapt(plda, m, V + shift, within_covar_scale=WS, between_covar_scale=BS, mean_diff_scale=0.0)
    c = _adapt(plda, m, V, within_covar_scale=WS, between_covar_scale=BS, mean_diff_scale=0.0)
    e = _adapt(plda, mu, V, within_covar_scale=WS, between_covar_scale=BS, mean_diff_scale=0.0)
    for out in (a, b, c):
        assert np.linalg.norm(out.mean - m) <= 1e-12 * np.linalg.norm(m)
    (Wa, Ba), (Wb, Bb), (Wc, Bc), (We, Be) = _cov(a), _cov(b), _cov(c), _cov(e)
    assert ref.rel_fro(Wa, Wb) <= 1e-10 and ref.rel_fro(Ba, Bb) <= 1e-10          # scale 1 == the shift folded into V
    assert ref.rel_fro(Wc, We) <= 1e-10 and ref.rel_fro(Bc, Be) <= 1e-10          # scale 0: the shift has no effect
    assert ref.rel_fro(Wa, Wc) > 1e-3                                              # ... and with scale 1 it has one


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_agrees_with_reference(d, seed):
    rng, plda, mu, W, B = _model(d, seed)
    m = mu + rng.standard_normal(d) * 0.7
    V = _spd(rng, d, 0.05) * rng.uniform(0.5, 3.0)         # some directions above the model's total covariance, some below
    n, s1, s2 = _moments(m, V, n=3000)
    for ws, bs, ms in ((WS, BS, 1.0), (0.3, 0.7, 1.0), (1.3, 0.0, 0.5)):
        from xvector_amd import backend
        out = backend.adapt_plda(plda, n, s1, s2, ws, bs, ms)
        mr, Wr, Br = ref.adapt_from_moments(mu, W, B, n, s1, s2, ws, bs, ms)
        W1, B1 = _cov(out)
        assert ref.rel_fro(W1, Wr) <= 1e-9 and ref.rel_fro(B1, Br) <= 1e-9
        assert np.linalg.norm(out.mean - mr) <= 1e-12 * max(np.linalg.norm(mr), 1.0)


@pytest.mark.parametrize("d", DIMS)
def test_zero_scales_change_only_the_mean(d):
    rng, plda, mu, W, B = _model(d)
    m = mu + rng.standard_normal(d)
    out = _adapt(plda, m, 3.0 * (W + B), within_covar_scale=0.0, between_covar_scale=0.0)
    W1, B1 = _cov(out)
    assert ref.rel_fro(W1, W) <= 1e-10 and ref.rel_fro(B1, B) <= 1e-10
    assert np.linalg.norm(out.mean - m) <= 1e-12 * np.linalg.norm(m)


def test_default_scales():
    import inspect
    from xvector_amd import backend
    p = inspect.signature(backend.adapt_plda).parameters
    assert [p[k].default for k in ("within_covar_scale", "between_covar_scale", "mean_diff_scale")] == [0.3, 0.7, 1.0]


def test_refusals():
    from xvector_amd import backend
    rng, plda, mu, W, B = _model(3)
    n, s1, s2 = _moments(mu, W + B)
    backend.adapt_plda(plda, n, s1, s2)
    bad = [
        dict(n=0), dict(n=-5), dict(n=float("nan")),
        dict(s1=s1[:2]), dict(s2=s2[:2]), dict(s2=s2[:, :2]), dict(s1=np.zeros(4), s2=np.zeros((4, 4))),
        dict(s1=np.array([1.0, np.nan, 0.0])), dict(s2=s2 * np.inf),
        dict(within_covar_scale=-0.1), dict(between_covar_scale=-1.0), dict(mean_diff_scale=-1e-9),
        dict(within_covar_scale=float("nan")), dict(between_covar_scale=float("inf")),
    ]
    for kw in bad:
        args = dict(n=n, s1=s1, s2=s2)
        args.update({k: kw.pop(k) for k in list(kw) if k in args})
        with pytest.raises(ValueError):
            backend.adapt_plda(plda, args["n"], args["s1"], args["s2"], **kw)


@pytest.mark.parametrize("binary", [True, False])
def test_output_round_trips(tmp_path, binary):
    from xvector_amd import backend
    rng, plda, mu, W, B = _model(20)
    out = _adapt(plda, mu + 0.3, W + B + _psd_rank(rng, 20, 3, 0.5), within_covar_scale=WS, between_covar_scale=BS)
    path = str(tmp_path / "plda_adapt")
    backend.write_plda(path, out, binary=binary)
    back = backend.read_plda(path)
    for a, b in ((back.mean, out.mean), (back.transform, out.transform), (back.psi, out.psi)):
        assert np.array_equal(a, b)
