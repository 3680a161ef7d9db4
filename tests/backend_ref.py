"""Test-side float64 reference of the scoring back-end, written from the formulas, independent of
xvector_amd/backend.py: the stage-9 preprocessing chain, Kaldi's PLDA TransformIvector and the closed-form LLR."""
import numpy as np


def chain(x, mean=None, transform=None, length_norm=True, plda=None, num_utts=None):
    """x[N, D] -> z[N, d] in float64: subtract mean, affine LDA (transform [d, D] or [d, D + 1]), scale to norm sqrt(d), then
    z = P (y - m) scaled by sqrt(d / sum z^2 / (psi + 1/n)).  plda = (m, P, psi) or None."""
    x = np.asarray(x, dtype=np.float64)
    if mean is not None:
        x = x - np.asarray(mean, dtype=np.float64)
    if transform is not None:
        t = np.asarray(transform, dtype=np.float64)
        D = x.shape[1]
        x = x @ t[:, :D].T + (t[:, D] if t.shape[1] == D + 1 else 0.0)
    d = x.shape[1]
    if length_norm:
        nrm = np.linalg.norm(x, axis=1, keepdims=True)
        x = x * np.where(nrm > 0, np.sqrt(d) / np.where(nrm > 0, nrm, 1.0), 1.0)
    if plda is not None:
        m, P, psi = (np.asarray(a, dtype=np.float64) for a in plda)
        z = (x - m) @ P.T
        n = np.ones(len(z)) if num_utts is None else np.asarray(num_utts, dtype=np.float64)
        dot = (z * z / (psi[None, :] + 1.0 / n[:, None])).sum(axis=1)
        x = z * np.sqrt(d / dot)[:, None]
    return x


def _avw(psi, n):
    psi = np.asarray(psi, dtype=np.float64)
    a = n * psi / (n * psi + 1.0)
    v = 1.0 + psi / (n * psi + 1.0)
    w = 1.0 + psi
    return a, v, w


def llr(z, n, t, psi):
    """Kaldi Plda::LogLikelihoodRatio of the enrolment mean z (n utterances) against the test vector t, in closed form."""
    a, v, w = _avw(psi, n)
    return (np.sum(a / v * z * t) - 0.5 * np.sum(t * t * (1.0 / v - 1.0 / w)) - 0.5 * np.sum(a * a * z * z / v)
            + 0.5 * np.sum(np.log(w) - np.log(v)))


def side_rows_enrol(z, n, psi):
    """Packed enrolment rows [N, 2d] and constants r[N] of z[N, d] with counts n[N]."""
    z = np.asarray(z, dtype=np.float64)
    n = np.asarray(n, dtype=np.float64)[:, None]
    a, v, w = _avw(np.asarray(psi, dtype=np.float64)[None, :], n)
    rows = np.hstack([a / v * z, 1.0 / v - 1.0 / w])
    r = -0.5 * np.sum(a * a * z * z / v, axis=1) + 0.5 * np.sum(np.log(w) - np.log(v), axis=1)
    return rows, r


def side_rows_test(t):
    t = np.asarray(t, dtype=np.float64)
    return np.hstack([t, -0.5 * t * t])


def side_rows_cosine(z):
    z = np.asarray(z, dtype=np.float64)
    return z / np.linalg.norm(z, axis=1, keepdims=True)
