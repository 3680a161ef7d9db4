"""Test-side float64 reference of unsupervised PLDA adaptation, written from the definition and independent of
xvector_amd/backend.py: whiten with the symmetric inverse square root of the model's total covariance T = W + B, keep the part
of the whitened in-domain covariance that exceeds the identity, map it back and share it out between W and B."""
import numpy as np


def _sym_pow(m, p):
    s, u = np.linalg.eigh((m + m.T) / 2)
    return (u * s ** p) @ u.T


def covariances(mean, transform, psi):
    """(W, B) of a diagonalised PLDA: W = P^-1 P^-T, B = P^-1 diag(psi) P^-T."""
    inv = np.linalg.inv(np.asarray(transform, dtype=np.float64))
    return inv @ inv.T, (inv * np.asarray(psi, dtype=np.float64)) @ inv.T


def diagonalise(B, W):
    """(P, psi) with P W P^T = I and P B P^T = diag(psi), psi descending, by symmetric whitening: S = W^-1/2, the
    eigenvectors V of S B S, P = V^T S.  Any such P gives the same log-likelihood ratios."""
    s = _sym_pow(W, -0.5)
    m = s @ B @ s
    psi, v = np.linalg.eigh((m + m.T) / 2)
    o = np.argsort(psi)[::-1]
    return v[:, o].T @ s, np.maximum(psi[o], 0.0)


def excess(W, B, V):
    """E = T^1/2 [T^-1/2 V T^-1/2 - I]_+ T^1/2 with T = W + B and [.]_+ the positive part of a symmetric matrix."""
    T = W + B
    th, tmh = _sym_pow(T, 0.5), _sym_pow(T, -0.5)
    d = tmh @ V @ tmh - np.eye(len(T))
    s, u = np.linalg.eigh((d + d.T) / 2)
    pos = (u * np.maximum(s, 0.0)) @ u.T
    return th @ pos @ th


def adapt(mu, W, B, m, V, within_scale, between_scale, mean_diff_scale=1.0):
    """-> (new mean, W_new, B_new): V (the in-domain covariance about its own mean m) is first widened by
    mean_diff_scale (m - mu)(m - mu)^T."""
    diff = np.asarray(m, dtype=np.float64) - np.asarray(mu, dtype=np.float64)
    E = excess(W, B, np.asarray(V, dtype=np.float64) + mean_diff_scale * np.outer(diff, diff))
    return np.array(m, dtype=np.float64), W + within_scale * E, B + between_scale * E


def adapt_from_moments(mu, W, B, n, s1, s2, within_scale, between_scale, mean_diff_scale=1.0):
    m = np.asarray(s1, dtype=np.float64) / n
    return adapt(mu, W, B, m, np.asarray(s2, dtype=np.float64) / n - np.outer(m, m), within_scale, between_scale, mean_diff_scale)


def rel_fro(got, want):
    return np.linalg.norm(got - want) / np.linalg.norm(want)
