"""Test-side float64 reference of the per-recording PCA and the projected PLDA, written from the rule in
include/xvector_hip.h with numpy.linalg.eigh and cholesky, independent of xvector_amd/backend.py; and a NumPy emulation of the
kernel's own Jacobi rotation order (round-robin, disjoint rotations applied together), from which the tests take the constant
of their error bounds."""
import numpy as np

import backend_ref as ref

TOL = 2.0 ** -58
MAX_SWEEPS = 30


def covariance(y):
    y = np.asarray(y, dtype=np.float64)
    n = y.shape[0]
    m = y.sum(axis=0) / n
    return y.T @ y / n - np.outer(m, m)


def sorted_eig(c):
    """(eigenvalues descending, eigenvectors as rows, each with its first component of largest magnitude positive)."""
    s, u = np.linalg.eigh((c + c.T) / 2)
    o = np.argsort(-s, kind="stable")
    rows = u[:, o].T.copy()
    for v in rows:
        if v[np.argmax(np.abs(v))] < 0:
            v *= -1.0
    return s[o], rows


def energy_rule(s, target):
    """p = min(k + 1, d), k the smallest count whose cumulative share exceeds target (d if none); None if the total is not > 0.
    Also the distance of the share at the decision point from the target."""
    s = np.asarray(s, dtype=np.float64)
    total = s.sum()
    if not (np.isfinite(total) and total > 0):
        return None, None
    share = np.cumsum(s) / total
    above = np.flatnonzero(share > target)
    k = int(above[0]) + 1 if above.size else s.size
    margin = min(abs(share[k - 1] - target), abs(share[k - 2] - target) if k >= 2 else np.inf)
    return min(k + 1, s.size), margin


def est_pca(y, target):
    """dict(A [p, d], eigvals [d], p, margin, gap = l_p / l_{p+1} (inf at p = d)) or None for the fallback."""
    c = covariance(y)
    if not np.all(np.isfinite(c)):
        return None
    s, rows = sorted_eig(c)
    p, margin = energy_rule(s, target)
    if p is None:
        return None
    gap = np.inf if p == s.size or s[p] <= 0 else s[p - 1] / s[p]
    return dict(A=rows[:p], eigvals=s, p=p, margin=margin, gap=gap, C=c)


def model_covariances(transform, psi):
    inv = np.linalg.inv(np.asarray(transform, dtype=np.float64))
    return inv @ inv.T, (inv * np.asarray(psi, dtype=np.float64)) @ inv.T


def project(mean, transform, psi, A):
    """Plda::ApplyTransform: -> dict(mean mu_g, transform P_g, psi psi_g, W W_g, B B_g)."""
    W, B = model_covariances(transform, psi)
    Wg, Bg = A @ W @ A.T, A @ B @ A.T
    t1 = np.linalg.inv(np.linalg.cholesky((Wg + Wg.T) / 2))
    m = t1 @ Bg @ t1.T
    s, v = np.linalg.eigh((m + m.T) / 2)
    o = np.argsort(-s, kind="stable")
    return dict(mean=A @ np.asarray(mean, dtype=np.float64), transform=v[:, o].T @ t1, psi=np.maximum(s[o], 0.0), W=Wg, B=Bg)


def transform_rows(y, M, c, psi):
    """z = M y + c, scaled by sqrt(p / sum z^2 / (psi + 1)) (TransformIvector, one utterance), float64.  M [p, d], c, psi [p]."""
    z = np.asarray(y, dtype=np.float64) @ np.asarray(M, dtype=np.float64).T + c
    p = z.shape[1]
    dot = (z * z / (np.asarray(psi, dtype=np.float64)[None, :] + 1.0)).sum(axis=1)
    return z * np.sqrt(p / dot)[:, None]


def operand_rows(y, M, c, psi):
    """(enrolment rows [n, 2p], r [n], test rows [n, 2p]) of the rows y under z = M y + c."""
    z = transform_rows(y, M, c, psi)
    e, r = ref.side_rows_enrol(z, np.ones(len(z)), psi)
    return e, r, ref.side_rows_test(z)


def llr_matrix(y, mean, transform, psi, target):
    """The recording's float64 score matrix under its own PCA (or the global model on the fallback), and p."""
    y = np.asarray(y, dtype=np.float64)
    est = est_pca(y, target)
    if est is None:
        P, m, ps = (np.asarray(a, dtype=np.float64) for a in (transform, mean, psi))
        M, c = P, -(P @ m)
    else:
        g = project(mean, transform, psi, est["A"])
        M, c, ps = g["transform"] @ est["A"], -(g["transform"] @ g["mean"]), g["psi"]
    e, r, t = operand_rows(y, M, c, ps)
    return e @ t.T + r[:, None], len(ps)


# ------------------------------------------------------------------------------------------------
# the kernel's rotation order, emulated
# ------------------------------------------------------------------------------------------------
def round_robin_pairs(m, r):
    """The m / 2 pairs (p < q) of step r of the circle method over m players (m even), player m - 1 fixed."""
    k = np.arange(1, m // 2)
    a = np.concatenate([[m - 1], (r + k) % (m - 1)])
    b = np.concatenate([[r], (r + m - 1 - k) % (m - 1)])
    return np.minimum(a, b), np.maximum(a, b)


def jacobi_round_robin(c, tol=TOL, max_sweeps=MAX_SWEEPS):
    """Cyclic Jacobi in the kernel's order: -> (eigenvalues in iteration order, eigenvectors as rows, sweeps, converged)."""
    a = np.array(c, dtype=np.float64)
    n = a.shape[0]
    m = (n + 1) & ~1
    vt = np.eye(n)
    for sweep in range(max_sweeps + 1):
        off = np.abs(a - np.diag(np.diag(a))).max() if n > 1 else 0.0
        if off <= tol * np.abs(np.diag(a)).max():
            return np.diag(a).copy(), vt, sweep, True
        if sweep == max_sweeps or not np.isfinite(off):
            break
        for r in range(m - 1):
            p, q = round_robin_pairs(m, r)
            keep = q < n
            p, q = p[keep], q[keep]
            apq = a[p, q]
            rot = apq != 0
            p, q, apq = p[rot], q[rot], apq[rot]
            if p.size == 0:
                continue
            theta = (a[q, q] - a[p, p]) / (2.0 * apq)
            t = np.where(theta >= 0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
            cs = 1.0 / np.sqrt(t * t + 1.0)
            sn = t * cs
            app, aqq = a[p, p] - t * apq, a[q, q] + t * apq
            rp, rq = a[p, :].copy(), a[q, :].copy()
            a[p, :], a[q, :] = cs[:, None] * rp - sn[:, None] * rq, sn[:, None] * rp + cs[:, None] * rq
            cp, cq = a[:, p].copy(), a[:, q].copy()
            a[:, p], a[:, q] = cs[None, :] * cp - sn[None, :] * cq, sn[None, :] * cp + cs[None, :] * cq
            a[p, p], a[q, q] = app, aqq
            a[p, q] = a[q, p] = 0.0
            a = np.triu(a) + np.triu(a, 1).T
            vp, vq = vt[p, :].copy(), vt[q, :].copy()
            vt[p, :], vt[q, :] = cs[:, None] * vp - sn[:, None] * vq, sn[:, None] * vp + cs[:, None] * vq
    return np.diag(a).copy(), vt, max_sweeps, False


def emulation_ratios(c):
    """The emulation's errors on c in units of d 2^-52 ||c||_2: (eigenvalues against eigvalsh, |V V^T - I|, |V C V^T - diag|)."""
    c = np.asarray(c, dtype=np.float64)
    d = c.shape[0]
    s, vt, sweeps, ok = jacobi_round_robin(c)
    assert ok
    unit = d * 2.0 ** -52 * np.linalg.norm(c, 2)
    o = np.argsort(-s, kind="stable")
    want = np.linalg.eigvalsh(c)[::-1]
    return (np.abs(s[o] - want).max() / unit, np.abs(vt @ vt.T - np.eye(d)).max() * np.linalg.norm(c, 2) / unit,
            np.abs(vt @ c @ vt.T - np.diag(s)).max() / unit, sweeps)
