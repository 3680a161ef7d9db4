"""An independent restatement of the VBx rule of include/xvector_hip.h in the GENERIC log-domain form: the full S x S transition
matrix in logarithms, a logsumexp forward-backward, pi from the log forward / backward variables.  On purpose a different
formulation from the product's linear one (backend.vbx_host, csrc/xv_vbx.hip).  ``dtype`` may be numpy.longdouble: the distance
between the float64 and the longdouble run is the yardstick of tests/test_gpu_vbx.py.  Also the synthetic cases the tests share."""
import functools

import numpy as np


def _lse(x, axis):
    m = np.max(x, axis=axis, keepdims=True)
    m = np.where(np.isfinite(m), m, 0)
    return np.squeeze(m, axis=axis) + np.log(np.sum(np.exp(x - m), axis=axis))


def vbx_ref(y, labels, n_spk, mean, transform, psi, fa=0.3, fb=17.0, loop_prob=0.99, init_smoothing=5.0, max_iters=40,
            epsilon=1e-6, dtype=np.float64):
    """y[T, D] in time order, labels[T] in [0, n_spk).  -> dict(gamma [T, S], pi [S], elbo [iters], iters, labels, margin): margin
    is the smallest gap between the largest and the second largest gamma of a row (1 for S = 1)."""
    f = dtype
    y = np.asarray(y).astype(f)
    mu, P, phi = (np.asarray(a).astype(f) for a in (mean, transform, psi))
    fa, fb, lp, smooth = f(fa), f(fb), f(loop_prob), f(init_smoothing)
    T, D = y.shape
    S = int(n_spk)
    half, one = f(0.5), f(1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        z = (y - mu) @ P.T
        rho = z * np.sqrt(phi)
        G = -half * ((z * z).sum(axis=1) + f(D) * np.log(f(2) * f(np.pi)))
        es = np.exp(smooth)
        gamma = np.full((T, S), one / (es + f(S - 1)), dtype=f)
        gamma[np.arange(T), np.asarray(labels)] = es / (es + f(S - 1))
        pi = np.full(S, one / f(S), dtype=f)
        elbo = []
        for it in range(int(max_iters)):
            N = gamma.sum(axis=0)
            invL = one / (one + fa / fb * N[:, None] * phi[None, :])
            alpha = fa / fb * invL * (gamma.T @ rho)
            lls = fa * (rho @ alpha.T - half * ((invL + alpha ** 2) @ phi)[None, :] + G[:, None])
            ltr = np.log(np.eye(S, dtype=f) * lp + (one - lp) * np.ones((S, 1), dtype=f) * pi[None, :])
            lf = np.empty((T, S), dtype=f)
            lb = np.zeros((T, S), dtype=f)
            lf[0] = np.log(pi) + lls[0]
            for t in range(1, T):
                lf[t] = lls[t] + _lse(lf[t - 1][:, None] + ltr, axis=0)
            for t in range(T - 2, -1, -1):
                lb[t] = _lse(ltr + (lls[t + 1] + lb[t + 1])[None, :], axis=1)
            tll = _lse(lf[T - 1], axis=0)
            gamma = np.exp(lf + lb - tll)
            e = tll + half * fb * (np.log(invL) - invL - alpha ** 2 + one).sum()
            pn = gamma[0] + (one - lp) * pi * np.exp(_lse(lf[:-1], axis=1)[:, None] + lb[1:] + lls[1:] - tll).sum(axis=0)
            pi = pn / pn.sum()
            elbo.append(e)
            if it > 0 and elbo[-1] - elbo[-2] < epsilon:
                break
    top = np.sort(gamma, axis=1)
    margin = float((top[:, -1] - top[:, -2]).min()) if S > 1 else 1.0
    return dict(gamma=gamma, pi=pi, elbo=np.asarray(elbo, dtype=f), iters=len(elbo), labels=np.argmax(gamma, axis=1).astype(np.int32),
                margin=margin)


def ref_distance(a64, ald):
    """(d_gamma, d_pi, d_elbo relative): the largest |difference| between the float64 and the longdouble run."""
    n = min(len(a64["elbo"]), len(ald["elbo"]))
    de = np.max(np.abs(a64["elbo"][:n].astype(np.longdouble) - ald["elbo"][:n]) / np.abs(ald["elbo"][:n]))
    return (float(np.max(np.abs(a64["gamma"] - ald["gamma"]))), float(np.max(np.abs(a64["pi"] - ald["pi"]))), float(de))


def model(D, seed=0, lo=8.0, hi=80.0):
    """A PLDA in Kaldi's diagonalised form: (mean [D], transform [D, D], psi [D] descending in [lo, hi]), float64."""
    rng = np.random.default_rng(1000 + seed)
    q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    transform = (q * np.exp(rng.uniform(-0.3, 0.3, D))[None, :]) @ np.linalg.qr(rng.standard_normal((D, D)))[0]
    psi = np.sort(np.exp(rng.uniform(np.log(lo), np.log(hi), D)))[::-1].copy()
    return 0.1 * rng.standard_normal(D), transform, psi


def turns_case(D, T, n_true, S, seed=0, turn=5, split=True, wrong=3, mdl=None):
    """One recording: T rows in turns of ``turn`` rows, n_true speakers taking turns in a fixed cycle; in the model's
    diagonalised space a speaker is N(0, psi) and a row its speaker + N(0, I).  The initial labels use S slots: the true speakers
    first; with ``split`` the last true speaker's later turns go to slot n_true (an over-split cluster); slots beyond are given to
    single rows; ``wrong`` rows carry another true speaker's label.  -> (y float32 [T, D], labels int32 [T], truth int32 [T])."""
    rng = np.random.default_rng(seed)
    mean, transform, psi = mdl if mdl is not None else model(D, seed)
    spk = rng.standard_normal((n_true, D)) * np.sqrt(psi)
    nturns = (T + turn - 1) // turn
    who = np.repeat(np.arange(nturns) % n_true, turn)[:T]
    z = spk[who] + rng.standard_normal((T, D))
    y = np.ascontiguousarray((np.linalg.solve(transform, z.T).T + mean).astype(np.float32))
    lab = who.copy()
    used = n_true
    if split and S > n_true and n_true >= 1:
        mine = np.flatnonzero(who == n_true - 1)
        lab[mine[mine.size // 2:]] = n_true
        used += 1
    free = rng.permutation(T)
    at = 0
    for s in range(used, S):                                    # the slots left over: one row each
        lab[free[at]] = s
        at += 1
    if n_true > 1:
        for i in free[at:at + wrong]:
            lab[i] = (who[i] + 1) % n_true
    return y, lab.astype(np.int32), who.astype(np.int32)


# (D, T, true speakers, S, seed): the recordings the CPU and GPU tests share.  The first is the split-cluster case: 60 rows in 12
# turns of 5, three true speakers, one split over two initial labels, three rows mislabelled.  The others cover D in {3, 10, 16, 128}
# (no multiple of the MFMA's 4; the maximum), S in {1, 2, 17, 64} (past one 16-wide tile; the cap) and T in {1, 2, 3, 17, 65, 130}
# (past a 16-row and a 64-row tile).
SPLIT_CASE = (16, 60, 3, 4, 0)
CASES = [SPLIT_CASE, (3, 17, 2, 2, 0), (10, 65, 4, 17, 0), (128, 130, 4, 64, 0), (128, 1, 1, 1, 0), (16, 2, 2, 2, 0), (10, 3, 1, 1, 0),
         (3, 130, 2, 3, 0), (16, 17, 2, 17, 0), (128, 65, 3, 4, 0)]


def make(case):
    """-> (y, labels, S, (mean, transform, psi))"""
    D, T, n_true, S, seed = case
    mdl = model(D, seed)
    y, lab, _ = turns_case(D, T, n_true, S, seed, mdl=mdl)
    return y, lab, S, mdl


def bound(d):
    """What a float64 evaluation in another formulation may differ from vbx_ref in float64 by, given d = the distance of vbx_ref
    in float64 from vbx_ref in longdouble on the same input: 64 d + 1e-13 (64x for sums over up to T D terms taken in another
    order and for another exp)."""
    return 64.0 * d + 1e-13


@functools.lru_cache(maxsize=None)
def reference(case, max_iters, epsilon):
    """(the float64 run, (d_gamma, d_pi, d_elbo)) of a case, computed once and shared: callers do not change it."""
    y, lab, S, mdl = make(case)
    r64 = vbx_ref(y, lab, S, *mdl, max_iters=max_iters, epsilon=epsilon)
    rld = vbx_ref(y, lab, S, *mdl, max_iters=max_iters, epsilon=epsilon, dtype=np.longdouble)
    return r64, ref_distance(r64, rld)
