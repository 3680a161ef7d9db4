"""Test-side NumPy restatement of xv_ahc_average_f64 (include/xvector_hip.h), independent of the kernel's
caching scheme: an fp64 ``avg`` array holds T / (size size) for every live pair c < e and -inf in dead and lower cells, so
``np.argmax`` on the flat array is the largest average with ties to the lexicographically smallest (c, e); after a merge only
row and column c are refreshed.

The state's evolution does not depend on the stop rule, so the merges of any (threshold, min_clusters) are a prefix of the full
dendrogram: ``dendrogram`` runs down to one cluster once, ``cut`` applies the stop rule, ``ahc`` is the two together.  When half
of the slots of the working arrays are dead they are compacted (order kept, so the tie rule is untouched); ``compact=False``
keeps the plain n x n arrays throughout."""
import numpy as np


def dendrogram(scores, compact=True):
    """scores[n, >= n]: only the strict upper triangle is used.  -> (a int32[n-1], b int32[n-1], score float64[n-1])."""
    s = np.asarray(scores)
    n = s.shape[0]
    T = np.triu(s[:, :n], 1).astype(np.float64)
    T = T + T.T
    slot = np.arange(n)                                   # working position -> original slot
    size = np.ones(n, dtype=np.int64)
    alive = np.ones(n, dtype=bool)
    avg = np.full((n, n), -np.inf)
    iu = np.triu_indices(n, 1)
    avg[iu] = T[iu] / 1.0
    ma, mb, ms = np.zeros(n - 1, np.int32), np.zeros(n - 1, np.int32), np.zeros(n - 1, np.float64)
    for m in range(n - 1):
        w = T.shape[0]
        c, e = divmod(int(np.argmax(avg)), w)
        ma[m], mb[m], ms[m] = slot[c], slot[e], avg[c, e]
        k = alive.copy()
        k[c] = k[e] = False
        T[c, k] = T[c, k] + T[e, k]
        T[k, c] = T[c, k]
        size[c] += size[e]
        alive[e] = False
        avg[e, :] = -np.inf
        avg[:, e] = -np.inf
        val = T[c] / (size[c] * size).astype(np.float64)  # the int64 product, then one division
        hi = k & (np.arange(w) > c)
        lo = k & (np.arange(w) < c)
        avg[c, hi] = val[hi]
        avg[lo, c] = val[lo]
        if compact and w > 64 and 2 * int(alive.sum()) <= w:
            keep = np.flatnonzero(alive)
            T = np.ascontiguousarray(T[np.ix_(keep, keep)])
            avg = np.ascontiguousarray(avg[np.ix_(keep, keep)])
            slot, size, alive = slot[keep], size[keep], alive[keep]
    return ma, mb, ms


def cut(n, merges, threshold=-np.inf, min_clusters=1):
    """The stop rule on a full dendrogram: stop when the cluster count equals min_clusters or when not (avg >= threshold)."""
    a, b, sc = merges
    m = 0
    while m < n - min_clusters and sc[m] >= threshold:
        m += 1
    return a[:m].copy(), b[:m].copy(), sc[:m].copy()


def labels(n, a, b):
    """labels[i] = the slot of i's cluster after the merges (b[m] merges into a[m] < b[m])."""
    lab = np.arange(n, dtype=np.int32)
    for c, e in zip(a, b):
        lab[lab == e] = c
    return lab


def ahc(scores, threshold=-np.inf, min_clusters=1, compact=True):
    """-> (labels int32[n], (a, b, score)) of xv_ahc_average_f64's semantics."""
    n = np.asarray(scores).shape[0]
    a, b, sc = cut(n, dendrogram(scores, compact), threshold, min_clusters)
    return labels(n, a, b), (a, b, sc)
