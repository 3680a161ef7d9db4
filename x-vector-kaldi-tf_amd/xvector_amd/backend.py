"""LDA + PLDA scoring back-end: what stages 8-9 of the recipe (run.sh) do with Kaldi binaries.

  fit_lda        ivector-compute-lda --total-covariance-factor f --dim d      (host, fp64)
  fit_plda       ivector-compute-plda --num-em-iters n  -> Plda (mean, transform, psi)   (host, fp64)
  moment_stats   the first and second moment of vectors on the device, in fp64 on the f64 MFMA (xv_moment_stats_f64)
  adapt_plda     ivector-adapt-plda: unsupervised adaptation of a Plda to those moments   (host, fp64)
  cluster_vectors / ahc   clustering-based adaptation: the N x N PLDA score matrix of unlabelled vectors and its
                 average-linkage agglomerative clustering, both on the device (xv_score_matrix_f32, xv_ahc_average_f64)
  diarize / score_blocks / ahc_batch   diarization: one such problem per recording, all recordings' score
                 blocks from one launch (xv_score_blocks_f32) and one workgroup per recording's dendrogram
                 (xv_ahc_average_batch_f64)
  est_pca / Plda.apply_transform / pca_plda_groups   the per-recording PCA of ivector-plda-scoring-dense --target-energy and the
                 PLDA projected into it: fp64 on the host, and every recording's eigenproblems side by side on
                 the device (xv_pca_plda_groups_f64, xv_backend_prepare_groups_f32) behind diarize / score_blocks(target_energy=)
  interpolate_plda   a Plda between two (the out-of-domain model and the one fitted on the clusters)   (host, fp64)
  read_plda / write_plda, read_transform / write_transform   Kaldi's <Plda> object and transform.mat, binary and text
  prepare        ivector-subtract-global-mean | transform-vec | ivector-normalize-length | Plda::TransformIvector on the GPU
                 (xv_backend_prepare_f32)
  Scorer         ivector-plda-scoring (and cosine scoring): the prepared operands on the device, dense (xv_score_matrix_f32)
                 or per trial (xv_score_pairs_f32) -- bit-identical, so the choice between them is free; with a cohort,
                 adaptive symmetric score normalisation (AS-norm): cohort scores in chunks, their top-N statistics per row
                 (xv_topk_row_stats_f32), the normalised score on the device
  eer            compute-eer

The fits run once on the host in float64 NumPy on purpose: they are eigenproblems on scatter matrices, cost O(N D^2) and are
where precision matters; the GPU carries the part that scales with the data (preparing vectors and scoring trials).
"""
import io
import logging
import os
import sys

import numpy as np

from . import hiplib

logger = logging.getLogger("plda_backend")

_TF = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "local", "tf")


def _kaldi_io():
    if _TF not in sys.path:
        sys.path.insert(0, _TF)
    import kaldi_io
    return kaldi_io


# ------------------------------------------------------------------------------------------------
# fits (host, fp64)
# ------------------------------------------------------------------------------------------------
def _groups(labels):
    """labels[N] (any hashable) -> list of index arrays, one per class, in order of first appearance."""
    order, index = [], {}
    for i, l in enumerate(labels):
        if l not in index:
            index[l] = len(order)
            order.append([])
        order[index[l]].append(i)
    return [np.asarray(g, dtype=np.int64) for g in order]


def _eigh_desc(m):
    s, u = np.linalg.eigh((m + m.T) / 2)
    o = np.argsort(s)[::-1]
    return s[o], u[:, o]


def scatter_matrices(x, labels):
    """(mean, Sw, St) of x[N, D] with class labels[N]; both covariances divided by N (Kaldi's CovarianceStats)."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    mean = x.mean(axis=0)
    xc = x - mean
    st = xc.T @ xc / n
    sw = np.zeros_like(st)
    for g in _groups(labels):
        d = xc[g] - xc[g].mean(axis=0)
        sw += d.T @ d
    return mean, sw / n, st


def fit_lda(x, labels, dim, total_covariance_factor=0.0, covariance_floor=1e-6):
    """ivector-compute-lda: -> transform [dim, D + 1] (float64), the affine map y = A x + a0 with a0 = -A mean in the last column.

    M = f St + (1 - f) Sw is whitened by T = diag(s)^-1/2 U^T (its eigendecomposition, eigenvalues floored at
    covariance_floor * max, Kaldi's ComputeNormalizingTransform), the top-dim eigenvectors V of T Sb T^T (descending) give
    A = V^T T.  So A M A^T = I and A Sb A^T is diagonal and descending."""
    mean, sw, st = scatter_matrices(x, labels)
    D = sw.shape[0]
    if not 0 < dim <= D:
        raise ValueError("LDA dim %d must be in 1..%d" % (dim, D))
    m = total_covariance_factor * st + (1.0 - total_covariance_factor) * sw
    s, u = _eigh_desc(m)
    s = np.maximum(s, s.max() * covariance_floor)
    t = (u / np.sqrt(s)).T
    sb = st - sw
    _, v = _eigh_desc(t @ sb @ t.T)
    a = v[:, :dim].T @ t
    return np.hstack([a, -(a @ mean)[:, None]])


class Plda(object):
    """Kaldi's two-covariance PLDA after diagonalisation: mean [d], transform P [d, d] with P W P^T = I, P B P^T = diag(psi),
    psi [d] descending (all float64)."""

    def __init__(self, mean, transform, psi):
        self.mean = np.asarray(mean, dtype=np.float64)
        self.transform = np.asarray(transform, dtype=np.float64)
        self.psi = np.asarray(psi, dtype=np.float64)
        d = self.mean.shape[0]
        assert self.transform.shape == (d, d) and self.psi.shape == (d,)

    @property
    def dim(self):
        return self.mean.shape[0]

    def covariances(self):
        """(within, between) = (P^-1 P^-T, P^-1 diag(psi) P^-T), the model's two covariances (float64)."""
        inv = np.linalg.inv(self.transform)
        return inv @ inv.T, (inv * self.psi) @ inv.T

    def apply_transform(self, A, covariances=None):
        """Kaldi's Plda::ApplyTransform: the model of the vectors u = A y, A [p, d].  mean A mu, covariances
        A W A^T and A B A^T, diagonalised again as ``plda_from_covariances`` does.  covariances: what ``covariances()`` returned,
        for callers that project one model many times.  -> Plda of dimension p."""
        A = np.asarray(A, dtype=np.float64)
        if A.ndim != 2 or A.shape[1] != self.dim or not 1 <= A.shape[0] <= self.dim:
            raise ValueError("apply_transform: the transform must be [p, %d] with 1 <= p <= %d" % (self.dim, self.dim))
        W, B = self.covariances() if covariances is None else covariances
        return plda_from_covariances(A @ self.mean, A @ B @ A.T, A @ W @ A.T)


def _spk_stats(x, groups):
    """(mu = mean of the speaker means, means[S, d], counts[S], within-speaker scatter) over `groups` (index arrays into x)."""
    means, counts = [], []
    within = np.zeros((x.shape[1], x.shape[1]))
    for g in groups:
        m = x[g].mean(axis=0)
        d = x[g] - m
        within += d.T @ d
        means.append(m)
        counts.append(len(g))
    means = np.asarray(means)
    return means.mean(axis=0), means, np.asarray(counts), within


def plda_em_step(means, counts, mu, within_scatter, n_total, B, W):
    """One EM iteration of the two-covariance model x = mu + y_s + e, y ~ N(0, B), e ~ N(0, W) (Kaldi PldaEstimator).  -> (B, W)."""
    binv = np.linalg.inv(B)
    winv = np.linalg.inv(W)
    b_stats = np.zeros_like(B)
    w_stats = within_scatter.copy()
    for n in np.unique(counts):
        sel = counts == n
        sigma = np.linalg.inv(binv + n * winv)
        sigma = (sigma + sigma.T) / 2
        m = means[sel] - mu                                  # [S_n, d]
        y = m @ (n * winv) @ sigma                           # rows: Sigma_n n W^-1 (m_s - mu)   (both symmetric)
        k = int(sel.sum())
        b_stats += k * sigma + y.T @ y
        r = m - y
        w_stats += n * (k * sigma + r.T @ r)
    return b_stats / len(counts), w_stats / n_total


def fit_plda(x, spk_groups, num_em_iters=10, return_history=False):
    """ivector-compute-plda.  x[N, d] (float64 or float32); spk_groups: list of index arrays (one per speaker).  Speakers with
    a single utterance are skipped with a warning (they carry no within-speaker information).  -> Plda (and the list of
    (B, W) after every iteration when return_history)."""
    x = np.asarray(x, dtype=np.float64)
    groups = [np.asarray(g) for g in spk_groups]
    single = sum(1 for g in groups if len(g) == 1)
    if single:
        logger.warning("Skipping %d speakers with only one utterance" % single)
    groups = [g for g in groups if len(g) > 1]
    if not groups:
        raise ValueError("fit_plda: no speaker with two or more utterances")
    mu, means, counts, within = _spk_stats(x, groups)
    n_total = int(counts.sum())
    logger.info("Accumulated stats from %d speakers (%d with only one utterance, skipped), consisting of %d utterances." %
                (len(groups), single, n_total))
    d = x.shape[1]
    B, W = np.eye(d), np.eye(d)
    history = []
    for _ in range(num_em_iters):
        B, W = plda_em_step(means, counts, mu, within, n_total, B, W)
        history.append((B, W))
    plda = plda_from_covariances(mu, B, W)
    return (plda, history) if return_history else plda


def plda_from_covariances(mu, B, W):
    """Diagonalise: C = chol(W), T1 = C^-1 (Kaldi's ComputeNormalizingTransform), V = eigenvectors of T1 B T1^T (descending),
    P = V^T T1, psi = the eigenvalues (floored at 0)."""
    t1 = np.linalg.inv(np.linalg.cholesky((W + W.T) / 2))
    s, v = _eigh_desc(t1 @ B @ t1.T)
    return Plda(mu, v.T @ t1, np.maximum(s, 0.0))


def adapt_plda(plda, n, sum, outer, within_covar_scale=0.3, between_covar_scale=0.7, mean_diff_scale=1.0):
    """ivector-adapt-plda (Kaldi's PldaUnsupervisedAdaptor::UpdatePlda): adapt `plda` to n unlabelled in-domain vectors given by
    their moments sum[d] = sum_i y_i and outer[d, d] = sum_i y_i y_i^T (moment_stats).  -> Plda.

    m = sum / n becomes the mean; V = outer / n - m m^T + mean_diff_scale (m - mu)(m - mu)^T is the in-domain total covariance.
    In the space of P' = diag(1 / sqrt(1 + psi)) P the model's total covariance is I, its within-speaker covariance
    diag(1 / (1 + psi)) and its between-speaker covariance diag(psi / (1 + psi)).  For every eigenvalue s_i > 1 of P' V P'^T
    (eigenvector p_i) the excess (s_i - 1) p_i p_i^T is shared out: within_covar_scale of it to W, between_covar_scale of it
    to B.  Directions in which the in-domain data varies less than the model are left alone.  The covariances are mapped back
    with P'^-1 and diagonalised again (plda_from_covariances)."""
    d = plda.dim
    for name, v in (("within_covar_scale", within_covar_scale), ("between_covar_scale", between_covar_scale),
                    ("mean_diff_scale", mean_diff_scale)):
        if not (np.isfinite(v) and v >= 0.0):
            raise ValueError("adapt_plda: %s must be in [0, inf), got %r" % (name, v))
    if not n >= 1:
        raise ValueError("adapt_plda: no vectors (n = %r)" % (n,))
    s1 = np.asarray(sum, dtype=np.float64)
    s2 = np.asarray(outer, dtype=np.float64)
    if s1.shape != (d,) or s2.shape != (d, d):
        raise ValueError("adapt_plda: moments of shape %r / %r do not fit a PLDA of dimension %d" % (s1.shape, s2.shape, d))
    if not (np.all(np.isfinite(s1)) and np.all(np.isfinite(s2))):
        raise ValueError("adapt_plda: the moments are not finite")
    m = s1 / n
    var = s2 / n - np.outer(m, m)
    diff = m - plda.mean
    var += mean_diff_scale * np.outer(diff, diff)
    p1 = plda.transform / np.sqrt(1.0 + plda.psi)[:, None]
    s, p = _eigh_desc(p1 @ var @ p1.T)
    w1 = np.diag(1.0 / (1.0 + plda.psi))
    b1 = np.diag(plda.psi / (1.0 + plda.psi))
    above = 0
    for i in range(d):
        if s[i] > 1.0:
            excess = (s[i] - 1.0) * np.outer(p[:, i], p[:, i])
            w1 += within_covar_scale * excess
            b1 += between_covar_scale * excess
            above += 1
    logger.info("Adapting to %d vectors: %d of %d eigenvalues of the in-domain covariance are above 1 in the model's space "
                "(largest %g)" % (n, above, d, s[0]))
    inv = np.linalg.inv(p1)
    return plda_from_covariances(m, inv @ b1 @ inv.T, inv @ w1 @ inv.T)


# ------------------------------------------------------------------------------------------------
# Kaldi I/O: <Plda> and transform.mat
# ------------------------------------------------------------------------------------------------
def _binary_body(write, a):
    """The bytes kaldi_io writes for one binary vector / matrix, without the stream's leading \\0B."""
    bio = io.BytesIO()
    write(bio, a)
    b = bio.getvalue()
    assert b[:2] == b"\x00B"
    return b[2:]


def _text_vector(v):
    return " [ " + "".join(repr(float(x)) + " " for x in v) + "]\n"


def _text_matrix(m):
    if m.size == 0:
        return " [ ]\n"
    return " [" + "".join("\n  " + "".join(repr(float(x)) + " " for x in row) for row in m) + "]\n"


def write_plda(path, plda, binary=True):
    """Kaldi's Plda::Write: <Plda> mean transform psi </Plda> (binary: \\0B, tokens with a trailing space, DV / DM framing)."""
    kio = _kaldi_io()
    with open(path, "wb") as f:
        if binary:
            f.write(b"\x00B<Plda> ")
            f.write(_binary_body(kio.write_vec_flt, plda.mean))
            f.write(_binary_body(kio.write_mat, plda.transform))
            f.write(_binary_body(kio.write_vec_flt, plda.psi))
            f.write(b"</Plda> ")
        else:
            f.write(("<Plda> " + _text_vector(plda.mean) + _text_matrix(plda.transform) + _text_vector(plda.psi) +
                     "</Plda> ").encode())


def _expect(fd, token):
    got = fd.read(len(token))
    if got != token:
        raise ValueError("expected %r, got %r" % (token, got))


def read_plda(path):
    """A Kaldi <Plda> object, binary or text."""
    kio = _kaldi_io()
    with open(path, "rb") as f:
        head = f.read(2)
        if head == b"\x00B":
            _expect(f, b"<Plda> ")
            mean = np.array(kio._read_vec_flt_binary(f), dtype=np.float64)
            transform = np.array(kio._read_mat_binary(f), dtype=np.float64)
            psi = np.array(kio._read_vec_flt_binary(f), dtype=np.float64)
            _expect(f, b"</Plda>")
            return Plda(mean, transform, psi)
        toks = (head + f.read()).decode().split()
    if not toks or toks[0] != "<Plda>" or toks[-1] != "</Plda>":
        raise ValueError("%s: not a Kaldi <Plda> object" % path)
    arrays, cur = [], None
    for t in toks[1:-1]:
        if t == "[":
            cur = []
        elif t == "]":
            arrays.append(np.array(cur, dtype=np.float64))
            cur = None
        else:
            cur.append(float(t))
    mean, transform, psi = arrays
    d = mean.shape[0]
    return Plda(mean, transform.reshape(d, d), psi)


def write_transform(path, m, binary=True):
    """transform.mat as ivector-compute-lda writes it (Matrix<BaseFloat>: FM)."""
    kio = _kaldi_io()
    m = np.asarray(m, dtype=np.float32)
    if binary:
        kio.write_mat(path, m)
    else:
        with open(path, "w") as f:
            f.write(_text_matrix(m))


def read_transform(path):
    """A Kaldi matrix file (binary FM / DM or text) as float32, the precision transform-vec applies it in."""
    kio = _kaldi_io()
    with open(path, "rb") as f:
        head = f.read(2)
        if head == b"\x00B":
            return np.array(kio._read_mat_binary(f), dtype=np.float32)
        toks = (head + f.read()).decode()
    rows = [l.replace("[", " ").replace("]", " ").split() for l in toks.splitlines()]
    rows = [r for r in rows if r]
    return np.array(rows, dtype=np.float32)


# ------------------------------------------------------------------------------------------------
# device side: prepare + score
# ------------------------------------------------------------------------------------------------
def kpad_for(k):
    return (k + hiplib.BACKEND_KSTEP - 1) // hiplib.BACKEND_KSTEP * hiplib.BACKEND_KSTEP


def _dev(a, device, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32 if dtype is None else dtype), device=device)


def prepare(x, side, num_utts=None, mean=None, transform=None, plda=None, length_norm=True, device="cuda:0"):
    """Operand rows of the scorers from raw vectors x[N, D] on the device (xv_backend_prepare_f32).

    side: hiplib.SIDE_PLAIN | SIDE_ENROL | SIDE_TEST | SIDE_COSINE;  mean: [D] subtracted first (None: nothing);
    transform: LDA [d, D] or [d, D + 1] (offset in the last column; None: no LDA); length_norm: scale to norm sqrt(d)
    (ivector-normalize-length); plda: Plda (None: no PLDA step; then only PLAIN / COSINE).  -> (rows[N, Kpad], r[N]) torch."""
    import torch
    hiplib.require_gpu()
    xt = x if isinstance(x, torch.Tensor) else _dev(x, device)
    xt = xt.to(device=device, dtype=torch.float32).contiguous()
    n, D = xt.shape
    a = a0 = None
    d = D
    if transform is not None:
        transform = np.asarray(transform)
        if transform.shape[1] not in (D, D + 1):
            raise ValueError("transform has %d columns, the vectors %d" % (transform.shape[1], D))
        d = transform.shape[0]
        a = _dev(transform[:, :D], device)
        a0 = _dev(transform[:, D], device) if transform.shape[1] == D + 1 else None
    if plda is not None and plda.dim != d:
        raise ValueError("PLDA dim %d != vector dim %d" % (plda.dim, d))
    k = 2 * d if side in (hiplib.SIDE_ENROL, hiplib.SIDE_TEST) else d
    out = torch.empty((n, kpad_for(k)), dtype=torch.float32, device=device)
    r = torch.empty(n, dtype=torch.float32, device=device)
    nu = None
    if num_utts is not None:
        nu = torch.as_tensor(np.ascontiguousarray(num_utts, dtype=np.int32), device=device)
    hiplib.backend_prepare(xt, out, side, num_utts=nu, mean=None if mean is None else _dev(mean, device), lda=a, lda_offset=a0,
                           length_norm=length_norm,
                           plda_transform=None if plda is None else _dev(plda.transform, device),
                           plda_mean=None if plda is None else _dev(plda.mean, device),
                           plda_psi=None if plda is None else _dev(plda.psi, device), r=r)
    return out, r


MOMENT_CHUNK_ROWS = 1 << 18        # rows per xv_moment_stats_f64 call of moment_stats: a constant, so the bits are too


def moment_stats(x_rows, dim=None, device="cuda:0"):
    """(n, sum[dim], outer[dim, dim]) of the first dim columns of x_rows[N, >= dim], float64 NumPy: sum = sum_i x_i,
    outer = sum_i x_i x_i^T, on the f64 MFMA (xv_moment_stats_f64).

    x_rows: a float32 torch tensor on the device whose row stride is a multiple of 4 (what prepare returns: the rows are used
    where they are), or a host array (uploaded chunk by chunk, rows padded to a multiple of 4 columns).  The rows go through
    the kernel in chunks of MOMENT_CHUNK_ROWS and the chunk results are added here in fp64 in chunk order, so the result's bits
    depend on the values alone, not on the memory that happens to be free."""
    import torch
    hiplib.require_gpu()
    on_device = isinstance(x_rows, torch.Tensor)
    if not on_device:
        x_rows = np.asarray(x_rows, dtype=np.float32)
    if x_rows.ndim != 2:
        raise ValueError("moment_stats: x_rows must be [N, D]")
    n = int(x_rows.shape[0])
    dim = int(x_rows.shape[1]) if dim is None else int(dim)
    if n < 1:
        raise ValueError("moment_stats: no vectors")
    if not 1 <= dim <= x_rows.shape[1]:
        raise ValueError("moment_stats: dim %d must be in 1..%d" % (dim, x_rows.shape[1]))
    if dim > hiplib.MOMENT_DIM_MAX:
        raise ValueError("moment_stats: dim %d exceeds %d, the limit of xv_moment_stats_f64" % (dim, hiplib.MOMENT_DIM_MAX))
    if on_device:
        x_rows = x_rows.to(device=device, dtype=torch.float32)
        if x_rows.stride(1) != 1 or x_rows.stride(0) % 4 or x_rows.data_ptr() % 16:
            x_rows = torch.nn.functional.pad(x_rows[:, :dim], (0, -dim % 4)).contiguous()
    rows = min(n, MOMENT_CHUNK_ROWS)
    s_d = torch.empty(dim, dtype=torch.float64, device=device)
    o_d = torch.empty((dim, dim), dtype=torch.float64, device=device)
    ws = torch.empty(hiplib.moment_stats_workspace_bytes(rows, dim), dtype=torch.uint8, device=device)
    stage = None if on_device else torch.zeros((rows, (dim + 3) // 4 * 4), dtype=torch.float32, device=device)
    total_s = np.zeros(dim)
    total_o = np.zeros((dim, dim))
    for i0 in range(0, n, MOMENT_CHUNK_ROWS):
        m = min(MOMENT_CHUNK_ROWS, n - i0)
        if on_device:
            chunk = x_rows[i0:i0 + m]
        else:
            stage[:m, :dim] = torch.as_tensor(np.ascontiguousarray(x_rows[i0:i0 + m, :dim]), device=device)
            chunk = stage[:m]
        hiplib.moment_stats(chunk, s_d, o_d, dim=dim, workspace=ws)
        total_s += s_d.cpu().numpy()
        total_o += o_d.cpu().numpy()
    return n, total_s, total_o


def interpolate_plda(plda_out, plda_in, alpha):
    """(1 - alpha) * plda_out + alpha * plda_in, mixed where the models are linear: with P the transform, the between- and
    within-speaker covariances B = P^-1 diag(psi) P^-T and W = P^-1 P^-T of both models and their means are mixed, and the mix
    is diagonalised again (plda_from_covariances).  -> Plda."""
    if not (np.isfinite(alpha) and 0.0 <= alpha <= 1.0):
        raise ValueError("interpolate_plda: alpha must be in [0, 1], got %r" % (alpha,))
    if plda_out.dim != plda_in.dim:
        raise ValueError("interpolate_plda: the models have dimensions %d and %d" % (plda_out.dim, plda_in.dim))
    parts = []
    for p in (plda_out, plda_in):
        inv = np.linalg.inv(p.transform)
        parts.append((p.mean, (inv * p.psi) @ inv.T, inv @ inv.T))
    mean, B, W = ((1.0 - alpha) * o + alpha * i for o, i in zip(*parts))
    return plda_from_covariances(mean, B, W)


# ------------------------------------------------------------------------------------------------
# clustering of unlabelled vectors by PLDA score
# ------------------------------------------------------------------------------------------------
AHC_MAX_BYTES = 12 << 30           # the fp64 state of ahc is at most this large by default (N = 32768 needs 8 GiB)
_FINITE_CHECK_ELEMS = 1 << 26      # elements per slice of the device-side check of the upper triangle


def labels_from_merges(n, a, b):
    """labels[i] (int32) = the slot of i's cluster after the merges (a[m], b[m]) in order: b[m] joins a[m] < b[m], and a cluster
    lives in the slot of its smallest member.  The host restatement of xv_ahc_average_f64's labels, for callers that cut the
    dendrogram elsewhere."""
    a = np.asarray(a, dtype=np.int64)
    b = np.asarray(b, dtype=np.int64)
    if a.shape != b.shape or a.ndim != 1:
        raise ValueError("labels_from_merges: a and b must be 1-D and of the same length")
    parent = np.arange(n, dtype=np.int64)
    for c, e in zip(a.tolist(), b.tolist()):
        if not (0 <= c < e < n) or parent[c] != c or parent[e] != e:
            raise ValueError("labels_from_merges: merge (%d, %d) does not join two live slots c < e" % (c, e))
        parent[e] = c
    for i in range(n):                                       # parents only decrease: parent[parent[i]] is final when i is reached
        parent[i] = parent[parent[i]]
    return parent.astype(np.int32)


def ahc(scores, threshold=0.0, num_clusters=None, max_bytes=AHC_MAX_BYTES):
    """Average-linkage agglomerative clustering of scores[N, N] (a float32 device tensor; only the strict upper triangle is
    used) on the device (xv_ahc_average_f64): merge the pair of clusters with the largest average score, ties to the
    lexicographically smallest pair, until no average reaches ``threshold``.  num_clusters given: stop at that many clusters at
    the latest (threshold None: at exactly that many).  -> (labels int32[N], (a int32[M], b int32[M], score float64[M])) as
    NumPy: labels[i] is the smallest member of i's cluster, merge m joined b[m] into a[m] at average score[m]."""
    import torch
    hiplib.require_gpu()
    if not (isinstance(scores, torch.Tensor) and scores.is_cuda and scores.dim() == 2 and scores.shape[0] == scores.shape[1]):
        raise ValueError("ahc: scores must be a device tensor [N, N]")
    n = int(scores.shape[0])
    if n < 1:
        raise ValueError("ahc: no items")
    if n > hiplib.AHC_MAX_N:
        raise ValueError("ahc: %d items exceed %d, the limit of xv_ahc_average_f64" % (n, hiplib.AHC_MAX_N))
    if threshold is None:
        if num_clusters is None:
            raise ValueError("ahc: threshold None needs num_clusters")
        threshold = -np.inf
    threshold = float(threshold)
    if np.isnan(threshold):
        raise ValueError("ahc: the threshold is NaN")
    min_clusters = 1 if num_clusters is None else int(num_clusters)
    if not 1 <= min_clusters <= n:
        raise ValueError("ahc: num_clusters %d must be in 1..%d" % (min_clusters, n))
    need = hiplib.ahc_average_workspace_bytes(n)
    if need > max_bytes:
        raise ValueError("ahc: %d items need a workspace of %d bytes, more than max_bytes = %d" % (n, need, max_bytes))
    scores = scores.to(torch.float32)
    if scores.stride(1) != 1 or scores.stride(0) % 4 or scores.data_ptr() % 16:
        scores = torch.nn.functional.pad(scores, (0, -n % 4)).contiguous()[:, :n]
    dev = scores.device
    rows = max(1, _FINITE_CHECK_ELEMS // n)
    col = torch.arange(n, device=dev)
    for i0 in range(0, n - 1, rows):
        blk = scores[i0:i0 + rows]
        lower = col[None, :] <= torch.arange(i0, i0 + blk.shape[0], device=dev)[:, None]
        if not bool((torch.isfinite(blk) | lower).all()):
            raise ValueError("ahc: the upper triangle of the score matrix holds a value that is not finite")
    with torch.cuda.device(dev):
        m_a = torch.empty(max(n - 1, 1), dtype=torch.int32, device=dev)
        m_b = torch.empty_like(m_a)
        m_s = torch.empty(max(n - 1, 1), dtype=torch.float64, device=dev)
        cnt = torch.empty(1, dtype=torch.int32, device=dev)
        lab = torch.empty(n, dtype=torch.int32, device=dev)
        hiplib.ahc_average(scores, threshold, min_clusters, m_a, m_b, m_s, cnt, lab)
        m = int(cnt.cpu()[0])
    return lab.cpu().numpy(), (m_a[:m].cpu().numpy(), m_b[:m].cpu().numpy(), m_s[:m].cpu().numpy())


def _self_operands(x, plda, mean, transform, device):
    """(E, r, T): the rows of x prepared as one-utterance enrolments (with their r) and as tests, the operands that score x against
    itself (the pair of prepare calls of the test-side AS-norm statistics)."""
    ln = transform is not None
    E, r = prepare(x, hiplib.SIDE_ENROL, np.ones(len(x), np.int32), mean, transform, plda, ln, device)
    T, _ = prepare(x, hiplib.SIDE_TEST, None, mean, transform, plda, ln, device)
    return E, r, T


def score_matrix_self(x, plda, mean=None, transform=None, device="cuda:0"):
    """S[N, ld] on the device, ld = N rounded up to a multiple of 4: S[i, j] = the PLDA LLR of vector i as a one-utterance
    enrolment against vector j as a test (``_self_operands``)."""
    import torch
    n = len(x)
    E, r, T = _self_operands(x, plda, mean, transform, device)
    s = torch.empty((n, (n + 3) // 4 * 4), dtype=torch.float32, device=device)
    hiplib.score_matrix(E, T, r, s)
    return s


def cluster_vectors(x, plda, mean=None, transform=None, threshold=0.0, num_clusters=None, device="cuda:0"):
    """Cluster the raw vectors x[N, D] by PLDA score: mean / transform run the stage-9 chain on the device first (None: the vectors
    are used as they are), the N x N score matrix stays there and goes through ``ahc``.  -> (labels, merges) as ``ahc``."""
    hiplib.require_gpu()
    n = len(x)
    if n < 1:
        raise ValueError("cluster_vectors: no vectors")
    if n > hiplib.AHC_MAX_N:
        raise ValueError("cluster_vectors: %d vectors exceed %d, the limit of xv_ahc_average_f64" % (n, hiplib.AHC_MAX_N))
    s = score_matrix_self(x, plda, mean, transform, device)
    return ahc(s[:, :n], threshold, num_clusters)


# ------------------------------------------------------------------------------------------------
# diarization: one small clustering problem per recording, all of them in one batch
# ------------------------------------------------------------------------------------------------
class GroupTables(object):
    """The ragged-batch tables of xv_score_blocks_f32 / xv_ahc_average_batch_f64 for groups of ``sizes`` rows, in that order:
    row0 int32 [G + 1] (prefix sums), ld int64 [G] (the row stride of a group's score block, its size rounded up to a multiple of
    4), score0 int64 [G] (element offsets of the blocks, packed back to back) and scores_elems; row0_d / score0_d are their device
    copies and status the device word both kernels report a skipped group in (zeroed here).  What ``score_blocks`` leaves here for
    the later stages: pca, an int32 device tensor [2 G], every group's retained dimension followed by the 0 / 1 / 2 fallback codes
    (None without a PCA); pca_host, its NumPy copy once ``ahc_batch`` has downloaded it; plain, the PLAIN-prepared device rows
    (None unless asked for with keep_plain)."""

    def __init__(self, sizes, device=None):
        self.sizes = np.asarray(sizes, dtype=np.int64).reshape(-1)
        if self.sizes.size < 1 or int(self.sizes.min()) < 1:
            raise ValueError("every group needs at least one row, and there must be a group")
        if int(self.sizes.sum()) > np.iinfo(np.int32).max:
            raise ValueError("too many rows for int32 row offsets")
        self.row0 = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int32)
        self.ld = (self.sizes + 3) & ~3
        elems = self.sizes * self.ld
        self.score0 = np.concatenate([[0], np.cumsum(elems)[:-1]]).astype(np.int64)
        self.scores_elems = int(elems.sum())
        self.n_rows = int(self.row0[-1])
        self.max_n = int(self.sizes.max())
        self.row0_d = self.score0_d = self.status = None
        self.pca = self.pca_host = self.plain = None
        if device is not None:
            import torch
            self.row0_d = torch.as_tensor(self.row0, device=device)
            self.score0_d = torch.as_tensor(self.score0, device=device)
            self.status = torch.zeros(1, dtype=torch.int32, device=device)

    def block(self, scores, g):
        """Group g's [n, n] view of the packed scores (a device tensor or a host array)."""
        n, ld, o = int(self.sizes[g]), int(self.ld[g]), int(self.score0[g])
        return scores[o:o + n * ld].reshape(n, ld)[:, :n]


def size_order(sizes):
    """(order, inverse): order lists the groups by size, descending (equal sizes keep their order), as the device wants them --
    workgroups tend to start in group order and the largest group runs longest (only speed depends on it); inverse[g] is the position of group g in order."""
    order = np.argsort(-np.asarray(sizes, dtype=np.int64), kind="stable")
    inverse = np.empty_like(order)
    inverse[order] = np.arange(order.size)
    return order, inverse


def _cut_runs(lo, hi, fits):
    """Cut the consecutive groups lo .. hi - 1 greedily into runs under a budget: -> [(a, b)], each run [a, b) grown while
    fits(a, b) says that groups [a, b) fit.  ValueError(g) when group g does not fit alone; the planners say it in their words."""
    runs, a = [], lo
    for g in range(lo, hi):
        if g > a and not fits(a, g + 1):
            runs.append((a, g))
            a = g
        if g == a and not fits(g, g + 1):
            raise ValueError(g)
    return runs + [(a, hi)] if hi > lo else runs


def plan_ahc_batch(sizes, max_bytes=AHC_MAX_BYTES, max_batch_n=hiplib.AHC_BATCH_MAX_N):
    """Cut the group list into calls of xv_ahc_average_batch_f64: -> (calls, routed).  calls: a list of (g_lo, g_hi, ws0, nbytes):
    groups [g_lo, g_hi) in one call, ws0 int64 [g_hi - g_lo] their byte offsets into a workspace of nbytes <= max_bytes.  A call
    is a run of consecutive groups, because a group's rows are found by a prefix-sum table.  routed: the groups above max_batch_n,
    which go through the single-problem ``ahc`` on their block.  A group whose own workspace exceeds max_bytes is an error."""
    max_batch_n = min(int(max_batch_n), hiplib.AHC_BATCH_MAX_N)
    sizes = np.asarray(sizes, dtype=np.int64).reshape(-1).tolist()
    routed = [g for g, n in enumerate(sizes) if n > max_batch_n]
    need = [0 if n > max_batch_n else hiplib.ahc_average_batch_workspace_bytes(n) for n in sizes]
    end = np.concatenate([[0], np.cumsum(need, dtype=np.int64)]).tolist()    # a call's workspace offsets: the sum of the needs before
    calls = []
    for lo, hi in zip([0] + [g + 1 for g in routed], routed + [len(sizes)]):       # the stretches between routed groups, in order
        try:
            for a, b in _cut_runs(lo, hi, lambda a, b: end[b] - end[a] <= max_bytes):
                calls.append((a, b, np.asarray(end[a:b], dtype=np.int64) - end[a], end[b] - end[a]))
        except ValueError as e:
            g = e.args[0]
            raise ValueError("ahc_batch: a group of %d items needs a workspace of %d bytes, more than max_bytes = %d" %
                             (sizes[g], need[g], max_bytes))
        if hi < len(sizes) and hiplib.ahc_average_workspace_bytes(sizes[hi]) > max_bytes:
            raise ValueError("ahc_batch: a group of %d items needs a workspace of more than max_bytes = %d" % (sizes[hi], max_bytes))
    return calls, routed


# ---- per-recording PCA (ivector-plda-scoring-dense --target-energy) ----
PCA_MAX_BYTES = 1 << 30            # the per-group tables and workspace of one xv_pca_plda_groups_f64 call are at most this large
PCA_INFO_NAMES = ("PCA applied", "fallback: no energy", "fallback: no convergence")


def target_energy_is_one(target_energy):
    """Kaldi's ApproxEqual(target_energy, 1.0, 0.001): the PCA is skipped altogether."""
    t = float(target_energy)
    return abs(t - 1.0) <= 0.001 * (abs(t) + 1.0)


def check_target_energy(target_energy):
    """The target energy as a float; ValueError unless it is in (0, 1] or approximately 1."""
    t = float(target_energy)
    if not np.isfinite(t) or not (target_energy_is_one(t) or 0.0 < t <= 1.0):
        raise ValueError("the target energy must be in (0, 1], got %r" % (target_energy,))
    return t


def energy_dim(eigvals, target_energy):
    """The retained dimension of the energy rule for eigenvalues sorted descending: with k the smallest count whose share
    (l_1 + .. + l_k) / total exceeds target_energy (d if none), p = min(k + 1, d) -- Kaldi's loop steps once past the count it
    summed.  None (the fallback) when the total is not finite or not > 0."""
    s = np.asarray(eigvals, dtype=np.float64)
    total = 0.0
    for v in s.tolist():
        total += v
    if not (np.isfinite(total) and total > 0.0):
        return None
    cum, k = 0.0, s.size
    for i, v in enumerate(s.tolist()):
        cum += v
        if cum / total > target_energy:
            k = i + 1
            break
    return min(k + 1, s.size)


def order_eigenpairs(s, u):
    """(eigenvalues descending, eigenvectors as ROWS): ties go to the smaller original column index, and every eigenvector's sign
    is fixed so that its first component of largest magnitude is positive."""
    s = np.asarray(s, dtype=np.float64)
    o = np.argsort(-s, kind="stable")
    rows = np.asarray(u, dtype=np.float64)[:, o].T.copy()
    at = np.argmax(np.abs(rows), axis=1)
    rows[rows[np.arange(rows.shape[0]), at] < 0] *= -1.0
    return s[o], rows


def est_pca(y, target_energy):
    """Kaldi's EstPca on one recording's rows y[n, d]: C = (1/n) sum y y^T - m m^T in float64, its eigenpairs
    ordered by ``order_eigenpairs``, the retained dimension by ``energy_dim``.  The vectors are NOT centred when projected:
    u = A y.  -> (A [p, d], eigvals [d] descending), or None for the fallback to the global model."""
    y = np.asarray(y, dtype=np.float64)
    if y.ndim != 2 or y.shape[0] < 1:
        raise ValueError("est_pca: y must be [n, d] with n >= 1")
    n = y.shape[0]
    m = y.sum(axis=0) / n
    C = y.T @ y / n - np.outer(m, m)
    if not np.all(np.isfinite(C)):
        return None
    s, rows = order_eigenpairs(*np.linalg.eigh((C + C.T) / 2))
    p = energy_dim(s, target_energy)
    if p is None:
        return None
    return rows[:p], s


def host_pca_tables(y, group_sizes, plda, target_energy):
    """The per-group tables of xv_pca_plda_groups_f64 from ``est_pca`` and ``Plda.apply_transform`` on the host, one recording
    after the other (the NumPy route xv_pca_plda_groups_f64 is measured against): -> dict(dim int32 [G], info int32 [G],
    psi [G, d], map [G, d, d], off [G, d]) with z = map y + off; a fallback group holds the global model."""
    y = np.asarray(y, dtype=np.float64)
    sizes = np.asarray(group_sizes, dtype=np.int64)
    G, d = sizes.size, plda.dim
    out = dict(dim=np.full(G, d, np.int32), info=np.zeros(G, np.int32), psi=np.zeros((G, d)), map=np.zeros((G, d, d)),
               off=np.zeros((G, d)))
    at = 0
    cov = plda.covariances()
    for g, n in enumerate(sizes.tolist()):
        est = est_pca(y[at:at + n, :d], target_energy)
        at += n
        if est is None:
            out["info"][g] = 1
            out["psi"][g], out["map"][g], out["off"][g] = plda.psi, plda.transform, -(plda.transform @ plda.mean)
            continue
        A = est[0]
        pg = plda.apply_transform(A, cov)
        p = A.shape[0]
        out["dim"][g] = p
        out["psi"][g, :p] = pg.psi
        out["map"][g, :p] = pg.transform @ A
        out["off"][g, :p] = -(pg.transform @ pg.mean)
    return out


def plan_pca_groups(n_groups, dim, max_bytes=PCA_MAX_BYTES, keep_pca=False):
    """Cut n_groups groups into calls of xv_pca_plda_groups_f64 whose per-group tables and workspace fit max_bytes:
    -> (groups per call, [(g_lo, g_hi)]).  One group alone above max_bytes is an error."""
    per = 8 * (3 * dim + (2 if keep_pca else 1) * dim * dim) + hiplib.pca_plda_groups_workspace_bytes(1, dim)
    if per > max_bytes:
        raise ValueError("pca_plda_groups: one group of dimension %d needs %d bytes, more than max_bytes = %d" % (dim, per, max_bytes))
    step = int(min(n_groups, max_bytes // per))
    return step, [(lo, min(lo + step, n_groups)) for lo in range(0, n_groups, step)]


def pca_plda_groups(y_rows, tables, plda, target_energy, grp_dim, grp_info, max_bytes=PCA_MAX_BYTES, keep_pca=False):
    """Every group's PCA and projected PLDA on the device (xv_pca_plda_groups_f64).  y_rows: float32 device rows [N, >= d], the
    vectors after mean subtraction, LDA and length normalisation (``prepare(..., SIDE_PLAIN, plda=None)``); tables: their
    GroupTables; grp_dim, grp_info: int32 device tensors [G] that receive every group's retained dimension and 0 / 1 / 2 (PCA
    applied / fallback for energy / fallback for non-convergence).  The fp64 model is uploaded once.  The group list is cut into
    calls whose tables and workspace fit max_bytes (``plan_pca_groups``); this GENERATOR yields, per call,
    (g_lo, g_hi, dict(eigvals [g, d], psi [g, d], map [g, d, d], off [g, d], pca [g, d, d] or None)) -- float64 device tensors
    that the next call overwrites, so the consumer launches what reads them (``hiplib.backend_prepare_groups``) before it asks
    for the next.  Nothing is synchronised or read back: a skipped group shows in tables.status."""
    import torch
    hiplib.require_gpu()
    target_energy = check_target_energy(target_energy)
    d, G = plda.dim, tables.sizes.size
    if d > hiplib.PCA_MAX_DIM:
        raise ValueError("pca_plda_groups: dimension %d exceeds %d, the limit of xv_pca_plda_groups_f64" % (d, hiplib.PCA_MAX_DIM))
    step, calls = plan_pca_groups(G, d, max_bytes, keep_pca)
    dev = y_rows.device
    f64 = dict(dtype=torch.float64, device=dev)
    W, B = plda.covariances()
    model = [torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev) for a in (plda.mean, W, B, plda.transform, plda.psi)]
    with torch.cuda.device(dev):
        t = dict(eigvals=torch.empty((step, d), **f64), psi=torch.empty((step, d), **f64), map=torch.empty((step, d, d), **f64),
                 off=torch.empty((step, d), **f64), pca=torch.empty((step, d, d), **f64) if keep_pca else None)
        ws = torch.empty(hiplib.pca_plda_groups_workspace_bytes(step, d), dtype=torch.uint8, device=dev)
        for lo, hi in calls:
            hiplib.pca_plda_groups(y_rows, tables.row0_d[lo:hi + 1], d, min(target_energy, 1.0), *model, grp_dim[lo:hi], grp_info[lo:hi],
                                   t["eigvals"], t["pca"], t["psi"], t["map"], t["off"], tables.status, ws)
            yield lo, hi, {k: (None if v is None else v[:hi - lo]) for k, v in t.items()}


def _nonfinite_upper(scores, tables):
    """A device bool: does the strict upper triangle of any group's block hold a value that is not finite?  No host sync."""
    import torch
    dev = scores.device
    n_d = torch.as_tensor(tables.sizes, device=dev)
    ld_d = torch.as_tensor(tables.ld, device=dev)
    bad = torch.zeros((), dtype=torch.bool, device=dev)
    for lo in range(0, scores.numel(), _FINITE_CHECK_ELEMS):
        chunk = scores[lo:lo + _FINITE_CHECK_ELEMS]
        idx = torch.arange(lo, lo + chunk.numel(), device=dev)
        g = torch.searchsorted(tables.score0_d, idx, right=True) - 1
        inside = g >= 0
        g = g.clamp_(min=0)
        local = idx - tables.score0_d[g]
        i, j = local // ld_d[g], local % ld_d[g]
        upper = inside & (j > i) & (j < n_d[g]) & (i < n_d[g])
        bad = bad | (upper & ~torch.isfinite(chunk)).any()
    return bad


def score_blocks(x, group_sizes, plda, mean=None, transform=None, device="cuda:0", target_energy=1.0, pca_max_bytes=PCA_MAX_BYTES,
                 keep_plain=False):
    """Every group's PLDA score matrix from one launch (xv_score_blocks_f32): x[N, D] raw vectors, group g the next
    group_sizes[g] rows.  The chain is that of ``score_matrix_self`` (two prepare calls over all rows, one-utterance enrolments),
    and a block holds the bits ``score_matrix_self`` gives that group's rows.  -> (scores, tables): the packed float32 device
    blocks and their GroupTables; tables.status stays on the device (``ahc_batch`` downloads it with its results).

    target_energy below 1 (ivector-plda-scoring-dense --target-energy): every group is scored under its own
    PCA and projected PLDA instead -- one PLAIN prepare without the PLDA, ``pca_plda_groups``, the grouped prepare for both
    sides, then the same scorer -- and tables.pca holds the retained dimensions and fallback codes (``GroupTables``).

    keep_plain: tables.plain is then the PLAIN-prepared device rows (mean, LDA, length normalisation; no PLDA) that ``vbx_groups``
    reads -- the PCA route's own, or one more prepare call on the default route."""
    import torch
    hiplib.require_gpu()
    target_energy = check_target_energy(target_energy)
    use_pca = not target_energy_is_one(target_energy)
    if use_pca and plda.dim > hiplib.PCA_MAX_DIM:
        raise ValueError("score_blocks: the per-recording PCA handles dimensions up to %d, the PLDA has %d" %
                         (hiplib.PCA_MAX_DIM, plda.dim))
    tables = GroupTables(group_sizes, device)
    n = len(x)
    if n != tables.n_rows:
        raise ValueError("score_blocks: %d vectors, but the group sizes add up to %d" % (n, tables.n_rows))
    ln = transform is not None
    if use_pca:
        d, G = plda.dim, tables.sizes.size
        Y, _ = prepare(x, hiplib.SIDE_PLAIN, None, mean, transform, None, ln, device)
        if Y.shape[1] < d:
            raise ValueError("PLDA dim %d != vector dim %d" % (d, Y.shape[1]))
        E = torch.empty((n, kpad_for(2 * d)), dtype=torch.float32, device=device)
        T = torch.empty_like(E)
        r = torch.empty(n, dtype=torch.float32, device=device)
        tables.pca = torch.empty(2 * G, dtype=torch.int32, device=device)
        grp_dim, grp_info = tables.pca[:G], tables.pca[G:]
        for lo, hi, t in pca_plda_groups(Y, tables, plda, target_energy, grp_dim, grp_info, pca_max_bytes):
            mx = int(tables.sizes[lo:hi].max())
            for side, out, rr in ((hiplib.SIDE_ENROL, E, r), (hiplib.SIDE_TEST, T, None)):
                hiplib.backend_prepare_groups(Y, tables.row0_d[lo:hi + 1], mx, d, grp_dim[lo:hi], t["psi"], t["map"], t["off"], side, out,
                                              rr, tables.status)
        if keep_plain:
            tables.plain = Y
    else:
        E, r, T = _self_operands(x, plda, mean, transform, device)
        if keep_plain:
            tables.plain, _ = prepare(x, hiplib.SIDE_PLAIN, None, mean, transform, None, ln, device)
    scores = torch.empty(tables.scores_elems, dtype=torch.float32, device=device)
    hiplib.score_blocks(E, T, r, tables.row0_d, tables.score0_d, tables.max_n, scores, tables.status)
    return scores, tables


def ahc_batch(scores, tables, thresholds, min_clusters, max_bytes=AHC_MAX_BYTES, max_batch_n=hiplib.AHC_BATCH_MAX_N):
    """Average-linkage clustering of every group's block of the packed ``scores`` (what ``score_blocks`` returns), one workgroup
    per group (xv_ahc_average_batch_f64).  thresholds float [G] and min_clusters int [G] are each group's stop rule, as in
    ``ahc``.  The group list is cut into calls whose workspaces fit max_bytes; a group above max_batch_n goes through ``ahc`` on
    its block (identical results by the kernels' contract).  Put large groups first (``diarize`` does): workgroups start in group
    order.  One download at the end: results, the kernels' status word, the finite check of the upper triangles and, when the
    scores came from a per-group PCA, tables.pca, whose host copy lands in tables.pca_host.
    -> (labels, merges): per group, in the given order, labels int32[n_g] (the local slot of each item's cluster) and
    (a int32[M], b int32[M], score float64[M])."""
    import torch
    hiplib.require_gpu()
    G = tables.sizes.size
    thr = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    minc = np.asarray(min_clusters, dtype=np.int64).reshape(-1)
    if thr.size != G or minc.size != G:
        raise ValueError("ahc_batch: %d groups, %d thresholds, %d min_clusters" % (G, thr.size, minc.size))
    if np.isnan(thr).any():
        raise ValueError("ahc_batch: a threshold is NaN")
    if (minc < 1).any() or (minc > tables.sizes).any():
        raise ValueError("ahc_batch: min_clusters must be in 1..n for every group")
    if not (isinstance(scores, torch.Tensor) and scores.is_cuda and scores.dim() == 1 and scores.dtype == torch.float32 and
            scores.numel() >= tables.scores_elems):
        raise ValueError("ahc_batch: scores must be the packed float32 device blocks of the tables")
    calls, routed = plan_ahc_batch(tables.sizes, max_bytes, max_batch_n)
    dev = scores.device
    n_rows = tables.n_rows
    with torch.cuda.device(dev):
        nonfinite = _nonfinite_upper(scores, tables)
        # a, b, labels, n_merges in one int32 buffer: one download
        ints = torch.empty(3 * n_rows + G, dtype=torch.int32, device=dev)
        m_a, m_b, lab, cnt = ints[:n_rows], ints[n_rows:2 * n_rows], ints[2 * n_rows:3 * n_rows], ints[3 * n_rows:]
        m_s = torch.empty(n_rows, dtype=torch.float64, device=dev)
        if calls:
            ws = torch.empty(max(c[3] for c in calls), dtype=torch.uint8, device=dev)
            ws0 = torch.as_tensor(np.concatenate([c[2] for c in calls]), device=dev)
            thr_d = torch.as_tensor(thr, device=dev)
            minc_d = torch.as_tensor(minc.astype(np.int32), device=dev)
            at = 0
            for lo, hi, _, _ in calls:
                hiplib.ahc_average_batch(scores, tables.row0_d[lo:hi + 1], tables.score0_d[lo:hi], ws0[at:at + hi - lo], thr_d[lo:hi],
                                         minc_d[lo:hi], int(tables.sizes[lo:hi].max()), m_a, m_b, m_s, cnt[lo:hi], lab, tables.status,
                                         ws)
                at += hi - lo
        flags = torch.cat([tables.status.to(torch.int32), nonfinite.to(torch.int32).reshape(1)] +
                          ([] if tables.pca is None else [tables.pca.to(torch.int32).reshape(-1)]))
        ints_h, m_s_h, flags_h = ints.cpu().numpy(), m_s.cpu().numpy(), flags.cpu().numpy()
    if flags_h[1]:
        raise ValueError("ahc_batch: the upper triangle of a group's score matrix holds a value that is not finite")
    if flags_h[0]:
        raise hiplib.XvectorHipError("ahc_batch: a kernel skipped a group that broke its contract (status %d)" % flags_h[0])
    if tables.pca is not None:
        tables.pca_host = flags_h[2:].copy()
    labels, merges = [None] * G, [None] * G
    for g in routed:
        labels[g], merges[g] = ahc(tables.block(scores, g), float(thr[g]), int(minc[g]), max_bytes)
    a_h, b_h, lab_h, cnt_h = ints_h[:n_rows], ints_h[n_rows:2 * n_rows], ints_h[2 * n_rows:3 * n_rows], ints_h[3 * n_rows:]
    for g in range(G):
        if labels[g] is None:
            r0, r1, m = int(tables.row0[g]), int(tables.row0[g + 1]), int(cnt_h[g])
            labels[g] = lab_h[r0:r1].copy()
            merges[g] = (a_h[r0:r0 + m].copy(), b_h[r0:r0 + m].copy(), m_s_h[r0:r0 + m].copy())
    return labels, merges


def diarize(x, group_sizes, plda, mean=None, transform=None, threshold=0.0, num_spk=None, device="cuda:0", target_energy=1.0,
            pca_report=None, vbx=None, vbx_report=None):
    """Cluster every recording's vectors on their own: x[N, D] raw vectors, recording g the next group_sizes[g] rows.  The
    recordings are sorted by size, descending, for the device, scored against themselves in one launch (``score_blocks``) and
    clustered one workgroup each (``ahc_batch``); the results come back in the caller's order.  threshold: the stop rule of every
    recording; num_spk (None, or one entry per recording, None or a count): a recording with a count stops at exactly
    min(count, n_g) clusters instead.  -> (labels int32[N]: the local slot of each vector's cluster within its recording,
    merges: per recording (a, b, score)).

    target_energy below 1: every recording is scored under its own PCA and projected PLDA (``score_blocks``); the default, 1.0,
    is the route without a PCA, unchanged.  pca_report (a dict, optional) then receives 'dim' and 'info', int32 [G] in the
    caller's order: each recording's retained dimension and 0 / 1 / 2 (PCA applied / fallback for energy / for non-convergence);
    they come down with ``ahc_batch``'s download.

    vbx (None: the route above, unchanged): a dict turns on VBx resegmentation (``vbx_groups``) after the clustering -- the scalars
    of ``check_vbx_params`` (absent ones take VBX_DEFAULTS), and optionally 'time_order' (int [N], in the caller's row order: entry
    row0[g] + t is the index, local to recording g, of its t-th vector in time; absent: the rows are in time order), 'keep' (bool
    [G]: these recordings keep their clustering, e.g. those with a speaker count) and 'max_bytes'.  The PLAIN-prepared rows already
    on the device are read again (under the GLOBAL PLDA, also when the clustering ran under a per-recording PCA), the clustering's
    labels, renamed to 0 .. S - 1 per recording, are the initial labels, and a recording's labels become VBx's.  A recording with
    more than hiplib.VBX_MAX_SPK clusters keeps its clustering, and so does one VBx reports info 2 for.  vbx_report (a dict,
    optional) receives, per recording in the caller's order, 'ran' (bool), 'iters', 'info' (int32; 0 where VBx did not run),
    'spk_before' and 'spk_after' (int32)."""
    hiplib.require_gpu()
    target_energy = check_target_energy(target_energy)
    sizes = np.asarray(group_sizes, dtype=np.int64).reshape(-1)
    thr, minc = diarize_stop_rules(sizes, threshold, num_spk)
    if vbx is not None:
        vbx = dict(vbx)
        vbx_order, vbx_keep, vbx_bytes = vbx.pop("time_order", None), vbx.pop("keep", None), vbx.pop("max_bytes", VBX_MAX_BYTES)
        vbx = check_vbx_params(**vbx)
        if plda.dim > hiplib.PCA_MAX_DIM:
            raise ValueError("diarize: VBx handles dimensions up to %d, the PLDA has %d" % (hiplib.PCA_MAX_DIM, plda.dim))
    x = np.asarray(x, dtype=np.float32)
    if sizes.size < 1 or int(sizes.min()) < 1 or x.ndim != 2 or int(sizes.sum()) != x.shape[0]:
        raise ValueError("diarize: x must be [N, D] and the group sizes, all at least 1, must add up to N")
    G, N = sizes.size, x.shape[0]
    order, _ = size_order(sizes)
    row0 = np.concatenate([[0], np.cumsum(sizes)])
    rows = np.concatenate([np.arange(row0[g], row0[g + 1]) for g in order])
    if vbx is not None:
        vbx_keep = np.zeros(G, bool) if vbx_keep is None else np.asarray(vbx_keep, dtype=bool).reshape(-1)
        if vbx_keep.size != G:
            raise ValueError("diarize: %d recordings, %d entries of vbx['keep']" % (G, vbx_keep.size))
        if vbx_order is not None:
            vbx_order = np.asarray(vbx_order, dtype=np.int64).reshape(-1)
            if vbx_order.size != N:
                raise ValueError("diarize: %d vectors, %d entries of vbx['time_order']" % (N, vbx_order.size))
            vbx_order = vbx_order[rows]
    # from here to the last lines everything is in the device's order
    scores, tables = score_blocks(x[rows], sizes[order], plda, mean, transform, device, target_energy, keep_plain=vbx is not None)
    lab_sorted, merges_sorted = ahc_batch(scores, tables, thr[order], minc[order])
    if pca_report is not None and tables.pca_host is not None:
        _to_callers_order(pca_report, dict(dim=tables.pca_host[:G], info=tables.pca_host[G:]), order)
    if vbx is not None:
        lab_sorted, rep = _diarize_vbx(tables, lab_sorted, plda, vbx, vbx_order, vbx_keep[order], vbx_bytes)
        if vbx_report is not None:
            _to_callers_order(vbx_report, rep, order)
    labels = np.empty(N, dtype=np.int32)
    labels[rows] = np.concatenate(lab_sorted)
    merges = [None] * G
    for k, g in enumerate(order.tolist()):
        merges[g] = merges_sorted[k]
    return labels, merges


def _to_callers_order(report, sorted_arrays, order):
    """report[name] = each per-recording array of sorted_arrays (in the device's order ``order``) in the caller's order."""
    for name, v in sorted_arrays.items():
        report[name] = np.empty_like(v)
        report[name][order] = v


def _diarize_vbx(tables, lab_sorted, plda, params, time_order, keep, max_bytes):
    """The VBx stage of ``diarize``, all of it in the device's order (that of ``tables``): lab_sorted, the clustering's labels per
    recording; time_order int [N] or None and keep bool [G] as ``diarize`` takes them, permuted.  -> (the labels, those of every
    recording that VBx ran on replaced by VBx's; the report arrays of ``diarize``'s vbx_report)."""
    import torch
    G = tables.sizes.size
    compact = [compact_labels(l) for l in lab_sorted]
    before = np.asarray([c[1] for c in compact], dtype=np.int32)
    run = np.flatnonzero(~keep & (before <= hiplib.VBX_MAX_SPK))
    rep = dict(ran=np.zeros(G, bool), iters=np.zeros(G, np.int32), info=np.zeros(G, np.int32), spk_before=before,
               spk_after=before.copy())
    out = list(lab_sorted)
    if run.size:
        Y, sub = tables.plain, tables
        if run.size < G:                                         # the rows of the recordings that run, gathered on the device
            sub = GroupTables(tables.sizes[run], Y.device)
            idx = np.concatenate([np.arange(tables.row0[k], tables.row0[k + 1]) for k in run])
            Y = Y.index_select(0, torch.as_tensor(idx, device=Y.device))
            time_order = None if time_order is None else time_order[idx]
        init = np.concatenate([compact[k][0] for k in run])
        res = vbx_groups(Y, sub, init, plda, time_order, before[run], max_bytes=max_bytes, **params)
        for j, k in enumerate(run.tolist()):
            rep["ran"][k], rep["iters"][k], rep["info"][k] = True, res["iters"][j], res["info"][j]
            if res["info"][j] == 0:
                out[k] = res["labels"][sub.row0[j]:sub.row0[j + 1]].copy()
                rep["spk_after"][k] = np.unique(out[k]).size
    return out, rep


def diarize_stop_rules(sizes, threshold=0.0, num_spk=None):
    """(thresholds float64 [G], min_clusters int64 [G]) of ``diarize``: the common threshold and 1, or for a recording with a
    speaker count -inf and min(count, n_g)."""
    sizes = np.asarray(sizes, dtype=np.int64)
    threshold = float(threshold)
    if np.isnan(threshold):
        raise ValueError("diarize: the threshold is NaN")
    thr = np.full(sizes.size, threshold)
    minc = np.ones(sizes.size, dtype=np.int64)
    if num_spk is not None:
        if len(num_spk) != sizes.size:
            raise ValueError("diarize: %d recordings, %d speaker counts" % (sizes.size, len(num_spk)))
        for g, k in enumerate(num_spk):
            if k is not None:
                if int(k) < 1:
                    raise ValueError("diarize: a speaker count must be at least 1, got %r" % (k,))
                thr[g] = -np.inf
                minc[g] = min(int(k), int(sizes[g]))
    return thr, minc


# ---- VBx resegmentation of every recording's vectors (the rule: include/xvector_hip.h) ----
VBX_MAX_BYTES = 1 << 30            # the workspace of one xv_vbx_groups_f64 call is at most this large
VBX_DEFAULTS = dict(fa=0.3, fb=17.0, loop_prob=0.99, init_smoothing=5.0, max_iters=40, epsilon=1e-6)


def check_vbx_params(fa=0.3, fb=17.0, loop_prob=0.99, init_smoothing=5.0, max_iters=40, epsilon=1e-6):
    """The VBx scalars as a dict of floats (max_iters an int); ValueError for one outside the range xv_vbx_groups_f64 takes."""
    fa, fb, loop_prob, init_smoothing, epsilon = (float(v) for v in (fa, fb, loop_prob, init_smoothing, epsilon))
    if not (np.isfinite(fa) and fa > 0.0):
        raise ValueError("vbx: fa must be finite and > 0, got %r" % fa)
    if not (np.isfinite(fb) and fb > 0.0):
        raise ValueError("vbx: fb must be finite and > 0, got %r" % fb)
    if not 0.0 <= loop_prob < 1.0:
        raise ValueError("vbx: loop_prob must be in [0, 1), got %r" % loop_prob)
    if not (np.isfinite(init_smoothing) and init_smoothing >= 0.0):
        raise ValueError("vbx: init_smoothing must be finite and >= 0, got %r" % init_smoothing)
    if int(max_iters) != max_iters or not 1 <= int(max_iters) <= hiplib.VBX_MAX_ITERS:
        raise ValueError("vbx: max_iters must be an integer in [1, %d], got %r" % (hiplib.VBX_MAX_ITERS, max_iters))
    if np.isnan(epsilon):
        raise ValueError("vbx: epsilon is NaN")
    return dict(fa=fa, fb=fb, loop_prob=loop_prob, init_smoothing=init_smoothing, max_iters=int(max_iters), epsilon=epsilon)


def compact_labels(labels):
    """(labels renamed to 0 .. S - 1 in ascending order of the old names, int32; S)."""
    names, inv = np.unique(np.asarray(labels), return_inverse=True)
    return inv.astype(np.int32).reshape(-1), int(names.size)


def vbx_host(y, init_labels, plda, n_spk=None, fa=0.3, fb=17.0, loop_prob=0.99, init_smoothing=5.0, max_iters=40, epsilon=1e-6):
    """The host float64 twin of xv_vbx_groups_f64 on ONE recording, in the kernel's linear form (the rule of
    include/xvector_hip.h, step for step; it stands beside ``est_pca`` / ``host_pca_tables``): y[T, >= d] the recording's rows in
    time order, after mean subtraction, LDA and length normalisation; init_labels[T] in [0, S); n_spk = S (None: the largest
    label + 1).  The forward and backward chains pay 2 T interpreter steps an iteration.
    -> dict(gamma [T, S], pi [S], elbo [n_iters], iters, info (0, or 2: labels are the initial ones), labels int32 [T])."""
    p = check_vbx_params(fa, fb, loop_prob, init_smoothing, max_iters, epsilon)
    fa, fb, lp, eps = p["fa"], p["fb"], p["loop_prob"], p["epsilon"]
    d = plda.dim
    y = np.asarray(y, dtype=np.float64)
    lab = np.asarray(init_labels, dtype=np.int64).reshape(-1)
    if y.ndim != 2 or y.shape[0] < 1 or y.shape[1] < d or lab.size != y.shape[0]:
        raise ValueError("vbx_host: y must be [T, >= %d] with T >= 1 and one initial label per row" % d)
    T = y.shape[0]
    S = int(lab.max()) + 1 if n_spk is None else int(n_spk)
    if not 1 <= S <= hiplib.VBX_MAX_SPK or int(lab.min()) < 0 or int(lab.max()) >= S:
        raise ValueError("vbx_host: 1 <= S <= %d and every initial label in [0, S)" % hiplib.VBX_MAX_SPK)
    phi = plda.psi
    with np.errstate(all="ignore"):
        z = (y[:, :d] - plda.mean) @ plda.transform.T
        rho = z * np.sqrt(phi)
        G = -0.5 * ((z * z).sum(axis=1) + d * np.log(2.0 * np.pi))
        es = np.exp(p["init_smoothing"])
        gamma = np.full((T, S), 1.0 / (es + S - 1))
        gamma[np.arange(T), lab] = es / (es + S - 1)
        pi = np.full(S, 1.0 / S)
        ratio = fa / fb
        elbo, info = [], 0
        a, beta, c = np.empty((T, S)), np.empty((T, S)), np.empty(T)
        for it in range(p["max_iters"]):
            N = gamma.sum(axis=0)
            invL = 1.0 / (1.0 + ratio * N[:, None] * phi[None, :])
            alpha = ratio * invL * (gamma.T @ rho)
            ll = fa * (rho @ alpha.T - 0.5 * ((invL + alpha * alpha) @ phi)[None, :] + G[:, None])
            m = ll.max(axis=1)
            b = np.exp(ll - m[:, None])
            v = pi * b[0]
            for t in range(T):
                if t:
                    v = (lp * a[t - 1] + (1.0 - lp) * pi) * b[t]
                c[t] = v.sum()
                a[t] = v / c[t]
            beta[T - 1] = 1.0
            for t in range(T - 2, -1, -1):
                w = b[t + 1] * beta[t + 1]
                beta[t] = (lp * w + (1.0 - lp) * (pi * w).sum()) / c[t + 1]
            gamma = a * beta
            e = (np.log(c) + m).sum() + 0.5 * fb * (np.log(invL) - invL - alpha * alpha + 1.0).sum()
            pn = gamma[0] + (1.0 - lp) * pi * (b[1:] * beta[1:] / c[1:, None]).sum(axis=0)
            norm = pn.sum()
            if not (np.all(np.isfinite(c)) and np.all(c != 0.0) and np.isfinite(e) and np.isfinite(norm) and norm != 0.0):
                info = 2
                break
            pi = pn / norm
            elbo.append(e)
            if it > 0 and elbo[-1] - elbo[-2] < eps:
                break
    labels = lab.astype(np.int32) if info else np.argmax(gamma, axis=1).astype(np.int32)
    return dict(gamma=gamma, pi=pi, elbo=np.asarray(elbo), iters=len(elbo) + (1 if info else 0), info=info, labels=labels)


def plan_vbx_groups(row0, dim, max_spk, max_bytes=VBX_MAX_BYTES):
    """Cut the groups of the prefix table row0 [G + 1] into calls of xv_vbx_groups_f64, runs of consecutive groups whose workspace
    fits max_bytes: -> [(g_lo, g_hi)].  One group alone above max_bytes is an error."""
    row0 = np.asarray(row0, dtype=np.int64)
    try:
        return _cut_runs(0, row0.size - 1,
                         lambda a, b: hiplib.vbx_groups_workspace_bytes(int(row0[b] - row0[a]), b - a, dim, max_spk) <= max_bytes)
    except ValueError as e:
        g = e.args[0]
        raise ValueError("vbx_groups: a group of %d rows needs a workspace of more than max_bytes = %d" %
                         (int(row0[g + 1] - row0[g]), max_bytes))


def vbx_groups(y_rows, tables, init_labels, plda, time_order=None, n_spk=None, fa=0.3, fb=17.0, loop_prob=0.99, init_smoothing=5.0,
               max_iters=40, epsilon=1e-6, max_bytes=VBX_MAX_BYTES, keep_gamma=False):
    """VBx resegmentation of every group on the device (xv_vbx_groups_f64).  y_rows: float32 device rows [N, >= d], the vectors
    after mean subtraction, LDA and length normalisation (``prepare(..., SIDE_PLAIN, plda=None)``); tables: their GroupTables;
    init_labels: int [N], per row, in [0, S_g); n_spk: int [G] (None: every group's largest label + 1), each at most
    hiplib.VBX_MAX_SPK; time_order: int [N] or None -- entry row0[g] + t is the index, local to group g, of its t-th vector in
    time (None: the rows are in time order).  The fp64 model is uploaded once, the group list is cut into calls whose workspace
    fits max_bytes (``plan_vbx_groups``), and everything comes down in one download at the end.
    -> dict(labels int32 [N] (per row, a slot of the initial labelling), iters, info int32 [G], n_spk int32 [G],
    pi float64 [G, max S], elbo float64 [G, max_iters] (NaN past iters), gamma float64 [N, max S] if keep_gamma)."""
    import torch
    hiplib.require_gpu()
    p = check_vbx_params(fa, fb, loop_prob, init_smoothing, max_iters, epsilon)
    d, G, N = plda.dim, tables.sizes.size, tables.n_rows
    if d > hiplib.PCA_MAX_DIM:
        raise ValueError("vbx_groups: dimension %d exceeds %d, the limit of xv_vbx_groups_f64" % (d, hiplib.PCA_MAX_DIM))
    lab = np.ascontiguousarray(init_labels, dtype=np.int32).reshape(-1)
    if lab.size != N or y_rows.shape[0] != N:
        raise ValueError("vbx_groups: %d rows in the tables, %d on the device, %d initial labels" % (N, y_rows.shape[0], lab.size))
    if n_spk is None:
        n_spk = np.maximum.reduceat(lab, tables.row0[:-1].astype(np.int64)) + 1
    spk = np.ascontiguousarray(n_spk, dtype=np.int32).reshape(-1)
    if spk.size != G or int(spk.min()) < 1 or int(spk.max()) > hiplib.VBX_MAX_SPK:
        raise ValueError("vbx_groups: one speaker count per group, each in [1, %d]" % hiplib.VBX_MAX_SPK)
    order = None
    if time_order is not None:
        order = np.ascontiguousarray(time_order, dtype=np.int32).reshape(-1)
        if order.size != N:
            raise ValueError("vbx_groups: %d rows, %d entries of the time order" % (N, order.size))
    ms, mi = int(spk.max()), p["max_iters"]
    calls = plan_vbx_groups(tables.row0, d, ms, max_bytes)
    dev = y_rows.device
    with torch.cuda.device(dev):
        model = [torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev) for a in (plda.mean, plda.transform, plda.psi)]
        ints_in = torch.as_tensor(np.concatenate([lab, spk] + ([] if order is None else [order])), device=dev)
        lab_d, spk_d = ints_in[:N], ints_in[N:N + G]
        order_d = None if order is None else ints_in[N + G:]
        # every result in one buffer, the float64 part first: one download
        n_f64 = G * ms + G * mi + (N * ms if keep_gamma else 0)
        out = torch.empty(8 * n_f64 + 4 * (N + 2 * G + 1), dtype=torch.uint8, device=dev)
        f64 = out[:8 * n_f64].view(torch.float64)
        i32 = out[8 * n_f64:].view(torch.int32)
        pi_d, elbo_d = f64[:G * ms].view(G, ms), f64[G * ms:G * (ms + mi)].view(G, mi)
        gamma_d = f64[G * (ms + mi):].view(N, ms) if keep_gamma else None
        labels_d, iters_d, info_d, status_d = i32[:N], i32[N:N + G], i32[N + G:N + 2 * G], i32[N + 2 * G:]
        f64.fill_(float("nan"))
        i32.zero_()
        ws = torch.empty(max(hiplib.vbx_groups_workspace_bytes(int(tables.row0[hi] - tables.row0[lo]), hi - lo, d, ms)
                             for lo, hi in calls), dtype=torch.uint8, device=dev)
        for lo, hi in calls:
            r0, r1 = int(tables.row0[lo]), int(tables.row0[hi])
            row0_d = tables.row0_d[lo:hi + 1] if r0 == 0 else tables.row0_d[lo:hi + 1] - r0
            hiplib.vbx_groups(y_rows[r0:r1], row0_d, d, None if order_d is None else order_d[r0:r1], lab_d[r0:r1], spk_d[lo:hi], ms,
                              *model, p["fa"], p["fb"], p["loop_prob"], p["init_smoothing"], mi, p["epsilon"], labels_d[r0:r1],
                              None if gamma_d is None else gamma_d[r0:r1], pi_d[lo:hi], elbo_d[lo:hi], iters_d[lo:hi], info_d[lo:hi],
                              status_d, ws)
        out_h = out.cpu().numpy()
    f64_h, i32_h = out_h[:8 * n_f64].view(np.float64), out_h[8 * n_f64:].view(np.int32)
    if i32_h[N + 2 * G]:
        raise hiplib.XvectorHipError("vbx_groups: the kernel skipped a group that broke its contract (status %d)" % i32_h[N + 2 * G])
    res = dict(labels=i32_h[:N].copy(), iters=i32_h[N:N + G].copy(), info=i32_h[N + G:N + 2 * G].copy(), n_spk=spk.copy(),
               pi=f64_h[:G * ms].reshape(G, ms).copy(), elbo=f64_h[G * ms:G * (ms + mi)].reshape(G, mi).copy())
    if keep_gamma:
        res["gamma"] = f64_h[G * (ms + mi):].reshape(N, ms).copy()
    return res


DENSE_MAX_BYTES = 1 << 30          # the dense score matrix of one trial list is at most this large


class CohortStatsError(ValueError):
    """A cohort score standard deviation that AS-norm would divide by is 0 or not finite.  side: 'enrol' | 'test'; row: the
    row of that side's vectors."""

    def __init__(self, side, row, std):
        ValueError.__init__(self, "AS-norm: the cohort scores of %s row %d have standard deviation %r (0 or not finite)" %
                            ("enrolment" if side == "enrol" else "test", row, std))
        self.side, self.row, self.std = side, row, std


class Scorer(object):
    """Prepared enrolment and test operands on the device.  scoring 'plda' (needs plda) or 'cosine'.  enrol[Ne, D] are speaker
    means of the raw vectors (num_utts[Ne] their utterance counts), test[Nt, D] raw vectors; mean / transform run the stage-9
    chain on the device first (None: the vectors are used as they are, e.g. already processed by Kaldi pipes).

    cohort[Nc, D] (raw vectors, the same chain as the test vectors) enables AS-norm with the top
    min(cohort_top_n, Nc) cohort scores of each side.  The cohort is prepared as test rows; for the test-side statistics the test
    vectors are prepared a second time as one-utterance enrolment rows (cosine: both sides are the cosine rows)."""

    def __init__(self, enrol, test, plda=None, num_utts=None, mean=None, transform=None, scoring="plda", device="cuda:0",
                 cohort=None, cohort_top_n=300):
        hiplib.require_gpu()
        self.device = device
        ln = transform is not None
        if scoring == "plda":
            if plda is None:
                raise ValueError("PLDA scoring needs a Plda")
            self.E, self.r = prepare(enrol, hiplib.SIDE_ENROL, num_utts, mean, transform, plda, ln, device)
            self.T, _ = prepare(test, hiplib.SIDE_TEST, None, mean, transform, plda, ln, device)
        elif scoring == "cosine":
            self.E, _ = prepare(enrol, hiplib.SIDE_COSINE, num_utts, mean, transform, plda, ln, device)
            self.T, _ = prepare(test, hiplib.SIDE_COSINE, None, mean, transform, plda, ln, device)
            self.r = None
        else:
            raise ValueError("scoring must be 'plda' or 'cosine'")
        self.scoring = scoring
        self.C = None
        self.stats_seconds = 0.0
        if cohort is not None:
            if len(cohort) == 0:
                raise ValueError("the cohort is empty")
            if cohort_top_n < 2:
                raise ValueError("cohort_top_n must be at least 2 (the std of one score is 0), got %d" % cohort_top_n)
            self.cohort_top_n = min(int(cohort_top_n), len(cohort))
            if scoring == "plda":
                self.C, _ = prepare(cohort, hiplib.SIDE_TEST, None, mean, transform, plda, ln, device)
                self.TE, self.rT = prepare(test, hiplib.SIDE_ENROL, np.ones(len(test), np.int32), mean, transform, plda, ln, device)
            else:
                self.C, _ = prepare(cohort, hiplib.SIDE_COSINE, None, mean, transform, plda, ln, device)
                self.TE, self.rT = self.T, None

    @property
    def shape(self):
        return self.E.shape[0], self.T.shape[0]

    def score_matrix(self):
        """S[Ne, Nt] on the device."""
        import torch
        s = torch.empty(self.shape, dtype=torch.float32, device=self.device)
        hiplib.score_matrix(self.E, self.T, self.r, s)
        return s

    def score_pairs(self, e_idx, t_idx):
        """score[i] of trial (e_idx[i], t_idx[i]) on the device."""
        import torch
        e = torch.as_tensor(np.ascontiguousarray(e_idx, dtype=np.int32), device=self.device)
        t = torch.as_tensor(np.ascontiguousarray(t_idx, dtype=np.int32), device=self.device)
        out = torch.empty(e.numel(), dtype=torch.float32, device=self.device)
        hiplib.score_pairs(self.E, self.T, self.r, e, t, out)
        return out

    def use_dense(self, n_trials):
        """Dense-then-gather when the list covers at least 1/8 of the matrix and the matrix fits DENSE_MAX_BYTES."""
        ne, nt = self.shape
        return ne * nt * 4 <= DENSE_MAX_BYTES and 8 * n_trials >= ne * nt

    def _raw_scores(self, e_idx, t_idx):
        """score[i] of the trial list on the device: the same bits whichever scorer runs."""
        if self.use_dense(e_idx.size):
            import torch
            s = self.score_matrix()
            flat = torch.as_tensor(e_idx * self.shape[1] + t_idx, device=self.device)
            return s.reshape(-1)[flat]
        return self.score_pairs(e_idx, t_idx)

    def cohort_stats(self, side, idx, chunk_rows=None, max_bytes=DENSE_MAX_BYTES):
        """(mu, sigma) on the device: mean and population std of the top cohort_top_n cohort scores of the rows idx of side
        'enrol' (the enrolment operands) or 'test' (the test vectors as one-utterance enrolments).  Rows go in chunks of at most
        chunk_rows (None: no limit) whose cohort score matrix fits max_bytes; a row's result does not depend on the chunking."""
        import torch
        if self.C is None:
            raise ValueError("cohort_stats needs a Scorer built with a cohort")
        if side == "enrol":
            ops, r = self.E, self.r
        elif side == "test":
            ops, r = self.TE, self.rT
        else:
            raise ValueError("side must be 'enrol' or 'test'")
        idx = torch.as_tensor(np.ascontiguousarray(idx, dtype=np.int64), device=self.device)
        n, nc = idx.numel(), self.C.shape[0]
        ldc = (nc + 3) // 4 * 4                                  # xv_topk_row_stats_f32 wants ld % 4 == 0
        rows = max_bytes // (ldc * 4)
        if chunk_rows is not None:
            rows = min(rows, int(chunk_rows))
        if rows < 1:
            raise ValueError("max_bytes %d holds no row of %d cohort scores" % (max_bytes, nc))
        rows = min(rows, max(n, 1), 65535 * 128)               # xv_score_matrix_f32 takes at most 65535 x 128 rows a launch
        mu = torch.empty(n, dtype=torch.float32, device=self.device)
        sd = torch.empty(n, dtype=torch.float32, device=self.device)
        ws = torch.empty((rows, ldc), dtype=torch.float32, device=self.device)
        for i0 in range(0, n, rows):
            sel = idx[i0:i0 + rows]
            m = sel.numel()
            hiplib.score_matrix(ops.index_select(0, sel), self.C, None if r is None else r.index_select(0, sel), ws[:m])
            hiplib.topk_row_stats(ws[:m, :nc], self.cohort_top_n, mu[i0:i0 + m], sd[i0:i0 + m])
        return mu, sd

    def score_trials(self, e_idx, t_idx, norm="none"):
        """score[i] of the trial list as a float32 NumPy array: the same bits whichever scorer runs.  norm 'asnorm' (needs a
        cohort): s' = 1/2 ((s - mu_e) / sigma_e + (s - mu_t) / sigma_t) in fp32 on the device, with the statistics of the
        enrolment and test rows the list references; CohortStatsError if one of their sigma is 0 or not finite."""
        e_idx = np.asarray(e_idx, dtype=np.int64)
        t_idx = np.asarray(t_idx, dtype=np.int64)
        if norm not in ("none", "asnorm"):
            raise ValueError("norm must be 'none' or 'asnorm'")
        if norm == "asnorm" and self.C is None:
            raise ValueError("AS-norm needs a Scorer built with a cohort")
        if e_idx.size == 0:
            return np.zeros(0, np.float32)
        s = self._raw_scores(e_idx, t_idx)
        if norm == "none":
            return s.cpu().numpy()
        import time
        import torch
        t0 = time.perf_counter()
        stats = []
        for side, ix, n in (("enrol", e_idx, self.shape[0]), ("test", t_idx, self.shape[1])):
            used = np.zeros(n, bool)                             # the rows the list references, without sorting the list
            used[ix] = True
            rows = np.flatnonzero(used)
            pos = (np.cumsum(used) - 1)[ix]
            mu, sd = self.cohort_stats(side, rows)
            bad = ~(torch.isfinite(sd) & (sd > 0))
            if bool(bad.any()):
                j = int(torch.nonzero(bad)[0, 0])
                raise CohortStatsError(side, int(rows[j]), float(sd[j]))
            p = torch.as_tensor(pos, device=self.device)
            stats.append((mu[p], sd[p]))
        torch.cuda.synchronize(self.device)
        self.stats_seconds = time.perf_counter() - t0
        (mu_e, sd_e), (mu_t, sd_t) = stats
        return (((s - mu_e) / sd_e + (s - mu_t) / sd_t) * 0.5).cpu().numpy()


# ------------------------------------------------------------------------------------------------
# EER (compute-eer)
# ------------------------------------------------------------------------------------------------
def eer(target_scores, nontarget_scores):
    """Kaldi compute-eer: -> (eer as a fraction, threshold).  Walk the sorted target scores upward until the nontarget score at
    the mirrored rank falls below the target score."""
    tgt = np.sort(np.asarray(target_scores, dtype=np.float32))
    non = np.sort(np.asarray(nontarget_scores, dtype=np.float32))
    if tgt.size == 0 or non.size == 0:
        raise ValueError("compute-eer needs target and nontarget scores")
    nt, nn = tgt.size, non.size
    pos = np.arange(nt - 1, dtype=np.int64)
    npos = np.maximum(nn - 1 - (nn * pos * 1.0 / nt).astype(np.int64), 0)
    stop = np.flatnonzero(non[npos] < tgt[pos])
    pos = int(stop[0]) if stop.size else nt - 1
    return pos * 1.0 / nt, float(tgt[pos])
