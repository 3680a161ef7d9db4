"""Timings of clustering-based PLDA adaptation on a planted-speaker set: the N x N PLDA score matrix (two
prepare calls + xv_score_matrix_f32) and its average-linkage clustering (xv_ahc_average_f64), each timed on its own with device
events after a warm-up; beside them the host route on the same machine: download the matrix, build the condensed distances,
scipy.cluster.hierarchy.linkage(method="average") (where scipy is missing: tests/ahc_ref.py at the sizes it can finish).
The kernel is timed twice: at threshold 0 (what `plda_backend.py cluster` runs; it stops at about the planted speakers) and down
to one cluster (the full dendrogram, which is what linkage computes).  At the smallest size the kernel's merges are compared
with the host's.      python tools/cluster_bench.py [--no-host] [N ...]      (default N = 2048 8192 16384; --no-host: the device
side alone, for sizes whose condensed distances the host has no room for)"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "x-vector-kaldi-tf_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

DIM, UTTS = 64, 8          # vector dimension (no LDA: the planted model is already diagonal), utterances per planted speaker


def planted(n, seed=0):
    """n vectors of n / UTTS speakers under a diagonal two-covariance model, shuffled; -> (x float32 [n, DIM], labels, Plda)."""
    from xvector_amd import backend
    rng = np.random.default_rng(seed)
    psi = np.sort(rng.uniform(2.0, 12.0, DIM))[::-1]
    spk = np.repeat(np.arange((n + UTTS - 1) // UTTS), UTTS)[:n]
    x = (rng.standard_normal((spk.max() + 1, DIM)) * np.sqrt(psi))[spk] + rng.standard_normal((n, DIM))
    perm = rng.permutation(n)
    return x[perm].astype(np.float32), spk[perm], backend.Plda(np.zeros(DIM), np.eye(DIM), psi)


def event_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b)


def main(sizes, host_route=True):
    import torch
    from xvector_amd import backend, hiplib
    hiplib.require_gpu()
    try:
        from scipy.cluster import hierarchy
    except ImportError:
        hierarchy = None
    x, _, plda = planted(512)
    backend.cluster_vectors(x, plda)                                     # warm-up: code objects, allocator
    print("| N | score matrix ms | ahc threshold 0: ms (merges, clusters, us / merge) | ahc full dendrogram: ms (us / merge) | "
          "download ms | condensed ms | host linkage ms | planted partition |")
    print("|---|---|---|---|---|---|---|---|")
    for n in sizes:
        x, spk, plda = planted(n)
        box = {}
        t_score = min(event_ms(lambda: box.update(s=backend.score_matrix_self(x, plda))) for _ in range(3))
        s = box["s"]
        ws = torch.empty(hiplib.ahc_average_workspace_bytes(n), dtype=torch.uint8, device=s.device)
        m_a = torch.empty(n, dtype=torch.int32, device=s.device); m_b = torch.empty_like(m_a)
        m_s = torch.empty(n, dtype=torch.float64, device=s.device)
        cnt = torch.empty(1, dtype=torch.int32, device=s.device); lab = torch.empty(n, dtype=torch.int32, device=s.device)
        run = lambda thr: hiplib.ahc_average(s[:, :n], thr, 1, m_a, m_b, m_s, cnt, lab, workspace=ws)
        t_full = min(event_ms(lambda: run(-np.inf)) for _ in range(2))
        full = (m_a[:n - 1].cpu().numpy(), m_b[:n - 1].cpu().numpy(), m_s[:n - 1].cpu().numpy())
        t_thr = min(event_ms(lambda: run(0.0)) for _ in range(2))
        merges = int(cnt.cpu()[0])
        labels = lab.cpu().numpy()
        pairs = lambda l: set(map(frozenset, [np.flatnonzero(l == v).tolist() for v in np.unique(l)]))
        planted_ok = pairs(labels) == pairs(spk)
        t0 = time.perf_counter()
        host = s[:, :n].cpu().numpy() if host_route else None
        t1 = time.perf_counter()
        if not host_route:
            t2 = t3 = t1
            host_name, host_heights = "not run", None
        elif hierarchy is not None:
            C = float(host.max()) + 1.0
            cond = C - host[np.triu_indices(n, 1)].astype(np.float64)
            t2 = time.perf_counter()
            Z = hierarchy.linkage(cond, method="average")
            t3 = time.perf_counter()
            host_name, host_heights = "scipy", np.sort(C - Z[:, 2])[::-1]
        elif n <= 4096:
            import ahc_ref
            t2 = time.perf_counter()
            host_heights = np.sort(ahc_ref.dendrogram(host)[2])[::-1]
            t3 = time.perf_counter()
            host_name = "ahc_ref"
        else:
            t2 = t3 = time.perf_counter()
            host_name, host_heights = "not run", None
        if host_heights is not None and n == sizes[0]:
            # the same dendrogram: sorted merge heights against the host's (scipy breaks ties and sums in another order)
            err = np.abs(np.sort(full[2])[::-1] - host_heights).max()
            print("<!-- N = %d: max |merge height - %s| = %.3e -->" % (n, host_name, err))
        print("| %d | %.2f | %.1f (%d, %d, %.1f) | %.1f (%.1f) | %.1f | %.1f | %s %.1f | %s |" %
              (n, t_score, t_thr, merges, n - merges, 1e3 * t_thr / max(merges, 1), t_full, 1e3 * t_full / max(n - 1, 1),
               1e3 * (t1 - t0), 1e3 * (t2 - t1), host_name, 1e3 * (t3 - t2), "recovered" if planted_ok else "NOT recovered"))
        sys.stdout.flush()
        del s, ws, host


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--no-host"]
    main([int(a) for a in args] or [2048, 8192, 16384], host_route=len(args) == len(sys.argv) - 1)
