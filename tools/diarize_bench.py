"""Timings of diarization on planted speakers: G recordings of n sub-segments each, every recording from SPK
planted speakers, shuffled.  Without --loop: backend.diarize (every recording's score block from one launch, one workgroup per
recording's clustering), wall time and device-event time of the whole call after a warm-up, and beside them its two device stages
on their own (the two prepare calls + xv_score_blocks_f32; xv_ahc_average_batch_f64).  With --loop: the per-recording Python loop
around backend.cluster_vectors, the only route before the batch existed; it needs nothing newer than §8.9, so it also runs on an
older checkout.  Both report how many recordings came out as their planted partition.
With --target-energy F below 1: backend.diarize under every recording's own PCA and projected PLDA, the new
device stage on its own (xv_pca_plda_groups_f64, every call of backend.pca_plda_groups), its share of the diarize call, and the host
route beside it: backend.host_pca_tables (est_pca + Plda.apply_transform per recording in NumPy, one host thread) feeding the same
grouped prepare and scorer.  At the default, 1.0, the tool's figures come from the unchanged path.
    python tools/diarize_bench.py [--loop] [--reps R] [--dim D] [--target-energy F] [G:n ...]
                                                            (default shapes 256:200 2048:100, R = 3, D = 64, the best is printed)"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "x-vector-kaldi-tf_amd"))
import numpy as np

DIM, SPK = 64, 4           # vector dimension, --dim sets it (no LDA: the planted model is already diagonal), planted speakers per recording


def planted(G, n, seed=0):
    """G recordings of n vectors; -> (x float32 [G n, DIM], speaker of each vector within its recording [G, n], Plda)."""
    from xvector_amd import backend
    rng = np.random.default_rng(seed)
    psi = np.sort(rng.uniform(2.0, 12.0, DIM))[::-1]
    spk = np.stack([rng.permutation(np.arange(n) % SPK) for _ in range(G)])
    centres = rng.standard_normal((G, SPK, DIM)) * np.sqrt(psi)
    x = centres[np.arange(G)[:, None], spk] + rng.standard_normal((G, n, DIM))
    return x.reshape(G * n, DIM).astype(np.float32), spk, backend.Plda(np.zeros(DIM), np.eye(DIM), psi)


def same_partition(a, b):
    return len(set(zip(a.tolist(), b.tolist()))) == len(set(a.tolist())) == len(set(b.tolist()))


def timed(fn):
    """(wall ms, device-event ms, result) of fn()."""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record(); out = fn(); b.record(); torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), a.elapsed_time(b), out


def best(fn, reps):
    runs = [timed(fn) for _ in range(reps)]
    return min(r[0] for r in runs), min(r[1] for r in runs), runs[-1][2]


def pca_main(shapes, reps, target_energy):
    """The --target-energy route: the device stage against the host loop, both feeding the same grouped prepare and scorer."""
    import torch
    from xvector_amd import backend, hiplib
    x, _, plda = planted(4, 50)
    backend.diarize(x, [50] * 4, plda, target_energy=target_energy)          # warm-up: code objects, allocator
    print("| G | n | d | diarize: wall ms | device-event ms | PCA + projected PLDA kernel ms (share of diarize) | grouped prepare x 2 ms "
          "| host est_pca + apply_transform loop: wall ms (ms / recording) | host route to the score blocks: wall ms | device route "
          "to the score blocks: wall ms | mean retained dim | fallbacks | planted partitions |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for G, n in shapes:
        x, spk, plda = planted(G, n)
        d = plda.dim
        sizes = [n] * G
        report = {}
        wall, dev, (labels, _) = best(lambda: backend.diarize(x, sizes, plda, target_energy=target_energy, pca_report=report), reps)
        ok = sum(same_partition(labels[g * n:(g + 1) * n], spk[g]) for g in range(G))
        Y, _ = backend.prepare(x, hiplib.SIDE_PLAIN, None, None, None, None, False)
        tables = backend.GroupTables(sizes, Y.device)
        dims = torch.empty(2 * G, dtype=torch.int32, device=Y.device)

        def stage():
            for _ in backend.pca_plda_groups(Y, tables, plda, target_energy, dims[:G], dims[G:]):
                pass
        _, t_pca, _ = best(stage, reps)
        E = torch.empty((G * n, backend.kpad_for(2 * d)), dtype=torch.float32, device=Y.device)
        T = torch.empty_like(E)
        r = torch.empty(G * n, dtype=torch.float32, device=Y.device)
        scores = torch.empty(tables.scores_elems, dtype=torch.float32, device=Y.device)

        def score(tabs):
            for side, out, rr in ((hiplib.SIDE_ENROL, E, r), (hiplib.SIDE_TEST, T, None)):
                hiplib.backend_prepare_groups(Y, tables.row0_d, n, d, tabs[0], tabs[1], tabs[2], tabs[3], side, out, rr, tables.status)
            hiplib.score_blocks(E, T, r, tables.row0_d, tables.score0_d, n, scores, tables.status)

        host = {}

        def host_tables():
            host["t"] = backend.host_pca_tables(Y.cpu().numpy()[:, :d], sizes, plda, target_energy)
        t_host = min(timed(host_tables)[0] for _ in range(min(reps, 2)))

        def host_route():
            host_tables()
            h = host["t"]
            score([torch.as_tensor(h[k], device=Y.device) for k in ("dim", "psi", "map", "off")])
        w_host = min(timed(host_route)[0] for _ in range(min(reps, 2)))
        host_scores = scores.clone()
        htabs = [torch.as_tensor(host["t"][k], device=Y.device) for k in ("dim", "psi", "map", "off")]
        _, t_prep, _ = best(lambda: [hiplib.backend_prepare_groups(Y, tables.row0_d, n, d, *htabs, side, out, rr, tables.status)
                                     for side, out, rr in ((hiplib.SIDE_ENROL, E, r), (hiplib.SIDE_TEST, T, None))], reps)
        w_dev, _, (dscores, _) = best(lambda: backend.score_blocks(x, sizes, plda, target_energy=target_energy), reps)
        agree = float((dscores - host_scores).abs().max())
        print("| %d | %d | %d | %.1f | %.1f | %.2f (%.0f %%) | %.2f | %.0f (%.2f) | %.0f | %.1f | %.2f | %d energy, %d convergence | %d of %d |"
              % (G, n, d, wall, dev, t_pca, 100.0 * t_pca / dev, t_prep, t_host, t_host / G, w_host, w_dev, float(report["dim"].mean()),
                 int((report["info"] == 1).sum()), int((report["info"] == 2).sum()), ok, G))
        print("  (largest difference between the two routes' scores: %.3g)" % agree)
        sys.stdout.flush()


def main(shapes, loop, reps):
    import torch
    from xvector_amd import backend, hiplib
    hiplib.require_gpu()
    x, _, plda = planted(4, 50)
    if loop:
        backend.cluster_vectors(x[:50], plda)                               # warm-up: code objects, allocator
        print("| G | n | loop of cluster_vectors: wall ms | device-event ms | ms / recording | planted partitions |")
        print("|---|---|---|---|---|---|")
    else:
        backend.diarize(x, [50] * 4, plda)
        print("| G | n | diarize: wall ms | device-event ms | prepare + score blocks ms | batch clustering kernel ms "
              "(merges / recording, us / merge of one recording) | planted partitions |")
        print("|---|---|---|---|---|---|---|")
    for G, n in shapes:
        x, spk, plda = planted(G, n)
        if loop:
            def run():
                return [backend.cluster_vectors(x[g * n:(g + 1) * n], plda)[0] for g in range(G)]
            wall, dev, labels = best(run, reps)
            ok = sum(same_partition(labels[g], spk[g]) for g in range(G))
            print("| %d | %d | %.1f | %.1f | %.3f | %d of %d |" % (G, n, wall, dev, wall / G, ok, G))
        else:
            sizes = [n] * G
            wall, dev, (labels, merges) = best(lambda: backend.diarize(x, sizes, plda), reps)
            ok = sum(same_partition(labels[g * n:(g + 1) * n], spk[g]) for g in range(G))
            _, t_score, (scores, tables) = best(lambda: backend.score_blocks(x, sizes, plda), reps)
            need = hiplib.ahc_average_batch_workspace_bytes(n)
            ws = torch.empty(G * need, dtype=torch.uint8, device=scores.device)
            ws0 = torch.arange(G, device=scores.device, dtype=torch.int64) * need
            thr = torch.zeros(G, dtype=torch.float64, device=scores.device)
            minc = torch.ones(G, dtype=torch.int32, device=scores.device)
            m_a = torch.empty(G * n, dtype=torch.int32, device=scores.device); m_b = torch.empty_like(m_a); lab = torch.empty_like(m_a)
            m_s = torch.empty(G * n, dtype=torch.float64, device=scores.device)
            cnt = torch.empty(G, dtype=torch.int32, device=scores.device)
            _, t_ahc, _ = best(lambda: hiplib.ahc_average_batch(scores, tables.row0_d, tables.score0_d, ws0, thr, minc, n, m_a, m_b, m_s,
                                                                cnt, lab, tables.status, ws), reps)
            per = float(cnt.cpu().numpy().mean())
            # a CU holds several of these workgroups, so this is an upper bound of one merge's latency when G exceeds the CU count
            print("| %d | %d | %.1f | %.1f | %.2f | %.2f (%.0f, %.2f) | %d of %d |" %
                  (G, n, wall, dev, t_score, t_ahc, per, 1e3 * t_ahc / max(per, 1.0) / max(1.0, G / 256.0), ok, G))
        sys.stdout.flush()


if __name__ == "__main__":
    args = sys.argv[1:]
    loop = "--loop" in args
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 3
    shapes = [tuple(int(v) for v in a.split(":")) for a in args if ":" in a] or [(256, 200), (2048, 100)]
    if "--dim" in args:
        DIM = int(args[args.index("--dim") + 1])
    target_energy = float(args[args.index("--target-energy") + 1]) if "--target-energy" in args else 1.0
    from xvector_amd import backend
    if backend.target_energy_is_one(backend.check_target_energy(target_energy)):
        main(shapes, loop, reps)
    else:
        pca_main(shapes, reps, target_energy)
