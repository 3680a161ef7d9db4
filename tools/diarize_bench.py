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
With --vbx: speakers take turns of 5 sub-segments (VBx models time), backend.diarize with and without
vbx={} and their difference, xv_vbx_groups_f64 on its own (every call of backend.vbx_groups, its download included), and the host
route beside it: backend.vbx_host looped over the recordings in NumPy, one host thread.  --threshold T sets the clustering's stop
rule (a high one over-splits: more initial speakers).  --vbx-probe: one recording of T = 4096, S = 16 at d = 128 and at d = 4, 10
iterations -- the two MFMA products shrink 32-fold with d, the one-wave chains do not, so the pair shows the chains' share.
    python tools/diarize_bench.py [--loop] [--reps R] [--dim D] [--target-energy F] [--vbx [--threshold T]] [--vbx-probe] [G:n ...]
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


def planted_turns(G, n, seed=0, turn=5):
    """``planted`` with the speakers taking turns of ``turn`` vectors in a fixed cycle instead of a shuffle."""
    from xvector_amd import backend
    rng = np.random.default_rng(seed)
    psi = np.sort(rng.uniform(2.0, 12.0, DIM))[::-1]
    spk = np.tile((np.arange(n) // turn) % SPK, (G, 1))
    centres = rng.standard_normal((G, SPK, DIM)) * np.sqrt(psi)
    x = centres[np.arange(G)[:, None], spk] + rng.standard_normal((G, n, DIM))
    return x.reshape(G * n, DIM).astype(np.float32), spk, backend.Plda(np.zeros(DIM), np.eye(DIM), psi)


def vbx_main(shapes, reps, threshold):
    """The --vbx route: diarize with and without VBx, the kernel on its own, the host loop of vbx_host."""
    import torch
    from xvector_amd import backend, hiplib
    hiplib.require_gpu()
    x, _, plda = planted_turns(4, 50)
    backend.diarize(x, [50] * 4, plda, threshold=threshold, vbx={})          # warm-up: code objects, allocator
    print("| G | n | d | diarize(): wall ms | device-event ms | diarize(vbx={}): wall ms | device-event ms | difference: wall ms "
          "| vbx_groups alone: wall ms (device-event ms) | host vbx_host loop: wall ms (ms / recording) | speakers before -> after "
          "| mean iterations | info 2 | planted partitions before -> after |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for G, n in shapes:
        x, spk, plda = planted_turns(G, n)
        sizes = [n] * G
        w0, d0, (lab0, _) = best(lambda: backend.diarize(x, sizes, plda, threshold=threshold), reps)
        rep = {}
        w1, d1, (lab1, _) = best(lambda: backend.diarize(x, sizes, plda, threshold=threshold, vbx={}, vbx_report=rep), reps)
        ok0 = sum(same_partition(lab0[g * n:(g + 1) * n], spk[g]) for g in range(G))
        ok1 = sum(same_partition(lab1[g * n:(g + 1) * n], spk[g]) for g in range(G))
        Y, _ = backend.prepare(x, hiplib.SIDE_PLAIN, None, None, None, None, False)
        tables = backend.GroupTables(sizes, Y.device)
        init = np.concatenate([backend.compact_labels(lab0[g * n:(g + 1) * n])[0] for g in range(G)])
        run = np.flatnonzero(rep["ran"])
        if run.size == 0:
            print("| %d | %d | %d | %.1f | %.1f | %.1f | %.1f | %.1f | no recording has at most %d clusters: lower --threshold |"
                  % (G, n, plda.dim, w0, d0, w1, d1, w1 - w0, hiplib.VBX_MAX_SPK))
            continue
        if run.size < G:                                         # the stage alone and the host loop: the recordings that ran
            rows = np.concatenate([np.arange(g * n, (g + 1) * n) for g in run])
            Y, init = Y[torch.as_tensor(rows, device=Y.device)], init[rows]
            tables = backend.GroupTables([n] * run.size, Y.device)
        wk, dk, res = best(lambda: backend.vbx_groups(Y, tables, init, plda), reps)
        Yh = Y.cpu().numpy()

        def host_loop():
            return [backend.vbx_host(Yh[g * n:(g + 1) * n], init[g * n:(g + 1) * n], plda) for g in range(run.size)]
        wh, _, host = min((timed(host_loop) for _ in range(min(reps, 2))), key=lambda r: r[0])
        same = sum(np.array_equal(host[g]["labels"], res["labels"][g * n:(g + 1) * n]) and host[g]["iters"] == res["iters"][g]
                   for g in range(run.size))
        print("| %d | %d | %d | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f (%.2f) | %.0f (%.2f) | %.2f -> %.2f | %.2f | %d | %d -> %d of %d |"
              % (G, n, plda.dim, w0, d0, w1, d1, w1 - w0, wk, dk, wh, wh / run.size, float(rep["spk_before"].mean()),
                 float(rep["spk_after"].mean()), float(rep["iters"][run].mean()) if run.size else 0.0, int((rep["info"] == 2).sum()),
                 ok0, ok1, G))
        print("  (recordings VBx ran on: %d of %d; those whose labels and iteration count agree between the kernel and the host "
              "loop: %d of %d)" % (run.size, G, same, run.size))
        sys.stdout.flush()


def vbx_probe(reps, T=4096, S=16, iters=10):
    """One recording of T vectors and S initial speakers, ``iters`` iterations (epsilon = -inf), at d = 128 and d = 4."""
    global DIM
    import torch
    from xvector_amd import backend, hiplib
    hiplib.require_gpu()
    print("| T | S | d | iterations | vbx_groups: device-event ms | ms / iteration |")
    print("|---|---|---|---|---|---|")
    for d in (128, 4):
        DIM = d
        x, spk, plda = planted_turns(1, T)
        Y = torch.as_tensor(x, device="cuda:0")
        tables = backend.GroupTables([T], Y.device)
        init = ((np.arange(T) // 5) % S).astype(np.int32)
        backend.vbx_groups(Y, tables, init, plda, max_iters=1)
        _, d1, _ = best(lambda: backend.vbx_groups(Y, tables, init, plda, max_iters=1, epsilon=-np.inf), reps)
        _, dn, res = best(lambda: backend.vbx_groups(Y, tables, init, plda, max_iters=iters + 1, epsilon=-np.inf), reps)
        assert res["iters"][0] == iters + 1 and res["info"][0] == 0
        print("| %d | %d | %d | %d | %.2f | %.3f |" % (T, S, d, iters + 1, dn, (dn - d1) / iters))
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
    if "--vbx-probe" in args:
        vbx_probe(reps)
    elif "--vbx" in args:
        vbx_main(shapes, reps, float(args[args.index("--threshold") + 1]) if "--threshold" in args else 0.0)
    elif backend.target_energy_is_one(backend.check_target_energy(target_energy)):
        main(shapes, loop, reps)
    else:
        pca_main(shapes, reps, target_energy)
