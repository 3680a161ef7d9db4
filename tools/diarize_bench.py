"""Timings of diarization on planted speakers: G recordings of n sub-segments each, every recording from SPK
planted speakers, shuffled.  Without --loop: backend.diarize (every recording's score block from one launch, one workgroup per
recording's clustering), wall time and device-event time of the whole call after a warm-up, and beside them its two device stages
on their own (the two prepare calls + xv_score_blocks_f32; xv_ahc_average_batch_f64).  With --loop: the per-recording Python loop
around backend.cluster_vectors, the only route before the batch existed; it needs nothing newer than §8.9, so it also runs on an
older checkout.  Both report how many recordings came out as their planted partition.
    python tools/diarize_bench.py [--loop] [--reps R] [G:n ...]        (default shapes 256:200 2048:100, R = 3, the best is printed)"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "x-vector-kaldi-tf_amd"))
import numpy as np

DIM, SPK = 64, 4           # vector dimension (no LDA: the planted model is already diagonal), planted speakers per recording


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
    shapes = [tuple(int(v) for v in a.split(":")) for a in args if ":" in a]
    main(shapes or [(256, 200), (2048, 100)], loop, reps)
