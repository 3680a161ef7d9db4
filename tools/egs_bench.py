"""Rates of the egs builder on the GPU on synthetic utterances of the recipe's shape (F = 23, T ~ U[600, 3000],
~70 % voiced, chunks of 200-400 frames, 64 per minibatch):
  1. xv_egs_chunks_f16 (voiced index built beforehand) in output frames/s, against the two-step path the tree already had:
     xv_cmn_sliding_scatter_f32 over whole utterances into a float32 no-silence table, then a torch row gather and .half();
  2. the same two from host arrays to host arrays (DeviceGather against FrontEnd.apply + torch gather + .half() + copy back);
  3. the whole `make_egs.py write` step on a data directory on disk (read, cut, tar), in output frames/s.
    python tools/egs_bench.py [--utts N] [--minibatches M] [--reps R]"""
import argparse, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWIN = os.path.join(ROOT, "x-vector-kaldi-tf_amd", "local", "tf")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "x-vector-kaldi-tf_amd")); sys.path.insert(0, TWIN)
import numpy as np

F, B = 23, 64


def synth(n_utts, seed):
    rng = np.random.default_rng(seed)
    lens = rng.integers(600, 3001, size=n_utts)
    mats = [(rng.standard_normal((int(t), F)) * 3 + 5).astype(np.float32) for t in lens]
    vads = [(rng.random(int(t)) < 0.7).astype(np.float32) for t in lens]
    return mats, vads


def chunk_table(counts, n_minibatches, seed):
    rng = np.random.default_rng(seed)
    cu, cf, cl, cd, pos = [], [], [], [], 0
    for _ in range(n_minibatches):
        n = int(rng.integers(200, 401))
        ok = np.flatnonzero(counts >= n)
        for u in rng.choice(ok, size=B).tolist():
            cu.append(u); cf.append(int(rng.integers(0, counts[u] - n + 1))); cl.append(n); cd.append(pos)
            pos += n * F
    return (np.array(cu, np.int32), np.array(cf, np.int32), np.array(cl, np.int32), np.array(cd, np.int64)), pos


def timed(fn, reps, sync):
    fn(); sync()
    best = float("inf")
    for _ in range(reps):
        sync(); t0 = time.perf_counter(); fn(); sync()
        best = min(best, time.perf_counter() - t0)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=600)
    ap.add_argument("--minibatches", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    from xvector_amd import egs, frontend, hiplib
    hiplib.require_gpu()
    sync = torch.cuda.synchronize
    mats, vads = synth(args.utts, 0)
    lens = np.array([m.shape[0] for m in mats], np.int32)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    raw, vad = np.concatenate(mats), np.concatenate(vads)
    counts = np.array([int(np.count_nonzero(v)) for v in vads])
    table, n_halves = chunk_table(counts, args.minibatches, 1)
    out_frames = n_halves // F
    print("%d utterances, %d raw frames, %d voiced; %d minibatches of %d chunks, %d output frames (%.0f %% of the voiced frames, with repeats)"
          % (args.utts, raw.shape[0], counts.sum(), args.minibatches, B, out_frames, 100.0 * out_frames / counts.sum()))
    dev = torch.device("cuda:0")
    x, v = torch.from_numpy(raw).to(dev), torch.from_numpy(vad).to(dev)
    us, ul = torch.from_numpy(starts).to(dev), torch.from_numpy(lens).to(dev)
    count, rows = hiplib.vad_compact(v, us, ul)
    assert np.array_equal(count.cpu().numpy(), counts)
    y = torch.zeros(n_halves, dtype=torch.float16, device=dev)
    t_compact = timed(lambda: hiplib.vad_compact(v, us, ul), args.reps, sync)
    t_fused = timed(lambda: hiplib.egs_chunks(x, us, ul, count, rows, table, counts, 300, True, 100, y), args.reps, sync)
    # the two-step path on the device: whole utterances -> float32 no-silence table, then gather + .half()
    voiced = vad != 0
    dst_row = torch.from_numpy(np.where(voiced, np.cumsum(voiced) - 1, -1).astype(np.int32)).to(dev)
    ostart = np.concatenate([[0], np.cumsum(counts)[:-1]])
    idx = torch.from_numpy(np.concatenate([ostart[u] + f + np.arange(n) for u, f, n in zip(*table[:3])]).astype(np.int64)).to(dev)
    tab = torch.zeros((int(counts.sum()), F), device=dev)
    t_cmn = timed(lambda: hiplib.cmn_sliding_scatter(x, us, ul, len(lens), int(lens.max()), 300, True, 100, dst_row, tab), args.reps, sync)
    two = [None]

    def gather():
        two[0] = tab.index_select(0, idx).half()
    t_gather = timed(gather, args.reps, sync)
    same = float((two[0].reshape(-1) == y).float().mean())
    print("device only (best of %d):" % args.reps)
    print("  xv_vad_compact_i32                      %8.3f ms   %.3e raw frames/s" % (t_compact * 1e3, raw.shape[0] / t_compact))
    print("  xv_egs_chunks_f16 (+ table upload)      %8.3f ms   %.3e output frames/s" % (t_fused * 1e3, out_frames / t_fused))
    print("  xv_cmn_sliding_scatter_f32, all frames  %8.3f ms" % (t_cmn * 1e3))
    print("  torch index_select + .half()            %8.3f ms" % (t_gather * 1e3))
    print("  two-step total                          %8.3f ms   %.3e output frames/s   (fused is %.2fx; %.4f of the halves identical)"
          % ((t_cmn + t_gather) * 1e3, out_frames / (t_cmn + t_gather), (t_cmn + t_gather) / t_fused, same))
    # host to host
    g = egs.DeviceGather("cuda:0", 300, True, 100)

    def fused_host():
        yy = g.alloc(n_halves)
        g(yy, raw, vad, starts, lens, table)
        return g.fetch(yy)
    fe = frontend.FrontEnd("cuda:0", 300, True, 100)
    idx_host = idx.cpu()

    def two_step_host():
        sel = fe.apply(mats, vads)
        t = torch.from_numpy(np.concatenate(sel)).to(dev)
        return t.index_select(0, idx.to(dev)).half().cpu().numpy()
    t_fh = timed(fused_host, max(args.reps // 2, 1), sync)
    t_th = timed(two_step_host, max(args.reps // 2, 1), sync)
    print("host arrays in, host float16 out:")
    print("  DeviceGather (upload, 2 kernels, copy back)         %8.1f ms   %.3e output frames/s" % (t_fh * 1e3, out_frames / t_fh))
    print("  FrontEnd.apply + torch gather + .half() + copy back %8.1f ms   %.3e output frames/s   (fused is %.2fx)"
          % (t_th * 1e3, out_frames / t_th, t_th / t_fh))
    del idx_host
    # the whole write step
    import kaldi_io
    with tempfile.TemporaryDirectory() as tmp:
        keys = ["utt%05d" % i for i in range(args.utts)]
        with kaldi_io.TableWriter(os.path.join(tmp, "feats.ark"), os.path.join(tmp, "feats.scp")) as tf, \
                kaldi_io.TableWriter(os.path.join(tmp, "vad.ark"), os.path.join(tmp, "vad.scp")) as tv:
            for k, m, vv in zip(keys, mats, vads):
                kaldi_io.write_mat(tf, m, key=k)
                kaldi_io.write_vec_flt(tv, vv, key=k)
        egs_dir = os.path.join(tmp, "egs")
        n_spk = max(args.utts // 8, B)
        cnt = egs.allocate([(k, int(c)) for k, c in zip(keys, counts)], [(k, i % n_spk) for i, k in enumerate(keys)], egs_dir,
                           num_repeats=max(2, (args.minibatches * B) // n_spk + 1), min_frames_per_chunk=200, max_frames_per_chunk=400,
                           frames_per_iter=args.minibatches * B * 300, num_archives=1, num_jobs=1, minibatch_size=B)
        w = egs.EgsWriter(egs_dir, os.path.join(tmp, "feats.scp"), os.path.join(tmp, "vad.scp"), F, B, shuffle=True, random_seed=2468, gather=g)
        t0 = time.perf_counter()
        w.write_job(os.path.join(egs_dir, "temp", "outputs.1"))
        t_write = time.perf_counter() - t0
        size = os.path.getsize(os.path.join(egs_dir, "egs.1.tar"))
        print("make_egs.py write, one archive of %d minibatches (%d output frames, %.0f MB tar) from files on local disk:" % (
            cnt[0], w.stats["frames_out"], size / 1e6))
        print("  %.2f s   %.3e output frames/s   (%d raw frames read)" % (t_write, w.stats["frames_out"] / t_write, w.stats["frames_in"]))


if __name__ == "__main__":
    main()
