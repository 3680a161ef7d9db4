"""Cost of compressed feature output on synthetic utterances of the recipe's shape (F = 23, T ~ U[600, 3000]):
  1. the encoder on the device (xv_cm_encode_f32: range, column statistics, elements -- three launches timed together with
     device events; `rocprofv3 --kernel-trace --stats -- python tools/compress_bench.py --device-only` splits them), and the
     copy back of the packed block against that of the fp32 table;
  2. host to host: Mfcc.compute on the same waves with compress=False (the plain path) and compress=True, and the write of
     what each returns to a local ark,scp pair.
Every figure is the best of --reps runs after a warm-up, with the spread (max - min) of those runs.
    python tools/compress_bench.py [--utts N] [--reps R] [--device-only]"""
import argparse, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWIN = os.path.join(ROOT, "x-vector-kaldi-tf_amd", "local", "tf")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "x-vector-kaldi-tf_amd")); sys.path.insert(0, TWIN)
import numpy as np

F = 23


def runs(fn, reps):
    """(best, spread) in seconds of ``fn() -> seconds`` over ``reps`` runs after one warm-up."""
    fn()
    t = [fn() for _ in range(reps)]
    return min(t), max(t) - min(t)


def wall(fn, sync):
    def one():
        sync(); t0 = time.perf_counter(); fn(); sync()
        return time.perf_counter() - t0
    return one


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=600)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device-only", action="store_true")
    args = ap.parse_args()
    import torch
    import kaldi_io
    from xvector_amd import compress, hiplib, mfcc
    hiplib.require_gpu()
    sync = torch.cuda.synchronize
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    T = rng.integers(600, 3001, size=args.utts).astype(np.int64)
    rows = int(T.sum())
    row0 = np.concatenate([[0], np.cumsum(T)[:-1]]).astype(np.int64)
    feats = torch.from_numpy((rng.standard_normal((rows, F)) * 3 + 5).astype(np.float32)).to(dev)
    offsets, sizes, total = compress.plan(T, F)
    d_row0, d_T, d_off = (torch.from_numpy(a).to(dev) for a in (row0, T.astype(np.int32), offsets))
    out = torch.empty(total, dtype=torch.uint8, device=dev)
    status = torch.empty(args.utts, dtype=torch.int32, device=dev)
    print("%d utterances, %d frames x %d: fp32 table %.1f MB, packed block %.1f MB (%.3f of it)"
          % (args.utts, rows, F, rows * F * 4 / 1e6, total / 1e6, total / (rows * F * 4.0)))

    def encode_events():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        hiplib.cm_encode(feats, d_row0, d_T, F, d_off, out, status)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e-3
    ms = lambda r: "%8.3f ms (spread %.3f)" % (r[0] * 1e3, r[1] * 1e3)  # noqa: E731
    r = runs(encode_events, args.reps)
    assert not status.any().item()
    print("device (best of %d):" % args.reps)
    print("  xv_cm_encode_f32, three launches       %s   %.1f GB/s of fp32 read once" % (ms(r), rows * F * 4 / r[0] / 1e9))
    print("  copy back, fp32 table                  %s" % ms(runs(wall(lambda: feats.cpu().numpy(), sync), args.reps)))
    print("  copy back, packed block                %s" % ms(runs(wall(lambda: out.cpu().numpy(), sync), args.reps)))
    if args.device_only:
        return
    # host to host: 8 kHz waves whose frame counts are T (--snip-edges=false: one frame per 80 samples)
    opts = mfcc.MfccOptions(sample_frequency=8000, num_ceps=F, high_freq=3700, snip_edges=False)
    waves = [rng.integers(-3000, 3000, size=int(t) * 80, dtype=np.int16) for t in T]
    keys = ["utt%05d" % i for i in range(args.utts)]
    eng = mfcc.Mfcc(opts, mfcc.VadOptions())
    got = {}

    def compute(flag):
        def fn():
            got[flag] = eng.compute(keys, waves, compress=flag)[0]
        return wall(fn, sync)

    with tempfile.TemporaryDirectory() as tmp:
        def write(flag):
            def fn():
                with kaldi_io.TableWriter(os.path.join(tmp, "f.ark"), os.path.join(tmp, "f.scp")) as w:
                    for k, f in zip(keys, got[flag]):
                        if flag:
                            kaldi_io.write_cm_payload(w, f.payload, f.rows, key=k)
                        else:
                            kaldi_io.write_mat(w, f, key=k)
                got["size", flag] = os.path.getsize(os.path.join(tmp, "f.ark"))
            return wall(fn, sync)
        print("host to host, %d samples in (best of %d):" % (sum(len(w) for w in waves), args.reps))
        tot = {}
        for flag in (False, True):
            c, w = runs(compute(flag), args.reps), runs(write(flag), args.reps)
            tot[flag] = (c[0] + w[0], c[1] + w[1])
            print("  compress=%-5s Mfcc.compute %s   write %s   ark %.1f MB" % (flag, ms(c), ms(w), got["size", flag] / 1e6))
        print("  compute + write: plain %.1f ms, compressed %.1f ms (%.2fx; spreads %.1f / %.1f ms)"
              % (tot[False][0] * 1e3, tot[True][0] * 1e3, tot[False][0] / tot[True][0], tot[False][1] * 1e3, tot[True][1] * 1e3))


if __name__ == "__main__":
    main()
