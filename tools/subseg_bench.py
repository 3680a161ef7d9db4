"""Wall time of sliding-window extraction next to the averaged mode on the same input: synthetic raw features
(23 dimensions) and VAD decisions (about three quarters voiced, in runs) of `--utts` utterances of 20-40 s held in memory, through
`Extractor.submit_raw` + `finish` (CMN 300 + selection on the device, default arithmetic) once per mode after one warm-up pass each:
  averaged   min-chunk-size 25, chunk-size 10000: one vector per utterance;
  sliding    window 150, period 75: one vector per sub-segment.
Prints one JSON line: the wall times, the vectors, and the packed rows of each mode (`Extractor.stats`) with their ratio.  Run it
under a time limit:
    timeout 600 python tools/subseg_bench.py [--utts 300] [--reps 3] [--topology ModelWithoutDropout]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "x-vector-kaldi-tf_amd")
sys.path.insert(0, ROOT); sys.path.insert(0, PKG); sys.path.insert(0, os.path.join(PKG, "local", "tf"))
import numpy as np


def synth(n_utts, seed):
    rng = np.random.default_rng(seed)
    mats, vads = [], []
    for _ in range(n_utts):
        t = int(rng.integers(2000, 4001))
        mats.append((rng.standard_normal((t, 23)) * 3 + 1.5).astype(np.float32))
        v = np.ones(t, np.float32)
        at = int(rng.integers(0, 200))
        while at < t:                                                   # 1-3 s voiced, 0.3-1 s silent
            at += int(rng.integers(100, 300))
            gap = int(rng.integers(30, 100))
            v[at:at + gap] = 0
            at += gap
        vads.append(v)
    return mats, vads


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=300)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--topology", default="ModelWithoutDropout")
    args = ap.parse_args()
    import torch
    from xvector_amd import engine, synthetic, topology
    topo = topology.get(args.topology)
    model = engine.select_model(synthetic.trained_like(topo, 23, seed=1), topo, "cuda:0")
    mats, vads = synth(args.utts, 7)
    out = dict(utts=args.utts, raw_frames=int(sum(m.shape[0] for m in mats)), arithmetic=model.arithmetic, reps=args.reps)
    for name, kw in (("averaged", {}), ("sliding", dict(window=150, period=75))):
        times = []
        for rep in range(args.reps + 1):                                # the first pass pins buffers and sizes the model's: not timed
            ex = engine.Extractor(model, 25, 10000, **kw)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            handle, lens, dropped = ex.submit_raw(mats, vads, 300, True)
            got = ex.finish(handle)
            if rep:
                times.append(time.perf_counter() - t0)
        vectors = sum(len(g[0]) if kw else 1 for g in got if g is not None)
        out[name] = dict(wall_s=[round(t, 4) for t in times], best_s=round(min(times), 4), vectors=int(vectors),
                         voiced_frames=int(lens.sum()), packed_rows=int(ex.stats["rows"]), batches=int(ex.stats["batches"]),
                         demoted=bool(ex.demoted), fallback_windows=int(ex.stats.get("fallback_windows", 0)))
    out["packed_row_ratio"] = round(out["sliding"]["packed_rows"] / float(out["averaged"]["packed_rows"]), 3)
    out["wall_ratio"] = round(out["sliding"]["best_s"] / out["averaged"]["best_s"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
