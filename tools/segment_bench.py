"""Wall time of the from-wav sliding job with and without segmentation, on synthetic 8 kHz recordings of
`--minutes` minutes (loud noise in turns of 1-6 s between pauses of 0.1-2 s, so that pauses fall on both sides of --segment-max-gap)
in a temporary directory:
  plain      `extract_embedding.py --wav-rspecifier scp:wav.scp --cmn-window 300 --window 150 --period 75 --subsegments-file F`:
             windows over the concatenated voiced frames of a recording;
  segmented  the same with `--segment-by-vad`: the VAD decisions become segments on the device, windows are cut inside them.
The two jobs do different work (other windows, CMN inside segments): there is no bar, the cost of the route's extra download and
wait per window of recordings is what is looked for.  Each runs as the command line a user would type, `--reps` times in turn;
reported are every wall time, the vectors and the segments.  Run it under a time limit:
    timeout 900 python tools/segment_bench.py [--recordings 64] [--minutes 5] [--reps 3] [--topology ModelWithoutDropout]"""
import argparse, json, os, re, shutil, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "x-vector-kaldi-tf_amd")
TWIN = os.path.join(PKG, "local", "tf")
sys.path.insert(0, ROOT); sys.path.insert(0, PKG); sys.path.insert(0, TWIN)
import numpy as np

FS = 8000


def synth(d, n_reco, minutes, seed):
    from xvector_amd import mfcc
    rng = np.random.default_rng(seed)
    n = int(minutes * 60 * FS)
    pool = rng.integers(-3000, 3001, n + 64 * FS).astype(np.int16)
    os.makedirs(os.path.join(d, "wav"))
    lines = []
    for u in range(n_reco):
        off = int(rng.integers(0, 64 * FS))
        env = np.ones(n, bool)
        at = int(rng.integers(0, 2 * FS))
        while at < n:
            at += int(rng.integers(FS, 6 * FS))
            gap = int(rng.integers(FS // 10, 2 * FS))
            env[at:at + gap] = False
            at += gap
        x = np.where(env, pool[off:off + n], pool[off:off + n] >> 10).astype(np.int16)
        path = os.path.join(d, "wav", "reco%03d.wav" % u)
        with open(path, "wb") as f:
            f.write(mfcc.wav_bytes(x, FS))
        lines.append("reco%03d %s\n" % (u, path))
    scp = os.path.join(d, "wav.scp")
    with open(scp, "w") as f:
        f.writelines(lines)
    return scp


def run(cmd, log):
    t0 = time.perf_counter()
    with open(log, "wb") as f:
        subprocess.run([sys.executable] + cmd, check=True, stdout=f, stderr=subprocess.STDOUT)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", type=int, default=64)
    ap.add_argument("--minutes", type=float, default=5.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--topology", default="ModelWithoutDropout")
    args = ap.parse_args()
    import models
    from xvector_amd import synthetic, topology
    conf, vconf = os.path.join(ROOT, "tests", "golden", "mfcc.conf"), os.path.join(ROOT, "tests", "golden", "vad.conf")
    d = tempfile.mkdtemp(prefix="segment_bench_")
    try:
        t0 = time.perf_counter()
        scp = synth(d, args.recordings, args.minutes, 0)
        print("%d recordings of %.1f min written in %.1f s" % (args.recordings, args.minutes, time.perf_counter() - t0), flush=True)
        topo = topology.get(args.topology)
        mdir = os.path.join(d, "nnet")
        models.Model.save_model(dict(weights=synthetic.trained_like(topo, 23, num_classes=8, seed=2024), topology=topo,
                                     model_class=args.topology, num_classes=8, feat_dim=23), mdir, None)
        common = [os.path.join(TWIN, "extract_embedding.py"), "--use-gpu=yes", "--min-chunk-size=50", "--cmn-window=300", "--window=150",
                  "--period=75", "--model-dir=" + mdir, "--wav-rspecifier=scp:" + scp, "--mfcc-config=" + conf, "--vad-config=" + vconf]
        times, found = dict(plain=[], segmented=[]), {}
        for rep in range(args.reps):
            for name, extra in (("plain", []), ("segmented", ["--segment-by-vad"])):
                o = os.path.join(d, "%s%d" % (name, rep))
                os.makedirs(o)
                log = os.path.join(d, name + ".log")
                times[name].append(run(common + extra + ["--subsegments-file=%s/subsegments" % o,
                                                         "--vector-wspecifier=ark,scp:%s/xvector.ark,%s/xvector.scp" % (o, o)], log))
                text = open(log, errors="replace").read()
                m = re.search(r"cut (\d+) segments", text)
                found[name] = dict(vectors=sum(1 for _ in open(os.path.join(o, "xvector.scp"))), segments=int(m.group(1)) if m else None,
                                   job=[ln.strip().split(" ] ")[-1] for ln in text.splitlines() if "Job wall clock" in ln or "Processed" in ln])
                print("rep %d %-9s %.2f s  %s" % (rep, name, times[name][-1], found[name]), flush=True)
                shutil.rmtree(o)
        print(json.dumps(dict(tool="segment_bench", recordings=args.recordings, minutes=args.minutes, topology=args.topology,
                              seconds_plain=[round(t, 3) for t in times["plain"]], seconds_segmented=[round(t, 3) for t in times["segmented"]],
                              best_plain=round(min(times["plain"]), 3), best_segmented=round(min(times["segmented"]), 3),
                              vectors_plain=found["plain"]["vectors"], vectors_segmented=found["segmented"]["vectors"],
                              segments=found["segmented"]["segments"])))
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
