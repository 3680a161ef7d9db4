"""Wall time of x-vector extraction from audio, two ways, on synthetic 8 kHz utterances of 20-40 s (bursts of loud
noise between quiet gaps, so that the energy VAD keeps roughly three quarters of the frames) in a temporary directory:
  A. the two-step route: `mfcc_vad.py compute-mfcc-vad` to plain float tables on disk, then `extract_embedding.py
     --feature-rspecifier scp:feats.scp --vad-rspecifier scp:vad.scp --cmn-window 300` (two processes);
  B. the direct route: `extract_embedding.py --wav-rspecifier scp:wav.scp --cmn-window 300` (one process, no table).
Each route runs as the command lines a user would type, `--reps` times in turn (A, B, A, B, ...); reported are every wall time, the
best of each route, the bytes each route wrote and whether the two x-vector arks are byte-equal.  Run it under a time limit:
    timeout 900 python tools/wav_direct_bench.py [--utts 2000] [--reps 2] [--topology ModelWithoutDropout]"""
import argparse, json, os, shutil, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "x-vector-kaldi-tf_amd")
TWIN = os.path.join(PKG, "local", "tf")
sys.path.insert(0, ROOT); sys.path.insert(0, PKG); sys.path.insert(0, TWIN)
import numpy as np

FS = 8000


def synth(d, n_utts, seed):
    """n_utts WAV files + wav.scp under d; returns (scp path, total samples)."""
    from xvector_amd import mfcc
    rng = np.random.default_rng(seed)
    pool = rng.integers(-3000, 3001, 64 * FS).astype(np.int16)         # every utterance is a slice of it under its own envelope
    total, lines = 0, []
    os.makedirs(os.path.join(d, "wav"))
    for u in range(n_utts):
        n = int(rng.integers(20 * FS, 40 * FS + 1))
        off = int(rng.integers(0, len(pool) - n + 1))
        env = np.ones(n, bool)
        at = int(rng.integers(0, 2 * FS))
        while at < n:                                                   # 1-3 s loud, 0.3-1 s quiet
            at += int(rng.integers(FS, 3 * FS))
            gap = int(rng.integers(3 * FS // 10, FS))
            env[at:at + gap] = False
            at += gap
        x = np.where(env, pool[off:off + n], pool[off:off + n] >> 10).astype(np.int16)
        path = os.path.join(d, "wav", "utt%05d.wav" % u)
        with open(path, "wb") as f:
            f.write(mfcc.wav_bytes(x, FS))
        lines.append("spk%03d-utt%05d %s\n" % (u % 200, u, path))
        total += n
    scp = os.path.join(d, "wav.scp")
    with open(scp, "w") as f:
        f.writelines(sorted(lines))
    return scp, total


def tree_bytes(d):
    return sum(os.path.getsize(os.path.join(r, f)) for r, _, fs in os.walk(d) for f in fs)


def run(cmd, log):
    t0 = time.perf_counter()
    with open(log, "ab") as f:
        subprocess.run([sys.executable] + cmd, check=True, stdout=f, stderr=subprocess.STDOUT)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--topology", default="ModelWithoutDropout")
    ap.add_argument("--keep", default="", help="copy the routes' logs to this directory")
    args = ap.parse_args()
    import models
    from xvector_amd import synthetic, topology
    conf, vconf = os.path.join(ROOT, "tests", "golden", "mfcc.conf"), os.path.join(ROOT, "tests", "golden", "vad.conf")
    d = tempfile.mkdtemp(prefix="wav_direct_bench_")
    try:
        t0 = time.perf_counter()
        scp, samples = synth(d, args.utts, 0)
        print("%d utterances, %.1f h of audio, %.0f MB of WAV written in %.1f s" % (
            args.utts, samples / FS / 3600.0, tree_bytes(os.path.join(d, "wav")) / 1e6, time.perf_counter() - t0), flush=True)
        topo = topology.get(args.topology)
        mdir = os.path.join(d, "nnet")
        models.Model.save_model(dict(weights=synthetic.trained_like(topo, 23, num_classes=8, seed=2024), topology=topo,
                                     model_class=args.topology, num_classes=8, feat_dim=23), mdir, None)
        common = ["--use-gpu=yes", "--min-chunk-size=25", "--chunk-size=10000", "--cmn-window=300", "--model-dir=" + mdir]
        times = dict(A=[], A_mfcc=[], A_extract=[], B=[])
        written, arks = {}, {}
        for rep in range(args.reps):
            a, b = os.path.join(d, "A%d" % rep), os.path.join(d, "B%d" % rep)
            os.makedirs(a); os.makedirs(b)
            t1 = run([os.path.join(TWIN, "mfcc_vad.py"), "compute-mfcc-vad", "--config", conf, "--vad-config", vconf, "scp:" + scp,
                      "ark,scp:%s/feats.ark,%s/feats.scp" % (a, a), "ark,scp:%s/vad.ark,%s/vad.scp" % (a, a)], os.path.join(d, "A.log"))
            t2 = run([os.path.join(TWIN, "extract_embedding.py")] + common + [
                "--feature-rspecifier=scp:%s/feats.scp" % a, "--vad-rspecifier=scp:%s/vad.scp" % a,
                "--vector-wspecifier=ark,scp:%s/xvector.ark,%s/xvector.scp" % (a, a)], os.path.join(d, "A.log"))
            t3 = run([os.path.join(TWIN, "extract_embedding.py")] + common + [
                "--wav-rspecifier=scp:" + scp, "--mfcc-config=" + conf, "--vad-config=" + vconf,
                "--vector-wspecifier=ark,scp:%s/xvector.ark,%s/xvector.scp" % (b, b)], os.path.join(d, "B.log"))
            times["A_mfcc"].append(t1); times["A_extract"].append(t2); times["A"].append(t1 + t2); times["B"].append(t3)
            written = dict(A=tree_bytes(a), B=tree_bytes(b))
            arks = dict(A=open(os.path.join(a, "xvector.ark"), "rb").read(), B=open(os.path.join(b, "xvector.ark"), "rb").read())
            n_vec = sum(1 for _ in open(os.path.join(b, "xvector.scp")))
            print("rep %d: A %.2f s (compute-mfcc-vad %.2f + extract %.2f), B %.2f s; arks equal: %s (%d vectors)" % (
                rep, t1 + t2, t1, t2, t3, arks["A"] == arks["B"], n_vec), flush=True)
            shutil.rmtree(a); shutil.rmtree(b)
        for name in ("A.log", "B.log"):
            tail = [ln for ln in open(os.path.join(d, name), errors="replace") if "Job wall clock" in ln or "Elapsed time" in ln]
            print("%s: %s" % (name, " | ".join(s.strip().split(" ] ")[-1] for s in tail[-2:])))
            if args.keep:
                os.makedirs(args.keep, exist_ok=True)
                shutil.copy(os.path.join(d, name), os.path.join(args.keep, "wav_direct_bench_" + name))
        best = {k: min(v) for k, v in times.items()}
        print(json.dumps(dict(tool="wav_direct_bench", utts=args.utts, audio_hours=round(samples / FS / 3600.0, 3), topology=args.topology,
                              seconds_A=[round(t, 3) for t in times["A"]], seconds_B=[round(t, 3) for t in times["B"]],
                              best_A=round(best["A"], 3), best_A_mfcc=round(best["A_mfcc"], 3), best_A_extract=round(best["A_extract"], 3),
                              best_B=round(best["B"], 3), speedup_B_over_A=round(best["A"] / best["B"], 3),
                              bytes_written_A=written["A"], bytes_written_B=written["B"], arks_equal=arks["A"] == arks["B"],
                              vectors=n_vec)))
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
