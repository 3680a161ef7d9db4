"""Rates of stage 2 on the GPU: wav-reverberate evaluations per second at 8 kHz for 2-minute utterances and
RIRs of L = 0.25 / 0.5 / 1 / 2 s, the foreground-noise and nested background-noise (music / babble) forms, with achieved op/s
and byte/s from shape-derived counts against both roofs; then `mfcc_vad.py compute-mfcc-feats` on an augmented wav.scp against
the clean one (wall clock, real-time factor, read / augment / MFCC / write split).
    python tools/augment_bench.py [--kernel-only] [--utts N] [--seconds S]
(--kernel-only: only the evaluation timings at a smaller size, the form run under rocprofv3 --kernel-trace --stats)."""
import argparse, os, shutil, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWIN = os.path.join(ROOT, "x-vector-kaldi-tf_amd", "local", "tf")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "x-vector-kaldi-tf_amd")); sys.path.insert(0, TWIN)
import numpy as np

FS = 8000
HBM_TBS = 8.0          # MI355X HBM3E peak
FP64_TFLOPS = 78.6     # MI355X vector fp64 peak (AMD's published figure; the convolution's FMAs are fp64)
FP32_TFLOPS = 157.3    # MI355X vector fp32 peak (MI355X_MICROARCH.md)


def rir_like(L, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(L)
    peak = L // 20
    h = rng.standard_normal(L) * 6000.0 * np.exp(-np.maximum(t - peak, 0) / (L / 6.0))
    h[:peak] *= 0.05
    h[peak] = 30000.0
    return np.clip(np.rint(h), -32767, 32767).astype(np.int16)


def counts(plan):
    """(flop, HBM bytes) the algorithm needs for a plan: 2 flop per tap met by a sample in the full and the early convolutions,
    one fp64 multiply-add per noise sample mixed; bytes: int16 inputs and noises read once, the fp64 waveform written by the
    convolution, read and written by the mix and read by the write, the int16 output written once."""
    flop = byts = 0
    for n in plan.nodes:
        N, y = n.N, n.N
        byts += 2 * N + 2 * n.M
        if n.rir is not None:
            r = n.rir[3] if n.rir[0] == "host" else None
            L = len(r)
            peak = int(np.argmax(r))
            from xvector_amd import augment
            s, e = augment.early_window(peak, L, float(n.rate))
            flop += 2 * N * L + 2 * N * (e - s)
            y = N + L - 1
            byts += 8 * y
        for s, _, off in n.noises:
            ln = s[1].M if s[0] == "node" else len(s[3])
            k = max(0, min(y - off, ln))
            flop += 2 * k
            byts += 2 * k
        byts += 8 * y * 3
    return flop, byts


def evaluate_rate(d, entries, label, reps):
    import torch
    from xvector_amd import augment
    aug = augment.Augmenter()
    parsed = [(k, augment.parse_rx(rx)) for k, rx in entries]
    plan = aug.plan(parsed)
    lens = plan.lengths()
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    out = torch.empty(int(offs[-1]), dtype=torch.int16, device="cuda")
    aug.run(plan, out, offs[:-1])
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        aug.run(plan, out, offs[:-1])
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    t = float(np.median(times))
    flop, byts = counts(plan)
    samples = int(sum(n.N for n in plan.top))
    line = ("%s: %d utts, %.2f h of 8 kHz audio: %.2f ms per batch (host planning of the launch included) = %.3g input samples/s "
            "(%.0fx real time); %.2f Tflop/s = %.1f %% of %.1f fp64 (%.1f %% of %.1f fp32), %.1f GB/s = %.2f %% of %.0f TB/s; "
            "%.1f flop/B" % (label, len(entries), samples / FS / 3600.0, t * 1e3, samples / t, samples / FS / t, flop / t / 1e12,
                             100 * flop / t / (FP64_TFLOPS * 1e12), FP64_TFLOPS, 100 * flop / t / (FP32_TFLOPS * 1e12), FP32_TFLOPS,
                             byts / t / 1e9, 100 * byts / t / (HBM_TBS * 1e12), HBM_TBS, flop / float(max(byts, 1))))
    print(line, flush=True)
    return line


def make_inputs(d, n_utts, seconds):
    from xvector_amd import mfcc, synthetic
    base = synthetic.speech_like_wave(FS * 60, FS, 3)
    paths = []
    for i in range(n_utts):
        w = np.tile(np.roll(base, 7919 * i), int(seconds // 60) + 1)[:int(FS * seconds)]
        p = os.path.join(d, "u%04d.wav" % i)
        open(p, "wb").write(mfcc.wav_bytes(w, FS))
        paths.append(p)
    for j, L in enumerate((2000, 4000, 8000, 16000)):
        open(os.path.join(d, "rir%d.wav" % L), "wb").write(mfcc.wav_bytes(rir_like(L, j), FS))
    for j in range(6):
        n = synthetic.speech_like_wave(FS * (5 + 7 * j), FS, 100 + j)
        open(os.path.join(d, "n%d.wav" % j), "wb").write(mfcc.wav_bytes(n, FS))
    return paths


def forms(d, paths, seconds):
    rv = {L: [("u%04d-reverb" % i, "wav-reverberate --shift-output=true --impulse-response=%s/rir%d.wav %s - |" % (d, L, p))
              for i, p in enumerate(paths)] for L in (2000, 4000, 8000, 16000)}
    noise = [("u%04d-noise" % i, "wav-reverberate --shift-output=true --additive-signals='%s/n%d.wav,%s/n%d.wav,%s/n%d.wav' "
              "--start-times='0,%.2f,%.2f' --snrs='15,10,5' %s - |" % (d, i % 6, d, (i + 1) % 6, d, (i + 2) % 6, seconds / 3,
                                                                      2 * seconds / 3, p)) for i, p in enumerate(paths)]
    bg = [("u%04d-babble" % i, "wav-reverberate --shift-output=true --additive-signals='%s' --start-times='0,0,0' --snrs='19,15,13' "
           "%s - |" % (",".join("wav-reverberate --duration=%.1f \"%s/n%d.wav\" - |" % (seconds, d, (i + k) % 6) for k in range(3)), p))
          for i, p in enumerate(paths)]
    return rv, noise, bg


def cli_rates(d, paths, rv, seconds):
    import kaldi_io
    import torch
    from xvector_amd import augment, mfcc
    conf = os.path.join(ROOT, "tests", "golden", "mfcc.conf")
    clean = os.path.join(d, "clean.scp")
    open(clean, "w").write("".join("u%04d %s\n" % (i, p) for i, p in enumerate(paths)))
    aug_scp = os.path.join(d, "aug.scp")
    open(aug_scp, "w").write("".join("%s %s\n" % e for e in rv))
    audio_s = len(paths) * seconds
    lines = []
    for label, scp in (("clean", clean), ("reverb L=1 s", aug_scp)):
        c0 = time.perf_counter()
        subprocess.check_call([sys.executable, os.path.join(TWIN, "mfcc_vad.py"), "compute-mfcc-feats", "--config=" + conf,
                               "scp:" + scp, "ark,scp:%s/f.ark,%s/f.scp" % (d, d)], stdout=subprocess.DEVNULL,
                              stderr=subprocess.DEVNULL)
        c1 = time.perf_counter()
        lines.append("CLI compute-mfcc-feats %s, %d x %.0f s (%.2f h): %.2f s wall = %.0fx real time (RTF %.2e)" %
                     (label, len(paths), seconds, audio_s / 3600.0, c1 - c0, audio_s / (c1 - c0), (c1 - c0) / audio_s))
        print(lines[-1], flush=True)
    # the phases of the augmented run, in process
    opts = mfcc.MfccOptions().update(mfcc.read_config(conf))
    eng = mfcc.Mfcc(opts)
    aug = augment.Augmenter()
    eng.compute(["warm"], [np.zeros(16000, np.int16)])
    t0 = time.perf_counter()
    plan = aug.plan([(k, augment.parse_rx(rx)) for k, rx in rv])
    items = [augment.Pending(n, plan) for n in plan.top]
    t1 = time.perf_counter()
    x = torch.zeros(int(sum(p.M for p in items)), dtype=torch.int16, device="cuda")
    offs = np.concatenate([[0], np.cumsum([p.M for p in items])[:-1]]).astype(np.int64)
    aug.run(plan, x, offs)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    feats, _, _ = augment.mfcc_compute(eng, aug, [k for k, _ in rv], items)
    t3 = time.perf_counter()
    with kaldi_io.TableWriter(os.path.join(d, "p.ark"), os.path.join(d, "p.scp")) as tw:
        for (k, _), f in zip(rv, feats):
            kaldi_io.write_mat(tw, f, key=k)
    t4 = time.perf_counter()
    lines.append("  augmented, in-process phases: read + plan %.2f s, augment alone %.2f s, augment + MFCC (one pass, samples stay "
                 "on the device) %.2f s, write %.2f s" % (t1 - t0, t2 - t1, t3 - t2, t4 - t3))
    print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--utts", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=120.0)
    a = ap.parse_args()
    import logging
    from xvector_amd import hiplib
    hiplib.require_gpu()
    logging.getLogger("augment").setLevel(logging.ERROR)   # the synthetic RIRs clip ~0.2 % of samples: one warning per utterance
    d = tempfile.mkdtemp(prefix="augment_bench_")
    try:
        n = 8 if a.kernel_only else a.utts
        paths = make_inputs(d, n, a.seconds)
        rv, noise, bg = forms(d, paths, a.seconds)
        reps = 2 if a.kernel_only else 5
        for L in (2000, 4000, 8000, 16000):
            evaluate_rate(d, rv[L], "reverb L=%d (%.2f s)" % (L, L / float(FS)), reps)
        evaluate_rate(d, noise, "foreground noise x3", reps)
        evaluate_rate(d, bg, "background (music / babble) x3 nested --duration", reps)
        if not a.kernel_only:
            cli_rates(d, paths, rv[8000], a.seconds)
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
