"""Rates of the stage-1 front-end: the MFCC kernel in frames/s for the recipe's 8 kHz config and 16 kHz Kaldi
defaults on user-sized batches (minutes of audio per utterance, thousands of utterances; device events after warm-up) with
achieved bytes/s and flop/s from shape-derived counts, the VAD kernel, and the `mfcc_vad.py compute-mfcc-vad` CLI on a directory
of synthetic WAV files (wall clock, real-time factor, split into read / upload + compute / write).
    python tools/mfcc_bench.py [--kernel-only] [--utts N] [--seconds S]
(--kernel-only: only the kernel timings, at a smaller size: the form run under rocprofv3 --kernel-trace --stats)."""
import argparse, os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWIN = os.path.join(ROOT, "x-vector-kaldi-tf_amd", "local", "tf")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "x-vector-kaldi-tf_amd")); sys.path.insert(0, TWIN)
import numpy as np

HBM_TBS = 8.0          # MI355X HBM3E peak
FP32_TFLOPS = 157.3    # MI355X vector fp32 peak (MI355X_MICROARCH.md)


def per_frame_counts(opts, tables, logmel):
    """(flop, HBM bytes) of one frame: the DSP arithmetic the algorithm needs, and the bytes that must cross HBM (each input
    sample once -- frames overlap, the repeats are cache hits -- plus the rows written)."""
    L, N = opts.frame_length_samples, opts.padded_length
    H = N // 2
    B, C = opts.num_mel_bins, opts.num_ceps
    flop = 3 * L                                  # dither add, DC sum + subtract
    flop += 2 * L + 3 * L                         # energy, pre-emphasis + window
    flop += 5 * H * int(np.log2(H))               # complex radix-2 FFT of N/2 points
    flop += 10 * H + 3 * H                        # split step, power
    flop += 2 * int(tables.mel_len.sum()) + B     # mel bank, log
    flop += 2 * B * C                             # lifter x DCT
    flop += L * 25 if opts.dither else 0          # Philox4x32-10 + Box-Muller (integer ops counted as ops)
    byts = 2 * opts.frame_shift_samples + 4 * C + (4 * B if logmel else 0)
    return flop, byts


def kernel_rates(fs, n_utts, seconds, reps=5):
    import torch
    from xvector_amd import hiplib, mfcc, synthetic
    opts = mfcc.MfccOptions() if fs == 16000 else mfcc.MfccOptions().update(
        mfcc.read_config(os.path.join(ROOT, "tests", "golden", "mfcc.conf")))
    tb = mfcc.MfccTables(opts)
    dev = tb.to_device("cuda:0")
    base = synthetic.speech_like_wave(int(fs * 60), fs, 1)
    rng = np.random.default_rng(0)
    n = int(fs * seconds)
    ns = (n - rng.integers(0, fs, n_utts)).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(ns)[:-1]]).astype(np.int64)
    T = opts.num_frames(ns).astype(np.int64)
    row0 = np.concatenate([[0], np.cumsum(T)[:-1]]).astype(np.int64)
    rows = int(T.sum())
    x = torch.empty(int(ns.sum()), dtype=torch.int16, device="cuda")
    tile = torch.from_numpy(base).cuda()
    for u in range(n_utts):                        # every utterance a rotated copy of the same minute (device-side fill)
        s = int(off[u])
        r = int(rng.integers(0, len(base)))
        left = int(ns[u])
        while left > 0:
            k = min(left, len(base) - r)
            x[s:s + k] = tile[r:r + k]
            s += k; left -= k; r = 0
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    d_off, d_ns, d_row0 = cu(off), cu(ns), cu(row0)
    d_key = cu(np.array([mfcc.dither_key("utt%06d" % u) for u in range(n_utts)], np.uint64).view(np.int64))
    feats = torch.empty((rows, opts.num_ceps), dtype=torch.float32, device="cuda")
    vad = torch.empty(rows, dtype=torch.float32, device="cuda")
    vopts = mfcc.VadOptions(vad_energy_threshold=5.5, vad_frames_context=2, vad_proportion_threshold=0.12)
    d_T = cu(T.astype(np.int32))
    out = {}
    for label, fn in (("mfcc", lambda: hiplib.mfcc(x, d_off, d_ns, d_row0, d_key, rows, dev, opts, feats)),
                      ("vad", lambda: hiplib.vad_energy(feats, d_row0, d_T, vopts, vad))):
        fn(); fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) / 1e3)
        out[label] = float(np.median(times))
    flop, byts = per_frame_counts(opts, tb, False)
    t = out["mfcc"]
    fr = rows / t
    line = ("%d Hz: %d utts x %.0f s (%d frames, %.2f h of audio): mfcc kernel %.2f ms = %.3g frames/s (%.0fx real time); "
            "%.1f GB/s (%.2f %% of %.0f TB/s HBM), %.2f Tflop/s (%.2f %% of %.1f fp32); vad kernel %.3f ms = %.3g frames/s" %
            (fs, n_utts, seconds, rows, ns.sum() / fs / 3600.0, t * 1e3, fr, ns.sum() / fs / t, fr * byts / 1e9,
             100 * fr * byts / (HBM_TBS * 1e12), HBM_TBS, fr * flop / 1e12, 100 * fr * flop / (FP32_TFLOPS * 1e12), FP32_TFLOPS,
             out["vad"] * 1e3, rows / out["vad"]))
    print(line, flush=True)
    print("  per frame: %d flop, %d HBM bytes (%.1f flop/B)" % (flop, byts, flop / float(byts)), flush=True)
    return line


def cli_rates(n_files, seconds):
    from xvector_amd import mfcc, synthetic
    import kaldi_io
    d = tempfile.mkdtemp(prefix="mfcc_bench_")
    base = synthetic.speech_like_wave(8000 * 60, 8000, 2)
    lines = []
    for i in range(n_files):
        w = np.roll(base, 7919 * i)[:int(8000 * seconds)] if seconds <= 60 else np.tile(np.roll(base, 7919 * i), int(seconds // 60) + 1)[:int(8000 * seconds)]
        p = os.path.join(d, "u%04d.wav" % i)
        open(p, "wb").write(mfcc.wav_bytes(w, 8000))
        lines.append("spk%02d-u%04d %s" % (i % 50, i, p))
    open(os.path.join(d, "wav.scp"), "w").write("\n".join(lines) + "\n")
    audio_s = n_files * seconds
    conf = os.path.join(ROOT, "tests", "golden", "mfcc.conf")
    vconf = os.path.join(ROOT, "tests", "golden", "vad.conf")
    # the phases, in process
    opts = mfcc.MfccOptions().update(mfcc.read_config(conf))
    vopts = mfcc.VadOptions().update(mfcc.read_config(vconf))
    eng = mfcc.Mfcc(opts, vopts)
    eng.compute(["warm"], [base[:80000]])
    t0 = time.perf_counter()
    items = [(k, mfcc.select_channel(k, *mfcc.load_wav(k, rx), opts)) for k, rx in mfcc.read_wav_scp(os.path.join(d, "wav.scp"))]
    t1 = time.perf_counter()
    feats, vads, _ = eng.compute([k for k, _ in items], [w for _, w in items])
    t2 = time.perf_counter()
    with kaldi_io.TableWriter(os.path.join(d, "f.ark"), os.path.join(d, "f.scp")) as tw, \
            kaldi_io.TableWriter(os.path.join(d, "v.ark"), os.path.join(d, "v.scp")) as tv:
        for (k, _), f, v in zip(items, feats, vads):
            kaldi_io.write_mat(tw, f, key=k)
            kaldi_io.write_vec_flt(tv, v, key=k)
    t3 = time.perf_counter()
    # the CLI as a user runs it (process start and torch import included)
    c0 = time.perf_counter()
    subprocess.check_call([sys.executable, os.path.join(TWIN, "mfcc_vad.py"), "compute-mfcc-vad", "--config=" + conf,
                           "--vad-config=" + vconf, "scp:" + os.path.join(d, "wav.scp"), "ark,scp:%s/g.ark,%s/g.scp" % (d, d),
                           "ark,scp:%s/w.ark,%s/w.scp" % (d, d)], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    c1 = time.perf_counter()
    line = ("CLI compute-mfcc-vad, %d WAV files x %.0f s (%.2f h of 8 kHz audio): %.2f s wall = %.0fx real time (RTF %.2e); "
            "in-process phases: read %.2f s, upload + compute + download %.2f s, write %.2f s" %
            (n_files, seconds, audio_s / 3600.0, c1 - c0, audio_s / (c1 - c0), (c1 - c0) / audio_s, t1 - t0, t2 - t1, t3 - t2))
    print(line, flush=True)
    import shutil
    shutil.rmtree(d, ignore_errors=True)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--utts", type=int, default=2000)
    ap.add_argument("--seconds", type=float, default=120.0)
    a = ap.parse_args()
    from xvector_amd import hiplib
    hiplib.require_gpu()
    if a.kernel_only:
        kernel_rates(8000, 200, 60.0, reps=3)
        kernel_rates(16000, 100, 60.0, reps=3)
        return
    kernel_rates(8000, a.utts, a.seconds)
    kernel_rates(16000, a.utts // 2, a.seconds)
    cli_rates(400, 60.0)


if __name__ == "__main__":
    main()
