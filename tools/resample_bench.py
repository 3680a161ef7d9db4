"""Rates of the resampler: the kernel's bytes/s for 16 k -> 8 k and 44.1 k -> 8 k on about 2^26 input samples
(device events after warm-up; bytes = 2 per int16 input sample + 4 per fp32 output sample, the traffic the algorithm needs),
its share of one MFCC window's device time, and the stage-1 job (`mfcc_vad.py compute-mfcc-vad`) on 16 kHz files with
--allow-downsample against the SAME audio stored at 8 kHz without resampling (wall clock of the CLI, alternating the two).
    python tools/resample_bench.py [--kernel-only] [--files N] [--seconds S]"""
import argparse, os, shutil, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWIN = os.path.join(ROOT, "x-vector-kaldi-tf_amd", "local", "tf")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "x-vector-kaldi-tf_amd")); sys.path.insert(0, TWIN)
import numpy as np

HBM_TBS = 8.0          # MI355X HBM3E peak; 6.29 TB/s is what a float4 copy reaches (MI355X_MICROARCH.md)
CONF = os.path.join(ROOT, "tests", "golden", "mfcc.conf")
VCONF = os.path.join(ROOT, "tests", "golden", "vad.conf")
INNER = 10             # launches per timed interval


def _events(torch, fn, reps):
    fn(); fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / 1e3)
    return float(np.median(times)), float(min(times)), float(max(times))


def kernel_rate(fi, fo=8000, total=1 << 26, seconds=60.0, reps=7):
    import torch
    from xvector_amd import hiplib, mfcc, resample, synthetic
    n = int(fi * seconds)
    n_utts = max(1, total // n)
    base = torch.from_numpy(synthetic.speech_like_wave(n, fi, 1)).cuda()
    rng = np.random.default_rng(0)
    lens = (n - rng.integers(0, fi, n_utts)).astype(np.int64)
    pl = resample.plan(lens, [fi] * n_utts, fo)
    x = torch.empty(pl.in_total, dtype=torch.int16, device="cuda")
    for o, m in zip(pl.utt[0].tolist(), lens.tolist()):
        x[o:o + m] = base[:m]
    y = torch.empty(pl.out_total, dtype=torch.float32, device="cuda")
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    first, ntaps, w, tiles = cu(pl.first), cu(pl.ntaps), cu(pl.w), cu(pl.tiles)
    hiplib.resample(x, pl.utt, pl.tab, first, ntaps, w, tiles, y)          # once through the binding: its argument checks
    # timed through the raw entry point, INNER launches per pair of events: the binding's host work (checks, the upload of the
    # utterance table) would otherwise sit between the events as idle device time of the kernel's own size
    import ctypes
    lib, d_utt = hiplib.load(), cu(pl.utt)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    args = (ptr(x), 0, ptr(d_utt[0]), ptr(d_utt[1]), ptr(d_utt[2]), ptr(d_utt[3]), ptr(d_utt[4]), n_utts,
            pl.tab.ctypes.data_as(ctypes.c_void_p), len(pl.tab), ptr(first), ptr(ntaps), ptr(w), ptr(tiles), len(pl.tiles), ptr(y),
            hiplib._stream())

    def launches():
        for _ in range(INNER):
            assert lib.xv_resample_f32(*args) == 0
    t, lo, hi = (v / INNER for v in _events(torch, launches, reps))
    n_in, n_out = int(lens.sum()), int(pl.out_samples.sum())
    byts = 2 * n_in + 4 * n_out
    # the MFCC launch on the window the resampler just filled (the recipe's 8 kHz config), for the share of device time
    opts = mfcc.MfccOptions().update(mfcc.read_config(CONF))
    line = ("%d -> %d Hz: %d utts, %d input samples (2^%.2f), %d tiles: resample kernel %.3f ms (min %.3f, max %.3f) = %.1f GB/s "
            "(%.1f %% of %.0f TB/s HBM peak) for %d B; %.3g input samples/s" %
            (fi, fo, n_utts, n_in, np.log2(n_in), len(pl.tiles), t * 1e3, lo * 1e3, hi * 1e3, byts / t / 1e9,
             100 * byts / t / (HBM_TBS * 1e12), HBM_TBS, byts, n_in / t))
    if fo == opts.sample_frequency:
        tb = mfcc.MfccTables(opts).to_device("cuda:0")
        T = opts.num_frames(pl.out_samples).astype(np.int64)
        row0 = np.concatenate([[0], np.cumsum(T)[:-1]]).astype(np.int64)
        rows = int(T.sum())
        feats = torch.empty((rows, opts.num_ceps), dtype=torch.float32, device="cuda")
        keys = cu(np.array([mfcc.dither_key("utt%06d" % u) for u in range(n_utts)], np.uint64).view(np.int64))
        d_off, d_ns, d_row0 = cu(pl.utt[2]), cu(pl.utt[3]), cu(row0)
        tm, _, _ = _events(torch, lambda: hiplib.mfcc(y, d_off, d_ns, d_row0, keys, rows, tb, opts, feats), reps)
        line += "; the MFCC launch on its output: %.3f ms, so resampling is %.1f %% of the window's two launches" % (
            tm * 1e3, 100 * t / (t + tm))
    print(line, flush=True)
    return line


def job_rates(n_files, seconds, rounds=3):
    """The CLI on n_files of `seconds` each: stored at 16 kHz and read with --allow-downsample, and the same audio (the 8 kHz
    wave the 16 kHz file was made from by doubling the rate with a 2x repeat) stored at 8 kHz: what the parent commit could do."""
    from xvector_amd import mfcc, synthetic
    d = tempfile.mkdtemp(prefix="resample_bench_")
    base = synthetic.speech_like_wave(int(8000 * seconds), 8000, 2)
    for rate, tag in ((8000, "8k"), (16000, "16k")):
        lines = []
        for i in range(n_files):
            w = np.roll(base, 7919 * i)
            p = os.path.join(d, "%s_u%04d.wav" % (tag, i))
            with open(p, "wb") as f:
                f.write(mfcc.wav_bytes(w if rate == 8000 else np.repeat(w, 2), rate))
            lines.append("spk%02d-u%04d %s" % (i % 50, i, p))
        with open(os.path.join(d, "wav_%s.scp" % tag), "w") as f:
            f.write("\n".join(lines) + "\n")

    def run(tag, *flags):
        t0 = time.perf_counter()
        subprocess.check_call([sys.executable, os.path.join(TWIN, "mfcc_vad.py"), "compute-mfcc-vad", "--config=" + CONF,
                               "--vad-config=" + VCONF] + list(flags) +
                              ["scp:" + os.path.join(d, "wav_%s.scp" % tag), "ark,scp:%s/f_%s.ark,%s/f_%s.scp" % (d, tag, d, tag),
                               "ark,scp:%s/v_%s.ark,%s/v_%s.scp" % (d, tag, d, tag)], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return time.perf_counter() - t0

    run("8k")                                      # warm the file cache and the code objects
    t8, t16 = [], []
    for _ in range(rounds):                        # alternating, as other work shares the host
        t8.append(run("8k"))
        t16.append(run("16k", "--allow-downsample=true"))
    rows8 = sum(1 for _ in open(os.path.join(d, "f_8k.scp")))
    rows16 = sum(1 for _ in open(os.path.join(d, "f_16k.scp")))
    audio_s = n_files * seconds
    line = ("CLI compute-mfcc-vad, %d files x %.0f s (%.2f h of audio), wall clock of %d alternating runs: stored at 8 kHz %s s "
            "(median %.2f); stored at 16 kHz with --allow-downsample %s s (median %.2f): %.2fx; %d / %d utterances written" %
            (n_files, seconds, audio_s / 3600.0, rounds, ", ".join("%.2f" % t for t in t8), np.median(t8),
             ", ".join("%.2f" % t for t in t16), np.median(t16), np.median(t16) / np.median(t8), rows8, rows16))
    print(line, flush=True)
    shutil.rmtree(d, ignore_errors=True)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--files", type=int, default=400)
    ap.add_argument("--seconds", type=float, default=60.0)
    a = ap.parse_args()
    from xvector_amd import hiplib
    hiplib.require_gpu()
    kernel_rate(16000)
    kernel_rate(44100)
    if not a.kernel_only:
        job_rates(a.files, a.seconds)


if __name__ == "__main__":
    main()
