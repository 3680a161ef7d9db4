"""Rates of the native SPHERE route: (a) the decode kernel's bytes/s on two-channel mu-law utterances of about
60 s (device events after warm-up; bytes = the raw bytes the utterances' tiles read + the samples written), next to the MFCC
launch on the window it filled; (b) the stage-1 job (`mfcc_vad.py compute-mfcc-vad`, recipe configs) on the SAME audio three
ways, alternating after a warm-up: as WAV paths (what the parent commit can do), as `cat x.wav |` pipes (one shell and one
process per utterance: a lower bound on what an `sph2pipe ... |` line costs) and as `sph2pipe -f wav -p -c N x.sph |` lines on
two-channel mu-law SPHERE files read natively (no sph2pipe program is needed, or started).
    python tools/sphere_bench.py [--kernel-only] [--files N] [--seconds S]"""
import argparse, ctypes, os, shutil, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWIN = os.path.join(ROOT, "x-vector-kaldi-tf_amd", "local", "tf")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "x-vector-kaldi-tf_amd")); sys.path.insert(0, TWIN)
import numpy as np

HBM_TBS = 8.0          # MI355X HBM3E peak; 6.29 TB/s is what a float4 copy reaches
COPY_TBS = 6.29
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


def lin2ulaw(x):
    """int16 -> the mu-law codes with the nearest expansion (a search over sphere.ULAW_TABLE)."""
    from xvector_amd import sphere
    tab = sphere.ULAW_TABLE.astype(np.int64)
    order = np.argsort(tab, kind="stable")
    vals = tab[order]
    x = np.asarray(x, np.int64)
    i = np.clip(np.searchsorted(vals, x), 1, 255)
    return order[np.where(np.abs(vals[i - 1] - x) <= np.abs(vals[i] - x), i - 1, i)].astype(np.uint8)


def sph_bytes(codes, rate):
    """[channels, samples] uint8 mu-law codes -> a SPHERE file with a 1024-byte header."""
    nch, n = codes.shape
    text = ("NIST_1A\n   1024\nsample_rate -i %d\nchannel_count -i %d\nsample_n_bytes -i 1\nsample_byte_format -s1 1\n"
            "sample_coding -s4 ulaw\nsample_count -i %d\nend_head\n" % (rate, nch, n))
    return text.encode() + b" " * (1024 - len(text)) + np.ascontiguousarray(codes.T).tobytes()


def kernel_rate(fmt, total=1 << 26, seconds=60.0, rate=8000, reps=7):
    """Both sides of two-channel mu-law files of ~`seconds` each, `total` samples in all, one launch; fmt 0 int16, 1 fp32 out."""
    import torch
    from xvector_amd import hiplib, mfcc, sphere, synthetic
    n = int(rate * seconds)
    n_files = max(1, total // (2 * n))
    rng = np.random.default_rng(0)
    lens = (n - rng.integers(0, rate, n_files)).astype(np.int64)
    base = np.stack([lin2ulaw(synthetic.speech_like_wave(n, rate, s)) for s in (1, 2)])
    raw_parts, raw_off, pos = [], [], 0
    for m in lens.tolist():
        raw_off.append(pos)
        reg = np.ascontiguousarray(base[:, :m].T).reshape(-1)
        raw_parts.append(reg)
        pad = -len(reg) % 16
        raw_parts.append(np.zeros(pad, np.uint8))
        pos += len(reg) + pad
    raw = torch.from_numpy(np.concatenate(raw_parts)).cuda()
    ns = np.repeat(lens, 2)
    off = np.concatenate([[0], np.cumsum(ns[:-1])]).astype(np.int64)
    utt = np.zeros((len(ns), sphere.DEC_FIELDS), np.int64)
    utt[:, sphere.RAW_OFF], utt[:, sphere.N_], utt[:, sphere.STRIDE] = np.repeat(raw_off, 2), ns, 2
    utt[:, sphere.CH_OFF], utt[:, sphere.CODING], utt[:, sphere.OUT_OFF] = np.tile([0, 1], n_files), sphere.ULAW, off
    tiles_h = sphere.tile_list(ns, off)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    tiles = cu(tiles_h)
    x = torch.empty(int(ns.sum()), dtype=torch.int16 if fmt == 0 else torch.float32, device="cuda")
    hiplib.wave_decode(raw, utt, tiles, x, fmt)                 # once through the binding: its argument checks
    got = x[:1000].cpu().numpy()
    assert np.array_equal(got, sphere.ULAW_TABLE[base[0, :1000]].astype(got.dtype))
    # timed through the raw entry point, INNER launches per pair of events (the binding's host work would sit between them)
    lib, d_utt = hiplib.load(), cu(utt)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    args = (ptr(raw), int(raw.numel()), ptr(d_utt), len(ns), ptr(tiles), len(tiles_h), ptr(x), fmt, hiplib._stream())

    def launches():
        for _ in range(INNER):
            assert lib.xv_wave_decode(*args) == 0
    t, lo, hi = (v / INNER for v in _events(torch, launches, reps))
    n_out = int(ns.sum())
    # each side reads its file's whole region (both channels lie in every 16 bytes), so the launch reads 2 bytes per sample
    byts = 2 * n_out + (2 if fmt == 0 else 4) * n_out
    line = ("mu-law, 2 channels, both sides, %s out: %d utts, %d samples (2^%.2f), %d tiles: decode kernel %.3f ms (min %.3f, max "
            "%.3f) = %.2f TB/s for %d B read + written (%.1f %% of the %.0f TB/s HBM peak, %.1f %% of the %.2f TB/s of a float4 "
            "copy); %.3g samples/s" % ("int16" if fmt == 0 else "fp32", len(ns), n_out, np.log2(n_out), len(tiles_h), t * 1e3,
                                        lo * 1e3, hi * 1e3, byts / t / 1e12, byts, 100 * byts / t / (HBM_TBS * 1e12), HBM_TBS,
                                        100 * byts / t / (COPY_TBS * 1e12), COPY_TBS, n_out / t))
    opts = mfcc.MfccOptions().update(mfcc.read_config(CONF))
    tb = mfcc.MfccTables(opts).to_device("cuda:0")
    T = opts.num_frames(ns).astype(np.int64)
    row0 = np.concatenate([[0], np.cumsum(T)[:-1]]).astype(np.int64)
    rows = int(T.sum())
    feats = torch.empty((rows, opts.num_ceps), dtype=torch.float32, device="cuda")
    keys = cu(np.array([mfcc.dither_key("utt%06d" % u) for u in range(len(ns))], np.uint64).view(np.int64))
    d_off, d_ns, d_row0 = cu(off), cu(ns), cu(row0)
    tm, _, _ = _events(torch, lambda: hiplib.mfcc(x, d_off, d_ns, d_row0, keys, rows, tb, opts, feats), reps)
    line += "; the MFCC launch on its output: %.3f ms, so decoding is %.1f %% of the window's two launches" % (tm * 1e3, 100 * t / (t + tm))
    print(line, flush=True)
    return line


def job_rates(n_utts, seconds, rounds=3):
    """The CLI on n_utts utterances of `seconds` each, three routes over the same samples."""
    from xvector_amd import mfcc, sphere, synthetic
    d = tempfile.mkdtemp(prefix="sphere_bench_")
    n = int(8000 * seconds)
    codes = np.stack([lin2ulaw(synthetic.speech_like_wave(n, 8000, s)) for s in (2, 3)])
    wav, pipe, sph = [], [], []
    for i in range(n_utts // 2):
        c = np.roll(codes, 7919 * i, axis=1)
        sp = os.path.join(d, "f%04d.sph" % i)
        with open(sp, "wb") as f:
            f.write(sph_bytes(c, 8000))
        for side in (0, 1):
            key = "spk%02d-f%04d-%s" % (i % 50, i, "AB"[side])
            wp = os.path.join(d, "f%04d_%s.wav" % (i, "AB"[side]))
            with open(wp, "wb") as f:
                f.write(mfcc.wav_bytes(sphere.ULAW_TABLE[c[side]], 8000))
            wav.append("%s %s" % (key, wp))
            pipe.append("%s cat %s |" % (key, wp))
            sph.append("%s sph2pipe -f wav -p -c %d %s |" % (key, side + 1, sp))
    for tag, lines in (("wav", wav), ("pipe", pipe), ("sph", sph)):
        with open(os.path.join(d, "wav_%s.scp" % tag), "w") as f:
            f.write("\n".join(lines) + "\n")

    def run(tag):
        t0 = time.perf_counter()
        subprocess.check_call([sys.executable, os.path.join(TWIN, "mfcc_vad.py"), "compute-mfcc-vad", "--config=" + CONF,
                               "--vad-config=" + VCONF, "scp:" + os.path.join(d, "wav_%s.scp" % tag),
                               "ark,scp:%s/f_%s.ark,%s/f_%s.scp" % (d, tag, d, tag), "ark,scp:%s/v_%s.ark,%s/v_%s.scp" % (d, tag, d, tag)],
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return time.perf_counter() - t0

    tags = ("wav", "pipe", "sph")
    for tag in tags:                               # warm the file cache and the code objects
        run(tag)
    times = {tag: [] for tag in tags}
    for _ in range(rounds):                        # alternating, as other work shares the host
        for tag in tags:
            times[tag].append(run(tag))
    same = all(open(os.path.join(d, "f_wav.ark"), "rb").read() == open(os.path.join(d, "f_%s.ark" % t), "rb").read() for t in tags[1:])
    med = {t: float(np.median(times[t])) for t in tags}
    spread = max(max(v) - min(v) for v in times.values())
    line = ("CLI compute-mfcc-vad, %d utterances x %.0f s (%.2f h of audio), wall clock of %d alternating runs after a warm-up: WAV "
            "paths %s s (median %.2f); `cat x.wav |` pipes %s s (median %.2f); native SPHERE mu-law (2 channels per file) %s s "
            "(median %.2f); native / WAV %.2fx, pipes / native %.2fx, largest spread within a route %.2f s; feature arks "
            "byte-identical across the three: %s" %
            (2 * (n_utts // 2), seconds, 2 * (n_utts // 2) * seconds / 3600.0, rounds, ", ".join("%.2f" % t for t in times["wav"]),
             med["wav"], ", ".join("%.2f" % t for t in times["pipe"]), med["pipe"], ", ".join("%.2f" % t for t in times["sph"]),
             med["sph"], med["sph"] / med["wav"], med["pipe"] / med["sph"], spread, same))
    print(line, flush=True)
    shutil.rmtree(d, ignore_errors=True)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--files", type=int, default=200, help="utterances of the stage-1 job (two per SPHERE file)")
    ap.add_argument("--seconds", type=float, default=60.0)
    a = ap.parse_args()
    from xvector_amd import hiplib
    hiplib.require_gpu()
    kernel_rate(0)
    kernel_rate(1)
    if not a.kernel_only:
        job_rates(a.files, a.seconds)


if __name__ == "__main__":
    main()
