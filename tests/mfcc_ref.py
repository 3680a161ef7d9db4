"""fp64 oracle of the MFCC + energy-VAD front-end, written from the restatement of Kaldi's algorithm and
sharing only the host-built tables (window, mel bank, lifter x DCT) with the device path.  The dither noise is restated here
exactly (Philox4x32-10 + Box-Muller in fp64), so dithered output is checked against the same noise."""
import numpy as np

FLT_EPSILON = 1.1920928955078125e-07
M32 = 0xFFFFFFFF


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Vectorised Philox4x32-10 on uint64 arrays holding 32-bit words."""
    c = [np.asarray(x, np.uint64) & M32 for x in (c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0 & M32), np.uint64(k1 & M32)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & M32, p1 & M32, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & M32, p0 & M32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & np.uint64(M32)
        k1 = (k1 + np.uint64(0xBB67AE85)) & np.uint64(M32)
    return c


def gauss(key, t, i):
    """N(0,1) of sample i of frame t of the utterance keyed ``key``: counter (i, t mod 2^32, t >> 32, 0)."""
    t = np.asarray(t, np.uint64)
    r = philox4x32_10(i, t & np.uint64(M32), t >> np.uint64(32), 0, key & M32, key >> 32)
    u1 = ((r[0] >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    u2 = (r[1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def frame_indices(opts, n):
    """[T, L] sample indices of every frame, reflected into [0, n)."""
    T = int(opts.num_frames(n))
    L = opts.frame_length_samples
    s = opts.first_sample(np.arange(T))[:, None] + np.arange(L)[None, :]
    while T and ((s < 0) | (s >= n)).any():
        s = np.where(s < 0, -s - 1, np.where(s >= n, 2 * n - 1 - s, s))
    return s


def mfcc(opts, tables, wave, key):
    """-> dict of float64 arrays: feats [T, C], logmel [T, B], mel [T, B], energy_raw [T] (sum of squares of the dithered frame),
    energy_dc [T] (after DC removal), power_sum [T] (sum over bins 0 .. N/2 - 1 of the power spectrum)."""
    wave = np.asarray(wave).astype(np.float64)
    n = wave.shape[0]
    idx = frame_indices(opts, n)
    T, L = idx.shape[0], opts.frame_length_samples
    N = opts.padded_length
    B, C = opts.num_mel_bins, opts.num_ceps
    x = wave[idx] if T else np.zeros((0, L))
    if opts.dither != 0 and T:
        x = x + opts.dither * gauss(key, np.arange(T)[:, None], np.arange(L)[None, :])
    energy_raw = (x * x).sum(axis=1)
    if opts.remove_dc_offset:
        x = x - x.mean(axis=1, keepdims=True)
    energy_dc = (x * x).sum(axis=1)
    log_e = np.log(np.maximum(energy_dc, FLT_EPSILON))
    p = opts.preemphasis_coefficient
    if p != 0:
        x = np.concatenate([x[:, :1] - p * x[:, :1], x[:, 1:] - p * x[:, :-1]], axis=1)
    x = x * tables.window.astype(np.float64)[None, :]
    if not opts.raw_energy:
        log_e = np.log(np.maximum((x * x).sum(axis=1), FLT_EPSILON))
    if opts.energy_floor > 0:
        log_e = np.maximum(log_e, np.log(opts.energy_floor))
    X = np.fft.rfft(x, n=N, axis=1)[:, :N // 2]
    P = X.real ** 2 + X.imag ** 2
    W = np.zeros((N // 2, B))
    for b in range(B):
        f, ln = int(tables.mel_first[b]), int(tables.mel_len[b])
        W[f:f + ln, b] = tables.mel_w[b, :ln]
    mel = P @ W
    logmel = np.log(np.maximum(mel, FLT_EPSILON))
    feats = logmel @ tables.lifter_dct.astype(np.float64).T
    if opts.use_energy:
        feats[:, 0] = log_e
    return dict(feats=feats.reshape(T, C), logmel=logmel.reshape(T, B), mel=mel.reshape(T, B), energy_raw=energy_raw,
                energy_dc=energy_dc, power_sum=P.sum(axis=1))


def vad(c0, vopts):
    """compute-vad on one utterance's c0 (float32 values, compared in fp64 against an fp64 threshold)."""
    c0 = np.asarray(c0, np.float32).astype(np.float64)
    T = c0.shape[0]
    if T == 0:
        return np.zeros(0, np.float32)
    thr = vopts.vad_energy_threshold + vopts.vad_energy_mean_scale * c0.sum() / T
    above = (c0 > thr).astype(np.int64)
    ctx = vopts.vad_frames_context
    cs = np.concatenate([[0], np.cumsum(above)])
    t = np.arange(T)
    lo, hi = np.maximum(t - ctx, 0), np.minimum(t + ctx, T - 1) + 1
    num, den = cs[hi] - cs[lo], hi - lo
    return (num.astype(np.float32) >= den.astype(np.float32) * np.float32(vopts.vad_proportion_threshold)).astype(np.float32)


def threshold(c0, vopts):
    c0 = np.asarray(c0, np.float32).astype(np.float64)
    return vopts.vad_energy_threshold + vopts.vad_energy_mean_scale * c0.sum() / max(c0.shape[0], 1)
