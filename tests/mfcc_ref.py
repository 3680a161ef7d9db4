"""fp64 oracle of the MFCC + energy-VAD front-end, written from the restatement of Kaldi's algorithm.

Two links carry the independence of the GPU comparisons.  ``mfcc`` computes with the product's own fp32 tables (window, sparse
mel bank, lifter x DCT: exactly what the device reads), so the kernel is pinned on the GPU against the oracle over those
tables; the tables themselves are pinned on the CPU (tests/test_mfcc_cpu.py) against ``window64`` / ``mel_dense64`` /
``lifter_dct64`` / ``twiddle64`` below, which are written from the definitions of §8.6 in fp64, take plain numbers and import
nothing of the product.  The dither noise is restated here exactly (Philox4x32-10 + Box-Muller in fp64), so dithered output is
checked against the same noise."""
import math

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


def window64(window_type, L, blackman_coeff=0.42):
    """The analysis window of L samples from its definition, fp64: with c_i = cos(2 pi i / (L - 1)), hanning 1/2 - c/2, hamming
    0.54 - 0.46 c, povey hanning^0.85, sine sin(pi i / (L - 1)), rectangular 1, blackman b - c/2 + (1/2 - b) cos(4 pi i / (L - 1))."""
    w = np.empty(L, np.float64)
    for i in range(L):
        x = i / float(L - 1)
        if window_type == "hanning":
            w[i] = 0.5 - 0.5 * math.cos(2.0 * math.pi * x)
        elif window_type == "hamming":
            w[i] = 0.54 - 0.46 * math.cos(2.0 * math.pi * x)
        elif window_type == "povey":
            w[i] = (0.5 - 0.5 * math.cos(2.0 * math.pi * x)) ** 0.85
        elif window_type == "sine":
            w[i] = math.sin(math.pi * x)
        elif window_type == "rectangular":
            w[i] = 1.0
        elif window_type == "blackman":
            w[i] = blackman_coeff - 0.5 * math.cos(2.0 * math.pi * x) + (0.5 - blackman_coeff) * math.cos(4.0 * math.pi * x)
        else:
            raise ValueError(window_type)
    return w


def mel64(f):
    return 1127.0 * math.log(1.0 + f / 700.0)


def mel_range64(fs, low, high):
    """(mel(low), mel(high)); high <= 0 counts down from the Nyquist frequency."""
    return mel64(low), mel64(high if high > 0 else 0.5 * fs + high)


def mel_dense64(fs, N, B, low, high):
    """The dense [N/2, B] mel weight matrix from the definition, fp64: FFT bin i (the Nyquist bin N/2 is never used) lies at
    m = mel(i fs / N); band b spans l, c, r = mel(low) + {b, b+1, b+2} delta, delta = (mel(high) - mel(low)) / (B + 1), and
    weighs the bin max(0, min((m - l) / (c - l), (r - m) / (r - c)))."""
    mlo, mhi = mel_range64(fs, low, high)
    delta = (mhi - mlo) / (B + 1)
    m = np.array([mel64(i * float(fs) / N) for i in range(N // 2)], np.float64)[:, None]
    b = np.arange(B, dtype=np.float64)[None, :]
    l, c, r = mlo + b * delta, mlo + (b + 1.0) * delta, mlo + (b + 2.0) * delta
    return np.maximum(0.0, np.minimum((m - l) / (c - l), (r - m) / (r - c)))


def dct64(B, C):
    """Rows 0 .. C - 1 of the orthonormal DCT-II of size B: row 0 is sqrt(1/B), row k sqrt(2/B) cos(pi k (j + 1/2) / B).  The
    angle is pi k (2j + 1) / 2B with the integer k (2j + 1) taken mod 4B (a whole turn), so an fp64 angle is never larger than
    2 pi and an entry that is 0 by the definition evaluates to < 1e-16, not to the 1e-14 that rounding an angle near 400 leaves."""
    d = np.empty((C, B), np.float64)
    for k in range(C):
        for j in range(B):
            turn = (k * (2 * j + 1)) % (4 * B)
            d[k, j] = math.sqrt(1.0 / B) if k == 0 else math.sqrt(2.0 / B) * math.cos(math.pi * turn / (2 * B))
    return d


def lifter64(C, Q):
    """The cepstral lifter 1 + Q/2 sin(pi k / Q); Q = 0: none."""
    return np.array([1.0 + 0.5 * Q * math.sin(math.pi * k / Q) if Q != 0 else 1.0 for k in range(C)], np.float64)


def lifter_dct64(B, C, Q):
    return lifter64(C, Q)[:, None] * dct64(B, C)


def twiddle64(N):
    """exp(-2 pi i k / N), k < N/2, as [N/2, 2] (re, im)."""
    return np.array([[math.cos(2.0 * math.pi * k / N), -math.sin(2.0 * math.pi * k / N)] for k in range(N // 2)], np.float64)


def half_ulp32(x):
    """Half an fp32 ulp of the fp64 values x (normal range): |x| in [2^(e-1), 2^e) has ulp 2^(e-24); 0 for x = 0.  What one
    rounding of x to fp32 may move it by."""
    x = np.asarray(x, np.float64)
    _, e = np.frexp(x)
    return np.where(x == 0, 0.0, 0.5 * np.ldexp(1.0, e - 24))


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
