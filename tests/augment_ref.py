"""fp64 oracle of wav-reverberate, written from the restatement of Kaldi's featbin/wav-reverberate.cc and
feat/signal.cc.  It shares nothing with the device path: the window edges, offsets and lengths are re-derived here with numpy
fp32 scalars, the convolution is exact in fp64 (direct, or fp64 FFT for large products)."""
import numpy as np

F32 = np.float32


def conv(x, h):
    """Full linear convolution in fp64."""
    if len(x) * len(h) <= 5e7:
        return np.convolve(x, h)
    n = len(x) + len(h) - 1
    m = 1 << (n - 1).bit_length()
    return np.fft.irfft(np.fft.rfft(x, m) * np.fft.rfft(h, m), m)[:n]


def window(peak, L, fs):
    s = int(F32(peak) - F32(0.001) * F32(fs))
    e = int(F32(peak) + F32(0.05) * F32(fs))
    return max(0, s), min(L, e)


def reverberate(x, fs, rir=None, noises=(), snrs=(), start_times=(), shift_output=False, volume=0.0, duration=0.0,
                normalize_output=True):
    """x, rir, noises: int16 (one channel each).  -> dict of the scalars, ``y`` (fp64 waveform after mixing, before the level),
    ``pre`` (fp64 output before truncation), ``out`` (int16) and ``clipped``."""
    x = np.asarray(x, np.float64)
    N = len(x)
    assert N > 0 and len(noises) == len(snrs) == len(start_times)
    p0 = float(np.dot(x, x)) / N
    peak = 0
    if rir is not None:
        h = np.asarray(rir, np.float64) / 32768.0
        peak = int(np.argmax(h))
        s, e = window(peak, len(h), fs)
        early = conv(x, h[s:e])
        E = float(np.dot(early, early)) / len(early)
        y = conv(x, h)
    else:
        E, y = p0, x.copy()
    pn, scales = [], []
    for n, snr, t in zip(noises, snrs, start_times):
        n = np.asarray(n, np.float64)
        p = float(np.dot(n, n)) / len(n) if len(n) else 0.0              # an empty noise is silent
        sc = float(F32(np.sqrt(10.0 ** (-float(F32(snr)) / 10.0) * E / p))) if p > 0 else 0.0
        off = int(F32(t) * F32(fs))
        k = min(len(y) - off, len(n))
        if k > 0:
            y[off:off + k] += sc * n[:k]
        pn.append(p)
        scales.append(sc)
    p1 = float(np.dot(y, y)) / len(y)
    if volume > 0:
        level = float(F32(volume))
    elif normalize_output and p1 > 0:
        level = float(F32(np.sqrt(p0 / p1)))
    else:
        level = 1.0
    shift = peak if shift_output and rir is not None else 0
    M = int(F32(duration) * F32(fs)) if duration > 0 else N
    idx = shift + np.arange(M) % N
    pre = y[idx] * level
    t = np.trunc(pre)
    out = np.clip(t, -32768, 32767).astype(np.int16)
    clipped = int(np.count_nonzero((t < -32768) | (t > 32767)))
    return dict(P0=p0, E=E, P1=p1, level=level, noise_power=pn, noise_scale=scales, y=y, pre=pre, out=out, clipped=clipped,
                shift=shift, M=M, idx=idx)
