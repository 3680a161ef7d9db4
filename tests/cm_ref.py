"""NumPy restatement of the CompressedMatrix encoding of include/xvector_hip.h, one operation of the header's
text per line: ``np.float32`` for every intermediate, ``astype(np.float64)`` where the text shows ``(double)``, ``np.sort`` for
the order statistics.  The GPU encoder (csrc/xv_compress.hip) is held to these bytes; the readers are held to the error bounds
on what it encodes.

Of a zero extreme the sign is fixed as the kernel's integer-key order fixes it (-0.0 for the minimum, +0.0 for the maximum when
both zeros occur): ``np.min`` / ``np.max`` leave that to the order of the reduction.  Only the sign bit of the header's ``gmin``
depends on it, no other byte does.
"""
import struct

import numpy as np

f32 = np.float32
U16_STEP = f32(1.52590218966964e-05)


def payload_bytes(rows, cols):
    if rows <= 0:
        return 0
    return 16 + (8 * cols + rows * cols if rows > 8 else 2 * rows * cols)


def global_range(m):
    """(gmin, grange) as float32."""
    gmin, gmax = f32(m.min()), f32(m.max())
    zeros = m == 0
    if gmin == 0 and np.any(zeros & np.signbit(m)):
        gmin = f32(-0.0)
    if gmax == 0 and np.any(zeros & ~np.signbit(m)):
        gmax = f32(0.0)
    if gmax == gmin:
        gmax = f32(np.float64(gmin) + (np.float64(1.0) + np.abs(np.float64(gmin))))
    return gmin, f32(gmax - gmin)


def to_int(d):
    """(int)trunc(d); INT_MIN for a NaN, an infinity or a value outside int (the header's rule, the x86 conversion)."""
    with np.errstate(all="ignore"):
        ok = np.abs(d) < 2147483648.0
        return np.where(ok, np.trunc(np.where(ok, d, 0.0)), -2147483648.0).astype(np.int64)


def u16(v, gmin, grange):
    f = ((np.asarray(v, f32) - gmin) / grange).astype(f32)
    f = np.minimum(np.maximum(f, f32(0)), f32(1))
    s = (f * f32(65535.0)).astype(f32)
    return to_int(s.astype(np.float64) + 0.499)


def from_u16(q, gmin, grange):
    step = f32(grange * U16_STEP)
    d = (step * np.asarray(q).astype(f32)).astype(f32)
    return (gmin + d).astype(f32)


def percentiles(m, gmin, grange):
    """[C, 4] int64: the four uint16 of every column."""
    T = m.shape[0]
    s = np.sort(m, axis=0)
    q = T // 4
    p0 = np.minimum(u16(s[0], gmin, grange), 65532)
    p25 = np.minimum(np.maximum(u16(s[q], gmin, grange), p0 + 1), 65533)
    p75 = np.minimum(np.maximum(u16(s[3 * q], gmin, grange), p25 + 1), 65534)
    p100 = np.maximum(u16(s[T - 1], gmin, grange), p75 + 1)
    return np.stack([p0, p25, p75, p100], axis=1)


def _segment(v, lo, hi, scale, base, bmin, bmax):
    f = (((v - lo) / (hi - lo)).astype(f32) * f32(scale)).astype(f32)
    return np.clip(base + to_int(f.astype(np.float64) + 0.5), bmin, bmax)


def encode(m):
    """-> (token, payload): b"CM " or b"CM2 " and the bytes that follow it in a record.  ``m``: finite float32 [T >= 1, C]."""
    m = np.ascontiguousarray(m, f32)
    T, C = m.shape
    assert T >= 1 and np.all(np.isfinite(m))
    gmin, grange = global_range(m)
    head = struct.pack("<ffii", gmin, grange, T, C)
    if T <= 8:
        return b"CM2 ", head + u16(m, gmin, grange).astype("<u2").tobytes()
    pct = percentiles(m, gmin, grange)
    P = from_u16(pct, gmin, grange)                       # [C, 4]
    P0, P25, P75, P100 = (P[None, :, i] for i in range(4))
    with np.errstate(all="ignore"):
        lo = _segment(m, P0, P25, 64.0, 0, 0, 64)
        mid = _segment(m, P25, P75, 128.0, 64, 64, 192)
        hi = _segment(m, P75, P100, 63.0, 192, 192, 255)
    b = np.where(m < P25, lo, np.where(m < P75, mid, hi)).astype(np.uint8)
    return b"CM ", head + pct.astype("<u2").tobytes() + np.ascontiguousarray(b.T).tobytes()


def record(key, m):
    token, payload = encode(m)
    return key.encode() + b" \0B" + token + payload


def bounds(m, payload, token):
    """Per-element decode error bound [T, C] (float64) of the payload of ``m``: for "CM " the half-step of the segment the VALUE
    lies in ((P25 - P0) / 128, (P75 - P25) / 256 or (P100 - P75) / 126) plus ONE 16-bit step (grange / 65535) plus 8 ulp of
    max(|gmin|, |gmax|, grange); for "CM2 " 0.501 of a 16-bit step plus 4 ulp.  (Not for a subnormal grange: the 16-bit step
    itself is then a rounded subnormal, and 65535 of them no longer add up to grange.)"""
    gmin, grange = np.frombuffer(payload[:8], "<f4")
    T, C = (int(v) for v in np.frombuffer(payload[8:16], "<i4"))
    gmin64, grange64 = float(gmin), float(grange)
    step = grange64 / 65535.0
    ulp = float(np.spacing(f32(max(abs(gmin64), abs(gmin64 + grange64), grange64))))
    if token == b"CM2 ":
        return np.full((T, C), 0.501 * step + 4 * ulp)
    pct = np.frombuffer(payload[16:16 + 8 * C], "<u2").reshape(C, 4).astype(np.int64)
    P = from_u16(pct, gmin, grange)
    P64 = P.astype(np.float64)
    half = np.where(m < P[None, :, 1], (P64[:, 1] - P64[:, 0])[None] / 128.0,
                    np.where(m < P[None, :, 2], (P64[:, 2] - P64[:, 1])[None] / 256.0, (P64[:, 3] - P64[:, 2])[None] / 126.0))
    return half + step + 8 * ulp


def cases(rng, T, C):
    """name -> float32 [T, C]: the contents the encoder is tested on."""
    g = (rng.standard_normal((T, C)) * 3).astype(f32)
    out = {"gauss": g, "ints": rng.integers(-2, 3, (T, C)).astype(f32), "const": np.full((T, C), f32(-7.25))}
    cc = g.copy()
    cc[:, C // 2] = f32(1.5)
    out["const_col"] = cc
    o = g.copy()
    o[:, 0] = (rng.standard_normal(T) * 1000).astype(f32)
    out["outlier_col"] = o
    z = rng.integers(-1, 2, (T, C)).astype(f32)
    z[rng.random((T, C)) < 0.5] *= f32(-1.0)                # zeros of both signs
    out["pm_zero"] = z
    out["pm_zero_nonneg"] = np.abs(rng.integers(0, 2, (T, C)).astype(f32)) * np.where(rng.random((T, C)) < 0.5, f32(-0.0), f32(1.0))
    # grange ~ 2^-128: subnormal, yet 65535 16-bit steps of it are still distinct subnormals (>= 2^-133 is needed for that)
    out["subnormal_range"] = (rng.random((T, C)).astype(f32) * f32(2.0 ** -100)) * f32(2.0 ** -28)
    return out
