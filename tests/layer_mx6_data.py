"""Emulation of XV_FMT_SPLIT6 rows and of the f16mx6 layer (xv_tdnn_layer_f16mx6: the cross terms of a hidden layer on
block-scaled e2m3 MFMAs), shared by tests/test_layer_mx6_cpu.py and tests/test_gpu_layer_mx6.py.  The block rule, the grid and the
rounding are those of tests/pair_mx6_data.py (encode_blocks, e2m3_rne); only the blocks differ: here a block is 16 CONSECUTIVE
channels -- channels 16b .. 16b + 15 of a frame on the activation side, of one tap's weight column on the weight side.

A stored row holds, per block: the fp16 hi of its 16 channels, the 32 e2m3 elements [2^11 lo | c] under the block's scale 2^-k, and
the byte 127 + k - 11 (the 2^-11 of the cross terms rides in the activation side's byte; the weight side stores 127 + k).  Decoding
returns hi + 2^-11 lo_q and, as a second plane, c_q."""
import numpy as np

import arith_emul as em
import pair_mx6_data as mx

LO_EXP = 11


def encode_rows(v):
    """v [n, C] fp32, C % 16 == 0, a block = 16 consecutive columns -> (hi, lo_q, c_q [n, C] fp64; k [n, C / 16])."""
    v = np.asarray(v, np.float32)
    n, C = v.shape
    hi, lo, c, k = mx.encode_blocks(v.reshape(n, C // 16, 16))
    return hi.reshape(n, C), lo.reshape(n, C), c.reshape(n, C), k


def stored_byte(k):
    """The byte an ACTIVATION block stores for scale exponent k."""
    return np.asarray(k) + 127 - LO_EXP


def decode_rows(v):
    """What xv_split6_decode_f32 returns for rows encoded from v: (fp32(hi + 2^-11 lo_q), fp32(c_q))."""
    hi, lo, c, _ = encode_rows(v)
    return (hi + lo / em.LO_SCALE).astype(np.float32), c.astype(np.float32)


def weight_planes(w):
    """w [K, Cin, Cout] -> (hi, lo_q, c_q) [K, Cin, Cout] fp64: a block = 16 consecutive input channels of one tap and column."""
    w = np.asarray(w, np.float32)
    K, cin, cout = w.shape
    hi, lo, c, _ = encode_rows(w.transpose(0, 2, 1).reshape(K * cout, cin))
    back = lambda p: p.reshape(K, cout, cin).transpose(0, 2, 1)
    return back(hi), back(lo), back(c)


def contract(x, w, dilation=1):
    """em.contract in the f16mx6 arithmetic: z = xh . wh + 2^-11 (lo_q(x) . c_q(w) + c_q(x) . lo_q(w)) over the taps, rows outside the
    buffer zero; and M = sum |terms|.  x [R, Cin] (gap rows zero), w [K, Cin, Cout] -> (z, M) fp64; also the three terms' own z."""
    xh, xl, xc, _ = encode_rows(x)
    wh, wl, wc = weight_planes(w)
    K = w.shape[0]
    h = (K - 1) // 2
    z = np.zeros((x.shape[0], w.shape[2]))
    M = np.zeros_like(z)
    parts = []
    for xp, wp, coef in ((xh, wh, 1.0), (xl, wc, 1.0 / em.LO_SCALE), (xc, wl, 1.0 / em.LO_SCALE)):
        zt = np.zeros_like(z)
        for k in range(K):
            xs = em._shifted(xp, (k - h) * dilation)
            zt += xs @ (wp[k] * coef)
            M += np.abs(xs) @ np.abs(wp[k] * coef)
        parts.append(zt)
        z += zt
    return z, M, parts


def product_error_bound(x, w, dilation=1):
    """Element-wise bound on |contract(x, w) - exact fp64 convolution| from the formats alone: pair_mx6_data.product_error_bound's
    argument on consecutive blocks, summed over the taps.  With Bx / Bw the block maxima over 15 (a block's half step is at most
    its maximum / 15), per product  2 2^-11 [Bx (|w| + Bw) + |x| Bw] + 3 2^-22 |x| |w|."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    K, cin, cout = w.shape

    def bmax(a):                                         # [n, C] -> block maxima broadcast back over the block
        n, C = a.shape
        return np.repeat(np.abs(a).reshape(n, C // 16, 16).max(-1), 16, -1)
    BX = bmax(x) / 15.0
    BW = bmax(w.transpose(0, 2, 1).reshape(K * cout, cin)).reshape(K, cout, cin).transpose(0, 2, 1) / 15.0
    aX, aW = np.abs(x), np.abs(w)
    h = (K - 1) // 2
    out = np.zeros((x.shape[0], cout))
    for k in range(K):
        off = (k - h) * dilation
        sx, sb = em._shifted(aX, off), em._shifted(BX, off)
        out += 2.0 * 2.0 ** -11 * (sb @ (aW[k] + BW[k]) + sx @ BW[k]) + 3.0 * 2.0 ** -22 * (sx @ aW[k])
    return out


def missing_taps(valid, K, dilation=1):
    """[R, K] bool: tap t of row r falls outside [0, R) or on a gap row (what the tap_bias table must not contribute)."""
    valid = np.asarray(valid).astype(bool)
    R = len(valid)
    h = (K - 1) // 2
    out = np.zeros((R, K), bool)
    for t in range(K):
        q = np.arange(R) + (t - h) * dilation
        ok = (q >= 0) & (q < R)
        out[:, t] = ~(ok & valid[np.clip(q, 0, R - 1)])
    return out
