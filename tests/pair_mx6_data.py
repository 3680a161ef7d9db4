"""Emulation of the block-scaled e2m3 cross terms of the f16mx6 pair kernel (csrc/xv_split6.h; tdnn_pair_pool_f16bf8_kernel<., true>
in csrc/xv_pair8.hip), shared by tests/test_pair_mx6_cpu.py and tests/test_gpu_pair_mx6.py.

Hardware semantics the emulation follows (tools/experiments/mx_probe.hip, part 3):
  * v_cvt_scalef32_2xpk16_fp6_f32 divides by the scale, rounds to nearest with ties to even on the e2m3 grid (subnormals 0.125 ..
    0.875 included) and saturates at +-7.5;
  * the scaled MFMA with cbsz:2 blgp:2 takes the scale byte of (row, K block) from the lane that holds that block's elements.

A block is the 16 channels one lane of the kernel holds of a 32-channel slab: channels (r & 3) + 8 (r >> 2) + 4 hh, r = 0 .. 15, of
the slab, for either lane half hh -- on the activation side for one frame, on the weight side for one column.  Its 32 values are
[2^11 lo | c]; m = their largest magnitude; the scale s is the largest power of two with s m <= 7.5 (1 when m = 0)."""
import numpy as np

import arith_emul as em

CMID = 512
E2M3_MAX = 7.5
E8M0_MIN = 16                                            # floor of a block's byte: XV_SPLIT6_E8M0_MIN
E2M3_GRID = np.array(sorted({m * 0.125 for m in range(8)} | {(1 + m / 8.0) * 2.0 ** e for e in range(3) for m in range(8)}))

# channel of (block b = 2 slab + hh, element r) for a 512-channel operand: [32, 16]
BLOCK_CHANNELS = np.array([[32 * (b >> 1) + (r & 3) + 8 * (r >> 2) + 4 * (b & 1) for r in range(16)] for b in range(CMID // 16)])


def e2m3_step(a):
    """The grid's step at magnitude a (a already scaled into the block's range)."""
    a = np.abs(np.asarray(a, np.float64))
    return np.where(a < 2.0, 0.125, np.where(a < 4.0, 0.25, 0.5))


def e2m3_rne(a):
    """Nearest e2m3 value, ties to even, saturating at +-7.5 (fp64 in, fp64 out)."""
    a = np.asarray(a, np.float64)
    mag = np.minimum(np.abs(a), 8.0)
    step = e2m3_step(mag)
    q = np.minimum(np.rint(mag / step) * step, E2M3_MAX)     # np.rint: ties to even; the grid's even codes are the even multiples
    return np.copysign(q, a)


def scale_exponent(m):
    """k with 1 / s = 2^k for the block maximum m (fp32 values): the rule of xv_split6_e8m0, stated on the value instead of
    the bits.  m = f 2^e, 1 <= f < 2: k = e - 2 for f <= 1.875, e - 1 above; m = 0: k = 0; floor E8M0_MIN - 127."""
    m = np.asarray(m, np.float64)
    f, e = np.frexp(m)                                   # m = f 2^e, 0.5 <= f < 1
    k = np.where(f <= 1.875 / 2.0, e - 3, e - 2)
    k = np.maximum(k, E8M0_MIN - 127)
    return np.where(m == 0, 0, k).astype(np.int64)


def encode_blocks(v):
    """v [..., 16] fp32 (one block per row of the last axis) -> (hi, lo_q, c_q, k): the fp16 main operand and the two DEQUANTISED
    cross-term operands q 2^k (lo_q stands for 2^11 lo: the product carries 2^-11), all as fp64 / fp32-exact values, and the
    block's scale exponent k [...]."""
    c = np.clip(np.asarray(v, np.float32), -em.SPLIT8_MAX, em.SPLIT8_MAX)
    hi = c.astype(np.float16).astype(np.float32)
    lo = ((c - hi) * np.float32(em.LO_SCALE)).astype(np.float64)
    c = c.astype(np.float64)
    m = np.maximum(np.abs(lo).max(-1), np.abs(c).max(-1))
    k = scale_exponent(m)
    s = np.ldexp(1.0, -k)[..., None]
    return hi.astype(np.float64), e2m3_rne(lo * s) / s, e2m3_rne(c * s) / s, k


def operand_planes(a, axis):
    """Planes (hi, lo_q, c_q) of a 512-channel operand in channel order: a [T, 512] with axis = 1 (activations: a block per frame) or
    [512, cout] with axis = 0 (weights: a block per column); and the scale exponents [T or cout, 32]."""
    a = np.asarray(a, np.float32)
    rows = a if axis == 1 else a.T
    hi, lo, c, k = encode_blocks(rows[:, BLOCK_CHANNELS])            # [n, 32, 16]
    out = []
    for p in (hi, lo, c):
        full = np.zeros(rows.shape)
        full[:, BLOCK_CHANNELS] = p
        out.append(full if axis == 1 else full.T)
    return out[0], out[1], out[2], k


def terms(H, w2):
    """[(z_t fp64, M_t)] of the three product terms of H [T, 512] . w2 [512, cout] in the f16mx6 arithmetic: fp16 . fp16, then
    2^-11 (lo_q(H) . c_q(w) + c_q(H) . lo_q(w))."""
    hh, hl, hc, _ = operand_planes(H, 1)
    wh, wl, wc, _ = operand_planes(w2, 0)
    out = []
    for xp, wp, coef in ((hh, wh, 1.0), (hl, wc, 1.0 / em.LO_SCALE), (hc, wl, 1.0 / em.LO_SCALE)):
        wp = wp * coef
        out.append((xp @ wp, np.abs(xp) @ np.abs(wp)))
    return out


def layer2_reference(H, l2, A):
    """(activation fp64, element bound) of act(float32(H) . w2 + b2) over the emulated terms: pair_data.layer2_reference with the
    e2m3 encoding in place of the bf8 one."""
    tz = terms(H, l2["w2"])
    b2 = 0.0 if l2["b2"] is None else l2["b2"].astype(np.float64)
    z = sum(t[0] for t in tz)
    M = sum(t[1] for t in tz) + np.abs(b2)
    zb = z + b2
    a = em.apply_act(zb, l2["act"], l2["alpha2"])
    return a, em.elementwise_bound(A, M, zb, a, None, l2["alpha2"])


def product_error_bound(X, W):
    """Element-wise bound on |emulated X . W - exact X . W| from the formats alone.  With x = xh + xl, |xl| <= 2^-11 |x| (fp16), the
    emulation drops xl wl (<= 2^-22 |x| |w|) and replaces wh by c_q(w), xh by c_q(x) in the cross terms (each off from w, x by the
    e2m3 half step, from wh, xh by 2^-11 |.| more) and 2^11 xl, 2^11 wl by their e2m3 values.  A block's half step is at most 0.25
    / s with s m >= 3.75: at most m / 15 (m: the block maximum, >= every |c| and 2^11 |lo| of the block).  Per product
        2^-11 [ (Bx/15) (|w| + Bw/15) + |x| Bw/15 ]  for each of the two cross terms, + 3 2^-22 |x| |w|."""
    X, W = np.asarray(X, np.float64), np.asarray(W, np.float64)

    def block_max(a, axis):
        rows = np.abs(a if axis == 1 else a.T)
        bm = np.repeat(rows[:, BLOCK_CHANNELS].max(-1)[:, :, None], 16, -1)
        full = np.zeros(rows.shape)
        full[:, BLOCK_CHANNELS] = bm
        return full if axis == 1 else full.T
    BX, BW = block_max(X, 1) / 15.0, block_max(W, 0) / 15.0
    aX, aW = np.abs(X), np.abs(W)
    return 2.0 * 2.0 ** -11 * (BX @ (aW + BW) + aX @ BW) + 3.0 * 2.0 ** -22 * (aX @ aW)


class Rows:
    """The row layout of the GPU test: chunks on 8-row starts with gaps, R rows in all (the interface of engine.BatchLayout that
    pair_data's block functions use)."""

    def __init__(self, starts, lens, R):
        self.row_start, self.row_len, self.rows = list(starts), list(lens), int(R)
        assert all(s % 8 == 0 for s in starts) and starts[-1] + lens[-1] <= R

    def row_valid(self):
        v = np.zeros(self.rows, np.uint8)
        for s, n in zip(self.row_start, self.row_len):
            v[s:s + n] = 1
        return v

    def pack(self, mats, host):
        for s, m in zip(self.row_start, mats):
            host[s:s + len(m)] = m
