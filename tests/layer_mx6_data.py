"""Emulation of XV_FMT_SPLIT6 rows and of the f16mx6 layer (xv_tdnn_layer_f16mx6: the cross terms of a hidden layer on
block-scaled e2m3 MFMAs), shared by tests/test_layer_mx6_cpu.py and tests/test_gpu_layer_mx6.py.  The block rule, the grid and the
rounding are those of tests/pair_mx6_data.py (encode_blocks, e2m3_rne); only the blocks differ: here a block is 16 CONSECUTIVE
channels -- channels 16b .. 16b + 15 of a frame on the activation side, of one tap's weight column on the weight side.

A stored row holds, per block: the fp16 hi of its 16 channels, the 32 e2m3 elements [2^11 lo | c] under the block's scale 2^-k, and
the byte 127 + k - 11 (the 2^-11 of the cross terms rides in the activation side's byte; the weight side stores 127 + k).  Decoding
returns hi + 2^-11 lo_q and, as a second plane, c_q.

Also the inputs both test files share: edge_layout (the rows of a (K, dilation) layer with chunks around the halo's length) and
hostile_blocks / hostile_rows (values on the encoder's edges)."""
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


def edge_lengths(h):
    """Chunks shorter than, equal to and one longer than the halo h, and a 150-frame chunk that ends the batch."""
    return [1, 2, h, h + 1, 97, 3, 150]


def edge_layout(K, dilation, lengths=None):
    """The row layout engine.BatchLayout gives a (K, dilation) layer -- gap h = (K - 1) / 2 dilation, chunks on 8-row starts -- for
    chunks shorter than, equal to and one longer than the halo, and a 150-frame chunk across the 256-row tile boundary.
    -> (valid uint8 [R], starts, lengths)."""
    from xvector_amd import engine
    h = (K - 1) // 2 * dilation
    lengths = edge_lengths(h) if lengths is None else list(lengths)
    lay = engine.BatchLayout(lengths, h, 8)
    return lay.row_valid().copy(), lay.row_start.tolist(), lengths


E2M3_TIES = np.array([(a + b) / 2.0 for a, b in zip(mx.E2M3_GRID[:-1], mx.E2M3_GRID[1:])])      # 31 midpoints, 0.0625 .. 7.25


def _f32_next(v, up):
    """The fp32 next to v > 0, above or below."""
    return np.nextafter(np.float32(v), np.float32(np.inf if up else 0.0))


def hostile_blocks(e_range=range(-16, 16), tiny=True, beyond=True):
    """[(tag, 16 fp32 values)]: blocks of 16 channels built to sit on the edges of the SPLIT6 encoder.  A tag names what the block is
    for; blocks with a magnitude beyond 57344 are tagged "beyond:...".  ``e_range``: the exponents of the 1.875 2^e maxima; ``tiny``:
    with the blocks below fp16's normal range; ``beyond``: with those beyond the clamp (the weight-side test leaves both out)."""
    out = []
    fill = np.array([0.4, -0.31, 0.23, 0.17, -0.11, 0.07, 0.05, -0.03, 0.36, 0.29, -0.19, 0.13, 0.09, -0.06, 0.04, 0.02])

    def put(tag, vals, at=None):
        b = np.zeros(16, np.float32)
        vals = np.asarray(vals, np.float32)
        b[:len(vals)] = vals
        if at is not None:                                   # move the first value to position ``at`` (< 15)
            b[[0, at]] = b[[at, 0]]
        if not beyond and np.abs(b).max() > em.SPLIT8_MAX:
            return
        out.append((("beyond:" if np.abs(b).max() > em.SPLIT8_MAX else "") + tag, b))

    # block maxima at 1.875 2^e and the fp32 on either side, the rest of the block small: the edge sets the scale
    for e in e_range:
        edge = np.float32(1.875 * 2.0 ** e)
        sign = -1.0 if e & 1 else 1.0
        for name, m in (("below", _f32_next(edge, False)), ("at", edge), ("above", _f32_next(edge, True))):
            put("edge %s %d" % (name, e), np.concatenate([[sign * m], fill[:15] * float(edge)]), at=(5 * e + 3) % 15)
        # ... and once where another element (4 x) sets it: the edge is an ordinary element (1.875 / 4 of the maximum)
        put("edge inside %d" % e, np.concatenate([[edge, -4.0 * float(edge) * 1.5], fill[:13] * float(edge)]), at=(3 * e + 7) % 13 + 2)
    # ties of the c half: anchor 6.0 2^k (scale exponent k), elements on every midpoint of the grid, both signs
    for k in (-3, 0, 5):
        ties = np.concatenate([E2M3_TIES, -E2M3_TIES]) * 2.0 ** k
        for i in range(0, len(ties), 14):
            put("c ties k %d" % k, np.concatenate([[6.0 * 2.0 ** k], ties[i:i + 14]]), at=(i // 14) % 15)
        # below half the first step, and just beyond it
        s = 2.0 ** k
        put("below first step k %d" % k, [6.0 * s, 0.0624 * s, -0.0624 * s, 0.03 * s, -0.03 * s, 0.0626 * s, -0.0626 * s, 0.001 * s])
        # ties of the lo' half in the steps 0.125 and 0.25: v = 5 2^k + t 2^(k - 11), hi = 5 2^k, lo' = t 2^k for |t| < 4
        t = E2M3_TIES[E2M3_TIES < 4.0]
        vals = np.concatenate([5.0 * s + t * s / em.LO_SCALE, 5.0 * s - t * s / em.LO_SCALE, -(5.0 * s + t[:8] * s / em.LO_SCALE)])
        for i in range(0, len(vals), 15):
            put("lo ties k %d" % k, vals[i:i + 15])
    put("zeros", np.zeros(16))
    put("minus zero", [-0.0, 1.0, -0.0, 0.25, -0.0])
    if tiny:
        # below 2^-25 hi is 0 and lo' = 2^11 v is the block's maximum: anchor 6.0 2^j / 2^11, lo' on every midpoint (step 0.5 too)
        for j in (-17, -40):
            ties = np.concatenate([E2M3_TIES, -E2M3_TIES]) * 2.0 ** j / em.LO_SCALE
            for i in range(0, len(ties), 14):
                put("tiny lo ties j %d" % j, np.concatenate([[6.0 * 2.0 ** j / em.LO_SCALE], ties[i:i + 14]]), at=(i // 14) % 15)
        # fp16's subnormal range: hi is a multiple of 2^-24, lo' is large against c
        put("fp16 subnormal", [2.0 ** -15 * 1.3, -2.0 ** -16 * 1.7, 2.0 ** -20 * 1.1, -2.0 ** -24 * 1.5, 2.0 ** -24 * 0.5, 2.0 ** -25,
                               -2.0 ** -25 * 1.001, 2.0 ** -14, np.nextafter(np.float32(2.0 ** -14), np.float32(0)), 2.0 ** -19 * 1.9])
        put("fp16 subnormal under a normal maximum", [0.37, 2.0 ** -15 * 1.3, -2.0 ** -18 * 1.7, 2.0 ** -24 * 1.5, -2.0 ** -14 * 0.99])
        put("fp32 denormals", [1e-40, -3e-42, 5e-45, -1e-39])
        put("1e-38", [1e-38] * 8 + [-1e-38] * 7)
    # the clamp: at 57344 nothing is reported, beyond it the status bit
    put("57344", [57344.0, -57344.0, 3.0, -100.0, 40000.0])
    over = _f32_next(57344.0, True)
    put("over by an ulp", [over, 1.0, 2.0])
    put("over by an ulp, negative", [-over, 1.0, 2.0])
    put("65504", [65504.0, -65504.0, 12.0])
    put("7e4", [7e4, -7e4, 5.0, 30000.0])
    put("inf", [np.inf, 1.0, -np.inf, 0.5])
    return out


def hostile_rows(C=64, **kw):
    """hostile_blocks laid out as rows of C channels (C % 16 == 0), the in-range blocks first: (rows [n, C] fp32, n_in = the
    number of leading rows without a magnitude beyond 57344, where = {tag: (row, block)} of the first block with that tag)."""
    blocks = hostile_blocks(**kw)
    blocks = [b for b in blocks if not b[0].startswith("beyond:")] + [b for b in blocks if b[0].startswith("beyond:")]
    per = C // 16
    n_in_blocks = sum(not t.startswith("beyond:") for t, _ in blocks)
    n_in = -(-n_in_blocks // per)
    flat = [b for _, b in blocks[:n_in_blocks]] + [np.zeros(16, np.float32)] * (n_in * per - n_in_blocks) + [b for _, b in blocks[n_in_blocks:]]
    tags = [t for t, _ in blocks[:n_in_blocks]] + ["pad"] * (n_in * per - n_in_blocks) + [t for t, _ in blocks[n_in_blocks:]]
    flat += [np.zeros(16, np.float32)] * (-len(flat) % per)
    rows = np.concatenate(flat).astype(np.float32).reshape(-1, C)
    where = {}
    for i, t in enumerate(tags):
        where.setdefault(t, (i // per, i % per))
    return rows, n_in, where


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
