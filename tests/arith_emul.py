"""Emulator of the split arithmetics of the forward GEMMs (bf16x3: csrc/xv_gemm3.hip; f16bf8: csrc/xv_split8.h, xv_gemm8*.hip).

Encoders are stated bit for bit; a contraction is formed from the EMULATED product terms, each exact in fp32 (fp16*fp16,
bf16*bf16 and bf8*bf8 products all fit in 24 bits), summed in fp64.  What is left between a kernel and this emulator is the
kernel's fp32 accumulation rounding, which the element-wise bound A * 2^-24 * M covers (M = sum |terms| + |bias|).

Hardware semantics the emulator follows (established on the device by tests/test_gpu_elementwise.py):
  * v_cvt_pk_bf8_f32 / v_cvt_scalef32_pk_bf8_f32 round to nearest, ties to even, with e5m2 subnormals;
  * the fp16 and f8f6f4 MFMAs honour subnormal inputs (no flush to zero).
"""
import numpy as np

SPLIT8_MAX = 57344.0            # largest finite e5m2, below fp16's 65504: the split8 encoders clamp to it
LO_SCALE = 2.0 ** 11            # l8 = e5m2(2^11 (c - hi)); the cross terms carry the E8M0 scale 2^-11
ACT = {"none": 0, "relu": 1, "lrelu": 2, "prelu": 3}


# ---------------------------------------------------------------------------------------------------------------------------
# encoders
# ---------------------------------------------------------------------------------------------------------------------------
def bf16_rne(a):
    """fp32 -> bf16 bit pattern (uint16), round to nearest, ties to even (finite inputs)."""
    u = np.asarray(a, np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def bf16_value(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def split3(x):
    """bf16x3 operand: hi = bf16_rne(x), lo = bf16_rne(x - hi) (x - hi is exact in fp32).  Returns fp32 values."""
    x = np.asarray(x, np.float32)
    hi = bf16_value(bf16_rne(x))
    lo = bf16_value(bf16_rne(x - hi))
    return hi, lo


def e5m2_bits(a):
    """fp32 -> e5m2 byte (uint8), round to nearest even, subnormals kept (|a| <= 57344: the callers clamp)."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.float8_e5m2)
    return t.view(torch.uint8).numpy()


def e5m2_value(bits):
    """e5m2 byte -> fp32 (e5m2 is the upper byte of an fp16)."""
    return (np.asarray(bits, np.uint8).astype(np.uint16) << 8).view(np.float16).astype(np.float32)


def split8_bytes(x):
    """split8 encoding of fp32 values: (hi fp16 bits uint16, l8 uint8, h8 uint8), as xv_split8_encode8 forms them."""
    c = np.clip(np.asarray(x, np.float32), -SPLIT8_MAX, SPLIT8_MAX)
    hi = c.astype(np.float16)
    lo = c - hi.astype(np.float32)                      # exact in fp32
    return hi.view(np.uint16), e5m2_bits(lo * np.float32(LO_SCALE)), e5m2_bits(c)


def split8(x):
    """split8 operand values (fp32): hi, l8 (unscaled byte value: the operand is 2^-11 l8), h8."""
    hb, lb, h8 = split8_bytes(x)
    return hb.view(np.float16).astype(np.float32), e5m2_value(lb), e5m2_value(h8)


def split8_weight_slot(w8):
    """The 16-byte cross slot of 8 weight channels: [8 x h8 | 8 x l8] (activations store [l8 | h8])."""
    _, l8, h8 = split8_bytes(w8)
    return np.concatenate([h8, l8])


def decode3(x):
    """What a bf16 split buffer decodes to: fp32(hi + lo)."""
    hi, lo = split3(x)
    return (hi + lo).astype(np.float32)


def decode8(x):
    """What a split8 buffer decodes to: fp32(hi + 2^-11 l8)."""
    hi, l8, _ = split8(x)
    return (hi + l8 * np.float32(1.0 / LO_SCALE)).astype(np.float32)


def _parts(arith, x, w):
    """[(x part, w part, coefficient)] of the product x*w in ``arith``; every part * part is exact in fp32."""
    if arith == "fp32":
        return [(np.asarray(x, np.float32), np.asarray(w, np.float32), 1.0)]
    if arith == "bf16x3":
        xh, xl = split3(x)
        wh, wl = split3(w)
        return [(xh, wh, 1.0), (xh, wl, 1.0), (xl, wh, 1.0)]
    if arith == "f16bf8":
        xh, xl8, xh8 = split8(x)
        wh, wl8, wh8 = split8(w)
        return [(xh, wh, 1.0), (xl8, wh8, 1.0 / LO_SCALE), (xh8, wl8, 1.0 / LO_SCALE)]
    raise ValueError(arith)


# ---------------------------------------------------------------------------------------------------------------------------
# contractions
# ---------------------------------------------------------------------------------------------------------------------------
def apply_act(z, act, alpha):
    if act == "relu":
        return np.maximum(z, 0.0)
    if act in ("lrelu", "prelu"):
        a = np.broadcast_to(np.asarray(alpha, np.float64), z.shape[-1:])
        return np.where(z > 0, z, a * z)
    return z


def epilogue(z, b, scale, shift, act, alpha):
    """act(z + b) * scale + shift in fp64 (scale / shift: the folded BN, passed directly; None = 1 / 0)."""
    zb = z + (0.0 if b is None else np.asarray(b, np.float64))
    y = apply_act(zb, act, alpha)
    if scale is not None:
        y = y * np.asarray(scale, np.float64)
    if shift is not None:
        y = y + np.asarray(shift, np.float64)
    return y


def _shifted(x, off):
    """rows r of the result = x[r + off] (zero outside the chunk: the per-chunk zero halo)."""
    T = x.shape[0]
    out = np.zeros_like(x)
    lo, hi = max(0, -off), min(T, T - off)
    if hi > lo:
        out[lo:hi] = x[lo + off:hi + off]
    return out


def contract(arith, x, w, dilation=1):
    """z[t] = sum_k x[t + (k - (K-1)/2) d] . w[k] over the emulated terms, and M = sum |terms|.  x [T, Cin], w [K, Cin, Cout]."""
    x = np.asarray(x, np.float32)
    w = np.asarray(w, np.float32)
    K = w.shape[0]
    h = (K - 1) // 2
    z = np.zeros((x.shape[0], w.shape[2]))
    M = np.zeros_like(z)
    for xp, wp, coef in _parts(arith, x, w):
        xp = xp.astype(np.float64)
        wp = wp.astype(np.float64) * coef
        for k in range(K):
            xs = _shifted(xp, (k - h) * dilation)
            z += xs @ wp[k]
            M += np.abs(xs) @ np.abs(wp[k])
    return z, M


def wgrad(arith, x, dz, K, dilation=1):
    """dw[k] = sum_r x[r + (k - (K-1)/2) d]^T dz[r] over the emulated terms (rows outside [0, R) are zero), and M = sum_r |terms|.
    x [R, Cin], dz [R, Cout] -> (dw fp64 [K, Cin, Cout], M)."""
    x = np.asarray(x, np.float32)
    dz = np.asarray(dz, np.float32)
    h = (K - 1) // 2
    dw = np.zeros((K, x.shape[1], dz.shape[1]))
    M = np.zeros_like(dw)
    for xp, zp, coef in _parts(arith, x, dz):
        xp = xp.astype(np.float64)
        zp = zp.astype(np.float64) * coef
        az = np.abs(zp)
        for k in range(K):
            xs = _shifted(xp, (k - h) * dilation)
            dw[k] += xs.T @ zp
            M[k] += np.abs(xs).T @ az
    return dw, M


def tdnn_layer(arith, x, w, b, scale, shift, act, alpha, dilation=1):
    """One layer on one chunk: (y fp64, z + b fp64, M = sum |terms| + |b|)."""
    z, M = contract(arith, x, w, dilation)
    if b is not None:
        z = z + np.asarray(b, np.float64)
        M = M + np.abs(np.asarray(b, np.float64))
    return epilogue(z, None, scale, shift, act, alpha), z, M


def fc(arith, x, w, b, scale, shift, act, alpha):
    """x [B, In] . w [In, Out] as a K = 1 layer over the rows."""
    return tdnn_layer(arith, x, np.asarray(w)[None], b, scale, shift, act, alpha, 1)


def toom_magnitude(x, w, dilation, G, BT, AT, rows_valid=None):
    """M of the Toom-Cook F(2,K) form over a whole packed buffer x [R, Cin] (gaps included, as the kernel sees it):
    M[2P+q] = sum_c sum_j |AT[q][j]| (sum_k |G[j][k]| |w[k]|) (sum_i |BT[j][i]| |d_i|), row pairs of each sub-problem
    (rows r, r + d with floor(r / d) even), d_i = x[sub + (2P - h + i) d] (zero outside the buffer)."""
    R = x.shape[0]
    K = w.shape[0]
    h = (K - 1) // 2
    J = K + 1
    G = np.abs(np.asarray(G, np.float64))
    BT = np.abs(np.asarray(BT, np.float64))
    AT = np.abs(np.asarray(AT, np.float64))
    ax = np.abs(np.asarray(x, np.float64))
    aw = np.abs(np.asarray(w, np.float64))
    U = np.einsum("jk,kco->jco", G, aw)                                   # [J, Cin, Cout]
    M = np.zeros((R, w.shape[2]))
    r = np.arange(R)
    sub, m = r % dilation, r // dilation
    base = (m // 2) * 2 - h
    for j in range(J):
        V = np.zeros_like(ax)
        for i in range(J):
            if BT[j, i] == 0:
                continue
            src = sub + (base + i) * dilation
            ok = (src >= 0) & (src < R)
            V[ok] += BT[j, i] * ax[src[ok]]
        P = V @ U[j]
        for q in range(2):
            sel = (m % 2) == q
            M[sel] += AT[q, j] * P[sel]
    return M


# ---------------------------------------------------------------------------------------------------------------------------
# the element-wise bound
# ---------------------------------------------------------------------------------------------------------------------------
U = 2.0 ** -24
ENC_SPLIT = 2.0 ** -17          # |decode3(v) - v| <= 2^-17 |v|: hi + lo carry 16 significant bits
ENC_SPLIT8 = 2.0 ** -13         # |decode8(v) - v| <= 2^-13 |v| + 2^-24 (the split8 encoder's documented error)


def accum_factor(depth, lam=1.0):
    """A = lam sqrt(depth): an output is accumulated by ``depth`` fp32 roundings, each at most u |partial sum| <= u M; with
    round-to-nearest their signs are independent, so they grow as sqrt(depth) (Higham & Mary 2019), not as depth."""
    return lam * np.sqrt(float(depth))


def elementwise_bound(A, M, zb, y, scale, alpha, fmt="f32"):
    """A 2^-24 M max(1, |alpha|) |scale| + the epilogue's roundings (z + b, the activation, the scale, the shift: 4 u of the
    magnitudes they see) + the output encoder's error for split / split8 outputs."""
    s = np.abs(np.broadcast_to(1.0 if scale is None else np.asarray(scale, np.float64), y.shape[-1:]))
    a = np.maximum(1.0, np.abs(np.broadcast_to(1.0 if alpha is None else np.asarray(alpha, np.float64), y.shape[-1:])))
    acc = A * U * M * a * s
    bnd = acc + 4 * U * (np.abs(zb) * a * s + np.abs(y))
    if fmt == "split":
        bnd = bnd + ENC_SPLIT * (np.abs(y) + bnd)
    elif fmt == "split8":
        bnd = bnd + ENC_SPLIT8 * (np.abs(y) + bnd) + U
    return bnd


def depth(arith, K, cin):
    """fp32 roundings on an output's accumulation chain: one per accumulator update of the MFMA sequence -- fp32: 32x32x2 (2
    products per update); bf16x3: 3 MFMAs of 16 products per 32-channel slab and tap, twice; f16bf8: 2 fp16 + 1 scaled-bf8 update
    per slab and tap; fp32tc: K + 1 transformed products per 2 channels plus the <= 6-row transform and the fold."""
    slabs = K * ((cin + 31) // 32)
    return {"fp32": K * cin / 2.0, "bf16x3": 6.0 * slabs, "f16bf8": 3.0 * slabs, "fp32tc": (K + 1) * cin / 2.0 + 16}[arith]
