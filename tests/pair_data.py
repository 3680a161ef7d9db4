"""Data and bounds for the fused layer-3+4 pair kernels (tdnn_pair_pool_kernel: csrc/xv_pair.hip; tdnn_pair_pool_f16bf8_kernel:
csrc/xv_pair8.hip), shared by tests/test_gpu_pair_elementwise.py and its CPU companion tests/test_pair_bounds_cpu.py.

The 512-channel intermediate H of these kernels lives in registers: only 8-row block statistics come out.  Integer data keep every
low plane (l8 / bf16 lo of x, w1, H, w2) zero, so a lost cross term passes.  Three constructions close that:

  * live_layer1: x and w1 = sign(n) (|n| + m q) with n exact in e5m2 and bf16, m in 0..3 and q below half an ulp of the high plane
    (2^-13 for f16bf8, 2^-10 for bf16x3): the high plane is n, the low plane m q, every emulated product a multiple of q and every
    partial sum below 2^24 q -- H is the same fp32 bits under any summation order, with or without FMA contraction, and its own
    low plane is not zero either;
  * select_w2: a one-hot layer 2 with weights 1, 2, 0.5 forwards decode(H) without a rounding -- the block statistics are then
    those of a known activation;
  * real_layer2: a realistic layer 2 on the exactly known H -- the emulator's terms of float32(H) . w2 give the reference and the
    magnitude M of the element-wise bound, which is carried through the pooling to a bound per block.

One act code serves both layers of a pair kernel (the C ABI has one act_kind), so the "select" layer 2 applies the same activation
with alpha2 in {0.25, 0.5}: exact on decode(H) (<= 16 significant bits).
"""
import numpy as np

import arith_emul as em

CMID = 512
LENS = [25, 1, 7, 8, 9, 130, 257, 3]
SHAPES = [(64, 64), (96, 192), (512, 1536)]
ARITHS = ["bf16x3", "f16bf8"]
Q = {"f16bf8": 2.0 ** -13, "bf16x3": 2.0 ** -10}
NVALS = np.array([0, 1, -1, 2, -2, 3, -3, 4, -4, 6, -6], np.float64)
# the activation of each shape: relu, lrelu, prelu and none all occur for each arithmetic over tests (a) and (c)
ACT_EXACT = {64: "prelu", 96: "lrelu", 512: "relu"}          # (a) and its control (b)
ACT_BOUND = {64: "none", 96: "relu", 512: "prelu"}           # (c)

# Layer 2 of a pair kernel: the fp32 roundings of one output's chain.  em.depth counts the accumulator updates of the 16 slabs;
# + 2: the partner's 256-channel partial sum and the bias, (yK + pb) + b2 (the bf16x3 kernel has one chain and the bias add).
A_PAIR = {a: em.accum_factor(em.depth(a, 1, CMID) + 2) for a in ARITHS}


def layout():
    from xvector_amd import engine
    return engine.BatchLayout(LENS, 1, 8)                     # 8 = hiplib.POOL_BLOCK_ROWS (asserted by the GPU test)


def _f32_exact(v):
    return np.array_equal(np.asarray(v, np.float64), np.asarray(v, np.float64).astype(np.float32).astype(np.float64))


def _live_values(rng, shape, q, density=1.0):
    """sign(n) (|n| + m q): the offset points AWAY from zero (towards zero it would cross a binade at |n| a power of two)."""
    n = rng.choice(NVALS, shape)
    if density < 1.0:
        n = n * (rng.random(shape) < density)
    m = rng.integers(0, 4, shape) * (n != 0)
    return (np.sign(n) * (np.abs(n) + m * q)).astype(np.float32)


def low_part(arith, v):
    return em.split8(v)[1] if arith == "f16bf8" else em.split3(v)[1]


def decode(arith, v):
    return (em.decode8 if arith == "f16bf8" else em.decode3)(v)


def terms(arith, x, w, swap=False):
    """[(z_t fp64, M_t)] of the three product terms of x [T, Cin] . w [Cin, Cout] (em._parts); swap: the l8 and h8 planes of x trade
    places (the byte order of the in-register H of the f16bf8 pair kernel)."""
    parts = em._parts(arith, np.asarray(x, np.float32), np.asarray(w, np.float32))
    if swap:
        assert arith == "f16bf8"
        (xh, wh, c0), (xl8, wh8, c1), (xh8, wl8, c2) = parts
        parts = [(xh, wh, c0), (xh8, wh8, c1), (xl8, wl8, c2)]
    out = []
    for xp, wp, coef in parts:
        xp, wp = xp.astype(np.float64), wp.astype(np.float64) * coef
        out.append((xp @ wp, np.abs(xp) @ np.abs(wp)))
    return out


def layer1_epilogue(z, d, check=False):
    """act(z + b1) * s1 + o1 in fp64, step by step; check: every step is exactly representable in fp32."""
    zb = z + d["b1"]
    av = em.apply_act(zb, d["act"], d["alpha1"])
    sv = av * d["s1"]
    H = sv + d["o1"]
    if check:
        assert _f32_exact(zb) and _f32_exact(av) and _f32_exact(sv) and _f32_exact(H)
    return H


def live_layer1(arith, cin, act, seed):
    """x chunks, w1, b1, s1, o1, alpha1 whose layer-1 output H is known exactly and live in every plane.  Returns a dict; ``H`` is
    fp32 [sum(LENS), CMID] over the frames of all chunks in order (``X`` likewise), ``Mq`` = max M / q."""
    q = Q[arith]
    rng = np.random.default_rng(seed)
    mats = [_live_values(rng, (t, cin), q) for t in LENS]
    w1 = _live_values(rng, (cin, CMID), q, min(1.0, 64.0 / cin))
    d = dict(arith=arith, cin=cin, act=act, q=q, mats=mats, w1=w1)
    d["b1"] = rng.integers(-4, 5, CMID).astype(np.float32)
    d["s1"] = rng.choice([0.5, 1.0, 2.0], CMID).astype(np.float32)
    d["o1"] = (rng.integers(-8, 9, CMID) * q).astype(np.float32)
    d["alpha1"] = None
    if act == "prelu":
        d["alpha1"] = rng.choice([0.25, 0.5], CMID).astype(np.float32)
    elif act == "lrelu":
        d["alpha1"] = np.array([0.25], np.float32)
    X = np.concatenate(mats)
    tz = terms(arith, X, w1)
    z, M = sum(t[0] for t in tz), sum(t[1] for t in tz)
    # every product is a multiple of q and every partial sum stays below 2^24 q: z is exact in fp32 in ANY order
    assert all(np.array_equal(t[0] / q, np.round(t[0] / q)) for t in tz)
    d["Mq"] = float(M.max() / q)
    assert d["Mq"] + 4 / q < 2 ** 24, d["Mq"] / 2 ** 24
    H = layer1_epilogue(z, d, check=True)
    assert np.abs(H).max() < em.SPLIT8_MAX
    d["X"], d["z"], d["H"] = X, z, H.astype(np.float32)
    # the point of the exercise: the low planes of both operands and of H are live, and so is every product term in every column
    for name, v in (("x", X), ("w1", w1), ("H", d["H"])):
        nz = v != 0
        assert (low_part(arith, v)[nz] != 0).mean() >= 1.0 / 3, name
    assert all((t[1].sum(0) > 0).all() for t in tz)
    return d


def layer1_mutant(d, drop=None):
    """float32 H of an emulator that loses product term ``drop`` (1 or 2: the cross terms) of layer 1."""
    tz = terms(d["arith"], d["X"], d["w1"])
    z = sum(t[0] for i, t in enumerate(tz) if i != drop)
    return layer1_epilogue(z, d).astype(np.float32)


def select_w2(cout, act, seed):
    """One-hot layer 2: column j = channel (7 j) % 512 times 1, 2 or 0.5 -- exact in every plane, its l8 / lo plane zero.  No
    bias, no BN; the pair's act code with an exact alpha2."""
    idx = (np.arange(cout) * 7) % CMID
    val = np.array([1.0, 2.0, 0.5], np.float32)[np.arange(cout) % 3]
    w2 = np.zeros((CMID, cout), np.float32)
    w2[idx, np.arange(cout)] = val
    alpha2 = None
    if act == "prelu":
        alpha2 = np.random.default_rng(seed).choice([0.25, 0.5], cout).astype(np.float32)
    elif act == "lrelu":
        alpha2 = np.array([0.5], np.float32)
    return dict(w2=w2, idx=idx, val=val, b2=None, s2=None, o2=None, alpha2=alpha2, act=act)


def select_activation(arith, H, l2, swap=False):
    """The exactly known layer-4 activation of the select layer: act(w2_sel * decode(H)).  swap: what a kernel with the l8 and
    h8 bytes of H exchanged would form (h8 . wh8 takes the place of l8 . wh8)."""
    if swap:
        hi, _, h8 = em.split8(H)
        dec = hi.astype(np.float64) + h8.astype(np.float64) / em.LO_SCALE
    else:
        dec = decode(arith, H).astype(np.float64)
    return em.apply_act(dec[:, l2["idx"]] * l2["val"].astype(np.float64), l2["act"], l2["alpha2"])


def real_layer2(cout, act, seed):
    """Realistic layer 2 (as tests/elementwise_data.py): the folded BN scale in +-[0.5, 2], negative scales included."""
    rng = np.random.default_rng(seed)
    f = lambda a: np.asarray(a, np.float32)
    w2 = f(rng.standard_normal((CMID, cout)) / np.sqrt(CMID))
    b2 = f(0.1 * rng.standard_normal(cout))
    s2 = f(rng.uniform(0.5, 2.0, cout) * rng.choice([-1.0, 1.0], cout))
    o2 = f(rng.standard_normal(cout))
    alpha2 = None
    if act == "prelu":
        alpha2 = f(0.1 + 0.05 * rng.standard_normal(cout))
    elif act == "lrelu":
        alpha2 = np.array([0.2], np.float32)
    return dict(w2=w2, b2=b2, s2=s2, o2=o2, alpha2=alpha2, act=act)


def layer2_reference(arith, H, l2, drop=None, swap=False):
    """(a fp64, element bound e) of act(float32(H) . w2 + b2) over the emulated terms; drop / swap build the mutants."""
    tz = terms(arith, H, l2["w2"], swap)
    z = sum(t[0] for i, t in enumerate(tz) if i != drop)
    M = sum(t[1] for t in tz) + np.abs(l2["b2"].astype(np.float64))
    zb = z + l2["b2"].astype(np.float64)
    a = em.apply_act(zb, l2["act"], l2["alpha2"])
    return a, em.elementwise_bound(A_PAIR[arith], M, zb, a, None, l2["alpha2"])


def scatter(lay, rows, cout):
    """frames-in-order [sum(LENS), cout] -> packed rows [lay.rows, cout] (gap rows zero)."""
    full = np.zeros((lay.rows, cout), rows.dtype)
    full[lay.row_valid().astype(bool)] = rows
    return full


# ---------------------------------------------------------------------------------------------------------------------------
# block statistics: the exact-data rule (was in tests/test_gpu_elementwise.py) and the bound for a bounded element error
# ---------------------------------------------------------------------------------------------------------------------------
def ulp32(v):
    return np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)


def _block_refs(layout, y_full, cout):
    """Per 8-row block of the exact y: fp64 (mean, M2) of the valid rows, |mean - y0| and s2 = sum (y - y0)^2 (y0 = the block's
    first row, valid whenever any row is), and the number of valid rows."""
    valid = layout.row_valid().astype(bool)
    R = len(valid)
    nb = (R + 7) // 8
    mean, m2, tmag, s2 = (np.zeros((nb, cout)) for _ in range(4))
    cnt = np.zeros(nb, int)
    for k in range(nb):
        rows = np.arange(8 * k, min(8 * k + 8, R))
        rows = rows[valid[rows]]
        cnt[k] = len(rows)
        if len(rows):
            assert rows[0] == 8 * k
            v = y_full[rows]
            mean[k] = v.mean(0)
            m2[k] = ((v - mean[k]) ** 2).sum(0)
            tmag[k] = np.abs(mean[k] - v[0])
            s2[k] = ((v - v[0]) ** 2).sum(0)
    return mean, m2, tmag, s2, cnt


def block_failures(blk, layout, y_full, cout, exact_counts=(1, 2, 4, 8)):
    """bool [blocks, 2, cout]: where the rule of _check_blocks is violated (not finite, not exact where it must be, off by more
    than 4 ulp elsewhere); and the mask of blocks with a valid row."""
    mean, m2, tmag, s2, cnt = _block_refs(layout, y_full, cout)
    live = cnt > 0
    exact = np.isin(cnt, exact_counts)
    got = blk[:len(cnt)].astype(np.float64)
    want = np.stack([mean, m2], 1)
    tol = np.stack([4 * ulp32(np.maximum(tmag, np.abs(mean))), 4 * ulp32(s2)], 1)
    tol[exact] = 0.0
    with np.errstate(invalid="ignore"):
        bad = ~(np.abs(got - want) <= tol)                    # (a NaN fails)
    bad[~live] = False
    return bad, live


def _check_blocks(blk, layout, y_full, cout, name, exact_counts=(1, 2, 4, 8)):
    """Blocks of 1, 2, 4 or 8 valid rows: (mean, M2) exact.  Others: within 4 ulp of the fp64 statistics, the ulp taken where the
    kernels round.  They shift by the block's first row y0 (s1, s2 = sums of d = y - y0, d^2: exact on this data), then
    t = s1 * fl(1/n), mean = y0 + t, M2 = fma(-t, s1, s2): the mean is off by <= 1.5 ulp(max(|t|, |mean|)), M2 by |s1| ulp(t) +
    0.5 ulp(M2) <= 2.5 ulp(s2) (s1 t <= s2 by Cauchy-Schwarz) -- ulp(s2), not ulp(M2), since s2 - s1^2 / n cancels.
    exact_counts=(): data whose shifted sums are NOT exact in fp32 -- the 4-ulp rule for every block."""
    bad, _ = block_failures(blk, layout, y_full, cout, exact_counts)
    assert not bad.any(), (name, np.argwhere(bad)[:5].tolist())


def shifted_sums_exact(layout, y_full):
    """Are d = y - y0, d^2 and their running sums over every block exactly representable in fp32?  Only then are the statistics
    of a block of 1, 2, 4 or 8 rows exact (the premise of _check_blocks' exact branch)."""
    valid = layout.row_valid().astype(bool)
    for k in range((len(valid) + 7) // 8):
        rows = np.arange(8 * k, min(8 * k + 8, len(valid)))
        rows = rows[valid[rows]]
        if len(rows) < 2:
            continue
        dd = y_full[rows] - y_full[rows[0]]
        if not (_f32_exact(dd) and _f32_exact(dd * dd) and _f32_exact(np.cumsum(dd, 0)) and _f32_exact(np.cumsum(dd * dd, 0))):
            return False
    return True


def block_stats64(layout, y_full):
    """fp64 (mean, M2) per block as the kernels store them: float32 [blocks, 2, cout], empty blocks zero."""
    mean, m2, _, _, _ = _block_refs(layout, y_full, y_full.shape[1])
    return np.stack([mean, m2], 1).astype(np.float32)


def block_bound_ratios(arith, blk, layout, a_full, e_full, scale, shift):
    """|stored - reference| / bound [blocks, 2, cout] for an activation known to within e per element (a_full, e_full: packed rows).
    Both kernels pool the activation shifted by the block's first row; with e_mean and sum e^2 over the valid rows of a block
        |mean_a err| <= e_mean + 4 ulp(max(|t|, |mean|))            (M2(a + d) - M2(a) = 2 sum (a - mean)(d - d_mean) + sum (d - d_mean)^2)
        |M2_a err|   <= 2 sqrt(M2 sum e^2) + sum e^2 + 4 ulp(s2)
    and the folded BN (mean' = s mean + o, M2' = s^2 M2) carries them to |s| (.) + 2 ulp(|mean'|) and s^2 (.) + 2 ulp(M2').  The
    f16bf8 kernel applies the BN to the block's (mean, M2).  The bf16x3 kernel applies it to every element BEFORE it pools, v = a s
    + o (a deviation from the formula of the issue that asked for these tests, which took both kernels to scale the statistics):
    two more roundings per element, u (|s a| + |s a + o|), which this function adds to e (divided by |s|: e is in units of
    the activation) for that kernel alone -- without them a replay of its pooling on a +- e misses the M2 bound by 1e-4 of it.
    Returns (ratio, live); blocks without a valid row must be exactly zero (ratio inf otherwise)."""
    cout = a_full.shape[1]
    mean, m2, tmag, s2, cnt = _block_refs(layout, a_full, cout)
    valid = layout.row_valid().astype(bool)
    nb = len(cnt)
    s = np.ones(cout) if scale is None else np.asarray(scale, np.float64)
    o = np.zeros(cout) if shift is None else np.asarray(shift, np.float64)
    if arith == "bf16x3" and (scale is not None or shift is not None):
        e_full = e_full + em.U * (np.abs(s * a_full) + np.abs(s * a_full + o)) / np.abs(s)
    emean, e2 = np.zeros((nb, cout)), np.zeros((nb, cout))
    for k in np.flatnonzero(cnt):
        rows = np.arange(8 * k, min(8 * k + 8, len(valid)))
        rows = rows[valid[rows]]
        emean[k] = e_full[rows].mean(0)
        e2[k] = (e_full[rows] ** 2).sum(0)
    bm = emean + 4 * ulp32(np.maximum(tmag, np.abs(mean)))
    b2 = 2 * np.sqrt(m2 * e2) + e2 + 4 * ulp32(s2)
    mean_s, m2_s = s * mean + o, s * s * m2
    live = cnt > 0
    mean_s[~live] = 0.0
    bound = np.stack([np.abs(s) * bm + 2 * ulp32(mean_s), s * s * b2 + 2 * ulp32(m2_s)], 1)
    want = np.stack([mean_s, m2_s], 1)
    got = blk[:nb].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.abs(got - want) / bound
    ratio[np.isnan(ratio)] = np.inf
    ratio[~live] = np.where(got[~live] == 0, 0.0, np.inf)
    return ratio, live


# ---------------------------------------------------------------------------------------------------------------------------
# faithful fp32 replays of the kernels (CPU companion)
# ---------------------------------------------------------------------------------------------------------------------------
def _f(v):
    return np.asarray(v, np.float64).astype(np.float32).astype(np.float64)   # one fp32 rounding of an fp64 expression


def layer2_replay(arith, H, l2):
    """fp32 activation of layer 2 accumulated as the kernels do: one fp32 rounding per MFMA (its dot product exact), in the
    kernel's term order.  f16bf8: per 256-channel half, per 32-channel slab the fp16 MFMA of channels 0-15, the scaled 8-bit MFMA
    of the slab before (both cross terms, K = 64), the fp16 MFMA of channels 16-31; the halves added, then the bias.  bf16x3: one
    chain over 16 slabs of lo.hi, hi.lo, hi.hi; then the bias."""
    H = np.asarray(H, np.float32)
    parts = [(xp.astype(np.float64), wp.astype(np.float64) * c) for xp, wp, c in em._parts(arith, H, l2["w2"])]
    cout = l2["w2"].shape[1]
    dot = lambda p, sl: parts[p][0][:, sl] @ parts[p][1][sl]
    if arith == "f16bf8":
        halves = []
        for h in range(2):
            acc = np.zeros((H.shape[0], cout))
            pend = None
            for u in range(8):
                c0 = 256 * h + 32 * u
                acc = _f(acc + dot(0, slice(c0, c0 + 16)))
                if pend is not None:
                    acc = _f(acc + pend)
                acc = _f(acc + dot(0, slice(c0 + 16, c0 + 32)))
                pend = dot(1, slice(c0, c0 + 32)) + dot(2, slice(c0, c0 + 32))
            halves.append(_f(acc + pend))
        y = _f(halves[0] + halves[1])
    else:
        y = np.zeros((H.shape[0], cout))
        for u in range(16):
            sl = slice(32 * u, 32 * u + 32)
            for p in (2, 1, 0):                               # Hl . wh, Hh . wl, Hh . wh
                y = _f(y + dot(p, sl))
    zb = _f(y + l2["b2"].astype(np.float64))
    al = l2["alpha2"]
    if l2["act"] == "relu":
        return np.maximum(zb, 0.0)
    if l2["act"] in ("lrelu", "prelu"):
        return np.where(zb > 0, zb, _f(np.broadcast_to(al.astype(np.float64), zb.shape[-1:]) * zb))
    return zb


def pool_replay(arith, layout, a_full, scale, shift):
    """The kernels' shifted-sum pooling replayed with an fp32 rounding per operation, on fp32 activations a_full (packed rows).
    f16bf8 (xv_pair8.hip pool_row): d = a - a0, s1 += d, s2 = fma(d, d, s2); mean = fma(fma(s1, 1/n, a0), s, o), M2 = max(fma(-(s1
    s1), 1/n, s2), 0) (s s).  bf16x3 (xv_pair.hip): v = a s + o per element, four-row partial sums of the lane groups added, mean =
    v0 + s1 / n, M2 = max(s2 - s1 s1 / n, 0)."""
    valid = layout.row_valid().astype(bool)
    cout = a_full.shape[1]
    nb = (len(valid) + 7) // 8
    s = np.ones(cout) if scale is None else np.asarray(scale, np.float64)
    o = np.zeros(cout) if shift is None else np.asarray(shift, np.float64)
    out = np.zeros((nb, 2, cout))
    a = _f(a_full)
    for k in range(nb):
        ok = np.zeros(8, bool)
        n_here = min(8, len(valid) - 8 * k)
        ok[:n_here] = valid[8 * k:8 * k + n_here]
        n = int(ok.sum())
        if n == 0:
            continue
        rows = np.zeros((8, cout))
        rows[:n_here] = a[8 * k:8 * k + n_here]
        rn = float(np.float32(1.0) / np.float32(n))
        if arith == "f16bf8":
            s1, s2 = np.zeros(cout), np.zeros(cout)
            for r in range(1, 8):
                d = _f(rows[r] - rows[0]) if ok[r] else np.zeros(cout)
                s1 = _f(s1 + d)
                s2 = _f(d * d + s2)
            mean_a = _f(s1 * rn + rows[0])
            m2_a = np.maximum(_f(-_f(s1 * s1) * rn + s2), 0.0)
            out[k, 0] = _f(mean_a * s + o)
            out[k, 1] = _f(m2_a * _f(s * s))
        else:
            v = _f(_f(rows * s) + o)
            p1, p2 = [], []
            for g in range(2):
                t1, t2 = np.zeros(cout), np.zeros(cout)
                for r in range(4 * g, 4 * g + 4):
                    d = _f(v[r] - v[0]) if ok[r] else np.zeros(cout)
                    t1 = _f(t1 + d)
                    t2 = _f(t2 + _f(d * d))
                p1.append(t1)
                p2.append(t2)
            s1, s2 = _f(p1[0] + p1[1]), _f(p2[0] + p2[1])
            out[k, 0] = _f(v[0] + _f(s1 * rn))
            out[k, 1] = np.maximum(_f(s2 - _f(_f(s1 * s1) * rn)), 0.0)
    return out.astype(np.float32)


def seed(arith, cin, test):
    """One seed per (arithmetic, shape, test 'a' / 'c'): the GPU tests and the CPU companion build the same numbers."""
    return 1000 * ARITHS.index(arith) + cin + {"a": 0, "c": 7}[test]
