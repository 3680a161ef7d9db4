"""Cases, data builders, fp64 references, the replay of the summation order and the bound functions of the per-tile tests of the two
fused epilogues of tdnn_gemm_bf16x3_kernel (csrc/xv_gemm3.hip, the block under `if (sums)` that Gemm3Params::cs_part / cs_r switch
on): xv_tdnn_layer_bf16x3_sums and xv_tdnn_layer_bf16x3_moments (tests/test_gpu_gemm_sums_elementwise.py and its CPU companion
tests/test_gemm_sums_bounds_cpu.py).  Everything here is NumPy; nothing needs the GPU.

What the epilogue does (read from the source)
---------------------------------------------
launch_gemm3 forces 128-row tiles when cs_part is set (`if (p.cs_part) wm = 2`): WM = 2, NT = 256 threads, NG = NT / 16 = 16 row
groups.  Thread tid holds the 8-column group cg = tid & 15 of the 128-column tile and the row group g = tid >> 4; it walks the
rows lr = g + 16 j, j = 0..7, of the tile in that order and skips rows past R (`if (gr >= p.R) continue`).  Per row it forms
v = (act(T + bias) * scale + shift) * keep, keep = 0 on a gap row (row_valid[gr] == 0) and 1 elsewhere (row_valid NULL: 1), stores
v as y, and accumulates

  _sums    (cs_r given):  cs1 += v in fp32 (starts at +0: the first addition is exact, 7 roundings),
                          cs2 = fmaf(v, r, cs2) in fp32 (the fused multiply-add is written in the source: 8 roundings); r is the
                          row gr of sum_r, stride ld_sum_r, fetched for every row below R whether valid or not -- a gap row
                          contributes v * r = 0 * r, which is 0 for every FINITE r;
  _moments (cs_r NULL):   ds1 += (double)v, ds2 = fma(d, d, ds2) in double (d * d of an fp32 number is exact in double, so the
                          fused and the plain form have the same bits: 7 and 8 roundings of 2^-53).

The 16 group sums of a column go through LDS as doubles (the fp32 ones converted exactly) and are added IN GROUP ORDER starting from
0.0: 15 roundings of 2^-53.  The result is stored at cs_part[(mt * 2 + which) * cout + column] for every column below cout; the
columns of a ragged last column tile come in whole 8-column groups (cout % 8 == 0 is the entry points' condition).  A tile made of
gap rows only stores sums of zeros: exact zeros, not "left alone".  The byte count of the workspace is ceil(R / 128) * 2 * cout * 8
(xv_col_sums_workspace_bytes).

Reference
---------
The reference of a slot is the fp64 sum (long double, rounded once) of the terms over the tile's rows [128 mt, min(128 (mt + 1),
R)): y and y * r for _sums, r and r^2 for _moments, formed from the fp32 rows THE KERNEL ITSELF WROTE (y * r and r * r of fp32
numbers are exact in long double).  Those rows are pinned separately: bit-identical to xv_tdnn_layer_bf16x3 on the same arguments,
which tests/test_gpu_elementwise.py holds element by element.  So a bound here measures the epilogue's summation alone.

Bounds (count without compiler contraction, as tests/bnback_data.py: contraction removes roundings; SLACK = 1 + 2^-10 carries the
second-order terms; U = 2^-24)
----------------------------------------------------------------------------------------------------------------------------
Every rounding of a running sum is relative to a partial sum of magnitude <= sum |terms| of the thread, and the threads' errors add
up to at most the same constant times sum_tile |terms|.

  _sums:     a thread makes 7 fp32 additions for sum y and 8 fused roundings for sum y r; both are covered by C_SUMS = 8.  The 15
             double additions are 15 * 2^-53 < 2^-49:   |part - ref| <= 8 * 2^-24 * sum_tile |term| * SLACK + 2^-48 * sum_tile |term|
  _moments:  double throughout, 8 + 15 = 23 roundings of 2^-53 < 2^-48:   |part - ref| <= 2^-48 * sum_tile |term|

These are the counts the source gives; they equal the ones stated with the task, nothing was changed after reading the code and
none of the constants is fitted: they were fixed before the first device run.  (The replay forms fmaf(v, r, cs2) as the fp64 sum
v * r + cs2 rounded to fp32: a double rounding that can differ from the fused result by 2^-29 ulp, far inside SLACK.)

Exact cases
-----------
x and w are integers in [-3, 3], the bias an integer in [-4, 4], the scale in {0.5, 1, 2}, the shift a multiple of 1/2 in [-2, 2],
alpha 0.25 or 0.5, sum_r integers in [0, 3].  Integers of that size are bf16 numbers (lo plane 0), the MFMAs add integers:
|z| <= 9 K cin + 4 <= 9 * 7 * 128 + 4 = 8068 < 2^13.  alpha z is a multiple of 1/4, times the scale a multiple of 1/8 with
|.| <= 2 * 8068, plus the shift: v is a multiple of 1/8 with |v| <= 16138 < 2^14, i.e. 17 bits.  A thread's fp32 sums: |sum y| <=
8 * 16138 < 2^17 (multiples of 1/8: 20 bits) and |sum y r| <= 8 * 3 * 16138 < 2^19 (multiples of 1/8: 22 bits): under 24 bits,
every fp32 operation is exact with or without fusing.  In _moments v^2 is a multiple of 1/64 below 2^28 (34 bits) and a tile's sum
of 128 of them stays below 2^35 (41 bits < 53): exact in double.  So every slot EQUALS the fp64 reference.  The CPU companion
asserts per case that every intermediate of the replay is exact and below 2^24 units of 1/8, and that a neighbouring case
(alpha = 0.3) is not exact.  Gap rows of sum_r hold +-3e38 (finite: 0 * 3e38 = 0), rows past R of every parent buffer NaN.

Forms (launch_gemm3's own rules, asserted per case by form_of): fp32-row input -> kt = 0 ("f32"); split input -> kt = K, and the
16 x 16 MFMA form ("split16") iff K > 1 and the number of 32-channel slabs ceil(cin / 32) is even, else the 32 x 32 form
("split32"); split input with K > 1 needs 2 <= (K - 1) * dilation <= 8."""
import numpy as np

import bnback_data as bd
import elementwise_data as ed
import pool_data as pd

U, F, D, SLACK = bd.U, bd.F, bd.D, bd.SLACK
LD = np.longdouble
TILE, GROUPS, THREAD_ROWS, COL_GROUP = 128, 16, 8, 8
C_SUMS = 8                              # fp32 roundings of a thread's running sum (7 for sum y, 8 for sum y r)
C_DOUBLE = 2.0 ** -48                   # > 23 * 2^-53: every double rounding of a slot
BIG = 3e38                              # what the gap rows of sum_r hold when row_valid is given
PAD_ROWS = 3                            # rows past R of every parent buffer (NaN)
ACT_CODE = {"none": 0, "relu": 1, "lrelu": 2, "prelu": 3}
RAGGED = (37, 1, 80, 2, 129, 130, 200, 64)        # gap 3: a gap over rows 127..129, chunks over 256, 384, 512, 640; 670 rows
GAP_TILE = ((3, 97), (260, 70), 333)              # (start, length) x 2, R: rows 128..255 are gap rows only
LARGE_MEAN_CHANNEL = 5


class Case(object):
    """entry: "sums" / "moments".  form: "f32" / "split32" / "split16".  rows: a row count, "ragged" or "gaptile".  valid: whether
    row_valid is passed.  epi: bias, scale, shift passed (_sums: else all NULL and no activation -- the trainer's form; _moments: the
    bias is always passed, scale and shift only with epi).  wide: y, sum_r, y_preact are column slices of wider parents."""

    def __init__(self, name, entry, form, cin, cout, K, dil, rows, valid, act, epi, ypre=False, wide=True, kind=None, seed=0, alpha=None):
        self.name, self.entry, self.form, self.cin, self.cout, self.K, self.dil = name, entry, form, cin, cout, K, dil
        self.rows, self.valid, self.act, self.epi, self.ypre, self.wide = rows, valid, act, epi, ypre, wide
        self.kind, self.seed, self.alpha = kind, seed, alpha
        self.exact = kind is None
        self.split = form != "f32"

    def but(self, **kw):
        c = Case.__new__(Case)
        c.__dict__.update(self.__dict__)
        c.__dict__.update(kw)
        return c


def form_of(split, K, cin, dil):
    """The kernel form launch_gemm3 selects (its conditions, restated): -> "f32" / "split32" / "split16"."""
    assert K in (1, 3, 5, 7) and dil >= 1 and (K - 1) * dil <= 8
    if not split:
        assert cin % 4 == 0
        return "f32"
    assert K == 1 or 2 <= (K - 1) * dil <= 8
    slabs = -(-cin // 32)
    return "split16" if K > 1 and slabs % 2 == 0 else "split32"


C = Case
EXACT_CASES = [
    # ---- xv_tdnn_layer_bf16x3_sums
    C("sums f32 K1 R1 cout8 trainer", "sums", "f32", 40, 8, 1, 1, 1, False, "none", False),
    C("sums f32 K3d2 R127 cout136 lrelu epi", "sums", "f32", 24, 136, 3, 2, 127, True, "lrelu", True),
    C("sums f32 K5 R129 cout192 trainer", "sums", "f32", 64, 192, 5, 1, 129, True, "none", False, wide=False),
    C("sums f32 K7 ragged cout256 prelu epi", "sums", "f32", 40, 256, 7, 1, "ragged", True, "prelu", True),
    C("sums split32 K1 R128 cout136 trainer", "sums", "split32", 96, 136, 1, 1, 128, False, "none", False),
    C("sums split32 K3d4 ragged cout256 trainer", "sums", "split32", 32, 256, 3, 4, "ragged", True, "none", False),
    C("sums split32 K5d2 R129 cout8 relu epi", "sums", "split32", 96, 8, 5, 2, 129, True, "relu", True),
    C("sums split16 K3 R127 cout192 trainer", "sums", "split16", 64, 192, 3, 1, 127, False, "none", False),
    C("sums split16 K5 ragged cout256 trainer", "sums", "split16", 128, 256, 5, 1, "ragged", True, "none", False, wide=False),
    C("sums split16 K7 gaptile cout136 trainer", "sums", "split16", 64, 136, 7, 1, "gaptile", True, "none", False),
    C("sums split16 K5d2 R1 cout8 lrelu epi", "sums", "split16", 128, 8, 5, 2, 1, True, "lrelu", True, alpha=0.5),
    C("sums split16 K3d2 R128 cout256 relu epi", "sums", "split16", 64, 256, 3, 2, 128, True, "relu", True),
    # ---- xv_tdnn_layer_bf16x3_moments
    C("moments f32 K5 ragged cout136 relu ypre", "moments", "f32", 24, 136, 5, 1, "ragged", True, "relu", False, ypre=True),
    C("moments f32 K3d4 R129 cout8 lrelu", "moments", "f32", 40, 8, 3, 4, 129, False, "lrelu", True),
    C("moments f32 K1 R127 cout256 prelu ypre", "moments", "f32", 64, 256, 1, 1, 127, True, "prelu", True, ypre=True),
    C("moments split32 K7 gaptile cout192 relu", "moments", "split32", 96, 192, 7, 1, "gaptile", True, "relu", False, wide=False),
    C("moments split32 K1 ragged cout256 lrelu ypre", "moments", "split32", 32, 256, 1, 1, "ragged", True, "lrelu", False, ypre=True),
    C("moments split32 K3d2 R129 cout136 none ypre", "moments", "split32", 96, 136, 3, 2, 129, True, "none", True, ypre=True),
    C("moments split16 K5d2 ragged cout136 prelu", "moments", "split16", 64, 136, 5, 2, "ragged", True, "prelu", True),
    C("moments split16 K3 R128 cout192 relu ypre", "moments", "split16", 128, 192, 3, 1, 128, False, "relu", False, ypre=True),
    C("moments split16 K7 R1 cout8 lrelu ypre", "moments", "split16", 64, 8, 7, 1, 1, True, "lrelu", True, ypre=True, alpha=0.5),
]
BOUND_CASES = [
    C("sums f32 K5 relu trainer", "sums", "f32", 64, 136, 5, 1, "ragged", True, "none", False, kind="relu", seed=1),
    C("sums f32 K7 hostile prelu epi", "sums", "f32", 40, 256, 7, 1, "ragged", True, "prelu", True, kind="hostile", seed=2),
    C("sums split32 K5 relu relu epi", "sums", "split32", 96, 192, 5, 1, "ragged", True, "relu", True, kind="relu", seed=3),
    C("sums split32 K7 hostile trainer", "sums", "split32", 96, 136, 7, 1, "ragged", True, "none", False, kind="hostile", seed=4),
    C("sums split16 K5 hostile trainer", "sums", "split16", 128, 256, 5, 1, "ragged", True, "none", False, kind="hostile", seed=5,
      wide=False),
    C("sums split16 K7 relu trainer", "sums", "split16", 64, 192, 7, 1, "ragged", True, "none", False, kind="relu", seed=6),
    C("moments f32 K5 relu relu ypre", "moments", "f32", 64, 136, 5, 1, "ragged", True, "relu", False, ypre=True, kind="relu", seed=7),
    C("moments f32 K7 hostile lrelu", "moments", "f32", 40, 192, 7, 1, "ragged", True, "lrelu", True, kind="hostile", seed=8),
    C("moments split32 K5 hostile prelu", "moments", "split32", 96, 256, 5, 1, "ragged", True, "prelu", False, kind="hostile", seed=9),
    C("moments split32 K7 relu relu", "moments", "split32", 32, 136, 7, 1, "ragged", True, "relu", False, kind="relu", seed=10),
    C("moments split16 K5 relu relu ypre", "moments", "split16", 128, 192, 5, 1, "ragged", True, "relu", False, ypre=True, kind="relu",
      seed=11, wide=False),
    C("moments split16 K7 hostile lrelu", "moments", "split16", 64, 256, 7, 1, "ragged", True, "lrelu", True, kind="hostile", seed=12),
]
del C
FORMS = ("f32", "split32", "split16")
# what the exact cases have to reach between them (asserted by the CPU companion)
NEED_TAPS = {(1, 1), (3, 1), (3, 2), (3, 4), (5, 1), (5, 2), (7, 1)}
NEED_ROWS = {1, 127, 128, 129, "ragged", "gaptile"}
NEED_COUT = {8, 136, 192, 256}


# ---------------------------------------------------------------------------------------------------------------------------
# rows and data
# ---------------------------------------------------------------------------------------------------------------------------
def rows_of(case):
    """(R, valid): valid[r] is False on a gap row.  A row count: no gap rows without row_valid, one in the middle with it (R > 1)."""
    if case.rows == "ragged":
        rs, R = pd.layout(RAGGED, 3)
        return R, bd.valid_of(rs, RAGGED, R)
    if case.rows == "gaptile":
        (s0, n0), (s1, n1), R = GAP_TILE
        return R, bd.valid_of((s0, s1), (n0, n1), R)
    R = int(case.rows)
    valid = np.ones(R, bool)
    if case.valid and R > 1:
        valid[R // 2] = False
    return R, valid


def tiles(R):
    return -(-R // TILE)


def workspace_bytes(R, cout):
    return tiles(R) * 2 * cout * 8


def build(case):
    """-> dict(R, valid, x [R, cin], w [K, cin, cout], b, scale, shift, alpha (None = NULL), act, sum_r [R, cout] or None).  Every
    row of x holds data, gap rows included (the mask, not a zero input, must keep them out).  `valid` is all True where the case
    passes no row_valid."""
    assert form_of(case.split, case.K, case.cin, case.dil) == case.form, case.name
    assert case.valid or isinstance(case.rows, int)
    R, valid = rows_of(case)
    cin, cout, K = case.cin, case.cout, case.K
    rng = np.random.default_rng(4242 + case.seed + 7 * cin + 3 * cout + K + case.dil)
    passed = case.entry == "moments" or case.epi           # whether the epilogue gets any parameter at all
    act = case.act if passed else "none"
    if case.exact:
        x = rng.integers(-3, 4, (R, cin)).astype(F)
        w = (rng.integers(-3, 4, (K, cin, cout)) * (rng.random((K, cin, cout)) < 0.5)).astype(F)
        b = rng.integers(-4, 5, cout).astype(F)
        scale = rng.choice([0.5, 1.0, 2.0], cout).astype(F)
        shift = (rng.integers(-4, 5, cout) * 0.5).astype(F)
        a0 = 0.25 if case.alpha is None else case.alpha
        alpha = {"lrelu": np.array([a0], F), "prelu": rng.choice([0.25, 0.5], cout).astype(F)}.get(act)
        r = rng.integers(0, 4, (R, cout)).astype(F)
    else:
        mats, w, b, scale, shift, alpha = ed.Case(case.name, "bf16x3", "bf16x3", cin, cout, K, case.dil, act, case.kind, seed=case.seed).data()
        x = np.concatenate(mats)[:R]
        assert len(x) == R
        b[LARGE_MEAN_CHANNEL] = 300.0                        # mean^2 / var ~ 1e5 in that channel
        r = (np.maximum(rng.standard_normal((R, cout)), 0) * 1.7).astype(F)           # post-ReLU rows
        if case.kind == "hostile":
            r = (r * 10.0 ** rng.uniform(-2, 1, cout)).astype(F)                       # column scales over three decades
    if not passed:
        b = scale = shift = alpha = None
    elif not case.epi:
        scale = shift = None
    if case.valid:
        r[~valid] = np.where(np.arange(int((~valid).sum())) % 2 == 0, BIG, -BIG).astype(F)[:, None]
    return dict(R=R, valid=valid, x=x, w=w, b=b, scale=scale, shift=shift, alpha=alpha, act=act,
                sum_r=r if case.entry == "sums" else None)


def layer_rows(case, d):
    """What the layer writes, evaluated in fp64 and rounded to fp32 once: dict(y masked, y_raw unmasked, ypre = z + b).  Output row
    t reads the input rows t + (k - (K - 1) / 2) * dilation, rows outside [0, R) as zeros.  On the exact cases this IS the kernel's
    output (asserted representable); on the bound cases it stands in for it on the CPU."""
    x, w = d["x"].astype(D), d["w"].astype(D)
    R, K, h = d["R"], case.K, (case.K - 1) // 2
    z = np.zeros((R, case.cout), D)
    for k in range(K):
        off = (k - h) * case.dil
        src = np.zeros_like(x)
        lo, hi = max(0, -off), min(R, R - off)
        if hi > lo:
            src[lo:hi] = x[lo + off:hi + off]
        z += src @ w[k]
    if d["b"] is not None:
        z = z + d["b"].astype(D)
    a = d["alpha"].astype(D) if d["alpha"] is not None else None
    if d["act"] == "relu":
        v = np.maximum(z, 0)
    elif d["act"] == "lrelu":
        v = np.maximum(a[0] * z, z)
    elif d["act"] == "prelu":
        v = np.maximum(z, 0) + a * np.minimum(z, 0)
    else:
        v = z
    if d["scale"] is not None:
        v = v * d["scale"].astype(D)
    if d["shift"] is not None:
        v = v + d["shift"].astype(D)
    y = np.where(d["valid"][:, None], v, 0.0)
    if case.exact and case.alpha in (None, 0.25, 0.5):
        assert bd.representable(y) and bd.representable(v) and bd.representable(z)
    return dict(y=y.astype(F), y_raw=v.astype(F), ypre=z.astype(F))


def wide_of(a, ld, col0):
    """[R + PAD_ROWS, ld] NaN-filled parent with a in its rows [0, R), columns [col0, col0 + C)."""
    parent = np.full((a.shape[0] + PAD_ROWS, ld), np.nan, F)
    parent[:a.shape[0], col0:col0 + a.shape[1]] = a
    return parent


def geometry(case):
    """(ldy, y col0, ld_sum_r, r col0, ldpre, ypre col0): every ld a multiple of 4, every col0 a multiple of 4 (16-byte aligned)."""
    c = case.cout
    return (c + 12, 4, c + 20, 8, c + 8, 4) if case.wide else (c, 0, c, 0, c, 0)


# ---------------------------------------------------------------------------------------------------------------------------
# reference, bound, replay
# ---------------------------------------------------------------------------------------------------------------------------
def terms(entry, y, r):
    yl = np.asarray(y, F).astype(LD)
    with np.errstate(all="ignore"):
        return yl, (yl * np.asarray(r, F).astype(LD) if entry == "sums" else yl * yl)


def parts_ref(entry, y, r=None):
    """(ref, mag) [tiles, 2, C] in fp64: the sum of the terms over each tile's rows and the sum of their magnitudes."""
    R, C = y.shape
    ref, mag = np.zeros((tiles(R), 2, C), D), np.zeros((tiles(R), 2, C), D)
    for k, t in enumerate(terms(entry, y, r)):
        for mt in range(tiles(R)):
            blk = t[mt * TILE:(mt + 1) * TILE]
            ref[mt, k], mag[mt, k] = blk.sum(0).astype(D), np.abs(blk).sum(0).astype(D)
    return ref, mag


def parts_bound(entry, mag):
    return (C_SUMS * U * SLACK + C_DOUBLE) * mag if entry == "sums" else C_DOUBLE * mag


BROKEN = ("drop15", "rows8g", "gaps", "stride", "tail", "shift", "colgroup", "neighbour", "fp32")


def replay_parts(entry, y, r=None, broken=None, y_raw=None, r_parent=None, r_col0=0, track=None):
    """[tiles, 2, C] fp64 partials in the epilogue's order: the thread (g, cg) takes the rows g + 16 j, j = 0..7, of the tile in fp32
    (_sums) or double (_moments); the groups g = 0..15 are then added in double.  Rows past R are skipped (adding +0 instead has
    the same bits).  track: a dict that receives the largest |intermediate| of the fp32 sums and the number of inexact fp32 steps.

    broken: "drop15" row group 15 dropped / "rows8g" rows 8 g + j (another order: the same answer in exact arithmetic) / "gaps" the
    unmasked rows y_raw summed / "stride" r read with stride C from the slice's first element inside r_parent / "tail" the last
    tile summed over 128 rows (NaN past R) / "shift" tile mt stored at mt + 1 / "colgroup" the last 8 columns left unwritten (NaN) /
    "neighbour" r of the next row / "fp32" fp32 accumulation in _moments."""
    R, Cc = y.shape
    nt = tiles(R)
    if broken == "gaps":
        y = y_raw
    if entry == "sums":
        if broken == "stride":
            r = r_parent.reshape(-1)[r_col0:r_col0 + R * Cc].reshape(R, Cc)
        elif broken == "neighbour":
            r = np.roll(r, -1, axis=0)
    fill = np.nan if broken == "tail" else 0.0

    def tile_of(a, mt):
        t = np.full((TILE, Cc), fill, F)
        blk = a[mt * TILE:(mt + 1) * TILE]
        t[:len(blk)] = blk
        if broken == "rows8g":
            return t.reshape(GROUPS, THREAD_ROWS, Cc).transpose(1, 0, 2)        # [j, g]: row 8 g + j
        return t.reshape(THREAD_ROWS, GROUPS, Cc)                                # [j, g]: row g + 16 j

    part = np.full((nt + 1, 2, Cc), np.nan, D)
    first = 1 if broken == "shift" else 0
    with np.errstate(all="ignore"):
        for mt in range(nt):
            Y = tile_of(y, mt)
            if entry == "sums" or broken == "fp32":
                Rr = tile_of(r, mt) if entry == "sums" else Y
                s1, s2 = np.zeros((GROUPS, Cc), F), np.zeros((GROUPS, Cc), F)
                for j in range(THREAD_ROWS):
                    e1 = s1.astype(D) + Y[j].astype(D)
                    e2 = s2.astype(D) + Y[j].astype(D) * Rr[j].astype(D)
                    s1, s2 = e1.astype(F), e2.astype(F)
                    if track is not None:
                        track["max"] = max(track.get("max", 0.0), float(np.abs(e1).max()), float(np.abs(e2).max()))
                        track["inexact"] = track.get("inexact", 0) + int((s1.astype(D) != e1).sum() + (s2.astype(D) != e2).sum())
                d1, d2 = s1.astype(D), s2.astype(D)
            else:
                d1, d2 = np.zeros((GROUPS, Cc), D), np.zeros((GROUPS, Cc), D)
                for j in range(THREAD_ROWS):
                    v = Y[j].astype(D)
                    d1, d2 = d1 + v, d2 + v * v
            a1, a2 = np.zeros(Cc, D), np.zeros(Cc, D)
            for g in range(GROUPS - 1 if broken == "drop15" else GROUPS):
                a1, a2 = a1 + d1[g], a2 + d2[g]
            part[mt + first, 0], part[mt + first, 1] = a1, a2
    if broken == "colgroup":
        part[:, :, Cc - COL_GROUP:] = np.nan
    return part[:nt]


def fold_ref(parts, N):
    """fp64 (mean, var, bound of mean, bound of var) of xv_bn_moments_fold_f32 FROM THE PARTIALS HANDED IN: the merge is the one of
    xv_col_sums_merge_f32 (bnback_data.col_sums_ref with the partials as its rows: one rounding to fp32 and DUST times the summed
    magnitudes), divided by N; var = S2 / N - mean^2 carries the dust of both of its terms."""
    s1, _, b1, _ = bd.col_sums_ref(parts[:, 0], None)
    s2, _, b2, _ = bd.col_sums_ref(parts[:, 1], None)
    n = D(F(N))
    m = s1 / n
    v = np.maximum(s2 / n - m * m, 0.0)
    dust1 = (b1 - bd.ulp32(s1) / 2) / n
    dust2 = (b2 - bd.ulp32(s2) / 2) / n
    return m, v, bd.ulp32(m) / 2 + dust1 + bd.DUST * np.abs(m), bd.ulp32(v) / 2 + dust2 + 2 * np.abs(m) * dust1 + bd.DUST * (s2 / n + m * m)
