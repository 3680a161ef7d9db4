"""The cases of tests/test_gpu_wgrad_elementwise.py (shapes, operand layouts, data, the accumulation factor A), shared with the CPU
companion tests/test_wgrad_emul_cpu.py so that both look at the same numbers.

An operand is described by how it lies in its parent buffer: ``(ld, off)`` = columns [off, off + C) of a buffer ``ld`` floats wide,
``rows = (before, after)`` = that many NaN rows in front of row 0 and behind row R - 1.  Everything outside the operand is NaN: a
kernel that reaches there (a tap shift with the wrong sign, a ragged tile that takes the next row's first columns) shows it."""
import numpy as np

import arith_emul as em

WR = 32                      # rows per step of both wgrad kernels (csrc/xv_train.hip, csrc/xv_wgrad.hip)


class Case(object):
    def __init__(self, name, R, cin, cout, K, dil, xs=None, zs=None, rows=(0, 0), relu=False, kind="int", seed=0):
        self.name, self.R, self.cin, self.cout, self.K, self.dil = name, R, cin, cout, K, dil
        self.xs, self.zs = xs or (cin, 0), zs or (cout, 0)            # (ld, off)
        self.rows, self.relu, self.kind, self.seed = rows, relu, kind, seed
        assert self.xs[0] >= self.xs[1] + cin and self.zs[0] >= self.zs[1] + cout

    # ---- data ---------------------------------------------------------------------------------------------------------------
    def data(self):
        """(x [R, Cin], dz [R, Cout]) fp32."""
        rng = np.random.default_rng(7000 + self.seed + self.R + 3 * self.cin + 5 * self.cout + 7 * self.K + self.dil)
        R, cin, cout = self.R, self.cin, self.cout
        if self.kind == "int":                    # integers in [-3, 3], about half zeros; x >= 0 as after a ReLU where asked
            x = rng.integers(-3, 4, (R, cin)) * (rng.random((R, cin)) < 0.58)
            dz = rng.integers(-3, 4, (R, cout)) * (rng.random((R, cout)) < 0.58)
            if self.relu:
                x = np.abs(x)
        else:
            if self.kind == "relu":               # post-ReLU activations: non-negative, about half zeros
                x = np.maximum(rng.standard_normal((R, cin)) * 1.5, 0)
            else:                                 # hostile: the channel scales of elementwise_data.Case.data (three decades, dead channels)
                ch = 10.0 ** rng.uniform(-2, 1, cin)
                ch[rng.random(cin) < 0.06] = 0
                x = np.maximum(rng.standard_normal((R, cin)) + 0.3, 0) * ch
            col = 10.0 ** rng.uniform(-4, -1, cout)                     # dz: per-column scales over three decades, non-zero column mean
            dz = (rng.standard_normal((R, cout)) + 0.25 * rng.standard_normal(cout)) * col
        return np.ascontiguousarray(x, np.float32), np.ascontiguousarray(dz, np.float32)

    def place(self, a, which):
        """The parent buffer of operand ``which`` ("x" | "dz"), NaN wherever the operand is not, and the index of the operand in it."""
        ld, off = self.xs if which == "x" else self.zs
        before, after = self.rows
        buf = np.full((before + a.shape[0] + after, ld), np.nan, np.float32)
        idx = (slice(before, before + a.shape[0]), slice(off, off + a.shape[1]))
        buf[idx] = a
        return buf, idx

    # ---- the accumulation chain -----------------------------------------------------------------------------------------------
    def splits(self, workspace_bytes):
        """Row splits of a launch, from the public xv_wgrad_workspace_bytes (0 = one split, straight into dw)."""
        per = self.K * self.cin * self.cout * 4
        assert workspace_bytes % per == 0
        return max(1, workspace_bytes // per)

    def rows_per_split(self, splits):
        return ((self.R + splits - 1) // splits + WR - 1) // WR * WR

    def A(self, arith, splits):
        """sqrt(depth), lambda = 1.  depth = accumulator updates of one split (fp32: one per 32x32x2 MFMA, 2 rows; bf16x3: 3 MFMAs
        per 16 rows) + the splits - 1 additions of the ordered merge."""
        rps = self.rows_per_split(splits)
        depth = (rps / 2.0 if arith == "fp32" else 3.0 * rps / 16.0) + splits - 1
        return em.accum_factor(depth)


def exact_ref(x, dz, K, dil):
    """int64 dw[K, Cin, Cout] and db[Cout] of integer-valued x, dz."""
    xi, zi = np.asarray(x).astype(np.int64), np.asarray(dz).astype(np.int64)
    assert np.array_equal(xi, x) and np.array_equal(zi, dz)
    R = xi.shape[0]
    assert R * 9 < 2 ** 24                        # every partial sum is an integer below 2^24: exact in fp32, and the bf16 lo planes are zero
    h = (K - 1) // 2
    # (float64 BLAS on integers below 2^53 is exact and much faster than numpy's int64 matmul)
    xf, zf = xi.astype(np.float64), zi.astype(np.float64)
    dw = np.stack([em._shifted(xf, (k - h) * dil).T @ zf for k in range(K)])
    return dw.astype(np.int64), zi.sum(0)


def db_bound(dz):
    """|db - sum dz| <= 15 2^-24 sum |dz| + 2^-24 |db|: 15 fp32 additions inside a 16-row step (worst case, no sqrt), double outside,
    one cast."""
    z = np.asarray(dz, np.float64)
    return 15 * em.U * np.abs(z).sum(0) + em.U * np.abs(z.sum(0))


C = Case
# ---- (a) exact known answers: what each case is there for --------------------------------------------------------------------
EXACT_CASES = [
    # R below one 32-row step / at the 16-row half and the step boundaries; K in {1, 3, 5, 7}, dilation in {1, 2, 3}
    C("R1 K5 (reach 2 > R: outer taps zero)", 1, 24, 64, 5, 1),
    C("R2 K7 d3 (reach 9: only the centre tap) scalar", 2, 23, 10, 7, 3),
    C("R5 K7 d2 (R < (K-1)d/2 = 6) 512x512", 5, 512, 512, 7, 2, relu=True),
    C("R15 K3 d2, C % 4 == 0 but not % 128", 15, 40, 48, 3, 2, relu=True),
    C("R16 K3, cin 128 cout 129 (second tile: one channel) scalar", 16, 128, 129, 3, 1),
    C("R17 K5 d2, cin 129 cout 128 scalar", 17, 129, 128, 5, 2),
    C("R31 K3 d3, 130 x 257 scalar", 31, 130, 257, 3, 3, relu=True),
    C("R32 K7, 64 x 96", 32, 64, 96, 7, 1),
    C("R33 K1, 96 x 10 scalar", 33, 96, 10, 1, 1),
    C("R300 K1 1536 x 512", 300, 1536, 512, 1, 1, relu=True),
    # the split rule: one split up to 4096 rows, then the ordered merge
    C("R4096 K3 (one split)", 4096, 132, 64, 3, 1),
    C("R4097 K5 (9 splits of 480)", 4097, 64, 130, 5, 1, relu=True),
    C("R19000 K7 512x512 (training shape: 9 splits of 2112, last one 2104 rows)", 19000, 512, 512, 7, 1, relu=True),
    # column slices of wider buffers (left: off 0, right: off = ld - C), NaN outside
    C("layer 0: 23 of 24 columns, dz right slice", 70, 23, 512, 5, 1, xs=(24, 0), zs=(1024, 512)),
    C("x right slice of 1024, dz left slice of 100 (vector path)", 100, 512, 96, 3, 2, xs=(1024, 512), zs=(100, 0), relu=True),
    C("ld % 4 != 0 with C % 4 == 0 (scalar path)", 45, 64, 64, 3, 1, xs=(67, 3), zs=(66, 0)),
    C("middle slice at column 1, ld % 4 == 0 (4-byte aligned only)", 45, 64, 64, 3, 1, xs=(72, 1), zs=(72, 5)),
    C("ragged tiles in slices: 129 of 200, 130 of 131", 40, 129, 130, 5, 1, xs=(200, 71), zs=(131, 0)),
    # row slices: NaN rows before row 0 and after row R - 1, where a wrong tap shift reaches
    C("row slice K5 d3, 8 NaN rows each side", 64, 40, 48, 5, 3, rows=(8, 8), relu=True),
    C("row slice scalar path K7 d1", 33, 23, 10, 7, 1, rows=(4, 4)),
    C("row + column slices under the split (10 splits of 512)", 5000, 64, 64, 3, 2, xs=(128, 64), zs=(96, 0), rows=(12, 12)),
]
SPLIT_CASES = ("R4097", "R19000", "row + column slices under the split")      # must report a workspace

# ---- (b) one-hot read-back ---------------------------------------------------------------------------------------------------
ONEHOT_CASES = [
    C("R70 K5 d2", 70, 40, 48, 5, 2),
    C("R33 K3 ragged 129 x 130", 33, 129, 130, 3, 1, xs=(133, 4)),
    C("R4500 K7 d3 (9 splits of 512)", 4500, 64, 64, 7, 3, rows=(24, 24)),
]


def onehot_rows(case, splits):
    """r* of the read-back: both ends, the 16-row half and the 32-row step boundaries, the first and last row of every split, rows
    within the tap reach of both ends."""
    R = case.R
    reach = (case.K - 1) // 2 * case.dil
    rps = case.rows_per_split(splits)
    want = {0, R - 1, 15, 16, 31, 32, reach - 1, reach, reach + 1, R - reach - 2, R - reach - 1, R - reach, 1, R - 2}
    for s in range(splits):
        want |= {s * rps, min(R, (s + 1) * rps) - 1}
    return sorted(r for r in want if 0 <= r < R)


def onehot_x(case):
    """General fp32 values: six decades, both signs, subnormals, zeros (no -0: a sum that starts at +0 cannot return it)."""
    rng = np.random.default_rng(99 + case.R)
    x = rng.standard_normal((case.R, case.cin)) * 10.0 ** rng.uniform(-3, 3, (case.R, case.cin))
    x = x.astype(np.float32)
    sel = rng.random(x.shape)
    x[sel < 0.05] = 0.0
    sub = (sel >= 0.05) & (sel < 0.10)
    x[sub] = (rng.integers(1, 2 ** 23, int(sub.sum())).astype(np.uint32) | (rng.integers(0, 2, int(sub.sum())).astype(np.uint32) << 31)).view(np.float32)
    return x


# ---- (c) element-wise bounds -------------------------------------------------------------------------------------------------
BOUND_CASES = [
    C("relu 300 x 512 x 512 K5", 300, 512, 512, 5, 1, kind="relu"),
    C("hostile 1000 x 96 x 200 K3 d2", 1000, 96, 200, 3, 2, kind="hostile"),
    C("relu layer 0: 2000 x 23 (of 24) x 512 K5", 2000, 23, 512, 5, 1, xs=(24, 0), kind="relu"),
    C("hostile 4097 x 130 x 257 K7 (9 splits)", 4097, 130, 257, 7, 1, kind="hostile"),
    C("relu 9000 x 256 x 384 K3 (18 splits)", 9000, 256, 384, 3, 1, zs=(512, 128), kind="relu"),
]
