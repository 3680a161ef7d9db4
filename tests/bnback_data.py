"""Cases, data builders, fp64 references, float32 replays and bound functions of the element-wise tests of the batch-norm / pooling
BACKWARD family of csrc/xv_train.hip (tests/test_gpu_bnback_elementwise.py and its CPU companion tests/test_bnback_bounds_cpu.py).

Everything here is NumPy; nothing needs the GPU.  U = 2^-24 is the unit roundoff of fp32: |fl(x) - x| <= U |x| for one correctly
rounded operation.  The build recipe (FLAGS of x-vector-kaldi-tf_amd/csrc/Makefile: -O3 -std=c++17 -fPIC, nothing else that touches
arithmetic; the CPU companion reads that line and asserts it has no fast-math or approximate-divide switch) leaves hipcc's default,
so fp32 division and sqrtf are the correctly rounded sequences (v_div_scale / v_div_fmas / v_div_fixup, v_sqrt + fix-up) and
denormals are kept.  The compiler contracts a * b + c into one FMA
where it likes: that removes roundings, never adds one, so every count below is for the form WITHOUT contraction (the replay rounds
every operation) and holds for the kernel a fortiori.  Second-order terms: the factor SLACK = 1 + 2^-10; underflow: TINY = 2^-126.

The reference of every bound is the fp64 evaluation of the kernel's formula ON THE fp32 INPUTS THE KERNEL RECEIVES (the fp32 sums,
moments and pooled statistics handed in), so a bound measures the kernel alone; whether the formula is the gradient is what the
autograd tests of tests/test_gpu_train_kernels.py keep checking.

Exact cases
-----------
eps = 0, var = 1/4 (rstd = 2), integer mean, gamma in quarters (one of them 0), n_frames a power of two, small-integer dh, r, h, mu,
dmu, dsig, sig in {1, 2}, chunk lengths 1, 2, 4, 8: every intermediate of every kernel is a dyadic rational of fewer than 24 bits,
so each fp32 operation is exact with or without contraction and the fp64 reference rounded once is the only right answer.  The CPU
companion proves this per case: the replay (every operation rounded) reproduces the reference bit for bit, and stops doing so at a
neighbouring case (var = 0.3).  Zeros are compared without their sign (0 * dh and -0 * r differ between a fused and a plain sum).

Column sums (col_sums_kernel -> col_sums_merge_kernel)
------------------------------------------------------
fp64 throughout: a wave adds the rows ty, ty + 4, ... of a 128-row split (a * b of two fp32 numbers is exact in fp64), the four
waves are added in order, the merge adds the splits g, g + 16, ... per group and the 16 groups in order; ONE rounding to fp32.  The
replay performs the same fp64 additions in the same order, so it has the kernel's bits.  Bound (as the issue states it):

    |sum - ref| <= ulp32(ref) / 2 + 2^-50 sum |terms|

(2^-50 is 8 fp64 roundings' worth; the worst case of the longest path -- 32 rows of a wave, 3 waves, ceil(splits / 16) splits, 15
groups -- would be 2^-53 times that depth; the replay, which has the kernel's bits, stays inside 2^-50 on every case.)

Coefficients (bn_coeffs_kernel, col_sums_merge_coeffs_kernel, bn_small_backward_kernel, pool_bn_coeffs_kernel)
--------------------------------------------------------------------------------------------------------------
fp64 expressions of the fp32 inputs, ONE rounding to fp32 each:  rstd = 1 / sqrt(var + eps),  dbeta = S1,
dgamma = rstd (S2 - mean S1),  A = gamma rstd,  B = -gamma rstd^2 dgamma / N,  K = -gamma rstd S1 / N + gamma rstd^2 mean dgamma / N.
The first three kernels pass S1, S2 through fp32 before they form dgamma, so there dbeta IS the fp32 sum handed in (bit for bit) and
|dgamma - ref| <= 1 ulp32(ref) + 2^-50 rstd (|S2| + |mean S1|)  (the rounding, and the 7 fp64 roundings of rstd, the product, the
difference and the last product, each relative to the cancelling pair at most).  pool_bn_coeffs_kernel keeps S1 = sum_b dmu_b and
S2 = sum_b dmu_b m_b + dsig_b s v_b / sig_b in fp64 (depth = ceil(chunks / 16) + 15 additions, 9 roundings inside a term: rstd 3,
s 1, the term's 3 products, 1 division, 1 sum), so  dbeta: ulp32 / 2 + depth 2^-53 sum |dmu|  and
dgamma: 1 ulp32 + (depth + 20) 2^-53 rstd (sum |terms| + |mean| sum |dmu|).

dz = A dh + B r + K (bn_act_backward_kernel, bn_act_backward_vec_kernel, bn_small_backward_kernel)
-----------------------------------------------------------------------------------------------
((A dh) + (B r)) + K with rounded coefficients: A dh carries the rounding of A, of the product and of both additions (4 U), B r the
same (4 U), K its own rounding and that of the last addition (2 U):

    |dz - ref| <= C_DZ U (|A dh| + |B r| + |K|),   C_DZ = 4      (5 with leaky ReLU: alpha * dr)

with the fp64 A, B, K.  ReLU at r <= 0 and gap rows: exactly 0.  With |mean| >> std, B r cancels against K and the bound is large
relative to dz: that is what the form delivers; the loss is measured against the exact gradient (bn_backward_true) and recorded.

Pooling backward (pool_backward_kernel; the dh inside pool_bn_act_backward_kernel)
-------------------------------------------------------------------------------
dh = dmu invT + ((dsig (h - mu)) invT) / sig, invT = fl(1 / T)  (pool_bn_act_backward: g0 = dmu invT, g1 = (dsig invT) / sig,
dh = g0 + g1 (h - mu): the same roundings in another order).  First term: invT, the product, the sum: 3 U.  Second term: the
difference, two products, invT, the division, the sum: 6 U.

    |dh - ref| <= E_dh = U (3 |dmu / T| + 6 |dsig (h - mu) / (T sig)|)

pool_bn_act_backward then forms dz from its own dh:  |dz - ref| <= |A| E_dh (1 + 8 U) + C_DZ U (|A dh| + |B r| + |K|).

bn_small_forward_kernel
-----------------------
mean and var are fp64 two-pass sums over 16 row groups (contraction off), one rounding each: ulp32 / 2 + (ceil(R / 16) + 19) 2^-53
of the summed magnitudes (a group's rows, 15 group additions, and d, d * d, the division and the rounded mean inside d).
scale = gamma * (1 / sqrtf(var + eps)), shift = beta - mean * scale are correctly rounded fp32 operations in fold_bn_kernel's
order: NumPy float32 gives the same bits from the kernel's own mean and var.  y = fma(x, scale, shift) is one rounding of the exact
value: |y - ref| <= ulp32(ref) / 2 (+ 2^-52 |ref| for the fp64 reference itself).

None of the constants is fitted: they were fixed from the code before the first device run."""
import numpy as np

import pool_data as pd

U = 2.0 ** -24
F = np.float32
D = np.float64
SLACK = 1 + 2.0 ** -10
TINY = 2.0 ** -126
DUST = 2.0 ** -50
C_DZ = 4
CS_ROWS, GROUPS = 128, 16
BN_EPS = 1e-3
POOL_EPS = 1e-5
ALPHA_EXACT, ALPHA = 0.25, 0.2
GRID_Y = 65535
SCALAR_GRID = 4096 * 256             # elements one grid of the scalar kernel covers before its stride loop wraps
ulp32, bits_equal, layout = pd.ulp32, pd.bits_equal, pd.layout

# ---------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------
CS_ROWS_LIST = (1, 3, 4, 5, 127, 128, 129, 2049)
CS_CHANNELS = (1, 3, 4, 5, 255, 256, 257, 260)
MERGE_SPLITS = (1, 15, 16, 17, 33)
BN_EXACT_C = (4, 5, 60, 63, 64, 65, 1028)
BN_EXACT_R = (1, 129, 4097)
BN_EXACT_SCALAR_WRAP = (4097, 257)                       # R * C > SCALAR_GRID on the scalar path
BN_SMALL_R = (1, 16, 128, 1024)
ACTS = ("none", "relu", "lrelu")
POOL_CHUNKS = (1, 15, 16, 17, 33, 129, 200, 2048)
POOL_EXACT_C = (4, 64, 516)                               # one float4, the split copy, more than one block of 512 channels
SMALL_FWD_R = (1, 16, 17, 1024)
SMALL_FWD_C = (1, 63, 64, 65)
LAYOUTS = {"ragged": (37, 1, 700, 2, 129, 513, 300, 64), "uniform": (130,) * 17}
BOUND_C = (24, 21)                                       # the vector kernels, the scalar ones
KINDS = ("relu", "mean200", "const", "gamma0", "outlier", "negative")


POOL_EXACT = ((1, 516), (15, 4), (16, 64), (17, 516), (33, 64), (129, 516), (200, 4), (2048, 64))       # (chunks, C)


def kind_of(c):
    return KINDS[c % len(KINDS)]


def bn_exact_shapes():
    """(R, C, act) of every exact BN-backward case, the one list both test modules walk: every activation at the small shapes,
    one per shape above 1000 rows."""
    out = []
    for R, C in [(R, C) for C in BN_EXACT_C for R in BN_EXACT_R] + [BN_EXACT_SCALAR_WRAP]:
        for j, act in enumerate(ACTS):
            if R <= 1000 or j == (R + C) % 3:
                out.append((R, C, act))
    return out


def bn_exact_cases(C=None):
    for R, c, act in bn_exact_shapes():
        if C is None or c == C:
            yield bn_exact_case(R, c, act, seed=R * 31 + c)


def bn_small_exact_cases(act):
    for R in BN_SMALL_R:
        for C in (4, 5, 63, 64, 65):
            yield bn_exact_case(R, C, act, seed=R + C, small=True)


def pool_exact_cases(nchunks, C):
    for act in ACTS:
        yield pool_exact_case(nchunks, C, act, seed=nchunks + C)


def pool_grid_limit_case():
    return pool_exact_case(GRID_Y, 4, "lrelu", seed=5, one_row=True)


def pool_sliced_case():
    """65540 one-row chunks: the second slice of the host loop of xv_pool_backward_f32."""
    return pool_exact_case(GRID_Y + 5, 4, "none", seed=7, one_row=True)


def odd_width(case, C):
    """The pooling case cut to its first C channels (pool_backward takes any width)."""
    full = case["h"].shape[1]
    cut = lambda a: np.concatenate([a[:, :C], a[:, full:full + C]], 1)
    return dict(case, h=case["h"][:, :C], pooled=cut(case["pooled"]), dpooled=cut(case["dpooled"]))


def canon(x):
    """The bits of x with -0 folded into +0."""
    return (np.ascontiguousarray(x, F) + F(0)).view(np.uint32)


def same(a, b):
    return np.array_equal(canon(a), canon(b))


def representable(x):
    """Whether every fp64 value is an fp32 number."""
    x = np.asarray(x, D)
    return bool(np.array_equal(x.astype(F).astype(D), x))


def valid_of(rs, rl, R):
    v = np.zeros(R, bool)
    for s, n in zip(rs, rl):
        v[s:s + max(int(n), 0)] = True
    return v


def apply_act(z, act, alpha):
    if act == "relu":
        return np.maximum(z, F(0))
    if act == "lrelu":
        return np.maximum(F(alpha) * z, z)
    return z


def ratio(err, bound):
    err, bound = np.asarray(err, D), np.asarray(bound, D)
    bad = ~np.isfinite(err)
    r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(np.max(np.where(bad, np.inf, r))) if r.size else 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# column sums
# ---------------------------------------------------------------------------------------------------------------------------
def _seq(x):
    s = np.zeros(x.shape[1:], D)
    for row in x:
        s = s + row
    return s


def replay_col_parts(a, b=None, drop_tail=False):
    """[splits, 2, C] fp64 partial sums in col_sums_kernel's order.  drop_tail: the broken variant without the c + 4 > C tail."""
    R, C = a.shape
    ad = a.astype(D)
    pr = ad * b.astype(D) if b is not None else np.zeros_like(ad)
    ns = -(-R // CS_ROWS)
    part = np.zeros((ns, 2, C), D)
    for j in range(ns):
        for k, m in enumerate((ad[j * CS_ROWS:(j + 1) * CS_ROWS], pr[j * CS_ROWS:(j + 1) * CS_ROWS])):
            w = [_seq(m[ty::4]) for ty in range(4)]
            part[j, k] = ((w[0] + w[1]) + w[2]) + w[3]
    if drop_tail and C % 4:
        part[:, :, C - C % 4:] = 0.0
    return part


def replay_merge(part, skip16=False):
    """fp64 [2, C] totals in col_sums_merge_kernel's order.  skip16: the broken variant whose groups skip split 16."""
    tot = np.zeros(part.shape[1:], D)
    for g in range(GROUPS):
        s = np.zeros(part.shape[1:], D)
        for j in range(g, part.shape[0], GROUPS):
            if not (skip16 and j == 16):
                s = s + part[j]
        tot = tot + s
    return tot


def replay_col_sums(a, b=None, drop_tail=False, skip16=False):
    t = replay_merge(replay_col_parts(a, b, drop_tail), skip16).astype(F)
    return t[0], (t[1] if b is not None else None)


def host_parts(a, b, valid=None):
    """What a producer leaves per 128-row tile: [sum a | sum a b] in fp64 over the valid rows (any order: NumPy's)."""
    R, C = a.shape
    ad = a.astype(D) if valid is None else np.where(valid[:, None], a.astype(D), 0.0)
    ns = -(-R // CS_ROWS)
    ws = np.zeros((ns, 2, C), D)
    for j in range(ns):
        ws[j, 0] = ad[j * CS_ROWS:(j + 1) * CS_ROWS].sum(0)
        ws[j, 1] = (ad[j * CS_ROWS:(j + 1) * CS_ROWS] * b[j * CS_ROWS:(j + 1) * CS_ROWS].astype(D)).sum(0)
    return ws


def col_case(R, C, seed, exact, with_b=True):
    """exact: integers in [-8, 8] (every sum below 2^24).  Otherwise ReLU-of-Gaussian data times Gaussian, with columns whose sum
    cancels to about 0 (c % 3 == 1: every row once with either sign) and a mean-200 column (c % 3 == 2)."""
    rng = np.random.default_rng(seed)
    if exact:
        a = rng.integers(-8, 9, size=(R, C)).astype(F)
        b = rng.integers(-8, 9, size=(R, C)).astype(F)
    else:
        a = rng.standard_normal((R, C)).astype(F)
        b = (np.maximum(rng.standard_normal((R, C)), 0) * 1.7).astype(F)
        half = R // 2
        a[half:2 * half, 1::3] = -a[:half, 1::3]
        b[half:2 * half, 1::3] = b[:half, 1::3]
        if R % 2:
            a[-1, 1::3] = 0
        b[:, 2::3] = (200.0 + 0.1 * rng.standard_normal((R, len(range(2, C, 3))))).astype(F)
    return dict(a=a, b=b if with_b else None, exact=exact)


def col_sums_ref(a, b):
    """(ref_a, ref_ab, bound_a, bound_ab) in fp64 from long-double sums."""
    al = a.astype(np.longdouble)
    ra = al.sum(0).astype(D)
    ba = ulp32(ra) / 2 + DUST * np.abs(a.astype(D)).sum(0)
    if b is None:
        return ra, None, ba, None
    p = al * b.astype(np.longdouble)
    rb = p.sum(0).astype(D)
    return ra, rb, ba, ulp32(rb) / 2 + DUST * np.abs(p).sum(0).astype(D)


def merge_case(nsplit, C, seed):
    """Hand-made fp64 partials whose totals are small integers although single partials are near 2^40 (an fp32 accumulator, or a
    skipped split, cannot produce them)."""
    rng = np.random.default_rng(seed)
    part = rng.integers(-1000, 1001, size=(nsplit, 2, C)).astype(D)
    big = np.ldexp(1.0, 40) + rng.integers(0, 1000, size=(2, C))
    if nsplit > 1:
        part[0] += big
        part[nsplit - 1] -= big
    return part


# ---------------------------------------------------------------------------------------------------------------------------
# BN backward
# ---------------------------------------------------------------------------------------------------------------------------
def coeffs64(s1, s2, mean, var, gamma, eps, N, no_mean_term=False):
    """(dgamma, dbeta, A, B, K) in fp64, the kernels' expressions.  no_mean_term: the broken variant whose K lacks its mean term."""
    s1, s2, mean, g = np.asarray(s1, D), np.asarray(s2, D), np.asarray(mean, D), np.asarray(gamma, D)
    rstd = 1.0 / np.sqrt(np.asarray(var, D) + D(F(eps)))
    N = D(F(N))
    dg = rstd * (s2 - mean * s1)
    A = g * rstd
    B = -g * rstd * rstd * dg / N
    K = -g * rstd * s1 / N
    if not no_mean_term:
        K = K + g * rstd * rstd * mean * dg / N
    return dg, s1, A, B, K


def act_grad(dr, r, act, alpha, ge=False):
    pos = (r >= 0) if ge else (r > 0)
    if act == "relu":
        return np.where(pos, dr, dr.dtype.type(0))
    if act == "lrelu":
        return np.where(pos, dr, dr.dtype.type(F(alpha)) * dr)
    return dr


def replay_small_sums(dh, r):
    """fp32 (S1, S2) of bn_small_backward_kernel: 16 row groups in fp64, merged in group order, through fp32."""
    a = dh.astype(D)
    p = a * r.astype(D)
    t1, t2 = np.zeros(a.shape[1], D), np.zeros(a.shape[1], D)
    for g in range(GROUPS):
        t1, t2 = t1 + _seq(a[g::GROUPS]), t2 + _seq(p[g::GROUPS])
    return t1.astype(F), t2.astype(F)


def sums_in(case, entry, skip16=False):
    """The fp32 (S1, S2) the coefficients are formed from, per entry point."""
    if entry == "sums":
        return case["s1"], case["s2"]
    if entry == "parts":
        t = replay_merge(case["parts"], skip16).astype(F)
        return t[0], t[1]
    return replay_small_sums(case["dh"], case["r"])


def replay_bn_backward(case, entry, broken=None):
    """(dgamma, dbeta, dz) in float32 with every operation rounded.  broken: None / "k_mean" / "mask" / "ge" / "skip16" / "gaps"."""
    s1, s2 = sums_in(case, entry, skip16=broken == "skip16")
    dg, db, A, B, K = coeffs64(s1, s2, case["mean"], case["var"], case["gamma"], case["eps"], case["N"], broken == "k_mean")
    A, B, K = A.astype(F), B.astype(F), K.astype(F)
    valid = case["valid"]
    if broken == "mask" and valid is not None:
        valid = np.roll(valid, 1)
    with np.errstate(all="ignore"):
        dr = (A * case["dh_in"] + B * case["r"]) + K
        dz = act_grad(dr, case["r"], case["act"], case["alpha"], ge=broken == "ge")
    if valid is not None:
        dz = np.where(valid[:, None], dz, F(np.nan) if broken == "gaps" else F(0))
    return dg.astype(F), db.astype(F), dz.astype(F)


def bn_backward_ref(case, entry):
    """fp64 reference and bounds: dict(dg, dg_bound, db, dz, dz_bound)."""
    s1, s2 = sums_in(case, entry)
    dg, db, A, B, K = coeffs64(s1, s2, case["mean"], case["var"], case["gamma"], case["eps"], case["N"])
    rstd = 1.0 / np.sqrt(case["var"].astype(D) + D(F(case["eps"])))
    dg_bound = ulp32(dg) + DUST * rstd * (np.abs(s2.astype(D)) + np.abs(case["mean"].astype(D) * s1.astype(D)))
    dh, r = case["dh"].astype(D), case["r"].astype(D)
    dr = A * dh + B * r + K
    mag = np.abs(A * dh) + np.abs(B * r) + np.abs(K)
    dz = act_grad(dr, r, case["act"], case["alpha"])
    bound = C_DZ * U * mag * SLACK + TINY
    if case["act"] == "relu":
        bound = np.where(r > 0, bound, 0.0)
    elif case["act"] == "lrelu":
        bound = np.where(r > 0, bound, float(F(case["alpha"])) * (C_DZ + 1) * U * mag * SLACK + TINY)
    if case["valid"] is not None:
        dz = np.where(case["valid"][:, None], dz, 0.0)
        bound = np.where(case["valid"][:, None], bound, 0.0)
    return dict(dg=dg, dg_bound=dg_bound, db=s1, dz=dz, dz_bound=bound)


def bn_backward_true(case):
    """The exact gradient (what fp64 autograd of BN over the valid rows gives) from the fp32 r and dh: batch moments, sums and the
    closed form in fp64 without passing anything through fp32.  -> (dz, dgamma, summand norm of dgamma)."""
    v = case["valid"] if case["valid"] is not None else np.ones(len(case["r"]), bool)
    r, dh = case["r"].astype(D), np.where(v[:, None], case["dh"].astype(D), 0.0)
    m = r[v].mean(0)
    var = ((r[v] - m) ** 2).mean(0)
    rstd = 1.0 / np.sqrt(var + D(F(case["eps"])))
    xhat = (r - m) * rstd
    n = v.sum()
    dg = (dh * xhat)[v].sum(0)
    dr = case["gamma"].astype(D) * rstd * (dh - dh[v].sum(0) / n - xhat * dg / n)
    dz = np.where(v[:, None], act_grad(dr, r, case["act"], case["alpha"]), 0.0)
    return dz, dg, np.sqrt(((dh * xhat)[v] ** 2).sum(0))


def _finish_bn(case):
    """s1, s2 (fp64 sums rounded once), the producer's partials and dh_in (NaN in the gap rows)."""
    valid, dh, r = case["valid"], case["dh"], case["r"]
    parts = host_parts(dh, r, valid)
    tot = parts.sum(0)
    case.update(s1=tot[0].astype(F), s2=tot[1].astype(F), parts=parts, dh_in=dh.copy())
    if valid is not None:
        case["dh_in"][~valid] = np.nan
    return case


def bn_exact_case(R, C, act, seed, small=False, var=0.25):
    """See "Exact cases" in the module docstring.  One gap row in the middle when R is odd and above 1 (so the valid rows are a power
    of two); small: no mask (bn_small_backward)."""
    rng = np.random.default_rng(seed)
    valid = None
    if not small:
        valid = np.ones(R, bool)
        if R > 1:
            valid[R // 2] = False
    n = R if valid is None else int(valid.sum())
    assert n & (n - 1) == 0
    dh = rng.integers(-2, 3, size=(R, C)).astype(F)
    r = rng.integers(0 if act == "relu" else -4, 5, size=(R, C)).astype(F)
    r[rng.random((R, C)) < 0.3] = 0
    if valid is not None:
        r[~valid] = 0
        dh[~valid] = 0
    gamma = (rng.integers(-8, 9, size=C) / 4.0).astype(F)
    gamma[C // 2] = 0
    return _finish_bn(dict(dh=dh, r=r, valid=valid, mean=rng.integers(-2, 3, size=C).astype(F), var=np.full(C, var, F), gamma=gamma,
                           eps=0.0, N=float(n), act=act, alpha=ALPHA_EXACT, exact=True))


def bn_bound_case(layout_name, C, act, seed, rows=None):
    """Realistic data (activation of Gaussian pre-activations) with the hostile channels of KINDS; rows: keep only the first `rows`
    rows and drop the mask (bn_small_backward)."""
    rng = np.random.default_rng(seed)
    lens = LAYOUTS[layout_name]
    rs, R = layout(lens)
    valid = valid_of(rs, lens, R)
    z = (rng.standard_normal((R, C)) * rng.uniform(0.5, 3.0, C) + rng.uniform(-2, 2, C)).astype(F)
    dh = rng.standard_normal((R, C)).astype(F)
    gamma = (1.0 + 0.2 * rng.standard_normal(C)).astype(F)
    rows_valid = np.nonzero(valid)[0]
    for c in range(C):
        k = kind_of(c)
        if k == "mean200":
            z[:, c] = (200.0 + 0.1 * rng.standard_normal(R)).astype(F)
        elif k == "const":
            z[:, c] = F(1.5)
        elif k == "gamma0":
            gamma[c] = 0
        elif k == "outlier":
            dh[rows_valid[rng.integers(len(rows_valid) if rows is None else min(rows, len(rows_valid)))], c] = 1e4
        elif k == "negative":
            z[:, c] = (-np.abs(rng.standard_normal(R)) - 0.1).astype(F)
    r = apply_act(z, act, ALPHA).astype(F)
    if rows is not None:
        keep = rows_valid[:rows]
        r, dh, valid = r[keep], dh[keep], None
        n = rows
        rr = r.astype(D)
    else:
        r[~valid] = 0
        dh[~valid] = 0
        n = int(valid.sum())
        rr = r[valid].astype(D)
    m = rr.mean(0)
    return _finish_bn(dict(dh=dh, r=r, valid=valid, mean=m.astype(F), var=((rr - m) ** 2).mean(0).astype(F), gamma=gamma, eps=BN_EPS,
                           N=float(n), act=act, alpha=ALPHA, exact=False, rs=rs, rl=np.asarray(lens, np.int32)))


# ---------------------------------------------------------------------------------------------------------------------------
# rows_affine (exact cases only)
# ---------------------------------------------------------------------------------------------------------------------------
def affine_case(R, C, seed):
    rng = np.random.default_rng(seed)
    valid = rng.random(R) < 0.8 if R > 1 else np.ones(R, bool)
    x = rng.integers(-8, 9, size=(R, C)).astype(F)
    x[~valid] = np.nan
    scale, shift = (rng.integers(-8, 9, size=C) / 4.0).astype(F), (rng.integers(-40, 41, size=C) / 8.0).astype(F)
    with np.errstate(all="ignore"):
        y = np.where(valid[:, None], x.astype(D) * scale + shift, 0.0)
    return dict(x=x, valid=valid, scale=scale, shift=shift, y=y)


# ---------------------------------------------------------------------------------------------------------------------------
# pooling backward
# ---------------------------------------------------------------------------------------------------------------------------
def _pool_layout(lens, gaps, lead, tail):
    rs = lead + np.concatenate([[0], np.cumsum(np.asarray(lens[:-1], np.int64) + gaps[:-1])])
    R = int(rs[-1] + lens[-1] + gaps[-1] + tail)
    return rs.astype(np.int32), R


def owner_of(rs, rl, R, shift=0):
    """Chunk index per row, -1 outside every chunk.  shift: the broken variant whose mask is one row late."""
    own = np.full(R, -1, np.int64)
    for b, (s, n) in enumerate(zip(rs, rl)):
        if n > 0:
            own[s + shift:min(s + shift + int(n), R)] = b
    return own


def pool_exact_case(nchunks, C, act, seed, one_row=False, var=0.25):
    """See "Exact cases".  Gaps of 0, 1 or 2 rows between chunks, 3 rows in front of chunk 0, 5 behind the last; h and r hold NaN
    outside the chunks."""
    rng = np.random.default_rng(seed)
    rl = np.ones(nchunks, np.int32) if one_row else (2 ** rng.integers(0, 4, size=nchunks)).astype(np.int32)
    gaps = np.zeros(nchunks, np.int64) if one_row else rng.integers(0, 3, size=nchunks)
    rs, R = _pool_layout(rl, gaps, 3, 5)
    own = owner_of(rs, rl, R)
    h = rng.integers(-4, 5, size=(R, C)).astype(F)
    r = rng.integers(0 if act == "relu" else -4, 5, size=(R, C)).astype(F)
    r[rng.random((R, C)) < 0.3] = 0
    h[own < 0] = np.nan
    r[own < 0] = np.nan
    pooled = np.concatenate([rng.integers(-2, 3, size=(nchunks, C)), 2 ** rng.integers(0, 2, size=(nchunks, C))], 1).astype(F)
    dpooled = rng.integers(-2, 3, size=(nchunks, 2 * C)).astype(F)
    cm = np.concatenate([rng.integers(-2, 3, size=(nchunks, C)), 2 ** rng.integers(1, 3, size=(nchunks, C))], 1).astype(F)
    gamma = (rng.integers(-8, 9, size=C) / 4.0).astype(F)
    gamma[C // 2] = 0
    n = 1
    while n < int(rl.sum()):
        n *= 2
    return dict(h=h, r=r, rs=rs, rl=rl, R=R, pooled=pooled, dpooled=dpooled, cm=cm, mean=rng.integers(-2, 3, size=C).astype(F),
                var=np.full(C, var, F), gamma=gamma, eps=0.0, N=float(n), act=act, alpha=ALPHA_EXACT, exact=True)


def pool_bound_case(layout_name, C, act, seed):
    """h = BN(r) of the BN bound case in fp32, pooled = [mean | sqrt(var + 1e-5)] of h per chunk and the chunk moments of r (fp64,
    rounded once), dpooled Gaussian with one 1e4 outlier per outlier channel."""
    bn = bn_bound_case(layout_name, C, act, seed)
    rng = np.random.default_rng(seed + 1000)
    rs, rl, valid = bn["rs"], bn["rl"], bn["valid"]
    R = len(valid)
    r = bn["r"]
    rstd = 1.0 / np.sqrt(bn["var"].astype(D) + D(F(BN_EPS)))
    beta = 0.1 * rng.standard_normal(C)
    h = ((r.astype(D) - bn["mean"].astype(D)) * rstd * bn["gamma"].astype(D) + beta).astype(F)
    nb = len(rl)
    pooled, cm = np.empty((nb, 2 * C), F), np.empty((nb, 2 * C), F)
    for b, (s, n) in enumerate(zip(rs, rl)):
        hb, rb = h[s:s + n].astype(D), r[s:s + n].astype(D)
        pooled[b, :C], pooled[b, C:] = hb.mean(0), np.sqrt(hb.var(0) + POOL_EPS)
        cm[b, :C], cm[b, C:] = rb.mean(0), rb.var(0)
    dpooled = rng.standard_normal((nb, 2 * C)).astype(F)
    for c in range(C):
        if kind_of(c) == "outlier":
            dpooled[rng.integers(nb), c + C * int(rng.integers(2))] = 1e4
    h[~valid] = np.nan
    r = r.copy()
    r[~valid] = np.nan
    return dict(h=h, r=r, rs=rs, rl=rl, R=R, pooled=pooled, dpooled=dpooled, cm=cm, mean=bn["mean"], var=bn["var"], gamma=bn["gamma"],
                eps=BN_EPS, N=bn["N"], act=act, alpha=ALPHA, exact=False)


def _per_row(case, own):
    """Row-wise views of the per-chunk numbers (rows outside every chunk borrow chunk 0; they are masked afterwards)."""
    C = case["h"].shape[1]
    o = np.maximum(own, 0)
    p, dp = case["pooled"][o], case["dpooled"][o]
    return p[:, :C], p[:, C:], dp[:, :C], dp[:, C:], case["rl"][o]


def replay_pool_dh(case, fused_order, broken=None):
    """float32 dh per row (NaN-free inside the chunks) in pool_backward_kernel's order or pool_bn_act_backward_kernel's (fused_order);
    broken: "mask" (one row late) / "invT" (1 / T of the next chunk)."""
    own = owner_of(case["rs"], case["rl"], case["R"], shift=1 if broken == "mask" else 0)
    mu, sig, dmu, dsig, T = _per_row(case, own)
    if broken == "invT":
        T = np.roll(case["rl"], -1)[np.maximum(own, 0)]
    with np.errstate(all="ignore"):
        invT = (F(1) / T.astype(F))[:, None]
        if fused_order:
            dh = dmu * invT + (dsig * invT / sig) * (case["h"] - mu)
        else:
            dh = dmu * invT + dsig * (case["h"] - mu) * invT / sig
    return dh.astype(F), own


def replay_pool_backward(case, broken=None):
    dh, own = replay_pool_dh(case, False, broken)
    return np.where((own >= 0)[:, None], dh, F(np.nan) if broken == "gaps" else F(0))


def pool_dh_ref(case):
    """(fp64 dh, E_dh) per row, 0 outside the chunks."""
    own = owner_of(case["rs"], case["rl"], case["R"])
    mu, sig, dmu, dsig, T = (x.astype(D) for x in _per_row(case, own))
    T = T[:, None]
    with np.errstate(all="ignore"):
        t1, t2 = dmu / T, dsig * (case["h"].astype(D) - mu) / (T * sig)
    inside = (own >= 0)[:, None]
    return np.where(inside, t1 + t2, 0.0), np.where(inside, U * (3 * np.abs(t1) + 6 * np.abs(t2)) * SLACK + TINY, 0.0), own


def pool_coeffs64(case, no_mean_term=False):
    """fp64 (dgamma, dbeta, A, B, K, sum |terms| of S2, sum |dmu|) of pool_bn_coeffs_kernel (chunks with row_len <= 0 skipped)."""
    C = case["h"].shape[1]
    keep = case["rl"] > 0
    p, dp, cm = case["pooled"][keep].astype(D), case["dpooled"][keep].astype(D), case["cm"][keep].astype(D)
    rstd = 1.0 / np.sqrt(case["var"].astype(D) + D(F(case["eps"])))
    s = case["gamma"].astype(D) * rstd
    terms = dp[:, :C] * cm[:, :C] + dp[:, C:] * s * cm[:, C:] / p[:, C:]
    absterms = np.abs(dp[:, :C] * cm[:, :C]) + np.abs(dp[:, C:] * s * cm[:, C:] / p[:, C:])
    s1, s2 = dp[:, :C].sum(0), terms.sum(0)
    dg, db, A, B, K = coeffs64(s1, s2, case["mean"], np.asarray(case["var"], D), case["gamma"], case["eps"], case["N"], no_mean_term)
    return dg, db, A, B, K, absterms.sum(0), np.abs(dp[:, :C]).sum(0)


def replay_pool_bn(case, broken=None):
    """(dgamma, dbeta, dz) of xv_pool_bn_act_backward_f32 in float32, every operation rounded; broken: None / "k_mean" / "mask" /
    "ge" / "invT" / "gaps"."""
    dg, db, A, B, K, _, _ = pool_coeffs64(case, broken == "k_mean")
    A, B, K = A.astype(F), B.astype(F), K.astype(F)
    dh, own = replay_pool_dh(case, True, broken)
    with np.errstate(all="ignore"):
        dr = (A * dh + B * case["r"]) + K
        dz = act_grad(dr, case["r"], case["act"], case["alpha"], ge=broken == "ge")
    dz = np.where((own >= 0)[:, None], dz, F(np.nan) if broken == "gaps" else F(0))
    return dg.astype(F), db.astype(F), dz.astype(F)


def pool_bn_ref(case):
    dg, db, A, B, K, absterms, absdmu = pool_coeffs64(case)
    dh, e_dh, own = pool_dh_ref(case)
    inside = (own >= 0)[:, None]
    r = np.where(inside, case["r"].astype(D), 0.0)
    dr = A * dh + B * r + K
    mag = np.abs(A * dh) + np.abs(B * r) + np.abs(K)
    dz = np.where(inside, act_grad(dr, r, case["act"], case["alpha"]), 0.0)
    bound = np.abs(A) * e_dh * (1 + 8 * U) + C_DZ * U * mag * SLACK + TINY
    if case["act"] == "relu":
        bound = np.where(r > 0, bound, 0.0)
    elif case["act"] == "lrelu":
        a = float(F(case["alpha"]))
        bound = np.where(r > 0, bound, a * (np.abs(A) * e_dh * (1 + 8 * U) + (C_DZ + 1) * U * mag * SLACK) + TINY)
    bound = np.where(inside, bound, 0.0)
    depth = -(-len(case["rl"]) // GROUPS) + 15
    rstd = 1.0 / np.sqrt(case["var"].astype(D) + D(F(case["eps"])))
    u53 = 2.0 ** -53
    return dict(dg=dg, dg_bound=ulp32(dg) + (depth + 20) * u53 * rstd * (absterms + np.abs(case["mean"].astype(D)) * absdmu),
                db=db, db_bound=ulp32(db) / 2 + depth * u53 * absdmu, dz=dz, dz_bound=bound)


# ---------------------------------------------------------------------------------------------------------------------------
# bn_small_forward
# ---------------------------------------------------------------------------------------------------------------------------
def small_fwd_case(R, C, seed, exact):
    """exact: every column holds m + s and m - s in equal numbers (one lone m in front when R is odd), s = 1/2: mean = m and, for even R,
    var = 1/4; eps = 0 (1/4 when R = 1, where var = 0).  Otherwise ReLU-of-Gaussian columns with a mean-200 column, a constant column,
    a gamma = 0 column and a 1e4 outlier."""
    rng = np.random.default_rng(seed)
    if exact:
        m = rng.integers(-6, 7, size=C).astype(D)
        sign = np.tile([0.5, -0.5], R // 2)[:, None] * np.ones((1, C))
        for c in range(C):
            sign[:, c] = rng.permutation(sign[:, c])
        x = (m + np.concatenate([np.zeros((R % 2, C)), sign])).astype(F)
        gamma, beta = (rng.integers(-8, 9, size=C) / 4.0).astype(F), (rng.integers(-16, 17, size=C) / 4.0).astype(F)
        return dict(x=x, gamma=gamma, beta=beta, eps=0.25 if R == 1 else 0.0, exact=True)
    x = (np.maximum(rng.standard_normal((R, C)), 0) * 1.7 + rng.uniform(-2, 2, C)).astype(F)
    gamma, beta = (1.0 + 0.2 * rng.standard_normal(C)).astype(F), (0.1 * rng.standard_normal(C)).astype(F)
    for c in range(C):
        k = kind_of(c)
        if k == "mean200":
            x[:, c] = (200.0 + 0.1 * rng.standard_normal(R)).astype(F)
        elif k == "const":
            x[:, c] = F(-37.25)
        elif k == "gamma0":
            gamma[c] = 0
        elif k == "outlier":
            x[rng.integers(R), c] = 1e4
    return dict(x=x, gamma=gamma, beta=beta, eps=BN_EPS, exact=False)


def fold32(mean, var, gamma, beta, eps):
    """float32 (scale, shift) in fold_bn_kernel's order."""
    sc = gamma * (F(1) / np.sqrt(var + F(eps)))
    return sc, beta - mean * sc


def replay_small_forward(case):
    x = case["x"].astype(D)
    R = x.shape[0]
    t = np.zeros(x.shape[1], D)
    for g in range(GROUPS):
        t = t + _seq(x[g::GROUPS])
    m = t / R
    d = x - m
    q = np.zeros(x.shape[1], D)
    for g in range(GROUPS):
        q = q + _seq((d * d)[g::GROUPS])
    mean, var = m.astype(F), (q / R).astype(F)
    with np.errstate(all="ignore"):
        sc, sf = fold32(mean, var, case["gamma"], case["beta"], case["eps"])
        y = (x * sc.astype(D) + sf.astype(D)).astype(F)
    return mean, var, y


def small_forward_ref(case):
    """fp64 (mean, var, bound of mean, bound of var) from long-double two-pass sums."""
    x = case["x"].astype(np.longdouble)
    R = x.shape[0]
    m = x.sum(0) / R
    v = ((x - m) ** 2).sum(0) / R
    m, v = m.astype(D), v.astype(D)
    depth = (-(-R // GROUPS) + 15 + 4) * 2.0 ** -53          # a group's rows, the 16 groups, d, d * d, the division, the mean inside d
    return m, v, ulp32(m) / 2 + depth * np.abs(case["x"].astype(D)).sum(0) / R, ulp32(v) / 2 + depth * v


# ---------------------------------------------------------------------------------------------------------------------------
# merge_moments / bn_moments_fold (exact cases only)
# ---------------------------------------------------------------------------------------------------------------------------
def pow2_lengths(n, total_log2, seed):
    """n powers of two that sum to 2^total_log2."""
    rng = np.random.default_rng(seed)
    ks = [total_log2]
    while len(ks) < n:
        cand = [i for i, k in enumerate(ks) if k > 0]
        i = cand[rng.integers(len(cand))]
        ks[i] -= 1
        ks.insert(i, ks[i])
    return (2 ** np.asarray(ks)).astype(np.int32)


def merge_moments_case(nchunks, C, seed):
    """Chunk means in 1/8, variances in 1/64, lengths powers of two that sum to 1024, plus one chunk of length 0 (NaN moments) in
    the middle that the merge must skip.  -> dict with the exact fp64 answer."""
    rng = np.random.default_rng(seed)
    rl = pow2_lengths(nchunks, 10, seed)
    cm = np.concatenate([rng.integers(-64, 65, size=(nchunks, C)) / 8.0, rng.integers(0, 256, size=(nchunks, C)) / 64.0], 1).astype(F)
    n = rl.astype(D)[:, None]
    mu = (n * cm[:, :C].astype(D)).sum(0) / 1024
    var = (n * (cm[:, C:].astype(D) + (cm[:, :C].astype(D) - mu) ** 2)).sum(0) / 1024
    at = nchunks // 2
    return dict(cm=np.insert(cm, at, np.nan, axis=0), rl=np.insert(rl, at, 0).astype(np.int32), mean=mu, var=var)


def moments_fold_case(nsplit, C, seed):
    """Partials [sum y | sum y^2] per 128 rows of columns m +- 1/2 (64 of each per tile); tile 1 (when there is one) is a gap tile of
    zeros, and tiles are dropped or kept so that n_frames is a power of two.  mean = m, var = 1/4, eps = 0: scale = 2 gamma."""
    rng = np.random.default_rng(seed)
    m = rng.integers(-6, 7, size=C).astype(D)
    part = np.zeros((nsplit, 2, C), D)
    live = [j for j in range(nsplit) if j != 1]
    n = 1
    while 2 * n <= len(live):
        n *= 2
    for j in live[:n]:
        part[j, 0], part[j, 1] = 128 * m, 128 * (m * m + 0.25)
    gamma, beta = (rng.integers(-8, 9, size=C) / 4.0).astype(F), (rng.integers(-16, 17, size=C) / 4.0).astype(F)
    return dict(part=part, R=nsplit * CS_ROWS, N=float(128 * n), gamma=gamma, beta=beta, mean=m, var=np.full(C, 0.25), scale=2.0 * gamma,
                shift=beta - 2.0 * gamma * m)
