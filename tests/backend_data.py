"""Data, replays, bounds and assertion functions for the element-wise tests of the scoring back-end (csrc/xv_backend.hip:
backend_prepare_kernel, score_matrix_kernel, score_pairs_kernel).  Shared by tests/test_gpu_backend_elementwise.py (the device)
and tests/test_backend_bounds_cpu.py (the replays, the bounds and the mutants, without a GPU).

Everything here is NumPy.  u = 2^-24 is the unit roundoff of fp32.

The scorers promise an order (include/xvector_hip.h): one fp32 accumulator per score, an fmaf chain with k
ascending from 0, then `+ r`.  `replay_scores` restates it with `fma32`, an exact fp32 fused multiply-add, so the device must give
its bits.  `prepare` is replayed in float32 in the kernel's order (`prepare_replay`) and bounded stage by stage against the fp64
reference (`prepare_bounds`); every constant of the bounds is a rounding count derived below, except LAMBDA of the two products."""
import functools
import math

import numpy as np

import backend_ref as ref

F = np.float32
U = 2.0 ** -24
TINY = 2.0 ** -100
SIDE_PLAIN, SIDE_ENROL, SIDE_TEST, SIDE_COSINE = 0, 1, 2, 3
KSTEP = 8

# The statistical factor of the two MFMA products of prepare (bound = LAMBDA * sqrt(depth) * u * sum|terms|).  Fixed on the CPU
# before the first device run: the smallest of {1, 2, 4} for which the float32 replay stays at or below 0.5 of every element's
# bound on every case of prepare_cases() (tests/test_backend_bounds_cpu.py re-checks it).  At LAMBDA = 1 the replay's worst
# ratio is 0.383 for the rows (the 1/v - 1/w half of an enrolment row, which no LAMBDA touches; the worst output that a product
# dominates, raw_test at d = 2, is at 0.276) and 0.076 for r, so 1 it is.
LAMBDA = 1


def roundup(a, b):
    return (a + b - 1) // b * b


# ---------------------------------------------------------------------------------------------------------------------------
# fma32: an exact fp32 fused multiply-add
# ---------------------------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """round_fp32(a * b + c) with ONE rounding, for fp32 inputs (arrays broadcast).  p = a * b is exact in float64 (48 bits).
    s = p + c is rounded to 53 bits; TwoSum gives its error exactly.  Where the sum was inexact and the last bit of s is 0, s
    moves one float64 ulp towards the exact value: that is round-to-odd, and 53 >= 2 * 24 + 2 makes the final rounding to fp32
    equal to the rounding of the exact value."""
    p = np.asarray(a, F).astype(np.float64) * np.asarray(b, F).astype(np.float64)
    c = np.asarray(c, F).astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (np.asarray(s).view(np.int64) & 1) == 0
    fix = (err != 0) & even
    if np.any(fix):
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return np.asarray(s).astype(F)


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------
# the scorers
# ---------------------------------------------------------------------------------------------------------------------------
STORED_ORDER = (0, 2, 4, 6, 1, 3, 5, 7)       # the LDS image of one 8-k group (score_matrix_kernel)


def replay_scores(E, T, r=None, mutant=None, check_tiny=False):
    """The documented order: acc = 0; for k ascending: acc = fma(E[e, k], T[t, k], acc); S = acc (+) r (r None: + 0.0).
    mutant "stored_order": the terms of every 8-k group are summed in the order they are stored in LDS; "drop_ragged_group":
    the last 8-k group of a ragged last 32-k slice is left out.  check_tiny: assert that no product or partial sum is a
    non-zero value below 2^-100 (subnormal handling is then not in question)."""
    E, T = np.asarray(E, F), np.asarray(T, F)
    kpad = E.shape[1]
    assert T.shape[1] == kpad and kpad % KSTEP == 0
    ks = list(range(kpad))
    if mutant == "stored_order":
        ks = [8 * (k // 8) + STORED_ORDER[k % 8] for k in ks]
    elif mutant == "drop_ragged_group":
        if kpad % 32:
            ks = ks[:-8]
    else:
        assert mutant is None
    acc = np.zeros((E.shape[0], T.shape[0]), F)
    for k in ks:
        acc = fma32(E[:, k, None], T[None, :, k], acc)
        if check_tiny:
            p = np.abs(E[:, k, None].astype(np.float64) * T[None, :, k].astype(np.float64))
            assert not np.any((p != 0) & (p < TINY)) and not np.any((acc != 0) & (np.abs(acc) < TINY))
    rr = np.zeros(E.shape[0], F) if r is None else np.asarray(r, F)
    return fma32(acc, F(1), rr[:, None])


def _pad(rows, kpad):
    out = np.zeros((rows.shape[0], kpad), F)
    out[:, :rows.shape[1]] = rows.astype(F)
    return out


def _assert_no_tiny(*arrays):
    for a in arrays:
        a = np.abs(np.asarray(a, np.float64))
        assert not np.any((a != 0) & (a < TINY))


def scorer_operands(dataset, kpad, ne, nt, seed=0):
    """(E[ne, kpad], T[nt, kpad], r[ne]) in fp32.  The data sets of the issue: "plda" (operand rows of the fp64 reference on
    synthetic vectors, d = K/2 with K = kpad - 2, so two zero pad columns), "normal", "same_sign" (|N| against -|N|: every term
    negative), "cancel" (adjacent terms of opposite sign and near-equal magnitude: |S| << sum|terms|)."""
    rng = np.random.default_rng([seed, kpad, ne, nt, sum(map(ord, dataset))])
    if dataset == "plda":
        d = kpad // 2 - 1
        psi = np.sort(10.0 ** rng.uniform(-2, 2, d))[::-1].astype(F).astype(np.float64)
        n = rng.integers(1, 12, ne)
        z = rng.standard_normal((ne, d)) * np.sqrt(psi + 1.0 / n[:, None])
        t = rng.standard_normal((nt, d)) * np.sqrt(psi + 1.0)
        rows, r = ref.side_rows_enrol(z, n, psi)
        E, T, r = _pad(rows, kpad), _pad(ref.side_rows_test(t), kpad), r.astype(F)
    elif dataset == "normal":
        E = rng.standard_normal((ne, kpad)).astype(F)
        T = rng.standard_normal((nt, kpad)).astype(F)
        r = (10 * rng.standard_normal(ne)).astype(F)
    elif dataset == "same_sign":
        E = np.abs(rng.standard_normal((ne, kpad))).astype(F)
        T = (-np.abs(rng.standard_normal((nt, kpad)))).astype(F)
        r = (10 * rng.standard_normal(ne)).astype(F)
    elif dataset == "cancel":
        h = kpad // 2
        me = np.abs(rng.standard_normal((ne, h))) + 0.1
        mt = np.abs(rng.standard_normal((nt, h))) + 0.1
        E, T = np.empty((ne, kpad)), np.empty((nt, kpad))
        E[:, 0::2], E[:, 1::2] = me, me * (1 + 1e-3 * rng.standard_normal((ne, h)))
        T[:, 0::2], T[:, 1::2] = mt, -mt * (1 + 1e-3 * rng.standard_normal((nt, h)))
        E, T = E.astype(F), T.astype(F)
        r = (1e-2 * rng.standard_normal(ne)).astype(F)
    else:
        raise KeyError(dataset)
    _assert_no_tiny(E, T, r)
    return E, T, r


@functools.lru_cache(maxsize=None)
def scorer_case(dataset, kpad, ne, nt):
    """The operands and both replays (with r, with r = None), computed once and shared; the arrays are read-only."""
    assert ne * nt * kpad <= 2e7
    E, T, r = scorer_operands(dataset, kpad, ne, nt)
    want_r = replay_scores(E, T, r, check_tiny=True)
    want_0 = replay_scores(E, T, None)
    if dataset == "cancel":
        mag = np.abs(E.astype(np.float64)) @ np.abs(T.astype(np.float64)).T
        assert np.median(np.abs(want_0) / mag) < 1e-2
    for a in (E, T, r, want_r, want_0):
        a.setflags(write=False)
    return dict(E=E, T=T, r=r, want_r=want_r, want_0=want_0)


KPADS = (8, 16, 24, 32, 40, 56, 64, 72, 104, 200, 400, 1024)
DATASETS = ("plda", "normal", "same_sign", "cancel")
_EDGES = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257)
EDGE_SHAPES = tuple(zip(_EDGES, _EDGES[::-1]))          # (1, 257) ... (257, 1): every value on both sides
PAIR_COUNTS = (1, 255, 256, 257, 5000)


def pair_list(m, ne, nt, seed=0):
    """A trial list of m pairs that holds (0, 0), (ne - 1, nt - 1) and repeats."""
    rng = np.random.default_rng([seed, m, ne, nt])
    ei = rng.integers(0, ne, m).astype(np.int32)
    ti = rng.integers(0, nt, m).astype(np.int32)
    ei[0], ti[0] = 0, 0
    if m > 1:
        ei[-1], ti[-1] = ne - 1, nt - 1
    if m > 4:
        ei[3], ti[3] = ei[2], ti[2]
        ei[m // 2], ti[m // 2] = ne - 1, nt - 1
    return ei, ti


def assert_bits_equal(got, want, what):
    got, want = np.asarray(got, F), np.asarray(want, F)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = bits(got) != bits(want)
    if bad.any():
        idx = tuple(int(i[0]) for i in np.nonzero(bad))
        raise AssertionError("%s: %d of %d elements differ from the replay; first at %s: got %r want %r" % (
            what, int(bad.sum()), bad.size, idx, float(got[idx]), float(want[idx])))


def integer_operands(kpad, ne, nt, seed=0):
    rng = np.random.default_rng([seed, kpad, ne, nt, 77])
    return (rng.integers(-3, 4, (ne, kpad)).astype(F), rng.integers(-3, 4, (nt, kpad)).astype(F), rng.integers(-50, 51, ne).astype(F))


def assert_integer_scores(got, E, T, r, what):
    """Integer operands in [-3, 3]: every partial sum is an integer below 2^24, so any order gives E T^T + r exactly."""
    want = E.astype(np.float64) @ T.astype(np.float64).T + (0.0 if r is None else r.astype(np.float64)[:, None])
    assert np.abs(want).max() < 2 ** 24
    bad = np.asarray(got, np.float64) != want
    assert not bad.any(), (what, int(bad.sum()), tuple(int(i[0]) for i in np.nonzero(bad)))


def onehot_operands(kpad, n_other, seed=0):
    rng = np.random.default_rng([seed, kpad, n_other, 99])
    return np.eye(kpad, dtype=F), rng.standard_normal((n_other, kpad)).astype(F)


def assert_onehot_scores(got, other, swapped, what):
    """E = identity: S[e, t] == T[t, e]; swapped (T = identity): S[e, t] == E[e, t].  Values, not bits: -0 becomes +0."""
    want = other if swapped else other.T
    bad = np.asarray(got, F) != want
    assert not bad.any(), (what, int(bad.sum()), tuple(int(i[0]) for i in np.nonzero(bad)))


# ---------------------------------------------------------------------------------------------------------------------------
# prepare: the float32 replay in the kernel's order
# ---------------------------------------------------------------------------------------------------------------------------
def _chain(xm, B):
    """acc[i, j] = fmaf chain over k ascending of xm[i, k] * B[j, k], from 0 (the f32-input MFMA over its k pairs)."""
    acc = np.zeros((xm.shape[0], B.shape[0]), F)
    for k in range(xm.shape[1]):
        acc = fma32(xm[:, k, None], B[None, :, k], acc)
    return acc


def _lanes(v, fill=0.0):
    """v[N, d] -> [N, blocks, 64]: column c sits in lane c % 64 of block c // 64 (the `for c = lane; c < d; c += 64` loops)."""
    n, d = v.shape
    nb = -(-d // 64)
    out = np.full((n, nb * 64), fill, F)
    out[:, :d] = v
    return out.reshape(n, nb, 64)


def _wave_sum(v):
    """The xor butterfly of wave_sum(): offsets 32, 16, ..., 1; fp32 additions."""
    for o in (32, 16, 8, 4, 2, 1):
        v = v[:, :o] + v[:, o:2 * o]
    return v[:, 0]


def _sumsq_fma(y, mutant=None):
    yl = _lanes(y)
    if mutant == "norm_tail_lanes" and y.shape[1] % 64 and y.shape[1] > 64:
        yl = yl[:, :-1]
    s = np.zeros((y.shape[0], 64), F)
    for b in range(yl.shape[1]):
        s = fma32(yl[:, b], yl[:, b], s)
    return _wave_sum(s)


def prepare_replay(case, mutant=None):
    """(rows[N, K], r[N]) in float32, operation by operation as backend_prepare_kernel performs them: fma32 for the two products
    and for the explicit fmaf norm sums, single fp32 operations elsewhere.  Mutants (the CPU companion applies them):
    "mu_ragged" (mu not subtracted in a ragged last 32-k slice), "a0_tail" (a0 left out for columns >= 32 * (d // 32)),
    "norm_tail_lanes" (the three norm sums miss the columns behind the last full 64), "psi_plus_one" (psi + 1 in place of
    psi + 1/n), "vw_swapped" (1/w - 1/v)."""
    x = np.asarray(case["x"], F)
    N, D = x.shape
    mu, A, a0 = case.get("mu"), case.get("A"), case.get("a0")
    P, m, psi, n = case.get("P"), case.get("m"), case.get("psi"), case.get("n")
    side = case["side"]
    xm = x - mu[None, :] if mu is not None else x.copy()
    if mutant == "mu_ragged" and mu is not None and A is not None and D % 32:
        xm[:, D - D % 32:] = x[:, D - D % 32:]
    if A is not None:
        d = A.shape[0]
        bias = np.zeros(d, F) if a0 is None else a0.copy()
        if mutant == "a0_tail":
            bias[32 * (d // 32):] = 0
        y = _chain(xm, A) + bias[None, :]
    else:
        d = D
        y = xm
    if case.get("length_norm", True):
        s = _sumsq_fma(y, mutant)
        with np.errstate(divide="ignore", invalid="ignore"):
            scale = np.where(s > 0, np.sqrt(F(d)) / np.sqrt(s), F(1)).astype(F)
        y = y * scale[:, None]
    nn = np.ones(N, F) if n is None else np.asarray(n).astype(F)
    if P is not None:
        y = _chain(y - m[None, :], P) + F(0)
        inv = F(1) / nn if mutant != "psi_plus_one" else np.ones(N, F)
        q = psi[None, :] + inv[:, None]
        tl = _lanes(y * y / q)
        if mutant == "norm_tail_lanes" and d % 64 and d > 64:
            tl = tl[:, :-1]
        s = np.zeros((N, 64), F)
        for b in range(tl.shape[1]):
            s = s + tl[:, b]
        s = _wave_sum(s)
        with np.errstate(divide="ignore", invalid="ignore"):
            scale = np.where(s > 0, np.sqrt(F(d) / s), F(1)).astype(F)
        y = y * scale[:, None]
    z = y
    r = np.zeros(N, F)
    if side == SIDE_ENROL:
        ps = psi[None, :]
        den = nn[:, None] * ps + F(1)
        a = nn[:, None] * ps / den
        v = F(1) + ps / den
        w = F(1) + ps
        first = a / v * z
        second = F(1) / v - F(1) / w if mutant != "vw_swapped" else F(1) / w - F(1) / v
        term = F(-0.5) * a * a * z * z / v + F(0.5) * (np.log(w) - np.log(v))
        tl = _lanes(term.astype(F))
        s = np.zeros((N, 64), F)
        for b in range(tl.shape[1]):
            s = s + tl[:, b]
        r = _wave_sum(s)
        rows = np.hstack([first, np.broadcast_to(second, first.shape)]).astype(F)
    elif side == SIDE_TEST:
        rows = np.hstack([z, F(-0.5) * z * z]).astype(F)
    elif side == SIDE_COSINE:
        s = _sumsq_fma(z, mutant)
        with np.errstate(divide="ignore", invalid="ignore"):
            scale = np.where(s > 0, F(1) / np.sqrt(s), F(1)).astype(F)
        rows = z * scale[:, None]
    else:
        rows = z * F(1)
    assert rows.dtype == F and r.dtype == F
    return rows, r


# ---------------------------------------------------------------------------------------------------------------------------
# prepare: the fp64 reference and its element-wise bounds
# ---------------------------------------------------------------------------------------------------------------------------
def prepare_reference(case):
    """(rows[N, K], r[N]) of tests/backend_ref.py in float64."""
    A, a0 = case.get("A"), case.get("a0")
    transform = None
    if A is not None:
        transform = A.astype(np.float64) if a0 is None else np.hstack([A.astype(np.float64), a0.astype(np.float64)[:, None]])
    plda = None if case.get("P") is None else (case["m"], case["P"], case["psi"])
    n = case.get("n")
    with np.errstate(divide="ignore", invalid="ignore"):
        z = ref.chain(case["x"], case.get("mu"), transform, case.get("length_norm", True), plda, n)
    side = case["side"]
    N = len(z)
    if side == SIDE_ENROL:
        return ref.side_rows_enrol(z, np.ones(N) if n is None else n, case["psi"])
    if side == SIDE_TEST:
        return ref.side_rows_test(z), np.zeros(N)
    if side == SIDE_COSINE:
        nrm = np.linalg.norm(z, axis=1, keepdims=True)
        return z / np.where(nrm > 0, nrm, 1.0), np.zeros(N)
    return z, np.zeros(N)


def prepare_bounds(case, lam=LAMBDA, with_terms=False):
    """The fp64 reference (rows, r) with a bound on |device - reference| for every element, propagated stage by stage.
    Only the two products use the statistical model lam * sqrt(depth) * u * sum|terms|; everything behind them is a dozen
    roundings and is counted in the worst case (each count is derived where it is used).  Also returns, for the CPU companion,
    the bound and the median |term| of every product output (with_terms)."""
    x = np.asarray(case["x"], np.float64)
    N, D = x.shape
    f64 = lambda a: None if a is None else np.asarray(a, np.float64)          # noqa: E731
    mu, A, a0, P, m, psi, n = (f64(case.get(k)) for k in ("mu", "A", "a0", "P", "m", "psi", "n"))
    side = case["side"]
    products = []
    xm = x - mu if mu is not None else x
    if A is not None:
        d = A.shape[0]
        y = xm @ A.T + (a0 if a0 is not None else 0.0)
        # D fmaf roundings, the rounding of x - mu and the addition of a0: D + 2 roundings against M0 = sum|A||x - mu| + |a0|
        M0 = np.abs(xm) @ np.abs(A).T + (np.abs(a0) if a0 is not None else 0.0)
        e = lam * math.sqrt(D + 2) * U * M0
        if with_terms:
            products.append(("lda", e, np.median(np.abs(xm[:, None, :] * A[None, :, :]), axis=2)))
    else:
        d = D
        y = xm
        e = U * np.abs(y) if mu is not None else np.zeros_like(y)          # the one subtraction
    depth = -(-d // 64) + 6                                                 # a lane's chain and the six levels of the butterfly
    if case.get("length_norm", True):
        ss = np.sum(y * y, axis=1)
        ok = ss > 0
        ssd = np.where(ok, ss, 1.0)
        scale = np.where(ok, np.sqrt(d / ssd), 1.0)
        # relative error of the scale: first order in the incoming errors, sum|y|e / sum y^2; its own arithmetic: the sum of
        # positive terms carries depth roundings, halved by the square root, then sqrtf(s), sqrtf(d) and the division: 3 more
        dscale = np.where(ok, np.sum(np.abs(y) * e, axis=1) / ssd + (depth / 2 + 3) * U, 0.0)
        y = y * scale[:, None]
        e = e * scale[:, None] + np.abs(y) * (dscale[:, None] + U)         # + u: the multiplication
    if P is not None:
        ym = y - m
        z = ym @ P.T
        # the incoming errors through |P|; d fmaf roundings and the rounding of y - m: d + 1 against sum|P||y - m|
        e = e @ np.abs(P).T + lam * math.sqrt(d + 1) * U * (np.abs(ym) @ np.abs(P).T)
        if with_terms:
            products.append(("plda", e, np.median(np.abs(ym[:, None, :] * P[None, :, :]), axis=2)))
        nn = np.ones(N) if n is None else n
        q = psi[None, :] + 1.0 / nn[:, None]
        S = np.sum(z * z / q, axis=1)
        ok = S > 0
        Sd = np.where(ok, S, 1.0)
        scale = np.where(ok, np.sqrt(d / Sd), 1.0)
        # S: per term z*z, 1/n, psi + 1/n and the division (4 roundings), the sum's depth, d / S (1); halved by the root, + sqrtf
        dscale = np.where(ok, np.sum(np.abs(z) * e / q, axis=1) / Sd + ((4 + depth + 1) / 2 + 1) * U, 0.0)
        y = z * scale[:, None]
        e = e * scale[:, None] + np.abs(y) * (dscale[:, None] + U)
    z = y
    br = np.zeros(N)
    if side == SIDE_ENROL:
        nn = (np.ones(N) if n is None else n)[:, None]
        a, v, w = ref._avw(psi[None, :], nn)
        # n psi (1 rounding), + 1 (1): den within 2u; a = n psi / den: 1 + 2 + 1 = 4u.  psi / den: 3u, 1 + it: v within 4u.
        # a / v: 4 + 4 + 1 = 9u, times z: 10u.  w = 1 + psi: u.
        first = a / v * z
        b_first = a / v * e + 10 * U * np.abs(first)
        # 1/v: 4 + 1 = 5u, 1/w: 1 + 1 = 2u, the subtraction 1 more; it cancels, so the count is against 1/v + 1/w
        second = 1.0 / v - 1.0 / w
        b_second = np.broadcast_to(6 * U * (1.0 / v + 1.0 / w), first.shape)
        rows = np.hstack([first, np.broadcast_to(second, first.shape)])
        brows = np.hstack([b_first, b_second])
        # r: T1 = a^2 z^2 / (2v): a (4u), (-a/2) a (4 + 1), z, z (2), / v (4 + 1): 16u, and 1 for T1 + T2: 17u; its z error
        # a^2 |z| e / v.  T2 = (log w - log v) / 2: logf within 2 ulp = 4u of its value, the arguments' u and 4u as absolute
        # errors, the subtraction and T1 + T2: (4 + 1 + 1) u against (|log w| + |log v|) / 2, plus 2.5u per column.
        T1 = a * a * z * z / (2 * v)
        L = 0.5 * (np.abs(np.log(w)) + np.abs(np.log(v))) * np.ones_like(z)
        r = -np.sum(T1, axis=1) + 0.5 * np.sum((np.log(w) - np.log(v)) * np.ones_like(z), axis=1)
        br = U * ((depth + 17) * np.sum(T1, axis=1) + (depth + 6) * np.sum(L, axis=1) + 2.5 * d) + np.sum(a * a * np.abs(z) * e / v, axis=1)
    elif side == SIDE_TEST:
        # -z^2 / 2: the halving is exact, one rounding of the product; z's error to second order
        rows = np.hstack([z, -0.5 * z * z])
        brows = np.hstack([e, np.abs(z) * e + 0.5 * e * e + U * 0.5 * z * z])
        r = np.zeros(N)
    elif side == SIDE_COSINE:
        ss = np.sum(z * z, axis=1)
        ok = ss > 0
        ssd = np.where(ok, ss, 1.0)
        scale = np.where(ok, 1.0 / np.sqrt(ssd), 1.0)
        # the fmaf sum (depth, halved), sqrtf and the division
        dscale = np.where(ok, np.sum(np.abs(z) * e, axis=1) / ssd + (depth / 2 + 2) * U, 0.0)
        rows = z * scale[:, None]
        brows = e * scale[:, None] + np.abs(rows) * (dscale[:, None] + U)
        r = np.zeros(N)
    else:
        rows, brows, r = z, e, np.zeros(N)
    want_rows, want_r = prepare_reference(case)                            # the reference proper: tests/backend_ref.py
    assert np.allclose(rows, want_rows, rtol=1e-9, atol=1e-12) and np.allclose(r, want_r, rtol=1e-9, atol=1e-12)
    return dict(rows=want_rows, brows=brows, r=want_r, br=br, products=products)


def assert_prepare_within(got_rows, got_r, bounds, what, limit=1.0):
    """Every element of the rows and of r within limit * its bound; an element whose bound is 0 must be equal.  Returns the
    worst ratios (rows, r)."""
    worst = []
    for got, want, bnd, name in ((got_rows, bounds["rows"], bounds["brows"], "rows"), (got_r, bounds["r"], bounds["br"], "r")):
        got = np.asarray(got, np.float64)
        assert got.shape == want.shape, (what, name, got.shape, want.shape)
        assert np.all(np.isfinite(got)), (what, name, "non-finite output")
        err = np.abs(got - want)
        ratio = np.where(bnd > 0, err / np.where(bnd > 0, bnd, 1.0), np.where(err > 0, np.inf, 0.0))
        worst.append(float(ratio.max()) if ratio.size else 0.0)
        if worst[-1] > limit:
            idx = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
            raise AssertionError("%s: %s%s is %.3f of its bound (got %r, want %r, bound %.3e); %d of %d elements over" % (
                what, name, tuple(int(i) for i in idx), worst[-1], float(got[idx]), float(want[idx]), float(bnd[idx]),
                int((ratio > limit).sum()), ratio.size))
    return tuple(worst)


def fraction_over(got_rows, got_r, bounds, affected_rows, affected_r=None):
    """The share of the affected elements (boolean masks) that exceed their bound: the measure of a mutant."""
    over = np.abs(np.asarray(got_rows, np.float64) - bounds["rows"]) > bounds["brows"]
    cnt, tot = int((over & affected_rows).sum()), int(affected_rows.sum())
    if affected_r is not None:
        over_r = np.abs(np.asarray(got_r, np.float64) - bounds["r"]) > bounds["br"]
        cnt, tot = cnt + int((over_r & affected_r).sum()), tot + int(affected_r.sum())
    return cnt / max(tot, 1), tot


# ---------------------------------------------------------------------------------------------------------------------------
# prepare: the cases
# ---------------------------------------------------------------------------------------------------------------------------
# (D, d, N): every D of {1, 2, 31, 33, 64, 65, 150, 600, 2048}, every d of {1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 150,
# 255, 256} and every N of {1, 31, 32, 33, 97} at least once; not the full product.
SHAPES = ((1, 1, 1), (2, 2, 31), (31, 31, 32), (33, 32, 33), (64, 33, 97), (65, 63, 1), (150, 64, 31), (600, 65, 32), (2048, 127, 33),
          (64, 128, 97), (150, 129, 33), (600, 150, 97), (2048, 255, 31), (65, 256, 32))

# name -> (side, mean, lda, offset, length_norm, plda, counts)
COMBOS = {
    "full_enrol": (SIDE_ENROL, True, True, True, True, True, True),          # what the product calls: the scoring chain
    "full_test": (SIDE_TEST, True, True, True, True, True, False),
    "full_cosine": (SIDE_COSINE, True, True, True, True, True, False),
    "raw_enrol": (SIDE_ENROL, False, False, False, False, True, True),       # Scorer(transform=None): processed vectors, d = D
    "raw_test": (SIDE_TEST, False, False, False, False, True, False),
    "plain_lda": (SIDE_PLAIN, True, True, True, True, False, False),         # compute-plda --lda
    "cosine_raw": (SIDE_COSINE, True, False, False, True, False, False),     # cosine without LDA or PLDA
    "no_offset_test": (SIDE_TEST, True, True, False, True, True, False),     # lda_offset = None
    "mean_no_lda_enrol": (SIDE_ENROL, True, False, False, True, True, True),
    "enrol_no_counts": (SIDE_ENROL, True, True, True, True, True, False),    # num_utts = None
    "plain_plda": (SIDE_PLAIN, True, True, True, True, True, False),
}


def realistic_case(combo, D, d, N, seed=0):
    """x ~ N(0.5, 1), mu ~ 0.5 + 0.1 N, A ~ N(0, 1/D), a0 ~ 0.1 N; P = (orthogonal) * U(0.5, 2), m ~ 0.3 N, psi log-uniform in
    [1e-2, 1e2] descending, counts 1..11.  Without an LDA the vectors have d = D columns (the d of the shape)."""
    side, has_mu, has_lda, has_off, ln, has_plda, has_n = COMBOS[combo]
    rng = np.random.default_rng([seed, D, d, N, sorted(COMBOS).index(combo)])
    if not has_lda:
        D = d
    case = dict(side=side, length_norm=ln, name="%s D%d d%d N%d" % (combo, D, d, N))
    case["x"] = (rng.standard_normal((N, D)) + 0.5).astype(F)
    if has_mu:
        case["mu"] = (0.5 + 0.1 * rng.standard_normal(D)).astype(F)
    if has_lda:
        case["A"] = (rng.standard_normal((d, D)) / math.sqrt(D)).astype(F)
        if has_off:
            case["a0"] = (0.1 * rng.standard_normal(d)).astype(F)
    if has_plda:
        q, _ = np.linalg.qr(rng.standard_normal((d, d)))
        case["P"] = (q * rng.uniform(0.5, 2.0, d)[None, :]).astype(F)
        case["m"] = (0.3 * rng.standard_normal(d)).astype(F)
        case["psi"] = np.sort(10.0 ** rng.uniform(-2, 2, d))[::-1].astype(F)
    if has_n:
        case["n"] = rng.integers(1, 12, N).astype(np.int32)
    return case


def prepare_cases():
    """Every combination at every shape: 11 x 14 cases, each a few ms of replay."""
    return [realistic_case(c, D, d, N) for c in COMBOS for (D, d, N) in SHAPES]


def product_case(D, d, N, lda=True, seed=1):
    """Layer (a): PLAIN, no PLDA, no length norm: the output is the product itself (or x - mu)."""
    rng = np.random.default_rng([seed, D, d, N, int(lda)])
    if not lda:
        D = d
    case = dict(side=SIDE_PLAIN, length_norm=False, name="product D%d d%d N%d lda%d" % (D, d, N, lda))
    case["x"] = (rng.standard_normal((N, D)) + 0.5).astype(F)
    case["mu"] = (0.5 + 0.1 * rng.standard_normal(D)).astype(F)
    if lda:
        case["A"] = (rng.standard_normal((d, D)) / math.sqrt(D)).astype(F)
        case["a0"] = (0.1 * rng.standard_normal(d)).astype(F)
    return case


def onehot_lda_case(D, N, seed=2):
    """A signed one-hot A with entries +-1, +-2 whose row j reads column k_j of x - mu: every k of the first, a middle and the
    (ragged) last 32-k slice, at most 256 of them.  out[i, j] must equal A[j, k_j] * (x[i, k_j] - mu[k_j]) exactly (scaling by
    1 or 2 is exact); no offset."""
    rng = np.random.default_rng([seed, D, N])
    ns = -(-D // 32)
    ks = sorted({k for s in {0, ns // 2, ns - 1} for k in range(32 * s, min(32 * s + 32, D))})
    d = len(ks)
    A = np.zeros((d, D), F)
    A[np.arange(d), ks] = rng.choice([-2.0, -1.0, 1.0, 2.0], d)
    case = dict(side=SIDE_PLAIN, length_norm=False, name="onehot D%d N%d" % (D, N))
    case["x"] = (rng.standard_normal((N, D)) + 0.5).astype(F)
    case["mu"] = (0.5 + 0.1 * rng.standard_normal(D)).astype(F)
    case["A"] = A
    want = (case["x"] - case["mu"][None, :])[:, ks] * A[np.arange(d), ks][None, :]
    return case, want.astype(F)


def integer_lda_case(D, d, N, seed=3):
    """Integer x in [-3, 3], mu in halves in [-0.5, 0.5], integer A in [-2, 2], integer a0: A (x - mu) + a0 is exact in any
    order; the largest magnitude, 2048 * 3.5 * 2 plus a0, stays below 2^24 in halves."""
    rng = np.random.default_rng([seed, D, d, N])
    case = dict(side=SIDE_PLAIN, length_norm=False, name="integer D%d d%d N%d" % (D, d, N))
    case["x"] = rng.integers(-3, 4, (N, D)).astype(F)
    case["mu"] = (rng.integers(-1, 2, D) / 2.0).astype(F)
    case["A"] = rng.integers(-2, 3, (d, D)).astype(F)
    case["a0"] = rng.integers(-9, 10, d).astype(F)
    want = (case["x"].astype(np.float64) - case["mu"]) @ case["A"].astype(np.float64).T + case["a0"]
    assert np.abs(want).max() * 2 < 2 ** 24
    return case, want


def exact_plda_case(d, N, side, seed=4):
    """The PLDA step with a known answer: no LDA, no length norm, P a signed permutation, m integer, psi in {0, 3, 15}, counts
    None (psi + 1/n = 1, 4, 16), x such that z_c = +-sqrt(psi_c + 1) in {+-1, +-2, +-4}.  Every term of the norm sum is exactly
    1, the sum is d in any order and the scale is sqrtf(d / d) = 1.  PLAIN gives z, TEST [z, -z^2/2] in every bit."""
    rng = np.random.default_rng([seed, d, N])
    perm = rng.permutation(d)
    sign = rng.choice([-1.0, 1.0], d)
    P = np.zeros((d, d), F)
    P[np.arange(d), perm] = sign
    psi = rng.choice([0.0, 3.0, 15.0], d).astype(F)
    m = rng.integers(-5, 6, d).astype(F)
    z = (rng.choice([-1.0, 1.0], (N, d)) * np.sqrt(psi + 1.0)[None, :]).astype(F)
    x = (z.astype(np.float64) @ P.astype(np.float64) + m).astype(F)          # P^T z + m: z = P (x - m)
    case = dict(side=side, length_norm=False, x=x, P=P, m=m, psi=psi, name="exact_plda d%d N%d side%d" % (d, N, side))
    return case, z


def zero_vector_case(combo, D, d, N, seed=5):
    """A realistic case without a mean or an LDA offset whose rows 0 and N - 1 are all-zero vectors."""
    case = realistic_case(combo, D, d, N, seed=seed)
    case.pop("mu", None)
    case.pop("a0", None)
    case["x"] = case["x"].copy()
    case["x"][0] = 0
    case["x"][-1] = 0
    case["name"] = "zero_vector " + case["name"]
    return case
