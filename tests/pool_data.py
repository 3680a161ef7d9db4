"""Cases, data builders, the float32 replay and the bound functions of the element-wise pooling tests
(tests/test_gpu_pool_elementwise.py and its CPU companion tests/test_pool_bounds_cpu.py).

Everything here is NumPy; nothing needs the GPU.  U = 2^-24 is the unit roundoff of fp32 (|fl(x) - x| <= U |x|), X = max_t |x| and
R = max_t x - min_t x of one channel over one chunk, M2 = sum_t (x - mean)^2.

The bounds of xv_stats_pool_f32 / xv_chunk_moments_f32 (stats_pool_kernel + stats_pool_merge_kernel, csrc/xv_pool.hip)
----------------------------------------------------------------------------------------------------------------------------
A lane reduces its rows in 8-row blocks (shifted by the block's first row), merges the blocks into a running (n, mean, M2) with Chan's
update, the four row phases of a wave are merged (xor 16, xor 32) and the splits of a long chunk after them.  Longest path:

    merges(len, split) = ceil(min(len, split) / 32) + 2 + (number of splits, if more than one)

Block mean  bm = v0 + (sum_i (v_i - v0)) / m:  7 differences (|d| <= 2X, U 2X each), 6 additions of partial sums <= 2kX (k = 2..7:
54 U X), all divided by 8 -> 8.5 U X; the division 2 U X, the last addition U X:  11.5 U X, counted as A_BLOCK_MEAN = 12.
Chan merge  mean' = mean + (bm - mean) w, w = m / (n + m) <= 1:  mean' is a convex combination of its inputs, so their errors do not
add: err' <= max(err) + the local roundings -- d (2 U X), w (U |d| w <= 2 U X), d w (2 U X), the sum (U X):  A_MERGE_MEAN = 7.

    |mean - mean_ref| <= (A_BLOCK_MEAN + A_MERGE_MEAN merges + 1) U X =: E_mean        (+ 1: second-order terms)

Block M2  = sum_i e_i^2, e_i = fl(fl(v_i - v0) - md):  e_i = (x_i - a) + eps_i with a = v0 + md and |eps_i| <= U (|x_i - v0| + |x_i - a|);
sum (x_i - a)^2 = M2_b + m (a - mean_b)^2 (second order), the cross term 2 sum |x_i - a| |eps_i| <= 2 U (sqrt(8) + 1) M2_b (Cauchy-Schwarz
with sum (x_i - v0)^2 <= 8 M2_b), 8 squarings and 7 additions of non-negative terms 8 U M2_b:  A_BLOCK_M2 = 16.
Chan merge  M2' = M2 + (bM2 + d d (n w)):  the non-negative term d^2 n w takes 4 roundings (w, n w, d d, the product), the two
additions one each:  A_MERGE_M2 = 6 on the path of every term.  All terms are non-negative, so

    relative part:  (A_BLOCK_M2 + A_MERGE_M2 merges) U M2

The cross term: a merge uses d = fl(bm - mean) of two ROUNDED means where the exact update has the difference of the exact ones:
|delta_d| <= 2 E_mean + U R.  With c_k = n m / (n + m) of merge k:  sum_k c_k d_k^2 <= M2 (it is what the merges add), and
sum_k c_k <= 3 len (c_k <= min(n, m): the block merges of all lanes together <= len, the phase merges <= len, the split merges <= len), so

    sum_k c_k (2 |d_k| delta + delta^2) <= 2 delta sqrt(3 len M2) + 3 len delta^2,     delta = 2 E_mean + U R

(sqrt(3 len M2) = len sqrt(3) sigma <= 3 len R: this is the issue's "range and max|x|" form with sigma in place of the range, never
larger).  The variance is M2 / len (one more rounding), the deviation sqrtf(var + eps): two roundings and the error of var through the
square root, |sqrt(a) - sqrt(b)| <= |a - b| / sqrt(b).

None of the constants is fitted: they were fixed from the code before the first device run."""

import numpy as np

U = 2.0 ** -24
EPS32 = np.float32(1e-5)
F = np.float32

A_BLOCK_MEAN, A_MERGE_MEAN = 12, 7
A_BLOCK_M2, A_MERGE_M2 = 16, 6
GRID_Z = 65535                       # chunks per launch of the slicing loops

# ---------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------
EXACT_LENS = ((1, 512), (2, 512), (4, 512), (8, 512), (16, 512), (32, 512), (64, 512), (64, 32))      # (len, split_rows)
INEXACT_NEIGHBOURS = ((3, 512), (96, 512), (48, 512), (96, 32))
LENS = (3, 5, 7, 9, 31, 33, 63, 65, 100, 128, 129, 511, 512, 513, 1025)
CHANNELS = (4, 60, 64, 68, 256, 260)
# (name, lengths of the batch, split_rows): "direct" has max_len <= split_rows (one kernel), the others go through the partials
MODES = (("direct", tuple(n for n in LENS if n <= 512), 512), ("split512", LENS, 512), ("split128", LENS, 128))
KINDS = ("relu", "const", "mean200", "spike", "alt")
BLOCK_LENS = (1, 7, 8, 9, 15, 17, 24, 25, 33, 10000)
BLOCK_EXACT_LENS = (8, 16, 64, 4096)
SOFTMAX_LENS = (1, 2, 255, 256, 257, 1023, 5000)
SOFTMAX_SPREADS = (0.0, 10.0, 80.0, 200.0)
SOFTMAX_PEAKS = (0, 63, 64, 127, 128, 255, 256, -1)      # where a lone maximum sits (one position per wave, both ends of a stride)
SCORE_CHANNELS = (4, 252, 256, 260, 508, 512, 516, 1536)
TANH_ARGS = np.array([0.0] + [s * a for a in (2.0 ** -149, 1e-30, 1e-4, 0.5, 9.0, 20.0, 44.5, 89.0, 1e4, np.inf) for s in (1, -1)], np.float32)
TANH_SATURATED = 89.0                # |x| >= this: the result is exactly +-1
AVG_DIMS = (1, 255, 257)


def merges(n, split):
    nsplit = -(-n // split)
    return -(-min(n, split) // 32) + 2 + (nsplit if nsplit > 1 else 0)


def layout(lens, gap=3, align=1):
    """row_start, total rows: `gap` rows before the first chunk and after every chunk, starts on multiples of `align`."""
    starts, r = [], gap
    for n in lens:
        r = -(-r // align) * align
        starts.append(r)
        r += n + gap
    return np.asarray(starts, np.int32), r


def channel(kind, n, rng):
    """One channel of n frames (float32)."""
    if kind == "relu":
        return (np.maximum(rng.standard_normal(n), 0) * 1.7 + 3.0 * rng.standard_normal()).astype(F)
    if kind == "const":
        return np.full(n, F(rng.uniform(-40, 40)), F)
    if kind == "mean200":
        return (200.0 + 0.1 * rng.standard_normal(n)).astype(F)
    if kind == "spike":
        x = np.zeros(n, F)
        x[rng.integers(n)] = 1e3
        return x
    if kind == "alt":
        return (50.0 + 1e-3 * (1 - 2 * (np.arange(n) & 1))).astype(F)
    raise ValueError(kind)


def kind_of(b, c):
    return KINDS[(b + c) % len(KINDS)]          # every kind in every batch, also at C = 4


def chunk(b, n, C, rng):
    return np.stack([channel(kind_of(b, c), n, rng) for c in range(C)], axis=1)


def batch(lens, C, seed, fill=np.nan, ld=None, col0=0):
    """(parent [rows, ld] filled with `fill`, row_start, list of chunk matrices); the chunks sit in columns [col0, col0 + C)."""
    rng = np.random.default_rng(seed)
    rs, rows = layout(lens)
    ld = C if ld is None else ld
    host = np.full((rows, ld), fill, F)
    mats = []
    for b, (s, n) in enumerate(zip(rs, lens)):
        m = chunk(b, n, C, rng)
        host[s:s + n, col0:col0 + C] = m
        mats.append(m)
    return host, rs, mats


def integer_chunk(n, C, seed):
    """Integers in [-64, 64] plus a constant integer offset per channel."""
    rng = np.random.default_rng(seed)
    return (rng.integers(-64, 65, size=(n, C)) + rng.integers(-100, 101, size=C)).astype(F)


# ---------------------------------------------------------------------------------------------------------------------------
# references (fp64) and bounds of stats_pool / chunk_moments
# ---------------------------------------------------------------------------------------------------------------------------
def moments_ref(m):
    """fp64 (mean, biased variance) over the frames of m [..., len, C]."""
    x = m.astype(np.float64)
    mean = x.mean(-2)
    return mean, ((x - mean[..., None, :]) ** 2).mean(-2)


def std32(var):
    """sqrtf((float)var + eps) in float32."""
    return np.sqrt(np.asarray(var).astype(F) + EPS32)


def moment_bounds(m, split):
    """Per channel: (bound of |mean - ref|, of |var - ref|, of |std - ref|) for the chunk(s) m [..., len, C]; see the module
    docstring."""
    x = m.astype(np.float64)
    n = x.shape[-2]
    k = merges(n, split)
    X = np.abs(x).max(-2)
    R = x.max(-2) - x.min(-2)
    mean, var = moments_ref(m)
    M2 = var * n
    e_mean = (A_BLOCK_MEAN + A_MERGE_MEAN * k + 1) * U * X
    delta = 2 * e_mean + U * R
    e_m2 = (A_BLOCK_M2 + A_MERGE_M2 * k) * U * M2 + 2 * delta * np.sqrt(3 * n * M2) + 3 * n * delta ** 2
    e_var = e_m2 / n + U * (var + e_m2 / n)
    s = var + float(EPS32)
    t = e_var + U * (s + e_var)                                  # |fl(var + eps) - (var_ref + eps)|
    e_std = t / np.sqrt(s) + U * (np.sqrt(s) + t / np.sqrt(s))
    return e_mean, e_var, e_std


# ---------------------------------------------------------------------------------------------------------------------------
# float32 replay of stats_pool_kernel + stats_pool_merge_kernel (without FMA contraction: on exact data every operation is
# exact either way)
# ---------------------------------------------------------------------------------------------------------------------------
UNROLL = 8


def _chan_merge(s, bmean, bm2, m):
    n, mean, m2 = s
    nn = F(n + m)
    if nn > 0:
        w = F(m) / nn
        d = bmean - mean
        mean = mean + d * w
        m2 = m2 + (bm2 + d * d * F(n * w))
        n = nn
    return n, mean, m2


def _replay_split(x):
    """(n, mean, M2) of the rows x [n_rows, C] as one wave of stats_pool_kernel forms them (read by phase 0)."""
    n_rows, C = x.shape
    lanes = []
    for phase in range(4):
        s = (F(0), np.zeros(C, F), np.zeros(C, F))
        r = phase
        while r + 4 * (UNROLL - 1) < n_rows:
            v = x[r:r + 4 * UNROLL:4]
            d = v[1:] - v[0]
            sumd = np.zeros(C, F)
            for i in range(UNROLL - 1):
                sumd = sumd + d[i]
            md = sumd * F(1.0 / UNROLL)
            bm = v[0] + md
            m2 = md * md
            for i in range(UNROLL - 1):
                e = d[i] - md
                m2 = m2 + e * e
            s = _chan_merge(s, bm, m2, F(UNROLL))
            r += 4 * UNROLL
        if r < n_rows:
            v = x[r::4]
            fm = F(v.shape[0])
            sumd = np.zeros(C, F)
            for i in range(1, v.shape[0]):
                sumd = sumd + (v[i] - v[0])
            md = sumd / fm
            bm = v[0] + md
            m2 = md * md
            for i in range(1, v.shape[0]):
                e = (v[i] - v[0]) - md
                m2 = m2 + e * e
            s = _chan_merge(s, bm, m2, fm)
        lanes.append(s)
    for off in (1, 2):                           # xor 16, then xor 32, on the phase number
        lanes = [_chan_merge(lanes[p], lanes[p ^ off][1], lanes[p ^ off][2], lanes[p ^ off][0]) for p in range(4)]
    return lanes[0]


def replay_moments(m, split):
    """float32 (mean, biased variance) of the chunk m [len, C] in the kernel's operation order."""
    m = np.ascontiguousarray(m, F)
    n = m.shape[0]
    with np.errstate(all="ignore"):
        if n <= split:                           # (a lone split still goes through the merge kernel when another chunk is long:
            cnt, mean, m2 = _replay_split(m)     #  merging into the empty state is exact)
            return mean, m2 / cnt
        s = (F(0), np.zeros(m.shape[1], F), np.zeros(m.shape[1], F))
        for b in range(0, n, split):
            part = _replay_split(m[b:b + split])
            cnt, mean, m2 = s
            mm = part[0]
            nn = F(cnt + mm)
            w = mm / nn
            d = part[1] - mean
            s = (nn, mean + d * w, m2 + (part[2] + d * d * F(cnt * w)))
        return s[1], s[2] / s[0]


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, F).view(np.uint32), np.ascontiguousarray(b, F).view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------------
# block statistics (xv_stats_pool_blocks_f32)
# ---------------------------------------------------------------------------------------------------------------------------
def blocks_of(m):
    """fp32 (mean, M2) per 8-row block of the chunk m, rounded once from fp64: [nb, 2, C]."""
    x = m.astype(np.float64)
    nb = -(-x.shape[0] // 8)
    out = np.empty((nb, 2, x.shape[1]), F)
    for i in range(nb):
        blk = x[8 * i:8 * i + 8]
        mu = blk.mean(0)
        out[i, 0] = mu
        out[i, 1] = ((blk - mu) ** 2).sum(0)
    return out


def dyadic_blocks(n, C, seed):
    """Block means that are multiples of 1/8 and M2 that are multiples of 1/64 (n % 8 == 0)."""
    rng = np.random.default_rng(seed)
    nb = n // 8
    out = np.empty((nb, 2, C), F)
    out[:, 0] = rng.integers(-8 * 160, 8 * 160 + 1, size=(nb, C)) / 8.0
    out[:, 1] = rng.integers(0, 64 * 2048, size=(nb, C)) / 64.0
    return out


def blocks_ref(blk, n):
    """The header's formula in long double on the fp32 blocks blk [nb, 2, C]: mean, var (clamped at 0), Q / len."""
    b = blk.astype(np.longdouble)
    cnt = np.minimum(8, n - 8 * np.arange(b.shape[0])).astype(np.longdouble)[:, None]
    S = (cnt * b[:, 0]).sum(0)
    Q = (b[:, 1] + cnt * b[:, 0] * b[:, 0]).sum(0)
    mean = S / n
    var = np.maximum(Q / n - mean * mean, 0)
    return mean.astype(np.float64), var.astype(np.float64), (Q / n).astype(np.float64)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x)).astype(F)).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------------
def dyadic_weights(n, seed, depth=10):
    """n weights 2^-k (k <= depth) that sum to 1 exactly; n <= 2^depth."""
    assert 1 <= n <= 2 ** depth
    rng = np.random.default_rng(seed)
    ks = [0]
    while len(ks) < n:
        cand = [i for i, k in enumerate(ks) if k < depth]
        i = cand[rng.integers(len(cand))]
        ks[i] += 1
        ks.insert(i, ks[i])
    w = np.ldexp(1.0, -np.asarray(ks))
    assert w.sum() == 1.0
    return rng.permutation(w).astype(F)


def attention_pool_ref(m, a):
    """Long-double s1 = sum a x, q = sum a x^2 - s1^2 (not clamped), s2 = sum a x^2 of the chunk(s) m [..., len, C] with weights
    a [..., len]."""
    x = m.astype(np.longdouble)
    w = a.astype(np.longdouble)[..., None]
    s1 = (w * x).sum(-2)
    s2 = (w * x * x).sum(-2)
    return s1, s2 - s1 * s1, s2


def attention_pool_bounds(m, a):
    """(mean ref, std ref, bound of mean, bound of std): 1 ulp for the mean (the cast of an fp64 sum) and 2 ulp for the std (three
    fp32 roundings of relative size U/2, U/2 and U: 2 U sd < 2 ulp), each plus what the fp64 sums carry: (len + 2) 2^-53 sum |a x|
    for the mean, (len + 2) 2^-53 (s2 + 2 |s1| sum |a x|) / (2 sd) through q = s2 - s1^2 and the square root for the std (len + 2:
    the additions on the longest path -- a lane's rows, two phase merges, the splits -- and the rounding of x^2)."""
    s1, q, s2 = attention_pool_ref(m, a)
    s1, q, s2 = s1.astype(np.float64), q.astype(np.float64), s2.astype(np.float64)
    sd = np.sqrt(np.maximum(q, 0) + float(EPS32))
    n = m.shape[-2]
    g = (n + 2) * 2.0 ** -53
    absx = (np.abs(a.astype(np.float64))[..., None] * np.abs(m.astype(np.float64))).sum(-2)
    return s1, sd, ulp32(s1) + g * absx, 2 * ulp32(sd) + g * (s2 + 2 * np.abs(s1) * absx) / (2 * sd)


def attention_pool_exact(m, a):
    """[float(m) | sqrtf(float(q) + eps)] where s1, s2 and q are exact in fp64 (dyadic weights, integer h)."""
    x = m.astype(np.float64)
    w = a.astype(np.float64)[:, None]
    s1 = (w * x).sum(0)
    q = (w * x * x).sum(0) - s1 * s1
    return s1.astype(F), np.sqrt(np.maximum(q, 0).astype(F) + EPS32)


def many_chunks(n, C, seed):
    """n chunks of lengths 1, 2, 3, 1, ... packed without gaps: (x [rows, C] post-ReLU-like, row_start, row_len)."""
    rng = np.random.default_rng(seed)
    rl = (np.arange(n) % 3 + 1).astype(np.int32)
    rs = np.concatenate([[0], np.cumsum(rl)[:-1]]).astype(np.int32)
    rows = int(rl.sum())
    x = (np.maximum(rng.standard_normal((rows, C)), 0) * 1.7 + 3.0 * rng.standard_normal(C)).astype(F)
    return x, rs, rl


def by_length(x, rs, rl):
    """[(indices of the chunks of length k, their rows [n_k, k, ...])] for the lengths that occur."""
    out = []
    for k in np.unique(rl):
        idx = np.nonzero(rl == k)[0]
        out.append((idx, x[rs[idx][:, None] + np.arange(k)[None, :]]))
    return out


def softmax_scores(n, spread, peak, rng):
    """fp32 scores of one chunk: uniform over `spread`; peak (a position or None): a lone maximum 100 above everything else."""
    s = (spread * rng.random(n) - 0.37 * spread).astype(F)
    if peak is not None:
        s[peak] = s.max() + F(100.0)
    return s


def softmax_cases():
    """(len, spread, peak position or None)"""
    out = [(n, sp, None) for n in SOFTMAX_LENS for sp in SOFTMAX_SPREADS]
    for n in SOFTMAX_LENS:
        for p in SOFTMAX_PEAKS:
            pos = n - 1 if p < 0 else p
            if pos < n and (n, 200.0, pos) not in out:
                out.append((n, 200.0, pos))
    return out


def softmax_ref(s):
    d = s.astype(np.float64) - float(s.max())
    e = np.exp(d)
    return e / e.sum(), np.abs(d)


TINY32 = float(np.finfo(np.float32).tiny)


def softmax_bound(a_ref, absd):
    return (absd + 4) * U * a_ref + TINY32


def chunk_average_ref(embs, lens):
    """The NumPy float32 expression of the reference for one utterance (tests/test_gpu_kernels.py::test_chunk_average_bit_exact)."""
    acc, tot = 0, 0.0
    for ln, ev in zip(lens, embs):
        tot += int(ln)
        acc = acc + int(ln) * ev
    acc = acc / tot
    return acc.astype(F)


def chunk_average_ref_batched(e, seg, lens):
    """The same float32 operations for many utterances at once (element-wise float32 operations do not depend on the batching)."""
    nutt = len(seg) - 1
    cnt = np.diff(seg)
    out = np.empty((nutt, e.shape[1]), F)
    lf = lens.astype(F)[:, None]
    for k in np.unique(cnt):
        idx = np.nonzero(cnt == k)[0]
        acc = np.zeros((len(idx), e.shape[1]), F)
        tot = np.zeros(len(idx), np.float64)
        for j in range(k):
            rows = seg[idx] + j
            acc = acc + lf[rows] * e[rows]
            tot += lens[rows]
        out[idx] = acc / tot.astype(F)[:, None]
    return out
