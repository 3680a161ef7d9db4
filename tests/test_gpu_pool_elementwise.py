"""Element-wise checks of the kernels that turn frames into the pooled vector: xv_stats_pool_f32 / xv_chunk_moments_f32 /
xv_stats_pool_blocks_f32 / xv_chunk_average_f32 (csrc/xv_pool.hip) and the attention forward xv_attention_scores_f32 /
xv_attention_softmax_f32 / xv_attention_pool_f32 (csrc/xv_attention.hip).  One relative-L2 number per chunk hides a wrong channel,
row phase, block count or slice of chunks:

* exact known answers: integer frames at the lengths where every count the kernel divides by is a power of two (settled by the
  float32 replay of tests/test_pool_bounds_cpu.py), dyadic block statistics, dyadic attention weights -- every output bit;
* element-wise bounds derived from the roundings of the longest path (tests/pool_data.py) on ordinary and hostile channels, at
  lengths around the 8-row block, the 32-row step and the split, channel counts around a wave and a workgroup, a column slice of
  a wider NaN-filled buffer; the worst ratio per quantity is printed at the end;
* more than 65535 chunks: the second slice of every host loop that cuts the chunk list for the grid limit;
* the contracts: ldh < C is refused, an empty chunk gives NaN and leaves its neighbours' bits alone.

Every reference is fp64 (or long double) NumPy of the formula of include/xvector_hip.h on exactly the arrays the kernel under
test received.  Outputs are NaN-poisoned, gap rows hold NaN, and a sentinel row behind every output must come back untouched."""
import ctypes

import numpy as np
import pytest

import pool_data as pd

pytestmark = pytest.mark.gpu

WORST = {}
EPS = float(pd.EPS32)
BAD_ARG = -1
SENTINEL = -12345.0


def _note(key, value):
    WORST[key] = max(WORST.get(key, 0.0), float(value))


@pytest.fixture(scope="module")
def env(oracle_mod):
    import torch
    from xvector_amd import hiplib
    hiplib.require_gpu()
    yield dict(torch=torch, hiplib=hiplib, lib=hiplib.load(), dev=torch.device("cuda:0"))
    if WORST:
        print("\nworst error / bound per quantity (pool element-wise):")
        for k in sorted(WORST):
            print("  %-58s %.3e" % (k, WORST[k]))


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _dev(env, a):
    return env["torch"].from_numpy(np.ascontiguousarray(a)).to(env["dev"])


def _out(env, nchunks, width):
    """NaN-poisoned [nchunks + 1, width]: the last row is a sentinel."""
    t = env["torch"].full((nchunks + 1, width), float("nan"), dtype=env["torch"].float32, device=env["dev"])
    t[nchunks] = SENTINEL
    return t


def _host(env, t, nchunks):
    env["torch"].cuda.synchronize()
    h = t.cpu().numpy()
    assert (h[nchunks] == SENTINEL).all(), "wrote behind the last chunk"
    return h[:nchunks]


def _ratio(err, bound):
    return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))


def stats_pool(env, h, C, rs, rl, split, raw, max_len=None):
    """xv_stats_pool_f32 (raw = 0) / xv_chunk_moments_f32 (raw = 1) through the raw binding: h is a device view [rows, C] whose row
    stride may exceed C.  Two runs must give the same bits."""
    torch, lib, dev = env["torch"], env["lib"], env["dev"]
    n = len(rl)
    max_len = int(max(rl)) if max_len is None else max_len
    need = int(lib.xv_stats_pool_workspace_bytes(C, n, max_len, split))
    assert (need > 0) == (max_len > split)
    rsd, rld = _dev(env, np.asarray(rs, np.int32)), _dev(env, np.asarray(rl, np.int32))
    res = []
    for _ in range(2):
        ws = torch.full((max(need // 4, 1),), float("nan"), dtype=torch.float32, device=dev)
        out = _out(env, n, 2 * C)
        if raw:
            rc = lib.xv_chunk_moments_f32(_p(h), h.stride(0), C, _p(rsd), _p(rld), n, max_len, split, _p(out), _p(ws), None)
        else:
            rc = lib.xv_stats_pool_f32(_p(h), h.stride(0), C, _p(rsd), _p(rld), n, max_len, split, EPS, _p(out), _p(ws), None)
        assert rc == 0, rc
        res.append(_host(env, out, n))
    assert np.array_equal(res[0].view(np.uint32), res[1].view(np.uint32)), "a second run gives other bits"
    return res[0]


# ---------------------------------------------------------------------------------------------------------------------------
# 1. xv_stats_pool_f32 / xv_chunk_moments_f32
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,split", pd.EXACT_LENS)
def test_moments_exact_on_integer_data(env, n, split):
    """Integer frames in [-64, 64] + a per-channel offset, lengths at which every count is a power of two: mean, biased variance
    and sqrtf(var + eps) are the fp64 answer rounded once, in every bit (C = 68: a full wave and one float4 of the next)."""
    C = 68
    lens = [n, n, n]
    rs, rows = pd.layout(lens)
    host = np.full((rows, C), np.nan, np.float32)
    mats = [pd.integer_chunk(n, C, seed=n * 1000 + split + b) for b in range(3)]
    for s, m in zip(rs, mats):
        host[s:s + n] = m
    h = _dev(env, host)
    mom = stats_pool(env, h, C, rs, lens, split, raw=1)
    pool = stats_pool(env, h, C, rs, lens, split, raw=0)
    for b, m in enumerate(mats):
        mean, var = pd.moments_ref(m)
        for name, got, ref in (("mean", mom[b, :C], mean.astype(np.float32)), ("var", mom[b, C:], var.astype(np.float32)),
                               ("pool mean", pool[b, :C], mean.astype(np.float32)), ("std", pool[b, C:], pd.std32(var))):
            bad = np.nonzero(got.view(np.uint32) != ref.view(np.uint32))[0]
            assert bad.size == 0, (n, split, b, name, len(bad), [(int(c), float(got[c]), float(ref[c])) for c in bad[:5]])


def _check_moments(env, name, host, view, C, rs, lens, mats, split):
    """Both entry points on one batch against the fp64 moments of each chunk, channel by channel.

    Bounds (derivation: tests/pool_data.py): with k = ceil(min(len, split) / 32) + 2 (+ the number of splits) merges on the longest
    path, |mean - ref| <= E_mean = (12 + 7 k + 1) 2^-24 max|x|;  |M2 - ref| <= (16 + 6 k) 2^-24 M2 + 2 d sqrt(3 len M2) + 3 len d^2
    with d = 2 E_mean + 2^-24 range (the rounded means in d d (n w));  var = M2 / len and std = sqrtf(var + eps) add their own
    roundings.  A constant channel: mean exact, var 0, std == sqrtf(eps)."""
    mom = stats_pool(env, view, C, rs, lens, split, raw=1)
    pool = stats_pool(env, view, C, rs, lens, split, raw=0)
    assert np.array_equal(mom[:, :C].view(np.uint32), pool[:, :C].view(np.uint32)), "the two entry points give other means"
    assert np.isfinite(mom).all() and np.isfinite(pool).all()
    fails = []
    for b, m in enumerate(mats):
        mean, var = pd.moments_ref(m)
        e_mean, e_var, e_std = pd.moment_bounds(m, split)
        kinds = [pd.kind_of(b, c) for c in range(C)]
        r = (_ratio(np.abs(mom[b, :C] - mean), e_mean), _ratio(np.abs(mom[b, C:] - var), e_var),
             _ratio(np.abs(pool[b, C:] - np.sqrt(var + EPS)), e_std))
        for q, v in zip(("mean", "var", "std"), r):
            _note("stats_pool %s / bound" % q, v)
            if v > 1:
                fails.append((b, len(m), q, v))
        rel = np.abs(mom[b, C:] - var) / np.maximum(var, 1e-300)
        for c in range(C):
            if kinds[c] == "const":
                assert mom[b, c] == m[0, c] and mom[b, C + c] == 0 and pool[b, C + c] == np.sqrt(pd.EPS32), (name, b, c)
            elif kinds[c] == "mean200":
                _note("stats_pool var relative error, mean-200 channel", rel[c])
    print("%s: worst ratios so far %s" % (name, {k: "%.3e" % v for k, v in WORST.items() if k.startswith("stats_pool")}))
    assert not fails, (name, fails[:8])


@pytest.mark.parametrize("C", pd.CHANNELS)
@pytest.mark.parametrize("mode", pd.MODES, ids=[m[0] for m in pd.MODES])
def test_moments_elementwise_bound(env, mode, C):
    name, lens, split = mode
    host, rs, mats = pd.batch(lens, C, seed=C * 7 + split + len(lens))
    _check_moments(env, "%s C %d" % (name, C), host, _dev(env, host), C, rs, lens, mats, split)


@pytest.mark.parametrize("mode", pd.MODES[::2], ids=[m[0] for m in pd.MODES[::2]])
def test_moments_on_a_column_slice(env, mode):
    """h = columns [8, 8 + 68) of a NaN-filled [rows, 96] buffer (ldh > C)."""
    name, lens, split = mode
    C, ld, col0 = 68, 96, 8
    host, rs, mats = pd.batch(lens, C, seed=99 + split, ld=ld, col0=col0)
    view = _dev(env, host)[:, col0:col0 + C]
    assert view.stride(0) == ld
    _check_moments(env, "%s slice" % name, host, view, C, rs, lens, mats, split)


@pytest.mark.parametrize("split", (512, 2), ids=("direct", "split2"))
def test_moments_more_than_65535_chunks(env, split):
    """65540 chunks of 1 to 3 frames at C = 4: the second slice of the host loop (out, workspace, row_start and row_len offset by
    hand).  Every row within the bound; rows 65534 ... 65539 equal, bit for bit, the same chunks run as a batch of their own."""
    C, n = 4, 65540
    x, rs, rl = pd.many_chunks(n, C, seed=split)
    h = _dev(env, x)
    for raw in (1, 0):
        got = stats_pool(env, h, C, rs, rl, split, raw=raw)
        assert np.isfinite(got).all()
        for idx, rows in pd.by_length(x, rs, rl):
            mean, var = pd.moments_ref(rows)
            e_mean, e_var, e_std = pd.moment_bounds(rows, split)
            ref2, e2 = (var, e_var) if raw else (np.sqrt(var + EPS), e_std)
            r1, r2 = _ratio(np.abs(got[idx, :C] - mean), e_mean), _ratio(np.abs(got[idx, C:] - ref2), e2)
            _note("stats_pool 65540 chunks mean / bound", r1)
            _note("stats_pool 65540 chunks %s / bound" % ("var" if raw else "std"), r2)
            assert r1 <= 1 and r2 <= 1, (raw, len(rows[0]), r1, r2)
        lo = pd.GRID_Z - 1
        small = stats_pool(env, h, C, rs[lo:], rl[lo:], split, raw=raw, max_len=3)
        assert np.array_equal(small.view(np.uint32), got[lo:].view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------------
# 2. xv_stats_pool_blocks_f32 on hand-made block statistics
# ---------------------------------------------------------------------------------------------------------------------------
def _run_blocks(env, blocks, lens, C):
    """blocks: list of [nb, 2, C] per chunk.  The chunks' blocks are laid out one after the other, each followed by one NaN block."""
    torch, hiplib = env["torch"], env["hiplib"]
    parts, rs, blk0 = [], [], 0
    for b in blocks:
        rs.append(8 * blk0)
        parts += [b, np.full((1, 2, C), np.nan, np.float32)]
        blk0 += b.shape[0] + 1
    stats = _dev(env, np.concatenate(parts))
    rsd, rld = _dev(env, np.asarray(rs, np.int32)), _dev(env, np.asarray(lens, np.int32))
    res = []
    for _ in range(2):
        out = _out(env, len(lens), 2 * C)
        hiplib.stats_pool_blocks(stats, C, rsd, rld, len(lens), EPS, out)
        res.append(_host(env, out, len(lens)))
    assert np.array_equal(res[0].view(np.uint32), res[1].view(np.uint32))
    return res[0]


@pytest.mark.parametrize("C", (4, 260))
def test_blocks_exact_on_dyadic_statistics(env, C):
    """Block means in 1/8, M2 in 1/64, lengths 8, 16, 64, 4096: S / len, Q / len and mean^2 are exact in fp64, so
    out = [float(mean) | sqrtf(float(var) + eps)] in every bit."""
    lens = list(pd.BLOCK_EXACT_LENS)
    blocks = [pd.dyadic_blocks(n, C, seed=n + C) for n in lens]
    got = _run_blocks(env, blocks, lens, C)
    for b, (blk, n) in enumerate(zip(blocks, lens)):
        mean, var, _ = pd.blocks_ref(blk, n)
        assert np.array_equal(got[b, :C].view(np.uint32), mean.astype(np.float32).view(np.uint32)), (n, "mean")
        assert np.array_equal(got[b, C:].view(np.uint32), pd.std32(var).view(np.uint32)), (n, "std")


@pytest.mark.parametrize("C", (4, 60, 260))
def test_blocks_elementwise(env, C):
    """Every residue of the block count against the unroll of 4, last blocks of 1 to 8 rows, the hostile channels as blocks.  The
    reference is the header's formula in long double on the same fp32 blocks, its last step sqrtf((float)var + eps) in float32 as
    the header states it: the mean within 1 ulp, the std within 1 ulp + 2^-52 nb (Q / len) / (2 sd) of the fp64 sums."""
    lens = list(pd.BLOCK_LENS)
    rng = np.random.default_rng(C)
    blocks = [pd.blocks_of(pd.chunk(b, n, C, rng)) for b, n in enumerate(lens)]
    got = _run_blocks(env, blocks, lens, C)
    assert np.isfinite(got).all()
    for b, (blk, n) in enumerate(zip(blocks, lens)):
        mean, var, qn = pd.blocks_ref(blk, n)
        sd = pd.std32(var).astype(np.float64)
        r1 = _ratio(np.abs(got[b, :C] - mean), pd.ulp32(mean))
        r2 = _ratio(np.abs(got[b, C:] - sd), pd.ulp32(sd) + 2.0 ** -52 * blk.shape[0] * qn / (2 * sd))
        _note("stats_pool_blocks mean / 1 ulp", r1)
        _note("stats_pool_blocks std / bound", r2)
        assert r1 <= 1 and r2 <= 1, (n, r1, r2)


def test_blocks_more_than_65535_chunks(env):
    """65540 one-block chunks of 1 to 8 rows at C = 4."""
    C, n = 4, 65540
    rng = np.random.default_rng(11)
    lens = (np.arange(n) % 8 + 1).astype(np.int32)
    stats = np.empty((n, 2, C), np.float32)
    stats[:, 0] = rng.standard_normal((n, C)) * 3
    stats[:, 1] = rng.random((n, C)) * 10 * (lens[:, None] > 1)
    out = _out(env, n, 2 * C)
    env["hiplib"].stats_pool_blocks(_dev(env, stats), C, _dev(env, (8 * np.arange(n)).astype(np.int32)), _dev(env, lens), n, EPS, out)
    got = _host(env, out, n)
    m = stats[:, 0].astype(np.float64)
    var = np.maximum((stats[:, 1].astype(np.float64) + lens[:, None] * m * m) / lens[:, None] - m * m, 0)
    sd = pd.std32(var).astype(np.float64)
    assert np.array_equal(got[:, :C], stats[:, 0])                             # n m / n: the mean itself
    bad = np.nonzero(~(np.abs(got[:, C:] - sd) <= pd.ulp32(sd) + 2.0 ** -52 * (var + m * m) / (2 * sd)))[0]
    assert bad.size == 0, (len(bad), bad[:5])


# ---------------------------------------------------------------------------------------------------------------------------
# 3. attention forward
# ---------------------------------------------------------------------------------------------------------------------------
def _scores(env, u_view, v, R, C, with_nl, ldn=None):
    torch, hiplib, dev = env["torch"], env["hiplib"], env["dev"]
    scores = torch.full((R + 1,), float("nan"), dtype=torch.float32, device=dev)
    scores[R] = SENTINEL
    nl = None
    if with_nl:
        parent = torch.full((R + 1, ldn or C), float("nan"), dtype=torch.float32, device=dev)
        nl = parent[:R, :C]
    hiplib.attention_scores(u_view, v, scores[:R], nl, rows=R)
    torch.cuda.synchronize()
    s = scores.cpu().numpy()
    assert s[R] == SENTINEL
    if with_nl:
        ph = parent.cpu().numpy()
        assert np.isnan(ph[R]).all() and np.isnan(ph[:, C:]).all(), "nonlin: wrote outside [R, C]"
        return s[:R], ph[:R, :C]
    return s[:R], None


@pytest.mark.parametrize("C", pd.SCORE_CHANNELS)
def test_attention_scores_elementwise(env, C):
    """Rows 0 ... 20: the designed tanh arguments, rotated so that each one meets every lane position; the other rows: ordinary
    data.  nonlin against fp64 tanh (absolute 5e-7; exactly +-1 for |x| >= 89); scores[r] against the fp64 dot product of v with
    the kernel's own nonlin: ceil(C / 256) 2^-24 sum_c |v_c n_c| (the fma chain of a lane) + 1 ulp (the cast).  u is a column
    slice of a wider buffer (ldu > C), nonlin too; scores have the same bits with and without nonlin."""
    torch, dev = env["torch"], env["dev"]
    rng = np.random.default_rng(C)
    args = pd.TANH_ARGS
    R = len(args) + 14
    u = (1.5 * rng.standard_normal((R, C))).astype(np.float32)
    u[:len(args)] = args[(np.arange(len(args))[:, None] + np.arange(C)[None, :]) % len(args)]
    v = (rng.standard_normal(C) * (2.0 / np.sqrt(C))).astype(np.float32)
    parent = np.full((R, C + 8), np.nan, np.float32)
    parent[:, 4:4 + C] = u
    ud = _dev(env, parent)[:, 4:4 + C]
    vd = _dev(env, v)
    s_nl, nl = _scores(env, ud, vd, R, C, True, ldn=C + 4)
    s_plain, _ = _scores(env, ud, vd, R, C, False)
    s_contig, _ = _scores(env, _dev(env, u), vd, R, C, False)
    assert np.array_equal(s_nl.view(np.uint32), s_plain.view(np.uint32)) and np.array_equal(s_nl.view(np.uint32), s_contig.view(np.uint32))
    t = np.tanh(u.astype(np.float64))
    err = np.abs(nl - t)
    _note("attention_scores nonlin abs error / 5e-7", err.max() / 5e-7)
    assert err.max() <= 5e-7, (err.max(), u[np.unravel_index(np.argmax(err), err.shape)])
    sat = np.abs(u) >= pd.TANH_SATURATED
    assert np.array_equal(nl[sat], np.sign(u[sat]))
    prod = np.abs(v.astype(np.float64)[None, :] * nl.astype(np.float64))
    ref = (v.astype(np.float64)[None, :] * nl.astype(np.float64)).sum(1)
    bound = -(-C // 256) * pd.U * prod.sum(1) + pd.ulp32(ref)
    r = _ratio(np.abs(s_nl - ref), bound)
    _note("attention_scores scores / bound", r)
    assert r <= 1, (C, r)


def test_attention_softmax_elementwise(env):
    """Every chunk of pd.softmax_cases() in one launch: fp64 softmax of the fp32 scores; |a - a_ref| <= (|s - max| + 4) 2^-24 a_ref
    (the subtraction, expf, the sum's cast, the division) + the smallest normal fp32 (a flushed subnormal is allowed); sum(a) within
    4 2^-24 of 1; a lone maximum 100 above the rest in every wave and at both ends of the 256-stride; gap rows untouched."""
    torch, hiplib, dev = env["torch"], env["hiplib"], env["dev"]
    cases = pd.softmax_cases()
    lens = [c[0] for c in cases]
    rs, rows = pd.layout(lens)
    rng = np.random.default_rng(17)
    s = np.full(rows, np.nan, np.float32)
    for (n, spread, peak), r0 in zip(cases, rs):
        s[r0:r0 + n] = pd.softmax_scores(n, spread, peak, rng)
    att = torch.full((rows,), float("nan"), dtype=torch.float32, device=dev)
    hiplib.attention_softmax(_dev(env, s), _dev(env, rs), _dev(env, np.asarray(lens, np.int32)), len(lens), att)
    torch.cuda.synchronize()
    a = att.cpu().numpy()
    owned = np.zeros(rows, bool)
    fails = []
    for (n, spread, peak), r0 in zip(cases, rs):
        owned[r0:r0 + n] = True
        got = a[r0:r0 + n]
        ref, absd = pd.softmax_ref(s[r0:r0 + n])
        assert np.isfinite(got).all() and (got >= 0).all(), (n, spread, peak)
        r = _ratio(np.abs(got - ref), pd.softmax_bound(ref, absd))
        dsum = abs(got.astype(np.float64).sum() - 1.0) / (4 * pd.U)
        _note("attention_softmax a / bound", r)
        _note("attention_softmax |sum a - 1| / (4 2^-24)", dsum)
        if r > 1 or dsum > 1:
            fails.append((n, spread, peak, r, dsum))
        if peak is not None:
            assert got[peak] == 1.0 and int(np.argmax(got)) == peak
    assert not fails, fails[:8]
    assert np.isnan(a[~owned]).all()


def attention_pool(env, h, C, att, rs, rl, split, max_len=None):
    torch, lib, dev = env["torch"], env["lib"], env["dev"]
    n = len(rl)
    max_len = int(max(rl)) if max_len is None else max_len
    need = int(lib.xv_attention_pool_workspace_bytes(C, n, max_len, split))
    assert (need > 0) == (max_len > split)
    rsd, rld = _dev(env, np.asarray(rs, np.int32)), _dev(env, np.asarray(rl, np.int32))
    res = []
    for _ in range(2):
        ws = torch.full((max(need // 8, 1),), float("nan"), dtype=torch.float64, device=dev)
        out = _out(env, n, 2 * C)
        rc = lib.xv_attention_pool_f32(_p(h), h.stride(0), C, _p(att), _p(rsd), _p(rld), n, max_len, split, EPS, _p(out), _p(ws), None)
        assert rc == 0, rc
        res.append(_host(env, out, n))
    assert np.array_equal(res[0].view(np.uint32), res[1].view(np.uint32)), "a second run gives other bits"
    return res[0]


@pytest.mark.parametrize("split", (512, 128, 32))
def test_attention_pool_exact_on_dyadic_weights(env, split):
    """Weights 2^-k that sum to 1, integer h: s1, s2 and q = s2 - s1^2 are exact in fp64, out = [float(m) | sqrtf(float(q) + eps)]."""
    C = 68
    lens = [1, 2, 7, 33, 100, 513, 1024] if split < 512 else [1, 2, 7, 33, 100, 512]
    rs, rows = pd.layout(lens)
    host = np.full((rows, C), np.nan, np.float32)
    a = np.full(rows, np.nan, np.float32)
    mats = [pd.integer_chunk(n, C, seed=n + split) for n in lens]
    wts = [pd.dyadic_weights(n, seed=n + split) for n in lens]
    for s, m, w in zip(rs, mats, wts):
        host[s:s + len(m)] = m
        a[s:s + len(m)] = w
    got = attention_pool(env, _dev(env, host), C, _dev(env, a), rs, lens, split)
    for b, (m, w) in enumerate(zip(mats, wts)):
        mean, sd = pd.attention_pool_exact(m, w)
        assert np.array_equal(got[b, :C].view(np.uint32), mean.view(np.uint32)), (len(m), "mean")
        assert np.array_equal(got[b, C:].view(np.uint32), sd.view(np.uint32)), (len(m), "std")


def _weights(env, kind, lens, rs, rows, seed):
    """fp32 weights per row (NaN in the gaps): the kernel's own softmax of random scores, or random positive numbers that do not
    sum to 1, or those normalised in fp32 and scaled by 1 +- 1e-7 (alternating by chunk)."""
    rng = np.random.default_rng(seed)
    a = np.full(rows, np.nan, np.float32)
    for b, (s, n) in enumerate(zip(rs, lens)):
        if kind == "softmax":
            a[s:s + n] = (3 * rng.standard_normal(n)).astype(np.float32)
        else:
            w = rng.random(n).astype(np.float32) + np.float32(1e-3)
            if kind == "unit":
                w = (w / w.sum(dtype=np.float64) * (1 + (1e-7 if b & 1 else -1e-7))).astype(np.float32)
            a[s:s + n] = w
    if kind != "softmax":
        return _dev(env, a)
    torch = env["torch"]
    att = torch.full((rows,), float("nan"), dtype=torch.float32, device=env["dev"])
    env["hiplib"].attention_softmax(_dev(env, a), _dev(env, rs), _dev(env, np.asarray(lens, np.int32)), len(lens), att)
    return att


def _check_attention_pool(env, name, view, C, rs, lens, mats, att, split):
    """out = [m | sqrt(max(q, 0) + eps)] against the long-double formula on the same fp32 h and att: the mean within 1 ulp, the std
    within 2 ulp, each plus what the fp64 sums carry (pool_data.attention_pool_bounds).  A constant channel follows the formula,
    clamp included: with weights that sum to 1 + 1e-7 its q is negative, with 1 - 1e-7 it is c^2 1e-7, not 0."""
    got = attention_pool(env, view, C, att, rs, lens, split)
    assert np.isfinite(got).all()
    a = att.cpu().numpy()
    fails = []
    for b, (m, s) in enumerate(zip(mats, rs)):
        mean, sd, e_mean, e_sd = pd.attention_pool_bounds(m, a[s:s + len(m)])
        r1, r2 = _ratio(np.abs(got[b, :C] - mean), e_mean), _ratio(np.abs(got[b, C:] - sd), e_sd)
        _note("attention_pool mean / bound", r1)
        _note("attention_pool std / bound", r2)
        if r1 > 1 or r2 > 1:
            fails.append((b, len(m), r1, r2))
    assert not fails, (name, fails[:8])


# random weights at every channel count; the kernel's own softmax and unit-sum weights at the smallest and the largest
APOOL_CASES = [(m, k, C) for m in pd.MODES for k in ("random", "softmax", "unit") for C in pd.CHANNELS if k == "random" or C in (4, 260)]


@pytest.mark.parametrize("mode,kind,C", APOOL_CASES, ids=["%s-%s-%d" % (m[0], k, C) for m, k, C in APOOL_CASES])
def test_attention_pool_elementwise(env, mode, kind, C):
    name, lens, split = mode
    host, rs, mats = pd.batch(lens, C, seed=C * 5 + split + len(lens))
    att = _weights(env, kind, lens, rs, len(host), seed=C + split)
    _check_attention_pool(env, "%s %s C %d" % (name, kind, C), _dev(env, host), C, rs, lens, mats, att, split)


def test_attention_pool_on_a_column_slice(env):
    lens, split = pd.LENS, 128
    C, ld, col0 = 68, 136, 68
    host, rs, mats = pd.batch(lens, C, seed=3, ld=ld, col0=col0)
    att = _weights(env, "softmax", lens, rs, len(host), seed=4)
    _check_attention_pool(env, "slice", _dev(env, host)[:, col0:col0 + C], C, rs, lens, mats, att, split)


@pytest.mark.parametrize("split", (512, 2), ids=("direct", "split2"))
def test_attention_pool_more_than_65535_chunks(env, split):
    C, n = 4, 65540
    x, rs, rl = pd.many_chunks(n, C, seed=split + 1)
    a = (np.random.default_rng(split).random(len(x)) + 0.01).astype(np.float32)
    h, att = _dev(env, x), _dev(env, a)
    got = attention_pool(env, h, C, att, rs, rl, split)
    assert np.isfinite(got).all()
    for (idx, rows), (_, wts) in zip(pd.by_length(x, rs, rl), pd.by_length(a, rs, rl)):
        mean, sd, e_mean, e_sd = pd.attention_pool_bounds(rows, wts)
        r1, r2 = _ratio(np.abs(got[idx, :C] - mean), e_mean), _ratio(np.abs(got[idx, C:] - sd), e_sd)
        _note("attention_pool 65540 chunks mean / bound", r1)
        _note("attention_pool 65540 chunks std / bound", r2)
        assert r1 <= 1 and r2 <= 1, (len(rows[0]), r1, r2)
    lo = pd.GRID_Z - 1
    small = attention_pool(env, h, C, att, rs[lo:], rl[lo:], split, max_len=3)
    assert np.array_equal(small.view(np.uint32), got[lo:].view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------------
# 4. xv_chunk_average_f32
# ---------------------------------------------------------------------------------------------------------------------------
def _chunk_average(env, e, seg, lens, dim):
    nutt = len(seg) - 1
    out = _out(env, nutt, dim)
    env["hiplib"].chunk_average(_dev(env, e), _dev(env, seg), _dev(env, lens), nutt, out)
    return _host(env, out, nutt)


@pytest.mark.parametrize("dim", pd.AVG_DIMS)
def test_chunk_average_bit_exact_at_odd_widths(env, dim):
    rng = np.random.default_rng(dim)
    cnt = np.array([1, 3, 1, 1, 4, 2, 1], np.int32)                  # utterances of a single chunk among the others
    seg = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    lens = rng.integers(25, 10001, size=seg[-1]).astype(np.int32)
    e = (5 * rng.standard_normal((seg[-1], dim))).astype(np.float32)
    got = _chunk_average(env, e, seg, lens, dim)
    for u in range(len(cnt)):
        ref = pd.chunk_average_ref(e[seg[u]:seg[u + 1]], lens[seg[u]:seg[u + 1]])
        assert np.array_equal(got[u].view(np.uint32), ref.view(np.uint32)), u


def test_chunk_average_more_than_65535_utterances(env):
    n, dim = 65540, 4
    rng = np.random.default_rng(2)
    cnt = (np.arange(n) % 3 + 1).astype(np.int32)
    seg = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    lens = rng.integers(25, 10001, size=seg[-1]).astype(np.int32)
    e = (5 * rng.standard_normal((seg[-1], dim))).astype(np.float32)
    got = _chunk_average(env, e, seg, lens, dim)
    ref = pd.chunk_average_ref_batched(e, seg, lens)
    bad = np.nonzero((got.view(np.uint32) != ref.view(np.uint32)).any(1))[0]
    assert bad.size == 0, (len(bad), bad[:5])
    for u in (0, 1, 2, pd.GRID_Z - 1, pd.GRID_Z, n - 1):            # and the loop form itself around the slice boundary
        assert pd.bits_equal(got[u], pd.chunk_average_ref(e[seg[u]:seg[u + 1]], lens[seg[u]:seg[u + 1]])), u


# ---------------------------------------------------------------------------------------------------------------------------
# 5. contracts
# ---------------------------------------------------------------------------------------------------------------------------
def test_ldh_below_c_is_refused(env):
    torch, lib, dev = env["torch"], env["lib"], env["dev"]
    C = 8
    h = torch.zeros((16, C), dtype=torch.float32, device=dev)
    rs, rl = _dev(env, np.array([0], np.int32)), _dev(env, np.array([4], np.int32))
    out = _out(env, 1, 2 * C)
    assert lib.xv_stats_pool_f32(_p(h), C - 4, C, _p(rs), _p(rl), 1, 4, 512, EPS, _p(out), None, None) == BAD_ARG
    assert lib.xv_chunk_moments_f32(_p(h), C - 4, C, _p(rs), _p(rl), 1, 4, 512, _p(out), None, None) == BAD_ARG
    assert lib.xv_stats_pool_f32(_p(h), 0, C, _p(rs), _p(rl), 1, 4, 512, EPS, _p(out), None, None) == BAD_ARG
    assert np.isnan(_host(env, out, 1)).all()                        # nothing was launched
    assert lib.xv_stats_pool_f32(_p(h), C, C, _p(rs), _p(rl), 1, 4, 512, EPS, _p(out), None, None) == 0
    assert np.isfinite(_host(env, out, 1)).all()


@pytest.mark.parametrize("split", (512, 32), ids=("direct", "split"))
def test_an_empty_chunk_gives_nan_and_leaves_its_neighbours_alone(env, split):
    """row_len <= 0: the chunk's row of out is NaN (as xv_stats_pool_blocks_f32 writes it), in the direct kernels and in the merge
    kernels; the other chunks have the bits they have without it."""
    C = 68
    lens = [40, 0, 7, -3, 100]
    keep = [0, 2, 4]
    real = [n for n in lens if n > 0]
    host, rs_real, mats = pd.batch(real, C, seed=split)
    rs = np.zeros(len(lens), np.int32)
    rs[keep] = rs_real
    rs[1], rs[3] = rs_real[1], 0
    h = _dev(env, host)
    att = _weights(env, "random", real, rs_real, len(host), seed=1)
    for raw in (0, 1):
        full = stats_pool(env, h, C, rs, lens, split, raw=raw)
        alone = stats_pool(env, h, C, rs_real, real, split, raw=raw)
        assert np.isnan(full[[1, 3]]).all()
        assert np.array_equal(full[keep].view(np.uint32), alone.view(np.uint32)) and np.isfinite(alone).all()
    full = attention_pool(env, h, C, att, rs, lens, split)
    alone = attention_pool(env, h, C, att, rs_real, real, split)
    assert np.isnan(full[[1, 3]]).all()
    assert np.array_equal(full[keep].view(np.uint32), alone.view(np.uint32)) and np.isfinite(alone).all()
