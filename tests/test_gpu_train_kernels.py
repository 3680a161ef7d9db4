"""GPU unit tests of the training-step kernels (csrc/xv_train.hip, xv_chunk_moments_f32 of xv_pool.hip, xv_fold_bn_f32 of xv_kernels.hip), one hiplib
wrapper at a time, each against a float64 statement of the same operation written here from its TF definition (numpy, or torch-CPU
float64 autograd for the backward ops).  No test compares one kernel with another and none uses oracle/train_ref.py.

Every output buffer is NaN-poisoned before the call (the in-place kernels -- prelu_backward, adam, ema, axpy, am_margin -- change
every element they own, so a skipped one shows up as the old value), and the shapes are chosen from the launch configurations in
xv_train.hip so that every loop and tail runs: the 64-lane class loop of softmax_ce over thousands of classes, the grid-stride loops
past one grid (am_margin: 4096 x 256 elements, prelu_backward: 65536 x 256), the unaligned scalar path of sumsq_partial_kernel, the
128-row splits and the 16-group ordered merges of the column sums, the 512-row split of the chunk moments."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RELU, LRELU = 1, 2
BN_EPS = 1e-3              # batch_norm_wrapper(epsilon=1e-3), tf_block.py
POOL_EPS = 1e-5            # VAR2STD_EPSILON, models.py:16 -- [mean, sqrt(var + 1e-5)], models.py:75-76
NAN = float("nan")
CM_BAR = 1e-4              # per-chunk variance: stats_pool_kernel (xv_pool.hip) merges 8-row blocks in fp32 (measured: up to 4.1e-5)


def _note(what, err):
    """Worst error of a quantity against its bar, printed (pytest -s) for the record."""
    print("worst %-40s %.3e" % (what, float(np.max(err))))


@pytest.fixture(scope="module")
def env():
    import torch
    from xvector_amd import engine, hiplib
    hiplib.require_gpu()
    return dict(torch=torch, hiplib=hiplib, engine=engine, dev=torch.device("cuda:0"))


def _dev(env, a):
    return env["torch"].from_numpy(np.ascontiguousarray(a)).to(env["dev"])


def _nan(env, *shape):
    return env["torch"].full(shape, NAN, dtype=env["torch"].float32, device=env["dev"])


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _ulp(a):
    """fp32 ulp of |a| (a float64 array): the spacing at the fp32 value nearest to it."""
    return np.spacing(np.abs(np.asarray(a, np.float64)).astype(np.float32)).astype(np.float64)


def _col_rel(got, ref):
    """Per-column relative L2 error (a column whose reference is all zero must be all zero)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    num = np.sqrt(((got - ref) ** 2).sum(axis=0))
    den = np.sqrt((ref ** 2).sum(axis=0))
    return np.where(den > 0, num / np.where(den > 0, den, 1.0), np.where(num > 0, np.inf, 0.0))


# ------------------------------------------------------------------------------------------------
# softmax cross-entropy: loss = mean_b [logsumexp(z_b) - z_b[label_b]], accuracy = mean_b [argmax z_b == label_b] (first maximum,
# as tf.argmax), dlogits = (softmax(z_b) - onehot(label_b)) / B
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 64, 257])
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 1000, 7323])
def test_softmax_ce_matches_float64(env, N, B):
    torch, hiplib = env["torch"], env["hiplib"]
    rng = np.random.default_rng(N * 1000 + B)
    z = np.clip(rng.standard_normal((B, N)) * 30.0, -80.0, 80.0).astype(np.float32)
    z[np.arange(B), rng.integers(0, N, B)] = 80.0                         # every row reaches +80 somewhere
    z[np.arange(B), rng.integers(0, N, B)] = -80.0
    lab = rng.integers(0, N, B).astype(np.int32)
    lab[0] = N - 1
    z[0] = 7.0                                                            # a row of identical logits: the first maximum is class 0
    if B > 1:
        lab[1] = 0
        z[1] = 7.0
    if B > 2:
        z[2] = -z[2]
        lab[2] = 0
    zd = z.astype(np.float64)
    mx = zd.max(axis=1, keepdims=True)
    lse = np.log(np.exp(zd - mx).sum(axis=1)) + mx[:, 0]
    loss_ref = float((lse - zd[np.arange(B), lab]).mean())
    acc_ref = np.float32(float((np.argmax(z, axis=1) == lab).sum()) / B)
    p = np.exp(zd - lse[:, None])
    p[np.arange(B), lab] -= 1.0
    dref = p / B

    logits, labels = _dev(env, z), _dev(env, lab)
    la, dl = _nan(env, 2), _nan(env, B, N)
    hiplib.softmax_ce(logits, labels, la, dl)
    la2 = _nan(env, 2)
    hiplib.softmax_ce(logits, labels, la2, None)
    la_h, dl_h, la2_h = _host(la), _host(dl), _host(la2)

    assert la_h[1] == acc_ref, (la_h[1], acc_ref)
    assert abs(float(la_h[0]) - loss_ref) <= 4 * _ulp(loss_ref) + 1e-30, (la_h[0], loss_ref)
    assert la_h.view(np.uint32).tolist() == la2_h.view(np.uint32).tolist()          # dlogits=None: the same loss bits
    assert np.isfinite(dl_h).all()
    err = np.abs(dl_h.astype(np.float64) - dref)
    _note("softmax_ce dlogits / ulp", err / np.maximum(_ulp(dref), 1e-45))
    _note("softmax_ce loss / ulp", abs(float(la_h[0]) - loss_ref) / _ulp(loss_ref))
    assert (err <= 2 * _ulp(dref) + 1e-37).all(), (float((err / np.maximum(_ulp(dref), 1e-45)).max()))
    assert (np.abs(dl_h.astype(np.float64).sum(axis=1)) <= 1e-5 / B).all()          # each row of softmax - onehot sums to 0


# ------------------------------------------------------------------------------------------------
# additive margin: z[b, j] = s * (cos[b, j] - m [j == label_b]), in place
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,scale", [(1, 1, 32.0), (3, 65, 30.0), (64, 7323, 32.0), (143, 7323, 30.0), (257, 7323, 32.0)])
def test_am_margin_matches_float64(env, B, N, scale):
    hiplib = env["hiplib"]
    margin = np.float32(0.2)
    rng = np.random.default_rng(B + N)
    cos = rng.uniform(-1, 1, (B, N)).astype(np.float32)
    lab = rng.integers(0, N, B).astype(np.int32)
    lab[0] = N - 1
    cos[0, N - 1] = margin                                      # cos == m at the label: exactly 0
    ref = cos.astype(np.float64)
    ref[np.arange(B), lab] -= float(margin)
    ref *= scale
    zt = _dev(env, cos)
    hiplib.am_margin(zt, _dev(env, lab), scale, float(margin))
    got = _host(zt).astype(np.float64)
    # s = 32 is exact, so one rounding of (cos - m): <= 1 ulp;  s = 30 adds the product's rounding: <= 1.5 ulp
    bar = 1.0 if scale == 32.0 else 1.5
    err = np.abs(got - ref)
    _note("am_margin s=%g / ulp" % scale, err / np.maximum(_ulp(ref), 1e-45))
    assert (err <= bar * _ulp(ref)).all(), float((err / np.maximum(_ulp(ref), 1e-45)).max())
    assert got[0, N - 1] == 0.0


# ------------------------------------------------------------------------------------------------
# L2 normalisation of rows, y = x / max(||x||, 1e-12) (F.normalize's definition), and its gradient:
#   ||x|| >= 1e-12:  dx = (dy - y <y, dy>) / ||x||        ||x|| < 1e-12:  dx = dy / 1e-12  (y is linear in x there)
# ------------------------------------------------------------------------------------------------
def _l2_rows(rng, C):
    x = rng.standard_normal((9, C))
    x[0] = 0.0                                      # all-zero row
    x[1] *= 1e-20                                   # far below the clamp (the squares underflow fp32, not fp64)
    x[2] *= 1e18                                    # squares far above fp32's range
    x[3] *= 0.5e-12 / np.linalg.norm(x[3])          # just below the clamp: ||x|| = 0.5e-12, y ~ 0.5 (the projection term matters)
    x[4] *= 4e-12 / np.linalg.norm(x[4])            # just above it
    x[5, :] = 0.0
    x[5, C - 1] = -3.0                              # a single non-zero entry, in the last lane's tail
    return x.astype(np.float32)


@pytest.mark.parametrize("C", [1, 63, 64, 65, 512, 1500])
def test_l2_normalize_rows_and_backward_match_float64(env, C):
    hiplib = env["hiplib"]
    rng = np.random.default_rng(C)
    x = _l2_rows(rng, C)
    xd = x.astype(np.float64)
    nref = np.sqrt((xd * xd).sum(axis=1))
    yref = xd / np.maximum(nref, 1e-12)[:, None]
    y, nrm = _nan(env, 9, C), _nan(env, 9)
    hiplib.l2_normalize_rows(_dev(env, x), y, nrm)
    y_h, n_h = _host(y).astype(np.float64), _host(nrm).astype(np.float64)
    assert np.isfinite(y_h).all() and np.isfinite(n_h).all()
    assert (np.abs(n_h - nref) <= _ulp(nref)).all(), (n_h, nref)
    row_ulp = _ulp(np.abs(yref).max(axis=1))[:, None]
    _note("l2_normalize y / row ulp", np.abs(y_h - yref) / np.maximum(row_ulp, 1e-45))
    assert (np.abs(y_h - yref) <= 4 * row_ulp).all(), float((np.abs(y_h - yref) / np.maximum(row_ulp, 1e-45)).max())
    assert (y_h[0] == 0).all() and n_h[0] == 0.0

    # backward, from the exact fp32 roundings of y and ||x|| (what the forward leaves), against the derivative at x
    dy = rng.standard_normal((9, C)).astype(np.float32)
    dy[0] = 0.0                                     # (with dy = 0 the zero row's gradient is exactly 0 as well)
    y32, n32 = yref.astype(np.float32), nref.astype(np.float32)
    dyd = dy.astype(np.float64)
    dot = (dyd * yref).sum(axis=1, keepdims=True)
    above = (nref >= 1e-12)[:, None]
    dxref = np.where(above, (dyd - yref * dot) / np.maximum(nref, 1e-12)[:, None], dyd / 1e-12)
    dx = _nan(env, 9, C)
    hiplib.l2_normalize_backward(_dev(env, dy), _dev(env, y32), _dev(env, n32), dx)
    dx_h = _host(dx).astype(np.float64)
    assert np.isfinite(dx_h).all()
    assert (dx_h[0] == 0).all()
    # the inputs are rounded to fp32 (y relative 2^-24 per entry): per row a few ulps of the row's largest |dy| / ||x||
    scale = np.abs(dyd).max(axis=1) / np.maximum(nref, 1e-12)
    row_ulp = _ulp(scale)[:, None]
    _note("l2_normalize_backward / row ulp", np.abs(dx_h - dxref) / np.maximum(row_ulp, 1e-45))
    assert (np.abs(dx_h - dxref) <= 4 * row_ulp).all(), float((np.abs(dx_h - dxref) / np.maximum(row_ulp, 1e-45)).max())


# ------------------------------------------------------------------------------------------------
# PReLU backward of r = max(z, 0) + alpha min(z, 0): dz = dr (z > 0) or alpha dr (z <= 0), dalpha terms dr min(z, 0).
# z == 0 takes the alpha side, as oracle/train_ref.py's relu(z) + alpha clamp(z, max=0) does under autograd (relu' (0) = 0,
# clamp' = 1 at the bound).  Bit-exact: one fp32 product per output either way.
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,C", [(1, 1), (5, 65), (37, 100), (32769, 513)])       # the last one: 16.8 M > 65536 x 256 elements
def test_prelu_backward_is_exact(env, R, C):
    hiplib = env["hiplib"]
    rng = np.random.default_rng(R * C)
    z = rng.standard_normal((R, C)).astype(np.float32)
    z[rng.random((R, C)) < 0.1] = 0.0
    z[0, 0] = 0.0
    g = rng.standard_normal((R, C)).astype(np.float32)
    alpha = (0.25 + 0.1 * rng.standard_normal(C)).astype(np.float32)
    dz_ref = np.where(z > 0, g, alpha[None, :] * g)
    da_ref = g * np.minimum(z, np.float32(0))
    drt, zt = _dev(env, g), _dev(env, z)
    hiplib.prelu_backward(drt, zt, _dev(env, alpha))
    assert np.array_equal(_host(drt), dz_ref)
    assert np.array_equal(_host(zt), da_ref)


# ------------------------------------------------------------------------------------------------
# Adam (tf.train.AdamOptimizer._apply_dense), restated in numpy float32 in the kernel's operation order (fp contract off):
#   m = m b1 + g (1 - b1);  v = v b2 + g g (1 - b2);  p = p - lr_t m / (sqrt(v) + eps)
# ------------------------------------------------------------------------------------------------
def _flat_size():
    """The trainer's flat parameter vector for the recipe's default model at 7323 targets, 30 features (trainer.py: every tensor padded
    to a multiple of 64 elements)."""
    from xvector_amd import topology
    topo = topology.get("ModelWithoutDropout")
    sizes, prev = [], 30
    for k, c in zip(topo["kernel_sizes"], topo["layer_sizes"]):
        sizes += [k * prev * c, c, c, c]
        prev = c
    prev *= 2
    for c in topo["embedding_sizes"]:
        sizes += [prev * c, c, c, c]
        prev = c
    sizes += [prev * 7323, 7323]
    return int(sum((s + 63) // 64 * 64 for s in sizes))


FLAT = _flat_size()


@pytest.mark.parametrize("n", [1, 255, 257, FLAT])
def test_adam_three_steps_bit_exact(env, n):
    hiplib = env["hiplib"]
    f = np.float32
    b1, b2, eps = f(0.9), f(0.999), f(1e-8)
    rng = np.random.default_rng(n)
    p = rng.standard_normal(n).astype(f)
    m, v = np.zeros(n, f), np.zeros(n, f)
    pt, mt, vt = _dev(env, p), _dev(env, m), _dev(env, v)
    for t in range(1, 4):
        g = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 2, n)).astype(f)
        g[::7] = 0.0                                            # g = 0 (with v = 0 on the first step)
        lr_t = f(1e-3 * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t))
        m = m * b1 + g * (f(1) - b1)
        v = v * b2 + g * g * (f(1) - b2)
        p = p - lr_t * m / (np.sqrt(v) + eps)
        hiplib.adam(pt, _dev(env, g), mt, vt, float(lr_t), 0.9, 0.999, 1e-8)
        for name, got, ref in (("m", mt, m), ("v", vt, v), ("p", pt, p)):
            got = _host(got)
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (t, name, int((got != ref).sum()))


# ------------------------------------------------------------------------------------------------
# EMA of the BN statistics (moving = decay moving + (1 - decay) batch) and axpy (y = y + a x), in ulps of the terms' magnitude
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 257, FLAT])
def test_ema_and_axpy_match_float64(env, n):
    hiplib = env["hiplib"]
    rng = np.random.default_rng(n + 1)
    a = (rng.standard_normal(n) * 3).astype(np.float32)
    b = (rng.standard_normal(n) * 3).astype(np.float32)
    decay = np.float32(0.95)
    ref = float(decay) * a.astype(np.float64) + (1.0 - float(decay)) * b.astype(np.float64)
    mag = np.abs(float(decay) * a.astype(np.float64)) + np.abs((1.0 - float(decay)) * b.astype(np.float64))
    at = _dev(env, a)
    hiplib.ema(at, _dev(env, b), float(decay))
    got = _host(at).astype(np.float64)
    # two products and a sum, each rounded once (no contraction in this kernel): <= 1.5 ulp of the terms' magnitude
    _note("ema error / ulp(|terms|)", np.abs(got - ref) / _ulp(mag))
    assert (np.abs(got - ref) <= 1.5 * _ulp(mag)).all()

    coef = np.float32(-0.37)
    ref = a.astype(np.float64) + float(coef) * b.astype(np.float64)
    mag = np.abs(a.astype(np.float64)) + np.abs(float(coef) * b.astype(np.float64))
    yt = _dev(env, a)
    hiplib.axpy(yt, _dev(env, b), float(coef))
    got = _host(yt).astype(np.float64)
    _note("axpy error / ulp(|terms|)", np.abs(got - ref) / _ulp(mag))
    assert (np.abs(got - ref) <= _ulp(mag)).all()


# ------------------------------------------------------------------------------------------------
# sum of squares (the L2 regulariser / gradient norms): fp64 sum, one rounding
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 5, 8191, 8193, 256 * 8192 + 7])
@pytest.mark.parametrize("offset", [0, 1])          # offset 1: x[1:], 4-byte aligned only -> the scalar path over everything
def test_sumsq_matches_float64(env, n, offset):
    hiplib = env["hiplib"]
    rng = np.random.default_rng(n)
    x = (rng.standard_normal(n + offset) * 10.0 ** rng.integers(-3, 3, n + offset)).astype(np.float32)
    ref = float((x[offset:].astype(np.float64) ** 2).sum())
    xt = _dev(env, x)[offset:]
    assert xt.is_contiguous()
    o1, o2 = _nan(env, 1), _nan(env, 1)
    hiplib.sumsq(xt, o1)
    hiplib.sumsq(xt, o2)
    g1, g2 = _host(o1), _host(o2)
    assert g1.view(np.uint32)[0] == g2.view(np.uint32)[0]
    _note("sumsq / ulp", abs(float(g1[0]) - ref) / _ulp(ref))
    assert abs(float(g1[0]) - ref) <= _ulp(ref), (float(g1[0]), ref)


# ------------------------------------------------------------------------------------------------
# batch normalisation in training mode over the VALID rows of a ragged layout (tf.nn.moments over all frames, biased variance)
# ------------------------------------------------------------------------------------------------
LAYOUTS = {
    "ragged": [37, 1, 700, 2, 129, 513, 300, 64],       # a chunk of one frame, chunks across the 512-row moment split
    "production": [300] * 64,                          # one minibatch of the recipe: R ~ 64 x 300, far above 16 x 128 rows
}


def _bn_case(env, layout, C, seed):
    rng = np.random.default_rng(seed)
    lay = env["engine"].BatchLayout(LAYOUTS[layout], 3)
    valid = lay.row_valid().astype(bool)
    R = lay.rows
    r = (rng.standard_normal((R, C)) * rng.uniform(0.5, 3.0, C) + rng.uniform(-2, 2, C)).astype(np.float32)
    r[:, C // 3] = (200.0 + 0.1 * rng.standard_normal(R)).astype(np.float32)          # mean 200, variance 1e-2
    r[~valid] = 0.0
    gamma = (1.0 + 0.2 * rng.standard_normal(C)).astype(np.float32)
    beta = (0.1 * rng.standard_normal(C)).astype(np.float32)
    return lay, valid, r, gamma, beta


def _moments(r, valid):
    v = r[valid].astype(np.float64)
    m = v.mean(axis=0)
    return m, ((v - m) ** 2).mean(axis=0)


def _sums_workspace(a, b, valid):
    """The [splits][2][C] float64 partial column sums a producer leaves per 128-row tile: [sum a | sum a*b] over the valid rows."""
    R, C = a.shape
    ns = (R + 127) // 128
    ws = np.zeros((ns, 2, C), np.float64)
    ad = np.where(valid[:, None], a.astype(np.float64), 0.0)
    bd = b.astype(np.float64)
    for j in range(ns):
        ws[j, 0] = ad[j * 128:(j + 1) * 128].sum(axis=0)
        ws[j, 1] = (ad[j * 128:(j + 1) * 128] * bd[j * 128:(j + 1) * 128]).sum(axis=0)
    return ws


@pytest.mark.parametrize("C", [24, 512, 1536])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_bn_train_forward_kernels_match_float64(env, layout, C):
    torch, hiplib = env["torch"], env["hiplib"]
    lay, valid, r, gamma, beta = _bn_case(env, layout, C, seed=C + len(layout))
    R, B = lay.rows, lay.nchunks
    rs, rl, vt = _dev(env, lay.row_start), _dev(env, lay.row_len), _dev(env, valid.astype(np.uint8))
    rt = _dev(env, r)
    # chunk moments: per chunk [mean || biased variance]
    cm = _nan(env, B, 2 * C)
    hiplib.chunk_moments(rt, rs, rl, B, lay.max_len, cm)
    cm_h = _host(cm).astype(np.float64)
    for b, (s, n) in enumerate(zip(lay.row_start, lay.row_len)):
        blk = r[s:s + n].astype(np.float64)
        m, v = blk.mean(axis=0), blk.var(axis=0)
        rms = np.sqrt(m * m + v)
        _note("chunk_moments mean / rms", np.abs(cm_h[b, :C] - m) / rms)
        _note("chunk_moments var rel", np.abs(cm_h[b, C:] - v) / np.maximum(v, 1e-30))
        assert (np.abs(cm_h[b, :C] - m) <= 1e-6 * rms).all(), (b, float((np.abs(cm_h[b, :C] - m) / rms).max()))
        assert (np.abs(cm_h[b, C:] - v) <= CM_BAR * v).all(), (b, float((np.abs(cm_h[b, C:] - v) / np.maximum(v, 1e-30)).max()))
    # merged over the batch, from fp32 chunk moments (any: here the exact ones rounded)
    mref, vref = _moments(r, valid)
    cm32 = np.zeros((B, 2 * C), np.float32)
    for b, (s, n) in enumerate(zip(lay.row_start, lay.row_len)):
        blk = r[s:s + n].astype(np.float64)
        cm32[b, :C], cm32[b, C:] = blk.mean(axis=0), blk.var(axis=0)
    mean, var = _nan(env, C), _nan(env, C)
    hiplib.merge_moments(_dev(env, cm32), rl, B, mean, var)
    m_h, v_h = _host(mean).astype(np.float64), _host(var).astype(np.float64)
    n_b = lay.row_len.astype(np.float64)[:, None]
    cmd = cm32.astype(np.float64)
    mu = (n_b * cmd[:, :C]).sum(axis=0) / n_b.sum()                  # the merge of exactly these fp32 chunk moments
    vm = (n_b * (cmd[:, C:] + (cmd[:, :C] - mu) ** 2)).sum(axis=0) / n_b.sum()
    rms = np.sqrt(mu * mu + vm)
    _note("merge_moments mean / rms", np.abs(m_h - mu) / rms)
    _note("merge_moments var rel", np.abs(v_h - vm) / vm)
    assert (np.abs(m_h - mu) <= 1e-6 * rms).all(), float((np.abs(m_h - mu) / rms).max())
    assert (np.abs(v_h - vm) <= 1e-6 * vm).all(), float((np.abs(v_h - vm) / vm).max())
    rms = np.sqrt(mref * mref + vref)
    # fold: scale = gamma / sqrt(var + eps), shift = beta - mean * scale (from the fp32 moments the kernels hand over)
    m32, v32 = mref.astype(np.float32), vref.astype(np.float32)
    scale, shift = hiplib.fold_bn(_dev(env, gamma), _dev(env, beta), _dev(env, m32), _dev(env, v32), BN_EPS)
    sc_ref = gamma.astype(np.float64) / np.sqrt(v32.astype(np.float64) + BN_EPS)
    sh_ref = beta.astype(np.float64) - m32.astype(np.float64) * sc_ref
    sc_h, sh_h = _host(scale).astype(np.float64), _host(shift).astype(np.float64)
    assert (np.abs(sc_h - sc_ref) <= 3 * _ulp(sc_ref)).all()
    assert (np.abs(sh_h - sh_ref) <= 3 * _ulp(np.abs(beta) + np.abs(m32 * sc_ref))).all()
    # rows: y = valid ? r * scale + shift : 0
    sc32, sh32 = sc_ref.astype(np.float32), sh_ref.astype(np.float32)
    y = _nan(env, R, C)
    hiplib.rows_affine(rt, _dev(env, sc32), _dev(env, sh32), vt, y)
    y_h = _host(y).astype(np.float64)
    yref = r.astype(np.float64) * sc32 + sh32.astype(np.float64)
    mag = np.abs(r.astype(np.float64) * sc32) + np.abs(sh32.astype(np.float64))
    assert (np.abs(y_h[valid] - yref[valid]) <= _ulp(mag[valid])).all()
    assert (y_h[~valid] == 0).all()
    # the one-launch moments + fold from a producer's partial sums [sum y | sum y^2] per 128-row tile
    ws = _dev(env, _sums_workspace(r, r, valid))
    mean, var = _nan(env, C), _nan(env, C)
    scale2, shift2 = hiplib.bn_moments_fold(ws, R, float(valid.sum()), _dev(env, gamma), _dev(env, beta), BN_EPS, mean, var)
    m_h, v_h = _host(mean).astype(np.float64), _host(var).astype(np.float64)
    _note("bn_moments_fold mean / rms", np.abs(m_h - mref) / rms)
    _note("bn_moments_fold var rel", np.abs(v_h - vref) / vref)
    assert (np.abs(m_h - mref) <= 1e-6 * rms).all(), float((np.abs(m_h - mref) / rms).max())
    assert (np.abs(v_h - vref) <= 1e-6 * vref).all(), float((np.abs(v_h - vref) / vref).max())
    sc_ref = gamma.astype(np.float64) / np.sqrt(v_h + BN_EPS)
    sh_ref = beta.astype(np.float64) - m_h * sc_ref
    assert (np.abs(_host(scale2) - sc_ref) <= 3 * _ulp(sc_ref)).all()
    assert (np.abs(_host(shift2) - sh_ref) <= 3 * _ulp(np.abs(beta) + np.abs(m_h * sc_ref))).all()


def _act64(torch, z, act, alpha):
    if act == "relu":
        return torch.relu(z)
    if act == "lrelu":
        return torch.maximum(alpha * z, z)
    return torch.relu(z) + alpha * torch.clamp(z, max=0.0)


def _bn_backward_ref(torch, z, valid, gamma, beta, act, alpha, dh):
    """fp64 autograd of h = BN_train(act(z)) over the valid rows; -> (dz, dgamma, dbeta, r, mean, var)."""
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    gt = torch.tensor(gamma, dtype=torch.float64, requires_grad=True)
    bt = torch.tensor(beta, dtype=torch.float64, requires_grad=True)
    al = alpha if act == "lrelu" else torch.tensor(alpha, dtype=torch.float64)
    r = _act64(torch, zt, act, al)[torch.from_numpy(valid)]
    m = r.mean(dim=0)
    v = ((r - m) ** 2).mean(dim=0)
    h = (r - m) / torch.sqrt(v + BN_EPS) * gt + bt
    (h * torch.tensor(dh[valid], dtype=torch.float64)).sum().backward()
    return zt.grad.numpy(), gt.grad.numpy(), bt.grad.numpy(), m.detach().numpy(), v.detach().numpy()


def _zcase(env, layout, C, act, seed):
    lay, valid, r, gamma, beta = _bn_case(env, layout, C, seed)
    rng = np.random.default_rng(seed + 1)
    z = r.copy()
    z[:, C // 3] = rng.standard_normal(z.shape[0])                 # (the cancellation channel belongs to the forward test)
    z[:, : C // 3] -= 1.0                                          # a third of the channels mostly negative
    z[np.abs(z) < 1e-3] = 0.5                                      # keep away from the kink (fp32 r vs fp64 r)
    gamma[C // 2] = 0.0                                            # a dead channel
    alpha = np.float32(0.2) if act == "lrelu" else (0.25 + 0.05 * rng.standard_normal(C)).astype(np.float32)
    if act == "relu":
        r32 = np.maximum(z, 0)
    elif act == "lrelu":
        r32 = np.maximum(alpha * z, z)
    else:
        r32 = np.maximum(z, 0) + alpha * np.minimum(z, 0)
    dh = rng.standard_normal(z.shape).astype(np.float32)
    return lay, valid, z, r32.astype(np.float32), gamma, beta, alpha, dh


@pytest.mark.parametrize("act", ["relu", "lrelu", "prelu"])
@pytest.mark.parametrize("C", [24, 512, 1536])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_bn_act_backward_matches_float64_autograd(env, layout, C, act):
    """bn_act_backward (column sums handed over), bn_act_backward_parts (128-row partial sums handed over, merged in the kernel) and
    col_sums_merge, with PReLU as bn_act_backward(act none) -> prelu_backward, the trainer's chain."""
    torch, hiplib = env["torch"], env["hiplib"]
    lay, valid, z, r32, gamma, beta, alpha, dh = _zcase(env, layout, C, act, seed=7 * C + len(layout))
    R = lay.rows
    dz_ref, dg_ref, db_ref, mref, vref = _bn_backward_ref(torch, z, valid, gamma, beta, act,
                                                          float(alpha) if act == "lrelu" else alpha, dh)
    n_frames = float(valid.sum())
    m32, v32 = mref.astype(np.float32), vref.astype(np.float32)
    # dgamma, dbeta are sums over the frames: their bars are relative to the L2 norm of the summands (sums of signed terms can cancel)
    xhat = (r32[valid].astype(np.float64) - mref) / np.sqrt(vref + BN_EPS)
    g_scale = np.sqrt(((dh[valid] * xhat) ** 2).sum(axis=0))
    b_scale = np.sqrt((dh[valid].astype(np.float64) ** 2).sum(axis=0))
    dh_in = dh.copy()
    dh_in[~valid] = NAN                                             # what lies in gap rows must not matter
    code = {"relu": RELU, "lrelu": LRELU, "prelu": 0}[act]
    alpha_arg = float(alpha) if act == "lrelu" else 0.0
    vt = _dev(env, valid.astype(np.uint8))
    args = (_dev(env, m32), _dev(env, v32), _dev(env, gamma), BN_EPS, n_frames, code, alpha_arg, vt)

    def check(dz, dgamma, dbeta, what):
        if act == "prelu":
            zt = _dev(env, z)
            hiplib.prelu_backward(dz, zt, _dev(env, alpha))
        dz_h, dg_h, db_h = _host(dz), _host(dgamma).astype(np.float64), _host(dbeta).astype(np.float64)
        assert (dz_h[~valid] == 0).all(), what                     # exactly 0 on every gap row
        e = _col_rel(dz_h[valid], dz_ref[valid])
        assert e.max() <= 2e-6, (what, float(e.max()), int(e.argmax()))
        _note("%s dz col rel" % what, e)
        _note("%s dgamma / |terms|" % what, np.abs(dg_h - dg_ref) / g_scale)
        _note("%s dbeta / |terms|" % what, np.abs(db_h - db_ref) / b_scale)
        assert (np.abs(dg_h - dg_ref) <= 2e-6 * g_scale).all(), (what, float((np.abs(dg_h - dg_ref) / g_scale).max()))
        assert (np.abs(db_h - db_ref) <= 2e-6 * b_scale).all(), (what, float((np.abs(db_h - db_ref) / b_scale).max()))

    # 1. the column sums handed over (fp32, as col_sums leaves them)
    s1 = (np.where(valid[:, None], dh.astype(np.float64), 0.0)).sum(axis=0).astype(np.float32)
    s2 = (np.where(valid[:, None], dh.astype(np.float64) * r32, 0.0)).sum(axis=0).astype(np.float32)
    dz, dg, db = _nan(env, R, C), _nan(env, C), _nan(env, C)
    hiplib.bn_act_backward(_dev(env, dh_in), _dev(env, r32), _dev(env, s1), _dev(env, s2), *args, dg, db, dz)
    check(dz, dg, db, "bn_act_backward")
    # 2. from the partial sums per 128-row tile (split + ordered merge inside the kernel)
    ws_h = _sums_workspace(dh, r32, valid)
    ws = _dev(env, ws_h)
    dz, dg, db = _nan(env, R, C), _nan(env, C), _nan(env, C)
    hiplib.bn_act_backward_parts(_dev(env, dh_in), _dev(env, r32), ws, *args, dg, db, dz)
    check(dz, dg, db, "bn_act_backward_parts")
    # 3. col_sums_merge of the same partials: one rounding of the fp64 totals
    sa, sab = _nan(env, C), _nan(env, C)
    hiplib.col_sums_merge(ws, R, C, sa, sab)
    tot = ws_h.sum(axis=0)
    assert (np.abs(_host(sa) - tot[0]) <= _ulp(np.abs(ws_h[:, 0]).sum(axis=0)) * 1.0001).all()
    assert (np.abs(_host(sab) - tot[1]) <= _ulp(np.abs(ws_h[:, 1]).sum(axis=0)) * 1.0001).all()


# ------------------------------------------------------------------------------------------------
# statistics pooling backward: pooled_b = [mean_t h || sqrt(var_t h + 1e-5)] per chunk (models.py:75-76)
# ------------------------------------------------------------------------------------------------
POOL_LENS = [1, 2, 37, 700, 5, 1, 2, 300]          # var = 0 (only eps left), two frames, a chunk past the 512-row split


def _pool_ref(torch, h, lay, dpooled):
    ht = torch.tensor(h, dtype=torch.float64, requires_grad=True)
    total, pooled = 0.0, []
    for b, (s, n) in enumerate(zip(lay.row_start, lay.row_len)):
        blk = ht[int(s):int(s) + int(n)]
        m = blk.mean(dim=0)
        sd = torch.sqrt(((blk - m) ** 2).mean(dim=0) + POOL_EPS)
        pooled.append(torch.cat([m, sd]).detach().numpy())
        total = total + (torch.cat([m, sd]) * torch.tensor(dpooled[b], dtype=torch.float64)).sum()
    total.backward()
    return ht, np.array(pooled)


@pytest.mark.parametrize("C", [13, 24, 1536])
def test_pool_backward_matches_float64_autograd(env, C):
    torch, hiplib = env["torch"], env["hiplib"]
    rng = np.random.default_rng(C)
    lay = env["engine"].BatchLayout(POOL_LENS, 3)
    valid = lay.row_valid().astype(bool)
    h = (rng.standard_normal((lay.rows, C)) * 2 + 1).astype(np.float32)
    h[:, 0] = 4.25                                           # a constant channel
    h[~valid] = 0.0
    dp = rng.standard_normal((lay.nchunks, 2 * C)).astype(np.float32)
    ht, pooled = _pool_ref(torch, h, lay, dp)
    dh = _nan(env, lay.rows, C)
    hiplib.pool_backward(_dev(env, h), _dev(env, lay.row_start), _dev(env, lay.row_len), lay.nchunks, _dev(env, pooled.astype(np.float32)),
                         _dev(env, dp), dh)
    dh_h = _host(dh).astype(np.float64)
    ref = ht.grad.numpy()
    assert (dh_h[~valid] == 0).all()
    for b, (s, n) in enumerate(zip(lay.row_start, lay.row_len)):
        got, want = dh_h[s:s + n], ref[s:s + n]
        e = np.sqrt(((got - want) ** 2).sum() / (want ** 2).sum())
        _note("pool_backward chunk rel", e)
        assert e <= 2e-6, (b, int(n), float(e))


@pytest.mark.parametrize("act", ["relu", "lrelu"])
@pytest.mark.parametrize("C", [24, 512, 1536])
def test_pool_bn_act_backward_matches_float64_autograd(env, C, act):
    """[act -> BN_train -> statistics pooling] backward of the last frame-level layer, in one kernel pair, against fp64 autograd of
    the three steps."""
    torch, hiplib = env["torch"], env["hiplib"]
    lay = env["engine"].BatchLayout(POOL_LENS, 3)
    valid = lay.row_valid().astype(bool)
    rng = np.random.default_rng(C + 5)
    C3 = C // 3
    z = (rng.standard_normal((lay.rows, C)) * 2 + 0.5).astype(np.float32)
    z[np.abs(z) < 1e-3] = 0.5
    z[~valid] = 0.0
    gamma = (1.0 + 0.2 * rng.standard_normal(C)).astype(np.float32)
    gamma[C3] = 0.0                                                     # a dead channel
    beta = (0.1 * rng.standard_normal(C)).astype(np.float32)
    alpha = 0.2
    dp = rng.standard_normal((lay.nchunks, 2 * C)).astype(np.float32)
    r32 = (np.maximum(z, 0) if act == "relu" else np.maximum(np.float32(alpha) * z, z)).astype(np.float32)
    # fp64 forward and autograd
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    gt = torch.tensor(gamma, dtype=torch.float64, requires_grad=True)
    bt = torch.tensor(beta, dtype=torch.float64, requires_grad=True)
    r = _act64(torch, zt, act, alpha)
    vm = torch.from_numpy(valid)
    m = r[vm].mean(dim=0)
    v = ((r[vm] - m) ** 2).mean(dim=0)
    h = (r - m) / torch.sqrt(v + BN_EPS) * gt + bt
    total, pooled, cm = 0.0, [], []
    for b, (s, n) in enumerate(zip(lay.row_start, lay.row_len)):
        blk, rb = h[int(s):int(s) + int(n)], r[int(s):int(s) + int(n)]
        mu = blk.mean(dim=0)
        sd = torch.sqrt(((blk - mu) ** 2).mean(dim=0) + POOL_EPS)
        pooled.append(torch.cat([mu, sd]).detach().numpy())
        cm.append(torch.cat([rb.mean(dim=0), ((rb - rb.mean(dim=0)) ** 2).mean(dim=0)]).detach().numpy())
        total = total + (torch.cat([mu, sd]) * torch.tensor(dp[b], dtype=torch.float64)).sum()
    total.backward()
    f32 = lambda a: _dev(env, np.asarray(a, np.float64).astype(np.float32))
    h32 = h.detach().numpy().astype(np.float32)
    h32[~valid] = 0.0
    dz, dg, db = _nan(env, lay.rows, C), _nan(env, C), _nan(env, C)
    hiplib.pool_bn_act_backward(_dev(env, h32), _dev(env, r32), _dev(env, lay.row_start), _dev(env, lay.row_len), lay.nchunks,
                                f32(pooled), _dev(env, dp), f32(cm), f32(m.detach().numpy()), f32(v.detach().numpy()), _dev(env, gamma),
                                BN_EPS, float(valid.sum()), {"relu": RELU, "lrelu": LRELU}[act], alpha, dg, db, dz)
    dz_h, dg_h, db_h = _host(dz).astype(np.float64), _host(dg).astype(np.float64), _host(db).astype(np.float64)
    dz_ref, dg_ref, db_ref = zt.grad.numpy(), gt.grad.numpy(), bt.grad.numpy()
    assert (dz_h[~valid] == 0).all()
    assert (dz_h[:, C3] == 0).all()
    for b, (s, n) in enumerate(zip(lay.row_start, lay.row_len)):
        got, want = dz_h[s:s + n], dz_ref[s:s + n]
        nw = np.sqrt((want ** 2).sum())
        e = np.sqrt(((got - want) ** 2).sum()) / nw if nw > 0 else float(np.abs(got).max())
        _note("pool_bn_act_backward dz chunk rel", e)
        assert e <= 2e-6, (b, int(n), float(e))
    # (bars relative to the L2 norm of the per-chunk summands, as in the test above)
    dmu, dsig = dp[:, :C].astype(np.float64), dp[:, C:].astype(np.float64)
    b_scale = np.sqrt((dmu ** 2).sum(axis=0))
    g_scale = np.sqrt(((dmu * np.array(cm)[:, :C]) ** 2 + (dsig * np.array(pooled)[:, C:]) ** 2).sum(axis=0)) * np.abs(
        1.0 / np.sqrt(v.detach().numpy() + BN_EPS)) + b_scale * np.abs(m.detach().numpy()) / np.sqrt(v.detach().numpy() + BN_EPS)
    _note("pool_bn_act_backward dbeta / |terms|", np.abs(db_h - db_ref) / b_scale)
    _note("pool_bn_act_backward dgamma / |terms|", np.abs(dg_h - dg_ref) / g_scale)
    assert (np.abs(db_h - db_ref) <= 2e-6 * b_scale).all(), float((np.abs(db_h - db_ref) / b_scale).max())
    assert (np.abs(dg_h - dg_ref) <= 2e-6 * g_scale).all(), float((np.abs(dg_h - dg_ref) / g_scale).max())


# ------------------------------------------------------------------------------------------------
# attention backward (csrc/xv_attention.hip), one kernel at a time, each from inputs made here -- a valid softmax computed on the
# host, pooled statistics consistent with h and att (fp64, rounded to fp32), tanh values up to +-1 -- and compared element by
# element with the fp64 evaluation of its formula on those same fp32 inputs.  The kernels are a handful of fp32 operations around
# double accumulators, so each bound is a worst-case count of roundings (u = 2^-24 relative each, no statistical factor) times the
# magnitudes the rounding sees; fused multiply-adds only remove roundings.  Second-order terms: the factor 1 + 2^-10; underflow:
# 2^-149.
# ------------------------------------------------------------------------------------------------
U24 = 2.0 ** -24
ATT_LENS = [1, 2, 31, 32, 33, 64, 1000, 5000]        # one row, the 32-row block of the pool backward +- 1, many blocks; 256-row loops of the softmax
ATT_CHANNELS = [4, 48, 256, 260, 1500]               # the 256-channel loop of a wave: 1 trip (partly filled), 1, 2 (4 channels in the second), 6
ATT_DIV = 5 * U24                                    # fp32 division: 2.5 ulp at worst (0.5 when correctly rounded)
SLACK = 1 + 2.0 ** -10
TINY = 2.0 ** -149


def _att_case(env, A, seed):
    """(layout, att [R] fp32 with NaN gap rows, per-chunk slices)."""
    lay = env["engine"].BatchLayout(ATT_LENS, 3)
    rng = np.random.default_rng(seed)
    att = np.full(lay.rows, NAN, np.float32)
    sl = [slice(int(s), int(s) + int(n)) for s, n in zip(lay.row_start, lay.row_len)]
    for s in sl:
        sc = 2.0 * rng.standard_normal(s.stop - s.start)
        e = np.exp(sc - sc.max())
        att[s] = (e / e.sum()).astype(np.float32)
    return lay, rng, att, sl


def _half(buf, C, side):
    return buf[:, :C] if side == "left" else buf[:, C:]


@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("A", ATT_CHANNELS)
def test_attention_pool_backward_elementwise(env, A, side):
    """dh[t, c] = a_t (g1 + 2 x g2), datt_t = sum_c x (g1 + x g2) with g2 = dsd / (2 sd), g1 = dm - 2 m g2.  h and dh are column
    slices (left / right half) of [R, 2C] buffers; gap rows and the other half of dh keep their NaN."""
    hiplib = env["hiplib"]
    C = A
    lay, rng, att, sl = _att_case(env, A, 100 + A)
    R, nb = lay.rows, lay.nchunks
    x = (rng.standard_normal((R, C)) * 1.7 + 3.0 * rng.standard_normal(C)).astype(np.float32)
    x[:, 1] = (100.0 + 1e-4 * rng.standard_normal(R)).astype(np.float32)      # large mean, tiny spread: sd ~ sqrt(eps)
    valid = lay.row_valid().astype(bool)
    hbuf = np.full((R, 2 * C), NAN, np.float32)
    _half(hbuf, C, side)[valid] = x[valid]
    pooled = np.zeros((nb, 2 * C), np.float32)
    for b, s in enumerate(sl):
        a64, x64 = att[s].astype(np.float64), x[s].astype(np.float64)
        m = a64 @ x64
        pooled[b] = np.concatenate([m, np.sqrt(np.maximum(a64 @ (x64 * x64) - m * m, 0.0) + POOL_EPS)]).astype(np.float32)
    assert pooled[-1, C + 1] < 3 * np.sqrt(POOL_EPS)                           # (att sums to 1 only to fp32 rounding: 1e4 (sum a - 1) adds to the variance)
    dp = rng.standard_normal((nb, 2 * C)).astype(np.float32)
    dp[[1, 6], C:] = 0.0                                                       # no gradient into sd
    dp[[2, 7], :C] = 0.0                                                       # no gradient into the mean
    hd = _dev(env, hbuf)
    dhbuf, datt = _nan(env, R, 2 * C), _nan(env, R)
    hiplib.attention_pool_backward(_half(hd, C, side), _dev(env, att), _dev(env, lay.row_start), _dev(env, lay.row_len), nb, max(ATT_LENS),
                                   _dev(env, pooled), _dev(env, dp), _half(dhbuf, C, side), datt)
    dh_all, da = _host(dhbuf).astype(np.float64), _host(datt).astype(np.float64)
    dh = _half(dh_all, C, side)
    assert np.isnan(_half(dh_all, C, "right" if side == "left" else "left")).all()      # the other half is not touched
    assert np.isnan(dh[~valid]).all() and np.isnan(da[~valid]).all()                     # gap rows are not written
    worst_h = worst_a = 0.0
    for b, s in enumerate(sl):
        xx, a = x[s].astype(np.float64), att[s].astype(np.float64)[:, None]
        pm, pd = pooled[b].astype(np.float64), dp[b].astype(np.float64)
        g2 = pd[C:] / (2 * pm[C:])
        g1 = pd[:C] - 2 * pm[:C] * g2
        p = 2 * xx * g2
        dh_ref = a * (g1 + p)
        da_ref = (xx * (g1 + xx * g2)).sum(1)
        # g2: one division.  g1: the error of g2 through 2 m, the rounding of 2 m g2, the subtraction.
        e2 = ATT_DIV * np.abs(g2)
        e1 = 2 * np.abs(pm[:C]) * e2 + U24 * np.abs(2 * pm[:C] * g2) + U24 * np.abs(g1)
        # dh: the errors of g1, g2 (the latter through 2 x), the roundings of 2 x g2, of the sum (<= u (|g1| + |2 x g2|)) and of a * (..)
        b_h = (a * (e1 + 2 * np.abs(xx) * e2 + U24 * np.abs(p) + U24 * (np.abs(g1) + np.abs(p))) + U24 * np.abs(dh_ref)) * SLACK + TINY
        # datt: the errors of g1, g2 through sum |x| (e1 + |x| e2) (the sum itself runs in double: C 2^-52 of the magnitudes), the cast
        mag = (np.abs(xx) * (np.abs(g1) + np.abs(xx * g2))).sum(1)
        b_a = ((np.abs(xx) * (e1 + np.abs(xx) * e2)).sum(1) + C * 2.0 ** -52 * mag + U24 * np.abs(da_ref)) * SLACK + TINY
        assert np.isfinite(dh[s]).all() and np.isfinite(da[s]).all()
        rh, ra = np.abs(dh[s] - dh_ref) / b_h, np.abs(da[s] - da_ref) / b_a
        worst_h, worst_a = max(worst_h, float(rh.max())), max(worst_a, float(ra.max()))
        assert (rh <= 1).all(), ("dh", A, side, b, np.unravel_index(np.argmax(rh), rh.shape), float(rh.max()))
        assert (ra <= 1).all(), ("datt", A, side, b, int(np.argmax(ra)), float(ra.max()))
        if b in (1, 6):                                                                    # dsd = 0: dh = a dm exactly one rounding
            assert (np.abs(dh[s] - dh_ref) <= U24 * np.abs(dh_ref) + TINY).all()
    _note("attention_pool_backward dh / bound (A %d)" % A, worst_h)
    _note("attention_pool_backward datt / bound (A %d)" % A, worst_a)


def test_attention_softmax_backward_elementwise(env):
    """ds_t = a_t (da_t - sum_tau a_tau da_tau), from att and datt made here; gap rows of dscores keep their NaN."""
    hiplib = env["hiplib"]
    lay, rng, att, sl = _att_case(env, 0, 7)
    R = lay.rows
    valid = lay.row_valid().astype(bool)
    da = np.full(R, NAN, np.float32)
    da[valid] = (rng.standard_normal(int(valid.sum())) * 10.0 ** rng.uniform(-2, 2, int(valid.sum())) + 3.0).astype(np.float32)
    ds = _nan(env, R)
    hiplib.attention_softmax_backward(_dev(env, att), _dev(env, da), _dev(env, lay.row_start), _dev(env, lay.row_len), lay.nchunks, ds)
    got = _host(ds).astype(np.float64)
    assert np.isnan(got[~valid]).all()
    worst = 0.0
    for s in sl:
        a, d = att[s].astype(np.float64), da[s].astype(np.float64)
        dot = a @ d
        ref = a * (d - dot)
        # the dot product and a (da - dot) are formed in double: (len + 8) 2^-53 of sum |a da| for the dot, 2^-52 for the difference and
        # the product; then two casts (u |ds| each) are allowed for the result
        n = s.stop - s.start
        bnd = (np.abs(a) * ((n + 8) * 2.0 ** -53 * (np.abs(a) @ np.abs(d)) + 2.0 ** -52 * (np.abs(d) + np.abs(dot))) + 2 * U24 * np.abs(ref)) * SLACK + TINY
        r = np.abs(got[s] - ref) / bnd
        worst = max(worst, float(r.max()))
        assert (r <= 1).all(), (n, int(np.argmax(r)), float(r.max()))
    assert got[sl[0]][0] == 0.0                                                            # one row: a = 1, ds = da - da
    _note("attention_softmax_backward ds / bound", worst)


@pytest.mark.parametrize("A", ATT_CHANNELS)
def test_attention_scores_backward_elementwise(env, A):
    """du = ds v (1 - n^2), nonlin <- ds n, with n up to +-(1 - 2^-20) and exact +-1, where 1 - n^2 cancels.  nonlin is the left
    half of its buffer, du the right half of its own; the other halves are not touched."""
    hiplib = env["hiplib"]
    rng = np.random.default_rng(300 + A)
    R = 1031                                                   # not a multiple of the 4 rows of a workgroup
    n = np.tanh(rng.standard_normal((R, A)) * 10.0 ** rng.uniform(-2, 1, (R, A))).astype(np.float32)
    sat = np.array([1.0, -1.0, 1 - 2.0 ** -20, -(1 - 2.0 ** -20), 1 - 2.0 ** -24, 0.0, 2.0 ** -13, -0.70710678], np.float32)
    pick = rng.random((R, A)) < 0.2
    n[pick] = rng.choice(sat, int(pick.sum()))
    n[0, :4] = sat[:4]
    v = (rng.standard_normal(A) * 0.3).astype(np.float32)
    ds = (rng.standard_normal(R) * 10.0 ** rng.uniform(-3, 1, R)).astype(np.float32)
    nbuf = np.full((R, 2 * A), NAN, np.float32)
    nbuf[:, :A] = n
    nd = _dev(env, nbuf)
    dubuf = _nan(env, R, 2 * A)
    hiplib.attention_scores_backward(nd[:, :A], _dev(env, ds), _dev(env, v), dubuf[:, A:])
    du_all, n_all = _host(dubuf).astype(np.float64), _host(nd).astype(np.float64)
    assert np.isnan(du_all[:, :A]).all() and np.isnan(n_all[:, A:]).all()
    n64, dsv = n.astype(np.float64), ds.astype(np.float64)[:, None] * v.astype(np.float64)
    ref = dsv * (1 - n64 * n64)
    # absolute, because 1 - n^2 cancels: n^2 is rounded (<= u, n^2 <= 1), 1 - fl(n^2) is exact from 0.5 up and rounded (<= u) below,
    # ds v is rounded and so is the product (u |ds v| each, 1 - n^2 <= 1): 4 u |ds v|
    bnd = 4 * U24 * np.abs(dsv) * SLACK + TINY
    r = np.abs(du_all[:, A:] - ref) / bnd
    assert (r <= 1).all(), (A, np.unravel_index(np.argmax(r), r.shape), float(r.max()))
    assert (du_all[:, A:][n64 * n64 == 1] == 0).all()                                     # exact +-1: exactly zero
    # nonlin after the call: ds n to one rounding
    g_ref = ds.astype(np.float64)[:, None] * n64
    assert (np.abs(n_all[:, :A] - g_ref) <= U24 * np.abs(g_ref) + TINY).all()
    _note("attention_scores_backward du / bound (A %d)" % A, float(r.max()))
