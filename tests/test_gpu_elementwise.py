"""Element-wise checks of every forward GEMM form (a relative-L2 number per chunk hides a wrong tap, slab, column or lane):

* exact known answers: integer data (x, w in [-3, 3], integer bias, BN scale / shift in {0.5, 1, 2} and halves passed directly,
  alpha 0.25 / 0.5) that every arithmetic computes exactly -- the output equals the fp64 oracle in EVERY element, gap rows are zero;
* read-back of the packed weights through the GEMM itself: one-hot input rows, every output is one encoded weight, bit for bit what
  tests/arith_emul.py says (this also settles that the fp16 / f8f6f4 MFMAs keep subnormal inputs);
* element-wise bounds on realistic and hostile data: |y - y_ref| <= A 2^-24 M max(1, |alpha|) |scale| + epilogue rounding (+ the
  output encoder's error), y_ref / M from the emulator of the split arithmetics (fp32 forms: the fp64 oracle), A fixed per form in
  tests/elementwise_data.py.  The worst ratio per form is printed at the end of the module.
"""
import math

import numpy as np
import pytest

import arith_emul as em
import elementwise_data as ed
from pair_data import _block_refs, _check_blocks  # noqa: F401  (shared with tests/test_gpu_pair_elementwise.py)

pytestmark = pytest.mark.gpu

WORST = {}


@pytest.fixture(scope="module")
def env(oracle_mod):
    import torch
    from xvector_amd import engine, hiplib
    hiplib.require_gpu()
    yield dict(torch=torch, hiplib=hiplib, engine=engine, oracle=oracle_mod, dev=torch.device("cuda:0"))
    if WORST:
        print("\nworst |y - y_ref| / bound per form (bound = A 2^-24 M max(1,|alpha|) |scale| + epilogue + encoder):")
        for name, (r, A) in WORST.items():
            print("  %-34s A = %7.1f   worst ratio %.3e" % (name, A, r))


FMT = {"f32": 0, "split": 1, "split8": 2}


def _tune(hiplib, tune):
    keys = {"fp32": hiplib.TUNE_FP32_GEMM, "rows": hiplib.TUNE_TILE_ROWS, "first": hiplib.TUNE_FIRST_TILES}
    return [(keys[k], v) for k, v in tune.items()]


def run_form(env, form, mats, w, b, scale, shift, act, alpha, dil=1, xfmt="f32", fmt="f32", tune=None, pool=False):
    """Pack ``mats`` with gap rows, run one forward form through the C ABI; returns (y fp32 [rows, cout] decoded, layout) or,
    with pool=True, (block statistics [blocks, 2, cout], layout).  form: fp32 | toom | rows | bf16x3 | f16bf8 | first."""
    torch, hiplib, engine, dev = env["torch"], env["hiplib"], env["engine"], env["dev"]
    K, cin, cout = w.shape
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    gap = max(1, (K - 1) * dil // 2)
    layout = engine.BatchLayout([m.shape[0] for m in mats], gap, math.lcm(8, 2 * dil))
    ld = {"rows": (cin + 3) // 4 * 4, "first": (cin + 7) // 8 * 8}.get(form, cin)
    host = np.zeros((layout.rows, ld), np.float32)
    layout.pack(mats, host)
    R = layout.rows
    rv = torch.from_numpy(layout.row_valid()).to(dev)
    wpad = np.zeros((K, ld, cout), np.float32)
    wpad[:, :cin] = w
    code = em.ACT[act]
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    x = t(host)
    if xfmt != "f32":
        x = hiplib.SplitBuf(R, cin, dev, FMT[xfmt])
        hiplib.split_encode(t(host), x)
    if pool:
        y = torch.full((hiplib.block_stats_floats(R, cout),), float("nan"), dtype=torch.float32, device=dev)
    elif fmt == "f32":
        y = torch.full((R, cout), float("nan"), dtype=torch.float32, device=dev)
    else:
        y = hiplib.SplitBuf(R, cout, dev, FMT[fmt])
        y.base.fill_(0x7b)                     # poison: fp16 0x7b7b = 61280, bf16 0x7b7b = 1.3e36
    args = (t(b), t(scale), t(shift), code, t(alpha))
    knobs = _tune(hiplib, tune or {})
    # the forms a knob forces exist only for some shapes (launch_gemm, launch_gemm8): refuse a case that would fall back quietly
    tiles128 = (R + 127) // 128 * ((cout + 127) // 128)
    if (tune or {}).get("fp32", 0) >= 2:
        assert cin % 32 == 0 and K in (1, 3, 5, 7) and tiles128 >= 768 and (K == 1 or tune["fp32"] == 2), "DMA-fed form not reachable"
    if form == "f16bf8" and (tune or {}).get("rows", 0) >= 512:
        assert K > 1 and cout % 256 == 0 and (pool or fmt != "f32"), "256 x 256 tile not reachable"
        assert tune["rows"] == 512 or ((cin + 31) // 32) % 2 == 0, "16 x 16 form needs an even number of slabs"
    try:
        for k, v in knobs:
            hiplib.set_tuning(k, v)
        if form == "fp32":
            wp = hiplib.pack_weights(t(w.reshape(K * cin, cout)))
            if pool:
                hiplib.tdnn_layer_pool(x, R, wp, *args, dil, rv, y, K=K)
            else:
                hiplib.tdnn_layer(x, wp, *args, K, dil, rv, y)
        elif form == "toom":
            hiplib.tdnn_layer(x, hiplib.pack_weights_toom(t(w)), *args, K, dil, rv, y)
        elif form == "rows":
            hiplib.tdnn_layer(x, hiplib.pack_weights_rows(t(wpad), ld), *args, K, 1, rv, y)
        elif form == "bf16x3":
            wp = hiplib.pack_weights_bf16x3(t(w))
            if pool:
                hiplib.tdnn_layer_pool(x, R, wp, *args, dil, rv, y)
            else:
                hiplib.tdnn_layer(x, wp, *args, K, dil, rv, y, None, rows=R)
        elif form == "f16bf8":
            wp = hiplib.pack_weights_f16bf8(t(w))
            if pool:
                hiplib.tdnn_layer_pool8(x, R, wp, *args, dil, rv, y)
            else:
                hiplib.tdnn_layer8(x, R, wp, *args, dil, rv, y, status)
        elif form == "first":
            hiplib.tdnn_first(x, R, hiplib.pack_first_bf16x3(t(wpad)), *args, dil, rv, y, status if fmt == "split8" else None)
        else:
            raise ValueError(form)
        torch.cuda.synchronize()
    finally:
        for k, _ in knobs:
            hiplib.set_tuning(k, 0)
    assert int(status.item()) == 0
    if pool:
        return y.cpu().numpy().reshape(-1, 2, cout), layout
    yh = (y if fmt == "f32" else hiplib.split_decode(y, R)).cpu().numpy()
    assert (yh[~layout.row_valid().astype(bool)] == 0).all()                 # gap rows: exact zeros
    return yh, layout


# ---------------------------------------------------------------------------------------------------------------------------
# 1. element-wise bounds on realistic and hostile data
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ed.BOUND_CASES, ids=[c.name for c in ed.BOUND_CASES])
def test_elementwise_bound(env, case):
    from test_toom_tables import _tables
    oracle = env["oracle"]
    mats, w, b, scale, shift, alpha = case.data()
    if case.big:                               # enough rows for the 128-row / DMA-fed forms (>= 768 tiles); the first chunks are checked
        rng = np.random.default_rng(7)
        mats = mats + [np.maximum(rng.standard_normal((300, case.cin)), 0).astype(np.float32) for _ in range(85)]
    y, layout = run_form(env, case.form, mats, w, b, scale, shift, case.act, alpha, case.dil, case.xfmt, case.fmt, case.tune)
    tiles128 = (layout.rows + 127) // 128 * ((case.cout + 127) // 128)
    if case.form == "fp32" and case.tune.get("fp32") == 1:      # the register-staged kernel takes 128-row tiles from 768 of them
        assert ("128-row" in case.name) == (tiles128 >= 768)
    if "16x16" in case.name:                                     # bf16x3: split input, K > 1, an even number of slabs
        assert case.xfmt == "split" and case.K > 1 and ((case.cin + 31) // 32) % 2 == 0
    A = case.A()
    Mt = None
    if case.form == "toom":
        G, SC, A1, _, _, BT = _tables(case.K)
        AT = [[1.0] * case.K + [0.0], [float(a) for a in A1]]
        host = np.zeros((layout.rows, case.cin), np.float32)
        layout.pack(mats, host)
        Mt = em.toom_magnitude(host, w, case.dil, [[float(g) for g in r] for r in G], [[float(v) for v in r] for r in BT], AT)
        Mt += np.abs(b)
    worst = 0.0
    for i, m in enumerate(mats[:len(ed.LENS)]):
        s, n = int(layout.row_start[i]), int(layout.row_len[i])
        got = y[s:s + n].astype(np.float64)
        assert np.isfinite(got).all()
        arith = "fp32" if case.arith in ("fp32", "fp32tc") else case.arith
        ref, zb, M = em.tdnn_layer(arith, m, w, b, scale, shift, case.act, alpha, case.dil)
        if arith == "fp32":
            ref = oracle.tdnn_layer(m, w, b, None, "none", None, case.dil, np.float64)
            zb = ref
            ref = em.epilogue(zb, None, scale, shift, case.act, alpha)
        if Mt is not None:
            M = Mt[s:s + n]
        bnd = em.elementwise_bound(A, M, zb, ref, scale, alpha, case.fmt)
        ratio = np.abs(got - ref) / bnd
        worst = max(worst, float(ratio.max()))
        assert (ratio <= 1).all(), (case.name, n, np.unravel_index(np.argmax(ratio), ratio.shape), float(ratio.max()))
    WORST[case.name] = (worst, A)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. exact known answers on integer data
# ---------------------------------------------------------------------------------------------------------------------------
EXACT_LENS = [25, 1, 130, 257, 64, 3, 700, 2]


def _int_data(rng, K, cin, cout, act, pool=False, lens=EXACT_LENS, density=0.3):
    mats = [rng.integers(-3, 4, (t, cin)).astype(np.float32) for t in lens]
    w = (rng.integers(-3, 4, (K, cin, cout)) * (rng.random((K, cin, cout)) < density)).astype(np.float32)
    b = rng.integers(-4, 5, cout).astype(np.float32)
    scale = rng.choice([1.0, 2.0] if pool else [0.5, 1.0, 2.0], cout).astype(np.float32)
    shift = (rng.integers(-4, 5, cout) * (1.0 if pool else 0.5)).astype(np.float32)
    alpha = None
    if act == "lrelu":
        alpha = np.array([0.5 if pool else 0.25], np.float32)
    elif act == "prelu":
        alpha = rng.choice([0.25, 0.5], cout).astype(np.float32)
    return mats, w, b, scale, shift, alpha


def _exact_ref(oracle, m, w, b, scale, shift, act, alpha, dil, ymax):
    z = oracle.tdnn_layer(m, w, b, None, "none", None, dil, np.float64)
    y = em.epilogue(z, None, scale, shift, act, alpha)
    # every partial sum stays below 2^24 (|z| <= sum |x w| + |b|) and |y| <= ymax: the data are exact in every arithmetic
    _, M = em.contract("fp32", m, w, dil)
    assert M.max(initial=0) + np.abs(b).max() < 2 ** 24 and np.abs(y).max(initial=0) <= ymax
    return y


EXACT_CASES = [
    # (name, form, cin, cout, K, dil, act, xfmt, fmt, tune)
    ("fp32 tdnn_gemm_kernel", "fp32", 23, 200, 5, 1, "prelu", "f32", "f32", {"fp32": 1}),
    ("fp32 tdnn_gemm_kernel ragged", "fp32", 40, 48, 3, 2, "lrelu", "f32", "f32", {"fp32": 1}),
    ("fp32 tdnn_gemm_dma_kernel", "fp32", 512, 512, 7, 1, "relu", "f32", "f32", {"fp32": 2}),
    ("fp32 tdnn_gemm_dma_kernel d3", "fp32", 64, 512, 3, 3, "none", "f32", "f32", {"fp32": 2}),
    ("fp32 tdnn_gemm_k1_kernel", "fp32", 512, 1536, 1, 1, "prelu", "f32", "f32", {"fp32": 3}),
    ("fp32tc toom<3>", "toom", 96, 200, 3, 1, "prelu", "f32", "f32", None),
    ("fp32tc toom<3> d8", "toom", 64, 64, 3, 8, "relu", "f32", "f32", None),
    ("fp32tc rows form", "rows", 23, 512, 5, 1, "lrelu", "f32", "f32", None),
    ("bf16x3 f32 in", "bf16x3", 40, 200, 3, 2, "lrelu", "f32", "f32", None),
    ("bf16x3 split 128", "bf16x3", 96, 48, 5, 1, "prelu", "split", "split", {"rows": 128}),
    ("bf16x3 split 256", "bf16x3", 96, 512, 7, 1, "relu", "split", "split", {"rows": 256}),
    ("bf16x3 split 16x16", "bf16x3", 64, 200, 5, 1, "prelu", "split", "f32", None),
    ("bf16x3 split K1", "bf16x3", 512, 1536, 1, 1, "none", "split", "split", None),
    ("bf16x3 first split", "first", 23, 512, 5, 1, "relu", "f32", "split", None),
    ("bf16x3 first split8", "first", 30, 288, 3, 1, "lrelu", "f32", "split8", None),
    ("f16bf8 128 f32", "f16bf8", 40, 200, 3, 2, "lrelu", "split8", "f32", {"rows": 128}),
    ("f16bf8 128 split8", "f16bf8", 64, 48, 5, 1, "prelu", "split8", "split8", {"rows": 128}),
    ("f16bf8 256 split", "f16bf8", 512, 512, 7, 1, "relu", "split8", "split", {"rows": 256}),
    ("f16bf8 512 split8", "f16bf8", 96, 512, 5, 1, "prelu", "split8", "split8", {"rows": 512}),
    ("f16bf8 1024 split8", "f16bf8", 512, 512, 5, 1, "relu", "split8", "split8", {"rows": 1024}),
    ("f16bf8 1024 split d3", "f16bf8", 128, 256, 3, 3, "lrelu", "split8", "split", {"rows": 1024}),
]


@pytest.mark.parametrize("name,form,cin,cout,K,dil,act,xfmt,fmt,tune", EXACT_CASES, ids=[c[0] for c in EXACT_CASES])
def test_exact_on_integer_data(env, name, form, cin, cout, K, dil, act, xfmt, fmt, tune):
    oracle = env["oracle"]
    rng = np.random.default_rng(cin + cout * 3 + K * 7 + dil)
    mats, w, b, scale, shift, alpha = _int_data(rng, K, cin, cout, act)
    n_check = len(mats)
    if (tune or {}).get("fp32", 0) >= 2:       # the DMA-fed forms need >= 768 tiles of 128 rows (else the register-staged kernel runs)
        mats = mats + [rng.integers(-3, 4, (300, cin)).astype(np.float32) for _ in range(85)]
    y, layout = run_form(env, form, mats, w, b, scale, shift, act, alpha, dil, xfmt, fmt, tune)
    for i, m in enumerate(mats[:n_check]):
        s, n = int(layout.row_start[i]), int(layout.row_len[i])
        ref = _exact_ref(oracle, m, w, b, scale, shift, act, alpha, dil, 2048)
        bad = np.argwhere(y[s:s + n] != ref)
        assert bad.size == 0, (name, n, bad[:5].tolist())


POOL_CASES = [
    ("fp32 pool", "fp32", 64, 200, 5, 1, "relu", "f32"),
    ("bf16x3 pool f32 in", "bf16x3", 64, 200, 3, 2, "prelu", "f32"),
    ("bf16x3 pool split", "bf16x3", 96, 512, 7, 1, "relu", "split"),
    ("f16bf8 pool8", "f16bf8", 64, 256, 5, 1, "lrelu", "split8"),
    ("f16bf8 pool8 K1", "f16bf8", 512, 1536, 1, 1, "relu", "split8"),
]


@pytest.mark.parametrize("name,form,cin,cout,K,dil,act,xfmt", POOL_CASES, ids=[c[0] for c in POOL_CASES])
def test_pool_block_statistics_exact_on_integer_data(env, name, form, cin, cout, K, dil, act, xfmt):
    """The fused pooling epilogues on integer y with |y| <= 512 (every square and partial sum of a block below 2^24): (mean, M2) of a block of 1, 2, 4 or 8 valid rows is exact,
    other blocks within 4 ulp of the fp64 statistics of the exact y."""
    oracle = env["oracle"]
    rng = np.random.default_rng(cin + cout + K)
    lens = [25, 1, 7, 130, 257, 3, 12, 64]
    mats, w, b, scale, shift, alpha = _int_data(rng, K, cin, cout, act, pool=True, lens=lens, density=min(0.1, 12.0 / (K * cin)))
    blk, layout = run_form(env, form, mats, w, b, scale, shift, act, alpha, dil, xfmt, pool=True)
    yfull = np.zeros((layout.rows, cout))
    for i, m in enumerate(mats):
        s, n = int(layout.row_start[i]), int(layout.row_len[i])
        yfull[s:s + n] = _exact_ref(oracle, m, w, b, scale, shift, act, alpha, dil, 512)
    _check_blocks(blk, layout, yfull, cout, name)


@pytest.mark.parametrize("arith", ["bf16x3", "f16bf8"])
@pytest.mark.parametrize("cin,cout,act", [(512, 1536, "relu"), (64, 64, "none"), (96, 192, "relu")])
def test_pair_kernels_exact_on_integer_data(env, arith, cin, cout, act):
    """tdnn_pair_pool(8): the layer-3 intermediate stays an integer <= 2048 (exact in bf16 hi + lo and in fp16), layer 4 an
    integer <= 512: block statistics exact / within 4 ulp as for the pooling epilogues."""
    torch, hiplib, engine, oracle, dev = env["torch"], env["hiplib"], env["engine"], env["oracle"], env["dev"]
    rng = np.random.default_rng(cin + cout)
    cmid = 512
    lens = [25, 1, 7, 8, 9, 130, 257, 3]
    mats = [rng.integers(-3, 4, (n, cin)).astype(np.float32) for n in lens]
    w1 = (rng.integers(-3, 4, (cin, cmid)) * (rng.random((cin, cmid)) < 3.0 / cin)).astype(np.float32)
    w2 = (rng.integers(-3, 4, (cmid, cout)) * (rng.random((cmid, cout)) < 1.0 / cmid)).astype(np.float32)
    b1, b2 = rng.integers(-4, 5, cmid).astype(np.float32), rng.integers(-4, 5, cout).astype(np.float32)
    s1, s2 = rng.choice([1.0, 2.0], cmid).astype(np.float32), rng.choice([1.0, 2.0], cout).astype(np.float32)
    o1, o2 = rng.integers(-2, 3, cmid).astype(np.float32), rng.integers(-2, 3, cout).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    layout = engine.BatchLayout(lens, 1, hiplib.POOL_BLOCK_ROWS)
    host = np.zeros((layout.rows, cin), np.float32)
    layout.pack(mats, host)
    fmt = hiplib.FMT_SPLIT8 if arith == "f16bf8" else hiplib.FMT_SPLIT
    xin = hiplib.SplitBuf(layout.rows, cin, dev, fmt)
    hiplib.split_encode(t(host), xin)
    blk = torch.full((hiplib.block_stats_floats(layout.rows, cout),), float("nan"), dtype=torch.float32, device=dev)
    code, rv = em.ACT[act], t(layout.row_valid())
    if arith == "f16bf8":
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        hiplib.tdnn_pair_pool8(xin, layout.rows, hiplib.pack_pair_f16bf8(t(w1), t(w2)), (t(b1), t(s1), t(o1), None),
                               (t(b2), t(s2), t(o2), None), code, rv, blk, status)
        assert int(status.item()) == 0
    else:
        hiplib.tdnn_pair_pool(xin, layout.rows, hiplib.pack_pair_bf16x3(t(w1), t(w2)), (t(b1), t(s1), t(o1), None),
                              (t(b2), t(s2), t(o2), None), code, rv, blk)
    torch.cuda.synchronize()
    yfull = np.zeros((layout.rows, cout))
    for i, m in enumerate(mats):
        s, n = int(layout.row_start[i]), int(layout.row_len[i])
        h = _exact_ref(oracle, m, w1[None], b1, s1, o1, act, None, 1, 2048)
        yfull[s:s + n] = _exact_ref(oracle, h, w2[None], b2, s2, o2, act, None, 1, 512)
    _check_blocks(blk.cpu().numpy().reshape(-1, 2, cout), layout, yfull, cout, "pair " + arith)


FC_CASES = [("xv_fc_f32", 77, 3072, 512, "relu"), ("fc_splitk", 64, 3072, 512, "prelu"), ("xv_fc_bf16x3", 77, 1536, 200, "lrelu")]


@pytest.mark.parametrize("which,B,In,Out,act", FC_CASES, ids=[c[0] for c in FC_CASES])
def test_fc_exact_on_integer_data_and_within_the_bound(env, which, B, In, Out, act):
    torch, hiplib, oracle, dev = env["torch"], env["hiplib"], env["oracle"], env["dev"]
    rng = np.random.default_rng(B + In + Out)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)

    def run(x, w, b, scale, shift, alpha):
        y = torch.full((B, Out), float("nan"), dtype=torch.float32, device=dev)
        if which == "xv_fc_bf16x3":
            hiplib.fc(t(x), hiplib.pack_weights_bf16x3(t(w[None])), t(b), t(scale), t(shift), em.ACT[act], t(alpha), y, None)
        elif which == "fc_splitk":
            assert hiplib.fc_splitk_supported(B, In, Out)
            hiplib.fc_splitk(t(x), hiplib.pack_weights(t(w)), t(b), t(scale), t(shift), em.ACT[act], t(alpha), y, None)
        else:
            hiplib.fc(t(x), hiplib.pack_weights(t(w)), t(b), t(scale), t(shift), em.ACT[act], t(alpha), y, None)
        torch.cuda.synchronize()
        return y.cpu().numpy().astype(np.float64)

    (x,), w, b, scale, shift, alpha = _int_data(rng, 1, In, Out, act, lens=[B], density=0.1)
    ref = _exact_ref(oracle, x, w, b, scale, shift, act, alpha, 1, 2048)
    assert np.array_equal(run(x, w[0], b, scale, shift, alpha), ref)
    # realistic data: pooled statistics-like input (non-negative means, spread deviations), element-wise bound
    x = np.concatenate([np.abs(rng.standard_normal((B, In // 2))), np.exp(0.5 * rng.standard_normal((B, In // 2)))], 1).astype(np.float32)
    w = (rng.standard_normal((In, Out)) / np.sqrt(In)).astype(np.float32)
    scale = np.exp(0.3 * rng.standard_normal(Out)).astype(np.float32)
    arith = "bf16x3" if which == "xv_fc_bf16x3" else "fp32"
    refy, zb, M = em.fc(arith, x, w, b, scale, shift, act, alpha)
    # fp32 FC (xv_fc_f32, split-K): 32x32x2 updates; bf16x3 FC: as the layer kernels
    A = em.accum_factor(em.depth(arith, 1, In))
    bnd = em.elementwise_bound(A, M, zb, refy, scale, alpha)
    ratio = np.abs(run(x, w, b, scale, shift, alpha) - refy) / bnd
    WORST[which] = (float(ratio.max()), A)
    assert (ratio <= 1).all(), float(ratio.max())


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the packed weights read back through the GEMM (one-hot rows)
# ---------------------------------------------------------------------------------------------------------------------------
def _probe_weights(rng, K, cin, cout):
    """Values that exercise the encoders: ties of fp16 / bf16 / e5m2, fp16 and e5m2 subnormals, the clamp, zeros."""
    w = rng.standard_normal((K, cin, cout)) * np.exp(2 * rng.standard_normal((K, cin, cout)))
    flat = w.reshape(-1)
    n = flat.size
    special = np.array([1 + 2 ** -11, 1 + 3 * 2 ** -11, 1 + 2 ** -8, 1 + 3 * 2 ** -8, 1e-7, 3e-6, 2 ** -24, 2 ** -25, 6.1e-5, 0.0,
                        -1 - 3 * 2 ** -11, 1 + 2 ** -11 + 2 ** -13 * 1.25, 7e4, -1e6, 57344.0, 1.5 * 2 ** -14, 1e-30])
    idx = rng.choice(n, min(n, 40 * len(special)), replace=False)
    flat[idx] = np.resize(special, len(idx)) * np.resize([1, -1, 0.5, 2.0 ** -12], len(idx))
    return w.astype(np.float32)


@pytest.mark.parametrize("form,K,cin,cout", [("bf16x3", 1, 64, 200), ("bf16x3", 5, 40, 48), ("f16bf8", 1, 64, 200),
                                             ("f16bf8", 3, 96, 512), ("first", 5, 23, 512)])
def test_packed_weights_read_back_through_the_gemm(env, form, K, cin, cout):
    """x = e_j (one nonzero frame between zero rows, K > 1): output row t of channel o is the encoded w[k, j, o] of one tap --
    wh + wl (bf16x3), wh + 2^-11 wl8 (f16bf8) -- bit for bit what the emulator encodes, subnormals and ties included."""
    rng = np.random.default_rng(K * 100 + cin)
    w = _probe_weights(rng, K, cin, cout)
    h = (K - 1) // 2
    T = K + 2
    mats = []
    for j in range(cin):                                 # chunk j: frame h + 1 is e_j, every other frame zero
        m = np.zeros((T, cin), np.float32)
        m[h + 1, j] = 1.0
        mats.append(m)
    xfmt = {"bf16x3": "split", "f16bf8": "split8", "first": "f32"}[form]
    y, layout = run_form(env, form, mats, w, None, None, None, "none", None, 1, xfmt, "f32" if form != "first" else "split")
    arith = "f16bf8" if form == "f16bf8" else "bf16x3"
    wc = np.clip(w, -em.SPLIT8_MAX, em.SPLIT8_MAX) if arith == "f16bf8" else w
    if arith == "f16bf8":
        hi, l8, _ = em.split8(wc)
        want = hi.astype(np.float64) + l8.astype(np.float64) / em.LO_SCALE
    else:
        hi, lo = em.split3(wc)
        want = hi.astype(np.float64) + lo
    want = want.astype(np.float32)                      # exact: wh + wl carries 16 bits, wh + 2^-11 wl8 14
    assert np.array_equal(want.astype(np.float64), (hi.astype(np.float64) + (l8 / em.LO_SCALE if arith == "f16bf8" else lo)))
    if form == "first":                                 # the first-layer kernel's output is itself bf16-split encoded
        want = em.decode3(want)
    for j in range(cin):
        s = int(layout.row_start[j])
        for k in range(K):
            got = y[s + h + 1 - (k - h)]                 # output row t reads frame t + (k - h)
            bad = np.flatnonzero(got != want[k, j])
            assert bad.size == 0, (form, j, k, bad[:4].tolist(), got[bad[:4]].tolist(), want[k, j][bad[:4]].tolist())


@pytest.mark.parametrize("arith", ["bf16x3", "f16bf8"])
@pytest.mark.parametrize("which", ["w1", "w2"])
def test_pair_packers_read_back_through_the_kernel(env, arith, which):
    """pack_pair_bf16x3 / pack_pair_f16bf8 read back through the pair kernels: one-hot rows, one frame per chunk, so every 8-row
    block holds one valid row and its mean IS that frame's layer-4 output.  which = w1: x = e_j, w2 = identity, mean[o] = the
    encoded w1[j, o] after the intermediate's own encoding; which = w2: w1 routes e_j to mid channel 8j with weight 1, mean[o] =
    the encoded w2[8j, o].  Bit for bit what tests/arith_emul.py says, subnormals, ties and the clamp included."""
    torch, hiplib, engine, dev = env["torch"], env["hiplib"], env["engine"], env["dev"]
    cin, cmid, cout = 64, 512, 512
    assert (hiplib.pair8_supported if arith == "f16bf8" else hiplib.pair_supported)(cin, cmid, cout)
    rng = np.random.default_rng(5 if which == "w1" else 6)
    if which == "w1":
        w1 = _probe_weights(rng, 1, cin, cmid)[0]
        w2 = np.eye(cmid, cout, dtype=np.float32)
    else:
        w1 = np.zeros((cin, cmid), np.float32)
        w1[np.arange(cin), 8 * np.arange(cin)] = 1.0
        w2 = _probe_weights(rng, 1, cmid, cout)[0]
    dec = em.decode8 if arith == "f16bf8" else em.decode3
    clip = (lambda a: np.clip(a, -em.SPLIT8_MAX, em.SPLIT8_MAX)) if arith == "f16bf8" else (lambda a: a)
    want = dec(dec(clip(w1))) if which == "w1" else dec(clip(w2))[8 * np.arange(cin)]      # [cin, cout]
    mats = [np.eye(1, cin, j, dtype=np.float32) for j in range(cin)]
    layout = engine.BatchLayout([1] * cin, 1, hiplib.POOL_BLOCK_ROWS)
    host = np.zeros((layout.rows, cin), np.float32)
    layout.pack(mats, host)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    xin = hiplib.SplitBuf(layout.rows, cin, dev, hiplib.FMT_SPLIT8 if arith == "f16bf8" else hiplib.FMT_SPLIT)
    hiplib.split_encode(t(host), xin)
    blk = torch.full((hiplib.block_stats_floats(layout.rows, cout),), float("nan"), dtype=torch.float32, device=dev)
    rv = t(layout.row_valid())
    if arith == "f16bf8":
        hiplib.tdnn_pair_pool8(xin, layout.rows, hiplib.pack_pair_f16bf8(t(w1), t(w2)), (None,) * 4, (None,) * 4, 0, rv, blk)
    else:
        hiplib.tdnn_pair_pool(xin, layout.rows, hiplib.pack_pair_bf16x3(t(w1), t(w2)), (None,) * 4, (None,) * 4, 0, rv, blk)
    torch.cuda.synchronize()
    got = blk.cpu().numpy().reshape(-1, 2, cout)[layout.row_start // 8, 0]
    bad = np.argwhere(got != want)
    assert bad.size == 0, (arith, which, bad[:4].tolist(), got[tuple(bad[:4].T)].tolist(), want[tuple(bad[:4].T)].tolist())
