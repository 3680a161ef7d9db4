"""XV_FMT_SPLIT6 and the f16mx6 layer (xv_tdnn_layer_f16mx6: a hidden layer's cross terms on block-scaled e2m3 MFMAs) held to the
emulation of tests/layer_mx6_data.py.  Producer: a layer's epilogue writes the 6-bit rows, bit for bit the CPU encoder of its
exactly known outputs.  Consumer: exact answers where every sum is exact, element bounds on random data, position independence,
tap_bias at chunk edges, the status bit, the refusal of an odd slab count.  Whole network: both forms against the fp64 oracle.

Shapes: cin 64 / 128 (one and two periods of the kernel's two-slab loop), cout 256 / 512 (one and two column tiles), K 5 / 7,
R = 300 rows (a full 256-row tile and a partial one), three chunks of 101 / 101 / 89 frames on 8-row starts with 3-row gaps: two
chunk edges inside the first tile, the third chunk across the tile boundary."""
import numpy as np
import pytest

import arith_emul as em
import layer_mx6_data as lx

pytestmark = pytest.mark.gpu

R = 300
STARTS, LENS = [0, 104, 208], [101, 101, 89]
SHAPES = [(64, 256, 5), (128, 512, 7), (64, 512, 7), (128, 256, 5)]
Q13 = 2.0 ** -13


def row_valid(starts=STARTS, lens=LENS, rows=R):
    v = np.zeros(rows, np.uint8)
    for s, n in zip(starts, lens):
        v[s:s + n] = 1
    return v


VALID = row_valid()


@pytest.fixture(scope="module")
def env(oracle_mod):
    import torch
    from xvector_amd import engine, hiplib, synthetic, topology
    hiplib.require_gpu()
    return dict(torch=torch, hiplib=hiplib, engine=engine, oracle=oracle_mod, synthetic=synthetic, topology=topology,
                dev=torch.device("cuda:0"))


def dev_t(env, a, dtype=np.float32):
    return None if a is None else env["torch"].from_numpy(np.ascontiguousarray(a, dtype)).to(env["dev"])


def run_layer(env, x, w, form, yfmt, bias=None, scale=None, shift=None, act="none", valid=VALID, tapbias=None, xbuf=None):
    """One layer on host rows x [rows, cin] (encoded into the format the form reads, or taken from ``xbuf``): form "mx6" = x in SPLIT6,
    f16mx6 weights; "bf8" = x in SPLIT8, f16bf8 weights.  The output (a fresh, zeroed SplitBuf) is read back through split_decode: (decoded [rows, cout], second plane or None, status, the output buffer)."""
    torch, hiplib, dev = env["torch"], env["hiplib"], env["dev"]
    rows = len(valid)
    cout = w.shape[2]
    wt = dev_t(env, w)
    if xbuf is None:
        xbuf = hiplib.SplitBuf(rows, w.shape[1], dev, hiplib.FMT_SPLIT6 if form == "mx6" else hiplib.FMT_SPLIT8)
        hiplib.split_encode(dev_t(env, x), xbuf, rows=rows)
    y = hiplib.SplitBuf(rows, cout, dev, yfmt)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    args = (dev_t(env, bias), dev_t(env, scale), dev_t(env, shift), em.ACT[act], None, 1, dev_t(env, valid, np.uint8), y, status)
    if form == "mx6":
        hiplib.tdnn_layer_mx6(xbuf, rows, hiplib.pack_weights_f16mx6(wt), *args, tapbias=dev_t(env, tapbias))
    else:
        hiplib.tdnn_layer8(xbuf, rows, hiplib.pack_weights_f16bf8(wt), *args, tapbias=dev_t(env, tapbias))
    cq = torch.zeros((rows, cout), dtype=torch.float32, device=dev) if yfmt == hiplib.FMT_SPLIT6 else None
    out = hiplib.split_decode(y, rows, cq=cq)
    torch.cuda.synchronize()
    return out.cpu().numpy(), None if cq is None else cq.cpu().numpy(), int(status.item()), y


# ---- exact data ------------------------------------------------------------------------------------------------------------------
def grid_values(rng, shape, cls, density):
    """sign(n) (|n| cls + j 2^-13), n in 0 .. 4, j in 0 .. 3 where n != 0: hi = n cls in fp16, 2^11 lo = j / 4 (the scheme of
    tests/test_gpu_pair_mx6.py's exact_case); cls per block so that the blocks of a row take different scales."""
    n = rng.choice(np.array([0, 1, -1, 2, -2, 3, -3, 4, -4], np.float64), shape) * (rng.random(shape) < density)
    j = rng.integers(0, 4, shape) * np.sign(n)
    return (n * cls + j * Q13).astype(np.float32)


def block_classes(rng, n, C, choices):
    return np.repeat(rng.choice(choices, (n, C // 16)), 16, -1)


@pytest.mark.parametrize("cin,cout,K", SHAPES[:2])
def test_producer_writes_the_cpu_encoders_rows(env, cin, cout, K):
    """A bf8 layer whose outputs are known exactly -- output channel o = cls[r-block] n + j 2^-13, picked from two input channels by
    a centre tap of ones (every product and sum exact in fp32, the inputs exact in split8) -- written as SPLIT6 rows: both decoded
    planes equal the CPU encoder's, bit for bit, with block scales that differ along a row (a scale taken from the wrong lane or
    block would show).  Gap rows and rows past R decode to zero."""
    hiplib = env["hiplib"]
    rng = np.random.default_rng(100 + cin)
    # inputs: channel pair (2p, 2p + 1) carries (n, j 2^-13); output o takes pair[o] with the weights (class of o's block, 1)
    npart = rng.choice(np.array([0, 1, -1, 2, -2, 3, -3, 4, -4], np.float64), (R, cin // 2)) * (rng.random((R, cin // 2)) < 0.9)
    jpart = rng.integers(0, 4, (R, cin // 2)) * np.sign(npart)
    x = np.zeros((R, cin), np.float32)
    x[:, 0::2], x[:, 1::2] = npart, jpart * Q13
    x[VALID == 0] = 0
    assert np.array_equal(em.decode8(x), x)
    pair = (np.arange(cout) * 7 + 3) % (cin // 2)
    ccls = np.repeat(rng.permutation(np.resize([1.0, 4.0, 0.5, 16.0, 1.0, 2.0], cout // 16)), 16)
    w = np.zeros((K, cin, cout), np.float32)
    w[K // 2, 2 * pair, np.arange(cout)] = ccls
    w[K // 2, 2 * pair + 1, np.arange(cout)] = 1.0
    Y = (npart[:, pair] * ccls + jpart[:, pair] * Q13) * (VALID[:, None] != 0)
    assert np.array_equal(Y, Y.astype(np.float32)) and len(np.unique(lx.encode_rows(Y)[3][5])) >= 3
    want, want_c = lx.decode_rows(Y)
    assert (want != want_c).mean() > 0.2                              # the low plane is live: hi + lo_q 2^-11 is not c_q
    got, got_c, status, ybuf = run_layer(env, x, w, "bf8", hiplib.FMT_SPLIT6)
    assert status == 0
    assert np.array_equal(got, want) and np.array_equal(got_c, want_c)
    assert not got[VALID == 0].any() and not got_c[VALID == 0].any()
    # rows past R: those of the last tile are written as zeros, the padding behind them was never touched
    tail_c = env["torch"].zeros((R + 250, cout), dtype=env["torch"].float32, device=env["dev"])
    tail = hiplib.split_decode(ybuf, R + 250, cq=tail_c)
    assert not tail[R:].any().item() and not tail_c[R:].any().item()


_CASES = {}


def exact_case(cin, cout, K):
    """x and w = sign(n) (|n| cls + j 2^-13) with per-block classes (x: 1, 4, 1/2; w: 1, 2; w sparse): every product of the three
    terms is a multiple of 2^-14 and every partial sum stays below 2^24 of them -- the pre-activation is the same fp32 under any
    summation order."""
    key = ("exact", cin, cout, K)
    if key not in _CASES:
        rng = np.random.default_rng(7 * cin + cout + K)
        x = grid_values(rng, (R, cin), block_classes(rng, R, cin, [1.0, 1.0, 4.0, 0.5]), 0.9)
        x[VALID == 0] = 0
        wcls = block_classes(rng, K * cout, cin, [1.0, 2.0]).reshape(K, cout, cin).transpose(0, 2, 1)
        w = grid_values(rng, (K, cin, cout), wcls, 12.0 / (K * cin))         # ~12 products per output: M stays below 2^24 quanta
        z, M, parts = lx.contract(x, w)
        _CASES[key] = (x, w, z, M, parts)
    return _CASES[key]


@pytest.mark.parametrize("cin,cout,K", SHAPES)
def test_consumer_exact_answers_on_grid_data(env, cin, cout, K):
    hiplib = env["hiplib"]
    x, w, z, M, parts = exact_case(cin, cout, K)
    quantum = 2.0 ** -14
    assert all(np.array_equal(p / quantum, np.round(p / quantum)) for p in parts) and M.max() < 2 ** 24 * quantum
    assert all(np.abs(p).sum(0).min() > 0 for p in parts)             # all three terms live in every column
    assert np.array_equal(z, z.astype(np.float32).astype(np.float64))
    y = z * (VALID[:, None] != 0)
    # read back through both 8- and 6-bit rows: the encoders are exact functions of the fp32 value
    got, got_c, status, _ = run_layer(env, x, w, "mx6", hiplib.FMT_SPLIT6)
    want, want_c = lx.decode_rows(y)
    assert status == 0 and np.array_equal(got, want) and np.array_equal(got_c, want_c)
    got8, _, status, _ = run_layer(env, x, w, "mx6", hiplib.FMT_SPLIT8)
    assert status == 0 and np.array_equal(got8, em.decode8(y.astype(np.float32)))


def random_case(cin, cout, K):
    key = ("random", cin, cout, K)
    if key not in _CASES:
        rng = np.random.default_rng(cin + cout + K)
        f = lambda a: np.asarray(a, np.float32)
        x = f(np.maximum(rng.standard_normal((R, cin)), 0) * 1.3 * np.ldexp(1.0, rng.integers(-2, 3, (R, 1))))
        x[VALID == 0] = 0
        w = f(rng.standard_normal((K, cin, cout)) / np.sqrt(K * cin))
        b, s, o = f(0.1 * rng.standard_normal(cout)), f(rng.uniform(0.5, 2, cout)), f(rng.standard_normal(cout))
        _CASES[key] = (x, w, b, s, o)
    return _CASES[key]


@pytest.mark.parametrize("cin,cout,K", SHAPES)
def test_consumer_element_bounds_on_random_data(env, cin, cout, K):
    """Reference: the emulated f16mx6 terms in fp64 (the encoding is emulated, not bounded) through the fp64 epilogue; bound:
    em.elementwise_bound with A = sqrt(3 updates per slab and tap) for the fp32 accumulation and the bf16-split output's 2^-17.
    The reference itself is within layer_mx6_data.product_error_bound of the exact convolution (the grid's steps)."""
    hiplib = env["hiplib"]
    x, w, b, s, o = random_case(cin, cout, K)
    z, M, _ = lx.contract(x, w)
    zb = z + b
    yref = em.epilogue(z, b, s, o, "relu", None) * (VALID[:, None] != 0)
    A = em.accum_factor(em.depth("f16bf8", K, cin))
    bound = em.elementwise_bound(A, M + np.abs(b), zb, yref, s, None, "split")
    got, _, status, _ = run_layer(env, x, w, "mx6", hiplib.FMT_SPLIT, b, s, o, "relu")
    ratio = np.abs(got - yref) / bound
    exact = em.contract("fp32", x, w)[0]
    print("f16mx6 %d -> %d K %d: worst |device - emulation| / bound %.3f; rel L2 of the pre-activation against fp64: emulation %.3e" %
          (cin, cout, K, float(ratio[VALID != 0].max()), np.linalg.norm(z - exact) / np.linalg.norm(exact)))
    assert status == 0 and not got[VALID == 0].any()
    assert (ratio[VALID != 0] <= 1).all(), (np.unravel_index(np.argmax(ratio), ratio.shape), float(ratio.max()))
    assert (np.abs(z - exact) <= lx.product_error_bound(x, w)).all()


def test_the_same_chunk_at_two_row_offsets_gives_the_same_bits(env):
    hiplib = env["hiplib"]
    cin, cout, K = 128, 512, 7
    x, w, b, s, o = random_case(cin, cout, K)
    batch, _, st, _ = run_layer(env, x, w, "mx6", hiplib.FMT_SPLIT8, b, s, o, "relu")
    assert st == 0
    # chunk 2 (rows 208 .. 296, across the tile boundary) alone at row 0, and the whole batch moved down by 8 rows
    alone_valid = row_valid([0], [89], 96)
    xa = np.zeros((96, cin), np.float32)
    xa[:89] = x[208:297]
    alone, _, st, _ = run_layer(env, xa, w, "mx6", hiplib.FMT_SPLIT8, b, s, o, "relu", valid=alone_valid)
    assert st == 0 and np.array_equal(alone[:89], batch[208:297]) and np.abs(alone[:89]).sum() > 0
    moved_valid = row_valid([8, 112, 216], LENS, R + 8)
    xm = np.zeros((R + 8, cin), np.float32)
    xm[8:] = x
    moved, _, st, _ = run_layer(env, xm, w, "mx6", hiplib.FMT_SPLIT8, b, s, o, "relu", valid=moved_valid)
    assert st == 0 and not moved[:8].any() and np.array_equal(moved[8:], batch)


def test_tap_bias_at_chunk_edges(env):
    """The per-row bias of a folded producer shift: bias - sum of the missing taps' constants, at every chunk edge and buffer end,
    on the exact data (integers for the table: the answer stays exact)."""
    hiplib = env["hiplib"]
    cin, cout, K = 64, 256, 5
    x, w, z, _, _ = exact_case(cin, cout, K)
    rng = np.random.default_rng(4)
    table = rng.integers(-3, 4, (K, cout)).astype(np.float32)
    bias = rng.integers(-3, 4, cout).astype(np.float32) + table.sum(0)
    miss = lx.missing_taps(VALID, K)
    assert miss[VALID != 0].any(1).sum() == 2 * (K // 2) * len(STARTS)
    y = (z + bias - miss.astype(np.float64) @ table) * (VALID[:, None] != 0)
    assert np.array_equal(y, y.astype(np.float32).astype(np.float64))
    got, got_c, st, _ = run_layer(env, x, w, "mx6", hiplib.FMT_SPLIT6, bias, tapbias=table)
    want, want_c = lx.decode_rows(y)
    assert st == 0 and np.array_equal(got, want) and np.array_equal(got_c, want_c)
    # the bf8 producer's SPLIT6 epilogue applies the same table
    got, _, st, _ = run_layer(env, x, w, "bf8", hiplib.FMT_SPLIT6, bias, tapbias=table)
    z8 = em.contract("f16bf8", x, w)[0]
    y8 = (z8 + bias - miss.astype(np.float64) @ table) * (VALID[:, None] != 0)
    assert st == 0 and np.array_equal(got, lx.decode_rows(y8)[0])


def test_status_bit_and_clamp_of_split6_rows(env):
    """A bias that takes one column beyond 57344 sets bit 0 and the row holds the clamped value; at 57344 exactly it does not."""
    hiplib = env["hiplib"]
    cin, cout, K = 64, 256, 5
    x, w, z, _, _ = exact_case(cin, cout, K)
    col = 37
    w, z = w.copy(), z.copy()
    w[:, :, col], z[:, col] = 0, 0                                 # the column is its bias alone
    for extra, flag in ((0.0, 0), (64.0, 1)):
        bias = np.zeros(cout, np.float32)
        bias[col] = 57344.0 + extra
        got, got_c, st, _ = run_layer(env, x, w, "mx6", hiplib.FMT_SPLIT6, bias)
        y = (z + bias) * (VALID[:, None] != 0)
        want, want_c = lx.decode_rows(y)                          # (the CPU encoder clamps as the device does)
        assert st == flag and got.max() == 57344.0 and np.array_equal(got, want) and np.array_equal(got_c, want_c)


def test_unsupported_shapes_are_refused(env):
    torch, hiplib, dev = env["torch"], env["hiplib"], env["dev"]
    assert hiplib.layer_mx6_supported(7, 1, 512, 512) and hiplib.layer_mx6_supported(5, 2, 64, 256)
    assert not hiplib.layer_mx6_supported(7, 1, 96, 256)              # three slabs
    assert not hiplib.layer_mx6_supported(7, 1, 64, 128) and not hiplib.layer_mx6_supported(1, 1, 64, 256)
    assert not hiplib.layer_mx6_supported(7, 2, 64, 256)              # (K - 1) dilation > 8
    w = torch.zeros((7, 96, 256), device=dev)
    with pytest.raises(hiplib.XvectorHipError, match="unsupported shape"):
        hiplib.pack_weights_f16mx6(w)
    # the layer itself: an odd number of slabs behind a hand-made pack
    fake = hiplib.PackedMx6(hiplib.pack_weights_f16bf8(w).wt, 7, 96, 256)
    x6 = hiplib.SplitBuf(64, 96, dev, hiplib.FMT_SPLIT6)
    y = hiplib.SplitBuf(64, 256, dev, hiplib.FMT_SPLIT8)
    with pytest.raises(hiplib.XvectorHipError, match=r"\(-2\)"):
        hiplib.tdnn_layer_mx6(x6, 64, fake, None, None, None, 0, None, 1, None, y)
    # SPLIT6 output from a form that has no such epilogue: a K = 1 layer
    w1 = hiplib.pack_weights_f16bf8(torch.zeros((1, 64, 256), device=dev))
    x8 = hiplib.SplitBuf(64, 64, dev, hiplib.FMT_SPLIT8)
    with pytest.raises(hiplib.XvectorHipError, match=r"\(-2\)"):
        hiplib.tdnn_layer8(x8, 64, w1, None, None, None, 0, None, 1, None, hiplib.SplitBuf(64, 256, dev, hiplib.FMT_SPLIT6))
    torch.cuda.synchronize()


def test_whole_network_with_and_without_the_mx6_layer(env):
    """DeviceModel(layer_mx6=True / False) on trained-like weights, utterances of 25 / 40 / 61 frames: both under the project's 1e-4
    against the fp64 oracle and within 2e-4 of each other (twice the bar: two results that each hold it); the ratio of the two
    errors and both load-time probes are printed, no bound is set on them.  select_model still admits f16bf8 for these weights."""
    engine, oracle = env["engine"], env["oracle"]
    topo = env["topology"].get("ModelWithoutDropout")
    w = env["synthetic"].trained_like(topo, 23, seed=1)
    mats = env["synthetic"].mfcc_like([25, 40, 61], 23, seed=3)
    refs = [oracle.embed_utterance(m, w, topo, 25, 10000, np.float64) for m in mats]
    out, errs = {}, {}
    for on in (True, False):
        model = engine.DeviceModel(w, topo, "cuda:0", precision="f16bf8", layer_mx6=on)
        assert model.layer_mx6 == on and model.mx6_layers == ({2} if on else set())
        got = engine.Extractor(model, 25, 10000, accuracy_probe=False).extract(mats)
        out[on] = [np.asarray(g, np.float64) for g in got]
        errs[on] = max(oracle.rel_l2(g, r) for g, r in zip(got, refs))
        assert errs[on] < 1e-4, (on, errs[on])
    between = max(oracle.rel_l2(a, b) for a, b in zip(out[True], out[False]))
    sel6 = engine.select_model(w, topo, "cuda:0").selection
    sel8 = engine.select_model(w, topo, "cuda:0", layer_mx6=False).selection
    print("x-vectors against the fp64 oracle, worst of three: mx6 layer %.3e, bf8 layer %.3e (ratio %.3f); between the two forms %.3e; "
          "load-time probe: mx6 %.3e, bf8 %.3e of limit %.1e" % (errs[True], errs[False], errs[True] / errs[False], between,
                                                                sel6.get("mx6_f16bf8_vs_bf16x3", sel6["f16bf8_vs_bf16x3"]),
                                                                sel8["f16bf8_vs_bf16x3"], sel6["f16bf8_limit"]))
    assert between < 2e-4
    assert sel6["selected"] == "f16bf8" and sel8["selected"] == "f16bf8" and sel8["layer_mx6"] is False
