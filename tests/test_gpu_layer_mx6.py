"""XV_FMT_SPLIT6 and the f16mx6 layer (xv_tdnn_layer_f16mx6: a hidden layer's cross terms on block-scaled e2m3 MFMAs) held to the
emulation of tests/layer_mx6_data.py.  Producer: a layer's epilogue writes the 6-bit rows, bit for bit the CPU encoder of its
exactly known outputs.  Consumer: exact answers where every sum is exact, element bounds on random data, position independence,
tap_bias at chunk edges, the status bit, the refusal of an odd slab count.  Whole network: both forms against the fp64 oracle.

Shapes: cin 64 / 128 (one and two periods of the kernel's two-slab loop), cout 256 / 512 (one and two column tiles), K 5 / 7,
R = 300 rows (a full 256-row tile and a partial one), three chunks of 101 / 101 / 89 frames on 8-row starts with 3-row gaps: two
chunk edges inside the first tile, the third chunk across the tile boundary.

The second half of the file takes the same checks to K = 3 (the extreme of the loop's compile-time schedule) and to dilations 1 .. 4 up
to the entry point's limit (K - 1) dilation = 8, on layer_mx6_data.edge_layout's rows: chunks of 1, 2, h, h + 1, 97, 3 and 150 frames
(h = the halo) with the layer's own gap, so that rows miss several taps and taps on both sides.  There too: the producer -> consumer
chain of the dilated topology on one buffer, every activation / scale / shift form of the 6-bit epilogue, the encoder, the decoder and
the weight pack on their own against hostile values, R = 256 / 257, and ModelWithoutDropoutTdnn end to end."""
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


def run_layer(env, x, w, form, yfmt, bias=None, scale=None, shift=None, act="none", valid=VALID, tapbias=None, xbuf=None, dilation=1,
              alpha=None):
    """One layer on host rows x [rows, cin] (encoded into the format the form reads, or taken from ``xbuf``): form "mx6" = x in SPLIT6,
    f16mx6 weights; "bf8" = x in SPLIT8, f16bf8 weights; ``alpha``: one value for "lrelu", one per channel for "prelu".  The output (a
    fresh, zeroed SplitBuf) is read back through split_decode: (decoded [rows, cout], second plane or None, status, the output buffer)."""
    torch, hiplib, dev = env["torch"], env["hiplib"], env["dev"]
    rows = len(valid)
    cout = w.shape[2]
    wt = dev_t(env, w)
    if xbuf is None:
        xbuf = hiplib.SplitBuf(rows, w.shape[1], dev, hiplib.FMT_SPLIT6 if form == "mx6" else hiplib.FMT_SPLIT8)
        hiplib.split_encode(dev_t(env, x), xbuf, rows=rows)
    y = hiplib.SplitBuf(rows, cout, dev, yfmt)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    args = (dev_t(env, bias), dev_t(env, scale), dev_t(env, shift), em.ACT[act], dev_t(env, alpha), dilation, dev_t(env, valid, np.uint8), y,
            status)
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


def producer_case(cin, cout, K, valid=VALID, seed=None, classes=(1.0, 4.0, 0.5, 16.0, 1.0, 2.0)):
    """Inputs and weights of a bf8 layer whose outputs are known exactly: channel pair (2p, 2p + 1) of x carries (n, j 2^-13); output
    o takes pair[o] through a centre tap with the weights (class of o's 16-column block, 1).  -> (x, w, Y = the layer's output)."""
    rows = len(valid)
    rng = np.random.default_rng(100 + cin if seed is None else seed)
    npart = rng.choice(np.array([0, 1, -1, 2, -2, 3, -3, 4, -4], np.float64), (rows, cin // 2)) * (rng.random((rows, cin // 2)) < 0.9)
    jpart = rng.integers(0, 4, (rows, cin // 2)) * np.sign(npart)
    x = np.zeros((rows, cin), np.float32)
    x[:, 0::2], x[:, 1::2] = npart, jpart * Q13
    x[valid == 0] = 0
    assert np.array_equal(em.decode8(x), x)
    pair = (np.arange(cout) * 7 + 3) % (cin // 2)
    ccls = np.repeat(rng.permutation(np.resize(list(classes), cout // 16)), 16)
    w = np.zeros((K, cin, cout), np.float32)
    w[K // 2, 2 * pair, np.arange(cout)] = ccls
    w[K // 2, 2 * pair + 1, np.arange(cout)] = 1.0
    Y = (npart[:, pair] * ccls + jpart[:, pair] * Q13) * (valid[:, None] != 0)
    assert np.array_equal(Y, Y.astype(np.float32))
    return x, w, Y


@pytest.mark.parametrize("cin,cout,K", SHAPES[:2])
def test_producer_writes_the_cpu_encoders_rows(env, cin, cout, K):
    """A bf8 layer whose outputs are known exactly -- output channel o = cls[r-block] n + j 2^-13, picked from two input channels by
    a centre tap of ones (every product and sum exact in fp32, the inputs exact in split8) -- written as SPLIT6 rows: both decoded
    planes equal the CPU encoder's, bit for bit, with block scales that differ along a row (a scale taken from the wrong lane or
    block would show).  Gap rows and rows past R decode to zero."""
    hiplib = env["hiplib"]
    x, w, Y = producer_case(cin, cout, K)
    assert len(np.unique(lx.encode_rows(Y)[3][5])) >= 3
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


def exact_case(cin, cout, K, dil=1, valid=VALID):
    """x and w = sign(n) (|n| cls + j 2^-13) with per-block classes (x: 1, 4, 1/2; w: 1, 2; w sparse): every product of the three
    terms is a multiple of 2^-14 and every partial sum stays below 2^24 of them -- the pre-activation is the same fp32 under any
    summation order.  ``valid``: the row layout (its length is the number of rows); gap rows of x are zero."""
    key = ("exact", cin, cout, K, dil, valid.tobytes())
    if key not in _CASES:
        rows = len(valid)
        for attempt in range(8):       # (a draw that leaves a column of the sparse w without one of the terms is drawn again)
            rng = np.random.default_rng(7 * cin + cout + K + (0 if valid is VALID else 1000 * dil + rows) + 7919 * attempt)
            x = grid_values(rng, (rows, cin), block_classes(rng, rows, cin, [1.0, 1.0, 4.0, 0.5]), 0.9)
            x[valid == 0] = 0
            wcls = block_classes(rng, K * cout, cin, [1.0, 2.0]).reshape(K, cout, cin).transpose(0, 2, 1)
            w = grid_values(rng, (K, cin, cout), wcls, 12.0 / (K * cin))     # ~12 products per output: M stays below 2^24 quanta
            z, M, parts = lx.contract(x, w, dil)
            if all(np.abs(p).sum(0).min() > 0 for p in parts) and M.max() < 2 ** 10:
                break
        _CASES[key] = (x, w, z, M, parts)
    return _CASES[key]


def assert_exact(z, M, parts):
    """What makes a case exact: every term a multiple of 2^-14, fewer than 2^24 of them in any partial sum, all three terms live in
    every column, the answer an fp32."""
    quantum = 2.0 ** -14
    assert all(np.array_equal(p / quantum, np.round(p / quantum)) for p in parts) and M.max() < 2 ** 24 * quantum
    assert all(np.abs(p).sum(0).min() > 0 for p in parts)
    assert np.array_equal(z, z.astype(np.float32).astype(np.float64))


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


def random_case(cin, cout, K, dil=1, valid=VALID):
    key = ("random", cin, cout, K, dil, valid.tobytes())
    if key not in _CASES:
        rows = len(valid)
        rng = np.random.default_rng(cin + cout + K + (0 if valid is VALID else 1000 * dil + rows))
        f = lambda a: np.asarray(a, np.float32)
        x = f(np.maximum(rng.standard_normal((rows, cin)), 0) * 1.3 * np.ldexp(1.0, rng.integers(-2, 3, (rows, 1))))
        x[valid == 0] = 0
        w = f(rng.standard_normal((K, cin, cout)) / np.sqrt(K * cin))
        b, s, o = f(0.1 * rng.standard_normal(cout)), f(rng.uniform(0.5, 2, cout)), f(rng.standard_normal(cout))
        _CASES[key] = (x, w, b, s, o)
    return _CASES[key]


def check_element_bounds(env, cin, cout, K, dil=1, valid=VALID):
    hiplib = env["hiplib"]
    x, w, b, s, o = random_case(cin, cout, K, dil, valid)
    z, M, _ = lx.contract(x, w, dil)
    zb = z + b
    yref = em.epilogue(z, b, s, o, "relu", None) * (valid[:, None] != 0)
    A = em.accum_factor(em.depth("f16bf8", K, cin))
    bound = em.elementwise_bound(A, M + np.abs(b), zb, yref, s, None, "split")
    got, _, status, _ = run_layer(env, x, w, "mx6", hiplib.FMT_SPLIT, b, s, o, "relu", valid=valid, dilation=dil)
    ratio = np.abs(got - yref) / bound
    exact = em.contract("fp32", x, w, dil)[0]
    print("f16mx6 %d -> %d K %d dilation %d: worst |device - emulation| / bound %.3f; rel L2 of the pre-activation against fp64: "
          "emulation %.3e" % (cin, cout, K, dil, float(ratio[valid != 0].max()), np.linalg.norm(z - exact) / np.linalg.norm(exact)))
    assert status == 0 and not got[valid == 0].any()
    assert (ratio[valid != 0] <= 1).all(), (np.unravel_index(np.argmax(ratio), ratio.shape), float(ratio.max()))
    assert (np.abs(z - exact) <= lx.product_error_bound(x, w, dil)).all()


@pytest.mark.parametrize("cin,cout,K", SHAPES)
def test_consumer_element_bounds_on_random_data(env, cin, cout, K):
    """Reference: the emulated f16mx6 terms in fp64 (the encoding is emulated, not bounded) through the fp64 epilogue; bound:
    em.elementwise_bound with A = sqrt(3 updates per slab and tap) for the fp32 accumulation and the bf16-split output's 2^-17.
    The reference itself is within layer_mx6_data.product_error_bound of the exact convolution (the grid's steps)."""
    check_element_bounds(env, cin, cout, K)


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


# ==================================================================================================================================
# K = 3, dilation, chunks around the halo's length, every epilogue form, the codec on its own, the tile's row edge, the dilated
# topology.  Row layout per case: layer_mx6_data.edge_layout (engine.BatchLayout with the layer's own gap (K - 1) / 2 dilation).
# ==================================================================================================================================
NEW_SHAPES = [(64, 256, 3, 1), (128, 256, 3, 2), (64, 512, 3, 3), (128, 256, 3, 4), (64, 256, 5, 2)]        # (cin, cout, K, dilation)
ALL_SHAPES = NEW_SHAPES + [(cin, cout, K, 1) for cin, cout, K in SHAPES]
_LAYOUTS = {}


def edge_valid(K, dil):
    if (K, dil) not in _LAYOUTS:
        _LAYOUTS[K, dil] = lx.edge_layout(K, dil)
    return _LAYOUTS[K, dil][0]


def test_the_edge_layouts_cannot_degenerate():
    """Every layout has rows with more than one missing tap (K > 3) or both outer taps missing, chunks shorter than the halo, and
    12 to 31 frames with a missing tap; the (K - 1) dilation = 8 shapes sit on the entry point's limit."""
    for cin, cout, K, dil in ALL_SHAPES:
        valid = edge_valid(K, dil)
        miss = lx.missing_taps(valid, K, dil)[valid != 0]
        assert 12 <= miss.any(1).sum() <= 31 and (miss.sum(1) > 1).any()
        assert (miss[:, :K // 2].any(1) & miss[:, K // 2 + 1:].any(1)).any()
        assert 296 <= len(valid) <= 320 and valid[250:260].all()          # a chunk across the 256-row tile boundary
    assert max((K - 1) * dil for _, _, K, dil in NEW_SHAPES) == 8


@pytest.mark.parametrize("cin,cout,K,dil", ALL_SHAPES)
def test_consumer_exact_answers_with_dilation_and_short_chunks(env, cin, cout, K, dil):
    """test_consumer_exact_answers_on_grid_data at K = 3 and at dilations 1 .. 4, on chunks of 1, 2, h, h + 1, 97, 3 and 150 frames."""
    hiplib = env["hiplib"]
    valid = edge_valid(K, dil)
    x, w, z, M, parts = exact_case(cin, cout, K, dil, valid)
    assert_exact(z, M, parts)
    y = z * (valid[:, None] != 0)
    got, got_c, status, _ = run_layer(env, x, w, "mx6", hiplib.FMT_SPLIT6, valid=valid, dilation=dil)
    want, want_c = lx.decode_rows(y)
    assert status == 0 and np.array_equal(got, want) and np.array_equal(got_c, want_c)
    assert not got[valid == 0].any() and not got_c[valid == 0].any()
    got8, _, status, _ = run_layer(env, x, w, "mx6", hiplib.FMT_SPLIT8, valid=valid, dilation=dil)
    assert status == 0 and np.array_equal(got8, em.decode8(y.astype(np.float32))) and not got8[valid == 0].any()


@pytest.mark.parametrize("cin,cout,K,dil", ALL_SHAPES)
def test_producer_writes_the_cpu_encoders_rows_with_dilation(env, cin, cout, K, dil):
    """test_producer_writes_the_cpu_encoders_rows at every (K, dilation): the centre tap of ones picks the row itself, whatever the
    other taps' rows hold; both planes of the 6-bit rows equal the CPU encoder's."""
    hiplib = env["hiplib"]
    valid = edge_valid(K, dil)
    x, w, Y = producer_case(cin, cout, K, valid, seed=300 + cin + K + 10 * dil)
    assert len(np.unique(lx.encode_rows(Y)[3][valid != 0])) >= 3
    want, want_c = lx.decode_rows(Y)
    assert (want != want_c).mean() > 0.2
    got, got_c, status, _ = run_layer(env, x, w, "bf8", hiplib.FMT_SPLIT6, valid=valid, dilation=dil)
    assert status == 0 and np.array_equal(got, want) and np.array_equal(got_c, want_c)
    assert not got[valid == 0].any() and not got_c[valid == 0].any()


def test_consumer_reads_the_rows_the_producer_stored(env):
    """The path of the dilated topology: a bf8 layer (128 -> 256, K = 3, dilation 2) writes 6-bit rows, an mx6 layer (256 -> 256, K = 3,
    dilation 3) reads that very buffer.  Exact data on both: the producer's outputs are grid values under per-block classes, the
    consumer's weights those of exact_case."""
    hiplib = env["hiplib"]
    valid = edge_valid(3, 3)                                        # one layout for both layers, its gap the larger halo
    x1, w1, Y = producer_case(128, 256, 3, valid, seed=77, classes=(1.0, 1.0, 4.0, 0.5))
    mid, mid_c, st, ybuf = run_layer(env, x1, w1, "bf8", hiplib.FMT_SPLIT6, valid=valid, dilation=2)
    want, want_c = lx.decode_rows(Y)
    assert st == 0 and np.array_equal(mid, want) and np.array_equal(mid_c, want_c)
    rng = np.random.default_rng(78)
    wcls = block_classes(rng, 3 * 256, 256, [1.0, 2.0]).reshape(3, 256, 256).transpose(0, 2, 1)
    w2 = grid_values(rng, (3, 256, 256), wcls, 12.0 / (3 * 256))
    z, M, parts = lx.contract(Y, w2, 3)
    assert_exact(z, M, parts)
    y = z * (valid[:, None] != 0)
    got, got_c, st, _ = run_layer(env, None, w2, "mx6", hiplib.FMT_SPLIT6, valid=valid, dilation=3, xbuf=ybuf)
    want, want_c = lx.decode_rows(y)
    assert st == 0 and np.array_equal(got, want) and np.array_equal(got_c, want_c)
    got8, _, st, _ = run_layer(env, None, w2, "mx6", hiplib.FMT_SPLIT8, valid=valid, dilation=3, xbuf=ybuf)
    assert st == 0 and np.array_equal(got8, em.decode8(y.astype(np.float32)))


@pytest.mark.parametrize("cin,cout,K,dil", [(64, 512, 3, 3), (64, 256, 5, 2)])
def test_tap_bias_at_chunk_edges_with_dilation(env, cin, cout, K, dil):
    """test_tap_bias_at_chunk_edges where a row misses several taps at once and taps on both sides (chunks shorter than the halo):
    the flag byte of gemm8_tap_flags holds them all."""
    hiplib = env["hiplib"]
    valid = edge_valid(K, dil)
    x, w, z, _, _ = exact_case(cin, cout, K, dil, valid)
    rng = np.random.default_rng(40 + K + dil)
    table = rng.integers(-3, 4, (K, cout)).astype(np.float32)
    bias = rng.integers(-3, 4, cout).astype(np.float32) + table.sum(0)
    miss = lx.missing_taps(valid, K, dil)
    mv = miss[valid != 0]
    assert (mv.sum(1) > 1).any() and (mv[:, :K // 2].any(1) & mv[:, K // 2 + 1:].any(1)).any() and not mv[:, K // 2].any()
    assert np.abs(table).sum(1).min() > 0                           # every tap's constants are live
    y = (z + bias - miss.astype(np.float64) @ table) * (valid[:, None] != 0)
    assert np.array_equal(y, y.astype(np.float32).astype(np.float64))
    got, got_c, st, _ = run_layer(env, x, w, "mx6", hiplib.FMT_SPLIT6, bias, tapbias=table, valid=valid, dilation=dil)
    want, want_c = lx.decode_rows(y)
    assert st == 0 and np.array_equal(got, want) and np.array_equal(got_c, want_c)
    # the bf8 producer's SPLIT6 epilogue applies the same table
    z8 = em.contract("f16bf8", x, w, dil)[0]
    y8 = (z8 + bias - miss.astype(np.float64) @ table) * (valid[:, None] != 0)
    assert np.array_equal(y8, y8.astype(np.float32).astype(np.float64))
    got, got_c, st, _ = run_layer(env, x, w, "bf8", hiplib.FMT_SPLIT6, bias, tapbias=table, valid=valid, dilation=dil)
    want, want_c = lx.decode_rows(y8)
    assert st == 0 and np.array_equal(got, want) and np.array_equal(got_c, want_c)


@pytest.mark.parametrize("cin,cout,K,dil", NEW_SHAPES)
def test_consumer_element_bounds_with_dilation(env, cin, cout, K, dil):
    """test_consumer_element_bounds_on_random_data, bound unchanged, at K = 3 and with dilation on the edge layout."""
    check_element_bounds(env, cin, cout, K, dil, edge_valid(K, dil))


def test_a_chunk_alone_gives_the_batchs_bits_at_dilation_3(env):
    hiplib = env["hiplib"]
    cin, cout, K, dil = 64, 512, 3, 3
    valid, starts, lens = lx.edge_layout(K, dil)
    x, w, b, s, o = random_case(cin, cout, K, dil, valid)
    batch, _, st, _ = run_layer(env, x, w, "mx6", hiplib.FMT_SPLIT8, b, s, o, "relu", valid=valid, dilation=dil)
    assert st == 0
    # the 150-frame chunk (across the tile boundary in the batch) and the 2- and 3-frame chunks (shorter than / equal to the halo)
    for c in (6, 1, 2):
        n, s0 = lens[c], starts[c]
        rows = (n + 3 + 7) // 8 * 8
        xa = np.zeros((rows, cin), np.float32)
        xa[:n] = x[s0:s0 + n]
        alone, _, st, _ = run_layer(env, xa, w, "mx6", hiplib.FMT_SPLIT8, b, s, o, "relu", valid=row_valid([0], [n], rows), dilation=dil)
        assert st == 0 and np.array_equal(alone[:n], batch[s0:s0 + n]) and np.abs(alone[:n]).sum() > 0 and not alone[n:].any()


# ---- epilogue forms --------------------------------------------------------------------------------------------------------------
def epilogue_params(cout, act, steep):
    """Integer bias in [-3, 3], scale from {1/2, 1, 2}, shift in halves in [-2, 2]; alpha 1/4 (LReLU), per channel 1/4 or 1/2 (PReLU);
    ``steep``: PReLU with 1/4 or 2 -- above 1 the LReLU form max(alpha z, z) is no longer the PReLU one, so a PReLU launch that takes
    the LReLU path shows."""
    rng = np.random.default_rng(50 + em.ACT[act] + 10 * steep)
    f = lambda a: np.asarray(a, np.float32)
    b, sc, sh = f(rng.integers(-3, 4, cout)), f(rng.choice([0.5, 1.0, 2.0], cout)), f(rng.integers(-4, 5, cout) / 2.0)
    alpha = {"lrelu": f([0.25]), "prelu": f(rng.choice([0.25, 2.0 if steep else 0.5], cout))}.get(act)
    assert alpha is None or act == "lrelu" or len(np.unique(alpha)) == 2
    return b, sc, sh, alpha


@pytest.mark.parametrize("act", ["relu", "lrelu", "prelu", "none", "prelu-steep"])
@pytest.mark.parametrize("cin,cout,K,dil", [(64, 256, 5, 1), (128, 256, 3, 2)])
def test_epilogue_forms_are_exact_in_six_bit_rows(env, cin, cout, K, dil, act):
    """activation, then scale / shift, then the encoder: the bf8 producer's 6-bit rows (wide_epilogue_split6, its three modes) and the
    mx6 consumer's 6- and 8-bit rows equal the CPU encoders of em.epilogue (fp64) of the exact pre-activation, bit for bit.  The
    parameters keep the fp64 answer an fp32; at least a fifth of the outputs are negative (the sign bits of both planes)."""
    hiplib = env["hiplib"]
    valid = VALID if dil == 1 else edge_valid(K, dil)
    x, w, z, M, parts = exact_case(cin, cout, K, dil, valid)
    assert_exact(z, M, parts)
    act, steep = act.split("-")[0], act.endswith("-steep")
    b, sc, sh, alpha = epilogue_params(cout, act, steep)
    kw = dict(valid=valid, dilation=dil, alpha=alpha)
    for form, zz in (("mx6", z), ("bf8", em.contract("f16bf8", x, w, dil)[0])):
        y = em.epilogue(zz, b, sc, sh, act, alpha) * (valid[:, None] != 0)
        assert np.array_equal(y, y.astype(np.float32).astype(np.float64)) and (y[valid != 0] < 0).mean() >= 0.2
        want, want_c = lx.decode_rows(y)
        got, got_c, st, _ = run_layer(env, x, w, form, hiplib.FMT_SPLIT6, b, sc, sh, act, **kw)
        assert st == 0 and np.array_equal(got, want) and np.array_equal(got_c, want_c), (form, act)
        assert not got[valid == 0].any() and not got_c[valid == 0].any()
        if form == "mx6":
            got8, _, st, _ = run_layer(env, x, w, form, hiplib.FMT_SPLIT8, b, sc, sh, act, **kw)
            assert st == 0 and np.array_equal(got8, em.decode8(y.astype(np.float32)))


# ---- the encoder, the decoder and the weight pack on their own -----------------------------------------------------------------------
def stored_scale_byte(env, buf, r, block):
    """The scale byte of (row r, 16-channel block) read from the raw buffer: slot 6 + (block & 1) of the row's 128-byte slab block >> 1,
    its third dword's low byte; the slots of a row are swizzled by (r >> 1) & 7 (include/xvector_hip.h)."""
    off = (env["hiplib"].SPLIT_PAD_BEFORE + r) * buf.row_bytes + (block >> 1) * 128 + (((6 + (block & 1)) ^ ((r >> 1) & 7)) << 4) + 8
    return int(buf.base[off].item())


def encode_decode(env, x):
    torch, hiplib, dev = env["torch"], env["hiplib"], env["dev"]
    n, C = x.shape
    buf = hiplib.SplitBuf(n, C, dev, hiplib.FMT_SPLIT6)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    hiplib.split_encode(dev_t(env, x), buf, status=status)
    cq = torch.full((n, C), 7.0, dtype=torch.float32, device=dev)
    out = hiplib.split_decode(buf, n, cq=cq)
    torch.cuda.synchronize()
    return out.cpu().numpy(), cq.cpu().numpy(), int(status.item()), buf


def test_encoder_and_decoder_on_hostile_rows(env):
    """xv_split6_encode_f32 / xv_split6_decode_f32 against layer_mx6_data.decode_rows, both planes bit for bit, on rows built to sit on
    the encoder's edges (layer_mx6_data.hostile_blocks): block maxima at 1.875 2^e and the fp32 on either side, every tie of the e2m3
    grid in both halves and all three step sizes, values below half the first step, denormals (the byte's floor), zeros, -0.0, fp16's
    subnormal range, the clamp at 57344.  The status word is set exactly when a magnitude exceeds 57344; the stored scale bytes of
    chosen blocks are read from the raw buffer (a decode alone would accept a byte and elements wrong in compensating ways).  NaN is
    outside the format's contract and is not in the rows."""
    rows, n_in, where = lx.hostile_rows()
    assert not np.isnan(rows).any() and np.isinf(rows[n_in:]).any()
    for x, flag in ((rows[:n_in], 0), (rows, 1)):
        got, got_c, st, buf = encode_decode(env, x)
        want, want_c = lx.decode_rows(x)
        bad = np.argwhere((got != want) | (got_c != want_c))
        assert not len(bad), (len(bad), [(int(r), int(c), float(x[r, c]), float(got[r, c]), float(want[r, c]), float(got_c[r, c]),
                                          float(want_c[r, c])) for r, c in bad[:6]])
        assert st == flag
    k = lx.encode_rows(rows)[3]
    seen = {}
    for tag in ("1e-38", "zeros", "edge at 3", "edge above 3", "edge below 3", "tiny lo ties j -40", "57344", "beyond:inf"):
        r, b = where[tag]
        seen[tag] = stored_scale_byte(env, buf, r, b)
        assert seen[tag] == int(lx.stored_byte(k[r, b])), (tag, seen[tag], int(lx.stored_byte(k[r, b])))
    assert seen["1e-38"] == 5 and seen["zeros"] == 116 and (seen["edge at 3"], seen["edge above 3"]) == (117, 118)
    print("SPLIT6 codec on %d hostile rows (%d beyond the clamp): equal to the CPU encoder; scale bytes %r" % (len(rows), len(rows) - n_in, seen))


def test_encoder_on_a_partly_empty_slab(env):
    """C = 40: the third block holds 8 channels, the fourth none; the reference is padded with zeros to 48 channels."""
    rows, n_in, _ = lx.hostile_rows()
    x = np.ascontiguousarray(np.concatenate([rows[:n_in, 8:40], rows[:n_in, 56:64]], 1))
    ref = np.zeros((n_in, 48), np.float32)
    ref[:, :40] = x
    got, got_c, st, buf = encode_decode(env, x)
    want, want_c = lx.decode_rows(ref)
    assert st == 0 and np.array_equal(got, want[:, :40]) and np.array_equal(got_c, want_c[:, :40]) and np.abs(got[:, 32:]).sum() > 0
    k = lx.encode_rows(ref)[3]
    for r in (0, 7, n_in - 1):
        assert stored_scale_byte(env, buf, r, 2) == int(lx.stored_byte(k[r, 2])) and stored_scale_byte(env, buf, r, 3) == 116


def hostile_weights():
    """w [3, 64, 256]: channels 0 .. 31 hold hostile blocks (the 1.875 boundary, ties of both halves, small values; fp16-normal
    magnitudes) scattered over (tap, block, column) among plain values, with a column whose blocks are zero; channels 32 .. 63 hold
    the fp16 hi of channels 0 .. 31 (their own lo' is 0)."""
    rng = np.random.default_rng(9)
    w = (rng.choice([-1.0, 1.0], (3, 64, 256)) * rng.uniform(0.01, 1.0, (3, 64, 256)) * np.ldexp(1.0, rng.integers(-3, 4, (3, 1, 256)))).astype(np.float32)
    blocks = lx.hostile_blocks(e_range=range(-8, 13), tiny=False, beyond=False)
    for i, (_, b) in enumerate(blocks):
        tap, blk, col = np.unravel_index((13 * i + 5) % (3 * 2 * 256), (3, 2, 256))
        w[tap, 16 * blk:16 * blk + 16, col] = b
    w[:, :, 100] = 0
    w[1, 16:32, 7] = 0
    w[:, 32:] = np.clip(w[:, :32], -em.SPLIT8_MAX, em.SPLIT8_MAX).astype(np.float16).astype(np.float32)
    return w, len(blocks)


def test_weight_pack_value_by_value(env):
    """pack_weights_f16mx6_kernel read back through the layer, plane by plane, exactly.  Input rows are one-hot (row 3 i + 1 holds
    channel i; output row 3 i + 2 - t then holds tap t of that channel for every column):
      pass 1, x = 1.0 (its block's scale holds 1.0 exactly, lo' = 0): the output is wh + 2^-11 lo_q(w) -- the fp16 plane and the
              lo' half, read through bf16-split rows (the fp32 answer through em.decode3);
      pass 2, x = 2^-30 (hi = 0, lo' = 2^-19 sets the scale, c rounds to 0): the output is 2^-30 c_q(w) -- the c half alone, exact;
      pass 3, x = 1.0 in channel i and -1.0 in channel 32 + i, whose weight is fp16(w[i]): the fp16 products cancel and the output
              is 2^-11 lo_q(w) -- the lo' half alone, exact.
    Reference: layer_mx6_data.contract, with the identities to weight_planes asserted here."""
    hiplib = env["hiplib"]
    w, nblocks = hostile_weights()
    wh, wl, wc = lx.weight_planes(w)
    assert nblocks > 100 and not wl[:, 32:].any() and np.array_equal(wh[:, 32:], wh[:, :32])
    assert (np.abs(wl[:, :32]) > 0).mean() > 0.5 and (wc != w).mean() > 0.5

    def one_hot(channels, value, mirror):
        rows = 3 * len(channels) + 2
        x = np.zeros((rows, 64), np.float32)
        for i, c in enumerate(channels):
            x[3 * i + 1, c] = value
            if mirror:
                x[3 * i + 1, 32 + c] = -value
        return x, np.ones(rows, np.uint8)

    def taps_of(z, channels):                              # [3, len(channels), 256]: tap t of channel i from row 3 i + 2 - t
        return np.stack([z[3 * np.arange(len(channels)) + 2 - t] for t in range(3)])

    for name, channels, value, mirror, plane in (("hi + lo'", range(64), 1.0, False, wh + wl / em.LO_SCALE),
                                                 ("c", range(64), 2.0 ** -30, False, 2.0 ** -30 * wc),
                                                 ("lo'", range(32), 1.0, True, wl[:, :32] / em.LO_SCALE)):
        x, valid = one_hot(list(channels), value, mirror)
        z = lx.contract(x, w)[0]
        assert np.array_equal(taps_of(z, channels), plane) and np.array_equal(z, z.astype(np.float32).astype(np.float64)), name
        got, _, st, _ = run_layer(env, x, w, "mx6", hiplib.FMT_SPLIT, valid=valid)
        want = em.decode3(z.astype(np.float32))
        if name != "hi + lo'":
            assert np.array_equal(want, z.astype(np.float32))                          # four significant bits: the rows hold it exactly
        bad = np.argwhere(got != want)
        assert st == 0 and not len(bad), (name, len(bad), [(int(r), int(c), float(got[r, c]), float(want[r, c])) for r, c in bad[:6]])


# ---- the row edge of the tile ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [256, 257])
def test_row_counts_at_the_tile_edge(env, rows):
    """R = 256 (no partial tile) and R = 257 (a second tile of one row, whose taps reach back into the first), the last chunk running
    up to the buffer's end: consumer and producer exact; the rows of the last tile past R decode to zero."""
    torch, hiplib = env["torch"], env["hiplib"]
    cin, cout, K = 64, 256, 5
    valid = row_valid([0, 104, 208], [101, 101, rows - 208], rows)
    assert valid[-1] == 1 and valid[255] == 1
    x, w, z, M, parts = exact_case(cin, cout, K, 1, valid)
    assert_exact(z, M, parts)
    got, got_c, st, ybuf = run_layer(env, x, w, "mx6", hiplib.FMT_SPLIT6, valid=valid)
    want, want_c = lx.decode_rows(z * (valid[:, None] != 0))
    assert st == 0 and np.array_equal(got, want) and np.array_equal(got_c, want_c) and np.abs(want[-1]).sum() > 0
    got8, _, st, ybuf8 = run_layer(env, x, w, "mx6", hiplib.FMT_SPLIT8, valid=valid)
    assert st == 0 and np.array_equal(got8, em.decode8((z * (valid[:, None] != 0)).astype(np.float32)))
    xp, wp, Y = producer_case(cin, cout, K, valid, seed=500 + rows)
    gotp, gotp_c, st, pbuf = run_layer(env, xp, wp, "bf8", hiplib.FMT_SPLIT6, valid=valid)
    wantp, wantp_c = lx.decode_rows(Y)
    assert st == 0 and np.array_equal(gotp, wantp) and np.array_equal(gotp_c, wantp_c) and np.abs(wantp[-1]).sum() > 0
    for buf in (ybuf, pbuf, ybuf8):
        six = buf.fmt == hiplib.FMT_SPLIT6
        tail_c = torch.zeros((rows + 250, cout), dtype=torch.float32, device=env["dev"]) if six else None
        tail = hiplib.split_decode(buf, rows + 250, cq=tail_c)
        assert not tail[rows:].any().item() and (tail_c is None or not tail_c[rows:].any().item())


# ---- the topology that runs K = 3 with dilation --------------------------------------------------------------------------------------
def test_dilated_network_with_and_without_the_mx6_layer(env):
    """ModelWithoutDropoutTdnn (kernel sizes 5, 3, 3, 1, 1; dilations 1, 2, 3, 1, 1): layer 1 (K = 3, dilation 2) writes the 6-bit rows
    and layer 2 (K = 3, dilation 3) reads them -- mx6_layers is {2}, asserted so that a change of the selection rule cannot leave this
    test believing it covers them.  Both forms under 1e-4 against the fp64 oracle and within 2e-4 of each other, as
    test_whole_network_with_and_without_the_mx6_layer holds the default topology."""
    engine, oracle = env["engine"], env["oracle"]
    topo = env["topology"].get("ModelWithoutDropoutTdnn")
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
    between = max(oracle.rel_l2(a, b) for a, b in zip(out[True], out[False]))
    print("dilated topology, x-vectors against the fp64 oracle, worst of three: mx6 layer %.3e, bf8 layer %.3e (ratio %.3f); between the "
          "two forms %.3e" % (errs[True], errs[False], errs[True] / errs[False], between))
    assert errs[True] < 1e-4 and errs[False] < 1e-4, errs
    assert between < 2e-4
