"""GPU parity tests of the f16bf8 arithmetic (xv_gemm8.hip, xv_gemm8_wide.hip, xv_gemm8_wide16.hip, xv_split8.h) through the C ABI against the fp64 oracle.

A product is xh*wh + 2^-11 (xl8*wh8 + xh8*wl8): one fp16 MFMA + one block-scaled bf8 MFMA instead of three bf16 MFMAs.
Per layer the result is good to ~1e-5 relative L2 (bf16x3: ~3e-6); the tolerance here is 4e-5, the north star's bar for
the whole network is 1e-4 (checked in test_gpu_forward.py for this precision as for the others).
"""
import numpy as np
import pytest

import arith_emul as em

pytestmark = pytest.mark.gpu

TOL_GEMM8 = 4e-5
CODE = {"none": 0, "relu": 1, "lrelu": 2, "prelu": 3}


@pytest.fixture(scope="module")
def env(oracle_mod):
    import torch
    from xvector_amd import engine, hiplib
    hiplib.require_gpu()
    return dict(torch=torch, hiplib=hiplib, engine=engine, oracle=oracle_mod, dev=torch.device("cuda:0"))


def _rand_bn(rng, c):
    return ((1 + 0.1 * rng.standard_normal(c)).astype(np.float32), (0.1 * rng.standard_normal(c)).astype(np.float32),
            (0.2 * rng.standard_normal(c)).astype(np.float32), np.exp(0.2 * rng.standard_normal(c)).astype(np.float32))


def _alpha(rng, act, cout):
    if act == "lrelu":
        return np.array([0.2], np.float32)
    if act == "prelu":
        return (0.1 + 0.05 * rng.standard_normal(cout)).astype(np.float32)
    return None


def test_split8_roundtrip_layout_and_overflow_flag(env):
    torch, hiplib, dev = env["torch"], env["hiplib"], env["dev"]
    rng = np.random.default_rng(0)
    R, C = 77, 80                                   # ragged last slab
    x = (rng.standard_normal((R, C)) * np.exp(1.5 * rng.standard_normal((R, C)))).astype(np.float32)   # |x| up to ~1e3
    x[3, 5] = 0.0
    x[4, 6] = 1e-7                                  # below fp16's normal range: kept to an absolute 2^-25
    x[5, :14] = [1 + 2 ** -11, 1 + 3 * 2 ** -11, -1 - 3 * 2 ** -11, 2 ** -24, 2 ** -25, 1.5 * 2 ** -14, 6e-5, 3e-6, 1.375, 1.125,
                 2 ** -17, 3 * 2 ** -17, 0.0, -0.0]          # fp16 / e5m2 ties, fp16 and e5m2 subnormals, zeros
    xd = torch.from_numpy(x).to(dev)
    buf = hiplib.SplitBuf(R, C, dev, hiplib.FMT_SPLIT8)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    hiplib.split_encode(xd, buf, status=status)
    back = hiplib.split_decode(buf, R).cpu().numpy()
    assert int(status.item()) == 0
    err = np.abs(back - x)
    assert (err <= np.maximum(np.abs(x) * 2.0 ** -13, 2.0 ** -24)).all()
    # bytes: slot g of a row-slab = fp16 hi of channels 8g..8g+7, physical slot = logical ^ ((row >> 1) & 7)
    raw = buf.base.cpu().numpy()[hiplib.SPLIT_PAD_BEFORE * buf.row_bytes:].reshape(-1, buf.row_bytes)
    r, c = 10, 37
    slab, g, e = c // 32, (c % 32) // 8, c % 8
    sw = (r >> 1) & 7
    hi = raw[r, slab * 128 + ((g ^ sw) << 4):][:16].view(np.float16)[e]
    assert hi == np.float16(x[r, c])
    cross = raw[r, slab * 128 + (((4 + g) ^ sw) << 4):][:16]
    h8 = (cross[8 + e:9 + e].astype(np.uint16) << 8).view(np.float16)[0]              # e5m2 = the upper byte of an fp16
    assert abs(float(h8) - x[r, c]) <= abs(x[r, c]) * 0.125
    l8 = (cross[e:e + 1].astype(np.uint16) << 8).view(np.float16)[0]
    assert abs(float(hi) + float(l8) / 2048 - x[r, c]) <= abs(x[r, c]) * 2.0 ** -13
    _split8_bytes_are_the_emulators(raw, x, R, C)
    # the padding channels of the last slab (80..95: groups 2 and 3 of slab 2) are zeros
    for r in range(R):
        sw = (r >> 1) & 7
        for slot in (2, 3, 6, 7):
            assert not raw[r, 2 * 128 + ((slot ^ sw) << 4):][:16].any()
    # range: |v| > 57344 clamps and raises the flag
    x[7, 7] = 1e6
    x[8, 1] = -7e4
    hiplib.split_encode(torch.from_numpy(x).to(dev), buf, status=status)
    back = hiplib.split_decode(buf, R).cpu().numpy()
    assert int(status.item()) == 1 and back[7, 7] == 57344.0 and back[8, 1] == -57344.0
    _split8_bytes_are_the_emulators(buf.base.cpu().numpy()[hiplib.SPLIT_PAD_BEFORE * buf.row_bytes:].reshape(-1, buf.row_bytes), x, R, C)


def _split8_bytes_are_the_emulators(raw, x, R, C):
    """Every byte of a split8 buffer (fp16 hi, l8, h8 of every element) against tests/arith_emul.py."""
    hi, l8, h8 = em.split8_bytes(x)
    r, c = np.arange(R)[:, None], np.arange(C)[None, :]
    slab, g, e = c // 32, (c % 32) // 8, c % 8
    sw = (r >> 1) & 7
    rows = np.broadcast_to(r, (R, C))
    hoff = slab * 128 + ((g ^ sw) << 4) + 2 * e
    got_hi = raw[rows, hoff].astype(np.uint16) | (raw[rows, hoff + 1].astype(np.uint16) << 8)
    xoff = slab * 128 + (((4 + g) ^ sw) << 4) + e
    assert np.array_equal(got_hi, hi)
    assert np.array_equal(raw[rows, xoff], l8)
    assert np.array_equal(raw[rows, xoff + 8], h8)


@pytest.mark.parametrize("tile_rows", [128, 256, 512, 1024])      # 512 / 1024 = the 256 x 256 tile on the 32 x 32 / 16 x 16 MFMA shapes
                                                                  # where the shape allows it, else the built-in choice
@pytest.mark.parametrize("cin,cout,K,dil,act,yfmt", [
    (512, 512, 5, 1, "relu", "split8"),       # layer 1 of the default topology
    (512, 512, 7, 1, "relu", "split"),        # layer 2, feeding the bf16x3 pair kernel
    (512, 512, 1, 1, "relu", "split8"),
    (512, 1536, 1, 1, "lrelu", "f32"),
    (512, 512, 3, 3, "relu", "split8"),       # dilated
    (512, 512, 3, 2, "prelu", "split"),
    (64, 48, 5, 1, "prelu", "split8"),        # ragged Cout: the general epilogue
    (40, 200, 3, 2, "lrelu", "f32"),          # Cin not a multiple of 32
    (96, 128, 7, 1, "none", "split8"),
])
def test_tdnn_layer_f16bf8_matches_oracle(env, cin, cout, K, dil, act, yfmt, tile_rows):
    torch, hiplib, engine, oracle, dev = env["torch"], env["hiplib"], env["engine"], env["oracle"], env["dev"]
    rng = np.random.default_rng(cin * 1000 + cout + K * 7 + dil + 2)
    lens = [25, 1, 130, 257, 64, 3, 700]
    mats = [(rng.standard_normal((t, cin)) * 2).astype(np.float32) for t in lens]
    w = (rng.standard_normal((K, cin, cout)) / np.sqrt(K * cin)).astype(np.float32)
    b = (0.1 * rng.standard_normal(cout)).astype(np.float32)
    bn = _rand_bn(rng, cout)
    alpha = _alpha(rng, act, cout)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    gap = max(1, (K - 1) * dil // 2)
    scale, shift = hiplib.fold_bn(*(t(a) for a in bn), 1e-3)
    wp = hiplib.pack_weights_f16bf8(t(w))
    assert wp.wt.numel() == hiplib.pack_weights_bf16x3(t(w)).wt.numel()

    def run(ms):
        layout = engine.BatchLayout([m.shape[0] for m in ms], gap)
        host = np.zeros((layout.rows, cin), np.float32)
        layout.pack(ms, host)
        xin = hiplib.SplitBuf(layout.rows, cin, dev, hiplib.FMT_SPLIT8)
        hiplib.split_encode(t(host), xin)
        rv = t(layout.row_valid())
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        if yfmt == "f32":
            y = torch.full((layout.rows, cout), float("nan"), dtype=torch.float32, device=dev)
        else:
            y = hiplib.SplitBuf(layout.rows, cout, dev, hiplib.FMT_SPLIT8 if yfmt == "split8" else hiplib.FMT_SPLIT)
            y.base.fill_(0x7b)                     # poison: fp16 0x7b7b = 61280, bf16 0x7b7b = 1.3e36
        hiplib.tdnn_layer8(xin, layout.rows, wp, t(b), scale, shift, CODE[act], t(alpha), dil, rv, y, status)
        yh = (y if yfmt == "f32" else hiplib.split_decode(y, layout.rows)).cpu().numpy()
        assert int(status.item()) == 0
        return [yh[s:s + n] for s, n in zip(layout.row_start, layout.row_len)], yh, layout

    hiplib.set_tuning(hiplib.TUNE_TILE_ROWS, tile_rows)
    try:
        outs, yh, layout = run(mats)
        alone, _, _ = run([mats[3]])
    finally:
        hiplib.set_tuning(hiplib.TUNE_TILE_ROWS, 0)
    for m, got in zip(mats, outs):
        ref = oracle.tdnn_layer(m, w, b, bn, act, alpha, dil, np.float64)
        assert np.isfinite(got).all()
        assert oracle.rel_l2(got, ref) < TOL_GEMM8, (m.shape[0], oracle.rel_l2(got, ref))
    assert (yh[~layout.row_valid().astype(bool)] == 0).all()          # gap rows: exact zeros
    assert np.array_equal(alone[0], outs[3])                            # batch composition does not change a result


def test_f16bf8_tile_heights_agree_bitwise(env):
    """128 x 128, 256 x 128 and 256 x 256 workgroup tiles accumulate every output element in the same order."""
    torch, hiplib, dev = env["torch"], env["hiplib"], env["dev"]
    rng = np.random.default_rng(5)
    R, cin, cout, K = 3000, 512, 512, 5
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    x = hiplib.SplitBuf(R, cin, dev, hiplib.FMT_SPLIT8)
    hiplib.split_encode(t(rng.standard_normal((R, cin)).astype(np.float32)), x)
    wp = hiplib.pack_weights_f16bf8(t((rng.standard_normal((K, cin, cout)) / 50).astype(np.float32)))
    outs = []
    for rows in (128, 256, 512):
        hiplib.set_tuning(hiplib.TUNE_TILE_ROWS, rows)
        try:
            y = hiplib.SplitBuf(R, cout, dev, hiplib.FMT_SPLIT8)
            hiplib.tdnn_layer8(x, R, wp, None, None, None, 1, None, 1, None, y)
            outs.append(y.base.cpu().numpy().copy())
        finally:
            hiplib.set_tuning(hiplib.TUNE_TILE_ROWS, 0)
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])


@pytest.mark.parametrize("K,dil", [(5, 1), (7, 1), (3, 1), (3, 3), (3, 4)])
def test_f16bf8_16x16_form_agrees_with_the_32x32_form(env, K, dil):
    """The 256 x 256 tile on v_mfma_f32_16x16x32_f16 + v_mfma_scale_f32_16x16x128_f8f6f4 (tap pairs) forms the same products as
    the 32 x 32 form and adds them in another order: equal to fp32 rounding, not bit for bit; several row and column tiles, a
    ragged last row tile, gap rows."""
    torch, hiplib, dev = env["torch"], env["hiplib"], env["dev"]
    rng = np.random.default_rng(50 + K + dil)
    R, cin, cout = 1500, 512, 512
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    x = hiplib.SplitBuf(R, cin, dev, hiplib.FMT_SPLIT8)
    hiplib.split_encode(t(rng.standard_normal((R, cin)).astype(np.float32)), x)
    wp = hiplib.pack_weights_f16bf8(t((rng.standard_normal((K, cin, cout)) / 50).astype(np.float32)))
    valid = np.ones(R, np.uint8)
    valid[700:704] = 0
    outs = []
    for rows in (512, 1024):
        hiplib.set_tuning(hiplib.TUNE_TILE_ROWS, rows)
        try:
            y = hiplib.SplitBuf(R, cout, dev, hiplib.FMT_SPLIT8)
            hiplib.tdnn_layer8(x, R, wp, None, None, None, 1, None, dil, t(valid), y)
            outs.append(hiplib.split_decode(y, R).cpu().numpy().astype(np.float64))
        finally:
            hiplib.set_tuning(hiplib.TUNE_TILE_ROWS, 0)
    assert np.abs(outs[0]).max() > 0.5
    assert np.linalg.norm(outs[0] - outs[1]) / np.linalg.norm(outs[0]) < 5e-6       # (measured 2.2e-6 ... 2.4e-6)
    assert (outs[1][700:704] == 0).all()


def test_f16bf8_overflow_sets_the_status_word(env):
    torch, hiplib, dev = env["torch"], env["hiplib"], env["dev"]
    R, cin, cout = 300, 64, 128
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    x = hiplib.SplitBuf(R, cin, dev, hiplib.FMT_SPLIT8)
    hiplib.split_encode(t(np.full((R, cin), 100.0, np.float32)), x)
    w = np.zeros((1, cin, cout), np.float32)
    w[0, :, 0] = 1.0                                 # column 0: 6400 -- fine; with bn scale 10: 64000 > 57344
    wp = hiplib.pack_weights_f16bf8(t(w))
    scale = t(np.full(cout, 10.0, np.float32))
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    y = hiplib.SplitBuf(R, cout, dev, hiplib.FMT_SPLIT8)
    hiplib.tdnn_layer8(x, R, wp, None, scale, None, 1, None, 1, None, y, status)
    got = hiplib.split_decode(y, R).cpu().numpy()
    assert int(status.item()) == 1 and (got[:, 0] == 57344.0).all() and (got[:, 1:] == 0).all()
    # the same values into fp32 rows or the bf16 split format: no clamp, no flag
    status.zero_()
    y32 = torch.empty((R, cout), dtype=torch.float32, device=dev)
    hiplib.tdnn_layer8(x, R, wp, None, scale, None, 1, None, 1, None, y32, status)
    assert int(status.item()) == 0 and (y32[:, 0] == 64000.0).all()


@pytest.mark.parametrize("cin,cout,K,dil,act,lens,tile_rows", [
    (512, 1536, 1, 1, "relu", [25, 1, 7, 8, 9, 130, 257, 1000], 0),
    (64, 200, 3, 1, "prelu", [300, 25, 64], 0),
    (40, 48, 5, 2, "lrelu", [1200, 33], 0),
    (96, 512, 3, 1, "relu", [25, 1, 7, 8, 9, 130, 257, 1000], 512),      # the 256 x 256 tile with the POOL epilogue
    (64, 256, 5, 1, "prelu", [300, 25, 64], 512),
    (64, 256, 5, 1, "prelu", [300, 25, 64], 1024),                         # ... and on the 16 x 16 MFMA shapes (an even number of slabs)
    (128, 512, 7, 1, "relu", [25, 1, 7, 8, 9, 130, 257, 1000], 1024),
    (64, 256, 3, 2, "lrelu", [300, 25, 64], 1024),
])
def test_tdnn_layer_pool_f16bf8_blocks_match_oracle(env, cin, cout, K, dil, act, lens, tile_rows):
    torch, hiplib, engine, oracle, dev = env["torch"], env["hiplib"], env["engine"], env["oracle"], env["dev"]
    rng = np.random.default_rng(cin + cout + K + len(lens) + 1)
    mats = [(rng.standard_normal((n, cin)) * 2).astype(np.float32) for n in lens]
    w = (rng.standard_normal((K, cin, cout)) / np.sqrt(K * cin)).astype(np.float32)
    b = (0.1 * rng.standard_normal(cout)).astype(np.float32)
    bn = _rand_bn(rng, cout)
    alpha = _alpha(rng, act, cout)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    layout = engine.BatchLayout(lens, max(1, (K - 1) * dil // 2), hiplib.POOL_BLOCK_ROWS)
    host = np.zeros((layout.rows, cin), np.float32)
    layout.pack(mats, host)
    xin = hiplib.SplitBuf(layout.rows, cin, dev, hiplib.FMT_SPLIT8)
    hiplib.split_encode(t(host), xin)
    scale, shift = hiplib.fold_bn(*(t(a) for a in bn), 1e-3)
    blk = torch.full((hiplib.block_stats_floats(layout.rows, cout),), float("nan"), dtype=torch.float32, device=dev)
    hiplib.set_tuning(hiplib.TUNE_TILE_ROWS, tile_rows)
    try:
        hiplib.tdnn_layer_pool8(xin, layout.rows, hiplib.pack_weights_f16bf8(t(w)), t(b), scale, shift, CODE[act], t(alpha), dil,
                                t(layout.row_valid()), blk)
    finally:
        hiplib.set_tuning(hiplib.TUNE_TILE_ROWS, 0)
    out = torch.full((len(lens), 2 * cout), float("nan"), dtype=torch.float32, device=dev)
    hiplib.stats_pool_blocks(blk, cout, t(layout.row_start), t(layout.row_len), len(lens), 1e-5, out)
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    for i, m in enumerate(mats):
        ref = oracle.stats_pool(oracle.tdnn_layer(m, w, b, bn, act, alpha, dil, np.float64), 1e-5, np.float64)
        assert oracle.rel_l2(got[i, :cout], ref[:cout]) < TOL_GEMM8, (i, lens[i])
        assert oracle.rel_l2(got[i, cout:], ref[cout:]) < TOL_GEMM8, (i, lens[i])


def test_first_layer_kernel_writes_split8(env):
    """xv_tdnn_first_f16bf8 = xv_tdnn_first_bf16x3 with the other output encoding: same values to the encoding's precision."""
    torch, hiplib, engine, oracle, dev = env["torch"], env["hiplib"], env["engine"], env["oracle"], env["dev"]
    rng = np.random.default_rng(11)
    feat, in_dim, cout, K = 23, 24, 512, 5
    lens = [25, 1, 130, 600, 3]
    mats = [(rng.standard_normal((n, feat)) * 3).astype(np.float32) for n in lens]
    w = np.zeros((K, in_dim, cout), np.float32)
    w[:, :feat] = rng.standard_normal((K, feat, cout)) / np.sqrt(K * feat)
    b = (0.1 * rng.standard_normal(cout)).astype(np.float32)
    bn = _rand_bn(rng, cout)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    layout = engine.BatchLayout(lens, 2, 8)
    host = np.zeros((layout.rows, in_dim), np.float32)
    layout.pack(mats, host)
    scale, shift = hiplib.fold_bn(*(t(a) for a in bn), 1e-3)
    first = hiplib.pack_first_bf16x3(t(w))
    rv = t(layout.row_valid())
    y3 = hiplib.SplitBuf(layout.rows, cout, dev)
    hiplib.tdnn_first(t(host), layout.rows, first, t(b), scale, shift, 1, None, 1, rv, y3)
    y8 = hiplib.SplitBuf(layout.rows, cout, dev, hiplib.FMT_SPLIT8)
    y8.base.fill_(0x7b)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    hiplib.tdnn_first(t(host), layout.rows, first, t(b), scale, shift, 1, None, 1, rv, y8, status)
    a, c = hiplib.split_decode(y3, layout.rows).cpu().numpy(), hiplib.split_decode(y8, layout.rows).cpu().numpy()
    assert int(status.item()) == 0 and np.isfinite(c).all()
    assert (np.abs(a - c) <= np.maximum(np.abs(a) * 2.0 ** -13, 2.0 ** -24)).all()
    assert (c[~layout.row_valid().astype(bool)] == 0).all()
    for i, m in enumerate(mats):
        s = int(layout.row_start[i])
        assert oracle.rel_l2(c[s:s + lens[i]], oracle.tdnn_layer(m, w[:, :feat], b, bn, "relu", None, 1, np.float64)) < TOL_GEMM8


def test_f16bf8_bad_arguments_fail_loudly(env):
    torch, hiplib, dev = env["torch"], env["hiplib"], env["dev"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    x8 = hiplib.SplitBuf(64, 64, dev, hiplib.FMT_SPLIT8)
    x3 = hiplib.SplitBuf(64, 64, dev)
    y = torch.empty((64, 32), dtype=torch.float32, device=dev)
    w9 = hiplib.pack_weights_f16bf8(t(np.zeros((9, 64, 32), np.float32)))
    with pytest.raises(hiplib.XvectorHipError, match="K in"):
        hiplib.tdnn_layer8(x8, 64, w9, None, None, None, 1, None, 1, None, y)
    w5 = hiplib.pack_weights_f16bf8(t(np.zeros((5, 64, 32), np.float32)))
    with pytest.raises(hiplib.XvectorHipError, match="dilation"):
        hiplib.tdnn_layer8(x8, 64, w5, None, None, None, 1, None, 3, None, y)
    with pytest.raises(AssertionError):
        hiplib.tdnn_layer8(x3, 64, w5, None, None, None, 1, None, 1, None, y)          # bf16 split input
    with pytest.raises(hiplib.XvectorHipError, match="act_alpha"):
        hiplib.tdnn_layer8(x8, 64, w5, None, None, None, 3, None, 1, None, y)
    assert hiplib.f16bf8_supported(5, 1) and hiplib.f16bf8_supported(3, 3) and hiplib.f16bf8_supported(1, 1)
    assert not hiplib.f16bf8_supported(9, 1) and not hiplib.f16bf8_supported(5, 3) and not hiplib.f16bf8_supported(4, 1)


@pytest.mark.parametrize("cin,cout,act,lens", [
    (512, 1536, "relu", [25, 1, 7, 8, 9, 130, 257, 1000]),      # layers 3 + 4 of the default topology
    (64, 64, "prelu", [300, 25, 64, 3]),                         # two slabs, one column group
    (96, 192, "lrelu", [1200, 33]),                              # long chunk: many blocks per chunk
    (512, 1536, "none", [40, 129]),
])
def test_tdnn_pair_pool_f16bf8_matches_oracle(env, cin, cout, act, lens):
    """xv_tdnn_pair_pool_f16bf8 (two K = 1 layers, the intermediate split over a pair of waves and kept in registers, pooling
    block statistics) + xv_stats_pool_blocks_f32 == statistics pooling of layer(layer(x)) in the fp64 oracle; the block
    statistics agree with the two-launch f16bf8 path; a chunk's result does not depend on its batch neighbours.  The element-level
    guarantees (exact answers and per-block bounds on data with live low planes) live in tests/test_gpu_pair_elementwise.py."""
    torch, hiplib, engine, oracle, dev = env["torch"], env["hiplib"], env["engine"], env["oracle"], env["dev"]
    cmid = 512
    assert hiplib.pair8_supported(cin, cmid, cout) and not hiplib.pair8_supported(cin, 256, cout) and not hiplib.pair8_supported(40, cmid, cout)
    rng = np.random.default_rng(cin + cout + len(lens) + 3)
    mats = [(rng.standard_normal((n, cin)) * 2).astype(np.float32) for n in lens]
    w1 = (rng.standard_normal((1, cin, cmid)) / np.sqrt(cin)).astype(np.float32)
    w2 = (rng.standard_normal((1, cmid, cout)) / np.sqrt(cmid)).astype(np.float32)
    b1 = (0.1 * rng.standard_normal(cmid)).astype(np.float32)
    b2 = (0.1 * rng.standard_normal(cout)).astype(np.float32)
    bn1, bn2 = _rand_bn(rng, cmid), _rand_bn(rng, cout)
    a1, a2 = _alpha(rng, act, cmid), _alpha(rng, act, cout)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    s1, o1 = hiplib.fold_bn(*(t(a) for a in bn1), 1e-3)
    s2, o2 = hiplib.fold_bn(*(t(a) for a in bn2), 1e-3)
    pair = hiplib.pack_pair_f16bf8(t(w1[0]), t(w2[0]))
    status = torch.zeros(1, dtype=torch.int32, device=dev)

    def run(ms):
        layout = engine.BatchLayout([m.shape[0] for m in ms], 1, hiplib.POOL_BLOCK_ROWS)
        host = np.zeros((layout.rows, cin), np.float32)
        layout.pack(ms, host)
        xin = hiplib.SplitBuf(layout.rows, cin, dev, hiplib.FMT_SPLIT8)
        hiplib.split_encode(t(host), xin)
        blk = torch.full((hiplib.block_stats_floats(layout.rows, cout),), float("nan"), dtype=torch.float32, device=dev)
        hiplib.tdnn_pair_pool8(xin, layout.rows, pair, (t(b1), s1, o1, t(a1)), (t(b2), s2, o2, t(a2)), CODE[act], t(layout.row_valid()),
                               blk, status)
        out = torch.full((len(ms), 2 * cout), float("nan"), dtype=torch.float32, device=dev)
        hiplib.stats_pool_blocks(blk, cout, t(layout.row_start), t(layout.row_len), len(ms), 1e-5, out)
        return out.cpu().numpy(), blk, layout, xin

    got, blk, layout, xin = run(mats)
    assert int(status.item()) == 0 and np.isfinite(got).all()
    for i, m in enumerate(mats):
        h = oracle.tdnn_layer(m, w1, b1, bn1, act, a1, 1, np.float64)
        ref = oracle.stats_pool(oracle.tdnn_layer(h, w2, b2, bn2, act, a2, 1, np.float64), 1e-5, np.float64)
        assert oracle.rel_l2(got[i, :cout], ref[:cout]) < 2 * TOL_GEMM8, (i, lens[i], oracle.rel_l2(got[i, :cout], ref[:cout]))
        assert oracle.rel_l2(got[i, cout:], ref[cout:]) < 2 * TOL_GEMM8, (i, lens[i], oracle.rel_l2(got[i, cout:], ref[cout:]))
    # the two-launch f16bf8 path on the same input: same quantity up to the arithmetic's rounding
    hmid = hiplib.SplitBuf(layout.rows, cmid, dev, hiplib.FMT_SPLIT8)
    rv = t(layout.row_valid())
    hiplib.tdnn_layer8(xin, layout.rows, hiplib.pack_weights_f16bf8(t(w1)), t(b1), s1, o1, CODE[act], t(a1), 1, rv, hmid)
    blk2 = torch.full_like(blk, float("nan"))
    hiplib.tdnn_layer_pool8(hmid, layout.rows, hiplib.pack_weights_f16bf8(t(w2)), t(b2), s2, o2, CODE[act], t(a2), 1, rv, blk2)
    b1_, b2_ = blk.cpu().numpy().reshape(-1, 2, cout), blk2.cpu().numpy().reshape(-1, 2, cout)
    has_frames = layout.row_valid().astype(bool)
    has_frames = np.pad(has_frames, (0, (-len(has_frames)) % 8)).reshape(-1, 8).any(axis=1)
    assert np.isfinite(b1_[has_frames]).all() and np.allclose(b1_[has_frames], b2_[has_frames], rtol=5e-3, atol=5e-4)
    alone, _, _, _ = run(mats[:1])
    assert np.array_equal(alone[0], got[0])


def test_pair_f16bf8_reports_an_out_of_range_intermediate(env):
    torch, hiplib, dev = env["torch"], env["hiplib"], env["dev"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    R, cin, cout = 256, 64, 64
    x = hiplib.SplitBuf(R, cin, dev, hiplib.FMT_SPLIT8)
    hiplib.split_encode(t(np.full((R, cin), 100.0, np.float32)), x)
    w1 = np.zeros((cin, 512), np.float32); w1[:, 5] = 10.0          # H[:, 5] = 64000 > 57344
    w2 = np.zeros((512, cout), np.float32)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    blk = torch.zeros(hiplib.block_stats_floats(R, cout), dtype=torch.float32, device=dev)
    hiplib.tdnn_pair_pool8(x, R, hiplib.pack_pair_f16bf8(t(w1), t(w2)), (None,) * 4, (None,) * 4, 1, None, blk, status)
    assert int(status.item()) == 1


@pytest.mark.parametrize("which", ["pool8", "pair8", "pool3", "pair3"])
def test_rows_past_the_batch_cannot_leak_into_the_pooling_blocks(env, which):
    """Activation buffers are recycled between batches of different sizes: the rows past R of an input may hold anything --
    including byte patterns that are NaN / Inf in fp16 or bf8.  The last 8-row block of a batch whose row count is not a
    multiple of 8 holds such rows next to real frames; its statistics must not notice (a `* 0` mask would turn NaN into NaN)."""
    torch, hiplib, engine, dev = env["torch"], env["hiplib"], env["engine"], env["dev"]
    rng = np.random.default_rng(3)
    cin, cmid, cout = 64, 512, 64
    lens = [29, 130]                                         # the last chunk ends 3 rows into its last block
    layout = engine.BatchLayout(lens, 1, hiplib.POOL_BLOCK_ROWS)
    R = int(layout.row_start[-1] + layout.row_len[-1] + 1)   # ... and the batch ends right behind its gap row
    assert R % 8 != 0 and R <= layout.rows
    host = np.zeros((layout.rows, cin), np.float32)
    layout.pack([(rng.standard_normal((n, cin)) * 2).astype(np.float32) for n in lens], host)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rv = t(layout.row_valid()[:R])
    w1 = (rng.standard_normal((cin, cmid)) / 8).astype(np.float32)
    w2 = (rng.standard_normal((cmid, cout)) / 22).astype(np.float32)
    fmt = hiplib.FMT_SPLIT8 if which.endswith("8") else hiplib.FMT_SPLIT
    outs = []
    for poison in (False, True):
        x = hiplib.SplitBuf(layout.rows, cin, dev, fmt)
        hiplib.split_encode(t(host[:R]), x, rows=R)
        if poison:
            x.base[(hiplib.SPLIT_PAD_BEFORE + R) * x.row_bytes:].fill_(0xFF)      # fp16 / bf16 NaN, bf8 NaN
        blk = torch.full((hiplib.block_stats_floats(R, cout),), float("nan"), dtype=torch.float32, device=dev)
        if which == "pool8":
            hiplib.tdnn_layer_pool8(x, R, hiplib.pack_weights_f16bf8(t(w1[None, :, :cout])), None, None, None, 1, None, 1, rv, blk)
        elif which == "pool3":
            hiplib.tdnn_layer_pool(x, R, hiplib.pack_weights_bf16x3(t(w1[None, :, :cout])), None, None, None, 1, None, 1, rv, blk)
        elif which == "pair8":
            hiplib.tdnn_pair_pool8(x, R, hiplib.pack_pair_f16bf8(t(w1), t(w2)), (None,) * 4, (None,) * 4, 1, rv, blk)
        else:
            hiplib.tdnn_pair_pool(x, R, hiplib.pack_pair_bf16x3(t(w1), t(w2)), (None,) * 4, (None,) * 4, 1, rv, blk)
        out = torch.empty((len(lens), 2 * cout), dtype=torch.float32, device=dev)
        hiplib.stats_pool_blocks(blk, cout, t(layout.row_start), t(layout.row_len), len(lens), 1e-5, out)
        outs.append(out.cpu().numpy())
    assert np.isfinite(outs[0]).all() and np.array_equal(outs[0], outs[1])


@pytest.mark.parametrize("which", ["pool8", "pair8", "pool3", "pair3"])
def test_block_statistics_do_not_depend_on_the_row_position(env, which):
    """The same frames moved down by 8, 16, 32, 64 or 128 rows give the same 8-row block statistics, BIT FOR BIT, one, two ...
    blocks further down: the pooling code of a block must not depend on which wave, lane half or unrolled instance handles it
    (the optimiser once contracted the sums of the two blocks a lane pools differently).  Full width: 1536 columns, so that the
    pair kernels' in-loop AND tail pooling are covered."""
    torch, hiplib, dev = env["torch"], env["hiplib"], env["dev"]
    R, cin, cmid, cout = 1024, 512, 512, 1536
    g = torch.Generator(device="cpu").manual_seed(5)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)
    w1, w2 = rnd(cin, cmid) / cin ** 0.5, rnd(cmid, cout) / cmid ** 0.5
    b1, b2 = rnd(cmid) * 0.1, rnd(cout) * 0.1
    x = torch.relu(rnd(R, cin)) * 1.3 - 0.4
    fmt = hiplib.FMT_SPLIT8 if which.endswith("8") else hiplib.FMT_SPLIT
    rv = torch.ones(R, dtype=torch.uint8, device=dev)
    if which == "pair8":
        pk = hiplib.pack_pair_f16bf8(w1, w2)
    elif which == "pair3":
        pk = hiplib.pack_pair_bf16x3(w1, w2)
    elif which == "pool8":
        pk = hiplib.pack_weights_f16bf8(w2[None])
    else:
        pk = hiplib.pack_weights_bf16x3(w2[None])

    def run(frames):
        xs = hiplib.SplitBuf(R, cin, dev, fmt)
        hiplib.split_encode(frames, xs)
        blk = torch.zeros(hiplib.block_stats_floats(R, cout), dtype=torch.float32, device=dev)
        if which == "pair8":
            hiplib.tdnn_pair_pool8(xs, R, pk, (b1, None, None, None), (b2, None, None, None), 1, rv, blk)
        elif which == "pair3":
            hiplib.tdnn_pair_pool(xs, R, pk, (b1, None, None, None), (b2, None, None, None), 1, rv, blk)
        elif which == "pool8":
            hiplib.tdnn_layer_pool8(xs, R, pk, b2, None, None, 1, None, 1, rv, blk)
        else:
            hiplib.tdnn_layer_pool(xs, R, pk, b2, None, None, 1, None, 1, rv, blk)
        return blk.view(-1, 2, cout).cpu().numpy()

    base = run(x)
    assert np.isfinite(base).all() and np.abs(base).max() > 0
    for shift in (8, 16, 32, 64, 128):
        moved = torch.zeros_like(x)
        moved[shift:] = x[:-shift]
        got = run(moved)
        nb = shift // 8
        assert np.array_equal(got[nb:], base[: R // 8 - nb]), "shift %d" % shift
