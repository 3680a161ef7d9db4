"""The f16mx6 form of the pair kernel (xv_tdnn_pair_pool_f16mx6: layer 4's cross terms on block-scaled e2m3 MFMAs) held to the
emulation of tests/pair_mx6_data.py: exact answers on data where every sum is exact, element-derived block bounds on random
data, position independence, the status word, and the whole network against the bf8 form.

Shapes: cin = cmid = 512, cout = 64 and 192, R = 136 rows (one full 128-row workgroup and a partial one), two chunks of 61 and 40
frames on 8-row starts with a 3-row gap."""
import numpy as np
import pytest

import arith_emul as em
import pair_data as pd
import pair_mx6_data as mx

pytestmark = pytest.mark.gpu

CIN = 512
R = 136
LAYOUT = mx.Rows([0, 64], [61, 40], R)
COUTS = [64, 192]
NONE4 = (None,) * 4


@pytest.fixture(scope="module")
def env(oracle_mod):
    import torch
    from xvector_amd import engine, hiplib, synthetic, topology
    hiplib.require_gpu()
    assert hiplib.POOL_BLOCK_ROWS == 8
    return dict(torch=torch, hiplib=hiplib, engine=engine, oracle=oracle_mod, synthetic=synthetic, topology=topology,
                dev=torch.device("cuda:0"))


def run(env, host, w1, w2, p1=NONE4, p2=NONE4, act="none", rows=R, valid=None, form="mx6"):
    """Encode host [rows, 512] as split8 and run a pair kernel on it (statistics buffer poisoned with NaN): (blocks [., 2, cout],
    status word)."""
    torch, hiplib, dev = env["torch"], env["hiplib"], env["dev"]
    cout = w2.shape[1]
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    xin = hiplib.SplitBuf(rows, CIN, dev, hiplib.FMT_SPLIT8)
    hiplib.split_encode(t(host[:rows]), xin, rows=rows)
    rv = torch.from_numpy(np.ascontiguousarray(LAYOUT.row_valid() if valid is None else valid)[:rows]).to(dev)
    blk = torch.full((hiplib.block_stats_floats(rows, cout),), float("nan"), dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    assert hiplib.pair_mx6_supported(CIN, pd.CMID, cout)
    if form == "mx6":
        hiplib.tdnn_pair_pool_mx6(xin, rows, hiplib.pack_pair_f16mx6(t(w1), t(w2)), tuple(t(a) for a in p1), tuple(t(a) for a in p2),
                                  em.ACT[act], rv, blk, status)
    else:
        hiplib.tdnn_pair_pool8(xin, rows, hiplib.pack_pair_f16bf8(t(w1), t(w2)), tuple(t(a) for a in p1), tuple(t(a) for a in p2),
                               em.ACT[act], rv, blk, status)
    torch.cuda.synchronize()
    return blk.cpu().numpy().reshape(-1, 2, cout), int(status.item())


def pack_rows(mats, rows=R, layout=LAYOUT):
    host = np.zeros((rows, CIN), np.float32)
    layout.pack(mats, host)
    return host


# ---- exact data ------------------------------------------------------------------------------------------------------------------
PERM = (np.arange(pd.CMID) * 5 + 3) % pd.CMID                 # layer 3 = a permutation: H[:, j] = x[:, PERM[j]], bit for bit
Q13 = 2.0 ** -13


def exact_case(cout, seed):
    """x (= H up to the permutation) and w2 = sign(n) (|n| + j 2^-13) with n on the e2m3 grid of its block and j <= 3 where n != 0: hi =
    n in fp16 (n + 2^-11 for |n| = 1/2, j = 3), 2^11 lo = j / 4.  Blocks come in magnitude classes (x: 1, 4, 1/2; w2: 1, 2) so that block
    scales differ between the blocks of a frame / a column; in class 4 the low plane falls on ties and below the grid's first step.
    Frames of chunk 0 repeat in groups of 8 (its pooling blocks hold equal rows: mean = the element, M2 = 0, exactly), frames of
    chunk 1 are all different."""
    rng = np.random.default_rng(seed)
    nv = np.array([0, 1, -1, 2, -2, 3, -3, 4, -4], np.float64)

    def values(shape, cls, density):
        n = rng.choice(nv, shape) * (rng.random(shape) < density)
        j = rng.integers(0, 4, shape) * np.sign(n)            # away from zero: towards zero it would cross a binade at a power of two
        return ((n * cls) + j * Q13).astype(np.float32)
    # H in channel order, one class per (frame, block); x = H permuted back
    def h_rows(T):
        cls = rng.choice([1.0, 1.0, 4.0, 0.5], (T, 32))
        full = np.zeros((T, pd.CMID))
        full[:, mx.BLOCK_CHANNELS] = np.repeat(cls[:, :, None], 16, -1)
        return values((T, pd.CMID), full, 0.9)
    H0 = np.repeat(h_rows(8), 8, 0)[:61]
    H1 = h_rows(40)
    clsw = rng.choice([1.0, 2.0], (cout, 32))
    fullw = np.zeros((cout, pd.CMID))
    fullw[:, mx.BLOCK_CHANNELS] = np.repeat(clsw[:, :, None], 16, -1)
    w2 = values((pd.CMID, cout), fullw.T, 1.0 / 32)
    H = np.concatenate([H0, H1])
    x = np.zeros_like(H)
    x[:, PERM] = H
    w1 = np.zeros((CIN, pd.CMID), np.float32)
    w1[PERM, np.arange(pd.CMID)] = 1.0
    assert np.array_equal(em.decode8(x), x)                   # the split8 buffer holds x exactly, so the permutation layer gives H = x
    return x, w1, H, w2


@pytest.mark.parametrize("cout", COUTS)
def test_exact_answers_on_grid_data(env, cout):
    """Every operand of layer 4 on the fp16 grid and, after its block's scale, on the e2m3 grid or a known rounding of it; every
    product a multiple of 2^-14 and every partial sum below 2^24 of them: the activation is the same fp32 bits under any
    summation order.  Chunk 0 (equal rows per block): (mean, M2) == (the element, 0) exactly.  Chunk 1: the rule of
    pair_data._check_blocks (exact where the shifted sums are exact in fp32, within 4 ulp of the fp64 statistics elsewhere)."""
    x, w1, H, w2 = exact_case(cout, 60 + cout)
    tz = mx.terms(H, w2)
    quantum = 2.0 ** -14                                      # cross terms: 2^-11 (multiples of 1/4) (multiples of 1/2); main term: 2^-11 (integers)
    assert all(np.array_equal(t[0] / quantum, np.round(t[0] / quantum)) for t in tz)
    M = sum(t[1] for t in tz)
    assert M.max() < 2 ** 24 * quantum, M.max()
    assert all((t[1].sum(0) > 0).all() for t in tz)           # all three terms live in every column
    hl, wl = mx.operand_planes(H, 1)[1], mx.operand_planes(w2, 0)[1]
    assert (hl != 0).mean() > 0.2 and (wl[w2 != 0] != 0).mean() > 0.5
    assert len(np.unique(mx.operand_planes(H, 1)[3][0])) >= 3 and len(np.unique(mx.operand_planes(w2, 0)[3][0])) >= 2
    y = sum(t[0] for t in tz)
    assert np.array_equal(y, y.astype(np.float32).astype(np.float64))
    blk, status = run(env, pack_rows([x[:61], x[61:]]), w1, w2)
    assert status == 0
    y_full = np.zeros((R, cout))
    LAYOUT.pack([y[:61], y[61:]], y_full)
    # chunk 0: blocks 0 .. 7 hold equal rows
    for k in range(8):
        assert np.array_equal(blk[k, 0].astype(np.float64), y_full[8 * k]), ("mean of block", k)
        assert not blk[k, 1].any(), ("M2 of block", k)
    exact = (1, 2, 4, 8) if pd.shifted_sums_exact(LAYOUT, y_full) else ()
    pd._check_blocks(blk, LAYOUT, y_full, cout, "f16mx6 exact %d" % cout, exact)
    live = np.pad(LAYOUT.row_valid(), (0, (-R) % 8)).reshape(-1, 8).any(1)
    assert (blk[:len(live)][~live] == 0).all()


# ---- random data -----------------------------------------------------------------------------------------------------------------
_L1 = {}


def live512(act):
    """pair_data.live_layer1 at cin = 512 (its H is known exactly and live in every plane); the first 101 frames are the two chunks."""
    if act not in _L1:
        _L1[act] = pd.live_layer1("f16bf8", CIN, act, pd.seed("f16bf8", CIN, "c"))
    return _L1[act]


@pytest.mark.parametrize("cout,act", [(64, "relu"), (192, "prelu")])
def test_block_bounds_on_random_layer2(env, cout, act):
    """pair_data.real_layer2 on the exactly known H of live_layer1.  Reference: the emulated f16mx6 terms of float32(H) . w2 in fp64;
    element bound elementwise_bound(A_PAIR, M, ...) (fp32 accumulation only: the encoding is emulated, not bounded); every block
    statistic within pair_data.block_bound_ratios."""
    d = live512(act)
    l2 = pd.real_layer2(cout, act, 77 + cout)
    X, H = d["X"][:101], d["H"][:101]
    blk, status = run(env, pack_rows([X[:61], X[61:]]), d["w1"], l2["w2"], (d["b1"], d["s1"], d["o1"], d["alpha1"]),
                      (l2["b2"], l2["s2"], l2["o2"], l2["alpha2"]), act)
    assert status == 0
    a, e = mx.layer2_reference(H, l2, pd.A_PAIR["f16bf8"])
    a_full, e_full = np.zeros((R, cout)), np.zeros((R, cout))
    LAYOUT.pack([a[:61], a[61:]], a_full)
    LAYOUT.pack([e[:61], e[61:]], e_full)
    ratio, live = pd.block_bound_ratios("f16bf8", blk, LAYOUT, a_full, e_full, l2["s2"], l2["o2"])
    print("f16mx6 512 -> 512 -> %d %s: worst |stored - reference| / bound: mean %.3e  M2 %.3e" % (cout, act, ratio[:, 0].max(), ratio[:, 1].max()))
    assert live.sum() == 13 and (ratio <= 1).all(), (np.unravel_index(np.argmax(ratio), ratio.shape), float(ratio.max()))
    # the bound does tell the two encodings apart: the bf8 emulation's activation is further from this one than the bound allows
    a8, _ = pd.layer2_reference("f16bf8", H, l2)
    assert (np.abs(a8 - a) > e).mean() > 0.1


def test_layer3_stages_are_those_of_the_bf8_pack(env):
    torch, hiplib, dev = env["torch"], env["hiplib"], env["dev"]
    g = torch.Generator(device="cpu").manual_seed(5)
    w1 = (torch.randn((CIN, pd.CMID), generator=g) / CIN ** 0.5).to(dev)
    for cout in COUTS:
        w2 = (torch.randn((pd.CMID, cout), generator=g) / pd.CMID ** 0.5).to(dev)
        p8, p6 = hiplib.pack_pair_f16bf8(w1, w2), hiplib.pack_pair_f16mx6(w1, w2)
        torch.cuda.synchronize()
        b8, b6 = p8.wt.view(torch.uint8).cpu().numpy().ravel(), p6.wt.view(torch.uint8).cpu().numpy().ravel()
        n3 = 2 * (CIN // 32) * 32768
        assert len(b8) == len(b6) == n3 + 4 * (cout // 64) * 32768
        assert np.array_equal(b8[:n3], b6[:n3])
        # layer 4: the fp16 fragments (the first 2 KB of every 4 KB unit) agree as well, the 8-bit fragments do not
        u8, u6 = b8[n3:].reshape(-1, 4096), b6[n3:].reshape(-1, 4096)
        assert np.array_equal(u8[:, :2048], u6[:, :2048]) and not np.array_equal(u8[:, 2048:], u6[:, 2048:])
        # ... and hold what the emulation says: per lane six dwords, then the block's E8M0 byte, zero-extended, and a zero
        tail = u6[:, 3072:].reshape(-1, 64, 16)
        k = mx.operand_planes(w2.cpu().numpy(), 0)[3]                        # [cout, 32]
        assert not tail[:, :, 9:].any() and set(np.unique(tail[:, :, 8]).tolist()) == set(np.unique(k + 127).tolist())


def random_case(cout, seed):
    rng = np.random.default_rng(seed)
    f = lambda a: np.asarray(a, np.float32)
    mats = [f(np.maximum(rng.standard_normal((n, CIN)), 0) * 1.3 - 0.4) for n in (61, 40)]
    w1 = f(rng.standard_normal((CIN, pd.CMID)) / np.sqrt(CIN))
    w2 = f(rng.standard_normal((pd.CMID, cout)) / np.sqrt(pd.CMID))
    p1 = (f(0.1 * rng.standard_normal(pd.CMID)), f(rng.uniform(0.5, 2, pd.CMID)), f(rng.standard_normal(pd.CMID)), None)
    p2 = (f(0.1 * rng.standard_normal(cout)), f(rng.uniform(0.5, 2, cout)), f(rng.standard_normal(cout)), None)
    return mats, w1, w2, p1, p2


@pytest.mark.parametrize("cout", COUTS)
def test_a_chunk_alone_and_a_shifted_batch_give_the_same_blocks(env, cout):
    """Bit for bit: chunk 1 alone at row 0 against the same chunk behind chunk 0 (blocks 8 .. 12), and the whole batch moved down
    by 8 rows (every block one further down, the first one empty)."""
    mats, w1, w2, p1, p2 = random_case(cout, 31 + cout)
    batch, st = run(env, pack_rows(mats), w1, w2, p1, p2, "relu")
    assert st == 0 and np.isfinite(batch).all() and (batch[:13, 1] > 0).mean() > 0.5     # (ReLU: some columns are dead in a block)
    alone_layout = mx.Rows([0], [40], 40)
    alone, st = run(env, pack_rows([mats[1]], 40, alone_layout), w1, w2, p1, p2, "relu", rows=40, valid=alone_layout.row_valid())
    assert st == 0 and np.array_equal(alone[:5], batch[8:13])
    moved_layout = mx.Rows([8, 72], [61, 40], R + 8)
    moved, st = run(env, pack_rows(mats, R + 8, moved_layout), w1, w2, p1, p2, "relu", rows=R + 8, valid=moved_layout.row_valid())
    assert st == 0 and not moved[0].any() and np.array_equal(moved[1:R // 8 + 1], batch[:R // 8])


def test_a_frame_of_zeros_gives_finite_output(env):
    """An all-zero H block has m = 0: scale 1, byte 127 - 11, elements 0.  Zero frames between ordinary ones, with and without the
    biases that would make H non-zero; and a whole batch of zeros without biases: every statistic exactly zero."""
    mats, w1, w2, p1, p2 = random_case(64, 9)
    mats[0][5:9] = 0
    mats[1][:] = 0
    for pa, pb in ((p1, p2), (NONE4, NONE4)):
        blk, st = run(env, pack_rows(mats), w1, w2, pa, pb, "relu")
        assert st == 0 and np.isfinite(blk).all()
    assert not blk[8:13].any()                                   # chunk 1 without biases: H = 0, y = 0
    blk, st = run(env, np.zeros((R, CIN), np.float32), w1, w2)
    assert st == 0 and not blk.any()


def test_status_bit_is_set_beyond_57344_and_only_then(env):
    """x = 4 against a w1 column of 224: H = 57344 exactly, the largest value the encoding holds -- no flag, and the statistics are
    exact (57344 = 7.0 at the block's scale 2^-13, times a weight on the grid).  One more (b1 = 1) sets bit 0 and the statistics
    are those of the clamped H, bit for bit.  The same overflow in a gap row or behind the last frame does not raise the flag."""
    cout, c = 64, 7
    rng = np.random.default_rng(11)
    w1 = np.zeros((CIN, pd.CMID), np.float32)
    w1[:64, c] = 224.0
    idx = (np.arange(cout) * 7) % pd.CMID
    assert idx[1] == c
    w2 = np.zeros((pd.CMID, cout), np.float32)
    w2[idx, np.arange(cout)] = np.array([1.0, 2.0, 3.0], np.float32)[np.arange(cout) % 3]
    b0 = rng.integers(-4, 5, pd.CMID).astype(np.float32)
    b0[mx.BLOCK_CHANNELS[np.argwhere(mx.BLOCK_CHANNELS == c)[0, 0]]] = 0.0      # (the block of channel c: its small values would round to 0 or 8192)
    b1 = b0.copy()
    b1[c] = 1.0
    host = pack_rows([np.full((61, CIN), 4.0, np.float32), np.full((40, CIN), 4.0, np.float32)])
    host[:, 64:] = 0
    blk0, st0 = run(env, host, w1, w2, (b0, None, None, None))
    blk1, st1 = run(env, host, w1, w2, (b1, None, None, None))
    assert st0 == 0 and st1 == 1
    live = np.pad(LAYOUT.row_valid(), (0, (-R) % 8)).reshape(-1, 8).any(1)
    assert blk0[live, 0, 1].tolist() == [2 * 57344.0] * int(live.sum()) and not blk0[:, 1, 1].any()
    assert np.array_equal(blk0, blk1)
    # the overflow only where no frame is
    frames = pack_rows([rng.integers(-3, 4, (n, CIN)).astype(np.float32) for n in (61, 40)])
    frames[:, 64:] = 0                                              # |H[c]| <= 64 * 3 * 224 + 1
    clean, st = run(env, frames, w1, w2, (b1, None, None, None))
    assert st == 0 and np.isfinite(clean).all()
    gaps = frames.copy()
    gaps[~LAYOUT.row_valid().astype(bool), :64] = 4.0
    got, st = run(env, gaps, w1, w2, (b1, None, None, None))
    assert st == 0 and np.array_equal(got, clean)
    allv = np.ones(R, np.uint8)
    _, st = run(env, gaps, w1, w2, (b1, None, None, None), valid=allv)
    assert st == 1


def test_device_model_takes_the_e2m3_kernel_and_is_no_less_accurate(env):
    """DeviceModel(precision="f16bf8") on the default topology launches the f16mx6 pair kernel.  Three MFCC-like utterances of 25 /
    40 / 61 frames against the fp64 oracle: its error is not above that of the bf8 pair kernel on the same inputs (the same model
    with the e2m3 pack taken away, so that its forward launches tdnn_pair_pool8) by more than 5 % -- the CPU simulation
    (tools/experiments/cross_term_mx6_sim.py) predicts 7-12 % LOWER; the 5 % is room for fp32 summation order."""
    engine, hiplib, oracle = env["engine"], env["hiplib"], env["oracle"]
    topo = env["topology"].get("ModelWithoutDropout")
    w = env["synthetic"].trained_like(topo, 23, seed=1)
    mats = env["synthetic"].mfcc_like([25, 40, 61], 23, seed=3)
    refs = [oracle.embed_utterance(m, w, topo, 25, 10000, np.float64) for m in mats]
    model = engine.DeviceModel(w, topo, "cuda:0", precision="f16bf8")
    assert model.pair8 is not None and model.pair_mx6 is not None
    calls = []
    real6, real8 = hiplib.tdnn_pair_pool_mx6, hiplib.tdnn_pair_pool8

    def err():
        got = engine.Extractor(model, 25, 10000, accuracy_probe=False).extract(mats)
        assert all(np.isfinite(g).all() for g in got)
        num = np.sqrt(sum(np.sum((np.asarray(g, np.float64) - r) ** 2) for g, r in zip(got, refs)))
        return num / np.sqrt(sum(np.sum(r ** 2) for r in refs)), max(oracle.rel_l2(g, r) for g, r in zip(got, refs))
    try:
        hiplib.tdnn_pair_pool_mx6 = lambda *a, **k: (calls.append("mx6"), real6(*a, **k))[1]
        hiplib.tdnn_pair_pool8 = lambda *a, **k: (calls.append("bf8"), real8(*a, **k))[1]
        e6, worst6 = err()
        assert calls and set(calls) == {"mx6"}
        del calls[:]
        model.pair_mx6 = None
        e8, worst8 = err()
        assert calls and set(calls) == {"bf8"}
    finally:
        hiplib.tdnn_pair_pool_mx6, hiplib.tdnn_pair_pool8 = real6, real8
    print("x-vectors of 25 / 40 / 61 frames against the fp64 oracle, relative L2 over the three: e2m3 layer 4 %.3e, bf8 %.3e "
          "(ratio %.3f); worst utterance %.3e / %.3e" % (e6, e8, e6 / e8, worst6, worst8))
    assert e6 <= 1.05 * e8
