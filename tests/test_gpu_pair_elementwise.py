"""The fused layer-3+4 pair kernels (tdnn_pair_pool_kernel, tdnn_pair_pool_f16bf8_kernel) held to exact answers and element-derived
bounds on data whose LOW planes are live (tests/pair_data.py; the CPU companion tests/test_pair_bounds_cpu.py shows that each
assertion here fails for an emulator that loses a cross term of either layer or swaps the l8 / h8 bytes of the in-register H):

* (a) layer 1 exact: live_layer1 + a one-hot layer 2 -- the block statistics are those of an exactly known activation;
* (b) control: the same layer-1 data through the observable single-layer forms must give H bit for bit (same MFMAs: if this
  fails too, the cause is the MFMA's internal adder and not the pair kernel);
* (c) layer 2 bounded: a realistic layer 2 on the exactly known H, every block and column within the bound that the element-wise
  bound A 2^-24 M implies for (mean, M2).  The worst ratio per case is printed at the end of the module;
* (d) the clamp at 57344 and the status word of the f16bf8 kernel, exactly.
"""
import numpy as np
import pytest

import arith_emul as em
import pair_data as pd
from test_gpu_elementwise import run_form

pytestmark = pytest.mark.gpu

WORST = {}
CASES = [(a, cin, cout) for a in pd.ARITHS for cin, cout in pd.SHAPES]
IDS = ["%s-%d-%d" % c for c in CASES]


@pytest.fixture(scope="module")
def env(oracle_mod):
    import torch
    from xvector_amd import engine, hiplib
    hiplib.require_gpu()
    assert hiplib.POOL_BLOCK_ROWS == 8
    yield dict(torch=torch, hiplib=hiplib, engine=engine, oracle=oracle_mod, dev=torch.device("cuda:0"))
    if WORST:
        print("\nworst |stored - reference| / block bound of the pair kernels (element bound A 2^-24 M carried through the pooling):")
        for name, (rm, r2, A) in WORST.items():
            print("  %-40s A = %5.1f   worst ratio mean %.3e   M2 %.3e" % (name, A, rm, r2))


_L1 = {}


def layer1(arith, cin, test):
    key = (arith, cin, test)
    if key not in _L1:                             # computed once, shared by (a), (b), (c); never modified
        act = (pd.ACT_EXACT if test == "a" else pd.ACT_BOUND)[cin]
        _L1[key] = pd.live_layer1(arith, cin, act, pd.seed(arith, cin, test))
    return _L1[key]


def run_pair(env, arith, layout, host, w1, w2, p1, p2, act, R=None, valid=None, tail_fill=None):
    """Encode host [rows, cin], run the pair kernel on its first R rows; returns (block statistics [blocks, 2, cout], status word
    or None).  The statistics buffer is poisoned with NaN.  tail_fill: byte written over the input buffer behind row R."""
    torch, hiplib, dev = env["torch"], env["hiplib"], env["dev"]
    cin, cout = w1.shape[0], w2.shape[1]
    R = layout.rows if R is None else R
    assert (hiplib.pair8_supported if arith == "f16bf8" else hiplib.pair_supported)(cin, pd.CMID, cout)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    xin = hiplib.SplitBuf(layout.rows, cin, dev, hiplib.FMT_SPLIT8 if arith == "f16bf8" else hiplib.FMT_SPLIT)
    hiplib.split_encode(t(host[:R]), xin, rows=R)
    if tail_fill is not None:
        xin.base[(hiplib.SPLIT_PAD_BEFORE + R) * xin.row_bytes:].fill_(tail_fill)
    rv = torch.from_numpy(np.ascontiguousarray((layout.row_valid() if valid is None else valid)[:R])).to(dev)
    blk = torch.full((hiplib.block_stats_floats(R, cout),), float("nan"), dtype=torch.float32, device=dev)
    status = None
    if arith == "f16bf8":
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        hiplib.tdnn_pair_pool8(xin, R, hiplib.pack_pair_f16bf8(t(w1), t(w2)), tuple(t(a) for a in p1), tuple(t(a) for a in p2),
                               em.ACT[act], rv, blk, status)
    else:
        hiplib.tdnn_pair_pool(xin, R, hiplib.pack_pair_bf16x3(t(w1), t(w2)), tuple(t(a) for a in p1), tuple(t(a) for a in p2),
                              em.ACT[act], rv, blk)
    torch.cuda.synchronize()
    return blk.cpu().numpy().reshape(-1, 2, cout), None if status is None else int(status.item())


def _pair_case(env, d, l2):
    layout = pd.layout()
    assert layout.rows <= 4 * 128
    host = np.zeros((layout.rows, d["cin"]), np.float32)
    layout.pack(d["mats"], host)
    blk, status = run_pair(env, d["arith"], layout, host, d["w1"], l2["w2"], (d["b1"], d["s1"], d["o1"], d["alpha1"]),
                           (l2["b2"], l2["s2"], l2["o2"], l2["alpha2"]), d["act"])
    assert status in (None, 0)
    return blk, layout


@pytest.mark.parametrize("arith,cin,cout", CASES, ids=IDS)
def test_layer1_exact_with_live_low_planes(env, arith, cin, cout):
    """live_layer1 + select_w2: the layer-4 activation is act(w2_sel decode(H_exact)), known exactly; (mean, M2) of every block
    within 4 ulp of its fp64 statistics (the rule of _check_blocks; its exact branch only where the shifted sums of this data
    are exact in fp32 -- they are not: squares of 15-bit differences), empty blocks zero."""
    d = layer1(arith, cin, "a")
    l2 = pd.select_w2(cout, d["act"], 5)
    blk, layout = _pair_case(env, d, l2)
    a = pd.scatter(layout, pd.select_activation(arith, d["H"], l2), cout)
    exact = (1, 2, 4, 8) if pd.shifted_sums_exact(layout, a) else ()
    bad, live = pd.block_failures(blk, layout, a, cout, exact)
    print("%s %d -> %d: %d of %d block statistics off" % (arith, cin, cout, bad.sum(), live.sum() * 2 * cout))
    pd._check_blocks(blk, layout, a, cout, "pair exact %s %d" % (arith, cin), exact)
    assert (blk[:len(live)][~live] == 0).all()


CONTROL = sorted({(a, cin, t) for a, cin, _ in CASES for t in "ac"})


@pytest.mark.parametrize("arith,cin,test", CONTROL, ids=["%s-%d-%s" % c for c in CONTROL])
def test_single_layer_control_exact_with_live_low_planes(env, arith, cin, test):
    """The layer-1 data of (a) and (c) through tdnn_layer8 (128- and 256-row tiles) / tdnn_layer with fp32 output: y == H_exact
    in EVERY element."""
    d = layer1(arith, cin, test)
    tunes = [{"rows": 128}, {"rows": 256}] if arith == "f16bf8" else [None]
    for tune in tunes:
        y, layout = run_form(env, arith, d["mats"], d["w1"][None], d["b1"], d["s1"], d["o1"], d["act"], d["alpha1"], 1,
                             "split8" if arith == "f16bf8" else "split", "f32", tune)
        got = y[layout.row_valid().astype(bool)]
        bad = np.argwhere(got != d["H"])
        assert bad.size == 0, (arith, cin, tune, len(bad), bad[:5].tolist(), d["Mq"] / 2 ** 24)


@pytest.mark.parametrize("arith,cin,cout", CASES, ids=IDS)
def test_layer2_block_bounds_on_exact_live_intermediate(env, arith, cin, cout):
    """live_layer1 + real_layer2.  Reference: the emulated terms of float32(H_exact) . w2 in fp64, e = elementwise_bound(A_PAIR, M,
    zb, a, None, alpha2) per element; every block and column of the stored (mean, M2) within pair_data.block_bound_ratios."""
    d = layer1(arith, cin, "c")
    l2 = pd.real_layer2(cout, d["act"], pd.seed(arith, cin, "c") + 1)
    blk, layout = _pair_case(env, d, l2)
    a, e = pd.layer2_reference(arith, d["H"], l2)
    ratio, live = pd.block_bound_ratios(arith, blk, layout, pd.scatter(layout, a, cout), pd.scatter(layout, e, cout), l2["s2"], l2["o2"])
    name = "pair %s %d -> 512 -> %d %s" % (arith, cin, cout, d["act"])
    print("%s: worst ratio mean %.3e  M2 %.3e" % (name, ratio[:, 0].max(), ratio[:, 1].max()))
    WORST[name] = (float(ratio[:, 0].max()), float(ratio[:, 1].max()), pd.A_PAIR[arith])
    assert live.sum() > 50 and (ratio <= 1).all(), (name, np.unravel_index(np.argmax(ratio), ratio.shape), float(ratio.max()))


def test_pair8_flag_and_clamp_are_exact(env):
    """x = 4 against a w1 column of 224: H = 57344 exactly, the largest value the split8 encoding holds -- no flag.  One more (b1
    = 1) sets bit 0 of the status word and the statistics are those of the clamped H, bit for bit those of the b1 = 0 run.  The
    same overflowing rows in a gap row or behind row R (a recycled buffer's tail) neither raise the flag nor move a statistic."""
    hiplib, engine = env["hiplib"], env["engine"]
    cin, cout, c = 64, 64, 7
    rng = np.random.default_rng(11)
    w1 = np.zeros((cin, pd.CMID), np.float32)
    w1[:, c] = 224.0
    idx = (np.arange(cout) * 7) % pd.CMID
    assert idx[1] == c
    w2 = np.zeros((pd.CMID, cout), np.float32)
    w2[idx, np.arange(cout)] = np.array([1.0, 2.0, 3.0], np.float32)[np.arange(cout) % 3]
    b0 = rng.integers(-4, 5, pd.CMID).astype(np.float32)
    b0[c] = 0.0
    b1 = b0.copy()
    b1[c] = 1.0
    none = (None,) * 4
    # every frame overflows by one
    layout = pd.layout()
    host = np.zeros((layout.rows, cin), np.float32)
    layout.pack([np.full((n, cin), 4.0, np.float32) for n in pd.LENS], host)
    blk0, st0 = run_pair(env, "f16bf8", layout, host, w1, w2, (b0, None, None, None), none, "none")
    blk1, st1 = run_pair(env, "f16bf8", layout, host, w1, w2, (b1, None, None, None), none, "none")
    assert st0 == 0 and st1 == 1
    H = np.tile(b0.astype(np.float64), (layout.rows, 1))
    H[:, c] = 57344.0
    y = (H[:, idx] * w2[idx, np.arange(cout)]) * layout.row_valid()[:, None]
    pd._check_blocks(blk0, layout, y, cout, "clamp")              # constant blocks: mean = the value, M2 = 0, exactly
    live = np.pad(layout.row_valid(), (0, (-layout.rows) % 8)).reshape(-1, 8).any(1)
    assert blk0[live, 0, 1].tolist() == [2 * 57344.0] * int(live.sum())
    assert np.array_equal(blk0, blk1)
    # the overflow only where no frame is: gap rows; rows behind R
    lens = [29, 130]
    layout = engine.BatchLayout(lens, 1, hiplib.POOL_BLOCK_ROWS)
    R = int(layout.row_start[-1] + layout.row_len[-1] + 1)
    assert R % 8 != 0 and R <= layout.rows
    host = np.zeros((layout.rows, cin), np.float32)
    layout.pack([rng.integers(-3, 4, (n, cin)).astype(np.float32) for n in lens], host)     # |H[c]| <= 64 * 3 * 224 + 1
    valid = layout.row_valid().astype(bool)
    clean, st = run_pair(env, "f16bf8", layout, host, w1, w2, (b1, None, None, None), none, "none", R=R)
    assert st == 0 and np.isfinite(clean).all() and np.abs(clean[:, 1]).max() > 0
    gaps = host.copy()
    gaps[~valid] = 4.0
    got, st = run_pair(env, "f16bf8", layout, gaps, w1, w2, (b1, None, None, None), none, "none", R=R)
    assert st == 0 and np.array_equal(got, clean)
    # 0x7b: fp16 0x7b7b = 61280, e5m2 0x7b = 57344 -- finite and far beyond the clamp after the layer
    got, st = run_pair(env, "f16bf8", layout, host, w1, w2, (b1, None, None, None), none, "none", R=R, tail_fill=0x7b)
    assert st == 0 and np.array_equal(got, clean)
    # ... and the same rows DO raise it once they count as frames
    allv = layout.row_valid().copy()
    allv[:] = 1
    _, st = run_pair(env, "f16bf8", layout, gaps, w1, w2, (b1, None, None, None), none, "none", R=R, valid=allv)
    assert st == 1
