"""CPU companion of tests/test_gpu_pair_elementwise.py: the data constructions of tests/pair_data.py have the properties the GPU
tests rely on, and the GPU assertions have the power to see what they are there for --

* builder properties: multiples of q, M / q < 2^24, live low planes, every step of the layer-1 epilogue exact in fp32 (asserted by
  the builder itself), and a random-order fp32 replay of the individual emulated products that equals z bit for bit;
* select_w2 forwards decode(H) without a rounding;
* mutants (an emulator that drops a cross term of layer 1 or of layer 2, or swaps the l8 and h8 planes of H) violate the SAME
  functions the GPU tests assert with -- in >= 90 % of the live blocks for the exact test, by >= 3x in the median over all live
  (block, column) entries of the mean and of M2 for the bound test -- while a faithful fp32 replay of the kernels stays within half the bound;
* the block bounds hold for the fp32 pooling replays on activations perturbed by the full element bound.

Measured here (worst over the three shapes): M / q = 0.06 2^24 (bf16x3) and 0.53 2^24 (f16bf8); faithful replay 0.18 of the element
bound and 0.17 of the block bound; median violation of the layer-2 mutants (a dropped cross term; per statistic, over all live
entries) 4.5x - 12x (f16bf8), 27x - 59x (bf16x3), the swapped bytes 19x - 55x: with the bound times 4 the f16bf8 cases fail.
"""
import numpy as np
import pytest

import arith_emul as em
import pair_data as pd

CASES = [(a, cin, cout) for a in pd.ARITHS for cin, cout in pd.SHAPES]
IDS = ["%s-%d-%d" % c for c in CASES]


@pytest.fixture(scope="module")
def lay():
    return pd.layout()


_L1 = {}


def layer1(arith, cin, test):
    key = (arith, cin, test)
    if key not in _L1:
        act = (pd.ACT_EXACT if test == "a" else pd.ACT_BOUND)[cin]
        _L1[key] = pd.live_layer1(arith, cin, act, pd.seed(arith, cin, test))        # (the builder's own asserts run here)
    return _L1[key]


def test_the_layout_is_the_one_the_issue_describes(lay):
    assert lay.rows <= 4 * 128 and lay.gap == 1 and (lay.row_start % 8 == 0).all()
    cnt = np.pad(lay.row_valid(), (0, (-lay.rows) % 8)).reshape(-1, 8).sum(1)
    assert {0, 1, 2, 3, 7, 8} <= set(cnt.tolist())            # empty, partially valid and full blocks


@pytest.mark.parametrize("test", ["a", "c"])
@pytest.mark.parametrize("arith,cin,cout", CASES, ids=IDS)
def test_layer1_is_exact_in_any_fp32_order(arith, cin, cout, test):
    d = layer1(arith, cin, test)
    assert d["Mq"] < 2 ** 24 and np.abs(d["H"]).max() < em.SPLIT8_MAX
    rng = np.random.default_rng(cin)
    rows = rng.choice(d["X"].shape[0], 6, replace=False)
    x = d["X"][rows]
    prods = []
    for xp, wp, coef in em._parts(arith, x, d["w1"]):
        p = xp[:, :, None].astype(np.float64) * wp[None].astype(np.float64) * coef           # [6, cin, 512]
        assert np.array_equal(p, p.astype(np.float32))                                        # each product exact in fp32
        prods.append(p.astype(np.float32))
    prods = np.concatenate(prods, 1)
    for _ in range(3):
        order = rng.permutation(prods.shape[1])
        z32 = np.cumsum(prods[:, order], axis=1, dtype=np.float32)[:, -1]                     # sequential fp32 accumulation
        assert np.array_equal(z32.astype(np.float64), d["z"][rows])


@pytest.mark.parametrize("arith,cin,cout", CASES, ids=IDS)
def test_select_w2_forwards_the_decoded_intermediate(arith, cin, cout):
    d = layer1(arith, cin, "a")
    l2 = pd.select_w2(cout, d["act"], 5)
    assert (np.count_nonzero(l2["w2"], axis=0) == 1).all() and (pd.low_part(arith, l2["w2"]) == 0).all()
    z, _ = em.contract(arith, d["H"], l2["w2"][None])
    want = pd.decode(arith, d["H"]).astype(np.float64)[:, l2["idx"]] * l2["val"]
    assert np.array_equal(z, want) and np.array_equal(want, want.astype(np.float32))
    a = pd.select_activation(arith, d["H"], l2)
    assert np.array_equal(a, a.astype(np.float32))             # the activation with alpha2 in {0.25, 0.5} stays exact


@pytest.mark.parametrize("arith,cin,cout", CASES, ids=IDS)
def test_exact_test_sees_a_lost_cross_term_of_layer1(lay, arith, cin, cout):
    """What test_layer1_exact_with_live_low_planes asserts with (pair_data.block_failures, the 4-ulp rule for every block: the
    shifted sums are not exact on this data) passes a faithful fp32 pooling replay and fails >= 90 % of the live blocks of every
    mutant, even with a pooling that is exact."""
    d = layer1(arith, cin, "a")
    l2 = pd.select_w2(cout, d["act"], 5)
    a = pd.scatter(lay, pd.select_activation(arith, d["H"], l2), cout)
    assert not pd.shifted_sums_exact(lay, a)                   # hence exact_counts=() in the GPU test
    bad, live = pd.block_failures(pd.pool_replay(arith, lay, a, None, None), lay, a, cout, ())
    assert live.sum() > 50 and not bad.any()
    mutants = [pd.select_activation(arith, pd.layer1_mutant(d, drop), l2) for drop in (1, 2)]
    if arith == "f16bf8":
        mutants.append(pd.select_activation(arith, d["H"], l2, swap=True))
    for am in mutants:
        bad, live = pd.block_failures(pd.block_stats64(lay, pd.scatter(lay, am, cout)), lay, a, cout, ())
        assert bad.any((1, 2))[live].mean() >= 0.9


def _bn_stats(lay, act_rows, l2):
    """Exact pooling + folded BN of an activation (frames in order): what a kernel with a perfect pooling would store."""
    blk = pd.block_stats64(lay, pd.scatter(lay, act_rows, act_rows.shape[1])).astype(np.float64)
    live = np.pad(lay.row_valid(), (0, (-lay.rows) % 8)).reshape(-1, 8).any(1)
    s, o = l2["s2"].astype(np.float64), l2["o2"].astype(np.float64)
    blk[:, 0] = (blk[:, 0] * s + o) * live[:, None]
    blk[:, 1] *= s * s
    return blk


@pytest.mark.parametrize("arith,cin,cout", CASES, ids=IDS)
def test_bound_test_sees_a_lost_cross_term_of_layer2(lay, arith, cin, cout):
    d = layer1(arith, cin, "c")
    l2 = pd.real_layer2(cout, d["act"], pd.seed(arith, cin, "c") + 1)
    a, e = pd.layer2_reference(arith, d["H"], l2)
    af, ef = pd.scatter(lay, a, cout), pd.scatter(lay, e, cout)
    # faithful replay: fp32 accumulation slab by slab in the kernel's term order, then the kernel's pooling
    rep = pd.layer2_replay(arith, d["H"], l2)
    assert (np.abs(rep - a) / e).max() <= 0.5
    blk = pd.pool_replay(arith, lay, pd.scatter(lay, rep, cout), l2["s2"], l2["o2"])
    ratio, live = pd.block_bound_ratios(arith, blk, lay, af, ef, l2["s2"], l2["o2"])
    assert ratio.max() <= 0.5
    mutants = [dict(drop=1), dict(drop=2)] + ([dict(swap=True)] if arith == "f16bf8" else [])
    for kw in mutants:
        am, _ = pd.layer2_reference(arith, d["H"], l2, **kw)
        ratio, live = pd.block_bound_ratios(arith, _bn_stats(lay, am, l2), lay, af, ef, l2["s2"], l2["o2"])
        # the median over ALL live (block, column) entries, for the mean and for M2 separately: a maximum over the columns
        # would pass a mutant whose typical statistic moves by less than the bound
        assert np.median(ratio[live][:, 0]) >= 3.0 and np.median(ratio[live][:, 1]) >= 3.0, kw


@pytest.mark.parametrize("arith,cin,cout", CASES, ids=IDS)
@pytest.mark.parametrize("sign", ["plus", "minus", "random"])
def test_block_bounds_hold_for_the_perturbed_activation(lay, arith, cin, cout, sign):
    """a +- e (less the rounding of the perturbed value to fp32, which e contains) through the fp32 pooling replays."""
    d = layer1(arith, cin, "c")
    l2 = pd.real_layer2(cout, d["act"], pd.seed(arith, cin, "c") + 1)
    a, e = pd.layer2_reference(arith, d["H"], l2)
    rng = np.random.default_rng(3)
    sg = {"plus": 1.0, "minus": -1.0, "random": rng.choice([-1.0, 1.0], a.shape)}[sign]
    pert = (a + sg * (e * (1 - 2.0 ** -23) - 2.0 ** -23 * np.abs(a))).astype(np.float32)
    assert (e >= 2.0 ** -22 * np.abs(a)).all() and (np.abs(pert - a) <= e).all()
    blk = pd.pool_replay(arith, lay, pd.scatter(lay, pert, cout), l2["s2"], l2["o2"])
    ratio, live = pd.block_bound_ratios(arith, blk, lay, pd.scatter(lay, a, cout), pd.scatter(lay, e, cout), l2["s2"], l2["o2"])
    assert live.any() and ratio.max() <= 1.0, float(ratio.max())


def test_block_bound_refuses_a_value_in_an_empty_block(lay):
    a = np.ones((lay.rows, 64)) * lay.row_valid()[:, None]
    blk = pd.block_stats64(lay, a)
    ratio, live = pd.block_bound_ratios("f16bf8", blk, lay, a, np.zeros_like(a), None, None)
    assert (~live).any() and ratio.max() == 0
    blk[np.flatnonzero(~live)[0], 0, 3] = 1e-30
    assert np.isinf(pd.block_bound_ratios("f16bf8", blk, lay, a, np.zeros_like(a), None, None)[0]).sum() == 1
    blk[np.flatnonzero(live)[0], 1, 5] = np.nan
    assert np.isinf(pd.block_bound_ratios("f16bf8", blk, lay, a, np.zeros_like(a), None, None)[0]).sum() == 2
