"""CPU companion of tests/test_gpu_pool_elementwise.py: what that module relies on is settled here, without a GPU.

* the float32 replay of stats_pool_kernel's merge order (tests/pool_data.py) is exact -- equal to the fp64 answer rounded once, bit
  for bit -- at the lengths of pd.EXACT_LENS on the integer data of the GPU test, and is NOT exact at their neighbours;
* the derived bounds of pool_data.moment_bounds hold for that replay on every channel kind, length and split of the GPU cases
  (the replay rounds every operation; the kernel, with FMA contraction, rounds fewer);
* the builders give what the GPU module assumes of them (dyadic weights, exact block statistics, every channel kind in a batch)."""
import numpy as np
import pytest

import pool_data as pd


@pytest.mark.parametrize("n,split", pd.EXACT_LENS)
def test_replay_is_exact_at_the_power_of_two_lengths(n, split):
    m = pd.integer_chunk(n, 64, seed=n * 1000 + split)
    mean, var = pd.moments_ref(m)
    got_mean, got_var = pd.replay_moments(m, split)
    assert pd.bits_equal(got_mean, mean.astype(np.float32))
    assert pd.bits_equal(got_var, var.astype(np.float32))
    assert float(np.abs(mean * 64).max()) < 2 ** 24 and np.array_equal(mean * 64, np.round(mean * 64))      # multiples of 1/64
    assert np.array_equal(var * n * 64, np.round(var * n * 64)) and float((var * n * 64).max()) < 2 ** 24   # M2: multiples of 1/64


@pytest.mark.parametrize("n,split", pd.INEXACT_NEIGHBOURS)
def test_replay_is_not_exact_at_a_neighbour(n, split):
    m = pd.integer_chunk(n, 64, seed=n * 1000 + split)
    mean, var = pd.moments_ref(m)
    got_mean, got_var = pd.replay_moments(m, split)
    assert not (pd.bits_equal(got_mean, mean.astype(np.float32)) and pd.bits_equal(got_var, var.astype(np.float32)))


@pytest.mark.parametrize("mode", pd.MODES, ids=[m[0] for m in pd.MODES])
def test_bounds_hold_for_the_replay(mode):
    _, lens, split = mode
    C = 20
    _, _, mats = pd.batch(lens, C, seed=split + len(lens))
    kinds = set()
    for b, m in enumerate(mats):
        mean, var = pd.moments_ref(m)
        e_mean, e_var, e_std = pd.moment_bounds(m, split)
        got_mean, got_var = pd.replay_moments(m, split)
        assert (np.abs(got_mean - mean) <= e_mean).all(), (b, m.shape)
        assert (np.abs(got_var - var) <= e_var).all(), (b, m.shape)
        assert (np.abs(pd.std32(got_var) - np.sqrt(var + float(pd.EPS32))) <= e_std).all(), (b, m.shape)
        for c in range(C):
            kinds.add(pd.kind_of(b, c))
            if pd.kind_of(b, c) == "const":
                assert got_var[c] == 0 and got_mean[c] == m[0, c]
    assert kinds == set(pd.KINDS)


def test_every_kind_occurs_at_four_channels():
    assert {pd.kind_of(b, c) for b in range(len(pd.LENS)) for c in range(4)} == set(pd.KINDS)


def test_merges_counts_the_longest_path():
    assert pd.merges(1, 512) == 3 and pd.merges(33, 512) == 4 and pd.merges(512, 512) == 18
    assert pd.merges(513, 512) == 16 + 2 + 2 and pd.merges(1025, 128) == 4 + 2 + 9


@pytest.mark.parametrize("n", (1, 2, 7, 33, 100, 513, 1024))
def test_dyadic_weights_sum_to_one_exactly(n):
    w = pd.dyadic_weights(n, seed=n)
    assert len(w) == n and w.astype(np.float64).sum() == 1.0
    assert (np.log2(w) == np.round(np.log2(w))).all() and w.min() >= 2.0 ** -10


@pytest.mark.parametrize("n", pd.BLOCK_EXACT_LENS)
def test_dyadic_blocks_have_an_exact_fp64_answer(n):
    blk = pd.dyadic_blocks(n, 8, seed=n)
    assert np.array_equal(blk[:, 0] * 8, np.round(blk[:, 0] * 8)) and np.array_equal(blk[:, 1] * 64, np.round(blk[:, 1] * 64))
    mean, var, _ = pd.blocks_ref(blk, n)
    b = blk.astype(np.float64)                                   # the same sums in fp64, another order: exact means equal
    S = (8 * b[::-1, 0]).sum(0)
    Q = (b[::-1, 1] + 8 * b[::-1, 0] ** 2).sum(0)
    assert np.array_equal(S / n, mean) and np.array_equal(Q / n - (S / n) ** 2, var)


def test_chunk_average_batched_reference_is_the_loop():
    rng = np.random.default_rng(5)
    cnt = rng.integers(1, 4, size=200)
    seg = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    lens = rng.integers(25, 10001, size=seg[-1]).astype(np.int32)
    e = (5 * rng.standard_normal((seg[-1], 7))).astype(np.float32)
    got = pd.chunk_average_ref_batched(e, seg, lens)
    for u in range(200):
        assert pd.bits_equal(got[u], pd.chunk_average_ref(e[seg[u]:seg[u + 1]], lens[seg[u]:seg[u + 1]])), u


def test_softmax_cases_put_a_lone_maximum_in_every_wave():
    peaks = {(n, p) for n, sp, p in pd.softmax_cases() if p is not None}
    assert {p // 64 % 4 for n, p in peaks} == {0, 1, 2, 3}
    assert {(257, 256), (5000, 4999), (255, 254), (1, 0)} <= peaks
