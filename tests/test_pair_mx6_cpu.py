"""The emulation of the f16mx6 pair kernel's e2m3 block encoding (tests/pair_mx6_data.py): the grid, the rounding, the scale rule,
and the emulated product against fp64 on the data of tests/pair_data.py.  CPU only; tests/test_gpu_pair_mx6.py holds the kernel to
this emulation."""
import numpy as np

import arith_emul as em
import pair_data as pd
import pair_mx6_data as mx


def test_e2m3_grid_and_rounding():
    g = mx.E2M3_GRID
    assert len(g) == 32 and g[0] == 0 and g[1] == 0.125 and g[8] == 1.0 and g[-1] == 7.5
    assert np.array_equal(g[:16], np.arange(16) * 0.125) and np.array_equal(g[16:24], 2 + np.arange(8) * 0.25)
    assert np.array_equal(g[24:], 4 + np.arange(8) * 0.5)
    assert np.array_equal(mx.e2m3_rne(g), g) and np.array_equal(mx.e2m3_rne(-g), -g)
    # ties go to the even code: midpoint between grid points i and i + 1 -> the one with an even index
    mid = (g[:-1] + g[1:]) / 2
    want = np.where(np.arange(31) % 2 == 0, g[:-1], g[1:])
    assert np.array_equal(mx.e2m3_rne(mid), want) and np.array_equal(mx.e2m3_rne(-mid), -want)
    # just off a tie: to the nearer neighbour
    assert np.array_equal(mx.e2m3_rne(mid + 1e-9), g[1:]) and np.array_equal(mx.e2m3_rne(mid - 1e-9), g[:-1])
    # saturation
    assert np.array_equal(mx.e2m3_rne([7.74, 7.75, 8.0, 100.0, 6e4, -7.76, -1e30]), [7.5, 7.5, 7.5, 7.5, 7.5, -7.5, -7.5])
    x = np.linspace(-7.5, 7.5, 4001)
    assert (np.abs(mx.e2m3_rne(x) - x) <= mx.e2m3_step(x) / 2).all()


def test_scale_rule():
    rng = np.random.default_rng(0)
    m = np.concatenate([np.ldexp(rng.uniform(1, 2, 4000), rng.integers(-20, 16, 4000)),
                        np.ldexp([1.0, 1.875, np.nextafter(np.float32(1.875), np.float32(2)), 1.9999999], 3)]).astype(np.float32)
    k = mx.scale_exponent(m)
    sm = m.astype(np.float64) * np.ldexp(1.0, -k)
    assert (sm <= 7.5).all() and (2 * sm > 7.5).all()         # the LARGEST power of two with s m <= 7.5
    assert k[-4:].tolist() == [1, 1, 2, 2]
    assert mx.scale_exponent(np.float32(0)) == 0
    assert mx.scale_exponent(np.float32(1e-38)) == mx.E8M0_MIN - 127
    # the bit trick of xv_split6_e8m0 is the same rule
    bits = m.view(np.int32).astype(np.int64)
    assert np.array_equal(((bits + 0x0FFFFF) >> 23) - 2 - 127, k)


def test_block_encoding_never_saturates_and_errs_by_half_a_step():
    rng = np.random.default_rng(1)
    v = (rng.standard_normal((3000, 16)) * np.ldexp(1.0, rng.integers(-12, 12, (3000, 1)))).astype(np.float32)
    v[:100] *= rng.random((100, 16)) < 0.3                   # sparse blocks
    v[100] = 0                                               # m = 0
    v[101, :] = 0
    v[101, 3] = 7e4                                          # clamped
    hi, lo_q, c_q, k = mx.encode_blocks(v)
    assert k[100] == 0 and not lo_q[100].any() and not c_q[100].any()
    c = np.clip(v, -em.SPLIT8_MAX, em.SPLIT8_MAX).astype(np.float64)
    lo = (c - hi) * em.LO_SCALE
    s = np.ldexp(1.0, -k)[:, None]
    assert c_q[101, 3] == 57344.0 and k[101] == 13           # 57344 = 1.75 2^15: s = 2^-13, 7.0 on the grid
    for val, q in ((lo, lo_q), (c, c_q)):
        assert (np.abs(q * s) <= mx.E2M3_MAX).all()
        assert np.isin(np.abs(q * s), mx.E2M3_GRID).all()
        assert (np.abs(q - val) * s <= mx.e2m3_step(val * s) / 2).all()
    # a block of one large and fifteen small values: only the large one keeps relative accuracy -- and only it matters to a dot product
    blk = np.full((1, 16), 1e-3, np.float32)
    blk[0, 0] = 5.0
    _, _, c_q, k = mx.encode_blocks(blk)
    assert k[0] == 0 and c_q[0, 0] == 5.0 and not c_q[0, 1:].any()


def test_block_channels_cover_every_channel_once():
    assert sorted(mx.BLOCK_CHANNELS.ravel().tolist()) == list(range(512))
    assert mx.BLOCK_CHANNELS[0].tolist() == [0, 1, 2, 3, 8, 9, 10, 11, 16, 17, 18, 19, 24, 25, 26, 27]
    assert mx.BLOCK_CHANNELS[3][0] == 36


def test_emulated_product_against_fp64_on_pair_data():
    """real_layer2 on the exactly known, live-plane H of pair_data.live_layer1: the emulated f16mx6 product within the bound the
    formats give (pair_mx6_data.product_error_bound).  The relative L2 figures of both emulations are printed (this H is made of
    small integers plus a low plane, which e5m2 holds exactly: not the data to rank the two formats on -- that is what
    tools/experiments/cross_term_mx6_sim.py and the GPU test on the whole network are for)."""
    d = pd.live_layer1("f16bf8", 64, "none", pd.seed("f16bf8", 64, "c"))
    H = d["H"][:101]
    for cout in (64, 192):
        l2 = pd.real_layer2(cout, "none", 3 + cout)
        exact = H.astype(np.float64) @ l2["w2"].astype(np.float64)
        z6 = sum(t[0] for t in mx.terms(H, l2["w2"]))
        z8 = sum(t[0] for t in pd.terms("f16bf8", H, l2["w2"]))
        bound = mx.product_error_bound(H, l2["w2"])
        assert (np.abs(z6 - exact) <= bound).all()
        e6, e8 = np.linalg.norm(z6 - exact) / np.linalg.norm(exact), np.linalg.norm(z8 - exact) / np.linalg.norm(exact)
        print("cout %d: rel L2 of the emulated product against fp64: e2m3 %.3e, bf8 %.3e; worst error / bound %.3f" %
              (cout, e6, e8, float((np.abs(z6 - exact) / bound).max())))
