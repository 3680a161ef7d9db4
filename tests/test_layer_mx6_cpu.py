"""The emulation of XV_FMT_SPLIT6 rows and of the f16mx6 layer's product (tests/layer_mx6_data.py): blocks of 16 consecutive
channels, the scale rule at its 1.875 boundary, the 2^-11 in the stored byte, and the emulated product against fp64 within the
bound the e2m3 grid's steps give.  CPU only; tests/test_gpu_layer_mx6.py holds the kernels to this emulation."""
import numpy as np

import arith_emul as em
import layer_mx6_data as lx
import pair_mx6_data as mx


def test_blocks_are_sixteen_consecutive_channels():
    """One large value moves the scale of its own block only: channels 16 .. 31, not 0 .. 15 or 32 .. 47."""
    v = np.full((2, 64), 0.25, np.float32)
    v[0, 17] = 100.0
    hi, lo, c, k = lx.encode_rows(v)
    assert k.shape == (2, 4) and k[0].tolist() == [-4, 4, -4, -4] and k[1].tolist() == [-4] * 4
    assert c[0, 17] == 96.0 and not c[0, 16:32][np.arange(16) != 1].any()        # 100 -> 6.0 2^4 (step 8); 0.25 is below half a step
    assert (c[0, :16] == 0.25).all() and (c[0, 32:] == 0.25).all() and (c[1] == 0.25).all()
    # the weight side: blocks run along the input channels of one tap and column
    w = np.full((3, 32, 4), 0.5, np.float32)
    w[1, 20, 2] = 64.0
    wh, wl, wc = lx.weight_planes(w)
    assert wc[1, 20, 2] == 64.0 and not wc[1, 16:32, 2][np.arange(16) != 4].any()
    assert (wc[1, :16, 2] == 0.5).all() and (wc[0] == 0.5).all() and (wc[1, :, 3] == 0.5).all()


def test_scale_rule_at_the_boundary_and_the_byte():
    """m = 1.875 2^e still takes 1 / s = 2^(e - 2) (1.875 2^2 = 7.5, the largest e2m3); the next fp32 takes 2^(e - 1).  The stored
    byte of an activation block is 127 + k - 11, never below XV_SPLIT6_E8M0_MIN - 11 = 5, and 116 for a block of zeros."""
    edge = np.float32(1.875 * 8)
    over = np.nextafter(edge, np.float32(100))
    v = np.zeros((4, 16), np.float32)
    v[0, 3], v[1, 3], v[2, 3] = edge, over, np.float32(1e-38)
    hi, lo, c, k = lx.encode_rows(v)
    assert k[:, 0].tolist() == [1, 2, mx.E8M0_MIN - 127, 0]
    assert c[0, 3] == 15.0 and c[1, 3] == 15.0                      # 7.5 2^1; 15.000001 / 4 = 3.75 + a bit: 3.75 2^2 (step 0.25 there)
    assert lx.stored_byte(k[:, 0]).tolist() == [117, 118, mx.E8M0_MIN - 11, 116] and mx.E8M0_MIN - 11 > 0
    assert not c[2].any() and not lo[2].any()
    # the byte carries the 2^-11: elements x 2^(byte - 127) is what the cross term needs, 2^-11 lo' q
    q = lo[0] * np.ldexp(1.0, -int(k[0, 0]))                          # the elements as stored
    assert np.array_equal(q * np.ldexp(1.0, int(lx.stored_byte(k[0, 0])) - 127), lo[0] / em.LO_SCALE)


def test_decode_is_hi_plus_quantised_lo():
    rng = np.random.default_rng(2)
    v = (rng.standard_normal((200, 64)) * np.ldexp(1.0, rng.integers(-6, 8, (200, 4)).repeat(16, 1))).astype(np.float32)
    v[5] = 0
    v[6, 3] = 7e4                                                   # clamped
    d, cq = lx.decode_rows(v)
    c = np.clip(v, -em.SPLIT8_MAX, em.SPLIT8_MAX)
    bm = np.repeat(np.abs(c).reshape(200, 4, 16).max(-1), 16, -1).astype(np.float64)
    # |decode - c| <= 2^-11 (half a step of the block) <= 2^-11 m / 15; |c_q - c| <= m / 15
    assert (np.abs(d.astype(np.float64) - c) <= 2.0 ** -11 * bm / 15 + 2.0 ** -24 * np.abs(c)).all()
    assert (np.abs(cq.astype(np.float64) - c) <= bm / 15).all()
    assert not d[5].any() and d[6, 3] == 57344.0
    # no worse than the split8 row it replaces, on the same data (its lo plane keeps 2 mantissa bits, e2m3 up to 3 under the block's scale)
    e6 = np.linalg.norm(d.astype(np.float64) - c)
    e8 = np.linalg.norm(em.decode8(c).astype(np.float64) - c)
    print("decode error over 200 x 64 values: split6 %.3e, split8 %.3e" % (e6, e8))


def test_emulated_layer_against_fp64_within_the_grid_bound():
    """K = 5 and 7, 64 -> 32 channels, ReLU-like frames with zero gap rows: |emulated - exact| <= product_error_bound everywhere."""
    rng = np.random.default_rng(3)
    for K in (5, 7):
        x = (np.maximum(rng.standard_normal((90, 64)), 0) * 1.3).astype(np.float32)
        x[40:43] = 0
        w = (rng.standard_normal((K, 64, 32)) / np.sqrt(K * 64)).astype(np.float32)
        z, M, parts = lx.contract(x, w)
        exact = em.contract("fp32", x, w)[0]
        bound = lx.product_error_bound(x, w)
        assert (np.abs(z - exact) <= bound).all()
        z8 = em.contract("f16bf8", x, w)[0]
        print("K = %d: rel L2 of the emulated product against fp64: e2m3 %.3e, bf8 %.3e; worst error / bound %.3f" %
              (K, np.linalg.norm(z - exact) / np.linalg.norm(exact), np.linalg.norm(z8 - exact) / np.linalg.norm(exact),
               float((np.abs(z - exact) / np.maximum(bound, 1e-300)).max())))
        assert all(np.abs(p).sum() > 0 for p in parts)


def test_missing_taps():
    valid = np.ones(20, np.uint8)
    valid[8:10] = 0
    m = lx.missing_taps(valid, 5)
    assert m[0].tolist() == [True, True, False, False, False] and m[19].tolist() == [False, False, False, True, True]
    assert m[7].tolist() == [False, False, False, True, True] and m[10].tolist() == [True, True, False, False, False]
    assert not m[3].any()
