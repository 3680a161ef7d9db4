"""The emulation of XV_FMT_SPLIT6 rows and of the f16mx6 layer's product (tests/layer_mx6_data.py): blocks of 16 consecutive
channels, the scale rule at its 1.875 boundary, the 2^-11 in the stored byte, and the emulated product against fp64 within the
bound the e2m3 grid's steps give -- at dilation 1 and, with answers written out by hand, at K = 3 and dilations 2 .. 4 -- and the two
input builders (edge_layout, hostile_rows).  CPU only; tests/test_gpu_layer_mx6.py holds the kernels to this emulation."""
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


# ---- dilation and K = 3: answers written out by hand ------------------------------------------------------------------------------
def test_missing_taps_with_dilation_and_chunks_shorter_than_the_halo():
    # K = 3, dilation 2, one chunk of 12 rows: taps at r - 2, r, r + 2
    m = lx.missing_taps(np.ones(12, np.uint8), 3, 2)
    assert m[0].tolist() == [True, False, False] and m[1].tolist() == [True, False, False] and not m[2:10].any()
    assert m[10].tolist() == [False, False, True] and m[11].tolist() == [False, False, True]
    # K = 3, dilation 3, a 2-frame chunk (rows 8, 9; halo 3) between two others: both outer taps fall into the gaps
    valid = np.zeros(24, np.uint8)
    valid[0:5], valid[8:10], valid[16:24] = 1, 1, 1
    m = lx.missing_taps(valid, 3, 3)
    assert m[8].tolist() == [True, False, True] and m[9].tolist() == [True, False, True]
    assert m[4].tolist() == [False, False, True] and m[1].tolist() == [True, False, False] and m[2].tolist() == [True, False, True]
    assert m[3].tolist() == [False, False, True] and m[16].tolist() == [True, False, False] and m[19].tolist() == [False, False, False]
    assert m[5].tolist() == [False, True, False] and m[12].tolist() == [False, True, True]      # gap rows: the centre tap is missing too
    # K = 5, dilation 2, a 3-frame chunk (rows 8 .. 10; halo 4): taps at r - 4, r - 2, r, r + 2, r + 4
    valid = np.zeros(24, np.uint8)
    valid[8:11] = 1
    m = lx.missing_taps(valid, 5, 2)
    assert m[8].tolist() == [True, True, False, False, True]
    assert m[9].tolist() == [True, True, False, True, True]
    assert m[10].tolist() == [True, False, False, True, True]


def test_contract_places_a_tap_at_its_dilated_offset():
    """One frame with a single 1.0 (its block's scale holds 1.0 exactly, lo' = 0), small integer weights: output row r - (t - h) d holds
    tap t's weight and nothing else."""
    for K, d in ((3, 2), (3, 3), (5, 2)):
        h = (K - 1) // 2
        x = np.zeros((24, 32), np.float32)
        x[12, 5] = 1.0
        w = np.zeros((K, 32, 16), np.float32)
        w[:, 5, :] = (np.arange(K)[:, None] + 1) * (np.arange(16)[None] + 1)
        z, M, parts = lx.contract(x, w, d)
        want = np.zeros((24, 16))
        for t in range(K):
            want[12 - (t - h) * d] = w[t, 5]
        assert np.array_equal(z, want) and np.array_equal(M, want) and not parts[1].any() and not parts[2].any()
        # the bound has the same support: a tap read at the wrong offset would bound the wrong rows
        b = lx.product_error_bound(x, w, d)
        assert np.array_equal(b > 0, want > 0)
    # dilation 1 is what the default still means
    assert np.array_equal(lx.contract(x, w)[0], lx.contract(x, w, 1)[0])


def test_emulated_dilated_layers_against_fp64_within_the_grid_bound():
    """K = 3 at dilations 1 .. 4 and K = 5 at dilation 2, 64 -> 32 channels, ReLU-like frames with zero gap rows: |emulated - exact|
    <= product_error_bound everywhere; the bound of another dilation does not hold the product (it is the dilation's own)."""
    rng = np.random.default_rng(5)
    for K, d in ((3, 1), (3, 2), (3, 3), (3, 4), (5, 2)):
        h = (K - 1) // 2 * d
        x = (np.maximum(rng.standard_normal((90, 64)), 0) * 1.3 * np.ldexp(1.0, rng.integers(-2, 3, (90, 1)))).astype(np.float32)
        x[40:40 + h] = 0
        w = (rng.standard_normal((K, 64, 32)) / np.sqrt(K * 64)).astype(np.float32)
        z, M, parts = lx.contract(x, w, d)
        exact = em.contract("fp32", x, w, d)[0]
        bound = lx.product_error_bound(x, w, d)
        ratio = float((np.abs(z - exact) / np.maximum(bound, 1e-300)).max())
        print("K = %d dilation %d: rel L2 of the emulated product against fp64 %.3e; worst error / bound %.3f" %
              (K, d, np.linalg.norm(z - exact) / np.linalg.norm(exact), ratio))
        assert (np.abs(z - exact) <= bound).all() and all(np.abs(p).sum() > 0 for p in parts)
        other = em.contract("fp32", x, w, d + 1)[0]
        assert not (np.abs(z - other) <= bound).all()


def test_edge_layout_has_short_chunks_and_crosses_the_tile():
    for K, d in ((3, 1), (3, 2), (3, 3), (3, 4), (5, 2), (5, 1), (7, 1)):
        h = (K - 1) // 2 * d
        valid, starts, lens = lx.edge_layout(K, d)
        assert lens == [1, 2, h, h + 1, 97, 3, 150] and all(s % 8 == 0 for s in starts) and valid.sum() == sum(lens)
        assert all(valid[s:s + n].all() and not valid[s + n:s + n + h].any() for s, n in zip(starts, lens)) and not valid[:h].any()
        assert starts[-1] < 256 < starts[-1] + lens[-1] and 296 <= len(valid) <= 320
        miss = lx.missing_taps(valid, K, d)[valid != 0]
        assert (miss.sum(1) > 1).any() and (miss[:, :K // 2].any(1) & miss[:, K // 2 + 1:].any(1)).any()
    assert lx.edge_layout(3, 3)[1] == [8, 16, 24, 32, 40, 144, 152] and len(lx.edge_layout(5, 2)[0]) == 320


def test_hostile_rows_sit_where_they_say():
    """The builder's own claims, from the emulator: the scale bytes of the tagged blocks (written out by hand), every tie of the grid
    in both halves, the rows beyond 57344 last."""
    rows, n_in, where = lx.hostile_rows()
    assert rows.shape[1] == 64 and 40 <= len(rows) <= 70
    assert np.abs(rows[:n_in]).max() == 57344.0 and (np.abs(rows[n_in:]).max(1) > 57344.0).all() and len(rows) > n_in
    hi, lo, c, k = lx.encode_rows(rows)
    byte = lambda tag: int(lx.stored_byte(k[where[tag]]))
    # 1.875 2^3 = 15: 1 / s = 2^1, the next fp32 2^2; one below still 2^1; 127 + k - 11
    assert (byte("edge below 3"), byte("edge at 3"), byte("edge above 3")) == (117, 117, 118)
    assert (byte("edge at -10"), byte("edge above -10")) == (104, 105) and byte("beyond:edge at 15") == 129    # (57344 = 1.75 2^15: k = 13)
    assert byte("zeros") == 116 and byte("1e-38") == 5 and byte("fp32 denormals") == 5 and mx.E8M0_MIN - 11 == 5
    assert not c[where["1e-38"][0], 16 * where["1e-38"][1]:][:16].any() and not lo[where["1e-38"][0], 16 * where["1e-38"][1]:][:16].any()
    assert byte("c ties k 0") == 116 and byte("c ties k 5") == 121 and byte("lo ties k -3") == 113 and byte("tiny lo ties j -17") == 99
    # every midpoint of the grid is met by an element of either half, under its block's scale
    s = np.repeat(np.ldexp(1.0, -k), 16, 1)
    cl = np.clip(rows, -em.SPLIT8_MAX, em.SPLIT8_MAX)
    lo_in = (cl - cl.astype(np.float16).astype(np.float32)).astype(np.float64) * em.LO_SCALE * s
    c_in = cl.astype(np.float64) * s
    for t in lx.E2M3_TIES:
        assert (lo_in == t).any() and (lo_in == -t).any() and (c_in == t).any() and (c_in == -t).any(), t
    assert np.abs(lo_in).max() <= 7.5 and np.abs(c_in).max() <= 7.5
    # fp16's subnormal range: lo' exceeds c there
    r, b = where["fp16 subnormal"]
    assert (np.abs(lo_in[r, 16 * b:16 * b + 16]) > np.abs(c_in[r, 16 * b:16 * b + 16])).sum() >= 5
