"""CPU tests of the split-arithmetic emulator (tests/arith_emul.py): known-answer encodings, exactness on dyadic data against the
fp64 oracle, and a power check of the element-wise bounds tests/test_gpu_elementwise.py applies (on the data it uses)."""
import numpy as np
import pytest

import arith_emul as em
import elementwise_data as ed


def _f32(*v):
    return np.array(v, np.float32)


def test_bf16_known_answers():
    x = _f32(1 + 2 ** -8, 1 + 3 * 2 ** -8, 1 + 2 ** -8 + 2 ** -20, 3.0, 0.0, -0.0, -2.0 ** -130, 1 - 2 ** -9)
    assert [int(v) for v in em.bf16_rne(x)] == [0x3F80, 0x3F82, 0x3F81, 0x4040, 0, 0x8000, 0x8008, 0x3F80]   # ties to even
    hi, lo = em.split3(x)
    assert list(lo[:3]) == [2 ** -8, -2 ** -8, -2 ** -8] and lo[3] == 0 and lo[6] == 0      # lo of the third: bf16(2^-20 - 2^-8)
    keep = np.arange(8) != 2
    assert (hi.astype(np.float64) + lo == x)[keep].all()


def test_split8_known_answers():
    x = _f32(1 + 2 ** -11, 1 + 3 * 2 ** -11, 1e6, -7e4, 57344.0, 65504.0, 1e-7, 2 ** -24, 2 ** -25, 0.0, 3.0, 1.5 * 2 ** -14)
    hi, l8, h8 = em.split8_bytes(x)
    assert [int(v) for v in hi] == [0x3C00, 0x3C02, 0x7B00, 0xFB00, 0x7B00, 0x7B00, 0x0002, 0x0001, 0x0000, 0, 0x4200, 0x0600]
    assert [int(v) for v in l8] == [0x3C, 0xBC, 0, 0, 0, 0, 0x83, 0, 0x04, 0, 0, 0]
    assert [int(v) for v in h8] == [0x3C, 0x3C, 0x7B, 0xFB, 0x7B, 0x7B, 0x00, 0x00, 0x00, 0, 0x42, 0x06]
    # the ties: fp16 1 + 2^-11 -> 1 (even), 1 + 3 2^-11 -> 1 + 2^-9 (even); e5m2 1.125 -> 1, 1.375 -> 1.5, 2^-17 -> 0
    assert [int(v) for v in em.e5m2_bits(_f32(1.125, 1.375, 2 ** -17, 3 * 2 ** -17, -1.125))] == [0x3C, 0x3E, 0x00, 0x02, 0xBC]
    # an all-zero lo block: values with 11 significant bits leave every l8 zero
    blk = _f32(*(np.arange(8) * 0.25 - 1))
    assert not em.split8_bytes(blk)[1].any()
    assert (em.decode8(blk) == blk).all()
    # weight slots put h8 first
    slot = em.split8_weight_slot(_f32(*([1 + 3 * 2 ** -11] * 8)))
    assert list(slot[:8]) == [0x3C] * 8 and list(slot[8:]) == [0xBC] * 8


def test_split8_encoding_error_is_the_documented_one():
    rng = np.random.default_rng(1)
    x = (rng.standard_normal(100000) * np.exp(3 * rng.standard_normal(100000))).astype(np.float32)
    x = np.clip(x, -57344, 57344)
    err = np.abs(em.decode8(x).astype(np.float64) - x)
    assert (err <= np.abs(x) * em.ENC_SPLIT8 + em.U).all()
    err3 = np.abs(em.decode3(x).astype(np.float64) - x)
    assert (err3 <= np.abs(x) * em.ENC_SPLIT).all()


@pytest.mark.parametrize("arith", ["fp32", "bf16x3", "f16bf8"])
@pytest.mark.parametrize("K,dil", [(5, 1), (3, 3), (1, 1), (7, 1)])
def test_emulation_is_exact_on_dyadic_data(oracle_mod, arith, K, dil):
    """Integers times 2^-4 are exact in every representation (split8 lo = 0, bf16 lo = 0): the emulated contraction is then the
    exact one, equal to the fp64 oracle in every element."""
    rng = np.random.default_rng(K * 10 + dil)
    cin, cout = 40, 24
    alpha = np.array([0.25])
    for T in (1, 3, 25, 64):
        x = (rng.integers(-48, 49, (T, cin)) / 16).astype(np.float32)
        w = rng.integers(-3, 4, (K, cin, cout)).astype(np.float32)
        b = rng.integers(-5, 6, cout).astype(np.float32)
        y, zb, M = em.tdnn_layer(arith, x, w, b, None, None, "lrelu", alpha, dil)
        ref = oracle_mod.tdnn_layer(x, w, b, None, "lrelu", alpha, dil, np.float64)
        assert np.array_equal(y, ref)
        assert (M >= np.abs(zb)).all()


@pytest.mark.parametrize("case", ed.BOUND_CASES, ids=[c.name for c in ed.BOUND_CASES])
def test_bounds_have_power(case):
    """On the data the GPU test uses, against the bound it applies (output encoder included), on the first 12 rows of the first
    three chunks (the ends of a chunk, where the halo is, and a whole short chunk):
    (1) at every element the bound lies below half the median magnitude of that element's nonzero products x_c,k * w_c,k,o: dropping
        or doubling one median product cannot hide under it.  On hostile data (input channels over three decades) the median product
        is far below the rounding of the large ones; there the statement is made for the 90th percentile, so it covers only the
        largest tenth of the products;
    (2) for f16bf8, leaving out the cross terms (hi * hi alone) exceeds the bound on at least 90 % of the elements.  Not for split8
        outputs: their encoder error (2^-13 relative) is as large as the cross terms themselves, so no bound that contains it can see
        them; there the exact tests and the weight read-back carry the cross terms."""
    mats, w, b, scale, shift, alpha = case.data()
    K = w.shape[0]
    arith = case.arith if case.arith != "fp32tc" else "fp32"
    A = case.A()
    h = (K - 1) // 2
    for m in mats[:3]:
        y, zb, M = em.tdnn_layer(arith, m, w, b, scale, shift, case.act, alpha, case.dil)
        bnd = em.elementwise_bound(A, M, zb, y, scale, alpha, case.fmt)          # the bound the GPU test applies
        s = np.abs(np.broadcast_to(1.0 if scale is None else scale, (w.shape[2],))).astype(np.float64)
        a = np.abs(np.broadcast_to(1.0 if alpha is None else alpha, (w.shape[2],))).astype(np.float64)
        # the magnitude of one product at the output: |x w| scaled by the epilogue (alpha only where the output is negative)
        gain = s * np.where(zb > 0, 1.0, np.where(np.asarray(case.act) == "relu", 0.0, a)) if case.act != "none" else s
        for t in range(min(m.shape[0], 12)):
            win = np.stack([m[t + (k - h) * case.dil] if 0 <= t + (k - h) * case.dil < m.shape[0] else np.zeros(m.shape[1], np.float32)
                            for k in range(K)])                              # [K, Cin]
            prods = np.abs(win.astype(np.float64)[:, :, None] * w.astype(np.float64)).reshape(-1, w.shape[2])
            prods = np.where(prods > 0, prods, np.nan)
            # hostile data (channel scales over three decades): a median product is far below the rounding of the big ones, so
            # there the statement is made for the product at the 90th percentile
            med = np.nanpercentile(prods, 90, axis=0) if case.kind == "hostile" else np.nanmedian(prods, axis=0)
            live = np.isfinite(med) & (gain[t] > 0)
            assert (bnd[t][live] < 0.5 * med[live] * gain[t][live]).all(), (case.name, t)
        if case.arith == "f16bf8" and case.fmt != "split8":
            hi = em.split8(m)[0]
            whi = em.split8(w)[0]
            y0 = em.epilogue(em.contract("fp32", hi, whi, case.dil)[0], b, scale, shift, case.act, alpha)
            live = (gain > 0) & (M > np.abs(b))                           # elements the contraction reaches
            frac = (np.abs(y0 - y) > bnd)[live].mean()
            assert live.mean() > 0.3 and frac >= 0.9, (case.name, frac)
