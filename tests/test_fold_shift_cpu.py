"""The algebra of the BN-shift fold (engine.shift_tap_table / engine.folded_row_bias) against a plain fp64 forward that adds
the shifts to the stored activations: a producer that stores u = scale * relu(z + b) without its shift, and a consumer whose bias
carries the shift's share per tap, give the consumer's pre-activation of the unfolded network -- at the chunk edges too, where
SAME padding reads zeros and not the shift.  No GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "x-vector-kaldi-tf_amd"))
from xvector_amd import engine  # noqa: E402

LENGTHS = [1, 2, 4, 9, 61]          # shorter than K (taps missing on both sides at once) up to well inside
GAP = 3                             # = the largest halo of the cases below
CASES = [(5, 1), (7, 1), (3, 2), (1, 1)]
C = 8
REL = 1e-12


def _layout():
    lay = engine.BatchLayout(LENGTHS, GAP, 1)
    valid = lay.row_valid()
    # the first chunk directly behind the lead rows, the last one ending ``gap`` rows before the end of the batch
    assert lay.lead == GAP and lay.row_start[0] == GAP and valid[GAP - 1] == 0 and valid[GAP] == 1
    assert lay.row_start[-1] + lay.row_len[-1] == lay.rows - GAP and valid[lay.rows - GAP - 1] == 1 and not valid[lay.rows - GAP:].any()
    return lay, valid


def _data(K, seed):
    rng = np.random.default_rng(seed)
    lay, valid = _layout()
    u = np.maximum(rng.standard_normal((lay.rows, C)), 0.0) * rng.uniform(0.5, 2.0, C)     # scale * relu(.): half of it zeros
    u *= valid[:, None]                                                                     # gap rows store 0
    shift = rng.standard_normal(C) * 0.7                                                    # both signs
    assert (shift > 0).any() and (shift < 0).any()
    w = rng.standard_normal((K, C, C)) / np.sqrt(K * C)
    bias = rng.standard_normal(C)
    return lay, valid, u, shift, w, bias


def _conv_same(x, w, dil):
    """sum_t x[r + (t - left) * dil] . w[t] with zeros outside [0, R) (fp64)."""
    K = w.shape[0]
    R = x.shape[0]
    halo = (K - 1) // 2 * dil
    xp = np.concatenate([np.zeros((halo, x.shape[1])), x, np.zeros((halo, x.shape[1]))])
    out = np.zeros((R, w.shape[2]))
    for t in range(K):
        out += xp[t * dil: t * dil + R] @ w[t]
    return out


@pytest.mark.parametrize("K,dil", CASES)
def test_folded_consumer_equals_forward_with_shifts(K, dil):
    lay, valid, u, shift, w, bias = _data(K, 100 * K + dil)
    y = (u + shift[None, :]) * valid[:, None]                   # what the unfolded producer stores: shift on frames, 0 on gap rows
    want = _conv_same(y, w, dil) + bias[None, :]
    taps = engine.shift_tap_table(w, shift)
    assert taps.shape == (K, C) and taps.dtype == np.float64
    got = _conv_same(u, w, dil) + engine.folded_row_bias(bias, taps, valid, dil)
    scale = np.abs(want).max()
    assert np.abs(got - want).max() <= REL * scale
    # every kind of row occurs: all taps there, some missing on the left, on the right, on both sides at once
    if K > 1:
        left = (K - 1) // 2
        vp = np.concatenate([np.zeros(left * dil), valid, np.zeros(left * dil)])
        miss_l = np.array([[vp[r + t * dil] == 0 for t in range(left)] for r in range(lay.rows)]).any(axis=1) & (valid == 1)
        miss_r = np.array([[vp[r + t * dil] == 0 for t in range(left + 1, K)] for r in range(lay.rows)]).any(axis=1) & (valid == 1)
        assert (miss_l & miss_r).any() and (miss_l & ~miss_r).any() and (~miss_l & miss_r).any() and (~miss_l & ~miss_r & (valid == 1)).any()


@pytest.mark.parametrize("K,dil", CASES)
def test_kernel_form_full_bias_minus_missing_taps(K, dil):
    """What the GEMM epilogue computes: bias_full = bias + sum_t c_t, less the c_t of a row's missing taps."""
    lay, valid, u, shift, w, bias = _data(K, 200 * K + dil)
    taps = engine.shift_tap_table(w, shift)
    full = bias + taps.sum(axis=0)
    left = (K - 1) // 2
    rows = engine.folded_row_bias(bias, taps, valid, dil)
    for r in np.nonzero(valid)[0]:
        b = full.copy()
        for t in range(K):
            q = r + (t - left) * dil
            if q < 0 or q >= lay.rows or not valid[q]:
                b -= taps[t]
        assert np.abs(b - rows[r]).max() <= REL * max(np.abs(rows[r]).max(), 1.0)


@pytest.mark.parametrize("K,dil", CASES)
def test_sum_of_taps_is_the_interior_correction(K, dil):
    lay, valid, u, shift, w, bias = _data(K, 300 * K + dil)
    taps = engine.shift_tap_table(w, shift)
    halo = (K - 1) // 2 * dil
    r = int(lay.row_start[-1]) + 30                              # well inside the 61-frame chunk
    assert valid[r - halo: r + halo + 1].all()
    rows = engine.folded_row_bias(bias, taps, valid, dil)
    want = bias + taps.sum(axis=0)
    assert np.abs(rows[r] - want).max() <= REL * np.abs(want).max()
    # and that is exactly the shift seen through all taps of the weights
    direct = np.einsum("c,kco->o", shift, w)
    assert np.abs(taps.sum(axis=0) - direct).max() <= REL * max(np.abs(direct).max(), 1.0)


def test_k1_consumer_gets_a_constant_only():
    lay, valid, u, shift, w, bias = _data(1, 7)
    taps = engine.shift_tap_table(w, shift)
    rows = engine.folded_row_bias(bias, taps, valid, 1)
    on_frames = rows[valid == 1]
    assert (on_frames == on_frames[0]).all()
    assert np.abs(on_frames[0] - (bias + shift @ w[0])).max() <= REL * np.abs(on_frames[0]).max()
