"""CPU companion of tests/test_gpu_backend_elementwise.py (no GPU): the exact fp32 fma of tests/backend_data.py against rational
arithmetic, the float32 replay of prepare against the bounds the device is held to, the size of those bounds against the terms
they guard, and the power of the assertion functions: each mutant of the issue, applied to a replay, fails the same functions
the device results go through."""
from fractions import Fraction

import numpy as np
import pytest

import backend_data as bd

F = np.float32


# ---------------------------------------------------------------------------------------------------------------------------
# fma32 against rational arithmetic
# ---------------------------------------------------------------------------------------------------------------------------
def _round_fp32(q):
    """Round the rational q to fp32, nearest even, in integer arithmetic (normal range only)."""
    if q == 0:
        return 0.0
    s = -1 if q < 0 else 1
    q = abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    assert Fraction(2) ** e <= q < Fraction(2) ** (e + 1) and -120 < e < 120
    scaled = q / Fraction(2) ** (e - 23)                     # in [2^23, 2^24)
    n, rem = divmod(scaled.numerator, scaled.denominator)
    twice = 2 * rem
    if twice > scaled.denominator or (twice == scaled.denominator and n & 1):
        n += 1
    return s * float(n) * 2.0 ** (e - 23)


def _triples(rng, n):
    a = (rng.standard_normal(n) * 2.0 ** rng.integers(-12, 13, n)).astype(F)
    b = (rng.standard_normal(n) * 2.0 ** rng.integers(-12, 13, n)).astype(F)
    c = (rng.standard_normal(n) * 2.0 ** rng.integers(-12, 13, n)).astype(F)
    q = n // 4                                               # a quarter: c close to -a b (the sum cancels to its last bits)
    p = a[:q].astype(np.float64) * b[:q].astype(np.float64)
    c[:q] = (-p * (1 + rng.integers(-4, 5, q) * 2.0 ** -24)).astype(F)
    # constructed exact ties: a b = 2^-24 * odd-ish half ulp of c = 1 + j 2^-23: a = 2^-12, b = 2^-12 -> a b = 2^-24 = ulp(c)/2
    t = n // 20
    j = rng.integers(0, 2 ** 23, t)
    c[q:q + t] = (1.0 + j * 2.0 ** -23).astype(F)
    a[q:q + t] = F(2.0 ** -12) * rng.choice([-1, 1], t).astype(F)
    b[q:q + t] = F(2.0 ** -12)
    # and near-ties below float64's reach: a b = +-2^-24 (1 - 2^-46), half an ulp of c less 2^-70, which a float64 addition
    # rounds to the tie itself (a cast of that sum then rounds to even where the exact value rounds towards c)
    a[q + t:q + 2 * t] = F(2.0 ** -12) * (F(1) + F(2.0 ** -23)) * rng.choice([-1, 1], t).astype(F)
    b[q + t:q + 2 * t] = F(2.0 ** -12) * (F(1) - F(2.0 ** -23))
    c[q + t:q + 2 * t] = (1.0 + rng.integers(0, 2 ** 23, t) * 2.0 ** -23).astype(F)
    return a, b, c


def test_fma32_matches_rational_arithmetic():
    rng = np.random.default_rng(20)
    a, b, c = _triples(rng, 100000)
    got = bd.fma32(a, b, c)
    assert got.dtype == F
    n_tie = 0
    for i in range(len(a)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        want = _round_fp32(exact)
        assert float(got[i]) == want, (i, float(a[i]), float(b[i]), float(c[i]), float(got[i]), want)
        if exact != 0:
            lo = Fraction(want)
            n_tie += abs(exact - lo) * 2 == Fraction(abs(float(np.spacing(F(want)))))
    assert n_tie >= 2000, n_tie                              # the constructed ties are ties
    # the naive float64 add-and-cast differs somewhere on this set: the test set can tell a double rounding
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)
    assert np.any(naive != got)
    # broadcasting and the fp32 add as fma(acc, 1, r)
    x = rng.standard_normal(1000).astype(F)
    y = rng.standard_normal(1000).astype(F)
    assert np.array_equal(bd.fma32(x, F(1), y), x + y)


# ---------------------------------------------------------------------------------------------------------------------------
# the scorer assertions have power
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dataset", ["plda", "cancel"])
@pytest.mark.parametrize("kpad", [40, 200])
def test_stored_order_mutant_fails_the_bit_test(dataset, kpad):
    case = bd.scorer_case(dataset, kpad, 33, 31)
    bd.assert_bits_equal(bd.replay_scores(case["E"], case["T"], case["r"]), case["want_r"], "clean replay")
    mut = bd.replay_scores(case["E"], case["T"], case["r"], mutant="stored_order")
    with pytest.raises(AssertionError):
        bd.assert_bits_equal(mut, case["want_r"], "stored order")
    share = float(np.mean(bd.bits(mut) != bd.bits(case["want_r"])))
    print("stored-order mutant, %s kpad %d: %.1f %% of the scores change bits" % (dataset, kpad, 100 * share))
    assert share > 0.2


@pytest.mark.parametrize("kpad", [8, 40, 72, 200])
def test_dropped_ragged_group_fails_integer_and_onehot(kpad):
    E, T, r = bd.integer_operands(kpad, 33, 31)
    bd.assert_integer_scores(bd.replay_scores(E, T, r), E, T, r, "clean")
    with pytest.raises(AssertionError):
        bd.assert_integer_scores(bd.replay_scores(E, T, r, mutant="drop_ragged_group"), E, T, r, "dropped group")
    eye, other = bd.onehot_operands(kpad, 37)
    bd.assert_onehot_scores(bd.replay_scores(eye, other), other, False, "clean")
    bd.assert_onehot_scores(bd.replay_scores(other, eye), other, True, "clean swapped")
    with pytest.raises(AssertionError):
        bd.assert_onehot_scores(bd.replay_scores(eye, other, mutant="drop_ragged_group"), other, False, "dropped group")
    with pytest.raises(AssertionError):
        bd.assert_onehot_scores(bd.replay_scores(other, eye, mutant="drop_ragged_group"), other, True, "dropped group")


def test_scorer_shapes_cover_the_issue():
    assert {a for a, _ in bd.EDGE_SHAPES} == {b for _, b in bd.EDGE_SHAPES} == {1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257}
    assert (1, 257) in bd.EDGE_SHAPES and (257, 1) in bd.EDGE_SHAPES
    assert {min(32, k - k // 32 * 32 or 32) // 8 for k in bd.KPADS} == {1, 2, 3, 4}          # 8-k groups of the last slice
    for m in bd.PAIR_COUNTS:
        ei, ti = bd.pair_list(m, 129, 131)
        pairs = list(zip(ei.tolist(), ti.tolist()))
        assert (0, 0) in pairs and (m == 1 or (128, 130) in pairs) and (m < 5 or len(set(pairs)) < m)


# ---------------------------------------------------------------------------------------------------------------------------
# prepare: the replay against the bounds, the bounds against the terms
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bounded_cases():
    return [(c, bd.prepare_bounds(c, with_terms=True)) for c in bd.prepare_cases()]


def test_prepare_cases_cover_the_issue():
    assert {s[0] for s in bd.SHAPES} == {1, 2, 31, 33, 64, 65, 150, 600, 2048}
    assert {s[1] for s in bd.SHAPES} == {1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 150, 255, 256}
    assert {s[2] for s in bd.SHAPES} == {1, 31, 32, 33, 97}


def test_prepare_replay_within_half_the_bound(bounded_cases):
    worst = {}
    for case, bounds in bounded_cases:
        rows, r = bd.prepare_replay(case)
        wr = bd.assert_prepare_within(rows, r, bounds, case["name"], limit=0.5)
        combo = case["name"].split()[0]
        worst[combo] = tuple(max(a, b) for a, b in zip(worst.get(combo, (0, 0)), wr))
    print("\nfloat32 replay of prepare, worst |replay - ref| / bound at LAMBDA = %d (rows, r):" % bd.LAMBDA)
    for k, v in worst.items():
        print("  %-20s %.3f %.3f" % (k, v[0], v[1]))


def test_lambda_is_the_smallest_that_holds():
    """LAMBDA is the smallest of {1, 2, 4} for which the replay stays at or below half of every bound."""
    def holds(lam):
        try:
            for case in bd.prepare_cases():
                rows, r = bd.prepare_replay(case)
                bd.assert_prepare_within(rows, r, bd.prepare_bounds(case, lam), case["name"], limit=0.5)
        except AssertionError:
            return False
        return True
    smaller = [lam for lam in (1, 2, 4) if lam < bd.LAMBDA]
    assert bd.LAMBDA in (1, 2, 4) and not any(holds(lam) for lam in smaller)


def test_product_bounds_stay_below_half_the_median_term(bounded_cases):
    worst = 0.0
    for case, bounds in bounded_cases:
        for name, e, med in bounds["products"]:
            live = med > 0
            ratio = float((e[live] / med[live]).max()) if live.any() else 0.0
            worst = max(worst, ratio)
            assert ratio < 0.5, (case["name"], name, ratio)
    print("worst product bound / median |term|: %.3e" % worst)


def test_enrol_without_counts_replays_as_counts_of_one():
    case = bd.realistic_case("enrol_no_counts", 150, 64, 33)
    ones = dict(case, n=np.ones(33, np.int32))
    a, b = bd.prepare_replay(case), bd.prepare_replay(ones)
    bd.assert_bits_equal(a[0], b[0], "rows")
    bd.assert_bits_equal(a[1], b[1], "r")


# ---------------------------------------------------------------------------------------------------------------------------
# prepare: the mutants
# ---------------------------------------------------------------------------------------------------------------------------
def _mutant_share(case, mutant, cols=None, with_r=False):
    """The share of the affected elements over their bound.  Affected: the elements the mutant changes at all (any bit of the
    clean replay), within ``cols`` when given."""
    bounds = bd.prepare_bounds(case)
    clean_rows, clean_r = bd.prepare_replay(case)
    bd.assert_prepare_within(clean_rows, clean_r, bounds, case["name"], limit=0.5)
    rows, r = bd.prepare_replay(case, mutant)
    aff = bd.bits(rows) != bd.bits(clean_rows)
    if cols is not None:
        keep = np.zeros(rows.shape[1], bool)
        keep[cols] = True
        aff &= keep[None, :]
    aff_r = (bd.bits(r) != bd.bits(clean_r)) if with_r else None
    share, total = bd.fraction_over(rows, r, bounds, aff, aff_r)
    with pytest.raises(AssertionError):
        bd.assert_prepare_within(rows, r, bounds, case["name"])
    err = np.abs(rows.astype(np.float64) - bounds["rows"])
    factor = float(np.median((err / np.maximum(bounds["brows"], 1e-300))[aff])) if aff.any() else 0.0
    print("mutant %-16s on %-34s %5d affected, %.1f %% over the bound, median error / bound %.3g" % (
        mutant, case["name"], total, 100 * share, factor))
    assert total > 0
    return share


@pytest.mark.parametrize("combo", ["plain_lda", "full_enrol"])
@pytest.mark.parametrize("D,d,N", [(33, 32, 33), (150, 129, 33), (65, 63, 31)])
def test_mutant_mu_not_subtracted_in_the_ragged_slice(combo, D, d, N):
    assert _mutant_share(bd.realistic_case(combo, D, d, N), "mu_ragged") >= 0.9


@pytest.mark.parametrize("D,d,N", [(64, 33, 97), (150, 129, 33), (600, 150, 97), (65, 63, 31)])
def test_mutant_a0_left_out_behind_the_last_full_block(D, d, N):
    case = bd.realistic_case("plain_lda", D, d, N)
    case["length_norm"] = False                              # the affected elements are then the columns themselves
    assert _mutant_share(case, "a0_tail", cols=np.arange(32 * (d // 32), d)) >= 0.9
    assert _mutant_share(bd.realistic_case("full_test", D, d, N), "a0_tail") >= 0.9


@pytest.mark.parametrize("combo", ["plain_lda", "cosine_raw", "full_enrol"])
@pytest.mark.parametrize("D,d,N", [(64, 65, 32), (150, 129, 33), (600, 150, 97), (2048, 255, 31)])
def test_mutant_norm_sum_misses_the_tail_lanes(combo, D, d, N):
    assert _mutant_share(bd.realistic_case(combo, D, d, N), "norm_tail_lanes") >= 0.9


@pytest.mark.parametrize("D,d,N", [(64, 33, 97), (150, 129, 33), (2, 2, 31)])
def test_mutant_psi_plus_one(D, d, N):
    case = bd.realistic_case("full_enrol", D, d, N)
    case["n"] = np.maximum(case["n"], 2)                     # n = 1 is where psi + 1 is right
    assert _mutant_share(case, "psi_plus_one") >= 0.9


@pytest.mark.parametrize("D,d,N", [(64, 33, 97), (150, 129, 33), (1, 1, 1)])
def test_mutant_v_and_w_swapped(D, d, N):
    case = bd.realistic_case("full_enrol", D, d, N)
    assert _mutant_share(case, "vw_swapped", cols=np.arange(d, 2 * d)) >= 0.9
