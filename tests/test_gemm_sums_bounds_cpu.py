"""CPU companion of tests/test_gpu_gemm_sums_elementwise.py: what that module relies on is settled here, without a GPU.

* the case table reaches every form, (K, dilation), row count, width and argument combination it has to, each form by
  launch_gemm3's own condition (whose source lines are pinned);
* the replay of the epilogue's summation order (tests/gemm_sums_data.py: fp32 per thread and double across the groups for _sums,
  double throughout for _moments) reproduces the fp64 reference of every exact case bit for bit with every fp32 intermediate exact
  and under 24 bits -- and stops being exact at a neighbouring non-dyadic case (alpha = 0.3);
* on every bound case the replay lies inside the bound;
* nine deliberately broken replays are fed to the GPU module's own checker; every one that changes the answer is rejected, on at
  least one case per form; the one that only changes the ORDER of a thread's rows (8 g + j instead of g + 16 j) has the same answer
  in exact arithmetic, so it must still PASS the exact cases -- that is asserted too;
* the checker looks at every slot of every case: one slot off by one unit, or left unwritten, fails it."""
import os

import numpy as np

import bnback_data as bd
import gemm_sums_data as gd
import test_gpu_gemm_sums_elementwise as gpu

F = np.float32
ALL_CASES = gd.EXACT_CASES + gd.BOUND_CASES
SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "x-vector-kaldi-tf_amd", "csrc", "xv_gemm3.hip")


def _fails(fn, *args, **kw):
    try:
        fn(*args, **kw)
    except AssertionError:
        return True
    return False


_BUILT = {}


def _built(case):
    """(d, rows, good replay) of a case, computed once and left unchanged."""
    if case.name not in _BUILT:
        d = gd.build(case)
        rows = gd.layer_rows(case, d)
        _BUILT[case.name] = (d, rows, gd.replay_parts(case.entry, rows["y"], d["sum_r"]))
    return _BUILT[case.name]


def _replay(case, broken=None, track=None):
    d, rows, _ = _built(case)
    _, _, ldr, rcol, _, _ = gd.geometry(case)
    parent = gd.wide_of(d["sum_r"], ldr, rcol) if case.entry == "sums" else None
    return gd.replay_parts(case.entry, rows["y"], d["sum_r"], broken, y_raw=rows["y_raw"], r_parent=parent, r_col0=rcol, track=track)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


# ---------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_launcher_rules_the_forms_are_derived_from_are_the_source_s():
    src = open(SOURCE).read()
    assert "const bool s16 = p.x_split && kt > 1 && (p.n_chunks & 1) == 0;" in src
    assert "if (p.cs_part) wm = 2;" in src
    assert "constexpr int NG = NT / 16;" in src and "const int lr = (tid >> 4) + (NT / 16) * j;" in src
    assert "cs2[i] = __builtin_fmaf(v[i], i < 4 ? rq[j][0][i] : rq[j][1][i - 4], cs2[i]);" in src
    assert "ds2[i] = __builtin_fma(d, d, ds2[i]);" in src


def test_the_exact_cases_reach_every_form_shape_and_argument():
    names = [c.name for c in ALL_CASES]
    assert len(set(names)) == len(names)
    for entry in ("sums", "moments"):
        cases = [c for c in gd.EXACT_CASES if c.entry == entry]
        assert {c.form for c in cases} == set(gd.FORMS)
        assert {c.valid for c in cases} == {True, False} and {c.wide for c in cases} == {True, False}
    ex = gd.EXACT_CASES
    for c in ALL_CASES:
        assert gd.form_of(c.split, c.K, c.cin, c.dil) == c.form and c.cout % 8 == 0
        R, valid = gd.rows_of(c)
        assert R <= 1000 and valid.any()
    assert {(c.K, c.dil) for c in ex} == gd.NEED_TAPS
    assert {c.rows for c in ex} == gd.NEED_ROWS and {c.cout for c in ex} == gd.NEED_COUT
    assert any(c.form == "f32" for c in ex)                                            # fp32 rows: always with ldx > cin (Staged)
    assert {1} <= {c.K for c in ex if c.form == "split32"} and any(c.K > 1 and -(-c.cin // 32) % 2 for c in ex if c.form == "split32")
    assert {c.K for c in ex if c.form == "split16"} == {3, 5, 7}
    assert {c.cin for c in ex if c.form == "split16"} == {64, 128} and {c.cin for c in ex if c.form == "split32"} == {32, 96}
    mom = [c for c in ex if c.entry == "moments"]
    assert {c.act for c in mom} >= {"relu", "lrelu", "prelu"} and {c.ypre for c in mom} == {True, False}
    sums = [c for c in ex if c.entry == "sums"]
    assert any(c.epi and c.act != "none" for c in sums) and any(not c.epi for c in sums)
    assert any(c.form == "split16" and c.K in (5, 7) and not c.epi for c in sums)      # the trainer's K = 5 / 7 input-gradient GEMMs
    # a last column tile with 1 and with 8 live 8-column groups, two column tiles
    assert {(c % 128) // 8 for c in gd.NEED_COUT} >= {1, 8} and max(gd.NEED_COUT) > 128
    # the ragged layout: a gap and chunks over the tile boundaries, a short last tile; the gap-tile layout: tile 1 holds no frame
    R, valid = gd.rows_of(gd.Case("", "sums", "f32", 4, 8, 1, 1, "ragged", True, "none", False))
    assert 600 <= R <= 800 and R % 128 and not valid[127] and not valid[128] and valid[126] and valid[130]
    assert all(valid[b - 1] and valid[b] for b in (256, 384, 512, 640))
    R, valid = gd.rows_of(gd.Case("", "sums", "f32", 4, 8, 1, 1, "gaptile", True, "none", False))
    assert not valid[128:256].any() and valid[:128].any() and valid[256:].any()
    # bound cases: each form with K = 5 and K = 7, about 700 rows, both entry points
    for entry in ("sums", "moments"):
        assert {(c.form, c.K) for c in gd.BOUND_CASES if c.entry == entry} == {(f, k) for f in gd.FORMS for k in (5, 7)}
    for c in ALL_CASES:
        d = gd.build(c)
        assert gd.workspace_bytes(d["R"], c.cout) == -(-d["R"] // 128) * 2 * c.cout * 8
        if c.entry == "sums" and c.valid and not d["valid"].all():
            assert (np.abs(d["sum_r"][~d["valid"]]) == F(gd.BIG)).all() and np.isfinite(d["sum_r"]).all()
        if not c.exact and d["b"] is not None:
            assert d["b"][gd.LARGE_MEAN_CHANNEL] == 300


# ---------------------------------------------------------------------------------------------------------------------------
# the replay
# ---------------------------------------------------------------------------------------------------------------------------
def test_replay_reproduces_every_exact_case_with_exact_intermediates():
    for case in gd.EXACT_CASES:
        d, rows, good = _built(case)
        gpu.check_parts(case, d, rows["y"], good)
        ref, mag = gd.parts_ref(case.entry, rows["y"], d["sum_r"])
        assert _same_bits(good + 0.0, ref + 0.0), case.name
        y8 = rows["y"].astype(np.float64) * 8
        assert np.array_equal(y8, np.round(y8)) and np.abs(y8).max() < 2 ** 17 + 32, case.name     # multiples of 1/8 below 2^14
        if case.entry == "sums":
            track = {}
            _replay(case, track=track)
            assert track["inexact"] == 0 and track["max"] * 8 < 2 ** 24, (case.name, track)
            assert track["max"] * 8 < 2 ** 22                                                       # the docstring's worst case
        else:
            assert (mag * 64).max() < 2 ** 53 and np.array_equal(mag * 64, np.round(mag * 64)), case.name
        if case.rows == "gaptile":
            assert (good[1] == 0).all()
        if not d["valid"].all():                       # the unmasked rows differ in the gap rows: the mask is what keeps them out
            assert (rows["y_raw"][~d["valid"]] != 0).any(), case.name


def test_a_neighbouring_non_dyadic_case_is_not_exact():
    """alpha = 0.3: alpha z is no short dyadic number any more, the fp32 sums round, and the equality check fails."""
    for name in ("sums f32 K3d2 R127 cout136 lrelu epi", "sums split16 K5d2 R1 cout8 lrelu epi", "moments f32 K3d4 R129 cout8 lrelu"):
        case = next(c for c in gd.EXACT_CASES if c.name == name)
        near = case.but(alpha=0.3, name=name + " alpha 0.3")
        d = gd.build(near)
        rows = gd.layer_rows(near, d)
        track = {}
        parts = gd.replay_parts(near.entry, rows["y"], d["sum_r"], track=track)
        if near.entry == "sums" and d["R"] > 1:
            assert track["inexact"] > 0
            assert _fails(gpu.check_parts, near, d, rows["y"], parts)
        y8 = rows["y"].astype(np.float64) * 8
        assert not np.array_equal(y8, np.round(y8))


def test_replay_lies_inside_every_bound():
    worst = {}
    for case in gd.BOUND_CASES:
        d, rows, good = _built(case)
        gpu.check_parts(case, d, rows["y"], good, lambda k, v: worst.__setitem__(k, v))
        assert 0 < worst[case.name] <= 1
        if case.entry == "sums":                          # the fp32 sums do round: the bound is not idle
            assert worst[case.name] > 0.01, (case.name, worst[case.name])
    print("\nworst |replay - ref| / bound per case:")
    for k, v in worst.items():
        print("  %-44s %.3e" % (k, v))


# ---------------------------------------------------------------------------------------------------------------------------
# the power of the checker
# ---------------------------------------------------------------------------------------------------------------------------
def _rejected_per_form(broken, cases):
    """Feeds the broken replay of every case to the checker.  A case passes only where the variant leaves every slot's bits as they
    were (nothing to see there: R = 1 has no row in group 15, a contiguous sum_r no other stride, ...).  -> forms with a rejection."""
    forms = set()
    for case in cases:
        d, rows, good = _built(case)
        parts = _replay(case, broken)
        if _fails(gpu.check_parts, case, d, rows["y"], parts):
            forms.add((case.entry, case.form))
        else:
            assert _same_bits(parts + 0.0, good + 0.0), (broken, case.name, "a changed answer passed the checker")
    return forms


def _every_form(entries):
    return {(e, f) for e in entries for f in gd.FORMS}


def test_row_group_15_dropped_is_rejected():
    assert _rejected_per_form("drop15", ALL_CASES) == _every_form(("sums", "moments"))


def test_gap_rows_not_masked_is_rejected():
    assert _rejected_per_form("gaps", ALL_CASES) == _every_form(("sums", "moments"))


def test_sum_r_read_with_stride_cout_is_rejected():
    assert _rejected_per_form("stride", [c for c in ALL_CASES if c.entry == "sums"]) == _every_form(("sums",))


def test_last_tile_summed_over_128_rows_is_rejected():
    assert _rejected_per_form("tail", ALL_CASES) == _every_form(("sums", "moments"))


def test_partial_stored_one_tile_late_is_rejected():
    assert _rejected_per_form("shift", ALL_CASES) == _every_form(("sums", "moments"))


def test_an_unwritten_column_group_is_rejected():
    assert _rejected_per_form("colgroup", ALL_CASES) == _every_form(("sums", "moments"))


def test_sum_r_of_the_neighbouring_row_is_rejected():
    assert _rejected_per_form("neighbour", [c for c in ALL_CASES if c.entry == "sums"]) == _every_form(("sums",))


def test_fp32_accumulation_in_moments_is_rejected_on_the_large_mean_channel():
    cases = [c for c in gd.BOUND_CASES if c.entry == "moments"]
    assert _rejected_per_form("fp32", cases) == _every_form(("moments",))
    for case in cases:
        d, rows, _ = _built(case)
        ref, mag = gd.parts_ref("moments", rows["y"])
        err = np.abs(_replay(case, "fp32") - ref)[:, 1, gd.LARGE_MEAN_CHANNEL]
        assert (err > gd.parts_bound("moments", mag)[:, 1, gd.LARGE_MEAN_CHANNEL]).any(), case.name


def test_another_row_order_has_the_same_exact_answer_and_stays_inside_the_bound():
    """Rows 8 g + j instead of g + 16 j: a wrong lane map of the ROWS A THREAD SUMS, not of the rows of the tile -- every row is still
    summed once, so in exact arithmetic the answer is the same: the exact cases must still pass, and the bound, which counts
    roundings and not their order, holds for it too.  (What tells the two orders apart is only the last bits of the fp32 sums.)"""
    differs = 0
    for case in ALL_CASES:
        d, rows, good = _built(case)
        parts = _replay(case, "rows8g")
        gpu.check_parts(case, d, rows["y"], parts)
        if case.exact:
            assert _same_bits(parts + 0.0, good + 0.0), case.name
        else:
            differs += not _same_bits(parts, good)
    assert differs > 0


def test_the_checker_takes_every_slot_of_every_case():
    """One slot moved by one unit of the data (exact cases: 1/8) or by twice its bound, or left as NaN, fails the check: the first
    and the last slot and one in between, in every case; so does a gap row of y that is not zero."""
    rng = np.random.default_rng(3)
    for case in ALL_CASES:
        d, rows, good = _built(case)
        ref, mag = gd.parts_ref(case.entry, rows["y"], d["sum_r"])
        bound = gd.parts_bound(case.entry, mag)
        n = good.size
        for at in (0, n - 1, int(rng.integers(n))):
            idx = np.unravel_index(at, good.shape)
            for value in (good[idx] + (0.125 if case.exact else 2 * bound[idx] + 1e-300), np.nan):
                bad = good.copy()
                bad[idx] = value
                assert _fails(gpu.check_parts, case, d, rows["y"], bad), (case.name, idx)
        if not d["valid"].all():
            y = rows["y"].copy()
            y[np.flatnonzero(~d["valid"])[-1], -1] = 1.0
            assert _fails(gpu.check_parts, case, d, y, good), case.name
