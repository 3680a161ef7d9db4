"""CPU companion of tests/test_gpu_bnback_elementwise.py: what that module relies on is settled here, without a GPU.

* the float32 replay of each kernel's operation order (tests/bnback_data.py, every operation rounded, nothing fused) passes the GPU
  module's own check_* functions on the exact cases -- so every intermediate of those cases is exact and FMA contraction cannot
  matter -- and fails them at a neighbouring non-dyadic case, so the exact cases are sharp;
* every derived bound holds for that replay on every bound case of the GPU module (the kernel, with contraction, rounds fewer);
* seven broken variants of the replay each fail the checkers: the power of the GPU module, measured before it sees a device."""
import os
import re

import numpy as np

import bnback_data as bd
import test_gpu_bnback_elementwise as gpu

F = np.float32


def _fails(fn, *args, **kw):
    try:
        fn(*args, **kw)
    except AssertionError:
        return True
    return False


def _bn_bound_cases():
    for layout in sorted(bd.LAYOUTS):
        for C in bd.BOUND_C:
            for act in ("relu", "lrelu"):
                yield bd.bn_bound_case(layout, C, act, seed=C + len(layout))


def _pool_cases(exact):
    if exact:                                               # the device module's list (65536 chunks are refused: nothing to replay)
        for nchunks, C in bd.POOL_EXACT:
            for case in bd.pool_exact_cases(nchunks, C):
                yield case
        yield bd.pool_grid_limit_case()
    else:
        for layout in sorted(bd.LAYOUTS):
            for C in (24, 260):
                for act in ("relu", "lrelu"):
                    yield bd.pool_bound_case(layout, C, act, seed=C + len(layout))


def _col_cases(exact):
    if exact:
        for R in bd.CS_ROWS_LIST:
            for C in bd.CS_CHANNELS:
                yield bd.col_case(R, C, seed=1000 * R + C, exact=True)
    else:
        for layout in sorted(bd.LAYOUTS):
            R = bd.layout(bd.LAYOUTS[layout])[1]
            for C in (24, 21, 260):
                yield bd.col_case(R, C, seed=R + C, exact=False)


# ---------------------------------------------------------------------------------------------------------------------------
# the replay on the exact cases
# ---------------------------------------------------------------------------------------------------------------------------
def test_replay_reproduces_the_exact_bn_backward_cases():
    for case in bd.bn_exact_cases():
        for entry in ("sums", "parts"):
            gpu.check_bn_backward(case, entry, *bd.replay_bn_backward(case, entry))
        ref = bd.bn_backward_ref(case, "sums")
        assert bd.representable(ref["dg"]) and bd.representable(ref["dz"])
        assert (ref["dz"][case["r"] == 0] == 0).all() if case["act"] == "relu" else True
    for act in bd.ACTS:
        for case in bd.bn_small_exact_cases(act):
            gpu.check_bn_backward(case, "small", *bd.replay_bn_backward(case, "small"))


def test_the_exact_bn_cases_cover_zero_activations_and_a_dead_channel():
    case = bd.bn_exact_case(129, 64, "lrelu", seed=1)
    ref = bd.bn_backward_ref(case, "sums")
    zero = (case["r"] == 0) & case["valid"][:, None]
    assert zero.sum() > 1000 and (case["gamma"] == 0).any()
    assert (ref["dz"][zero] != 0).any()                              # leaky ReLU at r == 0: alpha dr, not 0
    assert bd.BN_EXACT_SCALAR_WRAP[0] * bd.BN_EXACT_SCALAR_WRAP[1] > bd.SCALAR_GRID and bd.BN_EXACT_SCALAR_WRAP[1] % 4


def test_replay_reproduces_the_exact_pooling_cases():
    for case in _pool_cases(exact=True):
        gpu.check_pool_bn(case, *bd.replay_pool_bn(case))
        gpu.check_pool_backward(case, bd.replay_pool_backward(case))
        ref = bd.pool_bn_ref(case)
        assert bd.representable(ref["dg"]) and bd.representable(ref["db"]) and bd.representable(ref["dz"])
        own = bd.owner_of(case["rs"], case["rl"], case["R"])
        assert (own[:3] < 0).all() and (own[-5:] < 0).all() and own[3] == 0
        C = case["h"].shape[1]
        if C > 4 and case["act"] == "lrelu":                       # the odd-width pool_backward runs of the device module
            odd = bd.odd_width(case, C - 3)
            gpu.check_pool_backward(odd, bd.replay_pool_backward(odd))
    case = bd.pool_sliced_case()
    gpu.check_pool_backward(case, bd.replay_pool_backward(case))


def test_replay_reproduces_the_exact_column_sums():
    for case in _col_cases(exact=True):
        gpu.check_col_sums(case, *bd.replay_col_sums(case["a"], case["b"]))
    for nsplit in bd.MERGE_SPLITS:
        part = bd.merge_case(nsplit, 68, seed=nsplit)
        assert bd.same(bd.replay_merge(part).astype(F), part.sum(0).astype(F))
        if nsplit > 1:                                               # an fp32 accumulator loses the small integers next to 2^40
            assert not bd.same(part.astype(F).sum(0, dtype=F), part.sum(0).astype(F))


def test_replay_reproduces_the_exact_small_forward_cases():
    for R in bd.SMALL_FWD_R:
        for C in bd.SMALL_FWD_C:
            case = bd.small_fwd_case(R, C, seed=R + C, exact=True)
            gpu.check_small_forward(case, *bd.replay_small_forward(case))


def test_exact_moment_cases_have_an_exact_answer():
    for n in (1, 17, 40):
        case = bd.merge_moments_case(n, 8, seed=n)
        assert case["rl"].sum() == 1024 and (case["rl"] == 0).sum() == 1 and np.isnan(case["cm"][n // 2]).all()
        keep = case["rl"] > 0
        cm, w = case["cm"][keep].astype(np.longdouble), case["rl"][keep].astype(np.longdouble)[:, None]
        mu = (w * cm[:, :8])[::-1].sum(0) / 1024                    # another order, another precision: exact sums agree
        var = (w * (cm[:, 8:] + (cm[:, :8] - mu) ** 2))[::-1].sum(0) / 1024
        assert np.array_equal(mu.astype(np.float64), case["mean"]) and np.array_equal(var.astype(np.float64), case["var"])
        assert bd.representable(case["mean"])
    for nsplit in bd.MERGE_SPLITS:
        case = bd.moments_fold_case(nsplit, 8, seed=nsplit)
        tot = case["part"].sum(0)
        n = case["N"]
        assert n == 2 ** round(np.log2(n)) and np.array_equal(tot[0] / n, case["mean"]) and np.array_equal(tot[1] / n - case["mean"] ** 2, case["var"])
        assert bd.representable(case["scale"]) and bd.representable(case["shift"])


def test_build_recipe_leaves_fp32_division_and_sqrt_correctly_rounded():
    """The 6 U of the pooling gradient and the float32 fold of bn_small_forward count one rounding per division and square root:
    the compile flags of the HIP sources must not relax them."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "x-vector-kaldi-tf_amd", "csrc", "Makefile")).read()
    flags = re.findall(r"^FLAGS\s*:?=\s*(.*)$", text, re.M)
    assert len(flags) == 1 and "-O3" in flags[0] and "$(HIPCC) $(FLAGS) -c" in text
    for bad in ("fast-math", "fno-hip-fp32-correctly-rounded-divide-sqrt", "unsafe-math", "approx-func", "reciprocal-math", "-Ofast",
                "ffp-model", "fgpu-approx", "munsafe-fp-atomics", "fdenormal-fp-math", "fgpu-flush-denormals"):
        assert bad not in text, bad


def test_replay_is_not_exact_at_a_neighbour():
    """var = 0.3 instead of 1/4, a chunk of 3 rows instead of 4: the same replay no longer meets the exact check."""
    case = bd.bn_exact_case(129, 64, "none", seed=2, var=0.3)
    assert _fails(gpu.check_bn_backward, case, "sums", *bd.replay_bn_backward(case, "sums"))
    case = bd.pool_exact_case(17, 64, "none", seed=2, var=0.3)
    assert _fails(gpu.check_pool_bn, case, *bd.replay_pool_bn(case))
    case = bd.pool_exact_case(17, 64, "none", seed=2)
    case["rl"][case["rl"] == 4] = 3
    assert (case["rl"] == 3).any() and _fails(gpu.check_pool_backward, case, bd.replay_pool_backward(case))
    case = bd.small_fwd_case(16, 64, seed=2, exact=True)
    case["x"] = (case["x"] * F(1.1)).astype(F)
    assert _fails(gpu.check_small_forward, case, *bd.replay_small_forward(case))


# ---------------------------------------------------------------------------------------------------------------------------
# the bounds on the replay
# ---------------------------------------------------------------------------------------------------------------------------
def test_bounds_hold_for_the_replay_bn_backward():
    kinds = set()
    for case in _bn_bound_cases():
        for entry in ("sums", "parts"):
            gpu.check_bn_backward(case, entry, *bd.replay_bn_backward(case, entry))
        kinds |= {bd.kind_of(c) for c in range(case["r"].shape[1])}
        assert len(case["parts"]) >= (17 if len(case["rl"]) == 17 else 13)
    assert kinds == set(bd.KINDS)
    for act in ("relu", "lrelu"):
        for rows, C in ((700, 21), (64, 24)):
            case = bd.bn_bound_case("ragged", C, act, seed=rows, rows=rows)
            gpu.check_bn_backward(case, "small", *bd.replay_bn_backward(case, "small"))


def test_bounds_hold_for_the_replay_pooling():
    for case in _pool_cases(exact=False):
        gpu.check_pool_bn(case, *bd.replay_pool_bn(case))
        gpu.check_pool_backward(case, bd.replay_pool_backward(case))


def test_bounds_hold_for_the_replay_column_sums_and_small_forward():
    for case in _col_cases(exact=False):
        gpu.check_col_sums(case, *bd.replay_col_sums(case["a"], case["b"]))
    for R, C in ((64, 24), (700, 21), (1024, 65)):
        case = bd.small_fwd_case(R, C, seed=R * C, exact=False)
        gpu.check_small_forward(case, *bd.replay_small_forward(case))


def test_the_mean_200_channel_is_where_the_old_bar_would_fail():
    """The loss of the A dh + B r + K form on the mean-200 channel against the exact gradient, on the replay: well above the 2e-6
    relative-L2 bar of the autograd test (which leaves that channel out), inside the derived bound."""
    notes = {}
    case = bd.bn_bound_case("uniform", 24, "relu", seed=24 + 7)
    gpu.check_bn_backward(case, "sums", *bd.replay_bn_backward(case, "sums"), note=lambda k, v: notes.__setitem__(k, max(notes.get(k, 0), v)))
    print(notes)
    assert notes["sums dz / bound"] <= 1
    assert 2e-6 < notes["mean-200 channel: dz column rel-L2 vs exact gradient"] < 1e-2


# ---------------------------------------------------------------------------------------------------------------------------
# power: seven broken variants of the replay against the GPU module's checkers
# ---------------------------------------------------------------------------------------------------------------------------
def _power_cases():
    bn = [bd.bn_exact_case(129, C, act, seed=C) for C in (64, 65) for act in bd.ACTS] + list(_bn_bound_cases())
    pool = [bd.pool_exact_case(n, 64, act, seed=n) for n in (17, 200) for act in bd.ACTS] + list(_pool_cases(exact=False))
    col = [bd.col_case(R, C, seed=R + C, exact=True) for R in (129, 2049) for C in (255, 256, 257)] + list(_col_cases(exact=False))
    return bn, pool, col


def _count(variant, bn, pool, col):
    """(cases the variant applies to, cases on which at least one checker assertion fails)."""
    res = []
    if variant in ("k_mean", "mask", "ge", "gaps"):
        res += [_fails(gpu.check_bn_backward, c, "sums", *bd.replay_bn_backward(c, "sums", variant)) for c in bn]
        res += [_fails(gpu.check_pool_bn, c, *bd.replay_pool_bn(c, variant)) for c in pool]
    if variant in ("mask", "gaps", "invT"):
        res += [_fails(gpu.check_pool_backward, c, bd.replay_pool_backward(c, variant)) for c in pool]
    if variant == "invT":
        res += [_fails(gpu.check_pool_bn, c, *bd.replay_pool_bn(c, variant)) for c in pool]
    if variant == "skip16":
        res += [_fails(gpu.check_col_sums, c, *bd.replay_col_sums(c["a"], c["b"], skip16=True)) for c in col if len(c["a"]) > 16 * bd.CS_ROWS]
        res += [_fails(gpu.check_bn_backward, c, "parts", *bd.replay_bn_backward(c, "parts", variant)) for c in bn if len(c["parts"]) > 16]
    if variant == "tail":
        res += [_fails(gpu.check_col_sums, c, *bd.replay_col_sums(c["a"], c["b"], drop_tail=True)) for c in col if c["a"].shape[1] % 4]
    return len(res), sum(res)


VARIANTS = (("k_mean", "K without its mean term"), ("mask", "the valid mask one row late"), ("ge", "r >= 0 in place of r > 0"),
            ("skip16", "merge groups that skip split 16"), ("invT", "1 / T of the neighbouring chunk"), ("gaps", "gap rows left unwritten"),
            ("tail", "the c + 4 > C tail dropped"))


def test_every_broken_variant_fails_the_checkers():
    bn, pool, col = _power_cases()
    table = []
    for variant, what in VARIANTS:
        n, failed = _count(variant, bn, pool, col)
        table.append((what, failed, n))
    print("\nbroken variant: cases failed / cases it applies to")
    for what, failed, n in table:
        print("  %-36s %3d / %3d" % (what, failed, n))
    for what, failed, n in table:
        assert n > 0 and failed >= 1, (what, failed, n)
    # the variants that corrupt every case they apply to are caught on every one
    for what, failed, n in table:
        if what in ("the valid mask one row late", "gap rows left unwritten", "merge groups that skip split 16", "the c + 4 > C tail dropped"):
            assert failed == n, (what, failed, n)
