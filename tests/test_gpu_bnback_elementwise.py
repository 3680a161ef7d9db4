"""Element-wise checks of the batch-norm / pooling BACKWARD family of csrc/xv_train.hip and of the column sums that feed it:
xv_col_sums_f32 / xv_col_sums_merge_f32, xv_bn_act_backward_f32 / _split / _parts, xv_bn_small_forward_f32 / _backward,
xv_rows_affine_f32 / _split, xv_pool_backward_f32, xv_pool_bn_act_backward_f32, xv_merge_moments_f32, xv_bn_moments_fold_f32.
One relative-L2 number per column or chunk hides one wrong element, a mask off by one row, a wrong branch at r == 0 or a term that
is small on Gaussian data:

* exact known answers: inputs for which every intermediate is a short dyadic number (tests/bnback_data.py, "Exact cases"), at the
  channel counts of the vector and the scalar kernels, row counts around the 4096-row stride loop, split counts around the 16 merge
  groups, chunk counts in every row-group regime and at the grid limit -- every output bit;
* element-wise bounds counted from the roundings of the source (tests/bnback_data.py) on realistic data with the hostile channels
  kept in: mean 200 / std 0.1, a constant channel, gamma = 0, a 1e4 outlier, an all-negative pre-activation; the worst ratio per
  quantity and the loss of the mean-200 channel against the exact gradient are printed at the end;
* the contracts: ld < c and R <= 0 are refused, base pointers one and three floats past a 16-byte boundary give the right sums
  (the values only: a test cannot see which loads ran), an empty chunk adds nothing to the sums.

The check_* functions are plain NumPy: tests/test_bnback_bounds_cpu.py feeds them the float32 replay (they must pass) and seven
broken variants of it (they must fail).  Outputs are NaN-poisoned before every call, gap rows of dh hold NaN, and a sentinel row
behind every output must come back untouched."""
import ctypes

import numpy as np
import pytest

import arith_emul as ae
import bnback_data as bd

pytestmark = pytest.mark.gpu

WORST = {}
BAD_ARG = -1
SENTINEL = -12345.0
ACT_CODE = {"none": 0, "relu": 1, "lrelu": 2}
F = np.float32


def _note(key, value):
    WORST[key] = max(WORST.get(key, 0.0), float(value))


# ---------------------------------------------------------------------------------------------------------------------------
# checkers (NumPy only; shared with the CPU companion)
# ---------------------------------------------------------------------------------------------------------------------------
def _bits(name, got, ref64):
    got, ref = np.asarray(got, F), np.asarray(ref64).astype(F)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    bad = np.argwhere(bd.canon(got) != bd.canon(ref))
    assert bad.size == 0, (name, len(bad), [(tuple(int(i) for i in b), float(got[tuple(b)]), float(ref[tuple(b)])) for b in bad[:5]])


def _within(name, got, ref64, bound, note, key):
    got = np.asarray(got, np.float64)
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    r = bd.ratio(np.abs(got - ref64), bound)
    if note:
        note(key, r)
    if r > 1:
        err = np.where(np.isfinite(got), np.abs(got - ref64) - bound, np.inf)
        at = np.unravel_index(int(np.argmax(err)), err.shape)
        raise AssertionError((name, key, r, tuple(int(i) for i in at), float(got[at]), float(ref64[at]), float(bound[at])))


def check_col_sums(case, sum_a, sum_ab, note=None, name="col_sums"):
    """exact: the integer sums in every bit.  Otherwise |sum - ref| <= ulp32(ref) / 2 + 2^-50 sum |terms| per column."""
    ra, rb, ba, bb = bd.col_sums_ref(case["a"], case["b"])
    if case["exact"]:
        _bits(name + " sum_a", sum_a, ra)
        if rb is not None:
            _bits(name + " sum_ab", sum_ab, rb)
        return
    _within(name, sum_a, ra, ba, note, "col_sums sum_a / bound")
    if rb is not None:
        _within(name, sum_ab, rb, bb, note, "col_sums sum_ab / bound")


def check_bn_backward(case, entry, dgamma, dbeta, dz, note=None, name="bn_act_backward"):
    """entry: "sums" (xv_bn_act_backward_f32), "parts" (xv_bn_act_backward_parts_f32), "small" (xv_bn_small_backward_f32).
    dbeta is the fp32 sum handed in, bit for bit; dgamma within 1 ulp + the fp64 dust of S2 - mean S1; every dz element within
    C_DZ U (|A dh| + |B r| + |K|); exactly 0 on gap rows and, with ReLU, wherever r <= 0.  exact cases: every bit of all three."""
    ref = bd.bn_backward_ref(case, entry)
    name = "%s[%s]" % (name, entry)
    _bits(name + " dbeta", dbeta, ref["db"])
    dz = np.asarray(dz, F)
    if case["valid"] is not None:
        gaps = dz[~case["valid"]]
        assert (gaps == 0).all(), (name, "gap rows", int((gaps != 0).sum()) + int(np.isnan(gaps).sum()))
    if case["exact"]:
        _bits(name + " dgamma", dgamma, ref["dg"])
        _bits(name + " dz", dz, ref["dz"])
        return
    _within(name, dgamma, ref["dg"], ref["dg_bound"], note, "%s dgamma / bound" % entry)
    _within(name, dz, ref["dz"], ref["dz_bound"], note, "%s dz / bound" % entry)
    if note:
        true_dz, true_dg, g_scale = bd.bn_backward_true(case)
        v = case["valid"] if case["valid"] is not None else np.ones(len(dz), bool)
        for c in range(dz.shape[1]):
            if bd.kind_of(c) == "mean200":
                t = true_dz[v, c]
                note("mean-200 channel: dz column rel-L2 vs exact gradient", np.sqrt(((dz[v, c] - t) ** 2).sum() / (t ** 2).sum()))
                note("mean-200 channel: max |dz - exact| / max |dz|", np.abs(dz[v, c] - t).max() / np.abs(t).max())
                note("mean-200 channel: |dgamma - exact| / |summands|", abs(float(dgamma[c]) - true_dg[c]) / g_scale[c])


def check_pool_backward(case, dh, note=None, name="pool_backward"):
    """Every element within U (3 |dmu / T| + 6 |dsig (h - mu) / (T sig)|); rows outside the chunks exactly 0; exact cases: every bit."""
    ref, bound, own = bd.pool_dh_ref(case)
    dh = np.asarray(dh, F)
    out = dh[own < 0]
    assert (out == 0).all(), (name, "rows outside the chunks", int((out != 0).sum()) + int(np.isnan(out).sum()))
    if case["exact"]:
        _bits(name, dh, ref)
    else:
        _within(name, dh, ref, bound, note, "pool_backward dh / bound")


def check_pool_bn(case, dgamma, dbeta, dz, note=None, name="pool_bn_act_backward"):
    """dbeta and dgamma: one rounding of the fp64 chunk sums (+ their dust); dz within |A| E_dh + C_DZ U (|A dh| + |B r| + |K|); the
    rows in front of chunk 0, between chunks and behind the last chunk exactly 0; exact cases: every bit."""
    ref = bd.pool_bn_ref(case)
    own = bd.owner_of(case["rs"], case["rl"], case["R"])
    dz = np.asarray(dz, F)
    out = dz[own < 0]
    assert (out == 0).all(), (name, "rows outside the chunks", int((out != 0).sum()) + int(np.isnan(out).sum()))
    if case["exact"]:
        _bits(name + " dbeta", dbeta, ref["db"])
        _bits(name + " dgamma", dgamma, ref["dg"])
        _bits(name + " dz", dz, ref["dz"])
        return
    _within(name, dbeta, ref["db"], ref["db_bound"], note, "pool_bn_act_backward dbeta / bound")
    _within(name, dgamma, ref["dg"], ref["dg_bound"], note, "pool_bn_act_backward dgamma / bound")
    _within(name, dz, ref["dz"], ref["dz_bound"], note, "pool_bn_act_backward dz / bound")


def check_small_forward(case, mean, var, y, note=None, name="bn_small_forward"):
    """mean and var: the fp64 two-pass answer rounded once; y = fma(x, scale, shift) with the float32 fold of the kernel's own mean
    and var: half an ulp.  exact cases with an even row count: every bit of mean, var and y; a constant column has var == 0."""
    m, v, bm, bv = bd.small_forward_ref(case)
    mean, var, y = np.asarray(mean, F), np.asarray(var, F), np.asarray(y, F)
    R = len(case["x"])
    if case["exact"]:
        _bits(name + " mean", mean, m)
        _bits(name + " var", var, v)
    else:
        _within(name, mean, m, bm, note, "bn_small_forward mean / bound")
        _within(name, var, v, bv, note, "bn_small_forward var / bound")
    with np.errstate(all="ignore"):
        sc, sf = bd.fold32(mean, var, case["gamma"], case["beta"], case["eps"])
        ref = case["x"].astype(np.float64) * sc.astype(np.float64) + sf.astype(np.float64)
    if case["exact"] and R % 2 == 0:
        assert bd.representable(ref)
        _bits(name + " y", y, ref)
    else:
        _within(name, y, ref, bd.ulp32(ref) / 2 + 2.0 ** -52 * np.abs(ref), note, "bn_small_forward y / (ulp / 2)")


# ---------------------------------------------------------------------------------------------------------------------------
# device plumbing
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def env():
    import torch
    from xvector_amd import hiplib
    hiplib.require_gpu()
    yield dict(torch=torch, hiplib=hiplib, lib=hiplib.load(), dev=torch.device("cuda:0"))
    if WORST:
        print("\nworst error / bound per quantity (BN / pooling backward element-wise):")
        for k in sorted(WORST):
            print("  %-62s %.3e" % (k, WORST[k]))


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _dev(env, a):
    return env["torch"].from_numpy(np.ascontiguousarray(a)).to(env["dev"])


def _out(env, rows, width):
    """NaN-poisoned [rows + 1, width]: the last row is a sentinel."""
    t = env["torch"].full((rows + 1, width), float("nan"), dtype=env["torch"].float32, device=env["dev"])
    t[rows] = SENTINEL
    return t


def _host(env, t, rows=None):
    env["torch"].cuda.synchronize()
    h = t.cpu().numpy()
    rows = len(h) - 1 if rows is None else rows
    assert (h[rows] == SENTINEL).all(), "wrote behind the last row"
    return h[:rows]


def _vec(env, n):
    return _out(env, 1, n)


def _hvec(env, t):
    return _host(env, t)[0]


def _wide(env, a, ld, col0, fill=np.nan):
    """Device view of a [R, C] as columns [col0, col0 + C) of a `fill`-filled [R, ld] buffer."""
    host = np.full((a.shape[0], ld), fill, F)
    host[:, col0:col0 + a.shape[1]] = a
    return _dev(env, host)[:, col0:col0 + a.shape[1]]


def _offset(env, a, ld, floats=1):
    """Device view of a [R, C] with row stride ld whose base pointer is `floats` floats past a 16-byte boundary."""
    R, C = a.shape
    host = np.full(R * ld + floats, np.nan, F)
    host[floats:].reshape(R, ld)[:, :C] = a
    flat = _dev(env, host)
    assert flat.data_ptr() % 16 == 0
    return flat[floats:].view(R, ld)[:, :C]


def run_col_sums(env, case, a=None, b=None, runs=1):
    """xv_col_sums_f32 through the raw binding on device views a, b (default: contiguous copies); runs = 2: same bits twice."""
    torch, lib, dev = env["torch"], env["lib"], env["dev"]
    a = _dev(env, case["a"]) if a is None else a
    b = (_dev(env, case["b"]) if case["b"] is not None else None) if b is None else b
    R, C = case["a"].shape
    res = []
    for _ in range(runs):
        ws = torch.full((int(lib.xv_col_sums_workspace_bytes(R, C)) // 8 + 1,), float("nan"), dtype=torch.float64, device=dev)
        sa, sab = _vec(env, C), _vec(env, C)
        rc = lib.xv_col_sums_f32(_p(a), a.stride(0), _p(b), b.stride(0) if b is not None else 0, R, C, _p(sa), _p(sab) if b is not None else None,
                                 _p(ws), None)
        assert rc == 0, rc
        res.append((_hvec(env, sa), _hvec(env, sab) if b is not None else None))
        if b is None:
            assert np.isnan(_hvec(env, sab)).all()
    assert bd.bits_equal(res[0][0], res[-1][0]) and (b is None or bd.bits_equal(res[0][1], res[-1][1])), "a second run gives other bits"
    return res[0]


def run_bn_backward(env, case, entry, split=False, ld=None):
    """-> (dgamma, dbeta, dz[, decoded split copy]) of one entry point on the case; dh holds NaN in its gap rows.  ld: dh, r and dz
    are column slices of [R, ld] buffers (raw binding: the wrappers take contiguous tensors)."""
    torch, hiplib, lib = env["torch"], env["hiplib"], env["lib"]
    R, C = case["r"].shape
    code, alpha = ACT_CODE[case["act"]], float(case["alpha"])
    dg, db = _vec(env, C), _vec(env, C)
    mean, var, gamma = _dev(env, case["mean"]), _dev(env, case["var"]), _dev(env, case["gamma"])
    vt = _dev(env, case["valid"].astype(np.uint8)) if case["valid"] is not None else None
    buf = hiplib.SplitBuf(R, C, env["dev"]) if split else None
    if ld is not None:
        dh, r = _wide(env, case["dh_in"], ld, 4), _wide(env, case["r"], ld, 4)
        parent = _out(env, R, ld)
        dz = parent[:, 4:4 + C]
        coef = torch.full((3 * C,), float("nan"), dtype=torch.float32, device=env["dev"])
        s1, s2 = _dev(env, case["s1"]), _dev(env, case["s2"])
        rc = lib.xv_bn_act_backward_f32(_p(dh), _p(r), ld, R, C, _p(s1), _p(s2), _p(mean), _p(var),
                                        _p(gamma), float(case["eps"]), float(case["N"]), code, alpha, _p(vt), _p(dg), _p(db), _p(coef),
                                        _p(dz), None)
        assert rc == 0, rc
        ph = _host(env, parent, R)
        assert np.isnan(ph[:, :4]).all() and np.isnan(ph[:, 4 + C:]).all(), "wrote outside the column slice"
        return _hvec(env, dg), _hvec(env, db), ph[:, 4:4 + C]
    dh, r, dz = _dev(env, case["dh_in"]), _dev(env, case["r"]), _out(env, R, C)
    if entry == "sums":
        hiplib.bn_act_backward(dh, r, _dev(env, case["s1"]), _dev(env, case["s2"]), mean, var, gamma, case["eps"], case["N"], code, alpha, vt,
                               dg, db, dz[:R], dz_split=buf)
    elif entry == "parts":
        hiplib.bn_act_backward_parts(dh, r, _dev(env, case["parts"]), mean, var, gamma, case["eps"], case["N"], code, alpha, vt, dg, db,
                                     dz[:R], dz_split=buf)
    else:
        hiplib.bn_small_backward(dh, r, mean, var, gamma, case["eps"], code, alpha, dg, db, dz[:R])
    out = (_hvec(env, dg), _hvec(env, db), _host(env, dz, R))
    return out + (hiplib.split_decode(buf, R).cpu().numpy(),) if split else out


def _check_split(dz, dec):
    """The bf16 hi + lo copy decodes to the fp32 rows within 2^-17 relative."""
    assert (np.abs(dec.astype(np.float64) - dz) <= ae.ENC_SPLIT * np.abs(dz)).all()


def run_pool_bn(env, case, split=False, expect=0):
    torch, hiplib, lib = env["torch"], env["hiplib"], env["lib"]
    R, C = case["R"], case["h"].shape[1]
    dg, db, dz = _vec(env, C), _vec(env, C), _out(env, R, C)
    buf = hiplib.SplitBuf(R, C, env["dev"]) if split else None
    args = (_dev(env, case["h"]), _dev(env, case["r"]), _dev(env, case["rs"]), _dev(env, case["rl"]), len(case["rl"]), _dev(env, case["pooled"]),
            _dev(env, case["dpooled"]), _dev(env, case["cm"]), _dev(env, case["mean"]), _dev(env, case["var"]), _dev(env, case["gamma"]),
            case["eps"], case["N"], ACT_CODE[case["act"]], float(case["alpha"]), dg, db, dz[:R])
    if expect:
        with pytest.raises(hiplib.XvectorHipError):
            hiplib.pool_bn_act_backward(*args)
        assert np.isnan(_host(env, dz, R)).all() and np.isnan(_hvec(env, dg)).all()          # nothing was launched
        return None
    hiplib.pool_bn_act_backward(*args, dz_split=buf)
    out = (_hvec(env, dg), _hvec(env, db), _host(env, dz, R))
    return out + (hiplib.split_decode(buf, R).cpu().numpy(),) if split else out


def run_pool_backward(env, case, ld=None):
    hiplib, lib = env["hiplib"], env["lib"]
    R, C = case["R"], case["h"].shape[1]
    rs, rl, p, dp = _dev(env, case["rs"]), _dev(env, case["rl"]), _dev(env, case["pooled"]), _dev(env, case["dpooled"])
    if ld is None:
        dh = _out(env, R, C)
        hiplib.pool_backward(_dev(env, case["h"]), rs, rl, len(case["rl"]), p, dp, dh[:R])
        return _host(env, dh, R)
    parent = _out(env, R, ld)
    h = _wide(env, case["h"], ld, 0)
    rc = lib.xv_pool_backward_f32(_p(h), ld, C, _p(rs), _p(rl), len(case["rl"]), R, _p(p), _p(dp), _p(parent), None)
    assert rc == 0, rc
    ph = _host(env, parent, R)
    assert (ph[:, C:] == 0).all()                             # all R * ldh floats are written: the columns behind c are zeroed
    return ph[:, :C]


# ---------------------------------------------------------------------------------------------------------------------------
# 1. column sums
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", bd.CS_CHANNELS)
def test_col_sums_exact_on_integers(env, C):
    """Integers in [-8, 8]: every partial and total is an integer below 2^24, the answer is exact in every bit.  Rows 1 ... 2049 (17
    splits: one more than the merge groups); with and without b; a and b as column slices with lda, ldb > C; the base pointers one
    and three floats past a 16-byte boundary with lda % 4 == 0 (the host then picks the scalar loads; the test sees the sums only)."""
    for R in bd.CS_ROWS_LIST:
        case = bd.col_case(R, C, seed=1000 * R + C, exact=True)
        check_col_sums(case, *run_col_sums(env, case, runs=2))
        check_col_sums(dict(case, b=None), *run_col_sums(env, dict(case, b=None)))
        ld = C + 7 - (C + 7) % 4 + 4
        check_col_sums(case, *run_col_sums(env, case, _wide(env, case["a"], ld, 4), _wide(env, case["b"], ld + 4, 0)), name="slices")
        check_col_sums(case, *run_col_sums(env, case, _wide(env, case["a"], C + 3, 2), _wide(env, case["b"], C + 1, 1)), name="odd ld")
        check_col_sums(case, *run_col_sums(env, case, _offset(env, case["a"], ld), _offset(env, case["b"], ld, 3)), name="offset base")


@pytest.mark.parametrize("nsplit", bd.MERGE_SPLITS)
def test_col_sums_merge_on_hand_made_partials(env, nsplit):
    """xv_col_sums_merge_f32 alone: partials near 2^40 whose totals are small integers; 1, 15, 16, 17 and 33 splits."""
    C = 68
    part = bd.merge_case(nsplit, C, seed=nsplit)
    ref = part.sum(0)
    assert bd.representable(ref) and np.abs(ref).max() < 2 ** 24
    sa, sab = _vec(env, C), _vec(env, C)
    env["hiplib"].col_sums_merge(_dev(env, part), nsplit * bd.CS_ROWS - 5, C, sa, sab)
    assert bd.same(_hvec(env, sa), ref[0].astype(F)) and bd.same(_hvec(env, sab), ref[1].astype(F))
    assert bd.same(bd.replay_merge(part).astype(F), ref.astype(F))
    sa, sab = _vec(env, C), _vec(env, C)
    env["hiplib"].col_sums_merge(_dev(env, part), nsplit * bd.CS_ROWS, C, sa)                    # sum_ab = NULL
    assert bd.same(_hvec(env, sa), ref[0].astype(F)) and np.isnan(_hvec(env, sab)).all()


@pytest.mark.parametrize("C", (24, 21, 260))
@pytest.mark.parametrize("layout", sorted(bd.LAYOUTS))
def test_col_sums_elementwise_bound(env, layout, C):
    """Real data (Gaussian times ReLU-of-Gaussian, columns that cancel to about 0, a mean-200 column) over the rows of both layouts:
    one rounding of the fp64 sum, and the bits of the fp64 replay of the kernel's order of additions."""
    R = bd.layout(bd.LAYOUTS[layout])[1]
    case = bd.col_case(R, C, seed=R + C, exact=False)
    sa, sab = run_col_sums(env, case)
    check_col_sums(case, sa, sab, _note)
    ra, rab = bd.replay_col_sums(case["a"], case["b"])
    assert bd.bits_equal(sa, ra) and bd.bits_equal(sab, rab)
    cancel = np.abs(bd.col_sums_ref(case["a"], case["b"])[0][1::3])
    assert (cancel < 1e-3 * np.abs(case["a"]).sum(0)[1::3]).all()              # the cancelling columns do cancel


# ---------------------------------------------------------------------------------------------------------------------------
# 2. BN backward: exact answers
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", sorted({c for _, c, _ in bd.bn_exact_shapes()}))
def test_bn_act_backward_exact(env, C):
    """xv_bn_act_backward_f32 and xv_bn_act_backward_parts_f32 on the exact cases: dgamma, dbeta and every dz element equal the fp64
    answer; the gap row is exactly 0 although dh holds NaN there; r == 0 gives 0 with ReLU and alpha dr with leaky ReLU (alpha =
    1/4).  C % 4 == 0: the vector kernel; otherwise the scalar one (257 x 4097 elements: its stride loop wraps); 4097 rows: the
    4096-row loop of the vector kernel wraps.  C = 64 also with the bf16 split copy: dz has the same bits with and without it."""
    for case in bd.bn_exact_cases(C):
        R = len(case["r"])
        for entry in ("sums", "parts"):
            dg, db, dz = run_bn_backward(env, case, entry)
            check_bn_backward(case, entry, dg, db, dz)
            if C % 32 == 0:
                dg2, db2, dz2, dec = run_bn_backward(env, case, entry, split=True)
                assert bd.bits_equal(dz, dz2) and bd.bits_equal(dg, dg2) and bd.bits_equal(db, db2)
                _check_split(dz2, dec)
        if R <= 129:
            dg, db, dz = run_bn_backward(env, case, "sums", ld=C + 12 if C % 4 == 0 else C + 9)
            check_bn_backward(case, "sums", dg, db, dz, name="column slice")


@pytest.mark.parametrize("act", bd.ACTS)
def test_bn_small_backward_exact(env, act):
    for case in bd.bn_small_exact_cases(act):
        check_bn_backward(case, "small", *run_bn_backward(env, case, "small"), name="bn_small_backward")


# ---------------------------------------------------------------------------------------------------------------------------
# 3. BN backward: element-wise bounds, hostile channels kept
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ("relu", "lrelu"))
@pytest.mark.parametrize("C", bd.BOUND_C)
@pytest.mark.parametrize("layout", sorted(bd.LAYOUTS))
def test_bn_act_backward_elementwise_bound(env, layout, C, act):
    """Both entries on both layouts; the sums handed to xv_bn_act_backward_f32 come from xv_col_sums_f32 itself (checked on the
    way).  A gamma = 0 channel and, with ReLU, an all-negative one give dz == 0 in every row."""
    case = bd.bn_bound_case(layout, C, act, seed=C + len(layout))
    sums = dict(a=case["dh"], b=case["r"], exact=False)
    s1, s2 = run_col_sums(env, sums)
    check_col_sums(sums, s1, s2, _note)
    case = dict(case, s1=s1, s2=s2)
    for entry in ("sums", "parts"):
        dg, db, dz = run_bn_backward(env, case, entry)
        assert np.isfinite(dz).all()
        check_bn_backward(case, entry, dg, db, dz, _note)
        for c in range(C):
            if bd.kind_of(c) == "gamma0":
                assert (dz[:, c] == 0).all()
            if bd.kind_of(c) == "negative" and act == "relu":
                assert (dz[:, c] == 0).all()


@pytest.mark.parametrize("act", ("relu", "lrelu"))
def test_bn_small_backward_elementwise_bound(env, act):
    for rows, C in ((700, 21), (64, 24)):
        case = bd.bn_bound_case("ragged", C, act, seed=rows, rows=rows)
        dg, db, dz = run_bn_backward(env, case, "small")
        check_bn_backward(case, "small", dg, db, dz, _note, name="bn_small_backward")


# ---------------------------------------------------------------------------------------------------------------------------
# 4. rows_affine, bn_small_forward, merge_moments, bn_moments_fold
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", (4, 5, 63, 64, 65, 1028))
def test_rows_affine_exact(env, C):
    """Small integers times quarters plus eighths: x * scale + shift is exact fused or not.  x holds NaN in the rows that are not
    valid, y must be exactly 0 there; x and y as column slices (ldx, ldy > C; for C % 4 == 0 once aligned -- the vector kernel --
    and once not); C = 64 with the split copy."""
    hiplib, lib = env["hiplib"], env["lib"]
    for R in (1, 129, 4097):
        case = bd.affine_case(R, C, seed=R + C)
        vt, sc, sh = _dev(env, case["valid"].astype(np.uint8)), _dev(env, case["scale"]), _dev(env, case["shift"])
        y = _out(env, R, C)
        buf = hiplib.SplitBuf(R, C, env["dev"]) if C % 32 == 0 else None
        hiplib.rows_affine(_dev(env, case["x"]), sc, sh, vt, y[:R], y_split=buf)
        got = _host(env, y, R)
        assert bd.same(got, case["y"].astype(F)) and (got[~case["valid"]] == 0).all()
        if buf is not None:
            _check_split(got, hiplib.split_decode(buf, R).cpu().numpy())
        for ldx, ldy, col in ((C + 8, C + 12, 4), (C + 3, C + 1, 1)):
            parent = _out(env, R, ldy)
            x = _wide(env, case["x"], ldx, col)
            rc = lib.xv_rows_affine_f32(_p(x), ldx, R, C, _p(sc), _p(sh), _p(vt), _p(parent[:, col:]), ldy, None)
            assert rc == 0, rc
            ph = _host(env, parent, R)
            assert bd.same(ph[:, col:col + C], case["y"].astype(F)) and np.isnan(ph[:, :col]).all() and np.isnan(ph[:, col + C:]).all()


def _small_forward(env, case, ld=None):
    torch, hiplib = env["torch"], env["hiplib"]
    R, C = case["x"].shape
    mean, var = _vec(env, C), _vec(env, C)
    parent = _out(env, R, ld or C)
    x = _dev(env, case["x"]) if ld is None else _wide(env, case["x"], ld + 3, 2)
    hiplib.bn_small_forward(x, _dev(env, case["gamma"]), _dev(env, case["beta"]), case["eps"], mean[0], var[0], parent[:R, :C])
    ph = _host(env, parent, R)
    assert np.isnan(ph[:, C:]).all()
    return _hvec(env, mean), _hvec(env, var), ph[:, :C]


@pytest.mark.parametrize("C", bd.SMALL_FWD_C)
def test_bn_small_forward_exact(env, C):
    """Columns of m + 1/2 and m - 1/2 in equal numbers: mean = m, var = 1/4, scale = 2 gamma: mean, var and every y exact (R = 17: a
    lone m in front; mean exact, var = 4 / 17 rounded once, y to half an ulp; R = 1: var = 0, eps = 1/4).  Contiguous and as column
    slices with ldx, ldy > C.  1025 rows are refused."""
    for R in bd.SMALL_FWD_R:
        case = bd.small_fwd_case(R, C, seed=R + C, exact=True)
        check_small_forward(case, *_small_forward(env, case))
        check_small_forward(case, *_small_forward(env, case, ld=C + 5), name="column slice")
    lib = env["lib"]
    x, g = _dev(env, np.zeros((1025, C), F)), _dev(env, np.ones(C, F))
    mean, y = _vec(env, C), _out(env, 1025, C)
    assert lib.xv_bn_small_forward_f32(_p(x), C, 1025, C, _p(g), _p(g), 0.0, _p(mean), _p(mean), _p(y), C, None) == BAD_ARG
    assert lib.xv_bn_small_backward_f32(_p(x), _p(x), C, 1025, C, _p(g), _p(g), _p(g), 0.0, 0, 0.0, _p(mean), _p(mean), _p(y), None) == BAD_ARG
    assert np.isnan(_host(env, y, 1025)).all() and np.isnan(_hvec(env, mean)).all()


@pytest.mark.parametrize("R,C", ((64, 24), (700, 21), (1024, 65)))
def test_bn_small_forward_elementwise_bound(env, R, C):
    case = bd.small_fwd_case(R, C, seed=R * C, exact=False)
    mean, var, y = _small_forward(env, case)
    check_small_forward(case, mean, var, y, _note)
    for c in range(C):
        if bd.kind_of(c) == "const":
            assert var[c] == 0 and mean[c] == case["x"][0, c]
        if bd.kind_of(c) == "gamma0":
            assert (y[:, c] == case["beta"][c]).all()


@pytest.mark.parametrize("nchunks", (1, 17, 40))
def test_merge_moments_exact(env, nchunks):
    """Dyadic chunk moments, power-of-two lengths that sum to 1024: mean and var are the exact answer rounded once; the chunk of
    length 0 (NaN moments) is skipped."""
    C = 68
    case = bd.merge_moments_case(nchunks, C, seed=nchunks)
    mean, var = _vec(env, C), _vec(env, C)
    env["hiplib"].merge_moments(_dev(env, case["cm"]), _dev(env, case["rl"]), nchunks + 1, mean[0], var[0])
    assert bd.same(_hvec(env, mean), case["mean"].astype(F)) and bd.same(_hvec(env, var), case["var"].astype(F))


@pytest.mark.parametrize("nsplit", bd.MERGE_SPLITS)
def test_bn_moments_fold_exact(env, nsplit):
    C = 68
    case = bd.moments_fold_case(nsplit, C, seed=nsplit)
    mean, var = _vec(env, C), _vec(env, C)
    scale, shift = env["hiplib"].bn_moments_fold(_dev(env, case["part"]), case["R"], case["N"], _dev(env, case["gamma"]), _dev(env, case["beta"]),
                                                 0.0, mean[0], var[0])
    env["torch"].cuda.synchronize()
    for got, ref in ((_hvec(env, mean), case["mean"]), (_hvec(env, var), case["var"]), (scale.cpu().numpy(), case["scale"]),
                     (shift.cpu().numpy(), case["shift"])):
        assert bd.representable(ref) and bd.same(got, ref.astype(F))


# ---------------------------------------------------------------------------------------------------------------------------
# 5. pooling backward
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nchunks,C", bd.POOL_EXACT)
def test_pool_backward_family_exact(env, nchunks, C):
    """xv_pool_backward_f32 and xv_pool_bn_act_backward_f32 on the exact cases: chunk lengths 1, 2, 4, 8 with gaps of 0 to 2 rows, 3
    rows in front and 5 behind, NaN in h and r outside the chunks.  Chunk counts around the 16 merge groups and in the three
    row-group regimes of the element-wise kernel (16 groups, 11, 1)."""
    for case in bd.pool_exact_cases(nchunks, C):
        if C % 32 == 0:
            dg, db, dz, dec = run_pool_bn(env, case, split=True)
            _check_split(dz, dec)
            assert bd.bits_equal(dz, run_pool_bn(env, case)[2])
        else:
            dg, db, dz = run_pool_bn(env, case)
        check_pool_bn(case, dg, db, dz)
    check_pool_backward(case, run_pool_backward(env, case))
    if C > 4:
        odd = bd.odd_width(case, C - 3)
        check_pool_backward(odd, run_pool_backward(env, odd), name="pool_backward odd C")
        check_pool_backward(odd, run_pool_backward(env, odd, ld=C + 2), name="pool_backward ldh > C")


def test_pool_bn_act_backward_at_the_grid_limit(env):
    """65535 chunks of one row at C = 4 are accepted and exact; 65536 are refused before anything is launched."""
    case = bd.pool_grid_limit_case()
    check_pool_bn(case, *run_pool_bn(env, case))
    run_pool_bn(env, bd.pool_exact_case(bd.GRID_Y + 1, 4, "lrelu", seed=6, one_row=True), expect=BAD_ARG)


def test_pool_backward_more_than_65535_chunks(env):
    """65540 one-row chunks: the second slice of the host loop."""
    case = bd.pool_sliced_case()
    check_pool_backward(case, run_pool_backward(env, case))


@pytest.mark.parametrize("act", ("relu", "lrelu"))
@pytest.mark.parametrize("C", (24, 260))
@pytest.mark.parametrize("layout", sorted(bd.LAYOUTS))
def test_pool_backward_family_elementwise_bound(env, layout, C, act):
    case = bd.pool_bound_case(layout, C, act, seed=C + len(layout))
    dg, db, dz = run_pool_bn(env, case)
    assert np.isfinite(dz).all()
    check_pool_bn(case, dg, db, dz, _note)
    if act == "relu":
        check_pool_backward(case, run_pool_backward(env, case), _note)
        sub = bd.odd_width(case, 21)
        check_pool_backward(sub, run_pool_backward(env, sub, ld=23), _note, name="pool_backward C 21 ldh 23")


# ---------------------------------------------------------------------------------------------------------------------------
# 6. contracts
# ---------------------------------------------------------------------------------------------------------------------------
def test_short_row_strides_and_empty_matrices_are_refused(env):
    """ld < c (and R <= 0 for xv_pool_backward_f32) return XV_ERR_BAD_ARG before anything is launched."""
    torch, lib, dev = env["torch"], env["lib"], env["dev"]
    C, R = 8, 16
    x = torch.zeros((R, C), dtype=torch.float32, device=dev)
    v = torch.ones(4 * C, dtype=torch.float32, device=dev)
    out, o1 = _out(env, R, C), _vec(env, 4 * C)
    ws = torch.zeros(64 * C, dtype=torch.float64, device=dev)
    rs, rl = _dev(env, np.array([0], np.int32)), _dev(env, np.array([4], np.int32))
    for lda, ldb in ((C - 4, C), (C, C - 4), (0, C)):
        assert lib.xv_col_sums_f32(_p(x), lda, _p(x), ldb, R, C, _p(o1), _p(o1[0, C:]), _p(ws), None) == BAD_ARG
    assert lib.xv_col_sums_f32(_p(x), C - 1, None, 0, R, C, _p(o1), None, _p(ws), None) == BAD_ARG
    for ldx, ldy in ((C - 4, C), (C, C - 4)):
        assert lib.xv_rows_affine_f32(_p(x), ldx, R, C, _p(v), _p(v), None, _p(out), ldy, None) == BAD_ARG
        assert lib.xv_rows_affine_split_f32(_p(x), ldx, R, C, _p(v), _p(v), None, _p(out), ldy, None, None) == BAD_ARG
    bn = (_p(v), _p(v), _p(v), 1e-3, 16.0, 1, 0.0, None, _p(o1), _p(o1[0, C:]), _p(o1[0, 2 * C:]), _p(out))
    assert lib.xv_bn_act_backward_f32(_p(x), _p(x), C - 4, R, C, _p(v), _p(v), *bn, None) == BAD_ARG
    assert lib.xv_bn_act_backward_split_f32(_p(x), _p(x), C - 4, R, C, _p(v), _p(v), *bn, None, None) == BAD_ARG
    assert lib.xv_bn_act_backward_parts_f32(_p(x), _p(x), C - 4, R, C, _p(ws), *bn, None, None) == BAD_ARG
    assert lib.xv_pool_bn_act_backward_f32(_p(x), _p(x), C - 4, C, _p(rs), _p(rl), 1, R, _p(v), _p(v), _p(v), _p(v), _p(v), _p(v), 1e-3, 4.0,
                                           1, 0.0, _p(o1), _p(o1[0, C:]), _p(o1[0, 2 * C:]), _p(out), None, None) == BAD_ARG
    for ldh, rows in ((C - 4, R), (C, 0), (C, -1)):
        assert lib.xv_pool_backward_f32(_p(x), ldh, C, _p(rs), _p(rl), 1, rows, _p(v), _p(v), _p(out), None) == BAD_ARG
    assert np.isnan(_host(env, out, R)).all() and np.isnan(_hvec(env, o1)).all()       # nothing was launched
    assert lib.xv_pool_backward_f32(_p(x), C, C, _p(rs), _p(rl), 1, R, _p(v), _p(v), _p(out), None) == 0
    assert np.isfinite(_host(env, out, R)).all()


@pytest.mark.parametrize("empty", (0, -3))
def test_an_empty_chunk_adds_nothing(env, empty):
    """row_len <= 0 (pooled row NaN, as xv_stats_pool_f32 leaves it): dgamma, dbeta and dz of xv_pool_bn_act_backward_f32 and dh of
    xv_pool_backward_f32 have the bits they have without that chunk; its rows are zeroed."""
    C = 64
    case = bd.pool_exact_case(20, C, "lrelu", seed=3)
    at = 7
    ins = dict(case, rs=np.insert(case["rs"], at, case["rs"][at]), rl=np.insert(case["rl"], at, empty).astype(np.int32),
               pooled=np.insert(case["pooled"], at, np.nan, axis=0), dpooled=np.insert(case["dpooled"], at, 1.0, axis=0),
               cm=np.insert(case["cm"], at, np.nan, axis=0))
    ref, got = run_pool_bn(env, case), run_pool_bn(env, ins)
    check_pool_bn(case, *ref)
    for a, b in zip(ref, got):
        assert bd.bits_equal(a, b)
    assert bd.bits_equal(run_pool_backward(env, case), run_pool_backward(env, ins))
