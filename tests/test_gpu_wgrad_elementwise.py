"""Element-wise checks of the weight-gradient kernels xv_wgrad_f32 (csrc/xv_train.hip), xv_wgrad_bf16x3 and xv_wgrad_bias_bf16x3
(csrc/xv_wgrad.hip); a relative-L2 number over [K, Cin, Cout] hides a wrong tap, row end, tile edge or split:

* exact known answers: integer x, dz in [-3, 3] (every partial sum below 2^24, the bf16 lo planes zero) -- dw equals the int64
  reference in EVERY element for all three entry points, db equals sum_r dz; the shapes of tests/wgrad_data.py (R below a step and
  below the tap reach, the split + ordered merge, ragged tiles, the scalar load path, column and row slices in NaN-filled parents);
* one-hot read-back: dz = one 1 per column, so dw[k, :, o] IS one row of x (fp32: bit for bit, bf16x3: its hi + lo decoding, zero
  where the row falls outside [0, R)) -- the tap sign, the ends and the LDS transposition without any accumulation;
* element-wise bounds on realistic and hostile data: |dw - dw_ref| <= A 2^-24 M, dw_ref / M from tests/arith_emul.py, A fixed in
  tests/wgrad_data.py; |db - sum dz| <= 15 2^-24 sum |dz| + 2^-24 |db|.  The worst ratio per case is printed at the end;
* the 2^31-byte switch of the bf16x3 entry points, one row below it and at it.

Every call runs all three entry points: dw (with a sentinel tail) and db are NaN-poisoned, xv_wgrad_bias_bf16x3's dw must be the
bits of xv_wgrad_bf16x3's, and a second call must give the same bits."""
import ctypes

import numpy as np
import pytest

import arith_emul as em
import wgrad_data as wd

pytestmark = pytest.mark.gpu

WORST = {}
TAIL = 64                    # sentinel floats behind dw
SENTINEL = -12345.0


@pytest.fixture(scope="module")
def env(oracle_mod):
    import torch
    from xvector_amd import hiplib
    hiplib.require_gpu()
    yield dict(torch=torch, hiplib=hiplib, oracle=oracle_mod, dev=torch.device("cuda:0"))
    if WORST:
        print("\nworst |dw - dw_ref| / (A 2^-24 M) per case and entry point; worst |db - sum dz| / bound:")
        for name, (rows, rdb) in WORST.items():
            print("  %-44s %s   db %.3e" % (name, "   ".join("%s A = %5.1f ratio %.3e" % (a, A, r) for a, A, r in rows), rdb))


def _operands(env, case, x, dz):
    """Device views of x and dz inside their NaN-filled parents."""
    torch, dev = env["torch"], env["dev"]
    views = []
    for a, which in ((x, "x"), (dz, "dz")):
        buf, idx = case.place(a, which)
        views.append(torch.from_numpy(buf).to(dev)[idx])
    return views


def run_all(env, case, x, dz, bias=True):
    """dw of the three entry points + db, after the checks every call makes.  Returns (dw_f32, dw_bf16x3, db, splits)."""
    torch, hiplib, dev = env["torch"], env["hiplib"], env["dev"]
    K, cin, cout = case.K, case.cin, case.cout
    xd, zd = _operands(env, case, x, dz)
    n = K * cin * cout
    ws = hiplib.load().xv_wgrad_workspace_bytes(case.R, cin, cout, K)
    splits = case.splits(ws)

    def call(precision, with_db):
        buf = torch.full((n + TAIL,), float("nan"), dtype=torch.float32, device=dev)
        buf[n:] = SENTINEL
        db = torch.full((cout,), float("nan"), dtype=torch.float32, device=dev) if with_db else None
        hiplib.wgrad(xd, zd, K, case.dil, buf[:n].view(K, cin, cout), precision, db=db)
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert (host[n:] == SENTINEL).all(), (case.name, precision, "wrote behind dw")
        return host[:n].reshape(K, cin, cout), None if db is None else db.cpu().numpy()

    out = {}
    for key, precision, with_db in (("f32", "fp32", False), ("bf16x3", "bf16x3", False), ("bias", "bf16x3", True)):
        if with_db and not bias:
            continue
        dw, db = call(precision, with_db)
        dw2, db2 = call(precision, with_db)
        assert np.array_equal(dw.view(np.uint32), dw2.view(np.uint32)), (case.name, key, "a second call gives other bits")
        if with_db:
            assert np.array_equal(db.view(np.uint32), db2.view(np.uint32)), (case.name, "db: a second call gives other bits")
        out[key] = (dw, db)
    if bias:
        assert np.array_equal(out["bias"][0].view(np.uint32), out["bf16x3"][0].view(np.uint32)), (case.name, "bias entry: other dw bits")
    return out["f32"][0], out["bf16x3"][0], out["bias"][1] if bias else None, splits


def _first_bad(got, ref):
    bad = np.argwhere(~(got == ref))
    return [(tuple(int(i) for i in b), float(got[tuple(b)]), float(ref[tuple(b)])) for b in bad[:5]], len(bad)


# ---------------------------------------------------------------------------------------------------------------------------
# (a) exact known answers
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", wd.EXACT_CASES, ids=[c.name for c in wd.EXACT_CASES])
def test_exact_on_integer_data(env, case):
    x, dz = case.data()
    ref, dbref = wd.exact_ref(x, dz, case.K, case.dil)
    f32, b3, db, splits = run_all(env, case, x, dz)
    assert (splits > 1) == case.name.startswith(wd.SPLIT_CASES), (case.name, splits)      # the merge path is not skipped quietly
    for key, got in (("xv_wgrad_f32", f32), ("xv_wgrad_bf16x3", b3)):
        bad, nbad = _first_bad(got.astype(np.float64), ref.astype(np.float64))
        assert nbad == 0, (case.name, key, nbad, bad)
    bad, nbad = _first_bad(db.astype(np.float64), dbref.astype(np.float64))
    assert nbad == 0, (case.name, "db", nbad, bad)


# ---------------------------------------------------------------------------------------------------------------------------
# (b) one-hot read-back
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", wd.ONEHOT_CASES, ids=[c.name for c in wd.ONEHOT_CASES])
def test_one_hot_dz_reads_rows_of_x_back(env, case):
    """dz[r_j, o_j] = 1 for distinct columns o_j, zero elsewhere: dw[k, :, o_j] = x[r_j + (k - (K-1)/2) d] (zero outside [0, R)),
    every other column of dw exactly zero."""
    hiplib = env["hiplib"]
    K, d, R, cout = case.K, case.dil, case.R, case.cout
    x = wd.onehot_x(case)
    splits = case.splits(hiplib.load().xv_wgrad_workspace_bytes(R, case.cin, cout, K))
    rows = wd.onehot_rows(case, splits)
    assert (splits > 1) == ("splits" in case.name)
    rng = np.random.default_rng(R)
    h = (K - 1) // 2
    for g in range(0, len(rows), cout):                                                  # groups of up to cout rows, one column each
        grp = rows[g:g + cout]
        cols = rng.permutation(cout)[:len(grp)]
        dz = np.zeros((R, cout), np.float32)
        dz[grp, cols] = 1.0
        f32, b3, db, _ = run_all(env, case, x, dz)
        want = np.zeros((K, case.cin, cout), np.float32)
        for r, o in zip(grp, cols):
            for k in range(K):
                src = r + (k - h) * d
                if 0 <= src < R:
                    want[k, :, o] = x[src]
        for key, got, exp in (("xv_wgrad_f32", f32, want), ("xv_wgrad_bf16x3", b3, em.decode3(want) + np.float32(0))):   # (+ 0: a sum from +0 has no -0)
            bad = np.argwhere(got.view(np.uint32) != exp.view(np.uint32))
            assert bad.size == 0, (case.name, key, len(bad), [(tuple(int(i) for i in b), float(got[tuple(b)]), float(exp[tuple(b)])) for b in bad[:5]],
                                   "r*, o*:", list(zip(grp, cols.tolist()))[:8])
        assert np.array_equal(db, dz.sum(0))


# ---------------------------------------------------------------------------------------------------------------------------
# (c) element-wise bounds on realistic and hostile data
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", wd.BOUND_CASES, ids=[c.name for c in wd.BOUND_CASES])
def test_elementwise_bound(env, case):
    """|dw - dw_ref| <= A 2^-24 M in every element, A = sqrt(depth) with the depth of tests/wgrad_data.py (fixed before the first
    device run, not re-tuned).

    The bf16x3 kernel met this only after its cross terms got an accumulator of their own: with lo*hi, hi*lo and hi*hi in one
    accumulator "relu 300 x 512 x 512 K5" reached 1.242 (7 of 1 310 720 elements above 1).  Replaying that order on the CPU gave
    0.861 with one fp32 rounding of the accumulator per MFMA and 1.242, at the same tap, with two -- v_mfma_f32_32x32x16_bf16
    rounds per 8 products -- i.e. 6 roundings of the whole sum per 16 rows where this bound counts 3.  With the cross terms apart
    the hi*hi sum is rounded twice per 16 rows, the replay gives 0.583 and so does the device."""
    x, dz = case.data()
    f32, b3, db, splits = run_all(env, case, x, dz)
    assert (splits > 1) == ("splits" in case.name)
    rows = []
    fails = []
    for arith, got in (("fp32", f32), ("bf16x3", b3)):
        ref, M = em.wgrad(arith, x, dz, case.K, case.dil)          # fp32: the fp64 products themselves
        A = case.A(arith, splits)
        assert np.isfinite(got).all()
        err = np.abs(got.astype(np.float64) - ref)
        bnd = A * em.U * M
        ratio = np.where(bnd > 0, err / np.where(bnd > 0, bnd, 1.0), np.where(err > 0, np.inf, 0.0))    # M = 0: exactly zero
        worst = float(ratio.max())
        print("%s %s: A = %.2f, worst ratio %.3e at %s" % (case.name, arith, A, worst, np.unravel_index(np.argmax(ratio), ratio.shape)))
        rows.append((arith, A, worst))
        if worst > 1:
            fails.append((arith, worst, np.unravel_index(np.argmax(ratio), ratio.shape), int((ratio > 1).sum())))
    dbref = dz.astype(np.float64).sum(0)
    rdb = float((np.abs(db - dbref) / np.maximum(wd.db_bound(dz), 1e-300)).max())
    print("%s db: worst ratio %.3e" % (case.name, rdb))
    WORST[case.name] = (rows, rdb)
    assert not fails, (case.name, fails)
    assert rdb <= 1, (case.name, rdb)


# ---------------------------------------------------------------------------------------------------------------------------
# (d) the 2^31-byte switch of the bf16x3 entry points
# ---------------------------------------------------------------------------------------------------------------------------
BIG_LD, BIG_COUT, BIG_K = 512, 8, 3


def _big_operands(env, R):
    """Integer x [R, 512] (2 GB at R = 2^20), dz [R, 8], made on the device in slabs; about half zeros."""
    torch, dev = env["torch"], env["dev"]
    gen = torch.Generator(device=dev)
    gen.manual_seed(R)
    x = torch.empty((R, BIG_LD), dtype=torch.float32, device=dev)
    for r0 in range(0, R, 1 << 16):
        sl = x[r0:r0 + (1 << 16)]
        v = torch.randint(-3, 4, sl.shape, generator=gen, device=dev, dtype=torch.int8)
        keep = torch.rand(sl.shape, generator=gen, device=dev) < 0.58
        sl.copy_(v * keep)
    dz = (torch.randint(-3, 4, (R, BIG_COUT), generator=gen, device=dev, dtype=torch.int8)
          * (torch.rand((R, BIG_COUT), generator=gen, device=dev) < 0.58)).to(torch.float32)
    return x, dz


def _big_ref(x, dz, K, step=1 << 16):
    """fp64 dw [K, 512, 8] and db of integer data, in slabs of rows (exact: every sum is an integer below 2^24)."""
    R = x.shape[0]
    assert R * 9 < 2 ** 24
    h = (K - 1) // 2
    zh = dz.cpu().numpy().astype(np.float64)
    dw = np.zeros((K, x.shape[1], dz.shape[1]))
    for r0 in range(0, R, step):
        r1 = min(R, r0 + step)
        lo, hi = max(0, r0 - h), min(R, r1 + h)
        xs = x[lo:hi].cpu().numpy().astype(np.float64)
        for k in range(K):
            s = k - h                                                      # dw[k] += x[r + s]^T dz[r], r in [r0, r1), 0 <= r + s < R
            a, b = max(r0, -s), min(r1, R - s)
            dw[k] += xs[a + s - lo:b + s - lo].T @ zh[a:b]
    return dw, zh.sum(0)


def test_one_row_below_two_to_the_31_bytes_stays_exact(env):
    """R * ldx * 4 = 2^31 - 2048: the bf16x3 kernel itself runs, its 32-bit offsets wrap behind the last row (the steps that reach
    past R, the taps that reach past it) -- dw and db exact."""
    torch, hiplib, dev = env["torch"], env["hiplib"], env["dev"]
    R = (1 << 31) // (BIG_LD * 4) - 1
    x, dz = _big_operands(env, R)
    assert hiplib.wgrad_takes_bias("bf16x3", x, dz)
    dw = torch.full((BIG_K, BIG_LD, BIG_COUT), float("nan"), dtype=torch.float32, device=dev)
    db = torch.full((BIG_COUT,), float("nan"), dtype=torch.float32, device=dev)
    hiplib.wgrad(x, dz, BIG_K, 1, dw, "bf16x3", db=db)
    dw3 = torch.full_like(dw, float("nan"))
    hiplib.wgrad(x, dz, BIG_K, 1, dw3, "bf16x3")
    torch.cuda.synchronize()
    ref, dbref = _big_ref(x, dz, BIG_K)
    del x
    torch.cuda.empty_cache()
    for key, got in (("xv_wgrad_bias_bf16x3", dw), ("xv_wgrad_bf16x3", dw3)):
        bad, nbad = _first_bad(got.cpu().numpy().astype(np.float64), ref)
        assert nbad == 0, (key, nbad, bad)
    assert np.array_equal(db.cpu().numpy().astype(np.float64), dbref)


def test_at_two_to_the_31_bytes_bf16x3_is_the_fp32_kernel_and_the_bias_entry_refuses(env):
    torch, hiplib, dev = env["torch"], env["hiplib"], env["dev"]
    R = (1 << 31) // (BIG_LD * 4)
    x, dz = _big_operands(env, R)
    assert not hiplib.wgrad_takes_bias("bf16x3", x, dz)
    dw = torch.full((BIG_K, BIG_LD, BIG_COUT), float("nan"), dtype=torch.float32, device=dev)
    dw3 = torch.full_like(dw, float("nan"))
    hiplib.wgrad(x, dz, BIG_K, 1, dw, "fp32")
    hiplib.wgrad(x, dz, BIG_K, 1, dw3, "bf16x3")
    torch.cuda.synchronize()
    a, b = dw.cpu().numpy(), dw3.cpu().numpy()
    assert np.isfinite(a).all() and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # the raw binding: the Python wrapper asserts wgrad_takes_bias first
    lib = hiplib.load()
    ws = torch.empty(max(int(lib.xv_wgrad_bias_workspace_bytes(R, BIG_LD, BIG_COUT, BIG_K)), 8), dtype=torch.uint8, device=dev)
    db = torch.full((BIG_COUT,), float("nan"), dtype=torch.float32, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = lib.xv_wgrad_bias_bf16x3(p(x), BIG_LD, p(dz), BIG_COUT, R, BIG_LD, BIG_COUT, BIG_K, 1, p(dw3), p(db), p(ws), None)
    torch.cuda.synchronize()
    assert rc == -2, rc                                                   # XV_ERR_UNSUPPORTED
    assert np.isnan(db.cpu().numpy()).all()                              # and nothing was launched
    del x
    torch.cuda.empty_cache()
