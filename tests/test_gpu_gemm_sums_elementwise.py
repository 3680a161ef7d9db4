"""Per-tile checks of the two fused epilogues of tdnn_gemm_bf16x3_kernel (csrc/xv_gemm3.hip): xv_tdnn_layer_bf16x3_sums leaves
[sum y | sum y r] and xv_tdnn_layer_bf16x3_moments [sum r | sum r^2] per 128-row tile in the col_sums workspace, and the default
bf16x3 training step hands those partials straight to xv_bn_act_backward_parts_f32 / xv_bn_moments_fold_f32: a wrong partial is a
wrong gradient.  A merged sum compared with 1e-6 of the largest column hides one mis-weighted row, a small column or a wrong tile:

* exact known answers on integer data (tests/gemm_sums_data.py, "Exact cases"): EVERY (tile, which, column) slot equals the fp64
  sum over the tile's rows of the fp32 rows the kernel wrote, on fp32-row input, the 32 x 32 split form and the 16 x 16 split form
  (whose accumulators reach the epilogue tile by another lane map), every (K, dilation) the trainer uses, R = 1 / 127 / 128 / 129, a
  ragged layout, a tile of gap rows only (exact zeros), row_valid given and NULL (+-3e38 in the gap rows of sum_r), column slices
  of wider parents with NaN past R, every activation, with and without y_preact, all epilogue arguments or none;
* the rows themselves (y, y_preact) are bit-identical to xv_tdnn_layer_bf16x3 on the same arguments (128-row tiles), the same bits
  twice, and the same bits -- one partial per 128 rows -- with XV_TUNE_TILE_ROWS = 256 set; the workspace is overwritten in every slot
  and in no byte past xv_col_sums_workspace_bytes;
* element-wise bounds counted from the roundings of the source on realistic and hostile data with a mean-300 channel; the worst
  |part - ref| / bound per case is printed at the end; the kernel's own workspace through xv_col_sums_merge_f32 and
  xv_bn_moments_fold_f32 meets those consumers' bounds;
* the refusals of both entry points leave a poisoned y and workspace untouched.

check_parts and check_rows are plain NumPy: tests/test_gemm_sums_bounds_cpu.py feeds them the replay of the epilogue's summation
order (they must pass) and broken variants of it (they must fail)."""
import ctypes

import numpy as np
import pytest

import bnback_data as bd
import gemm_sums_data as gd

pytestmark = pytest.mark.gpu

WORST = {}
BAD_ARG, UNSUPPORTED = -1, -2
CANARY = 12345.0
F = np.float32


# ---------------------------------------------------------------------------------------------------------------------------
# checkers (NumPy only; shared with the CPU companion)
# ---------------------------------------------------------------------------------------------------------------------------
def check_rows(case, d, y):
    """Gap rows of y are exact zeros, every other element is finite."""
    y = np.asarray(y, F)
    assert y.shape == (d["R"], case.cout), (case.name, y.shape)
    gaps = y[~d["valid"]]
    assert (gaps == 0).all(), (case.name, "gap rows", int((gaps != 0).sum()))
    assert np.isfinite(y).all(), (case.name, "rows not finite")


def check_parts(case, d, y, parts, note=None):
    """Every (tile, which, column) slot of the workspace against the fp64 sum of the terms over the tile's rows, the terms formed
    from y, the fp32 rows the kernel itself wrote (and d["sum_r"]).  Exact cases: equality.  Otherwise |part - ref| <= bound.  A
    slot that was not written (NaN) fails either way; a tile of gap rows must hold exact zeros (its bound is 0)."""
    check_rows(case, d, y)
    parts = np.asarray(parts, np.float64)
    ref, mag = gd.parts_ref(case.entry, y, d["sum_r"])
    assert parts.shape == ref.shape, (case.name, parts.shape, ref.shape)
    if case.exact:
        bad = np.argwhere(~(parts == ref))
        assert bad.size == 0, (case.name, len(bad), [(tuple(int(i) for i in b), float(parts[tuple(b)]), float(ref[tuple(b)])) for b in bad[:5]])
        return
    bound = gd.parts_bound(case.entry, mag)
    ratio = bd.ratio(np.abs(parts - ref), bound)
    if note:
        note(case.name, ratio)
    if ratio > 1:
        err = np.where(np.isfinite(parts), np.abs(parts - ref) - bound, np.inf)
        at = np.unravel_index(int(np.argmax(err)), err.shape)
        raise AssertionError((case.name, ratio, tuple(int(i) for i in at), float(parts[at]), float(ref[at]), float(bound[at])))


def _note(key, value):
    WORST[key] = max(WORST.get(key, 0.0), float(value))


# ---------------------------------------------------------------------------------------------------------------------------
# device plumbing
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def env():
    import torch
    from xvector_amd import engine, hiplib
    hiplib.require_gpu()
    yield dict(torch=torch, hiplib=hiplib, engine=engine, lib=hiplib.load(), dev=torch.device("cuda:0"))
    if WORST:
        print("\nworst |part - ref| / bound per case (fused column-sum / moment epilogues of the bf16x3 GEMM):")
        for k in WORST:
            print("  %-44s %.3e" % (k, WORST[k]))


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _dev(env, a):
    return None if a is None else env["torch"].from_numpy(np.ascontiguousarray(a)).to(env["dev"])


class Staged(object):
    """The device arguments of one case: inputs uploaded once, outputs made per run."""

    def __init__(self, env, case, d):
        hiplib = env["hiplib"]
        self.env, self.case, self.d = env, case, d
        R, cin, cout = d["R"], case.cin, case.cout
        self.ldy, self.ycol, self.ldr, self.rcol, self.ldpre, self.pcol = gd.geometry(case)
        if case.split:
            self.xbuf = hiplib.SplitBuf(R, cin, env["dev"])
            hiplib.split_encode(_dev(env, d["x"]), self.xbuf)
            self.x, self.xfmt, self.ldx = ctypes.c_void_p(self.xbuf.ptr), hiplib.FMT_SPLIT, 0
        else:
            self.ldx = cin + 8                              # fp32 rows as a column slice: ldx > cin, NaN around it and past R
            self.xbuf = _dev(env, gd.wide_of(d["x"], self.ldx, 4))
            self.x, self.xfmt = _p(self.xbuf[:, 4:]), hiplib.FMT_F32
        self.w = hiplib.pack_weights_bf16x3(_dev(env, d["w"]))
        self.b, self.scale, self.shift, self.alpha = (_dev(env, d[k]) for k in ("b", "scale", "shift", "alpha"))
        self.rv = _dev(env, d["valid"].astype(np.uint8)) if case.valid else None
        self.r_host = gd.wide_of(d["sum_r"], self.ldr, self.rcol) if case.entry == "sums" else None
        self.r = _dev(env, self.r_host)
        self.slots = gd.tiles(R) * 2 * cout
        assert int(env["lib"].xv_col_sums_workspace_bytes(R, cout)) == gd.workspace_bytes(R, cout) == 8 * self.slots

    def run(self, entry):
        """entry: "sums" / "moments" / "plain" (xv_tdnn_layer_bf16x3 on the same arguments).  -> (y [R, cout], y_preact or None,
        workspace [tiles, 2, cout] or None); NaN-poisoned outputs, nothing outside the column slices, past R or past the workspace's
        byte count may change."""
        env, case, d = self.env, self.case, self.d
        torch, lib, dev = env["torch"], env["lib"], env["dev"]
        R, cout = d["R"], case.cout
        ypar = torch.full((R + gd.PAD_ROWS, self.ldy), float("nan"), dtype=torch.float32, device=dev)
        y = ypar[:, self.ycol:]
        ppar = pre = None
        if case.ypre and case.entry == "moments":
            ppar = torch.full((R + gd.PAD_ROWS, self.ldpre), float("nan"), dtype=torch.float32, device=dev)
            pre = ppar[:, self.pcol:]
        ws = torch.full((self.slots + 8,), float("nan"), dtype=torch.float64, device=dev)
        ws[self.slots:] = CANARY
        head = (self.x, self.xfmt, R, case.cin, self.ldx, _p(self.w.wt), _p(self.b), _p(self.scale), _p(self.shift), gd.ACT_CODE[d["act"]],
                _p(self.alpha), case.K, case.dil, cout, _p(self.rv), _p(y))
        if entry == "sums":
            rc = lib.xv_tdnn_layer_bf16x3_sums(*head, self.ldy, _p(self.r[:, self.rcol:]), self.ldr, _p(ws), None)
        elif entry == "moments":
            rc = lib.xv_tdnn_layer_bf16x3_moments(*head, self.ldy, _p(pre), self.ldpre if pre is not None else 0, _p(ws), None)
        else:
            rc = lib.xv_tdnn_layer_bf16x3(*head, env["hiplib"].FMT_F32, self.ldy, _p(pre), self.ldpre if pre is not None else 0, None)
        assert rc == 0, (case.name, entry, rc, lib.xv_last_error())
        torch.cuda.synchronize()
        out = []
        for par, col in ((ypar, self.ycol), (ppar, self.pcol)):
            if par is None:
                out.append(None)
                continue
            h = par.cpu().numpy()
            keep = np.zeros(h.shape, bool)
            keep[:R, col:col + cout] = True
            assert np.isnan(h[~keep]).all(), (case.name, entry, "wrote outside the column slice or past R")
            out.append(np.ascontiguousarray(h[:R, col:col + cout]))
        wh = ws.cpu().numpy()
        assert (wh[self.slots:] == CANARY).all(), (case.name, entry, "wrote past the workspace's byte count")
        if entry == "plain":
            assert np.isnan(wh[:self.slots]).all()
            out.append(None)
        else:
            assert not np.isnan(wh[:self.slots]).any(), (case.name, entry, "a workspace slot was not written")
            out.append(wh[:self.slots].reshape(gd.tiles(R), 2, cout))
        return out


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _with_tile_rows(env, rows, fn):
    hiplib = env["hiplib"]
    try:
        hiplib.set_tuning(hiplib.TUNE_TILE_ROWS, rows)
        return fn()
    finally:
        hiplib.set_tuning(hiplib.TUNE_TILE_ROWS, 0)


def _run_pinned(env, case, d):
    """One case through its entry point: (y, y_preact, parts) after the pins that hold in EVERY case -- the rows are those of the
    plain layer (128-row tiles) bit for bit, a second run and a run with XV_TUNE_TILE_ROWS = 256 give the same bits."""
    st = Staged(env, case, d)
    y, pre, parts = st.run(case.entry)
    y0, pre0, _ = _with_tile_rows(env, 128, lambda: st.run("plain"))
    assert _same(y, y0), (case.name, "y differs from xv_tdnn_layer_bf16x3")
    assert _same(pre, pre0), (case.name, "y_preact differs from xv_tdnn_layer_bf16x3")
    again = st.run(case.entry)
    assert all(_same(a, b) for a, b in zip((y, pre, parts), again)), (case.name, "a second run gives other bits")
    knob = _with_tile_rows(env, 256, lambda: st.run(case.entry))
    assert all(_same(a, b) for a, b in zip((y, pre, parts), knob)), (case.name, "XV_TUNE_TILE_ROWS = 256 changes the result")
    return st, y, pre, parts


# ---------------------------------------------------------------------------------------------------------------------------
# 1. exact answers
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", gd.EXACT_CASES, ids=[c.name for c in gd.EXACT_CASES])
def test_partials_exact_on_integer_data(env, case):
    """Every slot equals the fp64 reference; y (and y_preact) are also the known integer answer of the layer, so the sums are those
    of the final output when bias, scale, shift and an activation are passed."""
    d = gd.build(case)
    if case.rows == "ragged":                               # the ragged rows are a BatchLayout's
        lay = env["engine"].BatchLayout(gd.RAGGED, 3)
        assert lay.rows == d["R"] and np.array_equal(lay.row_valid().astype(bool), d["valid"])
    st, y, pre, parts = _run_pinned(env, case, d)
    check_parts(case, d, y, parts)
    rows = gd.layer_rows(case, d)
    assert np.array_equal(y, rows["y"]), (case.name, "y is not the exact answer")
    if pre is not None:
        assert np.array_equal(pre, rows["ypre"]), (case.name, "y_preact is not the exact answer")
    if case.rows == "gaptile":
        assert (parts[1] == 0).all() and (parts[0] != 0).any() and (parts[2] != 0).any()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. element-wise bounds, the consumers behind the workspace
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", gd.BOUND_CASES, ids=[c.name for c in gd.BOUND_CASES])
def test_partials_within_the_bound(env, case):
    """Realistic (post-ReLU) and hostile (channel scales over three decades, dead channels, heavy-tailed weights) x and w, a
    channel whose bias is 300 over a unit spread, post-ReLU sum_r (hostile: column scales over three decades).  Then the kernel's own
    workspace through its consumer: xv_col_sums_merge_f32 (one rounding of the fp64 sum of the partials + dust: bnback_data's
    bound for the merge) or xv_bn_moments_fold_f32 (mean, var from the same merge; scale, shift the float32 fold of the kernel's
    own mean and var, bit for bit)."""
    torch, hiplib, lib, dev = env["torch"], env["hiplib"], env["lib"], env["dev"]
    d = gd.build(case)
    st, y, pre, parts = _run_pinned(env, case, d)
    check_parts(case, d, y, parts, _note)
    R, C = d["R"], case.cout
    ws = _dev(env, parts)
    out = torch.full((4, C), float("nan"), dtype=torch.float32, device=dev)
    if case.entry == "sums":
        assert lib.xv_col_sums_merge_f32(_p(ws), R, C, _p(out[0]), _p(out[1]), None) == 0
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        for k in range(2):
            ref, _, bound, _ = bd.col_sums_ref(parts[:, k], None)
            r = bd.ratio(np.abs(got[k].astype(np.float64) - ref), bound)
            _note("%s -> col_sums_merge %s" % (case.name, ("sum y", "sum y r")[k]), r)
            assert r <= 1, (case.name, k, r)
        merged = bd.replay_merge(parts).astype(F)
        assert bd.bits_equal(got[0], merged[0]) and bd.bits_equal(got[1], merged[1])
    else:
        n = float(d["valid"].sum())
        rng = np.random.default_rng(case.seed)
        gamma, beta = (1.0 + 0.2 * rng.standard_normal(C)).astype(F), (0.1 * rng.standard_normal(C)).astype(F)
        g_dev, b_dev = _dev(env, gamma), _dev(env, beta)
        assert lib.xv_bn_moments_fold_f32(_p(ws), R, C, n, _p(g_dev), _p(b_dev), bd.BN_EPS, _p(out[0]), _p(out[1]), _p(out[2]), _p(out[3]),
                                          None) == 0
        torch.cuda.synchronize()
        mean, var, scale, shift = out.cpu().numpy()
        m, v, bm, bv = gd.fold_ref(parts, n)
        for name, g, ref, bound in (("mean", mean, m, bm), ("var", var, v, bv)):
            r = bd.ratio(np.abs(g.astype(np.float64) - ref), bound)
            _note("%s -> bn_moments_fold %s" % (case.name, name), r)
            assert r <= 1, (case.name, name, r)
        sc, sf = bd.fold32(mean, var, gamma, beta, bd.BN_EPS)
        assert bd.bits_equal(scale, sc) and bd.bits_equal(shift, sf)
        # the moments are those of the rows: in the large-mean channel (mean^2 / var ~ 1e5, where an fp32 sum of squares loses the
        # variance) one fp32 rounding of the variance plus 2^-46 of the two terms that cancel
        col = y[d["valid"], gd.LARGE_MEAN_CHANNEL].astype(np.float64)
        assert abs(float(var[gd.LARGE_MEAN_CHANNEL]) - col.var()) <= 2.0 ** -24 * col.var() + 2.0 ** -46 * (col.mean() ** 2 + col.var())


# ---------------------------------------------------------------------------------------------------------------------------
# 3. refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(env):
    """Each argument either entry point refuses, one at a time from a call that is accepted: the code the source gives, and nothing
    launched (y and the workspace keep their poison)."""
    torch, hiplib, lib, dev = env["torch"], env["hiplib"], env["lib"], env["dev"]
    R, cin, cout = 16, 32, 8
    x = torch.ones((R, cin), dtype=torch.float32, device=dev)
    w = hiplib.pack_weights_bf16x3(torch.ones((1, cin, 16), dtype=torch.float32, device=dev))
    y = torch.full((R + 1, 16), float("nan"), dtype=torch.float32, device=dev)
    r = torch.ones((R + 1, 16), dtype=torch.float32, device=dev)
    ws = torch.full((64,), float("nan"), dtype=torch.float64, device=dev)
    ws_odd = ctypes.c_void_p(ws.data_ptr() + 4)
    r_odd = ctypes.c_void_p(r.data_ptr() + 4)
    base = dict(x=_p(x), fmt=hiplib.FMT_F32, R=R, cin=cin, ldx=cin, wt=_p(w.wt), bias=None, scale=None, shift=None, act=0, alpha=None, K=1,
                dil=1, cout=cout, rv=None, y=_p(y), ldy=16, r=_p(r), ldr=16, pre=None, ldpre=0, ws=_p(ws))

    def call(entry, **kw):
        a = dict(base, **kw)
        head = (a["x"], a["fmt"], a["R"], a["cin"], a["ldx"], a["wt"], a["bias"], a["scale"], a["shift"], a["act"], a["alpha"], a["K"],
                a["dil"], a["cout"], a["rv"], a["y"], a["ldy"])
        if entry == "sums":
            return lib.xv_tdnn_layer_bf16x3_sums(*head, a["r"], a["ldr"], a["ws"], None)
        return lib.xv_tdnn_layer_bf16x3_moments(*head, a["pre"], a["ldpre"], a["ws"], None)

    both = [(dict(cout=12), UNSUPPORTED), (dict(ldy=18), UNSUPPORTED), (dict(ws=ws_odd), UNSUPPORTED),
            (dict(y=None), BAD_ARG), (dict(ws=None), BAD_ARG), (dict(x=None), BAD_ARG), (dict(wt=None), BAD_ARG),
            (dict(act=4), BAD_ARG), (dict(act=-1), BAD_ARG), (dict(fmt=2), BAD_ARG), (dict(fmt=-1), BAD_ARG),
            (dict(act=2, alpha=None), BAD_ARG), (dict(act=3, alpha=None), BAD_ARG), (dict(K=2), BAD_ARG), (dict(K=0), BAD_ARG)]
    sums_only = [(dict(ldr=18), UNSUPPORTED), (dict(ldr=4), UNSUPPORTED), (dict(r=r_odd), UNSUPPORTED), (dict(r=None), BAD_ARG)]
    for entry, table in (("sums", both + sums_only), ("moments", both)):
        for kw, code in table:
            assert call(entry, **kw) == code, (entry, kw, code, lib.xv_last_error())
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all()) and bool(torch.isnan(ws).all())          # nothing was launched
    for entry in ("sums", "moments"):                                           # and the call they were derived from is accepted
        assert call(entry) == 0, (entry, lib.xv_last_error())
    torch.cuda.synchronize()
    assert bool((y[:R, :cout] == cin).all()) and bool(torch.isnan(y[R:]).all()) and bool(torch.isnan(y[:, cout:]).all())
    got = ws.cpu().numpy()
    assert (got[:cout] == R * cin).all() and (got[cout:2 * cout] == R * cin * cin).all() and np.isnan(got[2 * cout:]).all()
