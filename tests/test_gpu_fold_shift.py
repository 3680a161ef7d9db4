"""The BN-shift fold on the device: the per-row bias of the f16bf8 GEMM family (tap_bias of xv_tdnn_layer_f16bf8 /
xv_tdnn_layer_pool_f16bf8), the load-time table kernel, and the folded network.

Per kernel form, on ONE layout of 264 rows (a full 256-row tile and a partial one; chunks on 8-row starts with >= 3 gap rows; chunks
shorter than K; a chunk that ends on row 127, the last row of a 128-row tile; a chunk that straddles row 256 AND ends on the last
row of the batch, so neighbour validity is read across tile edges from global memory and past R):
  (a) exact data (halves and small integers: every sum exact in fp32, the table too): activations u with bias_full and the table
      give bit for bit what the same kernel gives on y = u + shift with the plain bias; gap rows zero; output poisoned first;
  (b) random data: within the element-wise bound of the form's layer tests (tests/arith_emul.py) of the emulated arithmetic with
      the fp64 per-row bias;
  (c) the same chunk at two row offsets (inside a tile / straddling one and ending the batch): identical bits;
  (d) a K = 1 layer refuses a table.
The forms are forced with XV_TUNE_TILE_ROWS (the library does not report which kernel ran; launch_gemm8 refuses nothing quietly:
the shapes below satisfy what each forced form needs -- see the asserts in _run)."""
import numpy as np
import pytest

import arith_emul as em

pytestmark = pytest.mark.gpu

R = 264
STARTS = [8, 16, 24, 40, 104, 136, 240]
LENS = [1, 4, 9, 61, 24, 93, 24]            # chunk 4 (rows 104..127) and chunk 6 (240..263) carry the same frames
TWIN = (4, 6)
GAP = 3
# (name, tile knob, cin, cout, K, dil): the smallest shapes launch_gemm8 routes to each form under its knob
FORMS = [
    ("wide16 K=5", 1024, 64, 256, 5, 1),     # 16 x 16 MFMAs: an even number of slabs, Cout % 256 == 0
    ("wide16 K=7", 1024, 64, 256, 7, 1),
    ("wide16 K=3 d2", 1024, 64, 256, 3, 2),
    ("wide 32x32 K=3 d2", 512, 32, 256, 3, 2),   # one slab: the 16 x 16 form cannot take it
    ("wide 32x32 K=7", 512, 32, 256, 7, 1),
    ("128-row K=5", 128, 32, 128, 5, 1),
    ("128-row K=3 d2", 128, 32, 128, 3, 2),
    ("256-row K=7, ragged Cout", 256, 32, 136, 7, 1),
]


class Layout(object):
    """What the helpers of tests/pair_data.py and the checks below need of a batch layout, for hand-placed chunks."""

    def __init__(self):
        self.rows, self.row_start, self.row_len = R, np.array(STARTS, np.int32), np.array(LENS, np.int32)
        v = np.zeros(R, np.uint8)
        for s, n in zip(STARTS, LENS):
            assert s % 8 == 0 and not v[max(s - GAP, 0):s].any()
            v[s:s + n] = 1
        self._valid = v
        assert v[127] and not v[128] and v[255] and v[256] and v[R - 1]

    def row_valid(self):
        return self._valid

    def pack(self, mats):
        x = np.zeros((R, mats[0].shape[1]), np.float32)
        for s, m in zip(STARTS, mats):
            x[s:s + m.shape[0]] = m
        return x


@pytest.fixture(scope="module")
def env():
    import torch
    from xvector_amd import engine, hiplib
    hiplib.require_gpu()
    return dict(torch=torch, hiplib=hiplib, engine=engine, dev=torch.device("cuda:0"), lay=Layout())


def _run(env, tile, x_rows, w, bias, scale, shift, tapbias, dil, fmt="split8", pool=False):
    """One launch of the forced form on packed rows x_rows [R, cin]; returns (decoded fp32 [R, cout] or block statistics, raw bytes)."""
    torch, hiplib, dev, lay = env["torch"], env["hiplib"], env["dev"], env["lay"]
    K, cin, cout = w.shape
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    if tile >= 512:
        assert K > 1 and cout % 256 == 0 and (pool or fmt != "f32"), "256 x 256 tile not reachable"
        assert tile == 512 or ((cin + 31) // 32) % 2 == 0, "16 x 16 form needs an even number of slabs"
    x = hiplib.SplitBuf(R, cin, dev, hiplib.FMT_SPLIT8)
    hiplib.split_encode(t(x_rows), x)
    rv = torch.from_numpy(lay.row_valid()).to(dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    wp = hiplib.pack_weights_f16bf8(t(w))
    args = (t(bias), t(scale), t(shift), em.ACT["relu"], None)
    if pool:
        y = torch.full((hiplib.block_stats_floats(R, cout),), float("nan"), dtype=torch.float32, device=dev)
    elif fmt == "f32":
        y = torch.full((R, cout), float("nan"), dtype=torch.float32, device=dev)
    else:
        y = hiplib.SplitBuf(R, cout, dev, hiplib.FMT_SPLIT8 if fmt == "split8" else hiplib.FMT_SPLIT)
        y.base.fill_(0x7b)
    try:
        hiplib.set_tuning(hiplib.TUNE_TILE_ROWS, tile)
        if pool:
            hiplib.tdnn_layer_pool8(x, R, wp, *args, dil, rv, y, tapbias=t(tapbias))
        else:
            hiplib.tdnn_layer8(x, R, wp, *args, dil, rv, y, status, tapbias=t(tapbias))
        torch.cuda.synchronize()
    finally:
        hiplib.set_tuning(hiplib.TUNE_TILE_ROWS, 0)
    assert int(status.item()) == 0
    if pool:
        out = y.cpu().numpy().reshape(-1, 2, cout)
        return out, out.tobytes()
    if fmt == "f32":
        out = y.cpu().numpy()
        return out, out.tobytes()
    out = hiplib.split_decode(y, R).cpu().numpy()
    return out, y.base.cpu().numpy().tobytes()


def _exact_data(rng, K, cin, cout):
    """Halves and small integers: u >= 0 with zeros (a ReLU's output), shifts of both signs, sparse integer weights."""
    mats = [(rng.integers(0, 7, (n, cin)) * (rng.random((n, cin)) < 0.5) * 0.5).astype(np.float32) for n in LENS]
    mats[TWIN[1]] = mats[TWIN[0]].copy()
    w = (rng.integers(-3, 4, (K, cin, cout)) * (rng.random((K, cin, cout)) < 0.3)).astype(np.float32)
    shift_in = (rng.integers(-4, 5, cin) * 0.5).astype(np.float32)
    shift_in[shift_in == 0] = 1.5
    bias = rng.integers(-4, 5, cout).astype(np.float32)
    scale = rng.choice([0.5, 1.0, 2.0], cout).astype(np.float32)
    shift_out = (rng.integers(-4, 5, cout) * 0.5).astype(np.float32)
    return mats, w, shift_in, bias, scale, shift_out


def _fold(env, w, shift_in, bias):
    """(table fp32, bias_full fp32) from the load-time kernel, checked against the fp64 host form: one rounding each."""
    torch, hiplib, engine, dev = env["torch"], env["hiplib"], env["engine"], env["dev"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    tap, full = hiplib.fold_shift_taps(t(w), t(shift_in), t(bias))
    tap, full = tap.cpu().numpy(), full.cpu().numpy()
    taps64 = engine.shift_tap_table(w, shift_in)
    full64 = bias.astype(np.float64) + taps64.sum(axis=0)
    assert (tap == taps64.astype(np.float32)).all() and (full == full64.astype(np.float32)).all()
    return tap, full, taps64, full64


# every form into split8 rows; the 128 / 256-row kernel also into fp32 rows (its general store path; the 256 x 256 tiles write
# split formats only)
EXACT = [f + ("split8",) for f in FORMS] + [f + ("f32",) for f in FORMS if f[1] < 512]


@pytest.mark.parametrize("name,tile,cin,cout,K,dil,fmt", EXACT, ids=["%s -> %s" % (f[0], f[-1]) for f in EXACT])
def test_exact_fold_equals_shifted_input(env, name, tile, cin, cout, K, dil, fmt):
    lay = env["lay"]
    rng = np.random.default_rng(K * 100 + cin + tile)
    mats, w, shift_in, bias, scale, shift_out = _exact_data(rng, K, cin, cout)
    tap, full, taps64, full64 = _fold(env, w, shift_in, bias)
    assert (tap == taps64).all() and (full == full64).all()             # exact on this data
    u = lay.pack(mats)
    y_in = (u + shift_in[None, :]) * lay.row_valid()[:, None]            # what the unfolded producer stores
    assert np.abs(y_in).max() < 16 and (y_in * 2 == np.round(y_in * 2)).all()
    # every partial sum is a multiple of 1/2 far below 2^24: exact in fp32 in any order
    assert (np.abs(w).sum(axis=(0, 1)).max() * 16 + np.abs(full).max() + np.abs(tap).sum(0).max()) < 2 ** 20
    plain, plain_raw = _run(env, tile, y_in, w, bias, scale, shift_out, None, dil, fmt)
    fold, fold_raw = _run(env, tile, u, w, full, scale, shift_out, tap, dil, fmt)
    valid = lay.row_valid().astype(bool)
    assert np.isfinite(plain).all() and np.isfinite(fold).all()
    assert (plain[~valid] == 0).all() and (fold[~valid] == 0).all()
    assert (plain[valid] != 0).any()
    bad = np.argwhere(plain != fold)
    assert len(bad) == 0, (name, bad[:8].tolist())
    assert plain_raw == fold_raw
    # and the answer is the right one (fp64 oracle of the folded form)
    z = _conv_rows(u, w, dil) + env["engine"].folded_row_bias(bias, taps64, lay.row_valid(), dil)
    want = (np.maximum(z, 0) * scale + shift_out) * valid[:, None]
    assert (fold == want).all()
    # (c) position independence
    a, b = (slice(STARTS[i], STARTS[i] + LENS[i]) for i in TWIN)
    assert (fold[a] == fold[b]).all()


def _conv_rows(x, w, dil):
    K = w.shape[0]
    halo = (K - 1) // 2 * dil
    xp = np.concatenate([np.zeros((halo, x.shape[1])), x.astype(np.float64), np.zeros((halo, x.shape[1]))])
    return sum(xp[t * dil: t * dil + x.shape[0]] @ w[t].astype(np.float64) for t in range(K))


@pytest.mark.parametrize("name,tile,cin,cout,K,dil", FORMS, ids=[f[0] for f in FORMS])
def test_random_data_within_elementwise_bound(env, name, tile, cin, cout, K, dil):
    lay, engine = env["lay"], env["engine"]
    rng = np.random.default_rng(K * 7 + cin + tile)
    mats = [np.maximum(rng.standard_normal((n, cin)) * 1.5, 0).astype(np.float32) for n in LENS]
    mats[TWIN[1]] = mats[TWIN[0]].copy()
    w = (rng.standard_normal((K, cin, cout)) / np.sqrt(K * cin)).astype(np.float32)
    shift_in = (0.7 * rng.standard_normal(cin)).astype(np.float32)
    bias = (0.1 * rng.standard_normal(cout)).astype(np.float32)
    scale = np.exp(0.2 * rng.standard_normal(cout)).astype(np.float32)
    tap, full, taps64, full64 = _fold(env, w, shift_in, bias)
    fmt = "split8"
    got, _ = _run(env, tile, lay.pack(mats), w, full, scale, None, tap, dil, fmt)
    valid = lay.row_valid()
    rowbias = engine.folded_row_bias(bias, taps64, valid, dil)
    # the kernel forms (acc - c_t ...) + bias_full from fp32 constants: K more roundings on the chain, at magnitudes up to
    # |bias_full| + sum |c_t|, which also carry the constants' own rounding (<= u each)
    cmag = np.abs(full64) + np.abs(taps64).sum(axis=0)
    A = em.accum_factor(em.depth("f16bf8", K, cin) + K + 1)
    worst = 0.0
    for s, n, m in zip(STARTS, LENS, mats):
        z, M = em.contract("f16bf8", m, w, dil)
        zb = z + rowbias[s:s + n]
        ref = em.epilogue(zb, None, scale, None, "relu", None)
        bnd = em.elementwise_bound(A, M + cmag[None, :], zb, ref, scale, None, fmt)
        ratio = np.abs(got[s:s + n].astype(np.float64) - ref) / bnd
        worst = max(worst, float(ratio.max()))
        assert (ratio <= 1).all(), (name, s, np.unravel_index(np.argmax(ratio), ratio.shape), float(ratio.max()))
    print("%s: worst |y - y_ref| / bound = %.3e (A = %.1f)" % (name, worst, A))
    assert (got[~valid.astype(bool)] == 0).all()
    a, b = (slice(STARTS[i], STARTS[i] + LENS[i]) for i in TWIN)
    assert (got[a] == got[b]).all()                                       # (c)


def test_pool_entry_with_table(env):
    """xv_tdnn_layer_pool_f16bf8 at Cout = 256, K = 5 (the 16 x 16 form's POOL epilogue) and on the 128-row kernel's."""
    from pair_data import _check_blocks
    lay = env["lay"]
    for tile, cin, cout, K, dil in ((1024, 64, 256, 5, 1), (128, 32, 128, 5, 1), (1024, 64, 256, 3, 2)):
        rng = np.random.default_rng(tile + dil)
        mats, w, shift_in, bias, scale, shift_out = _exact_data(rng, K, cin, cout)
        scale = np.where(scale == 0.5, 1.0, scale).astype(np.float32)
        tap, full, taps64, _ = _fold(env, w, shift_in, bias)
        u = lay.pack(mats)
        y_in = (u + shift_in[None, :]) * lay.row_valid()[:, None]
        plain, plain_raw = _run(env, tile, y_in, w, bias, scale, shift_out, None, dil, pool=True)
        fold, fold_raw = _run(env, tile, u, w, full, scale, shift_out, tap, dil, pool=True)
        assert np.isfinite(fold).all() and fold_raw == plain_raw
        z = _conv_rows(u, w, dil) + env["engine"].folded_row_bias(bias, taps64, lay.row_valid(), dil)
        want = np.maximum(z, 0) * scale + shift_out
        _check_blocks(fold, lay, want, cout, "pool8 with a table, tile %d, K %d, dilation %d" % (tile, K, dil))


def test_k1_layer_refuses_a_table(env):
    torch, hiplib, dev = env["torch"], env["hiplib"], env["dev"]
    cin, cout = 32, 128
    w = torch.zeros((1, cin, cout), device=dev)
    wp = hiplib.pack_weights_f16bf8(w)
    x = hiplib.SplitBuf(R, cin, dev, hiplib.FMT_SPLIT8)
    y = hiplib.SplitBuf(R, cout, dev, hiplib.FMT_SPLIT8)
    table = torch.zeros((1, cout), device=dev)
    bias = torch.zeros(cout, device=dev)
    with pytest.raises(hiplib.XvectorHipError, match="tap_bias"):
        hiplib.tdnn_layer8(x, R, wp, bias, None, None, 1, None, 1, None, y, None, tapbias=table)
    blk = torch.zeros(hiplib.block_stats_floats(R, cout), device=dev)
    with pytest.raises(hiplib.XvectorHipError, match="tap_bias"):
        hiplib.tdnn_layer_pool8(x, R, wp, bias, None, None, 1, None, 1, None, blk, tapbias=table)
    hiplib.tdnn_layer8(x, R, wp, bias, None, None, 1, None, 1, None, y, None)            # and takes the call without one
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------
# the whole network
# ---------------------------------------------------------------------------------------------------------------------------
UTT_FRAMES = (25, 40, 61)


@pytest.fixture(scope="module")
def net(env, oracle_mod):
    from xvector_amd import synthetic, topology
    engine, hiplib, torch = env["engine"], env["hiplib"], env["torch"]
    topo = topology.get("ModelWithoutDropout")
    w = synthetic.trained_like(topo, 23, seed=1)
    mats = synthetic.mfcc_like(list(UTT_FRAMES), feat_dim=23, seed=3)
    refs = [oracle_mod.embed_utterance(m, w, topo, 25, 200, np.float64) for m in mats]
    out = {}
    for fold in (True, False):
        model = engine.DeviceModel(w, topo, "cuda:0", precision="f16bf8", fold_shift=fold)
        assert model.f16bf8 and model.fold_shift == fold
        stored = []
        real_first, real_layer8 = hiplib.tdnn_first, hiplib.tdnn_layer8

        def first(x, R_, wt, b, sc, sh, act, al, dil, rv, y, status=None):
            real_first(x, R_, wt, b, sc, sh, act, al, dil, rv, y, status)
            stored.append((hiplib.split_decode(y, R_).cpu().numpy(), rv.cpu().numpy().astype(bool)))

        def layer8(x, R_, wt, b, sc, sh, act, al, dil, rv, y, status=None, tapbias=None):
            real_layer8(x, R_, wt, b, sc, sh, act, al, dil, rv, y, status, tapbias=tapbias)
            stored.append((hiplib.split_decode(y, R_).cpu().numpy(), rv.cpu().numpy().astype(bool)))
        hiplib.tdnn_first, hiplib.tdnn_layer8 = first, layer8
        try:
            ex = engine.Extractor(model, 25, 200, accuracy_probe=False)
            vecs = ex.extract(mats)
        finally:
            hiplib.tdnn_first, hiplib.tdnn_layer8 = real_first, real_layer8
        assert not ex.demoted
        sel = engine.select_model(w, topo, "cuda:0", precision="f16bf8", fold_shift=fold).selection
        out[fold] = dict(stored=stored, err=max(oracle_mod.rel_l2(v, r) for v, r in zip(vecs, refs)), sel=sel, vecs=vecs)
    return out


def test_network_stores_relu_zeros(net):
    """Layers 0, 1 and 2 store scale * relu(.) with the fold: the CPU forward of this checkpoint gives 0.47-0.49 exact zeros."""
    for fold in (True, False):
        stored = net[fold]["stored"]
        assert len(stored) == 3, "expected the launches of layers 0, 1 and 2"
        for i, (y, valid) in enumerate(stored):
            frac = float((y[valid] == 0).mean())
            print("fold_shift=%s layer %d: %.4f of the stored activations of valid rows are exact zeros" % (fold, i, frac))
            assert (y[~valid] == 0).all()
            if fold:
                assert frac >= 0.40
            else:
                assert frac == 0.0


def test_network_accuracy_folded_and_unfolded(net, env):
    engine = env["engine"]
    for fold in (True, False):
        r = net[fold]
        print("fold_shift=%s: x-vector rel-L2 vs fp64 oracle %.3e, load-time probe f16bf8_vs_bf16x3 %.3e" % (
            fold, r["err"], r["sel"]["f16bf8_vs_bf16x3"]))
    print("ratio folded / unfolded: oracle %.3f, probe %.3f" % (net[True]["err"] / net[False]["err"],
                                                                net[True]["sel"]["f16bf8_vs_bf16x3"] / net[False]["sel"]["f16bf8_vs_bf16x3"]))
    assert net[True]["err"] < 1e-4 and net[False]["err"] < 1e-4
    assert net[True]["sel"]["selected"] == "f16bf8" and net[True]["sel"]["f16bf8_vs_bf16x3"] < engine.PROBE_LIMIT_F16BF8


def test_lrelu_model_keeps_the_unfolded_path(env):
    from xvector_amd import synthetic, topology
    engine = env["engine"]
    topo = topology.get("ModelL2LossWithoutDropoutLRelu")
    w = synthetic.trained_like(topo, 23, seed=1)
    mats = synthetic.mfcc_like(list(UTT_FRAMES), feat_dim=23, seed=3)
    vecs = {}
    for fold in (None, False):
        model = engine.DeviceModel(w, topo, "cuda:0", precision="f16bf8", fold_shift=fold)
        assert model.f16bf8 and not model.fold_shift and all("tapbias" not in L and "fbias" not in L for L in model.layers)
        vecs[fold] = np.stack(engine.Extractor(model, 25, 200, accuracy_probe=False).extract(mats))
    assert vecs[None].tobytes() == vecs[False].tobytes()
    with pytest.raises(AssertionError):
        engine.DeviceModel(w, topo, "cuda:0", precision="f16bf8", fold_shift=True)


def test_width_not_a_multiple_of_8_keeps_the_unfolded_path(env, oracle_mod):
    """The epilogues read a tap's constants 8 channels at a time, the f16bf8 kernels take any width: a model with a K > 1 layer
    (behind layer 0) of width 100 loads with the default ``fold_shift`` as it did before the fold existed -- unfolded -- and runs."""
    from xvector_amd import synthetic, topology
    engine = env["engine"]
    topo = dict(topology.get("ModelWithoutDropout"), layer_sizes=[64, 100, 64, 64, 96])
    assert topo["kernel_sizes"][1] > 1
    w = synthetic.trained_like(topo, 23, seed=5)
    mats = synthetic.mfcc_like(list(UTT_FRAMES), feat_dim=23, seed=3)
    engine.select_model(w, topo, "cuda:0", precision="f16bf8")              # (the load-time probe runs a forward: it must not raise)
    model = engine.DeviceModel(w, topo, "cuda:0", precision="f16bf8")
    assert model.f16bf8 and not model.fold_shift
    vecs = engine.Extractor(model, 25, 200, accuracy_probe=False).extract(mats)
    refs = [oracle_mod.embed_utterance(m, w, topo, 25, 200, np.float64) for m in mats]
    assert max(oracle_mod.rel_l2(v, r) for v, r in zip(vecs, refs)) < 1e-4
    with pytest.raises(AssertionError):
        engine.DeviceModel(w, topo, "cuda:0", precision="f16bf8", fold_shift=True)
    # the same network 104 wide takes the fold
    topo8 = dict(topo, layer_sizes=[64, 104, 64, 64, 96])
    assert engine.DeviceModel(synthetic.trained_like(topo8, 23, seed=5), topo8, "cuda:0", precision="f16bf8").fold_shift


def test_select_model_tries_unfolded_before_demoting(net, env, monkeypatch):
    """A checkpoint whose folded probe misses the limit that its unfolded probe meets keeps the unfolded f16bf8 arithmetic (the
    limit is moved between the two measured errors for the test; the fold's error is the larger one on this checkpoint)."""
    from xvector_amd import synthetic, topology
    engine = env["engine"]
    folded, plain = net[True]["sel"]["f16bf8_vs_bf16x3"], net[False]["sel"]["f16bf8_vs_bf16x3"]
    if not folded > plain:
        pytest.fail("the folded probe (%.3e) is not above the unfolded one (%.3e): DESIGN 9.7 no longer describes this tree" % (folded, plain))
    monkeypatch.setattr(engine, "PROBE_LIMIT_F16BF8", 0.5 * (folded + plain))
    topo = topology.get("ModelWithoutDropout")
    w = synthetic.trained_like(topo, 23, seed=1)
    model = engine.select_model(w, topo, "cuda:0", precision="f16bf8")
    sel = model.selection
    assert sel["selected"] == "f16bf8" and model.f16bf8 and not model.fold_shift and sel["fold_shift"] is False
    assert sel["f16bf8_vs_bf16x3"] == plain and sel["folded_f16bf8_vs_bf16x3"] == folded
