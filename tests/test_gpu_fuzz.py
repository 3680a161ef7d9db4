"""Randomised parity sweep (fixed seeds): random layer widths / kernel sizes / dilations / activations / pooling kind /
feature dims / utterance lengths / chunking / batch sizes through DeviceModel + Extractor, every precision, against the fp64
oracle.  Widths are multiples of 4 (the pooling and FC kernels require 16-byte rows and say so loudly otherwise)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_topologies_match_the_oracle(oracle_mod, seed):
    from xvector_amd import engine, hiplib, synthetic
    hiplib.require_gpu()
    rng = np.random.default_rng(seed)
    worst = {"fp32": 0.0, "bf16x3": 0.0}
    for case in range(14):
        step = int(rng.choice([4, 8, 32]))
        width = lambda lo, hi: max(step, int(rng.integers(lo, hi)) // step * step)      # noqa: E731
        attention = rng.random() < 0.3
        ks = [int(rng.choice([1, 3, 5, 7])) for _ in range(5)]
        ds = [int(rng.choice([1, 1, 2, 3])) if k > 1 else 1 for k in ks]
        ds = [d if (k - 1) * d <= 8 else 1 for k, d in zip(ks, ds)]
        last = width(8, 260)
        topo = dict(layer_sizes=[width(8, 200), width(8, 200), width(8, 200), width(8, 200), max(8, last // 8 * 8) if attention else last],
                    kernel_sizes=ks, dilations=ds, embedding_sizes=[width(4, 70), width(4, 70)],
                    activation=str(rng.choice(["relu", "lrelu", "prelu"])), lrelu_alpha=0.2, pooling="attention" if attention else "stats")
        F = int(rng.choice([23, 24, 30, 13, 40]))
        w = synthetic.trained_like(topo, F, 8, seed=int(rng.integers(1 << 30)))
        lens = [int(x) for x in rng.integers(1, 700, size=int(rng.integers(1, 9)))]
        mn, cs = int(rng.choice([1, 10, 25])), int(rng.choice([-1, 100, 333]))
        mats = [(rng.standard_normal((t, F)) * 3).astype(np.float32) for t in lens]
        refs = [oracle_mod.embed_utterance(m, w, topo, mn, cs, np.float64) for m in mats]
        for prec in ("fp32", "bf16x3"):
            model = engine.DeviceModel(w, topo, "cuda:0", precision=prec)
            got = engine.Extractor(model, mn, cs, max_batch_rows=int(rng.choice([64, 700, 262144]))).extract(mats)
            for g, r in zip(got, refs):
                assert (g is None) == (r is None), (case, prec, topo, lens, mn, cs)
                if g is not None:
                    worst[prec] = max(worst[prec], oracle_mod.rel_l2(g, r))
    # the north-star bar is 1e-4; exact-fp32 sits two orders below it on every topology
    assert worst["fp32"] < 1e-5 and worst["bf16x3"] < 1e-4, worst


@pytest.mark.parametrize("seed", [21, 22])
def test_random_topologies_through_the_first_layer_and_pair_kernels(oracle_mod, seed):
    """Random topologies of the shape the specialised kernels take -- layer 0 with K*ceil8(F) <= 128 and a width that is a
    multiple of 32; last two layers K = 1 around a 512-wide intermediate -- through DeviceModel + Extractor (bf16x3) against
    the fp64 oracle, with the kernels asserted to be the ones that ran; the same model with both switched off must agree to
    fp32 summation order."""
    from xvector_amd import engine, hiplib, synthetic
    hiplib.require_gpu()
    rng = np.random.default_rng(seed)
    worst = 0.0
    for case in range(6):
        F = int(rng.choice([23, 13, 24, 8]))
        k0 = int(rng.choice([3, 5])) if F > 16 else int(rng.choice([3, 5, 7]))
        ks = [k0, int(rng.choice([1, 3, 5])), int(rng.choice([3, 5, 7])), 1, 1]
        ds = [int(rng.choice([1, 2])) if k == 3 else 1 for k in ks]
        topo = dict(layer_sizes=[int(rng.choice([32, 64, 160, 512])), int(rng.choice([32, 96])), int(rng.choice([32, 64, 160])), 512,
                                 int(rng.choice([64, 192, 320, 1536]))],
                    kernel_sizes=ks, dilations=ds, embedding_sizes=[int(rng.choice([16, 40])), 16],
                    activation=str(rng.choice(["relu", "lrelu", "prelu"])), lrelu_alpha=0.2, pooling="stats")
        w = synthetic.trained_like(topo, F, 8, seed=int(rng.integers(1 << 30)))
        lens = [int(x) for x in rng.integers(1, 900, size=int(rng.integers(2, 10)))]
        mn, cs = int(rng.choice([1, 25])), int(rng.choice([-1, 200]))
        mats = [(rng.standard_normal((t, F)) * 3).astype(np.float32) for t in lens]
        refs = [oracle_mod.embed_utterance(m, w, topo, mn, cs, np.float64) for m in mats]
        model = engine.DeviceModel(w, topo, "cuda:0")
        assert model.pair is not None and model.first is not None, topo
        got = engine.Extractor(model, mn, cs, max_batch_rows=int(rng.choice([700, 262144]))).extract(mats)
        plain = engine.DeviceModel(w, topo, "cuda:0", pair_kernel=False, first_kernel=False)
        assert plain.pair is None and plain.first is None
        base = engine.Extractor(plain, mn, cs).extract(mats)
        for g, b, r in zip(got, base, refs):
            assert (g is None) == (r is None) == (b is None), (case, topo, lens, mn, cs)
            if g is not None:
                worst = max(worst, oracle_mod.rel_l2(g, r))
                assert oracle_mod.rel_l2(g, b) < 2e-5, (case, topo)
    assert worst < 1e-4, worst


@pytest.mark.parametrize("seed", [31, 32, 33])
def test_random_topologies_in_the_f16bf8_arithmetic(oracle_mod, seed):
    """Random topologies the f16bf8 path covers -- layer 0 of a shape the first-layer kernel takes, hidden layers with K in
    {1,3,5,7} and any width (ragged last slabs, column tiles that are not full), with and without the 512-wide K = 1 pair at the
    end -- through DeviceModel(precision="f16bf8") + Extractor against the fp64 oracle, the kernels asserted to be the ones
    that ran.  The bar is the north star's 1e-4; the arithmetic sits at 1-3e-5."""
    from xvector_amd import engine, hiplib, synthetic
    hiplib.require_gpu()
    rng = np.random.default_rng(seed)
    worst = 0.0
    for case in range(8):
        F = int(rng.choice([23, 13, 24, 8]))
        k0 = int(rng.choice([3, 5])) if F > 16 else int(rng.choice([3, 5, 7]))
        paired = rng.random() < 0.5
        n_hidden = int(rng.integers(1, 4))                                  # f16bf8 GEMM layers between layer 0 and the tail
        ks = [k0] + [int(rng.choice([1, 3, 5, 7])) for _ in range(n_hidden)] + ([1, 1] if paired else [int(rng.choice([1, 3]))])
        ds = [1] + [int(rng.choice([1, 2])) if k == 3 else 1 for k in ks[1:]]
        widths = [int(rng.choice([32, 64, 160, 512]))] + [int(rng.choice([32, 40, 96, 200, 256, 512])) for _ in range(n_hidden)]
        widths += [512, int(rng.choice([64, 192, 1536]))] if paired else [int(rng.choice([48, 256, 520]))]
        topo = dict(layer_sizes=widths, kernel_sizes=ks, dilations=ds, embedding_sizes=[int(rng.choice([16, 40])), 16],
                    activation=str(rng.choice(["relu", "lrelu", "prelu"])), lrelu_alpha=0.2, pooling="stats")
        w = synthetic.trained_like(topo, F, 8, seed=int(rng.integers(1 << 30)))
        lens = [int(x) for x in rng.integers(1, 900, size=int(rng.integers(2, 10)))]
        mn, cs = int(rng.choice([1, 25])), int(rng.choice([-1, 200]))
        mats = [(rng.standard_normal((t, F)) * 3).astype(np.float32) for t in lens]
        refs = [oracle_mod.embed_utterance(m, w, topo, mn, cs, np.float64) for m in mats]
        model = engine.DeviceModel(w, topo, "cuda:0", precision="f16bf8")
        # (the pair kernels take two K = 1 layers around a 512-wide intermediate with Cin % 32 == 0 and Cout % 64 == 0 -- a shape
        # the random draw can also hit without asking for it)
        expect_pair = ks[-1] == 1 and ks[-2] == 1 and widths[-2] == 512 and widths[-3] % 32 == 0 and widths[-1] % 64 == 0
        assert model.f16bf8 and (model.pair8 is not None) == expect_pair, topo
        # (the run-time accuracy probe is off: this test is about what the f16bf8 kernels themselves deliver -- on these narrow
        # random networks the probe's 3e-5 limit would move some of them to bf16x3, which is its job)
        ex = engine.Extractor(model, mn, cs, max_batch_rows=int(rng.choice([700, 262144])), accuracy_probe=False)
        got = ex.extract(mats)
        assert ex.stats.get("fallback_windows", 0) == 0
        for g, r in zip(got, refs):
            assert (g is None) == (r is None), (case, topo, lens, mn, cs)
            if g is not None:
                assert np.isfinite(g).all()
                worst = max(worst, oracle_mod.rel_l2(g, r))
    assert worst < 1e-4, worst


@pytest.mark.parametrize("seed", [11, 12])
def test_random_topologies_gradients_match_autograd(seed):
    """The training step (fp32 kernels) on random topologies -- widths, kernel sizes, dilations, activation, pooling kind,
    L2 term, dropout-free -- against the float64 autograd oracle: loss 1e-5, every gradient tensor 5e-4 relative L2 (relative to
    its own norm, or to a tenth of the median tensor norm where a gradient is zero by construction -- a shift in front of a batch
    normalisation -- and float32 leaves 1e-5 of the terms that cancel).  A failure message carries the oracle's kink margin: a pre-activation within float32 rounding (~1e-6 rms) of
    the activation's kink may fall on the other side of it on the GPU, which moves every gradient below it by 1 / sqrt(elements)
    (oracle/train_ref.py: kink_margin; tools/fuzz_many.py reports such cases apart)."""
    from oracle import train_ref
    from xvector_amd import hiplib, synthetic, trainer
    hiplib.require_gpu()
    rng = np.random.default_rng(seed)
    for case in range(5):
        width = lambda lo, hi: int(rng.integers(lo, hi)) // 4 * 4                        # noqa: E731
        attention = rng.random() < 0.4
        ks = [int(rng.choice([1, 3, 5, 7])) for _ in range(5)]
        ds = [int(rng.choice([1, 2])) if 1 < k < 7 else 1 for k in ks]
        topo = dict(layer_sizes=[width(16, 100), width(16, 100), width(16, 100), width(16, 100), width(16, 120) // 8 * 8],
                    kernel_sizes=ks, dilations=ds, embedding_sizes=[width(8, 48), width(8, 48)],
                    activation=str(rng.choice(["relu", "lrelu", "prelu"])), lrelu_alpha=0.2, l2_beta=float(rng.choice([0.0, 0.0002])),
                    dropout=False, head=None, pooling="attention" if attention else "stats")
        F, classes, B, T = int(rng.choice([23, 24, 13])), 7, int(rng.integers(3, 9)), int(rng.integers(40, 230))
        w = synthetic.trained_like(topo, F, classes, seed=int(rng.integers(1 << 30)))
        x = (rng.standard_normal((B, T, F)) * 3).astype(np.float32)
        lab = rng.integers(0, classes, B)
        loss, acc, grads = trainer.Trainer(w, topo).gradients(x, lab)
        rl, ra, _, _, rg = train_ref.train_step(w, {"t": 0, "m": {}, "v": {}}, topo, x, lab, 1e-3)
        assert abs(loss - rl) < 1e-5 * max(1.0, abs(rl)), (case, topo)
        bad = {}
        floor = 0.1 * float(np.median([np.linalg.norm(ref) for ref in rg.values()]))
        for n, ref in rg.items():
            e = float(np.linalg.norm(grads[n].cpu().numpy().astype(np.float64) - ref) / max(np.linalg.norm(ref), floor))
            if e > 5e-4:
                bad[n] = e
        assert not bad, ("kink margin %.1e" % train_ref.kink_margin[0], case, topo, bad)


@pytest.mark.parametrize("seed", [21, 22])
def test_random_topologies_bf16x3_step_with_reductions_from_their_producers(seed, monkeypatch):
    """The bf16x3 training step with its BN reductions taken from the GEMM epilogues / the pooling gradient's per-chunk form (default)
    against the same step with the separate passes (XVECTOR_TRAIN_FUSED_SUMS=0), on random topologies whose widths let the fused forms
    apply (multiples of 8; ragged last row tiles, dilations, K = 1 layers on split copies, leaky ReLU, both poolings): loss to 1e-4
    (the bound test_bf16x3_training_gradients puts on the arithmetic itself), every gradient tensor to 1e-1 of its norm (or of a tenth of the median norm).  That bound is the conditioning of these small
    random problems, not of the reductions: over 360 soaked cases (tools/fuzz_many.py) both forms sit 1e-2 ... 6e-2 from float64
    autograd in their worst tensor (fp32: 1e-5) and up to 6e-2 from each other (either one may be the farther), 2-6e-5 from its loss -- batch moments that differ in the last bit move a
    pre-activation across the activation's kink (margins of 5e-7) as readily as the split products do.  The reductions themselves are
    pinned to 1e-6 / 2e-6 by the kernel-level tests of tests/test_gpu_training.py; a wrong sum here would be an O(1) error."""
    from xvector_amd import hiplib, synthetic, trainer
    hiplib.require_gpu()
    rng = np.random.default_rng(seed)
    for case in range(4):
        width = lambda lo, hi: int(rng.integers(lo, hi)) // 8 * 8                        # noqa: E731
        ks = [int(rng.choice([1, 3, 5, 7])) for _ in range(5)]
        ds = [int(rng.choice([1, 2])) if 1 < k < 7 else 1 for k in ks]
        topo = dict(layer_sizes=[width(16, 140), width(32, 140), width(32, 140), width(16, 140), width(16, 200)],
                    kernel_sizes=ks, dilations=ds, embedding_sizes=[width(8, 48), width(8, 48)],
                    activation=str(rng.choice(["relu", "lrelu"])), lrelu_alpha=0.2, l2_beta=0.0,
                    dropout=False, head=None, pooling="attention" if rng.random() < 0.3 else "stats")
        F, classes, B, T = int(rng.choice([23, 24])), 7, int(rng.integers(3, 12)), int(rng.integers(40, 330))
        w = synthetic.trained_like(topo, F, classes, seed=int(rng.integers(1 << 30)))
        x = (rng.standard_normal((B, T, F)) * 3).astype(np.float32)
        lab = rng.integers(0, classes, B)
        res = []
        for flag in ("1", "0"):
            monkeypatch.setenv("XVECTOR_TRAIN_FUSED_SUMS", flag)
            loss, acc, grads = trainer.Trainer(w, topo, precision="bf16x3").gradients(x, lab)
            res.append((loss, {n: g.cpu().numpy().astype(np.float64) for n, g in grads.items()}))
        assert abs(res[0][0] - res[1][0]) <= 1e-4 * max(1.0, abs(res[1][0])), (case, topo)
        floor = 0.1 * float(np.median([np.linalg.norm(v) for v in res[1][1].values()]))
        bad = {n: e for n, e in ((n, float(np.linalg.norm(res[0][1][n] - v) / max(np.linalg.norm(v), floor))) for n, v in res[1][1].items()) if e > 1e-1}
        assert not bad, (case, topo, bad)


@pytest.mark.parametrize("seed", [61, 62, 63])
def test_random_shapes_through_the_16x16_f16bf8_kernel(oracle_mod, seed):
    """The 256 x 256 f16bf8 tile on the 16 x 16 MFMA shapes (round 4) at kernel level: random K in {3, 5, 7}, dilations up to a span
    of 8, an even number of 32-channel slabs, Cout in {256, 512, 768}, every activation, split8 / bf16-split / pooled output, ragged
    utterance lengths with gap rows -- against the fp64 oracle, gap rows exactly zero, an utterance alone == in the batch bitwise."""
    import torch
    from xvector_amd import engine, hiplib
    hiplib.require_gpu()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(seed)
    CODE = {"none": 0, "relu": 1, "lrelu": 2, "prelu": 3}
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    for case in range(5):
        K = int(rng.choice([3, 5, 7]))
        dil = int(rng.integers(1, 8 // (K - 1) + 1))
        cin = 64 * int(rng.integers(1, 9))
        cout = int(rng.choice([256, 512, 768]))
        act = str(rng.choice(["none", "relu", "lrelu", "prelu"]))
        mode = str(rng.choice(["split8", "split", "pool"]))
        lens = [int(x) for x in rng.integers(1, 600, size=int(rng.integers(1, 7)))]
        mats = [(rng.standard_normal((n, cin)) * 2).astype(np.float32) for n in lens]
        w = (rng.standard_normal((K, cin, cout)) / np.sqrt(K * cin)).astype(np.float32)
        b = (0.1 * rng.standard_normal(cout)).astype(np.float32)
        bn = ((1 + 0.1 * rng.standard_normal(cout)).astype(np.float32), (0.1 * rng.standard_normal(cout)).astype(np.float32),
              (0.2 * rng.standard_normal(cout)).astype(np.float32), np.exp(0.2 * rng.standard_normal(cout)).astype(np.float32))
        alpha = np.array([0.2], np.float32) if act == "lrelu" else (0.1 + 0.05 * rng.standard_normal(cout)).astype(np.float32) if act == "prelu" else None
        scale, shift = hiplib.fold_bn(*(t(a) for a in bn), 1e-3)
        wp = hiplib.pack_weights_f16bf8(t(w))
        gap = max(1, (K - 1) * dil // 2)

        def run(ms):
            layout = engine.BatchLayout([m.shape[0] for m in ms], gap, hiplib.POOL_BLOCK_ROWS if mode == "pool" else 1)
            host = np.zeros((layout.rows, cin), np.float32)
            layout.pack(ms, host)
            xin = hiplib.SplitBuf(layout.rows, cin, dev, hiplib.FMT_SPLIT8)
            hiplib.split_encode(t(host), xin)
            rv = t(layout.row_valid())
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            if mode == "pool":
                blk = torch.full((hiplib.block_stats_floats(layout.rows, cout),), float("nan"), dtype=torch.float32, device=dev)
                hiplib.tdnn_layer_pool8(xin, layout.rows, wp, t(b), scale, shift, CODE[act], t(alpha), dil, rv, blk)
                out = torch.full((len(ms), 2 * cout), float("nan"), dtype=torch.float32, device=dev)
                hiplib.stats_pool_blocks(blk, cout, t(layout.row_start), t(layout.row_len), len(ms), 1e-5, out)
                return out.cpu().numpy(), None, layout
            y = hiplib.SplitBuf(layout.rows, cout, dev, hiplib.FMT_SPLIT8 if mode == "split8" else hiplib.FMT_SPLIT)
            y.base.fill_(0x7b)
            hiplib.tdnn_layer8(xin, layout.rows, wp, t(b), scale, shift, CODE[act], t(alpha), dil, rv, y, status)
            assert int(status.item()) == 0
            yh = hiplib.split_decode(y, layout.rows).cpu().numpy()
            return [yh[s0:s0 + n] for s0, n in zip(layout.row_start, layout.row_len)], yh, layout

        hiplib.set_tuning(hiplib.TUNE_TILE_ROWS, 1024)
        try:
            outs, yh, layout = run(mats)
            alone, _, _ = run([mats[-1]])
        finally:
            hiplib.set_tuning(hiplib.TUNE_TILE_ROWS, 0)
        tag = (seed, case, K, dil, cin, cout, act, mode, lens)
        for i, m in enumerate(mats):
            ref = oracle_mod.tdnn_layer(m, w, b, bn, act, alpha, dil, np.float64)
            if mode == "pool":
                ref = oracle_mod.stats_pool(ref, 1e-5, np.float64)
                assert oracle_mod.rel_l2(outs[i][:cout], ref[:cout]) < 4e-5 and oracle_mod.rel_l2(outs[i][cout:], ref[cout:]) < 4e-5, tag
            else:
                assert np.isfinite(outs[i]).all() and oracle_mod.rel_l2(outs[i], ref) < 4e-5, (tag, oracle_mod.rel_l2(outs[i], ref))
        if mode == "pool":
            assert np.array_equal(alone[0], outs[-1]), tag
        else:
            assert (yh[~layout.row_valid().astype(bool)] == 0).all(), tag
            assert np.array_equal(alone[0], outs[-1]), tag


@pytest.mark.parametrize("seed", [71, 72])
def test_random_shapes_through_the_dma_fed_fp32_gemm(oracle_mod, seed):
    """The exact-fp32 GEMM fed by LDS-DMA (round 4) against its register-staged form: random K, dilation, Cin a multiple of 32, ragged
    Cout, row counts that are no multiple of anything, random gap rows -- the forms (incl. the K = 1 kernel on 16-channel slabs, rows and
    pooling epilogues) agree BIT FOR BIT (XV_TUNE_FP32_GEMM), rows past
    the end and columns past Cout come back as zeros from the descriptors' range check; a sample of rows against the fp64 oracle."""
    import torch
    from xvector_amd import hiplib
    hiplib.require_gpu()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(seed)
    for case in range(4):
        K = 1 if case == 0 else int(rng.choice([1, 3, 5, 7]))       # (K = 1 has a form of its own: 16-channel slabs, XV_TUNE_FP32_GEMM 3)
        dil = 1 if K == 1 else int(rng.integers(1, 8 // (K - 1) + 1))
        cin = 32 * int(rng.integers(1, 9))
        cout = int(rng.choice([128, 200, 512, 516, 640]))
        n_nt = (cout + 127) // 128
        R = int(rng.integers(768 // n_nt * 128 + 1, 768 // n_nt * 128 + 4000))           # just above the size where 128-row tiles are chosen
        act = int(rng.integers(0, 4))
        x = (torch.randn((R, cin), device=dev) * 2)
        valid = (torch.rand(R, device=dev) > 0.03).to(torch.uint8)
        x *= valid[:, None].float()
        w = torch.randn((K * cin, cout), device=dev) / (K * cin) ** 0.5
        wp = hiplib.pack_weights(w)
        bias = torch.randn(cout, device=dev) * 0.1
        scale = 1 + 0.1 * torch.randn(cout, device=dev)
        shift = 0.1 * torch.randn(cout, device=dev)
        alpha = torch.full((1,), 0.2, device=dev) if act == 2 else (0.1 + 0.05 * torch.randn(cout, device=dev)) if act == 3 else None
        outs, pools = [], []
        for form in (1, 2, 3, 0):                       # register-staged, DMA-fed, DMA-fed with K = 1 on 16-channel slabs, built-in choice
            hiplib.set_tuning(hiplib.TUNE_FP32_GEMM, form)
            try:
                y = torch.full((R, cout), float("nan"), device=dev)
                hiplib.tdnn_layer(x, wp, bias, scale, shift, act, alpha, K, dil, valid, y)
                outs.append(y.cpu().numpy())
                if cout % 4 == 0:                       # the same layer with the pooling epilogue (8-row block statistics instead of rows)
                    blk = torch.full((hiplib.block_stats_floats(R, cout),), float("nan"), device=dev)
                    hiplib.tdnn_layer_pool(x, R, wp, bias, scale, shift, act, alpha, dil, valid, blk, K=K)
                    pools.append(blk.cpu().numpy()[:(R + 7) // 8 * 2 * cout])
            finally:
                hiplib.set_tuning(hiplib.TUNE_FP32_GEMM, 0)
        tag = (seed, case, K, dil, cin, cout, R, act)
        assert np.isfinite(outs[1]).all(), tag
        assert all(np.array_equal(outs[0], o) for o in outs[1:]), tag
        assert all(np.array_equal(pools[0], q, equal_nan=True) for q in pools[1:]), tag
        # the first, the last and a few random rows against the fp64 definition (zero rows outside [0, R))
        xh, wh = x.cpu().numpy().astype(np.float64), w.cpu().numpy().astype(np.float64).reshape(K, cin, cout)
        a = None if alpha is None else alpha.cpu().numpy().astype(np.float64)
        for r in [0, 1, R - 1, R - 2] + [int(v) for v in rng.integers(0, R, 6)]:
            z = bias.cpu().numpy().astype(np.float64).copy()
            for k in range(K):
                rr = r + (k - (K - 1) // 2) * dil
                if 0 <= rr < R:
                    z += xh[rr] @ wh[k]
            v = z if act == 0 else np.maximum(z, 0) if act == 1 else np.maximum(a[0] * z, z) if act == 2 else np.maximum(z, 0) + a * np.minimum(z, 0)
            v = v * scale.cpu().numpy() + shift.cpu().numpy()
            if not int(valid[r].item()):
                v = np.zeros_like(v)
            assert np.linalg.norm(outs[1][r] - v) <= 2e-6 * max(np.linalg.norm(v), 1e-3) + 1e-6, (tag, r)


@pytest.mark.parametrize("seed", [41, 42])
def test_random_topologies_in_the_fp32tc_arithmetic(oracle_mod, seed):
    """The Toom-Cook path on shapes it was not tuned for: hidden widths that are multiples of 32 (so the K = 3 / 5 / 7 layers, dilated
    or not, take tdnn_gemm_toom_kernel) next to layers it does not take (K = 1, ragged widths: the direct fp32 kernels),
    first layers in the rows form for every feature dimension, random activations, lengths from 1 frame up, chunking on and off,
    batch budgets from a single tile to one batch -- against the fp64 oracle."""
    import torch  # noqa: F401
    from xvector_amd import engine, hiplib, synthetic
    rng = np.random.default_rng(seed)
    worst, toom_layers = 0.0, 0
    for case in range(6):
        F = int(rng.choice([23, 24, 30, 13, 40]))
        ks = [int(rng.choice([3, 5, 7]))] + [int(rng.choice([1, 3, 5, 7])) for _ in range(3)] + [int(rng.choice([1, 5]))]
        # (the direct kernels -- the last layer's pooling form among them -- take (K - 1) d <= 8)
        ds = [1] + [int(rng.choice([d for d in (1, 1, 2, 3) if (k - 1) * d <= 8])) if k > 1 else 1 for k in ks[1:]]
        widths = [int(rng.choice([32, 64, 96, 160])) for _ in range(4)] + [int(rng.choice([64, 100, 192]))]
        if case == 0:
            widths[1] = 40                                   # a layer whose input is no whole slab: not a Toom-Cook layer
        topo = dict(layer_sizes=widths, kernel_sizes=ks, dilations=ds, embedding_sizes=[int(rng.choice([16, 40])), 16],
                    activation=str(rng.choice(["relu", "lrelu", "prelu"])), lrelu_alpha=0.2, pooling="stats")
        w = synthetic.trained_like(topo, F, 8, seed=int(rng.integers(1 << 30)))
        lens = [int(x) for x in rng.integers(1, 700, size=int(rng.integers(1, 9)))]
        mn, cs = int(rng.choice([1, 10, 25])), int(rng.choice([-1, 100, 333]))
        mats = [(rng.standard_normal((t, F)) * 3).astype(np.float32) for t in lens]
        refs = [oracle_mod.embed_utterance(m, w, topo, mn, cs, np.float64) for m in mats]
        model = engine.DeviceModel(w, topo, "cuda:0", precision="fp32tc")
        in_dims = [model.in_dim] + widths[:-1]
        assert isinstance(model.layers[0]["wp"], hiplib.PackedRows)        # (layer 0, dilation 1: the rows form, whatever K and F)
        for li, (L, k, d, cin, cout) in list(enumerate(zip(model.layers, ks, ds, in_dims, widths)))[1:]:
            # (the last layer feeds the pooling epilogue of the direct kernel: never a Toom-Cook layer)
            want = k in (3, 5, 7) and cin % 32 == 0 and cout % 4 == 0 and li < len(ks) - 1
            assert isinstance(L["wp"], hiplib.PackedToom) == want, (case, k, d, cin, cout)
            toom_layers += want
            if want and d > 1:
                assert model.align % (2 * d) == 0 and model.align % 8 == 0      # chunks on multiples of 2 d rows (and of the pooling block)
        got = engine.Extractor(model, mn, cs, max_batch_rows=int(rng.choice([64, 700, 262144]))).extract(mats)
        for g, r in zip(got, refs):
            assert (g is None) == (r is None), (case, topo, lens, mn, cs)
            if g is not None:
                worst = max(worst, oracle_mod.rel_l2(g, r))
    assert toom_layers >= 4 and worst < 1e-5, (toom_layers, worst)
