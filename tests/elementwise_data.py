"""The cases of tests/test_gpu_elementwise.py (forms, shapes, data, the accumulation factor A), shared with the CPU power check of
tests/test_arith_emul_cpu.py so that both look at the same numbers."""
import numpy as np

import arith_emul as em

LENS = [25, 1, 130, 257, 64, 3, 700]            # chunks shorter than the halo, spanning tile boundaries
LAMBDA = {"fp32": 1.0, "fp32tc": 2.0, "bf16x3": 1.0, "f16bf8": 1.0}
# fp32tc: every product also carries the roundings of its transformed row (<= 6 rows summed) and of its transformed tap: lam 2


class Case(object):
    def __init__(self, name, arith, form, cin, cout, K, dil, act, data, fmt="f32", tune=None, big=False, xfmt="f32", seed=0):
        self.name, self.arith, self.form = name, arith, form
        self.cin, self.cout, self.K, self.dil, self.act, self.kind = cin, cout, K, dil, act, data
        self.fmt, self.tune, self.big, self.xfmt, self.seed = fmt, tune or {}, big, xfmt, seed

    def A(self):
        arith = "fp32" if self.form == "rows" else self.arith
        return em.accum_factor(em.depth(arith, self.K, self.cin), LAMBDA[arith])

    def data(self):
        """(mats, w [K, Cin, Cout], b, scale, shift, alpha) -- fp32, BN passed as its folded scale and shift."""
        from xvector_amd import synthetic
        rng = np.random.default_rng(1000 + self.seed)
        cin, cout, K = self.cin, self.cout, self.K
        if self.kind == "mfcc":
            mats = synthetic.mfcc_like(LENS, feat_dim=cin, seed=self.seed)
        elif self.kind == "relu":                 # post-ReLU activations: non-negative, mean > 0, about half zeros
            mats = [np.maximum(rng.standard_normal((t, cin)) * 1.5, 0).astype(np.float32) for t in LENS]
        else:                                      # hostile: channel scales over three decades, dead channels
            ch = 10.0 ** rng.uniform(-2, 1, cin)
            ch[rng.random(cin) < 0.06] = 0
            mats = [(np.maximum(rng.standard_normal((t, cin)) + 0.3, 0) * ch).astype(np.float32) for t in LENS]
        if self.kind == "hostile":
            w = rng.standard_t(3, (K, cin, cout)) / np.sqrt(3 * K * cin)
            scale = 10.0 ** rng.uniform(-1.5, 1.5, cout)
        else:
            w = rng.standard_normal((K, cin, cout)) / np.sqrt(K * cin)
            scale = np.exp(0.2 * rng.standard_normal(cout))
        b = 0.1 * rng.standard_normal(cout)
        shift = 0.1 * rng.standard_normal(cout)
        alpha = None
        if self.act == "lrelu":
            alpha = np.array([0.2])
        elif self.act == "prelu":
            alpha = 0.1 + 0.05 * rng.standard_normal(cout)
        f = lambda a: None if a is None else np.asarray(a, np.float32)
        return [np.ascontiguousarray(m, np.float32) for m in mats], f(w), f(b), f(scale), f(shift), f(alpha)


C = Case
BOUND_CASES = [
    # ---- fp32 (csrc/xv_kernels.hip launch_gemm): XV_TUNE_FP32_GEMM 1 = tdnn_gemm_kernel, 2 = tdnn_gemm_dma_kernel, 3 = tdnn_gemm_k1_kernel
    C("fp32 tdnn_gemm_kernel 64-row", "fp32", "fp32", 512, 512, 5, 1, "relu", "relu", tune={"fp32": 1}),
    C("fp32 tdnn_gemm_kernel 128-row", "fp32", "fp32", 64, 512, 5, 1, "relu", "relu", tune={"fp32": 1}, big=True),
    C("fp32 tdnn_gemm_kernel ragged", "fp32", "fp32", 40, 200, 3, 2, "lrelu", "hostile", tune={"fp32": 1}),
    C("fp32 tdnn_gemm_dma_kernel<7>", "fp32", "fp32", 512, 512, 7, 1, "relu", "relu", tune={"fp32": 2}, big=True),
    C("fp32 tdnn_gemm_dma_kernel<3> d3", "fp32", "fp32", 512, 512, 3, 3, "relu", "hostile", tune={"fp32": 2}, big=True),
    C("fp32 tdnn_gemm_k1_kernel", "fp32", "fp32", 512, 1536, 1, 1, "relu", "hostile", tune={"fp32": 3}, big=True),
    # ---- fp32tc: tdnn_gemm_toom_kernel<K> (xv_toom.hip), the rows form of layer 0 (tdnn_gemm_kernel<true,64> on the windows)
    C("fp32tc toom<3>", "fp32tc", "toom", 512, 512, 3, 1, "relu", "relu"),
    C("fp32tc toom<3> d2", "fp32tc", "toom", 512, 512, 3, 2, "relu", "hostile"),
    C("fp32tc toom<3> d3", "fp32tc", "toom", 96, 200, 3, 3, "prelu", "relu"),
    C("fp32tc toom<3> d8", "fp32tc", "toom", 64, 64, 3, 8, "relu", "relu"),
    C("fp32tc toom<5>", "fp32tc", "toom", 512, 512, 5, 1, "relu", "hostile"),
    C("fp32tc toom<5> d2", "fp32tc", "toom", 64, 48, 5, 2, "lrelu", "relu"),
    C("fp32tc toom<7>", "fp32tc", "toom", 512, 512, 7, 1, "relu", "relu"),
    C("fp32tc rows form", "fp32tc", "rows", 23, 512, 5, 1, "relu", "mfcc"),
    # ---- bf16x3: tdnn_gemm_bf16x3_kernel<SPLIT_A, K, POOL, WM, S16> (csrc/xv_gemm3.hip launch_gemm3), tdnn_first_kernel<MODE, false>
    C("bf16x3 f32 input", "bf16x3", "bf16x3", 512, 512, 5, 1, "relu", "relu"),
    C("bf16x3 split 128-row", "bf16x3", "bf16x3", 96, 512, 5, 1, "relu", "hostile", xfmt="split", fmt="split", tune={"rows": 128}),
    C("bf16x3 split 256-row", "bf16x3", "bf16x3", 96, 512, 7, 1, "prelu", "relu", xfmt="split", fmt="split", tune={"rows": 256}),
    C("bf16x3 split 16x16", "bf16x3", "bf16x3", 512, 512, 7, 1, "relu", "relu", xfmt="split", fmt="f32"),
    C("bf16x3 split ragged", "bf16x3", "bf16x3", 40, 200, 3, 2, "lrelu", "hostile", xfmt="split", fmt="split"),
    C("bf16x3 first layer", "bf16x3", "first", 23, 512, 5, 1, "relu", "mfcc", fmt="split"),
    # ---- f16bf8 (csrc/xv_gemm8.hip launch_gemm8): tdnn_gemm_f16bf8_kernel (128 / 256 rows), _wide_kernel (512: xv_gemm8_wide.hip), _wide16_kernel (1024: xv_gemm8_wide16.hip); tdnn_first_kernel<MODE, true>
    #      (the first-layer kernel forms bf16x3 products whatever it writes)
    C("f16bf8 128-row f32 out", "f16bf8", "f16bf8", 512, 512, 5, 1, "relu", "relu", xfmt="split8", tune={"rows": 128}),
    C("f16bf8 256-row split out", "f16bf8", "f16bf8", 64, 200, 3, 1, "relu", "relu", xfmt="split8", fmt="split", tune={"rows": 256}),
    C("f16bf8 wide 512 split out", "f16bf8", "f16bf8", 96, 512, 7, 1, "relu", "relu", xfmt="split8", fmt="split", tune={"rows": 512}),
    # a split8 output carries the encoder's 2^-13: as large as the cross terms, so this case cannot show them (CPU power check (2))
    C("f16bf8 wide 512 split8 out", "f16bf8", "f16bf8", 96, 512, 5, 1, "relu", "relu", xfmt="split8", fmt="split8", tune={"rows": 512}),
    C("f16bf8 wide16 1024 split out", "f16bf8", "f16bf8", 512, 512, 5, 1, "relu", "hostile", xfmt="split8", fmt="split", tune={"rows": 1024}),
    C("f16bf8 wide16 1024 d3", "f16bf8", "f16bf8", 128, 256, 3, 3, "lrelu", "relu", xfmt="split8", fmt="split", tune={"rows": 1024}),
    C("f16bf8 first layer split8", "bf16x3", "first", 23, 512, 5, 1, "relu", "mfcc", fmt="split8"),
]
