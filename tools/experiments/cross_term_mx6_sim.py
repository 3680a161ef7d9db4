"""EXPERIMENT -> SHIPPED for layer 4 (xv_tdnn_pair_pool_f16mx6): the cross terms of the f16bf8 arithmetic in block-scaled e2m3, simulated
on the CPU (fp64 accumulation, the forward of mixed_split_sim.py) with the K-block structure the pair kernel has:
  a block   = 16 channels of one frame / of one weight column (for layer 4 the 16 channels a lane of the pair kernel holds of a
              32-channel slab: (r & 3) + 8 (r >> 2) + 4 hh; for the other layers 16 consecutive input channels of a tap), its 32 values
              [2^11 lo | c] (activations) / [c | 2^11 lo] (weights)
  scale     = the largest power of two s with s max|block| <= 7.5, 1 for an all-zero block
  element   = e2m3(s value), nearest even (csrc/xv_split6.h)
  product   = xh wh + 2^-11 (e2m3(2^11 xl) e2m3(w) + e2m3(x) e2m3(2^11 wl)), xh / wh fp16
against the shipped e5m2 cross terms.  Weights: synthetic.trained_like; relative L2 of the x-vector against fp64.
Output (seeds 1 / 2 / 3):
  T = 200   shipped (e5m2 everywhere)   1.18e-05  1.09e-05  1.18e-05
  T = 200   layer 4 in e2m3             1.08e-05  1.01e-05  1.07e-05
  T = 200   layers 3 + 4 in e2m3        9.81e-06  8.72e-06  9.80e-06
  T = 200   layers 1 - 4 in e2m3        7.32e-06  7.79e-06  6.86e-06
  T = 40    shipped (e5m2 everywhere)   1.98e-05  1.72e-05  1.80e-05
  T = 40    layer 4 in e2m3             1.85e-05  1.65e-05  1.71e-05
On the GPU (tests/test_gpu_pair_mx6.py, utterances of 25 / 40 / 61 MFCC-like frames, seed 1): 1.818e-5 against 1.881e-5 for the bf8
pair kernel; the load-time probe of the benchmark's weights went from 1.630e-5 to 1.563e-5.
  python tools/experiments/cross_term_mx6_sim.py"""
import os, sys, numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "x-vector-kaldi-tf_amd")); sys.path.insert(0, os.path.join(ROOT, "tools/experiments"))
from oracle import oracle
from xvector_amd import synthetic
import mixed_split_sim as ms

def q(a, dt): return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dt).to(torch.float64).numpy()
def e5(a): return q(np.clip(a, -57344, 57344), torch.float8_e5m2)

def e2m3(a):                           # nearest even on the e2m3 grid, saturating at 7.5
    mag = np.minimum(np.abs(a), 8.0)
    step = np.where(mag < 2, 0.125, np.where(mag < 4, 0.25, 0.5))
    return np.copysign(np.minimum(np.rint(mag / step) * step, 7.5), a)

def pair_blocks(k):                    # [k / 16, 16]: the channels of each block
    if k == 512:                       # layer 4: the in-register H of the pair kernel
        return np.array([[32 * (b >> 1) + (r & 3) + 8 * (r >> 2) + 4 * (b & 1) for r in range(16)] for b in range(32)])
    return np.arange(k).reshape(-1, 16)

def mx6_planes(rows):                  # rows [n, K] (a block per row and 16-channel group) -> dequantised (2^11 lo, c) planes
    c = np.clip(rows, -57344, 57344)
    lo = (c - q(c, torch.float16)) * 2048
    idx = pair_blocks(rows.shape[1])
    m = np.maximum(np.abs(lo[:, idx]).max(-1), np.abs(c[:, idx]).max(-1))
    f, e = np.frexp(m)
    k = np.where(m == 0, 0, np.where(f <= 0.9375, e - 3, e - 2))
    s = np.ldexp(1.0, -k)[:, :, None]
    out = []
    for p in (lo, c):
        full = np.zeros_like(p)
        full[:, idx] = e2m3(p[:, idx] * s) / s
        out.append(full)
    return out

def make(layers6):
    state = {"layer": 1}               # (forward() runs layer 0 in bf16x3 itself: this is called for layers 1 .. 4 in turn)
    def mm(x, w):
        i = state["layer"]; state["layer"] = i % 4 + 1
        x32, w32 = x.astype(np.float32).astype(np.float64), w.astype(np.float32).astype(np.float64)
        xh, wh = q(x32, torch.float16), q(w32, torch.float16)
        if i in layers6 and x.shape[1] % 16 == 0:
            xl6, xc6 = mx6_planes(x32)
            wl6, wc6 = (p.T for p in mx6_planes(w32.T.copy()))
            return xh @ wh + (xl6 @ wc6 + xc6 @ wl6) / 2048
        xl, wl = x32 - xh, w32 - wh
        return xh @ wh + (e5(xl * 2048) @ e5(w32) + e5(x32) @ e5(wl * 2048)) / 2048
    return mm

if __name__ == "__main__":
    topo = dict(oracle.DEFAULT_TOPOLOGY)
    cases = (("shipped (e5m2 everywhere)", ()), ("layer 4 in e2m3", (4,)), ("layers 3 + 4 in e2m3", (3, 4)), ("layers 1 - 4 in e2m3", (1, 2, 3, 4)))
    for T in (200, 40):
        res = {name: [] for name, _ in cases}
        for seed in (1, 2, 3):
            weights = synthetic.trained_like(topo, 23, seed=seed)
            x = np.random.default_rng(0).standard_normal((T, 23)).astype(np.float32) * 3
            ref = ms.forward(x, weights, topo, ms.make_mm("exact"), first_exact=False)
            for name, layers6 in cases[:4 if T == 200 else 2]:
                res[name].append(oracle.rel_l2(ms.forward(x, weights, topo, make(layers6)), ref))
        for name, _ in cases[:4 if T == 200 else 2]:
            print("  T = %-5d %-27s %s" % (T, name, "  ".join("%.2e" % v for v in res[name])))
