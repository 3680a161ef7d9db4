"""The pair kernel (layers 3 + 4 + pooling statistics): bf16x3, 16 frames per wave (xv_pair.hip) against f16bf8 with the
reduction split over a pair of waves (xv_pair8.hip) and its f16mx6 form (layer 4's cross terms on block-scaled e2m3 MFMAs);
interleaved rounds.  argv[1] = rows (default 262144); argv[2] = input modes, comma-separated and interleaved round by round
(default "random"; PAIR8_BENCH_ZERO, below, applies to "random" only): "random" = dense frames, "relu" = max(N(0,1), 0) * 1.3
(about half the frames exact zeros, weights dense), "zeros" = all-zero frames and weights.  (The bf8 instantiation compiles to the same instructions as before the
f16mx6 form was added -- compared in the ISA -- so the f16bf8 line is also the A/B against the commit before.)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "x-vector-kaldi-tf_amd"))
import torch
from xvector_amd import hiplib
dev = torch.device("cuda:0"); R = int(sys.argv[1]) if len(sys.argv) > 1 else 262144
ZERO = os.environ.get("PAIR8_BENCH_ZERO", "")      # "w", "x" or "wx": zero weights / frames (how much of the time is the power limit)
MODES = sys.argv[2].split(",") if len(sys.argv) > 2 else ["random"]
assert all(m in ("random", "relu", "zeros") for m in MODES), MODES
cin, cmid, cout = 512, 512, int(os.environ.get('PAIR8_BENCH_COUT', '1536'))
w1 = torch.randn((cin, cmid), device=dev) / cin ** 0.5; w2 = torch.randn((cmid, cout), device=dev) / cmid ** 0.5
if 'w' in ZERO: w1.zero_(); w2.zero_()
b1 = torch.zeros(cmid, device=dev); b2 = torch.zeros(cout, device=dev); rv = torch.ones(R, dtype=torch.uint8, device=dev)
blk3 = torch.empty(hiplib.block_stats_floats(R, cout), device=dev); blk8 = torch.empty_like(blk3); blk6 = torch.empty_like(blk3)
status = torch.zeros(1, dtype=torch.int32, device=dev)
fns = {}
for m in MODES:
    wa, wb = (torch.zeros_like(w1), torch.zeros_like(w2)) if m == "zeros" else (w1, w2)
    p3, p8, p6 = hiplib.pack_pair_bf16x3(wa, wb), hiplib.pack_pair_f16bf8(wa, wb), hiplib.pack_pair_f16mx6(wa, wb)
    x = torch.relu(torch.randn((R, cin), device=dev)) * 1.3
    x = x - 0.4 if m == "random" else x * 0.0 if m == "zeros" else x
    if m == "random" and 'x' in ZERO: x.zero_()
    if m == "relu": print("relu mode: %.1f %% of the frames are exact zeros" % (100.0 * float((x == 0).float().mean())))
    x3 = hiplib.SplitBuf(R, cin, dev); hiplib.split_encode(x, x3)
    x8 = hiplib.SplitBuf(R, cin, dev, hiplib.FMT_SPLIT8); hiplib.split_encode(x, x8)
    del x
    tag = "" if MODES == ["random"] else " [%s]" % m
    fns["bf16x3, 16 frames/wave" + tag] = lambda x3=x3, p3=p3: hiplib.tdnn_pair_pool(x3, R, p3, (b1, None, None, None), (b2, None, None, None), 1, rv, blk3)
    fns["f16bf8, wave pairs" + tag] = lambda x8=x8, p8=p8: hiplib.tdnn_pair_pool8(x8, R, p8, (b1, None, None, None), (b2, None, None, None), 1, rv, blk8, status)
    fns["f16mx6, wave pairs" + tag] = lambda x8=x8, p6=p6: hiplib.tdnn_pair_pool_mx6(x8, R, p6, (b1, None, None, None), (b2, None, None, None), 1, rv, blk6, status)
times = {k: [] for k in fns}
for rnd in range(6):
    for name, fn in fns.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(8): fn()
        b.record(); torch.cuda.synchronize()
        if rnd: times[name].append(a.elapsed_time(b) / 8)
for name, t in times.items():
    t = sorted(t); med = t[len(t) // 2]
    print("layers 3+4+pool %-32s median %.3f ms (min %.3f, max %.3f; rounds %s)  %.0f TF algorithmic" %
          (name, med, t[0], t[-1], " ".join("%.3f" % v for v in times[name]), 2.0 * R * cin * (cmid + cout) / 1e9 / med))
if MODES[-1] != "zeros":                      # (the buffers hold the last mode's statistics; all-zero ones have no relative error)
    a, b = blk3.view(-1, 2, cout), blk8.view(-1, 2, cout)
    print("block statistics, f16bf8 vs bf16x3: mean rel L2 %.2e, M2 rel L2 %.2e, status %d" %
          (float((a[:, 0] - b[:, 0]).norm() / a[:, 0].norm()), float((a[:, 1] - b[:, 1]).norm() / a[:, 1].norm()), int(status.item())))
    b = blk6.view(-1, 2, cout)
    print("block statistics, f16mx6 vs bf16x3: mean rel L2 %.2e, M2 rel L2 %.2e" %
          (float((a[:, 0] - b[:, 0]).norm() / a[:, 0].norm()), float((a[:, 1] - b[:, 1]).norm() / a[:, 1].norm())))
