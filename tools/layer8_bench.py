"""bf16x3 against f16bf8 (one fp16 MFMA + one scaled bf8 MFMA per product), layer by layer, interleaved rounds in ONE process.
argv[1] = rows per batch (default 262144); argv[2] = input modes of the frames, comma-separated and interleaved round by round
(default "random"): "random" = dense frames (ReLU output with a BN shift added), "relu" = max(N(0,1), 0) * 1.3 (about half the
frames exact zeros in every plane, weights dense -- what a layer reads once the producer's BN shift sits in its bias), "zeros" =
all-zero frames AND weights (the full clock: the difference to it is the power limit).
The K > 1 shapes also run the e2m3 form of the cross terms (xv_tdnn_layer_f16mx6: FMT_SPLIT6 frames, f16mx6 weights) and the bf8
layer writing FMT_SPLIT6 rows -- the consumer's saving and the producer's cost of one mx6 layer; 16 x 16 MFMA form (tile 1024) only --,
and "f16mx6 -> split6", the e2m3 layer writing FMT_SPLIT6 rows itself (layer 1 of the step when both it and layer 2 run the e2m3
form).  Last comes layer 0 (xv_tdnn_first_*: 24 -> 512, K = 5) writing FMT_SPLIT8 against FMT_SPLIT6 rows, the producer's side of
layer 1's e2m3 form.  argv[3] = "mx6": only the K = 5 shape at tile 1024 and layer 0 (the forms that A/B)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "x-vector-kaldi-tf_amd"))
import torch
from xvector_amd import hiplib
dev = torch.device("cuda:0"); R = int(sys.argv[1]) if len(sys.argv) > 1 else 262144
MODES = sys.argv[2].split(",") if len(sys.argv) > 2 else ["random"]
assert all(m in ("random", "relu", "zeros") for m in MODES), MODES
ROUNDS, REPS = 5, 8
ONLY_MX6 = len(sys.argv) > 3 and sys.argv[3] == "mx6"
TILES = (1024,) if ONLY_MX6 else (128, 256, 512, 1024)          # XV_TUNE_TILE_ROWS: 512 = the 256 x 256 tile on 32 x 32 MFMAs, 1024 = on 16 x 16 MFMAs (the default form of the K > 1 shapes)
print("lib:", hiplib.SO_PATH, "rows:", R)
for (cin, cout, K) in ((512, 512, 5), (512, 512, 7), (512, 512, 1), (512, 1536, 1))[:1 if ONLY_MX6 else 4]:
    w = torch.randn((K, cin, cout), device=dev) / (K * cin) ** 0.5
    packed, frames = {}, {}
    for m in MODES:
        wm = torch.zeros_like(w) if m == "zeros" else w
        packed[m] = (hiplib.pack_weights_bf16x3(wm), hiplib.pack_weights_f16bf8(wm), hiplib.pack_weights_f16mx6(wm) if K > 1 else None)
        x = torch.relu(torch.randn((R, cin), device=dev)) * 1.3
        x = x - 0.4 if m == "random" else x * 0.0 if m == "zeros" else x
        if m == "relu" and K == 5: print("relu mode: %.1f %% of the frames are exact zeros" % (100.0 * float((x == 0).float().mean())))
        x3 = hiplib.SplitBuf(R, cin, dev); hiplib.split_encode(x, x3)
        x8 = hiplib.SplitBuf(R, cin, dev, hiplib.FMT_SPLIT8); hiplib.split_encode(x, x8)
        x6 = None
        if K > 1: x6 = hiplib.SplitBuf(R, cin, dev, hiplib.FMT_SPLIT6); hiplib.split_encode(x, x6)
        frames[m] = (x3, x8, x6)
        del x
    bias = torch.zeros(cout, device=dev); rv = torch.ones(R, dtype=torch.uint8, device=dev)
    y3 = hiplib.SplitBuf(R, cout, dev); y8 = hiplib.SplitBuf(R, cout, dev, hiplib.FMT_SPLIT8); y6 = y8.view(cout, hiplib.FMT_SPLIT6)
    blk = torch.empty(hiplib.block_stats_floats(R, cout), device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    fns = {}
    for m in MODES:
        (w3, w8, w6), (x3, x8, x6) = packed[m], frames[m]
        tag = "" if MODES == ["random"] else " [%s]" % m
        if cout == 1536:
            fns["bf16x3" + tag] = lambda x3=x3, w3=w3: hiplib.tdnn_layer_pool(x3, R, w3, bias, None, None, 1, None, 1, rv, blk)
            fns["f16bf8" + tag] = lambda x8=x8, w8=w8: hiplib.tdnn_layer_pool8(x8, R, w8, bias, None, None, 1, None, 1, rv, blk)
        else:
            fns["bf16x3" + tag] = lambda x3=x3, w3=w3: hiplib.tdnn_layer3(x3, R, w3, bias, None, None, 1, None, 1, rv, y3)
            fns["f16bf8" + tag] = lambda x8=x8, w8=w8: hiplib.tdnn_layer8(x8, R, w8, bias, None, None, 1, None, 1, rv, y8, status)
            fns["f16bf8 -> bf16 split" + tag] = lambda x8=x8, w8=w8: hiplib.tdnn_layer8(x8, R, w8, bias, None, None, 1, None, 1, rv, y3, status)
            if K > 1:
                fns["f16mx6" + tag] = lambda x6=x6, w6=w6: hiplib.tdnn_layer_mx6(x6, R, w6, bias, None, None, 1, None, 1, rv, y8, status)
                fns["f16bf8 -> split6" + tag] = lambda x8=x8, w8=w8: hiplib.tdnn_layer8(x8, R, w8, bias, None, None, 1, None, 1, rv, y6, status)
                fns["f16mx6 -> split6" + tag] = lambda x6=x6, w6=w6: hiplib.tdnn_layer_mx6(x6, R, w6, bias, None, None, 1, None, 1, rv, y6, status)
    tiles = TILES if K > 1 else TILES[:2]     # (a K = 1 layer has no 256 x 256 form: knobs 512 / 1024 would repeat the default)
    only16 = lambda n: n.startswith("f16mx6") or "split6" in n          # forms of the 16 x 16 MFMA kernel alone
    times = {(n, rows): [] for n in fns for rows in tiles if rows == 1024 or not only16(n)}
    for rnd in range(ROUNDS + 1):
        for rows in tiles:
            hiplib.set_tuning(hiplib.TUNE_TILE_ROWS, rows)
            for n, fn in fns.items():
                if (n, rows) not in times: continue
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(REPS): fn()
                b.record(); torch.cuda.synchronize()
                if rnd: times[(n, rows)].append(a.elapsed_time(b) / REPS)
    hiplib.set_tuning(hiplib.TUNE_TILE_ROWS, 0)
    # accuracy of both against the fp32 matmul of torch on a slice (rough; the parity tests are the real check)
    for (n, rows), t in times.items():
        t = sorted(t); med = t[len(t) // 2]
        alg = 2.0 * R * cin * cout * K / 1e9
        print("cin %d cout %4d K %d %-30s tile %4d: median %.3f ms (min %.3f, max %.3f)  %.0f TF algorithmic" % (cin, cout, K, n, rows, med, t[0], t[-1], alg / med))
    assert int(status.item()) == 0

# layer 0 of the step: MFCC-like rows (23 features in 24 columns), K = 5, 24 -> 512, ReLU + BN scale, no shift (the folded step)
cin, cout, K = 24, 512, 5
x = torch.randn((R, cin), device=dev) * 3.0; x[:, 23] = 0.0
w = torch.randn((K, cin, cout), device=dev) / (K * 23) ** 0.5; w[:, 23] = 0.0
wf = hiplib.pack_first_bf16x3(w)
bias = torch.randn(cout, device=dev) * 0.1; scale = 1.0 + 0.1 * torch.rand(cout, device=dev)
rv = torch.ones(R, dtype=torch.uint8, device=dev); status = torch.zeros(1, dtype=torch.int32, device=dev)
y8 = hiplib.SplitBuf(R, cout, dev, hiplib.FMT_SPLIT8); y6 = y8.view(cout, hiplib.FMT_SPLIT6)
fns = {"first -> split8": lambda: hiplib.tdnn_first(x, R, wf, bias, scale, None, 1, None, 1, rv, y8, status),
       "first -> split6": lambda: hiplib.tdnn_first(x, R, wf, bias, scale, None, 1, None, 1, rv, y6, status)}
times = {n: [] for n in fns}
for rnd in range(ROUNDS + 1):
    for n, fn in fns.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPS): fn()
        b.record(); torch.cuda.synchronize()
        if rnd: times[n].append(a.elapsed_time(b) / REPS)
for n, t in times.items():
    t = sorted(t)
    print("cin %d cout %4d K %d %-30s            median %.3f ms (min %.3f, max %.3f)" % (cin, cout, K, n, t[len(t) // 2], t[0], t[-1]))
assert int(status.item()) == 0
