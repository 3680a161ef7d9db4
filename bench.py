#!/usr/bin/env python
"""bench.py -- x-vector extraction throughput on MI355X (BASELINE.json metric: utterances/sec ==
x-vectors/sec, 512-d; % of MFMA peak on the TDNN GEMMs; % of HBM peak on statistics pooling).

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

Workload (per GPU, weak scaling): BASELINE.json configs[1] -- 10,000 synthetic utterances of 23-dim
MFCC, T ~ U{200..400} (seed 1234 + rank), default x-vector topology with seeded trained-like weights,
512-d embedding (``embed_layer-0/scores``).  One STEP = one pass of the hot path over that whole set:
for every ragged batch 5x TDNN GEMM -> statistics pooling -> segment FC, then the length-weighted chunk
average, then (N > 1) the single RCCL gather of the [10000, 512] blocks to rank 0.  Inputs (packed
feature batches) are resident in HBM before the timed region starts; nothing is skipped or cached.

Rank 0 prints ONE JSON line.  A plain run sets up, warms up, times the steps, writes ``--dump-outputs`` and prints the line
with what its own timed region measured: ``value`` / ``ms_per_step``, ``roofline`` for the GEMM kernels of the step (bf16x3
split-precision MFMA by default: tdnn_gemm_bf16x3_kernel for layers 0-2, tdnn_pair_pool_kernel for layers 3+4 + pooling
statistics, the FC) from algorithmic FLOPs / HIP-event time measured inside the timed region, the pooling launches' figure
(``pool_blocks`` behind the fused epilogue, ``roofline_pool`` without it) and ``accuracy_probe`` (what ``engine.select_model``
measured when it admitted the arithmetic for these weights).

``--full`` adds everything that takes runs or checks of its own, after the timed region: ``roofline.by_launch`` (extra passes
over the largest batch), ``roofline_pool`` of the standalone pooling kernel, the parity of sampled utterances against the fp64
oracle, ``with_ark_write`` and ``cpu_baseline``, a torch-CPU fp32 port of the reference forward (batch 1, like the reference)
timed on this box's host cores on a bounded sample: the faithful 2-thread figure, a thread sweep, and ``all_cores`` = the
reference's deployment shape (nj processes x 2 threads).  At N = 1 the full line also carries ``fp32_exact`` (the same step on
the exact-fp32 MFMA path), ``bf16x3`` (all layers in the bf16x3 arithmetic), ``e2e_ark_to_ark`` (ark bytes ->
Model.make_embedding -> ark bytes, PCIe and Kaldi parsing included; never ``value``), ``cli_job`` (the wall clock of one
``extract_embedding.py`` worker job from process birth to renamed ark,scp), ``config2_varlen`` (BASELINE configs[2]:
T in [25, 10000], length-bucketed), ``train_step`` (BASELINE configs[4]: one rank's share) and ``trained_checkpoint``.
``--mode train`` has nothing beyond its headline: ``--full`` changes nothing there.

``python bench.py --gpus N`` with N > 1 starts its own N ranks (xvector_amd/launch.py) when it is not already one.
``--dump-outputs DIR`` writes what the last timed step computed (``xvectors.npy``: [N x utts, 512] float32 in utterance order; in
``--mode train`` the timed steps' losses and the weights after them) for output-by-output comparison of two builds.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "x-vector-kaldi-tf_amd"))

MFMA_F32_PEAK = 157.3e12      # /opt/skills/guides/MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, 256 CU x 2.4 GHz
MFMA_BF16_PEAK = 2.5e15       # same guide: dense bf16 MFMA (AMD's 5 PF figure is 2:1 sparse)
HBM_PEAK = 8.0e12             # same guide: HBM3E 8 TB/s spec


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--utts", type=int, default=10000, help="utterances per GPU (configs[1]: 10000)")
    ap.add_argument("--tmin", type=int, default=200)
    ap.add_argument("--tmax", type=int, default=400)
    ap.add_argument("--batch-rows", type=int, default=262144)
    ap.add_argument("--full", action="store_true",
                    help="after the headline's timed steps, also run every other measurement and check of the line (per-launch and "
                         "standalone pooling figures, parity against the fp64 oracle, ark write, CPU baseline, the other arithmetics, "
                         "ark -> ark, CLI job, configs[2] and configs[4] legs); a plain run measures the headline alone")
    ap.add_argument("--cpu-budget", type=float, default=18.0, help="--full: seconds of CPU-baseline timing (0 = skip it and the parity check)")
    ap.add_argument("--e2e-utts", type=int, default=50000,
                    help="--full, N = 1 only: utterances of the ark -> ark sub-measurement through Model.make_embedding (0 = skip)")
    ap.add_argument("--no-fp32-leg", action="store_true", help="--full: skip the exact-fp32 sub-measurement (fp32_exact)")
    ap.add_argument("--parity-utts", type=int, default=40,
                    help="--full: utterances, spread over ALL batches of the step, checked against the fp64 oracle")
    ap.add_argument("--no-extra-legs", action="store_true", help="--full: skip config2_varlen, train_step and cli_job")
    ap.add_argument("--no-job-rehearsal", action="store_true", help="--full: skip cli_job.rehearsal_8x125k (the 1 M-utterance job's counts)")
    ap.add_argument("--no-fused-pool", action="store_true",
                    help="bf16x3: store the last layer and run the standalone pooling kernel (A/B against the fused epilogue)")
    ap.add_argument("--mode", choices=["extract", "train"], default="extract",
                    help="extract = the headline benchmark (default); train = BASELINE configs[4]: training steps on synthetic "
                         "64-chunk minibatches (SURVEY §8f-1), reported as chunks/s")
    ap.add_argument("--train-precision", choices=["fp32", "bf16x3"], default="fp32",
                    help="--mode train: arithmetic of the forward / input-gradient GEMMs")
    ap.add_argument("--train-class", default=None,
                    help="--mode train only: a model class of local/tf/models.py (e.g. ModelL2LossWithoutDropoutLReluAttention) "
                         "instead of the default ModelWithoutDropout network; implies its own head (softmax-CE)")
    ap.add_argument("--head", choices=["am_softmax", "softmax"], default="am_softmax",
                    help="--mode train: classification head (BASELINE configs[4] names AM-softmax; 'softmax' = the reference's head)")
    ap.add_argument("--precision", choices=["f16bf8", "bf16x3", "fp32", "fp32tc"], default="f16bf8",
                    help="GEMM arithmetic: f16bf8 (default) = one fp16 MFMA + one block-scaled bf8 MFMA of the cross terms per "
                         "product in the hidden layers, ~1.3e-5 rel-L2; bf16x3 = split-precision bf16 MFMA, ~5e-6; fp32 = exact "
                         "fp32-input MFMA.  All accumulate in fp32; the parity bar is 1e-4")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed path computed in its last step as DIR/<name>.npy (float32 / "
                         "float64, at most 64 MB in all; a fixed, seeded sample of rows beyond that).  The inputs are seeded: the same "
                         "arguments give the same inputs, so two builds can be compared output for output")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


DUMP_CAP_BYTES = 64 << 20


def _dump_outputs(path, arrays):
    """Write ``arrays`` ({name: ndarray}) as ``path/<name>.npy``, float32 / float64 kept as they are (other dtypes become
    float64).  Over DUMP_CAP_BYTES in all, every array with more than one row is cut to the same fixed, seeded sample of row
    indices (sorted), so that the files of two runs with the same arguments line up row for row."""
    import re
    os.makedirs(path, exist_ok=True)
    arrays = {k: (v if v.dtype in (np.float32, np.float64) else v.astype(np.float64)) for k, v in
              ((k, np.ascontiguousarray(v)) for k, v in arrays.items())}
    total = sum(v.nbytes for v in arrays.values())
    if total > DUMP_CAP_BYTES:
        keep = DUMP_CAP_BYTES / total
        for k, v in arrays.items():
            if v.ndim >= 1 and v.shape[0] > 1:
                n = max(1, int(v.shape[0] * keep))
                rows = np.sort(np.random.default_rng(0).choice(v.shape[0], size=n, replace=False))
                arrays[k] = np.ascontiguousarray(v[rows])
    for k, v in arrays.items():
        np.save(os.path.join(path, re.sub(r"[^A-Za-z0-9_.-]", "_", k) + ".npy"), v)


def _train_run(args, rank, world, dev, topo, feat, precision, steps, warmup, collect=False):
    """BASELINE configs[4]: minibatches of 64 chunks, one length T~U{200..400} per minibatch (create_egs.py:508-513), 64
    synthetic speakers, softmax-CE head as in models.py:96-113 (or the build-defined AM-softmax head), Adam; data parallel over
    ranks with bucketed gradient all-reduces.  A step = forward + backward + (all-reduce) + Adam on one resident minibatch per
    rank.  Returns the measurements as a dictionary; with ``collect``, ``outputs`` holds what the timed steps computed (the loss of
    each timed step, the weights after the last one)."""
    import torch
    import torch.distributed as dist
    from xvector_amd import synthetic, topology as tp, trainer
    B, n_spk = 64, 64
    head = args.head
    if args.train_class:
        topo = tp.get(args.train_class)
        head = "am_softmax" if (topo.get("head") or {}).get("type") == "am_softmax" else "softmax"
    weights = synthetic.reference_init(topo, feat, n_spk, seed=1)
    for k in list(weights):                                   # fan-in scaled start so that activations stay O(1)
        if k.endswith("/w:0") and weights[k].ndim == 3:
            weights[k] = (weights[k] * (np.sqrt(2.0 / (weights[k].shape[0] * weights[k].shape[1])) / 0.1)).astype(np.float32)
    if "attention/w:0" in weights:
        weights["attention/w:0"] = (weights["attention/w:0"] * (np.sqrt(1.0 / weights["attention/w:0"].shape[0]) / 0.1)).astype(np.float32)
    if head == "am_softmax" and not args.train_class:
        topo = tp.get("ModelWithoutDropoutAMSoftmax")        # same network, build-defined additive-margin head
    tr = trainer.Trainer(weights, topo, dev, precision=precision)
    rng = np.random.default_rng(1234 + rank)
    n_total = warmup + steps
    spk = rng.standard_normal((n_spk, feat)) * 2
    batches = []
    for _ in range(n_total):
        T = int(rng.integers(args.tmin, args.tmax + 1))
        lab = rng.integers(0, n_spk, B)
        batches.append(((spk[lab][:, None, :] + rng.standard_normal((B, T, feat)) * 3).astype(np.float16), lab.astype(np.int32)))

    def fence():
        torch.cuda.synchronize()
        if dist.is_initialized():
            dist.barrier()
        torch.cuda.synchronize()

    losses = []
    # one untimed step at the LONGEST minibatch first: torch's caching allocator then owns blocks every later step can be carved
    # from (each new length otherwise costs a round of hipMalloc calls -- a training run pays that in its first few hundred steps,
    # a 30-step measurement would be mostly that; steady state: tools/train_drift.py)
    lab0 = rng.integers(0, n_spk, B)
    tr.step((spk[lab0][:, None, :] + rng.standard_normal((B, args.tmax, feat)) * 3).astype(np.float16), lab0.astype(np.int32), 0.0)
    for i in range(warmup):
        tr.step(batches[i][0], batches[i][1], 1e-3)
    # the interpreter's cyclic garbage collector stays out of the timed region: a full collection of this process's object
    # graph is a 40 ms pause -- one of them inside a 30-step window moved the result from 3.7 to 4.8 ms per step
    import gc
    gc.collect()
    gc.disable()
    fence()
    t0 = time.perf_counter()
    per_step = []
    prev = None
    for i in range(warmup, n_total):
        t1 = time.perf_counter()
        # every step's loss is read back, one step late -- as Model.train_one_iteration does (Trainer.step_async): the host stages
        # minibatch i + 1 while the GPU finishes step i
        handle = tr.step_async(batches[i][0], batches[i][1], 1e-3)
        if prev is not None:
            losses.append(prev.result()[0])
        prev = handle
        per_step.append(time.perf_counter() - t1)
    losses.append(prev.result()[0])

    fence()
    dt = time.perf_counter() - t0
    gc.enable()
    if os.environ.get("XV_BENCH_STEP_TIMES") == "1":
        sys.stderr.write("step ms: " + " ".join("%.2f" % (t * 1e3) for t in per_step) + "\n")
    if dist.is_initialized():
        tmax = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax.item())
    frames = sum(b[0].shape[1] for b in batches[warmup:]) * B
    fwd = tp.flops_per_frame(topo, feat) * frames + B * steps * (tp.flops_per_utt(topo, 1) + 2 * 512 * n_spk)
    # MFMA-pipe time of a step at nominal rates: forward, input-gradient and weight-gradient GEMMs in the chosen arithmetic
    # (bf16x3: 3 bf16 MFMAs per product at 2.5 PF -- xv_wgrad_bf16x3 since round 4; fp32: the 157.3 TF fp32 MFMA)
    pipe = 3.0 * fwd * (3.0 / MFMA_BF16_PEAK if precision == "bf16x3" else 1.0 / MFMA_F32_PEAK)
    r = {"chunks_per_s": B * world * steps / dt, "ms_per_step": dt / steps * 1e3, "steps": steps, "warmup": warmup,
         "steps_per_s": steps / dt, "frames_per_s": frames * world / dt, "approx_tflops_fwd_bwd": 3.0 * fwd * world / dt / 1e12,
         "mfma_time_over_time": pipe / dt,
         "peak_note": "3 x forward FLOPs (forward, input gradient, weight gradient); MFMA-pipe time = all three at %s"
                      % ("2.5 PF / 3 (bf16x3: three bf16 MFMAs per product)" if precision == "bf16x3" else "the 157.3 TF fp32 MFMA peak"),
         "fused_bn_sums": bool(tr.fused_sums),
         "precision": precision, "head": head, "class": args.train_class or "ModelWithoutDropout",
         "first_loss": losses[0], "last_loss": losses[-1]}
    if collect:
        r["outputs"] = {"losses": np.asarray(losses, np.float64)}
        r["outputs"].update(("weights/" + k, v) for k, v in sorted(tr.export()[0].items()))
    return r


def bench_train(args, rank, world, dev, topo, feat):
    """``--mode train``: the training step as the headline of its own line."""
    import torch.distributed as dist
    r = _train_run(args, rank, world, dev, topo, feat, args.train_precision, args.steps, args.warmup, collect=bool(args.dump_outputs))
    if rank == 0:
        if args.dump_outputs:
            _dump_outputs(args.dump_outputs, r["outputs"])
        print(json.dumps({
            "metric": "training chunks/sec (64-chunk minibatches, 200-400 frames, 64-way %s, Adam)" % ("AM-softmax" if r["head"] == "am_softmax" else "softmax-CE"),
            "value": r["chunks_per_s"], "unit": "chunks/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": r["ms_per_step"], "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32" if args.train_precision == "fp32" else "f32 (fwd/dgrad GEMMs as bf16x3 split MFMA, f32 accumulate)",
            "data": "synthetic",
            "config": {"workload": "BASELINE configs[4]: training, B=64 chunks/minibatch/GPU, T~U{%d..%d}, 64 speakers, "
                                   "%s topology, head: %s%s" % (args.tmin, args.tmax, r["class"], r["head"],
                                   " (scale 30, margin 0.2; build-defined, the reference has softmax-CE only)" if r["head"] == "am_softmax" else ""),
                       "parallelism": "data parallel x%d, bucketed gradient all-reduces during the backward pass" % world},
            "steps_per_s": r["steps_per_s"], "frames_per_s": r["frames_per_s"],
            "approx_tflops_fwd_bwd": r["approx_tflops_fwd_bwd"], "mfma_time_over_time": r["mfma_time_over_time"],
            "first_loss": r["first_loss"], "last_loss": r["last_loss"]}))
    if dist.is_initialized():
        dist.destroy_process_group()


def _trained_checkpoint_leg(dev, feat):
    """The arithmetic the accuracy guard admits for a checkpoint that was TRAINED (300 Adam steps of the product's own training step
    on 64 synthetic speakers), its probe values, and its parity against the fp64 oracle on MFCC-like utterances -- every other
    weight set of this line is a draw (synthetic.trained_like)."""
    from oracle import oracle                                  # the checker, here as in the parity leg
    from xvector_amd import engine, synthetic, topology as tp
    topo = tp.get("ModelWithoutDropout")
    w, info = synthetic.trained_checkpoint(topo, feat, n_spk=64, steps=300, seed=3, device=dev)
    mats = synthetic.mfcc_like([25, 120, 300, 411], feat, seed=5)
    refs = [oracle.embed_utterance(m, w, topo, 25, 10000, np.float64) for m in mats]
    res = {"training": info, "parity_utterances": len(mats), "limit_f16bf8_vs_bf16x3": engine.PROBE_LIMIT_F16BF8}
    for precision in ("f16bf8", "bf16x3", "fp32"):
        model = engine.select_model(w, topo, dev, precision=precision)
        ex = engine.Extractor(model, 25, 10000)
        vecs = ex.extract(mats)
        sel = model.selection
        res[precision] = {"selected": ("bf16x3" if ex.demoted and sel["selected"] == "f16bf8" else sel["selected"]),
                          "load_time_probe": sel.get("f16bf8_vs_bf16x3"), "run_time_probe": ex.stats.get("probe_rel_l2_max"),
                          "demoted_at_run_time": bool(ex.demoted),
                          "parity_rel_l2_max_vs_fp64_oracle": float(max(oracle.rel_l2(v, r) for v, r in zip(vecs, refs)))}
    res["selected"] = res["f16bf8"]["selected"]
    res["probe"] = res["f16bf8"]["load_time_probe"]
    res["parity"] = res["f16bf8"]["parity_rel_l2_max_vs_fp64_oracle"]
    return res


def _kernel_source_sha():
    """Hash of the kernel sources: profiles/traffic.json is only quoted when it was measured on these very kernels."""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, "x-vector-kaldi-tf_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".h")):                       # device code (the host library, xv_host.cpp, moves no HBM traffic)
            h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:16]


def _traffic(batch_rows):
    """(bytes per launch or None, provenance) from profiles/traffic.json -- PMC counters come from separate rocprofv3 passes
    (tools/profile_round.sh), so the number is stamped with the kernel sources and batch size it was measured at and dropped
    when either differs from this run."""
    tpath = os.path.join(ROOT, "profiles", "traffic.json")
    if not os.path.exists(tpath):
        return None, "no profiles/traffic.json"
    try:
        t = json.load(open(tpath))
    except Exception:
        return None, "unreadable profiles/traffic.json"
    if t.get("kernel_sha") != _kernel_source_sha():
        return None, "profiles/traffic.json is stale: measured on other kernel sources (%s)" % t.get("kernel_sha")
    if t.get("batch_rows") != batch_rows:
        return None, "profiles/traffic.json was measured at batch_rows=%s" % t.get("batch_rows")
    return t.get("gemm_hbm_bytes_per_launch"), "%s; batch_rows %d; kernel sources %s" % (t.get("source"), t["batch_rows"], t["kernel_sha"])


def _resident_batches(args, model, lens, dev, feat, seed):
    """The workload in kernel layout, resident in HBM: length-bucketed ragged batches of <= batch_rows rows."""
    import torch
    from xvector_amd import engine
    gap, align = model.gap, model.align
    lead = (gap + align - 1) // align * align
    order = np.argsort(lens, kind="stable")
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    batches = []
    b0 = 0
    while b0 < len(order):
        rows, b1 = lead, b0
        while b1 < len(order) and (b1 == b0 or rows + int(engine.slot_rows(lens[order[b1]], gap, align)) <= args.batch_rows):
            rows += int(engine.slot_rows(lens[order[b1]], gap, align))
            b1 += 1
        lay = engine.BatchLayout(lens[order[b0:b1]], gap, align)
        rv = torch.from_numpy(lay.row_valid()).to(dev)
        x = torch.randn((lay.rows, model.in_dim), generator=gen, device=dev, dtype=torch.float32) * 3.0
        x *= rv[:, None].to(torch.float32)                        # gap rows are zero by contract
        x[:, feat:] = 0                                           # 23 MFCC dims live in a 24-column (16-B aligned) row
        batches.append(dict(x=x, rs=torch.from_numpy(lay.row_start).to(dev), rl=torch.from_numpy(lay.row_len).to(dev),
                            rv=rv, n=lay.nchunks, max_len=lay.max_len, lo=b0, hi=b1, rows=lay.rows,
                            frames=int(lay.row_len.sum()), lay=lay))
        b0 = b1
    return order, batches


def _mfma_units(model, topo, feat, frames, n_utts):
    """MFMA-pipe work of one pass in bf16-MFMA FLOP units: a product costs 3 in the bf16x3 arithmetic (first layer, embed FC,
    every layer of a bf16x3 model), 2 in the f16bf8 arithmetic (one fp16 MFMA at the bf16 rate + one scaled 8-bit MFMA that
    executes 2 products at twice that rate), and is priced separately (157.3 TF) on the exact-fp32 path."""
    from xvector_amd import topology as tp
    prev, units = feat, 0.0
    pair8 = getattr(model, "pair8", None) is not None
    for i, (k, c) in enumerate(zip(topo["kernel_sizes"], topo["layer_sizes"])):
        in_f16bf8 = getattr(model, "f16bf8", False) and ("wp8" in model.layers[i] or (pair8 and i >= len(model.layers) - 2))
        units += 2.0 * k * prev * c * frames * (2 if in_f16bf8 else 3)
        prev = c
    return units + 3.0 * tp.flops_per_utt(topo) * n_utts


def _varlen_leg(args, model, weights, topo, dev, feat, with_oracle):
    """BASELINE configs[2]: T ~ U{25..10000} (one utterance of exactly 25 and one of exactly 10000 frames among them),
    length-bucketed batches of <= batch_rows rows, chunking at 10000 (every utterance is one chunk), resident in HBM: 1 warm-up
    + 2 timed passes; parity of the shortest and the longest utterance against the fp64 oracle."""
    import torch
    from xvector_amd import hiplib, topology as tp
    n = 3000
    rng = np.random.default_rng(25_10000)
    lens = rng.integers(25, 10001, size=n).astype(np.int64)
    lens[0], lens[1] = 25, 10000
    order, batches = _resident_batches(args, model, lens, dev, feat, 4242)
    frames = int(lens.sum())
    model.reserve(max(b["rows"] for b in batches), max(b["n"] for b in batches), max(b["max_len"] for b in batches))
    P = torch.empty((n, model.pooled_dim), dtype=torch.float32, device=dev)
    E = torch.empty((n, model.embed_dim), dtype=torch.float32, device=dev)
    steps = 2
    ev = [[[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in batches] for _ in range(steps + 1)]

    def one(si):
        for bi, b in enumerate(batches):
            model.frame_level(b["x"], b["rs"], b["rl"], b["rv"], b["n"], b["max_len"], P[b["lo"]:b["hi"]], events=ev[si][bi])
        model.segment_level(P, E)
    one(0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for si in range(1, steps + 1):
        one(si)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    t_g = sum(e[0].elapsed_time(e[1]) for si in range(1, steps + 1) for e in ev[si]) * 1e-3 / steps
    fl = tp.flops_per_frame(topo, feat) * frames
    if model.precision == "fp32":
        frac = fl / t_g / MFMA_F32_PEAK
    else:
        frac = (_mfma_units(model, topo, feat, frames, n) - 3.0 * tp.flops_per_utt(topo) * n) / t_g / MFMA_BF16_PEAK
    out = {"value": n / dt, "unit": "utt/s", "frames_per_s": frames / dt, "utterances": n, "frames": frames,
           "batches": len(batches), "ms_per_pass": dt * 1e3, "passes": steps, "algorithmic_tflops": (fl + tp.flops_per_utt(topo) * n) / dt / 1e12,
           "frac": frac,
           "workload": "BASELINE configs[2]: %d utterances, T ~ U{25..10000} incl. T = 25 and T = 10000, length-bucketed batches of <= %d "
                       "rows, one chunk per utterance (chunk size 10000)" % (n, args.batch_rows),
           "frac_note": "MFMA-pipe time of the frame-level launches at nominal rates / their HIP-event time (as roofline.frac)"}
    if with_oracle:
        from oracle import oracle
        pos = {int(u): p for p, u in enumerate(order.tolist())}
        got = E.cpu().numpy()
        par = {}
        for u in (0, 1):
            p_ = pos[u]
            b = next(b for b in batches if b["lo"] <= p_ < b["hi"])
            j = p_ - b["lo"]
            lay = b["lay"]
            m = b["x"][int(lay.row_start[j]):int(lay.row_start[j]) + int(lay.row_len[j]), :feat].cpu().numpy()
            ref = oracle.forward(m, weights, topo, np.float64)
            par["T=%d" % lens[u]] = oracle.rel_l2(got[p_], ref)
        out["parity_rel_l2_vs_fp64_oracle"] = par
    del batches
    return out


def _cli_job_leg(args, ark_path, scp_path, model_dir, n):
    """One ``extract_embedding.py`` worker job as a user of the reference's extract_xvectors.sh:72-89 would run it -- a fresh
    process under the package's launcher, scp in, ark,scp out, forced 1-rank RCCL group so that the exchange is on the path --
    timed from outside (wall) with the job's own breakdown (xvector_amd/jobclock.py).  Run twice: the first RCCL communicator
    on a box loads librccl's device code cold."""
    import re
    import shutil
    import subprocess
    import tempfile
    out_dir = tempfile.mkdtemp(prefix="xv_bench_cli_", dir=os.path.dirname(ark_path))
    env = dict(os.environ, XV_FORCE_DIST="1", HSA_ENABLE_IPC_MODE_LEGACY="0", XVECTOR_PRECISION=args.precision,
               PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "x-vector-kaldi-tf_amd"), os.environ.get("PYTHONPATH", "")]))
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR"):
        env.pop(k, None)
    runs = {}
    try:
        # in this order: the product default (RCCL, device code pre-loaded under `import torch`) on a box that has run nothing yet, the
        # same warm, RCCL without the pre-load (what rounds 1-4 ran), the gloo gather (round 5's default), shard files
        for name, backend, shard, prewarm in (("default_first", None, "gather", None), ("default", None, "gather", None),
                                              ("rccl_no_prewarm", "nccl", "gather", "0"), ("gloo", "gloo", "gather", None),
                                              ("files", None, "files", None)):
            o_ark, o_scp = os.path.join(out_dir, "xvector_%s.ark" % name), os.path.join(out_dir, "xvector_%s.scp" % name)
            env["XVECTOR_SHARD_OUTPUT"] = shard
            env.pop("XVECTOR_DIST_BACKEND", None)
            env.pop("XVECTOR_RCCL_PREWARM", None)
            if backend:
                env["XVECTOR_DIST_BACKEND"] = backend
            if prewarm is not None:
                env["XVECTOR_RCCL_PREWARM"] = prewarm
            cmd = [sys.executable, "-m", "xvector_amd.launch", "--nproc", "1",
                   os.path.join(ROOT, "x-vector-kaldi-tf_amd", "local", "tf", "extract_embedding.py"), "--use-gpu", "yes",
                   "--min-chunk-size", "25", "--chunk-size", "10000", "--feature-rspecifier", "scp:" + scp_path,
                   "--vector-wspecifier", "ark,scp:%s,%s" % (o_ark, o_scp), "--model-dir", model_dir]
            t0 = time.perf_counter()
            run = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
            wall = time.perf_counter() - t0
            log = run.stdout.decode(errors="replace")
            if run.returncode != 0:
                return {"error": log[-800:]}
            clock = [ln for ln in log.splitlines() if "Job wall clock:" in ln]
            parts = dict((k.strip(" ;["), float(v)) for k, v in re.findall(r"([^,;\[\]]+?) (\d+\.\d+) s", clock[-1].split("Job wall clock:", 1)[1])) if clock else {}
            with open(o_scp) as f:
                written = sum(1 for _ in f)
            group = [ln for ln in log.splitlines() if "process group (" in ln]
            runs[name] = {"wall_s": wall, "utt_per_s": n / wall, "vectors_written": written, "breakdown_s": parts,
                          "transport": re.search(r"process group \((\w+)\)", group[-1]).group(1) if group else None}
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)
    return {"value": runs["default"]["utt_per_s"], "unit": "utt/s", "utterances": n, "wall_s": runs["default"]["wall_s"],
            "transport": runs["default"]["transport"], "breakdown_s": runs["default"]["breakdown_s"],
            "first_job_on_this_box": runs["default_first"],
            "rccl_gather": dict(runs["default"], first_job=runs["default_first"],
                                note="the product default since round 6: ONE RCCL gather; the worker pre-loads RCCL's device code under "
                                     "`import torch` (xvector_amd/rccl_prewarm.py).  `first_job`: librccl cold in the box's page cache"),
            "rccl_without_prewarm": dict(runs["rccl_no_prewarm"], note="XVECTOR_RCCL_PREWARM=0 XVECTOR_DIST_BACKEND=nccl: the communicator's device "
                                         "code loaded when the group comes up (rounds 1-4)"),
            "gloo_gather": dict(runs["gloo"], note="XVECTOR_DIST_BACKEND=gloo: the gather of the host-resident vectors over TCP loopback "
                                                   "(round 5's default for payloads up to 512 MB)"),
            "shard_files": dict(runs["files"], note="XVECTOR_SHARD_OUTPUT=files: one ark per rank + a concatenated scp (the reference's "
                                                    "own protocol, extract_xvectors.sh:83-95), no process group"),
            "path": "python -m xvector_amd.launch --nproc 1 extract_embedding.py scp: -> ark,scp: (tmpfs), forced 1-rank group; wall clock of "
                    "the whole job from outside"}


def _job_rehearsal_leg(args, model_dir, feat, cli):
    """BASELINE configs[3] (8 ranks x 125 k utterances) rehearsed at its real job COUNTS on the one GPU of this box: a 1 M-line scp
    through the scp-sharded CLI (`extract_embedding.py` under the package's launcher, extract_xvectors.sh:63-95's twin), ONE gather of
    1 M [emitted? | x-vector] rows (2 GB) into rank 0, which writes the 1 M-record ark + scp.  What cannot be real here: the ranks share
    one GPU (gloo transport -- RCCL refuses two ranks on a device -- and every utterance is 25 frames so that the shared device is not
    what the job waits for), and they are 4 of 250 k utterances each rather than 8 of 125 k: beside this process (and a test runner
    above it) no more than six processes may hold one device.  So `extraction` of the breakdown is replaced by the measured single-rank
    time of a 125 k-utterance shard at T ~ U{200..400} (cli_job's extraction seconds per utterance) in `predicted_per_rank_job_s`.  The
    table's LINES, the KEYS and the RECORDS rank 0 gathers and writes are at their real size."""
    import re
    import shutil
    import subprocess
    import tempfile
    ranks, per_rank, T = int(os.environ.get("XV_BENCH_REHEARSAL_RANKS", "4")), int(os.environ.get("XV_BENCH_REHEARSAL_UTTS", "250000")), 25
    n = ranks * per_rank
    node_ranks = 8                                                    # the job rehearsed: configs[3], n utterances over 8 GPUs
    shm_ok = os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK)
    work = tempfile.mkdtemp(prefix="xv_bench_1m_", dir="/dev/shm" if shm_ok else None)
    try:
        t0 = time.perf_counter()
        rng = np.random.default_rng(99)
        pool = (rng.standard_normal((251, T, feat)) * 3.0).astype(np.float32).reshape(251, -1).view(np.uint8)
        keys = np.char.add(np.char.add("spk", np.char.zfill((np.arange(n) % 9973).astype(str), 5)),
                           np.char.add("-utt", np.char.zfill(np.arange(n).astype(str), 7))).astype("S19")
        head = b" \x00BFM \x04" + np.int32(T).tobytes() + b"\x04" + np.int32(feat).tobytes()
        rec_len = 19 + len(head) + T * feat * 4
        fpath, spath = os.path.join(work, "feats.ark"), os.path.join(work, "feats.scp")
        with open(fpath, "wb") as f:                                  # uniform records, 64 k at a time (the whole ark is 2.3 GB)
            for lo in range(0, n, 65536):
                hi = min(n, lo + 65536)
                rec = np.empty((hi - lo, rec_len), np.uint8)
                rec[:, :19] = keys[lo:hi].view(np.uint8).reshape(hi - lo, 19)
                rec[:, 19:19 + len(head)] = np.frombuffer(head, np.uint8)
                rec[:, 19 + len(head):] = pool[np.arange(lo, hi) % 251]
                f.write(rec.data)
        with open(spath, "w") as f:
            f.write("".join("%s %s:%d\n" % (k, fpath, 20 + i * rec_len) for i, k in enumerate(keys.astype(str).tolist())))
        t_make = time.perf_counter() - t0
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", XVECTOR_PRECISION=args.precision, XVECTOR_DIST_BACKEND="gloo",
                   XVECTOR_DEVICE="cuda:0", PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "x-vector-kaldi-tf_amd"), os.environ.get("PYTHONPATH", "")]))
        for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR", "XV_FORCE_DIST", "XVECTOR_SHARD_OUTPUT"):
            env.pop(k, None)
        if ranks == 1:
            env["XV_FORCE_DIST"] = "1"                                 # (a one-rank group: the same sharded path, nothing shared)
        o_ark, o_scp = os.path.join(work, "xvector.ark"), os.path.join(work, "xvector.scp")
        cmd = [sys.executable, "-m", "xvector_amd.launch", "--nproc", str(ranks),
               os.path.join(ROOT, "x-vector-kaldi-tf_amd", "local", "tf", "extract_embedding.py"), "--use-gpu", "yes",
               "--min-chunk-size", "25", "--chunk-size", "10000", "--feature-rspecifier", "scp:" + spath,
               "--vector-wspecifier", "ark,scp:%s,%s" % (o_ark, o_scp), "--model-dir", model_dir]
        t0 = time.perf_counter()
        # (its own session: a job that overruns is stopped as a GROUP -- the launcher's ranks must not outlive it on the GPU)
        job = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, start_new_session=True)
        try:
            raw, _ = job.communicate(timeout=240)
        except subprocess.TimeoutExpired:
            import signal
            os.killpg(job.pid, signal.SIGKILL)
            job.communicate()
            return {"error": "the %d-rank rehearsal did not finish within 240 s (stopped)" % ranks}
        wall = time.perf_counter() - t0
        log = raw.decode(errors="replace")
        if job.returncode != 0:
            return {"error": log[-800:]}
        clock = [ln for ln in log.splitlines() if "Job wall clock:" in ln]
        parts = dict((k.strip(" ;["), float(v)) for k, v in re.findall(r"([^,;\[\]]+?) (\d+\.\d+) s", clock[-1].split("Job wall clock:", 1)[1])) if clock else {}
        with open(o_scp) as f:
            written = sum(1 for _ in f)
        ark_gb = os.path.getsize(o_ark) / 1e9
    finally:
        shutil.rmtree(work, ignore_errors=True)
    out = {"ranks": ranks, "utterances": n, "frames_per_utterance": T,
           "transport": "gloo (%d ranks on ONE device; RCCL over xGMI on the node)" % ranks,
           "wall_s": wall, "vectors_written": written, "xvector_ark_gb": ark_gb, "breakdown_s_rank0": parts, "input_made_s": t_make,
           "note": "%d ranks share this box's GPU and its host cores: model load, probe and extraction run %d-fold contended; the "
                   "table's lines, the gathered rows and bytes and the records written are those of the whole job" % (ranks, ranks)}
    # What a rank of the real job waits for, piece by piece: the pieces that follow the job's COUNTS (the 1 M-line table, the gathered
    # bytes, the records written) from rank 0 here; the pieces that belong to a rank's own device (runtime, weights + probe, first
    # window, the extraction of 125 k utterances at T ~ U{200..400}) from cli_job's single-rank job on this box, where nothing shares it
    cj = (cli or {}).get("breakdown_s") or {}
    ext = [v for k, v in cj.items() if k.startswith("extraction")]
    if parts and ext and cli.get("utterances") and ranks > 1:
        own = {k: cj.get(k, 0.0) for k in ("interpreter + imports", "weights read", "import torch", "hip runtime up",
                                           "weights packed on the device + accuracy probe", "first window launched", "wait for the process group")}
        own["extraction (125 k utterances at cli_job's rate)"] = ext[0] * (n / node_ranks) / cli["utterances"]
        counts = {k: parts.get(k, 0.0) for k in ("tables opened", "gather", "write", "rename")}
        out["predicted_breakdown_s"] = {"from_this_rehearsal": counts, "from_cli_job_single_rank": own}
        out["predicted_per_rank_job_s"] = sum(counts.values()) + sum(own.values())
        out["predicted_8gpu_utt_per_s"] = n / out["predicted_per_rank_job_s"]
        out["prediction"] = ("per-rank job of the 8 x 125 k configuration = [tables opened (1 M-line scp, with `import torch` beside it), gather (2 GB "
                             "into rank 0; gloo over loopback here, RCCL over xGMI on the node), write (1 M records by rank 0), rename (+ the closing "
                             "barrier)] of rank 0 here + [runtime, weights + probe, first window, extraction scaled to 125 k utterances] of cli_job")
    return out


def _fp32_leg(args, weights, topo, dev, batches, n_utts, frames, feat, precision="fp32", oracle_check=None):
    """The same step on the exact-fp32 MFMA path (v_mfma_f32_32x32x2_f32: exact products, fp32 accumulate), 1 warm-up + 2
    timed passes over the resident batches -- what the bf16x3 default is traded against."""
    import torch
    from xvector_amd import engine, hiplib, topology as tp
    model = engine.DeviceModel(weights, topo, dev, precision=precision)
    model.reserve(max(b["rows"] for b in batches), max(b["n"] for b in batches), max(b["max_len"] for b in batches))
    P = torch.empty((n_utts, model.pooled_dim), dtype=torch.float32, device=dev)
    E = torch.empty((n_utts, model.embed_dim), dtype=torch.float32, device=dev)
    steps = 4
    ev = [[[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in batches] for _ in range(steps + 1)]

    def one(si):
        for bi, b in enumerate(batches):
            # the batches were laid out with the 8-row chunk alignment of the fused path: a valid layout for this path too
            model.frame_level(b["x"], b["rs"], b["rl"], b["rv"], b["n"], b["max_len"], P[b["lo"]:b["hi"]], events=ev[si][bi])
        model.segment_level(P, E)
    one(0)                                              # (warm-up: fresh activation buffers, clock ramp -- ~3 batches' worth)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    passes = []
    for si in range(1, steps + 1):
        t1 = time.perf_counter()
        one(si)
        torch.cuda.synchronize()
        passes.append((time.perf_counter() - t1) * 1e3)
    dt = (time.perf_counter() - t0) / steps
    t_g = sum(e[0].elapsed_time(e[1]) for si in range(1, steps + 1) for e in ev[si]) * 1e-3
    fl = tp.flops_per_frame(topo, feat) * frames
    out = {"value": n_utts / dt, "unit": "utt/s", "ms_per_step": dt * 1e3, "steps": steps, "passes_ms": [round(t, 2) for t in passes],
           "algorithmic_tflops": (fl + tp.flops_per_utt(topo) * n_utts) / dt / 1e12,
           "tdnn_gemm_tflops": fl * steps / t_g / 1e12, "frac": fl * steps / t_g / MFMA_F32_PEAK, "peak_tflops": MFMA_F32_PEAK / 1e12,
           "kernel": "tdnn_gemm_dma_kernel (layers 1-4: v_mfma_f32_32x32x2_f32 fed by buffer_load ... lds, bit-identical to tdnn_gemm_kernel, "
                     "which still runs layer 0: Cin = 24 is no whole 32-channel slab); the last layer reduced to 8-row block statistics in its "
                     "epilogue + stats_pool_blocks_kernel"}
    if precision == "fp32tc":
        # executed multiplications: a K-tap layer the Toom-Cook kernel takes runs (K + 1) / 2 products per row instead of K
        in_dims = [feat] + [int(c) for c in topo["layer_sizes"][:-1]]
        ex = 0.0
        for k, d, cin, cout in zip(topo["kernel_sizes"], topo["dilations"], in_dims, topo["layer_sizes"]):
            taps = (k + 1) / 2.0 if hiplib.toom_supported(int(k), int(d), int(cin), int(cout)) else float(k)
            ex += 2.0 * taps * cin * cout
        out.update({"dtype": "f32 (exact fp32 products and fp32 accumulation; the K = 5 / K = 7 layers as Toom-Cook F(2, K) over time: "
                             "not bit-identical to fp32_exact)",
                    "frac": ex * frames * steps / t_g / MFMA_F32_PEAK,
                    "algorithmic_over_peak": fl * steps / t_g / MFMA_F32_PEAK,
                    "frac_note": "frac = EXECUTED multiplications (what the MFMAs run) against the 157.3 TF fp32-MFMA peak; "
                                 "algorithmic_over_peak / tdnn_gemm_tflops count the ALGORITHMIC multiplications (2 K Cin Cout per frame): "
                                 "above 1 is possible because fewer are executed -- a speed-up over the direct form's ceiling, not a roofline fraction",
                    "executed_tflops": ex * frames * steps / t_g / 1e12, "executed_frac": ex * frames * steps / t_g / MFMA_F32_PEAK,
                    "executed_over_algorithmic_flops": ex / tp.flops_per_frame(topo, feat),
                    "kernel": "tdnn_gemm_toom_kernel<5>, <7> (layers 1, 2: 6 / 8 transformed products per row pair on v_mfma_f32_32x32x2_f32, "
                              "csrc/xv_toom.hip); layers 0 (rows form), 3, 4 (+ pooling epilogue): tdnn_gemm_k1_kernel (K = 1 on 16-channel slabs, three "
                              "workgroups per CU, csrc/xv_kernels.hip); FC as fp32_exact"})
    if oracle_check is not None:
        out["parity_rel_l2_max_vs_fp64_oracle"] = oracle_check(E)
    return out


def _bf16x3_leg(args, weights, topo, dev, batches, n_utts, frames, feat, order, oracle_check):
    """The same step with EVERY layer in the bf16x3 arithmetic (three bf16 MFMAs per product; the default of round 1 and the
    twin an out-of-range window of the f16bf8 default falls back to): 1 warm-up + 3 timed passes over the resident batches."""
    import torch
    from xvector_amd import engine, hiplib, topology as tp
    model = engine.DeviceModel(weights, topo, dev, precision="bf16x3")
    model.reserve(max(b["rows"] for b in batches), max(b["n"] for b in batches), max(b["max_len"] for b in batches))
    P = torch.empty((n_utts, model.pooled_dim), dtype=torch.float32, device=dev)
    E = torch.empty((n_utts, model.embed_dim), dtype=torch.float32, device=dev)
    steps = 3
    ev = [[[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in batches] for _ in range(steps + 1)]

    def one(si):
        for bi, b in enumerate(batches):
            model.frame_level(b["x"], b["rs"], b["rl"], b["rv"], b["n"], b["max_len"], P[b["lo"]:b["hi"]], events=ev[si][bi])
        model.segment_level(P, E)
    one(0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for si in range(1, steps + 1):
        one(si)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    t_g = sum(e[0].elapsed_time(e[1]) for si in range(1, steps + 1) for e in ev[si]) * 1e-3
    fl = tp.flops_per_frame(topo, feat) * frames
    out = {"value": n_utts / dt, "unit": "utt/s", "ms_per_step": dt * 1e3, "steps": steps,
           "algorithmic_tflops": (fl + tp.flops_per_utt(topo) * n_utts) / dt / 1e12,
           "frac": 3 * fl * steps / t_g / MFMA_BF16_PEAK,
           "kernel": "tdnn_first_kernel + tdnn_gemm_bf16x3_kernel + tdnn_pair_pool_kernel (3 bf16 MFMAs per product); frac = executed "
                     "bf16 FLOPs / 2.5 PF"}
    if oracle_check is not None:
        out["parity_rel_l2_max_vs_fp64_oracle"] = oracle_check(E)
    return out


def _e2e_leg(args, weights, topo, feat, with_cli):
    """ark bytes in RAM -> Model.make_embedding (reader thread, native packer, H2D, kernels, D2H, writer thread) -> ark bytes:
    the PCIe- and parsing-inclusive rate of the drop-in entry point, model load included.  Returns (e2e record, cli_job record
    or None): the same features, as an ark + scp on tmpfs, also go through one worker job of the CLI."""
    import io
    import logging
    import shutil
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "x-vector-kaldi-tf_amd", "local", "tf"))
    import kaldi_io
    import models
    from xvector_amd import synthetic
    n = args.e2e_utts
    lens = synthetic.utterance_lengths(n, args.tmin, args.tmax, 4321)
    rng = np.random.default_rng(4321)
    pool = [(rng.standard_normal((args.tmax, feat)) * 3.0).astype(np.float32) for _ in range(257)]
    shm_ok = os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK)
    work = tempfile.mkdtemp(prefix="xv_bench_e2e_", dir="/dev/shm" if shm_ok else None)
    fpath, spath = os.path.join(work, "feats.ark"), os.path.join(work, "feats.scp")
    with kaldi_io.TableWriter(fpath, spath) as tw:
        for i in range(n):
            kaldi_io.write_mat(tw, pool[i % 257][:lens[i]], key="utt%07d" % i)
    with open(fpath, "rb") as f:
        data = f.read()
    tmp = os.path.join(work, "nnet")
    log = logging.getLogger("bench_e2e")
    log.addHandler(logging.NullHandler())
    log.propagate = False
    cli = None
    try:
        models.Model.save_model(dict(weights=weights, topology=topo, model_class="ModelWithoutDropout", num_classes=64, feat_dim=feat),
                                tmp, None)
        best, passes = None, []
        for _ in range(4):                                         # the first pass also pins the staging buffers and faults the read arenas in
            out = io.BytesIO()
            t0 = time.perf_counter()
            model = models.Model()
            model.make_embedding(io.BytesIO(data), out, tmp, 25, 10000, True, log)
            dt = time.perf_counter() - t0
            passes.append(dt)
            best = dt if best is None else min(best, dt)
        stats = getattr(model, "last_stats", {})
        nvec = out.getbuffer().nbytes // (len("utt0000000") + 1 + 2 + 3 + 1 + 4 + 512 * 4)
        # the same ark as a FILE in RAM (tmpfs): read() of a file releases the interpreter lock, the memcpy out of a BytesIO does
        # not -- this is what `extract_embedding.py ark:feats.ark ...` on a page-cached file sees
        fbest = None
        for _ in range(3):
            out = io.BytesIO()
            t0 = time.perf_counter()
            with open(fpath, "rb", buffering=0) as f:
                models.Model().make_embedding(f, out, tmp, 25, 10000, True, log)
            dt = time.perf_counter() - t0
            fbest = dt if fbest is None else min(fbest, dt)
        shm = {"value": n / fbest, "unit": "utt/s", "seconds": fbest, "input": "the same ark as a file on %s" % ("tmpfs (/dev/shm)" if shm_ok else "disk")}
        try:
            comp = _compressed_leg(kaldi_io, models, n, lens, feat, tmp, log)
        except Exception as e:                                     # a sub-record must not take the line down
            comp = {"error": repr(e)}
        if with_cli:
            try:
                cli = _cli_job_leg(args, fpath, spath, tmp, n)
            except Exception as e:                                 # a sub-record must not take the line down
                cli = {"error": repr(e)}
            if "error" not in cli and not args.no_job_rehearsal:
                try:
                    cli["rehearsal_8x125k"] = _job_rehearsal_leg(args, tmp, feat, cli)
                except Exception as e:
                    cli["rehearsal_8x125k"] = {"error": repr(e)}
    finally:
        shutil.rmtree(work, ignore_errors=True)
    res = {"value": n / best, "unit": "utt/s", "utterances": n, "vectors_written": int(nvec), "seconds": best,
           "ark_gb_in": len(data) / 1e9, "ark_gb_per_s": len(data) / 1e9 / best,
           "run_time_accuracy_probe": {k: stats.get(k) for k in ("probe_windows", "probe_rel_l2_max", "demoted") if k in stats},
           "passes_s": passes,
           "path": "ark bytes in host RAM (io.BytesIO) -> Model.make_embedding(min_chunk 25, chunk 10000) -> ark bytes in host RAM, "
                   "incl. Kaldi parsing, packing, H2D, D2H, FV serialisation and the run-time accuracy probe; best of 4 passes in one "
                   "process.  The FIRST pass (passes_s[0]) also loads the model (weights packed on the device, load-time accuracy "
                   "probe), pins the staging buffers and faults the read arenas in; later calls of the same process re-use the loaded "
                   "model of the same checkpoint (XVECTOR_MODEL_CACHE=0 turns that off)",
           "from_tmpfs_file": shm, "compressed_input": comp}
    return res, cli


def _compressed_leg(kaldi_io, models, n, lens, feat, model_dir, log):
    """The same number of utterances as Kaldi's DEFAULT feature records -- CompressedMatrix, "CM ": what steps/make_mfcc.sh writes and a
    feats.scp points at -- through the same entry point: the in-place reader decodes them natively (xv_ark_decode_cm).  Synthetic
    records (random bytes on the format's piecewise-linear scale, increasing per-column percentiles); the x-vectors of a sample are
    compared, byte for byte, with those of the same matrices decoded by the generic reader and stored as plain float matrices."""
    import io
    import struct
    rng = np.random.default_rng(99)
    recs = []
    for j in range(257):
        rows = int(lens[j % len(lens)])
        q = np.sort(rng.integers(2000, 63000, size=(feat, 4)), axis=1).astype(np.uint16) + np.arange(4, dtype=np.uint16)[None, :]
        recs.append(b" \0BCM " + struct.pack("<ffii", -10.0, 20.0, rows, feat) + q.tobytes() +
                    rng.integers(0, 256, size=(feat, rows), dtype=np.uint8).tobytes())
    data = b"".join(("utt%07d" % i).encode() + recs[i % 257] for i in range(n))
    best = None
    for _ in range(3):
        out = io.BytesIO()
        t0 = time.perf_counter()
        models.Model().make_embedding(io.BytesIO(data), out, model_dir, 25, 10000, True, log)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    nvec = out.getbuffer().nbytes // (len("utt0000000") + 1 + 2 + 3 + 1 + 4 + 512 * 4)
    sample = b"".join(("utt%07d" % i).encode() + recs[i] for i in range(257))
    plain = io.BytesIO()
    for key, m in kaldi_io.read_mat_ark(io.BytesIO(sample)):
        kaldi_io.write_mat(plain, m, key=key)
    o1, o2 = io.BytesIO(), io.BytesIO()
    models.Model().make_embedding(io.BytesIO(sample), o1, model_dir, 25, 10000, True, log)
    models.Model().make_embedding(io.BytesIO(plain.getvalue()), o2, model_dir, 25, 10000, True, log)
    return {"value": n / best, "unit": "utt/s", "seconds": best, "vectors_written": int(nvec), "ark_gb_in": len(data) / 1e9,
            "same_bytes_as_plain_float_input": bool(o1.getvalue() == o2.getvalue() and len(o1.getvalue()) > 0),
            "input": "Kaldi CompressedMatrix records (\"CM \", one byte per element) in host RAM"}


def main():
    args = parse()
    # `python bench.py --gpus N` (N > 1) outside a launcher: start the N ranks ourselves -- one process per GPU, the environment
    # contract of torch.distributed.run (xvector_amd/launch.py) -- and leave with the job's exit code
    from xvector_amd import launch
    rc = launch.relaunch_self_as_ranks(args.gpus)
    if rc is not None:
        raise SystemExit(rc)
    import torch
    import torch.distributed as dist
    from xvector_amd import dist as xdist, engine, hiplib, synthetic, topology as tp

    world_env = int(os.environ.get("WORLD_SIZE", "1"))
    if world_env != args.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d" % (args.gpus, world_env))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    visible = torch.cuda.device_count()
    if os.environ.get("XV_BENCH_SHARE_GPU") == "1" and visible > 0:
        # test mode (with XVECTOR_DIST_BACKEND=gloo): the N ranks share the GPUs that exist -- the control flow of an N-rank run
        # (launcher, group, sharded workload, gather, max-over-ranks timing) on a one-GPU box; the number it prints means nothing
        local = local % visible
    elif visible < args.gpus or local >= visible:
        raise SystemExit("bench.py: %d GPUs requested, %d visible" % (args.gpus, visible))
    rank, world = xdist.init_process_group()
    hiplib.require_gpu()
    dev = torch.device("cuda:%d" % local)
    torch.cuda.set_device(dev)

    topo = tp.get("ModelWithoutDropout")
    feat = 23
    if args.mode == "train":
        return bench_train(args, rank, world, dev, topo, feat)
    weights = synthetic.trained_like(topo, feat, seed=1)
    if args.no_fused_pool:
        model = engine.DeviceModel(weights, topo, dev, precision=args.precision, fused_pool=False)
    else:
        # the arithmetic is admitted per checkpoint (load-time accuracy probe, engine.select_model); what was measured goes into
        # the line.  A model the probe moved off f16bf8 would run -- and be reported -- in the arithmetic it was moved to.
        model = engine.select_model(weights, topo, dev, precision=args.precision)
    selection = dict(getattr(model, "selection", None) or {})

    # ---- synthetic workload resident in HBM: ragged batches in kernel layout -------------------
    lens = synthetic.utterance_lengths(args.utts, args.tmin, args.tmax, 1234 + rank)
    order, batches = _resident_batches(args, model, lens, dev, feat, 1234 + rank)
    n_utts = len(order)
    frames = int(lens.sum())
    model.reserve(max(b["rows"] for b in batches), max(b["n"] for b in batches), max(b["max_len"] for b in batches))
    E_all = torch.empty((n_utts, model.embed_dim), dtype=torch.float32, device=dev)
    P_all = torch.empty((n_utts, model.pooled_dim), dtype=torch.float32, device=dev)
    seg = torch.arange(n_utts + 1, dtype=torch.int32, device=dev)              # one chunk per utterance (T < 10000)
    clen = torch.from_numpy(lens[order].astype(np.int32)).to(dev)
    xvec = torch.empty_like(E_all)
    counts = [n_utts] * world

    n_steps_total = args.warmup + args.steps
    ev = [[[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in batches] for _ in range(n_steps_total)]
    ev_fc = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(n_steps_total)]
    ev_g = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(n_steps_total)]

    def step(si):
        for bi, b in enumerate(batches):
            model.frame_level(b["x"], b["rs"], b["rl"], b["rv"], b["n"], b["max_len"], P_all[b["lo"]:b["hi"]], events=ev[si][bi])
        ev_fc[si][0].record()
        model.segment_level(P_all, E_all)                 # embed_layer-0 once over all chunks of the step
        ev_fc[si][1].record()
        hiplib.chunk_average(E_all, seg, clen, n_utts, xvec)
        if dist.is_initialized():
            ev_g[si][0].record()
            got = xdist.gather_blocks(xvec, counts, 0)
            ev_g[si][1].record()
            return got
        return [xvec]

    def fence():
        torch.cuda.synchronize()
        if dist.is_initialized():
            dist.barrier()
        torch.cuda.synchronize()

    for si in range(args.warmup):
        step(si)
    import gc
    gc.collect()
    gc.disable()                             # (no 40 ms collector pause inside the timed region; see _train_run)
    fence()
    t0 = time.perf_counter()
    last = None
    for si in range(args.warmup, n_steps_total):
        last = step(si)
    fence()
    dt = time.perf_counter() - t0
    gc.enable()
    if dist.is_initialized():
        tmax = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax.item())
        dist.barrier()                       # the ranks part here: everything below is rank 0's own post-processing
    if args.dump_outputs and rank == 0:
        # the x-vectors of the last timed step in utterance order (rank r's block: its seeded set of --utts utterances; the
        # step ran them in length-sorted order)
        blocks = []
        for r, blk in enumerate(last):
            order_r = np.argsort(synthetic.utterance_lengths(args.utts, args.tmin, args.tmax, 1234 + r), kind="stable")
            v = np.empty((len(order_r), blk.shape[1]), np.float32)
            v[order_r] = blk.cpu().numpy()
            blocks.append(v)
        _dump_outputs(args.dump_outputs, {"xvectors": np.concatenate(blocks)})

    # ---- per-kernel time from the HIP events recorded inside the timed region ------------------
    t_gemm = t_pool = 0.0
    for si in range(args.warmup, n_steps_total):
        for bi in range(len(batches)):
            e = ev[si][bi]
            t_gemm += e[0].elapsed_time(e[1])
            t_pool += e[1].elapsed_time(e[2])
        t_gemm += ev_fc[si][0].elapsed_time(ev_fc[si][1])
    t_gemm, t_pool = t_gemm * 1e-3, t_pool * 1e-3
    fl_gemm = (tp.flops_per_frame(topo, feat) * frames + tp.flops_per_utt(topo) * n_utts) * args.steps
    paired = getattr(model, "pair", None) is not None
    launches_per_batch = len(model.layers) - (1 if paired else 0)
    n_gemm_launch = (launches_per_batch * len(batches) + 1) * args.steps
    C = topo["layer_sizes"][-1]
    by_pool = (4 * C * frames + 4 * 2 * C * n_utts) * args.steps
    pool_kernel, pool_launches = "stats_pool_kernel", len(batches) * args.steps
    t_blocks = t_pool
    if model.fused_pool and args.full:
        # the timed path reduces the last layer inside the GEMM epilogue; the standalone pooling kernel (attention-free models without the fused epilogue, training)
        # is timed here, outside the timed region, on a materialised [rows, 1536] fp32 activation of the largest batch
        pool_kernel = "stats_pool_kernel (standalone, measured outside the timed region: the timed path reduces the last layer " \
                      "to 8-row block statistics in the GEMM epilogue + stats_pool_blocks_kernel)"
        big = max(batches, key=lambda b: b["rows"])
        hbuf = torch.randn((big["rows"], C), device=dev, dtype=torch.float32)
        pout = torch.empty((big["n"], 2 * C), device=dev, dtype=torch.float32)
        need = hiplib.stats_pool_workspace_bytes(C, big["n"], big["max_len"], 512)
        ws = torch.empty((need + 3) // 4, device=dev, dtype=torch.float32) if need else None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = 10
        for i in range(reps + 2):
            if i == 2:
                e0.record()
            hiplib.stats_pool(hbuf, big["rs"], big["rl"], big["n"], big["max_len"], 512, tp.VAR2STD_EPSILON, pout, ws)
        e1.record()
        torch.cuda.synchronize()
        t_pool = e0.elapsed_time(e1) * 1e-3
        by_pool = (4 * C * big["frames"] + 4 * 2 * C * big["n"]) * reps
        pool_launches = reps
        del hbuf
    fl_total = (tp.flops_per_frame(topo, feat) * frames + tp.flops_per_utt(topo) * n_utts)

    if rank != 0:
        if dist.is_initialized():
            dist.destroy_process_group()
        return

    traffic, traffic_src = _traffic(args.batch_rows)
    if model.precision == "fp32":
        kern = {"kernel": "tdnn_gemm_kernel<true> (5 TDNN layers per batch + embed FC per step)",
                "peak": MFMA_F32_PEAK / 1e12, "frac": fl_gemm / t_gemm / MFMA_F32_PEAK,
                "peak_note": "fp32-input MFMA (v_mfma_f32_32x32x2_f32) dense peak"}
    elif getattr(model, "f16bf8", False):
        # MFMA time a product costs, in bf16-MFMA units: 3 in the bf16x3 arithmetic (first layer, pair kernel, embed FC);
        # 2 in the f16bf8 arithmetic (one fp16 MFMA at the bf16 rate + one scaled 8-bit MFMA that executes 2 products at
        # twice that rate).  frac = MFMA-pipe time at nominal rates / measured kernel time.
        pair8 = getattr(model, "pair8", None) is not None
        units = _mfma_units(model, topo, feat, frames, n_utts) * args.steps
        kern = {"kernel": "tdnn_first_kernel (layer 0, bf16x3) + tdnn_gemm_f16bf8_wide16_kernel (layers 1-2: fp16 MFMA + scaled bf8 MFMA "
                          "per product on the 16 x 16 shapes, v_mfma_f32_16x16x32_f16 + v_mfma_scale_f32_16x16x128_f8f6f4) + %s (layers 3+4 chained in registers, pooling statistics in its "
                          "epilogue) per batch, embed FC (bf16x3) per step" %
                          ("tdnn_pair_pool_f16bf8_kernel" if pair8 else "tdnn_pair_pool_kernel (bf16x3)"),
                "peak": fl_gemm / (units / MFMA_BF16_PEAK) / 1e12, "frac": units / t_gemm / MFMA_BF16_PEAK,
                "executed_bf16_equivalent_tflops": units / t_gemm / 1e12,
                "peak_note": "achieved = ALGORITHMIC (fp32-contraction) FLOPs.  A product costs 3 bf16 MFMAs in the bf16x3 kernels "
                             "and 1 fp16 MFMA + 2 products of a scaled 8-bit MFMA at twice the rate (= 2 bf16-MFMA times) in the "
                             "f16bf8 kernels; peak = algorithmic FLOPs / (MFMA-pipe time at 2.5 PF bf16 / 5 PF fp8 dense), "
                             "frac = that pipe time / measured kernel time"}
    else:
        kern = {"kernel": ("tdnn_gemm_bf16x3_kernel (layers 0-2) + tdnn_pair_pool_kernel (layers 3+4 chained in registers, pooling "
                           "statistics in its epilogue) per batch, embed FC per step" if paired else
                           "tdnn_gemm_bf16x3_kernel (5 TDNN layers per batch + embed FC per step)"),
                "peak": MFMA_BF16_PEAK / 3 / 1e12, "frac": 3 * fl_gemm / t_gemm / MFMA_BF16_PEAK,
                "executed_bf16_tflops": 3 * fl_gemm / t_gemm / 1e12,
                "peak_note": "achieved = ALGORITHMIC (fp32-contraction) FLOPs; every product costs 3 bf16 MFMAs, so "
                             "peak = 2.5 PFLOP/s dense bf16 MFMA / 3 and frac = executed bf16 FLOPs / 2.5 PF"}
    if args.full and getattr(model, "f16bf8", False):
        # per-launch breakdown from a few more (untimed) passes over the largest batch: HIP events between the launches
        big = max(batches, key=lambda b: b["rows"])
        passes = []
        for _ in range(6):
            marks = []
            model._frame_level_f16bf8(big["x"], big["rows"], big["rv"], model.status, marks)
            passes.append(marks)
        torch.cuda.synchronize()
        marks = passes[-1]
        prev_c, by = feat, []
        fl_layer = []
        for k, c in zip(topo["kernel_sizes"], topo["layer_sizes"]):
            fl_layer.append(2.0 * k * prev_c * c * big["frames"])
            prev_c = c
        spans = [(lab, float(np.median([pm[i][1].elapsed_time(pm[i + 1][1]) for pm in passes[1:]])) * 1e-3)
                 for i, (lab, ev) in enumerate(marks[1:])]
        n_l = len(model.layers)
        groups = [[0]] + [[i] for i in range(1, n_l - 2 if model.pair is not None else n_l - 1)] + \
                 ([[n_l - 2, n_l - 1]] if model.pair is not None else [[n_l - 1]])
        for (lab, t), idx in zip(spans, groups):
            cost = 2 if (idx[0] > 0 and (("wp8" in model.layers[idx[0]]) or getattr(model, "pair8", None) is not None)) else 3
            fl = sum(fl_layer[i] for i in idx)
            by.append({"launch": lab, "ms": t * 1e3, "algorithmic_tflops": fl / t / 1e12, "mfma_time_over_time": cost * fl / t / MFMA_BF16_PEAK})
        kern["by_launch"] = by
        kern["by_launch_note"] = "median of 5 extra passes over the largest batch (%d rows), HIP events between the launches" % big["rows"]
    out = {
        "metric": "utterances/sec (= x-vectors/sec, 512-d) on synthetic 23-dim MFCC, T~U[200,400]",
        "value": n_utts * world * args.steps / dt,
        "unit": "utt/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": dt / args.steps * 1e3,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": ("f32" if model.precision == "fp32" else
                  "f32 in/out, f32 accumulate; GEMM products as fp16 MFMA + 2^-11 x scaled bf8 MFMA of the cross terms (layers 1-4) "
                  "and bf16x3 split MFMA (layer 0, FC)" if getattr(model, "f16bf8", False) else
                  "f32 in/out, GEMMs as bf16x3 split MFMA (hi*hi+hi*lo+lo*hi) with f32 accumulate"),
        "data": "synthetic",
        "config": {"workload": "BASELINE configs[1]: %d utts/GPU, 23-dim MFCC, T~U{%d..%d}, default x-vector topology "
                               "[512,512,512,512,1536] k=[5,5,7,1,1], 512-d embed_layer-0" % (n_utts, args.tmin, args.tmax),
                   "utts_per_gpu": n_utts, "frames_per_gpu": frames, "batches_per_step": len(batches),
                   "batch_rows": args.batch_rows, "precision": selection.get("selected", args.precision),
                   "precision_requested": args.precision, "fused_pool": bool(model.fused_pool),
                   "pair_kernel": paired, "dist_initialized": bool(dist.is_initialized()),
                   "parallelism": ("one rank holds every utterance: no exchange at N = 1" if world == 1 else
                                   "utterance-sharded x%d, one %s gather per step" % (world, "RCCL (nccl backend over xGMI)" if dist.get_backend() == "nccl"
                                                                                       else dist.get_backend() + " (TEST MODE, ranks share a GPU)"))},
        "frames_per_s": frames * world * args.steps / dt,
        "algorithmic_tflops": fl_total * world * args.steps / dt / 1e12,
        "roofline": dict({"bound": "mfma", "achieved": fl_gemm / t_gemm / 1e12, "unit": "TFLOP/s", "traffic": traffic,
                          "traffic_source": traffic_src,
                          "avg_launch_ms": t_gemm / n_gemm_launch * 1e3, "launches": n_gemm_launch,
                          "algorithmic_gflop_per_launch": fl_gemm / n_gemm_launch / 1e9,
                          # how many times the fp32-MFMA ceiling (157.3 TF: what exact fp32 products could reach at most) the
                          # algorithmic rate is -- a speed-up over that ceiling, not a roofline fraction
                          "algorithmic_rate_over_fp32_mfma_ceiling": fl_gemm / t_gemm / MFMA_F32_PEAK}, **kern),
    }
    if not model.fused_pool or args.full:                   # (behind the fused epilogue the standalone kernel is timed by --full alone)
        out["roofline_pool"] = {"kernel": pool_kernel, "bound": "hbm", "achieved": by_pool / t_pool / 1e9,
                                "peak": HBM_PEAK / 1e9, "unit": "GB/s", "frac": by_pool / t_pool / HBM_PEAK,
                                "avg_launch_ms": t_pool / pool_launches * 1e3,
                                "algorithmic_mb_per_launch": by_pool / pool_launches / 1e6}
    out["accuracy_probe"] = dict(selection, note="engine.select_model: x-vectors of a fixed MFCC-like batch through these weights in "
                                 "f16bf8 vs bf16x3 (kept when <= f16bf8_limit), then bf16x3 vs exact fp32 if that failed")
    out["rccl_ranks"] = dist.get_world_size() if dist.is_initialized() else 0
    if dist.is_initialized():
        g = [ev_g[si][0].elapsed_time(ev_g[si][1]) for si in range(args.warmup, n_steps_total)]
        out["gather_ms"] = float(np.mean(g))
        out["gather_note"] = "HIP-event time of xdist.gather_blocks (ONE dist.gather of the [%d, %d] fp32 blocks to rank 0) per step, " \
                             "rank 0's stream" % (n_utts, model.embed_dim)
    if model.fused_pool:
        rows_total = sum(b["rows"] for b in batches)
        by_blk = ((rows_total + 7) // 8 * 2 * C * 4 + 4 * 2 * C * n_utts) * args.steps
        out["pool_blocks"] = {"kernel": "stats_pool_blocks_kernel", "bound": "hbm", "achieved": by_blk / t_blocks / 1e9,
                              "unit": "GB/s", "frac": by_blk / t_blocks / HBM_PEAK,
                              "avg_launch_ms": t_blocks / (len(batches) * args.steps) * 1e3}
    if not args.full:
        # a plain run ends here: the headline and what its own timed region measured
        print(json.dumps(out))
        if dist.is_initialized():
            dist.destroy_process_group()
        return

    if args.cpu_budget > 0:
        from oracle import oracle
        # parity check (oracle as the checker): utterances spread evenly over ALL batches of the step (positions in the
        # length-sorted order: the shortest and the longest utterance of the workload are among them)
        picks = sorted(set(np.linspace(0, n_utts - 1, max(2, args.parity_utts)).astype(int).tolist()))
        refs = []
        for p_ in picks:
            b = next(b for b in batches if b["lo"] <= p_ < b["hi"])
            j, lay = p_ - b["lo"], b["lay"]
            m = b["x"][int(lay.row_start[j]):int(lay.row_start[j]) + int(lay.row_len[j]), :feat].cpu().numpy()
            refs.append(oracle.embed_utterance(m, weights, topo, 25, 10000, np.float64))

        def parity_check(vectors):                     # vectors[p] = x-vector of the utterance at sorted position p
            got = vectors.cpu().numpy()
            return max(oracle.rel_l2(got[p_], r) for p_, r in zip(picks, refs))
        out["parity_utterances"] = len(picks)
        out["parity_batches_covered"] = len(set(next(i for i, b in enumerate(batches) if b["lo"] <= p_ < b["hi"]) for p_ in picks))
        out["parity_rel_l2_max_vs_fp64_oracle"] = parity_check(xvec)
    if args.cpu_budget > 0 and world == 1:
        from oracle import oracle, torch_ref
        sample_lens = synthetic.utterance_lengths(32, args.tmin, args.tmax, 1234)
        rng = np.random.default_rng(99)
        mats = [(rng.standard_normal((int(T), feat)) * 3.0).astype(np.float32) for T in sample_lens]
        logical, granted = os.cpu_count() or 1, torch_ref.effective_cores()
        # (i) one process, a few thread counts (2 = the reference's TF session config, local/tf/models.py:361-363): batch-1
        #     forwards do not scale to hundreds of threads;  (ii) the reference's deployment: nj processes x 2 threads
        #     (run.sh:229-247 -> extract_xvectors.sh:83-88) on every core this container is granted
        sweep = sorted(set(t for t in (2, 8, 32) if t <= max(2, granted)))
        share = args.cpu_budget / (len(sweep) + 2.0)
        res = {t: torch_ref.time_baseline(weights, topo, mats, t, max(1.5, share)) for t in sweep}
        best = max(res, key=lambda t: res[t][0])
        nproc = max(1, min(granted // 2, 64))
        dep_rate, dep_each = torch_ref.time_baseline_processes(weights, topo, mats, nproc, 2, max(2.0, 2 * share))
        # the port itself against the fp64 oracle ("CPU(fp32)-vs-fp64 oracle"), on two utterances of the sample
        port = torch_ref.TorchCpuModel(weights, topo)
        port_err = max(oracle.rel_l2(port.forward(m), oracle.forward(m, weights, topo, np.float64)) for m in mats[:2])
        gflop_per_utt = (tp.flops_per_frame(topo, feat) * float(np.mean(sample_lens)) + tp.flops_per_utt(topo)) / 1e9
        top_rate, top_cores = (dep_rate, 2 * nproc) if dep_rate > res[best][0] else (res[best][0], best)
        out["cpu_baseline"] = {"value": top_rate, "unit": "utt/s", "cores": top_cores, "kind": "port",
                               "gflops": top_rate * gflop_per_utt, "port_rel_l2_vs_fp64_oracle": port_err,
                               "sample": "torch-CPU fp32 (oneDNN) port of the reference forward, batch 1 per utterance as "
                                         "local/tf/models.py:401-414 runs it; a 32-utterance slice of the same length "
                                         "distribution cycled for %.1f s per single-process thread count %s and %.1f s for the "
                                         "all-cores deployment shape; value = the better of the two; host shows %d logical cores, "
                                         "the container is granted %d" % (max(1.5, share), sweep, max(2.0, 2 * share), logical, granted),
                               "by_threads": {str(t): res[t][0] for t in sweep},
                               "reference_faithful_2_threads": res.get(2, (None,))[0],
                               "all_cores": {"value": dep_rate, "unit": "utt/s", "processes": nproc, "threads_per_process": 2,
                                             "cores": 2 * nproc, "host_logical_cores": logical, "container_granted_cores": granted,
                                             "shape": "nj independent extractor processes x 2 intra-op threads, as run.sh:229-247 / "
                                                      "extract_xvectors.sh:83-88 deploy the reference (models.py:361-363)"}}
    if world == 1 and model.precision != "fp32" and not args.no_fp32_leg:
        out["fp32_exact"] = _fp32_leg(args, weights, topo, dev, batches, n_utts, frames, feat, "fp32",
                                      parity_check if args.cpu_budget > 0 else None)
        out["fp32_toomcook"] = _fp32_leg(args, weights, topo, dev, batches, n_utts, frames, feat, "fp32tc",
                                         parity_check if args.cpu_budget > 0 else None)
        if getattr(model, "f16bf8", False):
            out["bf16x3"] = _bf16x3_leg(args, weights, topo, dev, batches, n_utts, frames, feat, order,
                                        parity_check if args.cpu_budget > 0 else None)
    # ---- BASELINE configs[3] asks for the rate "incl. and excl. ark write": rank 0 writes the gathered x-vectors of ONE step
    #      as a Kaldi ark + scp (outside the timed region; `value` excludes it, `with_ark_write` folds its time into a step)
    if last is not None:
        import shutil
        import tempfile
        sys.path.insert(0, os.path.join(ROOT, "x-vector-kaldi-tf_amd", "local", "tf"))
        import kaldi_io
        tmp = tempfile.mkdtemp(prefix="xv_bench_")
        try:
            tw0 = time.perf_counter()
            host = torch.cat([b for b in last], dim=0).cpu().numpy()
            keys = ["utt%07d" % i for i in range(host.shape[0])]
            with kaldi_io.TableWriter(os.path.join(tmp, "xvector.ark"), os.path.join(tmp, "xvector.scp")) as tw:
                kaldi_io.write_vec_flt_batch(tw, keys, host)
            tw1 = time.perf_counter() - tw0
            out["with_ark_write"] = {"ark_write_s_per_step": tw1, "ark_mb": os.path.getsize(os.path.join(tmp, "xvector.ark")) / 1e6,
                                     "value_incl_write": n_utts * world / (dt / args.steps + tw1), "unit": "utt/s",
                                     "note": "D2H of the gathered [N,512] block + Kaldi ark,scp write by rank 0, serial after the step"}
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    extra = world == 1 and not args.no_extra_legs and model.precision != "fp32"
    if extra:
        # BASELINE configs[2] and configs[4] at one rank's share, time-boxed: a couple of passes / ten steps each
        try:
            out["config2_varlen"] = _varlen_leg(args, model, weights, topo, dev, feat, args.cpu_budget > 0)
        except Exception as e:                                     # a sub-record must not take the line down
            out["config2_varlen"] = {"error": repr(e)}
    if world == 1 and args.e2e_utts > 0 and model.precision != "fp32":
        del batches, E_all, P_all
        os.environ["XVECTOR_PRECISION"] = args.precision          # Model.load_model reads it
        e2e, cli = _e2e_leg(args, weights, topo, feat, extra)
        e2e["fraction_of_resident_rate"] = e2e["value"] / out["value"]
        if "from_tmpfs_file" in e2e:
            e2e["from_tmpfs_file"]["fraction_of_resident_rate"] = e2e["from_tmpfs_file"]["value"] / out["value"]
        out["e2e_ark_to_ark"] = e2e
        if cli is not None:
            out["cli_job"] = cli
    if extra:
        try:
            torch.cuda.empty_cache()
            tr = {}
            for prec in ("fp32", "bf16x3"):
                tr[prec] = _train_run(args, 0, 1, dev, tp.get("ModelWithoutDropout"), feat, prec, 30, 3)
            from xvector_amd import synthetic as _syn, trainer as _trn
            _topo = tp.get("ModelWithoutDropoutAMSoftmax")
            _x, _lab = next(_syn.speaker_minibatches(1, feat, 64, 64, args.tmin, args.tmax, seed=77))
            _, verdict = _trn.select_trainer(_syn.trained_like(_topo, feat, num_classes=64, seed=1), _topo, dev, None, _x, _lab)
            out["train_step"] = dict(tr["bf16x3"], fp32=tr["fp32"], product_default_probe=verdict,
                                     product_default="auto: Model.train_one_iteration (local/tf/models.py, the twin of the reference's "
                                                     "models.py:216-305) and train_dnn.py compute the FIRST minibatch's gradients in both arithmetics "
                                                     "and run the bf16x3 step (the top-level figures of this object) when they agree "
                                                     "(trainer.select_trainer; product_default_probe is that verdict on this workload), else the "
                                                     "exact-fp32 step (the `fp32` entry); XVECTOR_TRAIN_PRECISION=fp32|bf16x3 forces one",
                                     workload="BASELINE configs[4], one rank's share: 64-chunk minibatches, T ~ U{%d..%d}, 64 speakers, "
                                              "AM-softmax head, Adam; 30 timed steps after 3 (minibatch lengths are drawn per step: ten steps were too few for a steady figure)" % (args.tmin, args.tmax))
        except Exception as e:
            out["train_step"] = {"error": repr(e)}
        try:
            out["trained_checkpoint"] = _trained_checkpoint_leg(dev, feat)
        except Exception as e:
            out["trained_checkpoint"] = {"error": repr(e)}
    # the exact-fp32 legs are the ones in the reference's own arithmetic (models.py:60 is an fp32 conv1d): a compact copy inside
    # `roofline` so that a record which keeps only the contract's objects still carries them
    same = {}
    for key in ("fp32_toomcook", "fp32_exact"):
        leg = out.get(key)
        if isinstance(leg, dict) and "value" in leg:
            same[key] = {"utt_s": round(leg["value"], 1), "ms_per_step": round(leg["ms_per_step"], 3), "frac_of_157.3TF_executed": round(leg["frac"], 4),
                         "parity_rel_l2_max_vs_fp64_oracle": leg.get("parity_rel_l2_max_vs_fp64_oracle")}
            if "algorithmic_over_peak" in leg:
                same[key]["algorithmic_over_peak"] = round(leg["algorithmic_over_peak"], 4)
    if same:
        same["note"] = "same workload, same bench.py run; IEEE fp32 products + fp32 accumulation = the reference's arithmetic (models.py:60); the headline `value` is the tolerance-contract f16bf8 path"
        tr = out.get("train_step")
        if isinstance(tr, dict) and "ms_per_step" in tr:
            same["train_step_ms"] = {"bf16x3": round(tr["ms_per_step"], 3), "fp32": round(tr.get("fp32", {}).get("ms_per_step", float("nan")), 3)}
        cv = out.get("config2_varlen")
        if isinstance(cv, dict) and "value" in cv:
            same["config2_varlen_utt_s"] = round(cv["value"], 1)
        cj = out.get("cli_job")
        if isinstance(cj, dict):
            same["cli_job"] = {k: cj[k] for k in ("wall_s", "transport", "utterances") if k in cj}
            rh = cj.get("rehearsal_8x125k") or {}
            if "predicted_per_rank_job_s" in rh:
                same["cli_job"]["rehearsal_8x125k"] = {"wall_s_one_shared_gpu": round(rh["wall_s"], 3), "breakdown_s_rank0": rh["breakdown_s_rank0"],
                                                       "predicted_breakdown_s": rh["predicted_breakdown_s"],
                                                       "predicted_per_rank_job_s": round(rh["predicted_per_rank_job_s"], 3),
                                                       "predicted_8gpu_utt_per_s": round(rh["predicted_8gpu_utt_per_s"], 1)}
        out["roofline"]["same_arithmetic"] = same
    print(json.dumps(out))
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
