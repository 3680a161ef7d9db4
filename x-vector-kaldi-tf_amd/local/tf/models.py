"""MI355X-native twin of the reference's ``local/tf/models.py`` for the extraction path.

Same class names, constructor and method signatures as BUTSpeechFIT/x-vector-kaldi-tf so that
``local/tf/train_dnn.py`` (``eval('models.%s()' % name).build_model(...)``, train_dnn.py:492-494) and
``local/tf/extract_embedding.py`` (``Model().make_embedding(...)``, extract_embedding.py:129-132) can
import this module unchanged:

=======================  ====================================  =======================================
method                   reference                              here
=======================  ====================================  =======================================
build_model              local/tf/models.py:25-128 (+variants)  reference initialisers -> model dir
save_model               local/tf/models.py:130-141             weight dict -> model dir (+ ``done``)
load_model               local/tf/models.py:143-162             model dir -> weights resident in HBM
make_embedding           local/tf/models.py:356-432             ark stream -> batched HIP forward -> ark
get_models_weights       local/tf/models.py:180-214             {tf variable name: ndarray}
print_models_params      local/tf/models.py:171-178
train_one_iteration/eval local/tf/models.py:216-354             HIP training / eval step
=======================  ====================================  =======================================

There is no TensorFlow and no CPU path: the forward graph runs as hand-written gfx950 kernels behind
``libxvector_hip.so`` (include/xvector_hip.h); without that library or without a GPU every compute
method raises.  ``use_gpu`` is accepted for signature compatibility (the reference's shell driver always
passes ``--use-gpu=no``, extract_xvectors.sh:76,85) and ignored: the extractor always runs on the GPU
selected by ``XVECTOR_DEVICE`` / ``LOCAL_RANK`` (default ``cuda:0``).
"""
import io
import os
import sys
import time

import numpy as np

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if _PKG_ROOT not in sys.path:
    sys.path.insert(0, _PKG_ROOT)

import kaldi_io  # noqa: E402  (the sibling module, as in the reference)
from xvector_amd import engine, extract_stream, frontend, synthetic, topology, weights as wio  # noqa: E402

VAR2STD_EPSILON = topology.VAR2STD_EPSILON        # models.py:16


def _device():
    dev = os.environ.get("XVECTOR_DEVICE")
    if dev:
        return dev
    return "cuda:%d" % int(os.environ.get("LOCAL_RANK", "0"))


class VectorCollector(object):
    """In-memory sink of one rank's x-vectors (kaldi_io.write_vec_flt_batch hands over (keys, vectors) as they are): what a rank
    of a sharded job writes to instead of the output table, until the ONE gather at the end."""
    mode = "wb"

    def __init__(self):
        self.keys, self.blocks = [], []

    def write_vectors(self, keys, vecs):
        if len(keys):
            self.keys.extend(keys)
            self.blocks.append(np.asarray(vecs, dtype=np.float32).reshape(len(keys), -1))

    def write(self, data):
        raise IOError("the sharded extractor writes vectors, not bytes")

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def gather_shard_vectors(device_model, collector, shard_keys, rank, world):
    """The single exchange of a sharded job (extract_xvectors.sh:92-95 concatenates the jobs' outputs; here ONE gather does --
    over RCCL, or over gloo straight from host memory when xvector_amd.dist.gather_backend chose that for a small payload).  Every rank knows every shard's key list -- the line ranges of an scp, or the byte ranges of an indexed ark, are
    deterministic -- so only numbers travel: rank r sends one row per utterance of ITS shard, in input order,
    ``[emitted? | x-vector]``; the blocks are padded to the largest shard so that a single fixed-shape ``dist.gather`` moves
    everything (xvector_amd.dist).  On rank 0 returns ``[(keys, vectors, emitted)]`` per shard in rank order = input order:
    the shard's keys and one row per key as they lie in the gathered block (a view, nothing is copied), and the mask of the
    utterances that emitted a vector (the others were rejected for their length or by the VAD) -- what
    ``kaldi_io.write_vec_flt_batch(fd, keys, vectors, emitted)`` takes; None on the other ranks."""
    import torch
    from xvector_amd import dist as xdist, jobclock
    dim, dev = device_model.embed_dim, device_model.device
    mine = shard_keys[rank]
    block = np.zeros((len(mine), dim + 1), np.float32)
    if collector.keys:
        whole = len(collector.keys) == len(mine) and mine == collector.keys    # nothing was rejected: the usual case
        if whole:
            rows = slice(None)
        else:
            # the emitted keys are a subsequence of the shard's keys (make_embedding keeps input order)
            rows, j = np.empty(len(collector.keys), np.int64), 0
            for i, k in enumerate(mine):
                if j < len(rows) and collector.keys[j] == k:
                    rows[j] = i
                    j += 1
            if j != len(rows):
                raise RuntimeError("sharded extraction: emitted keys are not a subsequence of the shard's keys")
        block[rows, 0] = 1.0
        if whole and len(collector.blocks) == 1:
            block[:, 1:] = collector.blocks[0]
        else:
            block[rows, 1:] = np.concatenate(collector.blocks)
    xdist.wait_process_group()
    jobclock.mark("wait for the process group")
    import torch.distributed as dist
    host = dist.is_initialized() and dist.get_backend() == "gloo"          # (the block is host memory: no device round trip then)
    blocks = xdist.gather_blocks(torch.from_numpy(block) if host else torch.from_numpy(block).to(dev), [len(k) for k in shard_keys], 0)
    jobclock.mark("gather")
    if rank != 0:
        return None
    out = []
    for r in range(world):
        got = blocks[r].cpu().numpy()
        out.append((shard_keys[r], got[:, 1:], got[:, 0] > 0.5))
    return out


_SELECTED = {}           # checkpoint identity + request -> engine.select_model's report (see Model.load_model)
_IDLE_MODELS = {}        # the same key -> DeviceModels of finished make_embedding calls (at most _IDLE_KEEP per key)
_IDLE_KEEP = 1


def _checkpoint_identity(model_dir):
    """(path, mtime_ns, size) of every weight-bearing file of a model directory, or (None,) when there is nothing to stat."""
    ident = []
    for name in ("model.weights.npz", "model.index", "model.data-00000-of-00001"):
        path = os.path.join(model_dir, name)
        try:
            st = os.stat(path)
            ident.append((os.path.realpath(path), st.st_mtime_ns, st.st_size))
        except OSError:
            pass
    return (tuple(ident) or None,)


class _StepDone(object):
    """(loss, accuracy) of a trainer that only has the synchronous ``step`` (the duck type of xvector_amd.trainer's handle)."""

    def __init__(self, value):
        self._value = value

    def result(self):
        return self._value


class Model(object):
    """Default topology: 5 frame-level layers [512,512,512,512,1536], kernels [5,5,7,1,1],
    statistics pooling, 2 segment-level layers (models.py:27-29)."""

    window_frames = 1 << 21          # utterances are read from the stream in windows of up to ~2M frames ...
    first_window_frames = 1 << 18    # ... starting with one batch's worth and doubling (pipeline fill)
    # in-place reading: one arena = one window.  ALL windows have the same size: the reader (~7 GB/s) is barely faster than the
    # GPU consumes ark bytes (~6.3 GB/s at 230 k utt/s), so every window that is larger than the one before it stalls the GPU for
    # the difference of their read times -- a short first window followed by large ones (round 2's first choice: 48 -> 144 MB)
    # cost 7 % end to end (tools/arena_sweep.py).  64 MB = ~2300 utterances of 300 frames = three even batches.
    arena_bytes = 64 << 20
    first_arena_bytes = 64 << 20
    map_input = os.environ.get("XVECTOR_MAP_INPUT", "1") != "0"      # BytesIO / regular-file input: scan in place instead of reading
    # read arenas in rotation: one with the reader (being filled or waiting for room in the queue), two queued, one being
    # packed, one whose window is still in flight -- an arena goes back to the pool only when its window has been COLLECTED: an
    # f16bf8 window whose status word comes back set is packed a second time from the same addresses (Extractor.finish)
    arena_count = 5
    exchange_windows = int(os.environ.get("XVECTOR_EXCHANGE_WINDOWS", "0"))      # multi-GPU stream mode: see make_embedding
    max_batch_rows = 262144

    def __init__(self):
        self.graph = None            # kept for attribute compatibility (models.py:22-23)
        self.device_model = None
        self.num_classes = None

    # -- topology --------------------------------------------------------------------------------
    @classmethod
    def class_topology(cls):
        return topology.get(cls.__name__)

    # -- build / save / load ---------------------------------------------------------------------
    def build_model(self, num_classes, input_feature_dim, output_dir, logger=None):
        if logger is not None:
            logger.info("Start building the model ...")
        topo = self.class_topology()
        self.num_classes = num_classes
        seed = int(os.environ.get("XVECTOR_INIT_SEED", "0"))
        w = synthetic.reference_init(topo, input_feature_dim, num_classes, seed=seed)
        self.save_model(dict(weights=w, topology=topo, model_class=type(self).__name__,
                             num_classes=num_classes, feat_dim=input_feature_dim), output_dir, logger)
        if logger is not None:
            logger.info("Building finished.")

    @staticmethod
    def save_model(sess, output_dir, logger):
        """``sess`` is the TF session in the reference (models.py:131); here it is the state dict
        {weights, topology, model_class, num_classes, feat_dim}."""
        if logger is not None:
            logger.info("Start saving graph ...")
        wio.save_model_dir(output_dir, sess["weights"], sess["topology"], sess["model_class"],
                           sess["num_classes"], sess["feat_dim"])
        if logger is not None:
            logger.info("Graph saved in path: %s" % os.path.join(output_dir, "model"))

    def load_model(self, sess, input_dir, logger):
        """Load ``input_dir`` and make the weights resident on the GPU.  ``sess`` (a TF session in the
        reference, models.py:143) is accepted and ignored."""
        if logger is not None:
            logger.info("Start loading graph ...")
        from xvector_amd import jobclock
        w, meta = wio.load_model_dir(input_dir)
        jobclock.once("weights read")
        import torch
        jobclock.once("import torch")
        torch.cuda.init()
        jobclock.once("hip runtime up")
        if getattr(self, "prepin_staging", False):
            # the CLI worker: its pinned staging sets come up beside the weights (engine.prewarm_staging), not in front of its first window
            try:
                engine.prewarm_staging((int(w["frame_level_info_layer-0/w:0"].shape[1]) + 3) // 4 * 4, self.max_batch_rows)
            except Exception:
                pass
        self.meta = meta
        self.num_classes = meta["num_classes"]
        self.embedding_index = int(os.environ.get("XVECTOR_EMBEDDING_INDEX", "0"))   # models.py:159-160
        # GEMM arithmetic: "f16bf8" (default: hidden layers as fp16 MFMA + scaled bf8 MFMA of the cross terms, ~1e-5 rel-L2;
        # topologies it does not cover and out-of-range windows run as bf16x3), "bf16x3" (split-precision bf16 MFMA, ~5e-6)
        # or "fp32" (exact fp32 MFMA)
        # The arithmetic is chosen PER CHECKPOINT: engine.select_model runs a small fixed batch through the loaded weights in
        # the requested arithmetic and in the next more exact one and steps down (f16bf8 -> bf16x3 -> fp32) when they disagree by
        # more than the probe limits (2e-5 / 4e-5; the parity bar is 1e-4).  XVECTOR_ACCURACY_PROBE=0 takes the request as given.
        # The verdict is a property of the checkpoint: a process that loads the same files again (a service, bench.py's repeated
        # passes) re-uses it instead of probing again (keyed by the weight file's identity, the request and the limits).
        self.precision = os.environ.get("XVECTOR_PRECISION", "f16bf8")
        key = _checkpoint_identity(input_dir) + (self.precision, self.embedding_index, _device(), engine.PROBE_LIMIT_F16BF8,
                                                 engine.PROBE_LIMIT_BF16X3, os.environ.get("XVECTOR_ACCURACY_PROBE", "1"))
        known = _SELECTED.get(key)
        idle = _IDLE_MODELS.get(key)
        self._model_key = None
        if known is not None and idle and getattr(self, "_may_borrow", False):
            # the same checkpoint, loaded before in this process and not in use: its weights are packed on the device, its
            # activation buffers allocated, its bf16x3 twin (accuracy probe, out-of-range windows) built -- a service that
            # calls make_embedding per request pays the ~10 ms of all that once.  make_embedding hands the model back when it
            # returns normally.
            self.device_model = idle.pop()
            self._model_key = key
        elif known is not None:
            # (the verdict includes the forms the probe turned off for this checkpoint)
            self.device_model = engine.DeviceModel(w, meta["topology"], _device(), self.embedding_index, known["selected"],
                                                   fold_shift=False if known.get("fold_shift") is False else None,
                                                   layer_mx6=False if known.get("layer_mx6") is False else None,
                                                   first_mx6=False if known.get("first_mx6") is False else None)
            self.device_model.selection = dict(known, cached=True)
            self._model_key = key
        else:
            self.device_model = engine.select_model(w, meta["topology"], _device(), self.embedding_index, self.precision)
            if key[0] is not None:
                _SELECTED[key] = dict(getattr(self.device_model, "selection", None) or {})
                self._model_key = key
        sel = getattr(self.device_model, "selection", None) or {}
        if logger is not None:
            if sel.get("probed"):
                logger.info("GEMM arithmetic: %s (requested %s; accuracy probe: f16bf8 vs bf16x3 %.2e%s)" % (
                    sel["selected"], sel["requested"], sel["f16bf8_vs_bf16x3"],
                    ", bf16x3 vs fp32 %.2e" % sel["bf16x3_vs_fp32"] if "bf16x3_vs_fp32" in sel else ""))
            logger.info("Graph restored from path: %s" % input_dir)

    def create_one_hot_output_matrix(self, labels):          # models.py:164-169
        one_hot = np.zeros((len(labels), self.num_classes), dtype=np.int32)
        one_hot[np.arange(len(labels)), np.asarray(labels, dtype=np.int64)] = 1
        return one_hot

    def print_models_params(self, input_dir, logger=None):
        w, meta = wio.load_model_dir(input_dir)
        print('\n\nThe components are:\n')
        for name in wio.expected_names(meta["topology"]):
            if name.rsplit('/', 1)[-1] not in ("mean:0", "variance:0"):       # trainable variables only
                print(name)
        print('\n')

    def get_models_weights(self, input_dir, logger=None):
        """Twin of models.py:180-214: ``{tf variable name: float32 ndarray}`` of the trainable variables plus the BN moving
        statistics, printed one per line, cached in / served from ``<input_dir>/model.h5`` when ``h5py`` is installed (one
        dataset per variable, named like the variable -- the layout the reference writes).  Without ``h5py`` the dictionary
        is returned all the same and no file is written."""
        h5file = os.path.join(input_dir, 'model.h5')
        try:
            import h5py
        except ImportError:
            h5py = None
        if h5py is not None and os.path.exists(h5file):
            name2weights = {}

            def collect(name, node):
                if not isinstance(node, h5py.Group):
                    name2weights[name] = np.array(node[()])
            with h5py.File(h5file, 'r') as hf:
                hf.visititems(collect)
            return name2weights
        w, meta = wio.load_model_dir(input_dir)
        name2weights = {}
        for name in wio.expected_names(meta["topology"]):     # trainables first, then mean / variance: the reference's order
            if name.rsplit('/', 1)[-1] not in ("mean:0", "variance:0"):
                name2weights[name] = np.array(w[name], dtype=np.float32)      # own, writable arrays (the loader hands out views)
        for name in wio.expected_names(meta["topology"]):
            if name not in name2weights:
                name2weights[name] = np.array(w[name], dtype=np.float32)
        for name, mat in name2weights.items():
            print('%s  shape: %s' % (name, str(mat.shape)))
        if h5py is not None:
            with h5py.File(h5file, 'w') as hf:
                for name, mat in name2weights.items():
                    hf.create_dataset(name, data=mat.astype(np.float32))
        elif logger is not None:
            logger.info("h5py is not installed: %s not written" % h5file)
        return name2weights

    # -- training / diagnostics ---------------------------------------------------------
    def _trainer(self, input_dir, logger, first_batch=None):
        """The trainer of a model directory.  XVECTOR_TRAIN_PRECISION: "fp32" | "bf16x3" as given, "auto" (the default): bf16x3 when
        the gradients of ``first_batch`` = (x, labels) agree with the exact-fp32 ones (trainer.select_trainer), else fp32;
        without a first batch (eval) "auto" is fp32.  The verdict travels with the model (weights.save_train_verdict): the next
        iterations reuse it -- "fp32" for good (also after a non-finite bf16x3 loss, see train_one_iteration), "bf16x3" for ten
        iterations, then the probe runs again on that iteration's first minibatch."""
        from xvector_amd import trainer
        if logger is not None:
            logger.info("Start loading graph ...")
        w, meta = wio.load_model_dir(input_dir)
        self.meta = meta
        self.num_classes = meta["num_classes"]
        precision = os.environ.get("XVECTOR_TRAIN_PRECISION", "auto")
        adam = wio.load_optimizer_state(input_dir)
        self.train_precision_auto = precision == "auto"
        kept = wio.load_train_verdict(input_dir) if precision == "auto" and first_batch is not None else None
        if kept is not None:
            self.train_precision_verdict = dict(kept, iterations_since_probe=int(kept.get("iterations_since_probe", 0)) + 1, reused=True)
            tr = trainer.Trainer(w, meta["topology"], _device(), adam, precision=kept["selected"])
            if logger is not None:
                logger.info("Training arithmetic: %s (verdict of %d iteration(s) ago, kept with the model)" % (
                    kept["selected"], self.train_precision_verdict["iterations_since_probe"]))
        elif precision == "auto" and first_batch is not None:
            tr, verdict = trainer.select_trainer(w, meta["topology"], _device(), adam, first_batch[0], first_batch[1], logger)
            self.train_precision_verdict = dict(verdict, iterations_since_probe=0)
        else:
            tr = trainer.Trainer(w, meta["topology"], _device(), adam, precision="fp32" if precision == "auto" else precision)
        if logger is not None:
            logger.info("Graph restored from path: %s" % input_dir)
        return tr

    @staticmethod
    def _next_batch(data_loader, index, logger, what, meter):
        """One ``data_loader.pop()`` (examples_io.py:213-221,252-255) with the reference's two tolerated failures -- a
        ``queue.Empty`` timeout and a ``None`` batch (models.py:244-253): both are logged and reported as "no batch"."""
        import queue
        t0 = time.time()
        try:
            batch, labels = data_loader.pop()
        except queue.Empty:
            logger.warning('Timeout reach when reading %s %d' % (what, index))
            batch, labels = None, None
        else:
            if batch is None:
                logger.warning('batch_data is None for %s %d' % (what, index))
        meter.waited("disk", time.time() - t0)
        return batch, labels

    @staticmethod
    def _everyone_has(batch, device):
        """Data-parallel runs only: every optimizer step is a collective (Trainer.step all-reduces the gradient), so a
        rank may not skip a minibatch on its own.  The decision is made together -- one MIN all-reduce of a "have a
        batch" flag -- and either every rank steps or every rank skips (its batch, if it had one, is dropped)."""
        import torch.distributed as dist
        have = batch is not None
        if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
            return have
        import torch
        on_gpu = dist.get_backend() == "nccl"
        flag = torch.tensor([1 if have else 0], dtype=torch.int32, device=device if on_gpu else "cpu")
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        return bool(flag.item())

    def train_one_iteration(self, data_loader, args, logger):
        """Twin of models.py:216-305: one pass over ``data_loader`` (``.count`` minibatches of ``[B,T,F]`` float16/32 +
        int labels), Adam with ``args.learning_rate``, then the model (and the optimizer slots) are saved to
        ``args.output_dir``.  Reads the same ``args`` fields as the reference (learning_rate, print_interval,
        dropout_proportion, input_dir, output_dir, random_seed) and prints the same log lines (they are regex-parsed by
        ze_utils.py:126-127,498-499); the running averages behind those lines live in ``runstats.Meter``."""
        from xvector_amd import runstats
        keep_out = float(getattr(args, "dropout_proportion", 0.0) or 0.0)      # keep_prob = 1 - this, models.py:258
        seed = int(getattr(args, "random_seed", 0) or 0)                       # models.py:223,233
        tr = None                        # built on the first minibatch: its gradients decide the arithmetic (XVECTOR_TRAIN_PRECISION=auto)
        pending = None                   # (index, B, T, handle) of the step whose loss has not been read back yet
        meter = runstats.Meter(planned=data_loader.count, report_every=args.print_interval)
        for index in range(data_loader.count):
            batch, labels = self._next_batch(data_loader, index, logger, 'the minibatch index', meter)
            stepped_now = self._everyone_has(batch, _device())
            if not stepped_now:
                if batch is not None:
                    logger.warning('minibatch index %d skipped: another rank of the group has no batch' % index)
            else:
                if tr is None:           # every rank of the group is here with a minibatch: the probe's own collective lines up
                    tr = self._trainer(args.input_dir, logger, (batch, labels))
                t0 = time.time()
                # the step is enqueued; its loss is read back after the NEXT step has been enqueued (or at the end of the loop): the
                # GPU does not idle while the host stages a minibatch.  The log lines are averages over intervals of steps, which
                # the one-step lag does not change (an interval line waits for its own last step, below).
                launch = getattr(tr, "step_async", None)
                handle = launch(batch, labels, args.learning_rate, keep_out, seed) if launch is not None else \
                    _StepDone(tr.step(batch, labels, args.learning_rate, keep_out, seed))
                now = (index, batch.shape[0], batch.shape[1], handle)
                if pending is not None:
                    meter.stepped(pending[0], pending[1], pending[2], *self._finite(pending, tr, args.input_dir, logger))
                pending = now
                meter.waited("gpu", time.time() - t0)
            if pending is not None and (index == data_loader.count - 1 or meter.interval_due(index)):
                meter.stepped(pending[0], pending[1], pending[2], *self._finite(pending, tr, args.input_dir, logger))
                pending = None
            if not stepped_now:
                meter.skipped(index)     # (last word on this index: an index without a step never closes an interval)
            line = meter.interval_line(index)
            if line:
                logger.info(line)
        for line in meter.training_summary():
            logger.info(line)
        if tr is None:                   # not a single minibatch: the model goes out as it came in
            tr = self._trainer(args.input_dir, logger)
        if getattr(args, "save_model", True):          # data-parallel driver (train_dnn.py): only one rank of the group writes
            w, adam = tr.export()
            # optimizer slots first, the model (whose 'done' marker completes the directory) last
            os.makedirs(args.output_dir, exist_ok=True)
            wio.save_optimizer_state(args.output_dir, adam)
            if getattr(self, "train_precision_verdict", None) is not None:
                wio.save_train_verdict(args.output_dir, self.train_precision_verdict)
            self.save_model(dict(weights=w, topology=self.meta["topology"], model_class=self.meta["model_class"],
                                 num_classes=self.meta["num_classes"], feat_dim=self.meta["feat_dim"]), args.output_dir, logger)
        logger.info(meter.elapsed_line())

    def _finite(self, pending, tr, input_dir, logger):
        """(loss, accuracy) of a finished step.  A non-finite loss of the bf16x3 step that the gradient probe admitted ("auto") is
        this build's doing, not the reference's arithmetic: the iteration stops, nothing is saved, and the INPUT model's verdict is
        set to fp32 -- a rerun of this iteration (and every later one) trains in the exact-fp32 step.  A non-finite loss in fp32, or
        in an arithmetic the user forced, is reported as the reference would report it (it appears in the log lines)."""
        loss, accuracy = pending[3].result()
        if not np.isfinite(loss) and getattr(self, "train_precision_auto", False) and getattr(tr, "precision", "fp32") == "bf16x3":
            verdict = dict(getattr(self, "train_precision_verdict", None) or {}, selected="fp32", iterations_since_probe=0,
                           demoted="non-finite loss at minibatch %d of a bf16x3 iteration" % pending[0])
            try:
                wio.save_train_verdict(input_dir, verdict)
            except OSError:
                pass
            msg = ("non-finite training loss at minibatch %d in the bf16x3 arithmetic: iteration stopped, no model written; "
                   "'%s' is now marked for the exact-fp32 step -- rerun this iteration" % (pending[0], input_dir))
            if logger is not None:
                logger.error(msg)
            raise FloatingPointError(msg)
        return loss, accuracy

    def eval(self, data_loader, input_dir, use_gpu, logger):
        """Twin of models.py:307-354: loss / accuracy over ``data_loader`` in the eval phase (moving BN statistics)."""
        from xvector_amd import runstats
        tr = self._trainer(input_dir, logger)
        meter = runstats.Meter(planned=data_loader.count)
        for index in range(data_loader.count):
            batch, labels = self._next_batch(data_loader, index, logger, 'minibatch index', meter)
            if batch is None:
                continue
            loss, accuracy = tr.eval_batch(batch, labels)
            meter.stepped(index, batch.shape[0], batch.shape[1], loss, accuracy)
        for line in meter.eval_summary():
            logger.info(line)
        logger.info(meter.elapsed_line())

    def _exchange_shards(self, stash, rank, world, min_chunk_size, chunk_size, emit):
        """The one collective of the multi-GPU stream mode: every rank contributes the x-vectors of its shares of all
        windows as one block (counts follow from the deterministic partitions, so nothing but vectors travels); rank 0 cuts
        the blocks back into windows, restores the input order and emits them."""
        import torch
        from xvector_amd import dist as xdist
        dim, dev = self.device_model.embed_dim, self.device_model.device
        counts = [int(sum(len(sh[r]) for _, _, sh, _ in stash)) for r in range(world)]
        local = np.concatenate([v for _, _, _, v in stash]) if stash and counts[rank] else np.zeros((0, dim), np.float32)
        blocks = xdist.gather_blocks(torch.from_numpy(np.ascontiguousarray(local, dtype=np.float32)).to(dev), counts, 0)
        if rank != 0:
            return
        blocks = [b.cpu().numpy() for b in blocks]
        at = [0] * world
        for keys, lens, shards, _ in stash:
            full = np.zeros((len(keys), dim), np.float32)
            for r in range(world):
                n = len(shards[r])
                full[shards[r]] = blocks[r][at[r]:at[r] + n]
                at[r] += n
            valid = np.array([bool(engine.plan_chunks(int(t), min_chunk_size, chunk_size)) for t in lens], dtype=bool)
            emit(keys, lens, full, valid)

    def _extract_byte_ranges(self, input_stream, output_stream, model_dir, min_chunk_size, chunk_size, use_gpu, logger):
        """Multi-GPU extraction from a seekable ark FILE (no scp): instead of every rank parsing the whole stream, each rank
        runs ONE cheap index pass over the record headers (kaldi_io.index_mat_ark_file: a small pread per record, the matrices
        are hopped over), takes the records whose first byte falls into its 1/world slice of the payload bytes -- deterministic,
        so no rank has to tell another where to start -- reads ONLY those bytes (kaldi_io.FileRange) through the single-process
        pipeline, and the one gather at the end brings the vectors to rank 0, which knows every shard's keys from its own index.
        Returns False (nothing consumed) when this does not apply: no group, not a regular file, a record type the index does
        not take -- the caller then reads the stream the ordinary way (a pipe cannot be split)."""
        from xvector_amd import dist as xdist
        rank, world = xdist.group_shape()
        if world <= 1 or not kaldi_io.is_regular_file(input_stream):
            return False
        xdist.init_process_group_async()          # (the group comes up next to the index pass: ~1.2 us per record, 1.2 s for 1 M)
        index = kaldi_io.index_mat_ark_file(input_stream)
        if index is None:
            return False
        offsets, rows, _, keys = index
        first, last = int(offsets[0]), int(offsets[-1])
        cuts = np.searchsorted(offsets[:-1], [first + (last - first) * r // world for r in range(world + 1)], side="left")
        cuts[0], cuts[-1] = 0, len(keys)
        shard_keys = [keys[cuts[r]:cuts[r + 1]] for r in range(world)]
        collector = VectorCollector()
        mine = kaldi_io.FileRange(input_stream, offsets[cuts[rank]], offsets[cuts[rank + 1]])
        if logger is not None:
            logger.info("rank %d of %d: records %d..%d of %d, bytes %d..%d of the ark" % (
                rank, world, cuts[rank], cuts[rank + 1], len(keys), offsets[cuts[rank]], offsets[cuts[rank + 1]]))
        self.make_embedding(mine, collector, model_dir, min_chunk_size, chunk_size, use_gpu, logger, distributed=False)
        input_stream.seek(last)                                     # the caller's stream is consumed, as after a full read
        shards = gather_shard_vectors(self.device_model, collector, shard_keys, rank, world)
        if shards is not None:
            for skeys, vecs, emitted in shards:
                kaldi_io.write_vec_flt_batch(output_stream, skeys, vecs, emitted)
        return True

    # -- the hot path ------------------------------------------------------------------------------
    def make_embedding(self, input_stream, output_stream, model_dir, min_chunk_size, chunk_size, use_gpu, logger,
                       vad_stream=None, cmn_window=0, cmn_center=True, distributed=True, window=0, period=0, subsegments=None,
                       frame_shift=10.0):
        """Build-defined extension (defaults = the reference's behaviour): with ``cmn_window > 0`` and/or a
        ``vad_stream`` (ark stream or (key, vector) iterator, same key order as the features) the sliding-window CMN and
        the VAD frame selection that extract_xvectors.sh:68 runs as Kaldi binaries are done on the GPU first, so
        ``input_stream`` can carry raw features.  ``input_stream`` may also be a (key, matrix) iterator or a table with a
        ``blocks()`` method (kaldi_io.MatScp).  Under torchrun every
        rank reads the same stream and extracts its share of each window (one gather per window to rank 0) unless
        ``distributed=False`` says that the caller sharded the input itself.

        ``window`` > 0 (frames): sliding mode -- one x-vector per sub-segment of ``window`` frames cut every
        ``period`` frames (0: = window) instead of one per utterance, ``chunk_size`` ignored; sub-segment [first, end) of ``<utt>``
        is written under ``<utt>-<first>-<end>`` (8 digits each).  ``subsegments``: a text stream that gets one line per vector,
        ``<key> <utt> <start s> <end s>`` (a Kaldi segments file), frames turned into seconds with ``frame_shift`` milliseconds (a
        WaveTable input: its MFCC configuration's).  One process only.

        A WaveTable with a ``segmenter`` cuts every recording into segments first and extracts each segment as an
        utterance: sliding windows stay inside segments and are keyed ``<reco>-<first>-<end>`` in the recording's frames; without
        ``window`` one vector is written per segment, under its id in the segments file or ``<reco>-<first>-<end>``."""
        start_time = time.time()
        from_wav = isinstance(input_stream, extract_stream.WaveTable)
        sliding = int(window or 0) > 0
        if sliding:
            from xvector_amd import dist as xdist
            if distributed and xdist.group_shape()[1] > 1:
                raise ValueError("sliding-window extraction (window > 0) runs in one process: split the input and run one job per part")
            period = int(period) if period else int(window)
            if not 1 <= period <= int(window):
                raise ValueError("period must lie in [1, window] (period %d, window %d)" % (period, window))
            if int(window) < int(min_chunk_size):
                raise ValueError("window %d is shorter than min_chunk_size %d" % (window, min_chunk_size))
        elif period or subsegments is not None:
            raise ValueError("period and subsegments go with window > 0")
        if from_wav:
            # x-vectors straight from a wav.scp: the table makes its own VAD, the CMN is part of the route, and
            # one process reads the whole table -- refused before a file is read or a kernel launched
            from xvector_amd import dist as xdist
            if vad_stream is not None or cmn_window <= 0:
                raise ValueError("a WaveTable input takes no vad_stream (it computes the VAD itself) and needs cmn_window > 0")
            if distributed and xdist.group_shape()[1] > 1:
                raise ValueError("a WaveTable input is read by one process: sharding wav.scp across ranks is not supported")
        if distributed and not sliding and vad_stream is None and cmn_window <= 0 and self._extract_byte_ranges(
                input_stream, output_stream, model_dir, min_chunk_size, chunk_size, use_gpu, logger):
            return
        # three threads (xvector_amd.extract_stream): a reader parses the windows, this one runs them, a writer serialises the
        # vectors.  The reader starts BEFORE the model is loaded: the first arena is read and scanned while the weights are packed
        reader = input_stream.start() if from_wav else extract_stream.WindowReader(self, input_stream, vad_stream)
        try:
            try:
                self._may_borrow = os.environ.get("XVECTOR_MODEL_CACHE", "1") != "0"
                self.load_model(None, model_dir, logger)
            finally:
                self._may_borrow = False
            F_dim = self.device_model.feat_dim
            if from_wav and input_stream.opts.num_ceps != F_dim:
                raise ValueError("--num-ceps=%d of the MFCC configuration is not the model's feature dimension %d"
                                 % (input_stream.opts.num_ceps, F_dim))
            ex = engine.Extractor(self.device_model, min_chunk_size, chunk_size, max_batch_rows=self.max_batch_rows,
                                  window=int(window) if sliding else None, period=period if sliding else None)
            front = None
            if cmn_window > 0 or vad_stream is not None:
                front = frontend.FrontEnd(self.device_model.device, cmn_window, cmn_center)     # cmn_window <= 0: selection only

            # Multi-GPU (one process per GPU, torchrun) on a stream nobody can split (ark file, pipe): every rank reads the same
            # stream and extracts only its frame-balanced share of each window -- the partition follows from the lengths, so it
            # needs no communication -- keeps its x-vectors, and ONE gather at the very end brings them to rank 0, which restores
            # the input order and alone writes (the role of split_data.sh + nj jobs + `cat xvector.*.scp`,
            # extract_xvectors.sh:63-95).  An scp table is better served by extract_embedding.py's line-range sharding, where
            # the ranks do not even parse each other's utterances.
            from xvector_amd import dist as xdist, jobclock
            jobclock.once("weights packed on the device + accuracy probe")
            if distributed:
                # the group is only needed for the exchange at the end: it comes up on a side thread (RCCL's first communicator takes
                # about a second) while this one extracts; nothing is written to the output before the exchange
                rank, world = xdist.group_shape()
                if xdist.group_wanted():
                    if world > 1:
                        xdist.init_process_group_async()
                    else:
                        # a forced one-rank group (XV_FORCE_DIST=1): this process emits vectors as windows finish, and fd 1 points at
                        # stderr while a communicator comes up (dist.init_process_group) -- an 'ark:-' output would lose records to
                        # stderr.  Nothing to overlap with in this mode: the group comes up first.
                        xdist.wait_process_group()
            else:
                # the caller already gave every rank its own part of the input (extract_embedding.py shards scp tables by line
                # range): behave as a single process and leave the exchange to the caller
                rank, world = 0, 1

            writer = extract_stream.VectorWriter(output_stream, subsegments,
                                                 input_stream.opts.frame_shift if from_wav else frame_shift)
            run = extract_stream.Extraction(self, ex, front, writer, logger, min_chunk_size, chunk_size, rank, world)
            # software pipeline of depth 2 over the windows: the host work of window i+1 (packing, H2D, launches) is issued
            # before the vectors of window i are awaited and written, so the GPU never waits for the writer
            in_flight = None
            try:
                for keys, mats, vads in reader:
                    writer.check()
                    # a column count other than the model's goes down the checked NumPy packing path and raises there
                    addrs = mats.addrs if mats.uniform_cols() == F_dim else None
                    run.total_segments += len(keys)
                    nxt = run.submit(keys, mats, vads, addrs)
                    jobclock.once("first window launched")
                    arenas = [held for held in mats.holders if isinstance(held, kaldi_io.ArkArena)]
                    del mats
                    run.retire(in_flight, reader)
                    in_flight = (nxt, arenas)
                run.retire(in_flight, reader)
                if world > 1 and (run.stash or not self.exchange_windows):
                    run.exchange()
            finally:
                reader.cancel()                         # (no-op after a complete pass: the reader has already returned)
                writer.close()
        finally:
            reader.close()
        writer.check()

        if getattr(self, "_model_key", None) is not None and hasattr(self.device_model, "frame_level"):
            parked = _IDLE_MODELS.setdefault(self._model_key, [])         # (only after a complete pass: the model is in a known state)
            if len(parked) < _IDLE_KEEP and all(m is not self.device_model for m in parked):
                parked.append(self.device_model)
        st = ex.stats
        if st.get("probe_windows"):
            logger.info("Accuracy probe on the input: f16bf8 vs bf16x3 chunk vectors differ by at most %.2e over %d probed window(s)%s" % (
                st["probe_rel_l2_max"], st["probe_windows"],
                "; demoted to bf16x3 at window %d" % st["demoted_at_window"] if ex.demoted else ""))
        self.last_stats = dict(st, demoted=bool(getattr(ex, "demoted", False)),
                               selection=dict(getattr(self.device_model, "selection", None) or {}))
        segmented = from_wav and input_stream.segmenter is not None
        logger.info("Processed %d features of average size %d frames. Done %d and failed %d%s%s" %
                    (run.total_segments, st["frames"] / max(run.total_segments, 1), run.num_success, run.num_fail,
                     "; wrote %d sub-segment vectors" % run.num_vectors if sliding else "",
                     "; cut %d segments" % run.num_segments if segmented else ""))
        if segmented and (input_stream.segmenter.unknown() or input_stream.segmenter.skipped):
            logger.info("Skipped %d line(s) of the segments file whose recording is not in the wav.scp and %d empty segment(s)" %
                        (input_stream.segmenter.unknown(), input_stream.segmenter.skipped))
        logger.info("Total time for neural network computations is %.2f minutes." % (run.compute_time / 60.0))
        logger.info("Elapsed time for extracting whole embeddings is %.2f minutes." %
                    ((time.time() - start_time) / 60.0))


class ModelWithoutDropout(Model):                     # models.py:436
    pass


class ModelWithoutDropoutTdnn(Model):                 # models.py:538  (dilated)
    pass


class ModelWithoutDropoutPRelu(Model):                # models.py:643
    pass


class ModelL2LossWithoutDropoutPRelu(Model):          # models.py:746
    pass


class ModelL2LossWithoutDropoutLRelu(Model):          # models.py:866
    pass


class ModelL2LossWithoutDropoutLReluAttention(Model):    # models.py:985  (self-attentive pooling, attention/{w,b,v})
    pass


class ModelWithoutDropoutAMSoftmax(Model):            # build-defined (BASELINE configs[4]); see xvector_amd/topology.py
    pass


class ModelL2LossWithoutDropoutReluHeInit(Model):     # models.py:1118
    pass
