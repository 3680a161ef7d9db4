"""Stage 2 of the recipe on the MI355X: Kaldi's ``wav-reverberate`` evaluated in-process.

Kaldi's ``steps/data/reverberate_data_dir.py`` and ``augment_data_dir.py`` write no audio: they write wav.scp entries whose
last pipeline stage is ``wav-reverberate ... - |``.  This module

* parses such an entry into a tree (``parse_rx``): the input, the impulse response and every additive signal are rxfilenames
  themselves, so a nested ``wav-reverberate`` (the ``--duration`` repeat of background noises) becomes a child node, never a
  process; stages before the last one (sox) still run in the shell, except a single recognised ``sph2pipe`` command, which
  ``mfcc.load_wav`` reads in-process (xvector_amd/sphere.py);
* works out each node's output length and rate on the host (``Augmenter.plan``), decoding every distinct rxfilename once and
  forming every distinct impulse response once;
* evaluates the nodes on the GPU level by level (csrc/xv_augment.hip; children first), writing the top-level outputs straight
  into a device sample buffer, e.g. the one ``xv_mfcc_f32`` reads.

There is no CPU path: the arithmetic runs on the GPU, and a missing device is an error.
"""
import logging
import os
import shlex
import sys

import numpy as np

from . import hiplib, mfcc

logger = logging.getLogger("augment")

CONV_TILE = 2048                  # outputs per workgroup of the convolution (xv_augment.hip CTILE)
ELEM_TILE = 1024                  # samples per workgroup of the mix and write kernels (ET * EPT)
POWER_TILE = 16384                # samples per workgroup of the power kernel (PTILE)
UTT_FIELDS, REF_FIELDS = 16, 4    # include/xvector_hip.h XV_AUG_*
(X_OFF, N_, Y_OFF, Y_LEN, RIR, EARLY_TILE0, EARLY_NTILES, EARLY_LEN, REF0, NREF, SHIFT, M_, OUT_OFF, MIX_TILE0, MIX_NTILES,
 X_SEG) = range(16)
F32 = np.float32


class AugmentError(ValueError):
    pass


# ------------------------------------------------------------------------------------------------
# the wav-reverberate command line
# ------------------------------------------------------------------------------------------------
class ReverbOptions(mfcc._Options):
    """wav-reverberate's options under Kaldi's names, Kaldi's defaults."""
    _FIELDS = (
        ("shift_output", bool, False), ("impulse_response", str, ""), ("additive_signals", str, ""), ("snrs", str, ""),
        ("start_times", str, ""), ("volume", float, 0.0), ("duration", float, 0.0), ("normalize_output", bool, True),
        ("input_wave_channel", int, 0), ("rir_channel", int, 0), ("noise_channel", int, 0), ("multi_channel_output", bool, False),
    )


class Source(object):
    """A plain rxfilename: a path, ``-`` (standard input) or a ``cmd |`` pipe without wav-reverberate."""

    def __init__(self, rx):
        self.rx = rx

    def __repr__(self):
        return "Source(%r)" % self.rx


class Reverb(object):
    """One wav-reverberate evaluation.  ``input``, ``rir`` (or None) and ``noises`` are Source or Reverb nodes; ``snrs`` and
    ``start_times`` are fp32 values, one per noise."""

    def __init__(self, rx, opts, input, rir, noises, snrs, start_times):
        self.rx, self.opts, self.input, self.rir = rx, opts, input, rir
        self.noises, self.snrs, self.start_times = noises, snrs, start_times

    def __repr__(self):
        return "Reverb(input=%r, rir=%r, noises=%r, snrs=%r, start_times=%r)" % (self.input, self.rir, self.noises,
                                                                                  self.snrs, self.start_times)


def split_pipeline(cmd):
    """Split a shell command on the ``|`` outside quotes (single, double, backslash escapes as the shell reads them).  The
    stages come back as raw text: ``"|".join(stages)`` is ``cmd``."""
    stages, start, i, quote = [], 0, 0, None
    while i < len(cmd):
        c = cmd[i]
        if quote == "'":
            if c == "'":
                quote = None
        elif c == "\\":
            i += 1
        elif quote == '"':
            if c == '"':
                quote = None
        elif c in "'\"":
            quote = c
        elif c == "|":
            stages.append(cmd[start:i])
            start = i + 1
        i += 1
    if quote:
        raise AugmentError("unterminated %s quote in %r" % (quote, cmd))
    stages.append(cmd[start:])
    return stages


def _is_reverb(argv):
    return bool(argv) and os.path.basename(argv[0]) == "wav-reverberate"


def _floats(text, what):
    try:
        return [float(F32(v)) for v in text.split(",") if v != ""]
    except ValueError:
        raise AugmentError("wav-reverberate: invalid --%s=%r" % (what, text))


def parse_argv(argv, rx="", stdin=None):
    """wav-reverberate's arguments (without the program name) -> Reverb.  ``stdin``: the Source standing for ``-`` as the input
    (None: standard input)."""
    opts, pos = ReverbOptions(), []
    for a in argv:
        if a.startswith("--") and len(a) > 2:
            name, eq, value = a[2:].partition("=")
            if name.replace("-", "_") not in ReverbOptions.names():
                raise AugmentError("wav-reverberate: unknown option --%s" % name)
            if not eq and name.replace("-", "_") not in ("shift_output", "normalize_output", "multi_channel_output"):
                raise AugmentError("wav-reverberate: option --%s needs a value" % name)
            try:
                opts.set(name, value)
            except ValueError as e:
                raise AugmentError("wav-reverberate: %s" % e)
        else:
            pos.append(a)
    if opts.multi_channel_output:
        raise AugmentError("wav-reverberate: --multi-channel-output=true is not supported")
    if len(pos) != 2:
        raise AugmentError("wav-reverberate: expected <input-rxfilename> <output-wxfilename>, got %r" % (pos,))
    if pos[1] != "-":
        raise AugmentError("wav-reverberate: the output must be '-' (standard output), got %r" % pos[1])
    inp = (stdin or Source("-")) if pos[0] == "-" else parse_rx(pos[0])
    rir = parse_rx(opts.impulse_response) if opts.impulse_response else None
    noises = [parse_rx(s) for s in opts.additive_signals.split(",") if s != ""]
    snrs, times = _floats(opts.snrs, "snrs"), _floats(opts.start_times, "start-times")
    if len(snrs) != len(noises) or len(times) != len(noises):
        raise AugmentError("wav-reverberate: %d additive signals but %d --snrs and %d --start-times" % (len(noises), len(snrs),
                                                                                                      len(times)))
    if any(t < 0 for t in times):
        raise AugmentError("wav-reverberate: negative --start-times")
    return Reverb(rx, opts, inp, rir, noises, snrs, times)


def parse_rx(rx):
    """An rxfilename -> Source (no wav-reverberate in it: read as before) or Reverb (its last stage is wav-reverberate)."""
    rx = rx.strip()
    if not rx.endswith("|"):
        return Source(rx)
    stages = split_pipeline(rx[:-1])
    argvs = []
    for s in stages:
        try:
            argvs.append(shlex.split(s))
        except ValueError as e:
            raise AugmentError("cannot parse pipeline stage %r: %s" % (s, e))
    if any(_is_reverb(a) for a in argvs[:-1]):
        raise AugmentError("wav-reverberate is supported only as the last stage of a pipe: %r" % rx)
    if not _is_reverb(argvs[-1]):
        return Source(rx)
    before = "|".join(stages[:-1]) + "|" if len(stages) > 1 else None
    args = argvs[-1][1:]
    node = parse_argv(args, rx, Source(before) if before else None)
    if before and not (isinstance(node.input, Source) and node.input.rx == before):
        raise AugmentError("wav-reverberate reads a file but earlier pipeline stages write to it: %r" % rx)
    if not before and isinstance(node.input, Source) and node.input.rx == "-":
        raise AugmentError("wav-reverberate reads '-' but no pipeline stage writes to it: %r" % rx)
    return node


def is_augmented(rx):
    """Cheap test for wav.scp entries: could ``rx`` carry wav-reverberate (then ``parse_rx`` decides)."""
    return rx.rstrip().endswith("|") and "wav-reverberate" in rx


# ------------------------------------------------------------------------------------------------
# host planning
# ------------------------------------------------------------------------------------------------
def early_window(peak, L, fs):
    """Kaldi's early-reverb window [start, end) of an L-tap RIR: peak -/+ 0.001 / 0.05 s, evaluated in fp32, truncated, clamped."""
    start = int(F32(peak) - F32(0.001) * F32(fs))
    end = int(F32(peak) + F32(0.05) * F32(fs))
    return max(start, 0), min(end, L)


def output_length(duration, fs, n):
    return int(F32(duration) * F32(fs)) if duration > 0 else n


def sample_offset(t, fs):
    return int(F32(t) * F32(fs))


class _Rir(object):
    """An impulse response formed once: h = channel / 32768 (fp32), its first maximum and early window."""

    def __init__(self, x, fs):
        self.h = (x.astype(F32) * F32(1.0 / 32768))
        self.L = len(self.h)
        if self.L == 0:
            raise AugmentError("empty impulse response")
        self.peak = int(np.argmax(self.h))
        self.start, self.end = early_window(self.peak, self.L, fs)
        self.fs = fs


class _Node(object):
    """A Reverb placed in a plan: its level, sources, output length."""
    __slots__ = ("reverb", "key", "level", "x", "rir", "noises", "N", "M", "rate", "shift", "top", "out_off", "seq", "host_out")
    count = [0]


class Plan(object):
    """The host half of evaluating a batch: output lengths and rates known, every source decoded once."""

    def __init__(self):
        self.nodes, self.top = [], []
        self.decoded = {}             # rx -> (rate, int16 [channels, samples])
        self.rirs = {}                # (id of the RIR's source, channel) -> _Rir
        self.nested = {}              # rx -> _Node (a nested evaluation is done once per batch)

    def lengths(self):
        return [n.M for n in self.top]

    def rates(self):
        return [n.rate for n in self.top]


class Augmenter(object):
    """wav-reverberate over batches of wav.scp entries on one GPU."""

    def __init__(self, device="cuda:0"):
        self.device = device
        self.stats = dict(evaluations=0, levels=0, samples_out=0, clipped=0)

    # --- planning (host only; no GPU) ---
    def _decode(self, plan, key, src):
        if src.rx not in plan.decoded:
            if src.rx == "-":
                data = sys.stdin.buffer.read()
                try:
                    plan.decoded[src.rx] = mfcc.read_wav(data, key)
                except mfcc.WavError as e:
                    raise AugmentError(str(e))
            else:
                try:
                    plan.decoded[src.rx] = mfcc.load_wav(key, src.rx)
                except (mfcc.WavError, OSError) as e:
                    raise AugmentError("%s: cannot read %r: %s" % (key, src.rx, e))
        return plan.decoded[src.rx]

    def _signal(self, plan, key, src, channel, what):
        """-> ('host', (rx, channel), rate, int16 samples) or ('node', _Node, rate)."""
        if isinstance(src, Reverb):
            node = self._node(plan, key, src, top=False)
            if channel != 0:
                raise AugmentError("%s: %s channel %d of a one-channel wav-reverberate output" % (key, what, channel))
            return ("node", node, node.rate)
        rate, x = self._decode(plan, key, src)
        if not 0 <= channel < x.shape[0]:
            raise AugmentError("%s: %s channel %d of %d" % (key, what, channel, x.shape[0]))
        return ("host", (src.rx, channel), rate, x[channel])

    def _node(self, plan, key, rv, top):
        if not top and rv.rx and rv.rx in plan.nested:
            return plan.nested[rv.rx]
        o = rv.opts
        n = _Node()
        n.seq = _Node.count[0]
        _Node.count[0] += 1
        n.reverb, n.key, n.top = rv, key, top
        n.x = self._signal(plan, key, rv.input, o.input_wave_channel, "input")
        n.rate = n.x[2]
        fs = float(n.rate)
        n.N = self._length(plan, n.x)
        if n.N == 0:
            raise AugmentError("%s: empty input wave" % key)
        n.rir = None
        if rv.rir is not None:
            r = self._signal(plan, key, rv.rir, o.rir_channel, "impulse response")
            if r[2] != n.rate:
                raise AugmentError("%s: the impulse response's sample rate %g differs from the input's %g" % (key, r[2], n.rate))
            n.rir = r
        n.noises = []
        for src, snr, t in zip(rv.noises, rv.snrs, rv.start_times):
            s = self._signal(plan, key, src, o.noise_channel, "noise")
            if s[2] != n.rate:
                raise AugmentError("%s: an additive signal's sample rate %g differs from the input's %g" % (key, s[2], n.rate))
            n.noises.append((s, snr, sample_offset(t, fs)))
        n.M = output_length(o.duration, fs, n.N)
        n.shift = 0
        n.level = 1 + max([self._level(s) for s in [n.x, n.rir] + [s for s, _, _ in n.noises] if s is not None] + [-1])
        if o.shift_output and n.rir is not None:
            n.shift = self._rir(plan, n.rir).peak if n.rir[0] == "host" else None      # a nested RIR: known after its level
        n.out_off = None
        plan.nodes.append(n)
        if not top and rv.rx:
            plan.nested[rv.rx] = n
        return n

    @staticmethod
    def _level(sig):
        return sig[1].level if sig[0] == "node" else -1

    def _length(self, plan, sig):
        return sig[1].M if sig[0] == "node" else len(sig[3])

    def _host_samples(self, plan, sig):
        return sig[3]

    def _rir(self, plan, sig):
        k = sig[1] if sig[0] == "host" else ("node", id(sig[1]))
        if k not in plan.rirs:
            x = self._host_samples(plan, sig) if sig[0] == "host" else sig[1].host_out
            plan.rirs[k] = _Rir(x, float(sig[2]))
        return plan.rirs[k]

    def plan(self, entries, plan=None):
        """entries: [(key, Reverb)] -> Plan (the output length and rate of each entry known; nothing on the GPU yet).  Entries
        added to an existing plan share its decoded sources and impulse responses."""
        plan = plan or Plan()
        for key, rv in entries:
            plan.top.append(self._node(plan, key, rv, top=True))
        return plan

    @staticmethod
    def _reachable(tops):
        seen, todo = {}, list(tops)
        while todo:
            n = todo.pop()
            if id(n) in seen:
                continue
            seen[id(n)] = n
            todo += [s[1] for s in [n.x, n.rir] + [s for s, _, _ in n.noises] if s is not None and s[0] == "node"]
        return seen

    # --- evaluation ---
    def run(self, plan, out, out_offsets, sample_format=0, debug=False, tops=None):
        """Evaluate a plan (or only the entries ``tops`` of it, plan.top by default); entry i is written to out[out_offsets[i] ..
        + M_i) (a 1-D device tensor: int16 for sample_format 0, float32 for 1).  Returns per entry a dict of the scalars (P0, E,
        P1, level, noise powers and scales, clipped samples); with ``debug``, also the fp64 mixed waveform before the level
        (``y``) as a host array."""
        import torch
        hiplib.require_gpu()
        dev = torch.device(self.device)
        tops = plan.top if tops is None else tops
        assert len(tops) == len(out_offsets)
        for n, o in zip(tops, out_offsets):
            n.out_off = int(o)
        nodes_all = sorted(self._reachable(tops).values(), key=lambda n: n.seq)
        # one int16 pool for the batch: every host signal used as an input or noise, then every nested output
        pool_off, host_parts, total = {}, [], 0
        for n in nodes_all:
            for s in [n.x] + [s for s, _, _ in n.noises]:
                if s[0] == "host" and s[1] not in pool_off:
                    a = self._host_samples(plan, s)
                    pool_off[s[1]] = total
                    host_parts.append(a)
                    total += len(a)
        nested_off = {}
        for n in nodes_all:
            if not n.top:
                nested_off[id(n)] = total
                total += n.M
        host_pool = np.concatenate(host_parts + [np.zeros(total - sum(len(a) for a in host_parts) + 1, np.int16)])
        info = {}
        with torch.cuda.device(dev):
            sig = torch.from_numpy(host_pool).to(dev)
            levels = sorted(set(n.level for n in nodes_all))
            for lv in levels:
                nodes = [n for n in nodes_all if n.level == lv]
                self._run_level(plan, nodes, nodes_all, sig, pool_off, nested_off, out, sample_format, info, debug, dev)
                self.stats["levels"] += 1
        self.stats["evaluations"] += len(nodes_all)
        return [info[id(n)] for n in tops]

    def _sig_ref(self, s, pool_off, nested_off):
        """(offset in the pool, length) of an input / noise signal."""
        if s[0] == "host":
            return pool_off[s[1]], None
        return nested_off[id(s[1])], s[1].M

    def _run_level(self, plan, nodes, nodes_all, sig, pool_off, nested_off, out, fmt, info, debug, dev):
        import torch
        segs, seg_ix = [], {}

        def seg(off, ln):
            if (off, ln) not in seg_ix:
                seg_ix[(off, ln)] = len(segs)
                segs.append((off, ln))
            return seg_ix[(off, ln)]

        taps_parts, taps_off, taps_total = [], {}, 0
        jobs, conv_tiles, mix_tiles, write_top, write_nested = [], [], [], [], []
        refs, ref_snr, udesc, uparam, y_total = [], [], [], [], 0
        for u, n in enumerate(nodes):
            d = np.zeros(UTT_FIELDS, np.int64)
            x_off, _ = self._sig_ref(n.x, pool_off, nested_off)
            N = n.N
            d[X_OFF], d[N_], d[X_SEG] = x_off, N, seg(x_off, N)
            rir = self._rir(plan, n.rir) if n.rir is not None else None
            if rir is not None and n.shift is None:
                n.shift = rir.peak
            ylen = N + rir.L - 1 if rir is not None else N
            d[Y_OFF], d[Y_LEN] = y_total, ylen
            if rir is not None:
                k = id(rir)
                if k not in taps_off:
                    taps_off[k] = taps_total
                    taps_parts.append(rir.h)
                    taps_total += rir.L
                h0 = taps_off[k]
                d[RIR] = 1
                jobs.append((x_off, N, h0, rir.L, y_total))
                conv_tiles += [(len(jobs) - 1, t) for t in range(0, ylen, CONV_TILE)]
                W = rir.end - rir.start
                jobs.append((x_off, N, h0 + rir.start, W, -1))
                d[EARLY_TILE0] = len(conv_tiles)
                early = list(range(0, N + W - 1, CONV_TILE))
                d[EARLY_NTILES], d[EARLY_LEN] = len(early), N + W - 1
                conv_tiles += [(len(jobs) - 1, t) for t in early]
            d[REF0] = len(refs)
            for s, snr, off in n.noises:
                noff, nlen = self._sig_ref(s, pool_off, nested_off)
                if nlen is None:
                    nlen = len(self._host_samples(plan, s))
                refs.append((noff, nlen, off, seg(noff, nlen)))
                ref_snr.append(snr)
            d[NREF] = len(refs) - d[REF0]
            d[SHIFT], d[M_] = n.shift, n.M
            d[MIX_TILE0] = len(mix_tiles)
            mt = list(range(0, ylen, ELEM_TILE))
            d[MIX_NTILES] = len(mt)
            mix_tiles += [(u, t) for t in mt]
            if n.top:
                d[OUT_OFF] = n.out_off
                write_top += [(u, t) for t in range(0, n.M, ELEM_TILE)]
            else:
                d[OUT_OFF] = nested_off[id(n)]
                write_nested += [(u, t) for t in range(0, n.M, ELEM_TILE)]
            assert d[SHIFT] + min(N, n.M) <= ylen
            udesc.append(d)
            uparam.append((float(n.reverb.opts.volume), 1.0 if n.reverb.opts.normalize_output else 0.0))
            y_total += ylen
        U = len(nodes)
        cu = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).to(dev)  # noqa: E731
        seg_desc, power_tiles = [], []
        for si, (off, ln) in enumerate(segs):
            tl = list(range(0, ln, POWER_TILE))
            seg_desc.append((off, ln, len(power_tiles), len(tl)))
            power_tiles += [(si, t) for t in tl]
        t_seg = cu(np.array(seg_desc, np.int64).reshape(-1, 4), np.int64)
        t_utt = cu(np.stack(udesc), np.int64)
        t_refs = cu(np.array(refs, np.int64).reshape(-1, REF_FIELDS) if refs else np.zeros((1, REF_FIELDS), np.int64), np.int64)
        t_snr = cu(ref_snr or [0.0], np.float32)
        t_param = cu(uparam, np.float64)
        taps = cu(np.concatenate(taps_parts) if taps_parts else np.zeros(1, F32), np.float32)
        y = torch.empty(max(y_total, 1), dtype=torch.float64, device=dev)
        power_sumsq = torch.empty(max(len(power_tiles), 1), dtype=torch.float64, device=dev)
        conv_sumsq = torch.empty(max(len(conv_tiles), 1), dtype=torch.float64, device=dev)
        mix_sumsq = torch.empty(max(len(mix_tiles), 1), dtype=torch.float64, device=dev)
        utt_out = torch.empty((U, 4), dtype=torch.float64, device=dev)
        ref_power = torch.empty(max(len(refs), 1), dtype=torch.float64, device=dev)
        ref_scale = torch.empty(max(len(refs), 1), dtype=torch.float32, device=dev)
        clipped = torch.zeros(U, dtype=torch.int64, device=dev)
        if power_tiles:
            hiplib.augment_power(sig, t_seg, cu(power_tiles, np.int64), power_sumsq)
        if jobs:
            hiplib.augment_conv(sig, taps, cu(jobs, np.int64), cu(conv_tiles, np.int64), y, conv_sumsq)
        hiplib.augment_gains(t_utt, t_refs, t_snr, t_seg, power_sumsq, conv_sumsq, utt_out, ref_power, ref_scale)
        hiplib.augment_mix(sig, t_utt, t_refs, ref_scale, cu(mix_tiles, np.int64), y, mix_sumsq)
        hiplib.augment_level(t_utt, t_param, mix_sumsq, utt_out)
        if write_nested:
            hiplib.augment_write(y, t_utt, utt_out, cu(write_nested, np.int64), sig, 0, clipped)
        if write_top:
            hiplib.augment_write(y, t_utt, utt_out, cu(write_top, np.int64), out, fmt, clipped)
        # the scalars (a few doubles per evaluation) come back; the samples stay on the device
        uo, rp, rs, cl = utt_out.cpu().numpy(), ref_power.cpu().numpy(), ref_scale.cpu().numpy(), clipped.cpu().numpy()
        y_h = y.cpu().numpy() if debug else None
        for u, n in enumerate(nodes):
            d = udesc[u]
            r = slice(int(d[REF0]), int(d[REF0] + d[NREF]))
            rec = dict(key=n.key, P0=uo[u, 0], E=uo[u, 1], P1=uo[u, 2], level=uo[u, 3], noise_power=rp[r].copy(),
                       noise_scale=rs[r].copy(), clipped=int(cl[u]), M=n.M, shift=n.shift)
            for p in rec["noise_power"]:
                if p == 0:
                    logger.warning("%s: an additive signal is silent or empty; it adds nothing", n.key)
            if cl[u]:
                logger.warning("%s: %d samples clipped on writing", n.key, int(cl[u]))
            if debug:
                rec["y"] = y_h[int(d[Y_OFF]):int(d[Y_OFF] + d[Y_LEN])].copy()
            info[id(n)] = rec
            self.stats["samples_out"] += n.M
            self.stats["clipped"] += int(cl[u])
        # a nested output used as an impulse response is formed on the host (RIRs are short; the samples of utterances stay)
        for n in nodes:
            if not n.top and any(m.rir is not None and m.rir[0] == "node" and m.rir[1] is n for m in nodes_all):
                n.host_out = sig[nested_off[id(n)]:nested_off[id(n)] + n.M].cpu().numpy()

    def evaluate(self, entries, debug=False):
        """[(key, Reverb)] -> (list of int16 sample arrays, list of scalar dicts): the outputs brought back to the host."""
        import torch
        plan = self.plan(entries)
        lens = plan.lengths()
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        with torch.cuda.device(torch.device(self.device)):
            out = torch.empty(max(int(offs[-1]), 1), dtype=torch.int16, device=self.device)
            info = self.run(plan, out, offs[:-1], 0, debug)
            h = out.cpu().numpy()
        return [h[offs[i]:offs[i + 1]].copy() for i in range(len(lens))], info, plan


def duration_samples(key, rx, augmenter=None):
    """(samples, rate) of a wav.scp entry without evaluating it: an augmented entry's M from its options and inputs."""
    node = parse_rx(rx)
    if isinstance(node, Source):
        from . import sphere
        coded = sphere.recognise(key, rx)
        if coded is not None:                     # a recognised sph2pipe entry: its header says it
            return coded.n, coded.rate
        rate, x = mfcc.load_wav(key, rx)
        return x.shape[1], rate
    plan = (augmenter or Augmenter()).plan([(key, node)])
    return plan.top[0].M, plan.top[0].rate


class Pending(object):
    """An augmented wav.scp entry whose samples are not made yet: its output length ``M`` and ``rate`` are known, ``node`` is
    its place in ``plan`` (the plan it was planned into, which holds its decoded sources).  ``shape`` mirrors a 1-D sample
    array's."""

    def __init__(self, node, plan):
        self.node, self.plan = node, plan
        self.M, self.rate = node.M, node.rate
        self.shape = (node.M,)


def mfcc_compute(engine, augmenter, keys, items, vad=None, compress=False, device=False):
    """``mfcc.Mfcc.compute`` over a batch mixing clean waves (int16 arrays) and ``Pending`` entries: the augmented samples are
    written by the GPU straight into the buffer the MFCC kernel reads.  The entries of a batch may come from more than one
    plan (a reader plans an entry before it knows which batch takes it); each plan is evaluated on its own.
    ``compress``: as ``mfcc.Mfcc.compute``.  ``device``: ``mfcc.Mfcc.compute_device`` instead (the batch is one window, the
    results stay on the device; ``vad`` and ``compress`` do not apply)."""
    waves = [np.broadcast_to(np.int16(0), (it.M,)) if isinstance(it, Pending) else it for it in items]

    def fill(x, i, j, off):
        import torch
        sel = [k for k in range(i, j) if isinstance(items[k], Pending)]
        plans = []
        for k in sel:
            if not any(items[k].plan is p for p in plans):
                plans.append(items[k].plan)
        for p in plans:
            ks = [k for k in sel if items[k].plan is p]
            augmenter.run(p, x, [int(off[k - i]) for k in ks], 0 if x.dtype == torch.int16 else 1, tops=[items[k].node for k in ks])
    if device:
        return engine.compute_device(keys, waves, fill=fill)
    return engine.compute(keys, waves, vad=vad, fill=fill, compress=compress)
