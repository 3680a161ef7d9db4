"""Sample-rate conversion on the MI355X for --allow-downsample / --allow-upsample (csrc/xv_resample.hip).

Kaldi's ``ResampleWaveform``: a ``LinearResample`` (Hann-windowed sinc, 6 zeros, cutoff 0.99 of the lower Nyquist frequency)
applied once to the whole wave.  The host forms the tables of a rate pair (``tables``) and the layout of a launch (``plan``);
the sums run on the GPU, one fp32 ``fmaf`` chain per output sample in a fixed order, so a sample's bits depend on its own wave
only.  The result stays fp32 and goes straight into the buffer the MFCC kernel reads (``Resampler.run``).

There is no CPU path: a missing device is an error.
"""
import functools
import math

import numpy as np

from . import hiplib

NUM_ZEROS = 6
OUT_TILE = 1024                    # XV_RS_OUT_TILE: outputs per workgroup
MAX_TABLES = 8                     # XV_RS_MAX_TABLES: rate pairs per launch
TAB_FIELDS = 6                     # XV_RS_TAB_FIELDS: UI, UO, ROW, PHASE_OFF, W_OFF, SPAN


def _pair(fi, fo):
    if int(fi) != fi or int(fo) != fo or fi <= 0 or fo <= 0:
        raise ValueError("sample rates must be positive integers, got %r -> %r" % (fi, fo))
    if int(fi) == int(fo):
        raise ValueError("nothing to resample: both rates are %d" % fi)
    return int(fi), int(fo)


@functools.lru_cache(maxsize=None)
def _tables(fi, fo):
    g = math.gcd(fi, fo)
    Ui, Uo = fi // g, fo // g
    cutoff = float(np.float32(0.99 * 0.5 * min(fi, fo)))
    ww = NUM_ZEROS / (2.0 * cutoff)
    t_out = np.arange(Uo, dtype=np.float64) / float(fo)
    first = np.ceil((t_out - ww) * fi).astype(np.int64)
    last = np.floor((t_out + ww) * fi).astype(np.int64)
    ntaps = last - first + 1
    row = int(ntaps.max())
    j = np.arange(row, dtype=np.int64)[None, :]
    # Kaldi's FilterFunc takes the time difference as a float and evaluates in double
    t = ((first[:, None] + j) / float(fi) - t_out[:, None]).astype(np.float32).astype(np.float64)
    window = np.where(np.abs(t) < ww, 0.5 * (1.0 + np.cos(2.0 * math.pi * cutoff / NUM_ZEROS * t)), 0.0)
    nz = t != 0
    filt = np.where(nz, np.sin(2.0 * math.pi * cutoff * t) / (math.pi * np.where(nz, t, 1.0)), 2.0 * cutoff)
    w = (filt.astype(np.float32) * window.astype(np.float32)) / np.float32(fi)
    w = np.where(j < ntaps[:, None], w, np.float32(0)).astype(np.float32)
    # the span of a tile, for every phase its first output can have; the kernel stages [first tap of the first output, last tap
    # of the last one], which needs both ends non-decreasing from one output to the next
    o = np.arange(Uo + OUT_TILE, dtype=np.int64)
    k0 = first[o % Uo] + (o // Uo) * Ui
    end = k0 + ntaps[o % Uo]
    if np.any(np.diff(k0) < 0) or np.any(np.diff(end) < 0):
        raise ValueError("resampling %d -> %d: the tap ranges are not monotone" % (fi, fo))
    span = int((end[OUT_TILE - 1:OUT_TILE - 1 + Uo] - k0[:Uo]).max())
    for a in (first, ntaps, w):
        a.setflags(write=False)
    return Ui, Uo, first.astype(np.int32), ntaps.astype(np.int32), w, span


def tables(fi, fo):
    """-> (Ui, Uo, first [Uo] int32, ntaps [Uo] int32, w [Uo, row] float32) of the pair fi -> fo; cached, read-only."""
    return _tables(*_pair(fi, fo))[:5]


def num_output_samples(n, fi, fo):
    """Outputs of ``n`` input samples (LinearResample::GetNumOutputSamples with flush = true); n, fi may be arrays."""
    n, fi = np.asarray(n, np.int64), np.asarray(fi, np.int64)
    fo = np.asarray(fo, np.int64)
    g = np.gcd(fi, fo)
    L = n * (fo // g)
    tpo = fi // g
    last = L // tpo
    last = last - (last * tpo == L)
    return np.where(L <= 0, 0, last + 1).astype(np.int64)


class Plan(object):
    """The layout of one launch set: ``utt`` int64 [5, U] = (in_offset, in_samples, out_offset, out_samples, table) rows, ``tab``
    int64 [n_tables, TAB_FIELDS] descriptors, the concatenated ``first`` / ``ntaps`` / ``w`` tables, ``tiles`` int64 [n_tiles, 2] =
    (utterance, first output), ``pairs`` (the (fi, fo) of each table), ``in_total`` / ``out_total`` (elements the buffers need)."""

    def __init__(self, utt, tab, first, ntaps, w, tiles, pairs, in_total, out_total):
        self.utt, self.tab, self.first, self.ntaps, self.w, self.tiles = utt, tab, first, ntaps, w, tiles
        self.pairs, self.in_total, self.out_total = pairs, in_total, out_total

    @property
    def out_samples(self):
        return self.utt[3]


def pool(pairs):
    """The descriptors and concatenated tables of a list of (fi, fo) pairs: -> (tab, first, ntaps, w)."""
    tab = np.zeros((len(pairs), TAB_FIELDS), np.int64)
    firsts, ntapss, ws, po, wo = [], [], [], 0, 0
    for t, (fi, fo) in enumerate(pairs):
        Ui, Uo, first, ntaps, w, span = _tables(fi, fo)
        tab[t] = (Ui, Uo, w.shape[1], po, wo, span)
        firsts.append(first), ntapss.append(ntaps), ws.append(w.reshape(-1))
        po += Uo
        wo += w.size
    cat = lambda xs, dt: np.concatenate(xs) if xs else np.zeros(0, dt)  # noqa: E731
    return tab, cat(firsts, np.int32), cat(ntapss, np.int32), cat(ws, np.float32)


def tile_list(out_samples):
    """[n_tiles, 2] int64 = (utterance, first output) covering out_samples[u] outputs of every utterance in OUT_TILE steps."""
    out_samples = np.asarray(out_samples, np.int64)
    nt = (out_samples + OUT_TILE - 1) // OUT_TILE
    u = np.repeat(np.arange(len(out_samples), dtype=np.int64), nt)
    start = np.zeros(len(out_samples), np.int64)
    np.cumsum(nt[:-1], out=start[1:])
    o0 = (np.arange(int(nt.sum()), dtype=np.int64) - np.repeat(start, nt)) * OUT_TILE
    return np.stack([u, o0], axis=1) if len(u) else np.zeros((0, 2), np.int64)


def plan(lengths, rates, rate_out, in_offsets=None, out_offsets=None):
    """The launch layout for waves of ``lengths`` samples at ``rates`` (every one different from ``rate_out``).  Inputs and outputs
    lie back to back in utterance order unless ``in_offsets`` / ``out_offsets`` (elements) place them."""
    lengths = np.asarray(lengths, np.int64).reshape(-1)
    n = len(lengths)
    pairs = []
    table = np.zeros(n, np.int64)
    for i, r in enumerate(rates):
        pr = _pair(r, rate_out)
        if pr not in pairs:
            pairs.append(pr)
        table[i] = pairs.index(pr)
    assert len(table) == n and np.all(lengths >= 0)
    outs = num_output_samples(lengths, np.array([pairs[t][0] for t in table], np.int64), rate_out)

    def offsets(given, lens):
        if given is not None:
            return np.asarray(given, np.int64).reshape(-1)
        off = np.zeros(n, np.int64)
        np.cumsum(lens[:-1], out=off[1:])
        return off

    in_off, out_off = offsets(in_offsets, lengths), offsets(out_offsets, outs)
    utt = np.stack([in_off, lengths, out_off, outs, table]) if n else np.zeros((5, 0), np.int64)
    tab, first, ntaps, w = pool(pairs)
    return Plan(np.ascontiguousarray(utt), tab, first, ntaps, w, tile_list(outs), pairs,
                int((in_off + lengths).max()) if n else 0, int((out_off + outs).max()) if n else 0)


class Resampler(object):
    """Launches of xv_resample_f32 on the current stream of ``device``; the device copies of the tables are kept per pair list."""

    def __init__(self, device="cuda:0"):
        import torch
        hiplib.require_gpu()
        self.torch = torch
        self.device = torch.device(device)
        self._pools = {}
        self.stats = dict(launches=0, utterances=0, in_samples=0, out_samples=0)

    def _pool(self, pairs):
        key = tuple(pairs)
        if key not in self._pools:
            dev = lambda a: self.torch.from_numpy(np.ascontiguousarray(a)).to(self.device)  # noqa: E731
            tab, first, ntaps, w = pool(pairs)
            self._pools[key] = (tab, dev(first), dev(ntaps), dev(w))
        return self._pools[key]

    def run(self, inp, pl, out):
        """inp: the 1-D int16 or float32 device tensor holding every input at pl.utt[0]; out: the 1-D float32 device tensor the
        outputs go to at pl.utt[2].  Enqueues on the current stream; more than MAX_TABLES rate pairs take several launches."""
        torch = self.torch
        for t0 in range(0, len(pl.pairs), MAX_TABLES):
            pairs = pl.pairs[t0:t0 + MAX_TABLES]
            sel = np.flatnonzero((pl.utt[4] >= t0) & (pl.utt[4] < t0 + MAX_TABLES))
            utt = np.ascontiguousarray(pl.utt[:, sel])
            utt[4] -= t0
            tiles = pl.tiles if len(sel) == pl.utt.shape[1] else tile_list(utt[3])
            if not len(tiles):
                continue
            tab, first, ntaps, w = self._pool(pairs)
            hiplib.resample(inp, utt, tab, first, ntaps, w, torch.from_numpy(tiles).to(self.device), out)
            self.stats["launches"] += 1
        self.stats["utterances"] += pl.utt.shape[1]
        self.stats["in_samples"] += int(pl.utt[1].sum())
        self.stats["out_samples"] += int(pl.utt[3].sum())


def resample_waves(waves, rates, rate_out, device="cuda:0"):
    """Each 1-D int16 (or float32) wave at its rate -> its float32 wave at ``rate_out``, all in one launch."""
    import torch
    waves = [np.asarray(w).reshape(-1) for w in waves]
    dtype = np.int16 if all(w.dtype == np.int16 for w in waves) else np.float32
    pl = plan([len(w) for w in waves], rates, rate_out)
    rs = Resampler(device)
    with torch.cuda.device(rs.device):
        flat = np.concatenate([w.astype(dtype, copy=False) for w in waves]) if waves else np.zeros(0, dtype)
        inp = torch.from_numpy(flat if len(flat) else np.zeros(1, dtype)).to(rs.device)
        out = torch.zeros(max(pl.out_total, 1), dtype=torch.float32, device=rs.device)
        rs.run(inp, pl, out)
        y = out.cpu().numpy()
    return [y[o:o + m].copy() for o, m in zip(pl.utt[2].tolist(), pl.utt[3].tolist())]
