"""Stage 1 of the recipe on the MI355X: MFCC features and the energy VAD from wav.scp.

What ``steps/make_mfcc.sh`` (compute-mfcc-feats) and ``sid/compute_vad_decision.sh`` (compute-vad) do with Kaldi binaries:

* ``MfccOptions`` / ``VadOptions`` -- Kaldi's option names and Kaldi's defaults; a recipe's values arrive through a
  ``--config`` file (``read_config``), not through changed defaults.
* ``MfccTables`` -- every table the kernel reads, built here: the window and the lifter x DCT-II in fp64 rounded to fp32
  once, the twiddles exp(-2 pi i k / N) likewise, the sparse mel bank in fp32 the way Kaldi's MelBanks forms it.
* ``read_wav`` / ``read_wav_scp`` -- RIFF/WAVE 16-bit PCM (plain or WAVE_FORMAT_EXTENSIBLE), paths and ``cmd |`` pipes; a pipe
  that is one recognised ``sph2pipe`` command is read in-process (xvector_amd/sphere.py), and comes to
  ``Mfcc.compute`` as a ``CodedWave``: the file's bytes are uploaded as they are and decoded on the device (csrc/xv_sphere.hip).
* ``Mfcc.compute`` -- MFCC rows and VAD decisions of many utterances per launch (csrc/xv_mfcc.hip); the decisions come back as
  a ``frontend.VadRuns``, so they plug straight into ``FrontEnd.apply``.  A wave at another rate than ``--sample-frequency`` is
  resampled on the device in front of the kernel when ``--allow-downsample`` / ``--allow-upsample`` permits (xvector_amd/resample.py,
  DESIGN.md §8.11).

There is no CPU path: the arithmetic runs on the GPU, and a missing device is an error.
"""
import io
import logging
import math
import struct
import subprocess

import numpy as np

from . import compress as cm, frontend, hiplib, resample

logger = logging.getLogger("mfcc")

FLT_EPSILON = np.float32(1.1920928955078125e-07)
WINDOW_TYPES = ("hamming", "hanning", "povey", "rectangular", "sine", "blackman")


# ------------------------------------------------------------------------------------------------
# options and --config files
# ------------------------------------------------------------------------------------------------
class _Options(object):
    """Options as attributes, under Kaldi's names with '-' -> '_'.  ``_FIELDS``: (name, type, Kaldi default)."""
    _FIELDS = ()

    def __init__(self, **kw):
        for name, _, default in self._FIELDS:
            setattr(self, name, default)
        for k, v in kw.items():
            self.set(k, v)

    @classmethod
    def names(cls):
        return [n for n, _, _ in cls._FIELDS]

    def set(self, name, value):
        name = name.replace("-", "_")
        types = {n: t for n, t, _ in self._FIELDS}
        if name not in types:
            raise ValueError("unknown option --%s" % name.replace("_", "-"))
        setattr(self, name, _convert(name, types[name], value))

    def update(self, pairs):
        for k, v in pairs:
            self.set(k, v)
        return self


def _convert(name, typ, value):
    if not isinstance(value, str):
        return typ(value)
    if typ is bool:
        v = value.strip().lower()
        if v in ("true", "t", "1", ""):
            return True
        if v in ("false", "f", "0"):
            return False
        raise ValueError("option --%s: invalid boolean %r" % (name.replace("_", "-"), value))
    try:
        return typ(value.strip())
    except ValueError:
        raise ValueError("option --%s: invalid value %r" % (name.replace("_", "-"), value))


class MfccOptions(_Options):
    """compute-mfcc-feats' options (FrameExtractionOptions + MelBanksOptions + MfccOptions + the binary's own), Kaldi's defaults.
    ``seed`` is this implementation's: it keys the dither noise together with the utterance id."""
    _FIELDS = (
        ("sample_frequency", float, 16000.0), ("frame_length", float, 25.0), ("frame_shift", float, 10.0),
        ("dither", float, 1.0), ("preemphasis_coefficient", float, 0.97), ("remove_dc_offset", bool, True),
        ("window_type", str, "povey"), ("round_to_power_of_two", bool, True), ("blackman_coeff", float, 0.42),
        ("snip_edges", bool, True), ("allow_downsample", bool, False), ("allow_upsample", bool, False),
        ("max_feature_vectors", int, -1),
        ("num_mel_bins", int, 23), ("low_freq", float, 20.0), ("high_freq", float, 0.0), ("vtln_low", float, 100.0),
        ("vtln_high", float, -500.0), ("debug_mel", bool, False),
        ("num_ceps", int, 13), ("use_energy", bool, True), ("energy_floor", float, 0.0), ("raw_energy", bool, True),
        ("cepstral_lifter", float, 22.0), ("htk_compat", bool, False),
        ("channel", int, -1), ("min_duration", float, 0.0), ("vtln_warp", float, 1.0), ("subtract_mean", bool, False),
        ("output_format", str, "kaldi"), ("seed", int, 0),
    )

    @property
    def frame_length_samples(self):
        return int(self.sample_frequency * 0.001 * self.frame_length)

    @property
    def frame_shift_samples(self):
        return int(self.sample_frequency * 0.001 * self.frame_shift)

    @property
    def padded_length(self):
        n = self.frame_length_samples
        return 1 << max(0, (n - 1).bit_length()) if self.round_to_power_of_two else n

    def num_frames(self, n_samples):
        """Kaldi's NumFrames (flush=true); works on arrays."""
        n = np.asarray(n_samples, np.int64)
        L, S = self.frame_length_samples, self.frame_shift_samples
        if self.snip_edges:
            return np.where(n < L, 0, 1 + (n - L) // S)
        return (n + S // 2) // S

    def first_sample(self, t):
        L, S = self.frame_length_samples, self.frame_shift_samples
        t = np.asarray(t, np.int64)
        return t * S if self.snip_edges else t * S + S // 2 - L // 2

    def check(self, resample=False):
        """What the kernel does not implement raises (the analogue of XV_ERR_UNSUPPORTED on the host side).  ``resample``: the
        caller puts the resampler (xvector_amd/resample.py) in front of the kernel, as ``Mfcc`` does, so --allow-downsample /
        --allow-upsample pass; the kernel itself takes one rate."""
        if not self.round_to_power_of_two:
            raise NotImplementedError("--round-to-power-of-two=false (non-power-of-two FFT) is not supported")
        if self.htk_compat:
            raise NotImplementedError("--htk-compat=true is not supported")
        if self.vtln_warp != 1.0:
            raise NotImplementedError("VTLN (--vtln-warp != 1) is not supported")
        if (self.allow_downsample or self.allow_upsample) and not resample:
            raise NotImplementedError("resampling (--allow-downsample / --allow-upsample) is not supported")
        if self.subtract_mean or self.max_feature_vectors != -1 or self.output_format != "kaldi":
            raise NotImplementedError("--subtract-mean, --max-feature-vectors and --output-format are not supported")
        if self.window_type not in WINDOW_TYPES:
            raise ValueError("invalid --window-type %r" % self.window_type)
        if not 128 <= self.padded_length <= 1024:
            raise NotImplementedError("padded frame length %d outside [128, 1024]" % self.padded_length)
        if self.frame_shift_samples < 1 or self.frame_length_samples < 2:
            raise ValueError("frame length / shift too small for --sample-frequency=%g" % self.sample_frequency)
        if not 1 <= self.num_ceps <= self.num_mel_bins <= 128:
            raise ValueError("need 1 <= --num-ceps <= --num-mel-bins <= 128")
        if self.dither < 0:
            raise ValueError("--dither must be >= 0")
        return self


class VadOptions(_Options):
    """compute-vad's options, Kaldi's defaults."""
    _FIELDS = (
        ("vad_energy_threshold", float, 5.0), ("vad_energy_mean_scale", float, 0.5), ("vad_frames_context", int, 0),
        ("vad_proportion_threshold", float, 0.6), ("omit_unvoiced_utts", bool, False),
    )


def parse_config_lines(lines, source="config"):
    """Kaldi's ``--config`` syntax: one ``--name=value`` (or bare ``--flag``) per line; '#' starts a comment anywhere on a line.
    Returns [(name, value)] in file order (a later line wins when applied)."""
    out = []
    for no, line in enumerate(lines, 1):
        line = line.split("#", 1)[0].strip()
        if not line:
            continue
        if not line.startswith("--"):
            raise ValueError("%s:%d: expected --name=value, got %r" % (source, no, line))
        name, eq, value = line[2:].partition("=")
        name = name.strip()
        if not name or " " in name:
            raise ValueError("%s:%d: malformed option %r" % (source, no, line))
        out.append((name, value.strip() if eq else ""))
    return out


def read_config(path):
    with open(path, "rt") as f:
        return parse_config_lines(f, path)


def fnv1a64(key):
    h = 0xCBF29CE484222325
    for b in key.encode():
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def dither_key(utt, seed=0):
    """The 64-bit Philox key of an utterance: FNV-1a of its id XOR the seed."""
    return fnv1a64(utt) ^ (int(seed) & 0xFFFFFFFFFFFFFFFF)


# ------------------------------------------------------------------------------------------------
# tables
# ------------------------------------------------------------------------------------------------
def window_function(opts):
    """Kaldi's FeatureWindowFunction, fp64 -> fp32."""
    L = opts.frame_length_samples
    i = np.arange(L, dtype=np.float64)
    a = 2.0 * math.pi / (L - 1)
    t = opts.window_type
    if t == "hanning":
        w = 0.5 - 0.5 * np.cos(a * i)
    elif t == "sine":
        w = np.sin(0.5 * a * i)
    elif t == "hamming":
        w = 0.54 - 0.46 * np.cos(a * i)
    elif t == "povey":
        w = np.power(0.5 - 0.5 * np.cos(a * i), 0.85)
    elif t == "rectangular":
        w = np.ones(L)
    elif t == "blackman":
        b = opts.blackman_coeff
        w = b - 0.5 * np.cos(a * i) + (0.5 - b) * np.cos(2 * a * i)
    else:
        raise ValueError("invalid --window-type %r" % t)
    return w.astype(np.float32)


def _mel32(f):
    return np.float32(1127.0) * np.log(np.float32(1.0) + np.asarray(f, np.float32) / np.float32(700.0))


def mel_banks(opts):
    """Kaldi's MelBanks in fp32: -> (first bin [B] int32, weights [B, maxlen] float32, lengths [B] int32).  FFT bin i < N/2 (the
    Nyquist bin never) at i * fs / N gets a triangular weight when its mel lies strictly inside (left, right)."""
    f32 = np.float32
    N = opts.padded_length
    B = opts.num_mel_bins
    nyq = f32(0.5) * f32(opts.sample_frequency)
    lo = f32(opts.low_freq)
    hi = f32(opts.high_freq) if opts.high_freq > 0 else nyq + f32(opts.high_freq)
    if not (0 <= lo < nyq and 0 < hi <= nyq and hi > lo):
        raise ValueError("bad mel frequency range [%g, %g] for sample frequency %g" % (lo, hi, opts.sample_frequency))
    width = f32(opts.sample_frequency) / f32(N)
    mlo, mhi = _mel32(lo), _mel32(hi)
    delta = (mhi - mlo) / f32(B + 1)
    mel = _mel32(width * np.arange(N // 2, dtype=np.float32))
    firsts, rows = [], []
    for b in range(B):
        left = mlo + f32(b) * delta
        center = mlo + f32(b + 1) * delta
        right = mlo + f32(b + 2) * delta
        inside = (mel > left) & (mel < right)
        up = (mel - left) / (center - left)
        down = (right - mel) / (right - center)
        w = np.where(mel <= center, up, down).astype(np.float32)
        idx = np.flatnonzero(inside)
        if len(idx) == 0:
            raise ValueError("mel band %d has no FFT bin: too many --num-mel-bins for this frame length" % b)
        firsts.append(int(idx[0]))
        rows.append(w[idx[0]:idx[-1] + 1] * inside[idx[0]:idx[-1] + 1])
    maxlen = max(len(r) for r in rows)
    weights = np.zeros((B, maxlen), np.float32)
    for b, r in enumerate(rows):
        weights[b, :len(r)] = r
    return np.array(firsts, np.int32), weights, np.array([len(r) for r in rows], np.int32)


def lifter_dct(opts):
    """Rows 0 .. num_ceps - 1 of Kaldi's DCT-II matrix times the cepstral lifter, fp64 -> fp32."""
    B, C = opts.num_mel_bins, opts.num_ceps
    k = np.arange(C, dtype=np.int64)[:, None]
    n = np.arange(B, dtype=np.int64)[None, :]
    # cos(pi (2n + 1) k / 2B) with the angle reduced to [0, 2 pi) in integers: an entry that is 0 stays below 1e-16 (unreduced,
    # the rounding of an angle near 400 leaves 1e-14 there, times a lifter of up to 1 + Q/2)
    d = math.sqrt(2.0 / B) * np.cos(math.pi * (((2 * n + 1) * k) % (4 * B)).astype(np.float64) / (2.0 * B))
    d[0, :] = math.sqrt(1.0 / B)
    Q = opts.cepstral_lifter
    if Q != 0:
        d *= (1.0 + 0.5 * Q * np.sin(math.pi * np.arange(C) / Q))[:, None]
    return d.astype(np.float32)


def twiddles(opts):
    """exp(-2 pi i k / N) for k < N/2 as (re, im) fp32 pairs, fp64 -> fp32."""
    N = opts.padded_length
    ang = -2.0 * math.pi * np.arange(N // 2, dtype=np.float64) / N
    return np.stack([np.cos(ang), np.sin(ang)], axis=1).astype(np.float32)


class MfccTables(object):
    def __init__(self, opts, resample=False):
        opts.check(resample)
        self.window = window_function(opts)
        self.mel_first, self.mel_w, self.mel_len = mel_banks(opts)
        self.lifter_dct = lifter_dct(opts)
        self.twiddle = twiddles(opts)

    def to_device(self, device):
        import torch
        return {k: torch.from_numpy(np.ascontiguousarray(getattr(self, k))).to(device)
                for k in ("window", "mel_first", "mel_len", "mel_w", "lifter_dct", "twiddle")}


# ------------------------------------------------------------------------------------------------
# WAV input
# ------------------------------------------------------------------------------------------------
class WavError(ValueError):
    pass


_EXTENSIBLE = 0xFFFE
_PCM_GUID_TAIL = b"\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71"


def read_wav(data, name="wav"):
    """RIFF/WAVE bytes -> (sample rate, int16 [channels, samples]).  16-bit PCM only (format 1, or WAVE_FORMAT_EXTENSIBLE with
    the PCM sub-format); unknown chunks are skipped (with their pad byte when odd-sized); a ``data`` size of 0 or 0xFFFFFFFF
    (what piped writers put there) means "to the end of the stream"."""
    if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"WAVE":
        raise WavError("%s: not a RIFF/WAVE file" % name)
    pos, fmt = 12, None
    while pos + 8 <= len(data):
        cid, size = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
        pos += 8
        if cid == b"fmt ":
            if size < 16:
                raise WavError("%s: short fmt chunk" % name)
            tag, nch, rate, _, align, bits = struct.unpack("<HHIIHH", data[pos:pos + 16])
            if tag == _EXTENSIBLE:
                if size < 40 or data[pos + 24 + 2:pos + 40] != _PCM_GUID_TAIL or struct.unpack("<H", data[pos + 24:pos + 26])[0] != 1:
                    raise WavError("%s: WAVE_FORMAT_EXTENSIBLE with a non-PCM sub-format" % name)
            elif tag != 1:
                raise WavError("%s: unsupported WAV format tag %d (16-bit PCM only)" % (name, tag))
            if bits != 16:
                raise WavError("%s: %d-bit samples are not supported (16-bit PCM only)" % (name, bits))
            if nch < 1 or align != 2 * nch:
                raise WavError("%s: inconsistent fmt chunk" % name)
            fmt = (nch, rate)
        elif cid == b"data":
            if fmt is None:
                raise WavError("%s: data chunk before fmt chunk" % name)
            end = len(data) if size in (0, 0xFFFFFFFF) else pos + size
            if end > len(data):
                raise WavError("%s: truncated data chunk (%d of %d bytes)" % (name, len(data) - pos, size))
            nch = fmt[0]
            n = (end - pos) // (2 * nch)
            x = np.frombuffer(data, dtype="<i2", count=n * nch, offset=pos).astype(np.int16)
            return fmt[1], x.reshape(n, nch).T
        pos += size + (size & 1)
    raise WavError("%s: no data chunk" % name)


def read_wav_scp(path):
    """Generator of (key, rxfilename) of a wav.scp."""
    with open(path, "rt") as f:
        for line in f:
            line = line.strip()
            if not line:
                continue
            key, _, rx = line.partition(" ")
            if not rx.strip():
                raise WavError("%s: no wave for key %s" % (path, key))
            yield key, rx.strip()


def load_wav(key, rx):
    """The wave of a wav.scp entry, (rate, int16 [channels, samples]): a path, or a ``cmd |`` pipe whose non-zero exit is an error
    naming the key.  A pipe that is one recognised ``sph2pipe`` command is read in-process (xvector_amd/sphere.py, DESIGN.md
    §8.12); every other one runs in the shell."""
    if rx.endswith("|"):
        from . import sphere
        coded = sphere.recognise(key, rx)
        if coded is not None:
            return coded.rate, sphere.decode_host(coded)
        p = subprocess.run(rx[:-1], shell=True, stdout=subprocess.PIPE)
        if p.returncode != 0:
            raise WavError("%s: command %r exited with status %d" % (key, rx[:-1], p.returncode))
        data = p.stdout
    else:
        with open(rx, "rb") as f:
            data = f.read()
    return read_wav(data, key)


class Wave(np.ndarray):
    """The samples of a wave that is to be resampled: an array that carries its own ``rate`` (Hz).  ``Mfcc.compute`` reads it."""
    rate = None

    def __array_finalize__(self, obj):
        self.rate = getattr(obj, "rate", None)


class CodedWave(object):
    """One channel of a recognised SPHERE entry whose samples are still coded (xvector_amd/sphere.py): ``Mfcc.compute`` uploads
    the file's data region as it lies on disk and decodes it on the device.  ``shape`` mirrors a 1-D sample array's; ``coded``
    (a ``sphere.Coded``) says where the bytes are (``read_into`` / ``region``: one read, no pass over the samples); ``coding``,
    ``channels`` (of the file), ``channel`` (the one taken), ``rate`` and ``ident`` (the file's identity: entries of one file
    share one upload) are what the engine reads."""
    __slots__ = ("coded", "channel", "shape")

    def __init__(self, coded, channel):
        assert 0 <= channel < coded.channels
        self.coded, self.channel = coded, int(channel)
        self.shape = (coded.n,)

    coding = property(lambda self: self.coded.coding)
    channels = property(lambda self: self.coded.channels)
    rate = property(lambda self: self.coded.rate)
    ident = property(lambda self: self.coded.ident)

    def region(self):
        return self.coded.region()


def _select_rules(key, rate, nch, n, opts):
    """compute-mfcc-feats' utterance rules on what a header says (``nch`` channels of ``n`` samples at ``rate``): -> (channel,
    whether it is to be resampled), or None (skipped, with Kaldi's warning)."""
    ch = opts.channel
    if ch == -1:
        if nch > 1:
            logger.warning("Channel not specified but you have data with %d channels; defaulting to zero (key %s)", nch, key)
        ch = 0
    elif ch < 0 or ch >= nch:
        logger.warning("Invalid channel %d/%d for key %s; skipping", ch, nch, key)
        return None
    resample = rate != opts.sample_frequency
    if resample and not (opts.allow_downsample or opts.allow_upsample):
        logger.warning("Sample frequency %g of key %s differs from --sample-frequency=%g; skipping (no resampling)",
                       rate, key, opts.sample_frequency)
        return None
    if resample and not (opts.allow_downsample if rate > opts.sample_frequency else opts.allow_upsample):
        # Kaldi's KALDI_ERR text; the binary's catch block turns it into a warning and goes on to the next utterance
        logger.warning("Waveform and config sample Frequency mismatch: %g .vs %g (use --allow-%s=true to allow %s) (key %s); "
                       "skipping", rate, opts.sample_frequency, *(("downsample", "downsampling") if rate > opts.sample_frequency
                                                                  else ("upsample", "upsampling")), key)
        return None
    if n < opts.min_duration * rate:                           # the original length at the original rate, as in Kaldi
        logger.warning("File: %s is too short (%g sec): producing no output.", key, n / float(rate))
        return None
    return ch, resample


def select_channel(key, rate, x, opts):
    """compute-mfcc-feats' utterance rules: -> int16 [samples], or None (skipped, with Kaldi's warning).  A wave whose rate
    differs from --sample-frequency comes back as a ``Wave`` carrying that rate when --allow-downsample / --allow-upsample
    permits resampling it."""
    sel = _select_rules(key, rate, x.shape[0], x.shape[1], opts)
    if sel is None:
        return None
    ch, resample = sel
    w = np.ascontiguousarray(x[ch])
    if resample:
        w = w.view(Wave)
        w.rate = int(rate)
    return w


def select_coded(key, coded, opts):
    """``select_channel`` for a recognised SPHERE entry (a ``sphere.Coded``), from its header alone: -> a ``CodedWave`` (decoded
    on the device), a ``Wave`` (an entry that is to be resampled is decoded on the host), or None (skipped)."""
    from . import sphere
    sel = _select_rules(key, coded.rate, coded.out_channels, coded.n, opts)
    if sel is None:
        return None
    ch, resample = sel
    if resample:
        w = np.ascontiguousarray(sphere.decode_host(coded)[ch]).view(Wave)
        w.rate = int(coded.rate)
        return w
    return CodedWave(coded, ch if coded.channel is None else coded.channel)


# ------------------------------------------------------------------------------------------------
# the device path
# ------------------------------------------------------------------------------------------------
class Mfcc(object):
    """MFCC (+ VAD) of batches of utterances on one GPU.  ``window_samples``: the most samples uploaded per launch."""

    def __init__(self, opts, vad_opts=None, device="cuda:0", window_samples=1 << 26, with_logmel=False):
        import torch
        hiplib.require_gpu()
        self.torch = torch
        self.opts = opts.check(resample=True)
        self.vad_opts = vad_opts
        self.device = torch.device(device)
        self.window_samples = int(window_samples)
        self.with_logmel = with_logmel
        self.tables = MfccTables(opts, resample=True)
        self._resampler = None                   # resample.Resampler, made when the first wave at another rate arrives
        self._dev = self.tables.to_device(self.device)
        # own stream, as FrontEnd: the results go back to the host, nothing on the compute stream waits for them
        self._stream = torch.cuda.Stream(device=self.device)
        self.stats = dict(utterances=0, samples=0, frames=0, launches=0, resampled=0, decoded=0, raw_bytes=0)

    def _windows(self, lens):
        """``lens``: the samples each utterance takes on the device (a resampled one: its output and its input)."""
        i, n = 0, len(lens)
        while i < n:
            j, tot = i, 0
            while j < n and (j == i or tot + lens[j] <= self.window_samples):
                tot += lens[j]
                j += 1
            yield i, j
            i = j

    def _rates(self, waves, rates):
        """Per utterance: None (the wave has --sample-frequency) or the integer rate it is resampled from."""
        fs = self.opts.sample_frequency
        rates = [getattr(w, "rate", None) for w in waves] if rates is None else list(rates)
        assert len(rates) == len(waves)
        rates = [None if r is None or r == fs else r for r in rates]
        if any(r is not None and isinstance(w, CodedWave) for w, r in zip(waves, rates)):
            raise NotImplementedError("a CodedWave at another rate than --sample-frequency: decode it on the host (select_coded)")
        for r in rates:
            if r is None:
                continue
            if int(fs) != fs or int(r) != r or r <= 0:
                raise NotImplementedError("resampling %r -> %r: only integer sample rates are supported" % (r, fs))
            if not (self.opts.allow_downsample if r > fs else self.opts.allow_upsample):
                raise ValueError("Waveform and config sample Frequency mismatch: %g .vs %g (use --allow-%s=true to allow %s)"
                                 % ((r, fs) + (("downsample", "downsampling") if r > fs else ("upsample", "upsampling"))))
        return [None if r is None else int(r) for r in rates]

    def compute(self, keys, waves, vad=None, fill=None, compress=False, rates=None):
        """keys: utterance ids (they key the dither); waves: 1-D int16 (or float32) sample arrays.  ``rates``: the sample rate of
        each wave (None: ``--sample-frequency``, or the ``rate`` a ``Wave`` carries); a wave at another rate is uploaded as it is
        and resampled on the device (xvector_amd/resample.py) into the fp32 sample buffer the MFCC kernel reads, when
        --allow-downsample / --allow-upsample permits, and its frames are those of the resampled length.  A ``CodedWave`` among
        ``waves`` (a SPHERE entry at --sample-frequency) is uploaded as the bytes of its file and decoded on the device
        (csrc/xv_sphere.hip): per window the data regions of the distinct files go up in one uint8 side buffer
        (at most 4 bytes per sample of the window budget) and one launch writes their samples into the sample buffer.  Returns
        ``(feats, vads, logmel)``: float32 [T, num_ceps] per utterance, a ``frontend.VadRuns`` (None unless VAD options were
        given or ``vad`` is True), and the float32 [T, num_mel_bins] log-mel energies (None unless ``with_logmel``).
        ``fill(x, i, j, offsets)``: called with each window's device sample buffer after the upload, before the MFCC launch, for
        utterances i .. j - 1 at ``offsets`` (the augmented entries of xvector_amd/augment.py write their samples there).
        ``compress``: the features come back as ``compress.Packed`` records (``rows``, ``cols``, ``payload``: a Kaldi
        CompressedMatrix payload for ``kaldi_io.write_cm_payload``) encoded on this engine's stream behind the MFCC launch; the
        fp32 table is not downloaded, the VAD still reads it on the device.  An utterance without frames gives a float32
        [0, num_ceps] array, as without ``compress``."""
        rates = self._rates(waves, rates)
        waves = [w if isinstance(w, CodedWave) else np.asarray(w).reshape(-1) for w in waves]
        assert len(keys) == len(waves)
        do_vad = self.vad_opts is not None if vad is None else bool(vad)
        feats, logmels, runs = [], [], frontend.VadRuns() if do_vad else None
        lens = [w.shape[0] for w in waves]
        if any(r is not None for r in rates):
            fs = int(self.opts.sample_frequency)
            lens = [n if r is None else n + int(resample.num_output_samples(n, r, fs)) for n, r in zip(lens, rates)]
        for i, j in self._windows(lens):
            f, lm, v = self._launch(keys[i:j], waves[i:j], do_vad,
                                    None if fill is None else (lambda x, off, i=i, j=j: fill(x, i, j, off)), compress, rates[i:j])
            feats += f
            logmels += lm
            if do_vad:
                runs.add_run(*v)
        return feats, runs, (logmels if self.with_logmel else None)

    def _upload_parts(self, waves, rates, res, cod, ns, off):
        """The sample buffer of a window that holds resampled utterances (``res``: their indices) or coded ones (``cod``): fp32
        when anything is resampled or a plain wave is, else int16.  The plain utterances at --sample-frequency are uploaded in
        place (one copy per run of neighbours); the resampled ones are uploaded at their own rate into a side buffer and
        resampled into their spans; the coded ones are uploaded as the bytes of their files, each distinct file once, and
        decoded into their spans -- all on this engine's stream."""
        torch = self.torch
        plain = [k for k in range(len(waves)) if rates[k] is None and not isinstance(waves[k], CodedWave)]
        f32 = bool(len(res)) or any(waves[k].dtype != np.int16 for k in plain)
        dtype = np.float32 if f32 else np.int16
        x = torch.empty(max(int(ns.sum()), 1), dtype=torch.float32 if f32 else torch.int16, device=self.device)
        is_plain = np.zeros(len(waves) + 1, bool)
        is_plain[plain] = True
        i, n = 0, len(waves)
        while i < n:
            if not is_plain[i]:
                i += 1
                continue
            j = i
            while is_plain[j]:
                j += 1
            run = np.concatenate([w.astype(dtype, copy=False) for w in waves[i:j]])
            if len(run):
                x[int(off[i]):int(off[i]) + len(run)].copy_(torch.from_numpy(run))
            i = j
        if len(res):
            if self._resampler is None:
                self._resampler = resample.Resampler(self.device)
            side = [waves[k] for k in res]
            sdtype = np.float32 if any(w.dtype != np.int16 for w in side) else np.int16
            pl = resample.plan([w.shape[0] for w in side], [rates[k] for k in res], int(self.opts.sample_frequency), out_offsets=off[res])
            assert np.array_equal(pl.out_samples, ns[res])
            flat = np.concatenate([w.astype(sdtype, copy=False) for w in side])
            self._resampler.run(torch.from_numpy(flat if len(flat) else np.zeros(1, sdtype)).to(self.device), pl, x)
            self.stats["resampled"] += len(res)
        if len(cod):
            from . import sphere
            raw, utt, tiles = sphere.pack([(waves[k].coded, waves[k].channel) for k in cod], off[cod])
            hiplib.wave_decode(torch.from_numpy(raw).to(self.device), utt, torch.from_numpy(tiles).to(self.device), x, 1 if f32 else 0)
            self.stats["decoded"] += len(cod)
            self.stats["raw_bytes"] += len(raw)
        return x

    def compute_device(self, keys, waves, rates=None, fill=None):
        """``compute`` for ONE window whose results stay on the device (``_launch`` without the downloads): everything ``compute``
        accepts -- plain, resampled and coded waves, the ``fill`` hook -- but the caller does the batching: the waves of a call go
        up in one sample buffer.  Returns ``(feats, vad, row0, T, ready)``: the cuda tensors feats [max(rows, 1), num_ceps]
        float32 and vad [max(rows, 1)] float32 (None without VAD options), the host int64 arrays row0 / T (utterance u is rows
        row0[u] .. row0[u] + T[u] - 1) and an event recorded on this engine's stream behind the last launch: another stream waits
        for it before it reads the tensors, and keeps them referenced until its own work on them is done."""
        torch = self.torch
        rates = self._rates(waves, rates)
        waves = [w if isinstance(w, CodedWave) else np.asarray(w).reshape(-1) for w in waves]
        assert len(keys) == len(waves)
        fill_w = None if fill is None else (lambda x, off: fill(x, 0, len(waves), off))
        with torch.cuda.device(self.device), torch.cuda.stream(self._stream):
            y, vad, _, row0, T, _, _ = self._device_pass(keys, waves, self.vad_opts is not None, fill_w, rates)
            ready = torch.cuda.Event()
            ready.record(self._stream)
        return y, vad, row0, T, ready

    def _device_pass(self, keys, waves, do_vad, fill, rates, want_T=False):
        """Upload + (resample, decode, fill) + MFCC + VAD of one window, on the current stream: the device tensors y, vad (None
        without ``do_vad``) and lm (None without ``with_logmel``), the host arrays row0 and T, and the device copies of both
        (d_T: None unless ``do_vad`` or ``want_T``)."""
        torch, opts = self.torch, self.opts
        n = len(waves)
        ns = np.array([w.shape[0] for w in waves], np.int64)
        res = np.array([k for k in range(n) if rates is not None and rates[k] is not None], np.int64)
        if len(res):                                # frames, rows and offsets: of the lengths after resampling
            ns[res] = resample.num_output_samples(ns[res], np.array([rates[k] for k in res], np.int64), int(opts.sample_frequency))
        T = opts.num_frames(ns).astype(np.int64)
        row0 = np.zeros(n, np.int64)
        np.cumsum(T[:-1], out=row0[1:])
        rows = int(T.sum())
        off = np.zeros(n, np.int64)
        np.cumsum(ns[:-1], out=off[1:])
        cod = np.array([k for k in range(n) if isinstance(waves[k], CodedWave)], np.int64)
        parts = len(res) or len(cod)
        if not parts:
            dtype = np.float32 if any(w.dtype != np.int16 for w in waves) else np.int16
            flat = np.concatenate([w.astype(dtype, copy=False) for w in waves]) if n else np.zeros(0, dtype)
        keyv = np.array([dither_key(k, opts.seed) for k in keys], np.uint64).view(np.int64)
        C, B = opts.num_ceps, opts.num_mel_bins
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device, non_blocking=False)  # noqa: E731
        x = self._upload_parts(waves, rates, res, cod, ns, off) if parts else dev(flat if len(flat) else np.zeros(1, dtype))
        if fill is not None:
            fill(x, off)
        d_off, d_ns, d_row0, d_key = dev(off), dev(ns), dev(row0), dev(keyv)
        y = torch.empty((max(rows, 1), C), dtype=torch.float32, device=self.device)
        lm = torch.empty((max(rows, 1), B), dtype=torch.float32, device=self.device) if self.with_logmel else None
        hiplib.mfcc(x, d_off, d_ns, d_row0, d_key, rows, self._dev, opts, y, lm)
        d_T = dev(T.astype(np.int32)) if do_vad or want_T else None
        vad = None
        if do_vad:
            vad = torch.empty(max(rows, 1), dtype=torch.float32, device=self.device)
            hiplib.vad_energy(y, d_row0, d_T, self.vad_opts, vad)
        self.stats["utterances"] += n
        self.stats["samples"] += int(ns.sum())
        self.stats["frames"] += rows
        self.stats["launches"] += 1
        return y, vad, lm, row0, T, d_row0, d_T

    def _launch(self, keys, waves, do_vad, fill=None, compress=False, rates=None):
        torch, C = self.torch, self.opts.num_ceps
        with torch.cuda.device(self.device), torch.cuda.stream(self._stream):
            y, vad, lm, row0, T, d_row0, d_T = self._device_pass(keys, waves, do_vad, fill, rates, want_T=compress)
            rows = int(T.sum())
            if do_vad:
                vad_h = vad[:rows].cpu().numpy()
            if compress:
                block, records = cm.encode(y, row0, T, C, stream=self._stream, keys=keys, d_row0=d_row0, d_T=d_T)
            else:
                y_h = y[:rows].cpu().numpy()
            lm_h = lm[:rows].cpu().numpy() if lm is not None else None
        bounds = list(zip(row0.tolist(), (row0 + T).tolist()))
        if compress:
            feats = [p if p.rows else np.zeros((0, C), np.float32) for p in cm.packed(block, records, C)]
        else:
            feats = [y_h[a:b] for a, b in bounds]
        logmel = [lm_h[a:b] for a, b in bounds] if lm_h is not None else []
        v = None
        if do_vad:
            offs = np.concatenate([[0], np.cumsum(T)]).astype(np.int64)
            v = (vad_h, offs)
        return feats, logmel, v


def compute_vad(mats, vad_opts, device="cuda:0"):
    """compute-vad on feature matrices already in memory (the kernel reads column 0): -> ``frontend.VadRuns``."""
    import torch
    hiplib.require_gpu()
    dev = torch.device(device)
    T = np.array([m.shape[0] for m in mats], np.int64)
    row0 = np.zeros(len(mats), np.int64)
    np.cumsum(T[:-1], out=row0[1:])
    rows = int(T.sum())
    runs = frontend.VadRuns()
    if not len(mats):
        return runs
    c0 = np.zeros((max(rows, 1), 1), np.float32)
    for m, r in zip(mats, row0.tolist()):
        if m.shape[0]:
            c0[r:r + m.shape[0], 0] = m[:, 0]
    with torch.cuda.device(dev):
        out = torch.empty(max(rows, 1), dtype=torch.float32, device=dev)
        hiplib.vad_energy(torch.from_numpy(c0).to(dev), torch.from_numpy(row0).to(dev), torch.from_numpy(T.astype(np.int32)).to(dev),
                          vad_opts, out)
        runs.add_run(out[:rows].cpu().numpy(), np.concatenate([[0], np.cumsum(T)]).astype(np.int64))
    return runs


def wav_bytes(x, rate, extensible=False, streaming=False, extra_chunks=()):
    """int16 [samples] or [channels, samples] -> RIFF/WAVE bytes (tests and the bench tool write their inputs with it).
    ``streaming``: the RIFF and data sizes are 0xFFFFFFFF, as piped writers leave them; ``extra_chunks``: (id, payload) pairs
    placed before the data chunk."""
    x = np.asarray(x, np.int16)
    if x.ndim == 1:
        x = x[None]
    nch = x.shape[0]
    payload = np.ascontiguousarray(x.T).astype("<i2").tobytes()
    if extensible:
        fmt = struct.pack("<HHIIHHHHI", _EXTENSIBLE, nch, int(rate), int(rate) * 2 * nch, 2 * nch, 16, 22, 16, 0) + \
            struct.pack("<H", 1) + _PCM_GUID_TAIL
    else:
        fmt = struct.pack("<HHIIHH", 1, nch, int(rate), int(rate) * 2 * nch, 2 * nch, 16)
    body = io.BytesIO()
    body.write(b"WAVE")
    body.write(b"fmt " + struct.pack("<I", len(fmt)) + fmt)
    for cid, data in extra_chunks:
        body.write(cid + struct.pack("<I", len(data)) + data + (b"\x00" if len(data) & 1 else b""))
    body.write(b"data" + struct.pack("<I", 0xFFFFFFFF if streaming else len(payload)) + payload)
    b = body.getvalue()
    return b"RIFF" + struct.pack("<I", 0xFFFFFFFF if streaming else len(b)) + b
