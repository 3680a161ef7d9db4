"""NIST SPHERE files read natively: what ``sph2pipe -f wav -p [-c N] x.sph |`` in a wav.scp does, without the process
(csrc/xv_sphere.hip).

Every data-preparation script of the recipe writes its waves as such pipes.  This module

* reads the header (``parse_header``): ``NIST_1A``, the header size, ``name -type value`` lines up to ``end_head``;
* recognises the command (``parse_command``): one pipeline stage whose program is ``sph2pipe`` with ``-f wav`` / ``-f rif``,
  ``-p``, ``-c 1`` / ``-c 2`` and one input file -- anything else is not native and runs in the shell as before;
* puts the two together (``recognise``): a ``Coded`` describes where the samples of an entry lie in its file and how they are
  coded, from the header alone;
* decodes on the host (``decode_host``: RIRs, noises, the inputs of augmented entries, waves to be resampled) with two 256-entry
  G.711 tables built from the formulas of include/xvector_hip.h, and lays out the device decode of a feature window
  (``pack``: the raw data regions go to the GPU as they lie in the files, ``xv_wave_decode`` expands them there).

``XVECTOR_NATIVE_SPH=0`` in the environment sends every entry through the shell.
"""
import logging
import os
import shlex

import numpy as np

from . import mfcc

logger = logging.getLogger("mfcc")

DEC_TILE = 4096                   # XV_DEC_TILE: output elements per workgroup of xv_wave_decode
DEC_FIELDS = 8                    # XV_DEC_FIELDS: RAW_OFF, N, STRIDE, CH_OFF, CODING, OUT_OFF, two reserved
RAW_OFF, N_, STRIDE, CH_OFF, CODING, OUT_OFF = range(6)
PCM16_LE, PCM16_BE, ULAW, ALAW = range(4)       # XV_DEC_PCM16_LE ...
_CODINGS = {"pcm": "pcm", "ulaw": "ulaw", "mu-law": "ulaw", "pculaw": "ulaw", "alaw": "alaw"}
_MAGIC = b"NIST_1A\n"
_SHELL_META = frozenset("$`*?[]{}()<>&;!~#\n")          # anywhere in a command, quoted or not: the entry is left to the shell


# ------------------------------------------------------------------------------------------------
# G.711
# ------------------------------------------------------------------------------------------------
def _ulaw_table():
    u = ~np.arange(256, dtype=np.int32) & 0xFF
    t = (((u & 15) << 3) + 132) << ((u >> 4) & 7)
    return np.where(u & 128, 132 - t, t - 132).astype(np.int16)


def _alaw_table():
    a = np.arange(256, dtype=np.int32) ^ 0x55
    t = (a & 15) << 4
    s = (a >> 4) & 7
    t = t + np.where(s > 0, 0x108, 8)
    t = np.where(s > 1, t << np.maximum(s - 1, 0), t)
    return np.where(a & 128, t, -t).astype(np.int16)


ULAW_TABLE = _ulaw_table()
ALAW_TABLE = _alaw_table()
for _t in (ULAW_TABLE, ALAW_TABLE):
    _t.setflags(write=False)


# ------------------------------------------------------------------------------------------------
# the header
# ------------------------------------------------------------------------------------------------
class Header(object):
    """The fields of a SPHERE header that say where the samples are: ``size`` (bytes of the header), ``rate``, ``channels``,
    ``n_bytes`` per sample, ``byte_format`` ('01', '10' or '1'), ``coding`` ('pcm', 'ulaw' or 'alaw'), ``shorten`` (the
    coding carries an ``embedded-shorten`` suffix: the data are compressed) and ``sample_count`` (None when absent)."""
    __slots__ = ("size", "rate", "channels", "n_bytes", "byte_format", "coding", "shorten", "sample_count")


def parse_header(data, name="sph"):
    """The first bytes of a file (at least its whole header, or the file when it is shorter) -> Header."""
    if data[:8] != _MAGIC:
        raise mfcc.WavError("%s: not a NIST SPHERE file (no NIST_1A magic)" % name)
    nl = data.find(b"\n", 8)
    try:
        size = int(data[8:nl].strip()) if nl > 0 else -1
    except ValueError:
        size = -1
    if size < 16 or size % 8:
        raise mfcc.WavError("%s: bad SPHERE header size %r" % (name, bytes(data[8:max(nl, 8)][:16])))
    fields, ended = {}, False
    for line in bytes(data[nl + 1:size]).split(b"\n"):
        line = line.decode("latin-1").strip()
        if line == "end_head":
            ended = True
            break
        if not line or line.startswith(";"):
            continue
        parts = line.split(None, 2)
        if len(parts) == 3 and parts[1].startswith("-"):
            fields[parts[0]] = parts[2].strip()
    if not ended:
        raise mfcc.WavError("%s: SPHERE header without end_head in its %d bytes" % (name, size))

    def integer(field, default=None):
        if field not in fields:
            if default is None:
                raise mfcc.WavError("%s: SPHERE header without %s" % (name, field))
            return default
        try:
            return int(fields[field])
        except ValueError:
            raise mfcc.WavError("%s: SPHERE header field %s = %r is not an integer" % (name, field, fields[field]))

    h = Header()
    h.size = size
    h.rate = integer("sample_rate")
    h.channels = integer("channel_count")
    h.n_bytes = integer("sample_n_bytes")
    h.sample_count = integer("sample_count", -1)
    if h.sample_count < 0:
        h.sample_count = None
    coding = fields.get("sample_coding", "pcm").lower()
    base, _, rest = coding.partition(",")
    h.shorten = "embedded-shorten" in rest
    if base not in _CODINGS or (rest and not h.shorten):
        raise mfcc.WavError("%s: unknown SPHERE sample_coding %r" % (name, fields["sample_coding"]))
    h.coding = _CODINGS[base]
    h.byte_format = fields.get("sample_byte_format", "1" if h.n_bytes == 1 else "")
    if h.byte_format not in ("01", "10", "1"):
        raise mfcc.WavError("%s: SPHERE header with sample_byte_format %r" % (name, h.byte_format))
    if h.rate <= 0 or h.channels < 1 or h.n_bytes < 1:
        raise mfcc.WavError("%s: SPHERE header with sample_rate %d, channel_count %d, sample_n_bytes %d"
                            % (name, h.rate, h.channels, h.n_bytes))
    return h


def read_header(path, name="sph"):
    """-> (Header, size of the file in bytes, (st_dev, st_ino))."""
    try:
        with open(path, "rb") as f:
            st = os.fstat(f.fileno())
            data = f.read(1024)
            if data[:8] == _MAGIC:
                nl = data.find(b"\n", 8)
                try:
                    size = int(data[8:nl].strip()) if nl > 0 else 0
                except ValueError:
                    size = 0
                if 1024 < size <= 1 << 20:
                    data += f.read(size - 1024)
    except OSError as e:
        raise mfcc.WavError("%s: cannot read %r: %s" % (name, path, e))
    return parse_header(data, name), st.st_size, (st.st_dev, st.st_ino)


_WARNED = set()


def sample_count(h, file_bytes, name="sph", ident=None):
    """The samples (frames) of a file: the whole frames present after the header, capped at ``sample_count`` when the header has
    one.  A header that promises more than the file holds is warned about once per file."""
    present = max(file_bytes - h.size, 0) // (h.n_bytes * h.channels)
    if h.sample_count is None:
        return present
    if h.sample_count > present and ident not in _WARNED:
        if ident is not None:
            _WARNED.add(ident)
        logger.warning("%s: the SPHERE header promises %d samples, the file holds %d; reading those", name, h.sample_count, present)
    return min(present, h.sample_count)


# ------------------------------------------------------------------------------------------------
# the command
# ------------------------------------------------------------------------------------------------
class Command(object):
    """A recognised sph2pipe stage: the input ``path``, ``channel`` (None: all, else the 0-based index of ``-c``), ``pcm`` (-p)."""
    __slots__ = ("path", "channel", "pcm")


def parse_command(rx):
    """An rxfilename -> Command when it is exactly ``sph2pipe [-f wav|rif] [-p] [-c 1|2] <file> |`` (the options in any order,
    ``-f`` required), else None: the entry is not native and runs in the shell."""
    from . import augment
    rx = rx.strip()
    if not rx.endswith("|"):
        return None
    if any(c in _SHELL_META for c in rx[:-1]):
        return None                     # expansions, redirections, lists: only a shell knows what they come to
    try:
        stages = augment.split_pipeline(rx[:-1])
        if len(stages) != 1:
            return None
        argv = shlex.split(stages[0])
    except ValueError:                  # AugmentError is one: an unterminated quote is the shell's to report
        return None
    if not argv or os.path.basename(argv[0]) != "sph2pipe":
        return None
    fmt, chan, pcm, pos = None, None, False, []
    i = 1
    while i < len(argv):
        a = argv[i]
        if a in ("-f", "-c"):
            if i + 1 >= len(argv) or (fmt if a == "-f" else chan) is not None:
                return None
            if a == "-f":
                fmt = argv[i + 1]
            else:
                chan = argv[i + 1]
            i += 2
            continue
        if a == "-p":
            pcm = True
        elif a.startswith("-") and a != "-":
            return None                 # -t, -s, -u, -a, -h, joined forms such as -fwav: the binary's to interpret
        else:
            pos.append(a)
        i += 1
    if fmt not in ("wav", "rif") or chan not in (None, "1", "2") or len(pos) != 1 or pos[0] == "-":
        return None
    c = Command()
    c.path, c.channel, c.pcm = pos[0], None if chan is None else int(chan) - 1, pcm
    return c


class Coded(object):
    """Where the samples of a recognised entry lie: ``path``, ``ident`` ((st_dev, st_ino) of the file), ``data_off`` (the header
    size), ``n`` samples per channel, ``rate``, ``channels`` (of the file), ``stride`` (bytes of a frame), ``width`` (bytes of a
    sample), ``coding`` (PCM16_LE, PCM16_BE, ULAW, ALAW) and ``channel`` (None: every channel, else the one ``-c`` chose)."""
    __slots__ = ("path", "ident", "data_off", "n", "rate", "channels", "stride", "width", "coding", "channel")

    @property
    def out_channels(self):
        return self.channels if self.channel is None else 1

    @property
    def region_bytes(self):
        return self.n * self.stride

    def read_into(self, dst):
        """The data region (``region_bytes`` bytes as they lie in the file) into the uint8 array ``dst``: one read."""
        with open(self.path, "rb") as f:
            f.seek(self.data_off)
            got = f.readinto(memoryview(dst))
        if got != self.region_bytes:
            raise mfcc.WavError("%s: read %d of %d bytes" % (self.path, got, self.region_bytes))

    def region(self):
        """The data region as a uint8 array (one read)."""
        buf = np.empty(self.region_bytes, np.uint8)
        if len(buf):
            self.read_into(buf)
        return buf


def native_enabled():
    return os.environ.get("XVECTOR_NATIVE_SPH", "1").strip().lower() not in ("0", "false", "no", "off")


class NotNative(mfcc.WavError):
    """A SPHERE file this module does not decode (the entry runs in the shell)."""


def describe(key, cmd, h, file_bytes, ident=None):
    """The Coded of a recognised command on a file with header ``h``; ``NotNative`` (naming the key) for a file that is left to
    sph2pipe: shorten-compressed, more than two channels, PCM that is not 16-bit, G.711 without ``-p``."""
    if h.shorten:
        raise NotNative("%s: %r is shorten-compressed: not native" % (key, cmd.path))
    if h.channels not in (1, 2):
        raise NotNative("%s: channel_count %d of %r: not native" % (key, h.channels, cmd.path))
    if h.coding == "pcm":
        if h.n_bytes != 2 or h.byte_format not in ("01", "10"):
            raise NotNative("%s: %d-byte PCM (sample_byte_format %s) of %r: not native" % (key, h.n_bytes, h.byte_format, cmd.path))
        coding = PCM16_LE if h.byte_format == "01" else PCM16_BE
    else:
        if h.n_bytes != 1:
            raise NotNative("%s: %d-byte %s samples of %r: not native" % (key, h.n_bytes, h.coding, cmd.path))
        if not cmd.pcm:                                 # without -p sph2pipe leaves the G.711 codes as they are
            raise NotNative("%s: %s without -p: not native" % (key, h.coding))
        coding = ULAW if h.coding == "ulaw" else ALAW
    if cmd.channel is not None and cmd.channel >= h.channels:
        raise mfcc.WavError("%s: -c %d of a file with %d channel(s): %r" % (key, cmd.channel + 1, h.channels, cmd.path))
    c = Coded()
    c.path, c.ident, c.data_off, c.rate, c.channels = cmd.path, ident or (0, cmd.path), h.size, h.rate, h.channels
    c.width = h.n_bytes
    c.stride = h.n_bytes * h.channels
    c.coding, c.channel = coding, cmd.channel
    c.n = sample_count(h, file_bytes, key, ident)
    return c


def recognise(key, rx):
    """A wav.scp entry -> Coded when it is a recognised sph2pipe command on a file this module decodes, else None (the shell runs
    it as before).  Only the header is read.  A recognised command whose file cannot be read, is no SPHERE file or lacks the
    channel asked for is an error (``mfcc.WavError`` naming the key), as the failing command would be."""
    if not rx.rstrip().endswith("|") or "sph2pipe" not in rx or not native_enabled():
        return None
    cmd = parse_command(rx)
    if cmd is None:
        return None
    h, file_bytes, ident = read_header(cmd.path, key)
    try:
        return describe(key, cmd, h, file_bytes, ident)
    except NotNative as e:
        logger.info("%s; running the command", e)
        return None


def decode_bytes(raw, coding, channels):
    """A data region (uint8 array) -> int16 [channels, samples]."""
    if coding in (ULAW, ALAW):
        x = (ULAW_TABLE if coding == ULAW else ALAW_TABLE)[raw]
    else:
        x = raw[:len(raw) // 2 * 2].view("<i2" if coding == PCM16_LE else ">i2").astype(np.int16)
    n = len(x) // channels
    return np.ascontiguousarray(x[:n * channels].reshape(n, channels).T)


def decode_host(coded):
    """-> int16 [channels, samples]: every channel of the file, or the one the command's ``-c`` chose."""
    x = decode_bytes(coded.region(), coded.coding, coded.channels)
    return x if coded.channel is None else x[coded.channel:coded.channel + 1]


# ------------------------------------------------------------------------------------------------
# the layout of a device decode
# ------------------------------------------------------------------------------------------------
def tile_list(ns, out_offsets):
    """[n_tiles, 2] int64 = (utterance, o0) of xv_wave_decode: utterance u takes ceil((ns[u] + h) / DEC_TILE) tiles, h =
    out_offsets[u] mod 8 (tiles are cut at 16-byte boundaries of the output buffer)."""
    ns = np.asarray(ns, np.int64)
    h = np.asarray(out_offsets, np.int64) & 7
    nt = np.where(ns > 0, (ns + h + DEC_TILE - 1) // DEC_TILE, 0)
    u = np.repeat(np.arange(len(ns), dtype=np.int64), nt)
    start = np.zeros(len(ns), np.int64)
    np.cumsum(nt[:-1], out=start[1:])
    o0 = (np.arange(int(nt.sum()), dtype=np.int64) - np.repeat(start, nt)) * DEC_TILE
    return np.stack([u, o0], axis=1) if len(u) else np.zeros((0, 2), np.int64)


def pack(items, out_offsets):
    """The side buffer and descriptors of the coded utterances of a window.  ``items``: (Coded, channel) pairs; ``out_offsets``:
    the element each one's samples start at in the sample buffer.  -> (raw uint8 array holding each distinct file's data region
    once, every start a multiple of 16; utt int64 [U, DEC_FIELDS]; tiles)."""
    starts, total = {}, 0
    for c, _ in items:
        if c.ident + (c.data_off,) not in starts:
            starts[c.ident + (c.data_off,)] = (total, c)
            total += (c.region_bytes + 15) // 16 * 16
    raw = np.zeros(max(total, 16), np.uint8)
    for a, c in starts.values():
        if c.region_bytes:
            c.read_into(raw[a:a + c.region_bytes])
    utt = np.zeros((len(items), DEC_FIELDS), np.int64)
    for u, ((c, ch), off) in enumerate(zip(items, out_offsets)):
        utt[u, :6] = (starts[c.ident + (c.data_off,)][0], c.n, c.stride, ch * c.width, c.coding, int(off))
    return raw, utt, tile_list(utt[:, N_], utt[:, OUT_OFF])
