"""Reference side of the SPHERE tests (tests/test_sphere_cpu.py, tests/test_gpu_sphere.py): a writer of NIST SPHERE files, the
G.711 expansions as scalar formulas with no table, Python's ``audioop`` as the independent implementation where it imports,
and a linear -> mu-law encoder (by search over the 256 codes) for making speech-like coded files."""
import numpy as np

try:
    import audioop
except ImportError:                  # removed from the standard library in Python 3.13
    audioop = None

PCM16_LE, PCM16_BE, ULAW, ALAW = range(4)


def ulaw_formula(b):
    u = ~b & 0xFF
    t = (((u & 15) << 3) + 132) << ((u >> 4) & 7)
    return 132 - t if u & 128 else t - 132


def alaw_formula(b):
    a = (b ^ 0x55) & 0xFF
    t = (a & 15) << 4
    s = (a >> 4) & 7
    t += 0x108 if s else 8
    if s > 1:
        t <<= s - 1
    return t if a & 128 else -t


def formula_table(coding):
    f = ulaw_formula if coding in (ULAW, "ulaw") else alaw_formula
    return np.array([f(b) for b in range(256)], np.int64)


def audioop_table(coding):
    codes = bytes(range(256))
    lin = audioop.ulaw2lin(codes, 2) if coding in (ULAW, "ulaw") else audioop.alaw2lin(codes, 2)
    return np.frombuffer(lin, "<i2").astype(np.int64)


def decode(raw, coding, stride, ch_off, n, raw_off=0):
    """Samples 0 .. n - 1 of one channel of a raw data region (uint8 array), by the formulas: -> int16 [n]."""
    raw = np.asarray(raw, np.uint8)
    pos = raw_off + ch_off + stride * np.arange(n, dtype=np.int64)
    if coding in (ULAW, ALAW):
        return formula_table(coding)[raw[pos]].astype(np.int16)
    b0, b1 = raw[pos].astype(np.int64), raw[pos + 1].astype(np.int64)
    v = (b0 | (b1 << 8)) if coding == PCM16_LE else ((b0 << 8) | b1)
    return np.where(v >= 32768, v - 65536, v).astype(np.int16)


def lin2ulaw(x):
    """int16 samples -> the mu-law codes whose expansion is nearest (a search over the table: slow, exact, table-free)."""
    tab = formula_table(ULAW)
    order = np.argsort(tab, kind="stable")
    vals = tab[order]
    x = np.asarray(x, np.int64)
    i = np.clip(np.searchsorted(vals, x), 1, 255)
    pick = np.where(np.abs(vals[i - 1] - x) <= np.abs(vals[i] - x), i - 1, i)
    return order[pick].astype(np.uint8)


def sph_bytes(x, rate, coding="pcm", byte_format="01", header=1024, fields=None, shuffle=None, sample_count=True, coding_name=None):
    """A NIST SPHERE file.  ``x``: [channels, samples] (or [samples]) of what the file stores -- int16 samples for ``pcm``, uint8
    codes for ``ulaw`` / ``alaw``.  ``byte_format``: '01' little-endian, '10' big-endian (16-bit PCM).  ``header``: its size in
    bytes.  ``fields``: {name: value or None} overriding (None: dropping) header fields; ``coding_name``: the ``sample_coding``
    text (None: ``coding``; '' drops the field); ``sample_count``: False drops the field, an int overrides it; ``shuffle``: a seed
    for the order of the fields."""
    x = np.asarray(x)
    if x.ndim == 1:
        x = x[None]
    nch, n = x.shape
    if coding == "pcm":
        payload = np.ascontiguousarray(x.T).astype("<i2" if byte_format == "01" else ">i2").tobytes()
        nbytes, bf = 2, byte_format
    else:
        payload = np.ascontiguousarray(x.T).astype(np.uint8).tobytes()
        nbytes, bf = 1, "1"
    f = [("sample_rate", "-i", str(int(rate))), ("channel_count", "-i", str(nch)), ("sample_n_bytes", "-i", str(nbytes)),
         ("sample_byte_format", "-s%d" % len(bf), bf), ("sample_sig_bits", "-i", str(8 * nbytes)),
         ("database_id", "-s7", "testing"), ("speaking_mode", "-s11", "spontaneous")]
    name = coding if coding_name is None else coding_name
    if name:
        f.append(("sample_coding", "-s%d" % len(name), name))
    if sample_count is not False:
        f.append(("sample_count", "-i", str(n if sample_count is True else int(sample_count))))
    for k, v in (fields or {}).items():
        f = [e for e in f if e[0] != k]
        if v is not None:
            f.append((k, "-i" if isinstance(v, int) else "-s%d" % len(str(v)), str(v)))
    if shuffle is not None:
        f = [f[i] for i in np.random.default_rng(shuffle).permutation(len(f))]
    text = "NIST_1A\n%7d\n" % header + "".join("%s %s %s\n" % e for e in f) + "end_head\n"
    assert len(text) <= header
    return text.encode() + b" " * (header - len(text)) + payload
