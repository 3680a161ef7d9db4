"""Feature matrices as Kaldi CompressedMatrix records, encoded on the MI355X (csrc/xv_compress.hip).

What ``copy-feats --compress=true`` and ``compute-mfcc-feats --compress=true`` do on the host: a matrix of more than 8 rows
becomes a ``CM `` record (four uint16 percentiles per column, one byte per element), a shorter one a ``CM2 `` record (one uint16
per element).  The features are on the device when the MFCC kernel finishes, so they are encoded there and one byte per element
instead of four comes back over the bus.

* ``payload_bytes(rows, cols)`` -- the bytes that follow the token in a record (0 for an empty matrix: it stays an ``FM `` record).
* ``plan(T, cols)`` -- the offsets of the payloads in one output buffer, each a multiple of 16.
* ``encode(dev_feats, row0, T, cols)`` -- the payloads of ragged utterances that lie in a device matrix, as ``Packed`` records.
* ``encode_host(mats)`` -- the same for matrices in host memory, in windows of rows (copy-feats).

There is no CPU path: the arithmetic runs on the GPU, and a missing device is an error.
"""
import numpy as np

from . import hiplib

ALIGN = 16
MAX_COLS = 128
WINDOW_ROWS = 1 << 20             # rows uploaded per launch by encode_host


class CompressError(ValueError):
    pass


class Packed(object):
    """One matrix as a CompressedMatrix payload: ``rows``, ``cols`` and ``payload`` (a uint8 view into the block its launch
    brought back; what ``kaldi_io.write_cm_payload`` writes behind the token)."""
    __slots__ = ("rows", "cols", "payload")

    def __init__(self, rows, cols, payload):
        self.rows, self.cols, self.payload = int(rows), int(cols), payload

    @property
    def shape(self):
        return (self.rows, self.cols)


def payload_bytes(rows, cols):
    """16 + (rows > 8 ? 8 cols + rows cols : 2 rows cols); 0 for rows == 0 (xv_cm_payload_bytes, in Python: no library needed)."""
    rows, cols = int(rows), int(cols)
    if rows <= 0:
        return 0
    return 16 + (8 * cols + rows * cols if rows > 8 else 2 * rows * cols)


def plan(T, cols):
    """-> (offsets int64 [n], sizes int64 [n], total): utterance u's payload is ``sizes[u]`` bytes at ``offsets[u]`` of a buffer
    of ``total`` bytes; every offset is a multiple of 16."""
    T = np.asarray(T, np.int64).reshape(-1)
    sizes = np.where(T > 8, 16 + 8 * cols + T * cols, np.where(T > 0, 16 + 2 * T * cols, 0)).astype(np.int64)
    padded = (sizes + ALIGN - 1) // ALIGN * ALIGN
    offsets = np.zeros(len(T), np.int64)
    np.cumsum(padded[:-1], out=offsets[1:])
    return offsets, sizes, int(padded.sum())


def encode(dev_feats, row0, T, cols, stream=None, keys=None, d_row0=None, d_T=None):
    """dev_feats: float32 device rows [R, ld]; utterance u is rows row0[u] .. + T[u] (host arrays), columns 0 .. cols - 1.
    Runs the encoder on ``stream`` (a torch stream; None: the current one), brings the packed block back and returns
    ``(block, records)``: the host uint8 block and per utterance ``(offset, size, rows)``.  An utterance holding a NaN or an
    infinity raises ``CompressError`` naming it (``keys[u]`` when given).  ``d_row0`` / ``d_T``: the int64 / int32 device copies of
    row0 and T where the caller has them already."""
    import torch
    hiplib.require_gpu()
    T = np.asarray(T, np.int64).reshape(-1)
    row0 = np.asarray(row0, np.int64).reshape(-1)
    n = len(T)
    if not 1 <= cols <= MAX_COLS:
        raise CompressError("compressed output supports 1 .. %d columns, got %d" % (MAX_COLS, cols))
    if n and int(T.max()) * cols >= 1 << 31:
        raise CompressError("matrix too large to compress: rows * cols must be below 2^31")
    offsets, sizes, total = plan(T, cols)
    records = list(zip(offsets.tolist(), sizes.tolist(), T.tolist()))
    if total == 0:
        return np.zeros(0, np.uint8), records
    device = dev_feats.device
    with torch.cuda.device(device), torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(device)):
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
        d_row0 = up(row0) if d_row0 is None else d_row0
        d_T = up(T.astype(np.int32)) if d_T is None else d_T
        out = torch.empty(total, dtype=torch.uint8, device=device)
        status = torch.empty(n, dtype=torch.int32, device=device)
        hiplib.cm_encode(dev_feats, d_row0, d_T, cols, up(offsets), out, status)
        status_h = status.cpu().numpy()
        block = out.cpu().numpy()
    bad = np.flatnonzero(status_h)
    if len(bad):
        u = int(bad[0])
        name = keys[u] if keys is not None else "#%d" % u
        raise CompressError("Cannot compress the matrix of %s: %s" % (
            name, "it holds infinities or NaNs" if status_h[u] == 1 else "rows * cols must be below 2^31"))
    return block, records


def packed(block, records, cols):
    """The ``Packed`` records of an ``encode`` result."""
    return [Packed(rows, cols, block[off:off + size]) for off, size, rows in records]


def encode_host(mats, keys=None, device="cuda:0", window_rows=WINDOW_ROWS):
    """Matrices in host memory (any float dtype; converted to float32) -> a ``Packed`` each.  A launch takes a run of matrices
    of one width, at most ``window_rows`` rows of them.  A matrix without rows gives None (it stays a plain record)."""
    import torch
    hiplib.require_gpu()
    device = torch.device(device)
    out = [None] * len(mats)
    i = 0
    while i < len(mats):
        cols = mats[i].shape[1] if mats[i].ndim == 2 else 0
        j, rows = i, 0
        while j < len(mats) and (j == i or (rows + mats[j].shape[0] <= window_rows and mats[j].shape[1] == cols)):
            rows += mats[j].shape[0]
            j += 1
        T = np.array([m.shape[0] for m in mats[i:j]], np.int64)
        if rows:
            row0 = np.zeros(j - i, np.int64)
            np.cumsum(T[:-1], out=row0[1:])
            flat = np.concatenate([np.asarray(m, np.float32).reshape(-1, cols) for m in mats[i:j]])
            block, records = encode(torch.from_numpy(flat).to(device), row0, T, cols, keys=None if keys is None else keys[i:j])
            for k, p in enumerate(packed(block, records, cols)):
                if p.rows:
                    out[i + k] = p
        i = j
    return out
