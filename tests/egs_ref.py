"""NumPy oracle of the egs kernels (xv_vad_compact_i32, xv_egs_chunks_f16) and a NumPy stand-in for the gather step of
xvector_amd.egs.EgsWriter, so its host logic runs on the CPU.  Restates the published rule of Kaldi's SlidingWindowCmn (the comment
at the head of csrc/xv_frontend.hip); every window sum is taken afresh in float64 (no sliding), so it shares no summation order with
the kernel."""
import os

import numpy as np


def window_bounds(t, T, window, center, min_window):
    if center:
        ws = t - window // 2
        we = ws + window
    else:
        ws, we = t - window, t + 1
    if ws < 0:
        we -= ws
        ws = 0
    if not center and we > t:
        we = max(t + 1, min_window)
    if we > T:
        ws -= we - T
        we = T
        ws = max(ws, 0)
    return ws, we


def cmn_f64(x, window=300, center=True, min_window=100):
    """float64 [T, F]: x[t] - mean of the window around RAW frame t, every operation in float64."""
    x64 = np.asarray(x, np.float64)
    T = x64.shape[0]
    out = np.empty_like(x64)
    for t in range(T):
        ws, we = window_bounds(t, T, window, center, min_window)
        out[t] = x64[t] - x64[ws:we].sum(axis=0) / float(we - ws)
    return out


def voiced_rows(vad):
    return np.flatnonzero(np.asarray(vad) != 0)


def no_sil_f16(x, vad, window=300, center=True, min_window=100):
    """What the kernel serves for voiced frame j of the utterance: float16(float32(cmn_f64))[voiced], and the float64 values."""
    v = cmn_f64(x, window, center, min_window)[voiced_rows(vad)]
    return v.astype(np.float32).astype(np.float16), v


def half_ulp16(v):
    """Half the spacing of float16 at |v| (the spacing of the binade |v| lies in; subnormal spacing 2^-24 below 2^-14)."""
    a = np.abs(np.asarray(v, np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return 0.5 * 2.0 ** (e - 10)


class NumpyGather(object):
    """The three calls of xvector_amd.egs.DeviceGather in NumPy (alloc / gather / fetch), the table checked as the wrapper does."""

    def __init__(self, cmn_window=300, center=True, min_window=100):
        self.cmn_window, self.center, self.min_window = cmn_window, center, min_window
        self.calls = 0

    def alloc(self, n):
        return np.zeros(int(n), np.float16)

    def __call__(self, y, feats, vad, utt_start, utt_len, table):
        from xvector_amd import hiplib
        self.calls += 1
        tabs = [no_sil_f16(feats[s:s + n], vad[s:s + n], self.cmn_window, self.center, self.min_window)[0]
                for s, n in zip(np.asarray(utt_start).tolist(), np.asarray(utt_len).tolist())]
        counts = np.array([t.shape[0] for t in tabs], np.int32)
        F = feats.shape[1]
        cu, cf, cl, cd = hiplib.check_chunk_table(table, counts, F, y.size)
        for u, first, n, dst in zip(cu.tolist(), cf.tolist(), cl.tolist(), cd.tolist()):
            y[dst:dst + n * F] = tabs[u][first:first + n].reshape(-1)
        return counts

    def fetch(self, y):
        return y


# ------------------------------------------------------------------------------------------------
# fixtures shared by tests/test_egs_cpu.py and tests/test_gpu_egs.py
# ------------------------------------------------------------------------------------------------
def make_data_dir(path, n_spk, n_utt, t_lo, t_hi, F, seed, voiced_p=0.7):
    """A raw Kaldi data directory (feats.ark/scp, vad.ark/scp, utt2spk, spk2utt) of random utterances -> {utt: (mat, vad)}."""
    import kaldi_io
    rng = np.random.default_rng(seed)
    os.makedirs(path, exist_ok=True)
    utts = {}
    with kaldi_io.TableWriter(os.path.join(path, "feats.ark"), os.path.join(path, "feats.scp")) as tf, \
            kaldi_io.TableWriter(os.path.join(path, "vad.ark"), os.path.join(path, "vad.scp")) as tv:
        for s in range(n_spk):
            for j in range(n_utt):
                key = "spk%d-utt%d" % (s, j)
                T = int(rng.integers(t_lo, t_hi + 1))
                mat = (rng.standard_normal((T, F)) * 3 + 5 * rng.standard_normal(F)).astype(np.float32)
                vad = (rng.random(T) < voiced_p).astype(np.float32)
                kaldi_io.write_mat(tf, mat, key=key)
                kaldi_io.write_vec_flt(tv, vad, key=key)
                utts[key] = (mat, vad)
    with open(os.path.join(path, "utt2spk"), "wt") as f:
        f.write("".join("%s spk%d\n" % (k, int(k[3:k.index("-")])) for k in utts))
    with open(os.path.join(path, "spk2utt"), "wt") as f:
        for s in range(n_spk):
            f.write("spk%d %s\n" % (s, " ".join(k for k in utts if k.startswith("spk%d-" % s))))
    return utts


def write_table(path, mats):
    """mats: {utt: float32 [T, F]} -> <path>.ark / <path>.scp in dict order; returns the scp."""
    import kaldi_io
    with kaldi_io.TableWriter(path + ".ark", path + ".scp") as tw:
        for k, m in mats.items():
            kaldi_io.write_mat(tw, np.ascontiguousarray(m, np.float32), key=k)
    return path + ".scp"


def served_by_ranges_loader(ranges_file, scp, count, B, F):
    """(minibatches float32 [B, T, F], labels) in minibatch order 0 .. count-1, as examples_io.RangesDataLoader(shuffle=False)
    serves them (it pops the last first)."""
    import examples_io
    named = set(line.split()[0] for line in open(ranges_file) if line.strip())
    sub = "%s.%s" % (scp, os.path.basename(ranges_file))       # the loader takes an scp without a ranges entry for an error
    with open(sub, "wt") as f:
        f.write("".join(line for line in open(scp) if line.split()[0] in named))
    loader = examples_io.RangesDataLoader(ranges_file, sub, count, B, F, shuffle=False)
    got = [loader.pop() for _ in range(count)][::-1]
    assert loader.pop() == (None, None)
    return [d for d, _ in got], np.stack([l for _, l in got])


def read_tar(tar_path):
    """Members of an egs tar in member-name order minibatch_0 .. + the label file."""
    import io
    import tarfile
    with tarfile.open(tar_path, "r") as tar:
        names = tar.getnames()
        assert names == ["minibatch_%d.npy" % i for i in range(len(names))]
        members = [np.load(io.BytesIO(tar.extractfile(n).read())) for n in names]
    return members, np.load(tar_path[:-4] + ".npy")
