"""bench.py --dump-outputs: the files it writes (names, dtypes, the 64 MB cap and its seeded row sample).  CPU only."""
import importlib.util
import os

import numpy as np

from conftest import ROOT


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_small_outputs_are_written_whole(tmp_path):
    bench = _bench()
    x = np.arange(12, dtype=np.float32).reshape(3, 4)
    bench._dump_outputs(str(tmp_path), {"xvectors": x, "losses": np.array([1.5, 0.5]), "weights/tdnn0/w:0": np.ones(3, np.float16)})
    assert sorted(os.listdir(str(tmp_path))) == ["losses.npy", "weights_tdnn0_w_0.npy", "xvectors.npy"]
    got = np.load(str(tmp_path / "xvectors.npy"))
    assert got.dtype == np.float32 and np.array_equal(got, x)
    assert np.load(str(tmp_path / "losses.npy")).dtype == np.float64
    w = np.load(str(tmp_path / "weights_tdnn0_w_0.npy"))
    assert w.dtype == np.float64 and np.array_equal(w, np.ones(3))


def test_large_outputs_are_cut_to_the_same_seeded_rows(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 4096)
    x = np.random.default_rng(5).standard_normal((100, 16)).astype(np.float32)          # 6400 bytes: over the cap
    bench._dump_outputs(str(tmp_path / "a"), {"xvectors": x})
    bench._dump_outputs(str(tmp_path / "b"), {"xvectors": x.copy()})
    a, b = np.load(str(tmp_path / "a" / "xvectors.npy")), np.load(str(tmp_path / "b" / "xvectors.npy"))
    assert a.nbytes <= 4096 and a.shape[1] == 16 and a.shape[0] > 0 and np.array_equal(a, b)
    rows = [int(np.flatnonzero((x == r).all(axis=1))[0]) for r in a]
    assert rows == sorted(rows) and len(set(rows)) == len(rows)
