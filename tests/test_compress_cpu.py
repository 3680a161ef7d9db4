"""Compressed feature output without a GPU: the format and the decode-error bounds of the encoding as
tests/cm_ref.py restates it, through both readers; the record writer through a TableWriter; the CLI's --compress flags; the
derived byte counts."""
import io
import os

import numpy as np
import pytest

import cm_ref
import kaldi_io

SHAPES = [(T, C) for T in (1, 2, 8, 9, 10, 11, 12, 13, 63, 64, 65, 257, 1000, 4099) for C in (1, 23, 24)]
# the bounds assume a normal grange (cm_ref.bounds); the subnormal case is held to byte equality on the GPU instead
BOUNDED = ("gauss", "ints", "const", "const_col", "outlier_col", "pm_zero", "pm_zero_nonneg")


@pytest.fixture(scope="module")
def records():
    """[(key, matrix, token, payload)] over the shapes and contents, and the ark that holds them."""
    rng = np.random.default_rng(5)
    out, bio = [], io.BytesIO()
    for T, C in SHAPES:
        cs = cm_ref.cases(rng, T, C)
        cs["tiny_behind_large"] = (rng.standard_normal((T, C)) * 1e-3).astype(np.float32)
        cs["tiny_behind_large"][T // 2, C // 2] = np.float32(5e4)
        for name in BOUNDED + ("tiny_behind_large",):
            key = "%s-%dx%d" % (name, T, C)
            token, payload = cm_ref.encode(cs[name])
            kaldi_io.write_cm_payload(bio, np.frombuffer(payload, np.uint8), T, key=key)
            out.append((key, cs[name], token, payload))
    return out, bio.getvalue()


def _in_place(raw):
    got = {}
    for keys, addr, rows, cols, holder in kaldi_io.scan_mat_ark_windows(io.BytesIO(raw), lambda: kaldi_io.ArkArena(1 << 20), None,
                                                                       lambda a: None):
        am = kaldi_io.ArkMats()
        am.add(addr, rows, cols, holder)
        for j, k in enumerate(keys):
            got[k] = np.array(am[j])
    return got


def _hold(decoded, recs):
    worst = 0.0
    for key, m, token, payload in recs:
        d = decoded[key]
        assert d.shape == m.shape and d.dtype == np.float32, key
        err = np.abs(d.astype(np.float64) - m.astype(np.float64))
        bound = cm_ref.bounds(m, payload, token)
        assert np.all(err <= bound), (key, float((err / bound).max()))
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    print("worst error / bound: %.4f" % worst)


def test_python_reader_decodes_within_the_bounds(records):
    recs, raw = records
    decoded = dict(kaldi_io.read_mat_ark(io.BytesIO(raw)))
    assert list(decoded) == [r[0] for r in recs]
    _hold(decoded, recs)


def test_in_place_reader_decodes_within_the_bounds(records):
    recs, raw = records
    assert kaldi_io._host_lib() is not None and hasattr(kaldi_io._host_lib(), "xv_ark_decode_cm")
    decoded = _in_place(raw)
    assert list(decoded) == [r[0] for r in recs]
    _hold(decoded, recs)


def test_payload_bytes_and_tokens():
    from xvector_amd import compress, hiplib
    lib = hiplib.load()
    for rows, cols, want in ((0, 23, 0), (1, 1, 18), (1, 23, 16 + 46), (8, 23, 16 + 2 * 8 * 23), (9, 23, 16 + 8 * 23 + 9 * 23),
                             (9, 1, 16 + 8 + 9), (4099, 128, 16 + 8 * 128 + 4099 * 128), (360000, 23, 16 + 184 + 360000 * 23),
                             (16777215, 128, 16 + 1024 + 16777215 * 128)):
        assert compress.payload_bytes(rows, cols) == cm_ref.payload_bytes(rows, cols) == lib.xv_cm_payload_bytes(rows, cols) == want
    rng = np.random.default_rng(1)
    for T in range(1, 12):
        token, payload = cm_ref.encode(rng.standard_normal((T, 5)).astype(np.float32))
        assert token == (b"CM2 " if T <= 8 else b"CM ") and len(payload) == cm_ref.payload_bytes(T, 5)
    offsets, sizes, total = compress.plan([0, 1, 9, 0, 100], 23)
    assert sizes.tolist() == [0, 62, 16 + 184 + 207, 0, 16 + 184 + 2300]
    assert all(o % 16 == 0 for o in offsets) and offsets.tolist() == [0, 0, 64, 64 + 416, 64 + 416] and total == 64 + 416 + 2512


def test_percentiles_strictly_increase_on_constant_columns():
    rng = np.random.default_rng(2)
    for m in (np.full((40, 3), np.float32(2.5)), np.zeros((9, 2), np.float32), cm_ref.cases(rng, 100, 7)["const_col"],
              np.full((12, 1), np.float32(-1e30))):
        gmin, grange = cm_ref.global_range(m)
        pct = cm_ref.percentiles(m, gmin, grange)
        assert np.all(np.diff(pct, axis=1) > 0) and pct.min() >= 0 and pct.max() <= 65535
        token, payload = cm_ref.encode(m)
        (_, d), = kaldi_io.read_mat_ark(io.BytesIO(b"k \0B" + token + payload))
        assert np.all(np.abs(d.astype(np.float64) - m) <= cm_ref.bounds(m, payload, token))
    # a maximum column: the clamps at 65532 .. 65535 from above
    m = np.zeros((20, 2), np.float32)
    m[:, 1] = 1.0
    gmin, grange = cm_ref.global_range(m)
    assert cm_ref.percentiles(m, gmin, grange).tolist() == [[0, 1, 2, 3], [65532, 65533, 65534, 65535]]


def test_write_cm_payload_through_a_table_writer(tmp_path):
    rng = np.random.default_rng(3)
    mats = [("long-key-%d" % i, (rng.standard_normal((T, 23)) * 2).astype(np.float32)) for i, T in enumerate((30, 1, 9, 8, 0, 200))]
    ark, scp = str(tmp_path / "t.ark"), str(tmp_path / "t.scp")
    plain_ark, plain_scp = str(tmp_path / "p.ark"), str(tmp_path / "p.scp")
    with kaldi_io.TableWriter(ark, scp) as w, kaldi_io.TableWriter(plain_ark, plain_scp) as pw:
        for k, m in mats:
            kaldi_io.write_mat(pw, m, key=k)
            if m.shape[0] == 0:
                kaldi_io.write_mat(w, m, key=k)                 # a matrix without rows stays plain
            else:
                kaldi_io.write_cm_payload(w, np.frombuffer(cm_ref.encode(m)[1], np.uint8), m.shape[0], key=k)
    with pytest.raises(kaldi_io.BadInputFormat):
        kaldi_io.write_cm_payload(io.BytesIO(), b"", 0, key="k")
    by_scp = list(kaldi_io.read_mat_scp(scp))
    by_ark = list(kaldi_io.read_mat_ark(ark))
    assert [k for k, _ in by_scp] == [k for k, _ in mats] == [k for k, _ in by_ark]
    for (k, m), (_, a), (_, b) in zip(mats, by_scp, by_ark):
        assert a.shape == m.shape and np.array_equal(a, b)
        if m.shape[0]:
            token, payload = cm_ref.encode(m)
            assert np.all(np.abs(a.astype(np.float64) - m) <= cm_ref.bounds(m, payload, token))
    # the scp offset points just past "key ", as write_mat's does
    raw = open(ark, "rb").read()
    for line, (k, m) in zip(open(scp), mats):
        off = int(line.split(":")[-1])
        assert raw[off - len(k) - 1:off] == (k + " ").encode() and raw[off:off + 2] == b"\0B"
        token = b"FM " if m.shape[0] == 0 else b"CM2 " if m.shape[0] <= 8 else b"CM "
        assert raw[off + 2:off + 2 + len(token)] == token
    # the plain ark is larger by exactly the derived byte counts: "FM " + 10 bytes of dimensions + 4 per element against the
    # token + the payload
    want = sum((13 + 4 * m.size) - ((4 if m.shape[0] <= 8 else 3) + cm_ref.payload_bytes(*m.shape)) for _, m in mats if m.shape[0])
    assert os.path.getsize(plain_ark) - os.path.getsize(ark) == want


def test_compress_flag_parses_in_all_three_subcommands():
    import mfcc_vad
    for cmd, tail in (("compute-mfcc-feats", ["scp:w", "ark:o"]), ("compute-mfcc-vad", ["scp:w", "ark:o", "ark:v"]),
                      ("copy-feats", ["ark:i", "ark:o"])):
        for flag, want in (([], False), (["--compress"], True), (["--compress=true"], True), (["--compress=false"], False)):
            args = mfcc_vad.parse_args([cmd] + flag + tail)
            assert mfcc_vad._want_compress(args) is want, (cmd, flag)
            assert (args.feats_wspecifier if cmd != "copy-feats" else args.feats_rspecifier) in ("ark:o", "ark:i")
        with pytest.raises(ValueError):
            mfcc_vad._want_compress(mfcc_vad.parse_args([cmd, "--compress=maybe"] + tail))
