"""The CompressedMatrix encoder on the GPU (csrc/xv_compress.hip): payload bytes equal to the NumPy restatement
(tests/cm_ref.py) byte for byte, nothing written outside a payload, an utterance's bytes independent of its batch, a NaN or an
infinity refused per utterance, and the stage-1 CLI with --compress end to end."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import cm_ref

pytestmark = pytest.mark.gpu

STAGE_MAX = 8192              # CM_STAGE_MAX: a column of more rows is re-read from global memory in every radix pass
LENGTHS = (1, 2, 4, 5, 8, 9, 10, 11, 12, 13, 63, 64, 65, 255, 256, 257, 1000, 4099, STAGE_MAX + 809)
FILL = 0xA5


@pytest.fixture(scope="module")
def env():
    import torch
    from xvector_amd import compress, hiplib, mfcc, synthetic
    hiplib.require_gpu()
    return dict(torch=torch, compress=compress, hiplib=hiplib, mfcc=mfcc, synthetic=synthetic)


def _batch(C, seed):
    """The matrices of one launch of width C: every length, the kind of content rotating with it so that every kind meets short,
    medium and long columns over the five widths; every kind at lengths around the CM2 / CM switch and one tile."""
    rng = np.random.default_rng(seed)
    mats = []
    for i, T in enumerate(LENGTHS):
        cs = cm_ref.cases(rng, T, C)
        names = sorted(cs)
        picks = names if T in (8, 9, 257) else [names[(i + C) % len(names)], names[(i + C + 3) % len(names)]]
        mats += [("%s-%d" % (n, T), cs[n]) for n in picks]
    mats.insert(3, ("empty", np.zeros((0, C), np.float32)))
    return mats


def _launch(env, mats, C, pad_cols=3, gap=48, lead_rows=2):
    """One xv_cm_encode_f32 launch over ``mats`` laid out ragged in a wider device matrix (ld = C + pad_cols, NaN in the columns
    and rows no utterance owns), the payloads ``gap`` bytes apart in a buffer filled with FILL.  Returns (payloads, status):
    asserts that no byte outside the payloads changed."""
    torch, compress, hiplib = env["torch"], env["compress"], env["hiplib"]
    T = np.array([m.shape[0] for _, m in mats], np.int64)
    row0 = lead_rows + np.concatenate([[0], np.cumsum(T[:-1] + 1)]).astype(np.int64)        # one foreign row between utterances
    rows = int(row0[-1] + T[-1]) + 1
    host = np.full((rows, C + pad_cols), np.nan, np.float32)
    for (_, m), r in zip(mats, row0):
        host[r:r + m.shape[0], :C] = m
    sizes = np.array([cm_ref.payload_bytes(t, C) for t in T], np.int64)
    offsets = np.zeros(len(T), np.int64)
    np.cumsum(((sizes + 15) // 16 * 16 + gap)[:-1], out=offsets[1:])
    offsets += 16
    total = int(offsets[-1] + sizes[-1]) + 64
    dev = torch.device("cuda:0")
    out = torch.full((total,), FILL, dtype=torch.uint8, device=dev)
    status = torch.full((len(T),), -1, dtype=torch.int32, device=dev)
    hiplib.cm_encode(torch.from_numpy(host).to(dev), torch.from_numpy(row0).to(dev), torch.from_numpy(T.astype(np.int32)).to(dev), C,
                     torch.from_numpy(offsets).to(dev), out, status)
    got = out.cpu().numpy()
    untouched = np.ones(total, bool)
    for o, s in zip(offsets, sizes):
        untouched[o:o + s] = False
    assert np.all(got[untouched] == FILL), "bytes outside the payloads were written"
    return [got[o:o + s].tobytes() for o, s in zip(offsets, sizes)], status.cpu().numpy()


def _diff(name, got, want):
    if got == want:
        return None
    g, w = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    at = np.flatnonzero(g != w)
    return "%s: %d of %d bytes differ, first at %d (%d != %d)" % (name, len(at), len(w), at[0], g[at[0]], w[at[0]])


@pytest.mark.parametrize("C", (1, 13, 23, 24, 40))
def test_payload_bytes_equal_the_reference(env, C):
    mats = _batch(C, 100 + C)
    payloads, status = _launch(env, mats, C)
    assert not status.any()
    bad = [d for d in (_diff(n, p, cm_ref.encode(m)[1] if m.shape[0] else b"") for (n, m), p in zip(mats, payloads)) if d]
    assert not bad, "\n".join(bad)


def test_an_utterance_alone_has_the_bytes_it_has_in_a_batch(env):
    C = 23
    mats = _batch(C, 7)
    batch, _ = _launch(env, mats, C)
    for i in (0, 5, len(mats) // 2, len(mats) - 1):                # short, the CM2 / CM switch, a medium one, the longest
        alone, status = _launch(env, [mats[i]], C, pad_cols=0 if i % 2 else 9, gap=0, lead_rows=i)
        assert status.tolist() == [0] and alone[0] == batch[i], mats[i][0]


def test_a_nan_or_an_infinity_sets_only_its_own_status(env):
    C = 13
    rng = np.random.default_rng(3)
    mats = [("u%d" % i, (rng.standard_normal((T, C)) * 3).astype(np.float32)) for i, T in enumerate((40, 300, 5, 7, 9000, 64, 12))]
    clean, status = _launch(env, mats, C)
    assert not status.any()
    hurt = [(n, m.copy()) for n, m in mats]
    hurt[1][1][299, 12] = np.nan
    hurt[3][1][0, 0] = np.inf
    hurt[4][1][8999, 5] = -np.inf
    got, status = _launch(env, hurt, C)
    assert status.tolist() == [0, 1, 0, 1, 1, 0, 0]
    assert all(got[i] == clean[i] for i in (0, 2, 5, 6))
    # the Python layer names the utterance
    compress, torch = env["compress"], env["torch"]
    flat = np.concatenate([m for _, m in hurt])
    T = np.array([m.shape[0] for _, m in hurt])
    row0 = np.concatenate([[0], np.cumsum(T[:-1])])
    with pytest.raises(compress.CompressError, match="u1"):
        compress.encode(torch.from_numpy(flat).cuda(), row0, T, C, keys=[n for n, _ in hurt])
    block, records = compress.encode(torch.from_numpy(np.concatenate([m for _, m in mats])).cuda(), row0, T, C)
    assert [block[o:o + s].tobytes() for o, s, _ in records] == clean and all(o % 16 == 0 for o, _, _ in records)


def test_refused_widths(env):
    torch, hiplib = env["torch"], env["hiplib"]
    dev = torch.device("cuda:0")
    x = torch.zeros((4, 129), dtype=torch.float32, device=dev)
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)  # noqa: E731
    with pytest.raises(hiplib.XvectorHipError, match="n_cols"):
        hiplib.cm_encode(x, i64([0]), torch.tensor([4], dtype=torch.int32, device=dev), 129, i64([0]),
                         torch.zeros(4096, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.int32, device=dev))


# ------------------------------------------------------------------------------------------------
# the CLI
# ------------------------------------------------------------------------------------------------
def _run(args):
    cli = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "x-vector-kaldi-tf_amd", "local", "tf", "mfcc_vad.py")
    return subprocess.run([sys.executable, cli] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)


def test_cli_compressed_tables_end_to_end(env, tmp_path):
    import kaldi_io
    mfcc, syn = env["mfcc"], env["synthetic"]
    here = os.path.dirname(os.path.abspath(__file__))
    conf, vconf = os.path.join(here, "golden", "mfcc.conf"), os.path.join(here, "golden", "vad.conf")
    d = tmp_path
    fs = 8000

    def wav(name, x):
        path = str(d / name)
        with open(path, "wb") as f:
            f.write(mfcc.wav_bytes(x, fs))
        return path
    rng = np.random.default_rng(9)
    rir = rng.standard_normal(800) * 4000.0 * np.exp(-np.arange(800) / 150.0)
    rir[40] = 30000.0
    rir_path = wav("rir.wav", np.clip(np.rint(rir), -32767, 32767).astype(np.int16))
    lines = []
    # --snip-edges=false: (n + 40) // 80 frames.  2 frames, 8 and 9 (the CM2 / CM switch), none at all, ordinary lengths, and one
    # reverberated entry
    for i, n in enumerate((150, 600, 680, 30, 8000 * 3, 8000 * 2 + 123, 8000 * 5)):
        lines.append("utt%d %s" % (i, wav("utt%d.wav" % i, syn.speech_like_wave(n, fs, 50 + i))))
    lines.append("utt7-reverb wav-reverberate --shift-output=true --impulse-response=%s %s - |" % (rir_path, str(d / "utt4.wav")))
    (d / "wav.scp").write_text("\n".join(lines) + "\n")

    def compute(tag, flags):
        p = _run(["compute-mfcc-vad", "--config=" + conf, "--vad-config=" + vconf, "--write-num-frames=ark,t:%s/nf_%s" % (d, tag)] + flags +
                 ["scp:%s/wav.scp" % d, "ark,scp:%s/f_%s.ark,%s/f_%s.scp" % (d, tag, d, tag), "ark,scp:%s/v_%s.ark,%s/v_%s.scp" % (d, tag, d, tag)])
        assert p.returncode == 0, p.stdout.decode()
    compute("plain", [])
    compute("cm", ["--compress=true"])
    read = lambda name: open(str(d / name), "rb").read()  # noqa: E731
    plain = list(kaldi_io.read_mat_scp(str(d / "f_plain.scp")))
    assert [k for k, _ in plain] == [ln.split()[0] for ln in lines]
    assert sorted({m.shape[0] for _, m in plain})[:4] == [0, 2, 8, 9]
    # the compressed table is the reference encoding of the plain run's matrices (the dither is keyed: the fp32 rows are the same)
    want = io.BytesIO()
    for k, m in plain:
        if m.shape[0]:
            want.write(cm_ref.record(k, m))
        else:
            kaldi_io.write_mat(want, m, key=k)
    assert read("f_cm.ark") == want.getvalue()
    assert len(read("f_cm.ark")) < 0.3 * len(read("f_plain.ark"))
    assert read("nf_cm") == read("nf_plain") and read("v_cm.ark") == read("v_plain.ark")
    assert read("v_cm.scp").replace(b"v_cm", b"v_plain") == read("v_plain.scp")
    # the scp offsets lead to the records; the extractor's reader (kaldi_io.MatScp, in-place windows included) decodes them
    decoded = dict(kaldi_io.read_mat_ark(io.BytesIO(want.getvalue())))
    by_scp = dict(kaldi_io.MatScp(str(d / "f_cm.scp")))
    assert list(by_scp) == list(decoded) and all(np.array_equal(by_scp[k], decoded[k]) for k in decoded)
    seen = {}
    for keys, addr, rows, cols, holder in kaldi_io.MatScp(str(d / "f_cm.scp")).windows(lambda: kaldi_io.ArkArena(1 << 20), None, lambda a: None):
        am = kaldi_io.ArkMats()
        am.add(addr, rows, cols, holder)
        seen.update((k, np.array(am[j])) for j, k in enumerate(keys))
    assert list(seen) == list(decoded) and all(np.array_equal(seen[k], decoded[k]) for k in decoded)
    for k, m in plain:
        if m.shape[0]:
            token, payload = cm_ref.encode(m)
            assert np.all(np.abs(decoded[k].astype(np.float64) - m) <= cm_ref.bounds(m, payload, token)), k
    # copy-feats: plain -> compressed gives the same bytes; compressed -> plain gives the decoded rows as FM records
    p = _run(["copy-feats", "--compress=true", "scp:%s/f_plain.scp" % d, "ark,scp:%s/c.ark,%s/c.scp" % (d, d)])
    assert p.returncode == 0, p.stdout.decode()
    assert read("c.ark") == read("f_cm.ark") and read("c.scp").replace(b"/c.ark", b"/f_cm.ark") == read("f_cm.scp")
    p = _run(["copy-feats", "ark:%s/f_cm.ark" % d, "ark:%s/back.ark" % d])
    assert p.returncode == 0, p.stdout.decode()
    back = io.BytesIO()
    for k, m in decoded.items():
        kaldi_io.write_mat(back, m, key=k)
    assert read("back.ark") == back.getvalue()
