"""The egs kernels on the MI355X (csrc/xv_egs.hip) against the NumPy oracle tests/egs_ref.py, and make_egs.py end to end.

Bounds.  xv_egs_chunks_f16 returns half_rne(float(d)) of a float64 d = x[t] - sum / n.  On integer-valued features with |x| <= 1024
every partial sum of at most 650 terms is an integer below 2^53, so sum is exact in any order and the output must EQUAL the oracle's
float16(float32(x[t] - s / n)).  On Gaussian features the float64 value v of the oracle and the kernel's d differ by the order of the
float64 additions only (~1e-15 relative); a correct result is v rounded to float32 once (half a float32 ulp, 2^-24 |v|) and then to
float16 (half a float16 ulp): asserted as |got - v| <= ulp16(v)/2 + 2 * 2^-24 |v|."""
import os

import numpy as np
import pytest

import egs_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    from xvector_amd import hiplib
    hiplib.require_gpu()
    return dict(torch=torch, hiplib=hiplib)


def _dev(torch, a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


# ---------------------------------------------------------------------------------------------------------------------------------
# xv_vad_compact_i32
# ---------------------------------------------------------------------------------------------------------------------------------
def _vad_cases():
    rng = np.random.default_rng(0)
    vads = []
    for T in (0, 1, 63, 64, 65, 257):
        vads += [np.ones(T, np.float32), np.zeros(T, np.float32), (np.arange(T) % 2).astype(np.float32)]
    lead = np.concatenate([np.zeros(200, np.float32), (rng.random(57) < 0.6).astype(np.float32)])
    odd = np.array([0.5, 0, -1, 0, 0, 0.5, -1, -1, 0], np.float32)          # 0.5 and -1 count as voiced
    return vads + [lead, odd, (rng.random(257) < 0.7).astype(np.float32)]


def test_vad_compact_equals_flatnonzero_and_repeats_bit_for_bit(env):
    torch, hiplib = env["torch"], env["hiplib"]
    vads = _vad_cases()
    lens = np.array([len(v) for v in vads], np.int32)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    assert (starts[1:] > 0).any()
    flat = _dev(torch, np.concatenate(vads), np.float32)
    us, ul = _dev(torch, starts, np.int32), _dev(torch, lens, np.int32)
    runs = []
    for _ in range(2):
        count, rows = hiplib.vad_compact(flat, us, ul)
        runs.append((count.cpu().numpy(), rows.cpu().numpy()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    count, rows = runs[0]
    for u, v in enumerate(vads):
        want = np.flatnonzero(v)
        assert count[u] == len(want), u
        assert np.array_equal(rows[starts[u]:starts[u] + len(want)], want), u
        assert (rows[starts[u] + len(want):starts[u] + len(v)] == -1).all()          # the rest of the span is left alone


# ---------------------------------------------------------------------------------------------------------------------------------
# xv_egs_chunks_f16
# ---------------------------------------------------------------------------------------------------------------------------------
T_LIST = (5, 8, 9, 37, 300, 301, 650)
LEN_LIST = (2, 63, 64, 65, 200)
SENTINEL = np.float16(-77.0)


def _problem(F, ldx, integer, seed):
    """Utterances of every T in T_LIST (+ one with a leading unvoiced run of 320 > window 300), a chunk table with every length of
    LEN_LIST that fits, chunks at voiced frame 0 and ending on the last voiced frame, two overlapping chunks of one utterance,
    destinations shuffled with gaps between them."""
    rng = np.random.default_rng(seed)
    mats, vads = [], []
    for T in T_LIST:
        if integer:
            m = rng.integers(-1024, 1025, size=(T, F)).astype(np.float32)
        else:
            m = (rng.standard_normal((T, F)) * 3 + 5 * rng.standard_normal(F)).astype(np.float32)
        v = (rng.random(T) < 0.7).astype(np.float32)
        v[rng.integers(0, T)] = 1.0
        mats.append(m)
        vads.append(v)
    T = 650
    m = rng.integers(-1024, 1025, size=(T, F)).astype(np.float32) if integer else (rng.standard_normal((T, F)) * 3 - 2).astype(np.float32)
    v = np.concatenate([np.zeros(320, np.float32), (rng.random(T - 320) < 0.8).astype(np.float32)])
    mats.append(m)
    vads.append(v)
    vads[4][:] = 1.0                                       # T = 300 all voiced: 200- and 65-frame chunks fit
    counts = [int(np.count_nonzero(v)) for v in vads]
    chunks = []
    for u, c in enumerate(counts):
        for n in LEN_LIST:
            if n <= c:
                chunks.append((u, 0, n))                   # from voiced frame 0
                chunks.append((u, c - n, n))               # ending on the last voiced frame
        if c >= 3:
            chunks.append((u, 1, 2))
            chunks.append((u, 0, 3))                       # overlaps the one before
    assert all(any(n == want for _, _, n in chunks) for want in LEN_LIST)
    order = rng.permutation(len(chunks))
    dst = np.zeros(len(chunks), np.int64)
    pos = 3
    for c in order:
        dst[c] = pos
        pos += chunks[c][2] * F + int(rng.integers(0, 4))  # odd gaps: rows start on odd half-words
    lens = np.array([m.shape[0] for m in mats], np.int32)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    x = np.zeros((int(lens.sum()), ldx), np.float32)
    x[:, F:] = 1e30                                        # the padding columns must never be read into a mean
    x[:, :F] = np.concatenate(mats)
    table = tuple(np.array(a) for a in zip(*chunks)) + (dst,)
    return dict(mats=mats, vads=vads, counts=counts, x=x, lens=lens, starts=starts, table=table, y_elems=pos + 5, F=F)


def _run(env, p, window, center, min_window=100):
    torch, hiplib = env["torch"], env["hiplib"]
    x = _dev(torch, p["x"], np.float32)[:, :p["F"]] if p["x"].shape[1] > p["F"] else _dev(torch, p["x"], np.float32)
    us, ul = _dev(torch, p["starts"], np.int32), _dev(torch, p["lens"], np.int32)
    count, rows = hiplib.vad_compact(_dev(torch, np.concatenate(p["vads"]), np.float32), us, ul)
    counts = count.cpu().numpy()
    assert counts.tolist() == p["counts"]
    y = torch.full((p["y_elems"],), float(SENTINEL), dtype=torch.float16, device="cuda")
    hiplib.egs_chunks(x, us, ul, count, rows, p["table"], counts, window, center, min_window, y)
    return y.cpu().numpy()


def _covered(p):
    mask = np.zeros(p["y_elems"], bool)
    for u, first, n, dst in zip(*p["table"]):
        mask[dst:dst + n * p["F"]] = True
    return mask


CONFIGS = [(23, 23, 300, True), (23, 24, 8, True), (1, 1, 8, False), (40, 40, 300, False), (23, 23, 8, False), (40, 40, 8, True)]


@pytest.mark.parametrize("F,ldx,window,center", CONFIGS)
def test_chunks_equal_the_oracle_bit_for_bit_on_integer_features(env, F, ldx, window, center):
    p = _problem(F, ldx, True, seed=F + window)
    got = _run(env, p, window, center)
    tabs = [egs_ref.no_sil_f16(m, v, window, center, 100)[0] for m, v in zip(p["mats"], p["vads"])]
    for c, (u, first, n, dst) in enumerate(zip(*p["table"])):
        want = tabs[u][first:first + n].reshape(-1)
        assert np.array_equal(got[dst:dst + n * F].view(np.uint16), want.view(np.uint16)), (c, u, first, n)
    assert (got[~_covered(p)] == SENTINEL).all()           # nothing outside the chunks is written


@pytest.mark.parametrize("F,ldx,window,center", CONFIGS[:4])
def test_chunks_within_one_double_rounding_of_the_float64_value(env, F, ldx, window, center):
    p = _problem(F, ldx, False, seed=100 + F + window)
    got = _run(env, p, window, center).astype(np.float64)
    vals = [egs_ref.no_sil_f16(m, v, window, center, 100)[1] for m, v in zip(p["mats"], p["vads"])]
    worst = 0.0
    for c, (u, first, n, dst) in enumerate(zip(*p["table"])):
        v = vals[u][first:first + n].reshape(-1)
        err = np.abs(got[dst:dst + n * F] - v)
        bound = egs_ref.half_ulp16(v) + 2 * 2.0 ** -24 * np.abs(v)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (c, u, first, n, float((err / bound).max()))
    print("worst error / bound = %.4f" % worst)


def test_half_conversion_rounds_from_the_float32_value(env):
    """Two roundings, as NumPy's astype(float16) of the float32 CMN output: in a two-frame utterance d0 = (x0 - x1) / 2 exactly;
    x0 = 2 + 2^-10, x1 = -2^-25 give d0 = 1 + 2^-11 + 2^-26, which rounds to the float32 1 + 2^-11, a float16 tie that goes to the
    even 1.0 -- a single rounding from the float64 value would give 1 + 2^-10.  (Integer features can never land there: their d is
    k / n with n <= 650, at least 2^-11 / n relative from any float16 tie.)"""
    torch, hiplib = env["torch"], env["hiplib"]
    x0, x1 = np.float32(2 + 2.0 ** -10), np.float32(-2.0 ** -25)
    x = np.array([[x0, -x0, 4 * x0], [x1, -x1, 4 * x1]], np.float32)
    want = egs_ref.no_sil_f16(x, np.ones(2), 300, True, 100)[0]
    assert want[0].tolist() == [1.0, -1.0, 4.0] and np.float16(egs_ref.cmn_f64(x)[0, 0]) == np.float16(1 + 2.0 ** -10)
    us, ul = _dev(torch, [0], np.int32), _dev(torch, [2], np.int32)
    count, rows = hiplib.vad_compact(_dev(torch, np.ones(2), np.float32), us, ul)
    y = torch.zeros(6, dtype=torch.float16, device="cuda")
    hiplib.egs_chunks(_dev(torch, x, np.float32), us, ul, count, rows, (np.array([0]), np.array([0]), np.array([2]), np.array([0], np.int64)),
                      np.array([2]), 300, True, 100, y)
    assert np.array_equal(y.cpu().numpy().view(np.uint16), want.reshape(-1).view(np.uint16))


def test_chunks_within_one_fp16_ulp_of_the_front_end_kernel(env):
    """float16 of xv_cmn_sliding_scatter_f32's output (the path the extractor uses), sliced by the same table."""
    torch, hiplib = env["torch"], env["hiplib"]
    F = 23
    p = _problem(F, F, False, seed=9)
    got = _run(env, p, 300, True)
    x = _dev(torch, p["x"], np.float32)
    voiced = np.concatenate(p["vads"]) != 0
    dst_row = np.where(voiced, np.cumsum(voiced) - 1, -1).astype(np.int32)
    y32 = torch.zeros((int(voiced.sum()), F), device="cuda")
    hiplib.cmn_sliding_scatter(x, _dev(torch, p["starts"], np.int32), _dev(torch, p["lens"], np.int32), len(p["lens"]), int(p["lens"].max()),
                               300, True, 100, _dev(torch, dst_row, np.int32), y32)
    ref = y32.cpu().numpy()
    ostart = np.concatenate([[0], np.cumsum(p["counts"])[:-1]])
    same = total = 0
    for u, first, n, dst in zip(*p["table"]):
        want = ref[ostart[u] + first:ostart[u] + first + n].reshape(-1)
        g = got[dst:dst + n * F]
        w16 = want.astype(np.float16)
        ulp = np.spacing(np.maximum(np.abs(w16), np.float16(2.0 ** -14)).astype(np.float16)).astype(np.float64)
        assert (np.abs(g.astype(np.float64) - w16.astype(np.float64)) <= ulp).all()
        same += int(np.count_nonzero(g == w16))
        total += g.size
    assert same > 0.99 * total


def test_a_table_past_the_voiced_count_raises_before_any_launch(env):
    torch, hiplib = env["torch"], env["hiplib"]
    p = _problem(23, 23, True, seed=1)
    u = 3
    bad = (np.array([u]), np.array([p["counts"][u] - 1]), np.array([2]), np.array([0], np.int64))
    x = _dev(torch, p["x"], np.float32)
    us, ul = _dev(torch, p["starts"], np.int32), _dev(torch, p["lens"], np.int32)
    count, rows = hiplib.vad_compact(_dev(torch, np.concatenate(p["vads"]), np.float32), us, ul)
    y = torch.full((p["y_elems"],), float(SENTINEL), dtype=torch.float16, device="cuda")
    with pytest.raises(ValueError):
        hiplib.egs_chunks(x, us, ul, count, rows, bad, count.cpu().numpy(), 300, True, 100, y)
    torch.cuda.synchronize()
    assert (y.cpu().numpy() == SENTINEL).all()             # no kernel ran


# ---------------------------------------------------------------------------------------------------------------------------------
# end to end: make_egs.py prepare -> lists / info -> allocate -> write
# ---------------------------------------------------------------------------------------------------------------------------------
def test_make_egs_end_to_end_against_front_end_and_ranges_loader(env, tmp_path):
    import make_egs
    import ze_utils
    from xvector_amd import frontend
    B, F = 4, 23
    data, egs_dir = str(tmp_path / "data"), str(tmp_path / "egs")
    utts = egs_ref.make_data_dir(data, 5, 4, 60, 150, F, seed=17, voiced_p=0.75)
    temp = os.path.join(egs_dir, "temp")
    make_egs.main(["prepare", "--data", data, "--out-dir", os.path.join(temp, "no_sil"), "--min-len", "40", "--min-num-utts", "3"])
    ns = os.path.join(temp, "no_sil")
    make_egs.main(["lists", "--utt2spk", os.path.join(ns, "utt2spk"), "--spk2utt", os.path.join(ns, "spk2utt"), "--utt2num-frames",
                   os.path.join(ns, "utt2num_frames"), "--temp", temp, "--num-heldout-utts", "0"])
    make_egs.main(["info", "--egs-dir", egs_dir, "--feat-dim", str(F), "--num-repeats", "8", "--frames-per-iter", "1000000"])
    make_egs.main(["allocate", "--num-repeats=8", "--num-jobs=1", "--minibatch-size=%d" % B, "--min-frames-per-chunk=20",
                   "--max-frames-per-chunk=40", "--frames-per-iter=1000", "--num-archives=1",
                   "--utt2len-filename=" + os.path.join(temp, "utt2num_frames.train"), "--utt2int-filename=" + os.path.join(temp, "utt2int.train"),
                   "--egs-dir=" + egs_dir])
    make_egs.main(["write", "--random-seed=2468", "--feature-dim=%d" % F, "--minibatch-size=%d" % B, "--shuffle=True",
                   "--outputs-file=" + os.path.join(temp, "outputs.1"), "--egs-dir=" + egs_dir, "--feats-scp", os.path.join(data, "feats.scp"),
                   "--vad-scp", os.path.join(data, "vad.scp"), "--frame-budget", "700"])
    num_archives, feat_dim, counts = ze_utils.verify_egs_dir(egs_dir)
    assert (num_archives, feat_dim) == (1, F) and list(counts) == [1] and counts[1] >= 7
    kept = [l.split() for l in open(os.path.join(temp, "utt2num_frames.train"))]
    assert int(open(os.path.join(egs_dir, "info", "num_frames")).read()) == sum(int(n) for _, n in kept)
    assert dict((k, int(n)) for k, n in kept) == dict((k, int(np.count_nonzero(utts[k][1]))) for k, _ in kept)
    # the no-silence table by the parent's path (FrontEnd.apply) and by the oracle; chunks cut from both by the ranges loader
    keys = list(utts)
    fe = frontend.FrontEnd("cuda:0", 300, True, 100).apply([utts[k][0] for k in keys], [utts[k][1] for k in keys])
    scp_fe = egs_ref.write_table(str(tmp_path / "fe"), dict(zip(keys, fe)))
    scp_or = egs_ref.write_table(str(tmp_path / "or"), dict((k, egs_ref.cmn_f64(m)[egs_ref.voiced_rows(v)].astype(np.float32))
                                                            for k, (m, v) in utts.items()))
    count = counts[1]
    ranges = os.path.join(temp, "ranges.1")
    want_fe, want_labels = egs_ref.served_by_ranges_loader(ranges, scp_fe, count, B, F)
    want_or, _ = egs_ref.served_by_ranges_loader(ranges, scp_or, count, B, F)
    members, labels = egs_ref.read_tar(os.path.join(egs_dir, "egs.1.tar"))
    perm = np.random.RandomState(2468).permutation(np.arange(count))
    spk2int = dict(l.split() for l in open(os.path.join(temp, "spk2int")))
    assert len(members) == count and labels.shape == (count, B) and labels.max() < len(spk2int)
    agree = 0
    for i in range(count):
        a, b = want_fe[perm[i]], want_or[perm[i]]
        got = members[i]
        assert got.dtype == np.float16 and got.shape == a.shape
        assert np.array_equal(labels[i], want_labels[perm[i]])
        eq = a == b                                        # where the two CMN paths agree in float32: bit for bit
        agree += int(eq.sum())
        assert np.array_equal(got[eq], a.astype(np.float16)[eq])
        a16 = a.astype(np.float16)
        ulp = np.spacing(np.maximum(np.abs(a16), np.float16(2.0 ** -14)).astype(np.float16)).astype(np.float64)
        assert (np.abs(got.astype(np.float64) - a16.astype(np.float64)) <= ulp).all()
    assert agree > 0.99 * sum(m.size for m in members)
