"""Sliding-window extraction, the parts that need no GPU: the sub-segment plan against a brute-force loop, the
NumPy restatement of xv_cmn_sliding_gather_f32 (tests/subseg_ref.py) against the oracle's CMN + selection, the command line's
usage errors, the key and subsegments-file formats, and the ABI."""
import io

import numpy as np
import pytest

import subseg_ref

BASE = ["--vector-wspecifier", "ark,scp:/nonexistent/x.ark,/nonexistent/x.scp", "--model-dir", "/nonexistent/model",
        "--feature-rspecifier", "scp:feats.scp"]
RULES = [(150, 75, 25), (150, 150, 25), (64, 1, 64), (100, 30, 100), (10, 7, 1)]         # (window, period, min_chunk_size)


# ---- planning ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window,period,mn", RULES)
def test_plan_subsegments_against_the_loop(window, period, mn):
    from xvector_amd import engine
    for n in range(0, 701):
        plan = engine.plan_subsegments(n, mn, window, period)
        assert plan == subseg_ref.plan_loop(n, mn, window, period), n
        if n == 0 or n < mn:
            assert plan is None
            continue
        starts, lens = [s for s, _ in plan], [m for _, m in plan]
        assert starts == [k * period for k in range(len(plan))]
        assert all(m == window for m in lens[:-1]) and min(lens) >= mn and lens[-1] == min(window, n - starts[-1])
        if n <= window:
            assert plan == [(0, n)]
        # the union of the sub-segments is [0, N) exactly when the last candidate piece was kept (period <= window: no holes)
        k_last = 0 if n <= window else -(-(n - window) // period)
        last_kept = len(plan) == k_last + 1
        assert last_kept == (starts[-1] + lens[-1] == n)
        assert starts[-1] + lens[-1] <= n
        if not last_kept:
            assert min(window, n - k_last * period) < mn and len(plan) == k_last


def test_plan_subsegments_refuses_a_period_outside_the_window():
    from xvector_amd import engine
    for window, period in ((150, 151), (150, 0), (10, -1)):
        with pytest.raises(ValueError):
            engine.plan_subsegments(400, 25, window, period)
        with pytest.raises(ValueError):
            engine.plan_subsegment_table([400], 25, window, period)


@pytest.mark.parametrize("window,period,mn", RULES)
def test_plan_subsegment_table_equals_the_loop(window, period, mn):
    from xvector_amd import engine
    rng = np.random.default_rng(window * 1000 + period)
    lens = rng.integers(0, 700, size=200)
    lens[:6] = [0, mn, max(mn - 1, 0), window, window + 1, window + period]
    order, c_utt, c_start, c_len, seg = engine.plan_subsegment_table(lens, mn, window, period)
    plans = [subseg_ref.plan_loop(int(t), mn, window, period) for t in lens]
    want_order = sorted((i for i, p in enumerate(plans) if p), key=lambda i: lens[i])            # sorted() is stable
    assert order.tolist() == want_order
    assert np.array_equal(np.diff(seg), [len(plans[u]) for u in want_order]) and seg[0] == 0 and seg[-1] == len(c_utt)
    assert c_utt.tolist() == [u for u in want_order for _ in plans[u]]
    assert c_start.tolist() == [s for u in want_order for s, _ in plans[u]]
    assert c_len.tolist() == [m for u in want_order for _, m in plans[u]]
    assert all(a.dtype == np.int64 for a in (order, c_utt, c_start, c_len, seg))


def test_plan_subsegment_table_of_nothing():
    from xvector_amd import engine
    order, c_utt, c_start, c_len, seg = engine.plan_subsegment_table([0, 3, 24], 25, 150, 75)
    assert len(order) == len(c_utt) == len(c_start) == len(c_len) == 0 and seg.tolist() == [0]


def test_extractor_refuses_bad_windows_before_it_touches_the_model():
    from xvector_amd import engine

    class FakeModel(object):
        f16bf8 = False
    for kw in (dict(window=150, period=151), dict(window=150, period=0), dict(window=20), dict(period=75)):
        with pytest.raises(ValueError):
            engine.Extractor(FakeModel(), 25, -1, **kw)
    ex = engine.Extractor(FakeModel(), 25, -1, window=150)
    assert (ex.window, ex.period) == (150, 150)
    ex = engine.Extractor(FakeModel(), 25, -1)
    assert ex.window is None and ex.period is None


# ---- the gather's reference against the oracle chain --------------------------------------------------------------------------
def _utterances(rng, F=23):
    lens = [1000, 120, 700]                              # 120 < both CMN windows' 300; see the VADs below for 700
    mats = [(rng.standard_normal((t, F)) * 4 + 10 * rng.standard_normal(F)).astype(np.float32) for t in lens]
    vads = [(rng.random(t) < 0.7).astype(np.float32) for t in lens]
    vads[2][150:500] = 0                                 # a silent run longer than the CMN window of 300 (and of 61)
    vads[2][500:520] = 1
    return lens, mats, vads


@pytest.mark.parametrize("center,cmn", [(True, 300), (False, 300), (True, 61), (False, 61)])
def test_gather_reference_equals_the_oracle_chain(center, cmn):
    from oracle import oracle
    rng = np.random.default_rng(5)
    lens, mats, vads = _utterances(rng)
    F = 23
    start = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    x = np.concatenate(mats)
    count, rows = subseg_ref.voiced_lists(vads, start, lens, x.shape[0])
    cu, cf, cl = [], [], []
    for u in range(len(lens)):
        for s, m in subseg_ref.plan_loop(int(count[u]), 25, 150, 75):
            cu.append(u), cf.append(s), cl.append(m)
    crow = np.concatenate([[3], 3 + np.cumsum(np.asarray(cl) + 2)[:-1]]).astype(np.int64)          # two gap rows between the chunks
    y = np.zeros((int(crow[-1] + cl[-1] + 4), 24), np.float32)
    subseg_ref.gather(x, F, start, lens, count, rows, cu, cf, cl, crow, cmn, center, 100, y)
    used = np.zeros(y.shape[0], bool)
    for u, s, m, r in zip(cu, cf, cl, crow):
        sel = oracle.select_voiced(oracle.sliding_cmn(mats[u], cmn, center, 100), vads[u])
        # the same float64 window mean rounded to float32 once; the oracle slides its sum, the restatement adds the window afresh
        want, got = sel[s:s + m], y[r:r + m, :F]
        assert np.array_equal(got, want)
        used[r:r + m] = True
    assert not y[~used].any() and not y[:, F:].any()
    # no VAD at all: chunks of consecutive raw frames
    y2 = np.zeros((200, 24), np.float32)
    subseg_ref.gather(x, F, start, lens, None, None, [0, 1], [100, 0], [150, 40], [0, 160], cmn, center, 100, y2)
    for got, want in ((y2[:150, :F], oracle.sliding_cmn(mats[0], cmn, center, 100)[100:250]),
                      (y2[160:200, :F], oracle.sliding_cmn(mats[1], cmn, center, 100)[:40])):
        assert np.array_equal(got, want)


def test_gather_reference_skips_what_the_header_says():
    rng = np.random.default_rng(6)
    x = rng.standard_normal((50, 5)).astype(np.float32)
    count, rows = subseg_ref.voiced_lists([np.ones(50)], [0], [50], 50)
    y = np.zeros((20, 8), np.float32)
    # voiced index past the count; destination rows past y; an utterance out of range; a span leaving x
    subseg_ref.gather(x, 5, [0], [50], count, rows, [0, 0, 1], [45, 0, 0], [10, 10, 5], [0, 15, 10], 300, True, 100, y)
    assert y[:5, :5].all() and not y[5:15].any() and y[15:20, :5].all() and not y[:, 5:].any()
    y[:] = 0
    subseg_ref.gather(x, 5, [40], [50], None, None, [0], [0], [5], [0], 300, True, 100, y)
    assert not y.any()


# ---- the command line -----------------------------------------------------------------------------------------------------------
def _usage_error(argv, capsys):
    import extract_embedding as ee
    with pytest.raises(SystemExit) as e:
        ee.get_args(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_usage_errors_of_the_sliding_flags(capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert "--period goes with --window" in _usage_error(BASE + ["--period", "75"], capsys)
    assert "--subsegments-file goes with --window" in _usage_error(BASE + ["--subsegments-file", "s"], capsys)
    err = _usage_error(BASE + ["--window", "150", "--period", "151"], capsys)
    assert "--period" in err and "--window" in err
    err = _usage_error(BASE + ["--window", "50"], capsys)                              # the default --min-chunk-size is 100
    assert "--window" in err and "--min-chunk-size" in err
    err = _usage_error(BASE + ["--window", "20", "--min-chunk-size", "25"], capsys)
    assert "--window" in err and "--min-chunk-size" in err
    err = _usage_error(["--vector-wspecifier", "ark:x", "--model-dir", "/nonexistent/model", "--wav-rspecifier", "scp:wav.scp",
                        "--cmn-window", "300", "--window", "150", "--frame-shift", "10"], capsys)
    assert "--frame-shift" in err and "--wav-rspecifier" in err


def test_sliding_mode_refuses_more_than_one_rank(capsys, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    err = _usage_error(BASE + ["--window", "150"], capsys)
    assert "--window" in err and "WORLD_SIZE=2" in err and "one process" in err


def test_window_alone_sets_the_period(tmp_path, monkeypatch):
    import extract_embedding as ee
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    (tmp_path / "model.meta").write_text("{}")
    common = ["--vector-wspecifier", "ark:x", "--model-dir", str(tmp_path), "--feature-rspecifier", "scp:f.scp"]
    args = ee.get_args(common + ["--window", "150"])
    assert (args.window, args.period, args.frame_shift, args.subsegments_file) == (150, 150, 10.0, "")
    args = ee.get_args(common + ["--window", "150", "--period", "75", "--frame-shift", "12.5", "--subsegments-file", "S"])
    assert (args.window, args.period, args.frame_shift, args.subsegments_file) == (150, 75, 12.5, "S")
    args = ee.get_args(common)                                                           # nothing given: today's behaviour
    assert (args.window, args.period) == (0, 0)


def test_make_embedding_refuses_sliding_arguments_it_cannot_serve(monkeypatch):
    import models
    from xvector_amd import dist as xdist
    m = models.Model()
    for kw in (dict(window=150, period=151), dict(window=20), dict(period=75), dict(subsegments=io.StringIO())):
        with pytest.raises(ValueError):
            m.make_embedding(iter(()), io.BytesIO(), "/nonexistent/model", 25, -1, True, None, **kw)
    monkeypatch.setattr(xdist, "group_shape", lambda: (0, 2))
    with pytest.raises(ValueError, match="one process"):
        m.make_embedding(iter(()), io.BytesIO(), "/nonexistent/model", 25, -1, True, None, window=150)


# ---- keys and subsegments lines ---------------------------------------------------------------------------------------------------
class _Log(object):
    def __init__(self):
        self.lines = []

    def warning(self, msg):
        self.lines.append(msg)


def test_keys_and_subsegments_lines():
    from xvector_amd import extract_stream as xs
    import kaldi_io
    assert xs.subsegment_key("spk1-utt2", 0, 150) == "spk1-utt2-00000000-00000150"
    assert xs.subsegment_key("u", 12345678, 123456789) == "u-12345678-123456789"
    assert xs.subsegment_line("u-00000075-00000225", "u", 75, 225, 10.0) == "u-00000075-00000225 u 0.750 2.250\n"
    assert xs.subsegment_line("k", "u", 75, 226, 12.5) == "k u 0.938 2.825\n"
    assert xs.subsegment_line("k", "u", 0, 1, 10.0) == "k u 0.000 0.010\n"

    # Extraction.emit_subsegments + the writer thread: expanded keys, one line per vector, rejected utterances warned about
    class Ex(object):
        window = 150
    out, sub, log = io.BytesIO(), io.StringIO(), _Log()
    writer = xs.VectorWriter(out, sub, 12.5)
    run = xs.Extraction(None, Ex(), None, writer, log, 25, -1)
    assert run.sliding
    vecs = np.arange(12, dtype=np.float32).reshape(3, 4)
    spans = np.array([[0, 150], [75, 226], [3, 90]], np.int32)
    run.emit_subsegments(["a", "short", "empty", "b"], np.array([226, 10, 0, 87]), vecs, spans, np.array([0, 2, 2, 2, 3]))
    writer.close()
    writer.check()
    got = list(kaldi_io.read_vec_flt_ark(io.BytesIO(out.getvalue())))
    assert [k for k, _ in got] == ["a-00000000-00000150", "a-00000075-00000226", "b-00000003-00000090"]
    assert all(np.array_equal(v, vecs[i]) for i, (_, v) in enumerate(got))
    assert sub.getvalue() == ("a-00000000-00000150 a 0.000 1.875\na-00000075-00000226 a 0.938 2.825\n"
                              "b-00000003-00000090 b 0.037 1.125\n")
    assert (run.num_success, run.num_fail, run.num_vectors) == (2, 2, 3)
    assert len(log.lines) == 2 and "short" in log.lines[0] and "Zero-length" in log.lines[1]
    # without a window nothing changes: the writer takes (keys, vectors) and writes no line
    class Plain(object):
        pass
    out2, sub2 = io.BytesIO(), io.StringIO()
    writer = xs.VectorWriter(out2, sub2)
    run = xs.Extraction(None, Plain(), None, writer, log, 25, -1)
    assert not run.sliding
    run.emit(["a", "b"], np.array([100, 100]), vecs[:2], np.array([True, True]))
    writer.close()
    writer.check()
    assert [k for k, _ in kaldi_io.read_vec_flt_ark(io.BytesIO(out2.getvalue()))] == ["a", "b"] and sub2.getvalue() == ""


# ---- ABI ------------------------------------------------------------------------------------------------------------------------
def test_abi_has_the_gather():
    from xvector_amd import hiplib
    assert hiplib.ABI_VERSION >= 37 and "xv_cmn_sliding_gather_f32" in hiplib.SYMBOLS
    lib = hiplib.load()
    assert lib.xv_version() == hiplib.ABI_VERSION and lib.xv_cmn_sliding_gather_f32 is not None
    assert callable(hiplib.cmn_sliding_gather)
