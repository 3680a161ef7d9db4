"""Sliding-window extraction on the MI355X: xv_cmn_sliding_gather_f32 against its NumPy restatement
(tests/subseg_ref.py), the extractor's sliding mode on its three routes against the plan and the fp64 oracle, and the command line
from audio against the command line from tables."""
import ctypes
import logging
import os

import numpy as np
import pytest

import subseg_ref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

F = 23
KERNEL_LENS = [1, 2, 50, 299, 300, 301, 1000, 500, 900]
ROUTE_LENS = [30, 149, 150, 151, 226, 400, 1000, 10]
WINDOW, PERIOD, MIN_CHUNK = 150, 75, 25


def _close(got, ref):
    """The rule of tests/test_gpu_frontend.py: both sides round one float64 difference to float32; only the order of the float64
    additions differs."""
    assert got.shape == ref.shape and got.dtype == np.float32
    ulp = np.spacing(np.maximum(np.abs(ref), np.float32(1e-3)).astype(np.float32))
    assert np.all(np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= ulp)
    same = float(np.mean(got == ref))
    print("identical elements: %.6f of %d" % (same, got.size))
    assert same > 0.999


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kin():
    """Raw rows, VAD lists and a chunk table that exercises the kernel's paths; host arrays and their device copies."""
    import torch
    from xvector_amd import hiplib
    hiplib.require_gpu()
    rng = np.random.default_rng(2024)
    lens = np.array(KERNEL_LENS, np.int32)
    start = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    x24 = (rng.standard_normal((int(lens.sum()), 24)) * 4 + 10 * rng.standard_normal(24)).astype(np.float32)      # column 23: not a feature
    vads = [(rng.random(t) < 0.7).astype(np.float32) for t in lens]
    vads[0][:] = 1
    vads[7][:] = 1                                     # fully voiced
    vads[8][200:600] = 0                               # a 400-frame silent gap: longer than every CMN window used here
    vads[8][190:200] = 1
    vads[8][600:610] = 1
    count, rows = subseg_ref.voiced_lists(vads, start, lens, x24.shape[0])
    cu, cf, cl = [], [], []
    for u in range(len(lens)):
        for s, m in subseg_ref.plan_loop(int(count[u]), 1, 150, 75) or []:    # 150 voiced frames every 75
            cu.append(u), cf.append(s), cl.append(m)
    cu += [6, 6, 8, 8]
    cf += [10, 100, 120, 120]                          # 64 and 65 rows (the segment boundary); two identical chunks (across the gap)
    cl += [64, 65, 150, 150]
    n_good = len(cu)
    crow = (2 + np.concatenate([[0], np.cumsum(np.asarray(cl) + 3)[:-1]])).astype(np.int64)      # three untouched rows between chunks
    tail = int(crow[-1] + cl[-1] + 2)                  # the good chunks end before this row; the cut ones follow
    y_rows = tail + 50
    # chunks that must be cut: a voiced index past the count (10 of 30 rows exist), a negative first frame (rows 5 .. 11 of 12), rows
    # past the end of y (5 of 20) and before its start (2 of 20, the two leading rows), utterances that do not exist
    cu += [6, 5, 3, 3, len(lens), -1]
    cf += [int(count[6]) - 10, -5, 0, 0, 0, 0]
    cl += [30, 12, 20, 20, 10, 10]
    crow = np.concatenate([crow, [tail, tail + 30, tail + 45, -18, 0, 0]])
    order = np.arange(len(cu))[::-1]                   # listed in descending order
    tab = [np.asarray(a, np.int32)[order].copy() for a in (cu, cf, cl, crow)]

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return dict(torch=torch, hiplib=hiplib, lens=lens, start=start, x24=x24, vads=vads, count=count, rows=rows, tab=tab, y_rows=y_rows,
                n_good=n_good, good_rows=int(np.sum(cl[:n_good])), tail=tail, dev=dev, x24_d=dev(x24), x23_d=dev(x24[:, :F].copy()), d=[dev(a) for a in (start, lens, count, rows)],
                tab_d=[dev(a) for a in tab])


def _run(k, x_d, cmn, center, voiced=True, tab_d=None, y_rows=None):
    torch, hiplib = k["torch"], k["hiplib"]
    y = torch.zeros((y_rows or k["y_rows"], 24), device="cuda")
    s, n, c, r = k["d"]
    t = tab_d or k["tab_d"]
    hiplib.cmn_sliding_gather(x_d, s, n, c if voiced else None, r if voiced else None, t[0], t[1], t[2], t[3], 150, cmn, center, 100, y)
    return y.cpu().numpy()


@pytest.fixture(scope="module")
def kref(kin):
    """The restatement's output per (center, window): computed once."""
    cache = {}

    def get(center, cmn):
        if (center, cmn) not in cache:
            k = kin
            y = np.zeros((k["y_rows"], 24), np.float32)
            subseg_ref.gather(k["x24"][:, :F], F, k["start"], k["lens"], k["count"], k["rows"], *k["tab"], cmn, center, 100, y)
            y.setflags(write=False)
            cache[(center, cmn)] = y
        return cache[(center, cmn)]
    return get


@pytest.mark.parametrize("center,cmn", [(True, 300), (False, 300), (True, 61)])
@pytest.mark.parametrize("ldx", [23, 24])
def test_gather_matches_the_restatement(kin, kref, center, cmn, ldx):
    k = kin
    ref = kref(center, cmn)
    got = _run(k, k["x23_d"] if ldx == 23 else k["x24_d"][:, :F], cmn, center)
    written = ref[:, :F].any(axis=1)
    # every row of the good chunks but the 1-frame utterance's (x - x = 0), and the 10 + 7 + 5 + 2 rows left of the cut ones
    assert written.sum() == k["good_rows"] - 1 + 24 and k["good_rows"] > 4000
    _close(got[written][:, :F], ref[written][:, :F])
    # untouched rows and the 24th column stay zero: gap rows, what lies past a voiced count, before a negative first frame
    assert not got[~written].any() and not got[:, F:].any()
    # the cut chunks wrote what the header leaves them: 10 rows under the count limit, 7 rows from frame 0 on, 5 rows up to the end
    # of y, 2 rows from the start of y
    tail = k["tail"]
    assert got[tail:tail + 10, :F].all() and not got[tail + 10:tail + 35].any() and got[tail + 35:tail + 42, :F].all()
    assert not got[tail + 42:tail + 45].any() and got[tail + 45:, :F].all() and got.shape[0] == tail + 50
    assert got[:2, :F].all() and np.array_equal(got[:2], ref[:2])


def test_gather_null_vad_repeat_and_compact(kin):
    """Both VAD pointers NULL = an all-ones VAD; a second launch gives the same bits; xv_vad_compact_i32 gives the lists used here."""
    k, torch, hiplib = kin, kin["torch"], kin["hiplib"]
    lens, start = k["lens"], k["start"]
    cu, cf, cl = [], [], []
    for u in range(len(lens)):
        for s, m in subseg_ref.plan_loop(int(lens[u]), 1, 150, 75):
            cu.append(u), cf.append(s), cl.append(m)
    crow = 1 + np.concatenate([[0], np.cumsum(np.asarray(cl) + 1)[:-1]])
    tab_d = [k["dev"](np.asarray(a, np.int32)) for a in (cu, cf, cl, crow)]
    rows_all = int(crow[-1] + cl[-1]) + 1
    plain = _run(k, k["x23_d"], 300, True, voiced=False, tab_d=tab_d, y_rows=rows_all)
    ones_count, ones_rows = subseg_ref.voiced_lists([np.ones(t) for t in lens], start, lens, k["x24"].shape[0])
    saved = k["d"]
    try:
        k["d"] = [saved[0], saved[1], k["dev"](ones_count), k["dev"](ones_rows)]
        voiced = _run(k, k["x23_d"], 300, True, voiced=True, tab_d=tab_d, y_rows=rows_all)
    finally:
        k["d"] = saved
    assert plain[:, :F].any(axis=1).sum() == sum(cl) - 1 and np.array_equal(plain, voiced)      # (the 1-frame utterance: x - x = 0)
    a, b = _run(k, k["x24_d"][:, :F], 61, False), _run(k, k["x24_d"][:, :F], 61, False)
    assert np.array_equal(a, b)
    count_d, rows_d = hiplib.vad_compact(k["dev"](np.concatenate(k["vads"])), saved[0], saved[1])
    assert np.array_equal(count_d.cpu().numpy(), k["count"])
    got_rows = rows_d.cpu().numpy()
    for u in range(len(lens)):
        assert np.array_equal(got_rows[start[u]:start[u] + k["count"][u]], k["rows"][start[u]:start[u] + k["count"][u]])


def test_gather_refuses_bad_arguments_without_a_launch(kin):
    k, torch, hiplib = kin, kin["torch"], kin["hiplib"]
    lib = hiplib.load()
    y = torch.zeros((k["y_rows"], 24), device="cuda")
    x = k["x23_d"]
    s, n, c, r = k["d"]
    t = k["tab_d"]
    p = lambda a: None if a is None else ctypes.c_void_p(a.data_ptr())

    def call(**kw):
        a = dict(x=x, ldx=23, F=F, utt_start=s, utt_len=n, count=c, rows=r, cu=t[0], cf=t[1], cl=t[2], cr=t[3], n_chunks=t[0].numel(),
                 cmn=300, minw=100, y=y, ldy=24)
        a.update(kw)
        return lib.xv_cmn_sliding_gather_f32(p(a["x"]), a["ldx"], a["F"], x.shape[0], p(a["utt_start"]), p(a["utt_len"]), len(k["lens"]),
                                             p(a["count"]), p(a["rows"]), p(a["cu"]), p(a["cf"]), p(a["cl"]), p(a["cr"]), a["n_chunks"],
                                             150, a["cmn"], 1, a["minw"], p(a["y"]), a["ldy"], y.shape[0], None)
    bad = [dict(x=None), dict(utt_start=None), dict(utt_len=None), dict(cu=None), dict(cf=None), dict(cl=None), dict(cr=None),
           dict(y=None), dict(count=None), dict(rows=None), dict(cmn=0), dict(cmn=-3), dict(minw=0), dict(ldx=22), dict(ldy=22),
           dict(n_chunks=-1)]
    for kw in bad:
        assert call(**kw) == -1, kw                    # XV_ERR_BAD_ARG
        assert b"cmn_sliding_gather" in lib.xv_last_error()
    torch.cuda.synchronize()
    assert not y.cpu().numpy().any()                   # nothing was launched
    assert call(n_chunks=0) == 0 and call(n_chunks=0, x=None, y=None) == 0
    torch.cuda.synchronize()
    assert not y.cpu().numpy().any()
    assert call() == 0                                 # and the same arguments, all in order, do write
    torch.cuda.synchronize()
    assert y.cpu().numpy().any()


# ---------------------------------------------------------------------------------------------------------------------------------
# the extractor's sliding mode
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net():
    from xvector_amd import engine, hiplib, synthetic, topology
    hiplib.require_gpu()
    topo = topology.get("ModelWithoutDropout")
    w = synthetic.trained_like(topo, F, seed=3)
    rng = np.random.default_rng(77)
    mats = [(rng.standard_normal((t, F)) * 3 + 1.5).astype(np.float32) for t in ROUTE_LENS]
    vads = [(rng.random(t) < 0.7).astype(np.float32) for t in ROUTE_LENS]
    vads[2][:] = 1                                      # 150 voiced frames: exactly one window
    vads[5][100:380] = 0                                # 400 frames with a long silent run
    models = {}

    def model(precision):
        if precision not in models:
            models[precision] = engine.DeviceModel(w, topo, "cuda:0", precision=precision)
        return models[precision]
    return dict(engine=engine, topo=topo, w=w, mats=mats, vads=vads, model=model)


@pytest.fixture(scope="module")
def table_refs(net):
    """fp64 oracle x-vector of every sub-segment of the table route: computed once, shared by both arithmetics."""
    from oracle import oracle
    refs = []
    for m in net["mats"]:
        plan = subseg_ref.plan_loop(m.shape[0], MIN_CHUNK, WINDOW, PERIOD)
        refs.append(None if plan is None else [oracle.forward(m[s:s + n], net["w"], net["topo"], np.float64) for s, n in plan])
    return refs


@pytest.fixture(scope="module")
def raw_refs(net):
    """The oracle chain of the raw routes -- CMN, select, slice, forward -- and the RAW-frame span of every sub-segment."""
    from oracle import oracle
    refs = []
    for m, v in zip(net["mats"], net["vads"]):
        sel = oracle.select_voiced(oracle.sliding_cmn(m, 300, True, 100), v)
        plan = None if sel is None else subseg_ref.plan_loop(sel.shape[0], MIN_CHUNK, WINDOW, PERIOD)
        if plan is None:
            refs.append(None)
            continue
        voiced = np.flatnonzero(v != 0)
        refs.append(([oracle.forward(sel[s:s + n], net["w"], net["topo"], np.float64) for s, n in plan],
                     np.array([[voiced[s], voiced[s + n - 1] + 1] for s, n in plan], np.int32)))
    return refs


def _worst(vecs, refs):
    from oracle import oracle
    worst = max(oracle.rel_l2(v, r) for v, r in zip(vecs, refs))
    print("worst rel-L2 against the fp64 oracle over %d sub-segments: %.3e" % (len(refs), worst))
    return worst


@pytest.mark.parametrize("precision", ["f16bf8", "bf16x3"])
def test_table_route(net, table_refs, precision):
    """Counts and spans equal the plan (sub-segments of one utterance straddle batches at 700 rows); every vector within 5e-5 of
    the fp64 oracle on its slice; a one-window utterance agrees with the averaging extractor (len * e / len: at most an ulp)."""
    engine, mats = net["engine"], net["mats"]
    model = net["model"](precision)
    ex = engine.Extractor(model, MIN_CHUNK, 10000, window=WINDOW, period=PERIOD, max_batch_rows=700)
    got = ex.extract(mats)
    assert ex.stats["batches"] >= 4 and not ex.demoted and ex.stats.get("fallback_windows", 0) == 0
    assert len(got) == len(mats) and got[-1] is None                  # 10 rows < min_chunk_size: rejected
    flat_v, flat_r = [], []
    for m, g, refs in zip(mats, got, table_refs):
        plan = subseg_ref.plan_loop(m.shape[0], MIN_CHUNK, WINDOW, PERIOD)
        assert (plan is None) == (g is None)
        if plan is None:
            continue
        vecs, spans = g
        assert vecs.shape == (len(plan), model.embed_dim) and vecs.dtype == np.float32
        assert spans.dtype == np.int32 and spans.tolist() == [[s, s + n] for s, n in plan]
        flat_v.extend(vecs), flat_r.extend(refs)
    assert len(flat_v) == 26
    assert _worst(flat_v, flat_r) < 5e-5
    # as_array: the flat block in input order with per-utterance offsets
    ex2 = engine.Extractor(model, MIN_CHUNK, 10000, window=WINDOW, period=PERIOD, max_batch_rows=700)
    vecs, spans, off = ex2.finish(ex2.submit(mats), as_array=True)
    assert off.tolist() == np.concatenate([[0], np.cumsum([0 if g is None else len(g[0]) for g in got])]).tolist()
    assert np.array_equal(vecs, np.concatenate([g[0] for g in got if g is not None]))
    assert np.array_equal(spans, np.concatenate([g[1] for g in got if g is not None]))
    # N <= window: one sub-segment = the whole utterance = the one chunk of the averaging mode
    plain = engine.Extractor(model, MIN_CHUNK, -1).extract(mats)
    for i, t in enumerate(ROUTE_LENS):
        if MIN_CHUNK <= t <= WINDOW:
            np.testing.assert_allclose(got[i][0][0], plain[i], rtol=1e-6)


@pytest.mark.parametrize("rows", [700, 262144])
def test_raw_routes_agree_and_meet_the_oracle(net, raw_refs, rows):
    """submit_raw and submit_device_raw in sliding mode: the same kernel, plan and integers -> equal vectors and spans; both
    against the oracle chain; the spans are RAW frame indices."""
    import torch
    engine, mats, vads = net["engine"], net["mats"], net["vads"]
    if engine._host_lib() is None:
        pytest.skip("libxvector_host.so disabled: no submit_raw to compare with")
    model = net["model"]("bf16x3")
    ex = engine.Extractor(model, MIN_CHUNK, 10000, window=WINDOW, period=PERIOD, max_batch_rows=rows)
    handle, lens, dropped = ex.submit_raw(mats, vads, 300, True)
    a = ex.finish(handle)
    T = np.array(ROUTE_LENS, np.int64)
    row0 = np.concatenate([[0], np.cumsum(T)[:-1]])
    ex2 = engine.Extractor(model, MIN_CHUNK, 10000, window=WINDOW, period=PERIOD, max_batch_rows=rows)
    handle, lens2, dropped2 = ex2.submit_device_raw(torch.from_numpy(np.concatenate(mats)).cuda(), row0, T,
                                                    torch.from_numpy(np.concatenate(vads)).cuda(), 300, True)
    b = ex2.finish(handle)
    assert np.array_equal(lens, lens2) and np.array_equal(dropped, dropped2) and not dropped.any()
    assert np.array_equal(lens, [int((v != 0).sum()) for v in vads])
    assert ex.stats == ex2.stats and (rows != 700 or ex.stats["batches"] >= 3)
    flat_v, flat_r = [], []
    for ga, gb, ref in zip(a, b, raw_refs):
        assert (ga is None) == (gb is None) == (ref is None)
        if ref is None:
            continue
        assert np.array_equal(ga[0], gb[0]) and np.array_equal(ga[1], gb[1])
        assert np.array_equal(ga[1], ref[1]) and ga[1].dtype == np.int32
        flat_v.extend(ga[0]), flat_r.extend(ref[0])
    assert len(flat_v) >= 12
    assert _worst(flat_v, flat_r) < 5e-5
    # without a VAD: every frame, spans as on the table route
    ex3 = engine.Extractor(model, MIN_CHUNK, 10000, window=WINDOW, period=PERIOD, max_batch_rows=rows)
    handle, _, _ = ex3.submit_raw(mats, None, 300, True)
    c = ex3.finish(handle)
    ex4 = engine.Extractor(model, MIN_CHUNK, 10000, window=WINDOW, period=PERIOD, max_batch_rows=rows)
    handle, _, _ = ex4.submit_device_raw(torch.from_numpy(np.concatenate(mats)).cuda(), row0, T, None, 300, True)
    d = ex4.finish(handle)
    for m, gc, gd in zip(mats, c, d):
        plan = subseg_ref.plan_loop(m.shape[0], MIN_CHUNK, WINDOW, PERIOD)
        assert (plan is None) == (gc is None) == (gd is None)
        if plan is not None:
            assert np.array_equal(gc[0], gd[0]) and gc[1].tolist() == gd[1].tolist() == [[s, s + n] for s, n in plan]


def test_sliding_redo_on_the_twin_equals_bf16x3(net):
    """As test_device_front_end_redo_and_demotion_equal_bf16x3: a window with one utterance scaled by 1e6 trips the f16bf8 status
    word and comes back from the bf16x3 twin -- equal to the bf16x3 extractor's sliding output, vectors and spans."""
    engine, vads = net["engine"], net["vads"]
    if engine._host_lib() is None:
        pytest.skip("libxvector_host.so disabled: no submit_raw")
    loud = list(net["mats"])
    loud[6] = loud[6] * np.float32(1e6)
    for rows in (262144, 700):
        ref_ex = engine.Extractor(net["model"]("bf16x3"), MIN_CHUNK, 10000, window=WINDOW, period=PERIOD, max_batch_rows=rows)
        handle, lens, dropped = ref_ex.submit_raw(loud, vads, 300, True)
        want = ref_ex.finish(handle)
        ex = engine.Extractor(net["model"]("f16bf8"), MIN_CHUNK, 10000, window=WINDOW, period=PERIOD, max_batch_rows=rows,
                              accuracy_probe=False)
        handle, lens2, dropped2 = ex.submit_raw(loud, vads, 300, True)
        got = ex.finish(handle)
        assert ex.stats["fallback_windows"] == 1 and not ex.demoted
        assert ex._fallback_ex.window == WINDOW and ex._fallback_ex.period == PERIOD
        assert np.array_equal(lens, lens2) and np.array_equal(dropped, dropped2)
        for g, w in zip(got, want):
            assert (g is None) == (w is None)
            if g is not None:
                assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1])
        # inside the range nothing is repeated, and the probe runs on sub-segments as on chunks
        ex = engine.Extractor(net["model"]("f16bf8"), MIN_CHUNK, 10000, window=WINDOW, period=PERIOD, max_batch_rows=rows)
        handle, _, _ = ex.submit_raw(net["mats"], vads, 300, True)
        ex.finish(handle)
        assert ex.stats.get("fallback_windows", 0) == 0 and not ex.demoted and ex.stats["probe_windows"] == 1


# ---------------------------------------------------------------------------------------------------------------------------------
# the command line: from audio against from tables
# ---------------------------------------------------------------------------------------------------------------------------------
def test_cli_from_audio_equals_cli_from_tables(tmp_path, caplog):
    import extract_embedding as ee
    import kaldi_io
    import mfcc_vad
    import models
    from xvector_amd import mfcc, synthetic
    topo = synthetic.SMALL_TOPOLOGY
    mdir = str(tmp_path / "nnet")
    models.Model.save_model(dict(weights=synthetic.trained_like(topo, F, num_classes=8, seed=12), topology=topo, model_class="Model",
                                 num_classes=8, feat_dim=F), mdir, None)
    rng = np.random.default_rng(31)
    loud = lambda sec: rng.integers(-3000, 3001, int(round(sec * 8000))).astype(np.int16)
    quiet = lambda sec: rng.integers(-3, 4, int(round(sec * 8000))).astype(np.int16)
    waves = [("a-2s", loud(2.0)), ("b-6s", np.concatenate([loud(2.5), quiet(1.5), loud(2.0)])), ("c-4s", loud(4.0))]
    lines = []
    for key, wave in waves:
        (tmp_path / (key + ".wav")).write_bytes(mfcc.wav_bytes(wave, 8000))
        lines.append("%s %s\n" % (key, tmp_path / (key + ".wav")))
    scp = tmp_path / "wav.scp"
    scp.write_text("".join(lines))
    conf, vconf = os.path.join(GOLDEN, "mfcc.conf"), os.path.join(GOLDEN, "vad.conf")
    common = ["--min-chunk-size", "25", "--model-dir", mdir, "--cmn-window", "300", "--window", "150", "--period", "75"]
    caplog.set_level(logging.INFO, logger="extract_embedding")
    a, b = tmp_path / "A", tmp_path / "B"
    a.mkdir(), b.mkdir()
    ee.main(common + ["--wav-rspecifier", "scp:%s" % scp, "--mfcc-config", conf, "--vad-config", vconf,
                      "--vector-wspecifier", "ark,scp:%s,%s" % (a / "xvector.ark", a / "xvector.scp"), "--subsegments-file", str(a / "S")])
    log_a = caplog.text
    assert mfcc_vad.main(["compute-mfcc-vad", "--config", conf, "--vad-config", vconf, "scp:%s" % scp,
                          "ark,scp:%s,%s" % (b / "feats.ark", b / "feats.scp"), "ark,scp:%s,%s" % (b / "vad.ark", b / "vad.scp")]) == 0
    ee.main(common + ["--feature-rspecifier", "scp:%s" % (b / "feats.scp"), "--vad-rspecifier", "scp:%s" % (b / "vad.scp"),
                      "--vector-wspecifier", "ark,scp:%s,%s" % (b / "xvector.ark", b / "xvector.scp"), "--subsegments-file", str(b / "S2")])
    ark_a, ark_b = (a / "xvector.ark").read_bytes(), (b / "xvector.ark").read_bytes()
    sub_a, sub_b = (a / "S").read_text(), (b / "S2").read_text()
    assert len(ark_a) > 1000 and ark_a == ark_b and sub_a == sub_b
    assert sorted(os.listdir(a)) == ["S", "xvector.ark", "xvector.scp"]                  # temporaries renamed into place
    keys = [ln.split()[0] for ln in open(a / "xvector.scp")]
    sub = [ln.split() for ln in sub_a.splitlines()]
    assert [s[0] for s in sub] == keys and len(keys) >= 8
    vad = dict(kaldi_io.read_vec_flt_scp(str(b / "vad.scp")))
    seen = {}
    for key, utt, t0, t1 in sub:
        head, first, end = key.rsplit("-", 2)
        assert head == utt and len(first) == len(end) == 8 and utt in vad
        first, end = int(first), int(end)
        assert (t0, t1) == ("%.3f" % (first * 0.01), "%.3f" % (end * 0.01))
        voiced = np.flatnonzero(vad[utt] != 0)
        i0, i1 = np.searchsorted(voiced, first), np.searchsorted(voiced, end - 1)
        assert voiced[i0] == first and voiced[i1] == end - 1 and 25 <= i1 - i0 + 1 <= 150      # a span of voiced frames, ends voiced
        seen.setdefault(utt, []).append(i0)
    assert list(seen) == ["a-2s", "b-6s", "c-4s"]
    for utt, firsts in seen.items():
        assert firsts == [75 * k for k in range(len(firsts))]                             # every 75 VOICED frames
    assert keys == sorted(keys)
    assert "Done 3 and failed 0; wrote %d sub-segment vectors" % len(keys) in log_a
