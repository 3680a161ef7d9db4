"""xv_vbx_groups_f64 on the device against tests/vbx_ref.py, the rule's generic log-domain restatement.

The bound is measured per input, not fixed: with d the largest |difference| between vbx_ref in float64 and in numpy.longdouble, the
kernel may differ from the float64 reference by at most 64 d + 1e-13 (vbx_ref.bound) in gamma, pi and, relatively, the ELBO.
Labels must be equal exactly, on inputs whose reference argmax margin is at least 0.5 (asserted on the reference).  Every call
here pads the rows with NaN columns (ldy > dim), fills the workspace with 0xFF bytes and the outputs with sentinels."""
import ctypes
import os

import numpy as np
import pytest

import diar_ref
import vbx_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = -12345.5
ISENT = -7
NEG_INF = -np.inf
ID = lambda c: "D%d-T%d-S%d" % (c[0], c[1], c[3])


def _call(recs, mdl, max_spk=None, max_iters=10, eps=NEG_INF, with_gamma=True, pad=3, spk=None, rot=False, **scal):
    """One xv_vbx_groups_f64 call on recs = [(y [T, D], labels [T], S, row_of_t or None)].  -> dict of host arrays, sentinels where
    the kernel wrote nothing."""
    import torch
    from xvector_amd import hiplib
    D = mdl[0].size
    sizes = [len(r[0]) for r in recs]
    N, G = sum(sizes), len(recs)
    spk = np.asarray([r[2] for r in recs] if spk is None else spk, np.int32)
    ms = int(max(r[2] for r in recs)) if max_spk is None else max_spk
    Y = np.full((N, D + pad), np.nan, np.float32)
    Y[:, :D] = np.concatenate([r[0] for r in recs])
    row0 = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    order = None
    if rot or any(r[3] is not None for r in recs):
        order = np.concatenate([np.arange(len(r[0])) if r[3] is None else r[3] for r in recs]).astype(np.int32)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device=DEV)
    out = dict(labels=full((N,), ISENT, torch.int32), gamma=full((N, ms), SENT, torch.float64) if with_gamma else None,
               pi=full((G, ms), SENT, torch.float64), elbo=full((G, max_iters), SENT, torch.float64),
               iters=full((G,), ISENT, torch.int32), info=full((G,), ISENT, torch.int32), status=full((1,), 0, torch.int32))
    ws = full((hiplib.vbx_groups_workspace_bytes(N, G, D, ms),), 0xFF, torch.uint8)
    p = dict(fa=0.3, fb=17.0, loop_prob=0.99, init_smoothing=5.0)
    p.update(scal)
    hiplib.vbx_groups(t(Y), t(row0), D, None if order is None else t(order), t(np.concatenate([r[1] for r in recs]).astype(np.int32)),
                      t(spk), ms, t(mdl[0]), t(mdl[1]), t(mdl[2]), p["fa"], p["fb"], p["loop_prob"], p["init_smoothing"], max_iters, eps,
                      out["labels"], out["gamma"], out["pi"], out["elbo"], out["iters"], out["info"], out["status"], ws)
    torch.cuda.synchronize()
    res = {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}
    res["row0"] = row0
    return res


def _group(res, g, S):
    """Group g's own outputs, and a check that nothing was written beside them."""
    r0, r1 = res["row0"][g], res["row0"][g + 1]
    it = int(res["iters"][g])
    assert np.all(res["pi"][g, S:] == SENT) and np.all(res["elbo"][g, it:] == SENT)
    if res["gamma"] is not None:
        assert np.all(res["gamma"][r0:r1, S:] == SENT)
    return dict(labels=res["labels"][r0:r1], gamma=None if res["gamma"] is None else res["gamma"][r0:r1, :S], pi=res["pi"][g, :S],
                elbo=res["elbo"][g, :it], iters=it, info=int(res["info"][g]))


def _within_bound(got, ref, d, what):
    dg, dp, de = d
    eg, ep = np.abs(got["gamma"] - ref["gamma"]).max(), np.abs(got["pi"] - ref["pi"]).max()
    ee = (np.abs(got["elbo"] - ref["elbo"]) / np.abs(ref["elbo"])).max()
    print("%s: gamma %.2e = %.1f d  pi %.2e = %.1f d  elbo %.2e = %.1f d" % (what, eg, eg / max(dg, 1e-300), ep, ep / max(dp, 1e-300),
                                                                             ee, ee / max(de, 1e-300)))
    assert eg <= vbx_ref.bound(dg), (what, "gamma", eg, dg)
    assert ep <= vbx_ref.bound(dp), (what, "pi", ep, dp)
    assert ee <= vbx_ref.bound(de), (what, "elbo", ee, de)


@pytest.mark.parametrize("case", vbx_ref.CASES, ids=ID)
@pytest.mark.parametrize("iters", [1, 3, 10])
def test_against_the_reference(case, iters):
    ref, d = vbx_ref.reference(case, iters, NEG_INF)
    assert ref["margin"] >= 0.5 and ref["iters"] == iters
    y, lab, S, mdl = vbx_ref.make(case)
    res = _call([(y, lab, S, None)], mdl, max_iters=iters)
    assert res["status"].tolist() == [0]
    got = _group(res, 0, S)
    assert got["info"] == 0 and got["iters"] == iters
    _within_bound(got, ref, d, "%s, %d iterations" % (ID(case), iters))
    assert np.array_equal(got["labels"], ref["labels"])


def test_time_order_table_and_no_gamma():
    """row_of_t a non-trivial permutation: the rows shuffled in memory, visited in time order -- the reference on the time-ordered
    rows, per-row outputs at the shuffled places, and the bits of the identity run.  gamma = NULL changes no other output."""
    case = vbx_ref.SPLIT_CASE
    ref, d = vbx_ref.reference(case, 10, NEG_INF)
    y, lab, S, mdl = vbx_ref.make(case)
    plain = _group(_call([(y, lab, S, None)], mdl), 0, S)
    perm = np.random.default_rng(5).permutation(len(y))              # row_of_t: the t-th vector in time lies at row perm[t]
    assert not np.array_equal(perm, np.arange(len(y)))
    ys, labs = np.empty_like(y), np.empty_like(lab)
    ys[perm], labs[perm] = y, lab
    got = _group(_call([(ys, labs, S, perm)], mdl), 0, S)
    timed = dict(got, gamma=got["gamma"][perm], labels=got["labels"][perm])
    _within_bound(timed, ref, d, "row_of_t")
    assert np.array_equal(timed["labels"], ref["labels"])
    for k in ("gamma", "labels", "pi", "elbo"):
        assert np.array_equal(timed[k], plain[k]), k
    lean = _group(_call([(ys, labs, S, perm)], mdl, with_gamma=False), 0, S)
    assert lean["gamma"] is None
    for k in ("labels", "pi", "elbo", "iters", "info"):
        assert np.array_equal(lean[k], got[k]), k


BATCH = ((60, 3, 4), (1, 1, 1), (17, 2, 17), (130, 4, 64), (33, 2, 2))       # (T, true speakers, S); 130 x 64 leaves LDS


def test_batch_independence():
    """Five recordings of mixed (T, S) in one call: each one's outputs are bit-identical run alone, with the batch reversed, and
    run twice."""
    mdl = vbx_ref.model(16, 3)
    recs = []
    for k, (T, nt, S) in enumerate(BATCH):
        y, lab, _ = vbx_ref.turns_case(16, T, nt, S, 40 + k, mdl=mdl)
        recs.append((y, lab, S, None))
    first = _call(recs, mdl, max_iters=6, eps=1e-6)
    again = _call(recs, mdl, max_iters=6, eps=1e-6)
    back = _call(recs[::-1], mdl, max_iters=6, eps=1e-6)
    assert first["status"].tolist() == again["status"].tolist() == back["status"].tolist() == [0]
    for g, r in enumerate(recs):
        a = _group(first, g, r[2])
        alone = _group(_call([r], mdl, max_iters=6, eps=1e-6), 0, r[2])
        assert a["info"] == 0 and a["iters"] >= 2
        for other, what in ((_group(again, g, r[2]), "twice"), (_group(back, len(recs) - 1 - g, r[2]), "reversed"), (alone, "alone")):
            for k in ("labels", "gamma", "pi", "elbo", "iters", "info"):
                assert np.array_equal(a[k], other[k]), (g, what, k)


@pytest.mark.parametrize("case", vbx_ref.CASES, ids=ID)
def test_stop_rule(case):
    ref, d = vbx_ref.reference(case, 40, 1e-6)
    steps = np.diff(ref["elbo"])
    assert not np.any((steps >= 1e-6 / 1.5) & (steps <= 1.5e-6))      # every step of the reference is clear of the threshold
    y, lab, S, mdl = vbx_ref.make(case)
    res = _call([(y, lab, S, None)], mdl, max_iters=40, eps=1e-6)
    got = _group(res, 0, S)                                           # ... which checks the sentinels past grp_iters
    assert got["iters"] == ref["iters"] < 40 and got["info"] == 0
    assert np.all(res["elbo"][0, got["iters"]:] == SENT) and np.all(res["elbo"][0, :got["iters"]] != SENT)
    _within_bound(got, ref, d, "%s, stopped after %d" % (ID(case), got["iters"]))


@pytest.mark.parametrize("broken", ["grp_spk = 65", "a label equal to S", "a row_of_t entry equal to n_g"])
def test_a_group_outside_the_contract_is_skipped(broken):
    mdl = vbx_ref.model(16, 3)
    recs = []
    for k, (T, nt, S) in enumerate(((20, 2, 3), (12, 2, 3), (9, 1, 2))):
        y, lab, _ = vbx_ref.turns_case(16, T, nt, S, 60 + k, mdl=mdl)
        recs.append([y, lab, S, None])
    clean = _call(recs, mdl, max_spk=64, max_iters=4, rot=True)
    spk = [r[2] for r in recs]
    if broken == "grp_spk = 65":
        spk[1] = 65
    elif broken == "a label equal to S":
        recs[1][1] = recs[1][1].copy()
        recs[1][1][5] = recs[1][2]
    else:
        recs[1][3] = np.arange(12)
        recs[1][3][4] = 12
    res = _call(recs, mdl, max_spk=64, max_iters=4, spk=spk, rot=True)
    assert res["status"].tolist() == [1] and clean["status"].tolist() == [0]
    r0, r1 = res["row0"][1], res["row0"][2]
    assert np.all(res["labels"][r0:r1] == ISENT) and np.all(res["gamma"][r0:r1] == SENT) and np.all(res["pi"][1] == SENT)
    assert np.all(res["elbo"][1] == SENT) and res["iters"][1] == ISENT and res["info"][1] == ISENT
    for g in (0, 2):
        a, b = _group(res, g, recs[g][2]), _group(clean, g, recs[g][2])
        for k in ("labels", "gamma", "pi", "elbo", "iters", "info"):
            assert np.array_equal(a[k], b[k]), (g, k)


def test_host_refusals():
    """Every refusal returns its code and launches nothing: the output sentinels stay."""
    import torch
    from xvector_amd import hiplib
    lib = hiplib.require_gpu()
    D, N, G, ms, mi = 16, 24, 2, 4, 5
    mdl = vbx_ref.model(D, 3)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device=DEV)
    y = t(np.zeros((N, D + 4), np.float32))
    ten = dict(y=y, grp_row0=t(np.asarray([0, 10, 24], np.int32)), row_of_t=t(np.concatenate([np.arange(10), np.arange(14)]).astype(np.int32)),
               init_label=t(np.zeros(N, np.int32)), grp_spk=t(np.asarray([2, 3], np.int32)), mean=t(mdl[0]), transform=t(mdl[1]),
               psi=t(mdl[2]), labels=full((N + 1,), ISENT, torch.int32), gamma=full((N * ms + 1,), SENT, torch.float64),
               pi=full((G * ms + 1,), SENT, torch.float64), elbo=full((G * mi + 1,), SENT, torch.float64),
               grp_iters=full((G + 1,), ISENT, torch.int32), grp_info=full((G + 1,), ISENT, torch.int32),
               status=full((2,), 0, torch.int32), ws=full((hiplib.vbx_groups_workspace_bytes(N, G, D, ms) + 8,), 0xFF, torch.uint8))
    val = dict(ldy=D + 4, n_rows=N, n_groups=G, dim=D, max_spk=ms, fa=0.3, fb=17.0, loop_prob=0.99, smooth=5.0, max_iters=mi, eps=1e-6,
               ws_bytes=hiplib.vbx_groups_workspace_bytes(N, G, D, ms))
    off = {}                                                         # byte offsets added to a pointer

    def call():
        p = lambda k: None if ten[k] is None else ctypes.c_void_p(ten[k].data_ptr() + off.get(k, 0))
        return lib.xv_vbx_groups_f64(p("y"), val["ldy"], val["n_rows"], p("grp_row0"), val["n_groups"], val["dim"], p("row_of_t"),
                                     p("init_label"), p("grp_spk"), val["max_spk"], p("mean"), p("transform"), p("psi"), val["fa"],
                                     val["fb"], val["loop_prob"], val["smooth"], val["max_iters"], val["eps"], p("labels"), p("gamma"),
                                     p("pi"), p("elbo"), p("grp_iters"), p("grp_info"), p("status"), p("ws"), val["ws_bytes"], None)

    BAD, UNSUP = -1, -2
    refused = [("n_rows", 0, BAD), ("n_groups", 0, BAD), ("dim", 0, BAD), ("dim", 129, UNSUP), ("ldy", D - 1, BAD), ("max_spk", 0, BAD),
               ("max_spk", 65, BAD), ("max_iters", 0, BAD), ("max_iters", 101, BAD), ("fa", 0.0, BAD), ("fa", np.nan, BAD),
               ("fa", np.inf, BAD), ("fb", -1.0, BAD), ("fb", np.nan, BAD), ("loop_prob", 1.0, BAD), ("loop_prob", -0.01, BAD),
               ("loop_prob", np.nan, BAD), ("smooth", -0.5, BAD), ("smooth", np.nan, BAD), ("eps", np.nan, BAD),
               ("ws_bytes", val["ws_bytes"] - 1, BAD)]
    for k, v, code in refused:
        keep = val[k]
        val[k] = v
        assert call() == code, (k, v)
        assert hiplib.load().xv_last_error()
        val[k] = keep
    for k in ten:
        if k in ("row_of_t", "gamma"):
            continue
        keep = ten[k]
        ten[k] = None
        assert call() == BAD, ("NULL", k)
        ten[k] = keep
    for k in ten:                                                    # 4 bytes off: misaligned for fp64; 2 bytes off: for the rest
        off[k] = 4 if ten[k].dtype in (torch.float64, torch.uint8) else 2
        assert call() == BAD, ("misaligned", k)
        del off[k]
    assert hiplib.vbx_groups_workspace_bytes(N, G, 129, ms) == 0 and hiplib.vbx_groups_workspace_bytes(N, G, D, 65) == 0
    torch.cuda.synchronize()
    for k in ("labels", "grp_iters", "grp_info"):
        assert bool((ten[k] == ISENT).all()), k
    for k in ("gamma", "pi", "elbo"):
        assert bool((ten[k] == SENT).all()), k
    assert ten["status"].tolist() == [0, 0]
    # and the same arguments, untouched, run: row_of_t and gamma may be NULL
    ten["row_of_t"] = ten["gamma"] = None
    assert call() == 0
    torch.cuda.synchronize()
    assert ten["status"].tolist() == [0, 0] and ten["grp_iters"].tolist()[:G] != [ISENT] * G and ten["grp_iters"].tolist()[G] == ISENT


def test_a_nan_row_gives_info_2_and_the_initial_labels():
    """Data handling, not a fault: the call returns, the recording reports info 2 and keeps its initial labels; its neighbour in
    the batch is untouched by it."""
    case = vbx_ref.SPLIT_CASE
    y, lab, S, mdl = vbx_ref.make(case)
    bad = y.copy()
    bad[7, 2] = np.nan
    res = _call([(bad, lab, S, None), (y, lab, S, None)], mdl, max_iters=5)
    assert res["status"].tolist() == [0] and res["info"].tolist() == [2, 0]
    assert np.array_equal(res["labels"][:len(y)], lab) and 1 <= res["iters"][0] <= 5
    alone = _group(_call([(y, lab, S, None)], mdl, max_iters=5), 0, S)
    r0 = len(y)
    assert np.array_equal(res["labels"][r0:], alone["labels"]) and np.array_equal(res["gamma"][r0:, :S], alone["gamma"])


def test_backend_route_cuts_calls_and_agrees_with_the_host_twin():
    """backend.vbx_groups on a batch, cut into several calls by max_bytes: the results of the uncut call bit for bit, and the host
    twin's within the bound."""
    import torch
    from xvector_amd import backend, hiplib
    mdl = vbx_ref.model(16, 3)
    plda = backend.Plda(*mdl)
    ys, labs, spk = [], [], []
    for k, (T, nt, S) in enumerate(BATCH):
        y, lab, _ = vbx_ref.turns_case(16, T, nt, S, 40 + k, mdl=mdl)
        ys.append(y); labs.append(lab); spk.append(S)
    sizes = [len(y) for y in ys]
    Y = torch.as_tensor(np.concatenate(ys), device=DEV)
    orders = np.concatenate([np.random.default_rng(g).permutation(n) for g, n in enumerate(sizes)])
    one = backend.vbx_groups(Y, backend.GroupTables(sizes, DEV), np.concatenate(labs), plda, orders, spk, keep_gamma=True)
    cut = backend.vbx_groups(Y, backend.GroupTables(sizes, DEV), np.concatenate(labs), plda, orders, spk, keep_gamma=True,
                             max_bytes=hiplib.vbx_groups_workspace_bytes(130, 1, 16, 64))
    assert len(backend.plan_vbx_groups(backend.GroupTables(sizes).row0, 16, 64, hiplib.vbx_groups_workspace_bytes(130, 1, 16, 64))) > 1
    for k in one:
        assert np.array_equal(one[k], cut[k], equal_nan=True), k
    row0 = np.concatenate([[0], np.cumsum(sizes)])
    for g, S in enumerate(spk):
        o = orders[row0[g]:row0[g + 1]]
        host = backend.vbx_host(ys[g][o], labs[g][o], plda, S)
        ref = vbx_ref.vbx_ref(ys[g][o], labs[g][o], S, *mdl)
        dg = vbx_ref.ref_distance(ref, vbx_ref.vbx_ref(ys[g][o], labs[g][o], S, *mdl, dtype=np.longdouble))[0]
        assert one["iters"][g] == host["iters"] == ref["iters"] and one["info"][g] == 0 and ref["margin"] >= 0.5
        gam = one["gamma"][row0[g]:row0[g + 1], :S][o]
        assert np.abs(gam - ref["gamma"]).max() <= vbx_ref.bound(dg) and np.abs(host["gamma"] - ref["gamma"]).max() <= vbx_ref.bound(dg)
        assert np.array_equal(one["labels"][row0[g]:row0[g + 1]][o], ref["labels"])
        assert np.all(np.isnan(one["elbo"][g, host["iters"]:])) and not np.any(np.isnan(one["elbo"][g, :host["iters"]]))


E2E_THRESHOLD = 12.0            # over-splits the second recording (4 clusters for 2 speakers) under the model below
E2E_RECS = ((60, 3, 11), (45, 2, 12), (70, 4, 13))                  # (rows, speakers, seed)


def test_cli_end_to_end(tmp_path, caplog):
    """`plda_backend.py diarize --vbx --rttm` on three recordings of known turns, the second over-split by the threshold and
    listed out of time order in the segments file: the labels of tests/diar_ref.py's clustering (on the device's own scores)
    followed by vbx_ref on the time-ordered rows; the RTTM parses; without --vbx the files of the route without VBx."""
    import kaldi_io
    import plda_backend
    from xvector_amd import backend
    p = str(tmp_path)
    D = 16
    mdl = vbx_ref.model(D, 7)
    plda = backend.Plda(*mdl)
    xs, truth = [], []
    for T, nt, seed in E2E_RECS:
        y, _, who = vbx_ref.turns_case(D, T, nt, nt, seed, mdl=mdl, split=False, wrong=0)
        xs.append(y); truth.append(who)
    sizes = [len(x) for x in xs]
    G = len(sizes)
    # file order within a recording: in time, except the second recording, which is listed backwards
    file_rows = [np.arange(n) if g != 1 else np.arange(n)[::-1] for g, n in enumerate(sizes)]
    keys, seg_lines, vecs = [], [], []
    for g in range(G):
        for j in file_rows[g]:                                       # j: the position in time
            keys.append("reco%d-%04d" % (g, j))
            seg_lines.append("%s reco%d %.2f %.2f" % (keys[-1], g, 0.75 * j, 0.75 * j + 1.5))
            vecs.append(xs[g][j])
    open(p + "/segments", "w").write("\n".join(seg_lines) + "\n")
    with kaldi_io.TableWriter(p + "/xvector.ark", p + "/xvector.scp") as w:
        kaldi_io.write_vec_flt_batch(w, keys, vecs)
    backend.write_plda(p + "/plda", plda)
    tail = ["--threshold", str(E2E_THRESHOLD), p + "/plda", "scp:" + p + "/xvector.scp", p + "/segments"]
    with caplog.at_level("INFO", logger="plda_backend"):
        plda_backend.main(["diarize", "--vbx", "--rttm", p + "/vbx.rttm"] + tail + [p + "/vbx.labels"])
    plda_backend.main(["diarize", "--rttm", p + "/ahc.rttm"] + tail + [p + "/ahc.labels"])
    # the reference: the clustering on the device's own scores, in file order ...
    x_file = np.stack(vecs)
    model_read = backend.read_plda(p + "/plda")                      # what the command saw (the file holds float32)
    scores, _ = backend.score_blocks(x_file, sizes, model_read)
    clustered = diar_ref.cluster_groups(diar_ref.blocks(scores.cpu().numpy(), sizes), [E2E_THRESHOLD] * G, [1] * G)
    plain = backend.prepare(x_file, 0, None, None, None, None, False)[0].cpu().numpy()[:, :D]
    row0 = np.concatenate([[0], np.cumsum(sizes)])
    want_ahc, want_vbx, n_before, n_after = {}, {}, 0, 0
    recos_ahc, recos_vbx = [], []
    for g in range(G):
        slots = clustered[g][0]
        init, S = backend.compact_labels(slots)
        in_time = np.argsort(file_rows[g], kind="stable")            # file positions in (start, end, key) order
        ref = vbx_ref.vbx_ref(plain[row0[g]:row0[g + 1]][in_time], init[in_time], S, model_read.mean, model_read.transform,
                              model_read.psi)
        assert ref["margin"] >= 0.5
        after = np.empty(sizes[g], np.int32)
        after[in_time] = ref["labels"]
        n_before += S
        n_after += np.unique(after).size
        for want, recos, lab in ((want_ahc, recos_ahc, slots), (want_vbx, recos_vbx, after)):
            numbered = diar_ref.number_labels(lab)
            segs = []
            for i, l in enumerate(numbered):
                k = keys[row0[g] + i]
                want[k] = l
                j = file_rows[g][i]
                segs.append((diar_ref.to_ms("%.2f" % (0.75 * j)), diar_ref.to_ms("%.2f" % (0.75 * j + 1.5)), k, l))
            recos.append(("reco%d" % g, segs))
        if g == 1:
            assert S > 2 and np.unique(after).size == 2               # over-split by the threshold, mended by VBx
        assert np.array_equal(np.unique(after[in_time], return_inverse=True)[1], truth[g])
    assert open(p + "/vbx.labels").read() == "".join("%s %d\n" % (k, want_vbx[k]) for k in keys)
    assert open(p + "/ahc.labels").read() == "".join("%s %d\n" % (k, want_ahc[k]) for k in keys)
    assert open(p + "/vbx.rttm").read() == diar_ref.rttm(recos_vbx, 0)
    assert open(p + "/ahc.rttm").read() == diar_ref.rttm(recos_ahc, 0)
    for line in open(p + "/vbx.rttm"):                               # the RTTM parses
        f = line.split()
        assert len(f) == 10 and f[0] == "SPEAKER" and f[1] in ("reco0", "reco1", "reco2") and float(f[3]) >= 0 and float(f[4]) > 0
        assert int(f[7]) >= 1
    assert "VBx resegmentation: 3 recordings" in caplog.text and "%d speakers before and %d after" % (n_before, n_after) in caplog.text
    assert not os.path.exists(p + "/vbx.labels.tmp")


@pytest.mark.parametrize("target_energy", [1.0, 0.5])
def test_diarize_equals_its_stages(target_energy):
    """backend.diarize with VBx (and, at 0.5, the per-recording PCA) against its stages composed by hand, byte for byte: four
    recordings out of size order, the third told to stop at 70 clusters (above hiplib.VBX_MAX_SPK: it keeps its clustering), the
    second kept by the caller, every recording's rows in a shuffled time order.  Here VBx runs on one recording at a time, from the
    caller's side of the size order; the kernel's results do not depend on the batch (test_batch_independence)."""
    import torch
    from xvector_amd import backend, hiplib
    D, sizes = 16, [40, 9, 70, 25]
    mdl = vbx_ref.model(D, 7)
    plda = backend.Plda(*mdl)
    x = np.concatenate([vbx_ref.turns_case(D, T, nt, nt, 20 + g, mdl=mdl, split=False, wrong=0)[0]
                        for g, (T, nt) in enumerate(zip(sizes, (3, 2, 4, 2)))])
    G, row0 = len(sizes), np.concatenate([[0], np.cumsum(sizes)])
    keep = [False, True, False, False]
    time_order = np.concatenate([np.random.default_rng(g).permutation(n) for g, n in enumerate(sizes)])
    rep, pr = {}, {}
    labels, merges = backend.diarize(x, sizes, plda, threshold=E2E_THRESHOLD, num_spk=[None, None, 70, None], device=DEV,
                                     target_energy=target_energy, pca_report=pr, vbx=dict(time_order=time_order, keep=keep),
                                     vbx_report=rep)
    # by hand: sort by size, score, cluster ...
    order, inverse = backend.size_order(sizes)
    assert order.tolist() == [2, 0, 3, 1]
    rows = np.concatenate([np.arange(row0[g], row0[g + 1]) for g in order])
    thr, minc = np.asarray([E2E_THRESHOLD, E2E_THRESHOLD, NEG_INF, E2E_THRESHOLD]), np.asarray([1, 1, 70, 1])
    scores, tables = backend.score_blocks(x[rows], np.asarray(sizes)[order], plda, None, None, DEV, target_energy, keep_plain=True)
    lab_sorted, merges_sorted = backend.ahc_batch(scores, tables, thr[order], minc[order])
    want, ran = [], []
    for g in range(G):                                               # ... and VBx, recording by recording in the caller's order
        k = int(inverse[g])
        lab = lab_sorted[k]
        init, S = backend.compact_labels(lab)
        ran.append(not keep[g] and S <= hiplib.VBX_MAX_SPK)
        if ran[-1]:
            Y = tables.plain[int(tables.row0[k]):int(tables.row0[k + 1])].clone()
            res = backend.vbx_groups(Y, backend.GroupTables([sizes[g]], DEV), init, plda, time_order[row0[g]:row0[g + 1]], [S])
            if res["info"][0] == 0:
                lab = res["labels"]
        want.append(lab)
        for a, b in zip(merges[g], merges_sorted[k]):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), g
    want = np.concatenate(want)
    assert labels.dtype == want.dtype == np.int32 and labels.tobytes() == want.tobytes()
    assert ran == [True, False, False, True] and rep["ran"].tolist() == [True, False, False, True]
    assert rep["spk_before"][2] == 70 and np.unique(labels[row0[2]:row0[3]]).size == 70
    if target_energy == 1.0:
        assert pr == {}
    else:
        assert sorted(pr) == ["dim", "info"] and pr["dim"].shape == pr["info"].shape == (G,)
        assert np.array_equal(pr["dim"][order], tables.pca[:G].cpu().numpy()) and np.array_equal(pr["info"][order], tables.pca[G:].cpu().numpy())
