"""The scoring back-end on the MI355X: prepare against the float64 reference, the dense scorer within the fp32 summation bound,
the trial scorer bit for bit equal to the dense one, the plda_backend.py CLI end to end, and the four extraction arithmetics
compared on the task (PLDA scores and EER)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import backend_ref as ref
from conftest import ROOT, TWIN

pytestmark = pytest.mark.gpu


def _rand_plda(rng, d):
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    P = q * rng.uniform(0.5, 2.0, d)[None, :]
    psi = np.sort(rng.uniform(0.05, 5.0, d))[::-1]
    return rng.standard_normal(d) * 0.3, P, psi


def _rel_rows(got, want):
    return np.linalg.norm(got - want, axis=1) / np.maximum(np.linalg.norm(want, axis=1), 1e-30)


@pytest.mark.parametrize("N", [1, 31, 1000, 4099])
@pytest.mark.parametrize("D,d", [(64, 1), (64, 50), (64, 64), (512, 1), (512, 50), (512, 100), (512, 200), (512, 256)])
def test_prepare_matches_reference(N, D, d):
    from xvector_amd import backend, hiplib
    rng = np.random.default_rng(N * 7919 + D * 31 + d)
    x = (rng.standard_normal((N, D)) + 0.5).astype(np.float32)
    mean = (rng.standard_normal(D) * 0.1).astype(np.float32)
    transform = (rng.standard_normal((d, D + 1)) / np.sqrt(D)).astype(np.float32)
    m, P, psi = _rand_plda(rng, d)
    plda = backend.Plda(m.astype(np.float32), P.astype(np.float32), psi.astype(np.float32))
    pl = (plda.mean, plda.transform, plda.psi)
    counts = rng.integers(1, 12, N).astype(np.int32)
    z_enrol = ref.chain(x, mean, transform, True, pl, counts)
    z_test = ref.chain(x, mean, transform, True, pl, None)
    want_e, want_r = ref.side_rows_enrol(z_enrol, counts, plda.psi)
    for side, want, r_want, cnt in ((hiplib.SIDE_ENROL, want_e, want_r, counts), (hiplib.SIDE_TEST, ref.side_rows_test(z_test), None, None),
                                    (hiplib.SIDE_COSINE, ref.side_rows_cosine(z_test), None, None)):
        rows, r = backend.prepare(x, side, cnt, mean, transform, plda)
        rows, r = rows.cpu().numpy(), r.cpu().numpy()
        K = want.shape[1]
        assert rows.shape[1] % hiplib.BACKEND_KSTEP == 0 and np.all(rows[:, K:] == 0)
        rel = _rel_rows(rows[:, :K].astype(np.float64), want)
        assert rel.max() <= 1e-5, (side, rel.max())
        if r_want is not None:
            bound = 1e-5 * (np.abs(want_r) + np.sum(np.abs(want_e[:, :d] * z_enrol), axis=1) + d)
            assert np.all(np.abs(r - r_want) <= bound), (np.abs(r - r_want) / bound).max()
        else:
            assert np.all(r == 0)
    # no PLDA: LDA + length norm only (what compute-plda --lda and the cosine mode without a PLDA use)
    rows, _ = backend.prepare(x, hiplib.SIDE_PLAIN, None, mean, transform, None)
    rel = _rel_rows(rows.cpu().numpy()[:, :d].astype(np.float64), ref.chain(x, mean, transform, True))
    assert rel.max() <= 1e-5, rel.max()


def _operands(rng, n, K):
    kp = (K + 7) // 8 * 8
    a = np.zeros((n, kp), np.float32)
    a[:, :K] = rng.standard_normal((n, K)).astype(np.float32)
    return a


@pytest.mark.parametrize("K", [2, 100, 200, 400, 1024])
def test_score_matrix_within_fp32_bound(K):
    import torch
    from xvector_amd import hiplib
    rng = np.random.default_rng(K)
    for ne in (1, 17, 33, 257, 1000):
        for nt in (1, 31, 129, 2049):
            E, T = _operands(rng, ne, K), _operands(rng, nt, K)
            r = rng.standard_normal(ne).astype(np.float32) * 10
            s = torch.empty((ne, nt), dtype=torch.float32, device="cuda:0")
            hiplib.score_matrix(torch.from_numpy(E).cuda(), torch.from_numpy(T).cuda(), torch.from_numpy(r).cuda(), s)
            got = s.cpu().numpy().astype(np.float64)
            E64, T64 = E.astype(np.float64), T.astype(np.float64)
            want = E64 @ T64.T + r[:, None]
            bound = 4 * K * 2.0 ** -24 * (np.abs(r)[:, None] + np.abs(E64) @ np.abs(T64).T)
            assert np.all(np.abs(got - want) <= bound), (ne, nt, K, (np.abs(got - want) / bound).max())


def test_score_pairs_bit_identical_to_matrix():
    import torch
    from xvector_amd import hiplib
    rng = np.random.default_rng(5)
    for ne, nt, K in ((1, 1, 8), (37, 211, 200), (300, 1500, 400), (5, 9, 1024)):
        E = torch.from_numpy(_operands(rng, ne, K)).cuda()
        T = torch.from_numpy(_operands(rng, nt, K)).cuda()
        r = torch.from_numpy(rng.standard_normal(ne).astype(np.float32)).cuda()
        s = torch.empty((ne, nt), dtype=torch.float32, device="cuda:0")
        hiplib.score_matrix(E, T, r, s)
        s = s.cpu().numpy()
        m = 50000
        ei = rng.integers(0, ne, m).astype(np.int32)                 # random order, with repeats
        ti = rng.integers(0, nt, m).astype(np.int32)
        out = torch.empty(m, dtype=torch.float32, device="cuda:0")
        hiplib.score_pairs(E, T, r, torch.from_numpy(ei).cuda(), torch.from_numpy(ti).cuda(), out)
        got = out.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), s[ei, ti].view(np.uint32)), (ne, nt, K, np.abs(got - s[ei, ti]).max())


def test_score_pairs_independent_of_the_list():
    import torch
    from xvector_amd import backend
    rng = np.random.default_rng(11)
    ne, nt, K = 800, 9300, 200
    sc = backend.Scorer.__new__(backend.Scorer)
    sc.device = "cuda:0"
    sc.E = torch.from_numpy(_operands(rng, ne, K)).cuda()
    sc.T = torch.from_numpy(_operands(rng, nt, K)).cuda()
    sc.r = torch.from_numpy(rng.standard_normal(ne).astype(np.float32)).cuda()
    m = 1 << 20
    ei = rng.integers(0, ne, m)
    ti = rng.integers(0, nt, m)
    big = sc.score_pairs(ei, ti).cpu().numpy()
    for j in (0, 12345, m - 1):
        alone = sc.score_pairs(ei[j:j + 1], ti[j:j + 1]).cpu().numpy()
        assert alone.view(np.uint32)[0] == big.view(np.uint32)[j]
    # and whichever way score_trials goes (dense-then-gather or pairs), the same bits
    assert sc.use_dense(m) and not sc.use_dense(4000)
    assert np.array_equal(sc.score_trials(ei, ti).view(np.uint32), big.view(np.uint32))
    dense = sc.score_matrix().cpu().numpy()[ei[:4000], ti[:4000]]
    assert np.array_equal(sc.score_trials(ei[:4000], ti[:4000]).view(np.uint32), dense.view(np.uint32))


# ------------------------------------------------------------------------------------------------
# CLI end to end
# ------------------------------------------------------------------------------------------------
def _plda_data(rng, n_spk, D, n_range, spread=1.0):
    B = np.diag(rng.uniform(0.5, 3.0, D) * spread)
    A = rng.standard_normal((D, D)) / np.sqrt(D)
    W = A @ A.T + 0.3 * np.eye(D)
    mu = rng.standard_normal(D)
    spk = rng.multivariate_normal(np.zeros(D), B, n_spk) + mu
    labels, xs = [], []
    for s in range(n_spk):
        n = int(rng.integers(n_range[0], n_range[1] + 1))
        xs.append(spk[s] + rng.multivariate_normal(np.zeros(D), W, n))
        labels += [s] * n
    return np.vstack(xs).astype(np.float32), np.array(labels)


def _run(args, **kw):
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "x-vector-kaldi-tf_amd"), TWIN] + [env.get("PYTHONPATH", "")])
    return subprocess.run([sys.executable] + args, env=env, check=True, capture_output=True, text=True, timeout=600, **kw)


def test_score_cli_end_to_end(tmp_path):
    import kaldi_io
    from xvector_amd import backend
    rng = np.random.default_rng(3)
    D, dim = 64, 20
    x, lab = _plda_data(rng, 150, D, (3, 8))
    utts = ["spk%03d-u%03d" % (l, i) for i, l in enumerate(lab)]
    train = lab < 100
    p = str(tmp_path)
    with kaldi_io.TableWriter(p + "/train.ark", p + "/train.scp") as w:
        kaldi_io.write_vec_flt_batch(w, [u for u, t in zip(utts, train) if t], list(x[train]))
    with open(p + "/utt2spk", "w") as f:
        f.writelines("%s spk%03d\n" % (u, l) for u, l, t in zip(utts, lab, train) if t)
    spk2utt = {}
    for u, l, t in zip(utts, lab, train):
        if t:
            spk2utt.setdefault("spk%03d" % l, []).append(u)
    with open(p + "/spk2utt", "w") as f:
        f.writelines("%s %s\n" % (s, " ".join(us)) for s, us in spk2utt.items())
    cli = os.path.join(TWIN, "plda_backend.py")
    _run([cli, "mean", "scp:" + p + "/train.scp", p + "/mean.vec"])
    _run([cli, "compute-lda", "--dim", str(dim), "scp:" + p + "/train.scp", p + "/utt2spk", p + "/transform.mat"])
    _run([cli, "compute-plda", "--lda", p + "/transform.mat", p + "/spk2utt", "scp:" + p + "/train.scp", p + "/plda"])
    # evaluation: speakers 100..149 enrol their first 3 utterances, the rest are tests
    enrol_map, tests = {}, []
    for u, l in zip(utts, lab):
        if l >= 100:
            s = "spk%03d" % l
            if len(enrol_map.setdefault(s, [])) < 3:
                enrol_map[s].append(u)
            else:
                tests.append(u)
    ev = [i for i, l in enumerate(lab) if l >= 100]
    with kaldi_io.TableWriter(p + "/eval.ark", p + "/eval.scp") as w:
        kaldi_io.write_vec_flt_batch(w, [utts[i] for i in ev], list(x[ev]))
    with open(p + "/enrol_spk2utt", "w") as f:
        f.writelines("%s %s\n" % (s, " ".join(us)) for s, us in enrol_map.items())
    _run([os.path.join(TWIN, "speaker_mean.py"), p + "/enrol_spk2utt", p + "/eval.scp", p + "/spk.ark", p + "/spk.scp",
          p + "/num_utts.ark"])
    trials = [(s, t, "target" if t.startswith(s) else "nontarget") for s in enrol_map for t in tests]
    with open(p + "/trials", "w") as f:
        f.writelines("%s %s %s\n" % tr for tr in trials)
        f.write("spk999 %s nontarget\n" % tests[0])                 # missing enrolment key
        f.write("%s nosuchutt target\n" % trials[0][0])              # missing test key
    res = _run([cli, "score", "--num-utts=ark:" + p + "/num_utts.ark", "--mean", p + "/mean.vec", "--lda", p + "/transform.mat",
                p + "/plda", "scp:" + p + "/spk.scp", "scp:" + p + "/eval.scp", p + "/trials", p + "/scores"])
    assert "Key spk999 not present in training iVectors" in res.stderr and "Key nosuchutt not present in test iVectors" in res.stderr
    assert "2 had errors" in res.stderr
    lines = open(p + "/scores").read().splitlines()
    assert len(lines) == len(trials)
    got = {}
    for l, tr in zip(lines, trials):
        a, b, s = l.split()
        assert (a, b) == tr[:2]
        got[(a, b)] = float(s)
    # fp64 pipeline on the same files
    plda = backend.read_plda(p + "/plda")
    t = backend.read_transform(p + "/transform.mat")
    mean = kaldi_io.read_vec_flt(p + "/mean.vec")
    spk = dict(kaldi_io.read_vec_flt_scp(p + "/spk.scp"))
    ev_vec = dict(kaldi_io.read_vec_flt_scp(p + "/eval.scp"))
    nu = {l.split()[0]: int(l.split()[1]) for l in open(p + "/num_utts.ark")}
    pl = (plda.mean, plda.transform, plda.psi)
    worst = 0.0
    for s in enrol_map:
        z = ref.chain(spk[s][None], mean, t, True, pl, [nu[s]])[0]
        tz = ref.chain(np.stack([ev_vec[u] for u in tests]), mean, t, True, pl, None)
        for j, u in enumerate(tests):
            worst = max(worst, abs(got[(s, u)] - ref.llr(z, nu[s], tz[j], plda.psi)))
    print("score CLI vs fp64 pipeline: max |diff| = %.3e" % worst)
    assert worst <= 1e-3
    with open(p + "/eer_in", "w") as f:
        f.writelines("%s %s\n" % (l.split()[2], tr[2]) for l, tr in zip(lines, trials))
    eer = float(_run([cli, "compute-eer", p + "/eer_in"]).stdout.strip())
    print("CLI EER %.2f %%" % eer)
    assert 0.0 <= eer < 25.0


# ------------------------------------------------------------------------------------------------
# the four extraction arithmetics, compared on the task
# ------------------------------------------------------------------------------------------------
def test_arithmetics_on_the_task(default_weights):
    from xvector_amd import backend, engine, synthetic
    topo, w = default_weights
    mats, labels = [], []
    for xb, lab in synthetic.speaker_minibatches(24, n_spk=200, batch=64, tmin=200, tmax=400, seed=17):
        mats += [m.astype(np.float32) for m in xb]
        labels += lab.tolist()
    labels = np.array(labels)
    vecs = {}
    for precision in ("f16bf8", "bf16x3", "fp32", "fp32tc"):
        model = engine.select_model(w, topo, "cuda:0", precision=precision)
        assert model.selection["selected"] == precision, model.selection
        vecs[precision] = np.stack(engine.Extractor(model, 25, 200).extract(mats)).astype(np.float32)
    train = labels < 120
    x32 = vecs["fp32"]
    xt = x32[train]
    mean = xt.astype(np.float64).mean(axis=0)
    lda = backend.fit_lda(xt - mean, labels[train], 50)
    rows, _ = backend.prepare(xt, 0, mean=mean.astype(np.float32), transform=lda)
    groups = [np.flatnonzero(labels[train] == s) for s in np.unique(labels[train])]
    plda = backend.fit_plda(rows[:, :50].cpu().numpy(), groups)
    # evaluation speakers 120..199 with >= 4 utterances: the first 3 enrol, the rest test
    enrol_idx, test_idx, test_spk, spks = [], [], [], []
    for s in range(120, 200):
        u = np.flatnonzero(labels == s)
        if len(u) >= 4:
            spks.append(s)
            enrol_idx.append(u[:3])
            test_idx += u[3:].tolist()
            test_spk += [s] * (len(u) - 3)
    test_spk = np.array(test_spk)
    ei, ti = np.meshgrid(np.arange(len(spks)), np.arange(len(test_idx)), indexing="ij")
    target = np.array(spks)[ei.ravel()] == test_spk[ti.ravel()]
    scores, eers = {}, {}
    for precision, v in vecs.items():
        enrol = np.stack([v[i].astype(np.float64).mean(axis=0) for i in enrol_idx]).astype(np.float32)
        sc = backend.Scorer(enrol, v[test_idx], plda, np.full(len(spks), 3, np.int32), mean.astype(np.float32), lda)
        scores[precision] = sc.score_trials(ei.ravel(), ti.ravel()).astype(np.float64)
        eers[precision] = backend.eer(scores[precision][target], scores[precision][~target])[0]
    sd = scores["fp32"].std()
    n_tgt, n_non = int(target.sum()), int((~target).sum())
    report = {p: (np.abs(scores[p] - scores["fp32"]).max() / sd, 100 * eers[p]) for p in scores}
    for p, (dev, e) in report.items():
        print("arithmetic %-7s max|score - score_fp32| / std = %.3e   EER %.3f %%" % (p, dev, e))
    print("trials: %d target, %d nontarget" % (n_tgt, n_non))
    for p, (dev, e) in report.items():
        assert dev <= 1e-3, (p, dev)
        assert abs(eers[p] - eers["fp32"]) <= 1.0 / n_tgt + 1e-12, (p, eers[p], eers["fp32"])
    assert eers["fp32"] < 0.25, eers["fp32"]
