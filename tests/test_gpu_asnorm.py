"""AS-norm on the MI355X: the top-N row statistics kernel against float64 with padding and output poisoning,
its NaN and argument policy, its independence of the launch and the chunking, the Scorer's normalised scores against a float64
pipeline (PLDA and cosine), and the score CLI with --cohort."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import asnorm_ref
import backend_ref as ref
from conftest import ROOT, TWIN

pytestmark = pytest.mark.gpu


def _stats(x, top_n, ld=None, extra_out=5):
    """Run xv_topk_row_stats_f32 on the rows x[R, C] (stored at row stride ld, NaN in the padding) into NaN-poisoned outputs
    longer than R.  -> (mean[R], std[R]) as NumPy, after checking the tail stayed NaN."""
    import torch
    from xvector_amd import hiplib
    R, C = x.shape
    ld = ld or (C + 3) // 4 * 4
    buf = torch.full((R, ld), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :C] = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    mean = torch.full((R + extra_out,), float("nan"), dtype=torch.float32, device="cuda")
    std = torch.full((R + extra_out,), float("nan"), dtype=torch.float32, device="cuda")
    hiplib.topk_row_stats(buf[:, :C], top_n, mean, std)
    mean, std = mean.cpu().numpy(), std.cpu().numpy()
    assert np.all(np.isnan(mean[R:])) and np.all(np.isnan(std[R:]))
    return mean[:R], std[:R]


def _rows(rng, n_cols):
    """Test rows: mixed signs at several scales (up to 1e30, where fp32 sums of squares overflow), rows with +-0.0, rows of 3
    distinct values (a tie at the threshold)."""
    n_rows = 8 if n_cols < 100000 else 4
    rows = []
    for i in range(n_rows):
        kind = i % 4
        if kind == 0:
            r = rng.standard_normal(n_cols) * 10.0 ** rng.uniform(-3, 3)
        elif kind == 1:
            r = rng.standard_normal(n_cols) * 1e30
        elif kind == 2:
            r = rng.choice(np.array([-2.5, 0.75, 3.0]), n_cols)
        else:
            r = rng.standard_normal(n_cols)
            r[rng.random(n_cols) < 0.3] = 0.0
            r[rng.random(n_cols) < 0.3] = -0.0
        rows.append(r.astype(np.float32))
    return np.stack(rows)


@pytest.mark.parametrize("n_cols", [1, 2, 7, 300, 301, 4099, 32767, 32768, 32769, 200003])
def test_topk_stats_match_fp64(n_cols):
    rng = np.random.default_rng(n_cols)
    x = _rows(rng, n_cols)
    ld = (n_cols + 3) // 4 * 4 + 4                               # padding columns hold NaN
    for top_n in sorted({n for n in (1, 2, 300, n_cols) if n <= n_cols}):
        mu, sd = _stats(x, top_n, ld)
        x64 = np.sort(x.astype(np.float64), axis=1)[:, -top_n:]
        mu_ref, sd_ref = x64.mean(axis=1), x64.std(axis=1, ddof=0)
        scale = 1e-12 * np.abs(x64).mean(axis=1)
        for got, want in ((mu, mu_ref), (sd, sd_ref)):
            err = np.abs(got.astype(np.float64) - want)
            bound = 2.0 ** -23 * np.abs(want) + scale
            assert np.all(err <= bound), (n_cols, top_n, (err / np.maximum(bound, 1e-300)).max())


def test_nan_rows_and_bad_arguments():
    import torch
    from xvector_amd import hiplib
    rng = np.random.default_rng(5)
    x = rng.standard_normal((5, 1000)).astype(np.float32)
    x[1, 17] = np.float32(np.nan)
    x[3, 500] = np.array([0xFFC00000], np.uint32).view(np.float32)[0]       # a NaN with the sign bit set
    assert np.signbit(x[3, 500]) and np.isnan(x[3, 500])
    for top_n in (1, 10, 1000):
        mu, sd = _stats(x, top_n)
        assert np.all(np.isnan(mu[[1, 3]])) and np.all(np.isnan(sd[[1, 3]]))
        want_mu, want_sd = asnorm_ref.topn_stats(x[[0, 2, 4]], top_n)
        assert np.allclose(mu[[0, 2, 4]], want_mu, rtol=2e-7, atol=1e-12) and np.allclose(sd[[0, 2, 4]], want_sd, rtol=2e-7, atol=1e-12)
    lib = hiplib.require_gpu()
    buf = torch.zeros((4, 64), dtype=torch.float32, device="cuda")
    out = torch.full((8,), float("nan"), dtype=torch.float32, device="cuda")
    p, m, s = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(out.data_ptr() + 16)
    st = hiplib._stream()
    for ld, n_rows, n_cols, top_n, ptr in ((64, 4, 64, 0, p),                # top_n = 0
                                           (64, 4, 64, 65, p),               # top_n > n_cols
                                           (60, 4, 64, 8, p),                # ld < n_cols
                                           (62, 4, 60, 8, p),                # ld not a multiple of 4
                                           (64, 3, 60, 8, ctypes.c_void_p(buf.data_ptr() + 4))):   # base not 16-B aligned
        assert lib.xv_topk_row_stats_f32(ptr, ld, n_rows, n_cols, top_n, m, s, st) == -1     # XV_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


@pytest.mark.parametrize("n_cols", [2001, 50000])
def test_topk_stats_independent_of_the_launch(n_cols):
    rng = np.random.default_rng(n_cols)
    x = (rng.standard_normal((1000, n_cols)) * 3.0).astype(np.float32)
    top_n = 300
    full = _stats(x, top_n)
    again = _stats(x, top_n)
    wide = _stats(x[:50], top_n, ld=n_cols + (-n_cols) % 4 + 64)
    bits = lambda a: a.view(np.int32)
    for i in (0, 1, 37, 999):
        alone = _stats(x[i:i + 1], top_n)
        for a, b in zip(alone, full):
            assert bits(a)[0] == bits(b)[i]
    for a, b in zip(full, again):
        assert np.array_equal(bits(a), bits(b))
    for a, b in zip(wide, full):
        assert np.array_equal(bits(a), bits(b)[:50])


# ------------------------------------------------------------------------------------------------
# the Scorer and the CLI against the float64 pipeline
# ------------------------------------------------------------------------------------------------
def _plda_data(rng, n_spk, D, n_range):
    B = np.diag(rng.uniform(0.5, 3.0, D))
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


@pytest.fixture(scope="module")
def task():
    """Speakers 0-99 train the mean, LDA and PLDA; 100-149 enrol 3 utterances each and test the rest; 150-249 are the cohort."""
    from xvector_amd import backend
    rng = np.random.default_rng(11)
    D, dim = 64, 20
    x, lab = _plda_data(rng, 250, D, (3, 8))
    tr = lab < 100
    mean = x[tr].astype(np.float64).mean(axis=0).astype(np.float32)
    t = backend.fit_lda(x[tr].astype(np.float64) - x[tr].astype(np.float64).mean(axis=0), lab[tr], dim).astype(np.float32)
    y = ref.chain(x[tr], x[tr].astype(np.float64).mean(axis=0), t, True)
    plda = backend.fit_plda(y, [np.flatnonzero(lab[tr] == s) for s in range(100)])
    plda = backend.Plda(plda.mean.astype(np.float32), plda.transform.astype(np.float32), plda.psi.astype(np.float32))
    enrol, counts, tests, tlab = [], [], [], []
    for s in range(100, 150):
        ix = np.flatnonzero(lab == s)
        enrol.append(x[ix[:3]].astype(np.float64).mean(axis=0))
        counts.append(3)
        tests += list(ix[3:])
        tlab += [s] * (len(ix) - 3)
    cohort = x[lab >= 150]
    ee, tt = np.meshgrid(np.arange(50), np.arange(len(tests)), indexing="ij")
    return dict(enrol=np.array(enrol, np.float32), counts=np.array(counts, np.int32), test=x[tests], tlab=np.array(tlab),
                cohort=cohort, mean=mean, t=t, plda=plda, e_idx=ee.ravel(), t_idx=tt.ravel())


def _scorer(task, scoring, top_n):
    from xvector_amd import backend
    return backend.Scorer(task["enrol"], task["test"], task["plda"] if scoring == "plda" else None, task["counts"], task["mean"],
                          task["t"], scoring, cohort=task["cohort"], cohort_top_n=top_n)


def _fp64(task, scoring, top_n):
    pl = task["plda"]
    return asnorm_ref.pipeline(task["enrol"], task["counts"], task["test"], task["cohort"], task["mean"], task["t"],
                               (pl.mean, pl.transform, pl.psi) if scoring == "plda" else None, scoring, task["e_idx"],
                               task["t_idx"], top_n)


# Bound on the fp32 error of one PLDA / cosine score here (the raw scores measure 4.6e-5 / 2.4e-7).  A perturbation of at most eps
# per score moves every top-N order statistic, hence mu and sigma, by at most eps, so s' can move by
# 1/2 sum_side (2 eps / sigma + |s - mu| eps / sigma^2): with N = 2 sigma can be tiny and s' ill-conditioned.
SCORE_EPS = {"plda": 2e-4, "cosine": 2e-6}


@pytest.mark.parametrize("scoring", ["plda", "cosine"])
def test_asnorm_matches_fp64_pipeline(task, scoring):
    import torch
    from xvector_amd import backend
    nc = len(task["cohort"])
    for top_n in (2, 50, nc):
        sc = _scorer(task, scoring, top_n)
        e_idx, t_idx = task["e_idx"], task["t_idx"]
        raw = sc.score_trials(e_idx, t_idx)
        got = sc.score_trials(e_idx, t_idx, norm="asnorm")
        s64, want, Se64, St64 = _fp64(task, scoring, top_n)
        err = np.abs(got - want)
        print("%s N = %d: max |s' - fp64| = %.3e (raw %.3e)" % (scoring, top_n, err.max(), np.abs(raw - s64).max()))
        if top_n >= 50:
            assert err.max() <= 2e-3
        eps = SCORE_EPS[scoring]
        prop = 0.0
        for (mu, sd), ix in ((asnorm_ref.topn_stats(Se64, top_n), e_idx), (asnorm_ref.topn_stats(St64, top_n), t_idx)):
            prop = prop + 0.5 * (2 * eps / sd[ix] + np.abs(s64 - mu[ix]) * eps / sd[ix] ** 2)
        assert np.all(err <= 2e-3 + prop), (err / (2e-3 + prop)).max()
        plain = backend.Scorer(task["enrol"], task["test"], task["plda"] if scoring == "plda" else None, task["counts"],
                               task["mean"], task["t"], scoring)
        assert np.array_equal(raw, plain.score_trials(e_idx, t_idx))        # the cohort leaves the raw scores alone
        if top_n == nc:
            # S-norm from the GPU's own cohort score matrices, in NumPy
            Se = torch.empty((len(task["enrol"]), nc), device="cuda")
            St = torch.empty((len(task["test"]), nc), device="cuda")
            from xvector_amd import hiplib
            hiplib.score_matrix(sc.E, sc.C, sc.r, Se)
            hiplib.score_matrix(sc.TE, sc.C, sc.rT, St)
            Se, St = Se.cpu().numpy().astype(np.float64), St.cpu().numpy().astype(np.float64)
            snorm = asnorm_ref.asnorm(raw.astype(np.float64), Se.mean(1)[e_idx], Se.std(1)[e_idx], St.mean(1)[t_idx], St.std(1)[t_idx])
            assert np.abs(got - snorm).max() <= 1e-4, np.abs(got - snorm).max()


def _ragged(n):
    """A chunk size that cuts n rows into >= 3 chunks with a shorter last one."""
    c = max(1, n // 3 - 1)
    while n % c == 0:
        c -= 1
    return c


def test_cohort_stats_chunking_is_bit_exact(task):
    sc = _scorer(task, "plda", 50)
    nc = len(task["cohort"])
    row_bytes = (nc + 3) // 4 * 4 * 4
    for side, n in (("enrol", len(task["enrol"])), ("test", len(task["test"]))):
        idx = np.arange(n)[::-1].copy()
        one = [a.cpu().numpy() for a in sc.cohort_stats(side, idx)]
        c = _ragged(n)
        assert n // c >= 3 and n % c != 0
        for kw in (dict(max_bytes=row_bytes * c), dict(chunk_rows=c), dict(chunk_rows=c, max_bytes=row_bytes * (c + 5))):
            got = [a.cpu().numpy() for a in sc.cohort_stats(side, idx, **kw)]
            for a, b in zip(got, one):
                assert np.array_equal(a.view(np.int32), b.view(np.int32)), (side, kw)


def test_asnorm_refuses_a_zero_std(task):
    from xvector_amd import backend
    cohort = np.repeat(task["cohort"][:1], 5, axis=0)                 # every cohort score of a row is the same
    sc = backend.Scorer(task["enrol"], task["test"], task["plda"], task["counts"], task["mean"], task["t"], "plda", cohort=cohort,
                        cohort_top_n=5)
    with pytest.raises(backend.CohortStatsError, match="enrolment row"):
        sc.score_trials(task["e_idx"][:10], task["t_idx"][:10], norm="asnorm")


def _run(args, check=True):
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "x-vector-kaldi-tf_amd"), TWIN] + [env.get("PYTHONPATH", "")])
    return subprocess.run([sys.executable] + args, env=env, check=check, capture_output=True, text=True, timeout=600)


def test_score_cli_with_cohort(task, tmp_path):
    import kaldi_io
    from xvector_amd import backend
    p = str(tmp_path)
    ek = ["spk%03d" % i for i in range(len(task["enrol"]))]
    tk = ["utt%04d" % i for i in range(len(task["test"]))]
    ck = ["coh%04d" % i for i in range(len(task["cohort"]))]
    for name, keys, vec in (("enrol", ek, task["enrol"]), ("test", tk, task["test"]), ("cohort", ck, task["cohort"])):
        with kaldi_io.TableWriter("%s/%s.ark" % (p, name), "%s/%s.scp" % (p, name)) as w:
            kaldi_io.write_vec_flt_batch(w, keys, list(vec))
    open(p + "/num_utts.ark", "w").writelines("%s %d\n" % (k, n) for k, n in zip(ek, task["counts"]))
    kaldi_io.write_vec_flt(p + "/mean.vec", task["mean"])
    backend.write_transform(p + "/transform.mat", task["t"])
    backend.write_plda(p + "/plda", task["plda"])
    e_idx, t_idx = task["e_idx"], task["t_idx"]
    lab = ["target" if task["tlab"][b] == a + 100 else "nontarget" for a, b in zip(e_idx, t_idx)]
    with open(p + "/trials", "w") as f:
        f.writelines("%s %s %s\n" % (ek[a], tk[b], l) for a, b, l in zip(e_idx, t_idx, lab))
    cli = os.path.join(TWIN, "plda_backend.py")
    base = [cli, "score", "--num-utts=ark:" + p + "/num_utts.ark", "--mean", p + "/mean.vec", "--lda", p + "/transform.mat"]
    files = [p + "/plda", "scp:" + p + "/enrol.scp", "scp:" + p + "/test.scp", p + "/trials"]
    res = _run(base + ["--cohort", "scp:" + p + "/cohort.scp", "--cohort-top-n", "50"] + files + [p + "/scores_as"])
    nc = len(ck)
    assert "AS-norm: cohort of %d vectors, top-N 50" % nc in res.stderr, res.stderr
    lines = open(p + "/scores_as").read().splitlines()
    assert [tuple(l.split()[:2]) for l in lines] == [(ek[a], tk[b]) for a, b in zip(e_idx, t_idx)]
    got = np.array([float(l.split()[2]) for l in lines])
    assert all(l.split()[2] == "%g" % v for l, v in zip(lines, got))
    _, want, _, _ = _fp64(task, "plda", 50)
    print("CLI AS-norm vs fp64 pipeline: max |diff| = %.3e" % np.abs(got - want).max())
    assert np.abs(got - want).max() <= 2e-3 + 1e-5 * np.abs(want).max()        # + the %g rounding of the file
    # the clamp: N above the cohort size warns and scores with N = Nc
    res = _run(base + ["--cohort", "scp:" + p + "/cohort.scp", "--cohort-top-n", str(nc + 100)] + files + [p + "/scores_all"])
    assert "exceeds the cohort size %d" % nc in res.stderr and "top-N %d" % nc in res.stderr
    _, want_all, _, _ = _fp64(task, "plda", nc)
    got_all = np.array([float(l.split()[2]) for l in open(p + "/scores_all")])
    assert np.abs(got_all - want_all).max() <= 2e-3 + 1e-5 * np.abs(want_all).max()
    res = _run(base + ["--cohort", "scp:" + p + "/cohort.scp", "--cohort-top-n", "1"] + files + [p + "/scores_1"], check=False)
    assert res.returncode != 0 and "--cohort-top-n must be at least 2" in res.stderr and not os.path.exists(p + "/scores_1")
    # cosine with a cohort
    _run([cli, "score", "--scoring", "cosine", "--mean", p + "/mean.vec", "--lda", p + "/transform.mat", "--cohort",
          "scp:" + p + "/cohort.scp", "--cohort-top-n", "50"] + files + [p + "/scores_cos"])
    _, want_cos, _, _ = _fp64(task, "cosine", 50)
    got_cos = np.array([float(l.split()[2]) for l in open(p + "/scores_cos")])
    assert np.abs(got_cos - want_cos).max() <= 2e-3 + 1e-5 * np.abs(want_cos).max()
    # without --cohort: byte for byte what the unnormalised path writes
    _run(base + files + [p + "/scores_raw"])
    sc = backend.Scorer(task["enrol"], task["test"], task["plda"], task["counts"], task["mean"], task["t"], "plda")
    raw = sc.score_trials(e_idx, t_idx, norm="none")
    want_text = "".join("%s %s %g\n" % (ek[a], tk[b], s) for a, b, s in zip(e_idx, t_idx, raw.tolist()))
    assert open(p + "/scores_raw").read() == want_text
    # compute-eer on the normalised scores
    with open(p + "/eer_in", "w") as f:
        f.writelines("%s %s\n" % (l.split()[2], t) for l, t in zip(lines, lab))
    eer = float(_run([cli, "compute-eer", p + "/eer_in"]).stdout.strip())
    print("CLI AS-norm EER %.2f %%" % eer)
    assert 0.0 <= eer < 25.0
