"""xv_ahc_average_f64 on the MI355X against tests/ahc_ref.py: the merges bit for bit, on tie-free scores and
on integer scores full of ties (every fp64 sum exact, so the tie rule alone decides); independence of ld, the workspace and
what ran before; the argument policy; clustering-based adaptation end to end on planted speakers, in process and through
plda_backend.py."""
import ctypes
import functools
import os

import numpy as np
import pytest

import ahc_ref
import backend_ref as ref

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 17, 64, 65, 130, 257, 1025, 2050)
NINF = -np.inf


def _scores(n, kind):
    """scores[n, n] float32; 'normal': tie-free draws, 'ties': integers from {-2..2}."""
    rng = np.random.default_rng(1000 + n)
    if kind == "normal":
        return rng.standard_normal((n, n)).astype(np.float32)
    return rng.integers(-2, 3, (n, n)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _full(n, kind):
    """The reference's full dendrogram, computed once per (n, kind); every stop rule is a cut of it."""
    out = ahc_ref.dendrogram(_scores(n, kind))
    for a in out:
        a.setflags(write=False)
    return out


def _device_scores(s, ld):
    """s in the strict upper triangle of a [n, ld] device buffer; NaN everywhere else (diagonal, lower triangle, padding)."""
    import torch
    n = s.shape[0]
    host = np.full((n, ld), np.nan, np.float32)
    iu = np.triu_indices(n, 1)
    host[iu] = s[iu]
    return torch.from_numpy(host).cuda()


class Outputs(object):
    """Poisoned outputs, longer than needed."""

    def __init__(self, n):
        import torch
        self.n = n
        self.a = torch.full((n + 7,), -1, dtype=torch.int32, device="cuda")
        self.b = torch.full((n + 7,), -1, dtype=torch.int32, device="cuda")
        self.s = torch.full((n + 7,), float("nan"), dtype=torch.float64, device="cuda")
        self.m = torch.full((4,), -1, dtype=torch.int32, device="cuda")
        self.lab = torch.full((n + 5,), -1, dtype=torch.int32, device="cuda")

    def host(self):
        return [t.cpu().numpy() for t in (self.a, self.b, self.s, self.m, self.lab)]

    def untouched(self):
        a, b, s, m, lab = self.host()
        return bool(np.all(a == -1) and np.all(b == -1) and np.all(np.isnan(s)) and np.all(m == -1) and np.all(lab == -1))


def _run(dev_scores, n, threshold, min_clusters, workspace=None):
    from xvector_amd import hiplib
    out = Outputs(n)
    hiplib.ahc_average(dev_scores[:, :n], threshold, min_clusters, out.a, out.b, out.s, out.m, out.lab, workspace=workspace)
    return out


@pytest.mark.parametrize("kind", ["normal", "ties"])
@pytest.mark.parametrize("n", SIZES)
def test_exact(n, kind):
    s = _scores(n, kind)
    dev = _device_scores(s, (n + 3) // 4 * 4 + 4)
    configs = [(NINF, 1), (0.0, 1), (0.5, 1)] + ([(NINF, 5)] if n >= 5 else [])
    for threshold, min_clusters in configs:
        wa, wb, ws = ahc_ref.cut(n, _full(n, kind), threshold, min_clusters)
        a, b, sc, m, lab = _run(dev, n, threshold, min_clusters).host()
        k = len(wa)
        what = "n %d %s threshold %r min_clusters %d" % (n, kind, threshold, min_clusters)
        assert m[0] == k, what
        assert np.array_equal(a[:k], wa) and np.array_equal(b[:k], wb), what
        assert np.array_equal(sc[:k].view(np.int64), ws.view(np.int64)), what          # bit for bit
        assert np.array_equal(lab[:n], ahc_ref.labels(n, wa, wb)), what
        # the tails stay poisoned
        assert np.all(a[k:] == -1) and np.all(b[k:] == -1) and np.all(np.isnan(sc[k:])), what
        assert np.all(m[1:] == -1) and np.all(lab[n:] == -1), what
    if n >= 5:
        assert k == n - 5 and len(set(lab[:n].tolist())) == 5


@pytest.mark.parametrize("kind", ["normal", "ties"])
def test_independent_of_ld_workspace_and_history(kind):
    import torch
    from xvector_amd import hiplib
    n = 257
    s = _scores(n, kind)
    nbytes = hiplib.ahc_average_workspace_bytes(n)
    assert nbytes >= 8 * n * n
    runs = []
    for ld, fill in ((260, 0xFF), (272, 0x00), (260, 0x7F)):
        ws = torch.full((nbytes + 64,), fill, dtype=torch.uint8, device="cuda")
        dev = _device_scores(s, ld)
        runs.append(_run(dev, n, 0.0, 1, workspace=ws).host())
        runs.append(_run(dev, n, 0.0, 1, workspace=ws).host())         # again, on the workspace the first run left behind
    assert runs[0][3][0] > 0
    for r in runs[1:]:
        for x, y in zip(runs[0], r):
            assert x.tobytes() == y.tobytes()


def test_argument_policy():
    import torch
    from xvector_amd import hiplib
    lib = hiplib.require_gpu()
    n, ld = 12, 16
    dev = _device_scores(_scores(n, "normal"), ld)
    need = hiplib.ahc_average_workspace_bytes(n)
    assert need >= 8 * n * n and hiplib.ahc_average_workspace_bytes(0) == 0
    assert hiplib.ahc_average_workspace_bytes(hiplib.AHC_MAX_N + 1) == 0
    assert hiplib.ahc_average_workspace_bytes(hiplib.AHC_MAX_N) >= 8 * hiplib.AHC_MAX_N ** 2
    ws = torch.zeros(need + 64, dtype=torch.uint8, device="cuda")
    out = Outputs(n)
    BAD, UNSUPPORTED = -1, -2

    def call(scores_ptr=dev.data_ptr(), ld=ld, n=n, threshold=0.0, min_clusters=1, ws_bytes=need):
        return lib.xv_ahc_average_f64(ctypes.c_void_p(scores_ptr), ld, n, threshold, min_clusters, hiplib._ptr(out.a),
                                      hiplib._ptr(out.b), hiplib._ptr(out.s), hiplib._ptr(out.m), hiplib._ptr(out.lab),
                                      hiplib._ptr(ws), ws_bytes, hiplib._stream())

    cases = [("n = 0", dict(n=0), BAD), ("n < 0", dict(n=-3), BAD), ("ld < n", dict(ld=8), BAD), ("ld % 4", dict(ld=14), BAD),
             ("misaligned scores", dict(scores_ptr=dev.data_ptr() + 4), BAD), ("min_clusters 0", dict(min_clusters=0), BAD),
             ("min_clusters n + 1", dict(min_clusters=n + 1), BAD), ("NaN threshold", dict(threshold=float("nan")), BAD),
             ("small workspace", dict(ws_bytes=need - 1), BAD),
             ("n > XV_AHC_MAX_N", dict(n=hiplib.AHC_MAX_N + 1, ld=hiplib.AHC_MAX_N + 4, min_clusters=1), UNSUPPORTED)]
    for what, kw, code in cases:
        assert call(**kw) == code, what
        assert lib.xv_last_error(), what
    torch.cuda.synchronize()
    assert out.untouched()
    assert call() == 0                                           # and the same call with nothing wrong runs
    torch.cuda.synchronize()
    assert out.host()[3][0] == len(ahc_ref.cut(n, ahc_ref.dendrogram(_scores(n, "normal")), 0.0, 1)[0])


def test_host_api_refusals():
    import torch
    from xvector_amd import backend
    s = torch.zeros((6, 6), device="cuda")
    s[1, 4] = float("inf")
    with pytest.raises(ValueError, match="not finite"):
        backend.ahc(s)
    s[1, 4] = 0.0
    s[4, 1] = float("nan")                                       # the lower triangle and the diagonal are not looked at
    s[2, 2] = float("inf")
    lab, (a, b, sc) = backend.ahc(s, threshold=0.0)
    assert lab.tolist() == [0] * 6 and a.tolist() == [0] * 5 and b.tolist() == [1, 2, 3, 4, 5] and sc.tolist() == [0.0] * 5
    with pytest.raises(ValueError, match="max_bytes"):
        backend.ahc(s, max_bytes=100)
    with pytest.raises(ValueError):
        backend.ahc(s, num_clusters=7)
    with pytest.raises(ValueError):
        backend.ahc(s, threshold=None)
    with pytest.raises(ValueError):
        backend.ahc(s[:, :5])
    lab, (a, _, _) = backend.ahc(s, threshold=None, num_clusters=4)
    assert len(a) == 2 and lab.tolist() == [0, 0, 0, 3, 4, 5]
    lab, (a, _, _) = backend.ahc(s, threshold=1.0, num_clusters=4)          # num_clusters leaves the threshold alone
    assert len(a) == 0
    # N = AHC_MAX_N + 1 is refused before anything of that size exists: a 0-stride view stands in for the matrix
    big = torch.zeros(1, device="cuda").expand(32769, 32769)
    with pytest.raises(ValueError, match="exceed"):
        backend.ahc(big)


# ------------------------------------------------------------------------------------------------
# end to end on planted speakers
# ------------------------------------------------------------------------------------------------
D, DIM, THRESHOLD = 24, 16, -8.0
N_IN_SPK, N_IN_UTT = 40, 5


def _draw(rng, mix, mu, n_spk, n_utt, spk_std=5.0):
    spk = rng.standard_normal((n_spk, 1, D)) * spk_std
    x = (spk + rng.standard_normal((n_spk, n_utt, D))).reshape(n_spk * n_utt, D) @ mix + mu
    return x.astype(np.float32), np.repeat(np.arange(n_spk), n_utt)


def _partition(labels):
    out = {}
    for i, l in enumerate(np.asarray(labels).tolist()):
        out.setdefault(l, []).append(i)
    return set(frozenset(v) for v in out.values())


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from xvector_amd import backend
    rng = np.random.default_rng(11)
    mix = rng.standard_normal((D, D)) / np.sqrt(D)
    mu = rng.standard_normal(D)
    xo, lo = _draw(rng, mix, mu, 60, 6)                                  # out of domain, labelled
    xo64 = xo.astype(np.float64)
    t = backend.fit_lda(xo64 - xo64.mean(axis=0), list(lo), DIM).astype(np.float32)
    plda = backend.fit_plda(ref.chain(xo64, xo64.mean(axis=0), t, True), [np.flatnonzero(lo == s) for s in range(60)])
    xi, li = _draw(rng, mix, mu + 0.5 * rng.standard_normal(D), N_IN_SPK, N_IN_UTT)      # in domain: shifted mean, shuffled
    perm = rng.permutation(len(xi))
    xi, li = xi[perm], li[perm]
    mean_in = xi.astype(np.float64).mean(axis=0).astype(np.float32)
    return dict(t=t, plda=plda, xi=xi, li=li, mean_in=mean_in, xo=xo, lo=lo, p=str(tmp_path_factory.mktemp("cluster")))


def test_planted_speakers(world):
    from xvector_amd import backend
    xi, li, t, plda, mean_in = (world[k] for k in ("xi", "li", "t", "plda", "mean_in"))
    n = len(xi)
    # the fixture, not the kernel, carries the condition: the float64 reference on float64 scores recovers the planted speakers
    pl = (plda.mean, plda.transform, plda.psi)
    ones = np.ones(n)
    rows, r = ref.side_rows_enrol(ref.chain(xi, mean_in, t, True, pl, ones), ones, plda.psi)
    s64 = rows @ ref.side_rows_test(ref.chain(xi, mean_in, t, True, pl, None)).T + r[:, None]
    full = ahc_ref.dendrogram(s64)
    lab64, (a64, _, sc64) = ahc_ref.ahc(s64, threshold=THRESHOLD)
    print("float64 reference: %d merges, last accepted %.3f, first rejected %.3f" % (len(a64), sc64[-1], full[2][len(a64)]))
    assert _partition(lab64) == _partition(li) and len(a64) == n - N_IN_SPK
    # the device: the planted partition, and the reference's merges on the device's own fp32 matrix
    lab, (a, b, sc) = backend.cluster_vectors(xi, plda, mean=mean_in, transform=t, threshold=THRESHOLD)
    assert _partition(lab) == _partition(li)
    s32 = backend.score_matrix_self(xi, plda, mean_in, t)[:, :n].cpu().numpy()
    print("max |fp32 score - float64 score| = %.3e" % np.abs(s32 - s64).max())
    wl, (wa, wb, ws) = ahc_ref.ahc(s32, threshold=THRESHOLD)
    assert np.array_equal(a, wa) and np.array_equal(b, wb) and np.array_equal(sc.view(np.int64), ws.view(np.int64))
    assert np.array_equal(lab, wl) and np.array_equal(backend.labels_from_merges(n, a, b), lab)
    assert lab.dtype == np.int32 and a.dtype == np.int32 and sc.dtype == np.float64
    # num_clusters stops earlier; with threshold None it is the only stop
    lab50, (a50, _, _) = backend.cluster_vectors(xi, plda, mean=mean_in, transform=t, threshold=THRESHOLD, num_clusters=50)
    assert len(a50) == n - 50 and np.array_equal(a50, wa[:n - 50])
    lab7, _ = backend.cluster_vectors(xi, plda, mean=mean_in, transform=t, threshold=None, num_clusters=7)
    assert len(set(lab7.tolist())) == 7


def test_cli_route(world, caplog):
    """cluster -> spk2utt -> compute-plda --lda -> interpolate-plda -> score, through plda_backend.py's own entry point."""
    import kaldi_io
    import plda_backend
    from xvector_amd import backend
    p, xi, li = world["p"], world["xi"], world["li"]
    n = len(xi)
    keys = ["major-%04d" % i for i in range(n)]
    with kaldi_io.TableWriter(p + "/major.ark", p + "/major.scp") as w:
        kaldi_io.write_vec_flt_batch(w, keys, list(xi))
    backend.write_transform(p + "/transform.mat", world["t"])
    backend.write_plda(p + "/plda", world["plda"])
    with caplog.at_level("INFO", logger="plda_backend"):
        plda_backend.main(["cluster", "--lda", p + "/transform.mat", "--threshold", str(THRESHOLD), p + "/plda",
                           "ark:" + p + "/major.ark", p + "/utt2cluster"])
    assert "Clustered %d vectors of dimension %d into %d clusters (0 with a single vector)" % (n, DIM, N_IN_SPK) in caplog.text
    lines = [l.split() for l in open(p + "/utt2cluster").read().splitlines()]
    assert [l[0] for l in lines] == keys and all(len(l) == 2 for l in lines)
    names = [l[1] for l in lines]
    assert sorted(set(names)) == ["c%03d" % (i + 1) for i in range(N_IN_SPK)]            # 200 vectors: three digits
    assert _partition(names) == _partition(li)
    first = {}
    for i, c in enumerate(names):
        first.setdefault(c, i)
    assert sorted(first, key=first.get) == sorted(first)            # ranked by label = by the cluster's first vector
    # utt2cluster -> spk2utt, the in-domain model, the mix, the scores
    spk2utt = {}
    for k, c in lines:
        spk2utt.setdefault(c, []).append(k)
    with open(p + "/cluster2utt", "w") as f:
        f.writelines("%s %s\n" % (c, " ".join(u)) for c, u in spk2utt.items())
    plda_backend.main(["compute-plda", "--lda", p + "/transform.mat", p + "/cluster2utt", "ark:" + p + "/major.ark", p + "/plda_in"])
    plda_backend.main(["interpolate-plda", "--alpha", "0.5", p + "/plda", p + "/plda_in", p + "/plda_mix"])
    kaldi_io.write_vec_flt(p + "/mean.vec", world["mean_in"])
    trials = [(keys[i], keys[j]) for i in range(0, n, 7) for j in range(0, n, 3)]
    with open(p + "/trials", "w") as f:
        f.writelines("%s %s\n" % tr for tr in trials)
    plda_backend.main(["score", "--mean", p + "/mean.vec", "--lda", p + "/transform.mat", p + "/plda_mix", "ark:" + p + "/major.ark",
                       "ark:" + p + "/major.ark", p + "/trials", p + "/scores"])
    got = [l.split() for l in open(p + "/scores").read().splitlines()]
    assert [(g[0], g[1]) for g in got] == trials
    sc = np.array([float(g[2]) for g in got])
    assert np.all(np.isfinite(sc))
    same = np.array([li[keys.index(a)] == li[keys.index(b)] for a, b in trials])
    assert sc[same].mean() > sc[~same].mean()


def test_cli_refusals(world, tmp_path):
    import plda_backend
    from xvector_amd import backend
    p, q = world["p"], str(tmp_path)
    backend.write_transform(q + "/transform.mat", world["t"])
    backend.write_plda(q + "/plda", world["plda"])
    backend.write_plda(q + "/plda17", backend.plda_from_covariances(np.zeros(DIM + 1), np.eye(DIM + 1) * 2.0, np.eye(DIM + 1)))
    open(q + "/empty.ark", "wb").close()
    import kaldi_io
    with kaldi_io.TableWriter(q + "/v.ark", q + "/v.scp") as w:
        kaldi_io.write_vec_flt_batch(w, ["u%d" % i for i in range(6)], list(world["xi"][:6]))
    base = ["cluster", "--lda", q + "/transform.mat"]
    for argv, word in ((base + [q + "/plda", "ark:" + q + "/empty.ark", q + "/out1"], "no vectors"),
                       (base + [q + "/plda17", "ark:" + q + "/v.ark", q + "/out2"], "dimension"),
                       (base + ["--num-clusters", "7", q + "/plda", "ark:" + q + "/v.ark", q + "/out3"], "num-clusters")):
        with pytest.raises(SystemExit) as ei:
            plda_backend.main(argv)
        assert word in str(ei.value), ei.value
    assert not any(os.path.exists(q + "/out%d" % i) for i in (1, 2, 3))
