"""Timings of the scoring back-end: prepare at N = 100 k, D = 512; the dense scorer at Ne = Nt = 16384 against the
157.3 TF fp32-MFMA peak; the trial scorer at 2 M trials; the `plda_backend.py score` CLI on an SRE16-sized synthetic job with a
read / prepare / score / write breakdown.  Device events after warm-up.   python tools/backend_bench.py [--fit | --asnorm | --adapt]
(--fit: instead time the host fp64 LDA + PLDA fits at N = 100 k, D = 512; needs no GPU.  --asnorm: instead time AS-norm --
cohort scoring and the top-N statistics kernel separately at the recipe shape and at 50 k rows x 50 k cohort in 1 GiB chunks,
then the `score --cohort` CLI on the SRE16-sized job beside the same job without a cohort.  --adapt: instead time the fp64
moments kernel (xv_moment_stats_f64) at N = 10^6, d = 100 and 200 against the 78.6 TF fp64-MFMA peak and against NumPy's fp64
x.T @ x on the host's threads, then the whole `plda_backend.py adapt-plda --lda` command at N = 10^5, D = 512, d = 200)."""
import os, shutil, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWIN = os.path.join(ROOT, "x-vector-kaldi-tf_amd", "local", "tf")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "x-vector-kaldi-tf_amd")); sys.path.insert(0, TWIN)
import numpy as np

PEAK_TF = 157.3


def fit_timing():
    from xvector_amd import backend
    rng = np.random.default_rng(0)
    N, D, S = 100000, 512, 5000
    lab = rng.integers(0, S, N)
    x = rng.standard_normal((S, D))[lab] + rng.standard_normal((N, D))
    t0 = time.perf_counter()
    lda = backend.fit_lda(x, lab, 200)
    t1 = time.perf_counter()
    y = x @ lda[:, :D].T + lda[:, D]
    groups = [np.flatnonzero(lab == s) for s in range(S)]
    t2 = time.perf_counter()
    backend.fit_plda(y, groups)
    t3 = time.perf_counter()
    print("host fp64 fits, N = %d, D = %d, %d speakers: fit_lda (d = 200) %.2f s, fit_plda (d = 200, 10 EM iterations) %.2f s" %
          (N, D, S, t1 - t0, t3 - t2))


def timed(fn, reps):
    import torch
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def gpu_timing():
    import torch
    from xvector_amd import backend, hiplib
    dev = "cuda:0"
    rng = np.random.default_rng(1)
    N, D = 100000, 512
    x = torch.randn((N, D), device=dev)
    nu = torch.randint(1, 10, (N,), dtype=torch.int32, device=dev)
    mean = torch.randn(D, device=dev) * 0.1
    for d in (100, 200):
        lda = torch.randn((d, D), device=dev) / D ** 0.5
        a0 = torch.randn(d, device=dev)
        q, _ = np.linalg.qr(rng.standard_normal((d, d)))
        P = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(dev)
        m = torch.zeros(d, device=dev)
        psi = torch.from_numpy(np.sort(rng.uniform(0.1, 5, d))[::-1].astype(np.float32).copy()).to(dev)
        out = torch.empty((N, backend.kpad_for(2 * d)), device=dev)
        r = torch.empty(N, device=dev)
        ms = timed(lambda: hiplib.backend_prepare(x, out, hiplib.SIDE_ENROL, nu, mean, lda, a0, True, P, m, psi, r), 20)
        fl = 2.0 * N * d * (D + d)
        print("prepare (enrolment side) N = %d, D = %d, d = %d: %.3f ms = %.1f M vectors/s, %.1f TF/s algorithmic (%.0f GB/s of x)" %
              (N, D, d, ms, N / ms / 1e3, fl / ms / 1e9, N * D * 4 / ms / 1e6))
    n = 16384
    for K in (200, 400):
        E = torch.randn((n, K), device=dev)
        T = torch.randn((n, K), device=dev)
        r = torch.randn(n, device=dev)
        S = torch.empty((n, n), device=dev)
        ms = timed(lambda: hiplib.score_matrix(E, T, r, S), 10)
        tf = 2.0 * n * n * K / ms / 1e9
        print("score_matrix Ne = Nt = %d, K = %d: %.3f ms = %.1f TF/s algorithmic = %.2f of the %.1f TF fp32-MFMA peak "
              "(%.0f GB/s of scores written)" % (n, K, ms, tf, tf / PEAK_TF, PEAK_TF, n * n * 4 / ms / 1e6))
    ne, nt, M, K = 800, 9300, 2000000, 200
    E = torch.randn((ne, K), device=dev)
    T = torch.randn((nt, K), device=dev)
    r = torch.randn(ne, device=dev)
    ei = torch.randint(0, ne, (M,), dtype=torch.int32, device=dev)
    ti = torch.randint(0, nt, (M,), dtype=torch.int32, device=dev)
    out = torch.empty(M, device=dev)
    lib = hiplib.require_gpu()
    stream = hiplib._stream()
    call = lambda: lib.xv_score_pairs_f32(hiplib._ptr(E), hiplib._ptr(T), K, K, hiplib._ptr(ei), hiplib._ptr(ti), M, hiplib._ptr(r),
                                          hiplib._ptr(out), stream)
    ms = timed(call, 20)
    print("score_pairs %d trials (Ne = %d, Nt = %d, K = %d): %.3f ms = %.0f M trials/s" % (M, ne, nt, K, ms, M / ms / 1e3))
    Sd = torch.empty((ne, nt), device=dev)
    ms = timed(lambda: hiplib.score_matrix(E, T, r, Sd), 20)
    print("score_matrix on the same job (all %d cells): %.3f ms" % (ne * nt, ms))


def asnorm_timing(top_n=300):
    """Cohort scoring (xv_score_matrix_f32) and the top-N statistics (xv_topk_row_stats_f32), each timed on its own with device
    events: the recipe shape (800 enrolment + 9.3 k test rows against 2,000 cohort vectors, K = 2d = 200) and 50 k rows x
    50 k cohort in chunks of at most 1 GiB of scores (K = 200 and 400), as Scorer.cohort_stats runs them."""
    import torch
    from xvector_amd import backend, hiplib
    dev = "cuda:0"
    for name, rows, nc, Ks in (("recipe shape", 800 + 9300, 2000, (200,)), ("large shape", 50000, 50000, (200, 400))):
        ldc = (nc + 3) // 4 * 4
        chunk = min(rows, backend.DENSE_MAX_BYTES // (ldc * 4))
        ws = torch.empty((chunk, ldc), device=dev)
        mu = torch.empty(rows, device=dev)
        sd = torch.empty(rows, device=dev)
        for K in Ks:
            E = torch.randn((rows, K), device=dev)
            C = torch.randn((nc, K), device=dev)
            r = torch.randn(rows, device=dev)
            ev = []

            def run(record):
                for i0 in range(0, rows, chunk):
                    m = min(chunk, rows - i0)
                    a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
                    a.record()
                    hiplib.score_matrix(E[i0:i0 + m], C, r[i0:i0 + m], ws[:m])
                    b.record()
                    hiplib.topk_row_stats(ws[:m, :nc], top_n, mu[i0:i0 + m], sd[i0:i0 + m])
                    c.record()
                    if record:
                        ev.append((a, b, c))
            run(False)
            run(False)
            reps = 5 if rows * nc < 1e9 else 2
            for _ in range(reps):
                run(True)
            torch.cuda.synchronize()
            t_sc = sum(a.elapsed_time(b) for a, b, _ in ev) / reps
            t_st = sum(b.elapsed_time(c) for _, b, c in ev) / reps
            tf = 2.0 * rows * nc * K / t_sc / 1e9
            print("AS-norm %s: %d rows x %d cohort, K = %d, top-N %d, %d chunk(s) of <= %d rows: cohort scoring %.3f ms (%.1f TF/s = "
                  "%.2f of the %.1f TF fp32-MFMA peak), top-N stats %.3f ms (%.0f GB/s effective read of the scores) = %.0f %% of "
                  "the scoring time" % (name, rows, nc, K, top_n, (rows + chunk - 1) // chunk, chunk, t_sc, tf, tf / PEAK_TF, PEAK_TF,
                                        t_st, 4.0 * rows * nc / t_st / 1e6, 100.0 * t_st / t_sc))
            del E, C


PEAK_F64_TF = 78.6


def adapt_timing():
    """xv_moment_stats_f64 in one call at N = 10^6 (median of 5 timed launches after warm-up, device events; 2 N d^2 flop and
    4 N d bytes of input), NumPy's fp64 x.T @ x of the same rows on the host (conversion to fp64 not counted), and the whole
    adapt-plda command."""
    import torch
    import kaldi_io
    import plda_backend
    from xvector_amd import backend, hiplib
    dev = "cuda:0"
    N = 1000000
    for d in (100, 200):
        x = torch.randn((N, d), device=dev)
        s = torch.empty(d, dtype=torch.float64, device=dev)
        o = torch.empty((d, d), dtype=torch.float64, device=dev)
        ws = torch.empty(hiplib.moment_stats_workspace_bytes(N, d), dtype=torch.uint8, device=dev)
        for _ in range(2):
            hiplib.moment_stats(x, s, o, workspace=ws)
        ts = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); hiplib.moment_stats(x, s, o, workspace=ws); b.record(); torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        ms = float(np.median(ts))
        tf = 2.0 * N * d * d / ms / 1e9
        x64 = x.cpu().numpy().astype(np.float64)
        x64[:1000].T @ x64[:1000]                             # warm-up of the BLAS threads
        th = []
        for _ in range(3):
            t0 = time.perf_counter(); ref = x64.T @ x64; th.append(time.perf_counter() - t0)
        host = float(np.median(th)) * 1e3
        err = np.abs(o.cpu().numpy() - ref).max() / np.abs(ref).max()
        t0 = time.perf_counter(); backend.moment_stats(x, d); wall = (time.perf_counter() - t0) * 1e3
        print("moment_stats N = %d, d = %d: kernel %.3f ms (min %.3f, max %.3f) = %.1f TF/s algorithmic = %.2f of the %.1f TF "
              "fp64-MFMA peak, %.0f GB/s of x; workspace %.0f MB; backend.moment_stats (chunks of %d rows, results copied back "
              "and added on the host) %.1f ms; NumPy fp64 x.T @ x on %s threads %.1f ms = %.1fx the kernel; max |diff| / max = %.1e"
              % (N, d, ms, min(ts), max(ts), tf, tf / PEAK_F64_TF, PEAK_F64_TF, 4.0 * N * d / ms / 1e6, ws.numel() / 1e6,
                 backend.MOMENT_CHUNK_ROWS, wall, os.environ.get("OMP_NUM_THREADS", "all"), host, host / ms, err))
        del x, x64, ws
    rng = np.random.default_rng(4)
    n, D, d = 100000, 512, 200
    tmp = tempfile.mkdtemp(prefix="backend_bench_")
    with kaldi_io.TableWriter(tmp + "/major.ark", tmp + "/major.scp") as w:
        kaldi_io.write_vec_flt_batch(w, ["utt%06d" % i for i in range(n)], list(rng.standard_normal((n, D)).astype(np.float32)))
    backend.write_transform(tmp + "/transform.mat", rng.standard_normal((d, D + 1)) / D ** 0.5)
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    backend.write_plda(tmp + "/plda", backend.Plda(np.zeros(d), q, np.sort(rng.uniform(0.1, 5, d))[::-1]))
    args = ["adapt-plda", "--within-covar-scale", "0.75", "--between-covar-scale", "0.25", "--lda", tmp + "/transform.mat",
            tmp + "/plda", "scp:%s/major.scp" % tmp, tmp + "/plda_adapt"]
    plda_backend.main(args)                                   # warm-up
    t = [time.perf_counter()]
    plda = backend.read_plda(tmp + "/plda")
    vec = plda_backend.read_vectors("scp:%s/major.scp" % tmp)
    xs = np.stack(list(vec.values()))
    lda = backend.read_transform(tmp + "/transform.mat")
    t.append(time.perf_counter())
    rows, _ = backend.prepare(xs, hiplib.SIDE_PLAIN, mean=xs.astype(np.float64).mean(axis=0).astype(np.float32), transform=lda)
    torch.cuda.synchronize(); t.append(time.perf_counter())
    nn, s1, s2 = backend.moment_stats(rows, d)
    t.append(time.perf_counter())
    backend.write_plda(tmp + "/plda_adapt", backend.adapt_plda(plda, nn, s1, s2, 0.75, 0.25))
    t.append(time.perf_counter())
    w0 = time.perf_counter(); plda_backend.main(args); w1 = time.perf_counter()
    dt = np.diff(t)
    print("adapt-plda CLI, %d vectors, D = %d, d = %d: whole command %.2f s; steps: read %.2f s, mean + upload + prepare %.3f s, "
          "moments (incl. copy back) %.3f s, host fit + write %.3f s" % (n, D, d, w1 - w0, dt[0], dt[1], dt[2], dt[3]))
    shutil.rmtree(tmp)


def cli_job(cohort=False):
    """SRE16-sized: 800 enrolment speakers, 9.3 k test segments, 2 M trials, D = 512, LDA d = 100 (cohort: also the whole
    command with --cohort of 2,000 vectors, top-N 300, beside the same command without it)."""
    import torch
    import kaldi_io
    import plda_backend
    from xvector_amd import backend
    rng = np.random.default_rng(2)
    D, d, ne, nt, M = 512, 100, 800, 9300, 2000000
    tmp = tempfile.mkdtemp(prefix="backend_bench_")
    ek = ["spk%04d" % i for i in range(ne)]
    tk = ["seg%05d" % i for i in range(nt)]
    with kaldi_io.TableWriter(tmp + "/enrol.ark", tmp + "/enrol.scp") as w:
        kaldi_io.write_vec_flt_batch(w, ek, list(rng.standard_normal((ne, D)).astype(np.float32)))
    with kaldi_io.TableWriter(tmp + "/test.ark", tmp + "/test.scp") as w:
        kaldi_io.write_vec_flt_batch(w, tk, list(rng.standard_normal((nt, D)).astype(np.float32)))
    open(tmp + "/num_utts.ark", "w").writelines("%s %d\n" % (k, rng.integers(1, 6)) for k in ek)
    ei = rng.integers(0, ne, M); ti = rng.integers(0, nt, M)
    open(tmp + "/trials", "w").writelines("%s %s target\n" % (ek[a], tk[b]) for a, b in zip(ei, ti))
    kaldi_io.write_vec_flt(tmp + "/mean.vec", (rng.standard_normal(D) * 0.1).astype(np.float32))
    backend.write_transform(tmp + "/transform.mat", rng.standard_normal((d, D + 1)) / D ** 0.5)
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    backend.write_plda(tmp + "/plda", backend.Plda(np.zeros(d), q, np.sort(rng.uniform(0.1, 5, d))[::-1]))
    args = ["score", "--num-utts=ark:%s/num_utts.ark" % tmp, "--mean", tmp + "/mean.vec", "--lda", tmp + "/transform.mat",
            tmp + "/plda", "scp:%s/enrol.scp" % tmp, "scp:%s/test.scp" % tmp, tmp + "/trials", tmp + "/scores"]
    plda_backend.main(args)                                   # warm-up (library load, kernels)
    if cohort:
        nc = 2000
        with kaldi_io.TableWriter(tmp + "/cohort.ark", tmp + "/cohort.scp") as w:
            kaldi_io.write_vec_flt_batch(w, ["coh%04d" % i for i in range(nc)], list(rng.standard_normal((nc, D)).astype(np.float32)))
        cargs = args[:1] + ["--cohort", "scp:%s/cohort.scp" % tmp, "--cohort-top-n", "300"] + args[1:]
        plda_backend.main(cargs)                              # warm-up
        w = []
        for a in (args, cargs, args, cargs):
            t0 = time.perf_counter(); plda_backend.main(a); w.append(time.perf_counter() - t0)
        print("score CLI, %d enrolment speakers x %d test segments, %d trials, D = %d, d = %d: whole command %.2f / %.2f s without a "
              "cohort, %.2f / %.2f s with --cohort of %d vectors, top-N 300" % (ne, nt, M, D, d, w[0], w[2], w[1], w[3], nc))
        shutil.rmtree(tmp)
        return
    # the same steps as cmd_score, timed one by one
    t = [time.perf_counter()]
    plda = backend.read_plda(tmp + "/plda")
    enrol = plda_backend.read_vectors("scp:%s/enrol.scp" % tmp)
    test = plda_backend.read_vectors("scp:%s/test.scp" % tmp)
    nu = {k: int(v[0]) for k, v in plda_backend.read_table(tmp + "/num_utts.ark").items()}
    epos = {k: i for i, k in enumerate(enrol)}; tpos = {k: i for i, k in enumerate(test)}
    k1, k2, a, b = [], [], [], []
    for line in open(tmp + "/trials"):
        p = line.split()
        k1.append(p[0]); k2.append(p[1]); a.append(epos[p[0]]); b.append(tpos[p[1]])
    mean = kaldi_io.read_vec_flt(tmp + "/mean.vec").astype(np.float32)
    lda = backend.read_transform(tmp + "/transform.mat")
    t.append(time.perf_counter())
    sc = backend.Scorer(np.stack(list(enrol.values())), np.stack(list(test.values())), plda,
                        np.array([nu[k] for k in enrol], np.int32), mean, lda)
    torch.cuda.synchronize(); t.append(time.perf_counter())
    s = sc.score_trials(a, b)
    t.append(time.perf_counter())
    plda_backend.write_scores(tmp + "/scores", k1, k2, s)
    t.append(time.perf_counter())
    w0 = time.perf_counter(); plda_backend.main(args); w1 = time.perf_counter()
    dt = np.diff(t)
    print("score CLI, %d enrolment speakers x %d test segments, %d trials, D = %d, d = %d: whole command %.2f s; steps: read %.2f s, "
          "prepare %.3f s, score %.3f s (%s, incl. copy back), write %.2f s" %
          (ne, nt, M, D, d, w1 - w0, dt[0], dt[1], dt[2], "dense-then-gather" if sc.use_dense(M) else "pairs", dt[3]))
    shutil.rmtree(tmp)


if __name__ == "__main__":
    if "--fit" in sys.argv:
        fit_timing()
    elif "--adapt" in sys.argv:
        adapt_timing()
    elif "--asnorm" in sys.argv:
        asnorm_timing()
        cli_job(cohort=True)
    else:
        gpu_timing()
        cli_job()
