"""The per-recording PCA and the projected PLDA on the MI355X: xv_pca_plda_groups_f64 and
xv_backend_prepare_groups_f32 against tests/pca_ref.py, which is always fed the very fp32 rows the kernel read.

The constant of the eigen-solver's bounds: tests/pca_ref.py emulates the kernel's rotation order in NumPy; on the fixtures of this
file (pca_ref.emulation_ratios over every group of _rows(d) for d in DIMS) its largest errors, in units of d 2^-52 ||C||_2, were
EMULATED_RATIO = 1.5 (eigenvalues 0.37, orthogonality 1.49, residual 1.07; 3 to 15 sweeps).  The tests allow C_BOUND = 4 times
that, 6."""
import functools
import os

import numpy as np
import pytest

import backend_ref as ref
import pca_ref
import test_gpu_cluster as single

pytestmark = pytest.mark.gpu

DIMS = (1, 7, 8, 100, 128)
SIZES = (200, 1, 60, 2, 3)
TARGETS = (0.1, 0.5, 0.9)
EMULATED_RATIO = 1.5
C_BOUND = 4 * EMULATED_RATIO
EPS = 2.0 ** -52
POISON_I = -7


def _unit_rows(rng, d, n, n_spk=3, noise=0.6):
    """Planted speakers plus noise, length-normalised to sqrt(d), as the fp32 rows the kernel reads."""
    centers = rng.standard_normal((n_spk, d))
    y = centers[rng.integers(0, n_spk, n)] + noise * rng.standard_normal((n, d))
    y *= np.sqrt(d) / np.linalg.norm(y, axis=1, keepdims=True)
    return y.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _rows(d):
    rng = np.random.default_rng(100 + d)
    out = [_unit_rows(rng, d, n) for n in SIZES]
    for y in out:
        y.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _model(d):
    """A well-conditioned two-covariance model of dimension d, diagonalised by the product's own fit code."""
    from xvector_amd import backend
    rng = np.random.default_rng(7 + d)
    g = rng.standard_normal((d, d))
    h = rng.standard_normal((d, d))
    W = np.eye(d) + 0.3 * g @ g.T / d
    B = (h * (2.0 * 0.9 ** np.arange(d))) @ h.T / d + 0.05 * np.eye(d)
    return backend.plda_from_covariances(0.1 * rng.standard_normal(d), B, W)


def _launch(d, target, ys, fill=0x00, row0=None, n_rows=None, keep_pca=True):
    """One call on poisoned outputs: -> dict of host arrays (dim, info, eig, pca, psi, map, off) and status."""
    import torch
    from xvector_amd import hiplib
    plda = _model(d)
    G = len(ys)
    y = np.concatenate(ys)
    ld = (d + 3) // 4 * 4 + 4
    yd = torch.zeros((len(y) if n_rows is None else max(n_rows, len(y)), ld), dtype=torch.float32, device="cuda")
    yd[:len(y), :d] = torch.from_numpy(y).cuda()
    if n_rows is not None:
        yd = yd[:n_rows]
    if row0 is None:
        row0 = np.concatenate([[0], np.cumsum([len(a) for a in ys])])
    W, B = plda.covariances()
    f64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")
    out = dict(dim=torch.full((G + 3,), POISON_I, dtype=torch.int32, device="cuda"),
               info=torch.full((G + 3,), POISON_I, dtype=torch.int32, device="cuda"),
               eig=nan(G + 1, d), pca=nan(G + 1, d, d) if keep_pca else None, psi=nan(G + 1, d), map=nan(G + 1, d, d), off=nan(G + 1, d))
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = torch.full((hiplib.pca_plda_groups_workspace_bytes(G, d) + 64,), fill, dtype=torch.uint8, device="cuda")
    hiplib.pca_plda_groups(yd[:, :d], torch.from_numpy(np.asarray(row0, np.int32)).cuda(), d, target, f64(plda.mean), f64(W), f64(B),
                           f64(plda.transform), f64(plda.psi), out["dim"][:G], out["info"][:G], out["eig"], out["pca"], out["psi"],
                           out["map"], out["off"], status, ws)
    host = {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}
    host["status"] = status.cpu().tolist()
    return host


def _valid(host, g, d):
    """The bytes group g owns: what the contract says is written."""
    p = int(host["dim"][g])
    return b"".join([host["dim"][g:g + 1].tobytes(), host["info"][g:g + 1].tobytes(), host["eig"][g].tobytes(),
                     host["pca"][g, :p].tobytes(), host["psi"][g, :p].tobytes(), host["map"][g, :p].tobytes(), host["off"][g, :p].tobytes()])


def _check_untouched(host, g, d, whole):
    p = d if whole else int(host["dim"][g])
    lo = 0 if whole else p
    assert np.all(np.isnan(host["pca"][g, lo:])) and np.all(np.isnan(host["psi"][g, lo:])) and np.all(np.isnan(host["map"][g, lo:]))
    assert np.all(np.isnan(host["off"][g, lo:]))
    if whole:
        assert host["dim"][g] == POISON_I and host["info"][g] == POISON_I and np.all(np.isnan(host["eig"][g]))


@pytest.mark.parametrize("target", TARGETS)
@pytest.mark.parametrize("d", DIMS)
def test_groups_against_reference(d, target):
    plda = _model(d)
    ys = _rows(d)
    G = len(ys)
    host = _launch(d, target, ys)
    assert host["status"] == [0]
    # the guard entries behind the last group keep the poison
    assert np.all(host["dim"][G:] == POISON_I) and np.all(host["info"][G:] == POISON_I)
    assert all(np.all(np.isnan(host[k][G])) for k in ("eig", "pca", "psi", "map", "off"))
    W, B = pca_ref.model_covariances(plda.transform, plda.psi)
    for g, y in enumerate(ys):
        what = "d %d target %g group %d (n %d)" % (d, target, g, len(y))
        est = pca_ref.est_pca(y, target)
        # 1. grp_dim and grp_info
        if est is None:
            assert host["info"][g] == 1 and host["dim"][g] == d, what
            # 4. the fallback holds the global model, as exact copies
            assert np.array_equal(host["map"][g], plda.transform) and np.array_equal(host["psi"][g], plda.psi), what
            assert np.array_equal(host["off"][g], -np.cumsum(plda.transform * plda.mean, axis=1)[:, -1]), what
            assert np.array_equal(host["pca"][g], np.eye(d)) and np.all(host["eig"][g] == 0), what
            continue
        assert len(y) > 1, what
        p = est["p"]
        # the fixture, on the reference alone: the decision is not a coin toss, and (sizeable groups) neither is the subspace
        assert est["margin"] >= 1e-9, (what, est["margin"])
        if len(y) >= 60:
            assert est["gap"] >= 1.001, (what, est["gap"])
        assert host["info"][g] == 0 and host["dim"][g] == p, (what, host["dim"][g], p)
        _check_untouched(host, g, d, False)
        # 2. eigenvalues, orthonormality, residual
        C = est["C"]
        unit = C_BOUND * d * EPS * np.linalg.norm(C, 2)
        lam, A = host["eig"][g], host["pca"][g, :p]
        assert np.all(np.diff(lam) <= 0), what
        assert np.abs(lam - est["eigvals"]).max() <= unit, (what, np.abs(lam - est["eigvals"]).max() / unit)
        assert np.abs(A @ A.T - np.eye(p)).max() <= C_BOUND * d * EPS, (what, np.abs(A @ A.T - np.eye(p)).max() / (C_BOUND * d * EPS))
        assert np.abs(A @ C @ A.T - np.diag(lam[:p])).max() <= unit, (what, np.abs(A @ C @ A.T - np.diag(lam[:p])).max() / unit)
        at = np.argmax(np.abs(A), axis=1)
        assert np.all(A[np.arange(p), at] > 0), what
        # 3. the projected model, from the downloaded A: M+ = M A^T = P_g.  Cholesky's backward error d eps ||W_g|| passes through
        #    L^-1 on both sides, so the identities hold to d eps cond(W_g); the condition is taken as ||W||_2 ||W_g^-1||_2, which
        #    also covers the rounding of A W A^T itself, and diag(psi) carries the scale max(1, psi_1) on top
        Wg, Bg = A @ W @ A.T, A @ B @ A.T
        cond = np.linalg.norm(W, 2) * np.linalg.norm(np.linalg.inv(Wg), 2)
        M, psi, off = host["map"][g, :p], host["psi"][g, :p], host["off"][g, :p]
        Mp = M @ A.T
        bound = C_BOUND * d * EPS * cond
        assert np.abs(Mp @ Wg @ Mp.T - np.eye(p)).max() <= bound, (what, np.abs(Mp @ Wg @ Mp.T - np.eye(p)).max() / bound)
        scale = max(1.0, psi[0])
        assert np.abs(Mp @ Bg @ Mp.T - np.diag(psi)).max() <= bound * scale, (what, np.abs(Mp @ Bg @ Mp.T - np.diag(psi)).max() / bound)
        assert np.all(psi >= 0) and np.all(np.diff(psi) <= 0), what
        want = pca_ref.project(plda.mean, plda.transform, plda.psi, A)
        assert np.abs(psi - want["psi"]).max() <= bound * scale, (what, np.abs(psi - want["psi"]).max() / (bound * scale))
        c_bound = 2 * bound * np.linalg.norm(Mp, 2) * np.linalg.norm(plda.mean)
        assert np.abs(off + Mp @ (A @ plda.mean)).max() <= c_bound, (what, np.abs(off + Mp @ (A @ plda.mean)).max() / c_bound)


@pytest.mark.parametrize("d", [7, 128])
def test_bits_do_not_depend_on_the_batch(d):
    """5. every group's outputs under a permuted batch with a dirty workspace, without the pca output, and alone: the same bytes."""
    ys = _rows(d)
    G = len(ys)
    base = _launch(d, 0.5, ys)
    perm = [3, 0, 4, 2, 1]
    shuffled = _launch(d, 0.5, [ys[g] for g in perm], fill=0xFF)
    again = _launch(d, 0.5, [ys[g] for g in perm], fill=0x7F)
    assert base["status"] == [0] and shuffled["status"] == [0]
    for k, g in enumerate(perm):
        assert _valid(shuffled, k, d) == _valid(base, g, d), (d, g)
        assert _valid(again, k, d) == _valid(base, g, d), (d, g)
        alone = _launch(d, 0.5, [ys[g]], fill=0xA5)
        assert _valid(alone, 0, d) == _valid(base, g, d), (d, g)
    nop = _launch(d, 0.5, ys, keep_pca=False)
    for g in range(G):
        p = int(base["dim"][g])
        assert nop["dim"][g] == p and nop["map"][g, :p].tobytes() == base["map"][g, :p].tobytes()
        assert nop["psi"][g, :p].tobytes() == base["psi"][g, :p].tobytes() and nop["off"][g, :p].tobytes() == base["off"][g, :p].tobytes()


def test_skipped_groups_and_argument_policy():
    """6. a group whose rows lie outside the table sets status and writes nothing; the host refusals launch nothing."""
    import ctypes
    import torch
    from xvector_amd import hiplib
    d = 8
    ys = _rows(d)[:3]                                                # 200, 1, 60 rows
    row0 = [0, 200, 201, 261]
    base = _launch(d, 0.5, ys)
    for what, bad_row0, n_rows in (("rows past the table", [0, 200, 201, 262], 261), ("an empty group", [0, 200, 200, 261], 261),
                                   ("a negative start", [-1, 200, 201, 261], 261)):
        host = _launch(d, 0.5, ys, row0=bad_row0, n_rows=n_rows)
        bad = {"rows past the table": 2, "an empty group": 1, "a negative start": 0}[what]
        assert host["status"] == [1], what
        _check_untouched(host, bad, d, True)
        for g in range(3):
            if g != bad and bad_row0[g:g + 2] == row0[g:g + 2]:
                assert _valid(host, g, d) == _valid(base, g, d), (what, g)
    lib = hiplib.require_gpu()
    plda = _model(d)
    W, B = plda.covariances()
    f64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
    y = torch.from_numpy(np.concatenate(ys)).cuda()
    r0 = torch.from_numpy(np.asarray(row0, np.int32)).cuda()
    model = [f64(a) for a in (plda.mean, W, B, plda.transform, plda.psi)]
    gd = torch.full((3,), POISON_I, dtype=torch.int32, device="cuda")
    gi = torch.full((3,), POISON_I, dtype=torch.int32, device="cuda")
    outs = [torch.full(s, float("nan"), dtype=torch.float64, device="cuda") for s in ((3, d), (3, d, d), (3, d), (3, d, d), (3, d))]
    status = torch.zeros(2, dtype=torch.int32, device="cuda")
    need = hiplib.pca_plda_groups_workspace_bytes(3, d)
    assert need == 3 * 4 * d * d * 8 and hiplib.pca_plda_groups_workspace_bytes(0, d) == 0
    assert hiplib.pca_plda_groups_workspace_bytes(1, hiplib.PCA_MAX_DIM + 1) == 0
    ws = torch.zeros(need + 8, dtype=torch.uint8, device="cuda")
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)

    def call(**kw):
        a = dict(y=P(y), ldy=d, n_rows=261, row0=P(r0), G=3, dim=d, t=0.5, mean=P(model[0]), W=P(model[1]), B=P(model[2]),
                 P=P(model[3]), psi=P(model[4]), gd=P(gd), gi=P(gi), eig=P(outs[0]), pca=P(outs[1]), gpsi=P(outs[2]), gmap=P(outs[3]),
                 goff=P(outs[4]), status=P(status), ws=P(ws), ws_bytes=need)
        a.update(kw)
        return lib.xv_pca_plda_groups_f64(a["y"], a["ldy"], a["n_rows"], a["row0"], a["G"], a["dim"], a["t"], a["mean"], a["W"], a["B"],
                                          a["P"], a["psi"], a["gd"], a["gi"], a["eig"], a["pca"], a["gpsi"], a["gmap"], a["goff"],
                                          a["status"], a["ws"], a["ws_bytes"], hiplib._stream())

    cases = [(k + " NULL", {k: None}, -1) for k in ("y", "row0", "mean", "W", "B", "P", "psi", "gd", "gi", "eig", "gpsi", "gmap", "goff",
                                                    "status", "ws")]
    cases += [("misaligned psi", dict(psi=P(model[4], 4)), -1), ("misaligned map", dict(gmap=P(outs[3], 4)), -1),
              ("misaligned workspace", dict(ws=P(ws, 4)), -1), ("misaligned status", dict(status=P(status, 2)), -1),
              ("G 0", dict(G=0), -1), ("n_rows 0", dict(n_rows=0), -1), ("dim 0", dict(dim=0), -1), ("ldy < dim", dict(ldy=d - 1), -1),
              ("target 0", dict(t=0.0), -1), ("target > 1", dict(t=1.5), -1), ("target NaN", dict(t=float("nan")), -1),
              ("workspace too small", dict(ws_bytes=need - 8), -1), ("dim > XV_PCA_MAX_DIM", dict(dim=hiplib.PCA_MAX_DIM + 1), -2)]
    for what, kw, code in cases:
        assert call(**kw) == code, what
        assert lib.xv_last_error(), what
    torch.cuda.synchronize()
    assert gd.cpu().tolist() == [POISON_I] * 3 and all(bool(torch.isnan(o).all()) for o in outs) and status.cpu().tolist() == [0, 0]
    assert call() == 0 and call(pca=None) == 0
    torch.cuda.synchronize()
    assert gd.cpu().tolist() == base["dim"][:3].tolist() and status.cpu().tolist() == [0, 0]
    # the grouped prepare: sides, counts, ldo
    E = torch.full((261, 16), float("nan"), dtype=torch.float32, device="cuda")

    def prep(**kw):
        a = dict(y=P(y), ldy=d, n_rows=261, row0=P(r0), G=3, max_n=200, dim=d, gd=P(gd), gpsi=P(outs[2]), gmap=P(outs[3]), goff=P(outs[4]),
                 side=hiplib.SIDE_TEST, out=P(E), ldo=16, r=None, status=P(status))
        a.update(kw)
        return lib.xv_backend_prepare_groups_f32(a["y"], a["ldy"], a["n_rows"], a["row0"], a["G"], a["max_n"], a["dim"], a["gd"], a["gpsi"],
                                                 a["gmap"], a["goff"], a["side"], a["out"], a["ldo"], a["r"], a["status"], hiplib._stream())

    cases = [(k + " NULL", {k: None}, -1) for k in ("y", "row0", "gd", "gpsi", "gmap", "goff", "out", "status")]
    cases += [("side PLAIN", dict(side=hiplib.SIDE_PLAIN), -1), ("side COSINE", dict(side=hiplib.SIDE_COSINE), -1),
              ("ldo < 2 dim", dict(ldo=8), -1), ("ldo % 8", dict(ldo=20), -1), ("max_n 0", dict(max_n=0), -1), ("G 0", dict(G=0), -1),
              ("dim > XV_PCA_MAX_DIM", dict(dim=hiplib.PCA_MAX_DIM + 1, ldo=2 * hiplib.PCA_MAX_DIM + 8), -2)]
    for what, kw, code in cases:
        assert prep(**kw) == code, what
    torch.cuda.synchronize()
    assert bool(torch.isnan(E).all()) and status.cpu().tolist() == [0, 0]
    # a group above max_n, and a retained dimension outside [1, dim]: skipped, status set, their rows untouched
    assert prep(max_n=100) == 0
    torch.cuda.synchronize()
    got = E.cpu().numpy()
    assert status.cpu().tolist() == [1, 0] and np.all(np.isnan(got[:200])) and np.all(np.isfinite(got[200:]))
    status.zero_()
    E.fill_(float("nan"))
    gd[1] = d + 1
    assert prep() == 0
    got = E.cpu().numpy()
    assert status.cpu().tolist() == [1, 0] and np.all(np.isnan(got[200])) and np.all(np.isfinite(got[:200])) and np.all(np.isfinite(got[201:]))


@pytest.mark.parametrize("d", [7, 100, 128])
def test_prepare_groups(d):
    """7. the operand rows against pca_ref built from the DOWNLOADED M_g, c_g, psi_g and p_g."""
    import torch
    from xvector_amd import hiplib
    ys = _rows(d)
    G = len(ys)
    host = _launch(d, 0.5, ys)
    y = np.concatenate(ys)
    row0 = np.concatenate([[0], np.cumsum([len(a) for a in ys])]).astype(np.int32)
    yd = torch.from_numpy(y).cuda()
    f64 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    tabs = [torch.from_numpy(host["dim"][:G].copy()).cuda(), f64(host["psi"][:G]), f64(host["map"][:G]), f64(host["off"][:G])]
    tabs[1][torch.isnan(tabs[1])] = 1e300                            # what the kernel must not read
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    kp = (2 * d + 7) // 8 * 8
    runs = {}
    for ldo in (kp, kp + 24):
        for side in (hiplib.SIDE_ENROL, hiplib.SIDE_TEST):
            out = torch.full((len(y) + 1, ldo), float("nan"), dtype=torch.float32, device="cuda")
            r = torch.full((len(y) + 1,), float("nan"), dtype=torch.float32, device="cuda")
            hiplib.backend_prepare_groups(yd, torch.from_numpy(row0).cuda(), max(SIZES), d, *tabs, side, out[:len(y)], r[:len(y)], status)
            runs[ldo, side] = (out.cpu().numpy(), r.cpu().numpy())
            assert np.all(np.isnan(runs[ldo, side][0][-1])) and np.isnan(runs[ldo, side][1][-1])
    assert status.cpu().tolist() == [0]
    for g in range(G):
        p = int(host["dim"][g])
        rows = slice(int(row0[g]), int(row0[g + 1]))
        M, c, psi = host["map"][g, :p], host["off"][g, :p], host["psi"][g, :p]
        M32, c32, psi32 = (a.astype(np.float32).astype(np.float64) for a in (M, c, psi))
        want_e, want_r, want_t = pca_ref.operand_rows(ys[g], M32, c32, psi32)
        z = pca_ref.transform_rows(ys[g], M32, c32, psi32)
        for side, want in ((hiplib.SIDE_ENROL, want_e), (hiplib.SIDE_TEST, want_t)):
            got, r = runs[kp, side]
            wide, r_wide = runs[kp + 24, side]
            assert np.all(got[rows, 2 * p:] == 0) and np.all(wide[rows, 2 * p:] == 0), (d, g)           # exact zeros
            assert got[rows, :2 * p].tobytes() == wide[rows, :2 * p].tobytes() and r[rows].tobytes() == r_wide[rows].tobytes(), (d, g)
            rel = np.linalg.norm(got[rows, :2 * p] - want, axis=1) / np.maximum(np.linalg.norm(want, axis=1), 1e-30)
            assert rel.max() <= 1e-5, (d, g, side, rel.max())
            if side == hiplib.SIDE_ENROL:
                bound = 1e-5 * (np.abs(want_r) + np.sum(np.abs(want_e[:, :p] * z), axis=1) + p)
                assert np.all(np.abs(r[rows] - want_r) <= bound), (d, g, (np.abs(r[rows] - want_r) / bound).max())
            else:
                assert np.all(r[rows] == 0), (d, g)


# ------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------
D, DIM, THRESHOLD = single.D, single.DIM, single.THRESHOLD
RECORDINGS = ((2, 21, 0), (3, 15, 0), (4, 15, 1), (3, 23, 0), (1, 1, 0), (2, 35, 0))


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """test_gpu_diarize's world, smaller: an out-of-domain LDA + PLDA, recordings of planted speakers, one of a single vector."""
    from xvector_amd import backend
    rng = np.random.default_rng(29)
    mix = rng.standard_normal((D, D)) / np.sqrt(D)
    mu = rng.standard_normal(D)
    xo, lo = single._draw(rng, mix, mu, 60, 6)
    xo64 = xo.astype(np.float64)
    t = backend.fit_lda(xo64 - xo64.mean(axis=0), list(lo), DIM).astype(np.float32)
    plda = backend.fit_plda(ref.chain(xo64, xo64.mean(axis=0), t, True), [np.flatnonzero(lo == s) for s in range(60)])
    mu_in = mu + 0.5 * rng.standard_normal(D)
    xs, spk, sizes = [], [], []
    for n_spk, n_utt, drop in RECORDINGS:
        x, l = single._draw(rng, mix, mu_in, n_spk, n_utt)
        keep = rng.permutation(len(x))[:len(x) - drop]
        xs.append(x[keep]); spk.append(l[keep]); sizes.append(len(keep))
    x = np.concatenate(xs)
    mean_in = x.astype(np.float64).mean(axis=0).astype(np.float32)
    return dict(t=t, plda=plda, x=x, spk=spk, sizes=sizes, mean_in=mean_in, p=str(tmp_path_factory.mktemp("diar_pca")))


@pytest.mark.parametrize("target", [0.1, 0.5])
def test_score_blocks_against_fp64(world, target):
    """8. the blocks against the all-fp64 reference with its own eigh basis (the LLR does not depend on the basis inside the
    retained subspace).  The reference starts from the fp32 rows the PCA kernel read, the device's own PLAIN prepare."""
    from xvector_amd import backend, hiplib
    x, sizes, t, plda, mean_in = (world[k] for k in ("x", "sizes", "t", "plda", "mean_in"))
    scores, tables = backend.score_blocks(x, sizes, plda, mean_in, t, target_energy=target)
    assert tables.status.cpu().tolist() == [0]
    G = len(sizes)
    pca = tables.pca.cpu().numpy()
    Y, _ = backend.prepare(x, hiplib.SIDE_PLAIN, None, mean_in, t, None, True)
    Y = Y.cpu().numpy()[:, :DIM]
    got = scores.cpu().numpy()
    kpad = backend.kpad_for(2 * DIM)
    at = 0
    for g, n in enumerate(sizes):
        y = Y[at:at + n]
        at += n
        want, p = pca_ref.llr_matrix(y, plda.mean, plda.transform, plda.psi, target)
        est = pca_ref.est_pca(y, target)
        assert pca[g] == p and pca[G + g] == (1 if est is None else 0), g
        if est is not None:
            assert est["margin"] >= 1e-9 and est["gap"] >= 1.001, (g, est["margin"], est["gap"])
            gm = pca_ref.project(plda.mean, plda.transform, plda.psi, est["A"])
            M, c, psi = gm["transform"] @ est["A"], -(gm["transform"] @ gm["mean"]), gm["psi"]
        else:
            M, c, psi = plda.transform, -(plda.transform @ plda.mean), plda.psi
        e, r, tt = pca_ref.operand_rows(y, M, c, psi)
        z = pca_ref.transform_rows(y, M, c, psi)
        r_bound = 1e-5 * (np.abs(r) + np.sum(np.abs(e[:, :p] * z), axis=1) + p)
        bound = (2e-5 + 4 * kpad * 2.0 ** -24) * (np.abs(r)[:, None] + np.abs(e) @ np.abs(tt).T) + r_bound[:, None]
        blk = tables.block(got, g).astype(np.float64)
        assert np.all(np.abs(blk - want) <= bound), (g, n, p, (np.abs(blk - want) / bound).max())


def test_diarize_with_pca(world):
    from xvector_amd import backend
    x, sizes, spk, t, plda, mean_in = (world[k] for k in ("x", "sizes", "spk", "t", "plda", "mean_in"))
    counts = [r[0] for r in RECORDINGS]
    report = {}
    labels, merges = backend.diarize(x, sizes, plda, mean=mean_in, transform=t, num_spk=counts, target_energy=0.5, pca_report=report)
    for g, lab in enumerate(np.split(labels, np.cumsum(sizes)[:-1])):
        assert single._partition(lab) == single._partition(spk[g]), "recording %d" % g
    assert report["info"].tolist() == [0, 0, 0, 0, 1, 0] and report["dim"][4] == DIM and np.all(report["dim"][:4] < DIM)
    # the default is the route without a PCA, byte for byte
    base = backend.diarize(x, sizes, plda, mean=mean_in, transform=t, threshold=THRESHOLD)
    same = backend.diarize(x, sizes, plda, mean=mean_in, transform=t, threshold=THRESHOLD, target_energy=1.0)
    near = backend.diarize(x, sizes, plda, mean=mean_in, transform=t, threshold=THRESHOLD, target_energy=0.9995)
    for other in (same, near):
        assert other[0].tobytes() == base[0].tobytes()
        assert all(a.tobytes() == b.tobytes() and a.dtype == b.dtype for m, n in zip(other[1], base[1]) for a, b in zip(m, n))
    with pytest.raises(ValueError):
        backend.diarize(x, sizes, plda, mean=mean_in, transform=t, target_energy=0.0)
    big = backend.plda_from_covariances(np.zeros(130), np.eye(130) * 2.0, np.eye(130))
    with pytest.raises(ValueError, match="128"):
        backend.score_blocks(np.zeros((4, 130), np.float32), [4], big, target_energy=0.5)
    # the tables cut into calls of one group each: the same blocks
    one = backend.score_blocks(x, sizes, plda, mean_in, t, target_energy=0.5)[0].cpu().numpy()
    per = 8 * (3 * DIM + DIM * DIM) + 4 * DIM * DIM * 8
    assert [c for c in backend.plan_pca_groups(len(sizes), DIM, per)[1]] == [(g, g + 1) for g in range(len(sizes))]
    cut = backend.score_blocks(x, sizes, plda, mean_in, t, target_energy=0.5, pca_max_bytes=per)[0].cpu().numpy()
    assert one.tobytes() == cut.tobytes()


def test_cli_route(world, caplog):
    """9. `plda_backend.py diarize --target-energy 0.5` writes labels and an RTTM, and says what the PCA kept."""
    import kaldi_io
    import plda_backend
    from xvector_amd import backend
    p = world["p"]
    sizes = world["sizes"]
    n = sum(sizes)
    reco_of = np.repeat(np.arange(len(sizes)), sizes)
    within = np.concatenate([np.arange(m) for m in sizes])
    keys = ["reco%d-%04d" % (reco_of[i], within[i]) for i in range(n)]
    with open(p + "/segments", "w") as f:
        f.write("".join("%s reco%d %.2f %.2f\n" % (keys[i], reco_of[i], 0.75 * within[i], 0.75 * within[i] + 1.5) for i in range(n)))
    with kaldi_io.TableWriter(p + "/xvector.ark", p + "/xvector.scp") as w:
        kaldi_io.write_vec_flt_batch(w, keys, list(world["x"]))
    backend.write_transform(p + "/transform.mat", world["t"])
    backend.write_plda(p + "/plda", world["plda"])
    kaldi_io.write_vec_flt(p + "/mean.vec", world["mean_in"])
    with open(p + "/reco2num_spk", "w") as f:
        f.write("".join("reco%d %d\n" % (g, r[0]) for g, r in enumerate(RECORDINGS)))
    common = ["--mean", p + "/mean.vec", "--lda", p + "/transform.mat", "--reco2num-spk", p + "/reco2num_spk"]
    tail = [p + "/plda", "scp:" + p + "/xvector.scp", p + "/segments"]
    with caplog.at_level("INFO", logger="plda_backend"):
        plda_backend.main(["diarize"] + common + ["--target-energy", "0.5", "--rttm", p + "/pca.rttm"] + tail + [p + "/labels_pca"])
    report = {}
    labels, _ = backend.diarize(world["x"], sizes, world["plda"], mean=world["mean_in"], transform=world["t"],
                                num_spk=[r[0] for r in RECORDINGS], target_energy=0.5, pca_report=report)
    want = []
    for g, lab in enumerate(np.split(labels, np.cumsum(sizes)[:-1])):
        want += plda_backend.number_labels(lab)
    assert open(p + "/labels_pca").read() == "".join("%s %d\n" % (k, l) for k, l in zip(keys, want))
    assert open(p + "/pca.rttm").read().startswith("SPEAKER reco0 0 ")
    line = ("Per-recording PCA at target energy 0.5: mean retained dimension %.2f of %d; 1 recordings fell back to the global model "
            "(1 without energy, 0 without convergence)" % (float(report["dim"].mean()), DIM))
    assert line in caplog.text
    caplog.clear()
    with caplog.at_level("INFO", logger="plda_backend"):
        plda_backend.main(["diarize"] + common + ["--target-energy", "1.0"] + tail + [p + "/labels_one"])
        plda_backend.main(["diarize"] + common + tail + [p + "/labels_default"])
    assert "Per-recording PCA" not in caplog.text
    assert open(p + "/labels_one").read() == open(p + "/labels_default").read()
    assert os.path.exists(p + "/labels_pca") and not os.path.exists(p + "/labels_pca.tmp")
