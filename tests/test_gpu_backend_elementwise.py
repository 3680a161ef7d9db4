"""The three kernels behind every PLDA / cosine score (csrc/xv_backend.hip: backend_prepare_kernel, score_matrix_kernel,
score_pairs_kernel) on the MI355X, element by element.

The scorers are held to the bits of the order the header promises (one accumulator, an fmaf chain with k ascending from 0, then
`+ r`), restated on the CPU with an exact fp32 fma, and to exact known answers that do not depend on that fma (integer operands,
one-hot rows).  prepare is held (a) to the bits of its products, (b) to exact known answers, (c) on realistic data to per-element
bounds against the fp64 reference, propagated stage by stage, and (d) to its refusals.  Data, replays, bounds and assertion
functions: tests/backend_data.py; their CPU companion (what the replay reaches, what the mutants do): test_backend_bounds_cpu.py.

Every output is NaN-poisoned with sentinel rows and columns behind it, every device call runs twice and the two results are
compared in every bit, and every operand is a slice of a wider NaN-filled buffer."""
import ctypes

import numpy as np
import pytest

import backend_data as bd

pytestmark = pytest.mark.gpu

WORST = {}
BAD_ARG, UNSUPPORTED = -1, -2
F = np.float32
NAN = float("nan")


def _note(key, value):
    WORST[key] = max(WORST.get(key, 0.0), float(value))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if WORST:
        print("\nworst |device - ref| / bound per prepare case family (rows, r), LAMBDA = %d:" % bd.LAMBDA)
        for k in WORST:
            print("  %-32s %.3e" % (k, WORST[k]))


# ---------------------------------------------------------------------------------------------------------------------------
# device plumbing
# ---------------------------------------------------------------------------------------------------------------------------
def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, copy=True, order="C")).to("cuda:0")   # (shared arrays are read-only)


def _slice_of_nan(a, pad_cols, col0=0):
    """a[R, C] as the slice [:R, col0:col0 + C] of a NaN-filled [R + 1, C + pad_cols] device buffer."""
    import torch
    rows, cols = a.shape
    assert col0 <= pad_cols
    parent = torch.full((rows + 1, cols + pad_cols), NAN, dtype=torch.float32, device="cuda:0")
    view = parent[:rows, col0:col0 + cols]
    view.copy_(_dev(a))
    assert view.stride(0) == cols + pad_cols
    return view


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _scorer_operands(E, T, r):
    return _slice_of_nan(E, 8), _slice_of_nan(T, 8), _dev(r)


def _score_matrix(Ed, Td, rd):
    """S[Ne, Nt] from a NaN-filled [Ne + 2, roundup(Nt, 4) + 4] buffer; two runs with the same bits; nothing else written."""
    import torch
    from xvector_amd import hiplib
    ne, nt = Ed.shape[0], Td.shape[0]
    runs = []
    for _ in range(2):
        S = torch.full((ne + 2, bd.roundup(nt, 4) + 4), NAN, dtype=torch.float32, device="cuda:0")
        hiplib.score_matrix(Ed, Td, rd, S)
        runs.append(S.cpu().numpy())
    assert _same_bits(runs[0], runs[1]), "two runs of score_matrix differ"
    S = runs[0]
    assert np.isnan(S[ne:]).all() and np.isnan(S[:ne, nt:]).all(), "score_matrix wrote outside [Ne, Nt]"
    return S[:ne, :nt]


def _score_pairs(Ed, Td, rd, ei, ti):
    import torch
    from xvector_amd import hiplib
    m = len(ei)
    eid, tid = _dev(ei), _dev(ti)
    runs = []
    for _ in range(2):
        out = torch.full((m + 8,), NAN, dtype=torch.float32, device="cuda:0")
        hiplib.score_pairs(Ed, Td, rd, eid, tid, out)
        runs.append(out.cpu().numpy())
    assert _same_bits(runs[0], runs[1]), "two runs of score_pairs differ"
    assert np.isnan(runs[0][m:]).all(), "score_pairs wrote past its list"
    return runs[0][:m]


def _check_scorers(case, what, pair_counts=bd.PAIR_COUNTS):
    E, T, r = case["E"], case["T"], case["r"]
    ne, nt = E.shape[0], T.shape[0]
    Ed, Td, rd = _scorer_operands(E, T, r)
    bd.assert_bits_equal(_score_matrix(Ed, Td, rd), case["want_r"], what + " score_matrix")
    bd.assert_bits_equal(_score_matrix(Ed, Td, None), case["want_0"], what + " score_matrix r=None")
    for m in pair_counts:
        ei, ti = bd.pair_list(m, ne, nt)
        bd.assert_bits_equal(_score_pairs(Ed, Td, rd, ei, ti), case["want_r"][ei, ti], what + " score_pairs M=%d" % m)
    ei, ti = bd.pair_list(pair_counts[-1], ne, nt, seed=1)
    bd.assert_bits_equal(_score_pairs(Ed, Td, None, ei, ti), case["want_0"][ei, ti], what + " score_pairs r=None")


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the scorers, bit for bit against the documented order
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kpad", bd.KPADS)
@pytest.mark.parametrize("dataset", bd.DATASETS)
def test_scorers_have_the_documented_bits(dataset, kpad):
    """One to four 8-k groups in the last 32-k slice, one, two and many slices (the register prefetch across them), at
    (Ne, Nt) = (129, 131): a full 128-tile and a one-row / three-column edge tile on either side."""
    _check_scorers(bd.scorer_case(dataset, kpad, 129, 131), "%s kpad %d" % (dataset, kpad))


@pytest.mark.parametrize("ne,nt", bd.EDGE_SHAPES)
@pytest.mark.parametrize("kpad", [40, 200])
def test_scorers_have_the_documented_bits_at_tile_edges(kpad, ne, nt):
    for dataset in ("plda", "normal"):
        _check_scorers(bd.scorer_case(dataset, kpad, ne, nt), "%s kpad %d %d x %d" % (dataset, kpad, ne, nt), pair_counts=(1, 257))


@pytest.mark.parametrize("kpad", bd.KPADS)
def test_scorers_exact_on_integers(kpad):
    E, T, r = bd.integer_operands(kpad, 129, 131)
    Ed, Td, rd = _scorer_operands(E, T, r)
    bd.assert_integer_scores(_score_matrix(Ed, Td, rd), E, T, r, "score_matrix kpad %d" % kpad)
    bd.assert_integer_scores(_score_matrix(Ed, Td, None), E, T, None, "score_matrix r=None kpad %d" % kpad)
    ei, ti = bd.pair_list(5000, 129, 131)
    want = E.astype(np.float64) @ T.astype(np.float64).T + r[:, None]
    assert np.array_equal(_score_pairs(Ed, Td, rd, ei, ti).astype(np.float64), want[ei, ti])


def test_scorers_exact_on_integers_large():
    """1000 x 2049 x 1024: eight row tiles, seventeen column tiles with a one-column edge, 32 slices; the reference is a matmul."""
    E, T, r = bd.integer_operands(1024, 1000, 2049)
    Ed, Td, rd = _scorer_operands(E, T, r)
    bd.assert_integer_scores(_score_matrix(Ed, Td, rd), E, T, r, "score_matrix 1000 x 2049 x 1024")
    ei, ti = bd.pair_list(5000, 1000, 2049)
    want = np.einsum("ik,ik->i", E[ei].astype(np.float64), T[ti].astype(np.float64)) + r[ei]
    assert np.array_equal(_score_pairs(Ed, Td, rd, ei, ti).astype(np.float64), want)


@pytest.mark.parametrize("kpad", bd.KPADS)
def test_scorers_read_every_k_position(kpad):
    """E = identity: S[e, t] == T[t, e] for every k, i.e. every slot of the [k0 k2 k4 k6 | k1 k3 k5 k7] LDS image and every slice;
    then with the roles swapped."""
    eye, other = bd.onehot_operands(kpad, 67)
    Ed, Td, _ = _scorer_operands(eye, other, None)
    bd.assert_onehot_scores(_score_matrix(Ed, Td, None), other, False, "E = I, kpad %d" % kpad)
    bd.assert_onehot_scores(_score_matrix(Td, Ed, None), other, True, "T = I, kpad %d" % kpad)
    ei, ti = np.meshgrid(np.arange(kpad, dtype=np.int32), np.arange(67, dtype=np.int32), indexing="ij")
    got = _score_pairs(Ed, Td, None, ei.ravel(), ti.ravel()).reshape(kpad, 67)
    bd.assert_onehot_scores(got, other, False, "score_pairs E = I, kpad %d" % kpad)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. prepare
# ---------------------------------------------------------------------------------------------------------------------------
def _prepare(case):
    """(rows[N, K], r[N]) of hiplib.backend_prepare.  x is a column slice of a NaN-filled parent (ldx = D + 5), the LDA a column
    slice (ld_lda = D + 3), out has ldo = roundup(K, 8) + 8 and two sentinel rows, r two sentinel elements.  Checked here: two
    runs agree in every bit, columns [K, ldo) are exactly zero, the sentinels are untouched, r is exactly 0 off the enrolment
    side."""
    import torch
    from xvector_amd import hiplib
    x = np.asarray(case["x"], F)
    N, D = x.shape
    A = case.get("A")
    d = D if A is None else A.shape[0]
    side = case["side"]
    K = 2 * d if side in (bd.SIDE_ENROL, bd.SIDE_TEST) else d
    ldo = bd.roundup(K, 8) + 8
    xd = _slice_of_nan(x, 5, 2)
    Ad = None if A is None else _slice_of_nan(A, 3, 1)
    n = case.get("n")
    kw = dict(num_utts=None if n is None else _dev(np.asarray(n, np.int32)), mean=_dev(case.get("mu")), lda=Ad,
              lda_offset=_dev(case.get("a0")), length_norm=case.get("length_norm", True), plda_transform=_dev(case.get("P")),
              plda_mean=_dev(case.get("m")), plda_psi=_dev(case.get("psi")))
    runs = []
    for _ in range(2):
        out = torch.full((N + 2, ldo), NAN, dtype=torch.float32, device="cuda:0")
        rbuf = torch.full((N + 2,), NAN, dtype=torch.float32, device="cuda:0")
        hiplib.backend_prepare(xd, out, side, r=rbuf[:N], **kw)
        runs.append((out.cpu().numpy(), rbuf.cpu().numpy()))
    assert _same_bits(runs[0][0], runs[1][0]) and _same_bits(runs[0][1], runs[1][1]), "two runs of prepare differ: " + case["name"]
    out, rbuf = runs[0]
    assert np.isnan(out[N:]).all() and np.isnan(rbuf[N:]).all(), "prepare wrote past row N: " + case["name"]
    assert np.all(out[:N, K:] == 0), "columns [K, ldo) are not zero: " + case["name"]
    assert np.all(np.isfinite(out[:N, :K])) and np.all(np.isfinite(rbuf[:N])), "non-finite output: " + case["name"]
    if side != bd.SIDE_ENROL:
        assert np.all(rbuf[:N] == 0), "r must be 0 off the enrolment side: " + case["name"]
    return out[:N, :K], rbuf[:N]


# ---- (a) the products, bit for bit ----
@pytest.mark.parametrize("D,d,N", bd.SHAPES)
def test_prepare_products_have_the_fmaf_chain_bits(D, d, N):
    """PLAIN, no PLDA, no length norm: with an LDA the output is the fmaf chain over k ascending of (x - mu) A from 0, then + a0;
    without one it is x - mu."""
    for lda in (True, False):
        case = bd.product_case(D, d, N, lda)
        rows, _ = _prepare(case)
        bd.assert_bits_equal(rows, bd.prepare_replay(case)[0], case["name"])
    bare = bd.product_case(D, d, N, True, seed=6)          # mu == NULL and a0 == NULL: the chain of x A alone
    del bare["mu"], bare["a0"]
    bd.assert_bits_equal(_prepare(bare)[0], bd.prepare_replay(bare)[0], bare["name"] + " bare")


@pytest.mark.parametrize("D,N", [(1, 1), (2, 31), (31, 32), (33, 33), (64, 97), (65, 1), (150, 31), (600, 32), (2048, 33)])
def test_prepare_one_hot_lda_reads_every_k(D, N):
    case, want = bd.onehot_lda_case(D, N)
    rows, _ = _prepare(case)
    bad = rows != want
    assert not bad.any(), (case["name"], int(bad.sum()), tuple(int(i[0]) for i in np.nonzero(bad)))


# ---- (b) exact known answers ----
@pytest.mark.parametrize("D,d,N", bd.SHAPES)
def test_prepare_integer_lda_exact(D, d, N):
    case, want = bd.integer_lda_case(D, d, N)
    rows, _ = _prepare(case)
    bad = rows.astype(np.float64) != want
    assert not bad.any(), (case["name"], int(bad.sum()), tuple(int(i[0]) for i in np.nonzero(bad)))


@pytest.mark.parametrize("d,N", [(s[1], s[2]) for s in bd.SHAPES])
def test_prepare_plda_step_exact(d, N):
    """A signed permutation for P, psi + 1/n in {1, 4, 16} and z = +-sqrt(psi + 1): the norm sum is d in any order, the scale 1."""
    case, z = bd.exact_plda_case(d, N, bd.SIDE_PLAIN)
    bd.assert_bits_equal(_prepare(case)[0], z, case["name"])
    case["side"] = bd.SIDE_TEST
    bd.assert_bits_equal(_prepare(case)[0], np.hstack([z, F(-0.5) * z * z]), case["name"] + " TEST")
    case["side"] = bd.SIDE_ENROL
    rows, r = _prepare(case)
    zero = case["psi"] == 0
    assert np.all(rows[:, :d][:, zero] == 0) and np.all(rows[:, d:][:, zero] == 0), case["name"] + " ENROL psi = 0 columns"
    wr = bd.assert_prepare_within(rows, r, bd.prepare_bounds(case), case["name"] + " ENROL")
    _note("exact_plda enrol rows", wr[0]); _note("exact_plda enrol r", wr[1])


@pytest.mark.parametrize("combo", ["plain_lda", "cosine_raw", "full_cosine", "full_enrol", "raw_test", "plain_plda"])
@pytest.mark.parametrize("D,d,N", [(33, 32, 33), (150, 129, 97), (64, 65, 2)])
def test_prepare_zero_vector(combo, D, d, N):
    """An all-zero vector stays exactly zero through the length norm and the cosine packing (no NaN); with a PLDA it is the
    finite P(-m) chain of the reference."""
    case = bd.zero_vector_case(combo, D, d, N)
    rows, r = _prepare(case)
    if case.get("P") is None:
        assert np.all(rows[0] == 0) and np.all(rows[-1] == 0), case["name"]
    wr = bd.assert_prepare_within(rows, r, bd.prepare_bounds(case), case["name"])
    _note("zero_vector rows", wr[0]); _note("zero_vector r", wr[1])


# ---- (c) realistic data, element by element against the fp64 reference ----
@pytest.mark.parametrize("D,d,N", bd.SHAPES)
def test_prepare_within_elementwise_bounds(D, d, N):
    for combo in bd.COMBOS:
        case = bd.realistic_case(combo, D, d, N)
        rows, r = _prepare(case)
        wr = bd.assert_prepare_within(rows, r, bd.prepare_bounds(case), case["name"])
        _note(combo + " rows", wr[0])
        if case["side"] == bd.SIDE_ENROL:
            _note(combo + " r", wr[1])
        if combo == "enrol_no_counts":                       # num_utts = NULL is counts of 1, in every bit
            ones = dict(case, n=np.ones(N, np.int32))
            rows1, r1 = _prepare(ones)
            bd.assert_bits_equal(rows, rows1, case["name"] + " against counts of 1")
            bd.assert_bits_equal(r, r1, case["name"] + " r against counts of 1")


# ---- (d) refusals launch nothing ----
def _vp(t, offset=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + offset)


def test_prepare_refusals_launch_nothing():
    import torch
    from xvector_amd import hiplib
    lib = hiplib.require_gpu()
    N, D, d = 4, 16, 8
    x = torch.ones((N, 2056), dtype=torch.float32, device="cuda:0")
    A = torch.ones((260, 2056), dtype=torch.float32, device="cuda:0")
    vec = torch.ones((2056,), dtype=torch.float32, device="cuda:0")
    P = torch.eye(260, dtype=torch.float32, device="cuda:0")
    out = torch.full((N + 2, 528), NAN, dtype=torch.float32, device="cuda:0")
    r = torch.full((N + 2,), NAN, dtype=torch.float32, device="cuda:0")

    def call(ldx=2056, dim_in=D, lda=A, ld_lda=2056, dim=d, P_=None, m_=None, psi_=None, side=bd.SIDE_PLAIN, ldo=16):
        return lib.xv_backend_prepare_f32(_vp(x), ldx, N, dim_in, None, _vp(vec), _vp(lda), ld_lda, _vp(vec), dim, 1, _vp(P_), _vp(m_),
                                          _vp(psi_), side, _vp(out), ldo, _vp(r), None)

    rows = ((dict(ldo=12), BAD_ARG), (dict(ldo=4), BAD_ARG), (dict(ldo=0), BAD_ARG),                 # not a multiple of 8; below K
            (dict(side=bd.SIDE_TEST, P_=P, m_=vec, psi_=vec, ldo=8), BAD_ARG),                        # K = 16 > ldo
            (dict(P_=P), BAD_ARG), (dict(m_=vec, psi_=vec), BAD_ARG), (dict(P_=P, m_=vec), BAD_ARG),   # a partial PLDA
            (dict(side=bd.SIDE_ENROL), BAD_ARG), (dict(side=bd.SIDE_TEST), BAD_ARG),                   # no PLDA
            (dict(ld_lda=D - 1), BAD_ARG),
            (dict(lda=None, ld_lda=0, dim=d), BAD_ARG),                                                # no LDA, dim != dim_in
            (dict(dim_in=2049), UNSUPPORTED),
            (dict(dim=257, ldo=264), UNSUPPORTED),
            (dict(lda=None, ld_lda=0, dim_in=257, dim=257, ldo=264), UNSUPPORTED))
    for kw, code in rows:
        assert call(**kw) == code, kw
        assert len(lib.xv_last_error()) > 10, kw
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(r).all())          # nothing ran
    assert call() == 0
    torch.cuda.synchronize()
    flat = out.cpu().numpy().ravel()                                            # the rows lie ldo = 16 apart
    got = flat[:N * 16].reshape(N, 16)
    assert np.all(got[:, :d] == 1) and np.all(got[:, d:] == 0) and np.isnan(flat[N * 16:]).all()
    assert np.all(r.cpu().numpy()[:N] == 0) and np.isnan(r.cpu().numpy()[N:]).all()


def test_scorer_refusals_launch_nothing():
    import torch
    from xvector_amd import hiplib
    lib = hiplib.require_gpu()
    ne, nt, kpad, ldk = 4, 5, 16, 24
    E = torch.ones((ne + 1, 1048), dtype=torch.float32, device="cuda:0")
    T = torch.ones((nt + 1, 1048), dtype=torch.float32, device="cuda:0")
    r = torch.ones((ne,), dtype=torch.float32, device="cuda:0")
    S = torch.full((ne + 2, 8), NAN, dtype=torch.float32, device="cuda:0")
    idx = torch.zeros((6,), dtype=torch.int32, device="cuda:0")
    po = torch.full((8,), NAN, dtype=torch.float32, device="cuda:0")

    def matrix(kpad=kpad, ldk=ldk, lds=8, eoff=0, toff=0):
        return lib.xv_score_matrix_f32(_vp(E, eoff), _vp(T, toff), ldk, kpad, ne, nt, _vp(r), _vp(S), lds, None)

    def pairs(kpad=kpad, ldk=ldk, eoff=0, toff=0):
        return lib.xv_score_pairs_f32(_vp(E, eoff), _vp(T, toff), ldk, kpad, _vp(idx), _vp(idx), 6, _vp(r), _vp(po), None)

    rows = ((dict(kpad=12), BAD_ARG), (dict(kpad=0), BAD_ARG), (dict(kpad=1032, ldk=1048), UNSUPPORTED), (dict(ldk=18), BAD_ARG),
            (dict(ldk=8), BAD_ARG), (dict(eoff=4), BAD_ARG), (dict(toff=8), BAD_ARG))
    for kw, code in rows:
        for fn in (matrix, pairs):
            assert fn(**kw) == code, (fn.__name__, kw)
            assert len(lib.xv_last_error()) > 10, kw
    assert matrix(lds=nt - 1) == BAD_ARG and len(lib.xv_last_error()) > 10
    torch.cuda.synchronize()
    assert bool(torch.isnan(S).all()) and bool(torch.isnan(po).all())           # nothing ran
    assert matrix() == 0 and pairs() == 0
    torch.cuda.synchronize()
    got = S.cpu().numpy()
    assert np.all(got[:ne, :nt] == kpad + 1) and np.isnan(got[ne:]).all() and np.isnan(got[:ne, nt:]).all()
    assert np.all(po.cpu().numpy()[:6] == kpad + 1) and np.isnan(po.cpu().numpy()[6:]).all()
