"""xv_moment_stats_f64 on the MI355X: sum_i x_i and sum_i x_i x_i^T in fp64 on the f64 MFMA.  Exact on integer
data at the edges of the 16 x 16 x 4 tile and of the slab, within the order-independent summation bound on general data, exactly
symmetric, and bit-identical whatever the strides, the call before or the chunking of backend.moment_stats."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def _slab():
    from xvector_amd import hiplib
    return hiplib.MOMENT_SLAB


def _run(x, pad_x=4, pad_o=5, tail=3):
    """The kernel on x[n, dim] held in a buffer of row stride ceil4(dim) + pad_x whose padding columns are NaN; sum and outer
    are allocated `tail` elements / rows and pad_o columns longer and pre-filled with NaN.  -> (sum, outer) and checks that
    everything outside sum[0, dim) and the dim x dim block of outer is still NaN."""
    import torch
    from xvector_amd import hiplib
    n, dim = x.shape
    ldx = (dim + 3) // 4 * 4 + pad_x
    buf = np.full((n, ldx), np.nan, np.float32)
    buf[:, :dim] = x
    xd = torch.as_tensor(buf, device="cuda:0")
    s = torch.full((dim + tail,), float("nan"), dtype=torch.float64, device="cuda:0")
    o = torch.full((dim + tail, dim + pad_o), float("nan"), dtype=torch.float64, device="cuda:0")
    hiplib.moment_stats(xd, s, o, dim=dim)
    s, o = s.cpu().numpy(), o.cpu().numpy()
    assert np.all(np.isnan(s[dim:])) and np.all(np.isnan(o[dim:])) and np.all(np.isnan(o[:, dim:])), "wrote outside the result"
    return s[:dim].copy(), o[:dim, :dim].copy()


def _cases():
    from xvector_amd import hiplib
    S = hiplib.MOMENT_SLAB                                 # = XV_MOMENT_SLAB of the header (tests/test_moment_constants.py)
    ns = [1, 3, 4, 5, S - 1, S, S + 1, 3 * S + 7]
    dims = [1, 5, 16, 17, 100, 200, 256]
    pairs = set()
    for i, d in enumerate(dims):                           # every dim with three row counts, every row count with >= 2 dims
        for k in (0, 3, 5):
            pairs.add((d, ns[(i + k) % len(ns)]))
    pairs |= {(256, 3 * S + 7), (17, 3 * S + 7), (1, 1), (200, S + 1), (100, S - 1), (5, 4)}
    return sorted(pairs)


@pytest.mark.parametrize("dim,n", _cases())
def test_exact_on_integers(dim, n):
    rng = np.random.default_rng(dim * 100003 + n)
    xi = rng.integers(-64, 65, size=(n, dim)).astype(np.int64)
    s, o = _run(xi.astype(np.float32))
    assert np.array_equal(s, xi.sum(axis=0).astype(np.float64))
    assert np.array_equal(o, (xi.T @ xi).astype(np.float64))


def _general(kind, n, dim, seed):
    rng = np.random.default_rng(seed)
    if kind == "scales":
        x = rng.standard_normal((n, dim)) * 10.0 ** rng.uniform(-3, 3, size=(n, 1))
    else:
        x = 100.0 + rng.standard_normal((n, dim))
    return x.astype(np.float32)


@pytest.mark.parametrize("kind", ["scales", "offset"])
@pytest.mark.parametrize("n,dim", [(5000, 100), (4173, 37)])
def test_general_within_the_summation_bound(kind, n, dim):
    """|outer - x64^T x64| <= 2 n u sum_i |x_ij| |x_ik| (u = 2^-53): the order-independent bound of a length-n fp64 sum of
    exact products, once for the kernel and once for the NumPy reference; the same for sum with sum_i |x_ij|."""
    x = _general(kind, n, dim, 7 * n + dim)
    s, o = _run(x)
    x64 = x.astype(np.float64)
    ax = np.abs(x64)
    bound_o = 2.0 * n * U * (ax.T @ ax)
    bound_s = 2.0 * n * U * ax.sum(axis=0)
    ro = (np.abs(o - x64.T @ x64) / bound_o).max()
    rs = (np.abs(s - x64.sum(axis=0)) / bound_s).max()
    print("moments [%s n=%d d=%d]: worst |diff| / bound = %.3e (outer), %.3e (sum)" % (kind, n, dim, ro, rs))
    assert ro <= 1.0 and rs <= 1.0
    assert np.array_equal(o, o.T)


def test_structure_and_reproducibility():
    import torch
    from xvector_amd import hiplib
    n, dim = 2 * _slab() + 301, 50
    x = _general("offset", n, dim, 11)
    s0, o0 = _run(x)
    assert np.array_equal(o0, o0.T)
    s1, o1 = _run(x)                                       # twice
    assert np.array_equal(s0, s1) and np.array_equal(o0, o1)
    s2, o2 = _run(x, pad_x=0, pad_o=0, tail=0)             # other strides
    assert np.array_equal(s0, s2) and np.array_equal(o0, o2)
    s3, o3 = _run(x, pad_x=64, pad_o=11, tail=1)
    assert np.array_equal(s0, s3) and np.array_equal(o0, o3)
    _run(_general("scales", 3 * _slab() + 5, 200, 12))        # an unrelated launch of another size in between
    s4, o4 = _run(x)
    assert np.array_equal(s0, s4) and np.array_equal(o0, o4)
    # a larger workspace than needed, filled with NaN: every word that is read is written first
    xd = torch.as_tensor(np.ascontiguousarray(np.pad(x, ((0, 0), (0, 2)))), device="cuda:0")
    ws = torch.full((hiplib.moment_stats_workspace_bytes(n, dim) // 8 + 1000,), float("nan"), dtype=torch.float64, device="cuda:0")
    s = torch.empty(dim, dtype=torch.float64, device="cuda:0")
    o = torch.empty((dim, dim), dtype=torch.float64, device="cuda:0")
    hiplib.moment_stats(xd, s, o, dim=dim, workspace=ws)
    assert np.array_equal(s.cpu().numpy(), s0) and np.array_equal(o.cpu().numpy(), o0)


def test_backend_moment_stats_chunks(monkeypatch):
    import torch
    from xvector_amd import backend, hiplib
    n, dim, chunk = 12345, 33, 5000
    monkeypatch.setattr(backend, "MOMENT_CHUNK_ROWS", chunk)
    x = _general("offset", n, dim, 21)
    xd = torch.as_tensor(np.ascontiguousarray(np.pad(x, ((0, 0), (0, 7)))), device="cuda:0")      # row stride 40
    got_n, got_s, got_o = backend.moment_stats(xd, dim)
    want_s, want_o = np.zeros(dim), np.zeros((dim, dim))
    s = torch.empty(dim, dtype=torch.float64, device="cuda:0")
    o = torch.empty((dim, dim), dtype=torch.float64, device="cuda:0")
    for i0 in range(0, n, chunk):
        hiplib.moment_stats(xd[i0:i0 + chunk], s, o, dim=dim)
        want_s += s.cpu().numpy()
        want_o += o.cpu().numpy()
    assert got_n == n and np.array_equal(got_s, want_s) and np.array_equal(got_o, want_o)
    h_n, h_s, h_o = backend.moment_stats(x, dim)           # a host array goes the same way, chunk by chunk
    assert h_n == n and np.array_equal(h_s, want_s) and np.array_equal(h_o, want_o)
    x64 = x.astype(np.float64)
    assert np.allclose(got_o, x64.T @ x64, rtol=1e-12, atol=0) and np.allclose(got_s, x64.sum(axis=0), rtol=1e-12, atol=0)
    with pytest.raises(ValueError):
        backend.moment_stats(x[:0], dim)
    with pytest.raises(ValueError):
        backend.moment_stats(np.zeros((4, 300), np.float32))


def test_argument_errors_launch_nothing():
    import torch
    from xvector_amd import hiplib
    lib = hiplib.require_gpu()
    n, dim, ldx = 100, 20, 24
    x = torch.ones((n, ldx), dtype=torch.float32, device="cuda:0")
    s = torch.full((dim,), float("nan"), dtype=torch.float64, device="cuda:0")
    o = torch.full((dim, dim), float("nan"), dtype=torch.float64, device="cuda:0")
    need = hiplib.moment_stats_workspace_bytes(n, dim)
    assert need > 0 and hiplib.moment_stats_workspace_bytes(0, dim) == 0 and hiplib.moment_stats_workspace_bytes(n, 257) == 0
    ws = torch.zeros(need + 1024, dtype=torch.uint8, device="cuda:0")
    vp = lambda t: ctypes.c_void_p(t.data_ptr())          # noqa: E731

    def call(n_rows=n, d=dim, ld=ldx, ldo=dim, wsb=need, xp=None):
        return lib.xv_moment_stats_f64(vp(x) if xp is None else xp, ld, n_rows, d, vp(s), vp(o), ldo, vp(ws), wsb, None)

    BAD, UNSUP = -1, -2
    for kw, code in ((dict(d=0), UNSUP), (dict(d=257, ld=260, ldo=260), UNSUP), (dict(n_rows=0), BAD), (dict(ld=16), BAD),
                     (dict(ldo=dim - 1), BAD), (dict(wsb=need - 8), BAD), (dict(wsb=0), BAD), (dict(ld=ldx + 1), BAD),
                     (dict(xp=ctypes.c_void_p(x.data_ptr() + 4)), BAD)):
        assert call(**kw) == code, kw
        assert len(lib.xv_last_error()) > 10, kw
    torch.cuda.synchronize()
    assert bool(torch.isnan(s).all()) and bool(torch.isnan(o).all())          # nothing ran
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(s.cpu().numpy(), np.full(dim, float(n))) and np.array_equal(o.cpu().numpy(), np.full((dim, dim), float(n)))
