"""CPU companion of tests/test_gpu_wgrad_elementwise.py: the emulator's weight gradient (tests/arith_emul.py wgrad) is the exact one
on the integer data of the exact cases, and the element-wise bound the GPU test applies has power on the data it uses."""
import numpy as np
import pytest

import arith_emul as em
import wgrad_data as wd

SMALL_EXACT = [c for c in wd.EXACT_CASES if c.R * c.cin * c.cout * c.K <= 5000 * 64 * 64 * 3]


def _splits(case):
    from xvector_amd import hiplib
    return case.splits(hiplib.load().xv_wgrad_workspace_bytes(case.R, case.cin, case.cout, case.K))       # (host code: no GPU needed)


@pytest.mark.parametrize("arith", ["fp32", "bf16x3"])
@pytest.mark.parametrize("case", SMALL_EXACT, ids=[c.name for c in SMALL_EXACT])
def test_emulated_wgrad_is_exact_on_the_integer_data(case, arith):
    x, dz = case.data()
    assert ((x == 0).mean() > 0.3) and ((dz == 0).mean() > 0.3) and (not case.relu or (x >= 0).all())
    ref, dbref = wd.exact_ref(x, dz, case.K, case.dil)
    dw, M = em.wgrad(arith, x, dz, case.K, case.dil)
    assert np.array_equal(dw, ref.astype(np.float64))
    assert (M >= np.abs(dw)).all() and M.max() < 2 ** 24
    reach = (case.K - 1) // 2 * case.dil
    if case.R <= reach:                                        # the taps that reach past the chunk are entirely zero
        h = (case.K - 1) // 2
        dead = [k for k in range(case.K) if abs(k - h) * case.dil >= case.R]
        assert dead and not dw[dead].any()


def test_the_split_cases_are_the_ones_the_library_splits():
    for c in wd.EXACT_CASES:
        s = _splits(c)
        assert (s > 1) == c.name.startswith(wd.SPLIT_CASES), (c.name, s)
        if s > 1:
            assert c.rows_per_split(s) % wd.WR == 0 and (s - 1) * c.rows_per_split(s) < c.R
    last = [c for c in wd.EXACT_CASES if c.name.startswith("R19000")][0]
    s = _splits(last)
    assert (last.R - (s - 1) * last.rows_per_split(s)) % wd.WR != 0          # a last split that is not a whole number of steps


def _sample(n, rng, count=10):
    """Channels a power check looks at: both ends of the range (tile edges) and a few in between."""
    return np.unique(np.concatenate([np.arange(min(n, 4)), np.arange(max(0, n - 3), n), rng.integers(0, n, count)]))


@pytest.mark.parametrize("case", wd.BOUND_CASES, ids=[c.name for c in wd.BOUND_CASES])
def test_wgrad_bounds_have_power(case):
    """On the data and with the bound of the GPU test:
    (1) at every checked element (all taps, sampled channel pairs) the bound lies below half the median magnitude of that element's
        nonzero products x[r + s, c] dz[r, o] (hostile data: the 90th percentile, as in the forward check): a dropped or doubled
        median product cannot hide under it;
    (2) bf16x3 without the hi * lo term of one 64 x 64 wave tile exceeds the bound on most of that tile's elements."""
    x, dz = case.data()
    K, d = case.K, case.dil
    h = (K - 1) // 2
    splits = _splits(case)
    assert (splits > 1) == ("splits" in case.name)
    rng = np.random.default_rng(5)
    cs, os_ = _sample(case.cin, rng), _sample(case.cout, rng)
    live_x = np.flatnonzero(np.abs(x).sum(0) > 0)
    cs = np.intersect1d(cs, live_x)                            # (a dead input channel has no products: its gradient is exactly zero)
    ax, az = np.abs(x[:, cs].astype(np.float64)), np.abs(dz[:, os_].astype(np.float64))
    for arith in ("fp32", "bf16x3"):
        ref, M = em.wgrad(arith, x, dz, K, d)
        bnd = case.A(arith, splits) * em.U * M
        for k in range(K):
            prods = em._shifted(ax, (k - h) * d)[:, :, None] * az[:, None, :]              # [R, c, o]
            prods = np.where(prods > 0, prods, np.nan)
            med = np.nanpercentile(prods, 90, axis=0) if case.kind == "hostile" else np.nanmedian(prods, axis=0)
            b = bnd[k][np.ix_(cs, os_)]
            assert (b < 0.5 * med).all(), (case.name, arith, k, float((b / med).max()))
    # (2) the wave tile at channels [0, 64) x [0, 64) loses x_hi * dz_lo
    xh, _ = em.split3(x)
    _, zl = em.split3(dz)
    ci, co = min(64, case.cin), min(64, case.cout)
    drop, _ = em.wgrad("fp32", xh[:, :ci], zl[:, :co], K, d)
    ref, M = em.wgrad("bf16x3", x[:, :ci], dz[:, :co], K, d)
    bnd = case.A("bf16x3", splits) * em.U * M
    live = M > 0
    frac = (np.abs(drop) > bnd)[live].mean()
    assert frac > 0.5, (case.name, frac)
