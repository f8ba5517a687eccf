"""The NumPy definition of the statistics record (smol_amd/statistics.py): ``offer`` against a scalar loop, the moments
against two-pass NumPy, the blocking sums against directly formed block means, ``combine``, ``reweight`` and the binning."""

import numpy as np
import pytest

from smol_amd import statistics as st
from smol_amd.statistics import Statistics, StatisticsRecord

EPS = np.finfo(float).eps


def _rows(rng, ns, R, F, K):
    H = rng.normal(-3.0, 2.0, (ns, R))
    f = rng.normal(0.0, 1.0, (ns, R, F)) * np.pi
    cnt = rng.integers(0, 50, (ns, R, K)).astype(np.int32)
    return H, f, cnt


def _naive(spec, n_keys, H, f, cnt, keys):
    """The docstring of the module, one key, one sample, one scalar at a time."""
    rec = StatisticsRecord(spec, n_keys)
    ns, R = H.shape
    C, L = spec.n_columns, spec.n_levels
    x_all = spec.column_values(H, f, cnt)
    for s in range(ns):
        for r in range(R):
            k = int(keys[s][r])
            x = [float(v) for v in x_all[s, r]]
            if rec.n[k] == 0:
                for c in range(C):
                    rec.shift[k, c] = x[c]
            d = [np.float64(x[c]) - rec.shift[k, c] for c in range(C)]
            p = 0
            for a in range(C):
                rec.s1[k, a] = rec.s1[k, a] + d[a]
                for b in range(a, C):
                    rec.s2[k, p] = rec.s2[k, p] + d[a] * d[b]
                    p += 1
            for c in range(C):
                carry = d[c]
                for l in range(L):
                    rec.b2[k, l, c] = rec.b2[k, l, c] + carry * carry
                    if c == 0:
                        rec.nb[k, l] += 1
                    bit = np.uint64(1) << np.uint64(l)
                    if not rec.has[k, c] & bit:
                        rec.pend[k, l, c] = carry
                        rec.has[k, c] |= bit
                        break
                    carry = rec.pend[k, l, c] + carry
                    rec.has[k, c] &= ~bit
            if spec.n_bins:
                xv = np.float64(x[spec.hist_column])
                with np.errstate(invalid="ignore"):
                    q = np.floor_divide(xv - spec.hist_min, spec.hist_bin)
                if not np.isfinite(xv) or np.isnan(q) or q >= spec.n_bins:
                    rec.over[k] += 1
                elif q < 0:
                    rec.under[k] += 1
                else:
                    rec.hist[k, int(q)] += 1
            rec.n[k] += 1
    return rec


def _same(a, b):
    for f in st._ARRAYS:
        g, w = getattr(a, f), getattr(b, f)
        assert g.dtype == w.dtype and g.shape == w.shape, f
        np.testing.assert_array_equal(g, w, err_msg=f)


@pytest.mark.parametrize("keyed", [False, True])
def test_offer_equals_the_scalar_loop(keyed):
    rng = np.random.default_rng(3)
    ns, R, F, K = 37, 5, 4, 3
    H, f, cnt = _rows(rng, ns, R, F, K)
    H[11, 2] = np.inf  # (a row that is not finite goes to `over`)
    spec = Statistics(st.BY_STATE_POINT if keyed else st.BY_WALKER,
                      [st.ENTHALPY, st.feature(2), st.kind(K, 1), st.ENERGY, st.feature(0)], weights=rng.normal(size=F),
                      n_levels=4, hist=(st.kind(K, 1), 6, 5.0, 7.0))
    keys = np.array([rng.permutation(R) for _ in range(ns)]) if keyed else np.broadcast_to(np.arange(R), (ns, R))
    got = StatisticsRecord(spec, R)
    got.offer(H[:10], f[:10], cnt[:10], keys[:10] if keyed else None)  # (two calls: the record goes on)
    got.offer(H[10:], f[10:], cnt[10:], keys[10:] if keyed else None)
    _same(got, _naive(spec, R, H, f, cnt, keys))
    assert got.under.sum() > 0 and got.over.sum() > 0 and got.hist.sum() > 0
    assert (got.under + got.over + got.hist.sum(axis=1) == ns).all() and (got.n == ns).all()
    assert (got.nb[:, 3] == ns // 8).all()
    with pytest.raises(ValueError, match="permutation"):
        got.offer(H[:1], f[:1], cnt[:1], np.zeros(R, dtype=int))


def test_covariance_against_two_pass_numpy():
    """Within 4 n eps max|d_a| max|d_b|, the bound of two sequential sums of n terms; a column with mean 10^3 and spread 1
    passes because the sums run over x - shift, not over x."""
    rng = np.random.default_rng(5)
    ns, R = 4000, 3
    H = rng.normal(1.0e3, 1.0, (ns, R))
    f = np.stack([rng.normal(-2.0, 30.0, (ns, R)), H * 0.5 + rng.normal(0, 0.1, (ns, R))], axis=-1)
    spec = Statistics.per_walker([st.ENTHALPY, st.feature(0), st.feature(1)])
    rec = StatisticsRecord(spec, R).offer(H, f)
    x = spec.column_values(H, f)
    cov, mean = rec.covariance(), rec.mean()
    for r in range(R):
        d = np.abs(x[:, r] - x[0, r]).max(axis=0)
        bound = 4 * ns * EPS * d[:, None] * d[None, :]
        want = np.cov(x[:, r].T, ddof=0)
        err = np.abs(cov[r] - want)
        print("walker", r, "cov error / bound", (err / bound).max())
        assert (err <= bound).all()
        assert (np.abs(mean[r] - x[:, r].mean(axis=0)) <= 4 * ns * EPS * d).all()
    # the same sums without the shift miss that bound on the column at 10^3
    raw = (x[:, 0, 0] ** 2).sum() / ns - (x[:, 0, 0].sum() / ns) ** 2
    d0 = np.abs(x[:, 0, 0] - x[0, 0, 0]).max()
    print("unshifted error / bound", abs(raw - x[:, 0, 0].var()) / (4 * ns * EPS * d0 * d0))
    np.testing.assert_allclose(rec.heat_capacity(800.0), x[..., 0].var(axis=0) / (st.KB * 800.0 ** 2), rtol=1e-9)


def test_blocking_levels_are_the_variances_of_block_means():
    rng = np.random.default_rng(7)
    ns, R, L = 203, 2, 6  # (203 = 0b11001011: pending blocks on levels 0, 1, 3)
    H = np.cumsum(rng.normal(size=(ns, R)), axis=0) * 0.1 + 5.0  # (correlated: the estimates grow with the level)
    spec = Statistics.per_walker([st.ENTHALPY], n_levels=L)
    rec = StatisticsRecord(spec, R).offer(H, np.zeros((ns, R, 0)))
    err, unc, nb = rec.blocking()
    for l in range(L):
        m = ns // 2 ** l
        assert (nb[:, l] == m).all()
        bm = H[:m * 2 ** l].reshape(m, 2 ** l, R).mean(axis=1)
        want = np.sqrt(bm.var(axis=0) / (m - 1))
        # (b2 and the block means both come from sums of ~n terms of size <= max|d|: a relative 1e-9 is far above that)
        np.testing.assert_allclose(err[:, l, 0], want, rtol=1e-9)
        np.testing.assert_allclose(unc[:, l, 0], want / np.sqrt(2 * (m - 1)), rtol=1e-9)
    assert (np.diff(err[:, :5, 0], axis=1) > 0).all()
    se, tau = rec.standard_error(min_blocks=6), rec.autocorrelation_time(min_blocks=6)
    assert (se >= err[:, 0]).all() and (tau >= 0.5).all()
    # uncorrelated samples: the plateau is the naive error, tau about 1/2
    white = StatisticsRecord(Statistics.per_walker([st.ENTHALPY], n_levels=8), 1).offer(rng.normal(size=(4096, 1)), np.zeros((4096, 1, 0)))
    assert 0.3 < white.autocorrelation_time()[0, 0] < 0.9


def test_combine_of_a_split_stream():
    rng = np.random.default_rng(9)
    ns, R, F, K = 600, 4, 2, 2
    H, f, cnt = _rows(rng, ns, R, F, K)
    H += 1.0e3
    spec = Statistics.per_walker([st.ENTHALPY, st.feature(1), st.kind(K, 0)], n_levels=3, hist=(st.ENTHALPY, 16, 996.0, 0.5))
    whole = StatisticsRecord(spec, R).offer(H, f, cnt)
    a = StatisticsRecord(spec, R).offer(H[:250], f[:250], cnt[:250])
    b = StatisticsRecord(spec, R).offer(H[250:], f[250:], cnt[250:])
    both = StatisticsRecord.combine([a, b])
    for name in ("n", "hist", "under", "over"):
        np.testing.assert_array_equal(getattr(both, name), getattr(whole, name))
    assert both.spec.n_levels == 0 and both.b2.shape == (R, 0, 3)  # (blocking arrays are not merged)
    x = spec.column_values(H, f, cnt)
    d = np.abs(x - x[0]).max(axis=0)  # (R, C)
    bound = 4 * ns * EPS * d[:, :, None] * d[:, None, :]
    print("combine cov error / bound", (np.abs(both.covariance() - whole.covariance()) / bound).max())
    assert (np.abs(both.covariance() - whole.covariance()) <= bound).all()
    assert (np.abs(both.mean() - whole.mean()) <= 4 * ns * EPS * d).all()
    # an empty first part takes the second one's shift
    again = StatisticsRecord.combine([StatisticsRecord(spec, R), whole])
    np.testing.assert_array_equal(again.s2, whole.s2)
    np.testing.assert_array_equal(again.shift, whole.shift)


def test_reweight_shifts_a_gaussian_histogram():
    """A Gaussian enthalpy of mean mu and variance s^2 at beta reweighted to beta' has mean mu - (beta' - beta) s^2."""
    T0, T1 = 1000.0, 500.0
    mu, sig, width = -2.0, 0.05, 0.002
    n_bins = 1000
    hmin = mu - 0.5 * n_bins * width
    centre = hmin + (np.arange(n_bins) + 0.5) * width
    spec = Statistics.per_walker([st.ENTHALPY], hist=(st.ENTHALPY, n_bins, hmin, width))
    rec = StatisticsRecord(spec, 1)
    rec.hist[0] = np.round(1e9 * np.exp(-0.5 * ((centre - mu) / sig) ** 2)).astype(np.int64)
    mean, var = rec.reweight(T0, T1)
    want = mu - (1 / (st.KB * T1) - 1 / (st.KB * T0)) * sig ** 2
    print("reweighted mean", mean[0], "analytic", want)
    assert abs(want - mu) > 10 * width and abs(mean[0] - want) <= width
    assert abs(var[0] - sig ** 2) <= 0.02 * sig ** 2
    same, _ = rec.reweight(T0, T0)
    assert abs(same[0] - mu) <= width


def test_bins_at_exact_multiples_and_one_ulp_either_side():
    hmin, width, n_bins = -0.7, 0.1, 40
    k = np.arange(-2, n_bins + 2)
    edge = np.array([hmin + float(np.float64(width) * j) for j in k])
    edge = edge[(edge - hmin) / width == np.round((edge - hmin) / width)]  # (x - hist_min an exact multiple of the bin)
    exact = np.array([e for e in edge if np.fmod(e - hmin, width) == 0.0])
    assert len(exact) >= 5
    x = np.concatenate([exact, np.nextafter(exact, -np.inf), np.nextafter(exact, np.inf)])
    q = st.bin_of(x, hmin, width)
    # the exact floor of the rounded difference over the bin, by rational arithmetic
    from fractions import Fraction
    import math

    want = np.array([math.floor(Fraction(float(np.float64(v) - hmin)) / Fraction(width)) for v in x], dtype=np.float64)
    np.testing.assert_array_equal(q, want)
    n = len(exact)
    assert (q[:n] == np.round((exact - hmin) / width)).all()
    below = np.nextafter(exact, -np.inf) - hmin < exact - hmin  # (the ulp of x survives the subtraction)
    assert below.any() and (q[n:2 * n][below] == q[:n][below] - 1).all()
    # and the record files them accordingly
    spec = Statistics.per_walker([st.ENTHALPY], hist=(st.ENTHALPY, n_bins, hmin, width))
    rec = StatisticsRecord(spec, 1).offer(x[:, None], np.zeros((len(x), 1, 0)))
    inside = (want >= 0) & (want < n_bins)
    np.testing.assert_array_equal(rec.hist[0], np.bincount(want[inside].astype(int), minlength=n_bins))
    assert rec.under[0] == (want < 0).sum() and rec.over[0] == (want >= n_bins).sum()
