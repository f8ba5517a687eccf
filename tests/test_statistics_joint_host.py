"""The joint field of a statistics record (``Statistics(..., joint=)``; smolmc_set_statistics_joint), on the host:
``StatisticsRecord.offer`` against a loop over rows in the three key modes, the identity
``joint[k].sum() + joint_out[k] == n[k]``, ``combine``, the .npz round trip, the refusals of the spec, and the readers on
counts that are exact expectations: ``reweight_joint``, ``wham_joint``, ``from_ln_g``, ``coexistence``; and which state point
a key holds for a sampler (``Sampler.grid_state_points``, ``grid_ln_g``), without an engine."""

import os
import re

import numpy as np
import pytest

from smol_amd import capi, engine
from smol_amd import statistics as st
from smol_amd.statistics import Statistics, StatisticsRecord

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LN2 = float(np.log(2.0))


def loop_definition(keys, xa, xb, axis_a, axis_b, n_keys):
    """One row at a time: keys (rows,) with a negative key for a row that is offered to nobody."""
    (na, lo_a, w_a), (nb, lo_b, w_b) = axis_a, axis_b
    joint = np.zeros((n_keys, na, nb), dtype=np.int64)
    out = np.zeros(n_keys, dtype=np.int64)
    for k, a, b in zip(keys, xa, xb):
        if k < 0:
            continue
        qa, qb = np.floor_divide(a - lo_a, w_a), np.floor_divide(b - lo_b, w_b)
        if np.isfinite(a) and np.isfinite(b) and 0 <= qa < na and 0 <= qb < nb:
            joint[k, int(qa), int(qb)] += 1
        else:
            out[k] += 1
    return joint, out


def _rows(rng, ns, R):
    """Enthalpies and two features; feature 0 and 1 carry the values that test the edges of the axes
    (min = -1, bin = 0.5, 4 cells: the axis ends at 1; 1 - 2^-52 is the largest value whose distance from min is below 2 after
    rounding)."""
    H = rng.normal(size=(ns, R)) * 2.0
    f = rng.normal(size=(ns, R, 2))
    edges = [-1.0, -0.5, 0.0, 0.5, 1.0, np.nextafter(-1.0, -2.0), 1.0 - 2.0 ** -52, -1.5, 3.0, np.nan, np.inf, -np.inf]
    flat = f.reshape(-1, 2)
    for i, v in enumerate(edges):  # each special value on axis a with an ordinary partner, and on axis b likewise
        flat[2 * i, 0], flat[2 * i, 1] = v, 0.25
        flat[2 * i + 1, 0], flat[2 * i + 1, 1] = 0.25, v
    return H, f


AXIS = (4, -1.0, 0.5)
JOINT = ((st.feature(0), ) + AXIS, (st.feature(1), ) + AXIS)
COLS = [st.ENTHALPY, st.feature(0), st.feature(1)]


def _identity(rec):
    np.testing.assert_array_equal(rec.joint.sum(axis=(1, 2)) + rec.joint_out, rec.n)


def test_by_walker_equals_the_loop_edges_included():
    rng = np.random.default_rng(5)
    ns, R = 8, 7
    H, f = _rows(rng, ns, R)
    spec = Statistics.per_walker(COLS, n_levels=2, joint=JOINT)
    rec = StatisticsRecord(spec, R).offer(H[:3], f[:3]).offer(H[3:], f[3:])
    keys = np.tile(np.arange(R), ns)
    joint, out = loop_definition(keys, f[..., 0].ravel(), f[..., 1].ravel(), AXIS, AXIS, R)
    assert rec.joint.dtype == np.int64 and rec.joint_out.dtype == np.int64 and rec.joint.shape == (R, 4, 4)
    np.testing.assert_array_equal(rec.joint, joint)
    np.testing.assert_array_equal(rec.joint_out, out)
    _identity(rec)
    # the edge values of _rows: min itself is cell 0, min + n bin and everything beyond or not finite is outside
    one = StatisticsRecord(Statistics.per_walker(COLS, joint=JOINT), 1)
    for v, cell in ((-1.0, 0), (-0.5, 1), (0.0, 2), (0.5, 3), (1.0 - 2.0 ** -52, 3), (1.0, None), (np.nextafter(-1.0, -2.0), None),
                    (-1.5, None), (3.0, None), (np.nan, None), (np.inf, None), (-np.inf, None)):
        for axis in (0, 1):
            fresh = one.copy().offer(np.zeros((1, 1)), np.array([[[v, 0.25] if axis == 0 else [0.25, v]]]))
            if cell is None:
                assert fresh.joint_out[0] == 1 and not fresh.joint.any(), (v, axis)
            else:
                assert fresh.joint[0][(cell, 2) if axis == 0 else (2, cell)] == 1 and fresh.joint_out[0] == 0, (v, axis)
    assert out.sum() >= 14  # (seven kinds of outside values on either axis)
    # a value below min by less than half an ulp of the bin width is below min: its floor is -1, although its remainder
    # x - min + bin rounds to bin
    zero = StatisticsRecord(Statistics.per_walker(COLS, joint=((st.feature(0), 4, 0.0, 0.5), (st.feature(1), 4, 0.0, 0.5))), 1)
    for v, outside in ((-1e-17, True), (-5e-324, True), (0.0, False), (5e-324, False)):
        for pair in ([v, 0.25], [0.25, v]):
            fresh = zero.copy().offer(np.zeros((1, 1)), np.array([[pair]]))
            assert (fresh.joint_out[0], fresh.joint.sum()) == ((1, 0) if outside else (0, 1)), (v, pair)


def test_by_state_point_follows_the_keys():
    rng = np.random.default_rng(6)
    ns, R = 6, 5
    H, f = _rows(rng, ns, R)
    key_of_row = np.stack([rng.permutation(R) for _ in range(ns)])
    spec = Statistics.by_state_point(COLS, joint=JOINT)
    rec = StatisticsRecord(spec, R).offer(H, f, key_of_row=key_of_row)
    joint, out = loop_definition(key_of_row.ravel(), f[..., 0].ravel(), f[..., 1].ravel(), AXIS, AXIS, R)
    np.testing.assert_array_equal(rec.joint, joint)
    np.testing.assert_array_equal(rec.joint_out, out)
    _identity(rec)
    other = StatisticsRecord(Statistics.per_walker(COLS, joint=JOINT), R).offer(H, f)
    assert not np.array_equal(other.joint, rec.joint)
    np.testing.assert_array_equal(other.joint.sum(axis=0), rec.joint.sum(axis=0))


def test_by_bin_counts_the_rows_inside_the_bins_only():
    rng = np.random.default_rng(7)
    ns, R, nk = 6, 9, 4
    H, f = _rows(rng, ns, R)
    H[1, 2], H[4, 0] = np.nan, np.inf
    spec = Statistics.by_bin(st.ENTHALPY, nk, -2.0, 1.0, columns=COLS, joint=JOINT)
    rec = StatisticsRecord(spec).offer(H[:2], f[:2]).offer(H[2:], f[2:])
    with np.errstate(invalid="ignore"):
        q = np.floor_divide(H.ravel() + 2.0, 1.0)
    keys = np.where(np.isfinite(H.ravel()) & (q >= 0) & (q < nk), q, -1).astype(np.int64)
    assert (keys < 0).sum() == rec.key_under + rec.key_over > 2
    joint, out = loop_definition(keys, f[..., 0].ravel(), f[..., 1].ravel(), AXIS, AXIS, nk)
    np.testing.assert_array_equal(rec.joint, joint)
    np.testing.assert_array_equal(rec.joint_out, out)
    _identity(rec)
    assert rec.joint.sum() + rec.joint_out.sum() + rec.key_under + rec.key_over == ns * R
    # the key's own column may be an axis
    spec = Statistics.by_bin(st.ENTHALPY, nk, -2.0, 1.0, columns=COLS, joint=((st.ENTHALPY, 8, -2.0, 0.5), JOINT[1]))
    rec = StatisticsRecord(spec).offer(H, f)
    joint, out = loop_definition(keys, H.ravel(), f[..., 1].ravel(), (8, -2.0, 0.5), AXIS, nk)
    np.testing.assert_array_equal(rec.joint, joint)
    np.testing.assert_array_equal(rec.joint_out, out)
    for k in range(nk):  # a row of key k lies in the cells 2 k and 2 k + 1 of the enthalpy axis
        assert not np.delete(rec.joint[k], [2 * k, 2 * k + 1], axis=0).any()


def test_one_column_on_both_axes_fills_the_diagonal():
    rng = np.random.default_rng(8)
    ns, R = 5, 6
    H, f = _rows(rng, ns, R)
    spec = Statistics.per_walker(COLS, joint=(JOINT[0], JOINT[0]))
    assert spec.c_joint() == (1, 4, -1.0, 0.5, 1, 4, -1.0, 0.5)
    rec = StatisticsRecord(spec, R).offer(H, f)
    _identity(rec)
    assert rec.joint.sum() > 0
    off = rec.joint.copy()
    off[:, np.arange(4), np.arange(4)] = 0
    assert not off.any()
    # two widths of one column: cell (qa, qb) with qb = qa // 2
    spec = Statistics.per_walker(COLS, joint=(JOINT[0], (st.feature(0), 2, -1.0, 1.0)))
    rec = StatisticsRecord(spec, R).offer(H, f)
    qa, qb = np.nonzero(rec.joint.sum(axis=0))
    assert len(qa) and (qb == qa // 2).all()


def test_combine_copy_equals_and_the_npz_round_trip(tmp_path):
    rng = np.random.default_rng(9)
    ns, R = 10, 6
    H, f = _rows(rng, ns, R)
    occ = rng.integers(0, 2, size=(ns, R, 3))
    for spec in (Statistics.per_walker(COLS, joint=JOINT, hist=(st.ENTHALPY, 5, -2.0, 1.0)),
                 Statistics.by_bin(st.ENTHALPY, 4, -2.0, 1.0, columns=COLS, joint=JOINT, site_codes=2, sites=[2, 0])):
        kw = dict(occupancy=occ) if spec.site_codes else {}
        cut = lambda a, b: {k: v[a:b] for k, v in kw.items()}  # noqa: E731
        whole = StatisticsRecord(spec, R).offer(H, f, **kw)
        parts = [StatisticsRecord(spec, R).offer(H[:4], f[:4], **cut(0, 4)), StatisticsRecord(spec, R).offer(H[4:], f[4:], **cut(4, ns))]
        both = StatisticsRecord.combine(parts)
        np.testing.assert_array_equal(both.joint, whole.joint)
        np.testing.assert_array_equal(both.joint_out, whole.joint_out)
        np.testing.assert_array_equal(both.n, whole.n)
        assert both.spec.c_joint() == spec.c_joint()
        _identity(both)
        assert whole.equals(whole.copy())
        changed = whole.copy()
        changed.joint_out[0] += 1
        assert not whole.equals(changed)
        path = str(tmp_path / "record.npz")
        whole.save(path)
        back = StatisticsRecord.load(path)
        assert back.equals(whole) and back.spec.describe() == spec.describe()
        assert back.spec.c_joint() == spec.c_joint() and back.spec.joint_axes() == spec.joint_axes()
        for name in st._ARRAYS + st._SITE_ARRAYS + st._JOINT_ARRAYS:
            assert getattr(back, name).dtype == getattr(whole, name).dtype, name
    other = StatisticsRecord(Statistics.per_walker(COLS, joint=(JOINT[0], (st.feature(1), 4, -1.0, 0.25))), R).offer(H, f)
    with pytest.raises(ValueError, match="different joint fields"):
        StatisticsRecord.combine([StatisticsRecord(Statistics.per_walker(COLS, joint=JOINT), R).offer(H, f), other])


def test_a_record_without_the_keyword_is_as_before():
    rng = np.random.default_rng(3)
    ns, R = 7, 5
    H, f = _rows(rng, ns, R)
    plain = Statistics.per_walker(COLS, n_levels=3, hist=(st.ENTHALPY, 5, -2.0, 1.0))
    assert not plain.has_joint and plain.c_joint() is None and plain.joint_axes() is None and plain.describe()["joint"] is None
    a = StatisticsRecord(plain, R).offer(H, f)
    assert a.joint.shape == (R, 0, 0) and a.joint_out.shape == (R,) and not a.joint_out.any()
    b = StatisticsRecord(Statistics.per_walker(COLS, n_levels=3, hist=(st.ENTHALPY, 5, -2.0, 1.0), joint=JOINT), R).offer(H, f)
    for name in st._ARRAYS:
        np.testing.assert_array_equal(getattr(a, name), getattr(b, name), err_msg=name)
    assert not a.equals(b)
    for reader in (a.joint_histogram, lambda: a.marginal(0), lambda: a.free_energy_surface(300.0),
                   lambda: a.reweight_joint(1.0, 0.0, 1.0, 0.0), lambda: a.wham_joint(np.ones(R), np.zeros(R))):
        with pytest.raises(ValueError, match="needs a record with a joint field"):
            reader()


def test_every_refusal_of_the_spec():
    ok = (st.ENTHALPY, 4, 0.0, 1.0)
    with pytest.raises(ValueError, match="column a must be one of the record's columns"):
        Statistics.per_walker([st.ENTHALPY], joint=((st.feature(0), 4, 0.0, 1.0), ok))
    with pytest.raises(ValueError, match="column b must be one of the record's columns"):
        Statistics.per_walker([st.ENTHALPY], joint=(ok, (st.ENERGY, 4, 0.0, 1.0)))
    for n in (0, -1, 65537):
        with pytest.raises(ValueError, match=f"n_a must be 1..65536, got {n}"):
            Statistics.per_walker([st.ENTHALPY], joint=((st.ENTHALPY, n, 0.0, 1.0), ok))
        with pytest.raises(ValueError, match=f"n_b must be 1..65536, got {n}"):
            Statistics.per_walker([st.ENTHALPY], joint=(ok, (st.ENTHALPY, n, 0.0, 1.0)))
    for vmin, vbin in ((0.0, 0.0), (0.0, -1.0), (0.0, np.inf), (0.0, np.nan), (np.nan, 1.0), (-np.inf, 1.0)):
        with pytest.raises(ValueError, match="bin_a must be a positive finite number and min_a finite"):
            Statistics.per_walker([st.ENTHALPY], joint=((st.ENTHALPY, 4, vmin, vbin), ok))
        with pytest.raises(ValueError, match="bin_b must be a positive finite number and min_b finite"):
            Statistics.by_state_point([st.ENTHALPY], joint=(ok, (st.ENTHALPY, 4, vmin, vbin)))
    with pytest.raises(ValueError, match="joint= takes two axes"):
        Statistics.per_walker([st.ENTHALPY], joint=(ok,))
    with pytest.raises(ValueError, match="joint= takes two axes"):
        Statistics.per_walker([st.ENTHALPY], joint=(ok, (st.ENTHALPY, 4, 0.0)))
    assert Statistics.per_walker([st.ENTHALPY], joint=((st.ENTHALPY, 65536, 0.0, 1.0), (st.ENTHALPY, 1, 0.0, 1.0))).joint_n == (65536, 1)


# ---- the readers on exact expectations --------------------------------------------------------------------------------------
NA, NB = 6, 5
POINTS = [(1, 0), (1, 1), (2, 1), (2, 3), (3, 2), (1, 2)]  # (i_k, j_k): beta_k bin_a = i_k ln 2, beta_k mu_k bin_b = j_k ln 2


def _exact_grid():
    """An integer table g[a][b] and the records of POINTS whose counts are exact expectations: with unit bins and the
    centres at the integers a, b (min = -1/2), H_k = g 2^(-i_k a + j_k b) 2^m with m = i_k (NA - 1): integers."""
    rng = np.random.default_rng(11)
    g = rng.integers(1, 40, size=(NA, NB)).astype(np.int64)
    g[0, NB - 1] = g[NA - 1, 0] = 0  # (cells no key ever sees: ln g = -inf)
    a, b = np.arange(NA)[:, None], np.arange(NB)[None, :]
    spec = Statistics.by_state_point([st.ENERGY, ("kind", 0)], weights=[1.0], joint=((st.ENERGY, NA, -0.5, 1.0), (("kind", 0), NB, -0.5, 1.0)))
    rec = StatisticsRecord(spec, len(POINTS))
    for k, (i, j) in enumerate(POINTS):
        rec.joint[k] = g * 2 ** (-i * a + j * b + i * (NA - 1))
    rec.n = rec.joint.sum(axis=(1, 2))
    betas = np.array([i * LN2 for i, _ in POINTS])
    fields = np.array([j / i for i, j in POINTS])
    return g, rec, betas, fields


def _exact_moments(g, i, j):
    """Mean and covariance of (a, b) and P(b) under the weights g 2^(-i a + j b), in exact integer arithmetic up to the
    final divisions."""
    a, b = np.arange(NA), np.arange(NB)
    w = [[int(g[x, y]) * 2 ** (-i * x + j * y + i * (NA - 1)) for y in b] for x in a]
    z = sum(map(sum, w))
    sa = sum(x * w[x][y] for x in a for y in b)
    sb = sum(y * w[x][y] for x in a for y in b)
    saa = sum(x * x * w[x][y] for x in a for y in b)
    sbb = sum(y * y * w[x][y] for x in a for y in b)
    sab = sum(x * y * w[x][y] for x in a for y in b)
    mean = np.array([sa / z, sb / z])
    # (central moments from integer numerators: z s2 - s1 s1 over z^2, no cancellation in floating point)
    cov = np.array([[(z * saa - sa * sa) / z ** 2, (z * sab - sa * sb) / z ** 2], [(z * sab - sa * sb) / z ** 2, (z * sbb - sb * sb) / z ** 2]])
    pn = np.array([sum(w[x][y] for x in a) / z for y in b])
    return mean, cov, pn


def test_the_readers_of_the_histogram():
    g, rec, betas, fields = _exact_grid()
    joint, ca, cb = rec.joint_histogram()
    assert joint is rec.joint
    np.testing.assert_array_equal(ca, np.arange(NA, dtype=float))
    np.testing.assert_array_equal(cb, np.arange(NB, dtype=float))
    np.testing.assert_array_equal(rec.marginal(0), rec.joint.sum(axis=2))
    np.testing.assert_array_equal(rec.marginal(1), rec.joint.sum(axis=1))
    assert rec.marginal(0).shape == (len(POINTS), NA) and rec.marginal(1).shape == (len(POINTS), NB)
    with pytest.raises(ValueError, match="axis must be 0"):
        rec.marginal(2)
    T = 1.0 / (st.KB * betas)
    F = rec.free_energy_surface(T)
    assert F.shape == rec.joint.shape and np.isposinf(F[:, 0, NB - 1]).all() and np.isposinf(F[:, NA - 1, 0]).all()
    seen = rec.joint > 0
    assert np.isfinite(F[seen]).all() and (seen.sum(axis=(1, 2)) == NA * NB - 2).all()
    p = np.exp(-F * betas[:, None, None])
    np.testing.assert_allclose(p.sum(axis=(1, 2)), 1.0, rtol=1e-13)
    np.testing.assert_allclose(p, rec.joint / rec.joint.sum(axis=(1, 2), keepdims=True), rtol=1e-12)


def test_reweight_joint_reproduces_every_key_from_every_other():
    g, rec, betas, fields = _exact_grid()
    exact = [_exact_moments(g, i, j) for i, j in POINTS]
    for src in range(len(POINTS)):
        m1, c1, p1 = rec.reweight_joint(betas, fields, betas[src], fields[src])  # every key to state point src
        for k in range(len(POINTS)):
            np.testing.assert_allclose(m1[k], exact[src][0], rtol=1e-12, err_msg=f"mean {k} -> {src}")
            np.testing.assert_allclose(c1[k], exact[src][1], rtol=1e-12, err_msg=f"covariance {k} -> {src}")
            np.testing.assert_allclose(p1[k], exact[src][2], rtol=1e-12, err_msg=f"P(N) {k} -> {src}")
    binned = StatisticsRecord(Statistics.by_bin(st.ENTHALPY, 3, 0.0, 1.0, joint=((st.ENTHALPY, 2, 0.0, 1.0),) * 2))
    with pytest.raises(ValueError, match="not defined for a record keyed by bin"):
        binned.reweight_joint(1.0, 0.0, 2.0, 0.0)
    with pytest.raises(ValueError, match="not defined for a record keyed by bin"):
        binned.wham_joint(np.ones(3), np.zeros(3))


def test_wham_joint_returns_the_table_the_counts_were_made_of():
    g, rec, betas, fields = _exact_grid()
    ln_g, f = rec.wham_joint(betas, fields, tol=1e-12)
    assert ln_g.shape == (NA, NB) and f.shape == (len(POINTS),)
    assert np.isneginf(ln_g[0, NB - 1]) and np.isneginf(ln_g[NA - 1, 0])
    seen = g > 0
    d = ln_g[seen] - np.log(g[seen].astype(float))
    assert np.abs(d - d[0]).max() < 1e-9, np.abs(d - d[0]).max()
    # f_k = -ln Z_k up to the same constant
    a, b = np.arange(NA)[:, None], np.arange(NB)[None, :]
    z = np.array([(g * 2.0 ** (-i * a + j * b)).sum() for i, j in POINTS])
    np.testing.assert_allclose(f - f[0], -(np.log(z) - np.log(z[0])), atol=1e-9)
    # ... and from ln g every state point again, the sampled ones and one between them
    for k, (i, j) in enumerate(POINTS):
        mean, cov, pn = rec.from_ln_g(ln_g, betas[k], fields[k])
        want = _exact_moments(g, i, j)
        np.testing.assert_allclose(mean, want[0], rtol=1e-8)
        np.testing.assert_allclose(cov, want[1], rtol=1e-8)
        np.testing.assert_allclose(pn, want[2], rtol=1e-8)
        same = rec.reweight_joint(betas, fields, betas[k], fields[k])
        np.testing.assert_allclose(mean, same[0][0], rtol=1e-8)
    mean, cov, pn = rec.from_ln_g(ln_g, np.array([2 * LN2, 3 * LN2]), np.array([1.0, 1.0 / 3.0]))
    assert mean.shape == (2, 2) and cov.shape == (2, 2, 2) and pn.shape == (2, NB)
    np.testing.assert_allclose(mean[0], _exact_moments(g, 2, 2)[0], rtol=1e-8)
    np.testing.assert_allclose(mean[1], _exact_moments(g, 3, 1)[0], rtol=1e-8)
    # a key without counts is left out
    more = StatisticsRecord(rec.spec, len(POINTS) + 1)
    more.joint[:-1] = rec.joint
    ln_g2, f2 = more.wham_joint(np.append(betas, 1.0), np.append(fields, 0.0))
    np.testing.assert_array_equal(ln_g2, ln_g)
    assert np.isnan(f2[-1]) and np.array_equal(f2[:-1], f)
    with pytest.raises(ValueError, match="did not bring the free energies"):
        rec.wham_joint(betas, fields, tol=0.0, max_iter=3)
    with pytest.raises(ValueError, match="betas and"):
        rec.wham_joint(betas[:-1], fields)


def test_coexistence_finds_the_field_of_equal_weight():
    """ln g(a, b) = t(a) + s(b) - kappa b with s symmetric under b -> n_b - 1 - b and two peaks: P(N) at (beta, field) is
    exp(s(b) + (beta field - kappa) b), symmetric -- equal weight below and above the middle -- exactly at
    field = kappa / beta."""
    nb, kappa, beta = 12, 0.37, 2.5
    b = np.arange(nb)
    s = 3.0 * np.cos(2.0 * np.pi * (b - (nb - 1) / 2.0) / (nb - 1)) ** 2 * 2.0  # peaks at both ends, a valley between
    assert np.allclose(s, s[::-1]) and s[0] > s[nb // 2]
    t = -0.5 * (np.arange(4) - 1.0) ** 2
    ln_g = t[:, None] + (s - kappa * b)[None, :]
    spec = Statistics.by_state_point([st.ENERGY, ("kind", 0)], weights=[1.0], joint=((st.ENERGY, 4, -0.5, 1.0), (("kind", 0), nb, -0.5, 1.0)))
    rec = StatisticsRecord(spec, 1)
    for tol in (1e-6, 1e-11):
        field = rec.coexistence(ln_g, beta, (-1.0, 1.5), nb // 2, tol=tol)
        assert abs(field - kappa / beta) <= tol, (field, kappa / beta)
    pn = rec.from_ln_g(ln_g, beta, kappa / beta)[2]
    np.testing.assert_allclose(pn[:nb // 2].sum(), 0.5, rtol=1e-12)
    with pytest.raises(ValueError, match="does not change the sign"):
        rec.coexistence(ln_g, beta, (0.5, 1.5), nb // 2)
    with pytest.raises(ValueError, match="split must be 1..11"):
        rec.coexistence(ln_g, beta, (-1.0, 1.5), nb)


# ---- no engine involved ------------------------------------------------------------------------------------------------------
def test_the_constructors_pass_the_field_through():
    class Obs:
        n_kinds, kind_names = 2, ["A", "B"]

    joint = ((st.ENTHALPY, 7, -1.0, 0.25), (st.kind(Obs(), "B"), 9, -0.5, 1.0))
    cols = [st.ENTHALPY, st.kind(Obs(), "B")]
    specs = (Statistics.per_walker(cols, joint=joint), Statistics.by_state_point(cols, joint=joint),
             Statistics.by_bin(st.ENTHALPY, 3, 0.0, 1.0, columns=cols, joint=joint),
             Statistics.by_composition(Obs(), "B", 8, joint=joint), Statistics.on_wl_levels(-1.0, 0.1, 12, columns=cols, joint=joint))
    for spec in specs:
        ca, cb = spec.columns.index(st.ENTHALPY), spec.columns.index(("kind", 1))
        args = spec.c_joint()
        assert args == (ca, 7, -1.0, 0.25, cb, 9, -0.5, 1.0)
        assert [type(v) for v in args] == [int, int, float, float] * 2
        assert spec.joint_axes() == joint and StatisticsRecord(spec, 4).joint.shape[1:] == (7, 9)
        # the C arguments fit the entry point's signature
        restype, argtypes = engine.SYMBOLS["smolmc_set_statistics_joint"]
        assert len(argtypes) == 1 + len(args)
        for v, t in zip(args, argtypes[1:]):
            t(v)
    ca, cb = specs[0].joint_centres()
    np.testing.assert_allclose(ca, -1.0 + (np.arange(7) + 0.5) * 0.25)
    np.testing.assert_allclose(cb, np.arange(9.0))


def test_a_sampler_builds_its_schema_without_an_engine():
    from smol_amd import moca
    from tests.test_gpu_families import five_sampler, five_specs  # (no engine: the helpers build specs and a sampler)

    c, specs = five_specs()
    obs = specs["observables"]
    F = len(moca.Ensemble.from_cluster_expansion(c["sc"], c["coefs"]).natural_parameters)
    joint = ((st.ENERGY, 64, -10.0, 0.5), (st.kind(obs, 1), 55, -0.5, 1.0))
    spec = Statistics.by_state_point([st.ENERGY, st.kind(obs, 1)], weights=np.ones(F), joint=joint)
    sampler, ens = five_sampler(c, specs, statistics=spec)
    assert sampler._engine is None and sampler._statistics is spec and sampler._statistics.c_joint()[1::4] == (64, 55)
    # a canonical ensemble has no chemical potentials, a record by walker no state points: grid_ln_g says so, without an engine
    with pytest.raises(ValueError, match="semigrand ensemble"):
        sampler.grid_ln_g()
    for bad in (Statistics.per_walker([st.ENERGY, st.kind(obs, 1)], weights=np.ones(F), joint=joint),
                Statistics.by_state_point([st.ENERGY, st.kind(obs, 1)], weights=np.ones(F)),
                Statistics.by_state_point([st.ENERGY, st.kind(obs, 1)], weights=np.ones(F), joint=(joint[1], joint[0]))):
        other, _ = five_sampler(c, specs, statistics=bad)
        with pytest.raises(ValueError, match="grid_ln_g needs a sampler built with statistics=Statistics.by_state_point"):
            other.grid_ln_g()


def test_header_engine_and_capi_name_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "smolmc.h")).read()
    for name in ("smolmc_set_statistics_joint", "smolmc_statistics_joint_shape", "smolmc_get_statistics_joint"):
        assert re.search(r"\bint %s\(smolmc_handle \*h" % name, hdr), name
        assert name in engine.SYMBOLS
    assert len(engine.SYMBOLS["smolmc_statistics_joint_shape"][1]) == 9 and len(engine.SYMBOLS["smolmc_get_statistics_joint"][1]) == 3
    assert int(re.search(r"#define SMOLMC_MAX_STAT_JOINT_CELLS (\d+)", hdr).group(1)) == capi.MAX_STAT_JOINT_CELLS == st.MAX_JOINT_CELLS
    assert st._JOINT_ARRAYS == ("joint", "joint_out") and not set(st._JOINT_ARRAYS) & set(st._ARRAYS + st._SITE_ARRAYS)


# ---- Sampler.grid_state_points and grid_ln_g: the betas and fields of the keys, no engine ------------------------------------
def _semigrand_sampler(joint_a=st.ENERGY, kind_k=1, make=Statistics.by_state_point):
    """A sampler of the rocksalt case (cations Li+ / Mn3+ / Ti4+ = kinds 0..2, anions O2- / F- = kinds 3, 4) with chemical
    potentials, six walkers, and a record keyed by state point with the joint field (joint_a, kind kind_k)."""
    from smol_amd import moca
    from tests.test_gpu_families import NW, five_specs

    c, specs = five_specs()
    obs = specs["observables"]
    ens = moca.Ensemble.from_cluster_expansion(c["sc"], c["coefs"])
    ens.chemical_potentials = {sp: 0.0 for sp in ens.species}
    F = len(ens.natural_parameters)
    cols = [st.ENERGY, st.ENTHALPY, st.kind(obs, kind_k)]
    spec = make(cols, weights=np.ones(F - 1), joint=((joint_a, NA, -0.5, 1.0), (st.kind(obs, kind_k), NB, -0.5, 1.0)))
    sampler = moca.Sampler.from_ensemble(ens, temperature=3000.0, nwalkers=NW, seeds=list(range(3, 3 + NW)), rank=0, world_size=1,
                                         observables=obs, statistics=spec)
    return sampler, ens, spec


def test_grid_state_points_of_walkers_with_their_own_chemical_potentials():
    sampler, ens, spec = _semigrand_sampler()
    nw = len(sampler.mckernels)
    assert nw == len(POINTS) and sampler._engine is None
    temps = np.linspace(1000.0, 2000.0, nw)
    mu_mn = np.linspace(-0.3, 0.4, nw)
    for k, T in zip(sampler.mckernels, temps):
        k.temperature = T
    # Mn3+ is kind 1: its field is mu(Mn3+) less the value Li+ and Ti4+ share; the anions share one among themselves
    sampler.set_chemical_potentials([{"Li+": 0.05, "Mn3+": 0.05 + m, "Ti4+": 0.05, "O2-": -0.2, "F-": -0.2} for m in mu_mn])
    betas, fields = sampler.grid_state_points()
    np.testing.assert_allclose(betas, 1.0 / (st.KB * temps), rtol=1e-15)
    np.testing.assert_allclose(fields, mu_mn, rtol=0, atol=1e-15)
    # without per-walker values: the ensemble's own, at every key
    sampler.set_chemical_potentials(None)
    ens.chemical_potentials = {"Li+": 0.0, "Mn3+": 0.25, "Ti4+": 0.0, "O2-": 0.0, "F-": 0.0}
    np.testing.assert_array_equal(sampler.grid_state_points()[1], np.full(nw, 0.25))
    # the other species of the counted sublattice differ: one count is not the conjugate of the field
    sampler.set_chemical_potentials([{"Li+": 0.0, "Mn3+": 0.1, "Ti4+": 0.2, "O2-": 0.0, "F-": 0.0}] * nw)
    with pytest.raises(ValueError, match="the species beside Mn3\\+ hold different chemical potentials on one sublattice"):
        sampler.grid_state_points()
    # ... or the species of another sublattice do
    sampler.set_chemical_potentials([{"Li+": 0.0, "Mn3+": 0.1, "Ti4+": 0.0, "O2-": 0.0, "F-": 0.3}] * nw)
    with pytest.raises(ValueError, match="hold different chemical potentials on one sublattice"):
        sampler.grid_state_points()
    # a count of the two-species sublattice: F- is kind 4, its field mu(F-) - mu(O2-)
    other, _, _ = _semigrand_sampler(kind_k=4)
    other.set_chemical_potentials([{"Li+": 0.1, "Mn3+": 0.1, "Ti4+": 0.1, "O2-": -0.2, "F-": -0.2 + m} for m in mu_mn])
    np.testing.assert_allclose(other.grid_state_points()[1], mu_mn, rtol=0, atol=1e-15)
    # the enthalpy on axis a would count -mu N twice
    wrong, _, _ = _semigrand_sampler(joint_a=st.ENTHALPY)
    with pytest.raises(ValueError, match="needs statistics.ENERGY .* on axis a of the joint field"):
        wrong.grid_ln_g()


def test_grid_state_points_follow_the_grid_of_run_exchange():
    """What ``run_exchange`` leaves: the grid and the grid point of every engine state point when the call began."""
    from smol_amd import parallel

    sampler, ens, spec = _semigrand_sampler()
    nw = len(sampler.mckernels)
    temps, mu_mn = np.array([1200.0, 1800.0]), np.array([-0.2, 0.0, 0.3])
    rows = ens.walker_mu_rows([{"Li+": 0.0, "Mn3+": m, "Ti4+": 0.0, "O2-": 0.1, "F-": 0.1} for m in mu_mn])
    gx = parallel.GridExchange(temps, rows)
    assert gx.npoints == nw
    base = np.array([4, 0, 5, 1, 3, 2])
    sampler._grid, sampler._grid_base = gx, base
    # the kernels' own values follow the WALKERS and must not be read
    for k in sampler.mckernels:
        k.temperature = 77.0
    betas, fields = sampler.grid_state_points()
    np.testing.assert_allclose(betas, 1.0 / (st.KB * np.repeat(temps, 3)[base]), rtol=1e-15)
    np.testing.assert_allclose(fields, np.tile(mu_mn, 2)[base], rtol=0, atol=1e-15)
    np.testing.assert_array_equal(betas, 1.0 / (st.KB * gx.point_temperatures[base]))
    sampler._grid_keys_mixed = True
    with pytest.raises(ValueError, match="reset_statistics\\(\\) before the second call"):
        sampler.grid_state_points()


def test_grid_ln_g_is_wham_joint_at_the_samplers_state_points():
    g, rec, betas, fields = _exact_grid()
    sampler, ens, spec = _semigrand_sampler()
    temps = 1.0 / (st.KB * betas)
    for k, T in zip(sampler.mckernels, temps):
        k.temperature = T
    sampler.set_chemical_potentials([{"Li+": -0.1, "Mn3+": -0.1 + m, "Ti4+": -0.1, "O2-": 0.0, "F-": 0.0} for m in fields])
    held = StatisticsRecord(spec, len(POINTS))
    held.joint[:] = rec.joint
    held.n = rec.n.copy()

    class Handle:  # (what Sampler.statistics asks of its engine)
        def statistics(self):
            return held

    sampler._get_engine = lambda: Handle()
    ln_g, f = sampler.grid_ln_g()
    want = held.wham_joint(1.0 / (st.KB * temps), fields)
    np.testing.assert_allclose(ln_g, want[0], rtol=0, atol=1e-9)
    np.testing.assert_allclose(f, want[1], rtol=0, atol=1e-9)
    seen = g > 0
    d = ln_g[seen] - np.log(g[seen].astype(float))
    assert np.abs(d - d[0]).max() < 1e-8  # (the betas went through 1 / (kB T) and back: a rounding each way)
