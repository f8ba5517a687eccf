"""The site field of a statistics record (``Statistics(..., sites=, site_codes=)``; smolmc_set_statistics_sites), on the
host: ``StatisticsRecord.offer(..., occupancy=)`` against a direct one-hot sum in the three key modes, the identity
``site_counts[k].sum() + site_over[k] == M * n[k]``, ``combine``, the readers, and records without a field unchanged."""

import os
import re

import numpy as np
import pytest

from smol_amd import capi, engine
from smol_amd import statistics as st
from smol_amd.statistics import Statistics, StatisticsRecord
from tests import test_statistics_bins_host as bins_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def direct_sum(keys, occ, sites, S, n_keys):
    """One row at a time: keys (rows,) with a negative key for a row that is offered to nobody, occ (rows, N)."""
    counts = np.zeros((n_keys, len(sites), S), dtype=np.int64)
    over = np.zeros(n_keys, dtype=np.int64)
    for k, row in zip(keys, occ):
        if k < 0:
            continue
        for m, p in enumerate(sites):
            if row[p] < S:
                counts[k, m, row[p]] += 1
            else:
                over[k] += 1
    return counts, over


def _identity(rec):
    M = rec.site_counts.shape[1]
    np.testing.assert_array_equal(rec.site_counts.sum(axis=(1, 2)) + rec.site_over, M * rec.n)


def _rows(rng, ns, R, N, n_species):
    H = rng.normal(size=(ns, R)) * 3.0
    f = rng.normal(size=(ns, R, 2))
    occ = rng.integers(0, n_species, size=(ns, R, N)).astype(np.int32)
    return H, f, occ


@pytest.mark.parametrize("sites", [None, [11, 2, 7, 0, 5]])
@pytest.mark.parametrize("S", [3, 2])
def test_by_walker_equals_the_one_hot_sum(sites, S):
    rng = np.random.default_rng(5)
    ns, R, N = 6, 7, 13
    H, f, occ = _rows(rng, ns, R, N, 3)
    spec = Statistics.per_walker([st.ENTHALPY], n_levels=2, sites=sites, site_codes=S)
    rec = StatisticsRecord(spec, R)
    rec.offer(H[:2], f[:2], occupancy=occ[:2])
    rec.offer(H[2:], f[2:], occupancy=occ[2:])
    tracked = list(range(N)) if sites is None else sites
    keys = np.tile(np.arange(R), ns)
    counts, over = direct_sum(keys, occ.reshape(ns * R, N), tracked, S, R)
    assert rec.site_counts.dtype == np.int64 and rec.site_over.dtype == np.int64
    np.testing.assert_array_equal(rec.site_counts, counts)
    np.testing.assert_array_equal(rec.site_over, over)
    assert (over.sum() > 0) == (S == 2)  # (codes 2 land in site_over when the field has two codes)
    _identity(rec)
    np.testing.assert_array_equal(rec.n, ns)


def test_by_state_point_follows_the_key_of_every_row():
    rng = np.random.default_rng(6)
    ns, R, N, S = 5, 6, 9, 3
    H, f, occ = _rows(rng, ns, R, N, 4)  # (code 3 is outside the field)
    key_of_row = np.stack([rng.permutation(R) for _ in range(ns)])
    spec = Statistics.by_state_point([st.ENTHALPY], sites=[8, 1, 4], site_codes=S)
    rec = StatisticsRecord(spec, R).offer(H, f, key_of_row=key_of_row, occupancy=occ)
    counts, over = direct_sum(key_of_row.reshape(-1), occ.reshape(ns * R, N), [8, 1, 4], S, R)
    np.testing.assert_array_equal(rec.site_counts, counts)
    np.testing.assert_array_equal(rec.site_over, over)
    assert over.sum() > 0
    _identity(rec)
    # the same rows by walker give another field: the keys matter
    other = StatisticsRecord(Statistics.per_walker([st.ENTHALPY], sites=[8, 1, 4], site_codes=S), R).offer(H, f, occupancy=occ)
    assert not np.array_equal(other.site_counts, rec.site_counts)
    np.testing.assert_array_equal(other.site_counts.sum(axis=0), rec.site_counts.sum(axis=0))


@pytest.mark.parametrize("sites", [None, [3, 0, 6]])
def test_by_bin_rows_outside_the_bins_touch_nothing(sites):
    rng = np.random.default_rng(7)
    ns, R, N, S, nk = 8, 11, 7, 2, 4
    H, f, occ = _rows(rng, ns, R, N, 3)
    H[1, 2], H[3, 3] = np.nan, np.inf
    spec = Statistics.by_bin(st.ENTHALPY, nk, -2.0, 1.0, columns=[st.ENTHALPY, st.feature(0)], sites=sites, site_codes=S)
    rec = StatisticsRecord(spec)
    for a, b in ((0, 3), (3, ns)):
        rec.offer(H[a:b], f[a:b], occupancy=occ[a:b])
    q = st.bin_of(H.reshape(-1), -2.0, 1.0)
    inside = np.isfinite(H.reshape(-1)) & (q >= 0) & (q < nk)
    keys = np.where(inside, np.nan_to_num(q, nan=-1.0, posinf=-1.0, neginf=-1.0), -1).astype(np.int64)
    assert rec.key_under > 0 and rec.key_over > 2 and (keys >= 0).sum() == rec.n.sum()
    tracked = list(range(N)) if sites is None else sites
    counts, over = direct_sum(keys, occ.reshape(ns * R, N), tracked, S, nk)
    np.testing.assert_array_equal(rec.site_counts, counts)
    np.testing.assert_array_equal(rec.site_over, over)
    assert over.sum() > 0
    _identity(rec)
    # only rows outside: the field stays empty
    out = StatisticsRecord(spec).offer(np.full((2, R), 50.0), f[:2], occupancy=occ[:2])
    assert out.key_over == 2 * R and not out.site_counts.any() and not out.site_over.any() and not out.n.any()


def test_a_field_needs_occupancy_rows_of_one_size():
    spec = Statistics.per_walker([st.ENTHALPY], site_codes=2)
    rec = StatisticsRecord(spec, 3)
    with pytest.raises(ValueError, match="needs the occupancy"):
        rec.offer(np.zeros(3), np.zeros((3, 1)))
    rec.offer(np.zeros(3), np.zeros((3, 1)), occupancy=np.zeros((3, 5), dtype=np.int32))
    assert rec.site_counts.shape == (3, 5, 2)
    with pytest.raises(ValueError, match="tracks 5 sites"):
        rec.offer(np.zeros(3), np.zeros((3, 1)), occupancy=np.zeros((3, 6), dtype=np.int32))


def test_combine_adds_the_fields():
    rng = np.random.default_rng(8)
    ns, R, N = 6, 5, 8
    H, f, occ = _rows(rng, ns, R, N, 3)
    for spec in (Statistics.per_walker([st.ENTHALPY], sites=[1, 6, 2], site_codes=2),
                 Statistics.by_bin(st.ENTHALPY, 3, -3.0, 2.0, sites=None, site_codes=3)):
        parts = [StatisticsRecord(spec, R).offer(H[a:b], f[a:b], occupancy=occ[a:b]) for a, b in ((0, 2), (2, 3), (3, ns))]
        whole = StatisticsRecord(spec, R).offer(H, f, occupancy=occ)
        both = StatisticsRecord.combine(parts)
        np.testing.assert_array_equal(both.site_counts, whole.site_counts)
        np.testing.assert_array_equal(both.site_over, whole.site_over)
        np.testing.assert_array_equal(both.n, whole.n)
        _identity(both)
        assert both.copy().equals(both)
    a = StatisticsRecord(Statistics.per_walker([st.ENTHALPY], sites=[1, 6, 2], site_codes=2), R).offer(H, f, occupancy=occ)
    b = StatisticsRecord(Statistics.per_walker([st.ENTHALPY], sites=[1, 6, 3], site_codes=2), R).offer(H, f, occupancy=occ)
    with pytest.raises(ValueError, match="different site fields"):
        StatisticsRecord.combine([a, b])
    with pytest.raises(ValueError, match="different site fields"):
        StatisticsRecord.combine([a, StatisticsRecord(Statistics.per_walker([st.ENTHALPY]), R).offer(H, f)])


def test_frozen_order_uniform_and_frozen():
    R, N, S, ns = 2, 12, 3, 30
    spec = Statistics.per_walker([st.ENTHALPY], site_codes=S)
    # walker 0 frozen in one configuration of composition x = (1/2, 1/3, 1/6); walker 1 cycles every site through the
    # codes: uniform over the sites
    frozen = np.array([0] * 6 + [1] * 4 + [2] * 2, dtype=np.int32)
    occ = np.zeros((ns, R, N), dtype=np.int32)
    occ[:, 0] = frozen
    occ[:, 1] = (np.arange(ns) % S)[:, None]
    rec = StatisticsRecord(spec, R).offer(np.zeros((ns, R)), np.zeros((ns, R, 1)), occupancy=occ)
    x = np.array([0.5, 1.0 / 3.0, 1.0 / 6.0])
    got = rec.frozen_order()
    assert got[0] == pytest.approx(1.0 - (x * x).sum(), abs=1e-15)
    assert got[1] == pytest.approx(0.0, abs=1e-15)
    p = rec.site_occupancy()
    np.testing.assert_array_equal(p[0], np.eye(S)[frozen])
    np.testing.assert_allclose(p[1], np.full((N, S), 1.0 / 3.0), rtol=0, atol=1e-15)
    sub = rec.sublattice_occupancy([range(0, 6), range(6, 12)])
    assert sub.shape == (R, 2, S)
    np.testing.assert_allclose(sub[0], [[1, 0, 0], [0, 2.0 / 3.0, 1.0 / 3.0]], rtol=0, atol=1e-15)
    # no rows: NaN
    assert np.isnan(StatisticsRecord(spec, R, N).site_occupancy()).all()
    with pytest.raises(ValueError, match="site field"):
        StatisticsRecord(Statistics.per_walker([st.ENTHALPY]), R).site_occupancy()


def test_canonical_sites_against_a_hand_sum():
    # three levels at E = 0.5, 1.5, 2.5 (bin centres), two sites, two codes
    spec = Statistics.by_bin(st.ENTHALPY, 3, 0.0, 1.0, site_codes=2)
    H = np.array([[0.5, 0.5, 1.5, 2.5]])
    occ = np.array([[[0, 0], [0, 1], [1, 0], [1, 1]]], dtype=np.int32)
    rec = StatisticsRecord(spec).offer(H, np.zeros((1, 4, 1)), occupancy=occ)
    p = rec.site_occupancy()
    np.testing.assert_array_equal(p[0], [[1.0, 0.0], [0.5, 0.5]])
    ln_g = np.array([0.0, np.log(3.0), np.log(2.0)])
    T = 700.0
    beta = 1.0 / (st.KB * T)
    w = np.exp(ln_g - beta * np.array([0.5, 1.5, 2.5]))
    w /= w.sum()
    want = w[0] * p[0] + w[1] * p[1] + w[2] * p[2]
    got = rec.canonical_sites(ln_g, [T, 2 * T])
    assert got.shape == (2, 2, 2)
    np.testing.assert_allclose(got[0], want, rtol=1e-13, atol=0)
    np.testing.assert_allclose(got.sum(axis=2), 1.0, rtol=1e-13)
    # a level without a finite ln g is left out, as in ``canonical``
    ln_g2 = np.array([0.0, -np.inf, np.log(2.0)])
    w2 = np.array([np.exp(-beta * 0.5), 0.0, 2.0 * np.exp(-beta * 2.5)])
    w2 /= w2.sum()
    np.testing.assert_allclose(rec.canonical_sites(ln_g2, T)[0], w2[0] * p[0] + w2[2] * p[2], rtol=1e-13, atol=0)
    with pytest.raises(ValueError, match="keyed by bin"):
        StatisticsRecord(Statistics.per_walker([st.ENTHALPY], site_codes=2), 2).canonical_sites(ln_g, T)


def test_records_without_the_keywords_are_as_before():
    """One spec of tests/test_statistics_bins_host.py, its rows and its own row loop: every array as the loop gives it, the
    field empty, and a spec with a field gives the same arrays beside it."""
    rng = np.random.default_rng(3)
    ns, R = 9, 23
    H, f = bins_host._synthetic(rng, ns, R)
    H[2, 5], H[7, 0] = np.nan, np.inf
    kw = dict(columns=[st.feature(0), st.ENTHALPY, st.feature(1), st.feature(2)], hist=(st.feature(1), 6, -1500.0, 500.0))
    spec = Statistics.by_bin(st.ENTHALPY, 5, -3.0, 1.25, **kw)
    assert spec.site_codes == 0 and spec.sites is None and spec.c_sites() is None
    want = bins_host.loop_definition(spec, spec.column_values(H, f))
    rec = StatisticsRecord(spec).offer(H, f)
    for name in bins_host.BINNED_ARRAYS:
        np.testing.assert_array_equal(getattr(rec, name), want[name], err_msg=name)
    assert (rec.key_under, rec.key_over) == (want["key_under"], want["key_over"])
    assert rec.site_counts.shape == (5, 0, 0) and rec.site_over.shape == (5,) and not rec.site_over.any()
    occ = rng.integers(0, 2, size=(ns, R, 4)).astype(np.int32)
    with_field = StatisticsRecord(Statistics.by_bin(st.ENTHALPY, 5, -3.0, 1.25, site_codes=2, **kw)).offer(H, f, occupancy=occ)
    bins_host._same_record(with_field, rec, "a field changes no other array")
    # the per-walker mode likewise, blocking arrays included
    a = StatisticsRecord(Statistics.per_walker([st.ENTHALPY, st.feature(0)], n_levels=3), R).offer(H[:, :], f)
    b = StatisticsRecord(Statistics.per_walker([st.ENTHALPY, st.feature(0)], n_levels=3, sites=[0, 3], site_codes=1), R)
    b.offer(H, f, occupancy=occ)
    bins_host._same_record(b, a, "per walker")
    assert a.equals(a.copy()) and not a.equals(b)


def test_the_constructors_pass_the_field_through():
    class Obs:
        n_kinds, kind_names = 2, ["A", "B"]

    for spec in (Statistics.by_composition(Obs(), "B", 8, sites=[2, 1], site_codes=2),
                 Statistics.on_wl_levels(-1.0, 0.1, 12, sites=[2, 1], site_codes=2),
                 Statistics.by_state_point(sites=[2, 1], site_codes=2)):
        sites, n_sites, n_codes = spec.c_sites()
        assert sites.dtype == np.int32 and list(sites) == [2, 1] and (n_sites, n_codes) == (2, 2)
    assert Statistics.per_walker(site_codes=3).c_sites() == (None, 0, 3)


def test_header_engine_and_capi_name_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "smolmc.h")).read()
    for name in ("smolmc_set_statistics_sites", "smolmc_statistics_sites_shape", "smolmc_get_statistics_sites"):
        assert re.search(r"\bint %s\(smolmc_handle \*h" % name, hdr), name
        assert name in engine.SYMBOLS
    assert int(re.search(r"#define SMOLMC_MAX_STAT_SITE_CODES (\d+)", hdr).group(1)) == capi.MAX_STAT_SITE_CODES == st.MAX_SITE_CODES
