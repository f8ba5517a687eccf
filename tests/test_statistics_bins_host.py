"""Statistics keyed by bins of a column (statistics.Statistics.by_bin; SMOLMC_STAT_BY_BIN), on the host: the vectorised
``StatisticsRecord.offer`` against a plain per-row loop, its reduction to the per-walker mode, the exact microcanonical and
canonical averages of an enumerated 8-site case, record handling, and the C ABI as header, capi and engine.py state it."""

import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from smol_amd import capi, engine
from smol_amd import statistics as st
from smol_amd.statistics import Statistics, StatisticsRecord
from tests.cases import load_case, tables_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINNED_ARRAYS = ("n", "shift", "s1", "s2", "hist", "under", "over")


def _same_record(got, want, what=""):
    for f in st._ARRAYS:
        g, w = getattr(got, f), getattr(want, f)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, f, g.dtype, g.shape, w.dtype, w.shape)
        np.testing.assert_array_equal(g, w, err_msg=f"{what} {f}")
    assert (got.key_under, got.key_over) == (want.key_under, want.key_over), what


def loop_definition(spec, x):
    """The rule of the module docstring, one row at a time: x (ns, R, C) column values -> dict of the record's arrays."""
    nk, Cn, B = spec.n_keys, spec.n_columns, spec.n_bins
    out = dict(n=np.zeros(nk, dtype=np.int64), shift=np.zeros((nk, Cn)), s1=np.zeros((nk, Cn)), s2=np.zeros((nk, spec.n_pairs)),
               hist=np.zeros((nk, B), dtype=np.int64), under=np.zeros(nk, dtype=np.int64), over=np.zeros(nk, dtype=np.int64),
               key_under=0, key_over=0)
    pairs = [(a, b) for a in range(Cn) for b in range(a, Cn)]
    for s in range(x.shape[0]):
        for r in range(x.shape[1]):
            row = x[s, r]
            xv = row[spec.key_column]
            q = float(st.bin_of(xv, spec.key_min, spec.key_bin))
            if not np.isfinite(xv) or np.isnan(q) or q >= nk:
                out["key_over"] += 1
                continue
            if q < 0:
                out["key_under"] += 1
                continue
            k = int(q)
            if out["n"][k] == 0:
                out["shift"][k] = row
            d = row - out["shift"][k]
            for c in range(Cn):
                out["s1"][k, c] = out["s1"][k, c] + d[c]
            for p, (a, b) in enumerate(pairs):
                out["s2"][k, p] = out["s2"][k, p] + d[a] * d[b]
            if B:
                hv = row[spec.hist_column]
                hq = float(st.bin_of(hv, spec.hist_min, spec.hist_bin))
                if not np.isfinite(hv) or np.isnan(hq) or hq >= B:
                    out["over"][k] += 1
                elif hq < 0:
                    out["under"][k] += 1
                else:
                    out["hist"][k, int(hq)] += 1
            out["n"][k] += 1
    return out


def _synthetic(rng, ns, R, F=3):
    """(enthalpy (ns, R), features (ns, R, F)) with many significant bits."""
    return rng.normal(size=(ns, R)) * 3.0, rng.normal(size=(ns, R, F)) * np.array([1.0, 1e3, 1e-3])[:F]


# ---- 1: the definition ------------------------------------------------------------------------------------------------
def test_offer_equals_the_row_loop():
    rng = np.random.default_rng(3)
    ns, R = 9, 23
    H, f = _synthetic(rng, ns, R)
    H[2, 5], H[7, 0] = np.nan, np.inf  # (values that are not finite: key_over)
    f[4, 4, 1] = np.nan                # (a non-finite value in the histogram's column: the key's own over)
    spec = Statistics.by_bin(st.ENTHALPY, 5, -3.0, 1.25, columns=[st.feature(0), st.ENTHALPY, st.feature(1), st.feature(2)],
                             hist=(st.feature(1), 6, -1500.0, 500.0))
    x = spec.column_values(H, f)
    want = loop_definition(spec, x)
    assert want["key_under"] > 0 and want["key_over"] > 2 and want["n"].max() > ns  # (several rows per key and sample)
    assert want["under"].sum() > 0 and want["over"].sum() > 0
    # offered at once, and block by block (a key's shift comes from an earlier block)
    for cuts in ([0, ns], [0, 1, 4, ns]):
        rec = StatisticsRecord(spec)
        for a, b in zip(cuts[:-1], cuts[1:]):
            rec.offer(H[a:b], f[a:b])
        for name in BINNED_ARRAYS:
            np.testing.assert_array_equal(getattr(rec, name), want[name], err_msg=name)
        assert (rec.key_under, rec.key_over) == (want["key_under"], want["key_over"])
        assert rec.n.sum() + rec.key_under + rec.key_over == ns * R
        assert rec.pend.shape == (5, 0, 4) and rec.b2.shape == (5, 0, 4) and rec.nb.shape == (5, 0)
    # one sample as (R,) arrays
    one = StatisticsRecord(spec).offer(H[0], f[0])
    np.testing.assert_array_equal(one.s1, StatisticsRecord(spec).offer(H[:1], f[:1]).s1)
    # the order within a sample is part of the definition: reversed walkers give other sums
    rev = StatisticsRecord(spec).offer(H[:, ::-1], f[:, ::-1])
    np.testing.assert_array_equal(rev.n, want["n"])
    assert not np.array_equal(rev.s2, want["s2"])


# ---- 2: the reduction to the per-walker mode --------------------------------------------------------------------------
def test_reduces_to_the_per_walker_record():
    rng = np.random.default_rng(4)
    ns, R = 17, 11
    H, f = _synthetic(rng, ns, R)
    f[:, :, 0] = np.arange(R) + 0.5  # the key value: walker + 0.5
    cols = [st.feature(0), st.ENTHALPY, st.feature(1)]
    hist = (st.ENTHALPY, 8, -4.0, 1.0)
    binned = StatisticsRecord(Statistics.by_bin(st.feature(0), R, 0.0, 1.0, columns=cols, hist=hist)).offer(H, f)
    walker = StatisticsRecord(Statistics.per_walker(cols, n_levels=0, hist=hist), R).offer(H, f)
    _same_record(binned, walker, "bins of walker + 0.5")
    assert (binned.n == ns).all() and binned.key_under == binned.key_over == 0


# ---- 3: exactness on an enumerated case ---------------------------------------------------------------------------------
def _enumerated():
    """(E (256,), x (256, C), spec) of every state of fcc_prim222_aliased through the CPU oracle: the enthalpy and every
    feature as columns, bins narrow enough that every distinct enthalpy has its own key."""
    from oracle import oracle as orc

    name = "fcc_prim222_aliased"
    sc = load_case(name)["sc"]
    assert sc.num_sites == 8
    ev = orc.OracleEvaluator(tables_for(name, capi.FEATURES_INTERACTIONS))
    nat = ev.natural_parameters()
    states = np.array(list(itertools.product(range(2), repeat=8)), dtype=np.int32)
    feat = np.array([ev.feature_vector(o) for o in states])
    E = feat @ nat
    return E, feat


def test_microcanonical_and_canonical_are_exact():
    E, feat = _enumerated()
    # the levels: enthalpies closer than 1e-9 of the range are one level (symmetry-equivalent states differ by rounding)
    order = np.argsort(E)
    gaps = np.diff(E[order])
    tol = 1e-9 * (E.max() - E.min())
    level_of = np.empty(len(E), dtype=np.int64)
    level_of[order] = np.r_[0, np.cumsum(gaps > tol)]
    n_levels = level_of.max() + 1
    spacing = gaps[gaps > tol].min()
    assert 2 < n_levels <= 256
    kbin = spacing / 4
    kmin = E.min() - kbin / 2
    n_keys = int((E.max() - kmin) // kbin) + 1
    assert n_keys <= st.MAX_KEYS
    F = feat.shape[1]
    spec = Statistics.by_bin(st.ENTHALPY, n_keys, kmin, kbin, columns=[st.ENTHALPY] + [st.feature(i) for i in range(min(F, 8))])
    rec = StatisticsRecord(spec).offer(E[None, :], feat[None, :, :])  # every state once
    x = spec.column_values(E, feat)
    key = st.bin_of(E, kmin, kbin).astype(np.int64)
    assert rec.key_under == rec.key_over == 0 and rec.n.sum() == 256
    assert len(np.unique(key)) == n_levels and all(len(np.unique(key[level_of == l])) == 1 for l in range(n_levels))
    occupied = np.flatnonzero(rec.n)
    # the exact per-level means
    micro = rec.microcanonical()
    assert np.isnan(micro[rec.n == 0]).all()
    for k in occupied:
        np.testing.assert_allclose(micro[k], x[key == k].mean(axis=0), rtol=1e-12, atol=1e-12 * np.abs(x).max())
        np.testing.assert_allclose(rec.microcanonical_covariance()[k], np.cov(x[key == k].T, ddof=0), rtol=1e-9,
                                   atol=1e-12 * np.abs(x).max() ** 2)
    np.testing.assert_allclose(rec.key_centres(), 0.5 * (rec.key_edges()[:-1] + rec.key_edges()[1:]), rtol=1e-14)
    # canonical averages against the brute-force Boltzmann sums over the 256 states
    with np.errstate(divide="ignore"):
        ln_g = np.log(rec.n.astype(np.float64))  # (-inf on the empty keys: left out)
    temps = np.array([0.25, 1.0, 4.0]) * spacing / st.KB  # kB T below, at and above the level spacing
    got = rec.canonical(ln_g, temps)
    got_c = rec.canonical_heat_capacity(ln_g, temps)
    for i, T in enumerate(temps):
        w = np.exp(-(E - E.min()) / (st.KB * T))
        w /= w.sum()
        np.testing.assert_allclose(got[i], w @ x, rtol=1e-12, atol=1e-12 * np.abs(x).max())
        e = E - E.min()
        var = w @ (e - w @ e) ** 2
        np.testing.assert_allclose(got_c[i], var / (st.KB * T * T), rtol=1e-12)
    assert got_c[0] < got_c[1]  # (well below the spacing the heat capacity dies out)
    # level_values / bin centres stand in for the enthalpy when it is no column
    j = int(np.argmax(np.ptp(feat, axis=0)))  # (a feature that moves)
    nospec = Statistics.by_bin(st.feature(j), 4, float(feat[:, j].min()), float(np.ptp(feat[:, j])) / 3.5, columns=[st.feature(j)])
    r2 = StatisticsRecord(nospec).offer(E[None, :], feat[None, :, :])
    assert (r2.n > 0).sum() >= 2
    flat = r2.canonical(np.zeros(4), [1000.0], level_values=np.zeros(4))  # (equal weights on the occupied keys)
    np.testing.assert_allclose(flat[0], r2.mean()[r2.n > 0].mean(axis=0), rtol=1e-12)
    assert np.isfinite(r2.canonical(np.zeros(4), [1000.0])).all()
    with pytest.raises(ValueError, match="has no column"):
        r2.canonical_heat_capacity(np.zeros(4), [1000.0])


# ---- 4: record handling ---------------------------------------------------------------------------------------------------
def test_combine_and_the_methods_that_refuse():
    rng = np.random.default_rng(8)
    ns, R = 12, 19
    H, f = _synthetic(rng, ns, R)
    H[3, 3] = np.nan
    spec = Statistics.by_bin(st.ENTHALPY, 6, -3.0, 1.0, columns=[st.ENTHALPY, st.feature(0), st.feature(1)],
                             hist=(st.feature(0), 5, -2.0, 0.8))
    whole = StatisticsRecord(spec).offer(H, f)
    halves = [StatisticsRecord(spec).offer(H[:5], f[:5]), StatisticsRecord(spec).offer(H[5:], f[5:])]
    both = StatisticsRecord.combine(halves)
    for name in ("n", "hist", "under", "over"):
        np.testing.assert_array_equal(getattr(both, name), getattr(whole, name), err_msg=name)
    assert (both.key_under, both.key_over) == (whole.key_under, whole.key_over) and whole.key_under > 0 and whole.key_over > 0
    assert both.spec.binned and both.spec.c_bins() == spec.c_bins() and both.n_keys == 6
    n = whole.n.max()
    scale = np.abs(spec.column_values(np.nan_to_num(H), f)).max(axis=(0, 1))
    eps = np.finfo(float).eps
    live = whole.n > 0
    assert (np.abs(both.mean() - whole.mean())[live] <= 8 * n * eps * scale).all()
    assert (np.abs(both.covariance() - whole.covariance())[live] <= 16 * n * eps * scale[:, None] * scale[None, :]).all()
    # mixed modes, and bins that differ
    walker = StatisticsRecord(Statistics.per_walker([st.ENTHALPY, st.feature(0), st.feature(1)]), 6)
    with pytest.raises(ValueError, match="different key modes"):
        StatisticsRecord.combine([whole, walker])
    other = StatisticsRecord(Statistics.by_bin(st.ENTHALPY, 6, -3.0, 2.0, columns=[st.ENTHALPY, st.feature(0), st.feature(1)]))
    with pytest.raises(ValueError, match="different bins"):
        StatisticsRecord.combine([whole, other])
    for call in (whole.blocking, whole.standard_error, whole.autocorrelation_time, lambda: whole.reweight(1000.0, 900.0)):
        with pytest.raises(ValueError, match="keyed by bin \\(mode 2"):
            call()
    with pytest.raises(ValueError, match="needs a record keyed by bin"):
        walker.microcanonical()
    with pytest.raises(ValueError, match="key_of_row"):
        StatisticsRecord(spec).offer(H, f, key_of_row=np.arange(R))
    assert whole.copy().equals(whole) and not whole.copy().equals(both.offer(H[:1], f[:1]))


def test_spec_constructors():
    class Obs:
        n_kinds, kind_names = 3, ["A", "B", "Vac"]

    s = Statistics.by_composition(Obs, "B", 64)
    assert s.binned and s.key == st.BY_BIN == 2 and s.c_bins() == (0, 65, 0.0, 1.0) and s.columns == [("kind", 1), st.ENTHALPY]
    s = Statistics.by_composition(Obs, 2, 8, columns=[st.ENTHALPY, st.feature(1)])
    assert s.columns[0] == ("kind", 2) and s.key_column == 0 and s.n_keys == 9 and s.n_levels == 0
    s = Statistics.on_wl_levels(-1.5, 0.25, 12, columns=[st.feature(0)])
    assert s.columns == [st.ENTHALPY, st.feature(0)] and s.c_bins() == (0, 12, -1.5, 0.25)
    with pytest.raises(ValueError, match="key's column must be one of the record's columns"):
        Statistics.by_bin(st.feature(3), 4, 0.0, 1.0, columns=[st.ENTHALPY])
    plain = Statistics(2, [st.ENTHALPY])  # (key 2 without bins: not binned, the engine refuses it)
    assert not plain.binned and plain.c_bins() is None
    struct, keep = s.c_struct(4, 0)
    assert struct.key == 2 and struct.n_levels == 0 and struct.n_columns == 2


# ---- 5: the ABI -------------------------------------------------------------------------------------------------------------
def test_header_capi_and_engine_agree():
    text = open(os.path.join(ROOT, "include", "smolmc.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)

    def proto(name):
        return [" ".join(a.split()) for a in re.search(rf"int {name}\((.*?)\);", code, re.S).group(1).split(",")]

    assert proto("smolmc_set_statistics_binned") == ["smolmc_handle *h", "const smolmc_statistics *s", "int key_column", "int n_keys",
                                                     "double key_min", "double key_bin"]
    assert proto("smolmc_statistics_bins") == ["smolmc_handle *h", "int *key_column", "int *n_keys", "double *key_min",
                                               "double *key_bin", "int64_t *key_under", "int64_t *key_over"]
    assert proto("smolmc_set_statistics") == ["smolmc_handle *h", "const smolmc_statistics *s"]  # (unchanged)
    assert int(re.search(r"#define SMOLMC_STAT_BY_BIN (\d+)", text).group(1)) == capi.STAT_BY_BIN == st.BY_BIN == 2
    assert int(re.search(r"#define SMOLMC_MAX_STAT_KEYS (\d+)", text).group(1)) == capi.MAX_STAT_KEYS == st.MAX_KEYS == 65536
    assert capi.ABI_VERSION == int(re.search(r"#define SMOLMC_ABI_VERSION (\d+)", text).group(1)) == 8
    res, args = engine.SYMBOLS["smolmc_set_statistics_binned"]
    assert res is C.c_int and args == [C.c_void_p, C.POINTER(capi.smolmc_statistics), C.c_int, C.c_int, C.c_double, C.c_double]
    res, args = engine.SYMBOLS["smolmc_statistics_bins"]
    assert res is C.c_int and args == [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double),
                                       C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    # the struct did not change
    fields = re.search(r"typedef struct smolmc_statistics \{(.*?)\} smolmc_statistics;", code, re.S).group(1)
    names = re.findall(r"(\w+)\s*[,;]", fields)
    assert names == [f[0] for f in capi.smolmc_statistics._fields_] == ["key", "n_columns", "columns", "n_weights", "weights", "n_levels",
                                                                       "hist_column", "n_bins", "hist_min", "hist_bin"]
