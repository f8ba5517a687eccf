"""The statistics record on the device (csrc/statistics.hip; smolmc_set_statistics, SMOLMC_SAMPLE_STATISTICS,
smolmc_update_statistics): every array of the record equals statistics.StatisticsRecord.offer, the NumPy definition, fed
with the fetched columns -- array_equal, no tolerance -- and a run with the flag is the same chain as a run without."""

import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from smol_amd import capi, moca
from smol_amd import statistics as st
from smol_amd.observables import Observables
from smol_amd.statistics import Statistics, StatisticsRecord
from tests.cases import load_case, tables_for
from tests.test_gpu_observables import ENV, _handle, _rand_occ

pytestmark = pytest.mark.gpu
INT = capi.FEATURES_INTERACTIONS
BLOCKS = (1, 3, 67)  # 71 offers: pending blocks cross the block boundaries, levels 0..6 fill
THIN = 5
EPS = np.finfo(float).eps


@pytest.fixture
def clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def _same_record(got, want, what=""):
    for f in st._ARRAYS:
        g, w = getattr(got, f), getattr(want, f)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, f, g.dtype, g.shape, w.dtype, w.shape)
        np.testing.assert_array_equal(g, w, err_msg=f"{what} {f}")


def _semigrand(name, R, mu=0.15, mode=INT):
    """A semigrand flip handle of a golden case with its default observables: (engine, observables, supercell)."""
    from smol_amd.engine import Engine

    sc = load_case(name)["sc"]
    nsp = max(sc.model.prim.nspecies)
    table = np.zeros((sc.num_sites, nsp))
    table[:, 1:] = mu * np.arange(1, nsp)
    tab = tables_for(name, mode, mu_table=table)
    eng = Engine(tab, capi.make_config(R, capi.KERNEL_METROPOLIS, capi.STEP_FLIP))
    obs = Observables.from_supercell(sc, tables=tab)
    eng.set_observables(obs)
    return eng, obs, sc


def _run_blocks(eng, sizes=BLOCKS, thin=THIN, before_block=None, **kw):
    """Two blocks queued before the first fetch, then the rest: the fetched blocks in order."""
    out = []
    for i, ns in enumerate(sizes):
        if before_block is not None:
            before_block(i)
        eng.run_sampled_async(ns, thin, statistics=True, **kw)
        if i > 0:
            out.append(eng.fetch_samples())
    out.append(eng.fetch_samples())
    return out


def _offer_blocks(rec, blocks, keys=None):
    for i, b in enumerate(blocks):
        rec.offer(b["enthalpy"], b["features"], b.get("species_counts"), None if keys is None else keys[i])
    return rec


def _all_sources(eng, obs):
    return ([st.ENTHALPY] + [st.feature(i) for i in range(eng.F)] + [st.kind(obs, k) for k in range(obs.n_kinds)] + [st.ENERGY])


def _specs(eng, obs, sc, H):
    """H: enthalpies of a dry run, to place the histogram that leaves rows outside."""
    nat = eng.natural_parameters
    lo, hi = float(H.min()), float(H.max())
    return {
        "enthalpy": Statistics.per_walker([st.ENTHALPY], n_levels=8),
        # every source; the products d_a d_b of features and of the left-to-right energy agree only unfused
        "everything": Statistics.per_walker(_all_sources(eng, obs), weights=nat[:-1], n_levels=8,
                                            hist=(st.kind(obs, 1), sc.num_sites + 1, 0.0, 1.0)),
        "wide": Statistics.per_walker(_all_sources(eng, obs)[:32], weights=nat[:-1], n_levels=0),
        # the middle half of the enthalpies seen: rows in under and in over
        "outside": Statistics.per_walker([st.feature(0), st.ENTHALPY], n_levels=3,
                                         hist=(st.ENTHALPY, 7, lo + 0.25 * (hi - lo), (hi - lo) / 14)),
    }


# ---- 1: the record equals the definition ----------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [3, 70])
@pytest.mark.parametrize("name", ["fcc_prim222_aliased", "fcc3_indicator_skew", "fcc_conv444_pairs"])
def test_record_equals_the_definition(name, R, clean_env):
    eng, obs, sc = _semigrand(name, R)
    occ0 = _rand_occ(sc, np.random.default_rng(5), R)
    seeds = np.arange(R, dtype=np.uint64) + np.uint64(11)
    eng.set_state(occ0, seeds, 3000.0)
    H = eng.run_sampled(sum(BLOCKS), THIN)["enthalpy"]
    for what, spec in _specs(eng, obs, sc, H).items():
        eng.set_statistics(spec)
        assert eng.statistics_shape() == (R, spec.n_columns, spec.n_levels, spec.n_bins)
        _same_record(eng.statistics(), StatisticsRecord(spec, R), what + " empty")
        eng.set_state(occ0, seeds, 3000.0)
        blocks = _run_blocks(eng, observables=True)
        got = eng.statistics()
        want = _offer_blocks(StatisticsRecord(spec, R), blocks)
        _same_record(got, want, what)
        assert (got.n == sum(BLOCKS)).all()
        if spec.n_levels == 8:  # 71 = 0b1000111: levels 0..6 took blocks, level 7 none
            assert (got.nb[:, :7] > 0).all() and (got.nb[:, 7] == 0).all() and (got.has[:, 0] == 0b1000111).all()
        if spec.n_bins:
            assert got.hist.sum() > 0
        if what == "outside":
            assert got.under.sum() > 0 and got.over.sum() > 0
        if what == "everything":
            # this spec tells fused from unfused arithmetic: the enthalpy-energy entry of s2 with every product folded
            # into its sum (an exact fma: rational arithmetic, rounded once) differs from the record
            x = np.concatenate([spec.column_values(b["enthalpy"], b["features"], b["species_counts"]) for b in blocks])
            d = x - x[0]
            e = spec.n_columns - 1  # (row 0 of the triangle: entry e is s2[H, E])
            fused = np.zeros(R)
            for r in range(R):
                acc = 0.0
                for s in range(len(d)):
                    acc = float(Fraction(float(d[s, r, 0])) * Fraction(float(d[s, r, e])) + Fraction(acc))
                fused[r] = acc
            print(name, R, "walkers whose s2[H, E] differs when fused:", int((fused != got.s2[:, e]).sum()), "of", R)
            if name == "fcc_conv444_pairs":  # (256 sites: enthalpy and energy differences with many significant bits)
                assert (fused != got.s2[:, e]).any()
        # the same record with nothing but the statistics asked for: counts and rows stay on the device
        eng.set_statistics(spec)
        eng.set_state(occ0, seeds, 3000.0)
        dry = _run_blocks(eng, occupancy=False)
        assert all(d["occupancy"] is None and "species_counts" not in d for d in dry)
        _same_record(eng.statistics(), want, what + " alone")
    eng.close()


def test_thirty_two_columns(clean_env):
    """C = 32: the upper triangle has 528 entries, three to a thread.  The correlation-function tables of the rocksalt case
    give 27 features."""
    R = 70
    eng, obs, sc = _semigrand("rocksalt333_two_sublattices", R, mode=capi.FEATURES_CORRELATIONS)
    cols = _all_sources(eng, obs)
    assert len(cols) >= 32
    cols = cols[:1] + cols[-31:]  # (the enthalpy, the last features, every kind, the energy)
    spec = Statistics.per_walker(cols, weights=eng.natural_parameters[:-1], n_levels=0)
    assert spec.n_columns == 32 and spec.n_pairs == 528
    eng.set_statistics(spec)
    eng.set_state(_rand_occ(sc, np.random.default_rng(4), R), np.arange(R, dtype=np.uint64) + np.uint64(2), 3000.0)
    blocks = _run_blocks(eng, sizes=(2, 40, 5), observables=True)
    _same_record(eng.statistics(), _offer_blocks(StatisticsRecord(spec, R), blocks), "C = 32")
    eng.close()


# ---- 2: the chain is untouched ---------------------------------------------------------------------------------------------
def test_chains_do_not_change(clean_env):
    fn = None
    for which in ("lean", "lazy", "wang-landau"):
        got = []
        for with_stat in (False, True):
            eng, obs, occ, kw = _handle(which, 5, clean_env)
            fn = eng._lib.smolmc_debug_block_bytes
            fn.restype, fn.argtypes = C.c_longlong, [C.c_void_p]
            eng.set_statistics(Statistics.per_walker([st.ENTHALPY, st.feature(0)], n_levels=4, hist=(st.ENTHALPY, 8, -1.0, 0.5)))
            eng.run(13)
            eng.run_sampled_async(4, 9, statistics=with_stat, **kw)
            size = fn(eng._h)
            blocks = [eng.fetch_samples(), eng.run_sampled(2, 5, statistics=with_stat, **kw)]
            got.append((blocks, eng.get_state(), eng.statistics(), size))
            eng.close()
        (plain, st0, rec0, size0), (kept, st1, rec1, size1) = got
        assert size0 == size1 > 0, which  # (the downloaded part of the block is the flagless block's)
        for p, c in zip(plain, kept):
            assert set(p) == set(c)
            for key in p:
                assert np.array_equal(p[key], c[key]), (which, key)
        for key in st0:
            assert np.array_equal(st0[key], st1[key]), (which, key)
        assert (rec0.n == 0).all() and (rec1.n == 6).all()
        _same_record(rec1, _offer_blocks(StatisticsRecord(rec1.spec, 5), kept), which)


# ---- 3: by state point -------------------------------------------------------------------------------------------------------
def test_by_state_point_follows_the_exchanges(clean_env):
    R = 6
    eng, obs, sc = _semigrand("fcc_conv444_pairs", R)
    rows = np.zeros(eng._mu_shape())
    rows[:, 0, 1] = np.linspace(-0.2, 0.2, R)
    eng.set_walker_mu(rows)
    temps = np.linspace(2500.0, 4000.0, R)
    occ0 = _rand_occ(sc, np.random.default_rng(9), R)
    seeds = np.arange(R, dtype=np.uint64) + np.uint64(21)
    cols = [st.ENTHALPY, st.kind(obs, 1), st.feature(0)]
    even, odd = np.array([[0, 1], [2, 3], [4, 5]]), np.array([[1, 2], [3, 4]])
    records = {}
    for what, spec in (("point", Statistics.by_state_point(cols, n_levels=5, hist=(st.kind(obs, 1), sc.num_sites + 1, 0.0, 1.0))),
                       ("walker", Statistics.per_walker(cols, n_levels=5, hist=(st.kind(obs, 1), sc.num_sites + 1, 0.0, 1.0)))):
        eng.set_walker_mu(rows)  # (the walkers' points are named afresh: point p is walker p)
        eng.set_state(occ0, seeds, temps)
        eng.set_statistics(spec)
        keys = []

        def exchange(i):
            if i > 0:  # every pair accepted: even pairs, then odd pairs, ...
                pairs = even if i % 2 else odd
                eng.exchange_grid(pairs, np.full(len(pairs), -np.inf))
            keys.append(eng.state_points()[0].copy())

        blocks = _run_blocks(eng, sizes=(3, 4, 2, 6, 5), thin=7, before_block=exchange, observables=True)
        assert not np.array_equal(keys[-1], np.arange(R)) and all(sorted(k) == list(range(R)) for k in keys)
        got = eng.statistics()
        want = _offer_blocks(StatisticsRecord(spec, R), blocks, keys if what == "point" else None)
        _same_record(got, want, what)
        records[what] = got
    assert not np.array_equal(records["point"].s1, records["walker"].s1)
    assert not np.array_equal(records["point"].hist, records["walker"].hist)
    eng.close()


# ---- 4: between runs ---------------------------------------------------------------------------------------------------------
def test_between_runs_and_refusals(clean_env):
    from smol_amd.engine import EngineError

    R = 6
    eng, obs, sc = _semigrand("fcc_conv444_pairs", R)
    N, K, F = sc.num_sites, obs.n_kinds, eng.F
    err = (EngineError, ValueError)
    occ0 = _rand_occ(sc, np.random.default_rng(8), R)
    spec = Statistics.per_walker([st.ENTHALPY, st.kind(obs, 0), st.ENERGY], weights=eng.natural_parameters[:-1], n_levels=3,
                                 hist=(st.kind(obs, 0), N + 1, 0.0, 1.0))
    eng.set_statistics(spec)
    want = StatisticsRecord(spec, R)
    eng.set_state(occ0, np.arange(R, dtype=np.uint64), 3000.0)
    for n in (40, 25, 1):  # update_statistics after run: one offer of the current states
        eng.run(n)
        eng.update_statistics()
        s = eng.get_state()
        want.offer(s["enthalpy"], s["features"], obs.evaluate(s["occupancy"])[0])
        _same_record(eng.statistics(), want, "update")
    # set_state and discard_samples keep the record; ring offers continue it
    eng.set_state(occ0, np.arange(R, dtype=np.uint64) + np.uint64(50), 3000.0)
    _same_record(eng.statistics(), want, "set_state")
    eng.run_sampled_async(3, 7, statistics=True)
    eng.discard_samples()
    kept = eng.statistics()
    assert (kept.n == 6).all()
    eng.set_state(occ0, np.arange(R, dtype=np.uint64) + np.uint64(50), 3000.0)
    b = eng.run_sampled(3, 7, observables=True)  # (the same chain again, fetched this time)
    _offer_blocks(want, [b])
    _same_record(kept, want, "discard")
    eng.reset_statistics()
    _same_record(eng.statistics(), StatisticsRecord(spec, R), "reset")
    eng.update_statistics()
    assert (eng.statistics().n == 1).all()

    # the refusals, each by its message; the record in force stays as it was
    before = eng.statistics()
    shape = eng.statistics_shape()

    def refused(match, *args, **kw):
        with pytest.raises(err, match=match):
            eng.set_statistics(Statistics(*args, **kw))
        assert eng.statistics_shape() == shape
        _same_record(eng.statistics(), before, match)

    refused("key must be 0 \\(by walker\\) or 1 \\(by state point\\), got 2", 2, [st.ENTHALPY])
    refused("n_columns must be 1..32, got 0", 0, [])
    refused("n_columns must be 1..32, got 33", 0, [("source", 0)] * 33)
    refused("source 0 is named twice \\(columns 0 and 2\\)", 0, [st.ENTHALPY, st.feature(0), st.ENTHALPY])
    refused(f"column 1 has source {2 + F + K}, outside", 0, [st.ENTHALPY, ("source", 2 + F + K)])
    refused("column 0 has source -1, outside", 0, [("source", -1)])
    refused("n_weights = 99 is larger than the handle's", 0, [st.ENERGY], weights=np.ones(99))
    refused("n_levels must be 0..32, got 33", 0, [st.ENTHALPY], n_levels=33)
    refused("n_levels must be 0..32, got -1", 0, [st.ENTHALPY], n_levels=-1)
    refused("n_bins must be 0..65536, got 65537", 0, [st.ENTHALPY], hist=(st.ENTHALPY, 65537, 0.0, 1.0))
    refused("hist_bin must be a positive finite number", 0, [st.ENTHALPY], hist=(st.ENTHALPY, 4, 0.0, 0.0))
    refused("hist_bin must be a positive finite number", 0, [st.ENTHALPY], hist=(st.ENTHALPY, 4, 0.0, -1.0))
    bad = Statistics(0, [st.ENTHALPY], hist=(st.ENTHALPY, 4, 0.0, 1.0))
    bad.hist_column = 1
    with pytest.raises(err, match="hist_column = 1 is no index into the 1 columns"):
        eng.set_statistics(bad)
    # 6 keys x 32 levels x 32 columns is small; 65536 bins x 8 bytes x R must pass 1 GiB to be refused: not with R = 6
    _same_record(eng.statistics(), before, "after the refusals")
    with pytest.raises(err, match="while a statistics record with count columns depends on the observables"):
        eng.set_observables(None)
    with pytest.raises(err, match="while a statistics record with count columns depends on the observables"):
        eng.set_observables(obs)
    assert eng.observables_shape() == (K, obs.n_shells)
    _same_record(eng.statistics(), before, "after set_observables")
    eng.set_statistics(None)
    assert eng.statistics_shape() == (0, 0, 0, 0)
    with pytest.raises(err, match="SMOLMC_SAMPLE_STATISTICS without a statistics record"):
        eng.run_sampled_async(1, 5, statistics=True)
    assert eng.pending_samples()[0] == 0
    with pytest.raises(err, match="no statistics record set"):
        eng.update_statistics()
    with pytest.raises(err, match="no statistics record set"):
        eng.reset_statistics()
    # without observables a count column has no source; the other columns work, and set_observables is free again
    eng.set_observables(None)
    with pytest.raises(err, match="a kind count needs observables"):
        eng.set_statistics(Statistics.per_walker([st.ENTHALPY, ("source", 2 + F)]))
    assert eng.statistics_shape() == (0, 0, 0, 0)
    plain = Statistics.per_walker([st.ENTHALPY, st.ENERGY], weights=eng.natural_parameters[:-1], n_levels=2)
    eng.set_statistics(plain)
    b = eng.run_sampled(5, 5, statistics=True)
    _same_record(eng.statistics(), _offer_blocks(StatisticsRecord(plain, R), [b]), "no observables")
    eng.set_observables(obs)
    eng.close()


def test_refused_on_wang_landau_windows_and_beyond_one_gib(clean_env):
    from smol_amd.engine import Engine, EngineError
    from smol_amd import synth

    err = (EngineError, ValueError)
    eng, obs, occ, kw = _handle("wang-landau", 4, clean_env)
    vmin, vmax, _ = eng.wl_windows()  # (the config's window: set for every walker below, it is a valid set of windows)
    eng.set_statistics(Statistics.by_state_point([st.ENTHALPY]))  # (no windows set: allowed)
    eng.set_statistics(None)
    eng.set_wl_windows(vmin, vmax)
    with pytest.raises(err, match="keyed by state point on a Wang-Landau handle with per-walker windows"):
        eng.set_statistics(Statistics.by_state_point([st.ENTHALPY]))
    assert eng.statistics_shape() == (0, 0, 0, 0)
    eng.set_statistics(Statistics.per_walker([st.ENTHALPY]))
    assert eng.statistics_shape() == (4, 1, 0, 0)
    eng.close()
    # 4096 walkers x 65536 bins x 8 bytes = 2 GiB
    sc = synth.build_supercell(synth.build_cluster_model(synth.fcc_prim(), {2: 3.0}), [2, 2, 2])
    big = Engine(capi.TableSet.from_synth(sc, synth.random_coefs(sc.model), feature_mode=INT), capi.make_config(4096))
    with pytest.raises(err, match="is larger than 1 GiB"):
        big.set_statistics(Statistics.per_walker([st.ENTHALPY], hist=(st.ENTHALPY, 65536, 0.0, 1.0)))
    assert big.statistics_shape() == (0, 0, 0, 0)
    big.set_statistics(Statistics.per_walker([st.ENTHALPY], hist=(st.ENTHALPY, 1024, 0.0, 1.0)))
    assert big.statistics_shape() == (4096, 1, 0, 1024)
    big.close()


# ---- 5: the sampler ---------------------------------------------------------------------------------------------------------
def test_sampler_averages_agree_with_the_trace(clean_env):
    c = load_case("rocksalt333_two_sublattices")
    nw, T = 6, 3000.0
    ens = moca.Ensemble.from_cluster_expansion(c["sc"], c["coefs"])
    ens.chemical_potentials = {sp: 0.1 * (i - 1) for i, sp in enumerate(ens.species)}
    obs = Observables.from_supercell(c["sc"])
    K = obs.n_kinds
    spec = Statistics.per_walker([st.ENTHALPY] + [st.kind(obs, k) for k in range(K)], n_levels=4)
    s = moca.Sampler.from_ensemble(ens, temperature=T, nwalkers=nw, seeds=list(range(3, 3 + nw)), rank=0, world_size=1,
                                   observables=obs, statistics=spec)
    occ = _rand_occ(c["sc"], np.random.default_rng(12), nw)
    s.run(40 * 9, occ, thin_by=9)
    s.run(25 * 9, thin_by=9)  # (a second run: the record goes on)
    rec = s.statistics
    n = 65
    assert (rec.n == n).all()
    H = s.samples.get_trace_value("enthalpy", flat=False)[:, :, 0]
    cnt = s.samples.get_trace_value("species_counts", flat=False).astype(np.float64)
    x = np.concatenate([H[:, :, None], cnt], axis=2)  # (n, nw, C)
    d = np.abs(x - x[0]).max(axis=0)                  # (nw, C)
    bound = 4 * n * EPS * d[:, :, None] * d[:, None, :]
    cov = np.stack([np.cov(x[:, r].T, ddof=0) for r in range(nw)])
    assert (np.abs(rec.mean() - x.mean(axis=0)) <= 4 * n * EPS * d).all()
    assert (np.abs(rec.covariance() - cov) <= bound).all()
    kT2, beta = st.KB * T * T, 1.0 / (st.KB * T)
    assert (np.abs(rec.heat_capacity(T) - cov[:, 0, 0] / kT2) <= bound[:, 0, 0] / kT2 * (1 + 4 * EPS)).all()
    assert (np.abs(rec.susceptibility(T) - beta * cov[:, 1:, 1:]) <= beta * bound[:, 1:, 1:] * (1 + 4 * EPS)).all()
    assert cov[:, 1, 1].min() > 0  # (a semigrand run: the counts move)
    assert np.isfinite(rec.standard_error(min_blocks=4)).all()
    s.reset_statistics()
    assert (s.statistics.n == 0).all()
    with pytest.raises(ValueError, match="keeps no statistics record"):
        moca.Sampler.from_ensemble(ens, temperature=T, nwalkers=2, seeds=[1, 2], rank=0, world_size=1).statistics


def test_sampler_exchange_run_by_state_point(clean_env):
    from smol_amd import synth

    model = synth.build_cluster_model(synth.rocksalt_prim(), {2: 3.5})
    sc = synth.build_supercell(model, [3, 3, 3])
    ens = moca.Ensemble.from_cluster_expansion(sc, synth.random_coefs(model, seed=5, scale=0.05))
    names = ens.species
    ens.chemical_potentials = {names[0]: 0.1, names[1]: -0.2, names[2]: 0.05}
    temps = [3000.0, 3600.0, 4500.0]
    mus = [{names[0]: 0.1, names[1]: -0.2 + dm, names[2]: 0.05} for dm in np.linspace(-0.15, 0.15, 4)]
    nw = 12
    sampler = moca.Sampler.from_ensemble(ens, temperature=3000.0, nwalkers=nw, seeds=list(range(11, 11 + nw)),
                                         statistics=Statistics.by_state_point([st.ENTHALPY], n_levels=2))
    rng = np.random.default_rng(2)
    occ = np.zeros((nw, ens.num_sites), dtype=np.int32)
    occ[:, : sc.size] = rng.integers(0, 3, size=(nw, sc.size))
    gx = sampler.run_exchange(8, 200, occ, thin_by=100, grid=dict(temperatures=temps, chemical_potentials=mus, seed=4))
    assert 0 < gx.acceptance
    by = sampler.samples.by_state_point("enthalpy")[:, :, 0]  # (points, samples)
    n = by.shape[1]
    rec = sampler.statistics
    assert n == 16 and (rec.n == n).all()
    d = np.abs(by - by[:, :1]).max(axis=1)
    assert (np.abs(rec.mean()[:, 0] - by.mean(axis=1)) <= 4 * n * EPS * d).all()
    assert (np.abs(rec.variance()[:, 0] - by.var(axis=1)) <= 4 * n * EPS * d * d).all()
    H = sampler.samples.get_trace_value("enthalpy", flat=False)[:, :, 0]
    assert not (np.abs(rec.mean()[:, 0] - H.mean(axis=0)) <= 4 * n * EPS * d).all()  # (the walkers' means are others)
