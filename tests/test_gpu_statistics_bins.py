"""The statistics record keyed by bins of a column on the device (csrc/statistics.hip: the key pass and the reduction per
key, modes 1 and 2 of statistics_kernel; smolmc_set_statistics_binned, smolmc_statistics_bins): every array of the record
equals statistics.StatisticsRecord.offer in bin mode, the NumPy definition, fed with the fetched columns -- array_equal,
no tolerance, the two outside counters included -- and a run with the record is the same chain as a run without."""

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
BLOCKS = (1, 3, 67)  # 71 samples; two blocks queued before the first fetch
THIN = 5


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
    assert (got.key_under, got.key_over) == (want.key_under, want.key_over), what


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


def _run_blocks(eng, sizes=BLOCKS, thin=THIN, **kw):
    """Two blocks queued before the first fetch, then the rest: the fetched blocks in order."""
    out = []
    for i, ns in enumerate(sizes):
        eng.run_sampled_async(ns, thin, statistics=True, **kw)
        if i > 0:
            out.append(eng.fetch_samples())
    out.append(eng.fetch_samples())
    return out


def _offer_blocks(rec, blocks, reverse=False):
    flip = (lambda a: None if a is None else a[:, ::-1]) if reverse else (lambda a: a)
    for b in blocks:
        rec.offer(flip(b["enthalpy"]), flip(b["features"]), flip(b.get("species_counts")))
    return rec


def _all_sources(eng, obs):
    return ([st.ENTHALPY] + [st.feature(i) for i in range(eng.F)] + [st.kind(obs, k) for k in range(obs.n_kinds)] + [st.ENERGY])


def _specs(eng, obs, sc, H):
    """H: enthalpies of a dry run, to place bins that leave rows outside."""
    nat = eng.natural_parameters
    lo, hi = float(H.min()), float(H.max())
    mid, seventh = lo + 0.25 * (hi - lo), (hi - lo) / 14
    return {
        # (a) the middle half of the enthalpies seen in 7 bins: many rows per key, rows under and over
        "middle": Statistics.by_bin(st.ENTHALPY, 7, mid, seventh, columns=[st.feature(0), st.ENTHALPY, st.kind(obs, 1)]),
        # (b) per composition: N + 1 keys, mostly empty
        "composition": Statistics.by_composition(obs, 1, sc.num_sites),
        # (c) one key takes every row of the block in order
        "one": Statistics.by_bin(st.ENTHALPY, 1, lo - 1.0, (hi - lo) + 2.0, columns=[st.ENTHALPY, st.feature(eng.F - 1)]),
        # (d) the largest grid, the rows spread thin
        "thin": Statistics.by_bin(st.ENTHALPY, 65536, lo - (hi - lo) / 65000, (hi - lo) / 65000, columns=[st.ENTHALPY, st.kind(obs, 0)]),
        # (e) as many columns as the handle has sources, 32 at most (test_thirty_two_columns has a handle with 32)
        "wide": Statistics.by_bin(st.ENTHALPY, 7, mid, seventh, columns=_all_sources(eng, obs)[:32], weights=nat[:-1]),
        # (f) a histogram per key with rows in its own under and over
        "histogram": Statistics.by_composition(obs, 1, sc.num_sites, hist=(st.ENTHALPY, 7, mid, seventh)),
        # (g) every source; the products d_a d_b of features and of the left-to-right energy agree only unfused
        "everything": Statistics.by_bin(st.ENTHALPY, 9, lo - 0.3 * (hi - lo), 0.2 * (hi - lo), columns=_all_sources(eng, obs),
                                        weights=nat[:-1], hist=(st.kind(obs, 1), sc.num_sites + 1, 0.0, 1.0)),
    }


# ---- 1: the record equals the definition ----------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [3, 70, 300])
@pytest.mark.parametrize("name", ["fcc_prim222_aliased", "fcc_conv444_pairs"])
def test_record_equals_the_definition(name, R, clean_env):
    eng, obs, sc = _semigrand(name, R)
    occ0 = _rand_occ(sc, np.random.default_rng(5), R)
    seeds = np.arange(R, dtype=np.uint64) + np.uint64(11)
    eng.set_state(occ0, seeds, 3000.0)
    H = eng.run_sampled(sum(BLOCKS), THIN)["enthalpy"]
    order_shows = []
    for what, spec in _specs(eng, obs, sc, H).items():
        eng.set_statistics(spec)
        assert eng.statistics_shape() == (spec.n_keys, spec.n_columns, 0, spec.n_bins)
        assert eng.statistics_bins() == (spec.key_column, spec.n_keys, spec.key_min, spec.key_bin, 0, 0)
        _same_record(eng.statistics(), StatisticsRecord(spec), what + " empty")
        eng.set_state(occ0, seeds, 3000.0)
        blocks = _run_blocks(eng, observables=True)
        got = eng.statistics()
        want = _offer_blocks(StatisticsRecord(spec), blocks)
        _same_record(got, want, what)
        assert got.n.sum() + got.key_under + got.key_over == sum(BLOCKS) * R
        if what in ("middle", "wide"):
            assert got.key_under > 0 and got.key_over > 0 and got.n.max() > min(R, 32)
        if what == "composition":
            assert got.key_under == got.key_over == 0 and (name != "fcc_conv444_pairs" or (got.n == 0).sum() > 128)
        if what == "one":
            assert got.n[0] == sum(BLOCKS) * R
        if what == "thin":
            assert (got.n > 0).sum() > 1
        if what == "histogram":
            assert got.hist.sum() > 0 and got.under.sum() > 0 and got.over.sum() > 0
        if name == "fcc_conv444_pairs":
            # teeth: the rows of each sample in reversed walker order give other sums -- order is observable
            rev = _offer_blocks(StatisticsRecord(spec), blocks, reverse=True)
            np.testing.assert_array_equal(rev.n, got.n)
            if not (np.array_equal(rev.s1, got.s1) and np.array_equal(rev.s2, got.s2)):
                order_shows.append(what)
    print(name, R, "specs whose s1 or s2 differ with reversed walkers:", order_shows)
    if name == "fcc_conv444_pairs":  # (256 sites: differences with many significant bits)
        assert order_shows
    eng.close()


def test_thirty_two_columns(clean_env):
    """C = 32: the upper triangle has 528 entries, three to a thread.  The correlation-function tables of the rocksalt case
    give 27 features."""
    R = 70
    eng, obs, sc = _semigrand("rocksalt333_two_sublattices", R, mode=capi.FEATURES_CORRELATIONS)
    cols = _all_sources(eng, obs)
    assert len(cols) >= 32
    cols = cols[:1] + cols[-31:]  # (the enthalpy, the last features, every kind, the energy)
    eng.set_state(_rand_occ(sc, np.random.default_rng(4), R), np.arange(R, dtype=np.uint64) + np.uint64(2), 3000.0)
    H = eng.run_sampled(20, THIN)["enthalpy"]
    lo, hi = float(H.min()), float(H.max())
    spec = Statistics.by_bin(st.ENTHALPY, 5, lo + 0.2 * (hi - lo), 0.12 * (hi - lo), columns=cols, weights=eng.natural_parameters[:-1])
    assert spec.n_columns == 32 and spec.n_pairs == 528
    eng.set_statistics(spec)
    blocks = _run_blocks(eng, sizes=(2, 40, 5), observables=True)
    got = eng.statistics()
    _same_record(got, _offer_blocks(StatisticsRecord(spec), blocks), "C = 32")
    assert got.n.max() > 32 and got.key_under + got.key_over > 0
    eng.close()


# ---- 2: the other ways to offer ---------------------------------------------------------------------------------------------
def test_other_ways_to_offer(clean_env):
    R = 70
    eng, obs, sc = _semigrand("fcc_conv444_pairs", R)
    occ0 = _rand_occ(sc, np.random.default_rng(8), R)
    seeds = np.arange(R, dtype=np.uint64) + np.uint64(3)
    eng.set_state(occ0, seeds, 3000.0)
    H = eng.run_sampled(20, THIN)["enthalpy"]
    lo, hi = float(H.min()), float(H.max())
    spec = Statistics.by_bin(st.ENTHALPY, 7, lo + 0.25 * (hi - lo), (hi - lo) / 14, columns=[st.ENTHALPY, st.kind(obs, 1), st.ENERGY],
                             weights=eng.natural_parameters[:-1], hist=(st.kind(obs, 1), sc.num_sites + 1, 0.0, 1.0))
    eng.set_statistics(spec)
    eng.set_state(occ0, seeds, 3000.0)
    want = _offer_blocks(StatisticsRecord(spec), _run_blocks(eng, sizes=(2, 9, 4), observables=True))
    # the same record with nothing but the statistics asked for: counts and rows stay on the device
    eng.set_statistics(spec)
    eng.set_state(occ0, seeds, 3000.0)
    dry = _run_blocks(eng, sizes=(2, 9, 4), occupancy=False)
    assert all(d["occupancy"] is None and "species_counts" not in d for d in dry)
    _same_record(eng.statistics(), want, "alone")
    # update_statistics: exactly one sample of R rows
    for n in (40, 1):
        eng.run(n)
        eng.update_statistics()
        s = eng.get_state()
        before = want.n.sum() + want.key_under + want.key_over
        want.offer(s["enthalpy"], s["features"], obs.evaluate(s["occupancy"])[0])
        assert want.n.sum() + want.key_under + want.key_over == before + R
        _same_record(eng.statistics(), want, "update")
    # discard_samples and set_state leave the record alone; ring offers continue it
    eng.set_state(occ0, seeds + np.uint64(50), 3000.0)
    _same_record(eng.statistics(), want, "set_state")
    eng.run_sampled_async(3, 7, statistics=True)
    eng.discard_samples()
    kept = eng.statistics()
    eng.set_state(occ0, seeds + np.uint64(50), 3000.0)
    _offer_blocks(want, [eng.run_sampled(3, 7, observables=True)])  # (the same chain again, fetched this time)
    _same_record(kept, want, "discard")
    assert kept.key_under + kept.key_over > 0
    # reset: the empty record and zero outside counters
    eng.reset_statistics()
    _same_record(eng.statistics(), StatisticsRecord(spec), "reset")
    assert eng.statistics_bins()[4:] == (0, 0)
    eng.update_statistics()
    rec = eng.statistics()
    assert rec.n.sum() + rec.key_under + rec.key_over == R
    eng.close()


# ---- 3: the chain is untouched ---------------------------------------------------------------------------------------------
def test_chains_do_not_change(clean_env):
    for which in ("lean", "lazy", "wang-landau"):
        got = []
        for with_stat in (False, True):
            eng, obs, occ, kw = _handle(which, 5, clean_env)
            eng.set_statistics(Statistics.by_bin(st.ENTHALPY, 50, -500.0, 20.0, columns=[st.ENTHALPY, st.feature(0), st.kind(obs, 0)],
                                                 hist=(st.ENTHALPY, 8, -1.0, 0.5)))
            eng.run(13)
            eng.run_sampled_async(4, 9, statistics=with_stat, **kw)
            blocks = [eng.fetch_samples(), eng.run_sampled(2, 5, statistics=with_stat, **kw)]
            got.append((blocks, eng.get_state(), eng.statistics()))
            eng.close()
        (plain, st0, rec0), (kept, st1, rec1) = got
        for p, c in zip(plain, kept):
            assert set(p) == set(c)
            for key in p:
                assert np.array_equal(p[key], c[key]), (which, key)
        for key in st0:
            assert np.array_equal(st0[key], st1[key]), (which, key)
        assert rec0.n.sum() + rec0.key_under + rec0.key_over == 0 and rec1.n.sum() + rec1.key_under + rec1.key_over == 30


# ---- 4: a Wang-Landau handle -------------------------------------------------------------------------------------------------
def test_wang_landau_levels_and_windows(clean_env):
    R = 6
    eng, obs, occ, kw = _handle("wang-landau", R, clean_env)
    cfg = eng.config
    spec = Statistics.on_wl_levels(cfg.wl_min_enthalpy, cfg.wl_bin_size, eng.L, columns=[st.ENTHALPY, st.feature(0), st.kind(obs, 1)])
    assert spec.n_keys == eng.L and spec.key_column == 0
    eng.set_statistics(spec)
    blocks = _run_blocks(eng, sizes=(2, 5, 9), thin=11, observables=True, **kw)
    got = eng.statistics()
    _same_record(got, _offer_blocks(StatisticsRecord(spec), blocks), "levels")
    # key k is Wang-Landau level k: every walker stays inside the window, and the keys with rows are visited levels
    assert got.key_under == got.key_over == 0 and got.n.sum() == 16 * R
    visited = (eng.get_wl()["entropy"] > 0).any(axis=0)
    assert visited[got.n > 0].all()
    # with per-walker windows (the config's window for every walker: a valid set) it still sets and runs
    vmin, vmax, _ = eng.wl_windows()
    eng.set_wl_windows(vmin, vmax)
    eng.set_statistics(spec)
    blocks = _run_blocks(eng, sizes=(3, 4), thin=11, observables=True)  # (no Wang-Landau trace while windows are set)
    got = eng.statistics()
    _same_record(got, _offer_blocks(StatisticsRecord(spec), blocks), "windows")
    assert got.n.sum() == 7 * R
    eng.close()


# ---- 5: the refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_record_alone(clean_env):
    from smol_amd.engine import EngineError

    R = 6
    eng, obs, sc = _semigrand("fcc_conv444_pairs", R)
    err = (EngineError, ValueError)
    cols = [st.ENTHALPY, st.kind(obs, 0)]
    spec = Statistics.by_bin(st.kind(obs, 0), sc.num_sites + 1, 0.0, 1.0, columns=cols, hist=(st.ENTHALPY, 4, -1.0, 0.5))
    eng.set_statistics(spec)
    eng.set_state(_rand_occ(sc, np.random.default_rng(8), R), np.arange(R, dtype=np.uint64), 3000.0)
    eng.run_sampled(4, 5, statistics=True)
    before, shape, bins = eng.statistics(), eng.statistics_shape(), eng.statistics_bins()
    assert before.n.sum() == 4 * R

    def refused(match, bad):
        with pytest.raises(err, match=match):
            eng.set_statistics(bad)
        assert eng.statistics_shape() == shape and eng.statistics_bins() == bins
        _same_record(eng.statistics(), before, match)

    def binned(**change):
        s = Statistics.by_bin(st.ENTHALPY, 8, 0.0, 1.0, columns=cols)
        for k, v in change.items():
            setattr(s, k, v)
        return s

    refused("n_levels must be 0, got 3", binned(n_levels=3))
    refused("n_keys must be 1..65536, got 0", binned(n_keys=0))
    refused("n_keys must be 1..65536, got 65537", binned(n_keys=65537))
    refused("key_bin must be a positive finite number and key_min finite", binned(key_bin=0.0))
    refused("key_bin must be a positive finite number and key_min finite", binned(key_bin=-1.0))
    refused("key_bin must be a positive finite number and key_min finite", binned(key_bin=float("inf")))
    refused("key_bin must be a positive finite number and key_min finite", binned(key_min=float("nan")))
    refused("key_column = 2 is no index into the 2 columns", binned(key_column=2))
    refused("key_column = -1 is no index into the 2 columns", binned(key_column=-1))
    refused("a binned record has key 2 \\(by bin\\), got 0", binned(key=0))
    # 65536 keys x 65536 bins x 8 bytes: far beyond 1 GiB
    refused("is larger than 1 GiB", Statistics.by_bin(st.ENTHALPY, 65536, 0.0, 1.0, columns=cols, hist=(st.ENTHALPY, 65536, 0.0, 1.0)))
    # the checks smolmc_set_statistics makes
    refused("source 0 is named twice", Statistics.by_bin(st.ENTHALPY, 8, 0.0, 1.0, columns=[st.ENTHALPY, st.feature(0), st.ENTHALPY]))
    refused("n_bins must be 0..65536, got 65537", Statistics.by_bin(st.ENTHALPY, 8, 0.0, 1.0, columns=cols, hist=(st.ENTHALPY, 65537, 0.0, 1.0)))
    # key 2 without bins goes to smolmc_set_statistics and is refused with its text
    refused("key must be 0 \\(by walker\\) or 1 \\(by state point\\), got 2", Statistics(2, [st.ENTHALPY]))
    # the key column counts like any other column: the observables it reads cannot be replaced
    with pytest.raises(err, match="while a statistics record with count columns depends on the observables"):
        eng.set_observables(None)
    _same_record(eng.statistics(), before, "after set_observables")
    # a per-walker record in force reports no bins
    eng.set_statistics(Statistics.per_walker([st.ENTHALPY]))
    assert eng.statistics_bins() == (0, 0, 0.0, 0.0, 0, 0) and eng.statistics_shape() == (R, 1, 0, 0)
    eng.set_statistics(None)
    assert eng.statistics_bins() == (0, 0, 0.0, 0.0, 0, 0)
    eng.close()


# ---- 6: the sampler ---------------------------------------------------------------------------------------------------------
def test_sampler_by_composition_equals_the_traces(clean_env):
    c = load_case("rocksalt333_two_sublattices")
    nw, T = 6, 3000.0
    ens = moca.Ensemble.from_cluster_expansion(c["sc"], c["coefs"])
    ens.chemical_potentials = {sp: 0.1 * (i - 1) for i, sp in enumerate(ens.species)}
    obs = Observables.from_supercell(c["sc"])
    spec = Statistics.by_composition(obs, 1, c["sc"].num_sites, columns=[st.ENTHALPY] + [st.kind(obs, k) for k in range(obs.n_kinds)])
    s = moca.Sampler.from_ensemble(ens, temperature=T, nwalkers=nw, seeds=list(range(3, 3 + nw)), rank=0, world_size=1,
                                   observables=obs, statistics=spec)
    occ = _rand_occ(c["sc"], np.random.default_rng(12), nw)
    s.run(40 * 9, occ, thin_by=9)
    s.run(25 * 9, thin_by=9)  # (a second run: the record goes on)
    rec = s.statistics
    assert rec.n.sum() == 65 * nw and rec.key_under == rec.key_over == 0 and (rec.n > 0).sum() > 1
    H = s.samples.get_trace_value("enthalpy", flat=False)[:, :, 0]
    feats = s.samples.get_feature_vectors(flat=False)
    cnt = s.samples.get_trace_value("species_counts", flat=False)
    _same_record(rec, StatisticsRecord(spec).offer(H, feats, cnt), "sampler")
    # the mean count of the key's kind in key k is k
    kcol = spec.key_column
    live = rec.n > 0
    np.testing.assert_array_equal(rec.microcanonical()[live, kcol], np.flatnonzero(live).astype(np.float64))
    s.reset_statistics()
    assert s.statistics.n.sum() == 0


def test_sampler_wl_canonical(clean_env):
    from smol_amd import synth

    model = synth.build_cluster_model(synth.fcc_prim(), {2: 6.0, 3: 5.0})
    sc = synth.build_supercell(model, [5, 5, 5])
    ens = moca.Ensemble.from_cluster_expansion(sc, synth.random_coefs(model, seed=3))
    nsp = np.array([sc.model.prim.nspecies[b] for b in sc.site_b])
    occu = (np.random.default_rng(5).random(sc.num_sites) * nsp).astype(np.int32)
    h0 = float(ens.natural_parameters @ ens.compute_feature_vector(occu))
    spec = Statistics.on_wl_levels(h0 - 8.0, 0.5, 32, columns=[st.ENTHALPY, st.feature(1), st.feature(2)])
    sampler = moca.Sampler.from_ensemble(ens, h0 - 8.0, h0 + 8.0, 0.5, kernel_type="Wang-Landau", nwalkers=3, seeds=[1, 2, 3],
                                         check_period=150, flatness=0.2, statistics=spec)
    sampler.run(6000, np.vstack([occu] * 3), thin_by=100)
    rec = sampler.statistics
    assert rec.n.sum() == 60 * 3 and (rec.n > 0).sum() >= 2
    H = sampler.samples.get_trace_value("enthalpy", flat=False)[:, :, 0]
    _same_record(rec, StatisticsRecord(spec).offer(H, sampler.samples.get_feature_vectors(flat=False)), "wl sampler")
    S = sampler._get_engine().get_wl()["entropy"]
    seen = S > 0
    assert seen.any(axis=0)[rec.n > 0].all()  # (key k is level k: a key with rows is a visited level)
    with np.errstate(invalid="ignore"):
        ln_g = np.where(seen.any(axis=0), np.where(seen, S, 0.0).sum(axis=0) / seen.sum(axis=0), np.nan)
    temps = [500.0, 2000.0, 8000.0]
    got = sampler.wl_canonical(temps)
    assert got.shape == (3, 3) and np.isfinite(got).all()
    np.testing.assert_array_equal(got, rec.canonical(ln_g, temps))
    assert got[0, 0] <= got[1, 0] <= got[2, 0]  # (the mean enthalpy grows with the temperature)
    plain = moca.Sampler.from_ensemble(ens, h0 - 8.0, h0 + 8.0, 0.5, kernel_type="Wang-Landau", nwalkers=1, seeds=[1])
    with pytest.raises(ValueError, match="Statistics.on_wl_levels"):
        plain.wl_canonical(temps)
