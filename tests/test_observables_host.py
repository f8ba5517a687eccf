"""Observables on the host: the NumPy definition (smol_amd/observables.py) against a plain loop and against the
reference arithmetic of the correlation vector, the derived quantities, and the container / sampler bookkeeping of the
species_counts and pair_counts traces.  No GPU."""

import numpy as np
import pytest

from oracle import oracle as orc
from smol_amd import capi, engine, moca, observables, synth
from smol_amd.observables import Observables
from tests.cases import CASES, load_case, tables_for


def random_occupancy(sc, rng, n=None):
    nsp = np.array([sc.model.prim.nspecies[b] for b in sc.site_b])
    occ = (rng.random((n or 1, sc.num_sites)) * nsp).astype(np.int32)
    return occ if n else occ[0]


def loop_evaluate(obs, occ):
    """The definition, spelled out: one site and one bond at a time."""
    K = obs.n_kinds
    counts = np.zeros(K, dtype=np.int32)
    pairs = np.zeros((obs.n_shells, K, K), dtype=np.int32)
    kind = [int(obs.kind_base[s]) + int(occ[s]) if obs.kind_base[s] >= 0 else -1 for s in range(obs.num_sites)]
    for k in kind:
        if k >= 0:
            counts[k] += 1
    for s, bonds in enumerate(obs.shells):
        for i, j in bonds:
            if kind[i] >= 0 and kind[j] >= 0:
                pairs[s, kind[i], kind[j]] += 1
    return counts, pairs


@pytest.mark.parametrize("name", ["fcc3_indicator_skew", "fcc_prim222_aliased"])
def test_evaluate_is_the_plain_loop(name):
    sc = load_case(name)["sc"]
    obs = Observables.from_supercell(sc)
    assert obs.n_shells == sum(o.size == 2 for o in sc.model.orbits) and obs.default_kinds
    if name == "fcc_prim222_aliased":  # duplicate rows and i == i rows are there, and count as they stand
        assert any((b[:, 0] == b[:, 1]).any() for b in obs.shells)
        assert any(len(np.unique(b, axis=0)) < len(b) for b in obs.shells)
    rng = np.random.default_rng(11)
    occ = random_occupancy(sc, rng, 3)
    counts, pairs = obs.evaluate(occ)
    assert counts.dtype == np.int32 and pairs.dtype == np.int32
    assert counts.shape == (3, obs.n_kinds) and pairs.shape == (3, obs.n_shells, obs.n_kinds, obs.n_kinds)
    for r in range(3):
        c, p = loop_evaluate(obs, occ[r])
        np.testing.assert_array_equal(counts[r], c)
        np.testing.assert_array_equal(pairs[r], p)
    assert counts.sum(axis=-1).tolist() == [sc.num_sites] * 3
    for s, b in enumerate(obs.shells):
        assert pairs[:, s].sum(axis=(-1, -2)).tolist() == [len(b)] * 3
    # sites left out: neither counted nor bonded
    kb = obs.kind_base.copy()
    kb[::3] = -1
    part = Observables(kb, obs.n_kinds, obs.shells, site_ncodes=obs.site_ncodes)
    c, p = part.evaluate(occ[0])
    cl, pl = loop_evaluate(part, occ[0])
    np.testing.assert_array_equal(c, cl)
    np.testing.assert_array_equal(p, pl)
    assert c.sum() == sc.num_sites - len(kb[::3])
    # a single occupancy keeps its shape
    assert obs.evaluate(occ[0])[0].shape == (obs.n_kinds,)


@pytest.mark.parametrize("name", sorted(CASES))
def test_pair_cells_give_the_correlation_functions(name):
    """pair_correlations / bonds == the reference arithmetic of the pair orbits' correlation functions."""
    c = load_case(name)
    sc = c["sc"]
    tab = tables_for(name, capi.FEATURES_CORRELATIONS)
    obs = Observables.from_supercell(sc, tables=tab)
    occ = random_occupancy(sc, np.random.default_rng(CASES[name]["seed"]))
    corr = orc.OracleEvaluator(tab).correlations(occ)
    counts, pairs = obs.evaluate(occ)
    npair, worst = 0, 0.0
    for orb, rows in zip(sc.model.orbits, sc.full_indices):
        if orb.size != 2:
            continue
        got = obs.pair_correlations(pairs, orb) / len(rows)
        want = corr[orb.bit_id:orb.bit_id + len(orb)]
        worst = max(worst, float(np.max(np.abs(got - want))))
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
        npair += 1
    print(f"{name}: {npair} pair orbits, max |difference| {worst:.3g}")
    assert npair == obs.n_shells > 0


@pytest.mark.parametrize("name", ["fcc_conv444_pairs", "fcc3_indicator_skew", "rocksalt333_two_sublattices",
                                  "rocksalt333_vacancy_ewald"])
def test_counts_are_the_engines_species_counts(name):
    sc = load_case(name)["sc"]
    tab = tables_for(name, capi.FEATURES_INTERACTIONS)
    obs = Observables.from_supercell(sc)
    occ = random_occupancy(sc, np.random.default_rng(3), 5)
    counts, _ = obs.evaluate(occ)
    width = max(len(s["codes"]) for s in tab.sublattices)
    want = engine.species_counts(tab, occ, width=width)
    for k, sub in enumerate(tab.sublattices):
        got = obs.species_counts(counts, sub["active_sites"])
        assert got is not None and got.shape == (5, len(sub["codes"]))
        np.testing.assert_array_equal(got, want[:, k, :len(sub["codes"])])
    # fixed sublattices have a block too: every site is counted
    assert (counts.sum(axis=-1) == sc.num_sites).all()
    prim = sc.model.prim
    assert obs.n_kinds == sum(prim.nspecies[b] for b in {prim.labels.index(l) for l in prim.labels})


def l10_occupancy(sc):
    """Layers of A and B alternating along z on the conventional fcc cell."""
    z = sc.model.prim.frac_coords[sc.site_b][:, 2]
    return (np.abs(z - 0.5) < 1e-9).astype(np.int32)


def test_warren_cowley_values():
    sc = load_case("fcc_conv444_pairs")["sc"]
    obs = Observables.from_supercell(sc)
    first = int(np.argmin([sc.model.orbits[[o.id for o in sc.model.orbits].index(i)].diameter for i in obs.shell_orbit_ids]))
    # L1_0: 4 like and 8 unlike neighbours of 12 at c = 1/2
    occ = l10_occupancy(sc)
    counts, pairs = obs.evaluate(occ)
    assert counts.tolist() == [sc.num_sites // 2] * 2
    sym = pairs[first] + pairs[first].T
    assert sym[0, 0] * 2 == sym[0, 1] and sym.sum() == 12 * sc.num_sites
    alpha = obs.warren_cowley(counts, pairs)
    assert alpha.shape == (obs.n_shells, 2, 2)
    assert alpha[first, 0, 1] == -1.0 / 3.0 and alpha[first, 1, 0] == -1.0 / 3.0
    assert alpha[first, 0, 0] == 1.0 / 3.0
    # the sum rule, for any occupancy: sum_b c_b alpha_ab = 0
    rng = np.random.default_rng(20260101)
    occ = random_occupancy(sc, rng, 4)
    counts, pairs = obs.evaluate(occ)
    alpha = obs.warren_cowley(counts, pairs)
    cb = counts / counts.sum(axis=-1, keepdims=True)
    np.testing.assert_allclose((alpha * cb[:, None, None, :]).sum(axis=-1), 0.0, atol=1e-13)
    # a random alloy has no short-range order.  The first shell has 12 N / 2 = 1536 bonds, each seen from both ends:
    # about n = 1536 ends on A sites, so P(B | A) scatters by sqrt(c (1 - c) / n) = 0.013 and alpha_AB = 1 - P / c by
    # twice that, 0.026 (ends of one bond are not independent: an upper estimate of n would lower it); bound: 5 sigma
    assert np.all(np.abs(alpha[:, first, 0, 1]) < 5 * 0.026)
    # pair probabilities: symmetric, one per shell
    P = obs.pair_probabilities(pairs)
    np.testing.assert_allclose(P.sum(axis=(-1, -2)), 1.0, atol=1e-14)
    np.testing.assert_array_equal(P, np.swapaxes(P, -1, -2))
    # a kind without sites or bonds gives NaN, not a division error
    counts, pairs = obs.evaluate(np.zeros(sc.num_sites, dtype=np.int32))
    a = obs.warren_cowley(counts, pairs)
    assert a[first, 0, 0] == 0.0 and np.isnan(a[first, 1, 1]) and np.isnan(a[first, 0, 1])


def test_site_classes_give_the_long_range_order_parameter():
    sc = load_case("fcc_conv444_pairs")["sc"]
    layers = l10_occupancy(sc)  # the two sublattices of L1_0 as site classes
    obs = Observables.from_supercell(sc, site_classes=layers)
    assert obs.n_kinds == 4 and not obs.default_kinds
    counts, pairs = obs.evaluate(layers)  # the ordered state itself
    half = sc.num_sites // 2
    assert counts.tolist() == [half, 0, 0, half]  # A on class 0, B on class 1: order parameter 1
    c, _ = obs.evaluate(1 - layers)
    assert c.tolist() == [0, half, half, 0]  # the other domain
    assert obs.species_counts(counts, np.flatnonzero(layers == 0)).tolist() == [half, 0]
    assert obs.species_counts(counts, np.arange(sc.num_sites)) is None  # (two blocks: no slice of the vector)
    # the cells still contract to the correlation functions: a kind stands for one code
    tab = tables_for("fcc_conv444_pairs", capi.FEATURES_CORRELATIONS)
    occ = random_occupancy(sc, np.random.default_rng(5))
    corr = orc.OracleEvaluator(tab).correlations(occ)
    _, pairs = obs.evaluate(occ)
    orb = [o for o in sc.model.orbits if o.size == 2][0]
    np.testing.assert_allclose(obs.pair_correlations(pairs, orb) / len(obs.shells[0]), corr[orb.bit_id:orb.bit_id + len(orb)],
                               rtol=0, atol=1e-12)


def test_shells_beyond_the_cutoff_come_from_a_second_model():
    c = load_case("fcc_conv444_pairs")
    wide = synth.build_supercell(synth.build_cluster_model(synth.fcc_conventional_prim(), {2: 7.5}), [4, 4, 4])
    obs, more = Observables.from_supercell(c["sc"]), Observables.from_supercell(wide)
    assert more.n_shells > obs.n_shells and more.num_sites == obs.num_sites
    np.testing.assert_array_equal(more.kind_base, obs.kind_base)
    only = Observables.from_supercell(wide, orbits=[more.shell_orbit_ids[-1]])
    assert only.n_shells == 1 and np.array_equal(only.shells[0], more.shells[-1])


def test_malformed_observables_are_refused():
    kb = np.zeros(8, dtype=np.int32)
    bonds = np.array([[0, 1], [2, 3]])
    assert Observables.from_bonds(kb, 2, [bonds]).n_shells == 1
    with pytest.raises(ValueError, match="bond out of range"):
        Observables(kb, 2, [np.array([[0, 8]])])
    with pytest.raises(ValueError, match="bond out of range"):
        Observables(kb, 2, [np.array([[-1, 2]])])
    with pytest.raises(ValueError, match=r"\(nbonds, 2\)"):
        Observables(kb, 2, [np.array([0, 1, 2])])
    with pytest.raises(ValueError, match="n_kinds must be"):
        Observables(kb, 0)
    with pytest.raises(ValueError, match="n_kinds must be"):
        Observables(kb, 255)
    with pytest.raises(ValueError, match="kind out of range"):
        Observables(kb + 2, 2)
    with pytest.raises(ValueError, match=r"kind_base\[0\] \+ site_ncodes\[0\] = 0 \+ 3 is larger than n_kinds = 2"):
        Observables(kb, 2, site_ncodes=np.full(8, 3))
    with pytest.raises(ValueError, match="larger than MAX_OBS_CELLS"):
        Observables(kb, 33, [bonds] * 4)
    assert Observables(kb, 32, [bonds] * 4).n_shells == 4  # exactly MAX_OBS_CELLS cells
    with pytest.raises(ValueError, match="1-D integer"):
        Observables(kb.astype(float), 2)
    obs = Observables(kb, 2, [bonds])
    with pytest.raises(ValueError, match="kind out of range"):
        obs.evaluate(np.full(8, 2))
    with pytest.raises(ValueError, match="8 sites in the last axis"):
        obs.evaluate(np.zeros(7, dtype=np.int32))
    with pytest.raises(ValueError, match="needs site_ncodes"):
        obs.pair_correlations(obs.evaluate(np.zeros(8, dtype=np.int32))[1], None, shell=0)
    assert capi.MAX_OBS_CELLS == observables.MAX_OBS_CELLS and capi.SAMPLE_OBSERVABLES == 8


# ---- the traces in the container and the sampler -----------------------------------------------------------------
def _sampler(nw=3, with_obs=True, name="rocksalt333_two_sublattices"):
    c = load_case(name)
    ens = moca.Ensemble.from_cluster_expansion(c["sc"], c["coefs"])
    obs = Observables.from_supercell(c["sc"])
    s = moca.Sampler.from_ensemble(ens, temperature=900.0, nwalkers=nw, seeds=list(range(1, nw + 1)), rank=0, world_size=1,
                                   observables=obs if with_obs else None)
    return c["sc"], ens, obs, s


def _block(sc, ens, obs, n, nw, rng, occupancy=True):
    occ = random_occupancy(sc, rng, n * nw).reshape(n, nw, -1)
    counts, pairs = obs.evaluate(occ)
    F = len(ens.natural_parameters)
    return dict(occupancy=occ.astype(np.uint8) if occupancy else np.empty((0, nw, sc.num_sites), np.uint8),
                features=rng.normal(size=(n, nw, F)), enthalpy=rng.normal(size=(n, nw, 1)),
                temperature=np.full((n, nw, 1), 900.0), accepted=np.ones((n, nw, 1), bool),
                species_counts=counts, pair_counts=pairs), occ


def test_container_round_trips_the_traces(tmp_path):
    sc, ens, obs, sampler = _sampler()
    c = sampler.samples
    assert c.traced_values[-2:] == ("species_counts", "pair_counts")
    assert c._schema["species_counts"] == (np.dtype(np.int32), (3, obs.n_kinds))
    assert c._schema["pair_counts"] == (np.dtype(np.int32), (3, obs.n_shells, obs.n_kinds, obs.n_kinds))
    rng = np.random.default_rng(1)
    block, occ = _block(sc, ens, obs, 4, 3, rng)
    c.append_block(block, thinned_by=5)
    assert c.num_samples == 4 and c.total_mc_steps == 20
    np.testing.assert_array_equal(c.get_pair_counts(flat=False), block["pair_counts"])
    assert c.get_pair_counts().shape == (12, obs.n_shells, obs.n_kinds, obs.n_kinds)
    wc = c.warren_cowley(flat=False)
    np.testing.assert_array_equal(wc, observables.warren_cowley(block["species_counts"], block["pair_counts"]))
    assert c.warren_cowley(discard=1, thin_by=2).shape == (3,) + wc.shape[2:]
    c.to_npz(tmp_path / "c.npz")
    ways = [moca.SampleContainer.from_npz(tmp_path / "c.npz", ens), moca.SampleContainer.from_dict(c.as_dict(), ens)]
    want_mean, want_var = c.mean_composition(), c.composition_variance()
    stream = c.get_backend(str(tmp_path / "stream"))
    c.flush_to_backend(stream)
    ways.append(moca.SampleContainer.from_stream(str(tmp_path / "stream"), ens))
    for back in ways:
        for name in ("species_counts", "pair_counts"):
            got = back.get_trace_value(name, flat=False)
            assert got.dtype == np.int32
            np.testing.assert_array_equal(got, block[name])
        assert back.metadata["observables"]["n_kinds"] == obs.n_kinds and back.metadata["observables"]["default_kinds"]
        assert back.metadata["observables"]["kind_base"] == obs.kind_base.tolist()
        assert back.mean_composition() == want_mean and back.composition_variance() == want_var


def test_composition_getters_read_the_counts_and_agree_with_the_scan():
    sc, ens, obs, sampler = _sampler()
    c = sampler.samples
    block, occ = _block(sc, ens, obs, 5, 3, np.random.default_rng(2))
    c.append_block(block, thinned_by=1)
    _, _, _, plain = _sampler(with_obs=False)
    p = plain.samples
    p.append_block({k: v for k, v in block.items() if k not in ("species_counts", "pair_counts")}, thinned_by=1)
    for sub in c.sublattices:
        assert c._counted_on_device(sub, 0, 1) is not None  # (read from the trace, not scanned)
    for sub_c, sub_p in zip(c.sublattices, p.sublattices):
        for kw in (dict(), dict(discard=1, thin_by=2, flat=False)):
            np.testing.assert_array_equal(c.get_sublattice_species_counts(sub_c, **kw), p.get_sublattice_species_counts(sub_p, **kw))
            np.testing.assert_array_equal(c.get_sublattice_compositions(sub_c, **kw), p.get_sublattice_compositions(sub_p, **kw))
        np.testing.assert_array_equal(c.mean_sublattice_composition(sub_c), p.mean_sublattice_composition(sub_p))
        np.testing.assert_array_equal(c.sublattice_composition_variance(sub_c), p.sublattice_composition_variance(sub_p))
    for getter in ("get_species_counts", "get_compositions", "mean_composition", "composition_variance"):
        a, b = getattr(c, getter)(), getattr(p, getter)()
        assert a.keys() == b.keys()
        for sp in a:
            np.testing.assert_array_equal(a[sp], b[sp])
    # the occupancies must not have been touched: without them the getters still answer
    c._blocks[0]["occupancy"] = np.empty((0, 3, sc.num_sites), np.uint8)
    c._joined = {}
    assert c.mean_composition() == p.mean_composition()
    # kinds that are not the default ones: the scan again
    c.metadata["observables"]["default_kinds"] = False
    assert c._counted_on_device(c.sublattices[0], 0, 1) is None


def test_keep_occupancy_false_bookkeeping(tmp_path):
    sc, ens, obs, sampler = _sampler()
    c = sampler.samples
    rng = np.random.default_rng(3)
    first, _ = _block(sc, ens, obs, 3, 3, rng, occupancy=False)
    second, _ = _block(sc, ens, obs, 2, 3, rng, occupancy=False)
    c.append_block(first, thinned_by=7)
    c.append_block(second, thinned_by=7)
    final = random_occupancy(sc, rng, 3)
    c.set_last_occupancy(final)  # what Sampler.run(keep_occupancy=False) does with get_state at its end
    assert c.num_samples == len(c) == 5 and c.total_mc_steps == 35  # counted on the enthalpy column
    np.testing.assert_array_equal(c.last_occupancy(), final)
    assert c.last_occupancy().dtype == np.int32
    assert c.get_enthalpies().shape == (15,) and c.get_trace_value("species_counts", flat=False).shape == (5, 3, obs.n_kinds)
    assert set(c.mean_composition()) == set(ens.species) | {sp for s in c.sublattices for sp in s.species}
    for call in (lambda: c.get_occupancies(), lambda: c.get_minimum_enthalpy_occupancy(), lambda: c.get_sampled_species([0]),
                 lambda: c.get_trace_value("occupancy")):
        with pytest.raises(ValueError, match="keep_occupancy=False"):
            call()
    # out and back in: the one occupancy travels along
    c.to_npz(tmp_path / "c.npz")
    for back in (moca.SampleContainer.from_npz(tmp_path / "c.npz", ens), moca.SampleContainer.from_dict(c.as_dict(), ens)):
        assert back.num_samples == 5
        np.testing.assert_array_equal(back.last_occupancy(), final)
        np.testing.assert_array_equal(back.get_trace_value("pair_counts", flat=False), c.get_trace_value("pair_counts", flat=False))
        with pytest.raises(ValueError, match="keep_occupancy=False"):
            back.get_occupancies()
    # the option needs observables, and a stream holds its occupancies
    _, _, _, plain = _sampler(with_obs=False)
    with pytest.raises(ValueError, match="keep_occupancy=False needs a sampler built with observables="):
        plain.run(10, initial_occupancies=final, keep_occupancy=False)
    with pytest.raises(ValueError, match="stream_chunk"):
        sampler.run(10, initial_occupancies=final, keep_occupancy=False, stream_chunk=2)
    # a sampler's observables live on its sites
    with pytest.raises(ValueError, match="defined on 8 sites"):
        moca.Sampler.from_ensemble(ens, temperature=900.0, rank=0, world_size=1,
                                   observables=Observables(np.zeros(8, np.int32), 2, site_ncodes=np.full(8, 2)))
