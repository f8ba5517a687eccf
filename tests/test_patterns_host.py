"""Patterns on the host: the NumPy definition (smol_amd/patterns.py) against a plain loop, against the pair cells of the
observables and against the reference arithmetic of the correlation vector; the derived quantities, the C struct and the
Python-side refusals.  No GPU."""

import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import oracle as orc
from smol_amd import capi, moca, patterns
from smol_amd import statistics as st
from smol_amd.observables import Observables
from smol_amd.patterns import Patterns, PatternSet
from tests.cases import CASES, load_case, tables_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_occupancy(sc, rng, n=None):
    nsp = np.array([sc.model.prim.nspecies[b] for b in sc.site_b])
    occ = (rng.random((n or 1, sc.num_sites)) * nsp).astype(np.int32)
    return occ if n else occ[0]


def loop_evaluate(kind_base, sets, occ):
    """The definition, spelled out: one tuple and one site at a time.  ``sets``: (tuples, class map, classes) each."""
    out = []
    for tuples, cmap, ncls in sets:
        arity = len(tuples[0]) if len(tuples) else 1
        cells = [0] * (ncls ** arity) if len(tuples) else None
        for tup in tuples:
            cell, skip = 0, False
            for site in tup:
                if kind_base[site] < 0:
                    skip = True
                    break
                cls = cmap[kind_base[site] + occ[site]]
                if cls < 0:
                    skip = True
                    break
                cell = cell * ncls + cls
            if not skip:
                cells[cell] += 1
        out.append(cells)
    return out


def random_spec(rng, N=23, K=5):
    """Random sets of every arity 1..8 on N sites of width 1..3, some sites left out, -1 classes, duplicate tuples and
    tuples with repeated sites."""
    ncodes = rng.integers(1, 4, size=N)
    kind_base = np.array([rng.integers(0, K - n + 1) for n in ncodes], dtype=np.int32)
    kind_base[rng.random(N) < 0.2] = -1
    obs = Observables(kind_base, K, site_ncodes=ncodes)
    sets = []
    for arity in rng.permutation(np.arange(1, 9)):
        ncls = int(rng.integers(1, 3)) if arity > 5 else int(rng.integers(1, 4))
        cmap = rng.integers(-1, ncls, size=K).astype(np.int32)
        n = int(rng.integers(0, 40))
        tuples = rng.integers(0, N, size=(n, arity))
        if n > 4:
            tuples[1] = tuples[0]            # a duplicate
            tuples[2, :] = tuples[2, 0]      # one site, arity times
        sets.append(PatternSet(tuples, cmap, ncls))
    occ = (rng.random((4, N)) * ncodes).astype(np.int32)
    return obs, sets, occ


@pytest.mark.parametrize("seed", range(6))
def test_evaluate_is_the_plain_loop(seed):
    rng = np.random.default_rng(100 + seed)
    obs, sets, occ = random_spec(rng)
    spec = Patterns(obs, sets)
    assert spec.n_sets == 8 and sorted(s.arity for s in spec.sets) == list(range(1, 9))
    cells = spec.evaluate(occ)
    assert cells.dtype == np.int32 and cells.shape == (4, spec.n_cells)
    assert spec.n_cells == sum(s.n_classes ** s.arity for s in sets) and spec.cell_ptr[0] == 0
    plain = [(s.sites.tolist(), s.class_of_kind.tolist(), s.n_classes) for s in sets]
    counted = skipped = 0
    for r in range(4):
        want = loop_evaluate(obs.kind_base.tolist(), plain, occ[r].tolist())
        for t, w in enumerate(want):
            got = cells[r, spec.cell_ptr[t]:spec.cell_ptr[t + 1]]
            if w is None:
                assert not got.any()
                continue
            assert got.tolist() == w, (r, t)
            counted += sum(w)
            skipped += sets[t].n_tuples - sum(w)
    assert counted > 0 and skipped > 0  # (both branches of the definition were taken)
    # a single occupancy keeps its shape
    assert spec.evaluate(occ[0]).shape == (spec.n_cells,)
    np.testing.assert_array_equal(spec.evaluate(occ[0]), cells[0])


@pytest.mark.parametrize("name", ["fcc3_indicator_skew", "fcc_prim222_aliased", "rocksalt333_two_sublattices"])
def test_an_identity_set_of_arity_two_is_a_pair_shell(name):
    sc = load_case(name)["sc"]
    obs = Observables.from_supercell(sc)
    spec = Patterns.from_tuples(obs, obs.shells[:8], classes="kind")
    occ = random_occupancy(sc, np.random.default_rng(3), 5)
    _, pairs = obs.evaluate(occ)
    cells = spec.evaluate(occ)
    K = obs.n_kinds
    assert spec.n_cells == spec.n_sets * K * K
    np.testing.assert_array_equal(cells.reshape(5, spec.n_sets, K, K), pairs[:, :spec.n_sets])
    np.testing.assert_array_equal(spec.cells_of(cells, 1), pairs[:, 1])


@pytest.mark.parametrize("name", sorted(CASES))
def test_cells_give_the_correlation_functions(name):
    """correlations / tuples == the reference arithmetic of the correlation functions of every orbit of three sites or
    more (a case whose expansion stops at pairs has none); rtol=0, atol=1e-12 is the bound the pair form is held to
    (test_observables_host)."""
    c = load_case(name)
    sc = c["sc"]
    big = [o for o in sc.model.orbits if o.size >= 3]
    tab = tables_for(name, capi.FEATURES_CORRELATIONS)
    obs = Observables.from_supercell(sc, tables=tab)
    occ = random_occupancy(sc, np.random.default_rng(CASES[name]["seed"]))
    corr = orc.OracleEvaluator(tab).correlations(occ)
    worst, n = 0.0, 0
    for first in range(0, len(big), patterns.MAX_PATTERN_SETS):
        ids = [o.id for o in big[first:first + patterns.MAX_PATTERN_SETS]]
        spec = Patterns.from_supercell(sc, obs, orbits=ids)
        assert spec.set_orbit_ids == ids
        cells = spec.evaluate(occ)
        for orb, rows in zip(sc.model.orbits, sc.full_indices):
            if orb.id not in ids:
                continue
            got = spec.correlations(cells, orb) / len(rows)
            want = corr[orb.bit_id:orb.bit_id + len(orb)]
            worst = max(worst, float(np.max(np.abs(got - want))))
            np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
            n += 1
    print(f"{name}: {n} orbits of three sites or more, max |difference| {worst:.3g}")
    assert n == len(big)


def test_composition_census_folds_the_ordered_cells():
    # a hand-made case: four sites, binary, tetrahedra
    obs = Observables(np.zeros(6, np.int32), 2, site_ncodes=np.full(6, 2))
    tuples = np.array([[0, 1, 2, 3], [1, 2, 3, 4], [2, 3, 4, 5], [0, 0, 0, 0], [5, 4, 3, 2]])
    spec = Patterns.from_tuples(obs, [tuples], classes="code")
    occ = np.array([1, 0, 0, 1, 1, 1], dtype=np.int32)
    cells = spec.evaluate(occ)
    assert cells.sum() == 5 and cells[spec.cell(0, [1, 0, 0, 1])] == 1 and cells[spec.cell(0, [0, 0, 1, 1])] == 1
    assert cells[spec.cell(0, [0, 1, 1, 1])] == 1 and cells[spec.cell(0, [1, 1, 1, 1])] == 1 and cells[spec.cell(0, [1, 1, 1, 0])] == 1
    census, comp = spec.composition_census(cells, 0)
    assert comp.tolist() == [[4, 0], [3, 1], [2, 2], [1, 3], [0, 4]]  # 0, 1 .. 4 sites of class 1
    assert census.tolist() == [0, 0, 2, 2, 1]
    # three classes: ascending in (n_1, n_2); the census of random cells sums to the number of counted tuples
    comp3 = patterns.compositions(2, 3)
    assert comp3.tolist() == [[2, 0, 0], [1, 0, 1], [0, 0, 2], [1, 1, 0], [0, 1, 1], [0, 2, 0]]
    rng = np.random.default_rng(5)
    obs3, sets, occ3 = random_spec(rng)
    spec3 = Patterns(obs3, sets)
    cells3 = spec3.evaluate(occ3)
    for t, s in enumerate(sets):
        census, comp = spec3.composition_census(cells3, t)
        assert census.shape == (4, len(comp)) and (comp.sum(axis=1) == s.arity).all()
        np.testing.assert_array_equal(census.sum(axis=-1), spec3.cells_of(cells3, t).reshape(4, -1).sum(axis=-1))
    # probabilities: one per set, NaN where a set counted nothing
    P = spec.probabilities(cells)
    assert abs(P.sum() - 1.0) < 1e-15 and P[spec.cell(0, [1, 1, 1, 1])] == 0.2
    none = Patterns.from_tuples(obs, [tuples, np.zeros((0, 3), np.int64)], classes="code")
    P = none.probabilities(none.evaluate(occ))
    assert np.isnan(P[16:]).all() and abs(P[:16].sum() - 1.0) < 1e-15


def test_c_struct_packing():
    rng = np.random.default_rng(9)
    obs, sets, _ = random_spec(rng)
    spec = Patterns(obs, sets)
    s, keep = spec.c_struct()
    assert s.n_sets == 8
    assert [s.arity[t] for t in range(8)] == [x.arity for x in sets]
    assert [s.n_classes[t] for t in range(8)] == [x.n_classes for x in sets]
    K = obs.n_kinds
    assert [s.class_of_kind[i] for i in range(8 * K)] == [int(v) for x in sets for v in x.class_of_kind]
    ptr = [s.tuple_ptr[t] for t in range(9)]
    assert ptr == np.concatenate(([0], np.cumsum([x.n_tuples for x in sets]))).tolist()
    flat = [int(v) for x in sets for v in x.sites.reshape(-1)]
    assert [s.sites[i] for i in range(len(flat))] == flat
    assert all(a.flags["C_CONTIGUOUS"] for a in keep)
    assert C.sizeof(capi.smolmc_patterns) == 48  # int, five pointers: 8-byte aligned
    d = spec.describe()
    assert d["n_cells"] == spec.n_cells and d["cell_ptr"][-1] == spec.n_cells and len(d["class_of_kind"]) == 8


def test_from_supercell_defaults():
    name = "rocksalt333_two_sublattices"
    sc = load_case(name)["sc"]
    obs = Observables.from_supercell(sc)
    big = [(o, rows) for o, rows in zip(sc.model.orbits, sc.full_indices) if o.size >= 3]
    ids = [o.id for o, _ in big][:patterns.MAX_PATTERN_SETS]
    spec = Patterns.from_supercell(sc, obs, orbits=ids)
    assert spec.n_sets == len(ids) and spec.set_orbit_ids == ids
    for s, (o, rows) in zip(spec.sets, big):
        np.testing.assert_array_equal(s.sites, rows)  # row for row
        assert s.arity == o.size
        np.testing.assert_array_equal(s.class_of_kind, obs.kind_code)  # a kind's class is its species code
        assert s.n_classes == int(obs.kind_code.max()) + 1
    if len(big) > patterns.MAX_PATTERN_SETS:
        with pytest.raises(ValueError, match="name some with orbits="):
            Patterns.from_supercell(sc, obs)
    # other classes: an array over the kinds
    tm = np.where(obs.kind_code == 0, 0, 1).astype(np.int32)
    two = Patterns.from_supercell(sc, obs, orbits=ids[:1], classes=tm)
    assert two.sets[0].n_classes == 2 and two.n_cells == 2 ** two.sets[0].arity
    with pytest.raises(ValueError, match="no orbit with three sites or more"):
        Patterns.from_supercell(load_case("fcc_conv444_pairs")["sc"], Observables.from_supercell(load_case("fcc_conv444_pairs")["sc"]))


def test_malformed_specs_are_refused():
    obs = Observables(np.zeros(8, np.int32), 2, site_ncodes=np.full(8, 2))
    ident = np.arange(2)
    tri = np.array([[0, 1, 2], [2, 3, 4]])
    assert Patterns(obs, [PatternSet(tri, ident, 2)]).n_cells == 8
    with pytest.raises(ValueError, match="arity must be 1..8"):
        PatternSet(np.zeros((2, 9), np.int64), ident, 2)
    with pytest.raises(ValueError, match=r"\(ntuples, arity\) integer"):
        PatternSet(np.zeros(3, np.int64), ident, 2)
    with pytest.raises(ValueError, match="n_classes must be 1..255"):
        PatternSet(tri, ident, 256)
    with pytest.raises(ValueError, match="n_classes must be 1..255"):
        PatternSet(tri, ident * 0, 0)
    with pytest.raises(ValueError, match="class out of range"):
        PatternSet(tri, np.array([0, 2]), 2)
    with pytest.raises(ValueError, match="class out of range"):
        PatternSet(tri, np.array([0, -2]), 2)
    with pytest.raises(ValueError, match="holds 1..8 sets"):
        Patterns(obs, [])
    with pytest.raises(ValueError, match="holds 1..8 sets"):
        Patterns(obs, [PatternSet(tri, ident, 2)] * 9)
    with pytest.raises(ValueError, match="site out of range"):
        Patterns(obs, [PatternSet(np.array([[0, 1, 8]]), ident, 2)])
    with pytest.raises(ValueError, match="site out of range"):
        Patterns(obs, [PatternSet(np.array([[0, -1, 2]]), ident, 2)])
    with pytest.raises(ValueError, match="the observables have 2 kinds"):
        Patterns(obs, [PatternSet(tri, np.arange(3), 3)])
    six = np.zeros((1, 6), np.int64)
    four = np.array([0, 3])
    assert Patterns(obs, [PatternSet(six, four, 4)]).n_cells == capi.MAX_PATTERN_CELLS  # exactly 4096 cells
    with pytest.raises(ValueError, match="4097 cells, larger than MAX_PATTERN_CELLS"):
        Patterns(obs, [PatternSet(six, four, 4), PatternSet(np.zeros((1, 1), np.int64), ident * 0, 1)])
    spec = Patterns(obs, [PatternSet(tri, ident, 2)])
    with pytest.raises(ValueError, match="8 sites in the last axis"):
        spec.evaluate(np.zeros(7, dtype=np.int32))
    with pytest.raises(ValueError, match="kind out of range"):
        spec.evaluate(np.full(8, 2))
    with pytest.raises(ValueError, match='needs site_ncodes'):
        Patterns.class_map(Observables(np.zeros(8, np.int32), 2), "code")
    with pytest.raises(ValueError, match="pattern cell -1 is negative"):
        st.pattern(-1)
    with pytest.raises(ValueError, match="cell 8 outside the 8 cells"):
        st.Statistics.per_walker([st.pattern(8)]).sources(3, 2, n_cells=8)
    assert st.Statistics.per_walker([st.pattern(7)]).sources(3, 2, 1, 2, 8).tolist() == [2 + 3 + 2 + 1 + 48 + 7]
    # the sampler: patterns need the observables they rest on, and their sites
    c = load_case("rocksalt333_two_sublattices")
    ens = moca.Ensemble.from_cluster_expansion(c["sc"], c["coefs"])
    full = Observables.from_supercell(c["sc"])
    big = [o.id for o in c["sc"].model.orbits if o.size >= 3][:2]
    good = Patterns.from_supercell(c["sc"], full, orbits=big)
    kw = dict(temperature=900.0, nwalkers=2, seeds=[1, 2], rank=0, world_size=1)
    with pytest.raises(ValueError, match="patterns= needs observables="):
        moca.Sampler.from_ensemble(ens, patterns=good, **kw)
    with pytest.raises(ValueError, match="defined on 8 sites"):
        moca.Sampler.from_ensemble(ens, observables=full, patterns=spec, **kw)
    with pytest.raises(ValueError, match="pattern columns needs a sampler built with patterns="):
        moca.Sampler.from_ensemble(ens, observables=full, statistics=st.Statistics.per_walker([st.pattern(0)]), **kw)
    s = moca.Sampler.from_ensemble(ens, observables=full, patterns=good, **kw)
    assert s.samples.traced_values[-1] == "pattern_counts"
    assert s.samples._schema["pattern_counts"] == (np.dtype(np.int32), (2, good.n_cells))
    assert s.samples.metadata["patterns"]["cell_ptr"] == good.cell_ptr.tolist()


def test_container_round_trips_the_trace(tmp_path):
    c = load_case("rocksalt333_two_sublattices")
    sc = c["sc"]
    ens = moca.Ensemble.from_cluster_expansion(sc, c["coefs"])
    obs = Observables.from_supercell(sc)
    spec = Patterns.from_supercell(sc, obs, orbits=[o.id for o in sc.model.orbits if o.size >= 3][:3])
    nw, n = 3, 4
    s = moca.Sampler.from_ensemble(ens, temperature=900.0, nwalkers=nw, seeds=[1, 2, 3], rank=0, world_size=1, observables=obs,
                                   patterns=spec)
    rng = np.random.default_rng(1)
    occ = random_occupancy(sc, rng, n * nw).reshape(n, nw, -1)
    counts, pairs = obs.evaluate(occ)
    F = len(ens.natural_parameters)
    block = dict(occupancy=occ.astype(np.uint8), features=rng.normal(size=(n, nw, F)), enthalpy=rng.normal(size=(n, nw, 1)),
                 temperature=np.full((n, nw, 1), 900.0), accepted=np.ones((n, nw, 1), bool), species_counts=counts,
                 pair_counts=pairs, pattern_counts=spec.evaluate(occ))
    box = s.samples
    box.append_block(block, thinned_by=5)
    np.testing.assert_array_equal(box.get_pattern_counts(flat=False), block["pattern_counts"])
    assert box.get_pattern_counts().shape == (n * nw, spec.n_cells)
    np.testing.assert_array_equal(box.pattern_probabilities(flat=False), spec.probabilities(block["pattern_counts"]))
    box.to_npz(tmp_path / "c.npz")
    ways = [moca.SampleContainer.from_npz(tmp_path / "c.npz", ens), moca.SampleContainer.from_dict(box.as_dict(), ens)]
    want_meta = spec.describe()
    stream = box.get_backend(str(tmp_path / "stream"))
    box.flush_to_backend(stream)
    ways.append(moca.SampleContainer.from_stream(str(tmp_path / "stream"), ens))
    for back in ways:
        got = back.get_pattern_counts(flat=False)
        assert got.dtype == np.int32
        np.testing.assert_array_equal(got, block["pattern_counts"])
        assert back.metadata["patterns"] == want_meta
        np.testing.assert_array_equal(back.pattern_probabilities(), spec.probabilities(block["pattern_counts"]).reshape(n * nw, -1))
    plain = moca.Sampler.from_ensemble(ens, temperature=900.0, nwalkers=nw, seeds=[1, 2, 3], rank=0, world_size=1)
    with pytest.raises(ValueError, match="carry no pattern_counts trace"):
        plain.samples.get_pattern_counts()


def test_capi_constants_are_the_headers():
    text = open(os.path.join(ROOT, "include", "smolmc.h")).read()

    def header(name):
        return int(re.search(rf"#define {name} (\d+)", text).group(1))

    assert capi.SAMPLE_PATTERNS == header("SMOLMC_SAMPLE_PATTERNS") == 256
    assert capi.MAX_PATTERN_SETS == header("SMOLMC_MAX_PATTERN_SETS") == patterns.MAX_PATTERN_SETS
    assert capi.MAX_PATTERN_ARITY == header("SMOLMC_MAX_PATTERN_ARITY") == patterns.MAX_PATTERN_ARITY
    assert capi.MAX_PATTERN_CLASSES == header("SMOLMC_MAX_PATTERN_CLASSES") == patterns.MAX_PATTERN_CLASSES
    assert capi.MAX_PATTERN_CELLS == header("SMOLMC_MAX_PATTERN_CELLS") == patterns.MAX_PATTERN_CELLS
    assert capi.ABI_VERSION == header("SMOLMC_ABI_VERSION") == 8
    fields = re.search(r"typedef struct smolmc_patterns \{(.*?)\} smolmc_patterns;", text, re.S).group(1)
    names = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))
    assert names == [f[0] for f in capi.smolmc_patterns._fields_]
