"""Coordination environments on the host: the NumPy definition (smol_amd/environments.py) against a plain triple loop and
against the pair cells of the observables; the aliased cell, the -1 classes, the two ways to name a shell, the derived
quantities, the C struct and the Python-side refusals.  No GPU."""

import ctypes as C

import numpy as np
import pytest

from smol_amd import capi, environments
from smol_amd import statistics as st
from smol_amd.environments import Environments, EnvironmentSet
from smol_amd.observables import Observables
from smol_amd.statistics import Statistics, StatisticsRecord
from tests.cases import load_case

EVAL_CASES = ["fcc_prim666_triplets", "fcc3_indicator_skew", "fcc_prim222_aliased", "rocksalt333_two_sublattices"]


def random_occupancy(sc, rng, n):
    nsp = np.array([sc.model.prim.nspecies[b] for b in sc.site_b])
    return (rng.random((n, sc.num_sites)) * nsp).astype(np.int32)


def loop_evaluate(kind_base, spec, occ):
    """The definition, spelled out: one set, one centre and one slot at a time.  (cells, codes) of ONE occupancy."""
    cells, codes = [0] * spec.n_cells, []
    for e, s in enumerate(spec.sets):
        z, B = s.width, s.n_neigh_classes
        for centre, row in zip(s.centres.tolist(), s.neighbours.tolist()):
            a = -1 if kind_base[centre] < 0 else s.centre_class_of_kind[kind_base[centre] + occ[centre]]
            if a < 0:
                codes.append(-1)
                continue
            n = [0] * B
            for site in row:
                if site < 0 or kind_base[site] < 0:
                    continue
                b = s.neigh_class_of_kind[kind_base[site] + occ[site]]
                if b >= 0:
                    n[b] += 1
            code = int(a) * (z + 1) ** B + sum(n[b] * (z + 1) ** (B - 1 - b) for b in range(B))
            cells[int(spec.cell_ptr[e]) + code] += 1
            codes.append(code)
    return cells, codes


def case_spec(name):
    """The spec the device test evaluates on a case: the nearest-neighbour shell by distance with classes = species codes.
    The ternary fcc case has one centre class (13**3 cells a centre class: the spec holds one); the rocksalt case has the
    centres of either sublattice in a set of its own, their neighbours on the other sublattice, of another species width."""
    sc = load_case(name)["sc"]
    obs = Observables.from_supercell(sc)
    near = shell_lengths(sc)[0]
    if name == "rocksalt333_two_sublattices":
        sub = np.asarray(sc.site_b)
        sets = [Environments.from_supercell(sc, obs, distances=[near], centres=np.flatnonzero(sub == b)).sets[0] for b in (0, 1)]
        spec = Environments(obs, sets)
    elif obs.n_kinds == 3:
        spec = Environments.from_supercell(sc, obs, distances=[near], centre_classes=(np.zeros(3, np.int32), 1))
    else:
        spec = Environments.from_supercell(sc, obs, distances=[near])
    return sc, obs, spec


def shell_lengths(sc, n=2):
    """the n shortest bond lengths of a supercell's prim, ascending"""
    import itertools

    prim = sc.model.prim
    L, tau = np.asarray(prim.lattice, dtype=float), np.asarray(prim.frac_coords, dtype=float)
    r = sorted({round(float(np.linalg.norm((np.asarray(d) + tb - ta) @ L)), 6)
                for ta in tau for tb in tau for d in itertools.product(range(-2, 3), repeat=3)} - {0.0})
    return r[:n]


# ---- the definition --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EVAL_CASES)
def test_evaluate_is_the_plain_loop_on_the_cases(name):
    sc, obs, spec = case_spec(name)
    rng = np.random.default_rng(3)
    occ = random_occupancy(sc, rng, 4)
    cells, codes = spec.evaluate(occ), spec.codes(occ)
    assert cells.dtype == np.int32 and cells.shape == (4, spec.n_cells)
    assert codes.dtype == np.int32 and codes.shape == (4, spec.n_centres)
    for r in range(4):
        want_cells, want_codes = loop_evaluate(obs.kind_base, spec, occ[r])
        assert cells[r].tolist() == want_cells and codes[r].tolist() == want_codes
    # the cells of a set sum to its centres that are not skipped
    for e in range(spec.n_sets):
        mine = codes[:, spec.centre_ptr[e]:spec.centre_ptr[e + 1]]
        assert (cells[:, spec.cell_ptr[e]:spec.cell_ptr[e + 1]].sum(axis=1) == (mine >= 0).sum(axis=1)).all()
        assert (cells[:, spec.cell_ptr[e]:spec.cell_ptr[e + 1]] > 0).sum() > 4  # (several cells are hit)


@pytest.mark.parametrize("seed", range(5))
def test_evaluate_is_the_plain_loop_on_random_sets(seed):
    """Random rows with empty slots, repeated sites, self slots and duplicate centres; sites left out; -1 in both maps."""
    rng = np.random.default_rng(40 + seed)
    N, K = 29, 6
    ncodes = rng.integers(1, 4, size=N)
    kind_base = np.array([rng.integers(0, K - n + 1) for n in ncodes], dtype=np.int32)
    kind_base[rng.random(N) < 0.2] = -1
    obs = Observables(kind_base, K, site_ncodes=ncodes)
    sets = []
    for z, A, B in ((1, 3, 1), (12, 2, 2), (7, 2, 3), (4, 3, 4), (64, 1, 1)):
        n = int(rng.integers(0, 50))
        rows = rng.integers(-1, N, size=(n, z))
        cen = rng.integers(0, N, size=n)
        if n > 3:
            cen[1] = cen[0]
            rows[2, :] = cen[2]
        sets.append(EnvironmentSet(cen, rows, rng.integers(-1, A, size=K), A, rng.integers(-1, B, size=K), B))
    spec = Environments(obs, sets)
    assert spec.cell_ptr.tolist() == np.concatenate(([0], np.cumsum([s.n_centre_classes * (s.width + 1) ** s.n_neigh_classes
                                                                      for s in sets]))).tolist()
    occ = (rng.random((3, N)) * ncodes).astype(np.int32)
    cells, codes = spec.evaluate(occ), spec.codes(occ)
    for r in range(3):
        want_cells, want_codes = loop_evaluate(kind_base, spec, occ[r])
        assert cells[r].tolist() == want_cells and codes[r].tolist() == want_codes
    assert spec.evaluate(occ[0]).shape == (spec.n_cells,) and spec.codes(occ[None]).shape == (1, 3, spec.n_centres)


def test_first_moment_is_the_pair_counts_of_the_shell():
    """A set built from an observables shell listed in both directions, identity maps: sum n_b count[a, ...] equals
    pairs[s][a][b] + pairs[s][b][a], twice the diagonal entry for a == b."""
    sc = load_case("fcc_prim666_triplets")["sc"]
    obs = Observables.from_supercell(sc)
    K = obs.n_kinds
    assert K == 2 and obs.n_shells >= 2
    occ = (np.random.default_rng(5).random((6, sc.num_sites)) < 0.5).astype(np.int32)
    _, pairs = obs.evaluate(occ)
    off = 0
    for s, orbit in enumerate(obs.shell_orbit_ids[:3]):
        spec = Environments.from_supercell(sc, obs, orbits=[orbit], centre_classes="kind", neigh_classes="kind")
        cells = spec.evaluate(occ)
        d = spec.distribution(cells, 0).astype(np.int64)  # (6, K, z + 1, z + 1)
        n = np.arange(spec.sets[0].width + 1)
        sym = pairs[:, s].astype(np.int64) + np.swapaxes(pairs[:, s], -1, -2)
        for a in range(K):
            for b in range(K):
                shape = [1] * K
                shape[b] = len(n)
                moment = (d[:, a] * n.reshape(shape)).sum(axis=(1, 2))
                np.testing.assert_array_equal(moment, pairs[:, s, a, b].astype(np.int64) + pairs[:, s, b, a])
                if a == b:
                    np.testing.assert_array_equal(moment, 2 * pairs[:, s, a, a].astype(np.int64))
                else:
                    off += int((pairs[:, s, a, b] > 0).sum())
        np.testing.assert_allclose(spec.mean_coordination(cells, 0) * d.sum(axis=(2, 3))[..., None], sym, rtol=1e-14)
    assert off >= 12  # (several off-diagonal pair entries are non-zero)


def test_aliased_cell_counts_repeated_and_self_slots_as_listed():
    sc, obs, spec = case_spec("fcc_prim222_aliased")
    s = spec.sets[0]
    assert sc.num_sites == 8 and s.width == 12 and s.n_centres == 8
    assert any(len(set(row)) < len(row) for row in s.neighbours.tolist())       # a site twice in a row
    rows = s.neighbours.copy()
    rows[:, 0] = s.centres                                                           # ... and the centre itself
    spec = Environments(obs, [EnvironmentSet(s.centres, rows, s.centre_class_of_kind, s.n_centre_classes,
                                             s.neigh_class_of_kind, s.n_neigh_classes)])
    occ = random_occupancy(sc, np.random.default_rng(1), 5)
    cells, codes = spec.evaluate(occ), spec.codes(occ)
    for r in range(5):
        want_cells, want_codes = loop_evaluate(obs.kind_base, spec, occ[r])
        assert cells[r].tolist() == want_cells and codes[r].tolist() == want_codes
    # every slot counts: the n_b of a centre sum to the width
    z1 = s.width + 1
    assert ((codes % z1) + (codes // z1) % z1 == s.width).all()


def test_minus_one_skips_a_centre_and_only_drops_a_slot():
    obs = Observables(np.array([0, 0, 0, 0, -1], np.int32), 2, site_ncodes=np.full(5, 2))
    rows = np.array([[1, 2, 3, 4], [0, 0, -1, 2]])
    spec = Environments(obs, [EnvironmentSet([0, 1], rows, [0, -1], 1, [-1, 0], 1)])
    # centre 0 holds kind 0 (class 0); its neighbours 1, 2, 3 hold kinds 1, 0, 1, site 4 is not counted
    occ = np.array([0, 1, 0, 1, 0], np.int32)
    assert spec.codes(occ).tolist() == [2, -1]  # (centre 1 holds kind 1: centre class -1)
    assert spec.evaluate(occ).tolist() == [0, 0, 1, 0, 0]
    occ = np.array([0, 0, 0, 0, 1], np.int32)   # (no neighbour has a class: the centre still counts, with n = 0)
    assert spec.codes(occ).tolist() == [0, 0] and spec.evaluate(occ).tolist() == [2, 0, 0, 0, 0]
    # a centre that is not counted is skipped
    spec = Environments(obs, [EnvironmentSet([4], [[0, 1, 2, 3]], [0, 0], 1, [0, 0], 1)])
    assert spec.codes(occ).tolist() == [-1] and not spec.evaluate(occ).any()


def test_from_supercell_by_orbit_and_by_distance_give_the_same_rows():
    sc = load_case("fcc_prim666_triplets")["sc"]
    obs = Observables.from_supercell(sc)
    by_distance = Environments.from_supercell(sc, obs, distances=[shell_lengths(sc)[0]])
    by_cutoff = Environments.from_supercell(sc, obs, cutoff=shell_lengths(sc)[0] + 1e-3)
    found = None
    for orbit in obs.shell_orbit_ids:
        by_orbit = Environments.from_supercell(sc, obs, orbits=[orbit])
        if by_orbit.sets[0].width == 12:
            found = by_orbit
            break
    assert found is not None
    for spec in (by_distance, by_cutoff, found):
        s = spec.sets[0]
        assert s.width == 12 and s.centres.tolist() == list(range(sc.num_sites)) and (s.neighbours >= 0).all()
    for other in (by_cutoff, found):
        np.testing.assert_array_equal(np.sort(by_distance.sets[0].neighbours, axis=1), np.sort(other.sets[0].neighbours, axis=1))
    occ = random_occupancy(sc, np.random.default_rng(2), 3)
    np.testing.assert_array_equal(by_distance.evaluate(occ), found.evaluate(occ))
    with pytest.raises(ValueError, match="by orbits= or by cutoff="):
        Environments.from_supercell(sc, obs)


# ---- derived quantities ------------------------------------------------------------------------------------------------
def test_derived_quantities():
    sc, obs, spec = case_spec("fcc_prim666_triplets")
    s = spec.sets[0]
    assert (s.n_centre_classes, s.n_neigh_classes, s.width) == (2, 2, 12) and spec.n_cells == 2 * 13 * 13
    occ = random_occupancy(sc, np.random.default_rng(7), 5)
    cells, codes = spec.evaluate(occ), spec.codes(occ)
    counts, _ = obs.evaluate(occ)
    d = spec.distribution(cells, 0)
    assert d.shape == (5, 2, 13, 13) and d[0, 1, 3, 9] == cells[0, spec.cell(0, 1, (3, 9))]
    m = spec.marginal(cells, 0, 1)
    assert m.shape == (5, 2, 13)
    np.testing.assert_array_equal(m.sum(axis=-1), counts)               # (every site is a centre of its kind's class)
    np.testing.assert_array_equal(m, d.sum(axis=2))
    mean = spec.mean_coordination(cells, 0)
    np.testing.assert_allclose(mean.sum(axis=-1), 12.0, rtol=0, atol=1e-12)
    census, comp = spec.compositions(cells, 0)
    assert comp.shape[1] == 3 and (comp.sum(axis=1) == 12).all() and census.shape == (5, 2, len(comp))
    np.testing.assert_array_equal(census.sum(axis=-1), counts)          # (the fold loses no centre)
    full = comp[:, 2] == 0
    np.testing.assert_array_equal(census[..., full].sum(axis=-1), counts)  # (no empty slot on fcc)
    for row, n in zip(comp[full], census[0, 0, full]):
        assert n == d[0, 0, row[0], row[1]]
    ra = spec.random_alloy(counts, 0)
    assert ra.shape == d.shape
    np.testing.assert_allclose(ra.sum(axis=(1, 2, 3)), s.n_centres, rtol=1e-12)
    np.testing.assert_allclose(ra.sum(axis=(2, 3)), counts, rtol=1e-12)
    x = counts[0, 1] / counts[0].sum()
    np.testing.assert_allclose(ra[0, 0, 12, 0], counts[0, 0] * (1 - x) ** 12, rtol=1e-12)
    assert ra[0, 0, 5, 5] == 0.0                                         # (off the simplex)
    code = spec.code(0, 1, (4, 8))
    sites = spec.sites_with(codes[2], 0, code)
    assert sites.tolist() == [int(c) for c, k in zip(s.centres, codes[2]) if k == code]
    with pytest.raises(ValueError, match="one row"):
        spec.sites_with(codes, 0, code)
    with pytest.raises(ValueError, match="sum to 12 at most"):
        spec.cell(0, 0, (7, 6))


def test_statistics_sources_and_offer():
    stat = Statistics.per_walker([st.ENTHALPY, st.environment(2), st.pattern(1), st.environment(0)])
    assert stat.sources(3, 2, 0, 1, 5, 4).tolist() == [0, 2 + 3 + 2 + 24 + 5 + 2, 2 + 3 + 2 + 24 + 1, 2 + 3 + 2 + 24 + 5]
    assert stat.environment_columns() == [1, 3]
    with pytest.raises(ValueError, match="outside the 4 cells of the environment spec"):
        Statistics.per_walker([st.environment(4)]).sources(3, 2, 0, 0, 0, 4)
    with pytest.raises(ValueError, match="negative"):
        st.environment(-1)
    rng = np.random.default_rng(0)
    H, f = rng.random((6, 2)), rng.random((6, 2, 3))
    pat, env = rng.integers(0, 9, size=(6, 2, 5)), rng.integers(0, 9, size=(6, 2, 4))
    rec = StatisticsRecord(stat, 2)
    rec.offer(H, f, patterns=pat, environments=env)
    np.testing.assert_allclose(rec.mean()[:, 1], env[:, :, 2].mean(axis=0), rtol=1e-12)
    np.testing.assert_allclose(rec.mean()[:, 3], env[:, :, 0].mean(axis=0), rtol=1e-12)
    np.testing.assert_allclose(rec.mean()[:, 2], pat[:, :, 1].mean(axis=0), rtol=1e-12)


# ---- the C struct and the refusals ---------------------------------------------------------------------------------------
def test_c_struct_and_describe():
    sc, obs, spec = case_spec("rocksalt333_two_sublattices")
    b = spec.sets[1]  # (the second set with rows of another width)
    spec = Environments(obs, [spec.sets[0], EnvironmentSet(b.centres, b.neighbours[:, :4], b.centre_class_of_kind, b.n_centre_classes,
                                                           b.neigh_class_of_kind, b.n_neigh_classes)])
    assert spec.n_sets == 2 and (spec.sets[0].width, spec.sets[1].width) == (6, 4)
    s, keep = spec.c_struct()
    assert isinstance(s, capi.smolmc_environments) and s.n_sets == 2
    assert [s.width[e] for e in range(2)] == [x.width for x in spec.sets]
    assert [s.centre_ptr[e] for e in range(3)] == spec.centre_ptr.tolist()
    n0, z0 = spec.sets[0].n_centres, spec.sets[0].width
    assert s.centres[n0] == spec.sets[1].centres[0] and s.neighbours[n0 * z0] == spec.sets[1].neighbours[0, 0]
    assert C.sizeof(capi.smolmc_environments) == 9 * 8
    d = spec.describe()
    assert d["cell_ptr"] == spec.cell_ptr.tolist() and d["width"] == [x.width for x in spec.sets]
    assert (environments.MAX_ENV_SETS, environments.MAX_ENV_WIDTH, environments.MAX_ENV_CENTRE_CLASSES,
            environments.MAX_ENV_NEIGH_CLASSES, environments.MAX_ENV_CELLS) == (
        capi.MAX_ENV_SETS, capi.MAX_ENV_WIDTH, capi.MAX_ENV_CENTRE_CLASSES, capi.MAX_ENV_NEIGH_CLASSES, capi.MAX_ENV_CELLS)
    assert capi.SAMPLE_ENVIRONMENTS == 512


def test_validation_errors():
    obs = Observables(np.zeros(6, np.int32), 2, site_ncodes=np.full(6, 2))
    rows = np.array([[1, 2], [3, -1]])
    ok = lambda **kw: EnvironmentSet(**{**dict(centres=[0, 1], neighbours=rows, centre_class_of_kind=[0, 1], n_centre_classes=2,  # noqa: E731
                                              neigh_class_of_kind=[0, 1], n_neigh_classes=2), **kw})
    ok()
    with pytest.raises(ValueError, match="width must be 1..64"):
        ok(neighbours=np.zeros((2, 65), int))
    with pytest.raises(ValueError, match="width must be 1..64"):
        ok(neighbours=np.zeros((2, 0), int))
    with pytest.raises(ValueError, match="one row per centre"):
        ok(neighbours=rows[:1])
    with pytest.raises(ValueError, match="n_centre_classes must be 1..15"):
        ok(n_centre_classes=16)
    with pytest.raises(ValueError, match="n_neigh_classes must be 1..4"):
        ok(n_neigh_classes=5)
    with pytest.raises(ValueError, match="n_neigh_classes must be 1..4"):
        ok(n_neigh_classes=0)
    with pytest.raises(ValueError, match="centre_class_of_kind must hold -1 .. 1: class out of range"):
        ok(centre_class_of_kind=[0, 2])
    with pytest.raises(ValueError, match="neigh_class_of_kind must hold -1 .. 1: class out of range"):
        ok(neigh_class_of_kind=[-2, 0])
    with pytest.raises(ValueError, match="holds 1..8 sets, got 0"):
        Environments(obs, [])
    with pytest.raises(ValueError, match="holds 1..8 sets, got 9"):
        Environments(obs, [ok()] * 9)
    with pytest.raises(ValueError, match="class maps have 3 entries"):
        Environments(obs, [ok(centre_class_of_kind=[0, 1, 0], neigh_class_of_kind=[0, 1, 0])])
    with pytest.raises(ValueError, match="centre out of range"):
        Environments(obs, [ok(centres=[0, 6])])
    with pytest.raises(ValueError, match="neighbour slot out of range"):
        Environments(obs, [ok(neighbours=np.array([[1, 6], [0, 0]]))])
    with pytest.raises(ValueError, match="neighbour slot out of range"):
        Environments(obs, [ok(neighbours=np.array([[1, -2], [0, 0]]))])
    wide = np.zeros((1, 12), int)
    with pytest.raises(ValueError, match="4394 cells, larger than MAX_ENV_CELLS = 4096"):
        Environments(obs, [EnvironmentSet([0], wide, [0, 1], 2, [0, 1, ][:2], 3)])
    at_limit = Environments(obs, [EnvironmentSet([0], np.zeros((1, 7), int), [0, 0], 1, [0, 1], 4)])
    assert at_limit.n_cells == 4096
    with pytest.raises(ValueError, match='"kind", "code" or one integer per kind'):
        Environments.from_rows(obs, [0], rows[:1], centre_classes=np.zeros(3, int))
