"""Per-walker chemical potentials, the parts that need no GPU: the mapping of values to the rows of
smolmc_set_walker_mu, the host restatement of the chemical work, the sharding of the values by global walker, the
container's metadata and the argument handling of tools/mu_scan.py."""

import os
import subprocess
import sys

import numpy as np
import pytest

from smol_amd import capi, engine, moca, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _two_sublattice_ensemble():
    model = synth.build_cluster_model(synth.rocksalt_prim(anion_charges=(-2.0, -1.0)), {2: 4.5})
    sc = synth.build_supercell(model, [2, 2, 2])
    return sc, moca.Ensemble.from_cluster_expansion(sc, synth.random_coefs(model, seed=2))


def _reference_rows(ens, dicts):
    """Row k of walker r = the row the chemical_potentials setter writes on the sites of active sublattice k."""
    rows = []
    for d in dicts:
        ens.chemical_potentials = d
        rows.append([ens._mu_table[s.sites[0]].copy() for s in ens.active_sublattices])
    return np.array(rows)


def test_rows_of_a_two_sublattice_ensemble_follow_the_setters_table():
    sc, ens = _two_sublattice_ensemble()
    rng = np.random.default_rng(1)
    dicts = [{sp: float(rng.normal()) for sp in ens.species} for _ in range(5)]
    ens.chemical_potentials = dicts[0]
    rows = ens.walker_mu_rows(dicts)
    assert rows.shape == (5, 2, 3)
    np.testing.assert_array_equal(rows, _reference_rows(ens, dicts))
    assert np.all(rows[:, 1, 2] == 0.0)  # the anions have two species: their third column is unused
    # one dict of species -> array is the same thing
    cols = {sp: np.array([d[sp] for d in dicts]) for sp in ens.species}
    np.testing.assert_array_equal(ens.walker_mu_rows(cols), rows)
    # the rows are in the order of the tables' sublattices
    tab = ens.make_tables()
    assert tab.struct.n_sublattices == rows.shape[1] and tab.struct.mu_width == rows.shape[2]
    for k, sites in enumerate(tab.active_sites()):
        np.testing.assert_array_equal(np.sort(sites), np.sort(ens.active_sublattices[k].active_sites))


def test_rows_of_a_split_ensemble_keep_the_codes_columns():
    model = synth.build_cluster_model(synth.rocksalt_prim(), {2: 6.0})
    sc = synth.build_supercell(model, [2, 2, 2])
    ens = moca.Ensemble.from_cluster_expansion(sc, synth.random_coefs(model, seed=2))
    cation = next(i for i, s in enumerate(ens.sublattices) if len(s.species) == 3)
    sub = ens.sublattices[cation]
    occu = np.zeros(ens.num_sites, dtype=np.int32)
    occu[sub.sites] = np.random.default_rng(0).integers(0, 3, len(sub.sites))
    names = sub.species
    ens.chemical_potentials = {sp: 0.1 * i for i, sp in enumerate(ens.species)}
    ens.split_sublattice_by_species(cation, occu, [[names[0], names[2]], [names[1]]])
    dicts = [{names[0]: 0.3 * r, names[2]: -0.2 * r} for r in range(4)]
    rows = ens.walker_mu_rows(dicts)
    assert rows.shape == (4, 1, 3)
    np.testing.assert_array_equal(rows, _reference_rows(ens, dicts))
    np.testing.assert_array_equal(rows[:, 0, 1], 0.0)  # (code 1 left with the other partition)
    np.testing.assert_allclose(rows[:, 0, 2], [-0.2 * r for r in range(4)])


def test_missing_species_raise_like_the_setter():
    sc, ens = _two_sublattice_ensemble()
    some = {sp: 0.0 for sp in ens.species[:-1]}
    with pytest.raises(ValueError, match="Chemical potentials given are missing species"):
        ens.walker_mu_rows([some])
    with pytest.raises(ValueError, match="one value per walker"):
        ens.walker_mu_rows({sp: np.zeros(2 + i) for i, sp in enumerate(ens.species)})


def test_chemical_work_is_the_oracles_last_feature():
    from oracle import oracle as orc

    sc, ens = _two_sublattice_ensemble()
    rng = np.random.default_rng(3)
    dicts = [{sp: float(rng.normal()) for sp in ens.species} for _ in range(4)]
    rows = ens.walker_mu_rows(dicts)
    occ = np.zeros((4, ens.num_sites), dtype=np.int32)
    for s in ens.sublattices:
        occ[:, s.sites] = rng.choice(s.encoding, size=(4, len(s.sites)))
    ens.chemical_potentials = dicts[0]
    work = engine.chemical_work(ens.make_tables(), occ, rows)
    for r, d in enumerate(dicts):
        ens.chemical_potentials = d
        feat = orc.OracleEvaluator(ens.make_tables()).feature_vector(occ[r])
        assert work[r] == pytest.approx(feat[-1], rel=1e-13, abs=1e-13)


def _sampler(ens, nwalkers, values, **kw):
    return moca.Sampler.from_ensemble(ens, temperature=np.linspace(500.0, 900.0, 1)[0], nwalkers=nwalkers,
                                      seeds=list(range(1, nwalkers + 1)), chemical_potentials=values, **kw)


def test_values_are_sharded_by_global_walker_like_seeds():
    sc, ens = _two_sublattice_ensemble()
    rng = np.random.default_rng(5)
    dicts = [{sp: float(rng.normal()) for sp in ens.species} for _ in range(6)]
    ens.chemical_potentials = dicts[0]
    whole = _sampler(ens, 6, dicts, rank=0, world_size=1)
    assert whole.walker_chemical_potentials == ens.walker_chemical_potentials(dicts)
    assert [k.chemical_potentials for k in whole.mckernels] == whole.walker_chemical_potentials
    parts = [_sampler(ens, 6, dicts, rank=r, world_size=2) for r in range(2)]
    assert parts[0].walker_chemical_potentials + parts[1].walker_chemical_potentials == whole.walker_chemical_potentials
    for r, p in enumerate(parts):
        assert p.seeds == whole.seeds[3 * r:3 * r + 3]
        np.testing.assert_array_equal(p.samples.get_chemical_potentials(), whole.samples.get_chemical_potentials()[3 * r:3 * r + 3])
    with pytest.raises(ValueError, match="expected chemical potentials for 6 walkers"):
        whole.set_chemical_potentials(dicts[:4])
    # replica exchange is refused on such a sampler
    from smol_amd import parallel

    rex = parallel.ReplicaExchange(np.linspace(500.0, 900.0, 6), 6)
    with pytest.raises(ValueError, match="no valid move between walkers of different Hamiltonians"):
        parallel.run_replica_exchange(whole, rex, 1, 10)
    whole.set_chemical_potentials(None)
    assert whole.walker_chemical_potentials is None and "walker_chemical_potentials" not in whole.samples.metadata
    # an ensemble without chemical potentials has no chemical-work feature to price
    ens.chemical_potentials = None
    with pytest.raises(ValueError, match="need a semigrand ensemble"):
        _sampler(ens, 6, dicts, rank=0, world_size=1)


def test_container_keeps_the_values(tmp_path):
    sc, ens = _two_sublattice_ensemble()
    rng = np.random.default_rng(7)
    dicts = [{sp: float(rng.normal()) for sp in ens.species} for _ in range(3)]
    ens.chemical_potentials = dicts[0]
    sampler = _sampler(ens, 3, dicts, rank=0, world_size=1)
    c = sampler.samples
    want = np.array([[d[sp] for sp in ens.species] for d in dicts])
    np.testing.assert_array_equal(c.get_chemical_potentials(), want)
    assert c.get_chemical_potentials().shape == (3, len(ens.species))
    # a block of samples, then every way out and back in
    n = 4
    block = dict(occupancy=np.zeros((n, 3, ens.num_sites), np.uint8), features=np.zeros((n, 3, len(ens.natural_parameters))),
                 enthalpy=np.zeros((n, 3, 1)), temperature=np.full((n, 3, 1), 500.0), accepted=np.ones((n, 3, 1), bool))
    c.append_block(block, thinned_by=10)
    c.to_npz(tmp_path / "c.npz")
    back = moca.SampleContainer.from_npz(tmp_path / "c.npz", ens)
    np.testing.assert_array_equal(back.get_chemical_potentials(), want)
    assert back.metadata["walker_chemical_potentials"]["species"] == [str(s) for s in ens.species]
    again = moca.SampleContainer.from_dict(c.as_dict(), ens)
    np.testing.assert_array_equal(again.get_chemical_potentials(), want)
    stream = c.get_backend(str(tmp_path / "stream"))
    c.flush_to_backend(stream)
    streamed = moca.SampleContainer.from_stream(str(tmp_path / "stream"), ens)
    np.testing.assert_array_equal(streamed.get_chemical_potentials(), want)
    # without per-walker values: the ensemble's, for every walker
    plain = moca.Sampler.from_ensemble(ens, temperature=500.0, nwalkers=2, seeds=[1, 2], rank=0, world_size=1)
    np.testing.assert_array_equal(plain.samples.get_chemical_potentials(), np.tile(want[0], (2, 1)))


def test_config14_is_config3_with_a_grid():
    from smol_amd import workloads

    w = workloads.config14(count=128, dim=3, total=256, first=128)
    rows, (nT, nmu) = w.extras["walker_mu"], w.extras["grid"]
    assert rows.shape == (128, 1, 3) and (nT, nmu) == (4, 64) and w.temperature.shape == (128,)
    base = workloads._mu_rows(w.sc, workloads.CONFIG3_MU)[0]
    np.testing.assert_allclose(rows[:, 0, [0, 2]], np.tile(base[[0, 2]], (128, 1)))
    np.testing.assert_allclose(rows[:64, 0, 1] - base[1], np.linspace(-2.0, 2.0, 64))
    assert np.all(w.temperature[:64] == w.temperature[0]) and w.temperature[64] > w.temperature[0]  # global walkers 128 .. 255
    assert 14 in workloads.BUILDERS


def test_mu_scan_arguments():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "mu_scan.py"), "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--sweep" in out.stdout and "T x mu grid" in out.stdout
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import mu_scan
    finally:
        sys.path.pop(0)
    a = mu_scan.parse_args(["--config", "3", "--T", "30000", "40000", "--mu=-1:1:5", "--walkers", "2", "--sweep", "up,down", "--dry-run"])
    T, j = mu_scan.grid_of(a)
    assert len(T) == 20 and T[0] == 30000.0 and T[-1] == 40000.0 and j[:4].tolist() == [0, 0, 1, 1]
    stages = mu_scan.stages_of(a)
    assert len(stages) == 1 + 2 * 4 and stages[0].tolist() == [0, 1, 2, 3, 4]
    assert stages[4].tolist() == [4] * 5 and stages[-1].tolist() == [0] * 5  # all the way up, all the way down
    with pytest.raises(SystemExit):
        mu_scan.parse_args(["--config", "3", "--T", "1", "--mu", "0:1:2", "--sweep", "sideways"])
    with pytest.raises(SystemExit):
        mu_scan.parse_args(["--mson", "x.mson", "--T", "1", "--mu", "0:1:2"])  # (--species is needed)
