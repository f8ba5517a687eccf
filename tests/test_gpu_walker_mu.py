"""Per-walker chemical potentials (smolmc_set_walker_mu): a mu-T grid in one semigrand handle.

A walker's Philox stream depends on its seed alone, so walker r of a handle with per-walker rows is pinned by a
ONE-walker CPU oracle built with row r as its chemical-potential table, seed r's seed and start.  Occupancies and
counters bit-equal; enthalpies / features at the tolerances of tests/test_gpu_parity.py.

Settings of the cases (temperature, spread of mu) are the ones under which, on the oracle ALONE with one start and
one seed for all walkers, every walker accepts between 5 % and 95 % of 3000 flips and no two walkers end alike
(`_oracle_condition`, asserted in the parity test before the engine is compared): a case that froze, or in which mu
did nothing, would hide a kernel that ignores the rows.

rocksalt333_two_sublattices in correlation mode has several correlation functions per orbit on a multi-class model:
its Metropolis handle runs mc_lean_multi_kernel with lazy cluster features, where the chemical work is
one of the two scalar features the kernel carries.  On the oracle alone its walkers accept 0.22 - 0.34 at 20000 K,
as in interaction mode (the decisions are the same: only the trace differs)."""

import os

import numpy as np
import pytest

from smol_amd import capi
from tests.cases import GOLD, load_case, tables_for

pytestmark = pytest.mark.gpu

T = np.load(os.path.join(GOLD, "trajectories.npz"))
MODES = {"int": capi.FEATURES_INTERACTIONS, "corr": capi.FEATURES_CORRELATIONS}
RTOL, ATOL = 1e-10, 1e-9
CHUNKS = (1, 7, 16, 33, 500)


# ---- the cases: name -> (tables for a chemical-potential table, rows (R, n_sublattices, W), temperature, start) ----
class Case:
    """One model with R rows of chemical potentials: ``tables(mu_table)`` builds its TableSet, ``rows`` is
    (R, n_sublattices, mu_width) in the layout of smolmc_set_walker_mu, ``table_of(row)`` the per-site table a
    one-walker oracle of that row is created with."""

    def __init__(self, tables, num_sites, rows, temperature, start, step, family, bias=None):
        self.tables, self.N, self.T, self.start, self.step, self.family = tables, num_sites, temperature, start, step, family
        self.bias = bias
        W = np.asarray(rows).shape[-1]
        self.subs = self._make(np.zeros((num_sites, W))).active_sites()
        self.rows = np.ascontiguousarray(np.asarray(rows, dtype=np.float64).reshape(len(rows), len(self.subs), W))
        self.R = len(self.rows)

    def _make(self, mu_table):
        tab = self.tables(mu_table)
        if self.bias is not None:
            self.bias(tab)
        return tab

    def table_of(self, row):
        mu = np.zeros((self.N, self.rows.shape[-1]))
        for k, sites in enumerate(self.subs):
            mu[sites] = row[k]
        return mu

    def engine_tables(self, row=None):
        return self._make(self.table_of(np.zeros_like(self.rows[0]) if row is None else row))

    def config(self, R):
        return capi.make_config(R, capi.KERNEL_METROPOLIS, self.step)

    def starts(self, rng, R, same):
        occ = np.array([self.start(rng) for _ in range(1 if same else R)])
        return np.repeat(occ, R, axis=0) if same else occ


def _golden_case(name, mode, temperature, rows, family):
    c = load_case(name)
    nsp = np.array([c["model"].prim.nspecies[b] for b in c["sc"].site_b])
    N = c["sc"].num_sites
    return Case(lambda mu: tables_for(name, MODES[mode], mu_table=mu), N, rows, temperature,
                lambda rng: (rng.random(N) * nsp).astype(np.int32), capi.STEP_FLIP, family)


def _two_sublattice_rows():
    """rows G_mu * s, s in linspace(-2, 2, 5): G_mu is the per-site table of the golden trajectories"""
    tab = tables_for("rocksalt333_two_sublattices", MODES["int"], mu_table=T["G_mu"])
    base = np.array([T["G_mu"][sites[0]] for sites in tab.active_sites()])
    return np.array([base * s for s in np.linspace(-2.0, 2.0, 5)])


def _table_one():
    """TableFlip on one sublattice, as tests/test_gpu_table_flip.py builds it (Li+ / Mn3+ / Ti4+, one flip direction)"""
    from smol_amd import ewald as ew
    from smol_amd import synth
    from tests.test_table_flip import FLIP_TABLE, _neutral_occ

    model = synth.build_cluster_model(synth.rocksalt_prim(), {2: 3.5})
    sc = synth.build_supercell(model, [3, 3, 3])
    coefs = synth.random_coefs(model, seed=5, scale=0.05)
    ewt = ew.supercell_ewald(sc)

    def tables(mu):
        return capi.TableSet.from_synth(sc, coefs, ewald=ewt, ewald_coef=0.05, mu_table=mu, flip_table=FLIP_TABLE, swap_weight=0.2)

    # the flip direction 3 Mn3+ -> Li+ + 2 Ti4+ gains mu_Li - 3 mu_Mn + 2 mu_Ti: rows that move it from -0.6 to +0.6 eV.
    # On the oracle alone (one start, seed 777, 3000 steps) the walkers accept 0.52 / 0.48 / 0.44 / 0.38 / 0.33 / 0.29 at
    # 10000 K; at 6000 K and below the last three walk the same chain (the chain sits where the direction is infeasible)
    rows = np.array([[[0.1, -0.2 - d / 3.0, 0.05]] for d in np.linspace(-0.6, 0.6, 6)])
    return Case(tables, sc.num_sites, rows, 10000.0, lambda rng: _neutral_occ(sc, 3, rng), capi.STEP_TABLE_FLIP, "lean")


def _table_two():
    """TableFlip across the cation and the anion sublattice (tests/test_gpu_table_flip.py), with chemical potentials"""
    from smol_amd import moca, synth

    model = synth.build_cluster_model(synth.rocksalt_prim(anion_charges=(-2.0, -1.0)), {2: 4.5})
    sc = synth.build_supercell(model, [3, 3, 3])
    ens = moca.Ensemble.from_cluster_expansion(sc, synth.random_coefs(model, seed=8, scale=0.02), ewald_coefficient=0.05)
    table = np.asarray(ens.composition_space(optimize_basis=True, table_ergodic=True).flip_table)
    P = sc.size

    def tables(mu):
        ens.chemical_potentials = dict(zip(ens.species, list(mu[0, :3]) + list(mu[P, :2])))  # (cations, then anions)
        return ens.make_tables(flip_table=table, swap_weight=0.15)

    def start(rng):  # 17 Li+ + 8 Mn3+ + 2 Ti4+ = +49, 22 O2- + 5 F- = -49
        occ = np.zeros(sc.num_sites, dtype=np.int32)
        perm = rng.permutation(P)
        occ[perm[:8]] = 1
        occ[perm[8:10]] = 2
        occ[P + rng.permutation(P)[:5]] = 1
        return occ

    # (on the oracle alone, one start, seed 777, 3000 steps at 6000 K: acceptance 0.14 / 0.15 / 0.18 / 0.21 / 0.27)
    rows = np.array([[[0.0, d, -d], [0.0, 0.5 * d, 0.0]] for d in np.linspace(-0.6, 0.6, 5)])
    return Case(tables, sc.num_sites, rows, 6000.0, start, capi.STEP_TABLE_FLIP, "lean-multi")


def _arange_rows(nsp, dmus):
    return np.array([[np.arange(nsp) * d] for d in dmus])


CASES = {
    "fcc_prim666_triplets-corr": lambda: _golden_case("fcc_prim666_triplets", "corr", 3000.0, _arange_rows(2, np.linspace(-0.12, 0.12, 7)), "lean"),
    "fcc_conv444_pairs-int": lambda: _golden_case("fcc_conv444_pairs", "int", 3000.0, _arange_rows(2, np.linspace(-0.12, 0.12, 7)), "lean"),
    "rocksalt444_ewald-int": lambda: _golden_case("rocksalt444_ewald", "int", 40000.0, _arange_rows(3, np.linspace(-3.0, 3.0, 7)), "lean"),
    "rocksalt333_two_sublattices-int": lambda: _golden_case("rocksalt333_two_sublattices", "int", 20000.0, _two_sublattice_rows(), "lean-multi"),
    "rocksalt333_two_sublattices-corr": lambda: _golden_case("rocksalt333_two_sublattices", "corr", 20000.0, _two_sublattice_rows(), "lean-multi"),
    "table_flip_one_sublattice": _table_one,
    "table_flip_two_sublattices": _table_two,
}


# ---- R one-walker oracles as one object ------------------------------------------------------------------------
class OracleGrid:
    def __init__(self, case, rows=None):
        from oracle import oracle as orc

        self.case = case
        self.rows = case.rows if rows is None else rows
        self.walkers = [orc.OracleMC(case.engine_tables(row), case.config(1)) for row in self.rows]

    def set_state(self, occ, seeds, temps):
        temps = np.broadcast_to(np.asarray(temps, float), (len(self.walkers),))
        for r, w in enumerate(self.walkers):
            w.set_state(occ[r:r + 1], np.asarray(seeds[r:r + 1], dtype=np.uint64), temps[r:r + 1])

    def set_counters(self, n_steps, n_accepted):
        for r, w in enumerate(self.walkers):
            w.set_counters(n_steps[r:r + 1], n_accepted[r:r + 1])

    def run(self, n):
        for w in self.walkers:
            w.run(n)

    def get_state(self):
        st = [w.get_state() for w in self.walkers]
        return {k: np.concatenate([s[k] for s in st]) for k in st[0]}


def _oracle_condition(case):
    """On the oracle alone -- one start (default_rng(5), first draw) and seed 777 for every walker, 3000 steps: every
    walker's acceptance in (0.05, 0.95) and no two walkers with the same n_accepted AND final occupancy."""
    ora = OracleGrid(case)
    occ = case.starts(np.random.default_rng(5), case.R, same=True)
    ora.set_state(occ, np.full(case.R, 777, dtype=np.uint64), case.T)
    ora.run(3000)
    st = ora.get_state()
    acc = st["n_accepted"] / 3000.0
    print("oracle acceptance per walker:", np.round(acc, 4))
    assert np.all((acc > 0.05) & (acc < 0.95)), acc
    for a in range(case.R):
        for b in range(a + 1, case.R):
            assert not (st["n_accepted"][a] == st["n_accepted"][b] and np.array_equal(st["occupancy"][a], st["occupancy"][b])), (a, b)
    return acc


def _assert_same(a, b, feature_atol=1e-8):
    assert np.array_equal(a["occupancy"], b["occupancy"])
    assert np.array_equal(a["n_accepted"], b["n_accepted"])
    assert np.array_equal(a["n_steps"], b["n_steps"])
    assert np.array_equal(a["accepted"], b["accepted"])
    np.testing.assert_allclose(a["enthalpy"], b["enthalpy"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(a["features"], b["features"], rtol=RTOL, atol=feature_atol)


def _start(case, seed=5):
    rng = np.random.default_rng(seed)
    occ = case.starts(rng, case.R, same=False)
    seeds = np.arange(100, 100 + case.R, dtype=np.uint64) * np.uint64(7919)
    return occ, seeds


def _engine(case, R=None, row=None):
    from smol_amd.engine import Engine

    return Engine(case.engine_tables(row), case.config(case.R if R is None else R))


# ---- 1. oracle parity per family ---------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", ["1", "3e3", "1e9"], ids=["default-band", "wide-band", "always-exact"])
@pytest.mark.parametrize("name", list(CASES))
def test_walker_rows_match_one_walker_oracles(name, scale, monkeypatch):
    monkeypatch.setenv("SMOLMC_FAST_EPS_SCALE", scale)
    case = CASES[name]()
    if scale == "1":
        _oracle_condition(case)
    occ, seeds = _start(case)
    eng, ora = _engine(case), OracleGrid(case)
    eng.set_walker_mu(case.rows)
    info = eng.kernel_info()
    assert info.startswith(case.family + " ") and " walker_mu=1 " in info, info
    np.testing.assert_array_equal(eng.get_walker_mu(), case.rows)
    eng.set_state(occ, seeds, case.T)  # (the rows survive set_state and price the initial trace)
    ora.set_state(occ, seeds, case.T)
    _assert_same(eng.get_state(), ora.get_state(), feature_atol=ATOL)
    for chunk in CHUNKS:
        eng.run(chunk)
        ora.run(chunk)
        a = eng.get_state()
        _assert_same(a, ora.get_state())
    np.testing.assert_allclose(a["features"][:, -1], eng.chemical_work(a["occupancy"], case.rows), rtol=RTOL, atol=1e-8)
    np.testing.assert_allclose(a["features"][:, :-1], eng.eval_full(a["occupancy"])[:, :-1], rtol=RTOL, atol=1e-8)
    assert 0 < a["n_accepted"].sum() < a["n_steps"].sum()
    eng.close()


# ---- 2. equal rows are the uniform handle ------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_equal_rows_walk_the_chains_of_the_untouched_handle(name):
    case = CASES[name]()
    occ, seeds = _start(case)
    row = case.rows[1]
    plain, rows = _engine(case, row=row), _engine(case, row=row)
    rows.set_walker_mu(np.repeat(row[None], case.R, axis=0))
    assert "walker_mu=1" in rows.kernel_info() and "walker_mu" not in plain.kernel_info()
    np.testing.assert_array_equal(plain.get_walker_mu(), rows.get_walker_mu())
    temps = np.linspace(0.7, 1.3, case.R) * case.T
    for e in (plain, rows):
        e.set_state(occ, seeds, temps)
    for chunk in CHUNKS:
        plain.run(chunk)
        rows.run(chunk)
        a, b = plain.get_state(), rows.get_state()
        assert np.array_equal(a["occupancy"], b["occupancy"])
        assert np.array_equal(a["n_accepted"], b["n_accepted"]) and np.array_equal(a["n_steps"], b["n_steps"])
        np.testing.assert_allclose(a["enthalpy"], b["enthalpy"], rtol=0, atol=1e-10)
    assert 0 < a["n_accepted"].sum() < a["n_steps"].sum()
    plain.close()
    rows.close()


# ---- 3. sweep semantics --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fcc_prim666_triplets-corr", "rocksalt444_ewald-int", "rocksalt333_two_sublattices-int",
                                  "table_flip_one_sublattice"])
def test_setting_rows_between_runs_is_a_sweep(name):
    case = CASES[name]()
    occ, seeds = _start(case)
    eng = _engine(case, row=case.rows[0])
    eng.set_state(occ, seeds, case.T)
    eng.run(300)
    before = eng.get_state()
    new_rows = case.rows[::-1].copy()
    eng.set_walker_mu(new_rows)
    st = eng.get_state()
    assert np.array_equal(st["occupancy"], before["occupancy"]) and np.array_equal(st["n_steps"], before["n_steps"])
    np.testing.assert_allclose(st["features"][:, -1], eng.chemical_work(st["occupancy"], new_rows), rtol=RTOL, atol=ATOL)
    np.testing.assert_array_equal(st["features"][:, :-1], before["features"][:, :-1])  # CE and Ewald features unchanged
    np.testing.assert_allclose(st["enthalpy"], st["features"] @ eng.natural_parameters, rtol=RTOL, atol=ATOL)
    # the next 500 steps: fresh one-walker oracles of the new rows, from the occupancy and the counters of that moment
    ora = OracleGrid(case, new_rows)
    ora.set_state(st["occupancy"], seeds, case.T)
    ora.set_counters(st["n_steps"], st["n_accepted"])
    eng.run(500)
    ora.run(500)
    _assert_same(eng.get_state(), ora.get_state())
    # NULL: the create-time table again
    eng.set_walker_mu(None)
    assert "walker_mu" not in eng.kernel_info()
    st = eng.get_state()
    back = np.repeat(case.rows[:1], case.R, axis=0)
    np.testing.assert_array_equal(eng.get_walker_mu(), back)
    np.testing.assert_allclose(st["features"][:, -1], eng.chemical_work(st["occupancy"], back), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(st["features"], eng.eval_full(st["occupancy"]), rtol=RTOL, atol=1e-8)
    ora = OracleGrid(case, back)
    ora.set_state(st["occupancy"], seeds, case.T)
    ora.set_counters(st["n_steps"], st["n_accepted"])
    eng.run(200)
    ora.run(200)
    _assert_same(eng.get_state(), ora.get_state())
    eng.close()


# ---- 4. run_sampled ---------------------------------------------------------------------------------------------------
def _fugacity(tab):
    W = tab.struct.max_species
    f = np.full((tab.struct.num_sites, W), 1.0 / W)
    f[:, 0] = 0.5
    f[:, 1:] = 0.5 / max(W - 1, 1)
    tab.set_bias(capi.BIAS_FUGACITY, f)


@pytest.mark.parametrize("name,biased", [("fcc_prim666_triplets-corr", False), ("rocksalt444_ewald-int", False),
                                         ("rocksalt333_two_sublattices-int", False), ("fcc_conv444_pairs-int", True)])
def test_sampled_rows_equal_the_oracle_at_every_step(name, biased):
    case = CASES[name]()
    if biased:
        case.bias = _fugacity
    occ, seeds = _start(case)
    eng, ora = _engine(case), OracleGrid(case)
    eng.set_walker_mu(case.rows)
    eng.set_state(occ, seeds, case.T)
    ora.set_state(occ, seeds, case.T)
    ns, thin = 6, 37
    smp = eng.run_sampled(ns, thin, occupancy=True, bias=biased)
    for j in range(ns):
        ora.run(thin)
        b = ora.get_state()
        assert np.array_equal(smp["occupancy"][j], b["occupancy"])
        assert np.array_equal(smp["accepted"][j], b["accepted"])
        np.testing.assert_allclose(smp["enthalpy"][j], b["enthalpy"], rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(smp["features"][j], b["features"], rtol=RTOL, atol=1e-8)
        if biased:
            np.testing.assert_allclose(smp["bias"][j], np.concatenate([w.get_bias() for w in ora.walkers]), rtol=RTOL, atol=ATOL)
    _assert_same(eng.get_state(), ora.get_state())
    eng.close()


# ---- 5. the float32 accept bound follows the rows -------------------------------------------------------------------
def _mu_max(info):
    return float(info.split(" mu_max=")[1].split()[0])


def test_mu_max_follows_every_set_call():
    case = CASES["fcc_prim666_triplets-corr"]()
    eng = _engine(case)  # created with zeros
    rows = np.zeros_like(case.rows)
    rows[3, 0, 1] = -20.0
    rows[3, 0, 0] = 20.0
    eng.set_walker_mu(rows)
    assert _mu_max(eng.kernel_info()) == np.abs(rows).max() == 20.0
    eng.set_walker_mu(case.rows)
    assert _mu_max(eng.kernel_info()) == np.abs(case.rows).max()
    # a walker at +-20 eV next to walkers at the small rows: every decision still the oracle's
    occ, seeds = _start(case)
    mixed = case.rows.copy()
    mixed[3] = rows[3]
    eng.set_walker_mu(mixed)
    assert _mu_max(eng.kernel_info()) == 20.0
    ora = OracleGrid(case, mixed)
    eng.set_state(occ, seeds, case.T)
    ora.set_state(occ, seeds, case.T)
    eng.run(700)
    ora.run(700)
    _assert_same(eng.get_state(), ora.get_state())
    eng.close()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason(monkeypatch):
    from smol_amd.engine import Engine, EngineError

    case = CASES["fcc_prim666_triplets-corr"]()
    rows = case.rows
    # wrong shapes: ValueError on the Python side
    eng = _engine(case)
    for bad in (rows[:-1], rows[:, :, :1], rows.reshape(case.R, -1)):
        with pytest.raises(ValueError, match="shape"):
            eng.set_walker_mu(bad)
    # replay / exchange / temperature import while rows are set
    eng.set_walker_mu(rows)
    occ, seeds = _start(case)
    eng.set_state(occ, seeds, case.T)
    with pytest.raises(EngineError, match="smolmc_replay while per-walker chemical potentials are set"):
        eng.replay(np.zeros((case.R, 1, 2), dtype=np.int32), np.full((case.R, 1), 0.5))
    import torch

    buf = torch.ones(4 * case.R, dtype=torch.float64, device="cuda")
    with pytest.raises(EngineError, match="no valid move between walkers of different Hamiltonians"):
        eng.import_temperature(buf.data_ptr())
    with pytest.raises(EngineError, match="no valid move between walkers of different Hamiltonians"):
        eng.exchange_dev(case.R, 0, 0, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr())
    eng.set_walker_mu(None)
    eng.import_temperature(buf.data_ptr())  # (allowed again)
    eng.close()
    # no has_mu
    plain = Engine(tables_for("fcc_prim666_triplets", MODES["int"]), capi.make_config(3, capi.KERNEL_METROPOLIS, capi.STEP_SWAP))
    with pytest.raises(EngineError, match="without has_mu"):
        plain._chk(plain._lib.smolmc_set_walker_mu(plain._h, None))
    plain.close()
    # Wang-Landau
    wl = Engine(case.engine_tables(), capi.make_config(case.R, capi.KERNEL_WANGLANDAU, capi.STEP_FLIP, min_enthalpy=-50.0,
                                                       max_enthalpy=50.0, bin_size=0.5))
    with pytest.raises(EngineError, match="one density of states"):
        wl.set_walker_mu(rows)
    wl.close()
    # mc_kernel / the universal kernel (here: a model forced off the lean families): the `not lean:` reason comes along
    monkeypatch.setenv("SMOLMC_FORCE_GENERAL", "1")
    e2 = _engine(case)
    monkeypatch.delenv("SMOLMC_FORCE_GENERAL")
    assert not e2.kernel_info().startswith("lean") and e2.not_lean_reason()
    with pytest.raises(EngineError) as err:
        e2.set_walker_mu(rows)
    assert "only the lean kernel families" in str(err.value) and "not lean: " + e2.not_lean_reason() in str(err.value)
    with pytest.raises(EngineError, match="only the lean kernel families"):
        e2.get_walker_mu()
    e2.close()


def test_distance_handle_is_refused():
    from smol_amd import sqs, synth
    from smol_amd.engine import Engine, EngineError

    m = synth.build_cluster_model(synth.fcc_prim(), {2: 7.0, 3: 5.0})
    sc, tab = sqs.distance_tables(m, np.diag([2, 2, 2]), capi.FEATURES_CORRELATIONS)
    spec = sqs.distance_spec(m, capi.FEATURES_CORRELATIONS, None, None, 1.0, 1e-5, 1.0)
    eng = Engine(tab, capi.make_config(2, capi.KERNEL_METROPOLIS, capi.STEP_SWAP), distance=spec)
    with pytest.raises(EngineError, match="a distance handle has none"):
        eng.set_walker_mu(None)
    with pytest.raises(EngineError, match="a distance handle has none"):
        eng.get_walker_mu()
    eng.close()


# ---- 7. Sampler -----------------------------------------------------------------------------------------------------
def test_sampler_runs_a_grid_and_sweeps_it():
    """4 temperatures x 4 chemical potentials in one Sampler: the samples of the engine-level run of the same seeds;
    new values between two runs continue the chains at them; the container keeps the values."""
    from smol_amd import moca, synth
    from smol_amd.engine import Engine

    model = synth.build_cluster_model(synth.rocksalt_prim(), {2: 3.5})
    sc = synth.build_supercell(model, [3, 3, 3])
    ens = moca.Ensemble.from_cluster_expansion(sc, synth.random_coefs(model, seed=5, scale=0.05))
    names = ens.species
    ens.chemical_potentials = {names[0]: 0.1, names[1]: -0.2, names[2]: 0.05}
    nw = 16
    temps = np.repeat([2000.0, 3000.0, 4500.0, 7000.0], 4)
    grid = [{names[0]: 0.1, names[1]: -0.2 + d, names[2]: 0.05} for d in np.tile(np.linspace(-0.3, 0.3, 4), 4)]
    seeds = list(range(11, 11 + nw))
    sampler = moca.Sampler.from_ensemble(ens, temperature=2000.0, nwalkers=nw, seeds=seeds, chemical_potentials=grid)
    for k, T in zip(sampler.mckernels, temps):
        k.temperature = T
    assert [k.chemical_potentials for k in sampler.mckernels] == grid
    rng = np.random.default_rng(2)
    occ = np.zeros((nw, ens.num_sites), dtype=np.int32)
    occ[:, : sc.size] = rng.integers(0, 3, size=(nw, sc.size))
    sampler.run(2000, occ, thin_by=100)
    assert "walker_mu=1" in sampler.engine.kernel_info()
    rows = ens.walker_mu_rows(grid)
    eng = Engine(ens.make_tables(), capi.make_config(nw, capi.KERNEL_METROPOLIS, capi.STEP_FLIP))
    eng.set_walker_mu(rows)
    eng.set_state(occ, np.array([k.seed64 for k in sampler.mckernels], dtype=np.uint64), temps)
    smp = eng.run_sampled(20, 100)
    c = sampler.samples
    assert np.array_equal(c.get_occupancies(flat=False), smp["occupancy"])
    np.testing.assert_allclose(c.get_feature_vectors(flat=False), smp["features"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(c.get_enthalpies(flat=False).reshape(20, nw), smp["enthalpy"], rtol=RTOL, atol=ATOL)
    comp = (smp["occupancy"][:, :, : sc.size] == 1).mean(axis=(0, 2))
    assert len(set(np.round(comp, 6))) > 8  # the grid points differ
    # a sweep: new values between two runs
    grid2 = grid[::-1]
    sampler.set_chemical_potentials(grid2)
    sampler.run(1000, thin_by=100)
    eng.set_walker_mu(ens.walker_mu_rows(grid2))
    smp2 = eng.run_sampled(10, 100)
    assert np.array_equal(c.get_occupancies(flat=False)[20:], smp2["occupancy"])
    np.testing.assert_allclose(c.get_enthalpies(flat=False)[20:].reshape(10, nw), smp2["enthalpy"], rtol=RTOL, atol=ATOL)
    np.testing.assert_array_equal(c.get_chemical_potentials(), [[d[sp] for sp in names] for d in grid2])
    sampler.anneal([6000.0, 3000.0], 300, thin_by=100)  # (anneal keeps working: temperatures change, the rows stay)
    assert "walker_mu=1" in sampler.engine.kernel_info() and c.num_samples == 36
    eng.close()


# ---- 8. full size: config 14 (config 3 as a 32 T x 64 mu grid, 2048 walkers) ---------------------------------------
def test_config14_full_size_properties():
    import zlib

    from oracle import oracle as orc
    from smol_amd import synth, workloads
    from smol_amd.engine import Engine

    def checksum(x):
        return zlib.crc32(np.ascontiguousarray(x).tobytes())

    wl = workloads.config14()
    R, rows = wl.n_walkers, wl.extras["walker_mu"]
    assert R == 2048 and wl.extras["grid"] == (32, 64)
    a, b = Engine(wl.tables, wl.make_config()), Engine(wl.tables, wl.make_config())
    for e in (a, b):
        e.set_walker_mu(rows)
        e.set_state(wl.occupancy, wl.seeds, wl.temperature)
    info = a.kernel_info()
    assert info.startswith("lean ") and "field=1" in info and _mu_max(info) == np.abs(rows).max(), info
    a.run(1200)
    for chunk in (7, 593, 600):
        b.run(chunk)
    sa, sb = a.get_state(), b.get_state()
    assert checksum(sa["occupancy"]) == checksum(sb["occupancy"])
    assert checksum(sa["n_accepted"]) == checksum(sb["n_accepted"])
    # running trace == from-scratch evaluation: CE and Ewald entries by eval_full, the chemical work at the walkers' rows
    full = a.eval_full(sa["occupancy"])
    np.testing.assert_allclose(sa["features"][:, :-1], full[:, :-1], rtol=RTOL, atol=1e-7)
    work = a.chemical_work(sa["occupancy"], rows)
    np.testing.assert_allclose(sa["features"][:, -1], work, rtol=RTOL, atol=1e-7)
    want = np.concatenate([full[:, :-1], work[:, None]], axis=1) @ a.natural_parameters
    m = np.abs(want) > 1e-6
    worst = float(np.max(np.abs(sa["enthalpy"][m] - want[m]) / np.abs(want[m])))
    print(f"max relative enthalpy error [config14 running vs from scratch]: {worst:.2e}")
    assert worst < 1e-10
    acc = sa["n_accepted"] / 1200.0
    print("config14 acceptance: min %.3f mean %.3f max %.3f" % (acc.min(), acc.mean(), acc.max()))
    # oracle spot checks: the four corners of the grid
    ew = workloads._rocksalt(12)[2]
    for g in (0, 63, R - 64, R - 1):
        mu = np.zeros((wl.sc.num_sites, 3))
        mu[: wl.sc.size] = rows[g, 0]
        tab = capi.TableSet.from_synth(wl.sc, synth.random_coefs(wl.sc.model), ewald=ew, ewald_coef=0.1, mu_table=mu)
        ora = orc.OracleMC(tab, capi.make_config(1, capi.KERNEL_METROPOLIS, capi.STEP_FLIP))
        ora.set_state(wl.occupancy[g:g + 1], wl.seeds[g:g + 1], wl.temperature[g:g + 1])
        ora.run(1200)
        so = ora.get_state()
        assert np.array_equal(sa["occupancy"][g], so["occupancy"][0]), g
        assert sa["n_accepted"][g] == so["n_accepted"][0]
        assert abs(sa["enthalpy"][g] - so["enthalpy"][0]) < 1e-10 * abs(so["enthalpy"][0])
    a.close()
    b.close()
