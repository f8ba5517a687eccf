"""Population annealing on the device (smolmc_anneal_resample, smolmc_resample; pop_anneal.hip).

1. the device takes the map of the definition (parallel.PopulationAnnealing) and the rows move as the map says;
2. clones continue as fresh oracles: the test for hidden per-walker state (Ewald field, bias charges, lazy scalars);
3. Engine.resample with an explicit map, and every refusal;
4. the statistics of the whole scheme against exact enumeration, within the bounds measured on the CPU oracle;
5. Sampler.anneal_population.

The models are the small cases of tests/test_gpu_walker_mu.py with one create-time row of chemical potentials, the
biased handles of tests/test_gpu_bias.py, and mc_kernel / the universal kernel through their forcing switches.  Every
model names the factor T -> T / factor of its resampling step: chosen on the CPU oracle alone (the same chains) so that
at every shape some walker dies and some walker has two or more children (dead / with several children at R = 130 and
R = 40: lean 63 / 28 and 19 / 6 at 1.05; Ewald field 53 / 22 and 17 / 10, lean-multi 49 / 26 and 13 / 5, TableFlip 32 / 32
and 11 / 11, fugacity 25 / 25 and 9 / 9, square charge 39 / 25 and 9 / 7 at 1.2)."""

import numpy as np
import pytest

from smol_amd import capi, moca, parallel, synth
from smol_amd.engine import Engine, EngineError
from tests import pop_anneal_case as pc
from tests import wl_windows_case as wc
from tests.test_gpu_walker_mu import CASES, _assert_same

pytestmark = pytest.mark.gpu

PA = parallel.PopulationAnnealing
SHAPES = [(130, 1), (40, 2), (1, 1)]  # two wave boundaries and a tail; a population boundary inside a wave; one walker
SWITCHES = ("SMOLMC_FORCE_GENERAL", "SMOLMC_FORCE_UNIVERSAL", "SMOLMC_NO_LAZY_FEATURES")


class Model:
    def __init__(self, tables, config, start, T, factor, info, env=None, bias=False):
        self.tables, self.config, self.start, self.T, self.factor = tables, config, start, float(T), float(factor)
        self.info, self.env, self.bias = info, env, bias

    def engine(self, R, monkeypatch):
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        if self.env:
            monkeypatch.setenv(self.env, "1")
        eng = Engine(self.tables, self.config(R))
        info = eng.kernel_info()
        assert info.startswith(self.info[0]) and all(s in info for s in self.info[1:]), info
        return eng

    def starts(self, R):
        rng = np.random.default_rng(5)
        return np.array([self.start(rng) for _ in range(R)]), np.arange(100, 100 + R, dtype=np.uint64) * np.uint64(7919)


def _golden(name, factor, info, env=None):
    case = CASES[name]()
    return Model(case.engine_tables(case.rows[1]), case.config, case.start, case.T, factor, info, env)


def _biased(kind, T, factor):
    """the biased handles of tests/test_gpu_bias.py: rocksalt 3x3x3, flips; the square-charge one with the Ewald term (at
    3000 K that one freezes into one state within 300 steps: 50000 K, where the oracle accepts 0.72)"""
    model = synth.build_cluster_model(synth.rocksalt_prim(), {2: 6.0, 3: 4.5})
    sc = synth.build_supercell(model, [3, 3, 3])
    ens = moca.Ensemble.from_cluster_expansion(sc, synth.random_coefs(model, seed=4),
                                               ewald_coefficient=0.2 if kind == "square-charge" else None)
    names = ens.active_sublattices[0].species
    bias = (moca.FugacityBias(ens.sublattices, [{names[0]: 0.15, names[1]: 0.25, names[2]: 0.6}])
            if kind == "fugacity" else moca.SquareChargeBias(ens.sublattices, penalty=0.05))
    tab = ens.make_tables().set_bias(bias.bias_type, bias._table, bias.penalty)

    def start(rng):
        occ = np.zeros(sc.num_sites, dtype=np.int32)
        occ[: sc.size] = rng.integers(0, 3, size=sc.size)
        return occ

    return Model(tab, lambda R: capi.make_config(R, capi.KERNEL_METROPOLIS, capi.STEP_FLIP), start, T, factor,
                 ("lean ",), bias=True)


MODELS = {
    "lean": lambda: _golden("fcc_conv444_pairs-int", 1.05, ("lean ", "field=0")),
    "lean-ewald-field": lambda: _golden("rocksalt444_ewald-int", 1.2, ("lean ", "field=1")),
    "lean-multi": lambda: _golden("rocksalt333_two_sublattices-int", 1.2, ("lean-multi ",)),
    "lean-multi-lazy": lambda: _golden("rocksalt333_two_sublattices-corr", 1.2, ("lean-multi ", "lazy-features")),
    "table-flip": lambda: _golden("table_flip_one_sublattice", 1.2, ("lean ",)),
    "fugacity-bias": lambda: _biased("fugacity", 3000.0, 1.2),
    "square-charge-bias": lambda: _biased("square-charge", 50000.0, 1.2),
    "general-ewald-field": lambda: _golden("rocksalt444_ewald-int", 1.2, ("general ", "field=1"), "SMOLMC_FORCE_GENERAL"),
    "universal": lambda: _golden("fcc_conv444_pairs-int", 1.05, ("universal ",), "SMOLMC_FORCE_UNIVERSAL"),
}
_built = {}


def model(name):
    if name not in _built:
        _built[name] = MODELS[name]()
    return _built[name]


def _state(eng, m):
    st = eng.get_state()
    if m.bias:
        st["bias"] = eng.get_bias()
    return st


def _assert_rows(after, before, parent, bias):
    for k in ("occupancy", "features", "enthalpy", "accepted") + (("bias",) if bias else ()):
        assert np.array_equal(after[k], before[k][parent]), k
    for k in ("n_steps", "n_accepted"):  # the counters stay with the slot
        assert np.array_equal(after[k], before[k]), k


# ---- 1. the device takes the map of the definition -----------------------------------------------------------------
@pytest.mark.parametrize("R,P", SHAPES, ids=[f"R{r}-P{p}" for r, p in SHAPES])
@pytest.mark.parametrize("name", list(MODELS))
def test_device_takes_the_map_of_the_definition(name, R, P, monkeypatch):
    m = model(name)
    eng = m.engine(R, monkeypatch)
    occ, seeds = m.starts(R)
    eng.set_state(occ, seeds, m.T)
    eng.run(300)
    info, before = eng.kernel_info(), _state(eng, m)
    pa = PA([m.T, m.T / m.factor], populations=P, seed=3)
    words = pa.offset_words(0)
    res = eng.anneal_resample(np.full(P, pa.temperatures[1]), words, npop=P)
    n = R // P
    dead = multiple = 0
    for p in range(P):
        sl = slice(p * n, (p + 1) * n)
        q_np, _, href_np = PA.weights(before["enthalpy"][sl], pa.betas[0], pa.betas[1])
        assert res["href"][p] == href_np
        assert int(res["qsum"][p]) == sum(int(x) for x in res["q"][sl])
        dq = res["q"][sl].astype(np.int64) - q_np.astype(np.int64)
        print(f"{name} R={R} population {p}: max |q_dev - q_numpy| = {np.abs(dq).max()}")
        assert np.abs(dq).max() <= 1
        assert res["q"][sl].max() == 2 ** 40
        assert np.array_equal(res["parent"][sl], p * n + PA.parent_map(res["q"][sl], words[p]))
        cnt = PA.children(res["q"][sl], words[p])  # (on the definition alone: the case does something)
        dead, multiple = dead + int((cnt == 0).sum()), multiple + int((cnt >= 2).sum())
    print(f"{name} R={R} P={P}: {dead} dead walkers, {multiple} with two or more children")
    if R > 1:
        assert dead >= 1 and multiple >= 1
    after = _state(eng, m)
    _assert_rows(after, before, res["parent"], m.bias)
    assert eng.kernel_info() == info
    # the new temperatures are in force: a second step to the same temperature has db = 0, every weight is 1, the map
    # is the identity and nothing moves
    again = eng.anneal_resample(np.full(P, pa.temperatures[1]), pa.offset_words(1), npop=P)
    assert np.all(again["q"] == 2 ** 40) and np.all(again["qsum"] == n * 2 ** 40)
    assert np.array_equal(again["parent"], np.arange(R))
    same = _state(eng, m)
    for k in after:
        assert np.array_equal(same[k], after[k]), k
    eng.close()


# ---- 2. clones continue as fresh oracles ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MODELS))
def test_clones_continue_as_fresh_oracles(name, monkeypatch):
    from oracle import oracle as orc

    m = model(name)
    R, P = 40, 2
    eng = m.engine(R, monkeypatch)
    occ, seeds = m.starts(R)
    eng.set_state(occ, seeds, m.T)
    pa = PA([m.T, m.T / m.factor, m.T / m.factor ** 2], populations=P, seed=4)
    clones = 0
    for k in range(2):
        eng.run(200)
        res = eng.anneal_resample(np.full(P, pa.temperatures[k + 1]), pa.offset_words(k), npop=P)
        clones += int((res["parent"] != np.arange(R)).sum())
    assert clones >= 1
    st = eng.get_state()
    ora = orc.OracleMC(m.tables, m.config(R))
    ora.set_state(st["occupancy"], seeds, pa.temperatures[2])
    ora.set_counters(st["n_steps"], st["n_accepted"])
    if m.bias:
        np.testing.assert_allclose(eng.get_bias(), ora.get_bias(), rtol=1e-10, atol=1e-9)
    eng.run(200)
    ora.run(200)
    a, b = eng.get_state(), ora.get_state()
    _assert_same(a, b)
    assert np.all(a["n_steps"] == 600) and 0 < (a["n_accepted"] - st["n_accepted"]).sum() < 200 * R
    if m.bias:
        np.testing.assert_allclose(eng.get_bias(), ora.get_bias(), rtol=1e-10, atol=1e-9)
    eng.close()


# ---- 3. Engine.resample with an explicit map, and the refusals ------------------------------------------------------
@pytest.mark.parametrize("name", ["lean-ewald-field", "square-charge-bias", "lean-multi-lazy"])
def test_resample_with_an_explicit_map(name, monkeypatch):
    m = model(name)
    R = 9
    eng = m.engine(R, monkeypatch)
    occ, seeds = m.starts(R)
    temps = np.linspace(0.8, 1.2, R) * m.T
    eng.set_state(occ, seeds, temps)
    eng.run(150)
    before = _state(eng, m)
    parent = np.array([0, 0, 2, 7, 4, 4, 4, 7, 2])
    eng.resample(parent)
    _assert_rows(_state(eng, m), before, parent, m.bias)
    # the temperatures stayed with the slots: the chains continue as oracles at `temps`
    from oracle import oracle as orc

    ora = orc.OracleMC(m.tables, m.config(R))
    ora.set_state(before["occupancy"][parent], seeds, temps)
    ora.set_counters(before["n_steps"], before["n_accepted"])
    eng.run(150)
    ora.run(150)
    _assert_same(eng.get_state(), ora.get_state())
    eng.close()


def _refused(match):
    return pytest.raises((ValueError, EngineError), match=match)


def test_refusals(monkeypatch):
    m = model("lean")
    R = 8
    eng = m.engine(R, monkeypatch)
    occ, seeds = m.starts(R)
    eng.set_state(occ, seeds, m.T)
    before = eng.get_state()
    words = np.zeros(8, dtype=np.uint64)
    with _refused("out of range"):
        eng.resample([0, 1, 2, 3, 4, 5, 6, 8])
    with _refused("out of range"):
        eng.resample([-1, 1, 2, 3, 4, 5, 6, 7])
    with _refused("every source must map to itself"):
        eng.resample([1, 2, 2, 3, 4, 5, 6, 7])
    with pytest.raises(ValueError, match="one parent per walker"):
        eng.resample([0, 1, 2])
    with _refused("do not divide"):
        eng.anneal_resample(np.full(3, 500.0), words[:3], npop=3)
    with _refused("must be positive"):
        eng.anneal_resample([0.0], words[:1], npop=1)
    with pytest.raises(ValueError, match="one offset word per population"):
        eng.anneal_resample(np.full(2, 500.0), words[:1], npop=2)
    eng.set_temperature(np.array([m.T] * 6 + [m.T * 1.5] * 2))
    with _refused("population 1 are at different temperatures"):
        eng.anneal_resample(np.full(2, 500.0), words[:2], npop=2)
    eng.anneal_resample(np.full(4, 500.0), words[:4], npop=4)  # (populations of two: each at one temperature)
    case = CASES["fcc_conv444_pairs-int"]()
    eng.set_walker_mu(np.repeat(case.rows[:1], R, axis=0))
    with _refused("per-walker chemical potentials"):
        eng.resample(np.arange(R))
    with _refused("per-walker chemical potentials"):
        eng.anneal_resample([500.0], words[:1])
    eng.set_walker_mu(None)
    eng.resample(np.arange(R))
    after = eng.get_state()
    for k in ("n_steps", "n_accepted"):
        assert np.array_equal(after[k], before[k])
    eng.close()
    # Wang-Landau handles, with and without per-walker windows
    c = wc.case()
    wx = wc.windows(5)
    wl = Engine(c["tab"], wc.config(wx.R, wx.vmin[0], wx.vmax[0]))
    for _ in range(2):
        with _refused("Wang-Landau"):
            wl.resample(np.arange(wx.R))
        with _refused("Wang-Landau"):
            wl.anneal_resample([500.0], words[:1])
        wl.set_wl_windows(wx.vmin, wx.vmax)
    wl.close()
    # distance handles
    from smol_amd import sqs as sqs_mod
    from tests.test_gpu_sqs import setup

    mm, sc, tab, spec0, cfg = setup("binary444", capi.FEATURES_CORRELATIONS, capi.STEP_SWAP, 4)
    spec = sqs_mod.distance_spec(mm, capi.FEATURES_CORRELATIONS, np.zeros(spec0.struct.n_features), None, 1.0, 1e-5, 1.0)
    dist = Engine(tab, cfg, distance=spec)
    with _refused("distance handle"):
        dist.resample(np.arange(4))
    with _refused("distance handle"):
        dist.anneal_resample([500.0], words[:1])
    dist.close()


# ---- 4. statistics on the device ------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", pc.SEEDS)
def test_device_population_annealing_against_enumeration(seed):
    """The scheme of tests/test_pop_anneal_host.py through the device path; the bounds were measured on the oracle."""
    eng = Engine(wc.case()["tab"], pc.config(pc.WALKERS * pc.POPULATIONS))
    history = []
    pa, emean = pc.run_annealing(eng, seed, host_decide=False, history=history)
    dl, de = pa.log_partition_ratio() - pc.LNZ_EXACT, emean - pc.EMEAN_EXACT
    print(f"seed {seed}: sum ln Q - exact", np.round(dl, 4), " final mean enthalpy - exact", np.round(de, 5))
    print(f"   combined: {pa.combined_log_partition_ratio() - pc.LNZ_EXACT:+.4f} {pa.combine(emean) - pc.EMEAN_EXACT:+.5f}"
          f"   families {pa.n_families[-1]}  rho_t {np.round(pa.rho_t[-1], 2)}")
    assert pa.log_q.shape == (len(pc.TEMPERATURES) - 1, pc.POPULATIONS) and len(history) == len(pc.TEMPERATURES) - 1
    assert np.all(np.abs(dl) <= pc.LNZ_BOUND), dl
    assert np.all(np.abs(de) <= pc.EMEAN_BOUND), de
    assert abs(pa.combined_log_partition_ratio() - pc.LNZ_EXACT) <= pc.LNZ_BOUND
    assert abs(pa.combine(emean) - pc.EMEAN_EXACT) <= pc.EMEAN_BOUND
    eng.close()


# ---- 5. Sampler.anneal_population -----------------------------------------------------------------------------------
def test_sampler_anneal_population(tmp_path):
    from tests.cases import load_case

    c = load_case("fcc_conv444_pairs")
    sc = c["sc"]
    ens = moca.Ensemble.from_cluster_expansion(sc, c["coefs"])
    nw, P = 24, 2
    temps = np.geomspace(3000.0, 1000.0, 4)
    occ = (np.random.default_rng(4).random((nw, sc.num_sites)) < 0.5).astype(np.int32)

    def sampler():
        return moca.Sampler.from_ensemble(ens, temperature=3000.0, step_type="flip", nwalkers=nw, seeds=list(range(nw)))

    ref = sampler()
    ref.anneal(temps, 400, occ, thin_by=100)
    s = sampler()
    pa = s.anneal_population(temps, 400, occ, populations=P, thin_by=100, seed=2)
    a, b = s.samples, ref.samples
    assert a.num_samples == b.num_samples == 16
    for k in ("occupancy", "features", "enthalpy", "temperature", "accepted"):
        assert a.get_trace_value(k, flat=False).shape == b.get_trace_value(k, flat=False).shape, k
    np.testing.assert_array_equal(a.get_trace_value("temperature", flat=False), b.get_trace_value("temperature", flat=False))
    # the first temperature is plain sampling: the same chains as anneal
    np.testing.assert_array_equal(a.get_trace_value("occupancy", flat=False)[:4], b.get_trace_value("occupancy", flat=False)[:4])
    meta = a.metadata["population_annealing"]
    assert pa.log_q.shape == (3, P)
    np.testing.assert_array_equal(meta["log_partition_ratio"][-1], pa.log_q.sum(axis=0))
    np.testing.assert_array_equal(meta["log_partition_ratio"], np.vstack([np.zeros((1, P)), np.cumsum(pa.log_q, axis=0)]))
    assert np.array_equal(meta["n_families"][1:], pa.n_families) and meta["n_families"][0] == [nw // P] * P
    assert np.array_equal(meta["rho_t"][1:], pa.rho_t) and meta["temperatures"] == list(temps)
    assert np.all(np.asarray(meta["log_partition_ratio"][-1]) != 0.0)
    path = str(tmp_path / "samples.npz")
    a.to_npz(path)
    back = moca.SampleContainer.from_npz(path, ens)
    assert back.metadata["population_annealing"] == meta and back.num_samples == 16
