"""The adaptive step of population annealing on the device (smolmc_anneal_adaptive; the search phase of
pop_parent_kernel, pop_anneal.hip).

1. the device chooses the temperature of the definition (parallel.PopulationAnnealing.next_temperature) bit for bit, then
   takes the step of the definition to it, and the rows move as the map says;
2. the reached, forced and heating branches;
3. every refusal;
4. clones continue as fresh oracles after two adaptive steps;
5. the statistics of the whole scheme against exact enumeration, within the bounds measured on the CPU oracle;
6. Sampler.anneal_population(overlap=).

The models, their temperatures and start states are those of tests/test_gpu_pop_anneal.py.  Shape (520, 2) adds what no
test of the fixed step reaches: populations of 260, two chunks of the kernel's 256-thread loops with a tail of 4.

Bit equality of T' needs every decision of the bisection to survive the device's exp differing from NumPy's in its last
bit: a change of one q_j by +-1 moves either side of s 2^32 >= t n Q by at most n^2 2^32, so test 1 asserts that the
definition's smallest margin (|s 2^32 - t n Q| >> 32 over all evaluations, on the device's own enthalpies) is at least
4 n^2.  A condition of the case, not a skip: with the limit T / 3, overlap 0.85 and 16 halvings the smallest margins
on the CPU oracle's chains (the same chains), for the shapes (130, 1), (40, 2), (520, 2) with 4 n^2 = 6.8e4, 1.6e3, 2.7e5:
    lean (and universal)  7.3e11  9.2e9  2.4e12        lean-ewald-field    1.5e11  3.2e9  1.0e10
    table-flip            9.2e10  3.1e9  6.9e11        square-charge-bias  3.1e10  1.5e9  1.6e11
(one walker: the whole step is ok, the margin is (2^32 - t) 2^8 = 1.6e11); the heating steps at (40, 2): 1.7e9 and 1.0e9,
the forced step 1.2e14.  The least room is a factor 3.8e4."""

import numpy as np
import pytest

from smol_amd import moca, parallel
from smol_amd.engine import Engine, EngineError
from tests import pop_anneal_adaptive_case as ac
from tests import pop_anneal_case as pc
from tests import wl_windows_case as wc
from tests.test_gpu_pop_anneal import _assert_rows, _state, model
from tests.test_gpu_walker_mu import CASES, _assert_same

pytestmark = pytest.mark.gpu

PA = parallel.PopulationAnnealing
kB = parallel.kB
NAMES = ["lean", "lean-ewald-field", "table-flip", "square-charge-bias", "universal"]
SHAPES = [(130, 1), (40, 2), (1, 1), (520, 2)]
OVERLAP, N_ITER = 0.85, 16
TARGET = PA.target_word(OVERLAP)


def _start(name, R, monkeypatch, steps=300):
    m = model(name)
    eng = m.engine(R, monkeypatch)
    occ, seeds = m.starts(R)
    eng.set_state(occ, seeds, m.T)
    if steps:
        eng.run(steps)
    return m, eng


def _assert_named(eng, T):
    """smolmc_get_state_points reports T for every walker (it serves lean handles with a chemical-work feature only: the
    biased, the canonical and the universal handles here are refused whatever their temperatures, and say so)"""
    try:
        temps = eng.state_points()[1]
    except EngineError as err:
        assert "created without has_mu" in str(err) or "only the lean kernel families take them" in str(err)
        return
    assert np.all(temps == T)


def _check_step(m, before, res, words, T_old, T_new, P):
    """the step from T_old to T_new against the definition, as tests/test_gpu_pop_anneal.py holds the fixed step"""
    R = len(before["enthalpy"])
    n = R // P
    b0, b1 = 1.0 / (kB * T_old), 1.0 / (kB * T_new)
    for p in range(P):
        sl = slice(p * n, (p + 1) * n)
        q_np, _, href_np = PA.weights(before["enthalpy"][sl], b0, b1)
        assert res["href"][p] == href_np
        assert int(res["qsum"][p]) == sum(int(x) for x in res["q"][sl])
        dq = res["q"][sl].astype(np.int64) - q_np.astype(np.int64)
        assert np.abs(dq).max() <= 1
        assert res["q"][sl].max() == 2 ** 40
        assert np.array_equal(res["parent"][sl], p * n + PA.parent_map(res["q"][sl], words[p]))


# ---- 1. the device chooses the temperature of the definition --------------------------------------------------------
@pytest.mark.parametrize("R,P", SHAPES, ids=[f"R{r}-P{p}" for r, p in SHAPES])
@pytest.mark.parametrize("name", NAMES)
def test_device_chooses_the_step_of_the_definition(name, R, P, monkeypatch):
    m, eng = _start(name, R, monkeypatch)
    n = R // P
    info, before = eng.kernel_info(), _state(eng, m)
    beta = 1.0 / (kB * m.T)
    limit = m.T / 3
    T_np, reached_np, forced_np, margin = PA.next_temperature(before["enthalpy"].reshape(P, n), beta, limit, TARGET, N_ITER)
    print(f"{name} R={R} P={P}: T {m.T} -> {T_np} (limit {limit}), smallest margin {margin:.3e}, required {4 * n * n}")
    assert margin >= 4 * n * n  # the condition of the case (module docstring)
    words = PA([m.T], populations=P, seed=3).offset_words(0)
    res = eng.anneal_adaptive(limit, OVERLAP, words, npop=P, n_iter=N_ITER)
    assert (res["temperature"], res["reached"], res["forced"]) == (T_np, reached_np, forced_np)
    assert reached_np == (n == 1) and not forced_np
    _check_step(m, before, res, words, m.T, T_np, P)
    if n > 1:
        cnt = np.concatenate([PA.children(res["q"][p * n:(p + 1) * n], words[p]) for p in range(P)])
        assert (cnt == 0).sum() >= 1 and (cnt >= 2).sum() >= 1  # (on the definition alone: the step does something)
        for p in range(P):  # the step keeps the target, and wastes little of it (16 halvings of a factor 3)
            assert OVERLAP - 1e-6 <= PA.overlap(res["q"][p * n:(p + 1) * n])
        assert min(PA.overlap(res["q"][p * n:(p + 1) * n]) for p in range(P)) < OVERLAP + 0.01
    after = _state(eng, m)
    _assert_rows(after, before, res["parent"], m.bias)
    assert eng.kernel_info() == info
    _assert_named(eng, T_np)
    # the new temperature is in force: a fixed step to it has db = 0 and is the identity
    again = eng.anneal_resample(np.full(P, T_np), words, npop=P)
    assert np.all(again["q"] == 2 ** 40) and np.array_equal(again["parent"], np.arange(R))
    eng.close()


# ---- 2. the branches ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lean-ewald-field", "table-flip"])
def test_reached_step_lands_on_the_limit(name, monkeypatch):
    R, P = 130, 2
    m, eng = _start(name, R, monkeypatch)
    before = _state(eng, m)
    limit = m.T * 0.99
    words = PA([m.T], populations=P, seed=5).offset_words(0)
    assert PA.next_temperature(before["enthalpy"].reshape(P, -1), 1.0 / (kB * m.T), limit, TARGET, N_ITER)[:3] == (limit, True, False)
    res = eng.anneal_adaptive(limit, OVERLAP, words, npop=P)
    assert (res["temperature"], res["reached"], res["forced"]) == (limit, True, False)
    _check_step(m, before, res, words, m.T, limit, P)
    after = _state(eng, m)
    _assert_rows(after, before, res["parent"], m.bias)
    _assert_named(eng, limit)
    # at the limit: db = 0, every weight is 1, the map is the identity and nothing moves
    again = eng.anneal_adaptive(limit, OVERLAP, PA([m.T], populations=P, seed=5).offset_words(1), npop=P)
    assert (again["temperature"], again["reached"], again["forced"]) == (limit, True, False)
    assert np.all(again["q"] == 2 ** 40) and np.all(again["qsum"] == (R // P) * 2 ** 40)
    assert np.array_equal(again["parent"], np.arange(R))
    same = _state(eng, m)
    for k in after:
        assert np.array_equal(same[k], after[k]), k
    eng.close()


def test_forced_step(monkeypatch):
    """One halving towards a limit far away: the midpoint misses the target too, lo stays 0 and the step is hi."""
    R, P = 130, 1
    m, eng = _start("lean", R, monkeypatch)
    before = _state(eng, m)
    limit = m.T / 1000
    beta = 1.0 / (kB * m.T)
    T_np, reached_np, forced_np, margin = PA.next_temperature(before["enthalpy"].reshape(P, -1), beta, limit, TARGET, 1)
    assert forced_np and not reached_np and margin >= 4 * R * R
    assert T_np == 1.0 / (kB * (beta + 0.5 * (1.0 / (kB * limit) - beta)))
    words = PA([m.T], populations=P, seed=6).offset_words(0)
    res = eng.anneal_adaptive(limit, OVERLAP, words, npop=P, n_iter=1)
    assert (res["temperature"], res["reached"], res["forced"]) == (T_np, False, True)
    _check_step(m, before, res, words, m.T, T_np, P)
    assert PA.overlap(res["q"]) < OVERLAP
    _assert_rows(_state(eng, m), before, res["parent"], m.bias)
    _assert_named(eng, T_np)
    eng.close()


@pytest.mark.parametrize("name", ["lean", "square-charge-bias"])
def test_heating_step(name, monkeypatch):
    R, P = 40, 2
    m, eng = _start(name, R, monkeypatch)
    before = _state(eng, m)
    limit = m.T * 3
    T_np, reached_np, forced_np, margin = PA.next_temperature(before["enthalpy"].reshape(P, -1), 1.0 / (kB * m.T), limit, TARGET, N_ITER)
    print(f"{name}: heating {m.T} -> {T_np}, smallest margin {margin:.3e}")
    assert m.T < T_np < limit and not reached_np and not forced_np and margin >= 4 * (R // P) ** 2
    words = PA([m.T], populations=P, seed=7).offset_words(0)
    res = eng.anneal_adaptive(limit, OVERLAP, words, npop=P)
    assert (res["temperature"], res["reached"], res["forced"]) == (T_np, False, False)
    _check_step(m, before, res, words, m.T, T_np, P)
    for p in range(P):  # heating: the reference is the largest enthalpy of the population
        assert res["href"][p] == before["enthalpy"][p * 20:(p + 1) * 20].max()
    _assert_rows(_state(eng, m), before, res["parent"], m.bias)
    eng.close()


# ---- 3. the refusals ------------------------------------------------------------------------------------------------
def _refused(match):
    return pytest.raises((ValueError, EngineError), match=match)


def test_refusals(monkeypatch):
    R = 8
    m, eng = _start("lean", R, monkeypatch, steps=0)
    before = eng.get_state()
    words = np.zeros(8, dtype=np.uint64)
    # the new ones
    with _refused("overlap target must be positive"):
        eng.anneal_adaptive(500.0, 1e-12, words[:1])  # (the word of 1e-12 is 0)
    with pytest.raises(ValueError, match="target overlap must lie in"):
        eng.anneal_adaptive(500.0, 1.0, words[:1])
    with pytest.raises(ValueError, match="target overlap must lie in"):
        eng.anneal_adaptive(500.0, -0.5, words[:1])
    for bad in (0, 61, -3):
        with _refused("n_iter must lie in 1 .. 60"):
            eng.anneal_adaptive(500.0, 0.85, words[:1], n_iter=bad)
    for bad in (0.0, -300.0, np.inf, np.nan):
        with _refused("limit must be positive and finite"):
            eng.anneal_adaptive(bad, 0.85, words[:1])
    eng.set_temperature(np.array([m.T] * 4 + [m.T * 1.5] * 4))
    with _refused("populations are at different temperatures"):
        eng.anneal_adaptive(500.0, 0.85, words[:2], npop=2)  # (each population at one temperature: a fixed step is taken)
    # the old ones, through the new entry
    with _refused("do not divide"):
        eng.anneal_adaptive(500.0, 0.85, words[:3], npop=3)
    with pytest.raises(ValueError, match="one offset word per population"):
        eng.anneal_adaptive(500.0, 0.85, words[:1], npop=2)
    eng.set_temperature(np.array([m.T] * 6 + [m.T * 1.5] * 2))
    with _refused("population 1 are at different temperatures"):
        eng.anneal_adaptive(500.0, 0.85, words[:2], npop=2)
    eng.set_temperature(np.full(R, m.T))
    after = eng.get_state()
    for k in ("occupancy", "enthalpy", "n_steps", "n_accepted"):  # no refused call moved anything
        assert np.array_equal(after[k], before[k])
    case = CASES["fcc_conv444_pairs-int"]()
    eng.set_walker_mu(np.repeat(case.rows[:1], R, axis=0))  # (prices the chemical work anew: the enthalpies' last bits)
    with _refused("per-walker chemical potentials"):
        eng.anneal_adaptive(500.0, 0.85, words[:1])
    eng.set_walker_mu(None)
    after = eng.get_state()
    for k in ("occupancy", "n_steps", "n_accepted"):
        assert np.array_equal(after[k], before[k])
    _assert_named(eng, m.T)
    res = eng.anneal_adaptive(m.T / 2, 0.85, words[:2], npop=2)
    assert m.T / 2 <= res["temperature"] < m.T
    eng.close()
    # Wang-Landau handles, with and without per-walker windows
    c = wc.case()
    wx = wc.windows(5)
    wl = Engine(c["tab"], wc.config(wx.R, wx.vmin[0], wx.vmax[0]))
    for _ in range(2):
        with _refused("Wang-Landau"):
            wl.anneal_adaptive(500.0, 0.85, words[:1])
        wl.set_wl_windows(wx.vmin, wx.vmax)
    wl.close()
    # distance handles
    from smol_amd import capi
    from smol_amd import sqs as sqs_mod
    from tests.test_gpu_sqs import setup

    mm, sc, tab, spec0, cfg = setup("binary444", capi.FEATURES_CORRELATIONS, capi.STEP_SWAP, 4)
    spec = sqs_mod.distance_spec(mm, capi.FEATURES_CORRELATIONS, np.zeros(spec0.struct.n_features), None, 1.0, 1e-5, 1.0)
    dist = Engine(tab, cfg, distance=spec)
    with _refused("distance handle"):
        dist.anneal_adaptive(500.0, 0.85, words[:1])
    dist.close()


# ---- 4. clones continue as fresh oracles ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lean-ewald-field", "square-charge-bias"])
def test_clones_continue_as_fresh_oracles(name, monkeypatch):
    from oracle import oracle as orc

    R, P = 40, 2
    m, eng = _start(name, R, monkeypatch, steps=0)
    _, seeds = m.starts(R)
    pa = PA.adaptive(m.T, m.T / 3, OVERLAP, populations=P, seed=4)
    clones = 0
    for k in range(2):
        eng.run(200)
        res = eng.anneal_adaptive(pa.t_end, OVERLAP, pa.offset_words(k), npop=P)
        pa.append(res["temperature"], res["reached"], res["forced"])
        clones += int((res["parent"] != np.arange(R)).sum())
    assert clones >= 1 and m.T > pa.temperatures[1] > pa.temperatures[2] > m.T / 3
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


# ---- 5. statistics on the device ------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", pc.SEEDS)
def test_device_adaptive_annealing_against_enumeration(seed):
    """The scheme of tests/test_pop_anneal_adaptive_host.py through the device path; the bounds were measured on the
    oracle."""
    eng = Engine(wc.case()["tab"], pc.config(pc.WALKERS * pc.POPULATIONS))
    history = []
    pa, emean = ac.run_annealing(eng, seed, host_decide=False, history=history)
    dl, de = pa.log_partition_ratio() - pc.LNZ_EXACT, emean - pc.EMEAN_EXACT
    print(f"seed {seed}: {pa.n_steps} steps", np.round(pa.temperatures, 1))
    print("   sum ln Q - exact", np.round(dl, 4), " final mean enthalpy - exact", np.round(de, 5))
    print(f"   combined: {pa.combined_log_partition_ratio() - pc.LNZ_EXACT:+.4f} {pa.combine(emean) - pc.EMEAN_EXACT:+.5f}"
          f"   smallest overlap per step {np.round(pa.overlaps.min(axis=1), 4)}")
    assert pa.done and pa.temperatures[0] == ac.T_START and pa.temperatures[-1] == ac.T_END
    assert np.all(np.diff(pa.temperatures) < 0) and pa.n_steps < ac.FIXED_STEPS and not any(pa.forced)
    assert pa.log_q.shape == (pa.n_steps, pc.POPULATIONS) and len(history) == pa.n_steps
    _assert_named(eng, ac.T_END)
    assert np.all(pa.overlaps >= ac.OVERLAP - 1e-6)
    assert np.all(np.abs(dl) <= ac.LNZ_BOUND), dl
    assert np.all(np.abs(de) <= ac.EMEAN_BOUND), de
    assert abs(pa.combined_log_partition_ratio() - pc.LNZ_EXACT) <= ac.LNZ_BOUND
    assert abs(pa.combine(emean) - pc.EMEAN_EXACT) <= ac.EMEAN_BOUND
    eng.close()


# ---- 6. Sampler.anneal_population(overlap=) -------------------------------------------------------------------------
def test_sampler_anneal_population_adaptive(tmp_path):
    from tests.cases import load_case

    c = load_case("fcc_conv444_pairs")
    sc = c["sc"]
    ens = moca.Ensemble.from_cluster_expansion(sc, c["coefs"])
    nw, P = 24, 2
    occ = (np.random.default_rng(4).random((nw, sc.num_sites)) < 0.5).astype(np.int32)

    def sampler():
        return moca.Sampler.from_ensemble(ens, temperature=3000.0, step_type="flip", nwalkers=nw, seeds=list(range(nw)))

    ref = sampler()
    ref.anneal([3000.0], 400, occ, thin_by=100)
    s = sampler()
    with pytest.raises(ValueError, match="names the two ends"):
        s.anneal_population([3000.0, 2000.0, 1000.0], 400, occ, populations=P, overlap=0.85)
    with pytest.raises(ValueError, match="End temperature is greater"):
        s.anneal_population([1000.0, 3000.0], 400, occ, populations=P, overlap=0.85)
    pa = s.anneal_population((3000.0, 1000.0), 400, occ, populations=P, thin_by=100, seed=2, overlap=0.85)
    a = s.samples
    meta = a.metadata["population_annealing"]
    temps = meta["temperatures"]
    K = len(temps)
    print("chosen temperatures", np.round(temps, 1), " overlaps", np.round(meta["overlap"], 4).tolist())
    assert pa.done and 3 <= K == pa.n_steps + 1 and temps[0] == 3000.0 and temps[-1] == 1000.0 and np.all(np.diff(temps) < 0)
    assert temps == list(pa.temperatures) and a.num_samples == 4 * K
    np.testing.assert_array_equal(a.get_trace_value("temperature", flat=False)[:, 0, 0], np.repeat(temps, 4))
    # the first temperature is plain sampling: the same chains as anneal
    np.testing.assert_array_equal(a.get_trace_value("occupancy", flat=False)[:4], ref.samples.get_trace_value("occupancy", flat=False))
    assert pa.log_q.shape == (K - 1, P)
    np.testing.assert_array_equal(meta["log_partition_ratio"], np.vstack([np.zeros((1, P)), np.cumsum(pa.log_q, axis=0)]))
    assert np.array_equal(meta["n_families"][1:], pa.n_families) and np.array_equal(meta["rho_t"][1:], pa.rho_t)
    ovl = np.asarray(meta["overlap"])
    assert ovl.shape == (K - 1, 1 + P) and np.all(ovl[:, 0] == 0.85) and np.array_equal(ovl[:, 1:], pa.overlaps)
    assert np.all(ovl[:, 1:] >= 0.85 - 1e-6) and not any(pa.forced)
    path = str(tmp_path / "samples.npz")
    a.to_npz(path)
    back = moca.SampleContainer.from_npz(path, ens)
    assert back.metadata["population_annealing"] == meta and back.num_samples == 4 * K
