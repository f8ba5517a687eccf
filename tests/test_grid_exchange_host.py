"""Replica exchange across a mu-T grid, host side (parallel.GridExchange): the pair lists of the four moves, and the
move itself -- `decide`, the NumPy definition the device kernel is tested against (tests/test_gpu_grid_exchange.py) --
by brute force against the CPU oracle: one-walker oracles built with row s give H_s(x) for every state point s and
every configuration x, and the acceptance exponent of swapping the points of walker a (at s) and walker b (at t) is

    -beta_s [H_s(x_b) - H_s(x_a)] - beta_t [H_t(x_a) - H_t(x_b)].
"""

import numpy as np
import pytest

from smol_amd import parallel
from smol_amd.engine import species_counts
from tests.test_gpu_walker_mu import ATOL, CASES, RTOL

kB = parallel.kB


# ---- pair lists ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nT,nMu,replicas", [(2, 7, 1), (2, 3, 2), (1, 4, 3), (5, 1, 2), (3, 4, 1), (4, 5, 3), (1, 1, 2)])
def test_pair_lists(nT, nMu, replicas):
    gx = parallel.GridExchange(np.linspace(1000.0, 2000.0, nT), np.zeros((nMu, 1, 2)), replicas=replicas)
    assert gx.npoints == replicas * nT * nMu and len(gx.MOVES) == 4
    per_set = nT * nMu
    root = list(range(gx.npoints))

    def find(x):
        while root[x] != x:
            x = root[x]
        return x

    for move in gx.MOVES:
        pairs = gx.pairs(move)
        assert pairs.dtype == np.int32 and pairs.shape == (len(pairs), 2)
        assert len(np.unique(pairs)) == pairs.size  # every point in at most one pair of a move
        for s, t in pairs:
            assert s // per_set == t // per_set  # no pair crosses replica sets
            i_s, j_s, i_t, j_t = (s % per_set) // nMu, s % nMu, (t % per_set) // nMu, t % nMu
            assert (i_t - i_s, j_t - j_s) == ((1, 0) if move[0] == "T" else (0, 1))  # neighbours along the move's axis
            assert (i_s if move[0] == "T" else j_s) % 2 == move[1]
            root[find(s)] = find(t)
    # the four moves together connect each replica set (and nothing else)
    comps = {find(p) for p in range(gx.npoints)}
    assert len(comps) == replicas
    for rep in range(replicas):
        assert len({find(p) for p in range(rep * per_set, (rep + 1) * per_set)}) == 1
    # layout: p = (rep * nT + i) * nMu + j
    p = gx.npoints - 1
    assert gx.point_temperatures[p] == gx.temperatures[nT - 1] and np.array_equal(gx.point_rows[p], gx.rows[nMu - 1])
    assert gx.point_temperatures[nMu - 1] == gx.temperatures[0]


def test_log_u_is_a_function_of_seed_and_attempt():
    a, b = parallel.GridExchange([1.0, 2.0], np.zeros((2, 1, 2)), seed=5), parallel.GridExchange([1.0, 2.0], np.zeros((2, 1, 2)), seed=5)
    assert np.array_equal(a.log_u(3, 4), b.log_u(3, 4)) and not np.array_equal(a.log_u(3, 4), a.log_u(4, 4))
    assert np.array_equal(a.log_u(3, 4), np.log(parallel._philox_uniforms(5, 3, 4)))
    assert len(a.log_u(0, 0)) == 0


# ---- the formula, by brute force ------------------------------------------------------------------------------------
class Brute:
    """2 T x 3 rows of one case, random occupancies, walkers at a shuffled assignment; H[j][x] from the oracle"""

    def __init__(self, name):
        from oracle import oracle as orc

        case = CASES[name]()
        self.rows = case.rows[[0, len(case.rows) // 2, len(case.rows) - 1]]
        self.gx = parallel.GridExchange(case.T * np.array([1.0, 1.2]), self.rows, seed=11)
        R = self.gx.npoints
        rng = np.random.default_rng(17)
        self.occ = case.starts(rng, R, same=False)
        self.point_of = rng.permutation(R)
        self.H = np.empty((len(self.rows), R))  # H[j][x]: enthalpy of configuration x at row j
        for j, row in enumerate(self.rows):
            ora = orc.OracleMC(case.engine_tables(row), case.config(1))
            for x in range(R):
                ora.set_state(self.occ[x:x + 1], np.array([1], dtype=np.uint64), np.array([case.T]))
                self.H[j, x] = ora.get_state()["enthalpy"][0]
        tab = case.engine_tables()
        self.counts = species_counts(tab, self.occ, self.rows.shape[-1])
        self.R = R

    def H_at(self, point, x):
        return self.H[point % self.gx.nMu, x]


@pytest.fixture(scope="module", params=["fcc_conv444_pairs-int", "rocksalt333_two_sublattices-int"])
def brute(request):
    return Brute(request.param)


def test_exponent_is_the_brute_force_one(brute):
    gx, R = brute.gx, brute.R
    beta = 1.0 / (kB * gx.point_temperatures)
    enthalpy = np.array([brute.H_at(brute.point_of[w], w) for w in range(R)])
    walker_at = np.argsort(brute.point_of)
    seen = 0
    for move in gx.MOVES:
        res = gx.decide(enthalpy, brute.counts, brute.point_of, move, 0, record=False)
        want = []
        for s, t in gx.pairs(move):
            a, b = walker_at[s], walker_at[t]
            want.append(-beta[s] * (brute.H_at(s, b) - brute.H_at(s, a)) - beta[t] * (brute.H_at(t, a) - brute.H_at(t, b)))
        np.testing.assert_allclose(res["exponent"], np.array(want, dtype=np.float64).reshape(-1), rtol=RTOL, atol=ATOL)
        lu = gx.log_u(0, len(want))
        assert np.array_equal(res["accept"], (np.array(want).reshape(-1) >= 0) | (lu < np.array(want).reshape(-1)))
        seen += len(want)
    assert seen == 3 + 0 + 2 + 2  # ("T", 0): 3 pairs, ("T", 1): none on two temperatures, ("mu", 0 / 1): 2 each
    assert gx.acceptance == 0.0 and all(a.sum() == 0 for a in gx.attempted.values())  # (record=False)


def test_repriced_enthalpies_are_the_oracles(brute):
    gx, R = brute.gx, brute.R
    enthalpy = np.array([brute.H_at(brute.point_of[w], w) for w in range(R)])
    for move in gx.MOVES:
        n = len(gx.pairs(move))
        res = gx.decide(enthalpy, brute.counts, brute.point_of, move, 0, log_u=np.full(n, -np.inf), record=False)
        assert res["accept"].all()
        new = res["point_of"]
        want = np.array([brute.H_at(new[w], w) for w in range(R)])  # a -> H_t(x_a), b -> H_s(x_b), the others as before
        np.testing.assert_allclose(res["enthalpy"], want, rtol=RTOL, atol=ATOL)
        moved = new != brute.point_of
        assert moved.sum() == 2 * n and np.array_equal(res["enthalpy"][~moved], enthalpy[~moved])
        assert sorted(new) == list(range(R))
        # the chemical work gains what the enthalpy loses
        np.testing.assert_array_equal(res["enthalpy"], enthalpy - res["work_delta"])


def test_equal_rows_take_the_decisions_of_the_temperature_ladder():
    n, seed = 9, 23
    ladder = parallel.geometric_ladder(400.0, 2000.0, n)
    rng = np.random.default_rng(4)
    gx = parallel.GridExchange(ladder, rng.normal(size=(1, 2, 3)), seed=seed)
    rex = parallel.ReplicaExchange(ladder, per_rank=n, seed=seed)
    counts = rng.integers(0, 50, size=(n, 2, 3))
    point_of = np.arange(n)
    flips = 0
    for call in range(12):
        enthalpy = rng.normal(scale=0.3, size=n)
        before = rex.rung_of.copy()
        won = rex.decide(enthalpy)
        res = gx.decide(enthalpy, counts, point_of, ("T", call & 1), call)
        pairs = gx.pairs(("T", call & 1))
        assert [tuple(p) for p in pairs[res["accept"]]] == won
        assert np.array_equal(res["work_delta"], np.zeros(n)) and np.array_equal(res["enthalpy"], enthalpy)
        point_of = res["point_of"]
        assert np.array_equal(point_of, rex.rung_of)
        flips += int((before != rex.rung_of).sum())
    assert 0 < flips
    assert np.array_equal(gx.attempted[("T", 0)] + 0, rex.attempted[0::2]) and np.array_equal(gx.accepted[("T", 1)], rex.accepted[1::2])


# ---- Sampler / container, as far as they go without a GPU -------------------------------------------------------------
def _ensemble():
    from smol_amd import moca, synth

    model = synth.build_cluster_model(synth.rocksalt_prim(), {2: 3.5})
    sc = synth.build_supercell(model, [2, 2, 2])
    ens = moca.Ensemble.from_cluster_expansion(sc, synth.random_coefs(model, seed=5, scale=0.05))
    ens.chemical_potentials = dict(zip(ens.species, [0.1, -0.2, 0.05]))
    return ens


def test_a_sharded_sampler_refuses_run_exchange():
    from smol_amd import moca

    ens = _ensemble()
    mus = [dict(zip(ens.species, [0.1, -0.2 + d, 0.05])) for d in (-0.1, 0.1)]
    assert ens.walker_mu_dicts(ens.walker_mu_rows(mus)) == mus
    sampler = moca.Sampler.from_ensemble(ens, temperature=3000.0, nwalkers=4, seeds=[1, 2, 3, 4], rank=1, world_size=2)
    with pytest.raises(ValueError, match="sharded over several ranks"):
        sampler.run_exchange(1, 10, grid=dict(temperatures=[3000.0, 3600.0], chemical_potentials=mus))


def test_by_state_point_regroups_and_survives_npz(tmp_path):
    from smol_amd import moca

    ens = _ensemble()
    nw, ns = 4, 5
    sampler = moca.Sampler.from_ensemble(ens, temperature=3000.0, nwalkers=nw, seeds=[1, 2, 3, 4], rank=0, world_size=1)
    c = sampler.samples
    with pytest.raises(ValueError, match="no state_point trace"):
        c.by_state_point("enthalpy")
    before = dict(c._schema)
    rng = np.random.default_rng(0)
    point = np.array([rng.permutation(nw) for _ in range(ns)], dtype=np.int32)
    c._schema["state_point"] = (np.dtype(np.int32), (nw, 1))
    block = {k: np.zeros((ns,) + shape, dtype=dt) for k, (dt, shape) in before.items()}
    block["enthalpy"] = rng.normal(size=(ns, nw, 1))
    block["state_point"] = point[:, :, None]
    c.append_block(block, 10)
    c.metadata["state_points"] = dict(species=list(ens.species), temperatures=[3000.0, 3600.0],
                                      chemical_potentials=[[0.1, -0.3, 0.05], [0.1, -0.1, 0.05]], shape=[1, 2, 2])
    by = c.by_state_point("enthalpy", discard=1)
    assert by.shape == (nw, ns - 1, 1)
    for i in range(1, ns):
        for w in range(nw):
            assert by[point[i, w], i - 1, 0] == block["enthalpy"][i, w, 0]
    path = str(tmp_path / "c.npz")
    c.to_npz(path)
    back = moca.SampleContainer.from_npz(path, ens)
    assert back.metadata["state_points"] == c.metadata["state_points"]
    assert np.array_equal(back.by_state_point("enthalpy"), c.by_state_point("enthalpy"))
    assert back.get_trace_value("state_point", flat=False).dtype == np.int32
    # a plain block appended to the restored container: the walkers stay where the last sample left them
    plain = {k: np.zeros((2,) + shape, dtype=dt) for k, (dt, shape) in before.items()}
    back.append_block(plain, 10)
    got = back.get_trace_value("state_point", flat=False)
    assert got.shape == (ns + 2, nw, 1) and np.array_equal(got[ns:, :, 0], np.repeat(point[-1][None], 2, axis=0))
    c._state_point_now = point[0][:, None]  # (what run_exchange keeps: the assignment after its last attempt)
    c.append_block(plain, 10)
    assert np.array_equal(c.get_trace_value("state_point", flat=False)[ns:, :, 0], np.repeat(point[0][None], 2, axis=0))
    empty = moca.Sampler.from_ensemble(ens, temperature=3000.0, nwalkers=nw, seeds=[1, 2, 3, 4], rank=0, world_size=1).samples
    empty._schema["state_point"] = (np.dtype(np.int32), (nw, 1))
    with pytest.raises(ValueError, match="holds no sample yet"):
        empty.append_block(plain, 10)
