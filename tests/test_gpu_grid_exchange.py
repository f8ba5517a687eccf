"""Replica exchange across a mu-T grid, decided and applied on the device (smolmc_exchange_grid).

The move is defined by parallel.GridExchange.decide (pinned against the CPU oracle in tests/test_grid_exchange_host.py):
the kernel takes its decisions bit for bit, swaps temperature and row of the two walkers and re-prices chemical work and
enthalpy; occupancies, counters and the other features never move.  The grids are the cases of
tests/test_gpu_walker_mu.py: temperatures case.T x {1, 1.2} crossed with the case's rows (R <= 14); walker w starts at
state point w = i * nMu + j."""

import numpy as np
import pytest

from smol_amd import capi, parallel
from tests.cases import tables_for
from tests.test_gpu_walker_mu import ATOL, CASES, MODES, RTOL, OracleGrid, _assert_same

pytestmark = pytest.mark.gpu

NAMES = ["fcc_prim666_triplets-corr", "rocksalt444_ewald-int", "rocksalt333_two_sublattices-int",
         "rocksalt333_two_sublattices-corr", "table_flip_one_sublattice"]


def _errors():
    """(the binding raises argument problems as ValueError, the others as EngineError)"""
    from smol_amd.engine import EngineError

    return (EngineError, ValueError)


def _grid(case, seed=1):
    return parallel.GridExchange(case.T * np.array([1.0, 1.2]), case.rows, seed=seed)


# (tests/test_gpu_walker_mu.py's _start makes case.R walkers; the grids here hold 2 x case.R and more, so this one takes
# the number -- the same draws and seeds otherwise)
def _start(case, R, seed=5):
    rng = np.random.default_rng(seed)
    occ = case.starts(rng, R, same=False)
    seeds = np.arange(100, 100 + R, dtype=np.uint64) * np.uint64(7919)
    return occ, seeds


def _engine(case, gx, row=None, rows=True):
    """an engine of gx.npoints walkers, walker w at state point w"""
    from smol_amd.engine import Engine

    eng = Engine(case.engine_tables(row), case.config(gx.npoints))
    if rows:
        eng.set_walker_mu(gx.point_rows)
    occ, seeds = _start(case, gx.npoints)
    eng.set_state(occ, seeds, gx.point_temperatures)
    return eng, seeds


def _check_priced(eng, gx, point_of, st):
    """temperatures and rows are the permuted grid, exactly; chemical work and enthalpy are priced at them"""
    po, temps = eng.state_points()
    assert np.array_equal(po, point_of)
    assert np.array_equal(temps, gx.point_temperatures[point_of])
    assert np.array_equal(eng.get_walker_mu(), gx.point_rows[point_of])
    np.testing.assert_allclose(st["features"][:, -1], eng.chemical_work(st["occupancy"], gx.point_rows[point_of]), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(st["enthalpy"], st["features"] @ eng.natural_parameters, rtol=RTOL, atol=ATOL)


# ---- 1. device = host -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_device_takes_the_decisions_of_decide(name):
    case = CASES[name]()
    gx = _grid(case)
    eng, _ = _engine(case, gx)
    assert eng.kernel_info().startswith(case.family + " ")
    eng.run(300)
    info = eng.kernel_info()
    point_of = np.arange(gx.npoints)
    flags = []
    for attempt, move in enumerate(gx.MOVES):
        before = eng.get_state()
        res = gx.decide(before["enthalpy"], eng.species_counts(before["occupancy"]), point_of, move, attempt)
        pairs = gx.pairs(move)
        stats = np.zeros((len(pairs), 2), dtype=np.int64)
        eng.exchange_grid(pairs, gx.log_u(attempt, len(pairs)), stats)
        print(name, move, "exponents", np.round(res["exponent"], 3), "accepted", stats[:, 1])
        assert np.array_equal(stats[:, 0], np.ones(len(pairs), dtype=np.int64))
        assert np.array_equal(stats[:, 1].astype(bool), res["accept"])
        point_of = res["point_of"]
        st = eng.get_state()
        _check_priced(eng, gx, point_of, st)
        np.testing.assert_allclose(st["enthalpy"], res["enthalpy"], rtol=RTOL, atol=ATOL)
        assert np.array_equal(st["features"][:, :-1], before["features"][:, :-1])
        for key in ("occupancy", "n_steps", "n_accepted", "accepted"):
            assert np.array_equal(st[key], before[key]), key
        flags.append(res["accept"])
    flags = np.concatenate(flags)
    assert flags.any() and not flags.all(), flags  # (on `decide` alone: the case exercises both outcomes)
    assert eng.kernel_info() == info  # mu_max and the float32 accept bound: a permutation leaves them alone
    eng.close()


# ---- 2. the chains continue at their new points ----------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_chains_continue_as_fresh_oracles_of_the_new_points(name):
    case = CASES[name]()
    gx = _grid(case, seed=2)
    eng, seeds = _engine(case, gx)
    moved = 0
    for attempt in range(3):
        eng.run(200)
        move = gx.MOVES[(0, 2, 3)[attempt]]
        pairs = gx.pairs(move)
        stats = np.zeros((len(pairs), 2), dtype=np.int64)
        eng.exchange_grid(pairs, gx.log_u(attempt, len(pairs)), stats)
        moved += int(stats[:, 1].sum())
    assert moved > 0
    st = eng.get_state()
    point_of, temps = eng.state_points()
    rows = eng.get_walker_mu()
    assert np.array_equal(rows, gx.point_rows[point_of]) and not np.array_equal(point_of, np.arange(gx.npoints))
    ora = OracleGrid(case, rows)
    ora.set_state(st["occupancy"], seeds, temps)
    ora.set_counters(st["n_steps"], st["n_accepted"])
    eng.run(200)
    ora.run(200)
    _assert_same(eng.get_state(), ora.get_state())
    eng.close()


# ---- 3. forced cases -------------------------------------------------------------------------------------------------------
def test_forced_decisions():
    case = CASES["rocksalt333_two_sublattices-int"]()
    gx = _grid(case)
    eng, _ = _engine(case, gx)
    eng.run(300)
    st = eng.get_state()
    counts = eng.species_counts(st["occupancy"])
    point_of = np.arange(gx.npoints)
    # log u = 0: exactly the pairs whose exponent is >= 0
    move = ("T", 0)
    n = len(gx.pairs(move))
    res = gx.decide(st["enthalpy"], counts, point_of, move, 0, log_u=np.zeros(n), record=False)
    assert np.array_equal(res["accept"], res["exponent"] >= 0) and res["accept"].any() and not res["accept"].all()
    stats = np.zeros((n, 2), dtype=np.int64)
    eng.exchange_grid(gx.pairs(move), np.zeros(n), stats)
    assert np.array_equal(stats[:, 1].astype(bool), res["exponent"] >= 0)
    point_of = res["point_of"]
    assert np.array_equal(eng.state_points()[0], point_of)
    # log u = -inf: every pair, and the attempts add up in `stats`
    move = ("mu", 1)
    n = len(gx.pairs(move))
    stats = np.zeros((n, 2), dtype=np.int64)
    for _ in range(2):  # (twice: everybody is back)
        eng.exchange_grid(gx.pairs(move), np.full(n, -np.inf), stats)
    assert np.array_equal(stats, np.full((n, 2), 2))
    assert np.array_equal(eng.state_points()[0], point_of)
    _check_priced(eng, gx, point_of, eng.get_state())
    # no stats: nothing comes back, the move is made all the same
    eng.exchange_grid(gx.pairs(move), np.full(n, -np.inf))
    walker_at = np.argsort(point_of)
    swapped = point_of.copy()
    for s, t in gx.pairs(move):
        swapped[walker_at[s]], swapped[walker_at[t]] = t, s
    assert np.array_equal(eng.state_points()[0], swapped)
    _check_priced(eng, gx, swapped, eng.get_state())
    # an empty pair list is no move
    eng.exchange_grid(np.zeros((0, 2), dtype=np.int32), np.zeros(0))
    assert np.array_equal(eng.state_points()[0], swapped)
    eng.close()


def test_identical_points_accept_and_change_no_value():
    case = CASES["rocksalt333_two_sublattices-int"]()
    R = 6
    from smol_amd.engine import Engine

    eng = Engine(case.engine_tables(), case.config(R))
    rows = np.repeat(case.rows[1:2], R, axis=0)
    eng.set_walker_mu(rows)
    occ, seeds = _start(case, R)
    eng.set_state(occ, seeds, case.T)
    eng.run(300)
    before = eng.get_state()
    pairs = np.array([[0, 1], [2, 3], [4, 5]], dtype=np.int32)
    stats = np.zeros((3, 2), dtype=np.int64)
    eng.exchange_grid(pairs, np.zeros(3), stats)  # exponent 0: accepted even at log u = 0
    assert np.array_equal(stats, np.ones((3, 2), dtype=np.int64))
    point_of, temps = eng.state_points()
    assert np.array_equal(point_of, [1, 0, 3, 2, 5, 4]) and np.array_equal(temps, np.full(R, case.T))
    after = eng.get_state()
    for key in before:
        assert np.array_equal(after[key], before[key]), key
    assert np.array_equal(eng.get_walker_mu(), rows)
    eng.close()


# ---- 4. equal rows: the temperature exchange of smolmc_exchange_dev ------------------------------------------------
def test_equal_rows_decide_like_exchange_dev():
    import torch

    from smol_amd.engine import Engine

    case = CASES["fcc_prim666_triplets-corr"]()
    R, row, seed = 8, case.rows[2], 9
    ladder = np.linspace(0.7, 1.3, R) * case.T
    occ, seeds = _start(case, R)
    plain, grid = Engine(case.engine_tables(row), case.config(R)), Engine(case.engine_tables(row), case.config(R))
    for e in (plain, grid):
        e.set_state(occ, seeds, ladder)
    rex = parallel.ReplicaExchange(ladder, per_rank=R, seed=seed)
    gx = parallel.GridExchange(ladder, row[None], seed=seed)
    buf = torch.empty(R, dtype=torch.float64, device="cuda")
    accepted = 0
    for call in range(6):
        if call == 3:  # from here on with rows set, all equal: the same move
            grid.set_walker_mu(np.repeat(row[None], R, axis=0))
            base = grid.state_points()[0]
            assert np.array_equal(base, np.arange(R))  # (the call names the points anew)
            base = rex.rung_of.copy()
        for e in (plain, grid):
            e.run(150)
        plain.export_enthalpy(buf.data_ptr())
        plain.sync()
        rex.decide_on_device(plain, buf)
        # rung k is the grid's point k until the points are named anew at call 3, then point q is rung base[q]
        rungs = gx.pairs(("T", call & 1))
        pairs = rungs if call < 3 else np.argsort(base)[rungs]
        stats = np.zeros((len(pairs), 2), dtype=np.int64)
        grid.exchange_grid(pairs, gx.log_u(call, len(pairs)), stats)
        accepted += int(stats[:, 1].sum())
        po, temps = grid.state_points()
        rung_of = po if call < 3 else base[po]
        assert np.array_equal(rung_of, rex.rung_of)
        assert np.array_equal(temps, ladder[rex.rung_of])
    att, acc = rex.attempted.sum(), rex.accepted.sum()
    assert accepted == acc and 0 < acc < att
    a, b = plain.get_state(), grid.get_state()
    assert np.array_equal(a["occupancy"], b["occupancy"]) and np.array_equal(a["n_accepted"], b["n_accepted"])
    plain.close()
    grid.close()


# ---- 5. run_grid_exchange: host decisions = device decisions -------------------------------------------------------
@pytest.mark.parametrize("name", ["rocksalt444_ewald-int", "rocksalt333_two_sublattices-corr"])
def test_host_and_device_paths_of_run_grid_exchange_agree(name):
    case = CASES[name]()
    hist, states, grids = {}, {}, {}
    for host in (False, True):
        gx = _grid(case, seed=3)
        eng, _ = _engine(case, gx)
        hist[host] = []
        parallel.run_grid_exchange(eng, gx, 8, 100, host_decide=host, history=hist[host])
        states[host], grids[host] = eng.get_state(), gx
        assert np.array_equal(eng.state_points()[1], gx.point_temperatures[gx.point_of])
        assert np.array_equal(eng.get_walker_mu(), gx.point_rows[gx.point_of])
        eng.close()
    assert len(hist[False]) == 8 and all(np.array_equal(a, b) for a, b in zip(hist[False], hist[True]))
    assert not np.array_equal(hist[False][-1], np.arange(grids[False].npoints))
    for key in ("occupancy", "n_steps", "n_accepted", "accepted"):
        assert np.array_equal(states[False][key], states[True][key]), key
    # (the re-pricing sums are grouped differently on the two paths: not bit-equal)
    np.testing.assert_allclose(states[False]["enthalpy"], states[True]["enthalpy"], rtol=RTOL, atol=ATOL)
    for move in grids[False].MOVES:
        assert np.array_equal(grids[False].attempted[move], grids[True].attempted[move])
        assert np.array_equal(grids[False].accepted[move], grids[True].accepted[move])
    assert 0 < grids[False].acceptance < 1


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason(monkeypatch):
    from smol_amd.engine import Engine

    err = _errors()
    case = CASES["fcc_prim666_triplets-corr"]()
    gx = _grid(case)
    eng, _ = _engine(case, gx)
    R = gx.npoints
    ok = np.array([[0, 1], [2, 3]], dtype=np.int32)
    with pytest.raises(err, match="out of range 0 .. %d" % (R - 1)):
        eng.exchange_grid([[0, R]], [0.0])
    with pytest.raises(err, match="out of range"):
        eng.exchange_grid([[-1, 2]], [0.0])
    with pytest.raises(err, match="state point 1 appears in two pairs of one call"):
        eng.exchange_grid([[0, 1], [1, 2]], [0.0, 0.0])
    with pytest.raises(err, match="appears in two pairs of one call"):
        eng.exchange_grid([[4, 4]], [0.0])
    for bad in (np.nan, np.inf):
        with pytest.raises(err, match="log_u must be finite or -inf"):
            eng.exchange_grid(ok, [0.0, bad])
    with pytest.raises(ValueError, match="one log_u per pair"):
        eng.exchange_grid(ok, [0.0])
    with pytest.raises(ValueError, match="stats must be"):
        eng.exchange_grid(ok, [0.0, 0.0], np.zeros((2, 2), dtype=np.int32))
    assert np.array_equal(eng.state_points()[0], np.arange(R))  # (a refused call moves nothing)
    eng.close()
    # a handle with has_mu and no rows set is accepted: a pure temperature exchange
    eng, _ = _engine(case, gx, rows=False)
    eng.exchange_grid([[0, case.R]], [-np.inf])
    po, temps = eng.state_points()
    assert po[0] == case.R and po[case.R] == 0 and temps[0] == gx.temperatures[1] and temps[case.R] == gx.temperatures[0]
    assert "walker_mu" not in eng.kernel_info()
    # ... but not after a temperature-only device call moved the temperatures behind the points
    import torch

    buf = torch.full((R,), float(case.T), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    eng.import_temperature(buf.data_ptr())
    with pytest.raises(err, match="the state points have no temperatures"):
        eng.exchange_grid(ok, [0.0, 0.0])
    eng.set_temperature(gx.point_temperatures)
    eng.exchange_grid(ok, [0.0, 0.0])
    eng.close()
    # no has_mu
    plain = Engine(tables_for("fcc_prim666_triplets", MODES["int"]), capi.make_config(4, capi.KERNEL_METROPOLIS, capi.STEP_SWAP))
    with pytest.raises(err, match="smolmc_exchange_grid: the handle was created without has_mu"):
        plain.exchange_grid(ok, [0.0, 0.0])
    with pytest.raises(err, match="smolmc_get_state_points: the handle was created without has_mu"):
        plain.state_points()
    plain.close()
    # Wang-Landau
    wl = Engine(case.engine_tables(), capi.make_config(4, capi.KERNEL_WANGLANDAU, capi.STEP_FLIP, min_enthalpy=-50.0,
                                                       max_enthalpy=50.0, bin_size=0.5))
    with pytest.raises(err, match="smolmc_exchange_grid: a Wang-Landau handle estimates one density of states"):
        wl.exchange_grid(ok, [0.0, 0.0])
    wl.close()
    # mc_kernel / the universal kernel
    monkeypatch.setenv("SMOLMC_FORCE_GENERAL", "1")
    e2 = Engine(case.engine_tables(), case.config(4))
    monkeypatch.delenv("SMOLMC_FORCE_GENERAL")
    assert not e2.kernel_info().startswith("lean")
    with pytest.raises(err) as info:
        e2.exchange_grid(ok, [0.0, 0.0])
    assert "smolmc_exchange_grid: only the lean kernel families" in str(info.value) and "not lean: " + e2.not_lean_reason() in str(info.value)
    e2.close()


def test_distance_handle_is_refused():
    from smol_amd import sqs, synth
    from smol_amd.engine import Engine

    m = synth.build_cluster_model(synth.fcc_prim(), {2: 7.0, 3: 5.0})
    sc, tab = sqs.distance_tables(m, np.diag([2, 2, 2]), capi.FEATURES_CORRELATIONS)
    spec = sqs.distance_spec(m, capi.FEATURES_CORRELATIONS, None, None, 1.0, 1e-5, 1.0)
    eng = Engine(tab, capi.make_config(2, capi.KERNEL_METROPOLIS, capi.STEP_SWAP), distance=spec)
    with pytest.raises(_errors(), match="smolmc_exchange_grid: a distance handle has none"):
        eng.exchange_grid([[0, 1]], [0.0])
    eng.close()


# ---- 7. Sampler ---------------------------------------------------------------------------------------------------------
def test_sampler_traces_follow_the_exchanges(tmp_path):
    from smol_amd import moca, synth

    model = synth.build_cluster_model(synth.rocksalt_prim(), {2: 3.5})
    sc = synth.build_supercell(model, [3, 3, 3])
    ens = moca.Ensemble.from_cluster_expansion(sc, synth.random_coefs(model, seed=5, scale=0.05))
    names = ens.species
    ens.chemical_potentials = {names[0]: 0.1, names[1]: -0.2, names[2]: 0.05}
    temps = [3000.0, 3600.0, 4500.0]
    mus = [{names[0]: 0.1, names[1]: -0.2 + d, names[2]: 0.05} for d in np.linspace(-0.15, 0.15, 4)]
    nw = 12
    sampler = moca.Sampler.from_ensemble(ens, temperature=3000.0, nwalkers=nw, seeds=list(range(11, 11 + nw)))
    rng = np.random.default_rng(2)
    occ = np.zeros((nw, ens.num_sites), dtype=np.int32)
    occ[:, : sc.size] = rng.integers(0, 3, size=(nw, sc.size))
    gx = sampler.run_exchange(8, 200, occ, thin_by=100, grid=dict(temperatures=temps, chemical_potentials=mus, seed=4))
    c = sampler.samples
    assert c.num_samples == 16 and "walker_mu=1" in sampler.engine.kernel_info()
    point = c.get_trace_value("state_point", flat=False)[:, :, 0]
    assert point.dtype == np.int32 and point.shape == (16, nw)
    assert np.array_equal(point[0], np.arange(nw)) and np.array_equal(point[0], point[1])  # (nobody moved before the first attempt)
    assert all(sorted(row) == list(range(nw)) for row in point)
    assert 0 < gx.acceptance < 1 and not np.array_equal(point[-1], point[0])
    T = c.get_trace_value("temperature", flat=False)[:, :, 0]
    assert np.array_equal(T, gx.point_temperatures[point])
    # ... and the engine agrees with the last assignment, as do the kernels
    po, Tnow = sampler.engine.state_points()
    assert np.array_equal(Tnow, gx.point_temperatures[gx.point_of])
    assert [k.temperature for k in sampler.mckernels] == list(gx.point_temperatures[gx.point_of])
    assert [k.chemical_potentials for k in sampler.mckernels] == [mus[p % 4] for p in gx.point_of]
    assert sampler.walker_chemical_potentials == [mus[p % 4] for p in gx.point_of]
    np.testing.assert_array_equal(sampler.engine.get_walker_mu(), ens.walker_mu_rows([mus[p % 4] for p in gx.point_of]))
    # every sample is priced at the point it was taken at
    occs = c.get_occupancies(flat=False)
    work = c.get_feature_vectors(flat=False)[:, :, -1]
    for i in (0, 7, 15):
        rows = gx.point_rows[point[i]]
        np.testing.assert_allclose(work[i], sampler.engine.chemical_work(occs[i], rows), rtol=RTOL, atol=ATOL)
    # regrouped by point: row p is the chain of point p
    byT = c.by_state_point("temperature")
    assert byT.shape == (nw, 16, 1) and np.array_equal(byT[:, :, 0], np.repeat(gx.point_temperatures[:, None], 16, axis=1))
    H, byH = c.get_trace_value("enthalpy", flat=False), c.by_state_point("enthalpy", discard=4)
    assert byH.shape == (nw, 12, 1)
    for i in (4, 9, 15):
        assert np.array_equal(byH[point[i], i - 4, 0], H[i, :, 0])
    # the grid survives a round trip
    meta = c.metadata["state_points"]
    assert meta["shape"] == [1, 3, 4] and meta["temperatures"] == temps and meta["species"] == list(names)
    np.testing.assert_array_equal(meta["chemical_potentials"], [[d[sp] for sp in names] for d in mus])
    path = str(tmp_path / "exchange.npz")
    c.to_npz(path)
    back = moca.SampleContainer.from_npz(path, ens)
    assert back.metadata["state_points"] == _plain(meta)
    assert np.array_equal(back.by_state_point("enthalpy"), c.by_state_point("enthalpy"))
    # a second call continues: the grid of the last call, from the last sample
    after8 = np.array(gx.point_of)
    sampler.run_exchange(2, 200, thin_by=100)
    assert c.num_samples == 20 and np.array_equal(c.get_trace_value("state_point", flat=False)[16, :, 0], after8)
    # a plain run afterwards: nobody moves, the traces say where everybody is
    after10 = np.array(gx.point_of)
    sampler.run(300, thin_by=100)
    assert c.num_samples == 23
    assert np.array_equal(c.get_trace_value("state_point", flat=False)[20:, :, 0], np.repeat(after10[None], 3, axis=0))
    assert np.array_equal(c.get_trace_value("temperature", flat=False)[20:, :, 0], np.repeat(gx.point_temperatures[after10][None], 3, axis=0))
    occs, work = c.get_occupancies(flat=False), c.get_feature_vectors(flat=False)[:, :, -1]
    np.testing.assert_allclose(work[22], sampler.engine.chemical_work(occs[22], gx.point_rows[after10]), rtol=RTOL, atol=ATOL)
    # a sharded sampler is refused
    sharded = moca.Sampler.from_ensemble(ens, temperature=3000.0, nwalkers=nw, seeds=list(range(nw)), rank=0, world_size=2)
    with pytest.raises(ValueError, match="sharded over several ranks"):
        sharded.run_exchange(1, 100, occ[:6], grid=gx)


def _plain(meta):
    return dict(species=list(meta["species"]), temperatures=[float(t) for t in meta["temperatures"]],
                chemical_potentials=np.asarray(meta["chemical_potentials"], dtype=np.float64).tolist(), shape=list(meta["shape"]))


# ---- 8. sampling is unchanged by exchange ------------------------------------------------------------------------------
def test_exchange_leaves_the_sampled_distribution_alone():
    """fcc_conv444_pairs, 2 T x 7 rows x 64 replica sets = 896 walkers of 256 sites: 200 sweeps of burn-in, then 200
    blocks of one sweep + one attempt, against the same run without attempts.  Per state point the mean chemical
    work over the blocks, its standard error from the 64 replica-set means (independent sets in both runs).

    Temperatures 9000 K and 10800 K (3 x the case's 3000 K), the case's rows.  At 3000 K and 3600 K the model phase
    separates at the negative rows: independent walkers stay in the domains their random starts left them with, the
    standard error of the run WITHOUT exchange is 0.6 - 0.9 on means of 1 - 3, and adjacent points do not differ by
    10 of them (the run with exchange has 0.003 - 0.4 there: the hysteresis the move is for, and no reference to hold
    it against).  At 9000 K, on the CPU oracle alone (same sweeps, 64 walkers per point): adjacent points differ by
    more than 100 standard errors, and pairs of neighbours along mu / T would swap with probability 0.59 - 0.76 /
    0.54 - 0.87."""
    from smol_amd.engine import Engine

    case = CASES["fcc_conv444_pairs-int"]()
    reps, sweep, blocks = 64, case.N, 200
    means = {}
    for exchange in (False, True):
        gx = parallel.GridExchange(3.0 * case.T * np.array([1.0, 1.2]), case.rows, replicas=reps, seed=6)
        R = gx.npoints
        eng = Engine(case.engine_tables(), case.config(R))
        eng.set_walker_mu(gx.point_rows)
        occ, seeds = _start(case, R, seed=8)
        eng.set_state(occ, seeds, gx.point_temperatures)
        eng.run(200 * sweep)
        total = np.zeros(R)
        engine_point = np.arange(R)
        for _ in range(blocks):
            eng.run(sweep)
            if exchange:
                move = gx.move_of(gx.calls)
                pairs = gx.pairs(move)
                stats = np.zeros((len(pairs), 2), dtype=np.int64)
                eng.exchange_grid(engine_point[pairs], gx.log_u(gx.calls, len(pairs)), stats)
                gx.record(move, stats[:, 1])
                gx.calls += 1
                gx.point_of = eng.state_points()[0].astype(np.int64)
            work = eng.get_state(occupancy=False)["features"][:, -1]
            total[gx.point_of] += work  # (by state point)
        per_set = (total / blocks).reshape(reps, 2 * case.R)
        means[exchange] = (per_set.mean(axis=0), per_set.std(axis=0, ddof=1) / np.sqrt(reps), gx)
        eng.close()
    (m_ref, se_ref, _), (m_ex, se_ex, gx) = means[False], means[True]
    print("mean chemical work without exchange:", np.round(m_ref, 3), "\n  se", np.round(se_ref, 4))
    print("mean chemical work with exchange:   ", np.round(m_ex, 3), "\n  se", np.round(se_ex, 4))
    print("exchange acceptance:", gx.acceptance, {m: float(gx.accepted[m].sum() / max(gx.attempted[m].sum(), 1)) for m in gx.MOVES})
    # power: the points differ (on the run without exchange alone), and exchanges happen
    grid_ref = m_ref.reshape(2, case.R)
    gap = np.abs(np.diff(grid_ref, axis=1))
    se_pair = np.sqrt(se_ref.reshape(2, case.R)[:, 1:] ** 2 + se_ref.reshape(2, case.R)[:, :-1] ** 2)
    assert np.all(gap > 10 * se_pair), (gap, se_pair)
    assert 0.05 < gx.acceptance < 0.95
    z = np.abs(m_ex - m_ref) / np.sqrt(se_ex ** 2 + se_ref ** 2)
    print("z per point:", np.round(z, 2))
    assert np.all(np.abs(m_ex - m_ref) <= 5 * np.sqrt(se_ex ** 2 + se_ref ** 2)), z
