"""The minima record on the device (csrc/minima.hip; smolmc_set_minima, SMOLMC_SAMPLE_MINIMA, smolmc_update_minima): every
array of the record equals minima.MinimaRecord.offer, the NumPy definition, fed with the fetched columns -- array_equal, no
tolerance -- and a run with the flag is the same chain as a run without."""

import ctypes as C
import functools

import numpy as np
import pytest

from smol_amd import capi, moca
from smol_amd.minima import Minima, MinimaRecord
from smol_amd.observables import Observables
from tests.cases import load_case, tables_for
from tests.test_gpu_observables import ENV, _handle, _rand_occ

pytestmark = pytest.mark.gpu
INT = capi.FEATURES_INTERACTIONS
FIELDS = ("value", "enthalpy", "features", "occupancy", "counts", "walker", "sample", "step")
BLOCKS = (1, 3, 67)
THIN = 5


@pytest.fixture
def clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def _same_record(got, want, what=""):
    for f in FIELDS:
        g, w = getattr(got, f), getattr(want, f)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, f)
        np.testing.assert_array_equal(g, w, err_msg=f"{what} {f}")
    assert not (np.signbit(got.value) & (got.value == 0)).any()  # (no -0.0 among the values)
    assert (got.companions is None) == (want.companions is None) == bool(got.spec.n_axes), what
    if want.companions is not None:  # (per walker: every walker's occupancy at the offer walker 0's entry was taken from)
        assert got.companions.dtype == np.int32
        np.testing.assert_array_equal(got.companions, want.companions, err_msg=f"{what} companions")


def _semigrand(name, R, T=3000.0, mu=0.15):
    """A semigrand flip handle of a golden case with its default observables: (engine, observables, supercell)."""
    from smol_amd.engine import Engine

    sc = load_case(name)["sc"]
    nsp = max(sc.model.prim.nspecies)
    table = np.zeros((sc.num_sites, nsp))
    table[:, 1:] = mu * np.arange(1, nsp)
    tab = tables_for(name, INT, mu_table=table)
    eng = Engine(tab, capi.make_config(R, capi.KERNEL_METROPOLIS, capi.STEP_FLIP))
    obs = Observables.from_supercell(sc, tables=tab)
    eng.set_observables(obs)
    return eng, obs, sc


def _offer_blocks(rec, blocks, n_steps_end, thin=THIN):
    """Feed fetched blocks to the definition; the step of a row from the walkers' counters at the end of the last block."""
    total = sum(len(b["enthalpy"]) for b in blocks)
    at = 0
    for b in blocks:
        ns = len(b["enthalpy"])
        back = (total - 1 - (at + np.arange(ns))) * thin
        steps = n_steps_end[None, :] - back[:, None].astype(np.uint64)
        rec.offer(b["enthalpy"], b["features"], b["occupancy"], b.get("species_counts"), steps)
        at += ns
    return rec


def _run_blocks(eng, sizes=BLOCKS, thin=THIN, **kw):
    """Two blocks queued before the first fetch, then the rest: the fetched blocks in order."""
    out = []
    eng.run_sampled_async(sizes[0], thin, minima=True, **kw)
    for ns in sizes[1:]:
        eng.run_sampled_async(ns, thin, minima=True, **kw)
        out.append(eng.fetch_samples())
    out.append(eng.fetch_samples())
    return out


def _specs(eng, obs, sc):
    nat = eng.natural_parameters
    N = sc.num_sites
    K = obs.n_kinds
    one = np.zeros(K, dtype=np.int64)
    one[1] = 1
    two = np.zeros(K, dtype=np.int64)
    two[0], two[1] = 1, -1  # (N - 2 n_1 on a binary alloy: negative values, floor division)
    return {
        "walker-enthalpy": Minima.per_walker(),
        "walker-energy": Minima.per_walker(weights=nat[:-1]),  # (all but the chemical work)
        "one-axis": Minima.by_composition(obs, [1], extents=[N + 1], weights=nat[:-1]),
        # bin > 1, and an extent that leaves rows out: n_1 in [0, 2 (N // 4)) on axis 1
        "two-axes": Minima.by_composition(obs, [two, one], bins=[3, 2], extents=[N // 3 + 1, max(1, N // 4)]),
    }


# ---- 1: the record equals the definition; 3: the same record with the columns kept on the device ----------------------
@pytest.mark.parametrize("R", [3, 70])
@pytest.mark.parametrize("name", ["fcc_prim222_aliased", "fcc3_indicator_skew", "fcc_conv444_pairs"])
def test_record_equals_the_definition(name, R, clean_env):
    eng, obs, sc = _semigrand(name, R)
    fn = eng._lib.smolmc_debug_block_bytes
    fn.restype, fn.argtypes = C.c_longlong, [C.c_void_p]
    occ0 = _rand_occ(sc, np.random.default_rng(5), R)
    seeds = np.arange(R, dtype=np.uint64) + np.uint64(11)
    up = lambda x: (x + 255) & ~255  # noqa: E731
    for what, spec in _specs(eng, obs, sc).items():
        eng.set_minima(spec)
        assert eng.minima_shape() == (spec.n_slots(R), spec.n_axes)
        empty = eng.minima()
        _same_record(empty, MinimaRecord(spec, R, eng.F, eng.N, obs.n_kinds), what + " empty")
        eng.set_state(occ0, seeds, 3000.0)
        blocks = _run_blocks(eng, observables=True)
        got = eng.minima()
        end = eng.get_state()["n_steps"]
        want = _offer_blocks(MinimaRecord(spec, R, eng.F, eng.N, obs.n_kinds), blocks, end)
        _same_record(got, want, what)
        assert want.filled.any()
        values = np.concatenate([spec.values(b["enthalpy"], b["features"]).ravel() for b in blocks])
        print(name, R, what, "values", values.min(), values.max(), "filled", int(want.filled.sum()), "of", want.n_slots)
        if what.startswith("walker") and name == "fcc_conv444_pairs":  # (the case whose enthalpies and energies straddle zero)
            assert values.min() < 0 < values.max()
        if what == "two-axes":  # (rows were left out, and negative d_a met the floor division)
            key = np.concatenate([spec.keys(b["species_counts"], R, b["enthalpy"].shape).ravel() for b in blocks])
            cnt = np.concatenate([b["species_counts"].reshape(-1, obs.n_kinds) for b in blocks])
            assert (key < 0).any() and (key >= 0).any() and (cnt[:, 0] - cnt[:, 1] < 0).any()
        # minima alone: the rows, the counts and the scratch stay behind the downloaded part
        eng.set_minima(spec)
        eng.set_state(occ0, seeds, 3000.0)
        eng.run_sampled_async(BLOCKS[0], THIN, occupancy=False, minima=True)
        rows = BLOCKS[0] * R
        assert fn(eng._h) == up(rows * 8) + up(rows * eng.F * 8) + up(rows)
        eng.run_sampled_async(BLOCKS[1], THIN, occupancy=False, minima=True)
        dry = [eng.fetch_samples()]
        eng.run_sampled_async(BLOCKS[2], THIN, occupancy=False, minima=True)
        dry += [eng.fetch_samples(), eng.fetch_samples()]
        assert all(d["occupancy"] is None and "species_counts" not in d for d in dry)
        for d, b in zip(dry, blocks):
            np.testing.assert_array_equal(d["enthalpy"], b["enthalpy"])
        _same_record(eng.minima(), want, what + " alone")
    eng.close()


# ---- 2: ties -------------------------------------------------------------------------------------------------------------
def test_frozen_walkers_keep_the_first_offer(clean_env):
    """At 1e-3 K a flip handle freezes within a few sweeps: the enthalpy column repeats within and across blocks, and the
    entry names the first offer that reached the value."""
    R = 70
    eng, obs, sc = _semigrand("fcc_prim222_aliased", R)
    spec = Minima.per_walker()
    eng.set_minima(spec)
    eng.set_state(_rand_occ(sc, np.random.default_rng(2), R), np.arange(R, dtype=np.uint64), 1e-3)
    blocks = _run_blocks(eng, sizes=(3, 20, 9), thin=8, observables=True)
    H = np.concatenate([b["enthalpy"] for b in blocks])
    got = eng.minima()
    want = _offer_blocks(MinimaRecord(spec, R, eng.F, eng.N, obs.n_kinds), blocks, eng.get_state()["n_steps"], thin=8)
    _same_record(got, want)
    first = np.array([int(np.flatnonzero(H[:, r] == H[:, r].min())[0]) for r in range(R)])
    np.testing.assert_array_equal(got.sample, first)
    repeats = np.array([(H[:, r] == H[:, r].min()).sum() for r in range(R)])
    assert (repeats > 3).all() and (first < 31).all()  # (every walker froze: its lowest value repeats into the last block)
    eng.close()


def test_identical_chains_name_walker_zero(clean_env):
    R = 70
    eng, obs, sc = _semigrand("fcc_conv444_pairs", R)
    spec = Minima.by_composition(obs, [1], extents=[sc.num_sites + 1])
    eng.set_minima(spec)
    occ = np.tile(_rand_occ(sc, np.random.default_rng(3), 1), (R, 1))
    eng.set_state(occ, np.full(R, 77, dtype=np.uint64), 3000.0)
    blocks = _run_blocks(eng, sizes=(2, 5, 30), observables=True)
    assert all((b["enthalpy"] == b["enthalpy"][:, :1]).all() for b in blocks)
    got = eng.minima()
    assert got.filled.sum() > 3
    assert (got.walker[got.filled] == 0).all() and (got.walker[~got.filled] == -1).all()
    _same_record(got, _offer_blocks(MinimaRecord(spec, R, eng.F, eng.N, obs.n_kinds), blocks, eng.get_state()["n_steps"]))
    eng.close()


# ---- 4: the chain is untouched -----------------------------------------------------------------------------------------------
def test_chains_do_not_change(clean_env):
    for which in ("lean", "lazy", "wang-landau"):
        got = []
        for with_min in (False, True):
            eng, obs, occ, kw = _handle(which, 5, clean_env)
            eng.set_minima(Minima.per_walker())
            eng.run(13)
            blocks = [eng.run_sampled(4, 9, minima=with_min, **kw), eng.run_sampled(2, 5, minima=with_min, **kw)]
            got.append((blocks, eng.get_state(), eng.minima()))
            eng.close()
        (plain, st0, rec0), (kept, st1, rec1) = got
        for p, c in zip(plain, kept):
            assert set(p) == set(c)
            for key in p:
                assert np.array_equal(p[key], c[key]), (which, key)
        for key in st0:
            assert np.array_equal(st0[key], st1[key]), (which, key)
        assert not rec0.filled.any() and rec1.filled.all()


# ---- 5: every ring path -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["lean", "wang-landau", "lazy", "universal", "biased-general"])
def test_every_ring_path(which, clean_env):
    if which == "biased-general":
        clean_env.setenv("SMOLMC_NO_INKERNEL_BIAS", "1")
    R = 70
    eng, obs, occ, kw = _handle(which, R, clean_env)
    K = obs.n_kinds
    axis = np.zeros(K, dtype=np.int64)
    axis[K - 1] = 1
    for what, spec in (("walker", Minima.per_walker()),
                       ("keyed", Minima.by_composition(obs, [axis], bins=[2], extents=[eng.N // 2 + 1], weights=eng.natural_parameters))):
        eng.set_minima(spec)
        blocks = _run_blocks(eng, sizes=(2, 3, 4), thin=7, observables=True, **kw)
        got = eng.minima()
        want = _offer_blocks(MinimaRecord(spec, R, eng.F, eng.N, K), blocks, eng.get_state()["n_steps"], thin=7)
        _same_record(got, want, f"{which} {what}")
        assert want.filled.any()
    eng.close()


def test_vacancy_ewald_case(clean_env):
    R = 70
    eng, obs, sc = _semigrand("rocksalt333_vacancy_ewald", R)
    axis = np.zeros(obs.n_kinds, dtype=np.int64)
    axis[1] = 1
    for spec in (Minima.per_walker(weights=eng.natural_parameters[:-1]), Minima.by_composition(obs, [axis], extents=[sc.num_sites + 1])):
        eng.set_minima(spec)
        eng.set_state(_rand_occ(sc, np.random.default_rng(6), R), np.arange(R, dtype=np.uint64) + np.uint64(3), 3000.0)
        blocks = _run_blocks(eng, sizes=(1, 4, 3), observables=True)
        want = _offer_blocks(MinimaRecord(spec, R, eng.F, eng.N, obs.n_kinds), blocks, eng.get_state()["n_steps"])
        _same_record(eng.minima(), want)
    eng.close()


def test_relabelled_handle_gives_the_callers_numbering(clean_env):
    from smol_amd.engine import Engine
    from tests.test_gpu_capi_relabel import _model

    sc, ens, tab, occ, frozen = _model(capi.STEP_SWAP)
    R = len(occ)
    eng = Engine(tab, capi.make_config(R, capi.KERNEL_METROPOLIS, capi.STEP_SWAP))
    assert "relabelled=1" in eng.kernel_info(), eng.kernel_info()
    obs = Observables.from_supercell(sc)
    eng.set_observables(obs)
    spec = Minima.per_walker()
    eng.set_minima(spec)
    eng.set_state(occ, np.arange(R, dtype=np.uint64) + np.uint64(9), 4000.0)
    blocks = _run_blocks(eng, sizes=(2, 3, 4), thin=9, observables=True)
    got = eng.minima()
    _same_record(got, _offer_blocks(MinimaRecord(spec, R, eng.F, eng.N, obs.n_kinds), blocks, eng.get_state()["n_steps"], thin=9))
    np.testing.assert_array_equal(got.occupancy[:, frozen], occ[:, frozen])  # (the frozen sites, by the caller's numbers)
    eng.close()


# ---- 6: between runs ---------------------------------------------------------------------------------------------------------
def test_between_runs(clean_env):
    from smol_amd.engine import EngineError

    R = 6
    eng, obs, sc = _semigrand("fcc_conv444_pairs", R)
    N, K = sc.num_sites, obs.n_kinds
    err = (EngineError, ValueError)
    occ0 = _rand_occ(sc, np.random.default_rng(8), R)
    for spec in (Minima.per_walker(), Minima.by_composition(obs, [1], bins=[4], extents=[N // 4 + 1], weights=eng.natural_parameters[:-1])):
        eng.set_minima(spec)
        want = MinimaRecord(spec, R, eng.F, N, K)
        eng.set_state(occ0, np.arange(R, dtype=np.uint64), 3000.0)
        for n in (40, 25, 1):  # update_minima after run: one offer of the current states
            eng.run(n)
            eng.update_minima()
            st = eng.get_state()
            want.offer(st["enthalpy"], st["features"], st["occupancy"], obs.evaluate(st["occupancy"])[0], st["n_steps"])
            _same_record(eng.minima(), want)
        assert want.sample.max() > 0 or spec.n_axes
        # set_state and discard_samples keep the record; ring offers continue the numbering
        eng.set_state(occ0, np.arange(R, dtype=np.uint64) + np.uint64(50), 3000.0)
        _same_record(eng.minima(), want)
        eng.run_sampled_async(3, 7, observables=True, minima=True)
        eng.discard_samples()
        kept = eng.minima()
        assert kept.sample.max() <= 5
        eng.set_state(occ0, np.arange(R, dtype=np.uint64) + np.uint64(50), 3000.0)
        b = eng.run_sampled(3, 7, observables=True)  # (the same chain again, fetched this time)
        _offer_blocks(want, [b], eng.get_state()["n_steps"], thin=7)
        _same_record(kept, want)
        eng.reset_minima()
        _same_record(eng.minima(), MinimaRecord(spec, R, eng.F, N, K))
        eng.update_minima()
        assert eng.minima().sample.max() == 0  # (the numbering restarted)
    # the refusals, each by its message; the handle stays as it was
    keyed = eng.minima_shape()
    one = Minima.by_composition(obs, [1], extents=[4])
    with pytest.raises(err, match="n_weights = 99 is larger than the handle's"):
        eng.set_minima(Minima.per_walker(weights=np.ones(99)))
    for bins, extents in (([0], [4]), ([1], [0]), ([-3], [4])):
        with pytest.raises(err, match="each must be >= 1"):
            eng.set_minima(Minima.by_composition(obs, [1], bins=bins, extents=extents))
    with pytest.raises(err, match="slots, larger than the limit of 2\\^20"):
        eng.set_minima(Minima.by_composition(obs, [1, 0], extents=[1025, 1024]))
    assert eng.minima_shape() == keyed
    with pytest.raises(err, match="while a minima record keyed by composition depends on the observables"):
        eng.set_observables(None)
    with pytest.raises(err, match="while a minima record keyed by composition depends on the observables"):
        eng.set_observables(obs)
    assert eng.observables_shape() == (K, obs.n_shells) and eng.minima_shape() == keyed
    eng.set_minima(None)
    assert eng.minima_shape() == (0, 0)
    with pytest.raises(err, match="SMOLMC_SAMPLE_MINIMA without a minima record"):
        eng.run_sampled_async(1, 5, minima=True)
    assert eng.pending_samples()[0] == 0
    with pytest.raises(err, match="no minima record set"):
        eng.update_minima()
    eng.set_observables(None)
    with pytest.raises(err, match="keyed by composition needs observables"):
        eng.set_minima(one)
    assert eng.minima_shape() == (0, 0)
    # a per-walker record without observables: counts of width 0
    eng.set_minima(Minima.per_walker())
    b = eng.run_sampled(2, 5, minima=True)
    rec = eng.minima()
    assert rec.counts.shape == (R, 0) and rec.filled.all()
    np.testing.assert_array_equal(rec.value, b["enthalpy"].min(axis=0))
    eng.close()
    # 2^20 slots are allowed, a record beyond 1 GiB is not: 1728 sites make 2^20 entries of 1.8 KB
    from smol_amd import synth
    from smol_amd.engine import Engine

    big = synth.build_supercell(synth.build_cluster_model(synth.fcc_prim(), {2: 3.0}), [12, 12, 12])
    eng = Engine(capi.TableSet.from_synth(big, synth.random_coefs(big.model), feature_mode=INT), capi.make_config(1))
    wide = Observables.from_supercell(big)
    eng.set_observables(wide)
    with pytest.raises(err, match="is larger than 1 GiB"):
        eng.set_minima(Minima.by_composition(wide, [1, 0], extents=[1024, 1024]))
    assert eng.minima_shape() == (0, 0)
    eng.set_minima(Minima.by_composition(wide, [1], extents=[big.num_sites + 1]))
    assert eng.minima_shape() == (big.num_sites + 1, 1)
    eng.close()


# ---- 8: it finds ground states ----------------------------------------------------------------------------------------------
def test_it_finds_the_ground_state_of_every_composition(clean_env):
    """8 binary sites, 256 states, all enumerated.  A semigrand anneal of 64 walkers over a mu grid with a composition-keyed
    energy record fills all 9 compositions with states of the enumerated minimum energy."""
    R = 64
    eng, obs, sc = _semigrand("fcc_prim222_aliased", R)
    N = sc.num_sites
    assert N == 8 and obs.n_kinds == 2
    nat = eng.natural_parameters
    states = ((np.arange(256)[:, None] >> np.arange(N)) & 1).astype(np.int32)
    E = eng.eval_full(states)[:, :-1] @ nat[:-1]
    n1 = states.sum(axis=1)
    e_min = np.array([E[n1 == c].min() for c in range(N + 1)])
    spec = Minima.by_composition(obs, [1], extents=[N + 1], weights=nat[:-1])
    eng.set_minima(spec)
    # the grid: chemical potential differences that span the slopes of the energy against the composition
    slope = np.abs(np.diff(e_min)).max() * 1.5
    mus = np.linspace(-slope, slope, R)
    rows = np.zeros((R, 1, 2))
    rows[:, 0, 1] = mus
    eng.set_walker_mu(rows)
    eng.set_state(_rand_occ(sc, np.random.default_rng(1), R), np.arange(R, dtype=np.uint64) + np.uint64(100), 5000.0)
    for T in (5000.0, 2000.0, 800.0, 300.0, 100.0):
        eng.set_temperature(T)
        eng.run_sampled_async(64, 2, occupancy=False, minima=True)
        eng.fetch_samples()
    rec = eng.minima()
    assert rec.filled.all() and rec.n_slots == N + 1
    np.testing.assert_array_equal(rec.occupancy.sum(axis=1), np.arange(N + 1))
    np.testing.assert_array_equal(rec.counts[:, 1], np.arange(N + 1))
    e_rec = eng.eval_full(rec.occupancy)[:, :-1] @ nat[:-1]
    print("ground states", e_rec - e_min, rec.sample)
    np.testing.assert_array_equal(e_rec, e_min)
    np.testing.assert_allclose(rec.value, e_rec, rtol=1e-10, atol=0)
    eng.close()


# ---- 7: the sampler ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sampler_runs(energy):
    """Same seeds, kept occupancies against keep_occupancy=False plus minima=: (kept container, dry container)."""
    c = load_case("rocksalt333_two_sublattices")
    nw = 6
    out = []
    for keep in (True, False):
        ens = moca.Ensemble.from_cluster_expansion(c["sc"], c["coefs"])
        names = list(ens.species)
        ens.chemical_potentials = {sp: 0.1 * (i - 1) for i, sp in enumerate(names)}
        spec = Minima.per_walker(weights=Minima.energy_weights(ens) if energy else None)
        s = moca.Sampler.from_ensemble(ens, temperature=3000.0, nwalkers=nw, seeds=list(range(3, 3 + nw)), rank=0, world_size=1,
                                       minima=None if keep else spec)
        occ = _rand_occ(c["sc"], np.random.default_rng(12), nw)
        s.run(40 * 9, occ, thin_by=9, keep_occupancy=keep)
        s.run(25 * 9, thin_by=9, keep_occupancy=keep)  # (a second run: the record goes on)
        out.append(s)
    return out[0], out[1]


@pytest.mark.parametrize("energy", [False, True])
def test_sampler_getters_answer_from_the_record(energy, clean_env, tmp_path):
    kept, dry = (s.samples for s in _sampler_runs(energy))
    assert kept.num_samples == dry.num_samples == 65
    assert len(kept.natural_parameters) > kept._num_energy_coefs  # (energy and enthalpy differ: the chemical work)
    with pytest.raises(ValueError, match="keep_occupancy=False"):
        dry.get_occupancies()
    getter = "get_minimum_energy_occupancy" if energy else "get_minimum_enthalpy_occupancy"
    other = "get_minimum_enthalpy_occupancy" if energy else "get_minimum_energy_occupancy"
    np.testing.assert_array_equal(getattr(dry, getter)(flat=True), getattr(kept, getter)(flat=True))
    rec = dry.minima
    # (the record's energy is the left-to-right sum of the definition; get_energies takes a matrix product)
    values = rec.spec.values(kept.get_enthalpies(flat=False)[..., 0], kept.get_trace_value("features", flat=False))
    if energy:
        f = kept.get_trace_value("features", flat=False)[..., :rec.spec.n_weights]
        bound = 2 * rec.spec.n_weights * np.finfo(float).eps * (np.abs(f) @ np.abs(rec.spec.weights))  # (two sums of n terms)
        assert (np.abs(values - kept.get_energies(flat=False)[..., 0]) <= bound).all()
    np.testing.assert_array_equal(rec.value, values.min(axis=0) + 0.0)
    np.testing.assert_array_equal(rec.sample, values.argmin(axis=0))
    np.testing.assert_array_equal(rec.occupancy, kept.get_occupancies(flat=False)[values.argmin(axis=0), np.arange(6)])
    for call in (lambda: getattr(dry, getter)(discard=1), lambda: getattr(dry, getter)(thin_by=2), lambda: getattr(dry, other)()):
        with pytest.raises(ValueError, match="minima="):
            call()
    path = str(tmp_path / "c.npz")
    dry.to_npz(path)
    back = moca.SampleContainer.from_npz(path, dry.ensemble)
    assert back.minima.equals(rec) and back.minima.offers == 65 and back.minima.spec.n_weights == rec.spec.n_weights
    np.testing.assert_array_equal(getattr(back, getter)(), getattr(kept, getter)())
    again = moca.SampleContainer.from_dict(dry.as_dict(), dry.ensemble)
    assert again.minima.equals(rec)
    # clear_samples leaves the record alone, reset_minima empties it
    sampler = _sampler_runs(energy)[1]
    assert sampler.minima.equals(rec)


@pytest.mark.parametrize("energy", [False, True])
def test_sampler_getters_with_flat_false(energy, clean_env, tmp_path):
    """With ``flat=False`` the stored-occupancy getter (as the reference's, container.py:316-318) returns EVERY walker's
    occupancy at the sample where walker 0 was lowest -- ``occ[inds, arange(nw)][0]`` with inds of shape (nw, 1).  The
    record keeps those rows next to walker 0's entry (its companions)."""
    kept, dry = (s.samples for s in _sampler_runs(energy))
    getter = "get_minimum_energy_occupancy" if energy else "get_minimum_enthalpy_occupancy"
    want = getattr(kept, getter)(flat=False)
    assert want.shape == (6, dry.shape[1]) and len({w.tobytes() for w in want}) > 1
    np.testing.assert_array_equal(dry.minima.occupancy[0], want[0])
    got = getattr(dry, getter)(flat=False)
    assert got.dtype == want.dtype
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(want, kept.get_occupancies(flat=False)[dry.minima.sample[0]])
    path = str(tmp_path / "c.npz")
    dry.to_npz(path)
    np.testing.assert_array_equal(getattr(moca.SampleContainer.from_npz(path, dry.ensemble), getter)(flat=False), want)
    np.testing.assert_array_equal(getattr(moca.SampleContainer.from_dict(dry.as_dict(), dry.ensemble), getter)(flat=False), want)
    with pytest.raises(ValueError, match="minima="):
        getattr(dry, getter)(flat=False, discard=1)
