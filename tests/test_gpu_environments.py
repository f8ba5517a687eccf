"""Coordination environments on the device (the census in csrc/observables.hip; smolmc_set_environments,
smolmc_eval_environments, the SMOLMC_SAMPLE_ENVIRONMENTS column of the sample ring, the environment columns of a statistics
record): every cell and every code equals environments.Environments.evaluate / codes, the NumPy definition, entry for
entry -- int32 on both sides, no tolerance -- and a run with environments is the same chain as a run without."""

import ctypes as C

import numpy as np
import pytest

from smol_amd import capi, moca
from smol_amd import statistics as st
from smol_amd.environments import Environments, EnvironmentSet
from smol_amd.observables import Observables
from smol_amd.patterns import Patterns, PatternSet
from smol_amd.statistics import Statistics, StatisticsRecord
from tests.cases import load_case, tables_for
from tests.test_environments_host import case_spec, shell_lengths
from tests.test_gpu_observables import ENV, _rand_occ

pytestmark = pytest.mark.gpu
INT = capi.FEATURES_INTERACTIONS


@pytest.fixture
def clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def _same(got, want):
    assert got.dtype == np.int32 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    np.testing.assert_array_equal(got, want)


def _engine(name, R=3, step=capi.STEP_SWAP):
    from smol_amd.engine import Engine

    sc = load_case(name)["sc"]
    tab = tables_for(name, INT)
    return Engine(tab, capi.make_config(R, capi.KERNEL_METROPOLIS, step)), sc, tab


# ---- smolmc_eval_environments ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fcc_prim666_triplets", "fcc3_indicator_skew", "fcc_prim222_aliased",
                                  "rocksalt333_two_sublattices"])
def test_eval_equals_the_definition(name, clean_env):
    """216 sites, binary, z = 12: 338 cells, a histogram per wave; 60 sites (below a wavefront, no multiple of 16), ternary
    with B = 3: 2197 cells, the shared histogram; 8 sites whose 12-slot rows repeat sites and name the centre; centres on
    one sublattice with their neighbours on the other, of another species width, two sets with equal maps.  1, 3 and all
    occupancies, then the walkers' own states."""
    R = 3
    eng, _, tab = _engine(name, R)
    sc, obs, spec = case_spec(name)
    if name == "fcc_prim666_triplets":
        assert sc.num_sites == 216 and spec.sets[0].width == 12 and spec.n_cells == 338
    if name == "fcc3_indicator_skew":
        assert sc.num_sites == 60 and spec.sets[0].n_neigh_classes == 3 and spec.n_cells == 2197
    if name == "fcc_prim222_aliased":
        s = spec.sets[0]
        rows = s.neighbours.copy()
        rows[::2, 5] = s.centres[::2]  # (the rows repeat sites as they are; every other one names its centre too)
        spec = Environments(obs, [EnvironmentSet(s.centres, rows, s.centre_class_of_kind, s.n_centre_classes, s.neigh_class_of_kind,
                                                 s.n_neigh_classes)])
        assert sc.num_sites == 8 and s.width == 12 and all(len(set(r)) < 12 for r in rows.tolist())
        assert any(c in r for c, r in zip(s.centres.tolist(), rows.tolist()))
    if name == "rocksalt333_two_sublattices":
        sub = np.asarray(sc.site_b)
        assert spec.n_sets == 2
        for e, s in enumerate(spec.sets):
            assert (sub[s.centres] == e).all() and (sub[s.neighbours] == 1 - e).all() and s.width == 6
        assert sc.model.prim.nspecies[0] != sc.model.prim.nspecies[1]
    assert eng.environments_shape() == (0, 0, 0)
    eng.set_observables(obs)
    eng.set_environments(spec)
    assert eng.environments_shape() == (spec.n_sets, spec.n_cells, spec.n_centres)
    rng = np.random.default_rng(17)
    pool = _rand_occ(sc, rng, 130)
    want, want_codes = spec.evaluate(pool), spec.codes(pool)
    for e in range(spec.n_sets):
        assert want[:, spec.cell_ptr[e]:spec.cell_ptr[e + 1]].any(axis=0).sum() > 4  # (several cells of every set are hit)
    for nocc in (1, 3, 130):
        cells, codes = eng.environments(pool[:nocc], codes=True)
        _same(cells, want[:nocc])
        _same(codes, want_codes[:nocc])
        _same(eng.environments(pool[:nocc]), want[:nocc])
    # the codes alone (cells == NULL)
    codes = np.zeros((3, spec.n_centres), dtype=np.int32)
    p = pool[:3].astype(np.int32)
    assert eng._lib.smolmc_eval_environments(eng._h, p.ctypes.data_as(C.POINTER(C.c_int32)), 3, None,
                                             codes.ctypes.data_as(C.POINTER(C.c_int32))) == 0
    _same(codes, want_codes[:3])
    # occ = NULL: the walkers' current states, after a short run
    occ = pool[:R].copy()
    eng.set_state(occ, np.arange(R, dtype=np.uint64) + np.uint64(5), 2500.0)
    eng.run(300, sync=True)
    state = eng.get_state()
    assert not np.array_equal(state["occupancy"], occ)
    cells, codes = eng.environments(codes=True)
    _same(cells, spec.evaluate(state["occupancy"]))
    _same(codes, spec.codes(state["occupancy"]))
    # the sites of one environment, picked out of the codes
    code = int(codes[0][codes[0] >= 0][0])
    assert len(spec.sites_with(codes[0], 0, code)) == (codes[0, :spec.centre_ptr[1]] == code).sum() > 0
    # the observables' own answers are what they are without an environment spec
    with_spec = eng.observables(pool[:5])
    eng.set_environments(None)
    assert eng.environments_shape() == (0, 0, 0)
    for a, b in zip(with_spec, eng.observables(pool[:5])):
        np.testing.assert_array_equal(a, b)
    with pytest.raises((RuntimeError, ValueError), match="no environment spec set"):
        eng.environments(pool[:1])
    eng.close()


def _ternary(R=2):
    """The 60-site ternary handle with kinds per site class (six kinds) set as its observables."""
    eng, sc, tab = _engine("fcc3_indicator_skew", R)
    obs = Observables.from_supercell(sc, site_classes=np.arange(sc.num_sites) % 2)
    assert sc.num_sites == 60 and obs.n_kinds == 6
    eng.set_observables(obs)
    return eng, sc, obs


def _check(eng, spec, pool):
    eng.set_environments(spec)
    assert eng.environments_shape() == (spec.n_sets, spec.n_cells, spec.n_centres)
    want, want_codes = spec.evaluate(pool), spec.codes(pool)
    cells, codes = eng.environments(pool, codes=True)
    _same(cells, want)
    _same(codes, want_codes)
    return want


def test_synthetic_sets(clean_env):
    eng, sc, obs = _ternary()
    N = sc.num_sites
    rng = np.random.default_rng(23)
    pool = _rand_occ(sc, rng, 9)
    A3, A2, A1 = np.array([0, 1, 2, 0, 1, 2], np.int32), np.array([0, 1, 1, 1, 0, -1], np.int32), np.zeros(6, np.int32)
    B = {1: np.array([0, 0, -1, 0, 0, 0], np.int32), 2: np.array([0, 1, 1, 0, -1, 1], np.int32),
         3: np.array([0, 1, 2, 0, 1, 2], np.int32), 4: np.array([0, 1, 2, 3, 1, -1], np.int32)}

    def mk(n, z, a, na, b, empty=True):
        rows = rng.integers(-1 if empty else 0, N, size=(n, z))  # (-1: an empty slot)
        return EnvironmentSet(rng.integers(0, N, size=n), rows, a, na, B[b], b)

    # every centre count around a wavefront and a workgroup; z = 1, 12 and 64; B = 1 .. 4; rows with empty slots; two
    # neighbours with equal maps (sets 1, 2) and neighbours with different maps; 3403 cells: the shared histogram
    for n in (0, 1, 63, 64, 65, 257):
        spec = Environments(obs, [mk(n, 1, A3, 3, 4), mk(n, 12, A2, 2, 2), mk(n, 3, A2, 2, 2), mk(n, 64, A3, 3, 1),
                                  mk(n, 4, A1, 1, 4), mk(n, 12, A1, 1, 3)])
        assert spec.n_cells == 48 + 338 + 32 + 195 + 625 + 2197 and 4 * spec.n_cells > capi.MAX_ENV_CELLS
        want = _check(eng, spec, pool)
        if n:
            assert (want.sum(axis=1) > 0).all()
    # small enough for a histogram per wave: every z and B again, set by set
    for z, a, na, b in ((1, A3, 3, 1), (1, A3, 3, 4), (12, A2, 2, 1), (12, A2, 2, 2), (64, A3, 3, 1), (4, A1, 1, 4), (2, A3, 3, 3)):
        spec = Environments(obs, [mk(257, z, a, na, b)])
        assert 4 * spec.n_cells <= capi.MAX_ENV_CELLS
        want = _check(eng, spec, pool)
        assert (want > 1).any()  # (cells hit more than once: the adds meet)
    # full rows: the n_b of a centre sum to the width where every kind has a class
    spec = Environments(obs, [mk(300, 12, A1, 1, 3, empty=False)])
    want = _check(eng, spec, pool)
    codes = spec.codes(pool)
    assert (codes % 13 + codes // 13 % 13 + codes // 169 == 12).all() and (want.sum(axis=1) == 300).all()
    # 4096 cells exactly: the shared histogram
    spec = Environments(obs, [mk(900, 7, A1, 1, 4)])
    assert spec.n_cells == capi.MAX_ENV_CELLS
    _check(eng, spec, pool)
    # ... and one more cell is refused: the spec in force stays
    msg = _refused(eng, [7, 1], [1, 1], [4, 1], [A1, A1], [B[4], B[1]], [[0], [0]], [np.zeros((1, 7)), np.zeros((1, 1))])
    assert "more than SMOLMC_MAX_ENV_CELLS = 4096 cells" in msg
    assert eng.environments_shape() == (1, 4096, 900)
    _same(eng.environments(pool[:2]), spec.evaluate(pool[:2]))
    # eight sets in one spec, neighbours with equal maps among them
    maps = [rng.integers(-1, 2, size=6).astype(np.int32) for _ in range(6)]
    maps = [maps[0], maps[0], maps[1], maps[2], maps[2], maps[3], maps[4], maps[5]]
    spec = Environments(obs, [EnvironmentSet(rng.integers(0, N, size=90 + 7 * t), rng.integers(-1, N, size=(90 + 7 * t, 1 + 2 * t)),
                                             A3, 3, maps[t], 2) for t in range(8)])
    _check(eng, spec, pool)
    eng.close()


def test_patterns_and_environments_together_and_each_alone(clean_env):
    eng, sc, obs = _ternary(R=4)
    N = sc.num_sites
    rng = np.random.default_rng(31)
    pool = _rand_occ(sc, rng, 7)
    code = Patterns.class_map(obs, "code")
    pat = Patterns(obs, [PatternSet(rng.integers(0, N, size=(300, 3)), code[0], 3), PatternSet(rng.integers(0, N, size=(90, 2)), code[0], 3)])
    env = Environments(obs, [EnvironmentSet(rng.integers(0, N, size=200), rng.integers(-1, N, size=(200, 12)),
                                            np.array([0, 1, 1, 0, 1, 1], np.int32), 2, np.array([0, 1, 1, 0, 1, -1], np.int32), 2)])
    want_p, want_e = pat.evaluate(pool), env.evaluate(pool)
    eng.set_environments(env)
    _same(eng.environments(pool), want_e)
    eng.set_patterns(pat)
    _same(eng.environments(pool), want_e)
    _same(eng.patterns(pool), want_p)
    # one launch counts both: the ring with both flags, with one and with the observables
    eng.set_state(pool[:4], np.arange(4, dtype=np.uint64) + np.uint64(3), 3000.0)
    for kw in (dict(patterns=True, environments=True), dict(environments=True), dict(patterns=True),
               dict(patterns=True, environments=True, observables=True)):
        smp = eng.run_sampled(3, 7, **kw)
        assert ("pattern_counts" in smp) == ("patterns" in kw) and ("environment_counts" in smp) == ("environments" in kw)
        if "patterns" in kw:
            _same(smp["pattern_counts"], pat.evaluate(smp["occupancy"]))
        if "environments" in kw:
            _same(smp["environment_counts"], env.evaluate(smp["occupancy"]))
        if "observables" in kw:
            for got, want in zip((smp["species_counts"], smp["pair_counts"]), obs.evaluate(smp["occupancy"])):
                _same(got, want)
    eng.set_environments(None)
    _same(eng.patterns(pool), want_p)
    eng.close()


def test_relabelled_handle_takes_the_callers_numbering(clean_env):
    """The restricted-sites recipe of test_gpu_capi_relabel: the engine renumbers the sites; the centres and their rows go
    in by the caller's numbers and the codes come back in the caller's order of centres."""
    from smol_amd.engine import Engine
    from tests.test_gpu_capi_relabel import _model

    sc, ens, tab, occ, frozen = _model(capi.STEP_SWAP)
    R = len(occ)
    eng = Engine(tab, capi.make_config(R, capi.KERNEL_METROPOLIS, capi.STEP_SWAP))
    assert "relabelled=1" in eng.kernel_info(), eng.kernel_info()
    classes = np.zeros(sc.num_sites, dtype=np.int64)
    classes[frozen] = 1
    obs = Observables.from_supercell(sc, site_classes=classes)
    eng.set_observables(obs)
    spec = Environments.from_supercell(sc, obs, distances=[shell_lengths(sc)[0]], centre_classes="kind", neigh_classes="code")
    eng.set_environments(spec)
    pool = _rand_occ(sc, np.random.default_rng(8), 3)
    cells, codes = eng.environments(pool, codes=True)
    _same(cells, spec.evaluate(pool))
    _same(codes, spec.codes(pool))
    eng.set_state(occ, np.arange(R, dtype=np.uint64) + np.uint64(9), 4000.0)
    eng.run(200, sync=True)
    _same(eng.environments(), spec.evaluate(eng.get_state()["occupancy"]))
    smp = eng.run_sampled(2, 9, environments=True)
    _same(smp["environment_counts"], spec.evaluate(smp["occupancy"]))
    eng.close()


# ---- the ring --------------------------------------------------------------------------------------------------------
def _ring_handle(R, with_spec=True, with_patterns=False):
    eng, _, tab = _engine("fcc_prim666_triplets", R)
    sc, obs, spec = case_spec("fcc_prim666_triplets")
    obs = Observables.from_supercell(sc, tables=tab)
    eng.set_observables(obs)
    if with_patterns:
        eng.set_patterns(Patterns.from_supercell(sc, obs))
    if with_spec:
        eng.set_environments(spec)
    occ = (np.random.default_rng(21).random((R, sc.num_sites)) < 0.5).astype(np.int32)
    eng.set_state(occ, np.arange(R, dtype=np.uint64) + np.uint64(31), 3000.0)
    return eng, obs, spec, occ


@pytest.mark.parametrize("R", [1, 130])
def test_ring_column_equals_the_definition_on_the_blocks_occupancies(R, clean_env):
    eng, obs, spec, occ = _ring_handle(R)
    eng.run(11)
    smp = eng.run_sampled(3, 7, environments=True)
    assert "species_counts" not in smp and smp["occupancy"].shape == (3, R, eng.N)
    _same(smp["environment_counts"], spec.evaluate(smp["occupancy"]))
    both = eng.run_sampled(2, 7, environments=True, observables=True)
    _same(both["environment_counts"], spec.evaluate(both["occupancy"]))
    for got, want in zip((both["species_counts"], both["pair_counts"]), obs.evaluate(both["occupancy"])):
        _same(got, want)
    # without the occupancy column: the same cells, the rows stay on the device
    eng.set_state(occ, np.arange(R, dtype=np.uint64) + np.uint64(31), 3000.0)
    eng.run(11)
    eng.run_sampled_async(3, 7, occupancy=False, environments=True)
    npend, ns, flags = eng.pending_samples()
    assert (npend, ns) == (1, 3) and flags & capi.SAMPLE_ENVIRONMENTS and not flags & capi.SAMPLE_OCCUPANCY
    fn = eng._lib.smolmc_debug_block_bytes
    fn.restype, fn.argtypes = C.c_longlong, [C.c_void_p]
    up = lambda x: (x + 255) & ~255  # noqa: E731
    rows = 3 * R
    assert fn(eng._h) == up(rows * 8) + up(rows * eng.F * 8) + up(rows) + up(rows * spec.n_cells * 4)
    dry = eng.fetch_samples()
    assert dry["occupancy"] is None
    _same(dry["environment_counts"], smp["environment_counts"])
    np.testing.assert_array_equal(dry["enthalpy"], smp["enthalpy"])
    eng.close()


def test_chains_counts_pairs_and_pattern_cells_do_not_change(clean_env):
    """Same seeds with and without the spec and the flag: identical samples, final state and counters; the counts, pairs
    and pattern cells of a block are the same bits with and without an environment spec set."""
    got = []
    for mode in ("no spec", "spec, no flag", "flag"):
        eng, obs, spec, occ = _ring_handle(5, with_spec=mode != "no spec", with_patterns=True)
        eng.run(13)
        kw = dict(environments=True) if mode == "flag" else {}
        blocks = [eng.run_sampled(4, 9, observables=True, patterns=True, **kw), eng.run_sampled(2, 5, observables=True, patterns=True, **kw)]
        got.append((blocks, eng.get_state()))
        eng.close()
    (plain, st0) = got[0]
    assert all({"species_counts", "pair_counts", "pattern_counts"} <= set(b) for b in plain)
    for blocks, state in got[1:]:
        for p, c in zip(plain, blocks):
            for key in p:
                assert p[key].dtype == c[key].dtype and np.array_equal(p[key], c[key]), key
        for key in st0:
            assert np.array_equal(st0[key], state[key]), key
    assert all("environment_counts" in b for b in got[2][0]) and not any("environment_counts" in b for b in got[1][0])
    assert {"n_steps", "n_accepted"} <= set(st0)


def test_ring_discipline(clean_env):
    from smol_amd.engine import EngineError, RingFullError

    eng, obs, spec, occ = _ring_handle(4)
    err = (EngineError, ValueError)
    eng.run_sampled_async(2, 5, environments=True)
    eng.run_sampled_async(3, 4, environments=True, occupancy=False)  # (two blocks in flight)
    # the getter reads the block the next fetch delivers, and does not deliver it
    c0 = eng.sample_environments()
    assert c0.shape == (2, 4, spec.n_cells) and eng.pending_samples()[:2] == (2, 2)
    np.testing.assert_array_equal(c0, eng.sample_environments())
    with pytest.raises(RingFullError, match="sample ring full"):
        eng.run_sampled_async(1, 5, environments=True)
    a = eng.fetch_samples()
    _same(c0, spec.evaluate(a["occupancy"]))
    _same(a["environment_counts"], c0)
    c1 = eng.sample_environments()
    assert c1.shape == (3, 4, spec.n_cells) and eng.pending_samples()[:2] == (1, 3)
    b = eng.fetch_samples()
    assert b["occupancy"] is None
    _same(b["environment_counts"], c1)
    # a new spec while a counted block waits: refused; the block and the spec stay
    eng.run_sampled_async(1, 3, environments=True)
    with pytest.raises(err, match="waits in the ring"):
        eng.set_environments(spec)
    with pytest.raises(err, match="waits in the ring"):
        eng.set_environments(None)
    assert eng.pending_samples()[0] == 1 and eng.environments_shape() == (spec.n_sets, spec.n_cells, spec.n_centres)
    last = eng.fetch_samples()
    _same(last["environment_counts"], spec.evaluate(last["occupancy"]))
    # a block recorded without the flag refuses the getter
    eng.run_sampled_async(2, 5)
    with pytest.raises(err, match="environments were not recorded"):
        eng.sample_environments()
    assert "environment_counts" not in eng.fetch_samples()
    # the flag without a spec is refused and takes no slot
    eng.set_environments(None)
    with pytest.raises(err, match="call smolmc_set_environments first"):
        eng.run_sampled_async(1, 5, environments=True)
    assert eng.pending_samples()[0] == 0
    eng.close()


# ---- statistics --------------------------------------------------------------------------------------------------------
def _same_record(got, want, what=""):
    for f in st._ARRAYS:
        g, w = getattr(got, f), getattr(want, f)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, f)
        np.testing.assert_array_equal(g, w, err_msg=f"{what} {f}")


def test_statistics_read_the_environment_cells(clean_env):
    from smol_amd.engine import EngineError
    from tests.test_gpu_statistics import _run_blocks, _semigrand

    R = 6
    eng, obs, sc = _semigrand("fcc_prim222_aliased", R)
    pat = Patterns.from_supercell(sc, obs)
    eng.set_patterns(pat)  # (the environment cells lie behind the pattern cells)
    spec = Environments.from_supercell(sc, obs, distances=[shell_lengths(sc)[0]])
    eng.set_environments(spec)
    rows = np.zeros(eng._mu_shape())
    rows[:, 0, 1] = np.linspace(-0.2, 0.2, R)
    temps = np.linspace(2500.0, 4000.0, R)
    occ0 = _rand_occ(sc, np.random.default_rng(9), R)
    seeds = np.arange(R, dtype=np.uint64) + np.uint64(21)
    nc = spec.n_cells
    hit = np.flatnonzero(spec.evaluate(_rand_occ(sc, np.random.default_rng(1), 40)).any(axis=0))
    assert len(hit) >= 3
    cols = [st.ENTHALPY, st.environment(int(hit[0])), st.environment(int(hit[-1])), st.kind(obs, 1), st.pattern(3),
            st.environment(int(hit[1]))]
    hist = (st.environment(int(hit[1])), 64, 0.0, 1.0)
    even, odd = np.array([[0, 1], [2, 3], [4, 5]]), np.array([[1, 2], [3, 4]])
    records = {}
    for what, stat in (("point", Statistics.by_state_point(cols, n_levels=4, hist=hist)),
                       ("walker", Statistics.per_walker(cols, n_levels=4, hist=hist))):
        eng.set_walker_mu(rows)  # (the walkers' points are named afresh: point p is walker p)
        eng.set_state(occ0, seeds, temps)
        eng.set_statistics(stat)
        keys = []

        def exchange(i):
            if i > 0:  # every pair accepted: even pairs, then odd pairs, ...
                pairs = even if i % 2 else odd
                eng.exchange_grid(pairs, np.full(len(pairs), -np.inf))
            keys.append(eng.state_points()[0].copy())

        # blocks without the environment column: the record reads a hidden one
        blocks = _run_blocks(eng, sizes=(3, 4, 2, 6, 5), thin=7, before_block=exchange, observables=True, occupancy=True)
        want = StatisticsRecord(stat, R)
        for i, b in enumerate(blocks):
            assert "environment_counts" not in b
            want.offer(b["enthalpy"], b["features"], b["species_counts"], keys[i] if what == "point" else None,
                       patterns=pat.evaluate(b["occupancy"]), environments=spec.evaluate(b["occupancy"]))
        _same_record(eng.statistics(), want, what + " hidden")
        b = eng.run_sampled(4, 7, statistics=True, environments=True, patterns=True, observables=True, occupancy=False)
        want.offer(b["enthalpy"], b["features"], b["species_counts"], keys[-1] if what == "point" else None,
                   patterns=b["pattern_counts"], environments=b["environment_counts"])
        _same_record(eng.statistics(), want, what + " column")
        records[what] = eng.statistics()
    assert not np.array_equal(records["point"].s1, records["walker"].s1)
    assert (records["walker"].s1[:, [1, 2, 5]] != 0).any()
    # smolmc_update_statistics counts the environments of the current states first
    stat = Statistics.per_walker([st.environment(int(c)) for c in hit[:32]], n_levels=2)
    eng.set_statistics(stat)
    want = StatisticsRecord(stat, R)
    for n in (40, 25):
        eng.run(n)
        eng.update_statistics()
        s = eng.get_state()
        want.offer(s["enthalpy"], s["features"], patterns=pat.evaluate(s["occupancy"]), environments=spec.evaluate(s["occupancy"]))
        _same_record(eng.statistics(), want, "update")
    # a change of the spec while the record names its cells is refused; one cell beyond the spec is no source
    with pytest.raises((EngineError, ValueError), match="statistics record with environment columns"):
        eng.set_environments(None)
    with pytest.raises((EngineError, ValueError), match="statistics record with environment columns"):
        eng.set_environments(spec)
    with pytest.raises((EngineError, ValueError), match="statistics record with environment columns"):
        eng.set_patterns(None)  # (the sources of the environment cells lie behind the pattern cells)
    assert eng.environments_shape() == (spec.n_sets, nc, spec.n_centres)
    _same(eng.environments(occ0), spec.evaluate(occ0))
    with pytest.raises((EngineError, ValueError), match=f"outside the {nc} cells"):
        eng.set_statistics(Statistics.per_walker([st.environment(nc)]))
    top = 1 + eng.F + obs.n_kinds + pat.n_cells + nc
    with pytest.raises((EngineError, ValueError), match=f"source {top + 1}, outside 0..{top} .*{nc} environment cells"):
        eng.set_statistics(Statistics.per_walker([top + 1]))
    eng.set_statistics(None)
    eng.set_environments(None)
    with pytest.raises((EngineError, ValueError), match=f"source {top}, outside 0..{top - nc} "):
        eng.set_statistics(Statistics.per_walker([top]))  # (no spec: the range ends where it ends without)
    eng.close()


# ---- the refusals ------------------------------------------------------------------------------------------------------
def _refused(eng, width, na, nb, cmaps, nmaps, centres, rows, n_sets=None):
    """smolmc_set_environments on raw arrays: the call must fail; its message."""
    s = capi.smolmc_environments()
    i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)  # noqa: E731
    w, a, b = i32(width), i32(na), i32(nb)
    ca, cb = i32(np.stack([np.asarray(m) for m in cmaps])), i32(np.stack([np.asarray(m) for m in nmaps]))
    ptr = np.concatenate(([0], np.cumsum([len(c) for c in centres]))).astype(np.int64)
    cen = i32(np.concatenate([np.asarray(c).reshape(-1) for c in centres] + [np.zeros(1)]))
    nbr = i32(np.concatenate([np.asarray(r).reshape(-1) for r in rows] + [np.zeros(1)]))
    P = lambda x, ct=C.c_int32: x.ctypes.data_as(C.POINTER(ct))  # noqa: E731
    s.n_sets = len(width) if n_sets is None else n_sets
    s.width, s.n_centre_classes, s.n_neigh_classes = P(w), P(a), P(b)
    s.centre_class_of_kind, s.neigh_class_of_kind = P(ca), P(cb)
    s.centre_ptr, s.centres, s.neighbours = P(ptr, C.c_int64), P(cen), P(nbr)
    assert eng._lib.smolmc_set_environments(eng._h, C.byref(s)) != 0
    return eng._lib.smolmc_last_error().decode()


def test_refusals_name_their_reason_and_leave_the_spec(clean_env):
    from smol_amd import synth
    from smol_amd.engine import Engine, EngineError

    err = (EngineError, ValueError)
    eng, _, tab = _engine("fcc3_indicator_skew", 2)
    sc, _, spec = case_spec("fcc3_indicator_skew")
    obs = Observables.from_supercell(sc, tables=tab)
    ident, one = np.arange(3), np.zeros(3)
    cen, row = [0, 59], np.array([[1, 2], [3, -1]])
    raw = lambda **kw: _refused(eng, **{**dict(width=[2], na=[3], nb=[3], cmaps=[ident], nmaps=[ident], centres=[cen], rows=[row]), **kw})  # noqa: E731
    assert "no observables set" in raw()
    with pytest.raises(err, match="call set_observables first"):
        eng.set_environments(spec)
    eng.set_observables(obs)
    eng.set_environments(spec)
    pool = _rand_occ(sc, np.random.default_rng(2), 3)
    want = spec.evaluate(pool)

    def in_force():
        assert eng.environments_shape() == (spec.n_sets, spec.n_cells, spec.n_centres)
        _same(eng.environments(pool), want)

    assert "n_sets must be 1..8, got 0" in raw(n_sets=0)
    assert "n_sets must be 1..8, got 9" in raw(width=[2] * 9, na=[1] * 9, nb=[1] * 9, cmaps=[one] * 9, nmaps=[one] * 9, centres=[cen] * 9,
                                               rows=[row] * 9)
    assert "set 0 has width 0, outside 1..64" in raw(width=[0])
    assert "set 0 has width 65, outside 1..64" in raw(width=[65], rows=[np.zeros((2, 65))], nb=[1], nmaps=[one])
    assert "set 0 has 0 centre classes, outside 1..15" in raw(na=[0], cmaps=[one - 1])
    assert "set 0 has 16 centre classes, outside 1..15" in raw(na=[16])
    assert "set 0 has 0 neighbour classes, outside 1..4" in raw(nb=[0], nmaps=[one - 1])
    assert "set 0 has 5 neighbour classes, outside 1..4" in raw(nb=[5])
    msg = raw(cmaps=[[0, 3, 1]])
    assert "set 0 maps kind 1 to centre class 3, outside -1..2" in msg and "class out of range" in msg
    msg = raw(nmaps=[[0, 1, -2]])
    assert "set 0 maps kind 2 to neighbour class -2, outside -1..2" in msg and "class out of range" in msg
    msg = raw(centres=[[0, 60]])
    assert "set 0 centre 1 is site 60, 60 sites" in msg and "site out of range" in msg
    assert "centre 0 is site -1" in raw(centres=[[-1, 0]])
    msg = raw(rows=[np.array([[1, 2], [60, -1]])])
    assert "set 0 centre 1 slot 0 names site 60, 60 sites" in msg and "site out of range" in msg
    assert "slot 1 names site -2" in raw(rows=[np.array([[1, -2], [3, -1]])])
    assert "more than SMOLMC_MAX_ENV_CELLS = 4096 cells" in raw(width=[12], na=[2], cmaps=[[0, 1, 1]], rows=[np.zeros((2, 12))])
    in_force()
    # the observables may not change under the spec
    with pytest.raises(err, match="while an environment spec rests on the kinds"):
        eng.set_observables(obs)
    with pytest.raises(err, match="while an environment spec rests on the kinds"):
        eng.set_observables(None)
    in_force()
    # ... nor the spec under a block that waits, or under a record that names its cells (test_ring_discipline,
    # test_statistics_read_the_environment_cells); the Python side refuses a spec on other kinds or other sites
    with pytest.raises(ValueError, match="maps 2 kinds, the observables in force have 3"):
        eng.set_environments(Environments.from_rows(Observables(np.zeros(60, np.int32), 2), cen, row))
    with pytest.raises(ValueError, match="defined on 8 sites"):
        eng.set_environments(Environments.from_rows(Observables(np.zeros(8, np.int32), 3), [0], row[:1]))
    bad = pool.copy()
    bad[1, 5] = 3
    with pytest.raises(err, match="out of range"):
        eng.environments(bad)
    in_force()
    eng.close()
    # a launch that does not fit LDS: 21952 sites, the row, its classes and 4096 cells of either spec fit (60 KB), both do
    # not -- whichever comes second is refused and the first stays
    big = synth.build_supercell(synth.build_cluster_model(synth.fcc_prim(), {2: 3.0}), [28, 28, 28])
    eng = Engine(capi.TableSet.from_synth(big, synth.random_coefs(big.model), feature_mode=INT), capi.make_config(1))
    obs = Observables.from_supercell(big)
    eng.set_observables(obs)
    pat = Patterns(obs, [PatternSet(np.array([[0, 1], [5, 21951]]), np.array([0, 1], np.int32), 64)])
    env = Environments(obs, [EnvironmentSet([0, 21951], np.array([[1, 2, 3, -1, 5, 6, 7], [0, 1, 2, 3, 4, 5, 6]]), [0, 0], 1, [0, 1], 4)])
    small = Environments(obs, [EnvironmentSet([0, 21951], np.array([[1, 2], [21950, -1]]), [0, 1], 2, [0, 1], 2)])
    assert pat.n_cells == env.n_cells == 4096
    occ = _rand_occ(big, np.random.default_rng(4), 2)
    eng.set_patterns(pat)
    with pytest.raises(err, match="environments: a launch takes .* 65536 at most"):
        eng.set_environments(env)
    assert eng.environments_shape() == (0, 0, 0) and eng.patterns_shape() == (1, 4096)
    eng.set_environments(small)
    _same(eng.environments(occ), small.evaluate(occ))
    _same(eng.patterns(occ), pat.evaluate(occ))
    eng.set_patterns(None)
    eng.set_environments(env)
    _same(eng.environments(occ), env.evaluate(occ))
    with pytest.raises(err, match="patterns: with the environment spec in force a launch takes .* 65536 at most"):
        eng.set_patterns(pat)
    assert eng.patterns_shape() == (0, 0) and eng.environments_shape() == (1, 4096, 2)
    _same(eng.environments(occ), env.evaluate(occ))
    eng.close()


# ---- the sampler ---------------------------------------------------------------------------------------------------
def _sampler(with_spec, nw=6, **kw):
    c = load_case("rocksalt333_two_sublattices")
    ens = moca.Ensemble.from_cluster_expansion(c["sc"], c["coefs"])
    _, obs, spec = case_spec("rocksalt333_two_sublattices")
    s = moca.Sampler.from_ensemble(ens, temperature=3000.0, nwalkers=nw, seeds=list(range(3, 3 + nw)), rank=0, world_size=1,
                                   observables=obs, environments=spec if with_spec else None, **kw)
    return s, ens, spec, _rand_occ(c["sc"], np.random.default_rng(12), nw)


def test_sampler_traces_the_environments(clean_env, tmp_path):
    plain, ens, spec, occ = _sampler(False)
    counted, _, _, _ = _sampler(True)
    plain.run(12 * 9, occ, thin_by=9)
    counted.run(12 * 9, occ, thin_by=9)
    p, c = plain.samples, counted.samples
    assert c.num_samples == 12 and c.traced_values[-1] == "environment_counts" and "environment_counts" not in p.traced_values
    for name in p.traced_values:
        assert np.array_equal(p.get_trace_value(name, flat=False), c.get_trace_value(name, flat=False)), name
    cells = c.get_environment_counts(flat=False)
    _same(cells, spec.evaluate(c.get_occupancies(flat=False)))
    c.to_npz(tmp_path / "c.npz")
    back = moca.SampleContainer.from_npz(tmp_path / "c.npz", ens)
    _same(back.get_environment_counts(flat=False), cells)
    assert back.metadata["environments"] == spec.describe()
    with pytest.raises(ValueError, match="no environment_counts trace"):
        p.get_environment_counts()
    # keep_occupancy=False, then a second run: the chain goes on where the kept-occupancy sampler's does
    dry, _, _, _ = _sampler(True)
    dry.run(12 * 9, occ, thin_by=9, keep_occupancy=False)
    d = dry.samples
    with pytest.raises(ValueError, match="keep_occupancy=False"):
        d.get_occupancies()
    dry.run(5 * 9, thin_by=9, keep_occupancy=False)
    counted.run(5 * 9, thin_by=9)
    assert d.num_samples == c.num_samples == 17
    for name in ("enthalpy", "features", "accepted", "species_counts", "pair_counts", "environment_counts"):
        assert np.array_equal(d.get_trace_value(name, flat=False), c.get_trace_value(name, flat=False)), name
    np.testing.assert_array_equal(d.last_occupancy(), c.last_occupancy())
    _same(c.get_environment_counts(flat=False), spec.evaluate(c.get_occupancies(flat=False)))
