"""Patterns on the device (the census in csrc/observables.hip; smolmc_set_patterns, smolmc_eval_patterns, the
SMOLMC_SAMPLE_PATTERNS column of the sample ring, the pattern columns of a statistics record): every cell equals
patterns.Patterns.evaluate, the NumPy definition, entry for entry -- int32 on both sides, no tolerance -- and a run with
patterns is the same chain as a run without."""

import ctypes as C

import numpy as np
import pytest

from smol_amd import capi, moca
from smol_amd import statistics as st
from smol_amd.observables import Observables
from smol_amd.patterns import Patterns, PatternSet
from smol_amd.statistics import Statistics, StatisticsRecord
from tests.cases import load_case, tables_for
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


def _big_orbits(sc):
    return [o.id for o in sc.model.orbits if o.size >= 3]


# ---- smolmc_eval_patterns --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fcc_prim666_triplets", "fcc3_indicator_skew", "fcc_prim222_aliased",
                                  "rocksalt333_two_sublattices"])
def test_eval_equals_the_definition(name, clean_env):
    """216 sites, binary triplets: 8 cells a set, the lanes' packed counters; 60 sites (below a wavefront, no multiple of 16), ternary
    triplets: 27 cells, a histogram per wave; 8 sites whose tuples repeat sites and rows; tuples across two sublattices of
    different widths with class = species code.  1, 3 and all occupancies, then the walkers' own states."""
    R = 3
    eng, sc, tab = _engine(name, R)
    obs = Observables.from_supercell(sc, tables=tab)
    spec = Patterns.from_supercell(sc, obs, orbits=_big_orbits(sc)[:8])
    if name == "fcc_prim666_triplets":
        assert all(s.n_cells == 8 for s in spec.sets)
    if name == "fcc3_indicator_skew":
        assert sc.num_sites == 60 and all(s.n_cells == 27 for s in spec.sets)
    if name == "fcc_prim222_aliased":
        # (the aliased cell lists rows twice; its triplets name no site twice, so a third set does: every other row of the
        # second, its last site replaced by its first)
        twice = spec.sets[1].sites.copy()
        twice[::2, 2] = twice[::2, 0]
        spec = Patterns(obs, spec.sets + [PatternSet(twice, spec.sets[1].class_of_kind, spec.sets[1].n_classes)])
        assert any(len(np.unique(s.sites, axis=0)) < len(s.sites) for s in spec.sets)
        assert any((np.sort(s.sites, axis=1)[:, 1:] == np.sort(s.sites, axis=1)[:, :-1]).any() for s in spec.sets)
    if name == "rocksalt333_two_sublattices":
        widths = np.array([sc.model.prim.nspecies[b] for b in sc.site_b])
        assert any(len(set(widths[s.sites[0]].tolist())) > 1 for s in spec.sets)
    assert eng.patterns_shape() == (0, 0)
    eng.set_observables(obs)
    eng.set_patterns(spec)
    assert eng.patterns_shape() == (spec.n_sets, spec.n_cells)
    rng = np.random.default_rng(17)
    pool = _rand_occ(sc, rng, 130)
    want = spec.evaluate(pool)
    assert want.any(axis=0).sum() > spec.n_sets  # (several cells of every kind of set are hit)
    for nocc in (1, 3, 130):
        _same(eng.patterns(pool[:nocc]), want[:nocc])
    # occ = NULL: the walkers' current states, after a short run
    occ = pool[:R].copy()
    eng.set_state(occ, np.arange(R, dtype=np.uint64) + np.uint64(5), 2500.0)
    eng.run(300, sync=True)
    state = eng.get_state()
    assert not np.array_equal(state["occupancy"], occ)
    _same(eng.patterns(), spec.evaluate(state["occupancy"]))
    # the observables' own answers are what they are without a pattern spec
    with_spec = eng.observables(pool[:5])
    eng.set_patterns(None)
    assert eng.patterns_shape() == (0, 0)
    for a, b in zip(with_spec, eng.observables(pool[:5])):
        np.testing.assert_array_equal(a, b)
    with pytest.raises((RuntimeError, ValueError), match="no pattern spec set"):
        eng.patterns(pool[:1])
    eng.close()


def _ternary(R=2):
    """The 60-site ternary handle with kinds per site class (six kinds) set as its observables."""
    eng, sc, tab = _engine("fcc3_indicator_skew", R)
    obs = Observables.from_supercell(sc, site_classes=np.arange(sc.num_sites) % 2)
    assert sc.num_sites == 60 and obs.n_kinds == 6
    eng.set_observables(obs)
    return eng, sc, obs


def _check(eng, spec, pool):
    eng.set_patterns(spec)
    assert eng.patterns_shape() == (spec.n_sets, spec.n_cells)
    want = spec.evaluate(pool)
    _same(eng.patterns(pool), want)
    return want


def test_synthetic_sets(clean_env):
    eng, sc, obs = _ternary()
    N = sc.num_sites
    rng = np.random.default_rng(23)
    pool = _rand_occ(sc, rng, 9)
    code = (Patterns.class_map(obs, "code"))
    assert code[1] == 3
    tup = lambda n, m: rng.integers(0, N, size=(n, m))  # noqa: E731
    # arities 4 and 5 (records of 8 and of 16 bytes) and 8; every tuple count around a wavefront and a workgroup
    for n in (0, 1, 63, 64, 65, 257):
        spec = Patterns(obs, [PatternSet(tup(n, 4), code[0], 3), PatternSet(tup(n, 5), code[0], 3),
                              PatternSet(tup(n, 8), np.array([0, 1, 1, 0, 1, 1], np.int32), 2), PatternSet(tup(n, 1), code[0], 3),
                              PatternSet(tup(n, 3), np.array([0, 0, 1, 0, 0, 1], np.int32), 2)])
        want = _check(eng, spec, pool)
        for t in range(spec.n_sets):
            assert (want[:, spec.cell_ptr[t]:spec.cell_ptr[t + 1]].sum(axis=1) == n).all()  # (every site counted, every kind a class)
    # 3^5 = 243 cells: a histogram per wave; 3^7 = 2187: the shared copy
    for m, per_wave in ((5, True), (7, False)):
        spec = Patterns(obs, [PatternSet(tup(700, m), code[0], 3)])
        assert spec.n_cells == 3 ** m and (4 * spec.n_cells <= capi.MAX_PATTERN_CELLS) == per_wave
        want = _check(eng, spec, pool)
        assert (want > 1).any()  # (cells hit more than once: the adds meet)
    # ... and a set of few cells next to so many cells that the lanes' counts are added to the shared copy
    spec = Patterns(obs, [PatternSet(tup(700, 7), code[0], 3), PatternSet(tup(300, 2), np.array([0, 1, 1, 0, 1, 1], np.int32), 2)])
    _check(eng, spec, pool)
    # sets of few cells with more than 255 tuples a lane (256 lanes): the lanes' packed counts are added in between
    spec = Patterns(obs, [PatternSet(tup(255 * 256 + 700, 2), np.array([0, 1, 1, 0, 1, 1], np.int32), 2),
                          PatternSet(tup(2 * 255 * 256 + 3, 1), code[0], 3), PatternSet(tup(255 * 256, 4), np.array([0, 1, 1, 0, 1, 1], np.int32), 2)])
    assert all(s.n_cells <= 16 for s in spec.sets)
    _check(eng, spec, pool[:3])
    # four classes over the six kinds, arity 6: 4096 cells exactly
    four = np.array([0, 1, 2, 3, 1, 2], np.int32)
    spec = Patterns(obs, [PatternSet(tup(900, 6), four, 4)])
    assert spec.n_cells == capi.MAX_PATTERN_CELLS
    _check(eng, spec, pool)
    # ... and one more cell is refused: the spec in force stays
    msg = _refused(eng, [6, 1], [4, 1], [four, np.zeros(6)], [tup(2, 6), tup(2, 1)])
    assert "more than SMOLMC_MAX_PATTERN_CELLS = 4096 cells" in msg
    assert eng.patterns_shape() == (1, 4096)
    _same(eng.patterns(pool[:2]), spec.evaluate(pool[:2]))
    # eight sets with eight different maps in one spec, neighbours with equal maps among them
    maps = [rng.integers(0, 3, size=6).astype(np.int32) for _ in range(6)]
    maps = [maps[0], maps[0], maps[1], maps[2], maps[2], maps[3], maps[4], maps[5]]
    spec = Patterns(obs, [PatternSet(tup(90 + 7 * t, 1 + t % 4), maps[t], 3) for t in range(8)])
    _check(eng, spec, pool)
    eng.close()


def test_skipped_tuples(clean_env):
    """A map with -1 and every third site left out: each set both counts and skips tuples."""
    eng, sc, _ = _ternary()
    full = Observables.from_supercell(sc, site_classes=np.arange(sc.num_sites) % 2)
    kb = full.kind_base.copy()
    kb[::3] = -1
    obs = Observables(kb, full.n_kinds, site_ncodes=full.site_ncodes)
    eng.set_observables(obs)
    rng = np.random.default_rng(29)
    pool = _rand_occ(sc, rng, 7)
    cmap = np.array([0, -1, 1, 1, 0, -1], np.int32)
    sets = [PatternSet(rng.integers(0, sc.num_sites, size=(300, m)), cmap, 2) for m in (2, 3, 5)]
    spec = Patterns(obs, sets)
    want = _check(eng, spec, pool)
    for t, s in enumerate(sets):
        counted = want[:, spec.cell_ptr[t]:spec.cell_ptr[t + 1]].sum(axis=1)
        assert (counted > 0).all() and (counted < s.n_tuples).all()
    eng.close()


def test_relabelled_handle_takes_the_callers_numbering(clean_env):
    """The restricted-sites recipe of test_gpu_capi_relabel: the engine renumbers the sites; the tuples go in by the
    caller's numbers."""
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
    spec = Patterns.from_supercell(sc, obs, orbits=_big_orbits(sc)[:4], classes="kind")
    eng.set_patterns(spec)
    pool = _rand_occ(sc, np.random.default_rng(8), 3)
    _same(eng.patterns(pool), spec.evaluate(pool))
    eng.set_state(occ, np.arange(R, dtype=np.uint64) + np.uint64(9), 4000.0)
    eng.run(200, sync=True)
    _same(eng.patterns(), spec.evaluate(eng.get_state()["occupancy"]))
    smp = eng.run_sampled(2, 9, patterns=True)
    _same(smp["pattern_counts"], spec.evaluate(smp["occupancy"]))
    eng.close()


# ---- the ring --------------------------------------------------------------------------------------------------------
def _ring_handle(R, with_spec=True):
    eng, sc, tab = _engine("fcc_prim666_triplets", R)
    obs = Observables.from_supercell(sc, tables=tab)
    eng.set_observables(obs)
    spec = Patterns.from_supercell(sc, obs)
    if with_spec:
        eng.set_patterns(spec)
    occ = (np.random.default_rng(21).random((R, sc.num_sites)) < 0.5).astype(np.int32)
    eng.set_state(occ, np.arange(R, dtype=np.uint64) + np.uint64(31), 3000.0)
    return eng, obs, spec, occ


@pytest.mark.parametrize("R", [1, 130])
def test_ring_column_equals_the_definition_on_the_blocks_occupancies(R, clean_env):
    eng, obs, spec, occ = _ring_handle(R)
    eng.run(11)
    smp = eng.run_sampled(3, 7, patterns=True)
    assert "species_counts" not in smp and smp["occupancy"].shape == (3, R, eng.N)
    _same(smp["pattern_counts"], spec.evaluate(smp["occupancy"]))
    both = eng.run_sampled(2, 7, patterns=True, observables=True)
    _same(both["pattern_counts"], spec.evaluate(both["occupancy"]))
    for got, want in zip((both["species_counts"], both["pair_counts"]), obs.evaluate(both["occupancy"])):
        _same(got, want)
    # without the occupancy column: the same cells, the rows stay on the device
    eng.set_state(occ, np.arange(R, dtype=np.uint64) + np.uint64(31), 3000.0)
    eng.run(11)
    eng.run_sampled_async(3, 7, occupancy=False, patterns=True)
    npend, ns, flags = eng.pending_samples()
    assert (npend, ns) == (1, 3) and flags & capi.SAMPLE_PATTERNS and not flags & capi.SAMPLE_OCCUPANCY
    fn = eng._lib.smolmc_debug_block_bytes
    fn.restype, fn.argtypes = C.c_longlong, [C.c_void_p]
    up = lambda x: (x + 255) & ~255  # noqa: E731
    rows = 3 * R
    assert fn(eng._h) == up(rows * 8) + up(rows * eng.F * 8) + up(rows) + up(rows * spec.n_cells * 4)
    dry = eng.fetch_samples()
    assert dry["occupancy"] is None
    _same(dry["pattern_counts"], smp["pattern_counts"])
    np.testing.assert_array_equal(dry["enthalpy"], smp["enthalpy"])
    eng.close()


def test_chains_and_observables_do_not_change(clean_env):
    """Same seeds with and without the flag: identical samples, final state and counters; the counts and pairs of a block
    recorded with the observables' flag are the same bits with and without a pattern spec set."""
    got = []
    for mode in ("no spec", "spec, no flag", "flag"):
        eng, obs, spec, occ = _ring_handle(5, with_spec=mode != "no spec")
        eng.run(13)
        kw = dict(patterns=True) if mode == "flag" else {}
        blocks = [eng.run_sampled(4, 9, observables=True, **kw), eng.run_sampled(2, 5, observables=True, **kw)]
        got.append((blocks, eng.get_state()))
        eng.close()
    (plain, st0) = got[0]
    for blocks, state in got[1:]:
        for p, c in zip(plain, blocks):
            for key in p:
                assert p[key].dtype == c[key].dtype and np.array_equal(p[key], c[key]), key
        for key in st0:
            assert np.array_equal(st0[key], state[key]), key
    assert all("pattern_counts" in b for b in got[2][0]) and not any("pattern_counts" in b for b in got[1][0])
    assert {"n_steps", "n_accepted"} <= set(st0)


def test_ring_discipline(clean_env):
    from smol_amd.engine import EngineError, RingFullError

    eng, obs, spec, occ = _ring_handle(4)
    err = (EngineError, ValueError)
    eng.run_sampled_async(2, 5, patterns=True)
    eng.run_sampled_async(3, 4, patterns=True, occupancy=False)  # (two blocks in flight)
    # the getter reads the block the next fetch delivers, and does not deliver it
    c0 = eng.sample_patterns()
    assert c0.shape == (2, 4, spec.n_cells) and eng.pending_samples()[:2] == (2, 2)
    np.testing.assert_array_equal(c0, eng.sample_patterns())
    with pytest.raises(RingFullError, match="sample ring full"):
        eng.run_sampled_async(1, 5, patterns=True)
    a = eng.fetch_samples()
    _same(c0, spec.evaluate(a["occupancy"]))
    _same(a["pattern_counts"], c0)
    c1 = eng.sample_patterns()
    assert c1.shape == (3, 4, spec.n_cells) and eng.pending_samples()[:2] == (1, 3)
    b = eng.fetch_samples()
    assert b["occupancy"] is None
    _same(b["pattern_counts"], c1)
    # a new spec while a counted block waits: refused; the block and the spec stay
    eng.run_sampled_async(1, 3, patterns=True)
    with pytest.raises(err, match="waits in the ring"):
        eng.set_patterns(spec)
    with pytest.raises(err, match="waits in the ring"):
        eng.set_patterns(None)
    assert eng.pending_samples()[0] == 1 and eng.patterns_shape() == (spec.n_sets, spec.n_cells)
    last = eng.fetch_samples()
    _same(last["pattern_counts"], spec.evaluate(last["occupancy"]))
    # a block recorded without the flag refuses the getter
    eng.run_sampled_async(2, 5)
    with pytest.raises(err, match="patterns were not recorded"):
        eng.sample_patterns()
    assert "pattern_counts" not in eng.fetch_samples()
    # the flag without a spec is refused and takes no slot
    eng.set_patterns(None)
    with pytest.raises(err, match="call smolmc_set_patterns first"):
        eng.run_sampled_async(1, 5, patterns=True)
    assert eng.pending_samples()[0] == 0
    eng.close()


# ---- statistics --------------------------------------------------------------------------------------------------------
def _same_record(got, want, what=""):
    for f in st._ARRAYS:
        g, w = getattr(got, f), getattr(want, f)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, f)
        np.testing.assert_array_equal(g, w, err_msg=f"{what} {f}")


def test_statistics_read_the_pattern_cells(clean_env):
    from smol_amd.engine import EngineError
    from tests.test_gpu_statistics import _run_blocks, _semigrand

    R = 6
    eng, obs, sc = _semigrand("fcc_prim222_aliased", R)
    spec = Patterns.from_supercell(sc, obs)
    eng.set_patterns(spec)
    rows = np.zeros(eng._mu_shape())
    rows[:, 0, 1] = np.linspace(-0.2, 0.2, R)
    temps = np.linspace(2500.0, 4000.0, R)
    occ0 = _rand_occ(sc, np.random.default_rng(9), R)
    seeds = np.arange(R, dtype=np.uint64) + np.uint64(21)
    nc = spec.n_cells
    cols = [st.ENTHALPY, st.pattern(0), st.pattern(nc - 1), st.kind(obs, 1), st.pattern(3)]
    even, odd = np.array([[0, 1], [2, 3], [4, 5]]), np.array([[1, 2], [3, 4]])
    records = {}
    for what, stat in (("point", Statistics.by_state_point(cols, n_levels=4, hist=(st.pattern(3), 64, 0.0, 1.0))),
                       ("walker", Statistics.per_walker(cols, n_levels=4, hist=(st.pattern(3), 64, 0.0, 1.0)))):
        eng.set_walker_mu(rows)  # (the walkers' points are named afresh: point p is walker p)
        eng.set_state(occ0, seeds, temps)
        eng.set_statistics(stat)
        keys = []

        def exchange(i):
            if i > 0:  # every pair accepted: even pairs, then odd pairs, ...
                pairs = even if i % 2 else odd
                eng.exchange_grid(pairs, np.full(len(pairs), -np.inf))
            keys.append(eng.state_points()[0].copy())

        # blocks with the pattern column and blocks without: then the record reads a hidden one
        blocks = _run_blocks(eng, sizes=(3, 4, 2, 6, 5), thin=7, before_block=exchange, observables=True, occupancy=True)
        want = StatisticsRecord(stat, R)
        for i, b in enumerate(blocks):
            assert "pattern_counts" not in b
            want.offer(b["enthalpy"], b["features"], b["species_counts"], keys[i] if what == "point" else None,
                       patterns=spec.evaluate(b["occupancy"]))
        _same_record(eng.statistics(), want, what + " hidden")
        b = eng.run_sampled(4, 7, statistics=True, patterns=True, observables=True, occupancy=False)
        want.offer(b["enthalpy"], b["features"], b["species_counts"], keys[-1] if what == "point" else None,
                   patterns=b["pattern_counts"])
        _same_record(eng.statistics(), want, what + " column")
        records[what] = eng.statistics()
    assert not np.array_equal(records["point"].s1, records["walker"].s1)
    # smolmc_update_statistics counts the patterns of the current states first
    stat = Statistics.per_walker([st.pattern(c) for c in range(min(nc, 32))], n_levels=2)
    eng.set_statistics(stat)
    want = StatisticsRecord(stat, R)
    for n in (40, 25):
        eng.run(n)
        eng.update_statistics()
        s = eng.get_state()
        want.offer(s["enthalpy"], s["features"], patterns=spec.evaluate(s["occupancy"]))
        _same_record(eng.statistics(), want, "update")
    # a change of the spec while the record names its cells is refused; one cell beyond the spec is no source
    with pytest.raises((EngineError, ValueError), match="statistics record with pattern columns"):
        eng.set_patterns(None)
    assert eng.patterns_shape() == (spec.n_sets, nc)
    with pytest.raises((EngineError, ValueError), match=f"outside the {nc} cells"):
        eng.set_statistics(Statistics.per_walker([st.pattern(nc)]))
    top = 1 + eng.F + obs.n_kinds + nc
    with pytest.raises((EngineError, ValueError), match=f"source {top + 1}, outside 0..{top} .*{nc} pattern cells"):
        eng.set_statistics(Statistics.per_walker([top + 1]))
    eng.set_statistics(None)
    eng.set_patterns(None)
    with pytest.raises((EngineError, ValueError), match=f"source {top}, outside 0..{top - nc} "):
        eng.set_statistics(Statistics.per_walker([top]))  # (no spec: the range ends where it ends without)
    eng.close()


# ---- the refusals ------------------------------------------------------------------------------------------------------
def _refused(eng, arity, n_classes, maps, tuples, n_sets=None):
    """smolmc_set_patterns on raw arrays: the call must fail; its message."""
    s = capi.smolmc_patterns()
    ar, nc = np.ascontiguousarray(arity, dtype=np.int32), np.ascontiguousarray(n_classes, dtype=np.int32)
    cm = np.ascontiguousarray(np.stack([np.asarray(m) for m in maps]), dtype=np.int32)
    ptr = np.concatenate(([0], np.cumsum([len(t) for t in tuples]))).astype(np.int64)
    sites = np.ascontiguousarray(np.concatenate([np.asarray(t).reshape(-1) for t in tuples] + [np.zeros(1)]), dtype=np.int32)
    P = lambda a, ct: a.ctypes.data_as(C.POINTER(ct))  # noqa: E731
    s.n_sets = len(arity) if n_sets is None else n_sets
    s.arity, s.n_classes, s.class_of_kind = P(ar, C.c_int32), P(nc, C.c_int32), P(cm, C.c_int32)
    s.tuple_ptr, s.sites = P(ptr, C.c_int64), P(sites, C.c_int32)
    assert eng._lib.smolmc_set_patterns(eng._h, C.byref(s)) != 0
    return eng._lib.smolmc_last_error().decode()


def test_refusals_name_their_reason_and_leave_the_spec(clean_env):
    from smol_amd import synth
    from smol_amd.engine import Engine, EngineError

    err = (EngineError, ValueError)
    eng, sc, tab = _engine("fcc3_indicator_skew", 2)
    obs = Observables.from_supercell(sc, tables=tab)
    ident = np.arange(3)
    tri = np.array([[0, 1, 2], [3, 4, 59]])
    assert "no observables set" in _refused(eng, [3], [3], [ident], [tri])
    with pytest.raises(err, match="call set_observables first"):
        eng.set_patterns(Patterns.from_tuples(obs, [tri]))
    eng.set_observables(obs)
    spec = Patterns.from_supercell(sc, obs)
    eng.set_patterns(spec)
    pool = _rand_occ(sc, np.random.default_rng(2), 3)
    want = spec.evaluate(pool)

    def in_force():
        assert eng.patterns_shape() == (spec.n_sets, spec.n_cells)
        _same(eng.patterns(pool), want)

    assert "n_sets must be 1..8, got 0" in _refused(eng, [3], [3], [ident], [tri], n_sets=0)
    assert "n_sets must be 1..8, got 9" in _refused(eng, [1] * 9, [3] * 9, [ident] * 9, [tri[:, :1]] * 9)
    assert "set 0 has arity 0, outside 1..8" in _refused(eng, [0], [3], [ident], [tri])
    assert "set 1 has arity 9, outside 1..8" in _refused(eng, [3, 9], [3, 3], [ident, ident], [tri, np.zeros((1, 9))])
    assert "set 0 has 0 classes, outside 1..255" in _refused(eng, [3], [0], [ident * 0 - 1], [tri])
    assert "set 0 has 256 classes, outside 1..255" in _refused(eng, [1], [256], [ident], [tri[:, :1]])
    msg = _refused(eng, [3], [3], [[0, 3, 1]], [tri])
    assert "set 0 maps kind 1 to class 3, outside -1..2" in msg and "class out of range" in msg
    assert "maps kind 2 to class -2" in _refused(eng, [3], [3], [[0, 1, -2]], [tri])
    msg = _refused(eng, [3], [3], [ident], [np.array([[0, 1, 2], [3, 60, 4]])])
    assert "set 0 tuple 1 names site 60, 60 sites" in msg and "site out of range" in msg
    assert "names site -1" in _refused(eng, [3], [3], [ident], [np.array([[0, -1, 2]])])
    assert "more than SMOLMC_MAX_PATTERN_CELLS = 4096 cells" in _refused(eng, [8], [3], [ident], [np.zeros((1, 8))])
    in_force()
    # the observables may not change under the spec
    with pytest.raises(err, match="while a pattern spec rests on the kinds"):
        eng.set_observables(obs)
    with pytest.raises(err, match="while a pattern spec rests on the kinds"):
        eng.set_observables(None)
    in_force()
    # ... nor the spec under a block that waits, or under a record that names its cells (test_ring_discipline,
    # test_statistics_read_the_pattern_cells); the Python side refuses a spec on other kinds or other sites
    with pytest.raises(ValueError, match="maps 2 kinds, the observables in force have 3"):
        eng.set_patterns(Patterns.from_tuples(Observables(np.zeros(60, np.int32), 2), [tri]))
    with pytest.raises(ValueError, match="defined on 8 sites"):
        eng.set_patterns(Patterns.from_tuples(Observables(np.zeros(8, np.int32), 3), [tri[:1]]))
    bad = pool.copy()
    bad[1, 5] = 3
    with pytest.raises(err, match="out of range"):
        eng.patterns(bad)
    in_force()
    eng.close()
    # a launch that does not fit LDS: 50653 sites, the row and its classes side by side
    big = synth.build_supercell(synth.build_cluster_model(synth.fcc_prim(), {2: 3.0}), [37, 37, 37])
    eng = Engine(capi.TableSet.from_synth(big, synth.random_coefs(big.model), feature_mode=INT), capi.make_config(1))
    obs = Observables.from_supercell(big)
    eng.set_observables(obs)
    with pytest.raises(err, match="65536 at most"):
        eng.set_patterns(Patterns.from_tuples(obs, [tri]))
    assert eng.patterns_shape() == (0, 0)
    eng.close()


# ---- the sampler ---------------------------------------------------------------------------------------------------
def _sampler(with_patterns, nw=6, **kw):
    c = load_case("rocksalt333_two_sublattices")
    ens = moca.Ensemble.from_cluster_expansion(c["sc"], c["coefs"])
    obs = Observables.from_supercell(c["sc"])
    spec = Patterns.from_supercell(c["sc"], obs, orbits=_big_orbits(c["sc"])[:3])
    s = moca.Sampler.from_ensemble(ens, temperature=3000.0, nwalkers=nw, seeds=list(range(3, 3 + nw)), rank=0, world_size=1,
                                   observables=obs, patterns=spec if with_patterns else None, **kw)
    return s, ens, spec, _rand_occ(c["sc"], np.random.default_rng(12), nw)


def test_sampler_traces_the_patterns(clean_env, tmp_path):
    plain, ens, spec, occ = _sampler(False)
    counted, _, _, _ = _sampler(True)
    plain.run(12 * 9, occ, thin_by=9)
    counted.run(12 * 9, occ, thin_by=9)
    p, c = plain.samples, counted.samples
    assert c.num_samples == 12 and c.traced_values[-1] == "pattern_counts" and "pattern_counts" not in p.traced_values
    for name in p.traced_values:
        assert np.array_equal(p.get_trace_value(name, flat=False), c.get_trace_value(name, flat=False)), name
    cells = c.get_pattern_counts(flat=False)
    _same(cells, spec.evaluate(c.get_occupancies(flat=False)))
    np.testing.assert_array_equal(c.pattern_probabilities(flat=False), spec.probabilities(cells))
    c.to_npz(tmp_path / "c.npz")
    back = moca.SampleContainer.from_npz(tmp_path / "c.npz", ens)
    _same(back.get_pattern_counts(flat=False), cells)
    assert back.metadata["patterns"] == spec.describe()
    # keep_occupancy=False, then a second run: the chain goes on where the kept-occupancy sampler's does
    dry, _, _, _ = _sampler(True)
    dry.run(12 * 9, occ, thin_by=9, keep_occupancy=False)
    d = dry.samples
    with pytest.raises(ValueError, match="keep_occupancy=False"):
        d.get_occupancies()
    dry.run(5 * 9, thin_by=9, keep_occupancy=False)
    counted.run(5 * 9, thin_by=9)
    assert d.num_samples == c.num_samples == 17
    for name in ("enthalpy", "features", "accepted", "species_counts", "pair_counts", "pattern_counts"):
        assert np.array_equal(d.get_trace_value(name, flat=False), c.get_trace_value(name, flat=False)), name
    np.testing.assert_array_equal(d.last_occupancy(), c.last_occupancy())
    _same(c.get_pattern_counts(flat=False), spec.evaluate(c.get_occupancies(flat=False)))


def test_sampler_exchange_run_by_state_point(clean_env):
    from smol_amd import synth

    model = synth.build_cluster_model(synth.rocksalt_prim(), {2: 3.5})
    sc = synth.build_supercell(model, [3, 3, 3])
    ens = moca.Ensemble.from_cluster_expansion(sc, synth.random_coefs(model, seed=5, scale=0.05))
    names = ens.species
    ens.chemical_potentials = {names[0]: 0.1, names[1]: -0.2, names[2]: 0.05}
    temps = [3000.0, 3600.0, 4500.0]
    mus = [{names[0]: 0.1, names[1]: -0.2 + dm, names[2]: 0.05} for dm in np.linspace(-0.15, 0.15, 4)]
    nw = 12
    obs = Observables.from_supercell(sc)
    rng = np.random.default_rng(2)
    spec = Patterns.from_tuples(obs, [rng.integers(0, sc.size, size=(80, 3)), rng.integers(0, sc.num_sites, size=(50, 4))], classes="code")
    stat = Statistics.by_state_point([st.ENTHALPY, st.pattern(1), st.pattern(spec.n_cells - 2)], n_levels=2)
    sampler = moca.Sampler.from_ensemble(ens, temperature=3000.0, nwalkers=nw, seeds=list(range(11, 11 + nw)), observables=obs,
                                         patterns=spec, statistics=stat)
    occ = np.zeros((nw, ens.num_sites), dtype=np.int32)
    occ[:, : sc.size] = rng.integers(0, 3, size=(nw, sc.size))
    gx = sampler.run_exchange(8, 200, occ, thin_by=100, grid=dict(temperatures=temps, chemical_potentials=mus, seed=4))
    assert 0 < gx.acceptance
    box = sampler.samples
    cells = box.get_pattern_counts(flat=False)
    _same(cells, spec.evaluate(box.get_occupancies(flat=False)))
    by = box.by_state_point("pattern_counts")  # (points, samples, n_cells)
    point = box.get_trace_value("state_point", flat=False)[:, :, 0].astype(np.int64)
    assert by.shape == (nw, 16, spec.n_cells) and not np.array_equal(point, np.broadcast_to(np.arange(nw), point.shape))
    for s in range(16):
        np.testing.assert_array_equal(by[point[s], s], cells[s])
    # the record by state point averages the chains of the points (the bound of test_gpu_statistics: 4 n eps d)
    rec = sampler.statistics
    n = by.shape[1]
    assert (rec.n == n).all()
    for j, cell in ((1, 1), (2, spec.n_cells - 2)):
        x = by[:, :, cell].astype(np.float64)
        d = np.abs(x - x[:, :1]).max(axis=1)
        assert (np.abs(rec.mean()[:, j] - x.mean(axis=1)) <= 4 * n * np.finfo(float).eps * d).all()
