"""Observables on the device (csrc/observables.hip; smolmc_set_observables, smolmc_eval_observables, the
SMOLMC_SAMPLE_OBSERVABLES columns of the sample ring): every count equals observables.Observables.evaluate, the NumPy
definition, entry for entry -- int32 on both sides, no tolerance -- and a run with observables is the same chain as a
run without."""

import ctypes as C

import numpy as np
import pytest

from smol_amd import capi, moca
from smol_amd.observables import Observables
from tests.cases import load_case, tables_for

pytestmark = pytest.mark.gpu
INT, CORR = capi.FEATURES_INTERACTIONS, capi.FEATURES_CORRELATIONS
ENV = ("SMOLMC_FORCE_GENERAL", "SMOLMC_FORCE_UNIVERSAL", "SMOLMC_NO_WL_MULTI", "SMOLMC_LAUNCH_CHUNK", "SMOLMC_NO_INKERNEL_BIAS",
       "SMOLMC_NO_LAZY_FEATURES", "SMOLMC_NO_SITE_RELABEL")


def _rand_occ(sc, rng, n):
    nsp = np.array([sc.model.prim.nspecies[b] for b in sc.site_b])
    return (rng.random((n, sc.num_sites)) * nsp).astype(np.int32)


def _same(got, want):
    for g, w in zip(got, want):
        assert g.dtype == np.int32 and g.shape == w.shape
        np.testing.assert_array_equal(g, w)


@pytest.fixture
def clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


# ---- smolmc_eval_observables ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fcc_conv444_pairs", "fcc3_indicator_skew", "fcc_prim222_aliased",
                                  "rocksalt333_two_sublattices", "rocksalt333_vacancy_ewald"])
def test_eval_equals_the_definition(name, clean_env):
    """256 sites on a lean handle; 60 sites (N below a wavefront, 9 cells per shell, bond counts that are no multiple of
    256); 8 sites with duplicate and self bonds; kinds across two sublattices (25 cells per shell: the per-wave
    histograms); a fixed sublattice with a one-kind block.  1, 3 and 130 occupancies, then the walkers' own states."""
    from smol_amd.engine import Engine

    sc = load_case(name)["sc"]
    tab = tables_for(name, INT)
    R = 3
    eng = Engine(tab, capi.make_config(R, capi.KERNEL_METROPOLIS, capi.STEP_SWAP))
    obs = Observables.from_supercell(sc, tables=tab)
    assert eng.observables_shape() == (0, 0)
    eng.set_observables(obs)
    assert eng.observables_shape() == (obs.n_kinds, obs.n_shells)
    rng = np.random.default_rng(17)
    pool = _rand_occ(sc, rng, 130)
    want = obs.evaluate(pool)
    for nocc in (1, 3, 130):
        _same(eng.observables(pool[:nocc]), (want[0][:nocc], want[1][:nocc]))
    # occ = NULL: the walkers' current states, after a run
    occ = pool[:R].copy()
    if name == "fcc_conv444_pairs":
        occ = (rng.random((R, sc.num_sites)) < 0.5).astype(np.int32)
    eng.set_state(occ, np.arange(R, dtype=np.uint64) + np.uint64(5), 2500.0)
    eng.run(300, sync=True)
    st = eng.get_state()
    assert not np.array_equal(st["occupancy"], occ)
    _same(eng.observables(), obs.evaluate(st["occupancy"]))
    # sites left out and kinds chosen by the user: two classes of sites, every third site not counted
    classes = np.arange(sc.num_sites) % 2
    custom = Observables.from_supercell(sc, site_classes=classes)
    kb = custom.kind_base.copy()
    kb[::3] = -1
    custom = Observables(kb, custom.n_kinds, custom.shells, site_ncodes=custom.site_ncodes)
    eng.set_observables(custom)
    assert eng.observables_shape() == (custom.n_kinds, custom.n_shells)
    _same(eng.observables(pool[:7]), custom.evaluate(pool[:7]))
    # counts without any shell
    eng.set_observables(Observables(obs.kind_base, obs.n_kinds, site_ncodes=obs.site_ncodes))
    counts, pairs = eng.observables(pool[:5])
    assert pairs.shape == (5, 0, obs.n_kinds, obs.n_kinds)
    np.testing.assert_array_equal(counts, want[0][:5])
    eng.set_observables(None)
    assert eng.observables_shape() == (0, 0)
    with pytest.raises((RuntimeError, ValueError), match="no observables set"):
        eng.observables(pool[:1])
    eng.close()


def test_many_kinds_take_the_shared_histogram(clean_env):
    """18 site classes of a binary alloy: 36 kinds, 1296 cells per shell, 2592 in all -- more than fit one histogram per
    wave, and more than 16 kinds (the atomic form of the kind counts)."""
    from smol_amd.engine import Engine

    name = "fcc_conv444_pairs"
    sc = load_case(name)["sc"]
    eng = Engine(tables_for(name, INT), capi.make_config(2))
    base = Observables.from_supercell(sc)
    obs = Observables.from_supercell(sc, site_classes=np.arange(sc.num_sites) % 18, orbits=base.shell_orbit_ids[:2])
    assert obs.n_kinds == 36 and 4 * obs.n_shells * 36 * 36 > capi.MAX_OBS_CELLS
    eng.set_observables(obs)
    pool = _rand_occ(sc, np.random.default_rng(4), 9)
    _same(eng.observables(pool), obs.evaluate(pool))
    # ... and 5 classes: 10 kinds, 100 cells per shell -- atomics on a histogram per wave, ballots for the kind counts
    obs = Observables.from_supercell(sc, site_classes=np.arange(sc.num_sites) % 5)
    eng.set_observables(obs)
    _same(eng.observables(pool), obs.evaluate(pool))
    # ... and 300 shells of a binary alloy, 1200 cells of four per shell: ballots, the waves' sums added to one histogram
    obs = Observables(base.kind_base, 2, [base.shells[k % 4][(7 * k) % 400:(7 * k) % 400 + 301] for k in range(300)],
                      site_ncodes=base.site_ncodes)
    assert all(len(b) == 301 for b in obs.shells)
    assert 4 * obs.n_shells * 4 > capi.MAX_OBS_CELLS
    eng.set_observables(obs)
    _same(eng.observables(pool), obs.evaluate(pool))
    eng.close()


def test_relabelled_handle_takes_and_gives_the_callers_numbering(clean_env):
    """The restricted-sites recipe of test_gpu_capi_relabel: the engine renumbers the sites; kinds, bonds and occupancies
    go in by the caller's numbers."""
    from smol_amd.engine import Engine
    from tests.test_gpu_capi_relabel import _model

    sc, ens, tab, occ, frozen = _model(capi.STEP_SWAP)
    R = len(occ)
    eng = Engine(tab, capi.make_config(R, capi.KERNEL_METROPOLIS, capi.STEP_SWAP))
    assert "relabelled=1" in eng.kernel_info(), eng.kernel_info()
    # the frozen cations are a site class of their own: kinds that follow the CALLER's site numbers
    classes = np.zeros(sc.num_sites, dtype=np.int64)
    classes[frozen] = 1
    obs = Observables.from_supercell(sc, site_classes=classes)
    eng.set_observables(obs)
    pool = _rand_occ(sc, np.random.default_rng(8), 3)
    _same(eng.observables(pool), obs.evaluate(pool))
    eng.set_state(occ, np.arange(R, dtype=np.uint64) + np.uint64(9), 4000.0)
    eng.run(200, sync=True)
    _same(eng.observables(), obs.evaluate(eng.get_state()["occupancy"]))
    smp = eng.run_sampled(2, 9, observables=True)
    _same((smp["species_counts"], smp["pair_counts"]), obs.evaluate(smp["occupancy"]))
    eng.close()


# ---- the ring --------------------------------------------------------------------------------------------------------
def _handle(which, R, monkeypatch):
    """(engine, observables, initial occupancies, run_sampled keywords) of one of the ring's paths."""
    from smol_amd.engine import Engine

    rng = np.random.default_rng(21)
    kw = {}
    if which in ("lean", "universal"):
        name = "fcc_conv444_pairs"
        if which == "universal":
            monkeypatch.setenv("SMOLMC_FORCE_UNIVERSAL", "1")
        sc = load_case(name)["sc"]
        tab = tables_for(name, INT)
        cfg = capi.make_config(R, capi.KERNEL_METROPOLIS, capi.STEP_SWAP)
        occ = (rng.random((R, sc.num_sites)) < 0.5).astype(np.int32)
        want = "universal" if which == "universal" else "lean"
    elif which == "wang-landau":  # the snapshot path: one launch and one snapshot per sample
        from oracle import oracle as orc

        name = "fcc_conv444_pairs"
        sc = load_case(name)["sc"]
        tab = tables_for(name, INT)
        occ = np.tile((rng.random((1, sc.num_sites)) < 0.5).astype(np.int32), (R, 1))
        ev = orc.OracleEvaluator(tab)
        h0 = float(ev.feature_vector(occ[0]) @ ev.natural_parameters())
        cfg = capi.make_config(R, capi.KERNEL_WANGLANDAU, capi.STEP_SWAP, min_enthalpy=h0 - 6.1, max_enthalpy=h0 + 5.3,
                               bin_size=0.21, check_period=40, flatness=0.2)
        kw, want = dict(wl=True), ""
    elif which == "lazy":
        name = "rocksalt333_two_sublattices"
        sc = load_case(name)["sc"]
        tab = tables_for(name, CORR)
        cfg = capi.make_config(R, capi.KERNEL_METROPOLIS, capi.STEP_SWAP)
        occ = _rand_occ(sc, rng, R)
        want = "lazy-features"
    else:  # a biased handle on mc_kernel: the snapshot path again, with the bias column
        from tests.v6_cases import CASE, SPECS, build

        monkeypatch.setenv("SMOLMC_FORCE_GENERAL", "1")
        tab, cfg, occ0, temp = build("BG_sqc_swap_int", n_replicas=R)
        sc = load_case(CASE[SPECS["BG_sqc_swap_int"]["case"]])["sc"]
        occ = np.tile(occ0, (R, 1))
        kw, want = dict(bias=True), "general"
    eng = Engine(tab, cfg)
    assert want in eng.kernel_info(), eng.kernel_info()
    obs = Observables.from_supercell(sc, tables=tab)
    eng.set_observables(obs)
    eng.set_state(occ, np.arange(R, dtype=np.uint64) + np.uint64(31), 0.0 if which == "wang-landau" else 3000.0)
    return eng, obs, occ, kw


@pytest.mark.parametrize("R", [1, 130])
@pytest.mark.parametrize("which", ["lean", "wang-landau", "lazy", "universal", "biased-general"])
def test_ring_columns_equal_the_definition_on_the_blocks_occupancies(which, R, clean_env):
    eng, obs, occ, kw = _handle(which, R, clean_env)
    eng.run(11)
    smp = eng.run_sampled(3, 7, observables=True, **kw)
    assert smp["occupancy"].shape == (3, R, eng.N)
    assert len({smp["occupancy"][i].tobytes() for i in range(3)}) == 3 or R == 1  # (the samples differ: the chain moves)
    _same((smp["species_counts"], smp["pair_counts"]), obs.evaluate(smp["occupancy"]))
    # without the occupancy column: the same counts, the rows stay on the device
    eng.set_state(occ, np.arange(R, dtype=np.uint64) + np.uint64(31), 0.0 if which == "wang-landau" else 3000.0)
    eng.run(11)
    eng.run_sampled_async(3, 7, occupancy=False, observables=True, **kw)
    npend, ns, flags = eng.pending_samples()
    assert (npend, ns) == (1, 3) and flags & capi.SAMPLE_OBSERVABLES and not flags & capi.SAMPLE_OCCUPANCY
    H = np.empty((3, R))
    rows = np.empty((3, R, eng.N), dtype=np.uint8)
    P = lambda a, ct: a.ctypes.data_as(C.POINTER(ct))  # noqa: E731
    assert eng._lib.smolmc_get_samples_u8(eng._h, P(H, C.c_double), None, None, P(rows, C.c_uint8)) != 0
    assert b"occupancies were not recorded" in eng._lib.smolmc_last_error()
    assert eng.pending_samples()[0] == 1  # (the refused fetch delivered nothing)
    dry = eng.fetch_samples()
    assert dry["occupancy"] is None
    _same((dry["species_counts"], dry["pair_counts"]), (smp["species_counts"], smp["pair_counts"]))
    np.testing.assert_array_equal(dry["enthalpy"], smp["enthalpy"])
    eng.close()


def test_block_without_occupancy_downloads_no_occupancy_rows(clean_env):
    """The `used` bytes of a block are what its download moves (smolmc_debug_block_bytes: the block the next fetch
    delivers).  Columns are 256-byte aligned ranges of one arena: enthalpy, features, accepted, [occupancy], counts,
    pairs.  Without the occupancy column the rows lie behind the downloaded part."""
    eng, obs, occ, kw = _handle("lean", 130, clean_env)
    fn = eng._lib.smolmc_debug_block_bytes
    fn.restype, fn.argtypes = C.c_longlong, [C.c_void_p]
    R, N, F, ns = 130, eng.N, eng.F, 3
    rows = ns * R
    up = lambda x: (x + 255) & ~255  # noqa: E731
    cols = up(rows * 8) + up(rows * F * 8) + up(rows) + up(rows * obs.n_kinds * 4) + up(rows * obs.n_shells * obs.n_kinds ** 2 * 4)
    npad = (N + 15) // 16 * 16
    assert fn(eng._h) == -1
    eng.run_sampled_async(ns, 7, occupancy=False, observables=True)
    assert fn(eng._h) == cols
    a = eng.fetch_samples()
    eng.set_state(occ, np.arange(R, dtype=np.uint64) + np.uint64(31), 3000.0)
    eng.run_sampled_async(ns, 7, occupancy=True, observables=True)
    assert fn(eng._h) == cols + up(rows * npad)
    b = eng.fetch_samples()
    _same((a["species_counts"], a["pair_counts"]), (b["species_counts"], b["pair_counts"]))
    eng.close()


def test_chains_do_not_change(clean_env):
    """Same seeds with and without the flag: identical enthalpies, features, accepted flags, occupancies and final state."""
    for which in ("lean", "lazy", "wang-landau"):
        got = []
        for with_obs in (False, True):
            eng, obs, occ, kw = _handle(which, 5, clean_env)
            eng.run(13)
            blocks = [eng.run_sampled(4, 9, observables=with_obs, **kw), eng.run_sampled(2, 5, observables=with_obs, **kw)]
            got.append((blocks, eng.get_state()))
            eng.close()
        (plain, st0), (counted, st1) = got
        for p, c in zip(plain, counted):
            for key in p:
                assert np.array_equal(p[key], c[key]), (which, key)
            assert "species_counts" in c and "species_counts" not in p
        for key in st0:
            assert np.array_equal(st0[key], st1[key]), (which, key)


def test_ring_discipline(clean_env):
    from smol_amd.engine import EngineError, RingFullError

    eng, obs, occ, kw = _handle("lean", 4, clean_env)
    eng.run_sampled_async(2, 5, observables=True)
    eng.run_sampled_async(3, 4, observables=True)
    # the getter reads the block the next fetch delivers, and does not deliver it
    c0, p0 = eng.sample_observables()
    assert c0.shape == (2, 4, obs.n_kinds) and eng.pending_samples()[:2] == (2, 2)
    c0b, _ = eng.sample_observables()
    np.testing.assert_array_equal(c0, c0b)
    with pytest.raises(RingFullError, match="sample ring full"):
        eng.run_sampled_async(1, 5, observables=True)
    assert eng._lib.smolmc_run_sampled(eng._h, 1, 5, capi.SAMPLE_OBSERVABLES) == capi.ERR_RING_FULL
    a = eng.fetch_samples()
    _same((c0, p0), obs.evaluate(a["occupancy"]))
    _same((a["species_counts"], a["pair_counts"]), (c0, p0))
    c1, p1 = eng.sample_observables()
    assert c1.shape == (3, 4, obs.n_kinds) and eng.pending_samples()[:2] == (1, 3)
    b = eng.fetch_samples()
    _same((c1, p1), obs.evaluate(b["occupancy"]))
    # new observables while a counted block waits: refused; the block stays
    eng.run_sampled_async(1, 3, observables=True)
    with pytest.raises((EngineError, ValueError), match="waits in the ring"):
        eng.set_observables(obs)
    assert eng.pending_samples()[0] == 1
    eng.fetch_samples()
    # a block recorded without the flag refuses the getter
    eng.run_sampled_async(2, 5)
    with pytest.raises((EngineError, ValueError), match="observables were not recorded"):
        eng.sample_observables()
    plain = eng.fetch_samples()
    assert "species_counts" not in plain
    # the flag without observables is refused and takes no slot
    eng.set_observables(None)
    with pytest.raises((EngineError, ValueError), match="call smolmc_set_observables first"):
        eng.run_sampled_async(1, 5, observables=True)
    assert eng.pending_samples()[0] == 0
    eng.close()


def test_refusals_name_their_reason(clean_env):
    from smol_amd.engine import Engine, EngineError

    name = "fcc_conv444_pairs"
    sc = load_case(name)["sc"]
    eng = Engine(tables_for(name, INT), capi.make_config(2))
    obs = Observables.from_supercell(sc)
    lib, N = eng._lib, sc.num_sites

    def refused(kind_base, n_kinds, shell_ptr, bonds, n_shells):
        s = capi.smolmc_observables()
        kb, sp, bo = (np.ascontiguousarray(kind_base, dtype=np.int32), np.ascontiguousarray(shell_ptr, dtype=np.int64),
                      np.ascontiguousarray(bonds, dtype=np.int32))
        s.n_kinds, s.n_shells = n_kinds, n_shells
        s.kind_base = kb.ctypes.data_as(C.POINTER(C.c_int32))
        s.shell_ptr = sp.ctypes.data_as(C.POINTER(C.c_int64))
        s.bonds = bo.ctypes.data_as(C.POINTER(C.c_int32))
        assert lib.smolmc_set_observables(eng._h, C.byref(s)) != 0
        return lib.smolmc_last_error().decode()

    eng.set_observables(obs)
    kb = obs.kind_base
    assert "bond 1 = (3, 256) out of range (256 sites)" in refused(kb, 2, [0, 2], [[0, 1], [3, N]], 1)
    assert "bond 0 = (-1, 2) out of range" in refused(kb, 2, [0, 1], [[-1, 2]], 1)
    msg = refused(np.where(np.arange(N) == 7, 1, 0), 2, [0, 1], [[0, 1]], 1)
    assert "kind_base[7] + site_ncodes = 1 + 2 is larger than n_kinds = 2" in msg and "kind out of range" in msg
    msg = refused(kb, 33, [0, 1, 2, 3, 4], [[0, 1]] * 4, 4)
    assert "4356 cells, larger than SMOLMC_MAX_OBS_CELLS = 4096" in msg
    assert "n_kinds must be 1..254" in refused(kb, 255, [0], np.zeros((0, 2)), 0)
    assert "shell_ptr must be ascending from 0" in refused(kb, 2, [0, 2, 1], [[0, 1], [1, 2]], 2)
    # every refusal left the observables as they were
    assert eng.observables_shape() == (obs.n_kinds, obs.n_shells)
    pool = _rand_occ(sc, np.random.default_rng(2), 2)
    _same(eng.observables(pool), obs.evaluate(pool))
    bad = pool.copy()
    bad[1, 5] = 2
    with pytest.raises((EngineError, ValueError), match="out of range"):
        eng.observables(bad)
    with pytest.raises(ValueError, match="defined on 8 sites"):
        eng.set_observables(Observables(np.zeros(8, np.int32), 2))
    eng.close()
    # a row too long to stage in LDS next to the histograms: 50653 sites and 4096 cells
    from smol_amd import synth

    big = synth.build_supercell(synth.build_cluster_model(synth.fcc_prim(), {2: 3.0}), [37, 37, 37])
    tab = capi.TableSet.from_synth(big, synth.random_coefs(big.model), feature_mode=INT)
    eng = Engine(tab, capi.make_config(1))
    cells = Observables(np.zeros(big.num_sites, np.int32), 32, [np.array([[0, 1]])] * 4, site_ncodes=np.full(big.num_sites, 2))
    with pytest.raises((EngineError, ValueError), match="too long to stage in LDS"):
        eng.set_observables(cells)
    eng.set_observables(Observables.from_supercell(big))  # (four cells: fits)
    occ = _rand_occ(big, np.random.default_rng(1), 2)
    _same(eng.observables(occ), Observables.from_supercell(big).evaluate(occ))
    eng.close()


# ---- the sampler ---------------------------------------------------------------------------------------------------
def _sampler(obs_on, nw=6):
    c = load_case("rocksalt333_two_sublattices")
    ens = moca.Ensemble.from_cluster_expansion(c["sc"], c["coefs"])
    obs = Observables.from_supercell(c["sc"])
    s = moca.Sampler.from_ensemble(ens, temperature=3000.0, nwalkers=nw, seeds=list(range(3, 3 + nw)), rank=0, world_size=1,
                                   observables=obs if obs_on else None)
    return s, obs, _rand_occ(c["sc"], np.random.default_rng(12), nw)


def test_sampler_traces_and_compositions(clean_env):
    plain, obs, occ = _sampler(False)
    counted, _, _ = _sampler(True)
    plain.run(12 * 9, occ, thin_by=9)
    counted.run(12 * 9, occ, thin_by=9)
    p, c = plain.samples, counted.samples
    assert c.num_samples == 12 and "species_counts" in c.traced_values and "species_counts" not in p.traced_values
    for name in p.traced_values:
        assert np.array_equal(p.get_trace_value(name, flat=False), c.get_trace_value(name, flat=False)), name
    want = obs.evaluate(c.get_occupancies(flat=False))
    _same((c.get_trace_value("species_counts", flat=False), c.get_pair_counts(flat=False)), want)
    assert all(c._counted_on_device(sub, 0, 1) is not None for sub in c.sublattices)
    assert c.mean_composition() == p.mean_composition() and c.composition_variance() == p.composition_variance()
    assert c.mean_composition(discard=2, thin_by=3) == p.mean_composition(discard=2, thin_by=3)
    assert c.warren_cowley(flat=False).shape == (12, 6, obs.n_shells, obs.n_kinds, obs.n_kinds)
    # keep_occupancy=False, then a second run: the chain goes on exactly where the kept-occupancy sampler's does
    dry, _, _ = _sampler(True)
    dry.run(12 * 9, occ, thin_by=9, keep_occupancy=False)
    d = dry.samples
    assert d.num_samples == 12
    np.testing.assert_array_equal(d.last_occupancy(), c.last_occupancy())
    with pytest.raises(ValueError, match="keep_occupancy=False"):
        d.get_occupancies()
    for name in ("enthalpy", "features", "accepted", "species_counts", "pair_counts"):
        assert np.array_equal(d.get_trace_value(name, flat=False), c.get_trace_value(name, flat=False)), name
    assert d.mean_composition() == c.mean_composition()
    dry.run(5 * 9, thin_by=9, keep_occupancy=False)
    counted.run(5 * 9, thin_by=9)
    assert d.num_samples == c.num_samples == 17
    for name in ("enthalpy", "features", "accepted", "species_counts", "pair_counts"):
        assert np.array_equal(d.get_trace_value(name, flat=False), c.get_trace_value(name, flat=False)), name
    np.testing.assert_array_equal(d.last_occupancy(), c.last_occupancy())
    # ... and from a fresh handle, through last_occupancy (the path a restored container takes)
    dry._resume_at = None
    counted._resume_at = None
    dry.run(3 * 9, thin_by=9, keep_occupancy=False)
    counted.run(3 * 9, thin_by=9)
    assert np.array_equal(d.get_enthalpies(flat=False), c.get_enthalpies(flat=False))
    np.testing.assert_array_equal(d.last_occupancy(), c.last_occupancy())
