"""Structure factors on the device (csrc/structure.hip; smolmc_set_structure, smolmc_eval_structure, the
SMOLMC_SAMPLE_STRUCTURE columns of the sample ring, the intensity columns of the statistics record): every amplitude equals
structure.StructureFactor.evaluate, the NumPy definition, entry for entry -- int64 on both sides -- every intensity is the
same float64, and a run with the flag is the same chain as a run without."""

import ctypes as C

import numpy as np
import pytest

from smol_amd import capi, moca
from smol_amd import statistics as st
from smol_amd.observables import Observables
from smol_amd.statistics import Statistics, StatisticsRecord
from smol_amd.structure import StructureFactor, commensurate_points
from tests.cases import load_case, tables_for
from tests.test_gpu_observables import ENV, _rand_occ
from tests.test_gpu_statistics import _same_record, _semigrand

pytestmark = pytest.mark.gpu
INT = capi.FEATURES_INTERACTIONS
ERR = (RuntimeError, ValueError)


@pytest.fixture
def clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def _same(got, want):
    (ga, gi), (wa, wi) = got, want
    assert ga.dtype == np.int64 and ga.shape == wa.shape and gi.dtype == np.float64 and gi.shape == wi.shape
    np.testing.assert_array_equal(ga, wa)
    np.testing.assert_array_equal(gi, wi)  # (exact float64 equality)


def _some_intensities(sf_points, K, rng, n=12):
    Q = len(sf_points)
    its = [(0, 0, 0)] + [(int(rng.integers(Q)), int(rng.integers(K)), int(rng.integers(K))) for _ in range(n - 1)]
    return its


def _plan(eng):
    """The kernel the spec in force takes, in the words of ``capi.structure_plan``."""
    fn = eng._lib.smolmc_debug_structure_plan
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p] + [C.POINTER(C.c_int)] * 3
    m, a, b = C.c_int(), C.c_int(), C.c_int()
    assert fn(eng._h, C.byref(m), C.byref(a), C.byref(b)) == 0
    return ("mask",) if m.value else ("counters", a.value, b.value)


# ---- 1: smolmc_eval_structure ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fcc_conv444_pairs", "fcc3_indicator_skew", "fcc_prim222_aliased",
                                  "rocksalt333_two_sublattices", "rocksalt333_vacancy_ewald"])
def test_eval_equals_the_definition(name, clean_env):
    """All class representatives as points.  8 sites with at most 4 cells per point (N below a wavefront: one word of the
    mask kernel, not full); 3 kinds x up to 60 classes on a skew cell (the counter kernel, a counter set per wave); 256
    sites (four full words); kinds across two sublattices; a fixed sublattice with a one-kind block, and a sublattice left
    out.  1, 3 and 130 occupancies (the mask kernel's workgroups take four rows: a last workgroup with one, three and two),
    then the walkers' own states."""
    from smol_amd.engine import Engine

    sc = load_case(name)["sc"]
    tab = tables_for(name, INT)
    R = 3
    eng = Engine(tab, capi.make_config(R, capi.KERNEL_METROPOLIS, capi.STEP_SWAP))
    rng = np.random.default_rng(17)
    g = commensurate_points(sc)
    K = Observables.default_kind_base(sc)[1]
    sf = StructureFactor.from_supercell(sc, g, intensities=_some_intensities(g, K, rng))
    assert eng.structure_shape() == (0, 0, 0)
    eng.set_structure_factor(sf)
    assert eng.structure_shape() == (sf.n_points, sf.n_kinds, sf.n_intensities) == (sc.size, K, 12)
    if name == "fcc_prim222_aliased":
        assert sf.n_kinds * sf.n_phases == 4 and sc.num_sites < 64 and _plan(eng) == ("mask",)
    if name == "fcc3_indicator_skew":
        # 180 cells: 22 points a pass next to the row's 64 bytes, three passes for the 60 points
        assert sf.n_kinds == 3 and sf.n_phases == 60 and _plan(eng) == ("counters", capi.STRUCT_WAVES, 22)
        assert capi.structure_plan(60, 64, 3, 60, 60) == _plan(eng)
    if name == "fcc_conv444_pairs":
        assert _plan(eng) == ("mask",)
    pool = _rand_occ(sc, rng, 130)
    want = sf.evaluate(pool)
    assert np.any(want[1] != 0)
    for nocc in (1, 3, 130):
        _same(eng.structure_factor(pool[:nocc]), (want[0][:nocc], want[1][:nocc]))
    # occ = NULL: the walkers' current states, after a run
    occ = pool[:R].copy()
    if name == "fcc_conv444_pairs":
        occ = (rng.random((R, sc.num_sites)) < 0.5).astype(np.int32)
    eng.set_state(occ, np.arange(R, dtype=np.uint64) + np.uint64(5), 2500.0)
    eng.run(300, sync=True)
    state = eng.get_state()
    assert not np.array_equal(state["occupancy"], occ)
    _same(eng.structure_factor(), sf.evaluate(state["occupancy"]))
    # kinds chosen by the user, every third site not counted, a whole sublattice (basis site 0) left out
    custom = StructureFactor.from_supercell(sc, g[:5], site_classes=np.arange(sc.num_sites) % 2)
    kb = custom.kind_base.copy()
    kb[::3] = -1
    if sc.model.prim.nb > 1:
        kb[np.asarray(sc.site_b) == 0] = -1
    Kc = custom.n_kinds
    custom = StructureFactor(kb, Kc, custom.phase, custom.table, [(4, Kc - 1, 0), (2, 1, 1)], site_ncodes=custom.site_ncodes, bits=36)
    eng.set_structure_factor(custom)
    assert eng.structure_shape() == (5, Kc, 2)
    _same(eng.structure_factor(pool[:7]), custom.evaluate(pool[:7]))
    # amplitudes without any intensity
    bare = StructureFactor.from_supercell(sc, g[:3])
    eng.set_structure_factor(bare)
    amp, inten = eng.structure_factor(pool[:5])
    assert inten.shape == (5, 0)
    np.testing.assert_array_equal(amp, want[0][:5, :3])
    eng.set_structure_factor(None)
    assert eng.structure_shape() == (0, 0, 0)
    with pytest.raises(ERR, match="no structure-factor spec set"):
        eng.structure_factor(pool[:1])
    eng.close()


def test_thirty_six_kinds(clean_env):
    """18 site classes of a binary alloy on the 256-site cell: 36 kinds x 16 phase classes, the counter kernel; and 4
    classes, 8 kinds x 16 phase classes = 128 cells: the most the mask kernel takes."""
    from smol_amd.engine import Engine

    name = "fcc_conv444_pairs"
    sc = load_case(name)["sc"]
    eng = Engine(tables_for(name, INT), capi.make_config(2))
    g = commensurate_points(sc)
    sf = StructureFactor.from_supercell(sc, g, site_classes=np.arange(sc.num_sites) % 18,
                                        intensities=[(q, a, 35 - a) for q in (0, 9, 63) for a in (0, 17, 35)])
    assert sf.n_kinds == 36 and sf.n_kinds * sf.n_phases > capi.STRUCT_MASK_CELLS
    eng.set_structure_factor(sf)
    assert _plan(eng)[0] == "counters"
    pool = _rand_occ(sc, np.random.default_rng(4), 9)
    _same(eng.structure_factor(pool), sf.evaluate(pool))
    sf = StructureFactor.from_supercell(sc, g, site_classes=np.arange(sc.num_sites) % 4, intensities=[(q, a, 7 - a) for q in (0, 9, 63)
                                                                                                   for a in (0, 3, 7)])
    assert sf.n_kinds * sf.n_phases == capi.STRUCT_MASK_CELLS
    eng.set_structure_factor(sf)
    assert _plan(eng) == ("mask",)
    _same(eng.structure_factor(pool), sf.evaluate(pool))
    # ... and 40 classes at Gamma alone: 80 kinds x 1 phase class, more kinds than a wave has lanes to keep their masks
    # (the four basis sites of the cell are four classes of equal phase at Gamma: one class is given by hand)
    kinds = StructureFactor.from_supercell(sc, g[:1], site_classes=np.arange(sc.num_sites) % 40)
    sf = StructureFactor(kinds.kind_base, kinds.n_kinds, np.zeros((1, sc.num_sites), np.int64), np.array([[[1 << 36, 0]]]),
                         [(0, 3, 3), (0, 79, 64)], site_ncodes=kinds.site_ncodes, bits=36)
    assert sf.n_kinds == 80 and sf.n_phases == 1
    eng.set_structure_factor(sf)
    assert _plan(eng) == ("mask",)
    got = eng.structure_factor(pool)
    _same(got, sf.evaluate(pool))
    assert np.all(got[0][..., 1] == 0) and np.all(got[0][..., 0].sum(axis=-1) == sc.num_sites << 36)
    eng.close()


# ---- 2: the chunk boundaries ---------------------------------------------------------------------------------------------------
def _raw_spec(N, K, M, Q, rng, n_inten=6):
    """A spec made of random numbers: the engine knows no geometry."""
    phase = rng.integers(0, M, size=(Q, N))
    phase[:, :2] = [0, M - 1]
    table = rng.integers(-(1 << 36), (1 << 36) + 1, size=(Q, M, 2))
    its = [(Q - 1, K - 1, 0)] + [(int(rng.integers(Q)), int(rng.integers(K)), int(rng.integers(K))) for _ in range(n_inten - 1)]
    return StructureFactor(np.zeros(N, np.int32), K, phase, table, its, site_ncodes=np.full(N, K), bits=36)


def test_kernel_and_chunk_boundaries(clean_env):
    """On rows of 256 sites in 256 bytes.  Just below and just above: the cell count at which the mask kernel hands over to
    the counter kernel; more (kind, point) pairs than the mask kernel has threads; in the counter kernel a full pass of
    points and one point more; the last cell count with a counter set per wave and the first with one shared set; passes of
    the shared set; the largest cell count (one point per pass)."""
    from smol_amd.engine import Engine

    name = "fcc_conv444_pairs"
    sc = load_case(name)["sc"]
    eng = Engine(tables_for(name, INT), capi.make_config(2))
    N, npad = sc.num_sites, 256
    room, W = capi.STRUCT_LDS_BYTES - npad, capi.STRUCT_WAVES
    K = 2
    m_mask = capi.STRUCT_MASK_CELLS // K               # 64 classes: 128 cells, the last spec of the mask kernel
    q_pass = room // (4 * W * K * (m_mask + 1))        # 31 points of 130 cells fill one pass of the counter kernel
    m_waves = (room // (4 * W)) // K                   # 2040 classes: 4080 cells, the last spec with a set per wave
    q_shared = room // (4 * K * (m_waves + 1))         # 3 points of 4082 cells in one shared set
    m_max = capi.MAX_STRUCT_CELLS // K
    cases = [  # (M, Q, the kernel)
        (8, 128, ("mask",)), (8, 129, ("mask",)),      # 256 and 258 (kind, point) pairs: one pass of the threads, and two
        (m_mask, 3, ("mask",)), (m_mask + 1, 3, ("counters", W, 3)),
        (m_mask + 1, q_pass, ("counters", W, q_pass)), (m_mask + 1, q_pass + 1, ("counters", W, q_pass)),
        (m_waves, 3, ("counters", W, 1)), (m_waves + 1, q_shared, ("counters", 1, q_shared)),
        (m_waves + 1, q_shared + 1, ("counters", 1, q_shared)),
        (m_max, 2, ("counters", 1, 1)),
    ]
    assert (m_mask, q_pass, m_waves, q_shared, m_max) == (64, 31, 2040, 3, 6144)
    rng = np.random.default_rng(6)
    pool = (rng.random((5, N)) < 0.45).astype(np.int32)
    for M, Q, plan in cases:
        sf = _raw_spec(N, K, M, Q, rng)
        assert capi.structure_plan(N, npad, K, M, Q) == plan, (M, Q)
        eng.set_structure_factor(sf)
        assert _plan(eng) == plan, (M, Q, _plan(eng))
        _same(eng.structure_factor(pool), sf.evaluate(pool))
    eng.close()


# ---- 3: the relabelled handle -----------------------------------------------------------------------------------------------------
def test_relabelled_handle_takes_and_gives_the_callers_numbering(clean_env):
    from smol_amd.engine import Engine
    from tests.test_gpu_capi_relabel import _model

    sc, ens, tab, occ, frozen = _model(capi.STEP_SWAP)
    R = len(occ)
    eng = Engine(tab, capi.make_config(R, capi.KERNEL_METROPOLIS, capi.STEP_SWAP))
    assert "relabelled=1" in eng.kernel_info(), eng.kernel_info()
    classes = np.zeros(sc.num_sites, dtype=np.int64)
    classes[frozen] = 1  # kinds that follow the CALLER's site numbers
    g = commensurate_points(sc)[::9]
    rng = np.random.default_rng(8)
    sf = StructureFactor.from_supercell(sc, g, site_classes=classes)
    sf = StructureFactor(sf.kind_base, sf.n_kinds, sf.phase, sf.table, _some_intensities(g, sf.n_kinds, rng), site_ncodes=sf.site_ncodes,
                         bits=36)
    eng.set_structure_factor(sf)
    pool = _rand_occ(sc, rng, 3)
    _same(eng.structure_factor(pool), sf.evaluate(pool))
    eng.set_state(occ, np.arange(R, dtype=np.uint64) + np.uint64(9), 4000.0)
    eng.run(200, sync=True)
    _same(eng.structure_factor(), sf.evaluate(eng.get_state()["occupancy"]))
    smp = eng.run_sampled(2, 9, structure=True)
    _same((smp["structure_amplitudes"], smp["structure_intensities"]), sf.evaluate(smp["occupancy"]))
    eng.close()


# ---- 4: the ring ---------------------------------------------------------------------------------------------------------------------
def _ring_handle(R=3):
    from smol_amd.engine import Engine

    name = "fcc_conv444_pairs"
    sc = load_case(name)["sc"]
    eng = Engine(tables_for(name, INT), capi.make_config(R, capi.KERNEL_METROPOLIS, capi.STEP_SWAP))
    g = commensurate_points(sc)
    sf = StructureFactor.from_supercell(sc, g, intensities=[(q, a, b) for q in (0, 1, 21, 63) for a, b in ((0, 0), (0, 1), (1, 1))])
    eng.set_structure_factor(sf)
    occ = (np.random.default_rng(21).random((R, sc.num_sites)) < 0.5).astype(np.int32)
    seeds = np.arange(R, dtype=np.uint64) + np.uint64(31)
    eng.set_state(occ, seeds, 3000.0)
    return eng, sf, occ, seeds


def test_ring_columns_equal_the_definition_and_the_chain_does_not_change(clean_env):
    R = 3
    eng, sf, occ, seeds = _ring_handle(R)
    eng.run(11)
    smp = eng.run_sampled(3, 7, structure=True)
    assert smp["occupancy"].shape == (3, R, eng.N) and smp["structure_amplitudes"].shape == (3, R, sf.n_points, 2, 2)
    assert len({smp["occupancy"][i].tobytes() for i in range(3)}) == 3
    _same((smp["structure_amplitudes"], smp["structure_intensities"]), sf.evaluate(smp["occupancy"]))
    final = eng.get_state()
    # without the occupancy column: the same columns, the rows stay on the device
    eng.set_state(occ, seeds, 3000.0)
    eng.run(11)
    eng.run_sampled_async(3, 7, occupancy=False, structure=True)
    npend, ns, flags = eng.pending_samples()
    assert (npend, ns) == (1, 3) and flags & capi.SAMPLE_STRUCTURE and not flags & capi.SAMPLE_OCCUPANCY
    dry = eng.fetch_samples()
    assert dry["occupancy"] is None
    _same((dry["structure_amplitudes"], dry["structure_intensities"]), (smp["structure_amplitudes"], smp["structure_intensities"]))
    # a run without the flag: enthalpy, features, accept flags, occupancies and the final state are identical
    eng.set_state(occ, seeds, 3000.0)
    eng.run(11)
    plain = eng.run_sampled(3, 7)
    assert "structure_amplitudes" not in plain
    for key in plain:
        assert np.array_equal(plain[key], smp[key]), key
    for key in ("enthalpy", "features", "accepted"):
        assert np.array_equal(plain[key], dry[key]), key
    after = eng.get_state()
    for key in final:
        assert np.array_equal(final[key], after[key]), key
    eng.close()


def test_ring_discipline(clean_env):
    eng, sf, occ, seeds = _ring_handle(4)
    eng.run_sampled_async(2, 5, structure=True)
    eng.run_sampled_async(3, 4, structure=True)
    # the getter reads the block the next fetch delivers, and does not deliver it
    a0, i0 = eng.sample_structure()
    assert a0.shape == (2, 4, sf.n_points, 2, 2) and i0.shape == (2, 4, sf.n_intensities) and eng.pending_samples()[:2] == (2, 2)
    a = eng.fetch_samples()
    _same((a0, i0), sf.evaluate(a["occupancy"]))
    _same((a["structure_amplitudes"], a["structure_intensities"]), (a0, i0))
    b = eng.fetch_samples()
    assert b["structure_amplitudes"].shape[0] == 3
    _same((b["structure_amplitudes"], b["structure_intensities"]), sf.evaluate(b["occupancy"]))
    assert not np.array_equal(b["occupancy"][0], a["occupancy"][-1])
    # a new spec while a block with the columns waits: refused; the block stays
    eng.run_sampled_async(1, 3, structure=True)
    with pytest.raises(ERR, match="while a block recorded with SMOLMC_SAMPLE_STRUCTURE waits in the ring"):
        eng.set_structure_factor(sf)
    with pytest.raises(ERR, match="while a block recorded with SMOLMC_SAMPLE_STRUCTURE waits in the ring"):
        eng.set_structure_factor(None)
    assert eng.pending_samples()[0] == 1 and eng.structure_shape() == (sf.n_points, 2, sf.n_intensities)
    # discard_samples empties the ring; the spec can be set again
    eng.discard_samples()
    assert eng.pending_samples()[0] == 0
    eng.set_structure_factor(sf)
    # a block recorded without the flag refuses the getter
    eng.run_sampled_async(2, 5)
    with pytest.raises(ERR, match="structure factors were not recorded"):
        eng.sample_structure()
    assert "structure_amplitudes" not in eng.fetch_samples()
    # the flag without a spec is refused and takes no slot
    eng.set_structure_factor(None)
    with pytest.raises(ERR, match="SMOLMC_SAMPLE_STRUCTURE without a structure-factor spec"):
        eng.run_sampled_async(1, 5, structure=True)
    assert eng.pending_samples()[0] == 0
    eng.close()


# ---- 5: statistics with intensity columns -----------------------------------------------------------------------------------------
def _stat_handle(R):
    eng, obs, sc = _semigrand("fcc_conv444_pairs", R)
    g = commensurate_points(sc)
    # the superlattice points of the conventional cell, (1, 0, 0) and (1, 1, 0) in its reciprocal basis: g = 4 x that
    sf = StructureFactor.from_supercell(sc, np.array([[0, 0, 0], [4, 0, 0], [4, 4, 0]]), observables=obs,
                                        intensities=[(1, 1, 1), (2, 0, 1), (0, 1, 1)])
    eng.set_structure_factor(sf)
    return eng, obs, sc, sf


def _spec(by_point=False):
    make = Statistics.by_state_point if by_point else Statistics.per_walker
    return make([st.ENTHALPY, st.intensity(0), st.intensity(1)], n_levels=3, hist=(st.intensity(0), 16, 0.0, 0.03125))


def test_statistics_record_with_intensity_columns(clean_env):
    """256 sites, 70 walkers: where the statistics test found contraction to matter."""
    R = 70
    eng, obs, sc, sf = _stat_handle(R)
    occ0 = _rand_occ(sc, np.random.default_rng(5), R)
    seeds = np.arange(R, dtype=np.uint64) + np.uint64(11)
    spec = _spec()
    eng.set_statistics(spec)
    assert eng.statistics_shape() == (R, 3, 3, 16)
    eng.set_state(occ0, seeds, 3000.0)
    # two blocks queued before the first fetch, the columns fetched with them
    eng.run_sampled_async(3, 5, statistics=True, structure=True)
    eng.run_sampled_async(4, 5, statistics=True, structure=True)
    blocks = [eng.fetch_samples(), eng.fetch_samples()]
    want = StatisticsRecord(spec, R)
    for b in blocks:
        _same((b["structure_amplitudes"], b["structure_intensities"]), sf.evaluate(b["occupancy"]))
        want.offer(b["enthalpy"], b["features"], intensities=b["structure_intensities"])
    got = eng.statistics()
    _same_record(got, want, "two blocks")
    assert (got.n == 7).all() and got.hist.sum() + got.over.sum() == 7 * R and got.hist.sum() > 0 and np.any(got.s2[:, 3] != 0)
    # the same record with nothing but the statistics asked for: rows, amplitudes and intensities stay on the device
    eng.set_statistics(spec)
    eng.set_state(occ0, seeds, 3000.0)
    eng.run_sampled_async(3, 5, statistics=True, occupancy=False)
    eng.run_sampled_async(4, 5, statistics=True, occupancy=False)
    dry = [eng.fetch_samples(), eng.fetch_samples()]
    assert all(d["occupancy"] is None and "structure_intensities" not in d for d in dry)
    _same_record(eng.statistics(), want, "alone")
    # update_statistics after a plain run: one offer of the current states
    for n in (40, 1):
        eng.run(n)
        eng.update_statistics()
        s = eng.get_state()
        want.offer(s["enthalpy"], s["features"], intensities=sf.evaluate(s["occupancy"])[1])
        _same_record(eng.statistics(), want, "update")
    # the spec cannot change under the record
    with pytest.raises(ERR, match="while a statistics record with intensity columns depends on the spec"):
        eng.set_structure_factor(None)
    with pytest.raises(ERR, match="while a statistics record with intensity columns depends on the spec"):
        eng.set_structure_factor(sf)
    _same_record(eng.statistics(), want, "after the refusals")
    # with the record gone the spec can go, and then the intensity sources are out of range again
    eng.set_statistics(None)
    eng.set_structure_factor(None)
    with pytest.raises(ERR, match=f"column 1 has source {2 + eng.F + obs.n_kinds}, outside 0..{1 + eng.F + obs.n_kinds} "):
        eng.set_statistics(Statistics.per_walker([st.ENTHALPY, ("source", 2 + eng.F + obs.n_kinds)]))
    eng.close()


def test_statistics_by_state_point_after_an_exchange(clean_env):
    R = 6
    eng, obs, sc, sf = _stat_handle(R)
    rows = np.zeros(eng._mu_shape())
    rows[:, 0, 1] = np.linspace(-0.2, 0.2, R)
    eng.set_walker_mu(rows)
    eng.set_state(_rand_occ(sc, np.random.default_rng(9), R), np.arange(R, dtype=np.uint64) + np.uint64(21), np.linspace(2500.0, 4000.0, R))
    spec = _spec(by_point=True)
    eng.set_statistics(spec)
    want = StatisticsRecord(spec, R)
    keys = []
    for i, ns in enumerate((3, 4)):
        if i:
            pairs = np.array([[0, 1], [2, 3], [4, 5]])
            eng.exchange_grid(pairs, np.full(len(pairs), -np.inf))  # (every pair accepted)
        keys.append(eng.state_points()[0].copy())
        b = eng.run_sampled(ns, 7, statistics=True, structure=True)
        want.offer(b["enthalpy"], b["features"], None, keys[-1], intensities=b["structure_intensities"])
    assert not np.array_equal(keys[-1], np.arange(R))
    _same_record(eng.statistics(), want, "by state point")
    eng.close()


# ---- 6: the refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason(clean_env):
    from smol_amd.engine import Engine

    name = "fcc_conv444_pairs"
    sc = load_case(name)["sc"]
    eng = Engine(tables_for(name, INT), capi.make_config(2))
    lib, N = eng._lib, sc.num_sites
    good = StructureFactor.from_supercell(sc, commensurate_points(sc)[:4], intensities=[(1, 0, 1), (3, 1, 1)])
    eng.set_structure_factor(good)
    pool = _rand_occ(sc, np.random.default_rng(2), 2)
    want = good.evaluate(pool)
    P = lambda a, ct: a.ctypes.data_as(C.POINTER(ct))  # noqa: E731

    def refused(kind_base=None, K=2, phase=None, table=None, Q=None, M=None, intensity=((0, 0, 0),), scale=None, I=None):
        kb = np.ascontiguousarray(good.kind_base if kind_base is None else kind_base, dtype=np.int32)
        ph = np.ascontiguousarray(good.phase if phase is None else phase, dtype=np.uint16)
        tb = np.ascontiguousarray(good.table if table is None else table, dtype=np.int64)
        it = np.ascontiguousarray(intensity, dtype=np.int32).reshape(-1, 3)
        sc_ = np.ascontiguousarray(np.ones(len(it)) if scale is None else scale, dtype=np.float64)
        s = capi.smolmc_structure()
        s.n_kinds, s.n_points, s.n_phases = K, ph.shape[0] if Q is None else Q, tb.shape[1] if M is None else M
        s.n_intensities = len(it) if I is None else I
        s.kind_base, s.phase, s.table = P(kb, C.c_int32), P(ph, C.c_uint16), P(tb, C.c_int64)
        s.intensity, s.intensity_scale = P(it, C.c_int32), P(sc_, C.c_double)
        assert lib.smolmc_set_structure(eng._h, C.byref(s)) != 0
        # the handle is as it was
        assert eng.structure_shape() == (4, 2, 2)
        _same(eng.structure_factor(pool), want)
        return lib.smolmc_last_error().decode()

    M0 = good.n_phases
    bad = good.phase.copy()
    bad[2, 77] = M0
    assert f"phase[2][77] = {M0}, n_phases is {M0}: phase out of range" in refused(phase=bad)
    msg = refused(kind_base=np.where(np.arange(N) == 7, 1, 0))
    assert "kind_base[7] + site_ncodes = 1 + 2 is larger than n_kinds = 2" in msg and "kind out of range" in msg
    assert "n_kinds must be 1..254" in refused(K=255)
    assert "n_kinds must be 1..254" in refused(K=0)
    assert f"n_points must be 1..{capi.MAX_STRUCT_POINTS}, got {capi.MAX_STRUCT_POINTS + 1}" in refused(Q=capi.MAX_STRUCT_POINTS + 1)
    assert "n_points must be" in refused(Q=0)
    assert f"n_phases must be 1..{capi.MAX_STRUCT_PHASES}, got 65536" in refused(M=65536)
    big_m = capi.MAX_STRUCT_CELLS // 2 + 1
    assert (f"2 kinds x {big_m} phase classes = {2 * big_m} cells, larger than SMOLMC_MAX_STRUCT_CELLS = {capi.MAX_STRUCT_CELLS}"
            in refused(M=big_m))
    assert f"n_intensities must be 0..{capi.MAX_STRUCT_INTENSITIES}, got {capi.MAX_STRUCT_INTENSITIES + 1}" in refused(
        I=capi.MAX_STRUCT_INTENSITIES + 1)
    # 256 counted sites x 2^54 = 2^62: refused; one less passes the guard
    tb = good.table.copy()
    tb[1, 0, 1] = -(1 << 54)
    assert "256 counted sites x max|table| = 18014398509481984 reaches 2^62" in refused(table=tb)
    assert "intensity 1 names point 4, n_points is 4: point out of range" in refused(intensity=((0, 0, 0), (4, 0, 0)))
    assert "intensity 0 names kinds (0, 2), n_kinds is 2: kind out of range" in refused(intensity=((0, 0, 2),))
    assert "intensity 0 names kinds (-1, 0)" in refused(intensity=((0, -1, 0),))
    assert "intensity_scale[1] is not finite" in refused(intensity=((0, 0, 0), (1, 1, 1)), scale=[1.0, np.inf])
    assert "intensity_scale[0] is not finite" in refused(scale=[np.nan])
    # ... the guard's other side: accepted, and the amplitudes are still exact int64 sums
    tb[1, 0, 1] = -(1 << 54) + 1
    edge = StructureFactor(good.kind_base, 2, good.phase, tb, [(1, 0, 0)], site_ncodes=good.site_ncodes)
    eng.set_structure_factor(edge)
    _same(eng.structure_factor(pool), edge.evaluate(pool))
    eng.set_structure_factor(good)
    occ_bad = pool.copy()
    occ_bad[1, 5] = 2
    with pytest.raises(ERR, match="occupancy code 2 on site 5 gives kind 2, n_kinds = 2: kind out of range"):
        eng.structure_factor(occ_bad)
    with pytest.raises(ValueError, match="defined on 8 sites"):
        eng.set_structure_factor(StructureFactor(np.zeros(8, np.int32), 2, np.zeros((1, 8), np.int64), np.ones((1, 1, 2), np.int64)))
    eng.close()
    # a row too long to stage in LDS next to the counters of one point: 19683 sites and 12288 cells
    from smol_amd import synth

    big = synth.build_supercell(synth.build_cluster_model(synth.fcc_prim(), {2: 3.0}), [27, 27, 27])
    eng = Engine(capi.TableSet.from_synth(big, synth.random_coefs(big.model), feature_mode=INT), capi.make_config(1))
    rng = np.random.default_rng(1)
    assert capi.structure_plan(19683, 19696, 2, capi.MAX_STRUCT_CELLS // 2, 1) is None
    with pytest.raises(ERR, match="a row of 19683 sites is too long to stage in LDS next to the 12288 counters of a point"):
        eng.set_structure_factor(_raw_spec(big.num_sites, 2, capi.MAX_STRUCT_CELLS // 2, 1, rng))
    assert eng.structure_shape() == (0, 0, 0)
    sf = StructureFactor.from_supercell(big, np.array([[0, 0, 0], [9, 0, 0], [13, 5, 0]]), intensities=[(1, 1, 1), (2, 0, 1)])
    eng.set_structure_factor(sf)  # (at most 54 cells: the mask kernel, 308 words a row, the last one not full)
    assert _plan(eng) == ("mask",)
    occ = _rand_occ(big, rng, 2)
    _same(eng.structure_factor(occ), sf.evaluate(occ))
    eng.close()


# ---- 7: the sampler -------------------------------------------------------------------------------------------------------------------
def _sampler(sf_on, nw=6, **kw):
    c = load_case("rocksalt333_two_sublattices")
    ens = moca.Ensemble.from_cluster_expansion(c["sc"], c["coefs"])
    g = commensurate_points(c["sc"])
    K = Observables.default_kind_base(c["sc"])[1]
    sf = StructureFactor.from_supercell(c["sc"], g, intensities=[(q, a, a) for q in (0, 13, 26) for a in range(K)])
    s = moca.Sampler.from_ensemble(ens, temperature=3000.0, nwalkers=nw, seeds=list(range(3, 3 + nw)), rank=0, world_size=1,
                                   structure_factor=sf if sf_on else None, **kw)
    return s, sf, _rand_occ(c["sc"], np.random.default_rng(12), nw), ens


def test_sampler_traces_keep_occupancy_and_npz(clean_env, tmp_path):
    plain, sf, occ, ens = _sampler(False)
    traced, _, _, _ = _sampler(True)
    plain.run(12 * 9, occ, thin_by=9)
    traced.run(12 * 9, occ, thin_by=9)
    p, c = plain.samples, traced.samples
    assert c.num_samples == 12 and "structure_amplitudes" in c.traced_values and "structure_amplitudes" not in p.traced_values
    for name in p.traced_values:
        assert np.array_equal(p.get_trace_value(name, flat=False), c.get_trace_value(name, flat=False)), name
    amp, inten = c.get_trace_value("structure_amplitudes", flat=False), c.get_trace_value("structure_intensities", flat=False)
    assert amp.shape == (12, 6, sf.n_points, sf.n_kinds, 2)
    _same((amp, inten), sf.evaluate(c.get_occupancies(flat=False)))
    # keep_occupancy=False, then a second run: the chain goes on exactly where the kept-occupancy sampler's does
    dry, _, _, _ = _sampler(True)
    dry.run(12 * 9, occ, thin_by=9, keep_occupancy=False)
    d = dry.samples
    np.testing.assert_array_equal(d.last_occupancy(), c.last_occupancy())
    with pytest.raises(ValueError, match="keep_occupancy=False"):
        d.get_occupancies()
    dry.run(5 * 9, thin_by=9, keep_occupancy=False)
    traced.run(5 * 9, thin_by=9)
    assert d.num_samples == c.num_samples == 17
    for name in ("enthalpy", "features", "accepted", "structure_amplitudes", "structure_intensities"):
        assert np.array_equal(d.get_trace_value(name, flat=False), c.get_trace_value(name, flat=False)), name
    # the npz round trip carries both traces
    path = str(tmp_path / "samples.npz")
    c.to_npz(path)
    back = moca.SampleContainer.from_npz(path, ens)
    for name in ("structure_amplitudes", "structure_intensities", "enthalpy"):
        got = back.get_trace_value(name, flat=False)
        assert got.dtype == c.get_trace_value(name, flat=False).dtype
        assert np.array_equal(got, c.get_trace_value(name, flat=False)), name
    # a statistics record fed by the traced intensities
    spec = Statistics.per_walker([st.ENTHALPY, st.intensity(1)], n_levels=2)
    both, _, _, _ = _sampler(True, statistics=spec)
    both.run(12 * 9, occ, thin_by=9)
    want = StatisticsRecord(spec, 6)
    want.offer(c.get_trace_value("enthalpy", flat=False)[:12, :, 0], c.get_trace_value("features", flat=False)[:12], intensities=inten[:12])
    _same_record(both.statistics, want, "sampler")
    with pytest.raises(ValueError, match="needs a sampler built with structure_factor="):
        _sampler(False, statistics=spec)
