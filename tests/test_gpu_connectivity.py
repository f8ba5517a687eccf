"""Connectivity on the device (csrc/connectivity.hip; smolmc_set_connectivity, smolmc_eval_connectivity, the
SMOLMC_SAMPLE_CONNECTIVITY column of the sample ring, the connectivity columns of the statistics record): stats and labels
equal connectivity.Connectivity.evaluate, the NumPy definition, entry for entry, and a run with the flag is the same chain as
a run without."""

import ctypes as C

import numpy as np
import pytest

from smol_amd import capi, moca, synth
from smol_amd import connectivity as cn
from smol_amd import statistics as st
from smol_amd.connectivity import Connectivity, Graph
from smol_amd.observables import Observables
from smol_amd.statistics import Statistics, StatisticsRecord
from tests.cases import load_case, tables_for
from tests.test_gpu_observables import ENV
from tests.test_gpu_statistics import _same_record, _semigrand

pytestmark = pytest.mark.gpu
INT = capi.FEATURES_INTERACTIONS
ERR = (RuntimeError, ValueError)
NN, NNN = 4.09 / np.sqrt(2.0), 4.09  # nearest and next-nearest distance of the fcc cases (a = 4.09)


@pytest.fixture
def clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def _same(got, want):
    (gs, gl), (ws, wl) = got, want
    assert gs.dtype == np.int64 and gs.shape == ws.shape and gl.dtype == np.int32 and gl.shape == wl.shape
    np.testing.assert_array_equal(gs, ws)
    np.testing.assert_array_equal(gl, wl)


def _frac_occ(sc, rng, fractions, per=2):
    """``per`` rows per fraction: code 0 with that probability, else one of the site's other codes."""
    nsp = np.array([sc.model.prim.nspecies[b] for b in sc.site_b])
    rows = []
    for p in fractions:
        other = 1 + (rng.random((per, sc.num_sites)) * (nsp - 1)).astype(np.int32)
        rows.append(np.where(rng.random((per, sc.num_sites)) < p, 0, np.minimum(other, nsp - 1)).astype(np.int32))
    return np.concatenate(rows)


def _not_vacuous(stats, mixed=True):
    """From the definition alone: the rows hold a wrapping row, a row that does not wrap, and (``mixed``) a row with a
    wrapping component next to others."""
    s = stats.reshape(-1, cn.N_STATS)
    assert np.any(s[:, cn.WRAP_AXES] != 0) and np.any((s[:, cn.WRAP_AXES] == 0) & (s[:, cn.N_MEMBERS] > 0))
    assert not mixed or np.any((s[:, cn.N_WRAPPING] >= 1) & (s[:, cn.N_COMPONENTS] > 1))


def _fcc_handle(dims, R=2):
    from smol_amd.engine import Engine

    sc = synth.build_supercell(synth.build_cluster_model(synth.fcc_prim(), {2: 3.0}), dims)
    tab = capi.TableSet.from_synth(sc, synth.random_coefs(sc.model), feature_mode=INT)
    return Engine(tab, capi.make_config(R, capi.KERNEL_METROPOLIS, capi.STEP_SWAP)), sc


# ---- 1: smolmc_eval_connectivity ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fcc_conv444_pairs", "fcc3_indicator_skew", "fcc_prim222_aliased", "rocksalt333_two_sublattices"])
def test_eval_equals_the_definition(name, clean_env):
    """256 sites (a full workgroup of sites); a skew cell of 60; 8 sites whose bonds are self-image and two-image bonds;
    two sublattices with the members on one of them and two graphs of different member sets.  Member fractions on both
    sides of the fcc site threshold (0.199); 1, 3 and all rows, then the walkers' own states."""
    from smol_amd.engine import Engine

    sc = load_case(name)["sc"]
    R = 3
    eng = Engine(tables_for(name, INT), capi.make_config(R, capi.KERNEL_METROPOLIS, capi.STEP_SWAP))
    K = Observables.default_kind_base(sc)[1]
    if name == "rocksalt333_two_sublattices":
        # cations only, nearest cation neighbours (a / sqrt 2 = 2.97); kind 0 alone, and every cation kind but 0
        cations = list(range(K - 2))
        graphs = [dict(members=[0], cutoff=3.0), dict(members=cations[1:], cutoff=3.0)]
    elif name == "fcc_prim222_aliased":
        graphs = [dict(members=[0], cutoff=6.0), dict(members=[1], cutoff=NN + 0.01)]  # (6.0: a site is bonded to its own images)
    else:
        graphs = [dict(members=[0], cutoff=NN + 0.01), dict(members=[0], orbits=[o.id for o in sc.model.orbits
                                                                                 if o.size == 2 and abs(o.diameter - NNN) < 1e-6])]
    spec = Connectivity.from_supercell(sc, graphs)
    assert eng.connectivity_shape() == (0, 0)
    eng.set_connectivity(spec)
    assert eng.connectivity_shape() == (2, K)
    rng = np.random.default_rng(17)
    pool = _frac_occ(sc, rng, (0.1, 0.2, 0.4, 0.7), per=3)
    want = spec.evaluate(pool)
    if name == "fcc_prim222_aliased":
        assert np.any(want[0][..., cn.WRAP_AXES] != 0)
    else:  # (27 cations: too few for a wrapping component with others next to it; the larger cells have such rows)
        _not_vacuous(want[0][:, 0], mixed=not name.startswith("rocksalt"))
    for nocc in (1, 3, len(pool)):
        _same(eng.connectivity(pool[:nocc], labels=True), (want[0][:nocc], want[1][:nocc]))
    np.testing.assert_array_equal(eng.connectivity(pool), want[0])  # (stats alone)
    _same(eng.connectivity(pool, labels=True), want)                # (same input, same output)
    # occ = NULL: the walkers' current states, after a run
    occ = pool[-R:].copy()
    eng.set_state(occ, np.arange(R, dtype=np.uint64) + np.uint64(5), 2500.0)
    eng.run(300, sync=True)
    state = eng.get_state()
    assert not np.array_equal(state["occupancy"], occ)
    _same(eng.connectivity(labels=True), spec.evaluate(state["occupancy"]))
    # every third site left out, kinds split by site classes
    custom = Connectivity.from_supercell(sc, graphs[:1], site_classes=np.arange(sc.num_sites) % 2)
    kb = custom.kind_base.copy()
    kb[::3] = -1
    ncodes = np.array([sc.model.prim.nspecies[b] for b in sc.site_b])
    custom = Connectivity(kb, custom.n_kinds, [Graph([0, int(kb.max())], custom.graphs[0].bonds, custom.graphs[0].images)],
                          site_ncodes=ncodes)
    eng.set_connectivity(custom)
    _same(eng.connectivity(pool[:7], labels=True), custom.evaluate(pool[:7]))
    eng.set_connectivity(None)
    assert eng.connectivity_shape() == (0, 0)
    with pytest.raises(ERR, match="no connectivity spec set"):
        eng.connectivity(pool[:1])
    eng.close()


def _chain(N, order):
    """A ring of N sites, chain position p held by site order[p], bonds to the next position (the last one by image 1)."""
    bonds = [(order[p], order[(p + 1) % N]) for p in range(N)]
    images = [(0, 0, 0)] * (N - 1) + [(1, 0, 0)]
    return Connectivity(np.zeros(N, np.int32), 2, [Graph([1], bonds, images)], site_ncodes=np.full(N, 2))


def test_a_chain_of_diameter_255_converges_across_waves(clean_env):
    """257 x 1 x 1: a ring of 257 members wraps; with one site removed the 256 that remain are one component of diameter
    255, which the labels cross in many passes and over all four waves.  Once more with the sites permuted so that the
    smallest label sits in the middle of the chain, and in a random order."""
    eng, sc = _fcc_handle([257, 1, 1])
    N = sc.num_sites
    assert N == 257
    rng = np.random.default_rng(2)
    middle = np.roll(np.arange(N), 128)  # position 128 is site 0
    for order in (np.arange(N), middle, rng.permutation(N)):
        spec = _chain(N, [int(x) for x in order])
        eng.set_connectivity(spec)
        occ = np.ones((3, N), dtype=np.int32)
        occ[1, order[0]] = 0     # cut at position 0: positions 1..256 remain
        occ[2, order[77]] = 0    # cut elsewhere: the ring's closing bond joins the two ends
        want = spec.evaluate(occ)
        assert list(want[0][:, 0, cn.LARGEST]) == [257, 256, 256] and list(want[0][:, 0, cn.WRAP_AXES]) == [1, 0, 0]
        assert list(want[0][:, 0, cn.N_COMPONENTS]) == [1, 1, 1]
        _same(eng.connectivity(occ, labels=True), want)
        most, total = eng.connectivity_passes()
        assert 2 <= most <= N + 1 and total >= 3
    eng.close()


def test_343_sites_whose_row_is_padded(clean_env):
    eng, sc = _fcc_handle([7, 7, 7])
    assert sc.num_sites == 343 and eng.N == 343
    spec = Connectivity.from_supercell(sc, [dict(members=[0], cutoff=NN + 0.01), dict(members=[1], cutoff=NNN + 0.01)])
    eng.set_connectivity(spec)
    occ = _frac_occ(sc, np.random.default_rng(3), (0.1, 0.2, 0.4, 0.85), per=2)
    want = spec.evaluate(occ)
    _not_vacuous(want[0][:, 0])
    _same(eng.connectivity(occ, labels=True), want)
    eng.close()


def test_the_workloads_4096_sites_are_accepted(clean_env):
    """16 x 16 x 16, config 2's row: three rows around the threshold."""
    eng, sc = _fcc_handle([16, 16, 16], R=1)
    assert sc.num_sites == 4096 and capi.connectivity_lds_bytes(4096, 4096) is not None
    spec = Connectivity.from_supercell(sc, [dict(members=[0], cutoff=NN + 0.01)])
    eng.set_connectivity(spec)
    occ = _frac_occ(sc, np.random.default_rng(4), (0.12, 0.21, 0.5), per=1)
    want = spec.evaluate(occ)
    _not_vacuous(want[0])
    _same(eng.connectivity(occ, labels=True), want)
    eng.close()


def test_eight_graphs_and_kinds_beyond_one_mask_word(clean_env):
    from smol_amd.engine import Engine

    name = "fcc_conv444_pairs"
    sc = load_case(name)["sc"]
    eng = Engine(tables_for(name, INT), capi.make_config(2))
    rng = np.random.default_rng(5)
    pool = _frac_occ(sc, rng, (0.1, 0.2, 0.4), per=2)
    graphs = [dict(members=m, cutoff=c) for m in ([0], [1], [0, 1]) for c in (NN + 0.01, NNN + 0.01)]
    graphs += [dict(members=[0], cutoff=5.1), dict(members=[], cutoff=NN + 0.01)]  # (a third shell; a graph nobody is in)
    spec = Connectivity.from_supercell(sc, graphs)
    assert spec.n_graphs == 8
    eng.set_connectivity(spec)
    want = spec.evaluate(pool)
    _not_vacuous(want[0][:, 0])
    assert np.all(want[0][:, 7] == 0) and np.all(want[1][:, 7] == -1) and np.all(want[0][:, 4, cn.LARGEST] == sc.num_sites)
    _same(eng.connectivity(pool, labels=True), want)
    # 18 site classes of a binary alloy: 36 kinds; 40 classes: 80 kinds, members in the second word of the mask
    for n_classes in (18, 40):
        K = 2 * n_classes
        members = [k for k in range(K) if k % 2 == 0 and k % 6 != 2]  # code 0 of two classes in three
        spec = Connectivity.from_supercell(sc, [dict(members=members, cutoff=NN + 0.01), dict(members=[K - 1, K - 2], cutoff=5.1)],
                                           site_classes=np.arange(sc.num_sites) % n_classes)
        assert spec.n_kinds == K and (n_classes == 18 or spec.member_masks()[0, 1] != 0)
        eng.set_connectivity(spec)
        assert eng.connectivity_shape() == (2, K)
        want = spec.evaluate(pool)
        assert np.any(want[0][:, 0, cn.N_COMPONENTS] > 1) and np.any(want[0][:, 1, cn.N_MEMBERS] > 0)
        _same(eng.connectivity(pool, labels=True), want)
    eng.close()


# ---- 2: the relabelled handle -----------------------------------------------------------------------------------------------------
def test_relabelled_handle_takes_and_gives_the_callers_numbering(clean_env):
    from smol_amd.engine import Engine
    from tests.test_gpu_capi_relabel import _model

    sc, ens, tab, occ, frozen = _model(capi.STEP_SWAP)
    R = len(occ)
    eng = Engine(tab, capi.make_config(R, capi.KERNEL_METROPOLIS, capi.STEP_SWAP))
    assert "relabelled=1" in eng.kernel_info(), eng.kernel_info()
    classes = np.zeros(sc.num_sites, dtype=np.int64)
    classes[frozen] = 1  # kinds that follow the CALLER's site numbers
    spec = Connectivity.from_supercell(sc, [dict(members=[0], cutoff=3.0), dict(members=[1, 2], cutoff=3.0)], site_classes=classes)
    eng.set_connectivity(spec)
    rng = np.random.default_rng(8)
    pool = _frac_occ(sc, rng, (0.15, 0.3), per=2)
    want = spec.evaluate(pool)
    assert np.any(want[0][..., cn.N_COMPONENTS] > 1) and np.any(want[0][..., cn.WRAP_AXES] != 0)
    _same(eng.connectivity(pool, labels=True), want)
    eng.set_state(occ, np.arange(R, dtype=np.uint64) + np.uint64(9), 4000.0)
    eng.run(200, sync=True)
    _same(eng.connectivity(labels=True), spec.evaluate(eng.get_state()["occupancy"]))
    smp = eng.run_sampled(2, 9, connectivity=True)
    np.testing.assert_array_equal(smp["connectivity"], spec.evaluate(smp["occupancy"])[0])
    eng.close()


# ---- 3: the ring ---------------------------------------------------------------------------------------------------------------------
def _ring_handle(R=3):
    from smol_amd.engine import Engine

    name = "fcc_conv444_pairs"
    sc = load_case(name)["sc"]
    eng = Engine(tables_for(name, INT), capi.make_config(R, capi.KERNEL_METROPOLIS, capi.STEP_SWAP))
    spec = Connectivity.from_supercell(sc, [dict(members=[0], cutoff=NN + 0.01), dict(members=[1], cutoff=NNN + 0.01)])
    eng.set_connectivity(spec)
    occ = (np.random.default_rng(21).random((R, sc.num_sites)) < 0.8).astype(np.int32)  # a fifth of the sites hold code 0
    seeds = np.arange(R, dtype=np.uint64) + np.uint64(31)
    eng.set_state(occ, seeds, 3000.0)
    return eng, spec, occ, seeds


def test_ring_column_equals_the_definition_and_the_chain_does_not_change(clean_env):
    R = 3
    eng, spec, occ, seeds = _ring_handle(R)
    eng.run(11)
    smp = eng.run_sampled(3, 7, connectivity=True)
    assert smp["occupancy"].shape == (3, R, eng.N) and smp["connectivity"].shape == (3, R, 2, 24)
    assert smp["connectivity"].dtype == np.int64 and len({smp["occupancy"][i].tobytes() for i in range(3)}) == 3
    np.testing.assert_array_equal(smp["connectivity"], spec.evaluate(smp["occupancy"])[0])
    assert np.any(smp["connectivity"][..., 0, cn.N_COMPONENTS] > 1)
    final = eng.get_state()
    # without the occupancy column: the same column, the rows stay on the device
    eng.set_state(occ, seeds, 3000.0)
    eng.run(11)
    eng.run_sampled_async(3, 7, occupancy=False, connectivity=True)
    npend, ns, flags = eng.pending_samples()
    assert (npend, ns) == (1, 3) and flags & capi.SAMPLE_CONNECTIVITY and not flags & capi.SAMPLE_OCCUPANCY
    dry = eng.fetch_samples()
    assert dry["occupancy"] is None
    np.testing.assert_array_equal(dry["connectivity"], smp["connectivity"])
    # a run without the flag: enthalpy, features, accept flags, occupancies and the final state are identical
    eng.set_state(occ, seeds, 3000.0)
    eng.run(11)
    plain = eng.run_sampled(3, 7)
    assert "connectivity" not in plain
    for key in plain:
        assert np.array_equal(plain[key], smp[key]), key
    for key in ("enthalpy", "features", "accepted"):
        assert np.array_equal(plain[key], dry[key]), key
    after = eng.get_state()
    for key in final:
        assert np.array_equal(final[key], after[key]), key
    eng.close()


def test_ring_discipline(clean_env):
    eng, spec, occ, seeds = _ring_handle(4)
    eng.run_sampled_async(2, 5, connectivity=True)
    eng.run_sampled_async(3, 4, connectivity=True)
    # the getter reads the block the next fetch delivers, and does not deliver it
    c0 = eng.sample_connectivity()
    assert c0.shape == (2, 4, 2, 24) and eng.pending_samples()[:2] == (2, 2)
    a = eng.fetch_samples()
    np.testing.assert_array_equal(c0, spec.evaluate(a["occupancy"])[0])
    np.testing.assert_array_equal(a["connectivity"], c0)
    b = eng.fetch_samples()
    assert b["connectivity"].shape[0] == 3
    np.testing.assert_array_equal(b["connectivity"], spec.evaluate(b["occupancy"])[0])
    assert not np.array_equal(b["occupancy"][0], a["occupancy"][-1])
    # a new spec while a block with the column waits: refused; the block stays
    eng.run_sampled_async(1, 3, connectivity=True)
    with pytest.raises(ERR, match="while a block recorded with SMOLMC_SAMPLE_CONNECTIVITY waits in the ring"):
        eng.set_connectivity(spec)
    with pytest.raises(ERR, match="while a block recorded with SMOLMC_SAMPLE_CONNECTIVITY waits in the ring"):
        eng.set_connectivity(None)
    assert eng.pending_samples()[0] == 1 and eng.connectivity_shape() == (2, 2)
    # discard_samples empties the ring; the spec can be set again
    eng.discard_samples()
    assert eng.pending_samples()[0] == 0
    eng.set_connectivity(spec)
    # a block recorded without the flag refuses the getter
    eng.run_sampled_async(2, 5)
    with pytest.raises(ERR, match="connectivity stats were not recorded"):
        eng.sample_connectivity()
    assert "connectivity" not in eng.fetch_samples()
    # the flag without a spec is refused and takes no slot
    eng.set_connectivity(None)
    with pytest.raises(ERR, match="SMOLMC_SAMPLE_CONNECTIVITY without a connectivity spec"):
        eng.run_sampled_async(1, 5, connectivity=True)
    assert eng.pending_samples()[0] == 0
    eng.close()


# ---- 4: statistics with connectivity columns -----------------------------------------------------------------------------------------
def _stat_handle(R):
    eng, obs, sc = _semigrand("fcc_conv444_pairs", R)
    spec = Connectivity.from_supercell(sc, [dict(members=[1], cutoff=NN + 0.01)], observables=obs)
    eng.set_connectivity(spec)
    return eng, obs, sc, spec


def _spec(by_point=False):
    make = Statistics.by_state_point if by_point else Statistics.per_walker
    return make([st.ENTHALPY, st.connectivity(0, cn.LARGEST), st.connectivity(0, cn.WRAP_AXES)], n_levels=3,
                hist=(st.connectivity(0, cn.LARGEST), 16, 0.0, 16.0))


def test_statistics_record_with_connectivity_columns(clean_env):
    R = 70
    eng, obs, sc, spec_c = _stat_handle(R)
    occ0 = _frac_occ(sc, np.random.default_rng(5), (0.8,), per=R)  # a fifth of the sites hold code 1, the member
    seeds = np.arange(R, dtype=np.uint64) + np.uint64(11)
    spec = _spec()
    eng.set_statistics(spec)
    assert eng.statistics_shape() == (R, 3, 3, 16)
    eng.set_state(occ0, seeds, 3000.0)
    # two blocks queued before the first fetch, the column fetched with them
    eng.run_sampled_async(3, 5, statistics=True, connectivity=True)
    eng.run_sampled_async(4, 5, statistics=True, connectivity=True)
    blocks = [eng.fetch_samples(), eng.fetch_samples()]
    want = StatisticsRecord(spec, R)
    for b in blocks:
        np.testing.assert_array_equal(b["connectivity"], spec_c.evaluate(b["occupancy"])[0])
        want.offer(b["enthalpy"], b["features"], connectivity=spec_c.evaluate(b["occupancy"])[0])
    got = eng.statistics()
    _same_record(got, want, "two blocks")
    assert (got.n == 7).all() and got.hist.sum() + got.over.sum() == 7 * R and got.hist.sum() > 0 and np.any(got.s2[:, 3] != 0)
    # the same record with nothing but the statistics asked for: rows and stats stay on the device
    eng.set_statistics(spec)
    eng.set_state(occ0, seeds, 3000.0)
    eng.run_sampled_async(3, 5, statistics=True, occupancy=False)
    eng.run_sampled_async(4, 5, statistics=True, occupancy=False)
    dry = [eng.fetch_samples(), eng.fetch_samples()]
    assert all(d["occupancy"] is None and "connectivity" not in d for d in dry)
    _same_record(eng.statistics(), want, "alone")
    # update_statistics after a plain run: one offer of the current states
    for n in (40, 1):
        eng.run(n)
        eng.update_statistics()
        s = eng.get_state()
        want.offer(s["enthalpy"], s["features"], connectivity=spec_c.evaluate(s["occupancy"])[0])
        _same_record(eng.statistics(), want, "update")
    # the spec cannot change under the record
    with pytest.raises(ERR, match="while a statistics record with connectivity columns depends on the spec"):
        eng.set_connectivity(None)
    with pytest.raises(ERR, match="while a statistics record with connectivity columns depends on the spec"):
        eng.set_connectivity(spec_c)
    _same_record(eng.statistics(), want, "after the refusals")
    # with the record gone the spec can go, and then the connectivity sources are out of range again
    eng.set_statistics(None)
    eng.set_connectivity(None)
    with pytest.raises(ERR, match=f"column 1 has source {2 + eng.F + obs.n_kinds}, outside 0..{1 + eng.F + obs.n_kinds} "):
        eng.set_statistics(Statistics.per_walker([st.ENTHALPY, ("source", 2 + eng.F + obs.n_kinds)]))
    eng.close()


def test_statistics_by_state_point_after_an_exchange(clean_env):
    R = 6
    eng, obs, sc, spec_c = _stat_handle(R)
    rows = np.zeros(eng._mu_shape())
    rows[:, 0, 1] = np.linspace(-0.2, 0.2, R)
    eng.set_walker_mu(rows)
    eng.set_state(_frac_occ(sc, np.random.default_rng(9), (0.75,), per=R), np.arange(R, dtype=np.uint64) + np.uint64(21),
                  np.linspace(2500.0, 4000.0, R))
    spec = _spec(by_point=True)
    eng.set_statistics(spec)
    want = StatisticsRecord(spec, R)
    keys = []
    for i, ns in enumerate((3, 4)):
        if i:
            pairs = np.array([[0, 1], [2, 3], [4, 5]])
            eng.exchange_grid(pairs, np.full(len(pairs), -np.inf))  # (every pair accepted)
        keys.append(eng.state_points()[0].copy())
        b = eng.run_sampled(ns, 7, statistics=True, connectivity=True)
        want.offer(b["enthalpy"], b["features"], None, keys[-1], connectivity=spec_c.evaluate(b["occupancy"])[0])
    assert not np.array_equal(keys[-1], np.arange(R))
    _same_record(eng.statistics(), want, "by state point")
    eng.close()


# ---- 5: the refusals ----------------------------------------------------------------------------------------------------------------
def _raw_refusal(eng, kind_base, K, masks, ptr, bonds, images, G=None):
    P = lambda a, ct: a.ctypes.data_as(C.POINTER(ct))  # noqa: E731
    kb = np.ascontiguousarray(kind_base, dtype=np.int32)
    mk = np.ascontiguousarray(masks, dtype=np.uint64).reshape(-1, 4)
    pt = np.ascontiguousarray(ptr, dtype=np.int64)
    bd = np.ascontiguousarray(bonds, dtype=np.int32).reshape(-1, 2)
    im = np.ascontiguousarray(images, dtype=np.int8).reshape(-1, 3)
    s = capi.smolmc_connectivity()
    s.n_kinds, s.n_graphs = K, len(mk) if G is None else G
    s.kind_base, s.member_mask, s.bond_ptr = P(kb, C.c_int32), P(mk, C.c_uint64), P(pt, C.c_int64)
    s.bonds, s.images = P(bd, C.c_int32), P(im, C.c_int8)
    assert eng._lib.smolmc_set_connectivity(eng._h, C.byref(s)) != 0
    return eng._lib.smolmc_last_error().decode()


def test_refusals_name_their_reason(clean_env):
    from smol_amd.engine import Engine

    name = "fcc_conv444_pairs"
    sc = load_case(name)["sc"]
    eng = Engine(tables_for(name, INT), capi.make_config(2))
    N = sc.num_sites
    good = Connectivity.from_supercell(sc, [dict(members=[0], cutoff=NN + 0.01)])
    eng.set_connectivity(good)
    pool = _frac_occ(sc, np.random.default_rng(2), (0.3,), per=2)
    want = good.evaluate(pool)
    kb0, one = good.kind_base, [[1, 0, 0, 0]]

    def refused(**kw):
        a = dict(kind_base=kb0, K=2, masks=one, ptr=[0, 1], bonds=[(0, 1)], images=[(0, 0, 0)])
        a.update(kw)
        msg = _raw_refusal(eng, **a)
        # the handle is as it was
        assert eng.connectivity_shape() == (1, 2)
        _same(eng.connectivity(pool, labels=True), want)
        return msg

    assert f"graph 0 bond 1 = (3, {N}), {N} sites: bond out of range" in refused(ptr=[0, 2], bonds=[(0, 1), (3, N)], images=np.zeros((2, 3)))
    assert "bond out of range" in refused(bonds=[(-1, 0)])
    assert "graph 1 bond 0 = (256, 0)" in refused(masks=one * 2, ptr=[0, 1, 2], bonds=[(0, 1), (N, 0)], images=np.zeros((2, 3)))
    msg = refused(kind_base=np.where(np.arange(N) == 7, 1, 0))
    assert "kind_base[7] + site_ncodes = 1 + 2 is larger than n_kinds = 2" in msg and "kind out of range" in msg
    assert "graph 0 names member kind 2, n_kinds is 2: kind out of range" in refused(masks=[[5, 0, 0, 0]])
    assert "graph 0 names member kind 200, n_kinds is 2: kind out of range" in refused(masks=[[1, 0, 0, 1 << 8]])
    assert "n_kinds must be 1..254" in refused(K=255)
    assert f"n_graphs must be 1..{capi.MAX_CONN_GRAPHS}, got 0" in refused(G=0)
    assert f"n_graphs must be 1..{capi.MAX_CONN_GRAPHS}, got 9" in refused(masks=one * 9, ptr=[0] + [1] * 9)
    assert "has image (0, -8, 0), beyond SMOLMC_MAX_CONN_IMAGE = 7: image out of range" in refused(images=[(0, -8, 0)])
    assert "has image (8, 0, 0)" in refused(images=[(8, 0, 0)])
    # ... the limit itself is accepted
    edge = Connectivity(kb0, 2, [Graph([0], [(0, 1), (1, 0)], [(7, -7, 0), (0, 0, 7)])], site_ncodes=good.site_ncodes)
    eng.set_connectivity(edge)
    occ = np.zeros((1, N), np.int32)
    got = eng.connectivity(occ, labels=True)
    _same(got, edge.evaluate(occ))
    assert got[0][0, 0, cn.WRAP_AXES] == 7 and got[0][0, 0, cn.LARGEST] == 2
    eng.set_connectivity(good)
    with pytest.raises(ERR, match="SMOLMC_SAMPLE_CONNECTIVITY without a connectivity spec"):
        eng.set_connectivity(None)
        eng.run_sampled_async(1, 5, connectivity=True)
    eng.set_connectivity(good)
    occ_bad = pool.copy()
    occ_bad[1, 5] = 2
    with pytest.raises(ERR, match="occupancy code 2 on site 5 gives kind 2, n_kinds = 2: kind out of range"):
        eng.connectivity(occ_bad)
    with pytest.raises(ValueError, match="defined on 8 sites"):
        eng.set_connectivity(Connectivity(np.zeros(8, np.int32), 2, [Graph([0], [(0, 1)])]))
    eng.close()
    # rows whose path sums could leave their 16 bits (17^3 = 4913 sites), and rows the LDS plan cannot hold (27^3 = 19683)
    for dim, reason in ((17, "4913 sites x SMOLMC_MAX_CONN_IMAGE = 7 is larger than SMOLMC_MAX_CONN_PATH_SUM = 32767"),
                        (27, "a row of 19683 sites is too long for the LDS plan")):
        big, bsc = _fcc_handle([dim] * 3, R=1)
        assert (capi.connectivity_lds_bytes(bsc.num_sites, (bsc.num_sites + 15) // 16 * 16) is None) == (dim == 27)
        assert reason in _raw_refusal(big, np.zeros(bsc.num_sites), 2, one, [0, 1], [(0, 1)], [(0, 0, 0)])
        assert big.connectivity_shape() == (0, 0)
        big.close()


# ---- 6: the sampler -------------------------------------------------------------------------------------------------------------------
def _sampler(on, nw=6, **kw):
    c = load_case("rocksalt333_two_sublattices")
    ens = moca.Ensemble.from_cluster_expansion(c["sc"], c["coefs"])
    spec = Connectivity.from_supercell(c["sc"], [dict(members=[0], cutoff=3.0), dict(members=[1, 2], cutoff=4.3)])
    s = moca.Sampler.from_ensemble(ens, temperature=3000.0, nwalkers=nw, seeds=list(range(3, 3 + nw)), rank=0, world_size=1,
                                   connectivity=spec if on else None, **kw)
    return s, spec, _frac_occ(c["sc"], np.random.default_rng(12), (0.3,), per=nw), ens


def test_sampler_traces_keep_occupancy_and_npz(clean_env, tmp_path):
    plain, spec, occ, ens = _sampler(False)
    traced, _, _, _ = _sampler(True)
    plain.run(12 * 9, occ, thin_by=9)
    traced.run(12 * 9, occ, thin_by=9)
    p, c = plain.samples, traced.samples
    assert c.num_samples == 12 and "connectivity" in c.traced_values and "connectivity" not in p.traced_values
    for name in p.traced_values:
        assert np.array_equal(p.get_trace_value(name, flat=False), c.get_trace_value(name, flat=False)), name
    conn = c.get_trace_value("connectivity", flat=False)
    assert conn.shape == (12, 6, 2, 24) and conn.dtype == np.int64
    np.testing.assert_array_equal(conn, spec.evaluate(c.get_occupancies(flat=False))[0])
    assert c.metadata["connectivity"]["n_graphs"] == 2 and c.metadata["connectivity"]["members"] == [[0], [1, 2]]
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
    for name in ("enthalpy", "features", "accepted", "connectivity"):
        assert np.array_equal(d.get_trace_value(name, flat=False), c.get_trace_value(name, flat=False)), name
    # the npz round trip carries the trace and the spec's metadata
    path = str(tmp_path / "samples.npz")
    c.to_npz(path)
    back = moca.SampleContainer.from_npz(path, ens)
    for name in ("connectivity", "enthalpy"):
        got = back.get_trace_value(name, flat=False)
        assert got.dtype == c.get_trace_value(name, flat=False).dtype
        assert np.array_equal(got, c.get_trace_value(name, flat=False)), name
    assert back.metadata["connectivity"] == c.metadata["connectivity"]
    # a statistics record fed by the traced numbers
    stat = Statistics.per_walker([st.ENTHALPY, st.connectivity(1, cn.LARGEST)], n_levels=2)
    both, _, _, _ = _sampler(True, statistics=stat)
    both.run(12 * 9, occ, thin_by=9)
    want = StatisticsRecord(stat, 6)
    want.offer(c.get_trace_value("enthalpy", flat=False)[:12, :, 0], c.get_trace_value("features", flat=False)[:12], connectivity=conn[:12])
    _same_record(both.statistics, want, "sampler")
    with pytest.raises(ValueError, match="needs a sampler built with connectivity="):
        _sampler(False, statistics=stat)
    with pytest.raises(ValueError, match="connectivity= with windows="):
        moca.Sampler.from_ensemble(ens, temperature=3000.0, nwalkers=2, windows=object(), connectivity=spec)


def test_sampler_with_a_grid_exchange(clean_env):
    """run_exchange(grid=...): every sample's column is the definition of that sample's occupancy, exchanges or not."""
    model = synth.build_cluster_model(synth.rocksalt_prim(), {2: 3.5})
    sc = synth.build_supercell(model, [3, 3, 3])
    ens = moca.Ensemble.from_cluster_expansion(sc, synth.random_coefs(model, seed=5, scale=0.05))
    names = ens.species
    ens.chemical_potentials = {names[0]: 0.1, names[1]: -0.2, names[2]: 0.05}
    temps = [3000.0, 3600.0, 4500.0]
    mus = [{names[0]: 0.1, names[1]: -0.2 + dm, names[2]: 0.05} for dm in np.linspace(-0.15, 0.15, 4)]
    nw = 12
    spec = Connectivity.from_supercell(sc, [dict(members=[0], cutoff=3.0)])
    sampler = moca.Sampler.from_ensemble(ens, temperature=3000.0, nwalkers=nw, seeds=list(range(11, 11 + nw)), connectivity=spec)
    rng = np.random.default_rng(2)
    occ = np.zeros((nw, ens.num_sites), dtype=np.int32)
    occ[:, : sc.size] = rng.integers(0, 3, size=(nw, sc.size))
    gx = sampler.run_exchange(8, 200, occ, thin_by=100, grid=dict(temperatures=temps, chemical_potentials=mus, seed=4))
    assert 0 < gx.acceptance
    smp = sampler.samples
    conn = smp.get_trace_value("connectivity", flat=False)
    assert conn.shape == (16, nw, 1, 24)
    np.testing.assert_array_equal(conn, spec.evaluate(smp.get_occupancies(flat=False))[0])
    assert np.any(conn[..., 0, cn.N_COMPONENTS] > 1)
