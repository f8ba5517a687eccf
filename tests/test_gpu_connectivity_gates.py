"""Gated bonds on the device (csrc/connectivity.hip; smolmc_set_connectivity_gated): the stats and labels of graphs whose bond
rows carry gate sites equal connectivity.Connectivity.evaluate, the NumPy definition, entry for entry -- through
smolmc_eval_connectivity, the sample ring, the statistics record and the sampler -- and an ungated graph next to a gated
one is what it is alone."""

import ctypes as C

import numpy as np
import pytest

from smol_amd import capi, moca
from smol_amd import connectivity as cn
from smol_amd import statistics as st
from smol_amd.connectivity import Connectivity, Graph
from smol_amd.statistics import Statistics, StatisticsRecord
from tests.cases import load_case, tables_for
from tests.test_connectivity_gates_host import TETRA, check_ladder, ladder, ladder_rows, member_rows, rocksalt_cation_spec
from tests.test_gpu_connectivity import ERR, INT, NN, NNN, _fcc_handle, _frac_occ, _not_vacuous, _same
from tests.test_gpu_observables import ENV
from tests.test_gpu_statistics import _same_record, _semigrand

pytestmark = pytest.mark.gpu


@pytest.fixture
def clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def _tetra(members, cutoff, max_blocked):
    return dict(members=members, cutoff=cutoff, gate=dict(kinds=members, corners=2, max_blocked=max_blocked))


def _ungated(spec):
    """The same graphs without their gates: every row open when its ends are members."""
    return Connectivity(spec.kind_base, spec.n_kinds, [Graph(g.members, g.bonds, g.images) for g in spec.graphs],
                        site_ncodes=spec.site_ncodes)


# ---- 1: smolmc_eval_connectivity ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fcc_conv444_pairs", "fcc3_indicator_skew", "fcc_prim222_aliased", "rocksalt333_two_sublattices"])
def test_eval_equals_the_definition(name, clean_env):
    """The members and cutoffs of tests/test_gpu_connectivity.py with tetrahedral gates of the member kind, max_blocked 0
    and 1: 256 sites (a full workgroup of sites); a skew cell of 60; 8 sites whose channels have corners that are an end's
    image or each other; the cation sublattice of a rocksalt.  Member fractions on both sides of the 0-TM threshold (near
    0.55 for max_blocked = 0); 1, 3 and all rows, then the walkers' own states."""
    from smol_amd.engine import Engine

    sc = load_case(name)["sc"]
    R = 3
    eng = Engine(tables_for(name, INT), capi.make_config(R, capi.KERNEL_METROPOLIS, capi.STEP_SWAP))
    if name == "rocksalt333_two_sublattices":
        spec = rocksalt_cation_spec(sc, (0, 1))
    elif name == "fcc_prim222_aliased":
        spec = Connectivity.from_supercell(sc, [_tetra([0], 6.0, 0), _tetra([1], NN + 0.01, 0), _tetra([1], NN + 0.01, 1)])
    else:
        spec = Connectivity.from_supercell(sc, [_tetra([0], NN + 0.01, 0), _tetra([0], NN + 0.01, 1)])
    G = spec.n_graphs
    assert eng.connectivity_gates() == ((), 0)
    eng.set_connectivity(spec)
    assert eng.connectivity_shape() == (G, spec.n_kinds)
    gated, n_channels = eng.connectivity_gates()
    assert gated == tuple(range(G)) and n_channels > 0
    rng = np.random.default_rng(23)
    pool = _frac_occ(sc, rng, (0.3, 0.45, 0.6, 0.7, 0.85), per=3)
    want = spec.evaluate(pool)
    if name == "fcc_prim222_aliased":
        assert np.any(want[0][..., cn.WRAP_AXES] != 0) and np.any(want[0][..., cn.N_COMPONENTS] > 1)
    else:  # (27 cations: too few for a wrapping component with others next to it; the larger cells have such rows)
        _not_vacuous(want[0][:, 0], mixed=not name.startswith("rocksalt"))
    assert np.any(want[0] != _ungated(spec).evaluate(pool)[0])  # (the gates matter)
    assert np.any(want[0][:, -1] != want[0][:, -2])              # (and so does max_blocked)
    for nocc in (1, 3, len(pool)):
        _same(eng.connectivity(pool[:nocc], labels=True), (want[0][:nocc], want[1][:nocc]))
    np.testing.assert_array_equal(eng.connectivity(pool), want[0])  # (stats alone)
    # occ = NULL: the walkers' current states, after a run
    occ = pool[6:6 + R].copy()
    eng.set_state(occ, np.arange(R, dtype=np.uint64) + np.uint64(5), 2500.0)
    eng.run(300, sync=True)
    state = eng.get_state()
    assert not np.array_equal(state["occupancy"], occ)
    _same(eng.connectivity(labels=True), spec.evaluate(state["occupancy"]))
    # the ungated entry point takes the handle back to a spec without gates
    eng.set_connectivity(_ungated(spec))
    assert eng.connectivity_gates() == ((), 0)
    _same(eng.connectivity(pool[:4], labels=True), _ungated(spec).evaluate(pool[:4]))
    eng.close()


# ---- 2: gated and ungated graphs in one spec ---------------------------------------------------------------------------------------
def test_a_mixed_spec_and_the_ungated_graphs_as_they_are_alone(clean_env):
    """ungated (12 neighbours), gated, ungated (18 neighbours), gated by triangles with max_blocked = 1: one launch, the
    branch taken per graph, the open bits of one gated graph overwritten by the next."""
    from smol_amd.engine import Engine

    name = "fcc_conv444_pairs"
    sc = load_case(name)["sc"]
    eng = Engine(tables_for(name, INT), capi.make_config(2))
    plain = [dict(members=[0], cutoff=NN + 0.01), dict(members=[1], cutoff=NNN + 0.01)]
    graphs = [plain[0], _tetra([0], NN + 0.01, 0), plain[1],
              dict(members=[1], cutoff=NN + 0.01, gate=dict(kinds=[1], corners=1, max_blocked=1))]
    spec, alone = Connectivity.from_supercell(sc, graphs), Connectivity.from_supercell(sc, plain)
    pool = _frac_occ(sc, np.random.default_rng(6), (0.15, 0.35, 0.5, 0.65, 0.8), per=2)
    want = spec.evaluate(pool)
    _not_vacuous(want[0][:, 1])
    _not_vacuous(want[0][:, 3])
    assert np.any(want[0][:, 1] != want[0][:, 0])
    eng.set_connectivity(spec)
    assert eng.connectivity_gates()[0] == (1, 3)
    got = eng.connectivity(pool, labels=True)
    _same(got, want)
    eng.set_connectivity(alone)
    assert eng.connectivity_gates() == ((), 0)
    solo = eng.connectivity(pool, labels=True)
    _same(solo, alone.evaluate(pool))
    np.testing.assert_array_equal(solo[0], got[0][:, [0, 2]])
    np.testing.assert_array_equal(solo[1], got[1][:, [0, 2]])
    eng.close()


# ---- 3: the ladder ----------------------------------------------------------------------------------------------------------------
def test_a_ladder_of_129_rungs_across_the_waves(clean_env):
    """258 sites: chain and gate sites lie in all four waves.  The answers are worked out by hand (ladder_rows)."""
    M = 129
    eng, sc = _fcc_handle([2 * M, 1, 1])
    N = sc.num_sites
    assert N == 2 * M
    rng = np.random.default_rng(4)
    for order in (np.arange(N), rng.permutation(N)):
        order = [int(x) for x in order]
        spec = ladder(M, order)
        occ, answers = ladder_rows(M, order)
        want = spec.evaluate(occ)
        check_ladder(want[0], want[1], answers, order, M)
        eng.set_connectivity(spec)
        got = eng.connectivity(occ, labels=True)
        _same(got, want)
        check_ladder(got[0], got[1], answers, order, M)
        most, total = eng.connectivity_passes()
        assert 2 <= most <= N + 1 and total >= 4
    eng.close()


# ---- 4, 5: padded rows and the workload's row -------------------------------------------------------------------------------------
def test_343_sites_whose_row_is_padded(clean_env):
    eng, sc = _fcc_handle([7, 7, 7])
    assert sc.num_sites == 343 and eng.N == 343
    spec = Connectivity.from_supercell(sc, [_tetra([0], NN + 0.01, 0)])
    assert len(spec.graphs[0].bonds) == 8232
    eng.set_connectivity(spec)
    occ = member_rows(343, np.random.default_rng(3), (0.30, 0.45, 0.55, 0.65, 0.80), per=2)
    want = spec.evaluate(occ)
    _not_vacuous(want[0][:, 0])
    share = want[0][:, 0, cn.LARGEST] / want[0][:, 0, cn.N_MEMBERS]
    assert share[:2].max() < 0.5 and share[-2:].min() > 0.5  # (far below the threshold near 0.55, and far above it)
    _same(eng.connectivity(occ, labels=True), want)
    eng.close()


def test_the_workloads_4096_sites_with_tetrahedral_gates_are_accepted(clean_env):
    """16 x 16 x 16, config 2's row: 12 neighbours a site are three groups, 12 open bits, two bytes a site."""
    eng, sc = _fcc_handle([16, 16, 16], R=1)
    assert sc.num_sites == 4096 and capi.connectivity_lds_bytes(4096, 4096, capi.connectivity_open_bytes(12)) == 57744
    spec = Connectivity.from_supercell(sc, [_tetra([0], NN + 0.01, 0)])
    assert len(spec.graphs[0].bonds) == 98304
    eng.set_connectivity(spec)
    assert eng.connectivity_gates() == ((0,), 4096 * 12 * 2)
    occ = member_rows(4096, np.random.default_rng(4), (0.45, 0.55, 0.65), per=1)
    want = spec.evaluate(occ)
    _not_vacuous(want[0], mixed=False)
    _same(eng.connectivity(occ, labels=True), want)
    eng.close()


# ---- 6: the relabelled handle -----------------------------------------------------------------------------------------------------
def test_relabelled_handle_takes_and_gives_the_callers_numbering(clean_env):
    from smol_amd.engine import Engine
    from tests.test_gpu_capi_relabel import _model

    sc, ens, tab, occ, frozen = _model(capi.STEP_SWAP)
    R = len(occ)
    eng = Engine(tab, capi.make_config(R, capi.KERNEL_METROPOLIS, capi.STEP_SWAP))
    assert "relabelled=1" in eng.kernel_info(), eng.kernel_info()
    classes = np.zeros(sc.num_sites, dtype=np.int64)
    classes[frozen] = 1  # kinds that follow the CALLER's site numbers
    spec = rocksalt_cation_spec(sc, (0, 1), kinds=(0,), site_classes=classes)
    eng.set_connectivity(spec)
    assert eng.connectivity_gates()[0] == (0, 1)
    rng = np.random.default_rng(8)
    pool = _frac_occ(sc, rng, (0.5, 0.7, 0.85), per=2)
    want = spec.evaluate(pool)
    assert np.any(want[0][..., cn.N_COMPONENTS] > 1) and np.any(want[0][..., cn.WRAP_AXES] != 0)
    assert np.any(want[0] != _ungated(spec).evaluate(pool)[0]) and np.any(want[0][:, 0] != want[0][:, 1])
    _same(eng.connectivity(pool, labels=True), want)
    eng.set_state(occ, np.arange(R, dtype=np.uint64) + np.uint64(9), 4000.0)
    eng.run(200, sync=True)
    _same(eng.connectivity(labels=True), spec.evaluate(eng.get_state()["occupancy"]))
    smp = eng.run_sampled(2, 9, connectivity=True)
    np.testing.assert_array_equal(smp["connectivity"], spec.evaluate(smp["occupancy"])[0])
    eng.close()


# ---- 7: the ring and the statistics record ------------------------------------------------------------------------------------------
def test_ring_column_equals_the_definition_and_the_chain_does_not_change(clean_env):
    from smol_amd.engine import Engine

    name, R = "fcc_conv444_pairs", 3
    sc = load_case(name)["sc"]
    eng = Engine(tables_for(name, INT), capi.make_config(R, capi.KERNEL_METROPOLIS, capi.STEP_SWAP))
    spec = Connectivity.from_supercell(sc, [_tetra([0], NN + 0.01, 0), dict(members=[1], cutoff=NNN + 0.01), _tetra([0], NN + 0.01, 1)])
    eng.set_connectivity(spec)
    occ = member_rows(sc.num_sites, np.random.default_rng(21), (0.62,), per=R)
    seeds = np.arange(R, dtype=np.uint64) + np.uint64(31)
    eng.set_state(occ, seeds, 3000.0)
    eng.run(11)
    smp = eng.run_sampled(3, 7, connectivity=True)
    assert smp["occupancy"].shape == (3, R, eng.N) and smp["connectivity"].shape == (3, R, 3, 24)
    want = spec.evaluate(smp["occupancy"])[0]
    np.testing.assert_array_equal(smp["connectivity"], want)
    assert np.any(want != _ungated(spec).evaluate(smp["occupancy"])[0]) and np.any(want[..., 0, cn.N_COMPONENTS] > 1)
    final = eng.get_state()
    # without the occupancy column: the same column, the rows stay on the device
    eng.set_state(occ, seeds, 3000.0)
    eng.run(11)
    dry = eng.run_sampled(3, 7, occupancy=False, connectivity=True)
    assert dry["occupancy"] is None
    np.testing.assert_array_equal(dry["connectivity"], smp["connectivity"])
    # a run without the flag: enthalpy, features, accept flags, occupancies and the final state are identical
    eng.set_state(occ, seeds, 3000.0)
    eng.run(11)
    plain = eng.run_sampled(3, 7)
    assert "connectivity" not in plain
    for key in plain:
        assert np.array_equal(plain[key], smp[key]), key
    after = eng.get_state()
    for key in final:
        assert np.array_equal(final[key], after[key]), key
    eng.close()


def test_statistics_record_with_columns_of_a_gated_graph(clean_env):
    R = 12
    eng, obs, sc = _semigrand("fcc_conv444_pairs", R)
    spec_c = Connectivity.from_supercell(sc, [dict(members=[1], cutoff=NN + 0.01), _tetra([1], NN + 0.01, 0)], observables=obs)
    eng.set_connectivity(spec_c)
    spec = Statistics.per_walker([st.ENTHALPY, st.connectivity(1, cn.WRAPPING_SITES), st.connectivity(1, cn.N_MEMBERS),
                                  st.connectivity(1, cn.WRAP_AXES), st.connectivity(1, cn.LARGEST), st.connectivity(0, cn.LARGEST)], n_levels=3,
                                 hist=(st.connectivity(1, cn.LARGEST), 16, 0.0, 256.0))
    eng.set_statistics(spec)
    occ0 = 1 - member_rows(sc.num_sites, np.random.default_rng(5), (0.6,), per=R)  # (code 1, the member, on six sites in ten)
    seeds = np.arange(R, dtype=np.uint64) + np.uint64(11)
    eng.set_state(occ0, seeds, 3000.0)
    eng.run_sampled_async(3, 5, statistics=True, connectivity=True)
    eng.run_sampled_async(4, 5, statistics=True, connectivity=True)
    want = StatisticsRecord(spec, R)
    for b in (eng.fetch_samples(), eng.fetch_samples()):
        conn = spec_c.evaluate(b["occupancy"])[0]
        np.testing.assert_array_equal(b["connectivity"], conn)
        assert np.any(conn[..., 0, :] != conn[..., 1, :])
        want.offer(b["enthalpy"], b["features"], connectivity=conn)
    _same_record(eng.statistics(), want, "two blocks")
    # the same record with nothing but the statistics asked for: rows and stats stay on the device
    eng.set_statistics(spec)
    eng.set_state(occ0, seeds, 3000.0)
    eng.run_sampled_async(3, 5, statistics=True, occupancy=False)
    eng.run_sampled_async(4, 5, statistics=True, occupancy=False)
    assert all(d["occupancy"] is None for d in (eng.fetch_samples(), eng.fetch_samples()))
    _same_record(eng.statistics(), want, "alone")
    eng.set_statistics(None)
    eng.close()


# ---- 8: the refusals ----------------------------------------------------------------------------------------------------------------
def _raw(eng, spec, **kw):
    """smolmc_set_connectivity_gated with the arrays of ``spec``, those named in ``kw`` replaced: the message of the refusal."""
    P = lambda a, ct: a.ctypes.data_as(C.POINTER(ct))  # noqa: E731
    s, keep = spec.c_struct()
    _, (mask, most, ptr, sites) = spec.c_gates()
    a = dict(kind_base=keep[0], gate_mask=mask, max_blocked=most, gate_ptr=ptr, gate_sites=sites)
    a.update(kw)
    kb = np.ascontiguousarray(a["kind_base"], dtype=np.int32)
    gm = np.ascontiguousarray(a["gate_mask"], dtype=np.uint64)
    mb = np.ascontiguousarray(a["max_blocked"], dtype=np.int32)
    gp = np.ascontiguousarray(a["gate_ptr"], dtype=np.int64)
    gs = np.ascontiguousarray(a["gate_sites"], dtype=np.int32)
    s.kind_base = P(kb, C.c_int32)
    g = capi.smolmc_conn_gates()
    g.gate_mask, g.max_blocked, g.gate_ptr, g.gate_sites = P(gm, C.c_uint64), P(mb, C.c_int32), P(gp, C.c_int64), P(gs, C.c_int32)
    assert eng._lib.smolmc_set_connectivity_gated(eng._h, C.byref(s), C.byref(g)) != 0
    return eng._lib.smolmc_last_error().decode()


def test_refusals_name_their_reason_and_leave_the_spec(clean_env):
    from smol_amd.engine import Engine

    name = "fcc_conv444_pairs"
    sc = load_case(name)["sc"]
    eng = Engine(tables_for(name, INT), capi.make_config(2))
    N = sc.num_sites
    good = Connectivity.from_supercell(sc, [_tetra([0], NN + 0.01, 0)])
    eng.set_connectivity(good)
    gates = eng.connectivity_gates()
    pool = _frac_occ(sc, np.random.default_rng(2), (0.6,), per=2)
    want = good.evaluate(pool)
    # a small spec to spoil: bonds (0, 1) and (2, 3), one row with gates 4, 5 and one with gate 6
    small = Connectivity(good.kind_base, 2, [Graph([0], [(0, 1), (2, 3)], None, [[4, 5], [6]], [0])], site_ncodes=good.site_ncodes)

    def refused(spec=small, **kw):
        msg = _raw(eng, spec, **kw)
        assert eng.connectivity_shape() == (1, 2) and eng.connectivity_gates() == gates  # the handle is as it was
        _same(eng.connectivity(pool, labels=True), want)
        return msg

    assert f"bond row 1 has gate site {N}, {N} sites: gate site out of range" in refused(gate_sites=[4, 5, N])
    assert "bond row 0 has gate site -1" in refused(gate_sites=[-1, 5, 6])
    kb = good.kind_base.copy()
    kb[5] = -1
    assert "bond row 0 has gate site 5 with kind_base -1: a gate site must be a counted site" in refused(kind_base=kb)
    assert "bond row 0 has 5 gate sites, SMOLMC_MAX_CONN_GATES = 4: too many gates on a row" in refused(gate_ptr=[0, 5, 6],
                                                                                                        gate_sites=[4, 5, 6, 7, 8, 9])
    assert "gate_ptr[0] must be 0" in refused(gate_ptr=[1, 2, 3])
    assert "gate_ptr must not decrease" in refused(gate_ptr=[0, 2, 1])
    assert "graph 0 names gate kind 2, n_kinds is 2: kind out of range" in refused(gate_mask=[[5, 0, 0, 0]])
    assert "graph 0 names gate kind 130, n_kinds is 2: kind out of range" in refused(gate_mask=[[1, 0, 4, 0]])
    for bad in (-1, 5):
        assert f"graph 0 has max_blocked = {bad}, outside 0..SMOLMC_MAX_CONN_GATES = 4: max_blocked out of range" in refused(max_blocked=[bad])
    # a site of a gated graph with 70 neighbour entries: beyond the 64 the open-bit plan has room for; ungated it is accepted
    star = [(0, j) for j in range(1, 71)]
    wide = Connectivity(good.kind_base, 2, [Graph([0], star, None, [[j] for _, j in star], [0])], site_ncodes=good.site_ncodes)
    msg = refused(wide)
    assert "graph 0 is gated and a site has 70 neighbour entries, SMOLMC_MAX_CONN_GATED_NEIGHBOURS = 64" in msg
    # the limit itself, and what was refused above: accepted
    edge = Connectivity(good.kind_base, 2, [Graph([0], star[:64], None, [[j, j, 0, 0] for _, j in star[:64]], [0], 4)],
                        site_ncodes=good.site_ncodes)
    eng.set_connectivity(edge)
    _same(eng.connectivity(pool, labels=True), edge.evaluate(pool))
    eng.set_connectivity(_ungated(wide))
    _same(eng.connectivity(pool, labels=True), _ungated(wide).evaluate(pool))
    with pytest.raises(ValueError, match="defined on 8 sites"):
        eng.set_connectivity(Connectivity(np.zeros(8, np.int32), 2, [Graph([0], [(0, 1)], None, [[2]], [0])]))
    eng.close()


def test_a_gated_row_that_overflows_lds_is_refused_with_its_bytes(clean_env):
    """4096 sites with the 42 neighbours of three shells: 11 groups, 44 open bits, 6 bytes a site on top of 49552."""
    eng, sc = _fcc_handle([16, 16, 16], R=1)
    shells = Connectivity.from_supercell(sc, [dict(members=[0], cutoff=5.1)])
    g = shells.graphs[0]
    assert len(g.bonds) == 4096 * 42 and capi.connectivity_open_bytes(42) == 6
    assert capi.connectivity_lds_bytes(4096, 4096, 6) is None and capi.connectivity_lds_bytes(4096, 4096) == 49552
    gated = Connectivity(shells.kind_base, shells.n_kinds, [Graph([0], g.bonds, g.images, g.bonds[:, :1], [0])], site_ncodes=shells.site_ncodes)
    with pytest.raises(ERR, match="a gated row of 4096 sites is too long for the LDS plan: 6 bytes of open bits a site next to the rest "
                                  "make 74128 bytes, 65536 at most"):
        eng.set_connectivity(gated)
    assert eng.connectivity_shape() == (0, 0)
    eng.set_connectivity(shells)
    assert eng.connectivity_shape() == (1, 2)
    occ = member_rows(4096, np.random.default_rng(1), (0.1,), per=1)
    _same(eng.connectivity(occ, labels=True), shells.evaluate(occ))
    eng.close()


# ---- 9: the sampler -------------------------------------------------------------------------------------------------------------------
def test_sampler_traces_a_gated_spec(clean_env, tmp_path):
    c = load_case("rocksalt333_two_sublattices")
    ens = moca.Ensemble.from_cluster_expansion(c["sc"], c["coefs"])
    spec = rocksalt_cation_spec(c["sc"], (0, 1))
    nw = 6
    occ = _frac_occ(c["sc"], np.random.default_rng(12), (0.6,), per=nw)

    def sampler():
        return moca.Sampler.from_ensemble(ens, temperature=3000.0, nwalkers=nw, seeds=list(range(3, 3 + nw)), rank=0, world_size=1,
                                          connectivity=spec)

    traced, dry = sampler(), sampler()
    traced.run(10 * 9, occ, thin_by=9)
    smp = traced.samples
    conn = smp.get_trace_value("connectivity", flat=False)
    assert conn.shape == (10, nw, 2, 24) and conn.dtype == np.int64
    want = spec.evaluate(smp.get_occupancies(flat=False))[0]
    np.testing.assert_array_equal(conn, want)
    assert np.any(want != _ungated(spec).evaluate(smp.get_occupancies(flat=False))[0])
    meta = smp.metadata["connectivity"]
    assert meta["gate_kinds"] == [[0], [0]] and meta["max_blocked"] == [0, 1] and meta["n_gated_rows"] == [27 * 24] * 2
    dry.run(10 * 9, occ, thin_by=9, keep_occupancy=False)
    np.testing.assert_array_equal(dry.samples.get_trace_value("connectivity", flat=False), conn)
    np.testing.assert_array_equal(dry.samples.last_occupancy(), smp.last_occupancy())
    path = str(tmp_path / "samples.npz")
    smp.to_npz(path)
    back = moca.SampleContainer.from_npz(path, ens)
    assert back.metadata["connectivity"] == meta
    np.testing.assert_array_equal(back.get_trace_value("connectivity", flat=False), conn)
