"""Gated bonds on the host (smol_amd/connectivity.py): a bond row with gate sites is open when at most ``max_blocked`` of them
hold a kind outside ``gate_kinds``.  Hand-made ladders with answers worked out by hand, the ways rows combine, the channel
geometry of ``from_supercell(gate=...)``, ``evaluate`` against SciPy and against the union-find of the ungated host tests fed
with rows opened by a loop written here, the ungated spec as it was, and the refusals."""

import ctypes
import itertools

import numpy as np
import pytest

from smol_amd import capi, synth
from smol_amd import connectivity as cn
from smol_amd.connectivity import Connectivity, Graph
from tests.cases import load_case
from tests.test_connectivity_host import union_find_stats

NN = 4.09 / np.sqrt(2.0)  # nearest-neighbour distance of the fcc cases (a = 4.09)
TETRA = dict(kinds=[0], corners=2)


# ---- shared with the GPU tests -------------------------------------------------------------------------------------------
def ladder(M, order=None, n_sites=None):
    """A ring of M chain sites closed by image (1, 0, 0), bond p = (chain p, chain p + 1) gated by gate site p.  ``order``
    (2M site numbers) places chain position p on site order[p] and gate p on site order[M + p]; sites beyond 2M
    (``n_sites``) are in no graph.  Every site holds codes 0/1: chain sites have kinds 0/1 (1 the member), gate sites kinds
    2/3 (3 lets through)."""
    order = list(range(2 * M)) if order is None else [int(x) for x in order]
    N = 2 * M if n_sites is None else n_sites
    kb = np.full(N, -1, dtype=np.int32)
    kb[order[:M]], kb[order[M:]] = 0, 2
    bonds = [(order[p], order[(p + 1) % M]) for p in range(M)]
    images = [(0, 0, 0)] * (M - 1) + [(1, 0, 0)]
    gates = [[order[M + p]] for p in range(M)]
    return Connectivity(kb, 4, [Graph([1], bonds, images, gates, gate_kinds=[3])], site_ncodes=np.full(N, 2))


def ladder_rows(M, order=None, n_sites=None):
    """(occupancies, the expected (N_COMPONENTS, LARGEST, WRAP_AXES, sorted sizes) per row) of ``ladder``: all gates open;
    gate 5 closed; gates 5 and M - 3 closed; the gate of the closing bond closed."""
    order = list(range(2 * M)) if order is None else [int(x) for x in order]
    N = 2 * M if n_sites is None else n_sites
    occ = np.zeros((4, N), dtype=np.int32)
    occ[:, order] = 1
    occ[1, order[M + 5]] = 0
    occ[2, order[M + 5]] = occ[2, order[M + M - 3]] = 0
    occ[3, order[M + M - 1]] = 0
    inner = (M - 3) - 5  # chain positions 6 .. M - 3 are cut off from the rest
    return occ, [(1, M, 1, [M]), (1, M, 0, [M]), (2, max(inner, M - inner), 0, sorted([inner, M - inner])), (1, M, 0, [M])]


def check_ladder(stats, labels, want, order, M):
    for r, (ncomp, largest, axes, sizes) in enumerate(want):
        s = stats[r, 0]
        assert (s[cn.N_MEMBERS], s[cn.N_COMPONENTS], s[cn.LARGEST], s[cn.WRAP_AXES]) == (M, ncomp, largest, axes), r
        assert s[cn.SUM_SQ] == sum(x * x for x in sizes) and s[cn.N_WRAPPING] == (1 if axes else 0)
        lab = labels[r, 0]
        chain = np.asarray(order[:M])
        assert sorted(np.unique(lab[chain], return_counts=True)[1].tolist()) == sizes
        assert np.all(lab[np.asarray(order[M:])] == -1)


def fcc_cell(dims):
    return synth.build_supercell(synth.build_cluster_model(synth.fcc_prim(), {2: 3.0}), dims)


def member_rows(n_sites, rng, fractions, per=1):
    """Binary rows: code 0 (the member and the kind that lets through) with probability p."""
    return np.concatenate([(rng.random((per, n_sites)) >= p).astype(np.int32) for p in fractions])


def open_rows_by_hand(spec, g, occ):
    """The open rows of graph g in ONE occupancy, by a loop that shares no code with ``Connectivity.open_rows``."""
    gr = spec.graphs[g]
    kind = [int(spec.kind_base[s]) + int(occ[s]) if spec.kind_base[s] >= 0 else -1 for s in range(spec.num_sites)]
    out = []
    for (i, j), gates in zip(gr.bonds.tolist(), gr.gates.tolist()):
        blocked = sum(1 for t in gates if t >= 0 and kind[t] not in gr.gate_kinds)
        out.append(kind[i] in gr.members and kind[j] in gr.members and blocked <= gr.max_blocked)
    return np.asarray(out, dtype=bool)


def check_against_union_find(spec, occ):
    """``evaluate`` of every row equals the union-find of the ungated host tests over the rows opened by hand."""
    stats, labels = spec.evaluate(occ)
    for r in range(len(occ)):
        graphs = []
        for g, gr in enumerate(spec.graphs):
            keep = open_rows_by_hand(spec, g, occ[r])
            np.testing.assert_array_equal(spec.open_rows(occ[r], g), keep)
            graphs.append((set(gr.members), gr.bonds[keep], gr.images[keep].astype(np.int64)))
        ws, wl = union_find_stats(spec.kind_base, spec.n_kinds, graphs, occ[r])
        np.testing.assert_array_equal(stats[r], ws)
        np.testing.assert_array_equal(labels[r], wl)
    return stats, labels


# ---- the ladder ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [12, 33])
def test_ladder_known_answers(M):
    spec = ladder(M)
    occ, want = ladder_rows(M)
    stats, labels = check_against_union_find(spec, occ)
    check_ladder(stats, labels, want, list(range(2 * M)), M)
    # permuted, with sites that are in no graph
    order = np.random.default_rng(M).permutation(2 * M + 3)[: 2 * M]
    spec = ladder(M, order, 2 * M + 3)
    occ, want = ladder_rows(M, order, 2 * M + 3)
    stats, labels = check_against_union_find(spec, occ)
    check_ladder(stats, labels, want, [int(x) for x in order], M)


# ---- how rows combine ------------------------------------------------------------------------------------------------------
def _two_sites(rows, max_blocked=0, n_gate_sites=4):
    """Sites 0 and 1 (kinds 0/1, 1 the member) and gate sites 2.. (kinds 2/3, 3 lets through); rows = (i, j, w, gates)."""
    N = 2 + n_gate_sites
    kb = np.array([0, 0] + [2] * n_gate_sites, dtype=np.int32)
    return Connectivity(kb, 4, [Graph([1], [r[:2] for r in rows], [r[2] for r in rows], [list(r[3]) for r in rows], gate_kinds=[3],
                                      max_blocked=max_blocked)], site_ncodes=np.full(N, 2))


def _joined(spec, occ):
    stats, labels = spec.evaluate(np.asarray(occ, dtype=np.int32))
    return int(stats[0, cn.LARGEST]) == 2 and labels[0, 1] == 0


def test_two_rows_of_one_bond_open_if_either_is():
    spec = _two_sites([(0, 1, (0, 0, 0), [2]), (0, 1, (0, 0, 0), [3])])
    for a, b in itertools.product((0, 1), repeat=2):
        assert _joined(spec, [1, 1, a, b, 1, 1]) == bool(a or b)
        np.testing.assert_array_equal(spec.open_rows(np.array([1, 1, a, b, 1, 1]), 0), [bool(a), bool(b)])
    # the same bond listed from the other end with the other gate: still one adjacency
    spec = _two_sites([(0, 1, (0, 0, 0), [2]), (1, 0, (0, 0, 0), [3])])
    for a, b in itertools.product((0, 1), repeat=2):
        assert _joined(spec, [1, 1, a, b, 1, 1]) == bool(a or b)
    # ... but a different image is a different adjacency: closed gates on the direct bond leave the wrapping one
    spec = _two_sites([(0, 1, (0, 0, 0), [2]), (0, 1, (0, 1, 0), [3])])
    s = spec.evaluate(np.array([1, 1, 0, 1, 1, 1]))[0][0]
    assert s[cn.LARGEST] == 2 and s[cn.WRAP_AXES] == 0
    s = spec.evaluate(np.array([1, 1, 1, 1, 1, 1]))[0][0]
    assert s[cn.LARGEST] == 2 and s[cn.WRAP_AXES] == 2


def test_a_gate_free_duplicate_row_is_always_open():
    spec = _two_sites([(0, 1, (0, 0, 0), [2, 3]), (1, 0, (0, 0, 0), [])])
    assert spec.graphs[0].gated
    assert _joined(spec, [1, 1, 0, 0, 0, 0]) and not _joined(spec, [1, 0, 1, 1, 1, 1])


def test_a_row_in_one_direction_opens_the_reverse():
    """The bond is listed as (1, 0) only: site 1 still takes the label of site 0 over it."""
    spec = _two_sites([(1, 0, (0, 0, -1), [2])])
    stats, labels = spec.evaluate(np.array([[1, 1, 1, 0, 0, 0], [1, 1, 0, 1, 1, 1]], dtype=np.int32))
    assert labels[0, 0].tolist()[:2] == [0, 0] and labels[1, 0].tolist()[:2] == [0, 1]
    assert stats[0, 0, cn.WRAP_AXES] == 0 and stats[1, 0, cn.N_COMPONENTS] == 2


@pytest.mark.parametrize("max_blocked", range(5))
def test_max_blocked_on_a_four_gate_row(max_blocked):
    spec = _two_sites([(0, 1, (0, 0, 0), [2, 3, 4, 5])], max_blocked=max_blocked)
    for gates in itertools.product((0, 1), repeat=4):
        assert _joined(spec, [1, 1, *gates]) == (4 - sum(gates) <= max_blocked), gates


def test_a_gate_that_is_an_end_and_a_site_listed_twice():
    # gate = end 1 of its own bond; every site has kinds 0/1, member kind 1, gate kinds [1]: the member lets through
    kb = np.zeros(3, dtype=np.int32)
    spec = Connectivity(kb, 2, [Graph([1], [(0, 1)], None, [[1]], gate_kinds=[1])], site_ncodes=np.full(3, 2))
    assert spec.evaluate(np.array([1, 1, 0]))[0][0, cn.LARGEST] == 2
    # ... and with gate kinds [0] an end that is a member blocks its own bond
    spec = Connectivity(kb, 2, [Graph([1], [(0, 1)], None, [[1]], gate_kinds=[0])], site_ncodes=np.full(3, 2))
    assert spec.evaluate(np.array([1, 1, 0]))[0][0, cn.LARGEST] == 1
    # site 2 twice on a row: blocked, it counts twice
    for max_blocked, joined in ((0, False), (1, False), (2, True)):
        spec = Connectivity(kb, 2, [Graph([1], [(0, 1)], None, [[2, 2]], gate_kinds=[1], max_blocked=max_blocked)],
                            site_ncodes=np.full(3, 2))
        assert (spec.evaluate(np.array([1, 1, 0]))[0][0, cn.LARGEST] == 2) == joined
        assert spec.evaluate(np.array([1, 1, 1]))[0][0, cn.LARGEST] == 2
        ptr, sites = spec.graphs[0].gate_lists()
        assert ptr.tolist() == [0, 2] and sites.tolist() == [2, 2]


# ---- geometry ---------------------------------------------------------------------------------------------------------------
def _positions(sc):
    """(cartesian positions (N, 3), the supercell vectors as rows (3, 3))."""
    from smol_amd.structure import lattice_points_of

    prim = sc.model.prim
    L, tau = np.asarray(prim.lattice, dtype=float), np.asarray(prim.frac_coords, dtype=float)
    S = np.asarray(sc.scmatrix, dtype=np.int64)
    S = np.diag(S) if S.ndim == 1 else S
    n = lattice_points_of(sc)
    site_t = np.asarray(getattr(sc, "site_t", np.arange(sc.num_sites) % len(n)), dtype=np.int64)
    return (n[site_t] + tau[np.asarray(sc.site_b)]) @ L, S.astype(float) @ L


IMAGES = np.array(list(itertools.product(range(-2, 3), repeat=3)), dtype=float)


def _near(pos, cell, k, points, r):
    """The positions of the images of site k that lie at distance r from every one of ``points``."""
    cand = pos[k] + IMAGES @ cell
    ok = np.ones(len(cand), dtype=bool)
    for p in points:
        ok &= np.abs(np.linalg.norm(cand - p, axis=1) - r) < 1e-6
    return cand[ok]


@pytest.mark.parametrize("dims,sites,rows", [([4, 4, 4], 64, 1536), ([7, 7, 7], 343, 8232), ([16, 16, 16], 4096, 98304)])
def test_channel_row_counts(dims, sites, rows):
    sc = fcc_cell(dims)
    spec = Connectivity.from_supercell(sc, [dict(members=[0], cutoff=NN + 0.01, gate=TETRA)])
    g = spec.graphs[0]
    assert sc.num_sites == sites and g.bonds.shape == (rows, 2) and g.gates.shape == (rows, 2) and g.gates.min() >= 0
    assert g.gate_kinds == [0] and g.max_blocked == 0 and g.gated and spec.gated
    # two channels for each of the 12 directed bonds of every site
    plain = Connectivity.from_supercell(sc, [dict(members=[0], cutoff=NN + 0.01)]).graphs[0]
    assert len(plain.bonds) * 2 == rows
    np.testing.assert_array_equal(g.bonds[::2], plain.bonds)
    np.testing.assert_array_equal(g.images[1::2], plain.images)


def test_fcc_channels_are_tetrahedra_and_triangles():
    sc = fcc_cell([4, 4, 4])
    pos, cell = _positions(sc)
    tet = Connectivity.from_supercell(sc, [dict(members=[0], cutoff=NN + 0.01, gate=TETRA)]).graphs[0]
    for (i, j), w, (k, l) in zip(tet.bonds.tolist(), tet.images.astype(float), tet.gates.tolist()):
        ri, rj = pos[i], pos[j] + w @ cell
        assert abs(np.linalg.norm(rj - ri) - NN) < 1e-6
        ks, ls = _near(pos, cell, k, (ri, rj), NN), _near(pos, cell, l, (ri, rj), NN)
        d = np.linalg.norm(ks[:, None, :] - ls[None, :, :], axis=2)
        assert len(ks) and len(ls) and np.any(np.abs(d - NN) < 1e-6), (i, j, k, l)
    # one corner: the four common neighbours of a nearest-neighbour pair
    tri = Connectivity.from_supercell(sc, [dict(members=[0], cutoff=NN + 0.01, gate=dict(kinds=[0], corners=1))]).graphs[0]
    assert tri.gates.shape == (64 * 12 * 4, 1)
    seen = {}
    for (i, j), w, (k,) in zip(tri.bonds.tolist(), tri.images.tolist(), tri.gates.tolist()):
        ri, rj = pos[i], pos[j] + np.asarray(w, dtype=float) @ cell
        assert len(_near(pos, cell, k, (ri, rj), NN)) >= 1
        seen.setdefault((i, j, tuple(w)), set()).add(k)
    assert all(len(v) == 4 for v in seen.values()) and len(seen) == 64 * 12
    # every tetrahedron's corners are among the common neighbours of its bond
    for (i, j), w, (k, l) in zip(tet.bonds.tolist(), tet.images.tolist(), tet.gates.tolist()):
        assert {k, l} <= seen[(i, j, tuple(w))]


def test_aliased_cell_gates_coincide_and_still_evaluate():
    sc = load_case("fcc_prim222_aliased")["sc"]
    # (cutoff 6.0: a site is bonded to its own images, and a corner of a channel may be an end's image or the other corner's)
    spec = Connectivity.from_supercell(sc, [dict(members=[0], cutoff=6.0, gate=dict(kinds=[0], corners=1)),
                                            dict(members=[0], cutoff=6.0, gate=TETRA)])
    one, two = spec.graphs
    assert sc.num_sites == 8 and len(one.bonds) == 10080 and len(two.bonds) == 75840
    assert ((one.gates == one.bonds[:, :1]) | (one.gates == one.bonds[:, 1:])).any()
    assert ((two.gates == two.bonds[:, :1]) | (two.gates == two.bonds[:, 1:])).any() and (two.gates[:, 0] == two.gates[:, 1]).any()
    occ = member_rows(8, np.random.default_rng(3), (0.3, 0.5, 0.8), per=2)
    stats, _ = check_against_union_find(spec, occ)
    assert np.any(stats[..., cn.WRAP_AXES] != 0)
    # the gates close rows whose ends are members (whether that parts a component of so dense a graph is another matter)
    ends = (occ[:, one.bonds[:, 0]] == 0) & (occ[:, one.bonds[:, 1]] == 0)
    assert np.any(ends & ~spec.open_rows(occ, 0)) and np.any(spec.open_rows(occ, 0))


def rocksalt_cation_spec(sc, max_blocked=(0,), kinds=(0,), site_classes=None):
    """Gates on the cation sublattice of a rocksalt: the nearest cation-cation bonds (a / sqrt 2 = 2.97; the cutoff also
    takes the cation-anion bonds, which are dropped here), their tetrahedra of cations as gates; ``kinds`` are the members
    and the kinds that let through.  One graph per entry of ``max_blocked``."""
    plain = Connectivity.from_supercell(sc, [dict(members=list(kinds), cutoff=3.0)], site_classes=site_classes)
    g = plain.graphs[0]
    cation = np.asarray(sc.site_b)[g.bonds] == np.asarray(sc.site_b)[int(np.flatnonzero(plain.kind_base == 0)[0])]
    keep = cation.all(axis=1)
    bonds, images, gates = cn.channel_rows(g.bonds[keep], g.images[keep], corners=2)
    return Connectivity(plain.kind_base, plain.n_kinds, [Graph(kinds, bonds, images, gates, kinds, m) for m in max_blocked],
                        site_ncodes=plain.site_ncodes)


def test_species_names_and_two_sublattices():
    sc = load_case("rocksalt333_two_sublattices")["sc"]
    # with the cutoff alone a channel may have an anion for a corner: an anion has no kind that lets through
    names = sc.model.prim.species[0]
    byname = Connectivity.from_supercell(sc, [dict(members=[names[0]], cutoff=3.0, gate=dict(kinds=[names[0]], corners=2))])
    bykind = Connectivity.from_supercell(sc, [dict(members=[0], cutoff=3.0, gate=dict(kinds=[0], corners=2))])
    assert byname.graphs[0].gate_kinds == bykind.graphs[0].gate_kinds == [0] and byname.graphs[0].members == [0]
    np.testing.assert_array_equal(byname.graphs[0].gates, bykind.graphs[0].gates)
    # the cation sublattice alone: 27 cations, 12 directed bonds each, two tetrahedra a bond
    spec = rocksalt_cation_spec(sc, (0, 1))
    assert len(spec.graphs[0].bonds) == 27 * 12 * 2 and np.all(spec.kind_base[spec.graphs[0].gates] == 0)
    nsp = np.array([sc.model.prim.nspecies[b] for b in sc.site_b])
    rng = np.random.default_rng(5)
    occ = np.where(rng.random((8, sc.num_sites)) < 0.6, 0, np.minimum(1 + (rng.random((8, sc.num_sites)) * (nsp - 1)).astype(int), nsp - 1))
    stats, _ = check_against_union_find(spec, occ.astype(np.int32))
    assert np.any(stats[:, 0] != stats[:, 1])


# ---- evaluate against SciPy ------------------------------------------------------------------------------------------------
def test_evaluate_against_scipy_on_both_sides_of_the_transition():
    sparse = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components

    sc = fcc_cell([7, 7, 7])
    N = sc.num_sites
    spec = Connectivity.from_supercell(sc, [dict(members=[0], cutoff=NN + 0.01, gate=TETRA),
                                            dict(members=[0], cutoff=NN + 0.01, gate=dict(kinds=[0], corners=2, max_blocked=1))])
    occ = member_rows(N, np.random.default_rng(11), (0.30, 0.45, 0.55, 0.65, 0.80), per=2)
    stats, labels = spec.evaluate(occ)
    # the 0-TM threshold lies near 0.55: far below it no cluster wraps and the largest holds a small part of the members,
    # far above it one cluster wraps and holds most of them
    share = (stats[:, 0, cn.LARGEST] / stats[:, 0, cn.N_MEMBERS]).reshape(5, 2)
    wraps = (stats[:, 0, cn.WRAP_AXES] != 0).reshape(5, 2)
    assert share[0].max() < 0.5 and not wraps[0].any() and share[4].min() > 0.5 and wraps[4].all(), (share, wraps)
    assert np.all(stats[:, 1, cn.LARGEST] >= stats[:, 0, cn.LARGEST]) and np.any(stats[:, 1] != stats[:, 0])
    for r in range(len(occ)):
        for g, gr in enumerate(spec.graphs):
            keep = spec.open_rows(occ[r], g)
            i, j = gr.bonds[keep, 0], gr.bonds[keep, 1]
            m = sparse.coo_matrix((np.ones(len(i)), (i, j)), shape=(N, N))
            ncomp, comp = connected_components(m, directed=False)
            member = occ[r] == 0
            sizes = np.bincount(comp[member], minlength=ncomp)
            sizes = sizes[sizes > 0]
            s = stats[r, g]
            assert (s[cn.N_MEMBERS], s[cn.N_COMPONENTS], s[cn.LARGEST], s[cn.SUM_SQ]) == (member.sum(), len(sizes), sizes.max(), (sizes ** 2).sum())
            # the labels are the same partition, named by the smallest site
            lab = labels[r, g]
            assert np.all(lab[~member] == -1)
            for c in np.unique(comp[member]):
                sites = np.flatnonzero(member & (comp == c))
                assert np.all(lab[sites] == sites.min())
    check_against_union_find(spec, occ[[0, 4, 9]])


# ---- the ungated spec is what it was ---------------------------------------------------------------------------------------
def test_ungated_spec_is_unchanged():
    sc = fcc_cell([3, 3, 3])
    spec = Connectivity.from_supercell(sc, [dict(members=[0], cutoff=NN + 0.01), dict(members=[1], cutoff=4.1)])
    assert not spec.gated and spec.c_gates() is None and all(g.gates.shape == (len(g.bonds), 0) for g in spec.graphs)
    assert sorted(spec.to_metadata()) == ["members", "n_bonds", "n_graphs", "n_kinds"]
    s, keep = spec.c_struct()
    assert isinstance(s, capi.smolmc_connectivity) and len(keep) == 5
    kb, mask, ptr, bonds, images = keep
    assert (kb.dtype, mask.dtype, ptr.dtype, bonds.dtype, images.dtype) == (np.int32, np.uint64, np.int64, np.int32, np.int8)
    want = [spec.kind_base, spec.member_masks(), np.cumsum([0] + [len(g.bonds) for g in spec.graphs]),
            np.concatenate([g.bonds for g in spec.graphs]), np.concatenate([g.images for g in spec.graphs])]
    for got, w in zip(keep, want):
        assert got.tobytes() == np.ascontiguousarray(w, dtype=got.dtype).tobytes()
    assert ctypes.sizeof(capi.smolmc_connectivity) == 56
    # a gates array that names no site is no gate; the spec evaluates as without
    occ = member_rows(sc.num_sites, np.random.default_rng(1), (0.2, 0.5), per=3)
    g0 = spec.graphs[0]
    blank = Connectivity(spec.kind_base, spec.n_kinds, [Graph(g0.members, g0.bonds, g0.images, np.full((len(g0.bonds), 2), -1), [1], 3),
                                                        spec.graphs[1]], site_ncodes=spec.site_ncodes)
    assert not blank.gated and blank.c_gates() is None
    for a, b in zip(blank.evaluate(occ), spec.evaluate(occ)):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(spec.open_rows(occ, 0), (occ[:, g0.bonds[:, 0]] == 0) & (occ[:, g0.bonds[:, 1]] == 0))
    assert capi.connectivity_lds_bytes(4096, 4096) == capi.connectivity_lds_bytes(4096, 4096, 0) == 49552


def test_gated_spec_c_struct_metadata_and_lds_plan():
    sc = fcc_cell([4, 4, 4])
    spec = Connectivity.from_supercell(sc, [dict(members=[0], cutoff=NN + 0.01),
                                            dict(members=[0], cutoff=NN + 0.01, gate=dict(kinds=[0, 1], corners=1, max_blocked=1))])
    assert spec.gated and not spec.graphs[0].gated
    s, keep = spec.c_struct()
    assert len(keep) == 5
    g, (mask, most, ptr, sites) = spec.c_gates()
    assert isinstance(g, capi.smolmc_conn_gates) and ctypes.sizeof(capi.smolmc_conn_gates) == 32
    nb0, nb1 = (len(x.bonds) for x in spec.graphs)
    assert mask.tolist() == [[0, 0, 0, 0], [3, 0, 0, 0]] and most.tolist() == [0, 1]
    assert ptr.tolist() == [0] * (nb0 + 1) + list(range(1, nb1 + 1)) and sites.tolist() == spec.graphs[1].gates[:, 0].tolist()
    meta = spec.to_metadata()
    assert meta["gate_kinds"] == [[], [0, 1]] and meta["max_blocked"] == [0, 1] and meta["n_gated_rows"] == [0, nb1]
    assert meta["n_bonds"] == [nb0, nb1]
    # the plan: 12 neighbours are three groups, 12 bits, two bytes a site; config 2's row with them fits
    assert capi.connectivity_open_bytes(12) == 2 and capi.connectivity_open_bytes(8) == 1 and capi.connectivity_open_bytes(42) == 6
    assert capi.connectivity_lds_bytes(4096, 4096, 2) == 49552 + 8192
    assert capi.connectivity_lds_bytes(4096, 4096, 3) is not None and capi.connectivity_lds_bytes(4096, 4096, 4) is None


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason():
    kb = np.array([0, 0, 0, -1], dtype=np.int32)
    bonds = [(0, 1)]
    with pytest.raises(ValueError, match="5 gate sites, SMOLMC_MAX_CONN_GATES = 4: too many gates on a row"):
        Graph([0], bonds, None, [[2, 2, 2, 2, 2]])
    with pytest.raises(ValueError, match="too many gates on a row"):
        Graph([0], bonds, None, np.zeros((1, 5), dtype=np.int64))
    with pytest.raises(ValueError, match=r"gates must be an \(nbonds, m\) integer array"):
        Graph([0], bonds, None, [[2], [2]])
    with pytest.raises(ValueError, match=r"gates must be an \(nbonds, m\) integer array"):
        Graph([0], bonds, None, np.zeros((1, 2)))
    for bad in (-1, 5):
        with pytest.raises(ValueError, match=f"max_blocked must be 0..4, got {bad}: max_blocked out of range"):
            Graph([0], bonds, None, [[2]], [0], bad)
    with pytest.raises(ValueError, match="graph 0: gate site 4, 4 sites: gate site out of range"):
        Connectivity(kb, 2, [Graph([0], bonds, None, [[4]], [0])])
    with pytest.raises(ValueError, match="graph 0: gate site 3 has kind_base -1: a gate site must be a counted site"):
        Connectivity(kb, 2, [Graph([0], bonds, None, [[2, 3]], [0])])
    with pytest.raises(ValueError, match="graph 0: gate kind 2, n_kinds is 2: kind out of range"):
        Connectivity(kb, 2, [Graph([0], bonds, None, [[2]], [0, 2])])
    sc = fcc_cell([2, 2, 2])
    with pytest.raises(ValueError, match="corners must be 1 or 2, got 3"):
        Connectivity.from_supercell(sc, [dict(members=[0], cutoff=NN + 0.01, gate=dict(kinds=[0], corners=3))])
    with pytest.raises(ValueError, match=r"graph 0: gate=dict\(kinds=..., corners=1\|2, max_blocked=0\)"):
        Connectivity.from_supercell(sc, [dict(members=[0], cutoff=NN + 0.01, gate=dict(kind=[0]))])
    with pytest.raises(ValueError, match="graph 0: no counted site holds a species named 'Xx'"):
        Connectivity.from_supercell(sc, [dict(members=[0], cutoff=NN + 0.01, gate=dict(kinds=["Xx"]))])
