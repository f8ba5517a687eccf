"""Connectivity on the host (smol_amd/connectivity.py): the breadth-first definition against a weighted union-find written
here, exact known answers, the geometry of ``from_supercell``, the derived quantities, validation, the ctypes mirror and the
statistics columns fed by the connectivity numbers."""

import ctypes
import itertools
import os
import re

import numpy as np
import pytest

from smol_amd import capi, connectivity as cn, statistics as st
from smol_amd.connectivity import Connectivity, Graph
from tests.cases import load_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NN, NNN = 4.09 / np.sqrt(2.0), 4.09  # nearest and next-nearest distance of the fcc cases


# ---- the checker: a second implementation that shares no code with Connectivity.evaluate ------------------------------------
def union_find_stats(kind_base, n_kinds, graphs, occ):
    """(stats (G, 24), labels (G, N)) of ONE occupancy by a weighted union-find: every site keeps its displacement to its
    parent, a bond inside one tree whose displacements do not close marks the axes of the mismatch at the root."""
    N = len(kind_base)
    kinds = [int(kind_base[s]) + int(occ[s]) if kind_base[s] >= 0 else -1 for s in range(N)]
    stats = np.zeros((len(graphs), 24), dtype=np.int64)
    labels = np.full((len(graphs), N), -1, dtype=np.int32)
    for gi, (members, bonds, images) in enumerate(graphs):
        inside = [k in members for k in kinds]
        parent, disp, rank_size, axes = list(range(N)), [(0, 0, 0)] * N, [1] * N, [0] * N

        def find(x):
            path = []
            while parent[x] != x:
                path.append(x)
                x = parent[x]
            # compress: walk back from the root, summing the displacements
            for y in reversed(path):
                p = parent[y]
                if p != x:
                    disp[y] = tuple(a + b for a, b in zip(disp[y], disp[p]))
                    parent[y] = x
            return x

        for (i, j), w in zip(np.asarray(bonds).tolist(), np.asarray(images).tolist()):
            if not (inside[i] and inside[j]):
                continue
            ri, rj = find(i), find(j)
            di = disp[i] if i != ri else (0, 0, 0)
            dj = disp[j] if j != rj else (0, 0, 0)
            m = tuple(di[a] + w[a] - dj[a] for a in range(3))  # where rj lies as seen from ri
            if ri == rj:
                axes[ri] |= sum(1 << a for a in range(3) if m[a] != 0)
                continue
            if rank_size[ri] < rank_size[rj]:
                ri, rj, m = rj, ri, tuple(-x for x in m)
            parent[rj], disp[rj] = ri, m
            rank_size[ri] += rank_size[rj]
            axes[ri] |= axes[rj]
        comps = {}
        for s in range(N):
            if inside[s]:
                comps.setdefault(find(s), []).append(s)
        row = stats[gi]
        best = None
        for root, sites in comps.items():
            size, lab = len(sites), min(sites)
            labels[gi, sites] = lab
            row[0] += size
            row[1] += 1
            row[3] += size * size
            row[8 + int(np.floor(np.log2(size)))] += 1
            if axes[root]:
                row[4] += 1
                row[5] += size
                row[6] |= axes[root]
            if best is None or (size, -lab) > (best[0], -best[1]):
                best = (size, lab, axes[root])
        if best is not None:
            row[2], row[7] = best[0], best[2]
    return stats, labels


def check_against_union_find(spec, occ):
    stats, labels = spec.evaluate(occ)
    assert stats.dtype == np.int64 and labels.dtype == np.int32
    graphs = [(set(g.members), g.bonds, g.images) for g in spec.graphs]
    for r in range(len(occ)):
        ws, wl = union_find_stats(spec.kind_base, spec.n_kinds, graphs, occ[r])
        np.testing.assert_array_equal(stats[r], ws)
        np.testing.assert_array_equal(labels[r], wl)
    return stats, labels


def grid_bonds(shape):
    """Nearest-neighbour bonds of a simple periodic grid, each once (towards +a), with the image of the far end."""
    idx = np.arange(int(np.prod(shape))).reshape(shape)
    bonds, images = [], []
    for p in itertools.product(*[range(n) for n in shape]):
        for a in range(3):
            if shape[a] == 1:
                continue  # (no bond from a site to its own image)
            q = list(p)
            q[a] += 1
            w = [0, 0, 0]
            if q[a] == shape[a]:
                q[a], w[a] = 0, 1
            bonds.append((idx[p], idx[tuple(q)]))
            images.append(w)
    return np.array(bonds), np.array(images)


def _rand_occ(sc, rng, n, p=0.5):
    nsp = np.array([sc.model.prim.nspecies[b] for b in sc.site_b])
    occ = (rng.random((n, sc.num_sites)) * nsp).astype(np.int32)
    first = rng.random((n, sc.num_sites)) < p  # code 0 with probability p, the others share the rest
    return np.where(first, 0, np.maximum(occ, 1) % nsp).astype(np.int32)


# ---- 1. known answers --------------------------------------------------------------------------------------------------------
def test_all_members_on_fcc_prim_444_is_one_component_that_wraps_every_axis():
    from smol_amd import synth

    sc = synth.build_supercell(synth.build_cluster_model(synth.fcc_prim(), {2: 3.0}), [4, 4, 4])
    spec = Connectivity.from_supercell(sc, [dict(members=[0, 1], cutoff=NN + 0.01)])
    stats, labels = check_against_union_find(spec, np.zeros((1, 64), dtype=np.int32))
    row = stats[0, 0]
    assert row[cn.N_MEMBERS] == 64 and row[cn.N_COMPONENTS] == 1 and row[cn.LARGEST] == 64 and row[cn.SUM_SQ] == 64 * 64
    assert row[cn.N_WRAPPING] == 1 and row[cn.WRAPPING_SITES] == 64 and row[cn.WRAP_AXES] == 7 and row[cn.LARGEST_WRAP_AXES] == 7
    assert row[cn.HIST0 + 6] == 1 and row[cn.HIST0:].sum() == 1
    assert np.all(labels == 0)


@pytest.mark.parametrize("L", [5, 8])
def test_a_straight_line_wraps_its_axis_alone_and_not_at_all_when_cut(L):
    shape = (L, 3, 3)
    bonds, images = grid_bonds(shape)
    spec = Connectivity(np.zeros(L * 9, np.int32), 2, [Graph([1], bonds, images)])
    idx = np.arange(L * 9).reshape(shape)
    occ = np.zeros((2, L * 9), dtype=np.int32)
    occ[:, idx[:, 1, 2]] = 1
    occ[1, idx[2, 1, 2]] = 0  # the cut line
    stats, labels = check_against_union_find(spec, occ)
    a, b = stats[0, 0], stats[1, 0]
    assert (a[cn.N_MEMBERS], a[cn.N_COMPONENTS], a[cn.LARGEST], a[cn.WRAP_AXES], a[cn.N_WRAPPING], a[cn.WRAPPING_SITES]) == (L, 1, L, 1, 1, L)
    assert (b[cn.N_MEMBERS], b[cn.N_COMPONENTS], b[cn.LARGEST], b[cn.WRAP_AXES], b[cn.N_WRAPPING], b[cn.WRAPPING_SITES]) == (L - 1, 1, L - 1, 0, 0, 0)
    assert set(labels[0, 0][idx[:, 1, 2]]) == {idx[0, 1, 2]} and (labels[0, 0] >= 0).sum() == L
    # the same line along the other axes
    for axis, sel in ((1, idx[2, :, 0]), (2, idx[1, 2, :])):
        o = np.zeros((1, L * 9), dtype=np.int32)
        o[0, sel] = 1
        s, _ = check_against_union_find(spec, o)
        assert s[0, 0, cn.WRAP_AXES] == 1 << axis and s[0, 0, cn.LARGEST_WRAP_AXES] == 1 << axis


def test_self_image_and_two_image_bonds_wrap():
    one = Connectivity(np.zeros(1, np.int32), 1, [Graph([0], [(0, 0)], [(0, 1, 0)])])
    s, lab = check_against_union_find(one, np.zeros((1, 1), np.int32))
    assert s[0, 0, cn.WRAP_AXES] == 2 and s[0, 0, cn.N_WRAPPING] == 1 and s[0, 0, cn.LARGEST] == 1 and lab[0, 0, 0] == 0
    plain = Connectivity(np.zeros(1, np.int32), 1, [Graph([0], [(0, 0)], [(0, 0, 0)])])
    assert check_against_union_find(plain, np.zeros((1, 1), np.int32))[0][0, 0, cn.WRAP_AXES] == 0
    two = Connectivity(np.zeros(2, np.int32), 1, [Graph([0], [(0, 1), (0, 1)], [(0, 0, 0), (1, 0, 0)])])
    s, lab = check_against_union_find(two, np.zeros((1, 2), np.int32))
    assert s[0, 0, cn.WRAP_AXES] == 1 and s[0, 0, cn.LARGEST] == 2 and s[0, 0, cn.WRAPPING_SITES] == 2 and list(lab[0, 0]) == [0, 0]
    # one image alone does not wrap, whichever it is
    for w in ((0, 0, 0), (1, 0, 0), (-3, 2, 0)):
        open_ = Connectivity(np.zeros(2, np.int32), 1, [Graph([0], [(0, 1)], [w])])
        assert check_against_union_find(open_, np.zeros((1, 2), np.int32))[0][0, 0, cn.WRAP_AXES] == 0
    # a winding that is no unit vector: images (1, 0, 0) and (0, 0, -2) between the same sites close to (1, 0, 2)
    skew = Connectivity(np.zeros(2, np.int32), 1, [Graph([0], [(0, 1), (1, 0)], [(1, 0, 0), (0, 0, 2)])])
    assert check_against_union_find(skew, np.zeros((1, 2), np.int32))[0][0, 0, cn.WRAP_AXES] == 5


def test_duplicate_bonds_change_nothing_and_a_non_member_splits_a_line():
    bonds, images = grid_bonds((7, 1, 1))
    rng = np.random.default_rng(3)
    occ = (rng.random((6, 7)) < 0.7).astype(np.int32)
    occ[0] = [1, 1, 1, 0, 1, 1, 0]  # two pieces: sites 0-2 and 4-5 (6 is no member, so the ring is open)
    once = Connectivity(np.zeros(7, np.int32), 2, [Graph([1], bonds, images)])
    twice = Connectivity(np.zeros(7, np.int32), 2, [Graph([1], np.concatenate([bonds, bonds[::-1], bonds]),
                                                          np.concatenate([images, images[::-1], images]))])
    a, b = check_against_union_find(once, occ), check_against_union_find(twice, occ)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    row = a[0][0, 0]
    assert (row[cn.N_MEMBERS], row[cn.N_COMPONENTS], row[cn.LARGEST], row[cn.SUM_SQ], row[cn.WRAP_AXES]) == (5, 2, 3, 13, 0)
    assert list(a[1][0, 0]) == [0, 0, 0, -1, 4, 4, -1]


def test_histogram_bins_and_the_largest_among_equals():
    sizes = [1, 2, 3, 4, 255, 256]
    N = sum(sizes) + len(sizes)
    bonds, start, occ = [], 0, np.zeros((1, N), np.int32)
    for n in sizes:  # open chains, a non-member after each
        bonds += [(s, s + 1) for s in range(start, start + n - 1)]
        occ[0, start:start + n] = 1
        start += n + 1
    spec = Connectivity(np.zeros(N, np.int32), 2, [Graph([1], bonds)])
    s, lab = check_against_union_find(spec, occ)
    hist = s[0, 0, cn.HIST0:]
    assert list(hist[:9]) == [1, 2, 1, 0, 0, 0, 0, 1, 1] and hist.sum() == 6 and s[0, 0, cn.N_COMPONENTS] == 6
    assert s[0, 0, cn.LARGEST] == 256 and s[0, 0, cn.SUM_SQ] == sum(n * n for n in sizes)
    np.testing.assert_array_equal(cn.size_distribution(s)[0, 0], hist)
    # two components of equal size, only the one with the larger label wraps: the largest is the one with the smaller
    eq = Connectivity(np.zeros(4, np.int32), 1, [Graph([0], [(0, 1), (2, 3), (2, 3)], [(0, 0, 0), (0, 0, 0), (0, 0, 1)])])
    s, _ = check_against_union_find(eq, np.zeros((1, 4), np.int32))
    assert s[0, 0, cn.LARGEST] == 2 and s[0, 0, cn.LARGEST_WRAP_AXES] == 0 and s[0, 0, cn.WRAP_AXES] == 4
    eq = Connectivity(np.zeros(4, np.int32), 1, [Graph([0], [(0, 1), (2, 3), (0, 1)], [(0, 0, 0), (0, 0, 0), (0, 0, 1)])])
    assert check_against_union_find(eq, np.zeros((1, 4), np.int32))[0][0, 0, cn.LARGEST_WRAP_AXES] == 4


# ---- 2. from_supercell ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fcc_conv444_pairs", "fcc3_indicator_skew", "fcc_prim222_aliased"])
def test_bond_counts_are_the_coordination_numbers_and_both_directions_appear(name):
    sc = load_case(name)["sc"]
    near = Connectivity.from_supercell(sc, [dict(members=[0], cutoff=NN + 0.01)]).graphs[0]
    both = Connectivity.from_supercell(sc, [dict(members=[0], cutoff=NNN + 0.01)]).graphs[0]
    assert np.all(np.bincount(near.bonds[:, 0], minlength=sc.num_sites) == 12)
    assert np.all(np.bincount(both.bonds[:, 0], minlength=sc.num_sites) == 18)
    for g in (near, both):
        rows = {(int(i), int(j), *map(int, w)) for (i, j), w in zip(g.bonds, g.images)}
        assert len(rows) == len(g.bonds)  # (no row twice)
        assert all((j, i, -a, -b, -c) in rows for i, j, a, b, c in rows)
        assert not any(i == j and (a, b, c) == (0, 0, 0) for i, j, a, b, c in rows)
    # the next-nearest shell alone, named by its pair orbit
    orb = [o for o in sc.model.orbits if o.size == 2 and abs(o.diameter - NNN) < 1e-6]
    assert orb
    nnn = Connectivity.from_supercell(sc, [dict(members=[0], orbits=[o.id for o in orb])]).graphs[0]
    assert np.all(np.bincount(nnn.bonds[:, 0], minlength=sc.num_sites) == 6)
    if name == "fcc_prim222_aliased":
        # 2 x 2 x 2: the nearest neighbours reach a site by two images, and twice their distance away lie a site's own images
        assert len({(int(i), int(j)) for i, j in near.bonds}) < len(near.bonds)
        far = Connectivity.from_supercell(sc, [dict(members=[0], cutoff=6.0)]).graphs[0]
        own = far.bonds[:, 0] == far.bonds[:, 1]
        assert own.sum() == 12 * sc.num_sites and np.all(np.abs(far.images[own]).sum(axis=1) > 0)
    # the lengths, from the positions themselves
    from smol_amd.structure import lattice_points_of

    prim = sc.model.prim
    pos = (lattice_points_of(sc)[sc.site_t] + prim.frac_coords[sc.site_b]) @ prim.lattice
    S = np.asarray(sc.scmatrix, dtype=float) @ prim.lattice
    d = np.linalg.norm(pos[near.bonds[:, 1]] + near.images.astype(float) @ S - pos[near.bonds[:, 0]], axis=1)
    np.testing.assert_allclose(d, NN, atol=1e-9)


@pytest.mark.parametrize("name,cutoff", [("fcc3_indicator_skew", NN + 0.01), ("fcc_prim222_aliased", 6.0),
                                         ("fcc_prim222_aliased", NN + 0.01), ("rocksalt333_two_sublattices", 3.0)])
def test_random_occupancies_agree_with_the_union_find(name, cutoff):
    sc = load_case(name)["sc"]
    K = cn.Observables.default_kind_base(sc)[1]
    spec = Connectivity.from_supercell(sc, [dict(members=[0], cutoff=cutoff), dict(members=list(range(1, K)), cutoff=cutoff)])
    rng = np.random.default_rng(8)
    occ = np.concatenate([_rand_occ(sc, rng, 3, p) for p in (0.15, 0.3, 0.6)])
    stats, _ = check_against_union_find(spec, occ)
    assert np.any(stats[..., cn.WRAP_AXES] != 0)
    if name != "fcc_prim222_aliased":  # (eight sites with twelve neighbours each hang together)
        assert stats[..., cn.N_COMPONENTS].max() > 1 and np.any(stats[..., cn.WRAP_AXES] == 0)


def test_species_names_site_classes_and_refusals_of_from_supercell():
    sc = load_case("rocksalt333_two_sublattices")["sc"]
    by_name = Connectivity.from_supercell(sc, [dict(members=["Li+"], cutoff=3.0), dict(members=["F-", "O2-"], cutoff=3.0)])
    kb, K, _ = cn.Observables.default_kind_base(sc)
    assert by_name.graphs[0].members == [0] and by_name.graphs[1].members == [K - 2, K - 1] and by_name.n_kinds == K
    split = Connectivity.from_supercell(sc, [dict(members=[0], cutoff=3.0)], site_classes=np.arange(sc.num_sites) % 2)
    assert split.n_kinds == 2 * K
    with pytest.raises(ValueError, match="no counted site holds a species named 'Xe'"):
        Connectivity.from_supercell(sc, [dict(members=["Xe"], cutoff=3.0)])
    with pytest.raises(ValueError, match="give cutoff= or orbits=, one of them"):
        Connectivity.from_supercell(sc, [dict(members=[0])])
    small = load_case("fcc_prim222_aliased")["sc"]
    with pytest.raises(ValueError, match=r"beyond MAX_IMAGE = 7: image out of range"):
        Connectivity.from_supercell(small, [dict(members=[0], cutoff=48.0)])


def test_validation_names_its_reason():
    kb = np.zeros(4, np.int32)
    with pytest.raises(ValueError, match="n_graphs must be 1..8, got 0"):
        Connectivity(kb, 2, [])
    with pytest.raises(ValueError, match="n_graphs must be 1..8, got 9"):
        Connectivity(kb, 2, [Graph([0], [(0, 1)])] * 9)
    with pytest.raises(ValueError, match="graph 1: bond out of range"):
        Connectivity(kb, 2, [Graph([0], [(0, 1)]), Graph([0], [(0, 4)])])
    with pytest.raises(ValueError, match="graph 0: member kind 2, n_kinds is 2: kind out of range"):
        Connectivity(kb, 2, [Graph([0, 2], [(0, 1)])])
    with pytest.raises(ValueError, match="beyond MAX_IMAGE = 7: image out of range"):
        Graph([0], [(0, 1)], [(0, 8, 0)])
    with pytest.raises(ValueError, match="a path sum could overflow"):
        Connectivity(np.zeros(4682, np.int32), 2, [Graph([0], [(0, 1)])])
    Connectivity(np.zeros(4681, np.int32), 2, [Graph([0], [(0, 1)])])
    assert 4681 * cn.MAX_IMAGE <= cn.MAX_PATH_SUM < 4682 * cn.MAX_IMAGE
    with pytest.raises(ValueError, match="kind_base\\[1\\] \\+ site_ncodes\\[1\\] = 1 \\+ 2 is larger than n_kinds = 2"):
        Connectivity(np.array([0, 1, 0, 0]), 2, [Graph([0], [(0, 1)])], site_ncodes=np.full(4, 2))
    spec = Connectivity(kb, 2, [Graph([0], [(0, 1)])])
    with pytest.raises(ValueError, match="an occupancy code gives a kind out of range"):
        spec.evaluate(np.array([[0, 2, 0, 0]]))


# ---- 3. derived quantities -----------------------------------------------------------------------------------------------------
def test_derived_quantities():
    stats = np.zeros((4, 2, 24), dtype=np.int64)
    stats[:, 0, cn.N_MEMBERS] = [10, 10, 10, 0]
    stats[:, 0, cn.WRAPPING_SITES] = [5, 0, 10, 0]
    stats[:, 0, cn.WRAP_AXES] = [1, 0, 7, 0]
    stats[:, 0, cn.LARGEST] = [5, 4, 10, 0]
    stats[:, 0, cn.SUM_SQ] = [25 + 9 + 4, 16 + 36, 100, 0]
    p = cn.percolation_strength(stats)
    assert p.shape == (4, 2) and list(p[:3, 0]) == [0.5, 0.0, 1.0] and np.isnan(p[3, 0])
    m = cn.mean_finite_size(stats)
    assert m[0, 0] == 13 / 5 and m[1, 0] == 36 / 6 and np.isnan(m[2, 0])
    np.testing.assert_array_equal(cn.wrapping_probability(stats), [0.5, 0.0])
    np.testing.assert_array_equal(cn.wrapping_probability(stats, axes=[0]), [0.5, 0.0])
    np.testing.assert_array_equal(cn.wrapping_probability(stats, axes=[0, 2]), [0.25, 0.0])
    np.testing.assert_array_equal(cn.wrapping_probability(stats, axes=6), [0.25, 0.0])


# ---- 4. the header and the ctypes mirror ------------------------------------------------------------------------------------------
def test_ctypes_mirror_matches_the_header_and_the_abi_stays_8():
    import subprocess
    import tempfile

    fields = [n for n, _ in capi.smolmc_connectivity._fields_]
    names = ["N_MEMBERS", "N_COMPONENTS", "LARGEST", "SUM_SQ", "N_WRAPPING", "WRAPPING_SITES", "WRAP_AXES", "LARGEST_WRAP_AXES"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "smolmc.h"\nint main(){printf("%zu", sizeof(smolmc_connectivity));\n' +
           "".join(f'printf(" %zu", offsetof(smolmc_connectivity, {f}));\n' for f in fields) +
           'printf(" %d %d %d %d %d %d", SMOLMC_SAMPLE_CONNECTIVITY, SMOLMC_MAX_CONN_GRAPHS, SMOLMC_MAX_CONN_IMAGE, '
           "SMOLMC_MAX_CONN_PATH_SUM, SMOLMC_CONN_STATS, SMOLMC_ABI_VERSION);\n" +
           "".join(f'printf(" %d", SMOLMC_CONN_{n});\n' for n in names) + 'printf(" %d\\n", SMOLMC_CONN_HIST);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "p"), os.path.join(d, "p.c")])
        vals = [int(x) for x in subprocess.check_output([os.path.join(d, "p")]).split()]
    T = capi.smolmc_connectivity
    assert vals == [ctypes.sizeof(T)] + [getattr(T, f).offset for f in fields] + [
        capi.SAMPLE_CONNECTIVITY, capi.MAX_CONN_GRAPHS, capi.MAX_CONN_IMAGE, capi.MAX_CONN_PATH_SUM, capi.CONN_STATS, 8] + [
        getattr(cn, n) for n in names] + [cn.HIST0]
    assert capi.SAMPLE_CONNECTIVITY == 128 and capi.ABI_VERSION == 8
    assert (cn.MAX_GRAPHS, cn.MAX_IMAGE, cn.MAX_PATH_SUM, cn.N_STATS) == (capi.MAX_CONN_GRAPHS, capi.MAX_CONN_IMAGE, capi.MAX_CONN_PATH_SUM,
                                                                        capi.CONN_STATS)
    assert cn.HIST0 + cn.N_HIST == cn.N_STATS
    hdr = open(os.path.join(ROOT, "include", "smolmc.h")).read()
    assert re.search(r"#define SMOLMC_ABI_VERSION 8\b", hdr)
    # the LDS plan takes the workload's rows and the longest rows the path sums allow
    assert capi.connectivity_lds_bytes(4096, 4096) is not None and capi.connectivity_lds_bytes(4681, 4688) is not None
    assert capi.connectivity_lds_bytes(5500, 5504) is None
    # c_struct points at the object's own arrays
    spec = Connectivity(np.zeros(4, np.int32), 70, [Graph([1], [(0, 1)], [(0, 0, 1)]), Graph([0, 69], [(2, 3), (3, 0)], [(0, -7, 0), (1, 0, 0)])])
    s, keep = spec.c_struct()
    assert (s.n_kinds, s.n_graphs) == (70, 2) and [s.bond_ptr[i] for i in range(3)] == [0, 1, 3]
    assert [s.member_mask[i] for i in range(8)] == [2, 0, 0, 0, 1, 32, 0, 0]
    assert [s.bonds[i] for i in range(6)] == [0, 1, 2, 3, 3, 0] and [s.images[i] for i in range(9)] == [0, 0, 1, 0, -7, 0, 1, 0, 0]
    assert len(keep) == 5


# ---- 5. statistics with connectivity columns ------------------------------------------------------------------------------------
def test_statistics_columns_fed_by_connectivity():
    rng = np.random.default_rng(11)
    ns, R, F, K, I, G = 5, 4, 3, 2, 3, 2
    H, f = rng.normal(size=(ns, R)), rng.normal(size=(ns, R, F))
    cnt, inten = rng.integers(0, 9, size=(ns, R, K)), rng.random((ns, R, I))
    conn = rng.integers(0, 50, size=(ns, R, G, 24))
    spec = st.Statistics.per_walker(columns=(st.ENTHALPY, st.connectivity(0, cn.LARGEST), st.connectivity(1, cn.WRAP_AXES), st.intensity(2)),
                                    n_levels=2, hist=(st.connectivity(0, cn.LARGEST), 10, 0.0, 5.0))
    np.testing.assert_array_equal(spec.sources(F, K, I, G), [0, 2 + F + K + I + 2, 2 + F + K + I + 24 + 6, 4 + F + K])
    assert spec.connectivity_columns() == [1, 2] and spec.intensity_columns() == [3]
    x = spec.column_values(H, f, cnt, inten, conn)
    np.testing.assert_array_equal(x[..., 1], conn[..., 0, cn.LARGEST].astype(float))
    np.testing.assert_array_equal(x[..., 2], conn[..., 1, cn.WRAP_AXES].astype(float))
    np.testing.assert_array_equal(x[..., 3], inten[..., 2])
    s, keep = spec.c_struct(F, K, I, G)
    assert [s.columns[i] for i in range(4)] == [0, 12, 40, 9]
    with pytest.raises(ValueError, match="graph 1 outside the 1 graphs"):
        spec.sources(F, K, I, 1)
    with pytest.raises(ValueError, match="graph 0 outside the 0 graphs"):
        spec.sources(F, K, I)
    with pytest.raises(ValueError, match="connectivity column 24 outside 0..23"):
        st.connectivity(0, 24)
    rec = st.StatisticsRecord(spec, R)
    rec.offer(H, f, cnt, intensities=inten, connectivity=conn)
    plain = st.Statistics.per_walker(columns=(0, 1, 2, 3), n_levels=2, hist=(1, 10, 0.0, 5.0))
    ref = st.StatisticsRecord(plain, R)
    ref.offer(x[..., 0], x[..., 1:])
    for name in ("n", "shift", "s1", "s2", "has", "pend", "b2", "nb", "hist", "under", "over"):
        np.testing.assert_array_equal(getattr(rec, name), getattr(ref, name), err_msg=name)
    # calls without the fourth argument mean what they meant
    old = st.Statistics.per_walker(columns=(st.ENTHALPY, st.intensity(1), st.ENERGY), weights=np.array([1.0]))
    np.testing.assert_array_equal(old.sources(F, K, I), old.sources(F, K, I, 3))
    np.testing.assert_array_equal(old.column_values(H, f, cnt, inten), old.column_values(H, f, cnt, inten, conn))
