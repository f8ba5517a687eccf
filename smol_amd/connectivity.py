"""Connectivity of sampled states: connected components of the sites of chosen kinds, and whether they span the cell.

This module is the DEFINITION: ``Connectivity.evaluate`` in NumPy is what the device kernel (csrc/connectivity.hip,
``smolmc_eval_connectivity`` and the ``SMOLMC_SAMPLE_CONNECTIVITY`` column of the sample ring) matches entry for entry.
Everything is integer, so host and device agree bit for bit.

The *kind* of (site, code) is ``kind_base[site] + code`` as in ``observables.Observables``; ``kind_base[site] = -1`` leaves
the site out.  A spec holds 1..8 *graphs*.  A graph has a set of member kinds -- a site is a *member* in an occupancy when
its kind is in the set -- and bonds ``(i, j, w)``: site i of the home cell is joined to site j of the periodic image
displaced by ``w[0] S_0 + w[1] S_1 + w[2] S_2``, ``S_a`` the supercell vectors.  A bond is *active* when both ends are
members.  Duplicate rows, rows ``i == j`` with ``w != 0`` (a site bonded to its own image, in aliased cells) and two rows
joining the same sites by different images mean what they say.

A bond row may carry 0..4 *gate sites* (``Graph(gates=...)``, caller's site numbers; an occupancy is periodic, so a gate
site has no image).  A gate site is *blocked* when its kind is not in the graph's ``gate_kinds``; a site listed twice in a
row counts twice.  A row is *open* when both ends are members and at most ``max_blocked`` of its gate sites are blocked; a
row without gate sites is open whenever both ends are members.  The adjacency ``(i, j, w)`` with its reverse
``(j, i, -w)`` is active when at least one row that lists it, in either direction, is open: the two tetrahedra of an fcc
nearest-neighbour bond are two rows of the same bond with different gates (the 0-TM channels of a disordered rocksalt,
``max_blocked = 0``).  A graph none of whose rows has a gate site is *ungated*.

*Components* are the connected components of the members under the active bonds.  The *winding set* of a component is
the set of image sums over its closed paths, a subgroup of Z^3; the component *wraps axis a* when an element of the set
has a nonzero entry a.  However it is computed: give every site the image sum ``off`` along some path from one site of the
component, form ``m = off[i] + w - off[j]`` for each active bond; axis a wraps iff some ``m[a] != 0``.

    stats   (n, G, 24) int64   the columns below
    labels  (n, G, N)  int32   the smallest site number of the site's component, -1 for a non-member
"""

from __future__ import annotations

import itertools
from collections import deque

import numpy as np

from .observables import MAX_KINDS, Observables

MAX_GRAPHS = 8        # SMOLMC_MAX_CONN_GRAPHS
MAX_IMAGE = 7         # SMOLMC_MAX_CONN_IMAGE: |w_a| of a bond
MAX_GATES = 4         # SMOLMC_MAX_CONN_GATES: gate sites of a bond row
MAX_PATH_SUM = 32767  # the device keeps a path sum per axis in 16 bits: N x MAX_IMAGE must stay at or below this
N_STATS = 24          # SMOLMC_CONN_STATS
SITE_TOL = 1e-6       # two distances (in units of the lattice's length) are the same within this

# columns of stats
N_MEMBERS, N_COMPONENTS, LARGEST, SUM_SQ, N_WRAPPING, WRAPPING_SITES, WRAP_AXES, LARGEST_WRAP_AXES, HIST0 = range(9)
N_HIST = 16           # HIST0 + b: components with floor(log2 size) == b


class Graph:
    """One graph: ``members`` kinds, ``bonds`` (nb, 2) site pairs and ``images`` (nb, 3) of each bond; optionally
    ``gates`` (nb, m <= 4) gate sites of each bond row (-1: none; or a list of lists), the ``gate_kinds`` that do not block
    and ``max_blocked``, the blocked gate sites an open row may have."""

    def __init__(self, members, bonds, images=None, gates=None, gate_kinds=(), max_blocked=0):
        self.members = sorted({int(k) for k in members})
        b = np.asarray(bonds)
        if b.size == 0:
            b = np.zeros((0, 2), dtype=np.int32)
        if b.ndim != 2 or b.shape[1] != 2 or not np.issubdtype(b.dtype, np.integer):
            raise ValueError("bonds must be an (nbonds, 2) integer array")
        w = np.zeros((len(b), 3), dtype=np.int64) if images is None else np.asarray(images)
        if w.size == 0:
            w = np.zeros((0, 3), dtype=np.int64)
        if w.shape != (len(b), 3) or not np.issubdtype(w.dtype, np.integer):
            raise ValueError("images must be an (nbonds, 3) integer array, one row per bond")
        if np.abs(w).max(initial=0) > MAX_IMAGE:
            raise ValueError(f"a bond's image reaches {int(np.abs(w).max())}, beyond MAX_IMAGE = {MAX_IMAGE}: image out of range")
        self.bonds = np.ascontiguousarray(b, dtype=np.int32)
        self.images = np.ascontiguousarray(w, dtype=np.int8)
        self.gates = np.full((len(b), 0), -1, dtype=np.int32) if gates is None else _gate_array(gates, len(b))
        self.gate_kinds = sorted({int(k) for k in gate_kinds})
        self.max_blocked = int(max_blocked)
        if not 0 <= self.max_blocked <= MAX_GATES:
            raise ValueError(f"max_blocked must be 0..{MAX_GATES}, got {self.max_blocked}: max_blocked out of range")

    @property
    def gated(self):
        """A row of the graph has a gate site."""
        return bool((self.gates >= 0).any())

    def gate_lists(self):
        """(gate_ptr (nb + 1,) int64, gate_sites int32): the gate sites of row b are gate_sites[gate_ptr[b]:gate_ptr[b + 1]]."""
        has = self.gates >= 0
        ptr = np.concatenate(([0], np.cumsum(has.sum(axis=1)))).astype(np.int64)
        return ptr, np.ascontiguousarray(self.gates[has], dtype=np.int32)


def _gate_array(gates, nb):
    """(nb, m) int32, -1 for no gate, of an integer array or a list of lists (rows of different lengths)."""
    if not isinstance(gates, np.ndarray):
        rows = [list(r) for r in gates]
        m = max((len(r) for r in rows), default=0)
        if m > MAX_GATES:
            raise ValueError(f"a bond row has {m} gate sites, SMOLMC_MAX_CONN_GATES = {MAX_GATES}: too many gates on a row")
        gates = np.array([r + [-1] * (m - len(r)) for r in rows], dtype=np.int64).reshape(len(rows), m)
    g = np.asarray(gates)
    if g.ndim != 2 or len(g) != nb or (g.size and not np.issubdtype(g.dtype, np.integer)):
        raise ValueError("gates must be an (nbonds, m) integer array or a list of one list per bond row")
    if g.shape[1] > MAX_GATES:
        raise ValueError(f"a bond row has {g.shape[1]} gate sites, SMOLMC_MAX_CONN_GATES = {MAX_GATES}: too many gates on a row")
    return np.ascontiguousarray(np.where(g < 0, -1, g), dtype=np.int32)


class Connectivity:
    """Kinds and graphs of one supercell.

    kind_base    (N,) integers, -1 = the site is in no graph
    n_kinds      K
    graphs       1..8 ``Graph`` objects, or dicts / tuples of their arguments (members, bonds, images[, gates, gate_kinds,
                 max_blocked])
    site_ncodes  optional (N,): species codes each site can hold; with it every kind is checked to stay below K
    """

    def __init__(self, kind_base, n_kinds, graphs, site_ncodes=None):
        kb = np.asarray(kind_base)
        if kb.ndim != 1 or not np.issubdtype(kb.dtype, np.integer):
            raise ValueError("kind_base must be a 1-D integer array, one entry per site")
        self.kind_base = np.ascontiguousarray(np.where(kb < 0, -1, kb), dtype=np.int32)
        self.num_sites = N = len(self.kind_base)
        self.n_kinds = K = int(n_kinds)
        if not 1 <= K <= MAX_KINDS:
            raise ValueError(f"n_kinds must be 1..{MAX_KINDS}, got {K}")
        if self.kind_base.max(initial=-1) >= K:
            raise ValueError(f"kind_base holds {int(self.kind_base.max())}, n_kinds is {K}: kind out of range")
        if N * MAX_IMAGE > MAX_PATH_SUM:
            raise ValueError(f"{N} sites x MAX_IMAGE = {MAX_IMAGE} is larger than {MAX_PATH_SUM}: a path sum could overflow")
        self.graphs = []
        for g in graphs:
            if isinstance(g, dict):
                g = Graph(g["members"], g["bonds"], g.get("images"), g.get("gates"), g.get("gate_kinds", ()), g.get("max_blocked", 0))
            elif not isinstance(g, Graph):
                g = Graph(*g)
            self.graphs.append(g)
        self.n_graphs = G = len(self.graphs)
        if not 1 <= G <= MAX_GRAPHS:
            raise ValueError(f"n_graphs must be 1..{MAX_GRAPHS}, got {G}")
        for gi, g in enumerate(self.graphs):
            if g.members and not 0 <= min(g.members) <= max(g.members) < K:
                raise ValueError(f"graph {gi}: member kind {max(g.members) if max(g.members) >= K else min(g.members)}, "
                                 f"n_kinds is {K}: kind out of range")
            if g.bonds.min(initial=0) < 0 or g.bonds.max(initial=0) >= N:
                raise ValueError(f"graph {gi}: bond out of range ({N} sites)")
            if g.gates.max(initial=-1) >= N:
                raise ValueError(f"graph {gi}: gate site {int(g.gates.max())}, {N} sites: gate site out of range")
            used = g.gates[g.gates >= 0]
            if used.size and self.kind_base[used].min() < 0:
                s = int(used[np.argmin(self.kind_base[used])])
                raise ValueError(f"graph {gi}: gate site {s} has kind_base -1: a gate site must be a counted site")
            if g.gate_kinds and not 0 <= min(g.gate_kinds) <= max(g.gate_kinds) < K:
                raise ValueError(f"graph {gi}: gate kind {max(g.gate_kinds) if max(g.gate_kinds) >= K else min(g.gate_kinds)}, "
                                 f"n_kinds is {K}: kind out of range")
        self.site_ncodes = None
        if site_ncodes is not None:
            nc = np.asarray(site_ncodes, dtype=np.int64)
            if nc.shape != (N,) or nc.min(initial=1) < 1:
                raise ValueError("site_ncodes must hold one positive entry per site")
            counted = self.kind_base >= 0
            top = self.kind_base[counted] + nc[counted]
            if top.max(initial=0) > K:
                s = int(np.flatnonzero(counted)[np.argmax(top)])
                raise ValueError(f"kind_base[{s}] + site_ncodes[{s}] = {int(self.kind_base[s])} + {int(nc[s])} is larger than "
                                 f"n_kinds = {K}: kind out of range")
            self.site_ncodes = nc.astype(np.int32)
        self._adjacency = None

    # ---- constructors -------------------------------------------------------------------------------------------
    @classmethod
    def from_supercell(cls, sc, graphs, site_classes=None, observables=None):
        """Graphs built from the geometry of a ``synth`` or ``mson`` supercell.

        Each graph is ``dict(members=[kinds or species names], cutoff=r)`` -- every pair of sites at most ``r`` apart is
        bonded -- or ``dict(members=..., orbits=[pair orbit ids])`` -- the pairs at the distances of those orbits.  The
        bonds come from the lattice, the fractional coordinates and ``scmatrix``, not from ``full_indices``: every
        ``(i, j, w)`` with ``|r_j + w.S - r_i|`` equal to a wanted distance within ``SITE_TOL``, except ``i == j`` with
        ``w == 0``.  Each undirected bond so appears in both directions; small and aliased cells get their self-image and
        multi-image bonds.  Kinds: the default kinds of ``Observables.default_kind_base(sc)``, split by ``site_classes`` as
        ``Observables.from_supercell`` does, or those of ``observables``.  A species name stands for its kind on every
        sublattice that holds the species."""
        if observables is not None:
            if site_classes is not None:
                raise ValueError("give site_classes or observables, not both")
            kind_base, K, ncodes = observables.kind_base, observables.n_kinds, observables.site_ncodes
        elif site_classes is not None:
            o = Observables.from_supercell(sc, orbits=(), site_classes=site_classes)
            kind_base, K, ncodes = o.kind_base, o.n_kinds, o.site_ncodes
        else:
            kind_base, K, ncodes = Observables.default_kind_base(sc)
        prim = sc.model.prim
        species = getattr(prim, "species", None)
        site_b = np.asarray(sc.site_b, dtype=np.int64)
        made = []

        def kinds_named(gi, listed):
            kinds = set()
            for m in listed:
                if isinstance(m, str):
                    hits = set()
                    for s in range(sc.num_sites):
                        names = species[int(site_b[s])] if species is not None else None
                        if names is not None and m in names and kind_base[s] >= 0:
                            hits.add(int(kind_base[s]) + list(names).index(m))
                    if not hits:
                        raise ValueError(f"graph {gi}: no counted site holds a species named {m!r}")
                    kinds |= hits
                else:
                    kinds.add(int(m))
            return kinds

        for gi, g in enumerate(graphs):
            members = kinds_named(gi, g["members"])
            if ("cutoff" in g) == ("orbits" in g):
                raise ValueError(f"graph {gi}: give cutoff= or orbits=, one of them")
            if "cutoff" in g:
                bonds, images = geometric_bonds(sc, cutoff=float(g["cutoff"]))
            else:
                want = []
                for orb in sc.model.orbits:
                    if orb.id in g["orbits"]:
                        if getattr(orb, "size", None) != 2 and getattr(orb, "num_sites", 2) != 2:
                            raise ValueError(f"graph {gi}: orbit {orb.id} is no pair orbit")
                        want.append(float(orb.diameter))
                if len(want) != len(set(g["orbits"])):
                    raise ValueError(f"graph {gi}: orbits {sorted(g['orbits'])} are not all orbits of the model")
                bonds, images = geometric_bonds(sc, distances=want)
            gate = g.get("gate")
            if gate is None:
                made.append(Graph(members, bonds, images))
                continue
            unknown = set(gate) - {"kinds", "corners", "max_blocked"}
            if unknown or "kinds" not in gate:
                raise ValueError(f"graph {gi}: gate=dict(kinds=..., corners=1|2, max_blocked=0), got the keys {sorted(gate)}")
            bonds, images, gates = channel_rows(bonds, images, corners=int(gate.get("corners", 2)))
            made.append(Graph(members, bonds, images, gates, kinds_named(gi, gate["kinds"]), int(gate.get("max_blocked", 0))))
        return cls(kind_base, K, made, site_ncodes=ncodes)

    # ---- the definition ------------------------------------------------------------------------------------------
    def kinds_of(self, occupancies):
        """(..., N) int64 kinds of occupancies (..., N); -1 where the site is not counted."""
        occ = np.asarray(occupancies)
        if occ.shape[-1:] != (self.num_sites,) or not np.issubdtype(occ.dtype, np.integer):
            raise ValueError(f"occupancies must be integer arrays with {self.num_sites} sites in the last axis")
        kinds = np.where(self.kind_base >= 0, self.kind_base.astype(np.int64) + occ, -1)
        if occ.min(initial=0) < 0 or kinds.max(initial=-1) >= self.n_kinds:
            raise ValueError("an occupancy code gives a kind out of range")
        return kinds

    def _neighbours(self):
        """Per graph, per site: the list of (neighbour, image as seen from the site, adjacency) over the bonds, both ways;
        and per graph the adjacency of every bond row.  An *adjacency* is a number shared by the rows that list
        ``(i, j, w)`` or its reverse ``(j, i, -w)``: what the gates of a gated graph open or close together."""
        if self._adjacency is None:
            self._adjacency, self._row_adjacency = [], []
            for g in self.graphs:
                adj = [[] for _ in range(self.num_sites)]
                ids, of_row = {}, []
                for (i, j), w in zip(g.bonds.tolist(), g.images.tolist()):
                    fwd, back = (i, j, w[0], w[1], w[2]), (j, i, -w[0], -w[1], -w[2])
                    a = ids.setdefault(min(fwd, back), len(ids))
                    of_row.append(a)
                    adj[i].append((j, w[0], w[1], w[2], a))
                    adj[j].append((i, -w[0], -w[1], -w[2], a))
                self._adjacency.append(adj)
                self._row_adjacency.append((np.asarray(of_row, dtype=np.int64), len(ids)))
        return self._adjacency

    def open_rows(self, occupancies, g):
        """(..., nb_g) bool: the bond rows of graph ``g`` that are open in occupancies (..., N) -- both ends members and at
        most ``max_blocked`` of the row's gate sites blocked, a site listed twice counted twice."""
        kinds = self.kinds_of(occupancies)
        gr = self.graphs[g]
        is_member = np.zeros(self.n_kinds + 1, dtype=bool)  # (kind -1 reads the spare entry: no member, and it blocks)
        is_member[gr.members] = True
        member = is_member[kinds]
        is_open = member[..., gr.bonds[:, 0]] & member[..., gr.bonds[:, 1]]
        if gr.gates.shape[1]:
            passes = np.zeros(self.n_kinds + 1, dtype=bool)
            passes[gr.gate_kinds] = True
            has = gr.gates >= 0
            blocked = (has & ~passes[kinds[..., np.where(has, gr.gates, 0)]]).sum(axis=-1)
            is_open &= blocked <= gr.max_blocked
        return is_open

    def evaluate(self, occupancies):
        """(stats (..., G, 24) int64, labels (..., G, N) int32) of occupancies (..., N): a breadth-first search from
        every member not yet reached, in the order of the site numbers -- so the start is the component's label."""
        kinds = self.kinds_of(occupancies)
        occupancies = np.asarray(occupancies)
        lead = kinds.shape[:-1]
        kinds = kinds.reshape(-1, self.num_sites)
        n, G, N = len(kinds), self.n_graphs, self.num_sites
        stats = np.zeros((n, G, N_STATS), dtype=np.int64)
        labels = np.full((n, G, N), -1, dtype=np.int32)
        for gi, (g, adj) in enumerate(zip(self.graphs, self._neighbours())):
            is_member = np.zeros(self.n_kinds + 1, dtype=bool)
            is_member[g.members] = True
            of_row, n_adjacencies = self._row_adjacency[gi]
            for r in range(n):
                member = is_member[kinds[r]].tolist()  # (kind -1 reads the spare entry: no member)
                active = None
                if g.gated:  # an adjacency is active when one of its rows is open (both ends members then)
                    hit = np.zeros(n_adjacencies, dtype=bool)
                    hit[of_row[self.open_rows(occupancies.reshape(-1, N)[r], gi)]] = True
                    active = hit.tolist()
                label, st = labels[r, gi], stats[r, gi]
                off = [None] * N
                best = (0, 0)  # (size, -label) of the largest component so far
                for start in range(N):
                    if not member[start] or off[start] is not None:
                        continue
                    off[start] = (0, 0, 0)
                    queue, size, axes = deque([start]), 0, 0
                    while queue:
                        i = queue.popleft()
                        label[i] = start
                        size += 1
                        oi = off[i]
                        for j, wx, wy, wz, a in adj[i]:
                            if not member[j] if active is None else not active[a]:
                                continue
                            reach = (oi[0] + wx, oi[1] + wy, oi[2] + wz)
                            if off[j] is None:
                                off[j] = reach
                                queue.append(j)
                            elif off[j] != reach:
                                axes |= (reach[0] != off[j][0]) | (reach[1] != off[j][1]) << 1 | (reach[2] != off[j][2]) << 2
                    st[N_MEMBERS] += size
                    st[N_COMPONENTS] += 1
                    st[SUM_SQ] += size * size
                    st[HIST0 + size.bit_length() - 1] += 1
                    if axes:
                        st[N_WRAPPING] += 1
                        st[WRAPPING_SITES] += size
                        st[WRAP_AXES] |= axes
                    if size > best[0]:  # (among equals the first, which has the smallest label)
                        best = (size, -start)
                        st[LARGEST] = size
                        st[LARGEST_WRAP_AXES] = axes
        return stats.reshape(lead + (G, N_STATS)), labels.reshape(lead + (G, N))

    # ---- the C struct ------------------------------------------------------------------------------------------
    def member_masks(self):
        """(G, 4) uint64: bit k of the 256-bit row g says kind k is a member of graph g."""
        mask = np.zeros((self.n_graphs, 4), dtype=np.uint64)
        for gi, g in enumerate(self.graphs):
            for k in g.members:
                mask[gi, k >> 6] |= np.uint64(1) << np.uint64(k & 63)
        return mask

    def c_struct(self):
        """(capi.smolmc_connectivity, the arrays it points at -- keep them alive during the call)."""
        import ctypes as C

        from . import capi

        mask = self.member_masks()
        ptr = np.concatenate(([0], np.cumsum([len(g.bonds) for g in self.graphs]))).astype(np.int64)
        bonds = np.ascontiguousarray(np.concatenate([g.bonds for g in self.graphs]), dtype=np.int32)
        images = np.ascontiguousarray(np.concatenate([g.images for g in self.graphs]), dtype=np.int8)
        s = capi.smolmc_connectivity()
        s.n_kinds, s.n_graphs = self.n_kinds, self.n_graphs
        s.kind_base = self.kind_base.ctypes.data_as(C.POINTER(C.c_int32))
        s.member_mask = mask.ctypes.data_as(C.POINTER(C.c_uint64))
        s.bond_ptr = ptr.ctypes.data_as(C.POINTER(C.c_int64))
        s.bonds = bonds.ctypes.data_as(C.POINTER(C.c_int32))
        s.images = images.ctypes.data_as(C.POINTER(C.c_int8))
        return s, (self.kind_base, mask, ptr, bonds, images)

    @property
    def gated(self):
        """A graph of the spec has a gate site."""
        return any(g.gated for g in self.graphs)

    def gate_masks(self):
        """(G, 4) uint64: bit k of the 256-bit row g says a gate site of kind k does not block in graph g."""
        mask = np.zeros((self.n_graphs, 4), dtype=np.uint64)
        for gi, g in enumerate(self.graphs):
            for k in g.gate_kinds:
                mask[gi, k >> 6] |= np.uint64(1) << np.uint64(k & 63)
        return mask

    def c_gates(self):
        """(capi.smolmc_conn_gates, the arrays it points at) of a gated spec -- what ``smolmc_set_connectivity_gated`` takes
        next to ``c_struct()`` -- or None for a spec without gates."""
        if not self.gated:
            return None
        import ctypes as C

        from . import capi

        mask = self.gate_masks()
        most = np.asarray([g.max_blocked for g in self.graphs], dtype=np.int32)
        lists = [g.gate_lists() for g in self.graphs]
        counts = np.concatenate([np.diff(p) for p, _ in lists]) if lists else np.zeros(0, np.int64)
        ptr = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
        sites = np.ascontiguousarray(np.concatenate([s for _, s in lists]), dtype=np.int32)
        g = capi.smolmc_conn_gates()
        g.gate_mask = mask.ctypes.data_as(C.POINTER(C.c_uint64))
        g.max_blocked = most.ctypes.data_as(C.POINTER(C.c_int32))
        g.gate_ptr = ptr.ctypes.data_as(C.POINTER(C.c_int64))
        g.gate_sites = sites.ctypes.data_as(C.POINTER(C.c_int32))
        return g, (mask, most, ptr, sites)

    def to_metadata(self):
        """What a container's metadata keeps of the spec (``moca.Sampler``): its shape and the member kinds; of a gated spec
        also the gate kinds, ``max_blocked`` and the number of gated rows of every graph."""
        meta = dict(n_graphs=self.n_graphs, n_kinds=self.n_kinds, members=[list(g.members) for g in self.graphs],
                    n_bonds=[int(len(g.bonds)) for g in self.graphs])
        if self.gated:
            meta.update(gate_kinds=[list(g.gate_kinds) for g in self.graphs], max_blocked=[int(g.max_blocked) for g in self.graphs],
                        n_gated_rows=[int((g.gates >= 0).any(axis=1).sum()) for g in self.graphs])
        return meta

    @staticmethod
    def metadata_to_npz(conn):
        """The meta/* arrays of an .npz for the dict of ``to_metadata``: the ragged lists as values and offsets."""
        members = conn["members"]
        out = {"meta/conn_shape": np.asarray([conn["n_graphs"], conn["n_kinds"]], dtype=np.int64),
               "meta/conn_n_bonds": np.asarray(conn["n_bonds"], dtype=np.int64),
               "meta/conn_member_ptr": np.cumsum([0] + [len(m) for m in members]).astype(np.int64),
               "meta/conn_members": np.asarray([k for m in members for k in m], dtype=np.int32)}
        if "gate_kinds" in conn:  # a gated spec: the kinds that do not block, max_blocked and the gated rows per graph
            kinds = conn["gate_kinds"]
            out.update({"meta/conn_gate_kind_ptr": np.cumsum([0] + [len(m) for m in kinds]).astype(np.int64),
                        "meta/conn_gate_kinds": np.asarray([k for m in kinds for k in m], dtype=np.int32),
                        "meta/conn_max_blocked": np.asarray(conn["max_blocked"], dtype=np.int64),
                        "meta/conn_n_gated_rows": np.asarray(conn["n_gated_rows"], dtype=np.int64)})
        return out

    @staticmethod
    def metadata_from_npz(d):
        """The dict of ``to_metadata`` from the arrays of ``metadata_to_npz``, None when ``d`` holds none."""
        if "meta/conn_shape" not in d.files:
            return None
        ptr, flat = d["meta/conn_member_ptr"], d["meta/conn_members"].tolist()
        meta = dict(n_graphs=int(d["meta/conn_shape"][0]), n_kinds=int(d["meta/conn_shape"][1]),
                    members=[flat[int(a):int(b)] for a, b in zip(ptr[:-1], ptr[1:])], n_bonds=d["meta/conn_n_bonds"].tolist())
        if "meta/conn_gate_kinds" in d.files:
            ptr, flat = d["meta/conn_gate_kind_ptr"], d["meta/conn_gate_kinds"].tolist()
            meta.update(gate_kinds=[flat[int(a):int(b)] for a, b in zip(ptr[:-1], ptr[1:])],
                        max_blocked=d["meta/conn_max_blocked"].tolist(), n_gated_rows=d["meta/conn_n_gated_rows"].tolist())
        return meta


# ---- geometry -----------------------------------------------------------------------------------------------------------
def geometric_bonds(sc, cutoff=None, distances=None):
    """(bonds (nb, 2) int32, images (nb, 3) int8) of a ``synth`` or ``mson`` supercell: every (i, j, w) with
    ``|r_j + w.S - r_i|`` at most ``cutoff`` -- or equal to one of ``distances`` -- within ``SITE_TOL``, except i == j
    with w == 0; rows ordered by i, then by the displacement.  An image beyond ``MAX_IMAGE`` is refused."""
    from .structure import lattice_points_of

    prim = sc.model.prim
    L = np.asarray(prim.lattice, dtype=np.float64)
    tau = np.asarray(prim.frac_coords, dtype=np.float64)
    S = np.asarray(sc.scmatrix, dtype=np.int64)
    if S.ndim == 1:
        S = np.diag(S)
    n = lattice_points_of(sc)
    P, N = len(n), int(sc.num_sites)
    site_b = np.asarray(sc.site_b, dtype=np.int64)
    site_t = np.asarray(getattr(sc, "site_t", np.arange(N) % P), dtype=np.int64)
    Sinv = np.linalg.inv(S.astype(np.float64))
    det = int(round(abs(np.linalg.det(S.astype(np.float64)))))

    def cell_key(points):  # the class of a lattice point modulo the supercell, exact after rounding
        k = np.rint((points.astype(np.float64) @ Sinv) * det).astype(np.int64) % det
        return (k[:, 0] * det + k[:, 1]) * det + k[:, 2]

    order = np.argsort(cell_key(n))
    sorted_keys = cell_key(n)[order]
    # site index of (basis b, lattice point index t)
    site_of = np.full((len(tau), P), -1, dtype=np.int64)
    site_of[site_b, site_t] = np.arange(N)
    rmax = float(cutoff) if distances is None else max(distances, default=0.0)
    want = None if distances is None else np.asarray(sorted(distances), dtype=np.float64)
    Linv = np.linalg.inv(L)
    reach = np.ceil((rmax + SITE_TOL) * np.linalg.norm(Linv, axis=0) + 1).astype(int)  # |d_a + dtau_a| <= r |col a of L^-1|
    rows_b, rows_w = [], []
    for b, b2 in itertools.product(range(len(tau)), repeat=2):
        dtau = tau[b2] - tau[b]
        box = [range(-int(reach[a]) - 1, int(reach[a]) + 2) for a in range(3)]
        for d in itertools.product(*box):
            r = float(np.linalg.norm((np.asarray(d, dtype=np.float64) + dtau) @ L))
            if r < SITE_TOL:
                continue  # the site itself; its images are handled below (d a supercell vector: r > 0)
            if want is None:
                if r > rmax + SITE_TOL:
                    continue
            elif not np.any(np.abs(want - r) <= SITE_TOL):
                continue
            target = n + np.asarray(d, dtype=np.int64)      # (P, 3): lattice point of the far end, for every t
            pos = np.searchsorted(sorted_keys, cell_key(target))
            t2 = order[pos]
            w = np.rint((target - n[t2]).astype(np.float64) @ Sinv).astype(np.int64)
            if np.any(w @ S != target - n[t2]):
                raise RuntimeError("the far end of a bond is no lattice point of the supercell")
            if np.abs(w).max(initial=0) > MAX_IMAGE:
                raise ValueError(f"a bond of length {r:.6g} reaches image {int(np.abs(w).max())} of this supercell, beyond "
                                 f"MAX_IMAGE = {MAX_IMAGE}: image out of range")
            i, j = site_of[b, np.arange(P)], site_of[b2, t2]
            rows_b.append(np.stack([i, j], axis=1))
            rows_w.append(w)
    if not rows_b:
        return np.zeros((0, 2), dtype=np.int32), np.zeros((0, 3), dtype=np.int8)
    bonds, images = np.concatenate(rows_b), np.concatenate(rows_w)
    keep = np.lexsort((images[:, 2], images[:, 1], images[:, 0], bonds[:, 1], bonds[:, 0]))
    return bonds[keep].astype(np.int32), images[keep].astype(np.int8)


def channel_rows(bonds, images, corners=2):
    """(bonds, images, gates (nb', corners)): one row per *channel* of every bond row ``(i, j, w)`` of a bond list.  A channel
    is a set of ``corners`` (1 or 2) further sites of the unfolded lattice that are bonded to i, to j in image w and, for two
    corners, to each other, all by this bond list: the triangles and tetrahedra on the bond.  The gate sites are the
    corners folded back; in small and aliased cells one may coincide with an end or with the other corner.  A bond without
    a channel gets no row.  Rows keep the order of the bonds, the channels of a bond that of their corners."""
    if corners not in (1, 2):
        raise ValueError(f"corners must be 1 or 2, got {corners}: a channel is a triangle or a tetrahedron")
    nbr = {}
    for (i, j), w in zip(np.asarray(bonds).tolist(), np.asarray(images).tolist()):
        nbr.setdefault(i, set()).add((j, w[0], w[1], w[2]))
        nbr.setdefault(j, set()).add((i, -w[0], -w[1], -w[2]))
    rows_b, rows_w, rows_g = [], [], []
    for (i, j), w in zip(np.asarray(bonds).tolist(), np.asarray(images).tolist()):
        far = nbr[j]
        # the unfolded sites (k, u) bonded to both ends, the ends themselves left out
        common = sorted(c for c in nbr[i] if (c[0], c[1] - w[0], c[2] - w[1], c[3] - w[2]) in far
                        and c != (j, w[0], w[1], w[2]) and c != (i, 0, 0, 0))
        if corners == 1:
            channels = [(c[0],) for c in common]
        else:
            channels = [(c[0], d[0]) for n, c in enumerate(common) for d in common[n + 1:]
                        if (d[0], d[1] - c[1], d[2] - c[2], d[3] - c[3]) in nbr[c[0]]]
        for ch in channels:
            rows_b.append((i, j))
            rows_w.append(w)
            rows_g.append(ch)
    return (np.asarray(rows_b, dtype=np.int32).reshape(-1, 2), np.asarray(rows_w, dtype=np.int8).reshape(-1, 3),
            np.asarray(rows_g, dtype=np.int32).reshape(-1, corners))


# ---- derived quantities (host, pure NumPy on stats)-----------------------------------------------------------------------
def percolation_strength(stats):
    """wrapping_sites / n_members (..., G): the fraction of the members that lies in wrapping components; NaN without a
    member."""
    s = np.asarray(stats)
    with np.errstate(invalid="ignore", divide="ignore"):
        return s[..., WRAPPING_SITES] / s[..., N_MEMBERS].astype(np.float64)


def mean_finite_size(stats):
    """(sum_sq - largest^2) / (n_members - largest) (..., G): the mean size of the component a member lies in, the
    largest component left out.  The sum of the squared sizes of the WRAPPING components cannot be read from the columns
    (only their number and their sites), so the largest component stands for the spanning one, as is usual in finite
    cells; NaN when the largest component holds every member."""
    s = np.asarray(stats).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (s[..., SUM_SQ] - s[..., LARGEST] ** 2) / (s[..., N_MEMBERS] - s[..., LARGEST])


def wrapping_probability(stats, axes=None):
    """The fraction of the rows (first axis) in which a component wraps: any axis (``axes=None``), or every axis of
    ``axes`` (a 3-bit mask or a sequence of axis numbers) -- each possibly by another component.  (G,) or (..., G)."""
    s = np.asarray(stats)
    if axes is None:
        hit = s[..., WRAP_AXES] != 0
    else:
        mask = int(axes) if np.isscalar(axes) else sum(1 << int(a) for a in axes)
        hit = (s[..., WRAP_AXES] & mask) == mask
    return hit.mean(axis=0)


def size_distribution(stats):
    """The size histogram (..., G, 16): components with floor(log2 size) == b."""
    return np.asarray(stats)[..., HIST0:HIST0 + N_HIST]
