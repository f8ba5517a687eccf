"""Coordination environments of sampled states: how many sites of class a have exactly n_0 neighbours of class 0, n_1 of
class 1 ... in a shell.

This module is the DEFINITION: ``Environments.evaluate`` and ``Environments.codes`` in NumPy are what the device (the
census inside the observables' kernel, csrc/observables.hip: ``smolmc_eval_environments`` and the
``SMOLMC_SAMPLE_ENVIRONMENTS`` column of the sample ring) matches entry for entry.  Everything is int32, so the order of
summation is no concern.

A spec rests on an ``observables.Observables``: the *kind* of (site, code) is ``kind_base[site] + code`` and there are K
kinds.  It holds E sets, 1 <= E <= 8.  Set e has a width z (1..64), A centre classes (1..15) and B neighbour classes
(1..4), the maps ``centre_class_of_kind`` (K,) with values in -1 .. A - 1 and ``neigh_class_of_kind`` (K,) with values in
-1 .. B - 1, and n centres, each a site with a row of z neighbour sites; a slot that holds -1 is empty.  Per occupancy
and set, for every centre AS LISTED:

    a    = centre_class_of_kind[kind(centre)]      the centre is skipped when it is not counted or a == -1
    n_b  = #{slots of its row that are not empty, whose site is counted and whose neighbour class is b}
    code = a (z + 1)**B + sum_b n_b (z + 1)**(B - 1 - b);      cells[cell_ptr[e] + code] += 1

(row-major, class 0 most significant, as the cells of patterns and pairs are).  A slot whose site is not counted or has
class -1 adds to no n_b and does not skip the centre.  Duplicate centres, slots that repeat a site and slots that name the
centre itself, as in an aliased cell, count as they stand.  ``n_cells = sum_e A_e (z_e + 1)**B_e <= MAX_ENV_CELLS``: the
plain product, not the simplex -- wasteful, trivially indexable.  The pair counts of a shell are the first moment of this
distribution; a centre with its 12 fcc neighbours is out of reach of ``patterns`` (13 sites, 3**12 positional cells).
"""

from __future__ import annotations

import math

import numpy as np

from . import patterns as _patterns

MAX_ENV_SETS = 8             # SMOLMC_MAX_ENV_SETS
MAX_ENV_WIDTH = 64           # SMOLMC_MAX_ENV_WIDTH
MAX_ENV_CENTRE_CLASSES = 15  # SMOLMC_MAX_ENV_CENTRE_CLASSES: a site's two classes are staged as the nibbles of one byte
MAX_ENV_NEIGH_CLASSES = 4    # SMOLMC_MAX_ENV_NEIGH_CLASSES
MAX_ENV_CELLS = 4096         # SMOLMC_MAX_ENV_CELLS


def _class_map(m, n, what):
    m = np.asarray(m)
    if m.ndim != 1 or not np.issubdtype(m.dtype, np.integer):
        raise ValueError(f"{what} must be a 1-D integer array, one entry per kind")
    if m.min(initial=0) < -1 or m.max(initial=-1) >= n:
        raise ValueError(f"{what} must hold -1 .. {n - 1}: class out of range")
    return np.ascontiguousarray(m, dtype=np.int32)


class EnvironmentSet:
    """One set: ``centres`` (n,) sites, ``neighbours`` (n, z) sites or -1 for an empty slot, and the two class maps (K,)."""

    def __init__(self, centres, neighbours, centre_class_of_kind, n_centre_classes, neigh_class_of_kind, n_neigh_classes):
        c, nb = np.asarray(centres), np.asarray(neighbours)
        if c.size == 0:
            c = np.zeros(0, dtype=np.int32)
        if c.ndim != 1 or not np.issubdtype(c.dtype, np.integer):
            raise ValueError("centres must be a 1-D integer array of sites")
        if nb.ndim != 2 or nb.shape[0] != len(c) or (nb.size and not np.issubdtype(nb.dtype, np.integer)):
            raise ValueError("neighbours must be an (ncentres, width) integer array, one row per centre")
        if not 1 <= nb.shape[1] <= MAX_ENV_WIDTH:
            raise ValueError(f"width must be 1..{MAX_ENV_WIDTH}, got {nb.shape[1]}")
        self.centres = np.ascontiguousarray(c, dtype=np.int32)
        self.neighbours = np.ascontiguousarray(nb, dtype=np.int32)
        self.n_centre_classes, self.n_neigh_classes = int(n_centre_classes), int(n_neigh_classes)
        if not 1 <= self.n_centre_classes <= MAX_ENV_CENTRE_CLASSES:
            raise ValueError(f"n_centre_classes must be 1..{MAX_ENV_CENTRE_CLASSES}, got {self.n_centre_classes}")
        if not 1 <= self.n_neigh_classes <= MAX_ENV_NEIGH_CLASSES:
            raise ValueError(f"n_neigh_classes must be 1..{MAX_ENV_NEIGH_CLASSES}, got {self.n_neigh_classes}")
        self.centre_class_of_kind = _class_map(centre_class_of_kind, self.n_centre_classes, "centre_class_of_kind")
        self.neigh_class_of_kind = _class_map(neigh_class_of_kind, self.n_neigh_classes, "neigh_class_of_kind")
        if len(self.centre_class_of_kind) != len(self.neigh_class_of_kind):
            raise ValueError("the two class maps must have one entry per kind each")

    width = property(lambda self: self.neighbours.shape[1])
    n_centres = property(lambda self: len(self.centres))
    n_cells = property(lambda self: self.n_centre_classes * (self.width + 1) ** self.n_neigh_classes)
    shape = property(lambda self: (self.n_centre_classes,) + (self.width + 1,) * self.n_neigh_classes)


class Environments:
    """The spec: the observables whose kinds the class maps index, and 1..8 ``EnvironmentSet``s."""

    def __init__(self, observables, sets):
        self.observables = observables
        self.sets = list(sets)
        self.num_sites, self.n_kinds = observables.num_sites, observables.n_kinds
        if not 1 <= len(self.sets) <= MAX_ENV_SETS:
            raise ValueError(f"an environment spec holds 1..{MAX_ENV_SETS} sets, got {len(self.sets)}")
        for e, st in enumerate(self.sets):
            if len(st.centre_class_of_kind) != self.n_kinds:
                raise ValueError(f"set {e}: the class maps have {len(st.centre_class_of_kind)} entries, the observables have "
                                 f"{self.n_kinds} kinds")
            if st.centres.min(initial=0) < 0 or st.centres.max(initial=0) >= self.num_sites:
                raise ValueError(f"set {e}: centre out of range ({self.num_sites} sites)")
            if st.neighbours.min(initial=0) < -1 or st.neighbours.max(initial=0) >= self.num_sites:
                raise ValueError(f"set {e}: neighbour slot out of range ({self.num_sites} sites, -1 for an empty slot)")
        ptr = [0]
        for st in self.sets:
            ptr.append(ptr[-1] + st.n_cells)
        if ptr[-1] > MAX_ENV_CELLS:
            raise ValueError(f"{ptr[-1]} cells, larger than MAX_ENV_CELLS = {MAX_ENV_CELLS}")
        self.cell_ptr = np.asarray(ptr, dtype=np.int64)
        self.centre_ptr = np.concatenate(([0], np.cumsum([st.n_centres for st in self.sets]))).astype(np.int64)

    n_sets = property(lambda self: len(self.sets))
    n_cells = property(lambda self: int(self.cell_ptr[-1]))
    n_centres = property(lambda self: int(self.centre_ptr[-1]))

    # ---- constructors -------------------------------------------------------------------------------------------
    @classmethod
    def from_rows(cls, observables, centres, neighbours, centre_classes="kind", neigh_classes="kind"):
        """One set per entry of ``centres`` / ``neighbours`` (lists of (n,) and (n, z) arrays of sites in the caller's
        numbering; one pair of plain arrays makes one set).  The classes: one value for all sets or a list with one per
        set, each ``"kind"``, ``"code"``, a (K,) array (``patterns.Patterns.class_map``) or a pair (array, n_classes)."""
        if (len(centres) == 0 or np.ndim(centres[0]) == 0) and np.ndim(neighbours) == 2:  # (one set: sites, not arrays of sites)
            centres, neighbours = [centres], [neighbours]
        if len(centres) != len(neighbours):
            raise ValueError("centres and neighbours must list the same number of sets")

        def per_set(c):
            out = list(c) if isinstance(c, list) else [c] * len(centres)
            if len(out) != len(centres):
                raise ValueError("classes must be one value or a list with one entry per set")
            return [x if isinstance(x, tuple) else _patterns.Patterns.class_map(observables, x) for x in out]

        sets = [EnvironmentSet(c, nb, ca[0], ca[1], cb[0], cb[1])
                for c, nb, ca, cb in zip(centres, neighbours, per_set(centre_classes), per_set(neigh_classes))]
        return cls(observables, sets)

    @classmethod
    def from_supercell(cls, sc, observables, orbits=None, cutoff=None, distances=None, centres=None, centre_classes="code",
                       neigh_classes="code"):
        """One set per shell of ``sc``.  ``orbits``: pair-orbit ids, one set each -- the rows of ``sc.full_indices`` read
        in both directions, so that (i, j) puts j into the row of i and i into the row of j.  Otherwise ``cutoff`` or
        ``distances``: one set of the bonds ``connectivity.geometric_bonds`` finds.  Self-image and multi-image bonds of a
        small cell are kept as repeated slots.  ``centres``: the sites that are centres (default: every site with a
        neighbour), in ascending order; rows shorter than the widest are filled up with -1."""
        if sc.num_sites != observables.num_sites:
            raise ValueError("observables and supercell have different numbers of sites")
        if (orbits is None) == (cutoff is None and distances is None):
            raise ValueError("name the shell by orbits= or by cutoff= / distances=")
        shells = []
        if orbits is not None:
            by_id = {orb.id: np.asarray(rows, dtype=np.int64) for orb, rows in zip(sc.model.orbits, sc.full_indices) if orb.size == 2}
            for i in orbits:
                if i not in by_id:
                    raise ValueError(f"orbit {i} is no pair orbit of the supercell")
                shells.append(np.concatenate([by_id[i], by_id[i][:, ::-1]]))
        else:
            from .connectivity import geometric_bonds

            shells.append(geometric_bonds(sc, cutoff=cutoff, distances=distances)[0].astype(np.int64))
        cen, rows = [], []
        for bonds in shells:
            order = np.argsort(bonds[:, 0], kind="stable")
            bonds = bonds[order]
            who = np.unique(bonds[:, 0]) if centres is None else np.unique(np.asarray(centres, dtype=np.int64))
            n_of = np.bincount(bonds[:, 0], minlength=sc.num_sites)
            z = int(n_of[who].max(initial=0))
            if z < 1:
                raise ValueError("no centre has a neighbour in the shell")
            first = np.concatenate(([0], np.cumsum(n_of)))
            nb = np.full((len(who), z), -1, dtype=np.int32)
            for r, s in enumerate(who):
                nb[r, :n_of[s]] = bonds[first[s]:first[s + 1], 1]
            cen.append(who.astype(np.int32))
            rows.append(nb)
        return cls.from_rows(observables, cen, rows, centre_classes, neigh_classes)

    # ---- the definition ------------------------------------------------------------------------------------------
    def _codes(self, kinds, e):
        """codes (n, n_centres of set e) int64 of kinds (n, N), -1 for a skipped centre"""
        st = self.sets[e]
        z1, B = st.width + 1, st.n_neigh_classes
        ext = np.concatenate([kinds, np.full((len(kinds), 1), -1, dtype=np.int64)], axis=1)  # (slot -1 reads the last column)
        cb = np.append(st.neigh_class_of_kind.astype(np.int64), -1)                            # (kind -1 reads the last entry)
        ca = np.append(st.centre_class_of_kind.astype(np.int64), -1)
        b = cb[ext[:, st.neighbours]]                                                          # (n, ncentres, z)
        a = ca[kinds[:, st.centres]]                                                           # (n, ncentres)
        code = a * z1 ** B
        for k in range(B):
            code = code + (b == k).sum(axis=-1) * z1 ** (B - 1 - k)
        return np.where(a >= 0, code, -1)

    def evaluate(self, occupancies):
        """cells (..., n_cells) int32 of occupancies (..., N)."""
        kinds = self.observables.kinds_of(occupancies)
        lead = kinds.shape[:-1]
        kinds = kinds.reshape(-1, self.num_sites)
        n = len(kinds)
        out = np.zeros((n, self.n_cells), dtype=np.int64)
        row = np.arange(n, dtype=np.int64)[:, None]
        for e, st in enumerate(self.sets):
            code = self._codes(kinds, e)
            nc = st.n_cells
            out[:, self.cell_ptr[e]:self.cell_ptr[e + 1]] = np.bincount((row * nc + code)[code >= 0], minlength=n * nc).reshape(n, nc)
        return out.astype(np.int32).reshape(lead + (self.n_cells,))

    def codes(self, occupancies):
        """codes (..., n_centres) int32 of occupancies (..., N): the set-local code of every centre, set after set, -1 for
        a skipped centre."""
        kinds = self.observables.kinds_of(occupancies)
        lead = kinds.shape[:-1]
        kinds = kinds.reshape(-1, self.num_sites)
        out = np.concatenate([self._codes(kinds, e) for e in range(self.n_sets)], axis=1)
        return out.astype(np.int32).reshape(lead + (self.n_centres,))

    def code(self, e, a, counts):
        """The set-local code of a centre of class ``a`` with ``counts`` = (n_0 .. n_{B-1}) neighbours."""
        st = self.sets[e]
        if len(counts) != st.n_neigh_classes or min(counts) < 0 or sum(counts) > st.width or not 0 <= a < st.n_centre_classes:
            raise ValueError(f"set {e} takes a centre class in 0..{st.n_centre_classes - 1} and {st.n_neigh_classes} counts "
                             f"that sum to {st.width} at most")
        v = int(a)
        for n in counts:
            v = v * (st.width + 1) + int(n)
        return v

    def cell(self, e, a, counts):
        """The number of the cell of set ``e`` that counts centres of class ``a`` with ``counts`` neighbours."""
        return int(self.cell_ptr[e]) + self.code(e, a, counts)

    # ---- the C struct ------------------------------------------------------------------------------------------
    def c_struct(self):
        """(capi.smolmc_environments, the arrays it points at -- keep them alive during the call)."""
        import ctypes as C

        from . import capi

        i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)  # noqa: E731
        width = i32([st.width for st in self.sets])
        na = i32([st.n_centre_classes for st in self.sets])
        nb = i32([st.n_neigh_classes for st in self.sets])
        ca = i32(np.stack([st.centre_class_of_kind for st in self.sets]))
        cb = i32(np.stack([st.neigh_class_of_kind for st in self.sets]))
        ptr = np.ascontiguousarray(self.centre_ptr, dtype=np.int64)
        cen = i32(np.concatenate([st.centres for st in self.sets] + [np.zeros(1, np.int32)]))
        rows = i32(np.concatenate([st.neighbours.reshape(-1) for st in self.sets] + [np.zeros(1, np.int32)]))
        s = capi.smolmc_environments()
        s.n_sets = self.n_sets
        p = lambda v, t=C.c_int32: v.ctypes.data_as(C.POINTER(t))  # noqa: E731
        s.width, s.n_centre_classes, s.n_neigh_classes = p(width), p(na), p(nb)
        s.centre_class_of_kind, s.neigh_class_of_kind = p(ca), p(cb)
        s.centre_ptr = p(ptr, C.c_int64)
        s.centres, s.neighbours = p(cen), p(rows)
        return s, (width, na, nb, ca, cb, ptr, cen, rows)

    def describe(self):
        """What a container keeps of the spec (plain lists: it goes into the metadata of an npz or a stream)."""
        return dict(n_sets=self.n_sets, n_cells=self.n_cells, width=[st.width for st in self.sets],
                    n_centre_classes=[st.n_centre_classes for st in self.sets],
                    n_neigh_classes=[st.n_neigh_classes for st in self.sets], n_centres=[st.n_centres for st in self.sets],
                    cell_ptr=self.cell_ptr.tolist(), centre_class_of_kind=[st.centre_class_of_kind.tolist() for st in self.sets],
                    neigh_class_of_kind=[st.neigh_class_of_kind.tolist() for st in self.sets])

    @staticmethod
    def metadata_to_npz(env):
        """The meta/* arrays of an .npz for the dict of ``describe``."""
        return {"meta/env_shape": np.asarray([env["width"], env["n_centre_classes"], env["n_neigh_classes"], env["n_centres"]],
                                             dtype=np.int64),
                "meta/env_cell_ptr": np.asarray(env["cell_ptr"], dtype=np.int64),
                "meta/env_centre_class_of_kind": np.asarray(env["centre_class_of_kind"], dtype=np.int32),
                "meta/env_neigh_class_of_kind": np.asarray(env["neigh_class_of_kind"], dtype=np.int32)}

    @staticmethod
    def metadata_from_npz(d):
        """The dict of ``describe`` from the arrays of ``metadata_to_npz``, None when ``d`` holds none."""
        if "meta/env_shape" not in d.files:
            return None
        width, na, nb, ncen = (d["meta/env_shape"][i].tolist() for i in range(4))
        ptr = d["meta/env_cell_ptr"].tolist()
        return dict(n_sets=len(width), n_cells=int(ptr[-1]), width=width, n_centre_classes=na, n_neigh_classes=nb,
                    n_centres=ncen, cell_ptr=ptr, centre_class_of_kind=d["meta/env_centre_class_of_kind"].tolist(),
                    neigh_class_of_kind=d["meta/env_neigh_class_of_kind"].tolist())

    # ---- derived quantities (host) ---------------------------------------------------------------------------------
    def distribution(self, cells, e):
        """The cells of set ``e`` as an array (..., A, z + 1, ..., z + 1): the centre class, then one axis per neighbour
        class."""
        c = np.asarray(cells)[..., self.cell_ptr[e]:self.cell_ptr[e + 1]]
        return c.reshape(c.shape[:-1] + self.sets[e].shape)

    def marginal(self, cells, e, b):
        """(..., A, z + 1): how many centres of every class have n neighbours of class ``b``."""
        st = self.sets[e]
        if not 0 <= b < st.n_neigh_classes:
            raise ValueError(f"set {e} has neighbour classes 0..{st.n_neigh_classes - 1}")
        d = self.distribution(cells, e).astype(np.int64)
        drop = tuple(d.ndim - st.n_neigh_classes + k for k in range(st.n_neigh_classes) if k != b)
        return d.sum(axis=drop)

    def mean_coordination(self, cells, e):
        """(..., A, B): the mean number of neighbours of class b around a centre of class a (NaN where no centre has
        class a).  Its numerator is what the pair counts of the shell hold."""
        st = self.sets[e]
        n = np.arange(st.width + 1, dtype=np.float64)
        m = np.stack([(self.marginal(cells, e, b) * n).sum(axis=-1) for b in range(st.n_neigh_classes)], axis=-1)
        tot = self.distribution(cells, e).astype(np.int64).reshape(m.shape[:-1] + (-1,)).sum(axis=-1)
        with np.errstate(invalid="ignore", divide="ignore"):
            return m / tot[..., None]

    def compositions(self, cells, e):
        """Fold the product cells of set ``e`` to the simplex: (census (..., A, n_compositions) int64, compositions
        (n_compositions, B + 1)).  A composition is (n_0 .. n_{B-1}, the slots that are empty or have no class); the rows
        come from ``patterns.compositions(z, B + 1)`` with the slots without a class as its first column moved last."""
        st = self.sets[e]
        z, B = st.width, st.n_neigh_classes
        comp = _patterns.compositions(z, B + 1)           # (n_rest, n_0 .. n_{B-1}) with n_rest = z - the others
        d = self.distribution(cells, e).astype(np.int64)
        census = np.stack([d[(Ellipsis,) + tuple(int(x) for x in row[1:])] for row in comp], axis=-1)
        return census, np.concatenate([comp[:, 1:], comp[:, :1]], axis=1)

    def random_alloy(self, counts, e):
        """The cells of set ``e`` a random alloy of the sample's own composition is expected to have, (..., A, z + 1, ...)
        float64 like ``distribution``: ``counts`` (..., K) are the kind counts of the observables.  The centres are shared
        out over the centre classes as the counted kinds with a centre class are, N_a = n_centres c_a; every one of the z
        slots holds class b independently with p_b, the share of class b among the counted kinds with a neighbour class:
        cell (a, n_0 ..) = N_a z! / prod_b n_b! prod_b p_b**n_b where sum_b n_b = z, 0 elsewhere.  It assumes rows
        without empty slots whose sites all have a class, and sums to the number of centres."""
        st = self.sets[e]
        z, B = st.width, st.n_neigh_classes
        c = np.asarray(counts).astype(np.float64)
        fold = lambda m, n: np.stack([c[..., m == k].sum(axis=-1) for k in range(n)], axis=-1)  # noqa: E731
        ca, cb = fold(st.centre_class_of_kind, st.n_centre_classes), fold(st.neigh_class_of_kind, B)
        with np.errstate(invalid="ignore", divide="ignore"):
            Na = st.n_centres * ca / ca.sum(axis=-1, keepdims=True)
            p = cb / cb.sum(axis=-1, keepdims=True)
        out = np.zeros(c.shape[:-1] + st.shape)
        for row in _patterns.compositions(z, B):
            w = math.factorial(z)
            for n in row:
                w //= math.factorial(int(n))
            out[(Ellipsis,) + tuple(int(n) for n in row)] = Na * (w * np.prod(p ** row, axis=-1))[..., None]
        return out

    def sites_with(self, codes, e, code):
        """The centres of set ``e`` (sites, as listed) whose environment in ONE state has the set-local ``code``
        (``Environments.code``); ``codes`` (n_centres,) is a row of ``codes`` or of the engine's."""
        row = np.asarray(codes)
        if row.shape != (self.n_centres,):
            raise ValueError(f"codes must be one row of {self.n_centres} entries")
        return self.sets[e].centres[row[self.centre_ptr[e]:self.centre_ptr[e + 1]] == int(code)]
