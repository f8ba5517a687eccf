"""Species patterns on site tuples of sampled states: how often every pattern of classes occurs on the triplets,
tetrahedra ... of a list.

This module is the DEFINITION: ``Patterns.evaluate`` in NumPy is what the device (the census inside the observables'
kernel, csrc/observables.hip: ``smolmc_eval_patterns`` and the ``SMOLMC_SAMPLE_PATTERNS`` column of the sample ring)
matches entry for entry.  Everything is int32, so the order of summation is no concern.

A spec rests on an ``observables.Observables``: the *kind* of (site, code) is ``kind_base[site] + code`` and there are K
kinds.  It holds T sets, 1 <= T <= 8.  Set t has an arity m (1..8), a class map ``class_of_kind`` (K,) with values in
0 .. C - 1 or -1, and n site tuples (i_0 .. i_{m-1}).  Per occupancy and set, for every tuple AS LISTED:

    c_p = class_of_kind[kind(i_p)];   cells[cell_ptr[t] + sum_p c_p * C**(m - 1 - p)] += 1

(row-major, the first position most significant, as ``pairs[ka][kb]`` is).  A tuple is skipped when one of its sites is
not counted (``kind_base < 0``) or holds a kind whose class is -1.  Duplicate tuples and tuples that name a site twice, as
in an aliased cell, count as they stand.  ``n_cells = sum_t C_t**m_t <= MAX_PATTERN_CELLS``.  A set of arity 2 with the
identity class map is a pair shell of the observables.
"""

from __future__ import annotations

import itertools

import numpy as np

MAX_PATTERN_SETS = 8       # SMOLMC_MAX_PATTERN_SETS
MAX_PATTERN_ARITY = 8      # SMOLMC_MAX_PATTERN_ARITY
MAX_PATTERN_CLASSES = 255  # SMOLMC_MAX_PATTERN_CLASSES: a class is staged as one byte on the device, 0xff marks a skip
MAX_PATTERN_CELLS = 4096   # SMOLMC_MAX_PATTERN_CELLS


class PatternSet:
    """One set: ``sites`` (n, m) integer site tuples, ``class_of_kind`` (K,) integers in -1 .. ``n_classes`` - 1."""

    def __init__(self, sites, class_of_kind, n_classes):
        s = np.asarray(sites)
        if s.ndim != 2 or not np.issubdtype(s.dtype, np.integer):
            raise ValueError("sites must be an (ntuples, arity) integer array")
        if not 1 <= s.shape[1] <= MAX_PATTERN_ARITY:
            raise ValueError(f"arity must be 1..{MAX_PATTERN_ARITY}, got {s.shape[1]}")
        self.sites = np.ascontiguousarray(s, dtype=np.int32)
        self.n_classes = int(n_classes)
        if not 1 <= self.n_classes <= MAX_PATTERN_CLASSES:
            raise ValueError(f"n_classes must be 1..{MAX_PATTERN_CLASSES}, got {self.n_classes}")
        m = np.asarray(class_of_kind)
        if m.ndim != 1 or not np.issubdtype(m.dtype, np.integer):
            raise ValueError("class_of_kind must be a 1-D integer array, one entry per kind")
        if m.min(initial=0) < -1 or m.max(initial=-1) >= self.n_classes:
            raise ValueError(f"class_of_kind must hold -1 .. {self.n_classes - 1}: class out of range")
        self.class_of_kind = np.ascontiguousarray(m, dtype=np.int32)

    arity = property(lambda self: self.sites.shape[1])
    n_tuples = property(lambda self: self.sites.shape[0])
    n_cells = property(lambda self: self.n_classes ** self.arity)


class Patterns:
    """The spec: the observables whose kinds the class maps index, and 1..8 ``PatternSet``s."""

    def __init__(self, observables, sets, set_orbit_ids=None):
        self.observables = observables
        self.sets = list(sets)
        self.num_sites, self.n_kinds = observables.num_sites, observables.n_kinds
        if not 1 <= len(self.sets) <= MAX_PATTERN_SETS:
            raise ValueError(f"a pattern spec holds 1..{MAX_PATTERN_SETS} sets, got {len(self.sets)}")
        for t, st in enumerate(self.sets):
            if len(st.class_of_kind) != self.n_kinds:
                raise ValueError(f"set {t}: class_of_kind has {len(st.class_of_kind)} entries, the observables have "
                                 f"{self.n_kinds} kinds")
            if st.sites.min(initial=0) < 0 or st.sites.max(initial=0) >= self.num_sites:
                raise ValueError(f"set {t}: site out of range ({self.num_sites} sites)")
        ptr = [0]
        for st in self.sets:
            ptr.append(ptr[-1] + st.n_cells)
        if ptr[-1] > MAX_PATTERN_CELLS:
            raise ValueError(f"{ptr[-1]} cells, larger than MAX_PATTERN_CELLS = {MAX_PATTERN_CELLS}")
        self.cell_ptr = np.asarray(ptr, dtype=np.int64)
        self.set_orbit_ids = None if set_orbit_ids is None else [int(i) for i in set_orbit_ids]

    n_sets = property(lambda self: len(self.sets))
    n_cells = property(lambda self: int(self.cell_ptr[-1]))

    # ---- constructors -------------------------------------------------------------------------------------------
    @staticmethod
    def class_map(observables, classes="kind"):
        """(class_of_kind (K,), n_classes) of ``"kind"`` (the identity), ``"code"`` (a kind's species code; needs
        observables whose kinds stand for one code each) or an explicit (K,) array (classes 0 .. max, -1: skip)."""
        K = observables.n_kinds
        if isinstance(classes, str) and classes == "kind":
            return np.arange(K, dtype=np.int32), K
        if isinstance(classes, str) and classes == "code":
            if observables.kind_code is None:
                raise ValueError('classes="code" needs site_ncodes, and kinds that stand for one species code each')
            code = np.asarray(observables.kind_code, dtype=np.int32)
            return code, int(code.max(initial=0)) + 1
        m = np.asarray(classes)
        if m.shape != (K,) or not np.issubdtype(m.dtype, np.integer):
            raise ValueError(f'classes must be "kind", "code" or one integer per kind ({K})')
        return m.astype(np.int32), int(m.max(initial=0)) + 1

    @classmethod
    def from_tuples(cls, observables, tuples, classes="kind"):
        """One set per entry of ``tuples`` (each an (n, m) array of sites in the caller's numbering); ``classes``: one
        value for all sets or a list with one per set, each as ``class_map`` takes it or a pair (array, n_classes)."""
        tuples = list(tuples)
        per_set = classes if isinstance(classes, list) else [classes] * len(tuples)
        if len(per_set) != len(tuples):
            raise ValueError("classes must be one value or a list with one entry per set")
        sets = []
        for sites, c in zip(tuples, per_set):
            m, C = c if isinstance(c, tuple) else cls.class_map(observables, c)
            sets.append(PatternSet(sites, m, C))
        return cls(observables, sets)

    @classmethod
    def from_supercell(cls, sc, observables, orbits=None, classes="code"):
        """One set per orbit of ``sc`` with three sites or more (``sc.full_indices`` row for row); ``orbits`` restricts
        them to these orbit ids.  ``classes="code"`` maps a kind to its species code, so that the digits of a cell are the
        codes ``orbit.flat_tensor_indices`` strides over and ``correlations`` can contract the cells with the orbit's
        correlation tensors; an array (K,) names other classes.  Clusters beyond the expansion's cutoffs: pass the
        supercell of a second ``synth.build_cluster_model`` with larger cutoffs on the same prim."""
        if sc.num_sites != observables.num_sites:
            raise ValueError("observables and supercell have different numbers of sites")
        m, C = cls.class_map(observables, classes)
        sets, ids = [], []
        for orb, rows in zip(sc.model.orbits, sc.full_indices):
            if orb.size >= 3 and (orbits is None or orb.id in orbits):
                sets.append(PatternSet(np.asarray(rows, dtype=np.int32), m, C))
                ids.append(orb.id)
        if not sets:
            raise ValueError("no orbit with three sites or more" + ("" if orbits is None else f" among {list(orbits)}"))
        if len(sets) > MAX_PATTERN_SETS:
            raise ValueError(f"{len(sets)} orbits with three sites or more, a spec holds {MAX_PATTERN_SETS}: name some with orbits=")
        return cls(observables, sets, set_orbit_ids=ids)

    # ---- the definition ------------------------------------------------------------------------------------------
    def evaluate(self, occupancies):
        """cells (..., n_cells) int32 of occupancies (..., N)."""
        kinds = self.observables.kinds_of(occupancies)
        lead = kinds.shape[:-1]
        kinds = kinds.reshape(-1, self.num_sites)
        n = len(kinds)
        out = np.zeros((n, self.n_cells), dtype=np.int64)
        row = np.arange(n, dtype=np.int64)[:, None]
        for t, st in enumerate(self.sets):
            cmap = np.append(st.class_of_kind.astype(np.int64), -1)  # (kind -1 reads the last entry)
            c = cmap[kinds][:, st.sites]                               # (n, ntuples, m)
            ok = np.all(c >= 0, axis=-1)
            weight = st.n_classes ** np.arange(st.arity - 1, -1, -1, dtype=np.int64)
            cell = (c * weight).sum(axis=-1)
            nc = st.n_cells
            out[:, self.cell_ptr[t]:self.cell_ptr[t + 1]] = np.bincount((row * nc + cell)[ok], minlength=n * nc).reshape(n, nc)
        return out.astype(np.int32).reshape(lead + (self.n_cells,))

    def cell(self, t, classes):
        """The number of the cell of set ``t`` that counts the pattern ``classes`` (one class per position)."""
        st = self.sets[t]
        if len(classes) != st.arity or min(classes) < 0 or max(classes) >= st.n_classes:
            raise ValueError(f"set {t} takes {st.arity} classes in 0..{st.n_classes - 1}")
        v = 0
        for c in classes:
            v = v * st.n_classes + int(c)
        return int(self.cell_ptr[t]) + v

    # ---- the C struct ------------------------------------------------------------------------------------------
    def c_struct(self):
        """(capi.smolmc_patterns, the arrays it points at -- keep them alive during the call)."""
        import ctypes as C

        from . import capi

        arity = np.array([st.arity for st in self.sets], dtype=np.int32)
        ncls = np.array([st.n_classes for st in self.sets], dtype=np.int32)
        cmap = np.ascontiguousarray(np.stack([st.class_of_kind for st in self.sets]), dtype=np.int32)
        ptr = np.concatenate(([0], np.cumsum([st.n_tuples for st in self.sets]))).astype(np.int64)
        sites = np.ascontiguousarray(np.concatenate([st.sites.reshape(-1) for st in self.sets]), dtype=np.int32)
        if len(sites) == 0:
            sites = np.zeros(1, dtype=np.int32)
        s = capi.smolmc_patterns()
        s.n_sets = self.n_sets
        s.arity = arity.ctypes.data_as(C.POINTER(C.c_int32))
        s.n_classes = ncls.ctypes.data_as(C.POINTER(C.c_int32))
        s.class_of_kind = cmap.ctypes.data_as(C.POINTER(C.c_int32))
        s.tuple_ptr = ptr.ctypes.data_as(C.POINTER(C.c_int64))
        s.sites = sites.ctypes.data_as(C.POINTER(C.c_int32))
        return s, (arity, ncls, cmap, ptr, sites)

    def describe(self):
        """What a container keeps of the spec (plain lists: it goes into the metadata of an npz or a stream)."""
        return dict(n_sets=self.n_sets, n_cells=self.n_cells, arity=[st.arity for st in self.sets],
                    n_classes=[st.n_classes for st in self.sets], n_tuples=[st.n_tuples for st in self.sets],
                    cell_ptr=self.cell_ptr.tolist(), class_of_kind=[st.class_of_kind.tolist() for st in self.sets],
                    set_orbit_ids=self.set_orbit_ids)

    @staticmethod
    def metadata_to_npz(pat):
        """The meta/* arrays of an .npz for the dict of ``describe``."""
        return {"meta/pat_shape": np.asarray([pat["arity"], pat["n_classes"], pat["n_tuples"]], dtype=np.int64),
                "meta/pat_cell_ptr": np.asarray(pat["cell_ptr"], dtype=np.int64),
                "meta/pat_class_of_kind": np.asarray(pat["class_of_kind"], dtype=np.int32),
                "meta/pat_orbit_ids": np.asarray(pat["set_orbit_ids"] if pat["set_orbit_ids"] is not None else [], dtype=np.int64)}

    @staticmethod
    def metadata_from_npz(d):
        """The dict of ``describe`` from the arrays of ``metadata_to_npz``, None when ``d`` holds none."""
        if "meta/pat_shape" not in d.files:
            return None
        arity, ncls, ntup = (d["meta/pat_shape"][i].tolist() for i in range(3))
        ptr, ids = d["meta/pat_cell_ptr"].tolist(), d["meta/pat_orbit_ids"].tolist()
        return dict(n_sets=len(arity), n_cells=int(ptr[-1]), arity=arity, n_classes=ncls, n_tuples=ntup, cell_ptr=ptr,
                    class_of_kind=d["meta/pat_class_of_kind"].tolist(), set_orbit_ids=ids if ids else None)

    # ---- derived quantities (host) ---------------------------------------------------------------------------------
    def cells_of(self, cells, t):
        """The cells of set ``t`` as an array (..., C, ..., C), one axis per position."""
        st = self.sets[t]
        c = np.asarray(cells)[..., self.cell_ptr[t]:self.cell_ptr[t + 1]]
        return c.reshape(c.shape[:-1] + (st.n_classes,) * st.arity)

    def composition_census(self, cells, t):
        """Fold the ordered cells of set ``t`` into class-count compositions -- with two classes the tuples that hold
        0, 1 .. m sites of class 1: (census (..., n_compositions) int64, compositions (n_compositions, C)), the
        compositions in ascending order of (n_1, n_2 ...), n_0 = m - the rest."""
        st = self.sets[t]
        return composition_census(np.asarray(cells)[..., self.cell_ptr[t]:self.cell_ptr[t + 1]], st.arity, st.n_classes)

    def probabilities(self, cells):
        """Pattern probabilities (..., n_cells): every set's cells over their sum (NaN for a set that counted nothing)."""
        return probabilities(cells, self.cell_ptr)

    def correlations(self, cells, orbit, t=None):
        """Contract the cells of set ``t`` with the orbit's ``flat_correlation_tensors``: (..., K_orbit), the SUM over the
        set's tuples of every correlation function of the orbit; divided by the number of tuples it is the orbit's slice
        of the correlation vector.  Needs classes that are species codes (``classes="code"``); ``t`` defaults to the set
        built from that orbit (``from_supercell``)."""
        if t is None:
            if self.set_orbit_ids is None or orbit.id not in self.set_orbit_ids:
                raise ValueError(f"no set was built from orbit {orbit.id}: pass t=")
            t = self.set_orbit_ids.index(orbit.id)
        st = self.sets[t]
        if st.arity != orbit.size:
            raise ValueError(f"set {t} has arity {st.arity}, the orbit {orbit.size} sites")
        ct = np.asarray(orbit.flat_correlation_tensors)  # (K_orbit, S_0 * ... * S_{m-1})
        shape = np.asarray(orbit.corr_tensors).shape[1:]
        strides = [int(x) for x in orbit.flat_tensor_indices]
        c = np.asarray(cells)[..., self.cell_ptr[t]:self.cell_ptr[t + 1]]
        used = np.flatnonzero(np.any(c.reshape(-1, st.n_cells) != 0, axis=0))
        out = np.zeros(c.shape[:-1] + (ct.shape[0],))
        for v in used:
            digits = [(int(v) // st.n_classes ** (st.arity - 1 - p)) % st.n_classes for p in range(st.arity)]
            if any(d >= s for d, s in zip(digits, shape)):
                raise ValueError(f"cell {int(v)} of set {t} holds class {max(digits)}, which is no species code of the orbit's sites")
            out += c[..., v, None] * ct[:, sum(d * s for d, s in zip(digits, strides))]
        return out


def compositions(arity, n_classes):
    """(n_compositions, C) int64: the class counts (n_0 .. n_{C-1}) of ``arity`` sites, ascending in (n_1, n_2 ...)."""
    rest = [r for r in itertools.product(range(arity + 1), repeat=n_classes - 1) if sum(r) <= arity]
    return np.array([(arity - sum(r),) + r for r in sorted(rest)], dtype=np.int64).reshape(len(rest), n_classes)


def composition_census(set_cells, arity, n_classes):
    """See ``Patterns.composition_census``; ``set_cells`` (..., C**arity) are the cells of one set."""
    comp = compositions(arity, n_classes)
    index = {tuple(c): i for i, c in enumerate(comp.tolist())}
    cells = np.asarray(set_cells).astype(np.int64)
    if cells.shape[-1] != n_classes ** arity:
        raise ValueError(f"a set of arity {arity} with {n_classes} classes has {n_classes ** arity} cells, got {cells.shape[-1]}")
    out = np.zeros(cells.shape[:-1] + (len(comp),), dtype=np.int64)
    for v, digits in enumerate(itertools.product(range(n_classes), repeat=arity)):
        out[..., index[tuple(digits.count(k) for k in range(n_classes))]] += cells[..., v]
    return out, comp


def probabilities(cells, cell_ptr):
    """See ``Patterns.probabilities`` (a function of the arrays alone: a restored container has no more)."""
    c = np.asarray(cells).astype(np.float64)
    out = np.empty_like(c)
    with np.errstate(invalid="ignore", divide="ignore"):
        for a, b in zip(cell_ptr[:-1], cell_ptr[1:]):
            out[..., a:b] = c[..., a:b] / c[..., a:b].sum(axis=-1, keepdims=True)
    return out
