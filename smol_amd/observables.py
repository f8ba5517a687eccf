"""Observables of sampled states: species ("kind") counts and pair counts per bond shell.

This module is the DEFINITION: ``Observables.evaluate`` in NumPy is what the device kernel (csrc/observables.hip,
``smolmc_eval_observables`` and the ``SMOLMC_SAMPLE_OBSERVABLES`` columns of the sample ring) matches entry for entry.
Both vectors are int32, so the order of summation is no concern.

The *kind* of (site, code) is ``kind_base[site] + code``: codes of different sublattices -- or of site classes the user
chooses, e.g. the sublattices of an ordered structure -- go to different kinds; ``kind_base[site] = -1`` leaves a site out.

    counts[K]               how many counted sites hold each kind
    pairs[n_shells][K][K]   for each bond list ("shell") and each bond (i, j) AS GIVEN, cell (kind(i), kind(j)) gains 1;
                            a bond with an end that is not counted is skipped; duplicate rows and i == j rows of an aliased
                            cell count as they stand (the reference keeps duplicate clusters); the host symmetrises where
                            it wants unordered pairs.
"""

from __future__ import annotations

import numpy as np

MAX_OBS_CELLS = 4096  # SMOLMC_MAX_OBS_CELLS
MAX_KINDS = 254       # a kind is staged as one byte on the device, 0xff marks a site that is not counted


class Observables:
    """Kinds and bond shells of one supercell.

    kind_base    (N,) integers, -1 = the site is not counted
    n_kinds      K
    shells       sequence of (nbonds, 2) integer arrays of site pairs
    site_ncodes  optional (N,): species codes each site can hold; with it every kind is checked to stay below K (the
                 engine checks the same against its own tables) and ``pair_correlations`` knows the code of a kind
    """

    def __init__(self, kind_base, n_kinds, shells=(), site_ncodes=None, default_kinds=False, shell_orbit_ids=None):
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
        self.shells = []
        for s, b in enumerate(shells):
            b = np.asarray(b)
            if b.size == 0:
                b = np.zeros((0, 2), dtype=np.int32)
            if b.ndim != 2 or b.shape[1] != 2 or not np.issubdtype(b.dtype, np.integer):
                raise ValueError(f"shell {s}: bonds must be an (nbonds, 2) integer array")
            if b.min(initial=0) < 0 or b.max(initial=0) >= N:
                raise ValueError(f"shell {s}: bond out of range ({N} sites)")
            self.shells.append(np.ascontiguousarray(b, dtype=np.int32))
        self.n_shells = len(self.shells)
        if self.n_shells * K * K > MAX_OBS_CELLS:
            raise ValueError(f"{self.n_shells} shells x {K} x {K} kinds = {self.n_shells * K * K} cells, larger than "
                             f"MAX_OBS_CELLS = {MAX_OBS_CELLS}")
        self.site_ncodes = None
        self.kind_code = None  # (K,) the species code a kind stands for, -1: no site has it
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
            code = np.full(K, -1, dtype=np.int64)
            for base, n in {(int(b), int(n)) for b, n in zip(self.kind_base[counted], nc[counted])}:
                want = np.arange(n)
                have = code[base:base + n]
                if np.any((have >= 0) & (have != want)):
                    code = None  # (overlapping blocks: a kind stands for two codes)
                    break
                code[base:base + n] = want
            self.kind_code = code
        self.default_kinds = bool(default_kinds)
        self.shell_orbit_ids = None if shell_orbit_ids is None else [int(i) for i in shell_orbit_ids]

    # ---- constructors -------------------------------------------------------------------------------------------
    @classmethod
    def from_bonds(cls, kind_base, n_kinds, shells=(), site_ncodes=None):
        """Explicit arrays (mson / bridge models)."""
        return cls(kind_base, n_kinds, shells, site_ncodes=site_ncodes)

    @staticmethod
    def default_kind_base(sc):
        """(kind_base (N,), n_kinds, site_ncodes (N,)) of the default kinds of a synth supercell: one block per
        sublattice -- the basis sites of one symmetry label, as ``Processor.get_sublattices`` merges them -- in its
        encoding order, fixed (single-species) sublattices included."""
        prim = sc.model.prim
        base_of, K = {}, 0
        for b in range(prim.nb):
            if prim.labels[b] not in base_of:
                base_of[prim.labels[b]] = K
                K += int(prim.nspecies[b])
        kind_base = np.array([base_of[prim.labels[b]] for b in sc.site_b], dtype=np.int32)
        ncodes = np.array([prim.nspecies[b] for b in sc.site_b], dtype=np.int32)
        return kind_base, K, ncodes

    @classmethod
    def from_supercell(cls, sc, tables=None, orbits=None, site_classes=None):
        """Default kinds and the bond lists of the pair orbits of ``sc`` (``orbit.size == 2``; ``sc.full_indices`` row
        for row).  ``orbits``: restrict the shells to these orbit ids.  Shells beyond the expansion's cutoff: pass the
        supercell of a second ``synth.build_cluster_model`` with a larger pair cutoff on the same prim.
        ``site_classes`` (N,) integers: sites of different classes get different kind blocks even on one sublattice
        (the sublattices of an ordered structure: the counts are then its long-range order parameter).  ``tables``
        (a ``capi.TableSet``) is checked for the same number of sites."""
        if tables is not None and tables.struct.num_sites != sc.num_sites:
            raise ValueError("tables and supercell have different numbers of sites")
        kind_base, K, ncodes = cls.default_kind_base(sc)
        default = site_classes is None
        if site_classes is not None:
            classes = np.asarray(site_classes)
            if classes.shape != (sc.num_sites,):
                raise ValueError("site_classes must hold one entry per site")
            sublattice, base_of, K = kind_base, {}, 0
            kind_base = np.empty(sc.num_sites, dtype=np.int32)
            for s in range(sc.num_sites):  # one block per (sublattice, class), in the order of first appearance
                key = (int(sublattice[s]), int(classes[s]))
                if key not in base_of:
                    base_of[key] = K
                    K += int(ncodes[s])
                kind_base[s] = base_of[key]
        shells, ids = [], []
        for orb, rows in zip(sc.model.orbits, sc.full_indices):
            if orb.size == 2 and (orbits is None or orb.id in orbits):
                shells.append(np.asarray(rows, dtype=np.int32))
                ids.append(orb.id)
        return cls(kind_base, K, shells, site_ncodes=ncodes, default_kinds=default, shell_orbit_ids=ids)

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

    def evaluate(self, occupancies):
        """(counts (..., K) int32, pairs (..., n_shells, K, K) int32) of occupancies (..., N)."""
        kinds = self.kinds_of(occupancies)
        lead = kinds.shape[:-1]
        kinds = kinds.reshape(-1, self.num_sites)
        n, K = len(kinds), self.n_kinds
        row = np.arange(n, dtype=np.int64)[:, None]
        ok = kinds >= 0
        counts = np.bincount((row * K + kinds)[ok], minlength=n * K).reshape(n, K)
        pairs = np.zeros((n, self.n_shells, K, K), dtype=np.int64)
        for s, bonds in enumerate(self.shells):
            ka, kb = kinds[:, bonds[:, 0]], kinds[:, bonds[:, 1]]
            ok = (ka >= 0) & (kb >= 0)
            pairs[:, s] = np.bincount((row * (K * K) + ka * K + kb)[ok], minlength=n * K * K).reshape(n, K, K)
        return (counts.astype(np.int32).reshape(lead + (K,)),
                pairs.astype(np.int32).reshape(lead + (self.n_shells, K, K)))

    # ---- the C struct ------------------------------------------------------------------------------------------
    def c_struct(self):
        """(capi.smolmc_observables, the arrays it points at -- keep them alive during the call)."""
        import ctypes as C

        from . import capi

        ptr = np.concatenate(([0], np.cumsum([len(b) for b in self.shells]))).astype(np.int64)
        bonds = (np.concatenate(self.shells) if self.shells else np.zeros((0, 2), np.int32)).astype(np.int32)
        bonds = np.ascontiguousarray(bonds)
        s = capi.smolmc_observables()
        s.n_kinds, s.n_shells = self.n_kinds, self.n_shells
        s.kind_base = self.kind_base.ctypes.data_as(C.POINTER(C.c_int32))
        s.shell_ptr = ptr.ctypes.data_as(C.POINTER(C.c_int64))
        s.bonds = bonds.ctypes.data_as(C.POINTER(C.c_int32))
        return s, (self.kind_base, ptr, bonds)

    # ---- what a container keeps of the spec ------------------------------------------------------------------------
    def describe(self):
        """The kinds of the species_counts / pair_counts traces (plain lists: it goes into a container's metadata)."""
        return dict(n_kinds=self.n_kinds, n_shells=self.n_shells, default_kinds=self.default_kinds,
                    kind_base=self.kind_base.tolist(), site_ncodes=self.site_ncodes.tolist())

    @staticmethod
    def metadata_to_npz(obs):
        """The meta/* arrays of an .npz for the dict of ``describe``."""
        return {"meta/obs_kind_base": np.asarray(obs["kind_base"], dtype=np.int32),
                "meta/obs_site_ncodes": np.asarray(obs["site_ncodes"], dtype=np.int32),
                "meta/obs_shape": np.asarray([obs["n_kinds"], obs["n_shells"], int(obs["default_kinds"])], dtype=np.int64)}

    @staticmethod
    def metadata_from_npz(d):
        """The dict of ``describe`` from the arrays of ``metadata_to_npz``, None when ``d`` holds none."""
        if "meta/obs_kind_base" not in d.files:
            return None
        K, S, default = (int(x) for x in d["meta/obs_shape"])
        return dict(n_kinds=K, n_shells=S, default_kinds=bool(default), kind_base=d["meta/obs_kind_base"].tolist(),
                    site_ncodes=d["meta/obs_site_ncodes"].tolist())

    # ---- derived quantities (host) ---------------------------------------------------------------------------------
    def species_counts(self, counts, sites):
        """The slice of ``counts`` (..., K) that belongs to the sites ``sites`` -- a sublattice -- in code order, or None
        when those sites do not share one kind block of their own (then the counts cannot be read from the vector)."""
        return block_counts(self.kind_base, self.site_ncodes, counts, sites)

    pair_probabilities = staticmethod(lambda pairs: pair_probabilities(pairs))
    warren_cowley = staticmethod(lambda counts, pairs: warren_cowley(counts, pairs))

    def pair_correlations(self, pairs, orbit, shell=None):
        """Contract one shell's cells with the pair orbit's ``flat_correlation_tensors``: (..., K_orbit) -- the SUM over
        the shell's bonds of every correlation function of the orbit; divided by the number of bonds it is the
        orbit's slice of the correlation vector.  ``pairs`` (..., n_shells, K, K); ``shell`` defaults to the shell
        built from that orbit (``from_supercell``)."""
        if self.kind_code is None:
            raise ValueError("pair_correlations needs site_ncodes, and kinds that stand for one species code each")
        if shell is None:
            if self.shell_orbit_ids is None or orbit.id not in self.shell_orbit_ids:
                raise ValueError(f"no shell was built from orbit {orbit.id}: pass shell=")
            shell = self.shell_orbit_ids.index(orbit.id)
        ct = np.asarray(orbit.flat_correlation_tensors)  # (K_orbit, S0 * S1)
        stride = int(orbit.flat_tensor_indices[0])
        cells = np.asarray(pairs)[..., shell, :, :]
        code = self.kind_code
        used = np.argwhere(np.any(cells.reshape(-1, self.n_kinds, self.n_kinds) != 0, axis=0))
        out = np.zeros(cells.shape[:-2] + (ct.shape[0],))
        for a, b in used:
            out += cells[..., a, b, None] * ct[:, code[a] * stride + code[b]]
        return out


def block_counts(kind_base, site_ncodes, counts, sites):
    """See ``Observables.species_counts`` (a function of the arrays alone: a restored container has no more)."""
    kind_base = np.asarray(kind_base)
    sites = np.asarray(sites, dtype=np.int64)
    if len(sites) == 0:
        return None
    base = int(kind_base[sites[0]])
    if base < 0 or np.any(kind_base[sites] != base):
        return None
    n = int(np.asarray(site_ncodes)[sites].max()) if site_ncodes is not None else None
    others = np.ones(len(kind_base), dtype=bool)
    others[sites] = False
    ob = kind_base[others]
    if n is None:
        later = ob[ob > base]
        n = int(later.min() - base) if len(later) else np.asarray(counts).shape[-1] - base
    if site_ncodes is not None:
        on = np.asarray(site_ncodes)[others]
        if np.any((ob >= 0) & (ob < base + n) & (ob + on > base)):
            return None  # (another site's kinds reach into this block)
    elif np.any(ob == base):
        return None
    return np.asarray(counts)[..., base:base + n]


def _symmetrised(pairs):
    p = np.asarray(pairs).astype(np.int64)
    return p + np.swapaxes(p, -1, -2)


def pair_probabilities(pairs):
    """P_s(a, b) of unordered pairs: the symmetrised cells of every shell over their sum, (..., n_shells, K, K)."""
    sym = _symmetrised(pairs).astype(np.float64)
    tot = sym.sum(axis=(-1, -2), keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        return sym / tot


def warren_cowley(counts, pairs):
    """Warren-Cowley short-range order alpha_ab(s) = 1 - P_s(b | a) / c_b, (..., n_shells, K, K), from the symmetrised
    pairs: P_s(b | a) = sym[s][a][b] / sum_b' sym[s][a][b'], c_b = counts[b] / sum(counts).  Evaluated as one quotient of
    integers, (D - X) / D with X = sym[a][b] sum(counts) and D = (sum_b' sym[a][b']) counts[b], so that a rational
    value comes out as its nearest double.  NaN where kind a has no bond in the shell or kind b no site."""
    sym = _symmetrised(pairs)
    c = np.asarray(counts).astype(np.int64)
    X = sym * c.sum(axis=-1)[..., None, None, None]
    D = sym.sum(axis=-1, keepdims=True) * c[..., None, None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(D != 0, (D - X) / np.where(D != 0, D, 1), np.nan)
