"""Structure factors of sampled states: fixed-point amplitudes per wave vector and kind, and intensities made of them.

This module is the DEFINITION: ``StructureFactor.evaluate`` in NumPy is what the device kernel (csrc/structure.hip,
``smolmc_eval_structure`` and the ``SMOLMC_SAMPLE_STRUCTURE`` columns of the sample ring) matches entry for entry.

The *kind* of (site, code) is ``kind_base[site] + code`` as in ``observables.Observables``; ``kind_base[site] = -1`` leaves
the site out.  For every wave vector ("point") q each site j has a *phase class* ``phase[q][j] < M`` and every class a
fixed-point pair ``table[q][m] = (cos, -sin)`` of its phase angle, int64.  Per occupancy row

    amp[q][k][c] = sum over counted sites j with kind(j) == k of table[q][phase[q][j]][c]            (int64, c = 0, 1)
    inten[i]     = ((double)amp[q][a][0] * (double)amp[q][b][0] + (double)amp[q][a][1] * (double)amp[q][b][1]) * scale[i]
                   for intensity i = (q, a, b)

The sums are integer sums: their order is of no concern, so host and device agree bit for bit.  Every floating product
and sum of ``inten`` is rounded on its own (no fused multiply-add).  The engine knows no geometry: the caller supplies
``phase`` and ``table``, as it supplies the observables' bond lists; ``StructureFactor.from_supercell`` makes them for a
``synth`` or ``mson`` supercell.

Geometry (``from_supercell``).  The rows of ``S = scmatrix`` are the supercell vectors in units of the primitive ones.  A
wave vector commensurate with the supercell is ``k = S^-1 g`` with an integer triple g, in the primitive reciprocal
basis: ``k . n = n . S^-1 . g`` for a lattice point n.  With ``adj(S) = det(S) S^-1`` (integer) the lattice part of the
phase is exact: ``k . n = m / |det S|  (mod 1)`` with ``m = sign(det S) (n . adj(S) . g) mod |det S|``.  The basis offset
``k . tau_b`` is a float; it is folded in by giving each distinct (m, basis site) pair of a point a phase class of its
own with angle ``theta = 2 pi (m / |det S| + k . tau_b)`` and ``table = rint(cos(theta) 2^bits), rint(-sin(theta) 2^bits)``.
So A_k(q) = sum_j exp(-i k . r_j) = (amp[q][k][0] + i amp[q][k][1]) 2^-bits up to the rounding of the table.

Error of the fixed point.  Each table entry is off by at most half a unit, 2^-(bits + 1) after scaling, in the real and
in the imaginary part alike, so every term of the sum is off by at most 2^-(bits + 1) sqrt(2) in modulus and

    |A_fixed - A_exact| <= n_kind 2^-(bits + 1) sqrt(2)

for a kind held by n_kind sites (plus the error of cos and sin themselves, a few units of 2^-53 per term).  With
``bits = 36`` an amplitude of up to 65535 sites is below 2^52 in either part and converts to double exactly.
"""

from __future__ import annotations

import itertools

import numpy as np

from .observables import MAX_KINDS, Observables

MAX_POINTS = 4096        # SMOLMC_MAX_STRUCT_POINTS
MAX_PHASES = 65535       # SMOLMC_MAX_STRUCT_PHASES (a phase class is a uint16)
MAX_CELLS = 12288        # SMOLMC_MAX_STRUCT_CELLS: n_kinds x n_phases, the (kind, phase class) counters of one point
MAX_INTENSITIES = 4096   # SMOLMC_MAX_STRUCT_INTENSITIES


def _adjugate(S):
    """Integer adjugate of a 3 x 3 integer matrix: S @ adj = det(S) I."""
    S = [[int(x) for x in row] for row in np.asarray(S)]
    r0, r1, r2 = S

    def cross(a, b):
        return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]

    cols = [cross(r1, r2), cross(r2, r0), cross(r0, r1)]
    adj = np.array(cols, dtype=np.int64).T
    det = sum(r0[i] * cols[0][i] for i in range(3))
    return adj, int(det)


def lattice_points_of(sc):
    """(P, 3) int64 lattice points of a supercell in units of the primitive vectors (``synth`` keeps them so, ``mson``
    keeps pymatgen's fractional coordinates of the supercell)."""
    pts = np.asarray(sc.lattice_points)
    if np.issubdtype(pts.dtype, np.integer):
        return pts.astype(np.int64)
    n = pts @ np.asarray(sc.scmatrix, dtype=np.float64)
    if np.abs(n - np.rint(n)).max(initial=0.0) > 1e-6:
        raise ValueError("the supercell's lattice points are no integer combinations of the primitive vectors")
    return np.rint(n).astype(np.int64)


def commensurate_points(sc):
    """The ``|det S|`` integer triples g, one per class of wave vectors ``k = S^-1 g`` modulo reciprocal lattice
    vectors: g is taken modulo the lattice spanned by the columns of S.  Gamma (g = 0) comes first."""
    S = np.asarray(sc.scmatrix, dtype=np.int64)
    adjT, det = _adjugate(S.T)
    sgn = 1 if det > 0 else -1
    corners = np.array(list(itertools.product((0, 1), repeat=3)), dtype=np.int64) @ S.T
    lo, hi = corners.min(axis=0), corners.max(axis=0)
    grid = np.array(list(itertools.product(*[range(int(a), int(b) + 1) for a, b in zip(lo, hi)])), dtype=np.int64)
    f = sgn * (grid @ adjT)  # = |det| x the coordinates of g in the basis of the columns of S
    pts = grid[np.all((f >= 0) & (f < abs(det)), axis=1)]
    if len(pts) != abs(det):
        raise RuntimeError("enumeration of the commensurate wave vectors failed for this supercell matrix")
    return pts[np.lexsort((pts[:, 2], pts[:, 1], pts[:, 0]))]


class StructureFactor:
    """Kinds, phase classes and intensities of one supercell.

    kind_base        (N,) integers, -1 = the site is not counted
    n_kinds          K
    phase            (Q, N) integers < M: the phase class of every site for every point
    table            (Q, M, 2) integers: fixed-point (cos, -sin) of every phase class
    intensities      (I, 3) integers (point, kind a, kind b)
    intensity_scale  (I,) floats or one float; default 2^(-2 bits) / N_counted when ``bits`` is given, else 1 / N_counted
    site_ncodes      optional (N,): species codes each site can hold; with it every kind is checked to stay below K
    """

    def __init__(self, kind_base, n_kinds, phase, table, intensities=(), intensity_scale=None, site_ncodes=None, bits=None):
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
        ph, tb = np.asarray(phase), np.asarray(table)
        if ph.ndim != 2 or ph.shape[1] != N or not np.issubdtype(ph.dtype, np.integer):
            raise ValueError(f"phase must be a (n_points, {N}) integer array")
        if tb.ndim != 3 or tb.shape[0] != ph.shape[0] or tb.shape[2] != 2 or not np.issubdtype(tb.dtype, np.integer):
            raise ValueError("table must be a (n_points, n_phases, 2) integer array")
        self.n_points, self.n_phases = Q, M = int(tb.shape[0]), int(tb.shape[1])
        if not 1 <= Q <= MAX_POINTS:
            raise ValueError(f"n_points must be 1..{MAX_POINTS}, got {Q}")
        if not 1 <= M <= MAX_PHASES:
            raise ValueError(f"n_phases must be 1..{MAX_PHASES}, got {M}")
        if K * M > MAX_CELLS:
            raise ValueError(f"{K} kinds x {M} phase classes = {K * M} cells, larger than MAX_CELLS = {MAX_CELLS}")
        if ph.min(initial=0) < 0 or ph.max(initial=0) >= M:
            bad = int(ph.max(initial=0)) if ph.max(initial=0) >= M else int(ph.min(initial=0))
            raise ValueError(f"phase holds {bad}, n_phases is {M}: phase out of range")
        self.phase = np.ascontiguousarray(ph, dtype=np.uint16)
        self.table = np.ascontiguousarray(tb, dtype=np.int64)
        self.n_counted = int((self.kind_base >= 0).sum())
        peak = max(abs(int(self.table.max(initial=0))), abs(int(self.table.min(initial=0))))
        if self.n_counted * peak >= 1 << 62:
            raise ValueError(f"{self.n_counted} counted sites x max|table| = {peak} reaches 2^62: an amplitude could overflow")
        it = np.asarray(intensities, dtype=np.int64).reshape(-1, 3)
        self.n_intensities = I = len(it)
        if I > MAX_INTENSITIES:
            raise ValueError(f"n_intensities must be 0..{MAX_INTENSITIES}, got {I}")
        for i, (q, a, b) in enumerate(it):
            if not 0 <= q < Q:
                raise ValueError(f"intensity {i} names point {int(q)}, n_points is {Q}: point out of range")
            if not (0 <= a < K and 0 <= b < K):
                raise ValueError(f"intensity {i} names kinds ({int(a)}, {int(b)}), n_kinds is {K}: kind out of range")
        self.intensity = np.ascontiguousarray(it, dtype=np.int32)
        self.bits = None if bits is None else int(bits)
        if intensity_scale is None:
            unit = 1.0 if bits is None else 2.0 ** (-2 * self.bits)
            intensity_scale = unit / max(self.n_counted, 1)
        sc = np.ascontiguousarray(np.broadcast_to(np.asarray(intensity_scale, dtype=np.float64), (I,)))
        if not np.all(np.isfinite(sc)):
            raise ValueError("intensity_scale must be finite")
        self.intensity_scale = sc
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
        # geometry, when from_supercell made the arrays (the inverse transform needs it)
        self.points = None      # (Q, 3) int64 g
        self.scmatrix = None

    # ---- constructors -------------------------------------------------------------------------------------------
    @classmethod
    def from_supercell(cls, sc, points, site_classes=None, observables=None, intensities=None, bits=36):
        """Phase classes and tables of the wave vectors ``points`` on a ``synth`` or ``mson`` supercell.

        ``points``: an INTEGER array of triples g (``k = S^-1 g``, any integer g), or a FLOAT array of wave vectors k in
        the primitive reciprocal basis, checked to be commensurate (``S k`` integer to 1e-9).  Kinds: the default kinds
        of ``Observables.default_kind_base(sc)``, split by ``site_classes`` as ``Observables.from_supercell`` does, or
        those of ``observables``.  ``intensities``: (point, kind a, kind b) triples; default: none."""
        S = np.asarray(sc.scmatrix, dtype=np.int64)
        adj, det = _adjugate(S)
        if det == 0:
            raise ValueError("singular supercell matrix")
        pts = np.asarray(points)
        if pts.ndim != 2 or pts.shape[1] != 3 or len(pts) == 0:
            raise ValueError("points must be a non-empty (n_points, 3) array")
        if np.issubdtype(pts.dtype, np.integer):
            g = pts.astype(np.int64)
        else:
            gf = pts.astype(np.float64) @ S.T.astype(np.float64)  # S k
            if np.abs(gf - np.rint(gf)).max() > 1e-9:
                q = int(np.argmax(np.abs(gf - np.rint(gf)).max(axis=1)))
                raise ValueError(f"point {q} = {pts[q].tolist()} is not commensurate with the supercell (S k is not integer)")
            g = np.rint(gf).astype(np.int64)
        if observables is not None:
            if site_classes is not None:
                raise ValueError("give site_classes or observables, not both")
            kind_base, K, ncodes = observables.kind_base, observables.n_kinds, observables.site_ncodes
        else:
            kind_base, K, ncodes = Observables.default_kind_base(sc)
            if site_classes is not None:  # one block per (sublattice, class), as Observables.from_supercell numbers them
                classes = np.asarray(site_classes)
                if classes.shape != (sc.num_sites,):
                    raise ValueError("site_classes must hold one entry per site")
                sublattice, base_of, K = kind_base, {}, 0
                kind_base = np.empty(sc.num_sites, dtype=np.int32)
                for s in range(sc.num_sites):
                    key = (int(sublattice[s]), int(classes[s]))
                    if key not in base_of:
                        base_of[key] = K
                        K += int(ncodes[s])
                    kind_base[s] = base_of[key]
        n = lattice_points_of(sc)
        P, N = len(n), int(sc.num_sites)
        site_b = np.asarray(sc.site_b, dtype=np.int64)
        site_t = np.asarray(getattr(sc, "site_t", np.arange(N) % P), dtype=np.int64)
        tau = np.asarray(sc.model.prim.frac_coords, dtype=np.float64)
        nb, D, sgn = len(tau), abs(det), (1 if det > 0 else -1)
        Q = len(g)
        phase = np.zeros((Q, N), dtype=np.int64)
        tables = []
        for q in range(Q):
            ag = adj @ g[q]                             # det x k, integer
            m = (sgn * (n @ ag)) % D                    # (P,) the lattice part, exact
            off = tau @ (ag.astype(np.float64) / det)   # (nb,) k . tau_b
            key = m[site_t] * nb + site_b
            classes, inv = np.unique(key, return_inverse=True)
            phase[q] = inv.reshape(-1)
            t = (classes // nb) / D + off[classes % nb]
            theta = 2.0 * np.pi * (t - np.floor(t))
            tables.append(np.stack([np.rint(np.cos(theta) * 2.0 ** bits), np.rint(-np.sin(theta) * 2.0 ** bits)], axis=1))
        M = max(len(t) for t in tables)
        table = np.zeros((Q, M, 2), dtype=np.int64)
        for q, t in enumerate(tables):
            table[q, :len(t)] = t.astype(np.int64)
        sf = cls(kind_base, K, phase, table, () if intensities is None else intensities, site_ncodes=ncodes, bits=bits)
        sf.points, sf.scmatrix = g, S
        return sf

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
        """(amp (..., Q, K, 2) int64, inten (..., I) float64) of occupancies (..., N)."""
        kinds = self.kinds_of(occupancies)
        lead = kinds.shape[:-1]
        kinds = kinds.reshape(-1, self.num_sites)
        n, Q, K, M = len(kinds), self.n_points, self.n_kinds, self.n_phases
        ok = kinds >= 0
        row = (np.arange(n, dtype=np.int64)[:, None] * (K * M) + kinds * M)[ok]
        amp = np.empty((n, Q, K, 2), dtype=np.int64)
        for q in range(Q):
            # sites per (kind, phase class) cell, then the integer sum over the classes: the same sum in another order
            ph = np.broadcast_to(self.phase[q].astype(np.int64), kinds.shape)[ok]
            cells = np.bincount(row + ph, minlength=n * K * M).reshape(n, K, M)
            amp[:, q] = cells @ self.table[q]
        inten = self.intensities_of(amp)
        return amp.reshape(lead + (Q, K, 2)), inten.reshape(lead + (self.n_intensities,))

    def intensities_of(self, amp):
        """inten (..., I) of amp (..., Q, K, 2): every product and sum rounded on its own."""
        amp = np.asarray(amp)
        q, a, b = self.intensity[:, 0], self.intensity[:, 1], self.intensity[:, 2]
        A, B = amp[..., q, a, :].astype(np.float64), amp[..., q, b, :].astype(np.float64)
        re = A[..., 0] * B[..., 0]
        im = A[..., 1] * B[..., 1]
        return (re + im) * self.intensity_scale

    # ---- the C struct ------------------------------------------------------------------------------------------
    def c_struct(self):
        """(capi.smolmc_structure, the arrays it points at -- keep them alive during the call)."""
        import ctypes as C

        from . import capi

        s = capi.smolmc_structure()
        s.n_kinds, s.n_points, s.n_phases, s.n_intensities = self.n_kinds, self.n_points, self.n_phases, self.n_intensities
        s.kind_base = self.kind_base.ctypes.data_as(C.POINTER(C.c_int32))
        s.phase = self.phase.ctypes.data_as(C.POINTER(C.c_uint16))
        s.table = self.table.ctypes.data_as(C.POINTER(C.c_int64))
        s.intensity = self.intensity.ctypes.data_as(C.POINTER(C.c_int32))
        s.intensity_scale = self.intensity_scale.ctypes.data_as(C.POINTER(C.c_double))
        return s, (self.kind_base, self.phase, self.table, self.intensity, self.intensity_scale)

    def describe(self):
        """What a container keeps of the spec: the shape of the two traces, what the intensities are and their scale."""
        return dict(n_points=self.n_points, n_kinds=self.n_kinds, n_intensities=self.n_intensities, bits=self.bits,
                    intensities=self.intensity.tolist(), intensity_scale=self.intensity_scale.tolist(),
                    points=None if self.points is None else self.points.tolist())

    # ---- derived quantities (host) ---------------------------------------------------------------------------------
    def amplitudes(self, amp):
        """A_k(q) = sum_j exp(-i k . r_j) as complex128 (..., Q, K): ``amp 2^-bits``."""
        if self.bits is None:
            raise ValueError("the fixed-point scale is unknown: build the object with bits=")
        amp = np.asarray(amp)
        return (amp[..., 0].astype(np.float64) + 1j * amp[..., 1].astype(np.float64)) * 2.0 ** -self.bits

    def partial_structure_factors(self, amp):
        """S_ab(q) = Re(A_a(q) A_b(q)*) / N_counted, (..., Q, K, K)."""
        A = self.amplitudes(amp)
        return (A[..., :, None] * np.conj(A[..., None, :])).real / max(self.n_counted, 1)

    def pair_counts_from_amplitudes(self, amp, displacements):
        """The inverse transform: (..., n_displacements, K, K) floats, entry (d, a, b) the number of ordered pairs
        (i of kind a, j of kind b) with ``r_j - r_i = d`` modulo the supercell, d an integer lattice vector:

            n_ab(d) = (1 / P) sum_q Re(A_a(q)* A_b(q) exp(i k_q . d))

        It needs the amplitudes at ALL ``|det S|`` classes of wave vectors (``commensurate_points``) and a cell with
        one basis site per counted sublattice offset (every r_j - r_i must be a lattice vector)."""
        if self.points is None:
            raise ValueError("the inverse transform needs the geometry: build the object with from_supercell")
        adj, det = _adjugate(self.scmatrix)
        D = abs(det)
        if self.n_points != D:
            raise ValueError(f"the inverse transform needs all {D} classes of wave vectors, the object has {self.n_points}")
        d = np.asarray(displacements, dtype=np.int64).reshape(-1, 3)
        sgn = 1 if det > 0 else -1
        m = (sgn * (d @ adj @ self.points.T)) % D            # (nd, Q): k_q . d = m / D mod 1
        w = np.exp(2j * np.pi * m / D)
        A = self.amplitudes(amp)                              # (..., Q, K)
        corr = np.conj(A)[..., :, :, None] * A[..., :, None, :]   # (..., Q, K, K)
        return np.einsum("dq,...qab->...dab", w, corr).real / D


def amplitudes(amp, bits=36):
    """complex128 ``amp 2^-bits`` of amp (..., 2) int64."""
    amp = np.asarray(amp)
    return (amp[..., 0].astype(np.float64) + 1j * amp[..., 1].astype(np.float64)) * 2.0 ** -bits
