"""The lowest recorded states, per walker or per composition.

This module is the DEFINITION: ``MinimaRecord.offer`` in NumPy is what the device reduction (csrc/minima.hip,
``SMOLMC_SAMPLE_MINIMA`` and ``smolmc_update_minima``) matches entry for entry.

A *minima record* is a table of ``n_slots`` entries.  Every recorded sample is offered to the entry its key selects:

    per walker        n_slots = R, the key is the walker index
    per composition   on axis a: d_a = sum_k axis_weights[a][k] * counts[k] (int64), c_a = d_a // bins[a] (floor); the
                      row is skipped unless 0 <= c_a < extents[a] on every axis; the key is the mixed-radix number of
                      the c_a, axis 0 slowest; n_slots = prod(extents)

The value that is minimised is the enthalpy column, or ``sum_i weights[i] * features[i]`` taken left to right with every
product and sum rounded on its own (``acc = acc + w[i] * f[..., i]``).  Values are canonicalised with ``v + 0.0``; a NaN
never wins.  Offers are numbered from 0 since the last reset.  A strictly lower value replaces the entry; among equal
values the earliest offer wins, within one offer the lowest walker -- the order of ``argmin`` over the sample-major flat
view of the container.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

MAX_AXES = 4          # SMOLMC_MAX_MINIMA_AXES
MAX_SLOTS = 1 << 20

_FIELDS = ("value", "enthalpy", "features", "occupancy", "counts", "walker", "sample", "step")


def ordered_bits(x):
    """uint64 keys that order the way the doubles ``x`` do (the kernel's mapping): sign bit set gives ``~bits``, else
    ``bits | 1 << 63``.  Canonicalise -0.0 first (``x + 0.0``) where the two zeros must be one key."""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    top = np.uint64(1) << np.uint64(63)
    return np.where(b >> np.uint64(63) != 0, ~b, b | top)


def weighted_value(weights, features):
    """``sum_i weights[i] * features[..., i]`` left to right, each product and sum rounded on its own."""
    f = np.asarray(features, dtype=np.float64)
    acc = np.zeros(f.shape[:-1])
    for i, w in enumerate(np.asarray(weights, dtype=np.float64)):
        acc = acc + w * f[..., i]
    return acc


class Minima:
    """The spec of a record: what is minimised (``weights`` over the features, None: the enthalpy) and how it is keyed
    (``axis_weights`` (n_axes, K) with ``bins`` and ``extents``; none: one slot per walker)."""

    def __init__(self, weights=None, axis_weights=None, bins=None, extents=None):
        self.weights = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        if axis_weights is None:
            self.axis_weights = np.zeros((0, 0), dtype=np.int32)
            self.bins = self.extents = np.zeros(0, dtype=np.int32)
        else:
            aw = np.asarray(axis_weights)
            if aw.ndim != 2 or not np.issubdtype(aw.dtype, np.integer):
                raise ValueError("axis_weights must be an (n_axes, K) integer array")
            if not 1 <= len(aw) <= MAX_AXES:
                raise ValueError(f"a record keyed by composition has 1..{MAX_AXES} axes, got {len(aw)}")
            self.axis_weights = np.ascontiguousarray(aw, dtype=np.int32)
            self.bins = np.ascontiguousarray(np.ones(len(aw)) if bins is None else bins, dtype=np.int32).reshape(-1)
            self.extents = np.ascontiguousarray(extents, dtype=np.int32).reshape(-1)
            if len(self.bins) != len(aw) or len(self.extents) != len(aw):
                raise ValueError("one bin and one extent per axis")
            # (bins and extents below 1, too many slots: the engine refuses them, naming the reason)

    n_axes = property(lambda self: len(self.axis_weights))
    n_weights = property(lambda self: 0 if self.weights is None else len(self.weights))

    @classmethod
    def per_walker(cls, weights=None):
        return cls(weights=weights)

    @classmethod
    def by_composition(cls, observables, axes, bins=None, extents=None, weights=None):
        """Keyed by the kind counts of ``observables`` (an ``observables.Observables``, or its K): ``axes`` (n_axes, K)
        integer weights of the counts -- a single kind number stands for the axis that counts that kind."""
        K = int(getattr(observables, "n_kinds", observables))
        rows = []
        for a in ([axes] if isinstance(axes, (int, np.integer)) else axes):
            a = np.asarray(a)
            if a.ndim == 0:
                row = np.zeros(K, dtype=np.int64)
                row[int(a)] = 1
            else:
                row = np.asarray(a, dtype=np.int64)
            if row.shape != (K,):
                raise ValueError(f"an axis holds one integer weight per kind ({K}), got shape {row.shape}")
            rows.append(row)
        return cls(weights=weights, axis_weights=np.array(rows), bins=bins, extents=extents)

    @staticmethod
    def energy_weights(ensemble):
        """Natural parameters of the energy coefficients of an ensemble: with these the value of a record is what
        ``SampleContainer.get_energies`` gives, the enthalpy without the chemical work."""
        nat = np.asarray(ensemble.natural_parameters, dtype=np.float64)
        n = getattr(ensemble, "num_energy_coefs", len(nat))
        return np.ascontiguousarray(nat[:n])

    # ---- the definition ------------------------------------------------------------------------------------------
    def n_slots(self, n_walkers):
        return int(n_walkers) if self.n_axes == 0 else int(np.prod(self.extents.astype(np.int64)))

    def values(self, enthalpy, features):
        v = np.asarray(enthalpy, dtype=np.float64) if self.weights is None else weighted_value(self.weights, features)
        return v + 0.0

    def keys(self, counts, n_walkers, shape):
        """Slot of every row of ``shape`` (..., R); -1: the row is skipped."""
        if self.n_axes == 0:
            return np.broadcast_to(np.arange(n_walkers, dtype=np.int64), shape).copy()
        c = np.asarray(counts, dtype=np.int64).reshape(tuple(shape) + (-1,))
        key = np.zeros(shape, dtype=np.int64)
        ok = np.ones(shape, dtype=bool)
        for a in range(self.n_axes):
            d = (c * self.axis_weights[a].astype(np.int64)).sum(axis=-1)
            q = d // int(self.bins[a])
            ok &= (q >= 0) & (q < int(self.extents[a]))
            key = key * int(self.extents[a]) + q
        return np.where(ok, key, -1)

    def c_struct(self):
        """(capi.smolmc_minima, the arrays it points to)."""
        from . import capi

        f64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        keep = (self.weights, self.axis_weights, self.bins, self.extents)
        ptr = lambda a, t: a.ctypes.data_as(t) if a is not None and a.size else None
        s = capi.smolmc_minima(self.n_weights, ptr(self.weights, f64p), self.n_axes, ptr(self.axis_weights, i32p),
                               ptr(self.bins, i32p), ptr(self.extents, i32p))
        return s, keep

    def as_dict(self):
        return dict(weights=None if self.weights is None else self.weights.tolist(),
                    axis_weights=self.axis_weights.tolist(), bins=self.bins.tolist(), extents=self.extents.tolist())

    @classmethod
    def from_dict(cls, d):
        aw = d.get("axis_weights")
        return cls(d.get("weights"), aw if aw else None, d.get("bins") or None, d.get("extents") or None)


class MinimaRecord:
    """The entries of a record: value, enthalpy (n,), features (n, F), occupancy (n, N), counts (n, K), walker (n,),
    sample (n,) -- the offer number -- and step (n,).  An empty entry reads value +inf, walker -1, sample -1, zeros
    elsewhere."""

    def __init__(self, spec, n_walkers, n_features, n_sites, n_kinds=0):
        self.spec, self.n_walkers = spec, int(n_walkers)
        n = spec.n_slots(n_walkers)
        self.value = np.full(n, np.inf)
        self.enthalpy = np.zeros(n)
        self.features = np.zeros((n, int(n_features)))
        self.occupancy = np.zeros((n, int(n_sites)), dtype=np.int32)
        self.counts = np.zeros((n, int(n_kinds)), dtype=np.int32)
        self.walker = np.full(n, -1, dtype=np.int32)
        self.sample = np.full(n, -1, dtype=np.int64)
        self.step = np.zeros(n, dtype=np.uint64)
        # per walker: the companions of walker 0's entry, every walker's occupancy at the offer that entry was taken
        # from (what get_minimum_*_occupancy(flat=False) of the reference returns); None on a keyed record
        self.companions = np.zeros((n, int(n_sites)), dtype=np.int32) if spec.n_axes == 0 else None
        self.offers = 0

    n_slots = property(lambda self: len(self.value))

    def offer(self, enthalpy, features, occupancy, counts=None, steps=None):
        """Offer rows (ns, R) -- or one sample (R,) -- in order: each sample is one offer."""
        H = np.asarray(enthalpy, dtype=np.float64)
        H = H.reshape(-1, self.n_walkers)
        ns, R = H.shape
        feat = np.asarray(features, dtype=np.float64).reshape(ns, R, -1)
        occ = np.asarray(occupancy).reshape(ns, R, -1)
        K = self.counts.shape[1]
        cnt = None if counts is None or K == 0 else np.asarray(counts).reshape(ns, R, K)
        st = np.zeros((ns, R), dtype=np.uint64) if steps is None else np.asarray(steps, dtype=np.uint64).reshape(ns, R)
        v = self.spec.values(H, feat).reshape(-1)
        key = self.spec.keys(cnt, R, (ns, R)).reshape(-1)
        live = (key >= 0) & ~np.isnan(v)
        rows = np.flatnonzero(live)
        if len(rows):
            # the lowest value of every slot, then the lowest row that has it: a stable sort by (slot, value, row)
            order = rows[np.lexsort((rows, v[rows], key[rows]))]
            first = np.ones(len(order), dtype=bool)
            first[1:] = key[order[1:]] != key[order[:-1]]
            win = order[first]
            win = win[v[win] < self.value[key[win]]]
            slot = key[win]
            s, r = win // R, win % R
            self.value[slot] = v[win]
            self.enthalpy[slot] = H[s, r]
            self.features[slot] = feat[s, r]
            self.occupancy[slot] = occ[s, r]
            if cnt is not None:
                self.counts[slot] = cnt[s, r]
            self.walker[slot] = r
            self.sample[slot] = self.offers + s
            self.step[slot] = st[s, r]
            if self.companions is not None and (slot == 0).any():
                self.companions[:] = occ[s[slot == 0][0]]
        self.offers += ns
        return self

    @property
    def filled(self):
        return self.sample >= 0

    def best(self, n=1):
        """Slots of the ``n`` lowest filled entries, lowest first (ties: the lower slot)."""
        idx = np.flatnonzero(self.filled)
        return idx[np.argsort(self.value[idx], kind="stable")][:n]

    @classmethod
    def merge(cls, records):
        """One record from those of several ranks (or of consecutive parts of a run): lowest value, then rank order.
        Per walker the slots of the ranks are concatenated -- the walkers of a sharded sampler."""
        records = list(records)
        first = records[0]
        if first.spec.n_axes == 0:
            out = cls(first.spec, sum(r.n_walkers for r in records), first.features.shape[1], first.occupancy.shape[1],
                      first.counts.shape[1])
            for f in _FIELDS:
                setattr(out, f, np.concatenate([getattr(r, f) for r in records]))
            base = np.cumsum([0] + [r.n_walkers for r in records[:-1]])
            out.walker = np.concatenate([np.where(r.walker >= 0, r.walker + b, -1) for r, b in zip(records, base)]).astype(np.int32)
            out.offers = max(r.offers for r in records)
            # (the ranks' companions belong to their own walker 0: the merged record has none, unless there is one rank)
            out.companions = first.companions.copy() if len(records) == 1 and first.companions is not None else None
            return out
        out = first.copy()
        for r in records[1:]:
            take = r.value < out.value
            for f in _FIELDS:
                getattr(out, f)[take] = getattr(r, f)[take]
            out.offers = max(out.offers, r.offers)
        return out

    def copy(self):
        out = MinimaRecord.__new__(MinimaRecord)
        out.spec, out.n_walkers, out.offers = self.spec, self.n_walkers, self.offers
        for f in _FIELDS:
            setattr(out, f, getattr(self, f).copy())
        out.companions = None if self.companions is None else self.companions.copy()
        return out

    def as_dict(self):
        d = {f: getattr(self, f) for f in _FIELDS}
        d.update(offers=self.offers, n_walkers=self.n_walkers, spec=self.spec.as_dict(), companions=self.companions)
        return d

    @classmethod
    def from_dict(cls, d):
        out = cls.__new__(cls)
        out.spec, out.n_walkers, out.offers = Minima.from_dict(d["spec"]), int(d["n_walkers"]), int(d["offers"])
        dt = dict(occupancy=np.int32, counts=np.int32, walker=np.int32, sample=np.int64, step=np.uint64)
        for f in _FIELDS:
            setattr(out, f, np.array(d[f], dtype=dt.get(f, np.float64)))
        comp = d.get("companions")
        out.companions = None if comp is None else np.array(comp, dtype=np.int32)
        return out

    def equals(self, other):
        if (self.companions is None) != (other.companions is None):
            return False
        if self.companions is not None and not np.array_equal(self.companions, other.companions):
            return False
        return all(np.array_equal(getattr(self, f), getattr(other, f), equal_nan=f in ("enthalpy", "features"))
                   for f in _FIELDS)


def lower_hull(x, e):
    """Indices of the vertices of the lower convex hull of the points (x, e), by ascending x (Andrew's monotone chain;
    collinear points between two vertices are not vertices; of equal x the lowest e counts)."""
    x, e = np.asarray(x, dtype=np.float64), np.asarray(e, dtype=np.float64)
    order = np.lexsort((e, x))
    hull = []
    for i in order:
        if hull and x[hull[-1]] == x[i]:
            continue  # (same x, higher or equal e)
        while len(hull) >= 2:
            a, b = hull[-2], hull[-1]
            if (x[b] - x[a]) * (e[i] - e[a]) - (e[b] - e[a]) * (x[i] - x[a]) <= 0:
                hull.pop()
            else:
                break
        hull.append(int(i))
    return np.array(hull, dtype=np.int64)


def formation_energies(x, e):
    """``e`` minus the line through the end members (the points of lowest and highest ``x``)."""
    x, e = np.asarray(x, dtype=np.float64), np.asarray(e, dtype=np.float64)
    lo, hi = int(np.argmin(x)), int(np.argmax(x))
    if x[hi] == x[lo]:
        return e - e[lo]
    t = (x - x[lo]) / (x[hi] - x[lo])
    return e - ((1.0 - t) * e[lo] + t * e[hi])
