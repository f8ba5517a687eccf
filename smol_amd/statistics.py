"""Running moments, blocking sums and a histogram of the recorded samples, per walker, per state point or per bin of a
column.

This module is the DEFINITION: ``StatisticsRecord.offer`` in NumPy is what the device reduction (csrc/statistics.hip,
``SMOLMC_SAMPLE_STATISTICS`` and ``smolmc_update_statistics``) matches entry for entry.

A *statistics record* holds accumulators for ``n_keys = R`` keys.  One offer is one sample of all walkers; it gives each
key exactly one row of ``C`` column values ``x`` (the key of a row is its walker, or the state point the walker holds:
both are permutations), and the key's accumulators take the rows in order:

    if n == 0: shift[c] = x[c]                      the key's first offered value
    d[c] = x[c] - shift[c]
    s1[c] += d[c]
    s2[a,b] += d[a] * d[b]     for a <= b           upper triangle, row-major, C (C + 1) / 2 entries
    blocking (Flyvbjerg & Petersen 1989), per column c, levels l = 0 .. n_levels - 1:
        carry = d[c]
        for l: b2[l,c] += carry * carry; nb[l] += 1 (once per level, not per column)
               bit l of has[c] clear: pend[l,c] = carry, set the bit, stop
               else carry = pend[l,c] + carry, clear the bit
    histogram of column hist_column:
        q = floor_divide(x - hist_min, hist_bin); under += q < 0; over += q >= n_bins or x not finite; else hist[q] += 1
    n += 1

Every product and every sum is rounded on its own.  ``b2[l]`` is the sum of squares of the block SUMS of 2^l consecutive
samples (of d), ``nb[l]`` the number of complete blocks; ``pend[l]`` a block of 2^l samples that waits for its partner.

Keys by BINS of a column (``BY_BIN``, ``Statistics.by_bin``; SMOLMC_STAT_BY_BIN, smolmc_set_statistics_binned) gather
several rows of a sample, or none: microcanonical averages A(E) with the enthalpy as the key, averages per composition
with a kind count.  The spec names ``key_column`` (an index into ``columns``, like ``hist_column``), ``n_keys`` in
1..65536, ``key_min`` and ``key_bin`` > 0.  The rows of an offer are taken SAMPLE BY SAMPLE, AND WITHIN A SAMPLE IN
WALKER ORDER 0 .. R - 1.  For each row:

    q = floor_divide(x[key_column] - key_min, key_bin)     ``bin_of``: the bin function of the Wang-Landau step and of
                                                           the histogram above
    q < 0:                            key_under += 1       one int64 for the whole record
    q >= n_keys or x not finite:      key_over += 1
        (neither row is offered to any key)
    else: the row is offered to key q by the rule above: the key's first row is the shift, then s1, the s2 triangle, the
        per-key histogram of hist_column with the key's under and over, and n += 1

Blocking means nothing when successive rows of a key come from different walkers: this mode refuses ``n_levels != 0``; the
record's arrays keep their shapes with L = 0.  Every product and every sum is rounded on its own, as above.  The
walker-to-state-point map is not read.  The ORDER of a key's offers is part of the definition: sums of doubles depend on it.

A record may carry a SITE FIELD (``Statistics(..., sites=, site_codes=)``; smolmc_set_statistics_sites): ``site_counts``
(n_keys, M, S) and ``site_over`` (n_keys,), int64.  The M tracked sites are ``sites``, distinct site numbers in the caller's
numbering (None: all N sites, in order); S = ``site_codes``, 1..16.  For every row that the rule above offers to key k -- the
rows that increment ``n[k]``: one per key and sample in the two permutation modes, the rows inside the bins of a binned
record, never a row counted in ``key_under`` / ``key_over`` -- and every tracked site m with code c in the row's occupancy:

    c < S:      site_counts[k, m, c] += 1
    otherwise:  site_over[k] += 1

so that ``site_counts[k].sum() + site_over[k] == M * n[k]``.  ``site_counts[k, m, c] / n[k]`` is the site-resolved average
<delta(sigma_m, c)> of key k (``site_occupancy``).  Sums of integers: no order matters, the device gives the same numbers.

A record may carry a JOINT FIELD (``Statistics(..., joint=((col_a, n_a, min_a, bin_a), (col_b, n_b, min_b, bin_b)))``;
smolmc_set_statistics_joint): ``joint`` (n_keys, n_a, n_b) and ``joint_out`` (n_keys,), int64, a histogram of TWO of the
record's columns per key.  For every row that the rule above offers to key k (the rows that increment ``n[k]``, in any of
the three key modes):

    qa = floor_divide(x[col_a] - min_a, bin_a), qb = floor_divide(x[col_b] - min_b, bin_b)       ``bin_of``
    both values finite, 0 <= qa < n_a and 0 <= qb < n_b:    joint[k, qa, qb] += 1
    otherwise:                                              joint_out[k] += 1

so that ``joint[k].sum() + joint_out[k] == n[k]``.  Integer sums again: the device gives the same numbers.  With the key a
state point of a semigrand mu-T grid, axis a the energy E and axis b a count N this is H_k(E, N): ``reweight_joint`` moves
a state point in T AND mu, ``wham_joint`` joins the state points of a grid into ln g(E, N), ``coexistence`` finds the mu of
equal weight.  WHICH COLUMNS: on a semigrand handle E is ``ENERGY``, the weighted sum of the features with the natural
parameters as ``weights`` and weight 0 on the chemical-work feature -- NOT ``ENTHALPY``, which already contains -mu N and
would count the field twice; N is a kind count (``kind(obs, k)``), and the field conjugate to it is the chemical potential
of that kind's species less the one its sublattice's other species share.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from .minima import weighted_value

BY_WALKER, BY_STATE_POINT = 0, 1   # SMOLMC_STAT_BY_WALKER, SMOLMC_STAT_BY_STATE_POINT
BY_BIN = 2                         # SMOLMC_STAT_BY_BIN: bins of a column (Statistics.by_bin)
MAX_KEYS = 65536                   # SMOLMC_MAX_STAT_KEYS
MAX_COLUMNS = 32                   # SMOLMC_MAX_STAT_COLUMNS
MAX_LEVELS = 32                    # SMOLMC_MAX_STAT_LEVELS
MAX_BINS = 65536                   # SMOLMC_MAX_STAT_BINS
MAX_SITE_CODES = 16                # SMOLMC_MAX_STAT_SITE_CODES
KB = 8.617333262145e-5             # eV / K, SMOLMC_KB (smol/constants.py:4)

_ARRAYS = ("n", "shift", "s1", "s2", "has", "pend", "b2", "nb", "hist", "under", "over")
_SITE_ARRAYS = ("site_counts", "site_over")  # the site field (empty without one)
_JOINT_ARRAYS = ("joint", "joint_out")       # the joint field (empty without one)
MAX_JOINT_CELLS = 65536            # SMOLMC_MAX_STAT_JOINT_CELLS: the cells of one axis of a joint field
_MODE_NAMES = {BY_WALKER: "by walker", BY_STATE_POINT: "by state point", BY_BIN: "by bin"}

# ---- column sources: symbolic, resolved against a handle's (F, K) by Statistics.sources -------------------------------
ENTHALPY = ("enthalpy",)
ENERGY = ("energy",)       # the weighted sum of the features (``weights``): the energy of a semigrand run


def feature(i):
    return ("feature", int(i))


def intensity(i):
    """Intensity ``i`` of the structure-factor spec in force (``structure.StructureFactor``)."""
    return ("intensity", int(i))


def connectivity(g, column):
    """Number ``column`` (a column constant of ``smol_amd.connectivity``, 0..23) of graph ``g`` of the connectivity spec in
    force (``connectivity.Connectivity``), read as a double."""
    if not 0 <= int(column) < 24:
        raise ValueError(f"connectivity column {column} outside 0..23")
    return ("connectivity", int(g), int(column))


def pattern(c):
    """Cell ``c`` of the pattern spec in force (``patterns.Patterns``; ``Patterns.cell`` gives the number of a pattern), read
    as a double."""
    if int(c) < 0:
        raise ValueError(f"pattern cell {c} is negative")
    return ("pattern", int(c))


def environment(c):
    """Cell ``c`` of the environment spec in force (``environments.Environments``; ``Environments.cell`` gives the number of
    an environment), read as a double."""
    if int(c) < 0:
        raise ValueError(f"environment cell {c} is negative")
    return ("environment", int(c))


def kind(observables, name_or_k):
    """Count column of kind ``name_or_k`` of ``observables`` (an ``observables.Observables``): a kind number, or a name
    looked up in ``observables.kind_names`` when it has them."""
    if isinstance(name_or_k, (int, np.integer)):
        k = int(name_or_k)
    else:
        names = [str(x) for x in getattr(observables, "kind_names", None) or []]
        if str(name_or_k) not in names:
            raise ValueError(f"no kind named {name_or_k!r} among {names}")
        k = names.index(str(name_or_k))
    K = int(getattr(observables, "n_kinds", observables))
    if not 0 <= k < K:
        raise ValueError(f"kind {k} outside 0..{K - 1}")
    return ("kind", k)


def segments(n_features, n_kinds, n_intensities=0, n_graphs=0, n_cells=0, n_env_cells=0):
    """The column sources of the C ABI as ordered segments (tag, first source, width), for the sizes in force
    F, K, I, G, P (``n_cells``), E (``n_env_cells``):

        0                              enthalpy
        1 + i                          feature i
        1 + F + k                      kind k of the observables
        1 + F + K                      energy: the weighted sum of the features
        2 + F + K + i                  intensity i of the structure-factor spec
        2 + F + K + I + 24 g + c       connectivity: number c of graph g of the connectivity spec
        2 + F + K + I + 24 G + c       pattern: cell c of the pattern spec
        2 + F + K + I + 24 G + P + c   environment: cell c of the environment spec

    The five segments of ``families.FAMILIES`` come in the table's order; a size is 0 when no spec is in force."""
    out, first = [], 0
    for tag, width in (("enthalpy", 1), ("feature", n_features), ("kind", n_kinds), ("energy", 1), ("intensity", n_intensities),
                       ("connectivity", 24 * int(n_graphs)), ("pattern", n_cells), ("environment", n_env_cells)):
        out.append((tag, first, int(width)))
        first += int(width)
    return tuple(out)


# the tags whose range ``Statistics.sources`` checks: (what is counted, "... of the <which> spec", sources per unit)
_CHECKED = {"intensity": ("intensity", "intensities of the structure-factor", 1),
            "connectivity": ("graph", "graphs of the connectivity", 24),
            "pattern": ("cell", "cells of the pattern", 1), "environment": ("cell", "cells of the environment", 1)}


class Statistics:
    """The spec of a record: how it is keyed, its columns, the weights of the ENERGY column, the blocking levels and the
    histogram (``hist=(column, n_bins, hist_min, hist_bin)`` with ``column`` one of ``columns``).  A record keyed by bin
    (``by_bin``) also has ``bins=(column, n_keys, key_min, key_bin)``, ``column`` one of ``columns``; a spec with key
    ``BY_BIN`` and no ``bins`` is not binned, and the engine refuses it.  ``site_codes`` > 0 gives the record a site field
    (module docstring) of the sites ``sites`` (None: all sites) and the codes 0 .. ``site_codes`` - 1.
    ``joint=((col_a, n_a, min_a, bin_a), (col_b, n_b, min_b, bin_b))`` gives it a joint field (module docstring): ``col_a``
    and ``col_b`` are named like the histogram's column and must be among ``columns``; they may be the same column.  For
    T-mu reweighting on a semigrand handle axis a is ``ENERGY`` (not ``ENTHALPY``, which contains -mu N) and axis b a kind
    count.  A ValueError for an axis with ``n`` outside 1..65536, a bin width that is not a positive finite number or a
    minimum that is not finite: what smolmc_set_statistics_joint refuses."""

    def __init__(self, key=BY_WALKER, columns=(ENTHALPY,), weights=None, n_levels=0, hist=None, bins=None, sites=None,
                 site_codes=0, joint=None):
        self.key = int(key)
        self.columns = [tuple(c) if not isinstance(c, (int, np.integer)) else ("source", int(c)) for c in columns]
        self.weights = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        self.n_levels = int(n_levels)
        if hist is None:
            self.hist_column, self.n_bins, self.hist_min, self.hist_bin = 0, 0, 0.0, 1.0
        else:
            col, n_bins, hmin, hbin = hist
            col = tuple(col) if not isinstance(col, (int, np.integer)) else ("source", int(col))
            if col not in self.columns:
                raise ValueError("the histogram's column must be one of the record's columns")
            self.hist_column, self.n_bins, self.hist_min, self.hist_bin = self.columns.index(col), int(n_bins), float(hmin), float(hbin)
        self.key_column, self.n_keys, self.key_min, self.key_bin = 0, 0, 0.0, 0.0
        self.binned = bins is not None
        if bins is not None:
            col, n_keys, kmin, kbin = bins
            col = tuple(col) if not isinstance(col, (int, np.integer)) else ("source", int(col))
            if col not in self.columns:
                raise ValueError("the key's column must be one of the record's columns")
            self.key_column, self.n_keys, self.key_min, self.key_bin = self.columns.index(col), int(n_keys), float(kmin), float(kbin)
        self.site_codes = int(site_codes)
        self.sites = None if sites is None or not self.site_codes else np.ascontiguousarray(sites, dtype=np.int32).reshape(-1)
        # (ranges, duplicates, sizes: the engine refuses them, naming the reason)
        self.joint_columns, self.joint_n, self.joint_min, self.joint_bin = (0, 0), (0, 0), (0.0, 0.0), (0.0, 0.0)
        if joint is not None:
            if len(joint) != 2 or any(len(ax) != 4 for ax in joint):
                raise ValueError("joint= takes two axes ((col_a, n_a, min_a, bin_a), (col_b, n_b, min_b, bin_b))")
            cols = []
            for name, (col, n, vmin, vbin) in zip("ab", joint):
                col = tuple(col) if not isinstance(col, (int, np.integer)) else ("source", int(col))
                if col not in self.columns:
                    raise ValueError(f"the joint field's column {name} must be one of the record's columns")
                if not 1 <= int(n) <= MAX_JOINT_CELLS:
                    raise ValueError(f"the joint field's n_{name} must be 1..{MAX_JOINT_CELLS}, got {int(n)}")
                if not (np.isfinite(vbin) and float(vbin) > 0.0 and np.isfinite(vmin)):
                    raise ValueError(f"the joint field's bin_{name} must be a positive finite number and min_{name} finite")
                cols.append(self.columns.index(col))
            self.joint_columns = tuple(cols)
            self.joint_n = tuple(int(ax[1]) for ax in joint)
            self.joint_min = tuple(float(ax[2]) for ax in joint)
            self.joint_bin = tuple(float(ax[3]) for ax in joint)

    @classmethod
    def per_walker(cls, columns=(ENTHALPY,), **kw):
        return cls(BY_WALKER, columns, **kw)

    @classmethod
    def by_state_point(cls, columns=(ENTHALPY,), **kw):
        return cls(BY_STATE_POINT, columns, **kw)

    @classmethod
    def by_bin(cls, key, n_keys, key_min, key_bin, columns=(ENTHALPY,), weights=None, hist=None, sites=None, site_codes=0,
               joint=None):
        """Keyed by ``n_keys`` bins of width ``key_bin`` from ``key_min`` of the column ``key``, one of ``columns``."""
        return cls(BY_BIN, columns, weights, 0, hist, bins=(key, n_keys, key_min, key_bin), sites=sites, site_codes=site_codes,
                   joint=joint)

    @classmethod
    def by_composition(cls, obs, kind_name_or_k, num_sites, columns=None, **kw):
        """Keyed by the count of one kind of ``obs`` (an ``observables.Observables``): bins of width 1, ``num_sites + 1``
        keys, key k holds the rows with k sites of that kind.  ``columns`` defaults to the count and the enthalpy; the
        count is put in front when ``columns`` leaves it out."""
        key = kind(obs, kind_name_or_k)
        cols = [key, ENTHALPY] if columns is None else [tuple(c) if not isinstance(c, (int, np.integer)) else ("source", int(c))
                                                        for c in columns]
        if key not in cols:
            cols = [key] + cols
        return cls.by_bin(key, int(num_sites) + 1, 0.0, 1.0, cols, **kw)

    @classmethod
    def on_wl_levels(cls, min_enthalpy, bin_size, n_levels, columns=(ENTHALPY,), **kw):
        """Keyed by the enthalpy on a Wang-Landau handle's own ``(min_enthalpy, bin_size)`` with ``n_levels`` keys (the
        number of its levels, not blocking levels).  On a handle without windows key k IS Wang-Landau level k: both
        sides apply the same function to the same numbers.  With per-walker windows the record uses this GLOBAL grid;
        nothing is claimed about a walker's local level numbers.  The enthalpy is put in front of ``columns`` when they
        leave it out."""
        cols = [tuple(c) if not isinstance(c, (int, np.integer)) else ("source", int(c)) for c in columns]
        if ENTHALPY not in cols:
            cols = [ENTHALPY] + cols
        return cls.by_bin(ENTHALPY, int(n_levels), float(min_enthalpy), float(bin_size), cols, **kw)

    n_columns = property(lambda self: len(self.columns))
    n_weights = property(lambda self: 0 if self.weights is None else len(self.weights))
    n_pairs = property(lambda self: self.n_columns * (self.n_columns + 1) // 2)

    def site_list(self, num_sites):
        """The tracked sites as an index array into rows of ``num_sites`` sites (all of them when ``sites`` is None)."""
        return np.arange(int(num_sites)) if self.sites is None else self.sites.astype(np.int64)

    def c_sites(self):
        """The arguments of smolmc_set_statistics_sites behind the handle (sites or None, n_sites, n_codes), or None for a
        spec without a site field."""
        if not self.site_codes:
            return None
        return self.sites, 0 if self.sites is None else len(self.sites), self.site_codes

    has_joint = property(lambda self: self.joint_n[0] > 0)

    def c_joint(self):
        """The arguments of smolmc_set_statistics_joint behind the handle (column_a, n_a, min_a, bin_a, column_b, n_b,
        min_b, bin_b), or None for a spec without a joint field."""
        if not self.has_joint:
            return None
        return tuple(v for i in (0, 1) for v in (self.joint_columns[i], self.joint_n[i], self.joint_min[i], self.joint_bin[i]))

    def joint_axes(self):
        """The ``joint=`` argument that makes this spec's field again (None without one)."""
        if not self.has_joint:
            return None
        return tuple((self.columns[self.joint_columns[i]], self.joint_n[i], self.joint_min[i], self.joint_bin[i]) for i in (0, 1))

    def joint_centres(self):
        """(centres of axis a (n_a,), centres of axis b (n_b,)): min + (i + 1/2) bin."""
        return tuple(self.joint_min[i] + (np.arange(self.joint_n[i]) + 0.5) * self.joint_bin[i] for i in (0, 1))

    def describe(self):
        """The spec as plain values (it goes into a record's .npz, ``StatisticsRecord.save``); ``from_description`` is
        the inverse."""
        return dict(key=self.key, columns=[list(c) for c in self.columns],
                    weights=None if self.weights is None else self.weights.tolist(), n_levels=self.n_levels,
                    hist=None if not self.n_bins else [list(self.columns[self.hist_column]), self.n_bins, self.hist_min, self.hist_bin],
                    bins=None if not self.binned else [list(self.columns[self.key_column]), self.n_keys, self.key_min, self.key_bin],
                    sites=None if self.sites is None else self.sites.tolist(), site_codes=self.site_codes,
                    joint=None if not self.has_joint else [[list(c), n, lo, w] for c, n, lo, w in self.joint_axes()])

    @classmethod
    def from_description(cls, d):
        def axis(ax):
            return None if ax is None else (tuple(ax[0]),) + tuple(ax[1:])

        return cls(d["key"], [tuple(c) for c in d["columns"]], d["weights"], d["n_levels"], axis(d["hist"]), axis(d["bins"]),
                   d["sites"], d["site_codes"], None if d.get("joint") is None else tuple(axis(ax) for ax in d["joint"]))

    def sources(self, n_features, n_kinds, n_intensities=0, n_graphs=0, n_cells=0, n_env_cells=0):
        """int32 column sources of the C ABI (``segments``): a tagged column is its number within the segment of its tag,
        24 g + c for number c of graph g of the connectivity spec; a plain number is a source as it stands."""
        first_of = {tag: (first, width) for tag, first, width in
                    segments(n_features, n_kinds, n_intensities, n_graphs, n_cells, n_env_cells)}
        out = []
        for c in self.columns:
            if c[0] == "source":
                out.append(c[1])
                continue
            first, width = first_of[c[0]]
            if c[0] in _CHECKED:  # (the other ranges: the engine refuses them)
                one, many, unit = _CHECKED[c[0]]
                if not 0 <= c[1] < width // unit:
                    raise ValueError(f"{one} {c[1]} outside the {width // unit} {many} spec")
            out.append(first + (0 if len(c) == 1 else c[1] if len(c) == 2 else 24 * c[1] + c[2]))
        return np.asarray(out, dtype=np.int32)

    def tagged_columns(self, tag):
        """Indices into ``columns`` of the columns with ``tag``, in order."""
        return [i for i, c in enumerate(self.columns) if c[0] == tag]

    def count_columns(self):
        """Indices into ``columns`` of the kind counts, in order."""
        return self.tagged_columns("kind")

    def intensity_columns(self):
        """Indices into ``columns`` of the intensities, in order."""
        return self.tagged_columns("intensity")

    def connectivity_columns(self):
        """Indices into ``columns`` of the connectivity numbers, in order."""
        return self.tagged_columns("connectivity")

    def pattern_columns(self):
        """Indices into ``columns`` of the pattern cells, in order."""
        return self.tagged_columns("pattern")

    def environment_columns(self):
        """Indices into ``columns`` of the environment cells, in order."""
        return self.tagged_columns("environment")

    def column_values(self, enthalpy, features, counts=None, intensities=None, connectivity=None, patterns=None,
                      environments=None):
        """x (..., C) float64 of rows with enthalpy (...), features (..., F), counts (..., K) or None, intensities
        (..., I) or None, connectivity stats (..., G, 24) or None, pattern cells (..., n_cells) or None, environment cells
        (..., n_env_cells) or None."""
        H = np.asarray(enthalpy, dtype=np.float64)
        f = np.asarray(features, dtype=np.float64).reshape(H.shape + (-1,))
        given = dict(kind=counts, intensity=intensities, connectivity=connectivity, pattern=patterns, environment=environments)
        size = {tag: 0 if a is None else np.asarray(a).shape[-2 if tag == "connectivity" else -1] for tag, a in given.items()}
        segs = segments(f.shape[-1], size["kind"], size["intensity"], size["connectivity"], size["pattern"], size["environment"])
        x = np.empty(H.shape + (self.n_columns,))
        for j, src in enumerate(self.sources(f.shape[-1], *size.values())):
            tag, first, width = next((s for s in segs if s[1] <= src < s[1] + s[2]), (None, 0, 0))
            if tag is None:
                raise ValueError(f"column source {src} outside 0..{segs[-1][1] + segs[-1][2] - 1}")
            if tag == "enthalpy":
                x[..., j] = H
            elif tag == "feature":
                x[..., j] = f[..., src - first]
            elif tag == "energy":
                x[..., j] = weighted_value(self.weights if self.weights is not None else np.zeros(0), f)
            else:  # (a family's segment: its values, flat per row, read as doubles)
                x[..., j] = np.asarray(given[tag]).reshape(H.shape + (width,))[..., src - first].astype(np.float64)
        return x

    def c_struct(self, n_features, n_kinds, n_intensities=0, n_graphs=0, n_cells=0, n_env_cells=0):
        """(capi.smolmc_statistics, the arrays it points to)."""
        from . import capi

        cols = self.sources(n_features, n_kinds, n_intensities, n_graphs, n_cells, n_env_cells)
        keep = (cols, self.weights)
        s = capi.smolmc_statistics(
            self.key, len(cols), cols.ctypes.data_as(C.POINTER(C.c_int32)) if len(cols) else None, self.n_weights,
            self.weights.ctypes.data_as(C.POINTER(C.c_double)) if self.n_weights else None, self.n_levels,
            self.hist_column, self.n_bins, self.hist_min, self.hist_bin)
        return s, keep

    def c_bins(self):
        """The extra scalars of smolmc_set_statistics_binned (key_column, n_keys, key_min, key_bin), or None for a spec
        that is not binned (``connectivity.Connectivity.c_gates`` is the same idea)."""
        return (self.key_column, self.n_keys, self.key_min, self.key_bin) if self.binned else None


def bin_of(x, hist_min, hist_bin):
    """``floor_divide(x - hist_min, hist_bin)`` as float64: the exact floor division ``WLWindows.bins`` and the
    Wang-Landau step use (NaN where x is not finite)."""
    with np.errstate(invalid="ignore"):
        return np.floor_divide(np.asarray(x, dtype=np.float64) - hist_min, hist_bin)


def _logsumexp(a, axis):
    """ln sum exp(a) over ``axis``, shifted by the maximum; -inf where every entry is -inf."""
    top = a.max(axis=axis, keepdims=True)
    top = np.where(np.isfinite(top), top, 0.0)
    with np.errstate(divide="ignore"):
        return np.log(np.exp(a - top).sum(axis=axis)) + np.squeeze(top, axis=axis)


class StatisticsRecord:
    """The accumulators: n, under, over (n_keys,) int64; shift, s1 (n_keys, C); s2 (n_keys, C (C + 1) / 2); has (n_keys, C)
    uint64; pend, b2 (n_keys, n_levels, C); nb (n_keys, n_levels) int64; hist (n_keys, n_bins) int64.  A binned record
    (``spec.binned``) takes ``n_keys`` from the spec and counts the rows outside its bins in ``key_under`` and ``key_over``
    (ints; 0 in the other modes).  The site field: site_counts (n_keys, M, S), site_over (n_keys,) int64; M = 0 and S = 0
    without one.  With all sites tracked M is ``n_sites``, or, where that is not given, taken from the first occupancy rows
    offered.  The joint field: joint (n_keys, n_a, n_b), joint_out (n_keys,) int64; n_a = n_b = 0 without one."""

    def __init__(self, spec, n_keys=None, n_sites=None):
        self.spec = spec
        if spec.binned:
            n_keys = spec.n_keys
        nk, Cn, L, B = int(n_keys), spec.n_columns, spec.n_levels, spec.n_bins
        self.n = np.zeros(nk, dtype=np.int64)
        self.shift = np.zeros((nk, Cn))
        self.s1 = np.zeros((nk, Cn))
        self.s2 = np.zeros((nk, spec.n_pairs))
        self.has = np.zeros((nk, Cn), dtype=np.uint64)
        self.pend = np.zeros((nk, L, Cn))
        self.b2 = np.zeros((nk, L, Cn))
        self.nb = np.zeros((nk, L), dtype=np.int64)
        self.hist = np.zeros((nk, B), dtype=np.int64)
        self.under = np.zeros(nk, dtype=np.int64)
        self.over = np.zeros(nk, dtype=np.int64)
        self.key_under = 0
        self.key_over = 0
        M = 0 if not spec.site_codes else len(spec.sites) if spec.sites is not None else int(n_sites or 0)
        self.site_counts = np.zeros((nk, M, spec.site_codes), dtype=np.int64)
        self.site_over = np.zeros(nk, dtype=np.int64)
        self.joint = np.zeros((nk,) + tuple(spec.joint_n), dtype=np.int64)
        self.joint_out = np.zeros(nk, dtype=np.int64)

    n_keys = property(lambda self: len(self.n))

    def _not_binned(self, what):
        if self.spec.binned:
            raise ValueError(f"{what} is not defined for a record keyed by bin (mode {BY_BIN}, {_MODE_NAMES[BY_BIN]}): successive "
                             "rows of a key come from different walkers and state points")

    def _only_binned(self, what):
        if not self.spec.binned:
            raise ValueError(f"{what} needs a record keyed by bin (Statistics.by_bin), this one is keyed "
                             f"{_MODE_NAMES.get(self.spec.key, self.spec.key)}")

    # ---- the definition ------------------------------------------------------------------------------------------
    def _site_rows(self, occupancy, rows):
        """(inside (rows, M, S) int64 one-hot of the tracked sites' codes below S, outside (rows,) the codes not below S) of
        occupancy rows in the caller's numbering; the field takes its M from them when all sites are tracked."""
        spec = self.spec
        if occupancy is None:
            raise ValueError("a record with a site field needs the occupancy of the rows (offer(..., occupancy=))")
        occ = np.asarray(occupancy).reshape(rows, -1)
        sites = spec.site_list(occ.shape[1])
        if self.site_counts.shape[1] == 0 and not self.n.any():
            self.site_counts = np.zeros((self.n_keys, len(sites), spec.site_codes), dtype=np.int64)
        if len(sites) != self.site_counts.shape[1]:
            raise ValueError(f"the field tracks {self.site_counts.shape[1]} sites, the rows give {len(sites)}")
        sub = occ[:, sites].astype(np.int64)
        inside = (sub[:, :, None] == np.arange(spec.site_codes)[None, None, :]).astype(np.int64)
        return inside, sites.size - inside.sum(axis=(1, 2))

    def _joint_rows(self, x):
        """The flat cell qa n_b + qb of rows x (rows, C) in the joint field, -1 for a row that counts in ``joint_out``."""
        spec = self.spec
        inside = np.ones(len(x), dtype=bool)
        cell = np.zeros(len(x), dtype=np.int64)
        for i in (0, 1):
            xv = x[:, spec.joint_columns[i]]
            q = bin_of(xv, spec.joint_min[i], spec.joint_bin[i])
            with np.errstate(invalid="ignore"):
                ok = np.isfinite(xv) & ~np.isnan(q) & (q >= 0) & (q < spec.joint_n[i])
            inside &= ok
            cell = cell * spec.joint_n[i] + np.where(ok, q, 0.0).astype(np.int64)
        return np.where(inside, cell, -1)

    def offer(self, enthalpy, features, counts=None, key_of_row=None, intensities=None, connectivity=None, patterns=None,
              environments=None, occupancy=None):
        """Offer samples (ns, R) -- or one sample (R,) -- in order.  ``key_of_row`` (R,) or (ns, R): the key of every
        row, a permutation of 0 .. R - 1 per sample (None: the walker).  Vectorised over the keys, a loop over samples.
        ``occupancy`` (ns, R, N) or (R, N), in the caller's numbering: what a record with a site field counts; a record
        without one does not read it."""
        spec = self.spec
        if spec.binned:
            if key_of_row is not None:
                raise ValueError("a record keyed by bin takes the key of a row from its key column, not from key_of_row")
            return self._offer_binned(enthalpy, features, counts, intensities, connectivity, patterns, environments, occupancy)
        nk = self.n_keys
        H = np.asarray(enthalpy, dtype=np.float64).reshape(-1, nk)
        ns = len(H)
        f = np.asarray(features, dtype=np.float64).reshape(ns, nk, -1)
        cnt = None if counts is None else np.asarray(counts).reshape(ns, nk, -1)
        inten = None if intensities is None else np.asarray(intensities, dtype=np.float64).reshape(ns, nk, -1)
        conn = None if connectivity is None else np.asarray(connectivity).reshape(ns, nk, -1, 24)
        pat = None if patterns is None else np.asarray(patterns).reshape(ns, nk, -1)
        env = None if environments is None else np.asarray(environments).reshape(ns, nk, -1)
        x_all = spec.column_values(H, f, cnt, inten, conn, pat, env)
        if key_of_row is None:
            keys = np.broadcast_to(np.arange(nk), (ns, nk))
        else:
            keys = np.broadcast_to(np.asarray(key_of_row, dtype=np.int64), (ns, nk))
        if spec.site_codes:
            inside, outside = self._site_rows(occupancy, ns * nk)
            inside, outside = inside.reshape((ns, nk) + inside.shape[1:]), outside.reshape(ns, nk)
        Cn, L = spec.n_columns, spec.n_levels
        ia, ib = np.triu_indices(Cn)
        rows = np.arange(nk)
        one = np.uint64(1)
        for s in range(ns):
            if not np.array_equal(np.sort(keys[s]), rows):
                raise ValueError("key_of_row must be a permutation of the keys in every sample")
            x = np.empty((nk, Cn))
            x[keys[s]] = x_all[s]  # row r goes to key keys[s][r]
            first = self.n == 0
            self.shift[first] = x[first]
            d = x - self.shift
            self.s1 = self.s1 + d
            self.s2 = self.s2 + d[:, ia] * d[:, ib]
            carry = d.copy()
            live = np.ones((nk, Cn), dtype=bool)  # (all columns of a key walk the same levels)
            for l in range(L):
                if not live.any():
                    break
                bit = one << np.uint64(l)
                self.b2[:, l, :] = np.where(live, self.b2[:, l, :] + carry * carry, self.b2[:, l, :])
                self.nb[:, l] += live[:, 0]
                held = (self.has & bit) != 0
                park = live & ~held
                self.pend[:, l, :] = np.where(park, carry, self.pend[:, l, :])
                self.has = np.where(park, self.has | bit, self.has)
                go = live & held
                carry = np.where(go, self.pend[:, l, :] + carry, carry)
                self.has = np.where(go, self.has & ~bit, self.has)
                live = go
            if spec.n_bins:
                xv = x[:, spec.hist_column]
                q = bin_of(xv, spec.hist_min, spec.hist_bin)
                bad = ~np.isfinite(xv) | np.isnan(q)
                under = ~bad & (q < 0)
                over = bad | (q >= spec.n_bins)
                self.under += under
                self.over += over
                ok = ~(under | over)
                self.hist[rows[ok], q[ok].astype(np.int64)] += 1
            if spec.site_codes:  # (every key once: a plain indexed add)
                self.site_counts[keys[s]] += inside[s]
                self.site_over[keys[s]] += outside[s]
            if spec.has_joint:  # (every key once)
                cell = self._joint_rows(x)
                ok = cell >= 0
                self.joint.reshape(nk, -1)[rows[ok], cell[ok]] += 1
                self.joint_out += ~ok
            self.n += 1
        return self

    def _offer_binned(self, enthalpy, features, counts, intensities, connectivity, patterns, environments, occupancy=None):
        """The rule of the module docstring for samples (ns, R) -- or one sample (R,): the rows in sample-major,
        walker-minor order.  Vectorised over the keys: round j offers the j-th row of every key."""
        spec = self.spec
        if spec.n_levels:
            raise ValueError("a record keyed by bin keeps no blocking sums: n_levels must be 0")
        H = np.asarray(enthalpy, dtype=np.float64)
        H = H.reshape(1, -1) if H.ndim < 2 else H.reshape(len(H), -1)
        ns, R = H.shape

        def rows_of(a, dtype=None, tail=(-1,)):
            return None if a is None else np.asarray(a, dtype=dtype).reshape((ns, R) + tail)

        x = spec.column_values(H, rows_of(features, np.float64), rows_of(counts), rows_of(intensities, np.float64),
                               rows_of(connectivity, None, (-1, 24)), rows_of(patterns), rows_of(environments))
        x = x.reshape(ns * R, spec.n_columns)  # (row number = sample * R + walker: the order of the offers)
        xk = x[:, spec.key_column]
        q = bin_of(xk, spec.key_min, spec.key_bin)
        bad = ~np.isfinite(xk) | np.isnan(q)
        under = ~bad & (q < 0)
        over = bad | (q >= spec.n_keys)
        self.key_under += int(under.sum())
        self.key_over += int(over.sum())
        ok = ~(under | over)
        if spec.site_codes:  # (the rows inside the bins, each to its key)
            inside, outside = self._site_rows(occupancy, ns * R)
            np.add.at(self.site_counts, q[ok].astype(np.int64), inside[ok])
            np.add.at(self.site_over, q[ok].astype(np.int64), outside[ok])
        x, key = x[ok], q[ok].astype(np.int64)
        if spec.has_joint:  # (the rows inside the bins, each to its key)
            cell = self._joint_rows(x)
            into = cell >= 0
            np.add.at(self.joint.reshape(self.n_keys, -1), (key[into], cell[into]), 1)
            np.add.at(self.joint_out, key[~into], 1)
        # the rank of a row among the rows of its key, in row order
        order = np.argsort(key, kind="stable")
        sk = key[order]
        start = np.flatnonzero(np.r_[True, sk[1:] != sk[:-1]]) if len(sk) else np.zeros(0, dtype=np.int64)
        rank = np.empty(len(key), dtype=np.int64)
        rank[order] = np.arange(len(sk)) - np.repeat(start, np.diff(np.r_[start, len(sk)]))
        ia, ib = np.triu_indices(spec.n_columns)
        for j in range(int(rank.max()) + 1 if len(rank) else 0):
            sel = rank == j
            k, xj = key[sel], x[sel]  # (every key at most once)
            first = self.n[k] == 0
            self.shift[k[first]] = xj[first]
            d = xj - self.shift[k]
            self.s1[k] = self.s1[k] + d
            self.s2[k] = self.s2[k] + d[:, ia] * d[:, ib]
            if spec.n_bins:
                xv = xj[:, spec.hist_column]
                qh = bin_of(xv, spec.hist_min, spec.hist_bin)
                hbad = ~np.isfinite(xv) | np.isnan(qh)
                hunder = ~hbad & (qh < 0)
                hover = hbad | (qh >= spec.n_bins)
                self.under[k] += hunder
                self.over[k] += hover
                hok = ~(hunder | hover)
                self.hist[k[hok], qh[hok].astype(np.int64)] += 1
            self.n[k] += 1
        return self

    # ---- what users do with a record -------------------------------------------------------------------------------
    def _full_s2(self):
        Cn = self.spec.n_columns
        ia, ib = np.triu_indices(Cn)
        m = np.zeros((self.n_keys, Cn, Cn))
        m[:, ia, ib] = self.s2
        m[:, ib, ia] = self.s2
        return m

    def mean(self):
        """(n_keys, C): shift + s1 / n (NaN for a key without samples)."""
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.shift + self.s1 / self.n[:, None]

    def covariance(self):
        """(n_keys, C, C), the population covariance (ddof = 0): s2 / n - (s1 / n)(s1 / n)^T of the shifted values."""
        with np.errstate(invalid="ignore", divide="ignore"):
            m1 = self.s1 / self.n[:, None]
            return self._full_s2() / self.n[:, None, None] - m1[:, :, None] * m1[:, None, :]

    def variance(self):
        return np.einsum("kcc->kc", self.covariance())

    def _column(self, col):
        col = tuple(col)
        if col not in self.spec.columns:
            raise ValueError(f"the record has no column {col}")
        return self.spec.columns.index(col)

    def heat_capacity(self, temperature, column=ENTHALPY):
        """var(H) / (kB T^2) per key, from the enthalpy column (``temperature`` a scalar or one per key)."""
        T = np.broadcast_to(np.asarray(temperature, dtype=np.float64), (self.n_keys,))
        return self.variance()[:, self._column(column)] / (KB * T * T)

    def susceptibility(self, temperature):
        """beta x the covariance of the count columns, (n_keys, n_counts, n_counts)."""
        idx = self.spec.count_columns()
        if not idx:
            raise ValueError("the record has no count columns")
        T = np.broadcast_to(np.asarray(temperature, dtype=np.float64), (self.n_keys,))
        return self.covariance()[:, idx][:, :, idx] / (KB * T)[:, None, None]

    def blocking(self):
        """Per level l the error estimate of the mean from blocks of 2^l samples: (error (n_keys, L, C), its own
        uncertainty (n_keys, L, C), nb (n_keys, L)); a ValueError for a record keyed by bin.  The block means are the block sums / 2^l; their variance (ddof = 0)
        is b2 / (4^l nb) - m_l^2, with m_l the mean over the samples of the nb complete blocks: s1 less the blocks that
        still wait below level l, over nb 2^l.  The error is sqrt(var / (nb - 1)), its uncertainty
        error / sqrt(2 (nb - 1)) (Flyvbjerg & Petersen, eq. 28).  NaN where nb < 2."""
        self._not_binned("blocking")
        L = self.spec.n_levels
        size = (2.0 ** np.arange(L))[None, :, None]
        nb = self.nb[:, :, None].astype(np.float64)
        bits = ((self.has[:, None, :] >> np.arange(L, dtype=np.uint64)[None, :, None]) & np.uint64(1)).astype(bool)
        waiting = np.where(bits, self.pend, 0.0)
        below = np.cumsum(waiting, axis=1) - waiting  # (the pending blocks of the levels j < l)
        with np.errstate(invalid="ignore", divide="ignore"):
            m = (self.s1[:, None, :] - below) / (nb * size)
            var = self.b2 / (size * size * nb) - m * m
            err = np.sqrt(np.maximum(var, 0.0) / (nb - 1.0))
            unc = err / np.sqrt(2.0 * (nb - 1.0))
        bad = np.broadcast_to(nb < 2, err.shape)
        return np.where(bad, np.nan, err), np.where(bad, np.nan, unc), self.nb.copy()

    def standard_error(self, min_blocks=16):
        """(n_keys, C): the blocking error at the plateau.  The rule: the first level l whose estimate is not below the
        next one by more than that level's own uncertainty (err[l + 1] - err[l] <= unc[l]), among levels with at least
        ``min_blocks`` blocks; when no level qualifies, the largest estimate among the levels with ``min_blocks`` blocks
        (a lower bound: the run is too short for a plateau).  Without blocking levels: the naive sqrt(var / (n - 1))."""
        self._not_binned("standard_error")
        nk, Cn, L = self.n_keys, self.spec.n_columns, self.spec.n_levels
        with np.errstate(invalid="ignore", divide="ignore"):
            naive = np.sqrt(self.variance() / (self.n[:, None] - 1.0))
        if L == 0:
            return naive
        err, unc, nb = self.blocking()
        out = naive.copy()
        for k in range(nk):
            ok = np.flatnonzero(nb[k] >= min_blocks)
            if not len(ok):
                continue
            for c in range(Cn):
                pick = None
                for l in ok:
                    if l + 1 in ok and err[k, l + 1, c] - err[k, l, c] <= unc[k, l, c]:
                        pick = err[k, l, c]
                        break
                out[k, c] = pick if pick is not None else np.nanmax(err[k, ok, c])
        return out

    def autocorrelation_time(self, min_blocks=16):
        """(n_keys, C): the integrated autocorrelation time in samples, tau = (standard_error / naive error)^2 / 2
        (0.5 for uncorrelated samples)."""
        self._not_binned("autocorrelation_time")
        with np.errstate(invalid="ignore", divide="ignore"):
            naive = np.sqrt(self.variance() / (self.n[:, None] - 1.0))
            return 0.5 * (self.standard_error(min_blocks) / naive) ** 2

    @classmethod
    def combine(cls, records):
        """One record from those of several ranks or of the parts of a resumed run that hold the SAME keys: the pairwise
        merge of Chan et al. of n / shift / s1 / s2 (the second record's sums are moved to the first one's shift) and the
        sum of the histograms.  The blocking arrays are NOT merged (a block of 2^l samples does not span two records):
        the result has n_levels = 0.  Binned records of ONE spec merge key by key in the same way and their outside
        counters add; records of different modes, or binned ones of different bins, are refused.  Site fields of the same
        sites and codes add, and so do joint fields of the same axes; records of different fields are refused."""
        records = list(records)
        a = records[0]
        for b in records[1:]:
            if b.site_counts.shape != a.site_counts.shape or (a.spec.site_codes and not np.array_equal(
                    a.spec.site_list(a.site_counts.shape[1]), b.spec.site_list(b.site_counts.shape[1]))):
                raise ValueError(f"combine: records of different site fields ({a.site_counts.shape[1:]} and "
                                 f"{b.site_counts.shape[1:]} sites x codes, or different site lists)")
            if b.spec.c_joint() != a.spec.c_joint():
                raise ValueError(f"combine: records of different joint fields ({a.spec.c_joint()} and {b.spec.c_joint()})")
            if b.spec.key != a.spec.key or b.spec.binned != a.spec.binned:
                raise ValueError(f"combine: records of different key modes ({_MODE_NAMES.get(a.spec.key, a.spec.key)} and "
                                 f"{_MODE_NAMES.get(b.spec.key, b.spec.key)})")
            if a.spec.binned and a.spec.c_bins() != b.spec.c_bins():
                raise ValueError(f"combine: binned records of different bins ({a.spec.c_bins()} and {b.spec.c_bins()})")
        spec = Statistics(a.spec.key, a.spec.columns, a.spec.weights, 0,
                          None if not a.spec.n_bins else (a.spec.columns[a.spec.hist_column], a.spec.n_bins, a.spec.hist_min, a.spec.hist_bin),
                          bins=None if not a.spec.binned else (a.spec.columns[a.spec.key_column],) + a.spec.c_bins()[1:],
                          sites=a.spec.sites, site_codes=a.spec.site_codes, joint=a.spec.joint_axes())
        out = cls(spec, a.n_keys, a.site_counts.shape[1])
        out.key_under, out.key_over = a.key_under, a.key_over
        for f in ("n", "shift", "s1", "s2", "hist", "under", "over") + _SITE_ARRAYS + _JOINT_ARRAYS:
            setattr(out, f, getattr(a, f).copy())
        ia, ib = np.triu_indices(spec.n_columns)
        for b in records[1:]:
            empty = out.n == 0
            out.shift[empty] = b.shift[empty]
            # sums of (x - shift_out) from sums of (x - shift_b): x - shift_out = (x - shift_b) + delta
            delta = b.shift - out.shift
            nb = b.n[:, None].astype(np.float64)
            out.s2 = out.s2 + (b.s2 + delta[:, ia] * b.s1[:, ib] + delta[:, ib] * b.s1[:, ia] + nb * delta[:, ia] * delta[:, ib])
            out.s1 = out.s1 + (b.s1 + nb * delta)
            out.n = out.n + b.n
            out.hist = out.hist + b.hist
            out.under = out.under + b.under
            out.over = out.over + b.over
            out.key_under += b.key_under
            out.key_over += b.key_over
            out.site_counts = out.site_counts + b.site_counts
            out.site_over = out.site_over + b.site_over
            out.joint = out.joint + b.joint
            out.joint_out = out.joint_out + b.joint_out
        return out

    def reweight(self, temperature_from, temperature_to):
        """Single-histogram reweighting of the histogram's column (the enthalpy) from ``temperature_from`` to
        ``temperature_to``: (mean (n_keys,), variance (n_keys,)) of the bin centres under the weights
        hist x exp(-(beta_to - beta_from) E), the exponent shifted by its maximum.  A ValueError for a record keyed by
        bin (its rows have no one temperature): ``canonical`` is what such a record offers."""
        self._not_binned("reweight")
        spec = self.spec
        if not spec.n_bins:
            raise ValueError("the record keeps no histogram")
        Tf = np.broadcast_to(np.asarray(temperature_from, dtype=np.float64), (self.n_keys,))
        Tt = np.broadcast_to(np.asarray(temperature_to, dtype=np.float64), (self.n_keys,))
        centre = spec.hist_min + (np.arange(spec.n_bins) + 0.5) * spec.hist_bin
        db = (1.0 / (KB * Tt) - 1.0 / (KB * Tf))[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            logw = np.where(self.hist > 0, np.log(self.hist.astype(np.float64)), -np.inf) - db * centre[None, :]
            logw = logw - logw.max(axis=1, keepdims=True)
            w = np.exp(logw)
            z = w.sum(axis=1)
            mean = (w * centre).sum(axis=1) / z
            var = (w * (centre[None, :] - mean[:, None]) ** 2).sum(axis=1) / z
        return mean, var

    # ---- binned records: microcanonical averages and what follows from them with ln g ------------------------------
    def key_edges(self):
        """(n_keys + 1,): key k holds the rows with edges[k] <= x[key_column] < edges[k + 1] (up to the rounding of the
        exact floor division)."""
        self._only_binned("key_edges")
        return self.spec.key_min + np.arange(self.n_keys + 1) * self.spec.key_bin

    def key_centres(self):
        """(n_keys,): the middle of every key's bin."""
        self._only_binned("key_centres")
        return self.spec.key_min + (np.arange(self.n_keys) + 0.5) * self.spec.key_bin

    def microcanonical(self):
        """(n_keys, C): the mean of every column over the rows of a key, A(E) when the key is the enthalpy; NaN where
        n == 0."""
        self._only_binned("microcanonical")
        return self.mean()

    def microcanonical_covariance(self):
        """(n_keys, C, C): the population covariance of the columns within a key; NaN where n == 0."""
        self._only_binned("microcanonical_covariance")
        return self.covariance()

    def _canonical_weights(self, ln_g, temperatures, level_values):
        """(use (n_keys,) bool, E (n_used,), w (nT, n_used) normalised): the keys with rows and a finite ln g, their
        energies and their weights exp(ln g_k - beta E_k) / Z at every temperature, by log-sum-exp."""
        ln_g = np.asarray(ln_g, dtype=np.float64).reshape(-1)
        if len(ln_g) != self.n_keys:
            raise ValueError(f"ln_g has {len(ln_g)} entries, the record {self.n_keys} keys")
        use = (self.n > 0) & np.isfinite(ln_g)
        if not use.any():
            raise ValueError("no key has both rows and a finite ln g")
        if ENTHALPY in self.spec.columns:
            E = self.mean()[use, self.spec.columns.index(ENTHALPY)]
        elif level_values is not None:
            E = np.asarray(level_values, dtype=np.float64).reshape(-1)[use]
        else:
            E = self.key_centres()[use]
        T = np.atleast_1d(np.asarray(temperatures, dtype=np.float64))
        beta = 1.0 / (KB * T)
        logw = ln_g[use][None, :] - beta[:, None] * (E - E.min())[None, :]
        logw = logw - logw.max(axis=1, keepdims=True)
        w = np.exp(logw)
        return use, E, w / w.sum(axis=1, keepdims=True)

    def canonical(self, ln_g, temperatures, level_values=None):
        """(nT, C): <x>_T = sum_k xbar_k exp(ln g_k - beta E_k) / sum_k exp(ln g_k - beta E_k) over the keys with n > 0
        and a finite ``ln_g`` (n_keys,), by log-sum-exp.  xbar_k is ``microcanonical()``; E_k is the key's mean enthalpy
        when ``ENTHALPY`` is a column, otherwise ``level_values`` (n_keys,) or, without them, the bin centre.  The key is
        meant to be the enthalpy (``on_wl_levels``) and ``ln_g`` the density of states on the same bins, e.g. a
        Wang-Landau entropy."""
        self._only_binned("canonical")
        use, _, w = self._canonical_weights(ln_g, temperatures, level_values)
        return w @ self.mean()[use]

    def canonical_heat_capacity(self, ln_g, temperatures):
        """(nT,): var_T(H) / (kB T^2) with var_T(H) = sum_k w_k (var_k + (E_k - <E>)^2): the second moment of the enthalpy
        WITHIN every key plus the spread of the keys' means.  Needs the ``ENTHALPY`` column."""
        self._only_binned("canonical_heat_capacity")
        c = self._column(ENTHALPY)
        use, E, w = self._canonical_weights(ln_g, temperatures, None)
        T = np.atleast_1d(np.asarray(temperatures, dtype=np.float64))
        e = E - E.min()
        mean = w @ e
        within = self.variance()[use, c]
        var = (w * (within[None, :] + (e[None, :] - mean[:, None]) ** 2)).sum(axis=1)
        return var / (KB * T * T)

    # ---- the site field --------------------------------------------------------------------------------------------------
    def _with_sites(self, what):
        if not self.spec.site_codes:
            raise ValueError(f"{what} needs a record with a site field (Statistics(..., sites=, site_codes=))")

    def site_occupancy(self):
        """(n_keys, M, S): site_counts / n, how often tracked site m held code s among the rows of key k; NaN where
        n == 0."""
        self._with_sites("site_occupancy")
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.site_counts / self.n[:, None, None].astype(np.float64)

    def sublattice_occupancy(self, classes):
        """(n_keys, n_classes, S): the mean of ``site_occupancy`` over each class of sites; ``classes`` is a sequence of
        index lists into the TRACKED sites (positions 0 .. M - 1 of the field, not site numbers)."""
        p = self.site_occupancy()
        return np.stack([p[:, np.asarray(c, dtype=np.int64), :].mean(axis=1) for c in classes], axis=1)

    def frozen_order(self):
        """(n_keys,): mean_m sum_s p_m(s)^2 less the same number for the key's mean composition over the tracked sites,
        sum_s (mean_m p_m(s))^2.  0 for a field that is uniform over the sites (a walker that visits every ordering
        variant alike, or a disordered state), 1 - sum_s x_s^2 for a walker frozen in one configuration of composition
        x."""
        p = self.site_occupancy()
        return (p * p).sum(axis=2).mean(axis=1) - (p.mean(axis=1) ** 2).sum(axis=1)

    def canonical_sites(self, ln_g, temperatures, level_values=None):
        """(nT, M, S): the site field at every temperature from a record keyed by bin, sum_k w_k(T) p_k with p_k the field
        of level k (``site_occupancy``) and the weights of ``canonical``."""
        self._only_binned("canonical_sites")
        p = self.site_occupancy()
        use, _, w = self._canonical_weights(ln_g, temperatures, level_values)
        return np.tensordot(w, p[use], axes=(1, 0))

    # ---- the joint field -------------------------------------------------------------------------------------------------
    def _with_joint(self, what):
        if not self.spec.has_joint:
            raise ValueError(f"{what} needs a record with a joint field (Statistics(..., joint=))")

    def joint_histogram(self):
        """(joint (n_keys, n_a, n_b) int64, centres of axis a (n_a,), centres of axis b (n_b,))."""
        self._with_joint("joint_histogram")
        return (self.joint,) + self.spec.joint_centres()

    def marginal(self, axis):
        """(n_keys, n_a) for ``axis`` 0 and (n_keys, n_b) for 1: the joint field summed over the OTHER axis."""
        self._with_joint("marginal")
        if axis not in (0, 1):
            raise ValueError(f"marginal: axis must be 0 (a) or 1 (b), got {axis}")
        return self.joint.sum(axis=2 - axis)

    def free_energy_surface(self, temperature):
        """(n_keys, n_a, n_b): -kB T ln P(a, b) with P = joint / joint.sum() per key; +inf where the count is 0 (a key
        without counts is +inf everywhere).  ``temperature`` a scalar or one per key."""
        self._with_joint("free_energy_surface")
        T = np.broadcast_to(np.asarray(temperature, dtype=np.float64), (self.n_keys,))
        total = self.joint.sum(axis=(1, 2)).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            ln_p = np.log(self.joint.astype(np.float64)) - np.log(total)[:, None, None]
        return np.where(self.joint > 0, -(KB * T)[:, None, None] * ln_p, np.inf)

    @staticmethod
    def _joint_moments(logw, e, n):
        """Of weights exp(logw) (..., n_a, n_b) on the points (e[a], n[b]): (mean (..., 2), covariance (..., 2, 2) of
        (E, N), P(N) (..., n_b)).  The exponent is shifted by its maximum; NaN where no weight is finite."""
        with np.errstate(invalid="ignore", divide="ignore"):
            w = np.exp(logw - logw.max(axis=(-2, -1), keepdims=True))
            w = w / w.sum(axis=(-2, -1), keepdims=True)
            pa, pn = w.sum(axis=-1), w.sum(axis=-2)
            me, mn = (pa * e).sum(axis=-1), (pn * n).sum(axis=-1)
            de, dn = e - me[..., None], n - mn[..., None]
            cee, cnn = (pa * de * de).sum(axis=-1), (pn * dn * dn).sum(axis=-1)
            cen = (w * de[..., :, None] * dn[..., None, :]).sum(axis=(-2, -1))
        cov = np.stack([np.stack([cee, cen], axis=-1), np.stack([cen, cnn], axis=-1)], axis=-2)
        return np.stack([me, mn], axis=-1), cov, pn

    def reweight_joint(self, beta_from, field_from, beta_to, field_to):
        """Two-field single-histogram reweighting of every key from (beta_from, field_from) to (beta_to, field_to), each
        a scalar or one per key.  Axis a is the energy E and axis b the conjugate count N (on a semigrand handle
        ``ENERGY`` and a kind count, module docstring; beta = 1 / (kB T), the field the chemical potential conjugate to
        N).  The weights are joint x exp(-(beta_to - beta_from) E + (beta_to field_to - beta_from field_from) N) on the
        bin centres, the exponent shifted by its maximum.  Returns (mean (n_keys, 2), covariance (n_keys, 2, 2) of
        (E, N), P(N) (n_keys, n_b)); NaN for a key without counts.  A ValueError for a record keyed by bin: its rows have
        no one state point."""
        self._not_binned("reweight_joint")
        self._with_joint("reweight_joint")
        e, n = self.spec.joint_centres()
        bf, ff, bt, ft = (np.broadcast_to(np.asarray(v, dtype=np.float64), (self.n_keys,)) for v in
                          (beta_from, field_from, beta_to, field_to))
        with np.errstate(divide="ignore"):
            logw = (np.log(self.joint.astype(np.float64)) - ((bt - bf)[:, None] * e[None, :])[:, :, None]
                    + ((bt * ft - bf * ff)[:, None] * n[None, :])[:, None, :])
        return self._joint_moments(logw, e, n)

    def wham_joint(self, betas, fields, tol=1e-12, max_iter=100000):
        """The multiple-histogram method (Ferrenberg & Swendsen 1989) over the keys, which hold the KNOWN state points
        ``betas`` (n_keys,) and ``fields`` (n_keys,): in log space, with N_k the counts of key k inside its field,

            ln g(a, b) = ln sum_k joint[k, a, b] - ln sum_k N_k exp(f_k - beta_k E_a + beta_k field_k N_b)
            f_k = -ln sum_ab g(a, b) exp(-beta_k E_a + beta_k field_k N_b)

        iterated from f = 0 with f_0 held at 0 until no f_k moves by more than ``tol``.  Returns (ln_g (n_a, n_b), -inf
        where no key has a count; f (n_keys,)): ln g up to one constant.  Keys without counts are left out (their f is
        NaN).  A ValueError for a record keyed by bin, and when ``max_iter`` iterations do not reach ``tol``."""
        self._not_binned("wham_joint")
        self._with_joint("wham_joint")
        e, n = self.spec.joint_centres()
        beta = np.asarray(betas, dtype=np.float64).reshape(-1)
        field = np.asarray(fields, dtype=np.float64).reshape(-1)
        if len(beta) != self.n_keys or len(field) != self.n_keys:
            raise ValueError(f"wham_joint: {len(beta)} betas and {len(field)} fields for {self.n_keys} keys")
        total = self.joint.sum(axis=(1, 2))
        use = total > 0
        if not use.any():
            raise ValueError("wham_joint: no key has a count")
        # the exponent of key k on the grid: -beta_k E_a + beta_k field_k N_b
        expo = -beta[use, None, None] * e[None, :, None] + (beta * field)[use, None, None] * n[None, None, :]
        with np.errstate(divide="ignore"):
            ln_top = np.log(self.joint[use].sum(axis=0).astype(np.float64))
        ln_total = np.log(total[use].astype(np.float64))
        seen = np.isfinite(ln_top)
        fk = np.zeros(int(use.sum()))
        for _ in range(int(max_iter)):
            ln_g = np.where(seen, ln_top - _logsumexp(ln_total[:, None, None] + fk[:, None, None] + expo, axis=0), -np.inf)
            new = -_logsumexp((ln_g[None, :, :] + expo).reshape(len(fk), -1), axis=1)
            new = new - new[0]
            moved = np.abs(new - fk).max()
            fk = new
            if moved <= tol:
                break
        else:
            raise ValueError(f"wham_joint: {max_iter} iterations did not bring the free energies within {tol}")
        ln_g = np.where(seen, ln_top - _logsumexp(ln_total[:, None, None] + fk[:, None, None] + expo, axis=0), -np.inf)
        f = np.full(self.n_keys, np.nan)
        f[use] = fk
        return ln_g, f

    def from_ln_g(self, ln_g, beta, field):
        """What ``reweight_joint`` returns, at any (beta, field) (scalars, or arrays of one shape), from ln g (n_a, n_b)
        on this record's axes (``wham_joint``): the weights are exp(ln g - beta E + beta field N).  (mean (..., 2),
        covariance (..., 2, 2), P(N) (..., n_b))."""
        self._with_joint("from_ln_g")
        e, n = self.spec.joint_centres()
        ln_g = np.asarray(ln_g, dtype=np.float64)
        if ln_g.shape != (len(e), len(n)):
            raise ValueError(f"ln_g has shape {ln_g.shape}, the joint field {(len(e), len(n))}")
        b, f = np.broadcast_arrays(np.asarray(beta, dtype=np.float64), np.asarray(field, dtype=np.float64))
        logw = ln_g - b[..., None, None] * e[:, None] + (b * f)[..., None, None] * n[None, :]
        return self._joint_moments(logw, e, n)

    def coexistence(self, ln_g, beta, field_bracket, split, tol=1e-10, max_iter=200):
        """The field at which P(N) of ``from_ln_g(ln_g, beta, field)`` has equal weight below and above bin ``split``
        (sum over b < split = sum over b >= split: the equal-weight rule for the coexistence of two phases), by
        bisection within ``field_bracket = (lo, hi)`` until the bracket is no wider than ``tol``.  A ValueError when the
        difference of the two weights has the same sign at both ends."""
        self._with_joint("coexistence")
        split = int(split)
        if not 0 < split < self.spec.joint_n[1]:
            raise ValueError(f"coexistence: split must be 1..{self.spec.joint_n[1] - 1}, got {split}")

        def excess(field):  # weight below less weight above: falls as the field grows
            pn = self.from_ln_g(ln_g, beta, field)[2]
            return float(pn[:split].sum() - pn[split:].sum())

        lo, hi = (float(v) for v in field_bracket)
        d_lo, d_hi = excess(lo), excess(hi)
        if d_lo == 0.0:
            return lo
        if d_hi == 0.0:
            return hi
        if not d_lo * d_hi < 0.0:
            raise ValueError(f"coexistence: the bracket ({lo}, {hi}) does not change the sign of the weight difference "
                             f"({d_lo:.3g} and {d_hi:.3g})")
        for _ in range(int(max_iter)):
            if abs(hi - lo) <= tol:
                break
            mid = 0.5 * (lo + hi)
            d = excess(mid)
            if d == 0.0:
                return mid
            if (d < 0.0) == (d_lo < 0.0):
                lo, d_lo = mid, d
            else:
                hi = mid
        return 0.5 * (lo + hi)

    def equals(self, other):
        return (all(np.array_equal(getattr(self, f), getattr(other, f), equal_nan=True)
                    for f in _ARRAYS + _SITE_ARRAYS + _JOINT_ARRAYS)
                and (self.key_under, self.key_over) == (other.key_under, other.key_over))

    def copy(self):
        out = StatisticsRecord(self.spec, self.n_keys, self.site_counts.shape[1])
        for f in _ARRAYS + _SITE_ARRAYS + _JOINT_ARRAYS:
            setattr(out, f, getattr(self, f).copy())
        out.key_under, out.key_over = self.key_under, self.key_over
        return out

    def save(self, path):
        """The record as one .npz: every array under its name, the two outside counters, and the spec (``describe``) as
        JSON under ``meta/statistics``."""
        import json

        arrays = {f: getattr(self, f) for f in _ARRAYS + _SITE_ARRAYS + _JOINT_ARRAYS}
        np.savez_compressed(path, key_outside=np.asarray([self.key_under, self.key_over], dtype=np.int64),
                            **{"meta/statistics": np.asarray(json.dumps(self.spec.describe()))}, **arrays)

    @classmethod
    def load(cls, path):
        """The record ``save`` wrote, with its spec."""
        import json

        with np.load(path) as d:
            spec = Statistics.from_description(json.loads(str(d["meta/statistics"])))
            out = cls(spec, len(d["n"]), d["site_counts"].shape[1])
            for f in _ARRAYS + _SITE_ARRAYS + _JOINT_ARRAYS:
                setattr(out, f, d[f].copy())
            out.key_under, out.key_over = (int(v) for v in d["key_outside"])
        return out
