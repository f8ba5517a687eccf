"""ctypes mirror of include/smolmc.h (structs + flattening of model tables).

``TableSet`` flattens the Python-side tables (smol_amd.synth / imported arrays)
into the caller-owned, C-contiguous buffers ``smolmc_tables`` points at, and keeps
them alive -- the same job smol/utils/cluster/container.pyx does for the
reference's raw-pointer containers (container.pyx:31-32,99,115-117).

Dtype errors are raised as ``ValueError`` like the reference's typed memoryviews
("Buffer dtype mismatch", SURVEY.md §8b error conventions).
"""

from __future__ import annotations

import ctypes as C

import numpy as np

FEATURES_CORRELATIONS = 0
FEATURES_INTERACTIONS = 1
KERNEL_METROPOLIS = 0
KERNEL_WANGLANDAU = 1
STEP_FLIP = 0
STEP_SWAP = 1
STEP_TABLE_FLIP = 2
BIAS_NONE, BIAS_FUGACITY, BIAS_SQUARE_CHARGE, BIAS_SQUARE_HYPERPLANE = 0, 1, 2, 3
ABI_VERSION = 8
ERR_RING_FULL = 2  # SMOLMC_ERR_RING_FULL
SAMPLE_OCCUPANCY, SAMPLE_BIAS, SAMPLE_WL = 1, 2, 4  # SMOLMC_SAMPLE_* flags of smolmc_run_sampled
SAMPLE_OBSERVABLES = 8          # ... kind and pair counts of every row (smolmc_set_observables)
MAX_OBS_CELLS = 4096            # SMOLMC_MAX_OBS_CELLS
SAMPLE_MINIMA = 16              # ... every row is offered to the minima record (smolmc_set_minima)
MAX_MINIMA_AXES = 4             # SMOLMC_MAX_MINIMA_AXES
SAMPLE_STATISTICS = 32          # ... every row is offered to the statistics record (smolmc_set_statistics)
SAMPLE_STRUCTURE = 64           # ... structure-factor amplitudes and intensities of every row (smolmc_set_structure)
MAX_STRUCT_POINTS = 4096        # SMOLMC_MAX_STRUCT_POINTS
MAX_STRUCT_PHASES = 65535       # SMOLMC_MAX_STRUCT_PHASES
MAX_STRUCT_CELLS = 12288        # SMOLMC_MAX_STRUCT_CELLS: n_kinds x n_phases
MAX_STRUCT_INTENSITIES = 4096   # SMOLMC_MAX_STRUCT_INTENSITIES
STRUCT_LDS_BYTES = 65536        # the LDS of one workgroup of the structure kernels (structure.hip)
STRUCT_WAVES = 4                # counter kernel: its waves, a counter set per wave while they fit
STRUCT_MASK_CELLS = 128         # most (kind, phase class) cells of a point the bit-mask kernel takes
STRUCT_MASK_ROWS = 4            # ... the rows one of its workgroups takes: their kind masks share LDS


def structure_plan(n_sites, npad, n_kinds, n_phases, n_points):
    """The kernel a structure-factor spec takes on rows of ``n_sites`` sites in ``npad`` bytes (smolmc_sfac_plan in
    csrc/structure.hip): ("mask",) -- the bit-mask kernel; ("counters", counter sets per point, points per pass) -- the
    counter kernel; None when the row does not fit LDS next to the counters of one point."""
    cells = n_kinds * n_phases
    words = (n_sites + 63) // 64
    if cells <= STRUCT_MASK_CELLS and STRUCT_MASK_ROWS * n_kinds * words * 8 <= STRUCT_LDS_BYTES:
        return ("mask",)
    if npad + 4 * cells > STRUCT_LDS_BYTES:
        return None
    copies = STRUCT_WAVES if npad + 4 * STRUCT_WAVES * cells <= STRUCT_LDS_BYTES else 1
    return "counters", copies, min((STRUCT_LDS_BYTES - npad) // (4 * copies * cells), n_points)
SAMPLE_CONNECTIVITY = 128       # ... the connectivity stats of every row (smolmc_set_connectivity)
MAX_CONN_GRAPHS = 8             # SMOLMC_MAX_CONN_GRAPHS
MAX_CONN_IMAGE = 7              # SMOLMC_MAX_CONN_IMAGE
MAX_CONN_PATH_SUM = 32767       # SMOLMC_MAX_CONN_PATH_SUM: n_sites x MAX_CONN_IMAGE must not exceed it
CONN_STATS = 24                 # SMOLMC_CONN_STATS
CONN_WAVES = 4                  # the waves of one workgroup of the connectivity kernel
CONN_LDS_BYTES = 65536          # the LDS of one workgroup of the connectivity kernel (connectivity.hip)
MAX_CONN_GATES = 4              # SMOLMC_MAX_CONN_GATES: gate sites of a bond row
MAX_CONN_GATED_NEIGHBOURS = 64  # the longest neighbour list of a site in a gated graph: 8 bytes of open bits a site


def connectivity_open_bytes(n_neighbours):
    """The bytes of open bits a site takes in a gated graph whose longest neighbour list has ``n_neighbours`` entries (four
    to a group, a bit an entry)."""
    return (4 * ((n_neighbours + 3) // 4) + 7) // 8


def connectivity_lds_bytes(n_sites, npad, open_bytes=0):
    """The LDS a row of ``n_sites`` sites in ``npad`` bytes takes in the connectivity kernel (smolmc_conn_lds_bytes in
    csrc/connectivity.hip): a 64-bit word, a 16-bit size and a mask byte per site next to the row, the partial sums of
    four waves and, for a spec with a gated graph, ``open_bytes`` of open bits per site (the most a gated graph of the spec
    needs); None when that is more than one workgroup has."""
    up4 = lambda v: (v + 3) // 4 * 4  # noqa: E731
    b = 8 * n_sites + npad + up4(2 * n_sites) + up4(n_sites) + (CONN_WAVES * CONN_STATS + 4) * 4 + up4(open_bytes * n_sites)
    return b if b <= CONN_LDS_BYTES else None
SAMPLE_PATTERNS = 256           # ... the pattern cells of every row (smolmc_set_patterns)
MAX_PATTERN_SETS = 8            # SMOLMC_MAX_PATTERN_SETS
MAX_PATTERN_ARITY = 8           # SMOLMC_MAX_PATTERN_ARITY
MAX_PATTERN_CLASSES = 255       # SMOLMC_MAX_PATTERN_CLASSES
MAX_PATTERN_CELLS = 4096        # SMOLMC_MAX_PATTERN_CELLS
SAMPLE_ENVIRONMENTS = 512       # ... the environment cells of every row (smolmc_set_environments)
MAX_ENV_SETS = 8                # SMOLMC_MAX_ENV_SETS
MAX_ENV_WIDTH = 64              # SMOLMC_MAX_ENV_WIDTH
MAX_ENV_CENTRE_CLASSES = 15     # SMOLMC_MAX_ENV_CENTRE_CLASSES
MAX_ENV_NEIGH_CLASSES = 4       # SMOLMC_MAX_ENV_NEIGH_CLASSES
MAX_ENV_CELLS = 4096            # SMOLMC_MAX_ENV_CELLS
MAX_STEP_FLIPS = 8              # SMOLMC_MAX_STEP_FLIPS
STEP_ROW = 2 * MAX_STEP_FLIPS   # SMOLMC_STEP_ROW: int32 per step record (site, code) x 8, -1 = no flip

_i32p = C.POINTER(C.c_int32)
_i64p = C.POINTER(C.c_int64)
_f64p = C.POINTER(C.c_double)


class smolmc_tables(C.Structure):
    _fields_ = [
        ("num_sites", C.c_int32),
        ("size", C.c_int32),
        ("num_orbits", C.c_int32),
        ("num_corr", C.c_int32),
        ("max_species", C.c_int32),
        ("n_orb", C.c_int32),
        ("orb_id", _i32p),
        ("orb_bit_id", _i32p),
        ("orb_nsites", _i32p),
        ("orb_nfunc", _i32p),
        ("orb_tensor_len", _i32p),
        ("orb_stride_off", _i32p),
        ("tensor_indices", _i32p),
        ("orb_ctensor_off", _i64p),
        ("corr_tensors", _f64p),
        ("orb_itensor_off", _i64p),
        ("interaction_tensors", _f64p),
        ("offset", C.c_double),
        ("full_off", _i64p),
        ("full_idx", _i32p),
        ("site_ptr", _i64p),
        ("loc_orbit", _i32p),
        ("loc_ratio", _f64p),
        ("loc_nrows", _i32p),
        ("loc_off", _i64p),
        ("loc_idx", _i32p),
        ("feature_mode", C.c_int32),
        ("ce_coefs", _f64p),
        ("has_ewald", C.c_int32),
        ("ewald_dim", C.c_int32),
        ("ewald_width", C.c_int32),
        ("ewald_inds", _i32p),
        ("ewald_matrix", _f64p),
        ("ewald_coef", C.c_double),
        ("has_mu", C.c_int32),
        ("mu_width", C.c_int32),
        ("mu_table", _f64p),
        ("n_sublattices", C.c_int32),
        ("sub_site_ptr", _i64p),
        ("sub_active_sites", _i32p),
        ("sub_code_ptr", _i64p),
        ("sub_codes", _i32p),
        ("sub_probs", _f64p),
        ("ewald_charges", _f64p),
        ("n_flip_vectors", C.c_int32),
        ("flip_table", _i32p),
        ("flip_weights", _f64p),
        ("swap_weight", C.c_double),
        ("bias_type", C.c_int32),
        ("bias_width", C.c_int32),
        ("bias_table", _f64p),
        ("bias_penalty", C.c_double),
        ("bias_rows", C.c_int32),
        ("bias_intercepts", _f64p),
    ]


class smolmc_config(C.Structure):
    _fields_ = [
        ("n_replicas", C.c_int32),
        ("kernel_type", C.c_int32),
        ("step_type", C.c_int32),
        ("device", C.c_int32),
        ("wl_min_enthalpy", C.c_double),
        ("wl_max_enthalpy", C.c_double),
        ("wl_bin_size", C.c_double),
        ("wl_flatness", C.c_double),
        ("wl_mod_factor", C.c_double),
        ("wl_mod_divisor", C.c_double),
        ("wl_check_period", C.c_int64),
        ("wl_update_period", C.c_int64),
    ]


class smolmc_distance(C.Structure):
    """Mirror of ``smolmc_distance`` (include/smolmc.h): the objective of a distance handle."""

    _fields_ = [
        ("n_features", C.c_int32),
        ("target", _f64p),
        ("weights", _f64p),
        ("match_weight", C.c_double),
        ("match_tol", C.c_double),
        ("n_groups", C.c_int32),
        ("group_diameter", _f64p),
        ("feature_group", _i32p),
        ("kB", C.c_double),
    ]


DIST_MAX_FEATURES = 256  # SMOLMC_DIST_MAX_FEATURES


class smolmc_minima(C.Structure):
    """Mirror of ``smolmc_minima`` (include/smolmc.h); ``minima.Minima.c_struct`` fills it."""

    _fields_ = [
        ("n_weights", C.c_int),
        ("weights", _f64p),
        ("n_axes", C.c_int),
        ("axis_weights", _i32p),
        ("axis_bin", _i32p),
        ("axis_extent", _i32p),
    ]


STAT_BY_WALKER, STAT_BY_STATE_POINT, STAT_BY_BIN = 0, 1, 2  # SMOLMC_STAT_BY_*: the key modes of a statistics record
MAX_STAT_KEYS = 65536  # SMOLMC_MAX_STAT_KEYS: the bins of a record keyed by bin (smolmc_set_statistics_binned)
MAX_STAT_SITE_CODES = 16  # SMOLMC_MAX_STAT_SITE_CODES: the codes of a record's site field (smolmc_set_statistics_sites)
MAX_STAT_JOINT_CELLS = 65536  # SMOLMC_MAX_STAT_JOINT_CELLS: the cells of an axis of a record's joint field (smolmc_set_statistics_joint)


class smolmc_statistics(C.Structure):
    """Mirror of ``smolmc_statistics`` (include/smolmc.h); ``statistics.Statistics.c_struct`` fills it.  A record keyed
    by bin passes its four extra scalars beside the struct (smolmc_set_statistics_binned; ``Statistics.c_bins``)."""

    _fields_ = [
        ("key", C.c_int),
        ("n_columns", C.c_int),
        ("columns", _i32p),
        ("n_weights", C.c_int),
        ("weights", _f64p),
        ("n_levels", C.c_int),
        ("hist_column", C.c_int),
        ("n_bins", C.c_int),
        ("hist_min", C.c_double),
        ("hist_bin", C.c_double),
    ]


class smolmc_structure(C.Structure):
    """Mirror of ``smolmc_structure`` (include/smolmc.h); ``structure.StructureFactor.c_struct`` fills it."""

    _fields_ = [
        ("n_kinds", C.c_int),
        ("kind_base", _i32p),
        ("n_points", C.c_int),
        ("n_phases", C.c_int),
        ("phase", C.POINTER(C.c_uint16)),
        ("table", _i64p),
        ("n_intensities", C.c_int),
        ("intensity", _i32p),
        ("intensity_scale", _f64p),
    ]


class smolmc_connectivity(C.Structure):
    """Mirror of ``smolmc_connectivity`` (include/smolmc.h); ``connectivity.Connectivity.c_struct`` fills it."""

    _fields_ = [
        ("n_kinds", C.c_int),
        ("kind_base", _i32p),
        ("n_graphs", C.c_int),
        ("member_mask", C.POINTER(C.c_uint64)),
        ("bond_ptr", _i64p),
        ("bonds", _i32p),
        ("images", C.POINTER(C.c_int8)),
    ]


class smolmc_conn_gates(C.Structure):
    """Mirror of ``smolmc_conn_gates`` (include/smolmc.h); ``connectivity.Connectivity.c_gates`` fills it."""

    _fields_ = [
        ("gate_mask", C.POINTER(C.c_uint64)),
        ("max_blocked", _i32p),
        ("gate_ptr", _i64p),
        ("gate_sites", _i32p),
    ]


class smolmc_patterns(C.Structure):
    """Mirror of ``smolmc_patterns`` (include/smolmc.h); ``patterns.Patterns.c_struct`` fills it."""

    _fields_ = [
        ("n_sets", C.c_int),
        ("arity", _i32p),
        ("n_classes", _i32p),
        ("class_of_kind", _i32p),
        ("tuple_ptr", _i64p),
        ("sites", _i32p),
    ]


class smolmc_environments(C.Structure):
    """Mirror of ``smolmc_environments`` (include/smolmc.h); ``environments.Environments.c_struct`` fills it."""

    _fields_ = [
        ("n_sets", C.c_int),
        ("width", _i32p),
        ("n_centre_classes", _i32p),
        ("n_neigh_classes", _i32p),
        ("centre_class_of_kind", _i32p),
        ("neigh_class_of_kind", _i32p),
        ("centre_ptr", _i64p),
        ("centres", _i32p),
        ("neighbours", _i32p),
    ]


class smolmc_observables(C.Structure):
    """Mirror of ``smolmc_observables`` (include/smolmc.h); ``observables.Observables.c_struct`` fills it."""

    _fields_ = [
        ("n_kinds", C.c_int),
        ("kind_base", _i32p),
        ("n_shells", C.c_int),
        ("shell_ptr", _i64p),
        ("bonds", _i32p),
    ]


class DistanceSpec:
    """Kept-alive arrays + the ``smolmc_distance`` struct of one distance objective.

    target [F] (entry 0 unused), weights [F-1], groups: the diameter groups as
    (group_diameter [G] ascending, feature_group [F], -1 for entry 0)."""

    def __init__(self, target, weights, match_weight, match_tol, group_diameter, feature_group, kB):
        self.target = _arr(target, np.float64, "target")
        self.weights = _arr(weights, np.float64, "weights")
        self.group_diameter = _arr(group_diameter, np.float64, "group_diameter")
        self.feature_group = _arr(feature_group, np.int32, "feature_group")
        s = smolmc_distance()
        s.n_features = len(self.target)
        s.target = _ptr(self.target, C.c_double)
        s.weights = _ptr(self.weights, C.c_double)
        s.match_weight = float(match_weight)
        s.match_tol = float(match_tol)
        s.n_groups = len(self.group_diameter)
        s.group_diameter = _ptr(self.group_diameter, C.c_double)
        s.feature_group = _ptr(self.feature_group, C.c_int32)
        s.kB = float(kB)
        self.struct = s


def _arr(a, dtype, name):
    a = np.asarray(a)
    if a.dtype != dtype:
        if np.issubdtype(a.dtype, np.integer) and np.issubdtype(dtype, np.integer):
            a = a.astype(dtype)
        elif np.issubdtype(dtype, np.floating) and a.dtype.kind in "fiu":
            a = a.astype(dtype)
        else:
            raise ValueError(
                f"Buffer dtype mismatch for {name}: expected {np.dtype(dtype)} got {a.dtype}"
            )
    return np.ascontiguousarray(a)


def _ptr(a, ctype):
    return a.ctypes.data_as(C.POINTER(ctype))


class TableSet:
    """Flattened, kept-alive model tables + the ``smolmc_tables`` struct.

    Parameters mirror what the reference assembles across
    ClusterSubspace / ClusterExpansion / Processor / Ensemble:

    orbit_data       tuple of (id, bit_id, flat_corr_tensors[K,len], strides[I])
                     -- smol/utils/cluster/__init__.py:4-15
    full_indices     tuple of int32[J_full, I] per orbit -- clusterspace.py:1329-1366
    local_tables     dict site -> list of (orbit_pos, rows int32[J,I], ratio)
                     -- processor/expansion.py:120-138
    interaction_tensors  list [offset, T_1, ...] -- cofe/expansion.py:186-201
    coefs            natural parameters of the CE part (num_corr or num_orbits long)
    sublattices      list of dict(active_sites=int array, codes=int array); inactive
                     sublattices are simply omitted (mcusher.py:55-57)
    """

    def __init__(
        self,
        num_sites,
        size,
        num_orbits,
        num_corr,
        orbit_data,
        full_indices,
        local_tables,
        interaction_tensors,
        coefs,
        feature_mode,
        sublattices,
        nspecies_per_site=None,
        sublattice_probabilities=None,
        ewald_inds=None,
        ewald_matrix=None,
        ewald_coef=1.0,
        mu_table=None,
        ewald_charges=None,
        flip_table=None,
        flip_weights=None,
        swap_weight=0.1,
    ):
        self._keep = {}
        k = self._keep
        t = smolmc_tables()
        n_orb = len(orbit_data)
        if n_orb != num_orbits - 1:
            raise ValueError("orbit_data must hold num_orbits - 1 records")
        t.num_sites, t.size = int(num_sites), int(size)
        t.num_orbits, t.num_corr, t.n_orb = int(num_orbits), int(num_corr), n_orb
        for d in orbit_data:
            if not isinstance(d[0], (int, np.integer)):
                raise TypeError("id must be an integer.")  # container.pyx:52-53
            if not isinstance(d[1], (int, np.integer)):
                raise TypeError("bit_id must be an integer.")
            if not isinstance(d[2], np.ndarray) or not isinstance(d[3], np.ndarray):
                raise TypeError("correlation_tensors / tensor_indices must be numpy arrays.")
            if d[2].ndim != 2:
                raise ValueError("correlation_tensors must be 2D.")  # container.pyx:60-61
            if d[3].ndim != 1:
                raise ValueError("tensor_indices must be 1D.")
        k["orb_id"] = np.array([d[0] for d in orbit_data], dtype=np.int32)
        k["orb_bit_id"] = np.array([d[1] for d in orbit_data], dtype=np.int32)
        k["orb_nsites"] = np.array([len(d[3]) for d in orbit_data], dtype=np.int32)
        k["orb_nfunc"] = np.array([d[2].shape[0] for d in orbit_data], dtype=np.int32)
        k["orb_tensor_len"] = np.array([d[2].shape[1] for d in orbit_data], dtype=np.int32)
        if k["orb_nsites"].max(initial=0) > 6:
            raise ValueError("clusters larger than SMOLMC_MAX_CLUSTER_SITES=6 sites")
        so = np.concatenate(([0], np.cumsum(k["orb_nsites"])))[:-1]
        k["orb_stride_off"] = so.astype(np.int32)
        k["tensor_indices"] = np.concatenate(
            [_arr(d[3], np.int32, "tensor_indices") for d in orbit_data]
        ).astype(np.int32)
        lens = k["orb_nfunc"].astype(np.int64) * k["orb_tensor_len"]
        k["orb_ctensor_off"] = np.concatenate(([0], np.cumsum(lens)))[:-1].astype(np.int64)
        k["corr_tensors"] = np.concatenate(
            [_arr(d[2], np.float64, "correlation_tensors").ravel() for d in orbit_data]
        )
        k["orb_itensor_off"] = np.concatenate(
            ([0], np.cumsum(k["orb_tensor_len"].astype(np.int64)))
        )[:-1].astype(np.int64)
        if interaction_tensors is None:
            # evaluator.pyx:58-59 default: sum of correlation tensors over bit combos
            its = [d[2].sum(axis=0) for d in orbit_data]
            t.offset = 0.0
        else:
            if len(interaction_tensors) != num_orbits:
                raise ValueError(
                    "Number of cluster interaction tensors must be equal to the number of orbits."
                )
            its = [np.ravel(np.asarray(x, dtype=np.float64)) for x in interaction_tensors[1:]]
            t.offset = float(interaction_tensors[0])
        for x, ln in zip(its, k["orb_tensor_len"]):
            if x.size != ln:
                raise ValueError("interaction tensor size does not match its orbit")
        k["interaction_tensors"] = np.ascontiguousarray(np.concatenate(its), dtype=np.float64)
        # full tables
        fulls = [_arr(a, np.int32, "cluster indices") for a in full_indices]
        for a, I in zip(fulls, k["orb_nsites"]):
            if a.ndim != 2 or a.shape[1] != I:
                raise ValueError("All arrays must be 2D.")  # container.pyx:309-311
        k["full_off"] = np.concatenate(([0], np.cumsum([a.size for a in fulls]))).astype(np.int64)
        k["full_idx"] = (
            np.concatenate([a.ravel() for a in fulls]) if fulls else np.zeros(0, np.int32)
        ).astype(np.int32)
        # local tables
        site_ptr = np.zeros(num_sites + 1, dtype=np.int64)
        lo, lr, ln_, loff, lidx = [], [], [], [], []
        off = 0
        for s in range(num_sites):
            for pos, rows, ratio in local_tables.get(s, ()):
                rows = _arr(rows, np.int32, "local cluster indices")
                lo.append(pos)
                lr.append(ratio)
                ln_.append(rows.shape[0])
                loff.append(off)
                lidx.append(rows.ravel())
                off += rows.size
            site_ptr[s + 1] = len(lo)
        k["site_ptr"] = site_ptr
        k["loc_orbit"] = np.array(lo, dtype=np.int32)
        k["loc_ratio"] = np.array(lr, dtype=np.float64)
        k["loc_nrows"] = np.array(ln_, dtype=np.int32)
        k["loc_off"] = np.array(loff, dtype=np.int64)
        k["loc_idx"] = (np.concatenate(lidx) if lidx else np.zeros(0, np.int32)).astype(np.int32)
        # natural parameters
        t.feature_mode = int(feature_mode)
        nce = num_corr if feature_mode == FEATURES_CORRELATIONS else num_orbits
        coefs = _arr(coefs, np.float64, "coefficients")
        if len(coefs) != nce:
            raise ValueError(
                f"The provided coefficients are not the right length. Got {len(coefs)} "
                f"coefficients, the length must be {nce}"
            )  # expansion.py:97-103
        k["ce_coefs"] = coefs
        # ewald
        t.has_ewald = 0
        if ewald_matrix is not None:
            ei = _arr(ewald_inds, np.int32, "ewald_indices")
            em = _arr(ewald_matrix, np.float64, "ewald_matrix")
            if em.ndim != 2 or em.shape[0] != em.shape[1] or ei.shape[0] != num_sites:
                raise ValueError("malformed Ewald tables")
            k["ewald_inds"], k["ewald_matrix"] = ei, em
            t.has_ewald, t.ewald_dim, t.ewald_width = 1, em.shape[0], ei.shape[1]
            t.ewald_coef = float(ewald_coef)
            if ewald_charges is not None:
                ec = _arr(ewald_charges, np.float64, "ewald_charges")
                if ec.shape != (em.shape[0],):
                    raise ValueError("ewald_charges must have one entry per Ewald index")
                k["ewald_charges"] = ec
        # mu
        t.has_mu = 0
        if mu_table is not None:
            mu = _arr(mu_table, np.float64, "chemical potential table")
            if mu.ndim != 2 or mu.shape[0] != num_sites:
                raise ValueError("malformed chemical potential table")
            k["mu_table"] = mu
            t.has_mu, t.mu_width = 1, mu.shape[1]
        # sublattices
        subs = [s for s in sublattices if len(s["active_sites"]) > 0]
        t.n_sublattices = len(subs)
        k["sub_site_ptr"] = np.concatenate(
            ([0], np.cumsum([len(s["active_sites"]) for s in subs]))
        ).astype(np.int64)
        k["sub_active_sites"] = np.concatenate(
            [np.asarray(s["active_sites"]) for s in subs] or [np.zeros(0)]
        ).astype(np.int32)
        k["sub_code_ptr"] = np.concatenate(
            ([0], np.cumsum([len(s["codes"]) for s in subs]))
        ).astype(np.int64)
        k["sub_codes"] = np.concatenate(
            [np.asarray(s["codes"]) for s in subs] or [np.zeros(0)]
        ).astype(np.int32)
        if sublattice_probabilities is None:
            probs = np.full(len(subs), 1.0 / max(len(subs), 1))
        else:
            probs = np.asarray(sublattice_probabilities, dtype=np.float64)
            if len(probs) != len(subs):
                raise AttributeError(
                    "Sublattice probabilities needs to be the same length as sublattices."
                )  # mcusher.py:62-65
            if abs(probs.sum() - 1) > 1e-12:
                raise ValueError("Sublattice probabilities must sum to one.")
        k["sub_probs"] = np.ascontiguousarray(probs)
        if nspecies_per_site is None:
            ms = int(max([len(s["codes"]) for s in subs] + [1]))
        else:
            ms = int(np.max(nspecies_per_site))
        t.max_species = ms
        self.nspecies_per_site = (
            None if nspecies_per_site is None else np.asarray(nspecies_per_site, np.int32)
        )
        # TableFlip table (mcusher.py:489-551)
        t.n_flip_vectors = 0
        t.swap_weight = float(swap_weight)
        if flip_table is not None:
            ft = _arr(np.atleast_2d(flip_table), np.int32, "flip_table")
            d = int(k["sub_code_ptr"][-1])
            if ft.shape[1] != d:
                raise ValueError(f"flip_table must have {d} columns (species of the active sublattices)")
            if flip_weights is None:
                fw = np.ones(2 * len(ft))
            else:
                fw = np.asarray(flip_weights, dtype=np.float64)
                if len(fw) == len(ft):
                    fw = np.repeat(fw, 2)
                if len(fw) != 2 * len(ft):
                    raise ValueError(
                        f"{len(fw)} weights provided. You must provide either 1* or 2* weights "
                        f"given {len(ft)} flip vectors!"
                    )  # mcusher.py:523-530
            if np.any(np.abs(ft).sum(axis=1) // 2 > 8):
                raise ValueError("flip vectors changing more than 8 sites are not supported")
            k["flip_table"], k["flip_weights"] = ft, np.ascontiguousarray(fw)
            t.n_flip_vectors = len(ft)
        for name, ctype in smolmc_tables._fields_:
            if name in k:
                setattr(t, name, _ptr(k[name], ctype._type_))
        self.struct = t
        self.sublattices = subs
        self.num_features = nce + int(t.has_ewald) + int(t.has_mu)

    # convenience -------------------------------------------------------------
    @property
    def num_sites(self):
        return self.struct.num_sites

    @property
    def natural_parameters(self):
        p = list(self._keep["ce_coefs"])
        if self.struct.has_ewald:
            p.append(self.struct.ewald_coef)
        if self.struct.has_mu:
            p.append(-1.0)
        return np.array(p)

    def active_sites(self):
        """The active sites of every active sublattice, in the order of the struct (the order of the rows of
        smolmc_set_walker_mu)."""
        ptr = self._keep["sub_site_ptr"]
        return [np.asarray(self._keep["sub_active_sites"][ptr[k]:ptr[k + 1]], dtype=np.int64) for k in range(len(ptr) - 1)]

    def set_bias(self, bias_type, table=None, penalty=0.0, intercepts=None):
        """Attach (or clear) an MCBias term (smol/moca/kernel/bias.py): ``table`` is the
        reference's per-(site, species code) table -- fugacity fractions (BIAS_FUGACITY,
        bias.py:208-226), oxidation states (BIAS_SQUARE_CHARGE, bias.py:256-262) or, for
        BIAS_SQUARE_HYPERPLANE (bias.py:290-366), one table per hyperplane [rows, N, W] with the
        entry of the normal vector for that species, plus the intercepts b."""
        t = self.struct
        if bias_type == BIAS_NONE:
            t.bias_type, t.bias_width, t.bias_penalty, t.bias_rows = 0, 0, 0.0, 0
            t.bias_table = _f64p()
            t.bias_intercepts = _f64p()
            self._keep.pop("bias_table", None)
            self._keep.pop("bias_intercepts", None)
            return self
        if bias_type not in (BIAS_FUGACITY, BIAS_SQUARE_CHARGE, BIAS_SQUARE_HYPERPLANE):
            raise ValueError(f"unknown bias type {bias_type}")
        tb = _arr(table, np.float64, "bias_table")
        rows = 1
        if bias_type == BIAS_SQUARE_HYPERPLANE:
            if tb.ndim == 2:
                tb = tb[None]
            if tb.ndim != 3 or not 1 <= tb.shape[0] <= 4:
                raise ValueError("hyperplane bias tables must be [1..4 rows x num_sites x species]")
            rows = tb.shape[0]
            icpt = np.zeros(rows) if intercepts is None else _arr(intercepts, np.float64, "bias_intercepts")
            if icpt.shape != (rows,):
                raise ValueError("one intercept per hyperplane")
        shape = tb.shape[-2:]
        if tb.ndim < 2 or shape[0] != t.num_sites or shape[1] < t.max_species:
            raise ValueError("bias table must be [num_sites x >= max species per site]")
        if bias_type == BIAS_FUGACITY and not np.all(tb > 0):
            raise ValueError("fugacity fractions must be positive")
        if bias_type != BIAS_FUGACITY and not penalty > 0:
            raise ValueError("Penalty factor should be > 0!")  # bias.py:250-251, :328-329
        tb = np.ascontiguousarray(tb)
        self._keep["bias_table"] = tb
        t.bias_type, t.bias_width, t.bias_penalty = int(bias_type), shape[1], float(penalty)
        t.bias_table = _ptr(tb, C.c_double)
        t.bias_rows = rows
        if bias_type == BIAS_SQUARE_HYPERPLANE:
            self._keep["bias_intercepts"] = np.ascontiguousarray(icpt)
            t.bias_intercepts = _ptr(self._keep["bias_intercepts"], C.c_double)
        else:
            self._keep.pop("bias_intercepts", None)
            t.bias_intercepts = _f64p()
        return self

    @classmethod
    def from_synth(
        cls,
        sc,
        coefs,
        feature_mode=FEATURES_INTERACTIONS,
        ewald=None,
        ewald_coef=1.0,
        mu_table=None,
        ewald_charges="auto",
        flip_table=None,
        flip_weights=None,
        swap_weight=0.1,
        sublattice_probabilities=None,
    ):
        """Build from smol_amd.synth tables (SupercellTables + CE coefficients)."""
        model = sc.model
        prim = model.prim
        its = model.cluster_interaction_tensors(coefs)
        nsp = np.array([prim.nspecies[b] for b in sc.site_b], dtype=np.int32)
        subs = []
        for b in range(prim.nb):
            sites = np.flatnonzero(sc.site_b == b)
            S = prim.nspecies[b]
            subs.append(
                dict(active_sites=sites if S > 1 else np.zeros(0, int), codes=np.arange(S))
            )
        # merge symmetry-equivalent basis sites with identical site spaces into one
        # sublattice, as Processor.get_sublattices does (processor/base.py).
        merged = {}
        for b, s in enumerate(subs):
            key = prim.labels[b]
            if key in merged:
                merged[key]["active_sites"] = np.sort(
                    np.concatenate((merged[key]["active_sites"], s["active_sites"]))
                )
            else:
                merged[key] = s
        subs = list(merged.values())
        ce_coefs = (
            np.asarray(coefs, float)
            if feature_mode == FEATURES_CORRELATIONS
            else model.orbit_multiplicities.astype(float)
        )
        return cls(
            sc.num_sites,
            sc.size,
            model.num_orbits,
            model.num_corr_functions,
            model.orbit_data(),
            tuple(sc.full_indices),
            sc.local_tables(),
            its,
            ce_coefs,
            feature_mode,
            subs,
            nspecies_per_site=nsp,
            sublattice_probabilities=sublattice_probabilities,
            ewald_inds=None if ewald is None else ewald[0],
            ewald_matrix=None if ewald is None else ewald[1],
            ewald_coef=ewald_coef,
            mu_table=mu_table,
            ewald_charges=cls._synth_charges(sc, ewald, ewald_charges),
            flip_table=flip_table,
            flip_weights=flip_weights,
            swap_weight=swap_weight,
        )

    @staticmethod
    def _synth_charges(sc, ewald, ewald_charges):
        if ewald is None or ewald_charges is None:
            return None
        if isinstance(ewald_charges, str):  # "auto": the oxidation states of the prim cell
            prim = sc.model.prim
            inds = ewald[0]
            q = np.zeros(ewald[1].shape[0])
            for s in range(sc.num_sites):
                for code in range(prim.nspecies[sc.site_b[s]]):
                    if inds[s, code] >= 0:
                        q[inds[s, code]] = prim.charges[sc.site_b[s]][code]  # vacancies have no index
            return q
        return ewald_charges


def step_rows(steps, *lead):
    """Step records for smolmc_replay / smolmc_eval_delta: an int32 array (..., 2 k) of k <= 8
    (site, code) pairs per step -- or a list of steps, each a list of (site, code) tuples as the
    reference's ushers return them (mcusher.py:104-116) -- padded with -1 to SMOLMC_STEP_ROW."""
    if isinstance(steps, (list, tuple)) and (len(steps) == 0 or isinstance(steps[0], (list, tuple))) and not (
            len(steps) and len(steps[0]) and np.isscalar(steps[0][0])):
        out = np.full((len(steps), STEP_ROW), -1, dtype=np.int32)
        for i, st in enumerate(steps):
            if len(st) > MAX_STEP_FLIPS:
                raise ValueError(f"a step of {len(st)} flips exceeds SMOLMC_MAX_STEP_FLIPS = {MAX_STEP_FLIPS}")
            for j, (site, code) in enumerate(st):
                out[i, 2 * j], out[i, 2 * j + 1] = site, code
        return out.reshape(*lead, STEP_ROW) if lead else out
    a = np.asarray(steps)
    if not np.issubdtype(a.dtype, np.integer):
        raise ValueError("Buffer dtype mismatch for steps: expected int32")
    w = a.shape[-1] if a.ndim else 0
    if lead:
        a = a.reshape(*lead, -1)
        w = a.shape[-1]
    if w == 0 or w % 2 or w > STEP_ROW:
        raise ValueError(f"step records must hold 1..{MAX_STEP_FLIPS} (site, code) pairs")
    out = np.full(a.shape[:-1] + (STEP_ROW,), -1, dtype=np.int32)
    out[..., :w] = a
    return np.ascontiguousarray(out)


def make_config(
    n_replicas,
    kernel_type=KERNEL_METROPOLIS,
    step_type=STEP_SWAP,
    device=0,
    min_enthalpy=0.0,
    max_enthalpy=1.0,
    bin_size=1.0,
    flatness=0.8,
    mod_factor=1.0,
    mod_update=2.0,
    check_period=1000,
    update_period=1,
):
    """smolmc_config with the WangLandau defaults of kernel/wanglandau.py:34-38,105."""
    c = smolmc_config()
    c.n_replicas, c.kernel_type, c.step_type, c.device = (
        int(n_replicas),
        int(kernel_type),
        int(step_type),
        int(device),
    )
    c.wl_min_enthalpy, c.wl_max_enthalpy, c.wl_bin_size = (
        float(min_enthalpy),
        float(max_enthalpy),
        float(bin_size),
    )
    c.wl_flatness, c.wl_mod_factor, c.wl_mod_divisor = (
        float(flatness),
        float(mod_factor),
        float(mod_update),
    )
    c.wl_check_period, c.wl_update_period = int(check_period), int(update_period)
    return c
