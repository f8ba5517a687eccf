"""ctypes binding of the MI355X engine (libsmolmc_hip.so, C-ABI in include/smolmc.h).

There is NO CPU fallback: if the HIP library is missing, or no AMD GPU is visible,
every entry point raises.  (The CPU oracle under oracle/ is test infrastructure and
is never imported from this package.)
"""

from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import capi
from .families import BY_NAME, FAMILIES, trace_shape

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsmolmc_hip.so")
_LIB = None

_i32p, _f64p = C.POINTER(C.c_int32), C.POINTER(C.c_double)
_u64p, _u8p, _i64p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8), C.POINTER(C.c_int64)

# every symbol include/smolmc.h declares: (name, restype, argtypes)
_HP = C.c_void_p
SYMBOLS = {
    "smolmc_create": (C.c_int, [C.POINTER(capi.smolmc_tables), C.POINTER(capi.smolmc_config), C.POINTER(_HP)]),
    "smolmc_destroy": (C.c_int, [_HP]),
    "smolmc_last_error": (C.c_char_p, []),
    "smolmc_abi_version": (C.c_int, []),
    "smolmc_num_features": (C.c_int, [_HP]),
    "smolmc_wl_num_levels": (C.c_int, [_HP]),
    "smolmc_natural_parameters": (C.c_int, [_HP, _f64p]),
    "smolmc_set_state": (C.c_int, [_HP, _i32p, _u64p, _f64p, C.c_int]),
    "smolmc_set_temperature": (C.c_int, [_HP, _f64p]),
    "smolmc_set_walker_mu": (C.c_int, [_HP, _f64p]),
    "smolmc_get_walker_mu": (C.c_int, [_HP, _f64p]),
    "smolmc_exchange_grid": (C.c_int, [_HP, C.c_int, _i32p, _f64p, _i64p]),
    "smolmc_get_state_points": (C.c_int, [_HP, _i32p, _f64p]),
    "smolmc_set_wl_windows": (C.c_int, [_HP, _f64p, _f64p]),
    "smolmc_get_wl_windows": (C.c_int, [_HP, _f64p, _f64p, _i32p]),
    "smolmc_exchange_wl": (C.c_int, [_HP, C.c_int, _i32p, _f64p, _i64p]),
    "smolmc_wl_synchronise": (C.c_int, [_HP, C.c_int, _i32p, _f64p]),
    "smolmc_resample": (C.c_int, [_HP, _i32p]),
    "smolmc_anneal_resample": (C.c_int, [_HP, C.c_int, _f64p, _u64p, _i32p, _u64p, _u64p, _f64p]),
    "smolmc_anneal_adaptive": (C.c_int, [_HP, C.c_int, C.c_double, C.c_uint32, C.c_int, _u64p, _f64p, _i32p, _i32p, _u64p, _u64p, _f64p]),
    "smolmc_get_state": (C.c_int, [_HP, _i32p, _f64p, _f64p, _u64p, _u64p, _u8p]),
    "smolmc_get_wl": (C.c_int, [_HP, _f64p, _i64p, _i64p, _f64p, _f64p]),
    "smolmc_set_wl": (C.c_int, [_HP, _f64p, _i64p, _i64p, _f64p, _f64p]),
    "smolmc_set_counters": (C.c_int, [_HP, _u64p, _u64p]),
    "smolmc_get_bias": (C.c_int, [_HP, _f64p]),
    "smolmc_kernel_info": (C.c_int, [_HP, C.c_char_p, C.c_int]),
    "smolmc_run": (C.c_int, [_HP, C.c_int64]),
    "smolmc_sync": (C.c_int, [_HP]),
    "smolmc_run_sampled": (C.c_int, [_HP, C.c_int64, C.c_int64, C.c_int]),
    "smolmc_pending_samples": (C.c_int, [_HP, C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    "smolmc_discard_samples": (C.c_int, [_HP]),
    "smolmc_get_samples": (C.c_int, [_HP, _f64p, _f64p, _u8p, _i32p]),
    "smolmc_get_samples_u8": (C.c_int, [_HP, _f64p, _f64p, _u8p, _u8p]),
    "smolmc_get_samples_ex": (C.c_int, [_HP, _f64p, _f64p, _u8p, _u8p, _f64p, _f64p, _i64p, _i64p, _f64p, _f64p]),
    "smolmc_set_observables": (C.c_int, [_HP, C.POINTER(capi.smolmc_observables)]),
    "smolmc_observables_shape": (C.c_int, [_HP, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "smolmc_eval_observables": (C.c_int, [_HP, _i32p, C.c_int, _i32p, _i32p]),
    "smolmc_get_sample_observables": (C.c_int, [_HP, _i32p, _i32p]),
    "smolmc_set_minima": (C.c_int, [_HP, C.POINTER(capi.smolmc_minima)]),
    "smolmc_minima_shape": (C.c_int, [_HP, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "smolmc_update_minima": (C.c_int, [_HP]),
    "smolmc_reset_minima": (C.c_int, [_HP]),
    "smolmc_get_minima": (C.c_int, [_HP, _f64p, _f64p, _f64p, _i32p, _i32p, _i32p, _i64p, _u64p]),
    "smolmc_get_minima_companions": (C.c_int, [_HP, _i32p]),
    "smolmc_set_statistics": (C.c_int, [_HP, C.POINTER(capi.smolmc_statistics)]),
    "smolmc_set_statistics_binned": (C.c_int, [_HP, C.POINTER(capi.smolmc_statistics), C.c_int, C.c_int, C.c_double, C.c_double]),
    "smolmc_statistics_bins": (C.c_int, [_HP, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                         C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "smolmc_statistics_shape": (C.c_int, [_HP] + [C.POINTER(C.c_int)] * 4),
    "smolmc_update_statistics": (C.c_int, [_HP]),
    "smolmc_reset_statistics": (C.c_int, [_HP]),
    "smolmc_get_statistics": (C.c_int, [_HP, _i64p, _f64p, _f64p, _f64p, _u64p, _f64p, _f64p, _i64p, _i64p, _i64p, _i64p]),
    "smolmc_set_statistics_sites": (C.c_int, [_HP, _i32p, C.c_int, C.c_int]),
    "smolmc_statistics_sites_shape": (C.c_int, [_HP, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "smolmc_get_statistics_sites": (C.c_int, [_HP, _i64p, _i64p]),
    "smolmc_set_statistics_joint": (C.c_int, [_HP, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_double, C.c_double]),
    "smolmc_statistics_joint_shape": (C.c_int, [_HP] + [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double),
                                                        C.POINTER(C.c_double)] * 2),
    "smolmc_get_statistics_joint": (C.c_int, [_HP, _i64p, _i64p]),
    "smolmc_set_structure": (C.c_int, [_HP, C.POINTER(capi.smolmc_structure)]),
    "smolmc_structure_shape": (C.c_int, [_HP] + [C.POINTER(C.c_int)] * 3),
    "smolmc_eval_structure": (C.c_int, [_HP, _i32p, C.c_int, _i64p, _f64p]),
    "smolmc_get_sample_structure": (C.c_int, [_HP, _i64p, _f64p]),
    "smolmc_set_connectivity": (C.c_int, [_HP, C.POINTER(capi.smolmc_connectivity)]),
    "smolmc_set_connectivity_gated": (C.c_int, [_HP, C.POINTER(capi.smolmc_connectivity), C.POINTER(capi.smolmc_conn_gates)]),
    "smolmc_connectivity_shape": (C.c_int, [_HP] + [C.POINTER(C.c_int)] * 2),
    "smolmc_connectivity_gates": (C.c_int, [_HP, C.POINTER(C.c_int), C.POINTER(C.c_int64)]),
    "smolmc_eval_connectivity": (C.c_int, [_HP, _i32p, C.c_int, _i64p, _i32p]),
    "smolmc_get_sample_connectivity": (C.c_int, [_HP, _i64p]),
    "smolmc_set_patterns": (C.c_int, [_HP, C.POINTER(capi.smolmc_patterns)]),
    "smolmc_patterns_shape": (C.c_int, [_HP] + [C.POINTER(C.c_int)] * 2),
    "smolmc_eval_patterns": (C.c_int, [_HP, _i32p, C.c_int, _i32p]),
    "smolmc_get_sample_patterns": (C.c_int, [_HP, _i32p]),
    "smolmc_set_environments": (C.c_int, [_HP, C.POINTER(capi.smolmc_environments)]),
    "smolmc_environments_shape": (C.c_int, [_HP] + [C.POINTER(C.c_int)] * 3),
    "smolmc_eval_environments": (C.c_int, [_HP, _i32p, C.c_int, _i32p, _i32p]),
    "smolmc_get_sample_environments": (C.c_int, [_HP, _i32p]),
    "smolmc_replay": (C.c_int, [_HP, C.c_int64, _i32p, _f64p, _f64p, _u8p, _f64p, _f64p]),
    "smolmc_last_kernel_ms": (C.c_int, [_HP, C.POINTER(C.c_float)]),
    "smolmc_eval_full": (C.c_int, [_HP, _i32p, C.c_int, _f64p]),
    "smolmc_eval_delta": (C.c_int, [_HP, _i32p, _i32p, C.c_int, _f64p]),
    "smolmc_set_stream": (C.c_int, [_HP, C.c_void_p]),
    "smolmc_export_enthalpy_dev": (C.c_int, [_HP, C.c_void_p]),
    "smolmc_import_temperature_dev": (C.c_int, [_HP, C.c_void_p]),
    "smolmc_create_distance": (C.c_int, [C.POINTER(capi.smolmc_tables), C.POINTER(capi.smolmc_distance),
                                         C.POINTER(capi.smolmc_config), C.POINTER(_HP)]),
    "smolmc_get_best": (C.c_int, [_HP, _f64p, _f64p, _i32p, _u64p]),
    "smolmc_reset_best": (C.c_int, [_HP]),
    "smolmc_exchange_dev": (C.c_int, [_HP, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}


def source_digest(root=None):
    """sha256 over the kernel sources (smol_amd/csrc/*.h, *.hip, Makefile and include/smolmc.h, by
    sorted name) of the repository at ``root`` (default: this one).  profiles/pmc_constants.json
    carries the digest of the tree its counters were collected on, next to the per-kernel machine-code
    digest (codeobj.py) that bench.py compares: this one names the tree, that one says whether the
    kernel an entry was measured on is still the kernel that runs."""
    import glob
    import hashlib

    h = hashlib.sha256()
    here = _HERE if root is None else os.path.join(root, "smol_amd")
    src = os.path.join(here, "csrc")
    files = sorted(glob.glob(os.path.join(src, "*.h")) + glob.glob(os.path.join(src, "*.hip")))
    files += [os.path.join(src, "Makefile"), os.path.join(os.path.dirname(here), "include", "smolmc.h")]
    for f in files:
        h.update(os.path.basename(f).encode() + b"\0")
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


def load_library(path=None):
    """Load libsmolmc_hip.so; raises RuntimeError when it has not been built."""
    global _LIB
    if _LIB is not None and path is None:
        return _LIB
    p = path or os.environ.get("SMOLMC_LIB") or LIB_PATH  # SMOLMC_LIB: A/B builds of the kernels
    if not os.path.exists(p):
        raise RuntimeError(
            f"{p} not found: build the HIP engine first (python -c 'import __graft_entry__ as g; "
            "g.build()' or make -C smol_amd/csrc). smol_amd has no CPU fallback."
        )
    # One HIP runtime per process.  PyTorch's wheel bundles a libamdhip64 with the same soname as
    # /opt/rocm's; whichever is mapped first serves both, and torch finds "No HIP GPUs" when the
    # system copy got in before it (engine created first, torch imported later for a collective
    # or a stream).  So when torch is installed it is imported before the engine library.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(p)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype, fn.argtypes = res, args
    if lib.smolmc_abi_version() != capi.ABI_VERSION:
        raise RuntimeError("smolmc ABI version mismatch")
    if path is None:
        _LIB = lib
    return lib


def _p(a, ct):
    return None if a is None else a.ctypes.data_as(C.POINTER(ct))


def chemical_work(tables, occupancies, mu_rows):
    """The chemical-work feature (the last one of a semigrand model) on the host: sum over the active sites of
    mu[sublattice][species code], for occupancies (n, N) and rows (n, n_sublattices, mu_width) in the layout of
    smolmc_set_walker_mu."""
    occ = np.asarray(occupancies).reshape(-1, tables.struct.num_sites)
    sites_of = tables.active_sites()
    rows = np.asarray(mu_rows, dtype=np.float64).reshape(len(occ), len(sites_of), -1)
    out = np.zeros(len(occ))
    for k, sites in enumerate(sites_of):
        out += np.take_along_axis(rows[:, k, :], occ[:, sites].astype(np.int64), axis=1).sum(axis=1)
    return out


def species_counts(tables, occupancies, width=None):
    """Species counts per (active sublattice, species code), (n, n_sublattices, width) int64, of occupancies (n, N):
    the n(x) of the chemical work n(x) . mu (``width`` defaults to the tables' mu_width)."""
    occ = np.asarray(occupancies).reshape(-1, tables.struct.num_sites)
    sites_of = tables.active_sites()
    W = int(tables.struct.mu_width if width is None else width)
    out = np.zeros((len(occ), len(sites_of), W), dtype=np.int64)
    for k, sites in enumerate(sites_of):
        sub = occ[:, sites]
        for c in range(W):
            out[:, k, c] = (sub == c).sum(axis=1)
    return out


# the keywords of ``run_sampled`` / ``run_sampled_async`` and the SMOLMC_SAMPLE_* flag each one sets
SAMPLE_FLAGS = (("occupancy", capi.SAMPLE_OCCUPANCY), ("bias", capi.SAMPLE_BIAS), ("wl", capi.SAMPLE_WL),
                ("minima", capi.SAMPLE_MINIMA), ("statistics", capi.SAMPLE_STATISTICS)
                ) + tuple((fam.run_keyword, fam.flag) for fam in FAMILIES)
_CTYPE = {np.dtype(np.int32): C.c_int32, np.dtype(np.int64): C.c_int64, np.dtype(np.float64): C.c_double}


class EngineError(RuntimeError):
    pass


class RingFullError(EngineError):
    """smolmc_run_sampled refused a block: both ring slots hold blocks that were not fetched."""


class Engine:
    """One engine handle = R walkers of one ensemble on one GPU."""

    def __init__(self, tables: capi.TableSet, config: capi.smolmc_config, distance: capi.DistanceSpec = None):
        self._lib = load_library()
        self.tables, self.config, self.distance = tables, config, distance
        self._h = _HP()
        if distance is None:
            rc = self._lib.smolmc_create(C.byref(tables.struct), C.byref(config), C.byref(self._h))
        else:  # a distance-objective handle (smolmc_create_distance)
            rc = self._lib.smolmc_create_distance(C.byref(tables.struct), C.byref(distance.struct), C.byref(config),
                                                  C.byref(self._h))
        if rc:
            self._h = None
            self._chk(rc)
        # (scattered active sites -- restricted sites, sublattices split by species -- are renumbered INSIDE
        # smolmc_create since ABI 8, `kernel_info` says "relabelled=1": occupancies and step records cross the C-ABI
        # in the caller's numbering, nothing is translated here)
        self.R = config.n_replicas
        self.N = tables.struct.num_sites
        self.F = self._lib.smolmc_num_features(self._h)
        self.L = self._lib.smolmc_wl_num_levels(self._h)
        self.walker_mu_set = False  # per-walker chemical potentials in force (set_walker_mu)
        self.minima_spec = None     # the spec of the minima record in force (set_minima)
        self.statistics_spec = None  # the spec of the statistics record in force (set_statistics)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.smolmc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc:
            msg = self._lib.smolmc_last_error().decode()
            if rc == capi.ERR_RING_FULL:
                raise RingFullError(msg)
            # argument problems are ValueErrors like the reference's (expansion.py:97-103,
            # wanglandau.py:80-88); device problems are RuntimeErrors
            if any(k in msg for k in ("enthalpy", "mod_factor", "range", "must be", "larger")):
                raise ValueError(msg)
            raise EngineError(msg)

    @staticmethod
    def _occ32(occ, shape):
        occ = np.asarray(occ)
        if occ.dtype != np.int32:
            if not np.issubdtype(occ.dtype, np.integer):
                raise ValueError(
                    f"occupancy dtype is: {occ.dtype}, but should be integers!"
                )  # expansion.py:225-228
            occ = occ.astype(np.int32)
        return np.ascontiguousarray(occ).reshape(shape)

    # ---- state ----------------------------------------------------------------
    @property
    def natural_parameters(self):
        out = np.zeros(self.F)
        self._chk(self._lib.smolmc_natural_parameters(self._h, _p(out, C.c_double)))
        return out

    def set_state(self, occupancies, seeds=None, temperature=None, reset_aux=True):
        occ = self._occ32(occupancies, (self.R, self.N))
        seeds = (
            np.arange(self.R, dtype=np.uint64)
            if seeds is None
            else np.ascontiguousarray(seeds, dtype=np.uint64)
        )
        if len(seeds) != self.R:
            raise ValueError("Number of seeds does not match number of kernels!")  # sampler.py:107
        temp = np.ascontiguousarray(
            np.broadcast_to(np.asarray(1.0 if temperature is None else temperature, float), (self.R,))
        )
        self._chk(
            self._lib.smolmc_set_state(
                self._h, _p(occ, C.c_int32), _p(seeds, C.c_uint64), _p(temp, C.c_double), int(reset_aux)
            )
        )

    def set_temperature(self, temperature):
        temp = np.ascontiguousarray(np.broadcast_to(np.asarray(temperature, float), (self.R,)))
        self._chk(self._lib.smolmc_set_temperature(self._h, _p(temp, C.c_double)))

    # ---- per-walker chemical potentials ---------------------------------------------
    def _mu_shape(self):
        return (self.R, self.tables.struct.n_sublattices, self.tables.struct.mu_width)

    def set_walker_mu(self, rows):
        """Chemical potentials of every walker (smolmc_set_walker_mu): ``rows`` (R, n_sublattices, mu_width) -- the
        active sublattices in the tables' order, the columns the species codes as in the tables' ``mu_table`` -- or
        None for the table the handle was created with.  Chemical work and enthalpy of every walker are re-priced on
        the device from its current occupancy; between two ``run`` calls this is a mu sweep."""
        if rows is not None:
            rows = np.ascontiguousarray(rows, dtype=np.float64)
            if rows.shape != self._mu_shape():
                raise ValueError(f"expected chemical potentials of shape {self._mu_shape()} "
                                 f"(walkers, active sublattices, mu_width), got {rows.shape}")
        self._chk(self._lib.smolmc_set_walker_mu(self._h, _p(rows, C.c_double)))
        self.walker_mu_set = rows is not None

    def get_walker_mu(self):
        """(R, n_sublattices, mu_width): every walker's current row -- those of the last ``set_walker_mu``, moved by the
        exchanges of ``exchange_grid`` since -- the create-time rows when none are set."""
        out = np.zeros(self._mu_shape())
        self._chk(self._lib.smolmc_get_walker_mu(self._h, _p(out, C.c_double)))
        return out

    def _exchange_pairs(self, fn, pairs, log_u, stats):
        """The call both pair exchanges make: disjoint ``pairs`` (npairs, 2), one ``log_u`` per pair, ``stats`` or None."""
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        log_u = np.ascontiguousarray(log_u, dtype=np.float64).reshape(-1)
        if len(log_u) != len(pairs):
            raise ValueError(f"expected one log_u per pair: {len(pairs)} pairs, {len(log_u)} values")
        if stats is not None and not (isinstance(stats, np.ndarray) and stats.dtype == np.int64 and stats.flags.c_contiguous
                                      and stats.shape == (len(pairs), 2)):
            raise ValueError(f"stats must be a C-contiguous int64 array of shape ({len(pairs)}, 2)")
        self._chk(fn(self._h, len(pairs), _p(pairs, C.c_int32), _p(log_u, C.c_double), _p(stats, C.c_int64)))

    def exchange_grid(self, pairs, log_u, stats=None):
        """One exchange attempt across the mu-T grid, decided and applied on the device (smolmc_exchange_grid): for
        every pair (s, t) of ``pairs`` (npairs, 2) the walkers at the state points s and t swap temperature and row
        together when the move is accepted against ``log_u`` (npairs).  ``stats`` (npairs, 2) int64, when given, gains
        the attempts in column 0 and the acceptances in column 1 (this waits for the kernel); without it the call only
        queues work on the handle's stream."""
        self._exchange_pairs(self._lib.smolmc_exchange_grid, pairs, log_u, stats)

    def state_points(self):
        """(point_of (R,) int32, temperature (R,)): the state point every walker is at after the exchanges so far, and
        that point's temperature as it was set (smolmc_get_state_points)."""
        point_of, temp = np.empty(self.R, dtype=np.int32), np.empty(self.R)
        self._chk(self._lib.smolmc_get_state_points(self._h, _p(point_of, C.c_int32), _p(temp, C.c_double)))
        return point_of, temp

    # ---- per-walker Wang-Landau windows -----------------------------------------------
    def set_wl_windows(self, vmin, vmax):
        """Per-walker energy windows of a Wang-Landau handle (smolmc_set_wl_windows): walker r samples
        ``[vmin[r], vmax[r])`` with the handle's bin size; every window must give the handle's ``L`` by the rule
        ``ceil((vmax - vmin) / bin_size)``.  Estimator e is the window and density-of-states copy walker e holds after
        this call; ``get_wl`` / ``set_wl`` are in estimator order.  ``None, None`` returns to the config's window."""
        if (vmin is None) != (vmax is None):
            raise ValueError("vmin and vmax are given together, or both None")
        if vmin is not None:
            vmin = np.ascontiguousarray(vmin, dtype=np.float64).reshape(-1)
            vmax = np.ascontiguousarray(vmax, dtype=np.float64).reshape(-1)
            if len(vmin) != self.R or len(vmax) != self.R:
                raise ValueError(f"expected one window per walker: {self.R} walkers, {len(vmin)} / {len(vmax)} values")
        self._chk(self._lib.smolmc_set_wl_windows(self._h, _p(vmin, C.c_double), _p(vmax, C.c_double)))

    def wl_windows(self):
        """(vmin (R,), vmax (R,), estimator_of (R,) int32): the window every walker holds now and the estimator it
        belongs to (smolmc_get_wl_windows); the config's window and the identity while no windows are set."""
        vmin, vmax, est = np.empty(self.R), np.empty(self.R), np.empty(self.R, dtype=np.int32)
        self._chk(self._lib.smolmc_get_wl_windows(self._h, _p(vmin, C.c_double), _p(vmax, C.c_double), _p(est, C.c_int32)))
        return vmin, vmax, est

    def exchange_wl(self, pairs, log_u, stats=None):
        """One replica-exchange attempt between energy windows, decided and applied on the device
        (smolmc_exchange_wl): for every pair (s, t) of ``pairs`` (npairs, 2) the walkers that hold the estimators s and
        t swap them when both enthalpies lie in both windows and the move is accepted against ``log_u`` (npairs).
        ``stats`` as in ``exchange_grid``."""
        self._exchange_pairs(self._lib.smolmc_exchange_wl, pairs, log_u, stats)

    def wl_synchronise(self, copies, fetch=True):
        """One merge attempt of the copies of every window on the device (smolmc_wl_synchronise): group g is the
        estimators g * copies .. g * copies + copies - 1.  A group whose copies have one modification factor and are all
        flat takes the mean of their entropies in every copy, empty histograms and the factor divided by the config's
        divisor (``parallel.WLWindows.synchronise`` is the definition).  Valid on every Wang-Landau handle created with
        check period 0, with or without per-walker windows.  Returns dict(status (R / copies,) int32: 0 not all flat, 1
        merged, 2 factors differ; mod_factor (R / copies,): the groups' factors after the call) -- or None with
        ``fetch=False``, when the call only queues work on the handle's stream."""
        copies = int(copies)
        groups = self.R // copies if copies >= 1 and self.R % copies == 0 else 0  # (else: the call refuses and says why)
        out = dict(status=np.empty(groups, dtype=np.int32), mod_factor=np.empty(groups)) if fetch else None
        self._chk(self._lib.smolmc_wl_synchronise(self._h, copies, _p(out["status"], C.c_int32) if out else None,
                                                  _p(out["mod_factor"], C.c_double) if out else None))
        return out

    # ---- population annealing ------------------------------------------------------------
    def resample(self, parent):
        """Clone walkers by an explicit map on the device (smolmc_resample): slot m takes the state of slot
        ``parent[m]`` -- occupancy, features, enthalpy, accepted flag, bias, Ewald field.  Every source must map to
        itself; counters, seeds and temperatures stay with the slot.  Queued on the handle's stream."""
        parent = np.ascontiguousarray(parent, dtype=np.int32).reshape(-1)
        if len(parent) != self.R:
            raise ValueError(f"expected one parent per walker: {self.R} walkers, {len(parent)} entries")
        self._chk(self._lib.smolmc_resample(self._h, _p(parent, C.c_int32)))

    def anneal_resample(self, temperatures, offset_words, npop=1, outputs=True):
        """One population-annealing step on the device (smolmc_anneal_resample): the ``npop`` populations (equal
        blocks of slots) go to ``temperatures`` (npop,), are reweighted, resampled with one ``offset_words`` (npop,)
        uint64 each and cloned; the new temperatures are in force afterwards.  Returns dict(parent (R,) int32 slot
        numbers, q (R,) uint64, qsum (npop,) uint64, href (npop,)) -- or None with ``outputs=False``, when the call
        only queues work on the handle's stream."""
        npop = int(npop)
        temp = np.ascontiguousarray(np.broadcast_to(np.asarray(temperatures, float), (npop,)))
        words = np.ascontiguousarray(offset_words, dtype=np.uint64).reshape(-1)
        if len(words) != npop:
            raise ValueError(f"expected one offset word per population: {npop} populations, {len(words)} words")
        out = None
        if outputs:
            out = dict(parent=np.empty(self.R, dtype=np.int32), q=np.empty(self.R, dtype=np.uint64),
                       qsum=np.empty(npop, dtype=np.uint64), href=np.empty(npop))
        self._chk(self._lib.smolmc_anneal_resample(
            self._h, npop, _p(temp, C.c_double), _p(words, C.c_uint64),
            _p(out["parent"], C.c_int32) if out else None, _p(out["q"], C.c_uint64) if out else None,
            _p(out["qsum"], C.c_uint64) if out else None, _p(out["href"], C.c_double) if out else None))
        return out

    def anneal_adaptive(self, temperature_limit, overlap, offset_words, npop=1, n_iter=16):
        """One population-annealing step whose temperature the device chooses (smolmc_anneal_adaptive): the largest
        step from the populations' common temperature towards ``temperature_limit`` that keeps the overlap of the energy
        histograms at ``overlap`` in (0, 1) (the word t = int(overlap 2^32) decides), found with at most ``n_iter``
        bisections per population; then the step of ``anneal_resample`` to that temperature.  Returns its dict plus
        ``temperature`` (in force afterwards), ``reached`` (it is the limit) and ``forced`` (the target was not met at
        the resolution of the search)."""
        npop = int(npop)
        words = np.ascontiguousarray(offset_words, dtype=np.uint64).reshape(-1)
        if len(words) != npop:
            raise ValueError(f"expected one offset word per population: {npop} populations, {len(words)} words")
        t = int(float(overlap) * 2 ** 32)
        if not 0 <= t < 2 ** 32:
            raise ValueError(f"the target overlap must lie in (0, 1): {overlap}")
        out = dict(parent=np.empty(self.R, dtype=np.int32), q=np.empty(self.R, dtype=np.uint64),
                   qsum=np.empty(npop, dtype=np.uint64), href=np.empty(npop))
        temp, flags = np.empty(1), np.empty(1, dtype=np.int32)
        self._chk(self._lib.smolmc_anneal_adaptive(
            self._h, npop, float(temperature_limit), t, int(n_iter), _p(words, C.c_uint64), _p(temp, C.c_double),
            _p(flags, C.c_int32), _p(out["parent"], C.c_int32), _p(out["q"], C.c_uint64), _p(out["qsum"], C.c_uint64),
            _p(out["href"], C.c_double)))
        out.update(temperature=float(temp[0]), reached=bool(flags[0] & 1), forced=bool(flags[0] & 2))
        return out

    def species_counts(self, occupancies):
        """Species counts per (active sublattice, code) of occupancies (n, N), in the layout of ``set_walker_mu``."""
        return species_counts(self.tables, self._occ32(occupancies, (-1, self.N)))

    def chemical_work(self, occupancies, mu_rows):
        """The last feature of a semigrand handle, on the host: sum over the active sites of mu[sublattice][species
        code] for occupancies (n, N) and rows (n, n_sublattices, mu_width) -- what ``set_walker_mu`` prices on the
        device (``eval_full`` keeps the create-time table)."""
        return chemical_work(self.tables, self._occ32(occupancies, (-1, self.N)), mu_rows)

    def get_state(self, occupancy=True):
        occ = np.empty((self.R, self.N), dtype=np.int32) if occupancy else None
        feat = np.empty((self.R, self.F))
        H = np.empty(self.R)
        na = np.empty(self.R, dtype=np.uint64)
        ns = np.empty(self.R, dtype=np.uint64)
        la = np.empty(self.R, dtype=np.uint8)
        self._chk(
            self._lib.smolmc_get_state(
                self._h, _p(occ, C.c_int32), _p(feat, C.c_double), _p(H, C.c_double),
                _p(na, C.c_uint64), _p(ns, C.c_uint64), _p(la, C.c_uint8),
            )
        )
        return dict(occupancy=occ, features=feat, enthalpy=H, n_accepted=na, n_steps=ns,
                    accepted=la.astype(bool))

    def get_best(self):
        """Distance handles: per walker the lowest enthalpy seen, its distance features, occupancy and step."""
        score = np.empty(self.R)
        feat = np.empty((self.R, self.F))
        occ = np.empty((self.R, self.N), dtype=np.int32)
        step = np.empty(self.R, dtype=np.uint64)
        self._chk(self._lib.smolmc_get_best(self._h, _p(score, C.c_double), _p(feat, C.c_double),
                                            _p(occ, C.c_int32), _p(step, C.c_uint64)))
        return dict(score=score, features=feat, occupancy=occ, step=step)

    def reset_best(self):
        self._chk(self._lib.smolmc_reset_best(self._h))

    def get_enthalpy(self):
        """Current enthalpy of every walker (one device-to-host copy; the replica-exchange loop
        needs nothing else of the state)."""
        H = np.zeros(self.R)
        self._chk(self._lib.smolmc_get_state(self._h, None, None, _p(H, C.c_double), None, None, None))
        return H

    def get_wl(self):
        # (np.empty: every array is overwritten by the copy; zero-filling 40 MB per call showed in the
        # Sampler's per-sample Wang-Landau trace)
        S = np.empty((self.R, self.L))
        hist = np.empty((self.R, self.L), dtype=np.int64)
        occ = np.empty((self.R, self.L), dtype=np.int64)
        mf = np.empty((self.R, self.L, self.F))
        m = np.empty(self.R)
        self._chk(
            self._lib.smolmc_get_wl(
                self._h, _p(S, C.c_double), _p(hist, C.c_int64), _p(occ, C.c_int64),
                _p(mf, C.c_double), _p(m, C.c_double),
            )
        )
        return dict(entropy=S, histogram=hist, occurrences=occ, mean_features=mf, mod_factor=m)

    def set_wl(self, entropy=None, histogram=None, occurrences=None, mean_features=None, mod_factor=None):
        """Upload Wang-Landau aux arrays (the inverse of get_wl; None = keep what the device has)."""
        def arr(x, dt, shape):
            if x is None:
                return None
            x = np.ascontiguousarray(x, dtype=dt)
            if x.shape != shape:
                raise ValueError(f"expected an array of shape {shape}, got {x.shape}")
            return x

        RL = (self.R, self.L)
        S, hist, occ = arr(entropy, np.float64, RL), arr(histogram, np.int64, RL), arr(occurrences, np.int64, RL)
        mf, m = arr(mean_features, np.float64, RL + (self.F,)), arr(mod_factor, np.float64, (self.R,))
        self._chk(self._lib.smolmc_set_wl(self._h, _p(S, C.c_double), _p(hist, C.c_int64), _p(occ, C.c_int64),
                                          _p(mf, C.c_double), _p(m, C.c_double)))

    def set_counters(self, n_steps=None, n_accepted=None):
        """Step / accept counters of every walker (n_steps is the position in the random stream)."""
        ns = None if n_steps is None else np.ascontiguousarray(n_steps, dtype=np.uint64)
        na = None if n_accepted is None else np.ascontiguousarray(n_accepted, dtype=np.uint64)
        for x in (ns, na):
            if x is not None and x.shape != (self.R,):
                raise ValueError(f"expected {self.R} counters")
        self._chk(self._lib.smolmc_set_counters(self._h, _p(ns, C.c_uint64), _p(na, C.c_uint64)))

    def audit_drift(self):
        """Drift of the running trace against a from-scratch evaluation of the current
        occupancies (the batched full-vector kernel, evaluator.pyx:121-209): returns
        (max |features - recomputed|, max |enthalpy - natural_parameters . recomputed|).
        The reference bounds the analogous per-flip drift in tests/test_moca/test_processor.py
        :170-172; here it is the accumulated value after any number of steps."""
        st = self.get_state()
        full = self.eval_full(st["occupancy"])
        df = float(np.max(np.abs(st["features"] - full)))
        dh = float(np.max(np.abs(st["enthalpy"] - full @ self.natural_parameters)))
        return df, dh

    def kernel_info(self):
        """Kernel family this handle dispatches to, e.g. 'lean nslot=2 mm=2 field=0 lds=19968'; for a model on
        ``mc_kernel`` / the universal kernel the string ends with ' | not lean: <the first condition that failed>'."""
        buf = C.create_string_buffer(512)
        self._chk(self._lib.smolmc_kernel_info(self._h, buf, 512))
        return buf.value.decode()

    def not_lean_reason(self):
        """Why the model runs on ``mc_kernel`` / the universal kernel instead of a lean family: the first condition that
        failed at ``smolmc_create`` (None on a lean handle)."""
        info = self.kernel_info()
        return info.split(" | not lean: ", 1)[1] if " | not lean: " in info else None

    def get_bias(self):
        """trace.bias of every walker (models created with an MCBias term)."""
        b = np.zeros(self.R)
        self._chk(self._lib.smolmc_get_bias(self._h, _p(b, C.c_double)))
        return b

    # ---- hot path -------------------------------------------------------------
    def run(self, nsteps, sync=False):
        self._chk(self._lib.smolmc_run(self._h, int(nsteps)))
        if sync:
            self.sync()

    def sync(self):
        self._chk(self._lib.smolmc_sync(self._h))

    def _set_spec(self, fn, spec, defined_on=None, *shape):
        """The call every ``set_*`` makes: ``fn(handle, struct of spec)``, or ``fn(handle, NULL)`` for None.  A spec that
        names its sites (``defined_on``: the words of the message) must have the handle's number; ``shape``: what the
        spec's ``c_struct`` takes."""
        if spec is None:
            self._chk(fn(self._h, None))
            return
        if defined_on is not None and spec.num_sites != self.N:
            raise ValueError(f"{defined_on} defined on {spec.num_sites} sites, the handle has {self.N}")
        struct, keep = spec.c_struct(*shape)
        self._chk(fn(self._h, C.byref(struct)))
        del keep

    def _kernel_ms(self, hook, n=1):
        """The ``n`` floats of a ``smolmc_debug_*_kernel_ms`` hook of the library: one as a float, several as a list."""
        fn = getattr(self._lib, hook)
        fn.restype, fn.argtypes = C.c_int, [_HP, C.POINTER(C.c_float)]
        ms = (C.c_float * n)()
        self._chk(fn(self._h, ms))
        return float(ms[0]) if n == 1 else [float(x) for x in ms]

    # ---- the per-sample families (families.FAMILIES): what their public methods below share ---------------------------
    def _family_sizes(self, fam):
        """What ``smolmc_<stem>_shape`` gives, by the names of ``fam.sizes``: zeros when no spec is set."""
        v = [C.c_int() for _ in fam.sizes]
        self._chk(getattr(self._lib, f"smolmc_{fam.stem}_shape")(self._h, *[C.byref(x) for x in v]))
        return {name: int(x.value) for name, x in zip(fam.sizes, v)}

    def _set_family(self, fam, spec):
        """``smolmc_set_<stem>``; a spec that rests on another family must map that family's kinds in force."""
        if spec is not None and fam.rests_on is not None:
            K = self._family_sizes(BY_NAME[fam.rests_on])["n_kinds"]
            if spec.n_kinds != K:
                raise ValueError(f"{fam.noun} maps {spec.n_kinds} kinds, the {fam.rests_on} in force have {K} "
                                 f"(call set_{fam.rests_on} first)")
        self._set_spec(getattr(self._lib, f"smolmc_set_{fam.stem}"), spec, f"{fam.noun} {fam.verb}")

    @staticmethod
    def _family_arrays(fam, lead, sizes, make):
        """One array per trace of ``fam``, ``lead`` + the trace's shape, from ``make`` (np.zeros, np.empty)."""
        return [make(lead + trace_shape(dims, sizes), dtype=dtype) for _, dtype, dims in fam.traces]

    def _eval_family(self, fam, occupancies, extra=None):
        """``smolmc_eval_<stem>`` on occupancies (n, N), or on the walkers' current states: the traces of ``fam`` as a list
        of arrays (n, ...).  Where the call takes one more pointer, ``extra(n, sizes)`` gives its int32 array, or None for
        NULL; it is the last entry of the list."""
        sizes = self._family_sizes(fam)
        occ = None if occupancies is None else self._occ32(occupancies, (-1, self.N))
        n = self.R if occ is None else len(occ)
        out = self._family_arrays(fam, (n,), sizes, np.zeros)
        more = [] if extra is None else [extra(n, sizes)]
        self._chk(getattr(self._lib, f"smolmc_eval_{fam.stem}")(
            self._h, _p(occ, C.c_int32), n, *[_p(a, _CTYPE[a.dtype]) for a in out], *[_p(a, C.c_int32) for a in more]))
        return out + more

    def _sample_family(self, fam):
        """``smolmc_get_sample_<stem>``: the traces of ``fam``, (ns, R, ...) each, of the block ``fetch_samples`` would
        deliver next."""
        sizes = self._family_sizes(fam)
        _, ns, _ = self.pending_samples()
        out = self._family_arrays(fam, (ns, self.R), sizes, np.empty)
        self._chk(getattr(self._lib, f"smolmc_get_sample_{fam.stem}")(self._h, *[_p(a, _CTYPE[a.dtype]) for a in out]))
        return out

    # ---- observables: kind and pair counts on the device ----------------------------------
    def set_observables(self, obs):
        """The observables of this handle (smolmc_set_observables): an ``observables.Observables`` in the caller's site
        numbering, or None to remove them.  The engine copies and uploads; it refuses, naming the reason, a bond out
        of range, a kind beyond ``n_kinds``, more cells than ``capi.MAX_OBS_CELLS`` and a row too long for LDS."""
        self._set_family(BY_NAME["observables"], obs)

    def observables_shape(self):
        """(n_kinds, n_shells) in force, (0, 0) when none are set (smolmc_observables_shape)."""
        return tuple(self._family_sizes(BY_NAME["observables"]).values())

    def observables(self, occupancies=None):
        """(counts (n, K) int32, pairs (n, n_shells, K, K) int32) of occupancies (n, N) evaluated on the device
        (smolmc_eval_observables), or, with None, of the walkers' current states (n = R)."""
        return tuple(self._eval_family(BY_NAME["observables"], occupancies))

    def sample_observables(self):
        """(species_counts (ns, R, K), pair_counts (ns, R, n_shells, K, K)) of the block ``fetch_samples`` would
        deliver next; the block stays undelivered (smolmc_get_sample_observables)."""
        return tuple(self._sample_family(BY_NAME["observables"]))

    def observables_kernel_ms(self):
        """Device time of the last launch of the observables kernel in ms (HIP events; a measuring hook of the library,
        not part of the C-ABI)."""
        return self._kernel_ms("smolmc_debug_obs_kernel_ms")

    # ---- minima: the lowest recorded states, kept on the device ----------------------------
    def set_minima(self, spec):
        """The minima record of this handle (smolmc_set_minima): a ``minima.Minima``, or None to remove it.  A new spec
        starts an empty record.  The record lives as long as the handle: ``set_state`` and ``discard_samples`` leave it
        alone."""
        self._set_spec(self._lib.smolmc_set_minima, spec)
        self.minima_spec = spec

    def minima_shape(self):
        """(n_slots, n_axes) in force, (0, 0) when no record is set (smolmc_minima_shape)."""
        n, a = C.c_int(), C.c_int()
        self._chk(self._lib.smolmc_minima_shape(self._h, C.byref(n), C.byref(a)))
        return int(n.value), int(a.value)

    def update_minima(self):
        """Offer the walkers' current states to the record, one offer (smolmc_update_minima): for callers of ``run``."""
        self._chk(self._lib.smolmc_update_minima(self._h))

    def reset_minima(self):
        """Empty the record; the offer numbering restarts (smolmc_reset_minima)."""
        self._chk(self._lib.smolmc_reset_minima(self._h))

    def minima(self):
        """The record as a ``minima.MinimaRecord`` (smolmc_get_minima; waits for the handle's stream)."""
        from .minima import MinimaRecord

        if self.minima_spec is None:
            raise EngineError("no minima record set: call set_minima first")
        K = self.observables_shape()[0]
        rec = MinimaRecord(self.minima_spec, self.R, self.F, self.N, K)
        n, _ = self.minima_shape()
        if n != rec.n_slots:
            raise EngineError(f"the handle's record has {n} slots, the spec gives {rec.n_slots}")
        self._chk(self._lib.smolmc_get_minima(
            self._h, _p(rec.value, C.c_double), _p(rec.enthalpy, C.c_double), _p(rec.features, C.c_double),
            _p(rec.occupancy, C.c_int32), _p(rec.counts, C.c_int32) if K else None, _p(rec.walker, C.c_int32),
            _p(rec.sample, C.c_int64), _p(rec.step, C.c_uint64)))
        if rec.companions is not None:
            self._chk(self._lib.smolmc_get_minima_companions(self._h, _p(rec.companions, C.c_int32)))
        rec.offers = int(rec.sample.max(initial=-1)) + 1  # (at least: the engine keeps the count)
        return rec

    def minima_kernel_ms(self):
        """Device times of the three passes of the last minima reduction in ms (HIP events; a measuring hook of the
        library, not part of the C-ABI)."""
        return self._kernel_ms("smolmc_debug_minima_kernel_ms", 3)

    # ---- structure factors: fixed-point amplitudes and intensities on the device -------------
    def set_structure_factor(self, sf):
        """The structure-factor spec of this handle (smolmc_set_structure): a ``structure.StructureFactor`` in the caller's
        site numbering, or None to remove it.  The engine copies and uploads; it refuses, naming the reason, a phase or
        kind out of range, sizes beyond the ``capi.MAX_STRUCT_*`` limits, a table large enough to overflow an amplitude,
        and a row too long for LDS."""
        self._set_family(BY_NAME["structure"], sf)

    def structure_shape(self):
        """(n_points, n_kinds, n_intensities) in force, zeros when no spec is set (smolmc_structure_shape)."""
        return tuple(self._family_sizes(BY_NAME["structure"]).values())

    def structure_factor(self, occupancies=None):
        """(amp (n, Q, K, 2) int64, inten (n, I) float64) of occupancies (n, N) evaluated on the device
        (smolmc_eval_structure), or, with None, of the walkers' current states (n = R)."""
        return tuple(self._eval_family(BY_NAME["structure"], occupancies))

    def sample_structure(self):
        """(structure_amplitudes (ns, R, Q, K, 2), structure_intensities (ns, R, I)) of the block ``fetch_samples`` would
        deliver next; the block stays undelivered (smolmc_get_sample_structure)."""
        return tuple(self._sample_family(BY_NAME["structure"]))

    def structure_kernel_ms(self):
        """Device time of the last launch of the structure kernel in ms (HIP events; a measuring hook of the library,
        not part of the C-ABI)."""
        return self._kernel_ms("smolmc_debug_structure_kernel_ms")

    # ---- connectivity: connected components and percolation on the device --------------------
    def set_connectivity(self, spec):
        """The connectivity spec of this handle (smolmc_set_connectivity): a ``connectivity.Connectivity`` in the caller's
        site numbering, or None to remove it.  The engine copies and uploads; it refuses, naming the reason, a bond, kind
        or image out of range, more than ``capi.MAX_CONN_GRAPHS`` graphs and a row too long for the LDS plan.  A spec with
        gate sites goes through smolmc_set_connectivity_gated, which refuses likewise a gate site or gate kind out of range
        and a gated row whose open bits do not fit."""
        gates = None if spec is None else spec.c_gates()
        if gates is None:
            self._set_family(BY_NAME["connectivity"], spec)
            return
        if spec.num_sites != self.N:
            raise ValueError(f"the connectivity spec is defined on {spec.num_sites} sites, the handle has {self.N}")
        struct, keep = spec.c_struct()
        self._chk(self._lib.smolmc_set_connectivity_gated(self._h, C.byref(struct), C.byref(gates[0])))
        del keep, gates

    def connectivity_gates(self):
        """(the graphs of the spec in force that have gates, as a tuple of graph numbers; the channel records the kernel
        walks, over all neighbour-list entries of those graphs) -- ``((), 0)`` for an ungated spec or none
        (smolmc_connectivity_gates)."""
        mask, n = C.c_int(), C.c_int64()
        self._chk(self._lib.smolmc_connectivity_gates(self._h, C.byref(mask), C.byref(n)))
        return tuple(g for g in range(capi.MAX_CONN_GRAPHS) if mask.value >> g & 1), int(n.value)

    def connectivity_shape(self):
        """(n_graphs, n_kinds) in force, zeros when no spec is set (smolmc_connectivity_shape)."""
        return tuple(self._family_sizes(BY_NAME["connectivity"]).values())

    def connectivity(self, occupancies=None, labels=False):
        """stats (n, G, 24) int64 of occupancies (n, N) evaluated on the device (smolmc_eval_connectivity), or, with None,
        of the walkers' current states (n = R); with ``labels`` the pair (stats, labels (n, G, N) int32)."""
        stats, lab = self._eval_family(
            BY_NAME["connectivity"], occupancies,
            lambda n, sizes: np.full((n, sizes["n_graphs"], self.N), -1, dtype=np.int32) if labels else None)
        return (stats, lab) if labels else stats

    def sample_connectivity(self):
        """connectivity (ns, R, G, 24) of the block ``fetch_samples`` would deliver next; the block stays undelivered
        (smolmc_get_sample_connectivity)."""
        return self._sample_family(BY_NAME["connectivity"])[0]

    def connectivity_kernel_ms(self):
        """Device time of the last launch of the connectivity kernel in ms (HIP events; a measuring hook of the library,
        not part of the C-ABI)."""
        return self._kernel_ms("smolmc_debug_connectivity_kernel_ms")

    def connectivity_passes(self):
        """(most passes a (row, graph) took, their sum over all of them) in the last launch of the connectivity kernel (a
        measuring hook of the library, not part of the C-ABI)."""
        fn = self._lib.smolmc_debug_connectivity_passes
        fn.restype, fn.argtypes = C.c_int, [_HP, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
        most, total = C.c_longlong(), C.c_longlong()
        self._chk(fn(self._h, C.byref(most), C.byref(total)))
        return int(most.value), int(total.value)

    # ---- patterns: species patterns on site tuples, counted by the observables' kernel -------
    def set_patterns(self, spec):
        """The pattern spec of this handle (smolmc_set_patterns): a ``patterns.Patterns`` in the caller's site numbering,
        or None to remove it.  It rests on the observables in force, whose kinds its class maps index.  The engine copies
        and uploads; it refuses, naming the reason, a handle without observables, a site or class out of range, more
        cells than ``capi.MAX_PATTERN_CELLS`` and a launch that does not fit LDS."""
        self._set_family(BY_NAME["patterns"], spec)

    def patterns_shape(self):
        """(n_sets, n_cells) in force, zeros when no spec is set (smolmc_patterns_shape)."""
        return tuple(self._family_sizes(BY_NAME["patterns"]).values())

    def patterns(self, occupancies=None):
        """cells (n, n_cells) int32 of occupancies (n, N) evaluated on the device (smolmc_eval_patterns), or, with None, of
        the walkers' current states (n = R)."""
        return self._eval_family(BY_NAME["patterns"], occupancies)[0]

    def sample_patterns(self):
        """pattern_counts (ns, R, n_cells) of the block ``fetch_samples`` would deliver next; the block stays undelivered
        (smolmc_get_sample_patterns)."""
        return self._sample_family(BY_NAME["patterns"])[0]

    # ---- environments: coordination environments, counted by the observables' kernel ---------
    def set_environments(self, spec):
        """The environment spec of this handle (smolmc_set_environments): an ``environments.Environments`` in the caller's
        site numbering, or None to remove it.  It rests on the observables in force, whose kinds its class maps index.
        The engine copies and uploads; it refuses, naming the reason, a handle without observables, a site or class out of
        range, more cells than ``capi.MAX_ENV_CELLS`` and a launch that does not fit LDS."""
        self._set_family(BY_NAME["environments"], spec)

    def environments_shape(self):
        """(n_sets, n_cells, n_centres) in force, zeros when no spec is set (smolmc_environments_shape)."""
        return tuple(self._family_sizes(BY_NAME["environments"]).values())

    def environments(self, occupancies=None, codes=False):
        """cells (n, n_cells) int32 of occupancies (n, N) evaluated on the device (smolmc_eval_environments), or, with
        None, of the walkers' current states (n = R).  ``codes``: (cells, codes (n, n_centres) int32), the set-local code
        of every centre or -1 for a skipped one."""
        cells, out = self._eval_family(
            BY_NAME["environments"], occupancies,
            lambda n, sizes: np.zeros((n, sizes["n_centres"]), dtype=np.int32) if codes else None)
        return (cells, out) if codes else cells

    def sample_environments(self):
        """environment_counts (ns, R, n_cells) of the block ``fetch_samples`` would deliver next; the block stays
        undelivered (smolmc_get_sample_environments)."""
        return self._sample_family(BY_NAME["environments"])[0]

    # ---- statistics: running moments, blocking sums and a histogram, kept on the device -----
    def set_statistics(self, spec):
        """The statistics record of this handle (smolmc_set_statistics): a ``statistics.Statistics``, or None to remove
        it.  A new spec starts an empty record.  The record lives as long as the handle: ``set_state`` and
        ``discard_samples`` leave it alone.  A spec keyed by bin (``Statistics.by_bin``) goes through
        smolmc_set_statistics_binned, which refuses likewise blocking levels, ``n_keys`` outside 1..65536, a bin width that
        is not positive and finite and a key column outside the columns.  A spec with a site field
        (``Statistics(..., sites=, site_codes=)``) attaches it to the new record (smolmc_set_statistics_sites); when the
        engine refuses the field, the handle is left without a record.  A spec with a joint field
        (``Statistics(..., joint=)``) attaches that one next (smolmc_set_statistics_joint), with the same rule."""
        # (what ``statistics.segments`` takes: F, then every family's size in force, in the table's order)
        shape = () if spec is None else (self.F,) + tuple(self._family_sizes(fam)[fam.stat[2]] for fam in FAMILIES)
        bins = None if spec is None else spec.c_bins()
        if bins is None:
            self._set_spec(self._lib.smolmc_set_statistics, spec, None, *shape)
        else:
            struct, keep = spec.c_struct(*shape)
            self._chk(self._lib.smolmc_set_statistics_binned(self._h, C.byref(struct), *bins))
            del keep
        self.statistics_spec = spec
        field = None if spec is None else spec.c_sites()
        joint = None if spec is None else spec.c_joint()
        try:
            if field is not None:
                self.set_statistics_sites(*field)
            if joint is not None:
                self.set_statistics_joint(*joint)
        except (EngineError, ValueError):
            self._chk(self._lib.smolmc_set_statistics(self._h, None))
            self.statistics_spec = None
            raise

    def set_statistics_sites(self, sites, n_sites, n_codes):
        """smolmc_set_statistics_sites as it stands: attach a site field of ``n_codes`` codes on the sites ``sites`` (an
        int32 array in the caller's numbering, or None for all sites) to the record in force and zero the field;
        ``n_codes = 0`` detaches it.  ``set_statistics`` calls this for a spec that has a field."""
        a = None if sites is None else np.ascontiguousarray(sites, dtype=np.int32)
        self._chk(self._lib.smolmc_set_statistics_sites(self._h, _p(a, C.c_int32), int(n_sites), int(n_codes)))

    def statistics_sites_shape(self):
        """(n_sites, n_codes) of the site field in force, zeros when none is set (smolmc_statistics_sites_shape)."""
        m, c = C.c_int(), C.c_int()
        self._chk(self._lib.smolmc_statistics_sites_shape(self._h, C.byref(m), C.byref(c)))
        return int(m.value), int(c.value)

    def set_statistics_joint(self, column_a, n_a, min_a, bin_a, column_b=0, n_b=0, min_b=0.0, bin_b=0.0):
        """smolmc_set_statistics_joint as it stands: attach a joint field of ``n_a`` x ``n_b`` cells of the record's columns
        ``column_a`` and ``column_b`` (indices into the columns) to the record in force and zero the field; ``n_a = 0``
        detaches it.  ``set_statistics`` calls this for a spec that has a field (``Statistics.c_joint``)."""
        self._chk(self._lib.smolmc_set_statistics_joint(self._h, int(column_a), int(n_a), float(min_a), float(bin_a),
                                                        int(column_b), int(n_b), float(min_b), float(bin_b)))

    def statistics_joint_shape(self):
        """(column_a, n_a, min_a, bin_a, column_b, n_b, min_b, bin_b) of the joint field in force, zeros when none is set
        (smolmc_statistics_joint_shape)."""
        v = [t() for t in (C.c_int, C.c_int, C.c_double, C.c_double) * 2]
        self._chk(self._lib.smolmc_statistics_joint_shape(self._h, *[C.byref(x) for x in v]))
        return tuple(float(x.value) if isinstance(x, C.c_double) else int(x.value) for x in v)

    def statistics_bins(self):
        """(key_column, n_keys, key_min, key_bin, key_under, key_over) of the binned record in force, all zeros when the
        record in force is not binned or none is set (smolmc_statistics_bins; waits for the handle's stream)."""
        col, nk, kmin, kbin, under, over = C.c_int(), C.c_int(), C.c_double(), C.c_double(), C.c_int64(), C.c_int64()
        self._chk(self._lib.smolmc_statistics_bins(self._h, *[C.byref(x) for x in (col, nk, kmin, kbin, under, over)]))
        return int(col.value), int(nk.value), float(kmin.value), float(kbin.value), int(under.value), int(over.value)

    def statistics_shape(self):
        """(n_keys, n_columns, n_levels, n_bins) in force, zeros when no record is set (smolmc_statistics_shape)."""
        v = [C.c_int() for _ in range(4)]
        self._chk(self._lib.smolmc_statistics_shape(self._h, *[C.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    def update_statistics(self):
        """Offer the walkers' current states to the record, one offer (smolmc_update_statistics): for callers of ``run``."""
        self._chk(self._lib.smolmc_update_statistics(self._h))

    def reset_statistics(self):
        """Empty the record (smolmc_reset_statistics)."""
        self._chk(self._lib.smolmc_reset_statistics(self._h))

    def statistics(self):
        """The record as a ``statistics.StatisticsRecord`` (smolmc_get_statistics; waits for the handle's stream)."""
        from .statistics import StatisticsRecord

        if self.statistics_spec is None:
            raise EngineError("no statistics record set: call set_statistics first")
        n_sites, n_codes = self.statistics_sites_shape()
        rec = StatisticsRecord(self.statistics_spec, self.R, n_sites)
        if rec.site_counts.shape[1:] != (n_sites, n_codes):
            raise EngineError(f"the handle's site field has shape {(n_sites, n_codes)}, the spec gives {rec.site_counts.shape[1:]}")
        joint = self.statistics_joint_shape()
        if joint != (rec.spec.c_joint() or (0, 0, 0.0, 0.0) * 2):
            raise EngineError(f"the handle's joint field is {joint}, the spec gives {rec.spec.c_joint()}")
        shape = self.statistics_shape()
        want = (rec.n_keys, rec.spec.n_columns, rec.spec.n_levels, rec.spec.n_bins)
        if shape != want:
            raise EngineError(f"the handle's record has shape {shape}, the spec gives {want}")
        self._chk(self._lib.smolmc_get_statistics(
            self._h, _p(rec.n, C.c_int64), _p(rec.shift, C.c_double), _p(rec.s1, C.c_double), _p(rec.s2, C.c_double),
            _p(rec.has, C.c_uint64), _p(rec.pend, C.c_double), _p(rec.b2, C.c_double), _p(rec.nb, C.c_int64),
            _p(rec.hist, C.c_int64), _p(rec.under, C.c_int64), _p(rec.over, C.c_int64)))
        if rec.spec.binned:
            rec.key_under, rec.key_over = self.statistics_bins()[4:]
        if n_codes:
            self._chk(self._lib.smolmc_get_statistics_sites(self._h, _p(rec.site_counts, C.c_int64), _p(rec.site_over, C.c_int64)))
        if joint[1]:
            self._chk(self._lib.smolmc_get_statistics_joint(self._h, _p(rec.joint, C.c_int64), _p(rec.joint_out, C.c_int64)))
        return rec

    def statistics_kernel_ms(self):
        """Device time of the last statistics reduction in ms (HIP events; a measuring hook of the library, not part of
        the C-ABI)."""
        return self._kernel_ms("smolmc_debug_statistics_kernel_ms")

    def statistics_bins_kernel_ms(self):
        """Device times of the two launches of the last reduction of a binned record in ms, [the row keys, the reduction per
        key] (HIP events; a measuring hook of the library, not part of the C-ABI)."""
        return self._kernel_ms("smolmc_debug_statistics_bins_kernel_ms", 2)

    def statistics_sites_kernel_ms(self):
        """Device time of the site field's last launch in ms (HIP events; a measuring hook of the library, not part of the
        C-ABI)."""
        return self._kernel_ms("smolmc_debug_statistics_sites_kernel_ms")

    def statistics_joint_kernel_ms(self):
        """Device time of the joint field's last launch in ms (HIP events; a measuring hook of the library, not part of the
        C-ABI)."""
        return self._kernel_ms("smolmc_debug_statistics_joint_kernel_ms")

    def run_sampled(self, nsamples, thin_by, occupancy=True, packed=False, bias=False, wl=False, observables=False,
                    minima=False, statistics=False, structure=False, connectivity=False, patterns=False, environments=False):
        """Advance nsamples*thin_by steps recording one sample per walker every thin_by steps
        on the device; returns dict(enthalpy (ns,R), features (ns,R,F), accepted (ns,R) bool,
        occupancy (ns,R,N) or None[, bias (ns,R)][, the Wang-Landau trace][, species_counts, pair_counts]
        [, structure_amplitudes (ns,R,Q,K,2) int64, structure_intensities (ns,R,I)][, connectivity (ns,R,G,24) int64]
        [, pattern_counts (ns,R,n_cells) int32][, environment_counts (ns,R,n_cells) int32]).
        Occupancies come back as int32 (the reference's trace dtype) or, with ``packed``, as the ring's own
        uint8 -- a quarter of the transfer.  = ``run_sampled_async`` + ``fetch_samples``."""
        asked = locals()  # (the keywords as given: SAMPLE_FLAGS names them)
        self.run_sampled_async(nsamples, thin_by, **{keyword: asked[keyword] for keyword, _ in SAMPLE_FLAGS})
        return self.fetch_samples(packed=packed)

    def run_sampled_async(self, nsamples, thin_by, occupancy=True, bias=False, wl=False, observables=False, minima=False,
                          statistics=False, structure=False, connectivity=False, patterns=False, environments=False):
        """Queue one block of the device ring (smolmc_run_sampled): returns at once.  The ring has two
        slots; queue block k + 1 BEFORE fetching block k and the download of k overlaps the kernel of
        k + 1 (the order ``fetch_samples`` delivers in: oldest first).  ``observables``: the kind and pair
        counts of ``set_observables`` for every row, counted on the device; with ``occupancy=False`` the
        occupancy rows they are counted from never leave it.  ``minima``: every row is offered to the record of
        ``set_minima`` when the block's launches are through; what the reduction reads and the caller did not ask for
        stays on the device.  ``statistics``: likewise every row is offered to the record of ``set_statistics``.
        ``structure``: the amplitudes and intensities of ``set_structure_factor`` for every row, like ``observables``.
        ``connectivity``: the stats of ``set_connectivity`` for every row, likewise.  ``patterns``: the cells of
        ``set_patterns`` for every row, counted by the launch that counts the observables.  ``environments``: the cells of
        ``set_environments`` for every row, by the same launch."""
        asked = locals()  # (the keywords as given: SAMPLE_FLAGS names them)
        flags = sum(flag for keyword, flag in SAMPLE_FLAGS if asked[keyword])
        self._chk(self._lib.smolmc_run_sampled(self._h, int(nsamples), int(thin_by), flags))

    def pending_samples(self):
        """(blocks queued and not fetched, nsamples and flags of the block ``fetch_samples`` would deliver): the
        ring's own bookkeeping (smolmc_pending_samples) -- the arrays of a fetch are sized from it."""
        npend, ns, flags = C.c_int(), C.c_int64(), C.c_int()
        self._chk(self._lib.smolmc_pending_samples(self._h, C.byref(npend), C.byref(ns), C.byref(flags)))
        return int(npend.value), int(ns.value), int(flags.value)

    def discard_samples(self):
        """Forget every block of the ring (a sampling loop left half way must not hand its blocks to the next)."""
        self._chk(self._lib.smolmc_discard_samples(self._h))

    def fetch_samples(self, packed=False):
        """The oldest block queued with ``run_sampled_async`` that was not fetched yet (waits for ITS
        download only)."""
        npend, ns, flags = self.pending_samples()
        if npend == 0:
            raise EngineError("no samples recorded: call run_sampled_async first")
        H = np.empty((ns, self.R))
        feat = np.empty((ns, self.R, self.F))
        acc = np.empty((ns, self.R), dtype=np.uint8)
        with_occ = bool(flags & capi.SAMPLE_OCCUPANCY)
        extra, obs = {}, {}
        for fam in FAMILIES:
            if flags & fam.flag:  # (read before the fetch marks the block delivered)
                obs.update(zip((name for name, _, _ in fam.traces), self._sample_family(fam)))
        if flags & capi.SAMPLE_BIAS:
            extra["bias"] = np.empty((ns, self.R))
        if flags & capi.SAMPLE_WL:
            extra.update(entropy=np.empty((ns, self.R, self.L)), histogram=np.empty((ns, self.R, self.L), dtype=np.int64),
                         occurrences=np.empty((ns, self.R, self.L), dtype=np.int64),
                         mean_features=np.empty((ns, self.R, self.L, self.F)), mod_factor=np.empty((ns, self.R)))
        if packed or extra:
            occ = np.empty((ns, self.R, self.N), dtype=np.uint8) if with_occ else None
            self._chk(self._lib.smolmc_get_samples_ex(
                self._h, _p(H, C.c_double), _p(feat, C.c_double), _p(acc, C.c_uint8), _p(occ, C.c_uint8),
                _p(extra.get("bias"), C.c_double), _p(extra.get("entropy"), C.c_double),
                _p(extra.get("histogram"), C.c_int64), _p(extra.get("occurrences"), C.c_int64),
                _p(extra.get("mean_features"), C.c_double), _p(extra.get("mod_factor"), C.c_double)))
            if occ is not None and not packed:
                occ = occ.astype(np.int32)
        else:
            occ = np.empty((ns, self.R, self.N), dtype=np.int32) if with_occ else None
            self._chk(self._lib.smolmc_get_samples(self._h, _p(H, C.c_double), _p(feat, C.c_double),
                                                   _p(acc, C.c_uint8), _p(occ, C.c_int32)))
        return dict(enthalpy=H, features=feat, accepted=acc.astype(bool), occupancy=occ, **extra, **obs)

    def last_kernel_ms(self):
        ms = C.c_float()
        self._chk(self._lib.smolmc_last_kernel_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def replay(self, steps, uniforms, log_priori=None, with_priori=False):
        """steps (R, n, 2k) int32 with k <= 8 (site, code) pairs per record (padded to
        SMOLMC_STEP_ROW with -1), uniforms (R, n) float64, log_priori (R, n) or None (see
        smolmc_replay) -> (accepted (R,n) bool, H (R,n)[, log_priori used (R,n)])."""
        uniforms = np.ascontiguousarray(uniforms, dtype=np.float64).reshape(self.R, -1)
        n = uniforms.shape[1]
        steps = capi.step_rows(steps, self.R, n)
        lp = None if log_priori is None else np.ascontiguousarray(log_priori, dtype=np.float64).reshape(self.R, n)
        acc = np.zeros((self.R, n), dtype=np.uint8)
        H = np.zeros((self.R, n))
        lpo = np.zeros((self.R, n)) if with_priori else None
        self._chk(
            self._lib.smolmc_replay(
                self._h, n, _p(steps, C.c_int32), _p(uniforms, C.c_double), _p(lp, C.c_double),
                _p(acc, C.c_uint8), _p(H, C.c_double), _p(lpo, C.c_double),
            )
        )
        return (acc.astype(bool), H, lpo) if with_priori else (acc.astype(bool), H)

    # ---- evaluator level --------------------------------------------------------
    def eval_full(self, occupancies):
        occ = self._occ32(occupancies, (-1, self.N))
        out = np.zeros((len(occ), self.F))
        self._chk(self._lib.smolmc_eval_full(self._h, _p(occ, C.c_int32), len(occ), _p(out, C.c_double)))
        return out

    def eval_delta(self, occupancy, steps, single_step=None):
        """Feature changes of steps applied to ``occupancy`` (each step on its own, not chained), (n, F).

        ``steps`` as records: an ndarray of (n, 2k) int32 rows (site_0, code_0, ..., site_{k-1}, code_{k-1}),
        k <= 8, -1 = absent -- n steps, exactly what capi.step_rows makes of it; a flat record is one step.
        ``steps`` the way the reference's ushers return ONE step: a Python list of (site, code) tuples
        (mcusher.py:104-116).  An (n, 2) ndarray with n > 1 could be read either way -- n single flips or one step
        of n flips, and it silently changed meaning between rounds -- so it is refused unless ``single_step`` says
        which: True = one step of n flips, False = n steps of one flip.  ``single_step`` also overrides the default
        reading of the other spellings."""
        occ = self._occ32(occupancy, (self.N,))
        as_pairs = isinstance(steps, (list, tuple)) and len(steps) > 0 and all(
            isinstance(f, (list, tuple)) and len(f) == 2 for f in steps)
        a = np.asarray(steps, dtype=np.int32)
        if single_step is None:
            if isinstance(steps, np.ndarray) and a.ndim == 2 and a.shape[1] == 2 and a.shape[0] > 1:
                raise ValueError(
                    f"an ({a.shape[0]}, 2) array is ambiguous: {a.shape[0]} single-flip steps (single_step=False) or "
                    f"one step of {a.shape[0]} flips (single_step=True)?")
            single_step = a.ndim == 1 or as_pairs
        if single_step:
            a = a.reshape(1, -1)  # one step: flat record, a list of (site, code) tuples, or pair rows
        steps = capi.step_rows(a)
        out = np.zeros((len(steps), self.F))
        self._chk(
            self._lib.smolmc_eval_delta(
                self._h, _p(occ, C.c_int32), _p(steps, C.c_int32), len(steps), _p(out, C.c_double)
            )
        )
        return out

    # ---- device plumbing ----------------------------------------------------------
    def set_stream(self, stream_ptr):
        self._chk(self._lib.smolmc_set_stream(self._h, C.c_void_p(int(stream_ptr))))

    def export_enthalpy(self, dev_ptr):
        self._chk(self._lib.smolmc_export_enthalpy_dev(self._h, C.c_void_p(int(dev_ptr))))

    def import_temperature(self, dev_ptr):
        self._chk(self._lib.smolmc_import_temperature_dev(self._h, C.c_void_p(int(dev_ptr))))

    def exchange_dev(self, n_total, first, parity, enthalpy_all_ptr, ladder_ptr, log_u_ptr, rung_of_ptr, stats_ptr=0):
        """One exchange attempt of a temperature ladder decided on the device (smolmc_exchange_dev): device
        pointers in, this handle's temperatures follow the new rung assignment; asynchronous."""
        self._chk(self._lib.smolmc_exchange_dev(
            self._h, int(n_total), int(first), int(parity), C.c_void_p(int(enthalpy_all_ptr)), C.c_void_p(int(ladder_ptr)),
            C.c_void_p(int(log_u_ptr)), C.c_void_p(int(rung_of_ptr)), C.c_void_p(int(stats_ptr)) if stats_ptr else None))
