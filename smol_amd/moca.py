"""Host-side mirror of smol.moca's interface for the accelerated path.

Same names, argument meaning and error behaviour as the reference objects they stand
in for, so user scripts and parity tests read like smol's own:

    Sublattice                      smol/moca/sublattice.py:23
    ClusterExpansionProcessor       smol/moca/processor/expansion.py:39
    ClusterDecompositionProcessor   smol/moca/processor/expansion.py:243
    EwaldProcessor                  smol/moca/processor/ewald.py:26
    CompositeProcessor              smol/moca/processor/composite.py:18
    Ensemble                        smol/moca/ensemble.py:102
    Metropolis / WangLandau         smol/moca/kernel/metropolis.py:52, wanglandau.py:17
    Trace                           smol/moca/trace.py:8
    SampleContainer                 smol/moca/sampler/container.py:25
    Sampler                         smol/moca/sampler/sampler.py:22

What differs, by design: the boundary sits at the *Sampler* level.  A
Sampler owns ONE engine handle holding all its walkers on one GPU; ``run`` advances
every walker ``thin_by`` steps per kernel launch instead of looping over Python kernel
objects one flip at a time.  The per-flip ``Processor`` methods are kept (GPU-backed,
one launch per call) for parity tests and user-side checks, not for sampling.

Everything here drives the HIP engine through smol_amd.engine; there is no CPU path.
"""

from __future__ import annotations

import json
import os
import warnings
from datetime import datetime
from types import SimpleNamespace

import numpy as np

from . import capi
from .engine import Engine
from .families import BY_NAME, FAMILIES, trace_shape

kB = 8.617333262145e-5  # smol/constants.py:4


# --------------------------------------------------------------------------- #
class Trace(SimpleNamespace):
    """Namespace of ndarrays recorded during sampling (smol/moca/trace.py:8-46)."""

    def __init__(self, /, **kwargs):
        if not all(isinstance(v, np.ndarray) for v in kwargs.values()):
            raise TypeError("Trace only supports attributes of type ndarray.")
        super().__init__(**kwargs)

    @property
    def names(self):
        return tuple(self.__dict__.keys())

    def items(self):
        yield from self.__dict__.items()

    def __setattr__(self, name, value):
        if isinstance(value, float):
            value = np.array([value], dtype=np.float64)
        if isinstance(value, int):
            value = np.array([value], dtype=np.int32)
        if not isinstance(value, np.ndarray):
            raise TypeError("Trace only supports attributes of type ndarray.")
        self.__dict__[name] = value

    def as_dict(self):
        return self.__dict__.copy()


class StepTrace(Trace):
    """Trace of one attempted step: the walker's values plus ``delta_trace``, the changes the step
    made to them (smol/moca/trace.py:46-90); ``names`` / ``items`` skip the inner trace."""

    def __init__(self, /, **kwargs):
        super().__init__(**kwargs)
        self.__dict__["delta_trace"] = Trace()

    @property
    def names(self):
        return tuple(n for n in self.__dict__ if n != "delta_trace")

    def items(self):
        for name, value in self.__dict__.items():
            if name != "delta_trace":
                yield name, value

    def __setattr__(self, name, value):
        if name == "delta_trace":
            raise ValueError("Attribute name 'delta_trace' is reserved.")
        super().__setattr__(name, value)

    def as_dict(self):
        d = self.__dict__.copy()
        d["delta_trace"] = d["delta_trace"].as_dict()
        return d


class Sublattice:
    """Sites sharing one site space (smol/moca/sublattice.py:23-107)."""

    def __init__(self, species, sites, charges=None):
        self.species = tuple(species)
        # oxidation state of every species (0 for a vacancy); used by CompositionSpace
        given = [0] * len(self.species) if charges is None else list(charges)
        self.charges = tuple(0 if q is None else q for q in given)
        self.sites = np.unique(np.asarray(sites, dtype=np.int64))
        self.active_sites = self.sites.copy()
        if len(self.species) <= 1:
            self.restrict_sites(self.sites)
        self.encoding = np.arange(len(self.species), dtype=np.int32)

    @property
    def is_active(self):
        return len(self.active_sites) > 0

    @property
    def restricted_sites(self):
        return np.setdiff1d(self.sites, self.active_sites)

    def restrict_sites(self, sites):
        sites = set(int(s) for s in sites)
        self.active_sites = np.array([i for i in self.active_sites if i not in sites], dtype=np.int64)

    def reset_restricted_sites(self):
        if len(self.species) > 1:
            self.active_sites = self.sites.copy()

    def _code_of(self, sp):
        if isinstance(sp, (int, np.integer)):
            code = int(sp)
            if code not in self.encoding:
                raise ValueError(f"code {code} is not in this sublattice's encoding {self.encoding}")
            return code
        return int(self.encoding[self.species.index(sp)])

    def split_by_species(self, occu, species_in_partitions):
        """Split into one sublattice per partition of this one's species, by what occupies each
        site in ``occu`` (smol/moca/sublattice.py:109-186): partition p gets the sites holding
        one of its species (given as species or as codes), keeps those codes as its encoding, and a
        single-species partition is restricted (inactive).  The ACTIVE sites are listed code by code in
        ascending code order, as the reference lists them; ``sites`` is sorted (the constructor's np.unique)."""
        occu = np.asarray(occu)
        out = []
        for partition in species_in_partitions:
            codes = sorted(self._code_of(sp) for sp in partition)
            where = [int(np.where(self.encoding == c)[0][0]) for c in codes]
            sites = np.concatenate([self.sites[occu[self.sites] == c] for c in codes] + [np.zeros(0, np.int64)])
            actives = np.concatenate([self.active_sites[occu[self.active_sites] == c] for c in codes]
                                     + [np.zeros(0, np.int64)])
            # (`sites` stays what the constructor makes of it -- sorted, np.unique, sublattice.py:57 -- only the
            # ACTIVE sites are listed code by code, :176-178: reset_restricted_sites then restores sorted sites)
            part = Sublattice([self.species[i] for i in where], sites, [self.charges[i] for i in where])
            part.active_sites = actives.astype(np.int64)
            part.encoding = np.array(codes, dtype=np.int32)
            if len(codes) == 1:
                part.restrict_sites(part.sites)
            out.append(part)
        return out

    def __eq__(self, other):
        """Same species, encoding and sites (restrictions are not compared, sublattice.py:188-199)."""
        return (isinstance(other, Sublattice) and self.species == other.species
                and np.array_equal(self.encoding, other.encoding) and np.array_equal(self.sites, other.sites))

    __hash__ = None

    def as_dict(self):
        """JSON-able record (sublattice.py:201-217)."""
        return dict(species=list(self.species), charges=list(self.charges), sites=self.sites.tolist(),
                    encoding=self.encoding.tolist(), active_sites=self.active_sites.tolist())

    @classmethod
    def from_dict(cls, d):
        sub = cls(d["species"], d["sites"], d.get("charges"))
        sub.sites = np.array(d["sites"], dtype=np.int64)
        sub.encoding = np.array(d["encoding"], dtype=np.int32)
        sub.active_sites = np.array(d["active_sites"], dtype=np.int64)
        return sub


# --------------------------------------------------------------------------- #
# processors
# --------------------------------------------------------------------------- #
def default_species(prim):
    names = []
    for b, S in enumerate(prim.nspecies):
        names.append([f"{chr(65 + b)}{c}" for c in range(S)])
    return names


def _eval_device():
    """HIP device of the one-walker evaluation handles: this rank's GPU under a one-process-per-GPU
    launcher (LOCAL_RANK), else device 0."""
    if "LOCAL_RANK" not in os.environ:
        return 0
    from . import parallel

    return parallel.local_device(int(os.environ["LOCAL_RANK"]))


class Processor:
    """Base of the GPU-backed processors (smol/moca/processor/base.py:26)."""

    def __init__(self, supercell, coefficients):
        self.supercell = supercell
        self.cluster_subspace = supercell.model
        self.coefs = np.asarray(coefficients, dtype=np.float64)
        self.size = supercell.size
        self.num_sites = supercell.num_sites
        self.supercell_matrix = supercell.scmatrix
        self._eval_engine = None
        self._eval_tables = None

    # -- pieces of the flattened tables this processor contributes --------------
    def _table_kwargs(self):
        raise NotImplementedError

    def _make_tables(self, mu_table=None, sublattices=None):
        kw = self._table_kwargs()
        tab = capi.TableSet.from_synth(
            self.supercell, kw["ce_coefs_expansion"], feature_mode=kw["feature_mode"],
            ewald=kw.get("ewald"), ewald_coef=kw.get("ewald_coef", 1.0), mu_table=mu_table,
            ewald_charges=kw.get("ewald_charges", "auto"),
        )
        if kw.get("ce_natural") is not None:
            tab._keep["ce_coefs"][:] = kw["ce_natural"]
        if kw.get("interaction_tensors") is not None:
            its = kw["interaction_tensors"]
            flat = np.concatenate([np.ravel(np.asarray(x, dtype=np.float64)) for x in its[1:]])
            if flat.size != tab._keep["interaction_tensors"].size:
                raise ValueError(
                    "The number of cluster interaction tensors must match the number of orbits"
                )
            tab._keep["interaction_tensors"][:] = flat
            tab.struct.offset = float(its[0])
        if sublattices is not None:
            _override_sublattices(tab, sublattices)
        return tab

    def _engine(self):
        if self._eval_engine is None:
            self._eval_tables = self._make_tables()
            self._eval_engine = Engine(self._eval_tables, capi.make_config(1, device=_eval_device()))
        return self._eval_engine

    _feature_slice = slice(None)

    # -- reference API -----------------------------------------------------------
    def compute_feature_vector(self, occupancy):
        try:
            occupancy = np.array(occupancy, dtype=np.int32)
        except ValueError:
            types = {type(n) for n in occupancy}
            raise ValueError(f"occupancy contains {types}, but should be integers!")
        out = self._engine().eval_full(occupancy[None, :])[0][self._feature_slice]
        return float(out[0]) if self._scalar_feature else out

    _scalar_feature = False

    def compute_feature_vector_change(self, occupancy, flips):
        try:
            occupancy = np.array(occupancy, dtype=np.int32)
        except ValueError:
            types = {type(n) for n in occupancy}
            raise ValueError(f"occupancy contains {types}, but should be integers!")
        flips = list(flips)
        if len(flips) > capi.MAX_STEP_FLIPS:
            # sequential semantics (expansion.py:217-229): chain in records of eight flips
            total = 0.0
            occ = occupancy.copy()
            for i in range(0, len(flips), capi.MAX_STEP_FLIPS):
                chunk = flips[i:i + capi.MAX_STEP_FLIPS]
                total = total + self.compute_feature_vector_change(occ, chunk)
                for s, c in chunk:
                    occ[s] = c
            return total
        out = self._engine().eval_delta(occupancy, capi.step_rows([flips]))[0][self._feature_slice]
        return float(out[0]) if self._scalar_feature else out

    def compute_property(self, occupancy):
        return np.dot(self.coefs, self.compute_feature_vector(occupancy))

    def compute_property_change(self, occupancy, flips):
        return np.dot(self.coefs, self.compute_feature_vector_change(occupancy, flips))

    def compute_average_drift(self, iterations=1000, rng=None):
        """Average forward / reverse drift of local updates (processor/base.py:270-312)."""
        rng = np.random.default_rng(rng)
        prim = self.supercell.model.prim
        nsp = np.array([prim.nspecies[b] for b in self.supercell.site_b])
        active = np.flatnonzero(nsp > 1)
        occ = (rng.random(self.num_sites) * nsp).astype(np.int32)
        fwd = rev = 0.0
        f_prev = self.compute_feature_vector(occ)
        for _ in range(iterations):
            s = int(rng.choice(active))
            c = int((occ[s] + 1 + rng.integers(0, nsp[s] - 1)) % nsp[s])
            d = self.compute_feature_vector_change(occ, [(s, c)])
            new = occ.copy()
            new[s] = c
            dr = self.compute_feature_vector_change(new, [(s, int(occ[s]))])
            f_new = self.compute_feature_vector(new)
            fwd += np.sum(np.abs(f_new - f_prev - d))
            rev += np.sum(np.abs(f_prev - f_new - dr))
            occ, f_prev = new, f_new
        return fwd / iterations, rev / iterations

    def get_sublattices(self):
        """One Sublattice per distinct site space (processor/base.py get_sublattices)."""
        prim = self.supercell.model.prim
        names = getattr(prim, "species", None) or default_species(prim)
        groups = {}
        for b in range(prim.nb):
            key = prim.labels[b]
            sites = np.flatnonzero(self.supercell.site_b == b)
            if key in groups:
                groups[key][1].append(sites)
            else:
                groups[key] = (names[b], [sites], prim.charges[b])
        return [Sublattice(sp, np.concatenate(st), q) for sp, st, q in groups.values()]

    @property
    def allowed_species(self):
        """Species names of every site's site space, in code order (processor/base.py:104-107)."""
        prim = self.supercell.model.prim
        names = getattr(prim, "species", None) or default_species(prim)
        return [list(names[b]) for b in self.supercell.site_b]

    def encode_occupancy(self, occupancy):
        """Species names (or codes already) -> int32 codes (processor/base.py:228-237)."""
        allowed = self.allowed_species
        if len(occupancy) != len(allowed):
            raise ValueError(f"occupancy has {len(occupancy)} entries, the supercell {len(allowed)} sites")
        return np.array([sp if isinstance(sp, (int, np.integer)) else species.index(sp)
                         for species, sp in zip(allowed, occupancy)], dtype=np.int32)

    def decode_occupancy(self, encoded_occupancy):
        """int codes -> species names (processor/base.py:239-243)."""
        return [species[int(i)] for i, species in zip(encoded_occupancy, self.allowed_species)]


class ClusterExpansionProcessor(Processor):
    """Correlation-vector features (smol/moca/processor/expansion.py:39-241)."""

    def __init__(self, supercell, coefficients):
        if len(coefficients) != supercell.model.num_corr_functions:
            raise ValueError(
                f"The provided coefficients are not the right length. Got {len(coefficients)} "
                f"coefficients, the length must be {supercell.model.num_corr_functions} based on "
                "the provided cluster subspace."
            )
        super().__init__(supercell, coefficients)

    def _table_kwargs(self):
        return dict(feature_mode=capi.FEATURES_CORRELATIONS, ce_coefs_expansion=self.coefs)


class ClusterDecompositionProcessor(Processor):
    """Cluster-interaction features (smol/moca/processor/expansion.py:243-489)."""

    def __init__(self, supercell, interaction_tensors, coefficients=None):
        model = supercell.model
        if len(interaction_tensors) != model.num_orbits:
            raise ValueError(
                f"The number of cluster interaction tensors must match the number  of orbits in "
                f"the subspace. Got {len(interaction_tensors)} interaction tensors, but need "
                f"{model.num_orbits}  for the given cluster_subspace."
            )
        coefficients = model.orbit_multiplicities if coefficients is None else coefficients
        super().__init__(supercell, np.asarray(coefficients, dtype=np.float64))
        self._interaction_tensors = interaction_tensors

    def _table_kwargs(self):
        return dict(
            feature_mode=capi.FEATURES_INTERACTIONS,
            ce_coefs_expansion=np.zeros(self.supercell.model.num_corr_functions),
            ce_natural=self.coefs,
            interaction_tensors=self._interaction_tensors,
        )


class DistanceProcessor(Processor):
    """Distance of the feature vector from a target (smol/moca/processor/distance.py:20-182):
    ``d = -w L + ||W (f - f_T)||_1`` with L the largest diameter up to which every feature matches the target
    within match_tol.  Features are the reference's intensive distance vector [L or 0, |f_1 - t_1|, ...].
    ``supercell``: a supercell of the build's tables (synth / mson), or a cluster subspace together with
    ``supercell_matrix`` (the reference's call shape).  Evaluated on a distance-objective engine handle
    (smolmc_create_distance); an Ensemble / Sampler on such a processor runs the distance kernel."""

    feature_mode = capi.FEATURES_CORRELATIONS

    def __init__(self, supercell, supercell_matrix=None, target_vector=None, match_weight=1.0, match_tol=1e-5,
                 target_weights=None, use_concentration=False):
        if supercell_matrix is not None:  # (cluster_subspace, supercell_matrix)
            from . import sqs

            supercell, _ = sqs.distance_tables(supercell, supercell_matrix, self.feature_mode)
        model = supercell.model
        if len(getattr(model, "external_terms", []) or []) > 0:
            raise ValueError("The given cluster subspace cannot have external terms.")  # distance.py:76-77
        if use_concentration:
            raise NotImplementedError("use_concentration: the build's tables carry the fitted site bases only")
        if match_weight < 0:
            raise ValueError("The match weight must be a positive number.")  # distance.py:79-80
        if len(target_weights) != len(target_vector) - 1:  # distance.py:82-87
            raise ValueError(
                f"The length of target_weights must be equal to the length ofthe target vector minus one "
                f"{len(target_vector) - 1}. \nGot {len(target_weights)} instead.")
        self.target_vector = np.asarray(target_vector, dtype=np.float64)
        self.match_tol = match_tol
        super().__init__(supercell, np.concatenate([[-match_weight], target_weights]))  # distance.py:95
        self._dist_engine = None

    def distance_spec(self, kB=1.0):
        """The capi.DistanceSpec of this objective (temperatures in units of kB)."""
        from . import sqs

        return sqs.distance_spec(self.cluster_subspace, self.feature_mode, self.target_vector, self.coefs[1:],
                                 -self.coefs[0], self.match_tol, kB)

    def _table_kwargs(self):
        return dict(feature_mode=self.feature_mode,
                    ce_coefs_expansion=np.ones(self.cluster_subspace.num_corr_functions),
                    interaction_tensors=getattr(self, "_interaction_tensors", None))

    def _engine(self):
        if self._dist_engine is None:
            self._eval_tables = self._make_tables()
            self._dist_engine = Engine(self._eval_tables, capi.make_config(1, device=_eval_device()),
                                       distance=self.distance_spec())
        return self._dist_engine

    def compute_feature_vector_distances(self, occupancy, flips):
        """[distances before, distances after] the flips, entry 0 = 0 (evaluator.pyx:319-437)."""
        occupancy = np.array(occupancy, dtype=np.int32)
        occu_f = occupancy.copy()
        for site, code in flips:
            occu_f[site] = code
        out = self._engine().eval_full(np.stack([occupancy, occu_f]))
        out[:, 0] = 0.0
        return out

    def exact_match_max_diameter(self, distance_vector):
        """Largest diameter for which all features are exactly matched (distance.py:307-332, :454-472)."""
        from . import sqs

        gd, fg = sqs.diameter_groups(self.cluster_subspace, self.feature_mode)
        return sqs.exact_match_max_diameter(distance_vector, gd, fg, self.match_tol)


class CorrelationDistanceProcessor(DistanceProcessor):
    """Distance from a target correlation vector (distance.py:185-333)."""

    feature_mode = capi.FEATURES_CORRELATIONS

    def __init__(self, supercell, supercell_matrix=None, use_concentration=False, target_vector=None,
                 match_weight=1.0, target_weights=None, match_tol=1e-5):
        model = supercell.model if supercell_matrix is None else getattr(supercell, "subspace", supercell)
        F = model.num_corr_functions
        target_vector = np.zeros(F) if target_vector is None else target_vector
        target_weights = np.ones(F - 1) if target_weights is None else target_weights
        super().__init__(supercell, supercell_matrix, target_vector, match_weight, match_tol, target_weights,
                         use_concentration)


class ClusterInteractionDistanceProcessor(DistanceProcessor):
    """Distance from a target cluster-interaction vector (distance.py:335-472); interaction tensors default to
    those of every coefficient 1 (:392-404)."""

    feature_mode = capi.FEATURES_INTERACTIONS

    def __init__(self, supercell, supercell_matrix=None, interaction_tensors=None, use_concentration=False,
                 target_vector=None, match_weight=1.0, target_weights=None, match_tol=1e-5):
        model = supercell.model if supercell_matrix is None else getattr(supercell, "subspace", supercell)
        F = model.num_orbits
        target_vector = np.zeros(F) if target_vector is None else target_vector
        target_weights = np.ones(F - 1) if target_weights is None else target_weights
        if interaction_tensors is not None and len(interaction_tensors) != F:
            raise ValueError(
                f"The number of cluster interaction tensors must match the number  of orbits in the subspace. Got "
                f"{len(interaction_tensors)} interaction tensors, but need {F}  for the given cluster_subspace.")
        self._interaction_tensors = interaction_tensors
        super().__init__(supercell, supercell_matrix, target_vector, match_weight, match_tol, target_weights,
                         use_concentration)

    @property
    def interaction_tensors(self):
        return self._interaction_tensors


class EwaldProcessor(Processor):
    """Electrostatic feature (smol/moca/processor/ewald.py:26-203).

    ``ewald_term`` is ``(ewald_inds, ewald_matrix[, charges])``; when None it is computed with the
    build's own Ewald sum (smol_amd.ewald; values unpinned vs pymatgen).  The optional
    per-entry ``charges`` (length M) let the engine factorise the matrix (compact Ewald / potential
    field); without them they are taken from the prim cell's oxidation states."""

    _scalar_feature = True

    def __init__(self, supercell, ewald_term=None, coefficient=1.0, use_term="total"):
        super().__init__(supercell, np.asarray(coefficient, dtype=np.float64))
        if ewald_term is None:  # (use_term: EwaldTerm.ewald_term_options, cofe/extern/ewald.py:28,159-177)
            from . import ewald as _ew

            ewald_term = _ew.supercell_ewald(supercell, use_term=use_term)
        self._ewald_inds = np.ascontiguousarray(ewald_term[0], dtype=np.int32)
        self.ewald_matrix = np.ascontiguousarray(ewald_term[1], dtype=np.float64)
        self._ewald_charges = (np.ascontiguousarray(ewald_term[2], dtype=np.float64)
                               if len(ewald_term) > 2 and ewald_term[2] is not None else "auto")
        self._feature_slice = slice(supercell.model.num_orbits, supercell.model.num_orbits + 1)

    def _table_kwargs(self):
        m = self.supercell.model
        return dict(
            feature_mode=capi.FEATURES_INTERACTIONS,
            ce_coefs_expansion=np.zeros(m.num_corr_functions),
            ce_natural=np.zeros(m.num_orbits),
            ewald=(self._ewald_inds, self.ewald_matrix),
            ewald_coef=float(self.coefs),
            ewald_charges=self._ewald_charges,
        )

    def compute_property(self, occupancy):
        return self.coefs * self.compute_feature_vector(occupancy)

    def compute_property_change(self, occupancy, flips):
        return self.coefs * self.compute_feature_vector_change(occupancy, flips)


class CompositeProcessor(Processor):
    """CE + external term (smol/moca/processor/composite.py:18-190)."""

    def __init__(self, supercell):
        super().__init__(supercell, np.zeros(0))
        self._processors = []

    @property
    def processors(self):
        return self._processors

    def add_processor(self, processor):
        if isinstance(processor, CompositeProcessor):
            raise AttributeError("A CompositeProcessor can not be added into another CompositeProcessor")
        if processor.supercell is not self.supercell:
            raise ValueError("processors must share the supercell")
        if len(self._processors) >= 2 or (self._processors and not isinstance(processor, EwaldProcessor)):
            raise ValueError("supported composition: one cluster processor followed by one EwaldProcessor")
        self._processors.append(processor)
        self.coefs = np.append(self.coefs, processor.coefs)
        self._eval_engine = None

    def _table_kwargs(self):
        if not self._processors:
            raise ValueError("empty CompositeProcessor")
        kw = dict(self._processors[0]._table_kwargs())
        if len(self._processors) == 2:
            ew = self._processors[1]
            kw["ewald"] = (ew._ewald_inds, ew.ewald_matrix)
            kw["ewald_coef"] = float(ew.coefs)
            kw["ewald_charges"] = ew._ewald_charges
        return kw


def _override_sublattices(tab, sublattices):
    """Re-point a TableSet's sublattice arrays at user-given Sublattice objects."""
    import ctypes as C

    subs = [s for s in sublattices if s.is_active]
    k = tab._keep
    k["sub_site_ptr"] = np.concatenate(([0], np.cumsum([len(s.active_sites) for s in subs]))).astype(np.int64)
    k["sub_active_sites"] = np.concatenate([s.active_sites for s in subs]).astype(np.int32)
    k["sub_code_ptr"] = np.concatenate(([0], np.cumsum([len(s.encoding) for s in subs]))).astype(np.int64)
    k["sub_codes"] = np.concatenate([s.encoding for s in subs]).astype(np.int32)
    probs = getattr(tab, "_user_probs", None)
    k["sub_probs"] = np.full(len(subs), 1.0 / len(subs)) if probs is None else np.asarray(probs, float)
    t = tab.struct
    t.n_sublattices = len(subs)
    for name, ct in (("sub_site_ptr", C.c_int64), ("sub_active_sites", C.c_int32),
                     ("sub_code_ptr", C.c_int64), ("sub_codes", C.c_int32), ("sub_probs", C.c_double)):
        setattr(t, name, k[name].ctypes.data_as(C.POINTER(ct)))


# --------------------------------------------------------------------------- #
class Ensemble:
    """Thermodynamic ensemble (smol/moca/ensemble.py:102-430)."""

    def __init__(self, processor, sublattices=None, chemical_potentials=None):
        if isinstance(processor, DistanceProcessor) and chemical_potentials is not None:
            raise ValueError("a distance ensemble takes no chemical potentials")
        self._processor = processor
        self._sublattices = processor.get_sublattices() if sublattices is None else sublattices
        self.natural_parameters = np.array(processor.coefs, dtype=np.float64)  # ensemble.py:126
        self.thermo_boundaries = {}
        self._chemical_potentials = None
        self._mu_table = None
        self.chemical_potentials = chemical_potentials

    @classmethod
    def from_cluster_expansion(cls, supercell, coefficients, processor_type="decomposition",
                               ewald_term=None, ewald_coefficient=None, **kwargs):
        """Counterpart of Ensemble.from_cluster_expansion (ensemble.py:133-217) for the
        build's own tables: ``supercell`` is a smol_amd.synth.SupercellTables and
        ``coefficients`` the expansion coefficients (num_corr_functions long).  When
        ``ewald_coefficient`` is given an EwaldProcessor is composed in."""
        if hasattr(supercell, "subspace") and hasattr(supercell, "ce_coefs"):
            # the reference's own call shape: (cluster_expansion, supercell_matrix) with an expansion
            # loaded from smol's serialization (smol_amd.mson.load_mson)
            return cls.from_mson(supercell, coefficients, processor_type=processor_type, **kwargs)
        model = supercell.model
        if processor_type == "decomposition":
            ce = ClusterDecompositionProcessor(supercell, model.cluster_interaction_tensors(coefficients))
        elif processor_type == "expansion":
            ce = ClusterExpansionProcessor(supercell, coefficients)
        else:
            raise ValueError(f"Processor type {processor_type} not supported!")
        if ewald_coefficient is None:
            return cls(ce, **kwargs)
        comp = CompositeProcessor(supercell)
        comp.add_processor(ce)
        comp.add_processor(EwaldProcessor(supercell, ewald_term, ewald_coefficient))
        return cls(comp, **kwargs)

    @classmethod
    def from_mson(cls, model, supercell_matrix, processor_type="decomposition", **kwargs):
        """Ensemble of a model serialized by smol (``ClusterExpansion.as_dict`` JSON / a notebook
        ``save_work`` file, or an already loaded smol_amd.mson.MsonClusterExpansion) on a
        supercell: what ``Ensemble.from_cluster_expansion(expansion, supercell_matrix)`` builds in
        the reference (ensemble.py:133-217) -- a cluster processor, composed with an
        EwaldProcessor carrying the last fitted coefficient when the subspace has an EwaldTerm."""
        from . import mson

        ce = model if isinstance(model, mson.MsonClusterExpansion) else mson.load_mson(model)
        cell = ce.subspace.supercell(supercell_matrix)
        ewald_term = coef = None
        if ce.subspace.ewald_term is not None:
            ewald_term, coef = ce.ewald_tables(cell), float(ce.coefs[-1])  # (inds, matrix, charges)
        return cls.from_cluster_expansion(cell, ce.ce_coefs, processor_type=processor_type,
                                          ewald_term=ewald_term, ewald_coefficient=coef, **kwargs)

    # -- properties ----------------------------------------------------------------
    @property
    def processor(self):
        return self._processor

    @property
    def num_sites(self):
        return self._processor.num_sites

    @property
    def num_energy_coefs(self):
        return len(self._processor.coefs)

    @property
    def system_size(self):
        return self._processor.size

    @property
    def sublattices(self):
        return self._sublattices

    @property
    def active_sublattices(self):
        return [s for s in self._sublattices if s.is_active]

    @property
    def restricted_sites(self):
        return np.concatenate([s.restricted_sites for s in self._sublattices] + [np.zeros(0, int)])

    @property
    def species(self):
        return [sp for s in self.active_sublattices for sp in s.species]

    @property
    def chemical_potentials(self):
        return self._chemical_potentials

    @chemical_potentials.setter
    def chemical_potentials(self, value):
        """ChemicalPotentialManager.__set__ (ensemble.py:35-73)."""
        had = self._chemical_potentials is not None
        if value is not None and isinstance(self._processor, DistanceProcessor):
            raise ValueError("a distance ensemble takes no chemical potentials")
        if value is None:
            if had:
                self.natural_parameters = self.natural_parameters[:-1]
                self.thermo_boundaries.pop("chemical_potentials", None)
            self._chemical_potentials, self._mu_table = None, None
            return
        value = {k: float(v) for k, v in value.items() if k in self.species}
        if set(value) != set(self.species):
            raise ValueError(
                "Chemical potentials given are missing species. Values must be given for each of "
                f"the following: {self.species}"
            )
        if not had:
            self.natural_parameters = np.append(self.natural_parameters, -1.0)  # ensemble.py:25,61-65
        self._chemical_potentials = value
        num_cols = max(max(s.encoding) for s in self._sublattices) + 1  # _build_table :90-99
        table = np.zeros((self.num_sites, num_cols))
        for s in self.active_sublattices:
            table[s.sites[:, None], s.encoding] = [value[sp] for sp in s.species]
        self._mu_table = table
        self.thermo_boundaries["chemical_potentials"] = value

    def walker_chemical_potentials(self, values):
        """Per-walker chemical potentials as a list of R dicts species -> value, from a sequence of R dicts or one
        dict species -> array of length R; every dict is held to the species of the active sublattices as the
        ``chemical_potentials`` setter holds its value."""
        if isinstance(values, dict):
            cols = {k: np.atleast_1d(np.asarray(v, dtype=np.float64)) for k, v in values.items()}
            lengths = {len(v) for v in cols.values()}
            if len(lengths) != 1:
                raise ValueError("per-walker chemical potentials: every species needs one value per walker")
            values = [{k: v[r] for k, v in cols.items()} for r in range(lengths.pop())]
        out = []
        for value in values:
            value = {k: float(v) for k, v in value.items() if k in self.species}
            if set(value) != set(self.species):
                raise ValueError(
                    "Chemical potentials given are missing species. Values must be given for each of "
                    f"the following: {self.species}"
                )
            out.append(value)
        return out

    def walker_mu_rows(self, values):
        """Per-walker chemical potentials in the layout of ``Engine.set_walker_mu`` -- (R, active sublattices, columns
        of the chemical-potential table) -- through the sublattices' species / encoding, the mapping the
        ``chemical_potentials`` setter builds its table with."""
        dicts = self.walker_chemical_potentials(values)
        num_cols = max(max(s.encoding) for s in self._sublattices) + 1
        act = self.active_sublattices
        rows = np.zeros((len(dicts), len(act), num_cols))
        for k, s in enumerate(act):
            rows[:, k, s.encoding] = [[d[sp] for sp in s.species] for d in dicts]
        return rows

    def walker_mu_dicts(self, rows):
        """The inverse of ``walker_mu_rows``: rows (R, active sublattices, columns) -> R dicts species -> value."""
        rows = np.asarray(rows, dtype=np.float64)
        return [{sp: float(row[k, c]) for k, s in enumerate(self.active_sublattices) for sp, c in zip(s.species, s.encoding)}
                for row in rows]

    def restrict_sites(self, sites):
        for s in self._sublattices:
            s.restrict_sites(sites)

    def reset_restricted_sites(self):
        for s in self._sublattices:
            s.reset_restricted_sites()

    def split_sublattice_by_species(self, sublattice_id, occu, species_in_partitions):
        """Replace sublattice ``sublattice_id`` by its split by occupying species
        (ensemble.py:288-321), e.g. Li/vacancy, transition metals and O of one site space as
        sublattices that swaps cannot mix.  The chemical potentials are rebuilt for the species that
        remain on active sublattices."""
        splits = self._sublattices[sublattice_id].split_by_species(occu, species_in_partitions)
        self._sublattices = (list(self._sublattices[:sublattice_id]) + splits
                             + list(self._sublattices[sublattice_id + 1:]))
        if self._chemical_potentials is not None:
            self.chemical_potentials = {sp: self._chemical_potentials[sp] for sp in self.species}

    def composition_space(self, charge_balanced=True, other_constraints=None, optimize_basis=False,
                          table_ergodic=False):
        """CompositionSpace over ALL sublattices of this ensemble, sizes reduced by their gcd,
        as TableFlip builds it (mcusher.py:489-518)."""
        from .composition import CompositionSpace

        sizes = np.array([len(s.sites) for s in self._sublattices], dtype=np.int64)
        sizes = sizes // np.gcd.reduce(sizes)
        spaces = [list(zip(s.species, s.charges)) for s in self._sublattices]
        return CompositionSpace(spaces, sizes, charge_neutral=charge_balanced,
                                other_constraints=other_constraints, optimize_basis=optimize_basis,
                                table_ergodic=table_ergodic)

    # -- tables for the engine -----------------------------------------------------
    def make_tables(self, flip_table=None, flip_weights=None, swap_weight=0.1):
        """Flattened tables of this ensemble, in its own site numbering (restricted sites and sublattices split by
        species leave active sites scattered: smolmc_create renumbers them behind the C-ABI, ``kernel_info`` then
        says "relabelled=1", and callers never see it)."""
        tab = self._processor._make_tables(mu_table=self._mu_table, sublattices=self._sublattices)
        if flip_table is not None:
            tab = self._with_flip_table(tab, flip_table, flip_weights, swap_weight)
        return tab

    def _with_flip_table(self, tab, flip_table, flip_weights, swap_weight):
        """Attach a TableFlip table.  The reference's flip vectors span the species of ALL
        sublattices in order (mcusher.py:489-503); the engine wants the active ones only."""
        import ctypes as C

        ft = np.atleast_2d(np.asarray(flip_table, dtype=np.int64))
        widths = [len(s.species) for s in self._sublattices]
        act = [s.is_active for s in self._sublattices]
        if ft.shape[1] == sum(widths):
            cols, off = [], 0
            for w, a in zip(widths, act):
                if a:
                    cols += list(range(off, off + w))
                elif np.any(ft[:, off:off + w] != 0):
                    raise ValueError("flip table changes species on an inactive sublattice")
                off += w
            ft = ft[:, cols]
        elif ft.shape[1] != sum(w for w, a in zip(widths, act) if a):
            raise ValueError("flip_table width does not match the sublattice species")
        ft = np.ascontiguousarray(ft, dtype=np.int32)
        fw = np.ones(2 * len(ft)) if flip_weights is None else np.asarray(flip_weights, dtype=np.float64)
        if len(fw) == len(ft):
            fw = np.repeat(fw, 2)
        if len(fw) != 2 * len(ft):
            raise ValueError(
                f"{len(fw)} weights provided. You must provide either 1* or 2* weights given "
                f"{len(ft)} flip vectors!"
            )
        tab._keep["flip_table"], tab._keep["flip_weights"] = ft, np.ascontiguousarray(fw)
        t = tab.struct
        t.n_flip_vectors = len(ft)
        t.swap_weight = float(swap_weight)
        t.flip_table = ft.ctypes.data_as(C.POINTER(C.c_int32))
        t.flip_weights = tab._keep["flip_weights"].ctypes.data_as(C.POINTER(C.c_double))
        return tab

    def _eval(self):
        # content key: a different restriction of the same size, or a new mu table that reuses
        # the id() of a freed one, must rebuild the handle
        key = (None if self._mu_table is None else self._mu_table.tobytes(),
               tuple(np.asarray(s.active_sites).tobytes() + b"|" + np.asarray(s.encoding).tobytes()
                     for s in self._sublattices))
        if getattr(self, "_eval_key", None) != key:
            self._eval_tables = self.make_tables()
            self._eval_engine = Engine(self._eval_tables, capi.make_config(1, device=_eval_device()),
                                       distance=self.distance_spec())
            self._eval_key = key
        return self._eval_engine

    def distance_spec(self, kB=1.0):
        """The distance objective of an ensemble on a distance processor (None otherwise)."""
        p = self._processor
        return p.distance_spec(kB) if isinstance(p, DistanceProcessor) else None

    def compute_feature_vector(self, occupancy):
        """ensemble.py:323-351."""
        return self._eval().eval_full(np.asarray(occupancy, dtype=np.int32)[None, :])[0]

    def compute_feature_vector_change(self, occupancy, step):
        """ensemble.py:353-376 (steps of up to SMOLMC_MAX_STEP_FLIPS flips, e.g. TableFlip's)."""
        return self._eval().eval_delta(np.asarray(occupancy, dtype=np.int32), capi.step_rows([list(step)]))[0]


# --------------------------------------------------------------------------- #
# kernels (specifications of what the engine runs for each walker)
# --------------------------------------------------------------------------- #
STEP_TYPES = {"flip": capi.STEP_FLIP, "swap": capi.STEP_SWAP, "table-flip": capi.STEP_TABLE_FLIP,
              "tableflip": capi.STEP_TABLE_FLIP}


# --------------------------------------------------------------------------- #
# bias terms (smol/moca/kernel/bias.py)
# --------------------------------------------------------------------------- #
class MCBias:
    """Host record of a bias term: builds the per-(site, species code) table the engine
    consumes (smol/moca/kernel/bias.py:24-93)."""

    bias_type = capi.BIAS_NONE
    penalty = 0.0

    def __init__(self, sublattices):
        self.sublattices = list(sublattices)
        self.active_sublattices = [s for s in self.sublattices if s.is_active]
        self.spec = dict(type=self.__class__.__name__)

    def _shape(self):
        return (sum(len(s.sites) for s in self.sublattices),
                max(int(max(s.encoding)) for s in self.sublattices) + 1)


class FugacityBias(MCBias):
    """Fugacity-fraction bias (bias.py:96-226): bias = sum_sites log f(site, species)."""

    bias_type = capi.BIAS_FUGACITY

    def __init__(self, sublattices, fugacity_fractions=None):
        super().__init__(sublattices)
        self._species = [set(s.species) for s in self.active_sublattices]
        if fugacity_fractions is None:
            # the reference takes the prim's site compositions (bias.py:139-141); the synthetic
            # prims carry none, so the default is the uniform composition
            fugacity_fractions = [{sp: 1.0 / len(s.species) for sp in s.species}
                                  for s in self.active_sublattices]
        self.fugacity_fractions = fugacity_fractions

    @property
    def fugacity_fractions(self):
        return self._fus

    @fugacity_fractions.setter
    def fugacity_fractions(self, value):
        value = [dict(v) for v in value]
        if not all(sum(fus.values()) == 1 for fus in value):
            raise ValueError("Fugacity ratios must add to one.")  # bias.py:161-162
        if len(value) != len(self._species):
            raise ValueError("one fugacity-fraction dictionary per active sublattice is required")
        for spec, vals in zip(self._species, value):
            if spec != set(vals.keys()):
                raise ValueError(
                    "Fugacity fractions given are missing or not valid species.\n"
                    f"Values must be given for each  of the following: {self._species}"
                )  # bias.py:163-170
        self._fus = value
        table = np.ones(self._shape())  # _build_fu_table (bias.py:208-226)
        for fus, s in zip(value, self.active_sublattices):
            table[s.sites[:, None], s.encoding] = np.array([fus[sp] for sp in s.species])[None, :]
        self._table = table
        self.spec["fugacity_fractions"] = value

    def compute_bias(self, occupancy):
        return float(sum(np.log(self._table[i, c]) for i, c in enumerate(occupancy)))


class SquareChargeBias(MCBias):
    """Square-charge bias (bias.py:229-277): bias = -penalty * (net charge)^2."""

    bias_type = capi.BIAS_SQUARE_CHARGE

    def __init__(self, sublattices, penalty=0.5):
        super().__init__(sublattices)
        if penalty <= 0:
            raise ValueError("Penalty factor should be > 0!")
        self.penalty = float(penalty)
        table = np.zeros(self._shape())
        for s in self.sublattices:
            table[s.sites[:, None], s.encoding] = np.array(s.charges, dtype=float)[None, :]
        self._table = table
        self.spec["penalty"] = self.penalty

    def compute_bias(self, occupancy):
        c = self._table[np.arange(len(occupancy)), occupancy].sum()
        return float(-self.penalty * c**2)


class SquareHyperplaneBias(MCBias):
    """Square hyperplane bias (bias.py:290-366): bias = -penalty * ||A n - b||^2 with n the
    species counts of the occupancy in "counts" format -- the species of every sublattice in
    order, concatenated over ALL sublattices (occu_utils.py:8-23,62-100) -- i.e. a penalty on the
    distance from composition constraints A n = b (per supercell).  Up to four hyperplanes."""

    bias_type = capi.BIAS_SQUARE_HYPERPLANE

    def __init__(self, sublattices, hyperplane_normals, hyperplane_intercepts, penalty=0.5):
        super().__init__(sublattices)
        if penalty <= 0:
            raise ValueError("Penalty factor should be > 0!")
        self.penalty = float(penalty)
        self._A = np.atleast_2d(np.array(hyperplane_normals, dtype=int))
        self._b = np.atleast_1d(np.array(hyperplane_intercepts, dtype=int))
        self.d = sum(len(s.species) for s in self.sublattices)
        if self._A.shape != (len(self._b), self.d):
            raise ValueError(f"hyperplane_normals must be [len(intercepts) x {self.d}] (one column per "
                             "species of every sublattice)")
        if not 1 <= len(self._b) <= 4:
            raise NotImplementedError("the engine supports 1 to 4 hyperplanes")
        # get_dim_ids_table (occu_utils.py:8-23): dimension of (site, code) in the counts vector
        n_sites, width = self._shape()
        self._dim_ids_table = -np.ones((n_sites, width), dtype=int)
        off = 0
        for s in self.sublattices:
            self._dim_ids_table[s.sites[:, None], s.encoding] = off + np.arange(len(s.species))[None, :]
            off += len(s.species)
        table = np.zeros((len(self._b), n_sites, width))
        valid = self._dim_ids_table >= 0
        for r in range(len(self._b)):
            table[r][valid] = self._A[r][self._dim_ids_table[valid]]
        self._table = table
        self.intercepts = self._b.astype(float)
        self.spec.update(penalty=self.penalty, hyperplane_normals=self._A.tolist(),
                         hyperplane_intercepts=self._b.tolist())

    def counts(self, occupancy):
        """occu_to_counts (occu_utils.py:62-100)."""
        ids = self._dim_ids_table[np.arange(len(occupancy)), occupancy]
        return np.bincount(ids[ids >= 0], minlength=self.d)

    def compute_bias(self, occupancy):
        n = self.counts(np.asarray(occupancy))
        return float(-self.penalty * np.sum((self._A @ n - self._b) ** 2))


BIAS_TYPES = {"fugacity": FugacityBias, "fugacity-bias": FugacityBias, "fugacitybias": FugacityBias,
              "square-charge": SquareChargeBias, "square-charge-bias": SquareChargeBias,
              "squarechargebias": SquareChargeBias,
              "square-hyperplane": SquareHyperplaneBias, "square-hyperplane-bias": SquareHyperplaneBias,
              "squarehyperplanebias": SquareHyperplaneBias}


def mcbias_factory(bias_type, sublattices, **kwargs):
    """bias.py mcbias_factory: class from its (hyphenated / camel-case) name."""
    key = str(bias_type).lower().replace("_", "-")
    if key not in BIAS_TYPES:
        raise NotImplementedError(f"{bias_type} is not implemented on the MI355X engine "
                                  f"(available: FugacityBias, SquareChargeBias, SquareHyperplaneBias).")
    return BIAS_TYPES[key](sublattices, **kwargs)


class MCKernel:
    """Per-walker kernel record (smol/moca/kernel/base.py:169-343).  Holds the parameters
    the reference keeps per kernel object; the stepping itself happens on the GPU."""

    kernel_type = None
    valid_bias = ("FugacityBias", "SquareChargeBias", "SquareHyperplaneBias")

    def __init__(self, ensemble, step_type, *args, seed=None, bias_type=None, bias_kwargs=None, **kwargs):
        # any spelling the reference's class_name_from_str accepts (class_utils.py:10-34):
        # "TableFlip", "Table-Flip", "table-flip", "Flip", "swap", ...
        key = str(step_type).lower().replace("-", "").replace("_", "")
        key = "table-flip" if key == "tableflip" else key
        if key not in STEP_TYPES:
            raise ValueError(
                f"{step_type} is not a valid MCUsher for this kernel (supported: Flip, Swap, TableFlip)."
            )
        step_type = key
        self._ensemble = ensemble
        self.natural_params = ensemble.natural_parameters
        self.step_type = step_type
        # MCUsher arguments (TableFlip: flip_table, flip_weights, swap_weight; mcusher.py:414-426)
        self.usher_kwargs = {k: kwargs[k] for k in ("flip_table", "flip_weights", "swap_weight")
                             if k in kwargs}
        if STEP_TYPES[step_type] == capi.STEP_TABLE_FLIP and self.usher_kwargs.get("flip_table") is None:
            # TableFlip.__init__ (mcusher.py:489-518): no table given -> build it from the
            # sublattices' species / charges with a CompositionSpace
            self.usher_kwargs["flip_table"] = ensemble.composition_space(
                charge_balanced=kwargs.get("charge_balanced", True),
                other_constraints=kwargs.get("other_constraints"),
                optimize_basis=kwargs.get("optimize_basis", False),
                table_ergodic=kwargs.get("table_ergodic", False),
            ).flip_table
        self._seed = seed if seed is not None else np.random.SeedSequence().entropy
        # the walker's own chemical potentials (Sampler.set_chemical_potentials), else the ensemble's
        self.chemical_potentials = ensemble.chemical_potentials
        self.spec = dict(kernel=self.__class__.__name__, seed=self._seed, step=step_type)
        self._bias = None
        if bias_type is not None:  # kernel/base.py:229-235
            self.bias = mcbias_factory(bias_type, ensemble.sublattices, **(bias_kwargs or {}))

    @property
    def bias(self):
        return self._bias

    @bias.setter
    def bias(self, bias):
        if self.valid_bias is None:
            raise ValueError("Cannot apply bias to Wang-Landau simulation!")  # wanglandau.py:127-128
        if bias.__class__.__name__ not in self.valid_bias:
            raise ValueError(f"{type(bias)} is not a valid MCBias for this kernel.")  # base.py:281-282
        self._bias = bias
        self.spec["bias"] = bias.spec

    @property
    def ensemble(self):
        return self._ensemble

    @property
    def seed(self):
        return self._seed

    @property
    def seed64(self):
        return np.uint64(int(self._seed) & 0xFFFFFFFFFFFFFFFF)

    # -- single-kernel stepping (kernel/base.py:100-166,287-289,345-366) -----------------
    # The reference steps ONE chain on the host through these; here they drive a one-walker
    # engine handle owned by the kernel (same kernels, same random stream as walker 0 of a
    # Sampler seeded with this kernel's seed).  An interface for tests, notebooks and custom
    # drivers -- a launch per step -- not the sampling path (Sampler.run).
    _owner = None  # (sampler, local walker) once a Sampler took this kernel

    def _solo(self):
        if getattr(self, "_solo_sampler", None) is None:
            container = Sampler._container_for(self._ensemble, self, 1)
            container.metadata["walker_range"] = (0, 1, 1)
            self._solo_sampler = Sampler([self], container, device=_eval_device(), _bind=False)
        return self._solo_sampler

    def _walker_trace(self, tr, w=0):
        return StepTrace(**{k: (np.asarray(v[w]).astype(np.int32) if k == "occupancy" else np.asarray(v[w]))
                        for k, v in tr.items()})

    def set_aux_state(self, occupancy, *args, **kwargs):
        """Load ``occupancy`` as this kernel's chain state: features, enthalpy, bias, Ewald field,
        species counts and (Wang-Landau) the current bin are recomputed from it on the device; the
        random stream, counters and Wang-Landau arrays carry on (kernel/base.py:287-289,
        wanglandau.py:290-300)."""
        self._solo()._load_state(np.asarray(occupancy))

    def compute_initial_trace(self, occupancy):
        """Trace of ``occupancy`` before any step (kernel/base.py:345-366)."""
        solo = self._solo()
        solo._load_state(np.asarray(occupancy))
        tr = self._walker_trace(solo._current_trace(solo._get_engine()))
        tr.accepted = np.array([True], dtype=bool)
        return tr

    def single_step(self, occupancy):
        """Attempt one MC step from ``occupancy`` (kernel/base.py:145-166): the step is proposed,
        priced and accepted / rejected on the device; ``occupancy`` is updated in place when the step
        is accepted and the trace carries ``delta_trace`` (features, enthalpy, bias changes of the
        PROPOSED step when accepted, zero otherwise -- the rejected proposal never leaves the GPU)."""
        solo = self._solo()
        eng = solo._get_engine()
        occupancy_in = occupancy
        solo._load_state(np.asarray(occupancy))
        before = solo._current_trace(eng)
        eng.run(1)
        tr = self._walker_trace(solo._current_trace(eng))
        delta = tr.delta_trace
        delta.features = tr.features - before.features[0]
        delta.enthalpy = np.array(tr.enthalpy[0] - before.enthalpy[0, 0], dtype=np.float64)
        if self._bias is not None:
            delta.bias = np.array(tr.bias[0] - before.bias[0, 0], dtype=np.float64)
        if isinstance(occupancy_in, np.ndarray):
            occupancy_in[:] = tr.occupancy
            tr.occupancy = occupancy_in
        self._last_trace = tr
        return tr

    @property
    def trace(self):
        """Trace of the last ``single_step`` / of this kernel's walker in its Sampler."""
        if getattr(self, "_last_trace", None) is not None:
            return self._last_trace
        if self._owner is not None:
            sampler, w = self._owner
            return self._walker_trace(sampler._current_trace(sampler._get_engine()), w)
        raise AttributeError("no step has been taken with this kernel yet")


class Metropolis(MCKernel):
    """Metropolis-Hastings kernel (smol/moca/kernel/metropolis.py:52-100)."""

    kernel_type = capi.KERNEL_METROPOLIS

    def __init__(self, ensemble, step_type, temperature, *args, seed=None, **kwargs):
        super().__init__(ensemble, step_type, *args, seed=seed, **kwargs)
        self.kB = kB
        self.temperature = temperature

    @property
    def temperature(self):
        return self._temperature

    @temperature.setter
    def temperature(self, temperature):
        self._temperature = float(temperature)
        self.beta = 1.0 / (self.kB * self._temperature)  # kernel/base.py:418-422


class UniformlyRandom(MCKernel):
    """A kernel that accepts every proposed step (smol/moca/kernel/random.py:16-38): the infinite-
    temperature limit of Metropolis -- exponent = log a-priori factor (+ delta bias) -- which is
    exactly what the engine's Metropolis kernels compute at beta = 0.  No ``temperature`` in its
    trace, as in the reference (it is not a thermal kernel)."""

    kernel_type = capi.KERNEL_METROPOLIS
    engine_temperature = np.inf  # beta = 1 / (kB T) = 0 on the device


class WangLandau(MCKernel):
    """Wang-Landau kernel (smol/moca/kernel/wanglandau.py:17-300)."""

    kernel_type = capi.KERNEL_WANGLANDAU
    valid_bias = None  # "Wang-Landau does not need bias" (wanglandau.py:24)

    def __init__(self, ensemble, step_type, min_enthalpy, max_enthalpy, bin_size, *args,
                 flatness=0.8, mod_factor=1.0, check_period=1000, update_period=1,
                 mod_update=None, seed=None, **kwargs):
        if min_enthalpy > max_enthalpy:
            raise ValueError("min_enthalpy can not be larger than max_enthalpy.")
        if (max_enthalpy - min_enthalpy) / bin_size <= 1:
            raise ValueError(
                "The values provided for min and max enthalpy and bin sizer result in a single bin!"
            )
        if mod_factor <= 0:
            raise ValueError("mod_factor must be greater than 0.")
        super().__init__(ensemble, step_type, *args, seed=seed, **kwargs)
        self.flatness, self.check_period, self.update_period = flatness, check_period, update_period
        self._m0 = mod_factor
        self._window = (min_enthalpy, max_enthalpy, bin_size)
        # mod_update (wanglandau.py:100-105): a number divides the modification factor on the device;
        # a callable is applied by the host at every flatness check (Sampler._wl_host_checks: the
        # launches are then split at the check period and the device never checks by itself)
        self._mod_callable = mod_update if callable(mod_update) else None
        self._mod_divisor = 2.0 if (mod_update is None or callable(mod_update)) else float(mod_update)
        self._levels = np.arange(min_enthalpy, max_enthalpy, bin_size)
        self.spec.update(min_enthalpy=min_enthalpy, max_enthalpy=max_enthalpy, bin_size=bin_size,
                         flatness=flatness, check_period=check_period, update_period=update_period,
                         levels=self._levels.tolist())

    @property
    def bin_size(self):
        return self._window[2]

    # -- state of this kernel's walker (wanglandau.py:150-173), read from the device -------
    def _wl_row(self):
        if self._owner is not None:
            sampler, w = self._owner
        else:
            sampler, w = self._solo(), 0
        wl = sampler._get_engine().get_wl()
        return {k: v[w] for k, v in wl.items()}

    @property
    def levels(self):
        """Visited enthalpy levels."""
        return self._levels[self._wl_row()["entropy"] > 0]

    @property
    def entropy(self):
        """log(dos) on visited levels."""
        S = self._wl_row()["entropy"]
        return S[S > 0]

    @property
    def dos(self):
        """Density of states on visited levels."""
        S = self.entropy
        return np.exp(S - S.min())

    @property
    def histogram(self):
        """Histogram on visited levels."""
        row = self._wl_row()
        return row["histogram"][row["entropy"] > 0]

    @property
    def mod_factor(self):
        return float(self._wl_row()["mod_factor"])


KERNELS = {"metropolis": Metropolis, "wanglandau": WangLandau, "wang-landau": WangLandau,
           "uniformlyrandom": UniformlyRandom, "uniformly-random": UniformlyRandom, "random": UniformlyRandom}


def mckernel_factory(kernel_type, ensemble, step_type, *args, **kwargs):
    """smol/moca/kernel/__init__.py:35-56."""
    key = str(kernel_type).lower().replace("_", "")
    if key not in KERNELS:
        raise NotImplementedError(f"{kernel_type} is not implemented on the MI355X engine.")
    return KERNELS[key](ensemble, step_type, *args, **kwargs)


# --------------------------------------------------------------------------- #
# sample storage
# --------------------------------------------------------------------------- #
def _merge_walkers(a):
    """(samples, walkers, ...) -> (samples * walkers, ...), sample-major, singleton axes dropped
    (what the reference calls "flat", container.py:514-519)."""
    return np.squeeze(a.reshape((a.shape[0] * a.shape[1],) + a.shape[2:]))


class SampleContainer:
    """Thinned samples of one Sampler (interface of smol/moca/sampler/container.py:25-660).

    Storage follows the engine, not the reference's pre-allocated append-and-slice arrays: the
    device ring of ``smolmc_run_sampled`` hands over whole *blocks* of samples
    ``(n, nwalkers, ...)``; the container keeps the blocks as delivered and joins them once,
    lazily, when a getter first needs them.  ``allocate`` / ``vacuum`` therefore have nothing
    to do and exist only because callers written for smol invoke them.  The HDF5 backend is
    replaced by ``to_npz`` / ``from_npz`` (h5py is not available)."""

    def __init__(self, ensemble, sample_trace, sampling_metadata=None):
        self._ensemble = ensemble
        self.natural_parameters = ensemble.natural_parameters
        self._num_energy_coefs = ensemble.num_energy_coefs
        self.metadata = dict(sampling_metadata or {})
        # name -> (dtype, per-sample shape): the schema of a block
        self._schema = {k: (v.dtype, tuple(v.shape[1:])) for k, v in sample_trace.items()}
        self._blocks = [{k: v for k, v in sample_trace.items()}] if len(sample_trace.enthalpy) else []
        self._joined = {}
        self._total_steps = 0
        # walker -> state point after the last exchange attempt (Sampler.run_exchange keeps it): what a block without
        # the state_point trace is filled with; None: the last sample's
        self._state_point_now = None

    # ---- block store ---------------------------------------------------------------
    def append_block(self, block, thinned_by):
        """Append ``n`` consecutive samples: ``block[name]`` has shape (n, nwalkers, ...)."""
        n = len(block["enthalpy"])
        entry = {}
        for name, (dtype, shape) in self._schema.items():
            if name == "state_point" and name not in block:  # (a plain run after run_exchange: nobody moves)
                now = self._state_point_now
                if now is None:  # (a restored container: where the last sample left the walkers)
                    if not self._blocks:
                        raise ValueError("a block without state_point for a container that traces it and holds no sample yet")
                    now = self._blocks[-1]["state_point"][-1]
                block = dict(block, state_point=np.broadcast_to(now, (n,) + shape))
            arr = np.asarray(block[name], dtype=dtype)
            # (occupancy: a run with keep_occupancy=False stores that of its final sample only)
            entry[name] = arr.reshape(((-1 if name == "occupancy" else n),) + shape)
        self._blocks.append(entry)
        self._joined = {}
        self._total_steps += n * int(thinned_by)

    def save_sampled_trace(self, trace, thinned_by):
        """One sample (container.py:384-397): a block of length one."""
        self.append_block({k: np.asarray(v)[None] for k, v in trace.items()}, thinned_by)

    def _col(self, name):
        """All samples of one traced value, (nsamples, nwalkers, ...).  Joined per name and on
        demand: a mean enthalpy does not concatenate gigabytes of occupancies."""
        if name not in self._joined:
            dt, shape = self._schema[name]
            parts = [b[name] for b in self._blocks]
            self._joined[name] = (parts[0] if len(parts) == 1 else np.concatenate(parts) if parts
                                  else np.empty((0,) + shape, dtype=dt))
            if len(parts) > 1:  # keep one copy: the blocks now alias the joined array
                at = 0
                for b in self._blocks:
                    n = len(b[name])
                    b[name] = self._joined[name][at:at + n]
                    at += n
        return self._joined[name]

    def _all(self):
        return {k: self._col(k) for k in self._schema}

    @property
    def _trace(self):
        return Trace(**self._all())

    def allocate(self, nsamples):
        """No-op: blocks arrive sized by the device ring (container.py:409-413 pre-allocates)."""

    def vacuum(self):
        """No-op: there is no slack to give back (container.py:415-418)."""

    def clear(self):
        self._blocks, self._joined, self._total_steps = [], {}, 0

    def last_occupancy(self):
        """Occupancies (nwalkers, N) of the most recent sample (no join of the blocks)."""
        return self._blocks[-1]["occupancy"][-1].astype(np.int32)

    def set_last_occupancy(self, occupancy):
        """The occupancy of the most recent sample, for a block that was recorded without occupancies
        (``Sampler.run(keep_occupancy=False)``): ``last_occupancy`` and a continuation work as before."""
        dt, shape = self._schema["occupancy"]
        self._blocks[-1]["occupancy"] = np.asarray(occupancy, dtype=dt).reshape((1,) + shape)
        self._joined.pop("occupancy", None)

    def _need_occupancies(self):
        if any(len(b["occupancy"]) != len(b["enthalpy"]) for b in self._blocks):
            raise ValueError("these samples were taken with keep_occupancy=False: only the occupancy of the final sample of "
                             "each run is stored (last_occupancy); sample with keep_occupancy=True for per-sample occupancies")

    # ---- bookkeeping -----------------------------------------------------------------
    ensemble = property(lambda self: self._ensemble)
    sublattices = property(lambda self: self._ensemble.sublattices)
    num_samples = property(lambda self: sum(len(b["enthalpy"]) for b in self._blocks))
    total_mc_steps = property(lambda self: self._total_steps)
    shape = property(lambda self: self._schema["occupancy"][1])
    traced_values = property(lambda self: tuple(self._schema))

    def __len__(self):
        return self.num_samples

    def sampling_efficiency(self, discard=0, flat=True):
        """Fraction of recorded samples whose last step was accepted (container.py:131-142)."""
        acc = self._col("accepted")[discard:]
        eff = acc.mean(axis=0)
        return eff.mean() if flat else eff

    # ---- selection + reductions --------------------------------------------------------
    def _select(self, name, discard, thin_by):
        """Samples discard + thin_by - 1, discard + 2 thin_by - 1, ... of one traced value in
        its storage dtype (the reference's selection rule, container.py:181-199)."""
        if name == "occupancy":
            self._need_occupancies()
        return self._col(name)[discard + thin_by - 1:: thin_by]

    def get_trace_value(self, name, discard=0, thin_by=1, flat=True):
        picked = self._select(name, discard, thin_by)
        if name == "occupancy":  # stored as bytes, the reference's trace.occupancy is int32
            picked = picked.astype(np.int32)
        return _merge_walkers(picked) if flat else picked

    def mean_trace_value(self, name, discard=0, thin_by=1, flat=True):
        return self.get_trace_value(name, discard, thin_by, flat).mean(axis=0)

    def trace_value_variance(self, name, discard=0, thin_by=1, flat=True):
        return self.get_trace_value(name, discard, thin_by, flat).var(axis=0)

    def get_temperatures(self, discard=0, thin_by=1):
        return self.get_trace_value("temperature", discard, thin_by)

    def by_state_point(self, name, discard=0):
        """A traced value regrouped by the state point it was sampled at (``Sampler.run_exchange``): (npoints,
        nsamples, ...) instead of (nsamples, nwalkers, ...).  Every sample holds each point once, so nothing is
        dropped: row p is the chain of point p, whichever walker was there."""
        if "state_point" not in self._schema:
            raise ValueError("these samples carry no state_point trace: they were not taken by Sampler.run_exchange")
        point = self._col("state_point")[discard:, :, 0].astype(np.int64)
        if name == "occupancy":
            self._need_occupancies()
        vals = self._col(name)[discard:]
        if name == "occupancy":
            vals = vals.astype(np.int32)
        out = np.empty_like(vals)
        out[np.arange(len(point))[:, None], point] = vals
        return np.swapaxes(out, 0, 1)

    def get_energies(self, discard=0, thin_by=1, flat=True):
        """Energy = natural parameters . features over the energy coefficients only
        (the chemical work / bias terms are not part of it, container.py:217-233)."""
        n = self._num_energy_coefs
        if len(self.natural_parameters) == n:
            return self.get_trace_value("enthalpy", discard, thin_by, flat)
        feats = self.get_trace_value("features", discard, thin_by, flat=False)
        energies = (feats[..., :n] @ self.natural_parameters[:n])[..., None]
        return _merge_walkers(energies) if flat else energies

    def _argmin_occupancy(self, values, discard, thin_by, flat):
        where = values.argmin(axis=0)
        occ = self._select("occupancy", discard, thin_by)
        if flat:
            occ = _merge_walkers(occ)
            return occ[where].astype(np.int32)
        return occ[where, np.arange(self.shape[0])][0].astype(np.int32)

    def _minimum_from_record(self, energy, discard, thin_by, flat):
        """The minimum-occupancy getters of samples taken with keep_occupancy=False: answered from the per-walker minima
        record the sampler kept on the device (``Sampler.from_ensemble(minima=)``), or None when it cannot answer.  The
        record holds every walker's lowest sample, earliest first among equals: the flat argmin is its lowest entry."""
        rec = self.minima
        if rec is None or rec.spec.n_axes or discard != 0 or thin_by != 1 or rec.offers != self.num_samples:
            return None
        n = self._num_energy_coefs
        same = energy and len(self.natural_parameters) == n
        if rec.spec.weights is None:
            if energy and not same:
                return None
        elif not (energy or same) or not np.array_equal(rec.spec.weights, self.natural_parameters[:n]):
            return None
        if not rec.filled.any():
            return None
        if not flat:
            # (container.py:316-318 takes EVERY walker's occupancy at the sample where walker 0 was lowest: the
            # companions the record keeps next to walker 0's entry)
            return None if rec.companions is None or rec.sample[0] < 0 else rec.companions.astype(np.int32)
        order = np.lexsort((rec.walker, rec.sample, np.where(rec.filled, rec.value, np.inf)))
        return rec.occupancy[order[0]].astype(np.int32)

    def _minimum_occupancy(self, energy, discard, thin_by, flat):
        if any(len(b["occupancy"]) != len(b["enthalpy"]) for b in self._blocks):
            occ = self._minimum_from_record(energy, discard, thin_by, flat)
            if occ is not None:
                return occ
            raise ValueError("these samples were taken with keep_occupancy=False and no minima record answers this call: "
                             "sample with Sampler.from_ensemble(minima=Minima.per_walker(...)) for the quantity asked for "
                             "(discard=0, thin_by=1), or with keep_occupancy=True")
        values = self.get_energies(discard, thin_by, flat) if energy else self.get_enthalpies(discard, thin_by, flat)
        return self._argmin_occupancy(values, discard, thin_by, flat)

    def get_minimum_enthalpy_occupancy(self, discard=0, thin_by=1, flat=True):
        return self._minimum_occupancy(False, discard, thin_by, flat)

    def get_minimum_energy_occupancy(self, discard=0, thin_by=1, flat=True):
        return self._minimum_occupancy(True, discard, thin_by, flat)

    @property
    def minima(self):
        """The ``minima.MinimaRecord`` the sampler stored after its last run (None: sampled without ``minima=``)."""
        d = self.metadata.get("minima")
        if d is None:
            return None
        from .minima import MinimaRecord

        return MinimaRecord.from_dict(d)

    def set_minima(self, record):
        self.metadata["minima"] = record.as_dict()

    # ---- compositions --------------------------------------------------------------------
    def get_sublattice_species_counts(self, sublattice, discard=0, thin_by=1, flat=True):
        """Counts of each species of one sublattice, last axis ordered like its site space
        (container.py:349-382)."""
        if not any(sublattice is s for s in self.sublattices):
            raise ValueError(
                "Sublattice provided is not recognized.\n Provide one included in the sublattices "
                "attribute of this SampleContainer."
            )
        counts = self._counted_on_device(sublattice, discard, thin_by)
        if counts is None:
            occ = self._select("occupancy", discard, thin_by)[..., sublattice.sites]
            counts = np.stack([(occ == code).sum(axis=-1) for code in np.asarray(sublattice.encoding)],
                              axis=-1).astype(float)
        return _merge_walkers(counts) if flat else counts

    def _counted_on_device(self, sublattice, discard, thin_by):
        """The species counts of one sublattice read from the ``species_counts`` trace (counted on the device,
        ``Sampler.from_ensemble(observables=)``) when the kinds are the default ones and the sublattice has a block of
        its own; else None: the occupancies are scanned."""
        obs = self.metadata.get("observables")
        if "species_counts" not in self._schema or not obs or not obs.get("default_kinds"):
            return None
        from .observables import block_counts

        picked = self._select("species_counts", discard, thin_by)
        blk = block_counts(np.asarray(obs["kind_base"]), np.asarray(obs["site_ncodes"]), picked, sublattice.sites)
        if blk is None or np.asarray(sublattice.encoding).max(initial=0) >= blk.shape[-1]:
            return None
        # (C order, like the scan's stack: the reductions then add in the same order and give the same bits)
        return blk[..., np.asarray(sublattice.encoding)].astype(float, order="C")

    def get_pair_counts(self, discard=0, thin_by=1, flat=True):
        """The ``pair_counts`` trace: (..., n_shells, K, K) int32 cells of every sample, bonds as listed."""
        return self.get_trace_value("pair_counts", discard, thin_by, flat)

    def warren_cowley(self, discard=0, thin_by=1, flat=True):
        """Warren-Cowley short-range order alpha_ab(shell) of every sample, (..., n_shells, K, K), from the
        ``species_counts`` and ``pair_counts`` traces (``observables.warren_cowley``)."""
        from .observables import warren_cowley

        if "pair_counts" not in self._schema:
            raise ValueError("these samples carry no pair_counts trace: sample with Sampler.from_ensemble(observables=)")
        wc = warren_cowley(self._select("species_counts", discard, thin_by), self._select("pair_counts", discard, thin_by))
        return wc.reshape((wc.shape[0] * wc.shape[1],) + wc.shape[2:]) if flat else wc

    def get_pattern_counts(self, discard=0, thin_by=1, flat=True):
        """The ``pattern_counts`` trace: (..., n_cells) int32 cells of every sample, tuples as listed; the metadata's
        ``patterns`` entry says where every set's cells start (``cell_ptr``) and what its classes are."""
        if "pattern_counts" not in self._schema:
            raise ValueError("these samples carry no pattern_counts trace: sample with Sampler.from_ensemble(patterns=)")
        return self.get_trace_value("pattern_counts", discard, thin_by, flat)

    def pattern_probabilities(self, discard=0, thin_by=1, flat=True):
        """Pattern probabilities of every sample, (..., n_cells): every set's cells over their sum
        (``patterns.probabilities``)."""
        from .patterns import probabilities

        cells = self.get_pattern_counts(discard, thin_by, flat)
        return probabilities(cells, [int(x) for x in self.metadata["patterns"]["cell_ptr"]])

    def get_environment_counts(self, discard=0, thin_by=1, flat=True):
        """The ``environment_counts`` trace: (..., n_cells) int32 cells of every sample; the metadata's ``environments``
        entry says where every set's cells start (``cell_ptr``), its width and what its classes are."""
        if "environment_counts" not in self._schema:
            raise ValueError("these samples carry no environment_counts trace: sample with Sampler.from_ensemble(environments=)")
        return self.get_trace_value("environment_counts", discard, thin_by, flat)

    def get_species_counts(self, discard=0, thin_by=1, flat=True):
        """Counts per species name summed over the sublattices that host it (container.py:336-347)."""
        out = {}
        for sub in self.sublattices:
            counts = self.get_sublattice_species_counts(sub, discard, thin_by, flat)
            for j, sp in enumerate(sub.species):
                out[sp] = out.get(sp, 0) + counts[..., j].astype(np.int64)
        return out

    def get_sublattice_compositions(self, sublattice, discard=0, thin_by=1, flat=True):
        return self.get_sublattice_species_counts(sublattice, discard, thin_by, flat) / len(sublattice.sites)

    def get_compositions(self, discard=0, thin_by=1, flat=True):
        """Fraction of ALL sites held by each species (container.py:240-243)."""
        return {sp: c / self.shape[1] for sp, c in self.get_species_counts(discard, thin_by, flat).items()}

    def mean_composition(self, discard=0, thin_by=1, flat=True):
        return {sp: c.mean(axis=0) for sp, c in self.get_compositions(discard, thin_by, flat).items()}

    def composition_variance(self, discard=0, thin_by=1, flat=True):
        return {sp: c.var(axis=0) for sp, c in self.get_compositions(discard, thin_by, flat).items()}

    def mean_sublattice_composition(self, sublattice, discard=0, thin_by=1, flat=True):
        return self.get_sublattice_compositions(sublattice, discard, thin_by, flat).mean(axis=0)

    def sublattice_composition_variance(self, sublattice, discard=0, thin_by=1, flat=True):
        return self.get_sublattice_compositions(sublattice, discard, thin_by, flat).var(axis=0)

    def get_orbit_factors(self, function_orbit_ids, discard=0, thin_by=1, flat=True):
        """Sum of natural_parameter * feature over the functions of each orbit id
        (container.py:269-280)."""
        vals = self.natural_parameters * self.get_feature_vectors(discard=discard, thin_by=thin_by, flat=flat)
        ids = np.asarray(function_orbit_ids)
        return np.array([np.sum(vals[..., ids == i]) for i in range(len(self.natural_parameters))])

    # ---- persistence -----------------------------------------------------------------------
    def to_npz(self, path):
        """Checkpoint (.npz stand-in for to_hdf5, container.py:615): one array per trace name +
        nsamples / total_mc_steps, like the HDF5 'trace' group."""
        extra = {}
        wmu = self.metadata.get("walker_chemical_potentials")
        if wmu is not None:  # per-walker chemical potentials (Sampler.set_chemical_potentials)
            extra = {"meta/walker_mu_species": np.array(wmu["species"]), "meta/walker_mu_values": np.asarray(wmu["values"], dtype=np.float64)}
        pts = self.metadata.get("state_points")
        if pts is not None:  # the mu-T grid of Sampler.run_exchange
            extra.update({"meta/state_point_species": np.array(pts["species"]),
                          "meta/state_point_temperatures": np.asarray(pts["temperatures"], dtype=np.float64),
                          "meta/state_point_values": np.asarray(pts["chemical_potentials"], dtype=np.float64),
                          "meta/state_point_shape": np.asarray(pts["shape"], dtype=np.int64)})
        pop = self.metadata.get("population_annealing")
        if pop is not None:  # the record of Sampler.anneal_population
            extra.update({"meta/pop_anneal_temperatures": np.asarray(pop["temperatures"], dtype=np.float64),
                          "meta/pop_anneal_seed": np.asarray([pop["populations"], pop["seed"]], dtype=np.int64),
                          "meta/pop_anneal_log_partition_ratio": np.asarray(pop["log_partition_ratio"], dtype=np.float64),
                          "meta/pop_anneal_n_families": np.asarray(pop["n_families"], dtype=np.int64),
                          "meta/pop_anneal_rho_t": np.asarray(pop["rho_t"], dtype=np.float64)})
            if "overlap" in pop:  # an adaptive schedule: the target and the overlap of every step and population
                extra["meta/pop_anneal_overlap"] = np.asarray(pop["overlap"], dtype=np.float64).reshape(len(pop["overlap"]), -1)
        for fam in FAMILIES:  # what the specs of the derived traces said of themselves
            meta = self.metadata.get(fam.keyword)
            if meta is not None and fam.saved:
                extra.update(fam.spec.metadata_to_npz(meta))
        rec = self.minima
        if rec is not None:  # the minima record: its arrays, the spec and the two counters
            spec = rec.spec
            extra.update({f"meta/minima_{f}": getattr(rec, f) for f in
                          ("value", "enthalpy", "features", "occupancy", "counts", "walker", "sample", "step")})
            if rec.companions is not None:
                extra["meta/minima_companions"] = rec.companions
            extra.update({"meta/minima_shape": np.asarray([rec.offers, rec.n_walkers, spec.n_weights, spec.n_axes], dtype=np.int64),
                          "meta/minima_weights": np.zeros(0) if spec.weights is None else spec.weights,
                          "meta/minima_axis_weights": spec.axis_weights, "meta/minima_bins": spec.bins,
                          "meta/minima_extents": spec.extents})
        np.savez_compressed(path, nsamples=self.num_samples, total_mc_steps=self._total_steps,
                            **{f"trace/{k}": v for k, v in self._all().items()}, **extra)

    def get_chemical_potentials(self):
        """(walkers, species of the active sublattices): the chemical potentials every walker was sampled at -- the
        per-walker values of ``Sampler.set_chemical_potentials``, else the ensemble's for every walker."""
        wmu = self.metadata.get("walker_chemical_potentials")
        if wmu is not None:
            return np.asarray(wmu["values"], dtype=np.float64)
        mu = self._ensemble.chemical_potentials
        if mu is None:
            raise ValueError("the ensemble has no chemical potentials")
        return np.tile([mu[sp] for sp in self._ensemble.species], (self.shape[0], 1))

    def get_sampled_species(self, indices, flat=True):
        """Species of every site for the samples ``indices`` -- what ``get_sampled_structures``
        (container.py:144-181) returns as pymatgen Structures, here as lists of species names in site
        order (``Processor.decode_occupancy``; lattice and coordinates are the supercell's own)."""
        indices = [indices] if isinstance(indices, (int, np.integer)) else list(indices)
        occupancies = self.get_occupancies(flat=flat)[indices]
        decode = self._ensemble.processor.decode_occupancy
        if flat:
            return [decode(occu) for occu in occupancies]
        return [[decode(occu) for occu in walkers] for walkers in occupancies]

    def get_sampled_structures(self, indices, flat=True):
        raise NotImplementedError("pymatgen Structures are not built here; get_sampled_species(indices) gives the "
                                  "species of every site, in the site order of the supercell")

    def to_hdf5(self, file_path):
        """container.py:615: HDF5 needs h5py, which this build does not depend on -- the same content
        goes to ``to_npz`` (one file) or to the streaming directory of ``get_backend``."""
        raise NotImplementedError("HDF5 output needs h5py; use to_npz(path) / from_npz, or Sampler.run(..., "
                                  "stream_chunk=n, stream_file=directory) and SampleContainer.from_stream")

    @classmethod
    def from_hdf5(cls, file_path, swmr_mode=False, ensemble=None):
        raise NotImplementedError("HDF5 input needs h5py; use from_npz(path, ensemble) or from_stream(directory, ensemble)")

    def as_dict(self):
        """JSON-able record of the samples (container.py:525-547): every traced value as nested
        lists with its dtype, the counters and the sampling metadata.  The ensemble itself is a set
        of flattened tables here, not a serialisable object: ``from_dict`` takes it as an argument."""
        return {
            "@class": self.__class__.__name__,
            "nsamples": self.num_samples,
            "total_mc_steps": self._total_steps,
            "metadata": _jsonable(self.metadata),
            "sublattices": [sub.as_dict() for sub in self.sublattices],
            "natural_parameters": np.asarray(self.natural_parameters).tolist(),
            "trace": {k: {"dtype": str(v.dtype), "data": v.tolist()} for k, v in self._all().items()},
        }

    @classmethod
    def from_dict(cls, d, ensemble):
        """Container of ``as_dict``'s record on ``ensemble`` (container.py:549-575)."""
        arrays = {k: np.array(v["data"], dtype=np.dtype(v["dtype"])) for k, v in d["trace"].items()}
        n = int(d["nsamples"])
        c = cls(ensemble, Trace(**{k: v[:0] for k, v in arrays.items()}), d.get("metadata"))
        if n:
            c.append_block({k: v[:n] for k, v in arrays.items()}, 0)
        c._total_steps = int(d["total_mc_steps"])
        return c

    # Streaming backend: a directory of part-NNNNNN.npz files + manifest.json.  It stands in for the
    # HDF5 file of the reference (container.py:420-437 flush_to_backend, :439-504 get_backend; h5py is
    # not available here): every flush writes the samples held in memory as the next part and drops
    # them, so a long run keeps at most one chunk on the host.  Appending to an existing directory
    # continues its numbering, as the reference appends to an existing file.
    def get_backend(self, file_path, alloc_nsamples=0, swmr_mode=False):
        return NpzStream(file_path, self)

    def flush_to_backend(self, backend):
        backend.write(self)
        self.clear()

    @classmethod
    def from_stream(cls, path, ensemble):
        """All parts of a streaming directory as one container (the reference's from_hdf5)."""
        man = NpzStream.read_manifest(path)
        c = None
        for i in range(man["nparts"]):
            d = np.load(os.path.join(path, f"part-{i:06d}.npz"))
            arrays = {k[6:]: d[k] for k in d.files if k.startswith("trace/")}
            if c is None:
                c = cls(ensemble, Trace(**{k: v[:0] for k, v in arrays.items()}), man.get("metadata"))
            c.append_block(arrays, 0)
        if c is None:
            raise ValueError(f"{path} holds no samples")
        c._total_steps = int(man["total_mc_steps"])
        return c

    @classmethod
    def from_npz(cls, path, ensemble):
        d = np.load(path)
        n = int(d["nsamples"])
        arrays = {k[6:]: d[k][:n] for k in d.files if k.startswith("trace/")}
        c = cls(ensemble, Trace(**{k: v[:0] for k, v in arrays.items()}))
        c.append_block(arrays, 0)
        c._total_steps = int(d["total_mc_steps"])
        if "meta/walker_mu_values" in d.files:
            c.metadata["walker_chemical_potentials"] = dict(species=[str(s) for s in d["meta/walker_mu_species"]],
                                                            values=d["meta/walker_mu_values"].tolist())
        if "meta/state_point_values" in d.files:
            c.metadata["state_points"] = dict(species=[str(s) for s in d["meta/state_point_species"]],
                                              temperatures=d["meta/state_point_temperatures"].tolist(),
                                              chemical_potentials=d["meta/state_point_values"].tolist(),
                                              shape=[int(x) for x in d["meta/state_point_shape"]])
        for fam in FAMILIES:
            meta = fam.spec.metadata_from_npz(d) if fam.saved else None
            if meta is not None:
                c.metadata[fam.keyword] = meta
        if "meta/minima_shape" in d.files:
            offers, nw, n_weights, n_axes = (int(x) for x in d["meta/minima_shape"])
            rec = {f: d[f"meta/minima_{f}"] for f in ("value", "enthalpy", "features", "occupancy", "counts", "walker", "sample", "step")}
            rec.update(offers=offers, n_walkers=nw,
                       companions=d["meta/minima_companions"] if "meta/minima_companions" in d.files else None,
                       spec=dict(weights=d["meta/minima_weights"].tolist() if n_weights else None,
                                 axis_weights=d["meta/minima_axis_weights"].tolist() if n_axes else None,
                                 bins=d["meta/minima_bins"].tolist(), extents=d["meta/minima_extents"].tolist()))
            c.metadata["minima"] = rec
        if "meta/pop_anneal_temperatures" in d.files:
            c.metadata["population_annealing"] = dict(
                temperatures=d["meta/pop_anneal_temperatures"].tolist(),
                populations=int(d["meta/pop_anneal_seed"][0]), seed=int(d["meta/pop_anneal_seed"][1]),
                log_partition_ratio=d["meta/pop_anneal_log_partition_ratio"].tolist(),
                n_families=d["meta/pop_anneal_n_families"].tolist(), rho_t=d["meta/pop_anneal_rho_t"].tolist())
            if "meta/pop_anneal_overlap" in d.files:
                c.metadata["population_annealing"]["overlap"] = d["meta/pop_anneal_overlap"].tolist()
        return c


class NpzStream:
    """Writer side of the streaming directory (see SampleContainer.get_backend)."""

    def __init__(self, path, container):
        self.path = str(path)
        os.makedirs(self.path, exist_ok=True)
        if os.path.exists(os.path.join(self.path, "manifest.json")):
            self.manifest = self.read_manifest(self.path)
            if self.manifest["traced_values"] != list(container.traced_values) or \
                    self.manifest["shape"] != list(container.shape):
                raise RuntimeError(
                    f"Backend file {self.path} holds samples of another shape / set of traced values."
                )
        else:
            self.manifest = dict(nparts=0, nsamples=0, total_mc_steps=0, shape=list(container.shape),
                                 traced_values=list(container.traced_values),
                                 metadata=_jsonable(container.metadata))
            self._save_manifest()

    @staticmethod
    def read_manifest(path):
        with open(os.path.join(path, "manifest.json")) as f:
            return json.load(f)

    def _save_manifest(self):
        tmp = os.path.join(self.path, "manifest.json.tmp")
        with open(tmp, "w") as f:
            json.dump(self.manifest, f)
        os.replace(tmp, os.path.join(self.path, "manifest.json"))  # readers never see a torn manifest

    def write(self, container):
        n = container.num_samples
        if n == 0:
            return
        np.savez(os.path.join(self.path, f"part-{self.manifest['nparts']:06d}.npz"),
                 **{f"trace/{k}": v for k, v in container._all().items()})
        self.manifest["nparts"] += 1
        self.manifest["nsamples"] += n
        self.manifest["total_mc_steps"] += container.total_mc_steps
        self._save_manifest()

    def close(self):
        pass


def _jsonable(x):
    if isinstance(x, dict):
        return {str(k): _jsonable(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_jsonable(v) for v in x]
    if isinstance(x, np.ndarray):
        return x.tolist()
    if isinstance(x, (np.integer, np.floating, np.bool_)):
        return x.item()
    return x if isinstance(x, (str, int, float, bool, type(None))) else repr(x)


def _install_reductions():
    """get_X / mean_X / X_variance / get_minimum_X for the scalar-like traced values: the
    reference writes these ~20 methods out one by one (container.py:201-333); they all are one
    selection followed by one NumPy reduction."""
    plural = {"occupancy": "occupancies", "enthalpy": "enthalpies", "features": "feature_vectors"}
    singular = {"enthalpy": "enthalpy", "features": "feature_vector", "energy": "energy"}

    def selector(field):
        def get(self, discard=0, thin_by=1, flat=True):
            return self.get_trace_value(field, discard, thin_by, flat)
        return get

    for field, name in plural.items():
        fn = selector(field)
        fn.__name__ = f"get_{name}"
        setattr(SampleContainer, fn.__name__, fn)

    def reducer(getter_name, how):
        def red(self, discard=0, thin_by=1, flat=True):
            return getattr(getattr(self, getter_name)(discard, thin_by, flat), how)(axis=0)
        return red

    for field, name in singular.items():
        getter = "get_energies" if field == "energy" else f"get_{plural[field]}"
        for pattern, how in ((f"mean_{name}", "mean"), (f"{name}_variance", "var")):
            fn = reducer(getter, how)
            fn.__name__ = pattern
            setattr(SampleContainer, pattern, fn)
        if field != "features":
            fn = reducer(getter, "min")
            fn.__name__ = f"get_minimum_{name}"
            setattr(SampleContainer, fn.__name__, fn)


_install_reductions()


# --------------------------------------------------------------------------- #
class Sampler:
    """MCMC driver (smol/moca/sampler/sampler.py:22-445) on the batched GPU engine.

    Multi-GPU: walkers are independent (sampler.py:111-116,436-440), so a Sampler built with
    ``rank`` / ``world_size`` (default: taken from an initialised torch.distributed process
    group, else a single rank) owns only its contiguous block ``walker_range`` of the
    ``nwalkers`` global walkers on the device of its rank.  Seeds and initial occupancies are
    indexed by GLOBAL walker, so walker g runs the same chain whatever the world size;
    ``global_statistics`` all-reduces the running sums over ranks (RCCL), the only collective."""

    def __init__(self, kernels, container, engine=None, walker_range=None, device=0, world_size=1,
                 _bind=True):
        self._kernels = kernels
        if _bind:  # kernel-level accessors (WangLandau.dos, MCKernel.trace) read this sampler's engine
            for w, k in enumerate(kernels):
                k._owner = (self, w)
        self._container = container
        self._container.metadata["kernels"] = [k.spec for k in kernels]
        self._engine = engine
        self._engine_key = None
        self._walker_range = walker_range or (0, len(kernels))
        self._device, self._world = int(device), int(world_size)
        self._state_loaded = False  # walker states uploaded to the engine at least once
        self._resume_at = None      # (container, its sample count) the device state equals, see _load_state
        self._kept_last = False     # the container holds the one sample a streamed run kept (keep_last_chunk)
        self._walker_mu = None      # per-walker chemical potentials of this rank's walkers (list of dicts), or None
        self._walker_mu_dirty = False  # ... not yet on the engine
        self._wl_windows = None     # replica-exchange Wang-Landau: the parallel.WLWindows of this sampler's walkers
        self._wl_synchronise = False  # ... whose copies are merged between launches: the handle has check period 0
        self._traced = {}           # family name (families.FAMILIES) -> the spec evaluated on the device for every sample
        self._minima = None         # minima.Minima: the lowest samples are kept on the device, or None
        self._minima_offers = 0     # samples offered to the record since it was last emptied
        self._statistics = None     # statistics.Statistics: moments, blocking sums and a histogram kept on the device, or None
        self._grid = None           # parallel.GridExchange of the last run_exchange across a mu-T grid, or None
        self._grid_base = None      # ... engine state point q is the grid's point _grid_base[q] since that call began
        self._grid_record_base = None  # the numbering under which the record has taken rows since it was last emptied
        self._grid_keys_mixed = False  # a record keyed by state point took rows under two different numberings

    @classmethod
    def from_ensemble(cls, ensemble, *args, step_type=None, kernel_type=None, seeds=None,
                      nwalkers=1, rank=None, world_size=None, device=None, chemical_potentials=None, windows=None,
                      observables=None, minima=None, statistics=None, structure_factor=None, connectivity=None,
                      patterns=None, environments=None, synchronise=False, **kwargs):
        """sampler.py:52-139: default step 'flip' when chemical potentials are set else
        'swap'; default kernel Metropolis; one kernel (seed) per walker.

        ``windows``: a ``parallel.WLWindows`` -- replica-exchange Wang-Landau.  ``min_enthalpy``, ``max_enthalpy``
        and ``bin_size`` are then the GLOBAL range the windows cut up; kernel w is estimator w of ``windows`` and is
        built with that estimator's window (its ``levels`` / ``entropy`` / ``histogram`` are the estimator's, whichever
        walker updates it), ``nwalkers`` defaults to ``windows.R``, and ``run_exchange`` samples with exchanges.
        ``synchronise=True`` (with ``windows``): the copies of a window go through the Wang-Landau stages together --
        the engine handle is created with check period 0 (the kernels' ``check_period`` keeps the value given), and
        ``run_exchange(..., sync_every=k)`` merges them between launches (``Engine.wl_synchronise``); on such a sampler
        nothing else checks flatness, so a run without ``sync_every`` keeps every factor where it is.

        ``observables``: an ``observables.Observables`` -- its kind counts and pair counts are evaluated on the device
        for every sample and traced as ``species_counts`` (K,) and ``pair_counts`` (n_shells, K, K), int32.

        ``minima``: a ``minima.Minima`` -- every recorded sample is offered to a minima record kept on the device
        (``Sampler.minima``); a record keyed by composition needs ``observables`` too.

        ``statistics``: a ``statistics.Statistics`` -- every recorded sample is offered to a statistics record kept on the
        device (``Sampler.statistics``): running moments, blocking sums and a histogram per walker or per state point,
        whether the trace is kept or not; count columns need ``observables`` too, intensity columns ``structure_factor``.
        A spec keyed by bins of a column (``Statistics.by_bin``, ``by_composition``, ``on_wl_levels``) keeps moments and a
        histogram per bin instead: microcanonical averages, averages per composition (``Sampler.wl_canonical``).

        ``structure_factor``: a ``structure.StructureFactor`` -- its amplitudes and intensities are evaluated on the device
        for every sample and traced as ``structure_amplitudes`` (Q, K, 2) int64 and ``structure_intensities`` (I,).

        ``connectivity``: a ``connectivity.Connectivity`` -- the components of its graphs are labelled on the device for every
        sample and their 24 numbers per graph traced as ``connectivity`` (G, 24) int64; connectivity columns of a
        statistics record need it.

        ``patterns``: a ``patterns.Patterns`` on the ``observables`` given here -- the species patterns on its site tuples
        are counted on the device for every sample, by the launch that counts the observables, and traced as
        ``pattern_counts`` (n_cells,) int32; pattern columns of a statistics record need it.

        ``environments``: an ``environments.Environments`` on the ``observables`` given here -- the coordination environments
        of its centres are counted on the device for every sample, by the same launch, and traced as ``environment_counts``
        (n_cells,) int32; environment columns of a statistics record need it.  With ``keep_occupancy=False`` the occupancies
        stay on the device.  A sampler sharded across ranks is out of scope: every rank traces its own walkers."""
        from . import parallel

        given = locals()  # (the family keywords as given: the table names them)
        traced = {fam: given[fam.keyword] for fam in FAMILIES if given[fam.keyword] is not None}
        if windows is not None and traced:
            raise ValueError(f"{next(iter(traced)).keyword}= with windows=: the samples of per-walker windows do not come from the "
                             "sample ring")
        for fam in traced:
            if fam.rests_on is not None and BY_NAME[fam.rests_on] not in traced:
                raise ValueError(f"{fam.keyword}= needs {BY_NAME[fam.rests_on].keyword}=: the class maps of {fam.a_spec} index the "
                                 f"kinds of the {fam.rests_on}")
        if synchronise and windows is None:
            raise ValueError("synchronise=True needs windows=: the copies of a window are what is merged "
                             "(parallel.WLWindows(n_windows=1, copies=nwalkers) for plain multi-walker Wang-Landau)")
        if windows is not None:
            sampler = cls._from_ensemble_windows(ensemble, windows, *args, step_type=step_type, kernel_type=kernel_type, seeds=seeds,
                                                 nwalkers=nwalkers, rank=rank, world_size=world_size, device=device, **kwargs)
            if synchronise and sampler._kernels[0]._mod_callable is not None:
                raise ValueError("synchronise=True with a callable mod_update: the merge divides the factor by a constant")
            sampler._wl_synchronise = bool(synchronise)
            if minima is not None:
                sampler._set_minima(minima)
            if statistics is not None:
                sampler._set_statistics(statistics)
            return sampler

        if step_type is None:
            step_type = "flip" if ensemble.chemical_potentials is not None else "swap"
        if kernel_type is None:
            kernel_type = "Metropolis"
        if seeds is not None and len(seeds) != nwalkers:
            raise ValueError("Number of seeds does not match number of kernels!")
        if rank is None or world_size is None:
            rank, world_size = parallel.rank_and_world()
        first, count = parallel.shard(nwalkers, rank, world_size)
        if count == 0:
            raise ValueError(f"rank {rank} of {world_size} would own no walker: nwalkers={nwalkers}")
        local_seeds = [None] * count if seeds is None else list(seeds[first:first + count])
        kernels = [mckernel_factory(kernel_type, ensemble, step_type, *args, seed=s, **kwargs)
                   for s in local_seeds]
        container = cls._container_for(ensemble, kernels[0], count)
        container.metadata["walker_range"] = (first, count, nwalkers)
        if device is None:
            device = parallel.local_device(rank)
        sampler = cls(kernels, container, walker_range=(first, count), device=device, world_size=world_size)
        if chemical_potentials is not None:
            sampler.set_chemical_potentials(chemical_potentials)
        for fam, spec in traced.items():  # (in the table's order: a family comes after the one it rests on)
            sampler._set_traced(fam, spec)
        if minima is not None:
            sampler._set_minima(minima)
        if statistics is not None:
            sampler._set_statistics(statistics)
        return sampler

    def _set_statistics(self, spec):
        for fam in FAMILIES:
            tag, noun, _ = fam.stat
            if spec.tagged_columns(tag) and fam.name not in self._traced:
                raise ValueError(f"a statistics record with {noun} columns needs a sampler built with {fam.keyword}=")
        self._statistics = spec
        if self._engine is not None:
            self._engine.set_statistics(spec)

    @property
    def statistics(self):
        """The statistics record of THIS rank's walkers (a ``statistics.StatisticsRecord``) as the handle holds it.  The
        ranks of a sharded sampler hold different walkers: their records stand side by side, they are not merged
        (``StatisticsRecord.combine`` merges records of the same keys)."""
        if self._statistics is None:
            raise ValueError("this sampler keeps no statistics record: build it with Sampler.from_ensemble(statistics=)")
        return self._get_engine().statistics()

    def reset_statistics(self):
        """Empty the record; ``clear_samples`` leaves it alone."""
        if self._statistics is None:
            raise ValueError("this sampler keeps no statistics record: build it with Sampler.from_ensemble(statistics=)")
        self._get_engine().reset_statistics()
        self._grid_record_base, self._grid_keys_mixed = None, False

    def _set_minima(self, spec):
        if spec.n_axes and "observables" not in self._traced:
            raise ValueError("a minima record keyed by composition needs a sampler built with observables=")
        self._minima, self._minima_offers = spec, 0
        if self._engine is not None:
            self._engine.set_minima(spec)

    @property
    def minima(self):
        """The minima record of this sampler's walkers (a ``minima.MinimaRecord``), merged over the ranks of a sharded
        sampler: lowest value, then rank order (a per-walker record: the walkers of all ranks)."""
        from . import parallel
        from .minima import MinimaRecord

        if self._minima is None:
            raise ValueError("this sampler keeps no minima record: build it with Sampler.from_ensemble(minima=)")
        rec = self._local_minima()
        if self._world > 1 and parallel.is_initialized():
            import torch.distributed as dist

            parts = [None] * self._world
            dist.all_gather_object(parts, rec)
            rec = MinimaRecord.merge(parts)
        return rec

    def _local_minima(self):
        """The record of this rank's walkers, as the handle holds it."""
        rec = self._get_engine().minima()
        rec.offers = self._minima_offers
        return rec

    def reset_minima(self):
        """Empty the record; ``clear_samples`` leaves it alone."""
        if self._minima is None:
            raise ValueError("this sampler keeps no minima record: build it with Sampler.from_ensemble(minima=)")
        self._get_engine().reset_minima()
        self._minima_offers = 0

    def _set_traced(self, fam, spec):
        """Trace ``spec`` of the family ``fam`` with every sample: the container's schema gains the family's traces, its
        metadata what the spec says of itself."""
        nw, N = self.samples.shape
        if spec.num_sites != N:
            raise ValueError(f"{fam.noun} {fam.verb} defined on {spec.num_sites} sites, the ensemble has {N}")
        if fam.name == "observables" and spec.site_ncodes is None:
            raise ValueError("observables for a sampler need site_ncodes (Observables.from_supercell gives them)")
        if fam.rests_on is not None:
            base = self._traced.get(fam.rests_on)
            if base is None or spec.n_kinds != base.n_kinds:
                raise ValueError(f"{fam.noun} must rest on the sampler's {fam.rests_on}: its class maps index their kinds")
        if self.samples.num_samples:
            raise ValueError(f"the container holds samples without {fam.traces_noun}: clear_samples() first")
        for name, dtype, dims in fam.traces:
            self.samples._schema[name] = (np.dtype(dtype), (nw,) + trace_shape(dims, spec))
        self.samples.metadata[fam.keyword] = getattr(spec, fam.describe)()
        self._traced[fam.name] = spec
        if self._engine is not None:
            getattr(self._engine, fam.set)(spec)

    @classmethod
    def _from_ensemble_windows(cls, ensemble, wx, *args, step_type=None, kernel_type=None, seeds=None, nwalkers=1, rank=None,
                               world_size=None, device=None, min_enthalpy=None, max_enthalpy=None, bin_size=None, **kwargs):
        from . import parallel

        if min_enthalpy is None and len(args) >= 3:  # (the reference's positional spelling)
            min_enthalpy, max_enthalpy, bin_size, args = args[0], args[1], args[2], args[3:]
        if min_enthalpy is None or max_enthalpy is None or bin_size is None:
            raise ValueError("windows= needs min_enthalpy, max_enthalpy and bin_size: the global range the windows cut up")
        if KERNELS.get(str(kernel_type).lower().replace("_", "")) is not WangLandau:
            raise ValueError("windows= needs kernel_type='Wang-Landau'")
        if (float(min_enthalpy), float(max_enthalpy), float(bin_size)) != (wx.min_enthalpy, wx.max_enthalpy, wx.bin_size):
            raise ValueError(f"min_enthalpy, max_enthalpy, bin_size = {(min_enthalpy, max_enthalpy, bin_size)} are not the "
                             f"global range of the windows, {(wx.min_enthalpy, wx.max_enthalpy, wx.bin_size)}")
        if nwalkers in (1, None):
            nwalkers = wx.R
        if nwalkers != wx.R:
            raise ValueError(f"the windows have {wx.R} estimators, the sampler {nwalkers} walkers")
        if rank is None or world_size is None:
            rank, world_size = parallel.rank_and_world()
        if world_size != 1:
            raise ValueError("replica-exchange Wang-Landau runs inside one engine handle: no sharding over ranks")
        if seeds is not None and len(seeds) != nwalkers:
            raise ValueError("Number of seeds does not match number of kernels!")
        if step_type is None:
            step_type = "flip" if ensemble.chemical_potentials is not None else "swap"
        kernels = []
        for e in range(wx.R):
            k = WangLandau(ensemble, step_type, float(wx.vmin[e]), float(wx.vmax[e]), wx.bin_size, *args,
                           seed=None if seeds is None else seeds[e], **kwargs)
            k._levels = wx.vmin[e] + np.arange(wx.Lw) * wx.bin_size  # (exactly Lw levels, as the engine counts them)
            k.spec.update(levels=k._levels.tolist(), window=int(wx.window_of[e]), copy=int(wx.copy_of[e]))
            kernels.append(k)
        container = cls._container_for(ensemble, kernels[0], wx.R)
        container._schema["wl_estimator"] = (np.dtype(np.int32), (wx.R, 1))
        container.metadata["walker_range"] = (0, wx.R, wx.R)
        container.metadata["wl_windows"] = dict(min_enthalpy=wx.min_enthalpy, max_enthalpy=wx.max_enthalpy, bin_size=wx.bin_size,
                                                n_windows=wx.n_windows, copies=wx.copies, window_bins=wx.Lw, stride_bins=wx.Ls)
        sampler = cls(kernels, container, walker_range=(0, wx.R), device=parallel.local_device(rank) if device is None else device,
                      world_size=1)
        sampler._wl_windows = wx
        return sampler

    @property
    def walker_chemical_potentials(self):
        """The chemical potentials of this rank's walkers (a list of dicts species -> value), None: the ensemble's."""
        return self._walker_mu

    def set_chemical_potentials(self, values):
        """Per-walker chemical potentials: a mu-T grid in one engine handle.  ``values``: a sequence of dicts
        species -> value or one dict species -> array, indexed by GLOBAL walker like seeds (or by this rank's
        walkers), so walker g runs the same chain at any world size; None: the ensemble's own again.  The ensemble
        must have chemical potentials (they are the table the handle is created with).  Between two ``run`` calls
        this is a mu sweep: the walkers continue from their last samples, re-priced at their new values."""
        ens = self._kernels[0].ensemble
        if values is None:
            self._walker_mu, self._walker_mu_dirty = None, self._walker_mu is not None
            self.samples.metadata.pop("walker_chemical_potentials", None)
            for k in self._kernels:
                k.chemical_potentials = ens.chemical_potentials
            return
        if ens.chemical_potentials is None:
            raise ValueError("per-walker chemical potentials need a semigrand ensemble: set ensemble.chemical_potentials first")
        if not isinstance(self._kernels[0], Metropolis) or isinstance(self._kernels[0], WangLandau):
            raise ValueError("per-walker chemical potentials run the Metropolis kernel only")
        dicts = ens.walker_chemical_potentials(values)
        first, count = self._walker_range
        nglobal = self.samples.metadata.get("walker_range", (0, count, count))[2]
        if len(dicts) == nglobal:
            dicts = dicts[first:first + count]
        elif len(dicts) != count:
            raise ValueError(f"expected chemical potentials for {nglobal} walkers (or this rank's {count}), got {len(dicts)}")
        self._walker_mu, self._walker_mu_dirty = dicts, True
        for k, d in zip(self._kernels, dicts):
            k.chemical_potentials = d
        self.samples.metadata["walker_chemical_potentials"] = dict(
            species=list(ens.species), values=[[d[sp] for sp in ens.species] for d in dicts])

    def _apply_walker_mu(self, eng):
        """The rows on the engine before its state is loaded or continued (a new handle starts without them)."""
        if self._walker_mu_dirty:
            ens = self._kernels[0].ensemble
            eng.set_walker_mu(None if self._walker_mu is None else ens.walker_mu_rows(self._walker_mu))
            self._walker_mu_dirty = False

    @staticmethod
    def _container_for(ensemble, k0, count):
        """Empty SampleContainer with the trace schema of kernel ``k0`` for ``count`` walkers."""
        F = len(ensemble.natural_parameters)
        # occupancies are STORED as the device ring's bytes (a quarter of the int32 the reference
        # keeps) and handed out as int32 by the container's getters
        per_walker = dict(occupancy=((ensemble.num_sites,), np.uint8), features=((F,), np.float64),
                          enthalpy=((1,), np.float64))
        if isinstance(k0, Metropolis):
            per_walker["temperature"] = ((1,), np.float64)
        per_walker["accepted"] = ((1,), bool)
        if k0.bias is not None:  # trace.bias (kernel/base.py:362-363)
            per_walker["bias"] = ((1,), np.float64)
        if isinstance(k0, WangLandau):  # wanglandau.py:268-288
            L = len(k0._levels)
            per_walker.update(histogram=((L,), np.int64), occurrences=((L,), np.int64),
                              entropy=((L,), np.float64), cumulative_mean_features=((L, F), np.float64),
                              mod_factor=((1,), np.float64))
        schema = Trace(**{k: np.empty((0, count) + shp, dtype=dt) for k, (shp, dt) in per_walker.items()})
        return SampleContainer(ensemble, schema, ensemble.thermo_boundaries)

    # -- accessors -----------------------------------------------------------------
    mckernels = property(lambda self: self._kernels)
    seeds = property(lambda self: [k.seed for k in self._kernels])
    samples = property(lambda self: self._container)
    walker_range = property(lambda self: self._walker_range)

    @property
    def engine(self):
        return self._get_engine()

    def efficiency(self, discard=0, flat=True):
        return self.samples.sampling_efficiency(discard=discard, flat=flat)

    def clear_samples(self):
        self.samples.clear()

    def global_statistics(self, discard=0):
        """Sums over ALL walkers of ALL ranks of the recorded samples: walkers, samples, mean
        enthalpy, enthalpy variance, acceptance.  One all-reduce of five float64 (identity
        without a process group)."""
        import torch

        from . import parallel

        H = self.samples.get_enthalpies(discard=discard, flat=False).astype(np.float64)
        acc = self.samples.get_trace_value("accepted", discard=discard, flat=False)
        local = torch.tensor([float(H.shape[1]), float(H.size), float(H.sum()), float((H * H).sum()),
                              float(acc.sum())], dtype=torch.float64)
        if parallel.collective_device() == "cuda":
            local = local.cuda(self._device)
        w, n, s1, s2, a = parallel.global_sums(local).cpu().numpy()
        mean = s1 / max(n, 1.0)
        return dict(walkers=int(w), samples=int(n), mean_enthalpy=mean,
                    enthalpy_variance=s2 / max(n, 1.0) - mean * mean, acceptance=a / max(n, 1.0))

    # -- engine plumbing -------------------------------------------------------------
    def _model_key(self):
        """Content key of everything baked into the engine handle: the chemical-potential table,
        the active sites of every sublattice and the bias table (an id()/count key would miss a
        different restriction of the same size or a recycled id)."""
        import hashlib

        k0 = self._kernels[0]
        ens = k0.ensemble
        h = hashlib.blake2b(digest_size=16)
        mu = ens._mu_table
        h.update(b"mu" if mu is None else np.ascontiguousarray(mu).tobytes())
        for sub in ens.sublattices:
            h.update(np.ascontiguousarray(sub.active_sites, dtype=np.int64).tobytes() + b"|")
            h.update(np.ascontiguousarray(sub.encoding, dtype=np.int64).tobytes() + b"/")
        h.update(repr(getattr(k0, "kB", None)).encode())  # (a distance handle's temperatures are in units of kB)
        if k0.bias is not None:
            h.update(np.ascontiguousarray(k0.bias._table).tobytes())
            h.update(repr((k0.bias.bias_type, k0.bias.penalty)).encode())
            icpt = getattr(k0.bias, "intercepts", None)
            if icpt is not None:
                h.update(b"icpt" + np.ascontiguousarray(icpt, dtype=np.float64).tobytes())
        for name in sorted(k0.usher_kwargs):  # flip table / weights / swap_weight are baked in too
            v = k0.usher_kwargs[name]
            h.update(name.encode() + (b"none" if v is None else np.ascontiguousarray(v, dtype=np.float64).tobytes()))
        return h.hexdigest(), self._device

    def _get_engine(self, device=None):
        if device is not None:
            self._device = int(device)
        k0 = self._kernels[0]
        ens = k0.ensemble
        key = self._model_key()
        if self._engine is None or self._engine_key != key:
            tables = ens.make_tables(**k0.usher_kwargs)
            dist = None
            if isinstance(ens.processor, DistanceProcessor):
                if not isinstance(k0, Metropolis):
                    raise ValueError("a distance ensemble runs the Metropolis kernel only")
                if k0.bias is not None:
                    raise ValueError("a distance ensemble takes no bias term")
                dist = ens.distance_spec(kB=k0.kB)
            if k0.bias is not None:
                tables.set_bias(k0.bias.bias_type, k0.bias._table, k0.bias.penalty,
                                intercepts=getattr(k0.bias, "intercepts", None))
            if isinstance(k0, WangLandau):
                # (a callable mod_update: flatness checks on the host, check period 0 switches the
                # device's own check off; synchronise=True likewise: the copies of a window are checked together,
                # between launches, by Engine.wl_synchronise)
                cfg = capi.make_config(
                    len(self._kernels), capi.KERNEL_WANGLANDAU, STEP_TYPES[k0.step_type], self._device,
                    min_enthalpy=k0._window[0], max_enthalpy=k0._window[1], bin_size=k0._window[2],
                    flatness=k0.flatness, mod_factor=k0._m0, mod_update=k0._mod_divisor,
                    check_period=0 if (k0._mod_callable is not None or self._wl_synchronise) else k0.check_period,
                    update_period=k0.update_period,
                )
            else:
                cfg = capi.make_config(len(self._kernels), capi.KERNEL_METROPOLIS,
                                       STEP_TYPES[k0.step_type], self._device)
            self._engine = Engine(tables, cfg, distance=dist)
            # the families in the table's order, a family behind the one it rests on; the two records behind all of them:
            # their keys and columns name the specs in force
            for fam in FAMILIES:
                if fam.name in self._traced:
                    getattr(self._engine, fam.set)(self._traced[fam.name])
            if self._minima is not None:  # (a new handle starts an empty record)
                self._engine.set_minima(self._minima)
                self._minima_offers = 0
            if self._statistics is not None:
                self._engine.set_statistics(self._statistics)
            if self._wl_windows is not None:  # (kernel e was built with estimator e's window: cfg holds window 0)
                self._engine.set_wl_windows(self._wl_windows.vmin, self._wl_windows.vmax)
            self._engine_key = key
            self._state_loaded = False
            self._walker_mu_dirty = self._walker_mu is not None
        return self._engine

    def _temperatures(self):
        """Temperature of every walker as the engine wants it (Wang-Landau: unused; UniformlyRandom:
        infinite, i.e. beta = 0)."""
        return np.array([getattr(k, "temperature", getattr(k, "engine_temperature", 0.0)) for k in self._kernels],
                        dtype=np.float64)

    def _local_occupancies(self, occupancies):
        """Accepts this rank's walkers (count, N), all walkers (nwalkers, N) -- the rank takes
        its block -- or a 1-D occupancy for a single walker (sampler.py:442-end)."""
        occ = np.asarray(occupancies)
        first, count = self._walker_range
        nglobal = self.samples.metadata.get("walker_range", (0, count, count))[2]
        N = self.samples.shape[1]
        if occ.shape == (count, N):
            pass
        elif occ.shape == (nglobal, N):
            occ = occ[first:first + count]
        elif occ.ndim == 1 and count == 1 and occ.shape[0] == N:
            occ = occ.reshape(1, N)
        else:
            raise AttributeError(
                "The given initial occupancies have incompompatible dimensions. Shape should be "
                f"{self.samples.shape}."
            )
        return occ.astype(np.int32, copy=False)  # (the engine copies it to the device)

    def _load_state(self, initial_occupancies):
        """Walker states on the device.  ``None`` = continue from the last recorded sample: that
        IS the device state when nothing else touched the engine or the container since the
        last run (the steps after the last sample of a run are never taken), so nothing is
        uploaded -- only the temperatures are refreshed (anneal changes them between runs)."""
        eng = self._get_engine()
        self._apply_walker_mu(eng)
        if initial_occupancies is None:
            if self._state_loaded and self._resume_at == (id(self.samples), self.samples.num_samples):
                eng.set_temperature(self._temperatures())
                return None
            initial_occupancies = self.samples.last_occupancy()
        occupancies = self._local_occupancies(initial_occupancies)
        seeds = np.array([k.seed64 for k in self._kernels], dtype=np.uint64)
        # a kernel's Generator, accept counters and WL aux arrays persist across run()
        # calls of one sampler (sampler.py:254-262): only the first call starts fresh
        eng.set_state(occupancies, seeds, self._temperatures(), reset_aux=not self._state_loaded)
        self._state_loaded = True
        return occupancies

    def setup_sample(self, initial_occupancies):
        """sampler.py:386-434: copy / reshape occupancies, set aux states, initial trace."""
        occupancies = self._load_state(initial_occupancies)
        return occupancies, self._current_trace(self._get_engine())

    def _current_trace(self, eng):
        st = eng.get_state()
        nw = len(self._kernels)
        tr = Trace(occupancy=st["occupancy"], features=st["features"],
                   enthalpy=st["enthalpy"].reshape(nw, 1))
        k0 = self._kernels[0]
        if isinstance(k0, Metropolis):
            tr.temperature = self._temperatures().reshape(nw, 1)
        tr.accepted = st["accepted"].reshape(nw, 1)
        if k0.bias is not None:
            tr.bias = eng.get_bias().reshape(nw, 1)
        if isinstance(k0, WangLandau):
            wl = eng.get_wl()
            tr.histogram, tr.occurrences, tr.entropy = wl["histogram"], wl["occurrences"], wl["entropy"]
            tr.cumulative_mean_features = wl["mean_features"]
            tr.mod_factor = wl["mod_factor"].reshape(nw, 1)
        for fam in FAMILIES:
            if fam.name in self._traced:
                values = getattr(eng, fam.eval)()
                for (name, _, _), v in zip(fam.traces, values if isinstance(values, tuple) else (values,)):
                    setattr(tr, name, v)
        return tr

    def _sample_blocks(self, nsteps, initial_occupancies, thin_by, max_block=0, state_loaded=False, keep_occupancy=True):
        """Generator over blocks of thinned samples, dict name -> (n, nwalkers, ...): the unit
        the device ring delivers (``smolmc_run_sampled``): the samples of a block are recorded on
        the device -- inside one launch for Metropolis kernels, as launch + snapshot pairs queued without
        a host round trip for biased and Wang-Landau kernels (trace.bias; the per-walker L and L x F
        arrays of the Wang-Landau trace) -- and the block's download overlaps the next block's kernel."""
        if nsteps % thin_by != 0:
            warnings.warn(
                f"The number of steps {nsteps} is not a multiple of thin_by  {thin_by}. The last "
                f"{nsteps % thin_by} will be ignored.",
                category=RuntimeWarning,
            )
        if not state_loaded:
            self._load_state(initial_occupancies)
        self._resume_at = None
        eng = self._get_engine()
        nsamples = nsteps // thin_by
        k0 = self._kernels[0]
        is_wl, has_bias = isinstance(k0, WangLandau), k0.bias is not None
        if is_wl and k0._mod_callable is not None:
            # a callable mod_update (wanglandau.py:100-105): the flatness checks run on the host between
            # launches, so these samples come back one launch at a time
            if self._wl_windows is not None:
                raise ValueError("a callable mod_update with per-walker windows: the host-side check is walker-indexed")
            for _ in range(nsamples):
                self._wl_run_with_host_checks(eng, thin_by)
                self._offer_current(eng)
                yield {k: v[None] for k, v in self._current_trace(eng).items()}
            return
        if is_wl and self._wl_windows is not None:
            # per-walker windows: the Wang-Landau arrays are estimator-indexed and the ring's snapshot rows
            # walker-indexed (smolmc_run_sampled refuses that column), so these samples too come back one launch at a
            # time; occupancy, features, enthalpy: by walker; the Wang-Landau arrays: by ESTIMATOR; wl_estimator: the
            # estimator every walker holds
            for _ in range(nsamples):
                eng.run(thin_by)
                self._offer_current(eng)
                tr = {k: v[None] for k, v in self._current_trace(eng).items()}
                tr["wl_estimator"] = eng.wl_windows()[2].reshape(1, -1, 1)
                yield tr
            return
        nw, N = len(self._kernels), k0.ensemble.num_sites
        # bytes of one sample of all walkers in the ring: occupancy bytes + features (+ the Wang-Landau trace:
        # entropy / histogram / occurrences [L] and the mean features [L x F] of every walker, wanglandau.py:247-251)
        F = len(k0.ensemble.natural_parameters)
        per_sample = nw * ((N if keep_occupancy else 0) + 8 * F + 17)
        for name, spec in self._traced.items():  # (the derived traces: their cells at their width)
            per_sample += nw * sum(np.dtype(dtype).itemsize * int(np.prod(trace_shape(dims, spec)))
                                   for _, dtype, dims in BY_NAME[name].traces)
        if is_wl:
            L = len(k0._levels)
            per_sample += nw * L * (24 + 8 * F)
        per_block = max(1, min(nsamples, (256 << 20) // max(1, per_sample)))  # <= ~256 MiB per ring slot
        # ... and several blocks per run, so that the download of one overlaps the kernel of the next (the ring
        # has two slots: block k + 1 is queued before block k is fetched)
        if nsamples * per_sample > (32 << 20):
            per_block = min(per_block, max(1, -(-nsamples // 8)))
        if max_block > 0:
            per_block = min(per_block, int(max_block))
        temps = self._temperatures().reshape(1, nw, 1)
        sizes = [min(per_block, nsamples - start) for start in range(0, nsamples, per_block)]

        asked = {BY_NAME[name].run_keyword: True for name in self._traced}

        def queue(n):
            eng.run_sampled_async(n, thin_by, occupancy=keep_occupancy, bias=has_bias, wl=is_wl,
                                  minima=self._minima is not None, statistics=self._statistics is not None, **asked)
            if self._minima is not None:
                self._minima_offers += n

        # Block i + 1 is queued before block i is handed out, so a consumer that stops early -- a `break` out of
        # Sampler.sample(), an exception in run() between two blocks -- leaves a block on the (cached) engine's ring.
        # The ring is emptied when this generator starts and when it ends, however it ends: the next run's first
        # fetch is its own first block.
        eng.discard_samples()
        try:
            yield from self._ring_blocks(eng, sizes, queue, temps, nw, k0, has_bias, is_wl)
        finally:
            eng.discard_samples()

    def _offer_current(self, eng):
        """The host-stepped paths offer the walkers' states themselves, so the record means the same on every path."""
        if self._minima is not None:
            eng.update_minima()
            self._minima_offers += 1
        if self._statistics is not None:
            eng.update_statistics()

    @staticmethod
    def _ring_blocks(eng, sizes, queue, temps, nw, k0, has_bias, is_wl):
        if sizes:
            queue(sizes[0])
        for i, n in enumerate(sizes):
            if i + 1 < len(sizes):
                queue(sizes[i + 1])
            ring = eng.fetch_samples(packed=True)
            occ = ring["occupancy"]  # (None: recorded without, see Sampler.run(keep_occupancy=False))
            block = dict(occupancy=np.empty((0, nw, eng.N), dtype=np.uint8) if occ is None else occ, features=ring["features"],
                         enthalpy=ring["enthalpy"][..., None], temperature=np.broadcast_to(temps, (n, nw, 1)),
                         accepted=ring["accepted"][..., None])
            if not isinstance(k0, Metropolis):  # (UniformlyRandom, Wang-Landau: no temperature in the trace)
                del block["temperature"]
            if has_bias:
                block["bias"] = ring["bias"][..., None]
            if is_wl:
                block.update(histogram=ring["histogram"], occurrences=ring["occurrences"], entropy=ring["entropy"],
                             cumulative_mean_features=ring["mean_features"], mod_factor=ring["mod_factor"][..., None])
            block.update({name: ring[name] for fam in FAMILIES for name, _, _ in fam.traces if name in ring})
            yield block

    def _wl_run_with_host_checks(self, eng, nsteps):
        """``nsteps`` Wang-Landau steps with the flatness check of wanglandau.py:253-264 done on the
        host, so that ``mod_update`` can be any callable (:100-105): the launches end where the step
        counter reaches a multiple of ``check_period``; there every walker whose histogram is flat
        (all visited bins above ``flatness`` times their mean, at least two visited) gets its
        histogram cleared and its modification factor mapped through the callable."""
        k0 = self._kernels[0]
        period = int(k0.check_period)
        done = int(eng.get_state(occupancy=False)["n_steps"][0])  # (all walkers of a sampler step together)
        left = int(nsteps)
        while left > 0:
            n = min(left, period - done % period)
            eng.run(n)
            done += n
            left -= n
            if done % period == 0:
                wl = eng.get_wl()
                S, hist, m = wl["entropy"], wl["histogram"], wl["mod_factor"]
                changed = False
                for r in range(len(m)):
                    seen = S[r] > 0
                    if seen.sum() >= 2 and (hist[r][seen] > k0.flatness * hist[r][seen].mean()).all():
                        hist[r] = 0
                        m[r] = self._kernels[r]._mod_callable(m[r])
                        changed = True
                if changed:
                    eng.set_wl(histogram=hist, mod_factor=m)

    def aux_checkpoint(self):
        """Everything beyond the occupancies that a run needs to continue bit-for-bit in another
        process -- the reference reserves ``aux_checkpoint`` for this and never fills it
        (sampler/container.py:89,539-541): step / accept counters (the walkers' positions in their
        random streams) and, for Wang-Landau, the entropy / histogram / occurrences / mean-feature
        arrays and the modification factors.  Restore with ``restore_aux`` after ``setup_sample`` (or
        a first ``run``) with the checkpoint's ``occupancy``."""
        eng = self._get_engine()
        st = eng.get_state()
        ck = dict(occupancy=st["occupancy"], n_steps=st["n_steps"], n_accepted=st["n_accepted"])
        if isinstance(self._kernels[0], WangLandau):
            ck.update({"wl_" + k: v for k, v in eng.get_wl().items()})
        return ck

    def restore_aux(self, checkpoint):
        """Put a checkpoint of ``aux_checkpoint`` back in a (possibly fresh) engine handle: occupancies
        and seeds with ``reset_aux=True`` -- the seeds only travel with a reset, smolmc.h -- then the
        checkpoint's counters and Wang-Landau arrays on top of the reset state."""
        eng = self._get_engine()
        seeds = np.array([k.seed64 for k in self._kernels], dtype=np.uint64)
        eng.set_state(self._local_occupancies(checkpoint["occupancy"]), seeds, self._temperatures(), reset_aux=True)
        eng.set_counters(checkpoint["n_steps"], checkpoint["n_accepted"])
        if isinstance(self._kernels[0], WangLandau):
            eng.set_wl(checkpoint["wl_entropy"], checkpoint["wl_histogram"], checkpoint["wl_occurrences"],
                       checkpoint["wl_mean_features"], checkpoint["wl_mod_factor"])
        self._state_loaded = True
        self._resume_at = (id(self.samples), self.samples.num_samples)

    def sample(self, nsteps, initial_occupancies, thin_by=1, progress=False):
        """Generator over thinned traces, one Trace per sample (sampler.py:164-210)."""
        for block in self._sample_blocks(nsteps, initial_occupancies, thin_by):
            for i in range(len(block["enthalpy"])):
                tr = Trace(**{k: np.asarray(v[i]) for k, v in block.items()})
                tr.occupancy = tr.occupancy.astype(np.int32)  # (trace.occupancy is int32 in the reference)
                yield tr

    def _need_start(self, initial_occupancies):
        """A run starts from ``initial_occupancies`` or from the last saved sample: refuse when there is neither."""
        if initial_occupancies is None and self.samples.num_samples == 0:
            raise RuntimeError("There are no saved samples to obtain the initial occupancies."
                               "These must be provided.")

    def run(self, nsteps, initial_occupancies=None, thin_by=1, progress=False, stream_chunk=0,
            stream_file=None, keep_last_chunk=False, swmr_mode=False, keep_occupancy=True):
        """sampler.py:212-301.  ``stream_chunk`` > 0 writes every chunk of samples to the streaming
        directory ``stream_file`` (see SampleContainer.get_backend) and keeps none in memory.

        ``keep_occupancy=False`` (a sampler built with ``observables=`` only): the occupancies of the samples never
        leave the device -- their species and pair counts do; the container stores the occupancy of the final
        sample of this call alone, so ``last_occupancy`` and a continuation work as before."""
        if not keep_occupancy:
            has_field = self._statistics is not None and self._statistics.site_codes > 0  # (the record's site field)
            if not self._traced and self._minima is None and not has_field:  # (a family that rests on the observables comes with them)
                raise ValueError("keep_occupancy=False needs a sampler built with observables=, minima=, structure_factor= or connectivity=: nothing else of the "
                                 "occupancies would be recorded")
            if stream_chunk > 0:
                raise ValueError("keep_occupancy=False with stream_chunk: every part of a stream holds its occupancies")
        self._need_start(initial_occupancies)
        if initial_occupancies is not None and self.samples.num_samples > 0:
            warnings.warn(
                "Initial occupancies where provided with a pre-existing set of samples.\n Make "
                "real sure that is what you want. If not, reset the samples in the sampler.",
                RuntimeWarning,
            )
        backend, last = None, None
        if stream_chunk > 0:  # sampler.py:264-301; the backend is a directory of .npz parts here
            if stream_file is None:
                stream_file = os.path.join(os.getcwd(), "moca-samples-" + datetime.now().strftime("%Y-%m-%d-%H%M%S%f"))
            backend = self.samples.get_backend(stream_file, nsteps // thin_by, swmr_mode=swmr_mode)
        self._load_state(initial_occupancies)
        if backend is not None and self._kept_last:
            self.samples.clear()  # the sample kept by the previous streamed run is already in its stream
        self._kept_last = False
        recorded = False
        without = {} if keep_occupancy else dict(keep_occupancy=False)
        for block in self._sample_blocks(nsteps, None, thin_by, max_block=stream_chunk, state_loaded=True, **without):
            self.samples.append_block(block, thinned_by=thin_by)
            recorded = True
            if backend is not None:
                # the most recent sample, whether or not this block fills a chunk: the tail flush
                # below must leave the FINAL recorded sample behind, not the end of the last full chunk
                last = {k: np.array(v[-1:]) for k, v in block.items()}
                if self.samples.num_samples >= stream_chunk:
                    self.samples.flush_to_backend(backend)
        if backend is not None:
            self.samples.flush_to_backend(backend)  # (the tail shorter than a chunk)
            backend.close()
            if keep_last_chunk and last is not None:  # the last sample stays in memory, e.g. to start the next run from it
                self.samples.append_block(last, thinned_by=0)
                self._kept_last = True
        if not keep_occupancy and recorded:  # (the walkers' current states ARE the final sample)
            self.samples.set_last_occupancy(self._get_engine().get_state()["occupancy"])
        if self._minima is not None:  # (this rank's walkers, like everything else in its container)
            self.samples.set_minima(self._local_minima())
        # the device now holds the last recorded sample (see _load_state)
        self._resume_at = (id(self.samples), self.samples.num_samples)

    def _run_exchange_wl(self, n_exchanges, steps_between, initial_occupancies, thin_by, wx, sync_every=None,
                         final_mod_factor=None):
        """run_exchange for replica-exchange Wang-Landau, see there."""
        if wx is not self._wl_windows:
            raise ValueError("run_exchange(windows=) takes the WLWindows this sampler was built with (Sampler.from_ensemble(windows=))")
        if sync_every is not None and not self._wl_synchronise:
            raise ValueError("sync_every= needs a sampler built with Sampler.from_ensemble(..., windows=, synchronise=True): "
                             "its handle has check period 0, so that no copy of a window leaves its stage alone")
        if sync_every is not None and int(sync_every) < 1:
            raise ValueError("sync_every must be at least 1")
        if final_mod_factor is not None and sync_every is None:
            raise ValueError("final_mod_factor= needs sync_every=: the windows' factors are those of the merge attempts")
        thin_by = int(steps_between if thin_by is None else thin_by)
        self._need_start(initial_occupancies)
        self._load_state(initial_occupancies)
        eng = self._get_engine()
        for i in range(int(n_exchanges)):
            for block in self._sample_blocks(steps_between, None, thin_by, state_loaded=True):
                self.samples.append_block(block, thinned_by=thin_by)
            wx.attempt(eng)
            if sync_every is not None and (i + 1) % int(sync_every) == 0:
                wx.sync_attempt(eng)
                if final_mod_factor is not None and wx.converged(final_mod_factor):
                    break
        if sync_every is not None:
            self.samples.metadata["wl_synchronise"] = dict(sync_every=int(sync_every), merges=wx.merges.tolist(),
                                                           mod_factor=wx.mod_factor.tolist())
        wx.estimator_of = eng.wl_windows()[2].astype(np.int64)
        self._resume_at = None  # (the last sample precedes the last exchange: a continuation reloads nothing it could trust)
        return wx

    def wl_joined_entropy(self):
        """(levels (L,), ln g (L,), visited (L,) bool) over the GLOBAL bin grid of a sampler built with ``windows=``:
        ``windows.join`` of the estimators' entropies as they are on the device now."""
        if self._wl_windows is None:
            raise ValueError("wl_joined_entropy needs a sampler built with Sampler.from_ensemble(..., windows=)")
        ln_g, _, visited = self._wl_windows.join(self._get_engine().get_wl()["entropy"])
        return self._wl_windows.levels(), ln_g, visited

    def wl_entropy_on_levels(self):
        """ln g (L,) on the bin grid of a Wang-Landau sampler's statistics record (``Statistics.on_wl_levels``), NaN on the
        levels nobody visited: ``wl_joined_entropy`` when windows are set, otherwise the mean over the kernels of their
        entropies on the levels each of them visited."""
        if not isinstance(self._kernels[0], WangLandau):
            raise ValueError("wl_entropy_on_levels needs a Wang-Landau sampler")
        if self._wl_windows is not None:
            _, ln_g, visited = self.wl_joined_entropy()
            return np.where(visited, ln_g, np.nan)
        S = self._get_engine().get_wl()["entropy"]  # (R, L)
        seen = S > 0
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(seen.any(axis=0), np.where(seen, S, 0.0).sum(axis=0) / seen.sum(axis=0), np.nan)

    def wl_canonical(self, temperatures):
        """(nT, C): the canonical averages of the record's columns at ``temperatures`` from ONE Wang-Landau run,
        ``record.canonical(wl_entropy_on_levels(), temperatures)``.  The sampler's record must be keyed by the enthalpy on
        the handle's own levels (``Statistics.on_wl_levels`` with the kernels' min_enthalpy and bin_size, or the windows'
        global grid)."""
        spec = self._statistics
        if spec is None or not spec.binned or spec.columns[spec.key_column] != ("enthalpy",):
            raise ValueError("wl_canonical needs a sampler built with statistics=Statistics.on_wl_levels(...)")
        ln_g = self.wl_entropy_on_levels()
        if len(ln_g) != spec.n_keys:
            raise ValueError(f"the record has {spec.n_keys} keys, the Wang-Landau handle {len(ln_g)} levels: build the record with "
                             "Statistics.on_wl_levels on the handle's own (min_enthalpy, bin_size, number of levels)")
        return self.statistics.canonical(ln_g, temperatures)

    def wl_canonical_sites(self, temperatures):
        """(nT, M, S): the site field at ``temperatures`` from ONE Wang-Landau run,
        ``record.canonical_sites(wl_entropy_on_levels(), temperatures)``: the mean structure of every level, weighted as
        ``wl_canonical`` weights the columns.  The sampler's record must be as for ``wl_canonical`` and carry a site field
        (``Statistics.on_wl_levels(..., sites=, site_codes=)``)."""
        spec = self._statistics
        if spec is None or not spec.binned or spec.columns[spec.key_column] != ("enthalpy",) or not spec.site_codes:
            raise ValueError("wl_canonical_sites needs a sampler built with statistics=Statistics.on_wl_levels(..., site_codes=)")
        ln_g = self.wl_entropy_on_levels()
        if len(ln_g) != spec.n_keys:
            raise ValueError(f"the record has {spec.n_keys} keys, the Wang-Landau handle {len(ln_g)} levels: build the record with "
                             "Statistics.on_wl_levels on the handle's own (min_enthalpy, bin_size, number of levels)")
        return self.statistics.canonical_sites(ln_g, temperatures)

    def _joint_kind(self):
        """(sublattice, species) that the b column of the record's joint field counts; a ValueError unless the sampler's
        record is keyed by state point and has a joint field whose a column is ``statistics.ENERGY`` and whose b column is
        a kind count."""
        from .statistics import BY_STATE_POINT

        spec = self._statistics
        obs = self._traced.get("observables")
        col = None if spec is None or not spec.has_joint else spec.columns[spec.joint_columns[1]]
        if spec is None or spec.binned or spec.key != BY_STATE_POINT or col is None or col[0] != "kind" or obs is None:
            raise ValueError("grid_ln_g needs a sampler built with statistics=Statistics.by_state_point(..., joint=(energy axis, "
                             "kind-count axis)) and observables=")
        if spec.columns[spec.joint_columns[0]] != ("energy",):
            raise ValueError("grid_ln_g needs statistics.ENERGY (the weighted sum of the features, weight 0 on the chemical work) on "
                             f"axis a of the joint field, not {spec.columns[spec.joint_columns[0]]}: the enthalpy contains -mu N already")
        base, ncodes = np.asarray(obs.kind_base), obs.site_ncodes
        if ncodes is None:
            raise ValueError("grid_ln_g needs observables with site_ncodes: which species a kind counts is not known")
        for sub in self._kernels[0].ensemble.active_sublattices:
            sites = np.asarray(sub.sites)
            hit = (base[sites] >= 0) & (base[sites] <= col[1]) & (col[1] < base[sites] + np.asarray(ncodes)[sites])
            if hit.any():
                if not hit.all() or len(set(base[sites].tolist())) != 1:
                    raise ValueError(f"grid_ln_g: kind {col[1]} is no species count of one whole sublattice")
                code = col[1] - int(base[sites[0]])
                enc = [int(c) for c in sub.encoding]
                if code not in enc:
                    raise ValueError(f"grid_ln_g: kind {col[1]} is code {code}, which its sublattice does not hold")
                return sub, sub.species[enc.index(code)]
        raise ValueError(f"grid_ln_g: kind {col[1]} counts no site of an active sublattice")

    def grid_state_points(self):
        """(betas (R,), fields (R,)) of the state points that the keys of the sampler's record hold, for the count on axis
        b of its joint field: beta = 1 / (kB T) and the field conjugate to that count, the chemical potential of its
        species less the value that the other species of its sublattice share -- the semigrand weight is
        exp(-beta (E - field N)) up to a constant exactly when they share one, and when the species of every other
        active sublattice share one among themselves; a ValueError otherwise.  State point p is walker p until
        ``run_exchange`` names a grid; then it is the grid point that walker p held when the last ``run_exchange`` began.
        The engine names its state points afresh there, so a record that goes on through a second ``run_exchange`` which
        begins from exchanged walkers mixes state points in its keys: that is refused here until ``reset_statistics``."""
        from .statistics import KB

        sub, species = self._joint_kind()
        ens = self._kernels[0].ensemble
        gx = self._grid
        nw = len(self._kernels)
        if self._grid_keys_mixed:
            raise ValueError("grid_ln_g: the record took rows of two run_exchange calls that numbered the state points "
                             "differently: reset_statistics() before the second call, then its keys hold one state point each")
        if gx is not None:  # (the engine's state point q is the grid's point base[q] since the last run_exchange began)
            base = self._grid_base
            mus = ens.walker_mu_dicts(gx.point_rows[base])
            temps = np.asarray(gx.point_temperatures[base], dtype=np.float64)
        else:
            mus = self._walker_mu if self._walker_mu is not None else [ens.chemical_potentials] * nw
            temps = np.asarray([k.temperature for k in self._kernels], dtype=np.float64)
        if mus[0] is None:
            raise ValueError("grid_ln_g needs a semigrand ensemble: set ensemble.chemical_potentials first")
        fields = np.zeros(nw)
        for p, mu in enumerate(mus):
            by_name = {str(k): float(v) for k, v in mu.items()}
            for s in ens.active_sublattices:
                others = {by_name[str(sp)] for sp in s.species if not (s is sub and str(sp) == str(species))}
                if len(others) > 1:
                    raise ValueError(f"grid_ln_g: at state point {p} the species beside {species} hold different chemical "
                                     f"potentials on one sublattice ({sorted(others)}): one count is not the conjugate of the field")
                if s is sub:
                    fields[p] = by_name[str(species)] - (others.pop() if others else 0.0)
        return 1.0 / (KB * temps), fields

    def grid_ln_g(self, tol=1e-12, max_iter=100000):
        """(ln g (n_a, n_b), f (R,)): the state points of the sampler's mu-T grid joined by the multiple-histogram method,
        ``record.wham_joint(betas, fields)`` with the sampler's own temperatures and chemical potentials per state point
        (``grid_state_points``).  The record must be keyed by state point and carry a joint field with the energy
        (``statistics.ENERGY``, not the enthalpy) on axis a and a kind count on axis b; a ValueError otherwise, also for
        another column on axis a."""
        betas, fields = self.grid_state_points()
        return self.statistics.wham_joint(betas, fields, tol=tol, max_iter=max_iter)

    def run_exchange(self, n_exchanges, steps_between, initial_occupancies=None, thin_by=None, grid=None, windows=None,
                     sync_every=None, final_mod_factor=None):
        """``windows`` (a ``parallel.WLWindows``, the one of ``Sampler.from_ensemble(windows=)``): replica-exchange
        Wang-Landau -- ``n_exchanges`` times ``steps_between`` steps on every walker, then one exchange attempt between
        neighbouring windows (``Engine.exchange_wl``), the even and the odd move taking turns.  Walkers swap ESTIMATORS,
        never occupancies: the int32 trace ``wl_estimator`` says which estimator each walker held at every sample, the
        Wang-Landau traces (entropy, histogram, ...) are in estimator order.  ``sync_every=k`` (a sampler built with
        ``synchronise=True``): after every k-th attempt the copies of every window are merged on the device when all of
        them are flat (``windows.sync_attempt``); ``samples.metadata["wl_synchronise"]`` records ``sync_every``, the
        ``merges`` per window and the windows' ``mod_factor``.  ``final_mod_factor``: the run ends at the merge attempt
        after which every window's factor is at or below it.  Returns ``windows``.  Otherwise:

        Sampling with replica exchange across a mu-T grid (hyper-parallel tempering): ``n_exchanges`` times
        ``steps_between`` steps on every walker, then one exchange attempt, decided and applied on the device
        (``Engine.exchange_grid``); the four moves of the grid take turns.  ``grid``: a ``parallel.GridExchange`` whose
        rows are ``ensemble.walker_mu_rows(...)`` of the chemical potentials along the mu axis, or a dict
        ``temperatures=, chemical_potentials= (a list of dicts), replicas=1, seed=0`` to build one; None: the grid of
        the last call.  Walker w starts at point ``grid.point_of[w]`` (a new grid: point w) and swaps points, never
        occupancies: each sample's ``temperature`` is the walker's temperature at that time, the int32 trace
        ``state_point`` says where it was (``samples.by_state_point`` regroups), ``samples.metadata["state_points"]``
        holds the grid, and afterwards the kernels' ``temperature`` / ``chemical_potentials`` and
        ``walker_chemical_potentials`` are the current assignment.  ``thin_by`` defaults to ``steps_between``."""
        from . import parallel

        if windows is not None or (grid is None and self._wl_windows is not None):
            return self._run_exchange_wl(n_exchanges, steps_between, initial_occupancies, thin_by,
                                         windows if windows is not None else self._wl_windows, sync_every, final_mod_factor)
        if sync_every is not None or final_mod_factor is not None:
            raise ValueError("sync_every= / final_mod_factor= belong to replica-exchange Wang-Landau (windows=)")
        return self._run_exchange_grid(n_exchanges, steps_between, initial_occupancies, thin_by, grid)

    def _run_exchange_grid(self, n_exchanges, steps_between, initial_occupancies, thin_by, grid):
        """run_exchange across a mu-T grid, see there."""
        from . import parallel

        if self._world > 1:
            raise ValueError("run_exchange on a sampler sharded over several ranks: the exchange across a mu-T grid runs "
                             "inside one engine handle (an exchange across ranks would gather counts as well as enthalpies)")
        ens = self._kernels[0].ensemble
        if not isinstance(self._kernels[0], Metropolis) or isinstance(self._kernels[0], WangLandau):
            raise ValueError("run_exchange runs the Metropolis kernel only")
        if ens.chemical_potentials is None:
            raise ValueError("run_exchange needs a semigrand ensemble: set ensemble.chemical_potentials first")
        if isinstance(grid, dict):
            spec = dict(grid)
            grid = parallel.GridExchange(spec.pop("temperatures"), ens.walker_mu_rows(spec.pop("chemical_potentials")), **spec)
        gx = grid if grid is not None else getattr(self, "_grid", None)
        if gx is None:
            raise ValueError("run_exchange needs a grid of state points")
        nw = len(self._kernels)
        if gx.npoints != nw:
            raise ValueError(f"the grid has {gx.npoints} state points, the sampler {nw} walkers")
        thin_by = int(steps_between if thin_by is None else thin_by)
        if "state_point" not in self.samples._schema:
            if self.samples.num_samples:
                raise ValueError("the container holds samples without a state_point trace: clear_samples() first")
            self.samples._schema["state_point"] = (np.dtype(np.int32), (nw, 1))
        base = np.asarray(gx.point_of, dtype=np.int64).copy()  # (what ``bind`` takes below: engine point q is grid point base[q])
        if self._statistics is not None:  # (until reset_statistics the record's keys hold rows under ONE numbering, or are mixed)
            if self._grid_record_base is not None and not np.array_equal(base, self._grid_record_base):
                self._grid_keys_mixed = True
            self._grid_record_base = base
        self._grid, self._grid_base = gx, base
        dicts = ens.walker_mu_dicts(gx.rows)
        self.samples.metadata["state_points"] = dict(
            species=list(ens.species), temperatures=[float(t) for t in gx.temperatures],
            chemical_potentials=[[d[sp] for sp in ens.species] for d in dicts], shape=[gx.replicas, gx.nT, gx.nMu])

        def assign(dirty):
            """the kernels and this sampler's per-walker values follow gx.point_of"""
            j = np.asarray(gx.point_of) % gx.nMu
            self.set_chemical_potentials([dicts[k] for k in j])
            self._walker_mu_dirty = dirty
            for k, T in zip(self._kernels, gx.point_temperatures[gx.point_of]):
                k.temperature = T
            self.samples._state_point_now = np.asarray(gx.point_of, dtype=np.int32).reshape(nw, 1)

        assign(True)
        self._need_start(initial_occupancies)
        self._load_state(initial_occupancies)
        eng = self._get_engine()
        engine_point, read_back = gx.bind()
        for _ in range(int(n_exchanges)):
            for block in self._sample_blocks(steps_between, None, thin_by, state_loaded=True):
                n = len(block["occupancy"])
                block["state_point"] = np.broadcast_to(np.asarray(gx.point_of, dtype=np.int32).reshape(1, nw, 1), (n, nw, 1))
                self.samples.append_block(block, thinned_by=thin_by)
            gx.attempt(eng, engine_point)
            read_back(eng)
            assign(False)  # (the engine holds them already)
        self._resume_at = (id(self.samples), self.samples.num_samples)
        return gx

    def anneal(self, temperatures, mcmc_steps, initial_occupancies=None, thin_by=1, progress=False,
               **kwargs):
        """Simulated annealing (sampler.py:303-384): one ``run`` per temperature, each continuing
        from the last sample of the previous one."""
        if not isinstance(self._kernels[0], Metropolis):
            raise AttributeError("anneal is only available for samplers with a thermal kernel")
        if temperatures[0] < temperatures[-1]:
            raise ValueError(
                "End temperature is greater than start temperature "
                f"{temperatures[-1]:.2f} > {temperatures[0]:.2f}."
            )
        start = initial_occupancies
        for temperature in temperatures:
            for kernel in self._kernels:
                kernel.temperature = temperature
            self.run(mcmc_steps, initial_occupancies=start, thin_by=thin_by, progress=progress)
            start = None

    def anneal_population(self, temperatures, mcmc_steps, initial_occupancies=None, populations=1, thin_by=1, seed=0,
                          overlap=None, n_iter=16, max_steps=1000):
        """Population annealing (Hukushima & Iba 2003; Machta, PRE 82, 026704), the counterpart of ``anneal``: the
        walkers are ``populations`` equal blocks that cool together.  ``mcmc_steps`` steps are sampled at
        ``temperatures[0]``; at every later temperature each population is reweighted by exp(-dbeta H), resampled to
        constant size and cloned on the device (``Engine.anneal_resample``), then sampled for ``mcmc_steps`` steps --
        the sample layout of ``anneal``.  Returns the ``parallel.PopulationAnnealing`` that holds the running
        ``log_q`` and the lineage; ``samples.metadata["population_annealing"]`` records, per temperature and
        population, ``log_partition_ratio`` (ln Z(T) - ln Z(temperatures[0]), 0 in the first row), ``n_families`` and
        ``rho_t``, and survives ``to_npz`` / ``from_npz``.

        With ``overlap`` in (0, 1) the schedule is adaptive: ``temperatures`` names the two ends (T0, T_end), and every
        step is the largest one at which the energy histograms of the two temperatures still overlap by ``overlap``,
        chosen on the device from the populations themselves (``Engine.anneal_adaptive``, at most ``n_iter`` bisections
        per step, at most ``max_steps`` steps).  The chosen ladder is the metadata's ``temperatures``, and ``overlap``
        holds one row [target, overlap of population 0, 1, ...] per step."""
        from . import parallel

        if not isinstance(self._kernels[0], Metropolis):
            raise AttributeError("anneal_population is only available for samplers with a thermal kernel")
        temperatures = [float(t) for t in temperatures]
        if len(temperatures) < 1:
            raise ValueError("anneal_population needs at least one temperature")
        if overlap is not None and len(temperatures) != 2:
            raise ValueError("anneal_population with a target overlap chooses its own schedule: temperatures names the "
                             f"two ends (T0, T_end), not {len(temperatures)} values")
        if temperatures[0] < temperatures[-1]:
            raise ValueError(
                "End temperature is greater than start temperature "
                f"{temperatures[-1]:.2f} > {temperatures[0]:.2f}."
            )
        nw, P = len(self._kernels), int(populations)
        if P < 1 or nw % P:
            raise ValueError(f"{P} populations do not divide the sampler's {nw} walkers into equal blocks")
        if self._world > 1:
            raise ValueError("anneal_population on a sampler sharded over several ranks: a population is resampled "
                             "inside one engine handle")
        if self._walker_mu is not None:
            raise ValueError("anneal_population with per-walker chemical potentials: walkers of different "
                             "Hamiltonians are no population")
        self._need_start(initial_occupancies)
        if overlap is None:
            pa = parallel.PopulationAnnealing(temperatures, populations=P, seed=seed)
        else:
            pa = parallel.PopulationAnnealing.adaptive(temperatures[0], temperatures[1], overlap, populations=P, seed=seed,
                                                       n_iter=n_iter, max_steps=max_steps)
        n = nw // P
        lpr, nfam, rho, ovl = [[0.0] * P], [[n] * P], [[1.0] * P], []
        k = 0
        while True:
            if k == 0:
                for kernel in self._kernels:
                    kernel.temperature = temperatures[0]
                self._load_state(initial_occupancies)
            else:
                if overlap is None:
                    temperature = temperatures[k]
                    for kernel in self._kernels:
                        kernel.temperature = temperature
                    res = self._get_engine().anneal_resample(np.full(P, temperature), pa.offset_words(k - 1), npop=P)
                else:
                    pa.check_room()
                    res = self._get_engine().anneal_adaptive(pa.t_end, pa.overlap_value, pa.offset_words(k - 1), npop=P,
                                                             n_iter=pa.n_iter)
                    temperature = res["temperature"]
                    pa.append(temperature, res["reached"], res["forced"],
                              [pa.overlap(res["q"][p * n:(p + 1) * n]) for p in range(P)])
                    ovl.append([pa.overlap_value] + pa.overlaps[-1].tolist())
                    for kernel in self._kernels:  # (the engine holds the temperature already)
                        kernel.temperature = temperature
                pa.record(res["parent"], res["qsum"], res["href"], k - 1)
                lpr.append(pa.log_partition_ratio().tolist())
                nfam.append(pa.n_families[-1].tolist())
                rho.append(pa.rho_t[-1].tolist())
            for block in self._sample_blocks(mcmc_steps, None, thin_by, state_loaded=True):
                self.samples.append_block(block, thinned_by=thin_by)
            k += 1
            if pa.done if overlap is not None else k >= len(temperatures):
                break
        meta = dict(temperatures=[float(t) for t in pa.temperatures], populations=P, seed=int(seed), log_partition_ratio=lpr,
                    n_families=nfam, rho_t=rho)
        if overlap is not None:
            meta["overlap"] = ovl
        self.samples.metadata["population_annealing"] = meta
        self._resume_at = (id(self.samples), self.samples.num_samples)
        return pa
