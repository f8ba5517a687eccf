"""The per-sample measurement families: what is derived from every sampled state on the device and travels with it.

``FAMILIES`` is the one ordered table ``engine.py``, ``moca.py`` and ``statistics.py`` read: which derived traces exist,
what they are called, how big they are and what rests on what.  Its order is the order of the traces in a block of the
sample ring and in ``SampleContainer.traced_values``, and the order of the families' segments among the column sources of
a statistics record (``statistics.segments``).  Minima and statistics are records that READ these families; they are not
in the table.

A trace's per-walker shape is a tuple of numbers and of size names.  A name is an attribute of the family's spec object
(a sampler builds its schema before an engine exists) and, on a handle, one of the numbers its ``*_shape`` reader returns
(``Family.sizes``, in the reader's order).
"""

from __future__ import annotations

from collections import namedtuple

import numpy as np

from . import capi
from .connectivity import Connectivity
from .environments import Environments
from .observables import Observables
from .patterns import Patterns
from .structure import StructureFactor

Family = namedtuple("Family", [
    "name",          # the key of the family: in BY_NAME, in ``Sampler._traced``
    "keyword",       # the keyword of ``Sampler.from_ensemble`` = the key of the container's metadata
    "run_keyword",   # the keyword of ``Engine.run_sampled`` / ``run_sampled_async`` ...
    "flag",          # ... and the SMOLMC_SAMPLE_* flag it sets
    "stem",          # smolmc_set_<stem>, smolmc_<stem>_shape, smolmc_eval_<stem>, smolmc_get_sample_<stem>;
                     # Engine.<stem>_shape, Engine.sample_<stem>
    "set",           # the Engine method that takes the spec ...
    "eval",          # ... and the one that evaluates occupancies: one array per trace, in order
    "sizes",         # the names of what <stem>_shape returns
    "traces",        # ((trace name, dtype, per-walker shape), ...)
    "rests_on",      # the family whose kinds the spec's class maps index, or None
    "stat",          # (the tag of the family's columns in a statistics record, what a message calls such a column,
                     # the size its segment of the column sources is counted in)
    "noun", "verb",  # "the pattern spec" "is": the words of the messages ...
    "a_spec",        # ... "a pattern spec" (where the family rests on another) ...
    "traces_noun",   # ... "the pattern_counts trace"
    "spec",          # the spec class
    "describe",      # its method that says what a container's metadata keeps
    "saved",         # the class packs that metadata into the meta/* arrays of an .npz (metadata_to_npz, metadata_from_npz)
])

FAMILIES = (
    Family(name="observables", keyword="observables", run_keyword="observables", flag=capi.SAMPLE_OBSERVABLES,
           stem="observables", set="set_observables", eval="observables", sizes=("n_kinds", "n_shells"),
           traces=(("species_counts", np.int32, ("n_kinds",)), ("pair_counts", np.int32, ("n_shells", "n_kinds", "n_kinds"))),
           rests_on=None, stat=("kind", "count", "n_kinds"), noun="the observables", verb="are", a_spec=None,
           traces_noun="the observables' traces", spec=Observables, describe="describe", saved=True),
    # (the structure-factor metadata is not written to an .npz: the two traces are, the points and scales are not)
    Family(name="structure", keyword="structure_factor", run_keyword="structure", flag=capi.SAMPLE_STRUCTURE,
           stem="structure", set="set_structure_factor", eval="structure_factor", sizes=("n_points", "n_kinds", "n_intensities"),
           traces=(("structure_amplitudes", np.int64, ("n_points", "n_kinds", 2)),
                   ("structure_intensities", np.float64, ("n_intensities",))),
           rests_on=None, stat=("intensity", "intensity", "n_intensities"), noun="the structure factors", verb="are", a_spec=None,
           traces_noun="the structure factors' traces", spec=StructureFactor, describe="describe", saved=False),
    Family(name="connectivity", keyword="connectivity", run_keyword="connectivity", flag=capi.SAMPLE_CONNECTIVITY,
           stem="connectivity", set="set_connectivity", eval="connectivity", sizes=("n_graphs", "n_kinds"),
           traces=(("connectivity", np.int64, ("n_graphs", capi.CONN_STATS)),),
           rests_on=None, stat=("connectivity", "connectivity", "n_graphs"), noun="the connectivity spec", verb="is", a_spec=None,
           traces_noun="the connectivity trace", spec=Connectivity, describe="to_metadata", saved=True),
    Family(name="patterns", keyword="patterns", run_keyword="patterns", flag=capi.SAMPLE_PATTERNS,
           stem="patterns", set="set_patterns", eval="patterns", sizes=("n_sets", "n_cells"),
           traces=(("pattern_counts", np.int32, ("n_cells",)),),
           rests_on="observables", stat=("pattern", "pattern", "n_cells"), noun="the pattern spec", verb="is",
           a_spec="a pattern spec", traces_noun="the pattern_counts trace", spec=Patterns, describe="describe", saved=True),
    Family(name="environments", keyword="environments", run_keyword="environments", flag=capi.SAMPLE_ENVIRONMENTS,
           stem="environments", set="set_environments", eval="environments", sizes=("n_sets", "n_cells", "n_centres"),
           traces=(("environment_counts", np.int32, ("n_cells",)),),
           rests_on="observables", stat=("environment", "environment", "n_cells"), noun="the environment spec", verb="is",
           a_spec="an environment spec", traces_noun="the environment_counts trace", spec=Environments, describe="describe",
           saved=True),
)
BY_NAME = {fam.name: fam for fam in FAMILIES}


def trace_shape(dims, sizes):
    """The per-walker shape ``dims`` of a trace: its names looked up in ``sizes``, a spec object or the dict a handle's
    ``*_shape`` reader gave."""
    get = sizes.__getitem__ if isinstance(sizes, dict) else lambda name: getattr(sizes, name)
    return tuple(d if isinstance(d, int) else int(get(d)) for d in dims)
