#!/usr/bin/env python3
"""Record how the REFERENCE's compiled ClusterSpaceEvaluator answers the one call the bridge makes on it.

Run where a checkout of the reference exists (needs Cython, gcc; same out-of-tree build as make_golden.py):

    python tests/golden/make_bridge_golden.py

smol_amd.bridge reads an evaluator's orbit tuples through ``__reduce__`` (evaluator.pyx:65-77): the tuples are a
private ``cdef tuple`` (container.pxd:22).  For every site of the model of tests/test_bridge_reference_core.py, in
both forms smol's processors construct (correlation: orbit tuples only; decomposition: + interaction tensors), this
script builds the reference's own evaluator and records its reply: the reply's class, whether its first argument is
the orbit tuple the evaluator was built from, the remaining arguments, and whether ``_orbit_data`` is visible.

Output: tests/golden/bridge_evaluator_reduce.npz (data only).
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))  # tests/
sys.path.insert(0, HERE)

import make_golden  # noqa: E402
from test_bridge_reference_core import smol_like_ensemble  # noqa: E402


def main():
    ev = make_golden.build_reference_core()[0]
    out = {}
    for d in (0, 1):
        replies = {}

        def make_evaluator(site, args):
            e = ev.ClusterSpaceEvaluator(*args)
            replies[site] = (args[0], e, e.__reduce__())
            return e

        smol_like_ensemble(make_evaluator, bool(d), False, False)
        sites = sorted(replies)
        first_e, first_reply = replies[sites[0]][1], replies[sites[0]][2]
        out["evaluator_type"] = np.array(f"{type(first_e).__module__}.{type(first_e).__qualname__}")
        out["reply_type"] = np.array(f"{first_reply[0].__module__}.{first_reply[0].__qualname__}")
        out["has_orbit_data"] = np.array(hasattr(first_e, "_orbit_data"))
        out[f"d{d}_sites"] = np.array(sites, dtype=np.int64)
        out[f"d{d}_reply_len"] = np.array([len(replies[s][2][1]) for s in sites], dtype=np.int64)
        out[f"d{d}_orbit_data_is_input"] = np.array([replies[s][2][1][0] is replies[s][0] for s in sites])
        out[f"d{d}_scalars"] = np.array([replies[s][2][1][1:5] for s in sites], dtype=np.float64)
        inter = [replies[s][2][1][5] for s in sites]
        out[f"d{d}_interaction_counts"] = np.array([len(t) for t in inter], dtype=np.int64)
        out[f"d{d}_interaction_sizes"] = np.array([a.size for t in inter for a in t], dtype=np.int64)
        out[f"d{d}_interactions"] = np.concatenate([np.ravel(a) for t in inter for a in t]).astype(np.float64)
    np.savez_compressed(os.path.join(HERE, "bridge_evaluator_reduce.npz"), **out)


if __name__ == "__main__":
    main()
