#!/usr/bin/env python3
"""What the species patterns of sampled states cost, counted on the device against counted on the host, one
JSON line into profiles/patterns_timing.jsonl:

  shape    config 2 (the headline: R = 4096 walkers of N = 4096 sites): one set per triplet orbit of the expansion and the
           nearest-neighbour tetrahedra, which come from a second cluster model with a quadruplet cutoff; classes are the
           species codes
  blocks   --samples samples per block, one sample per sweep (thin_by = N steps per walker); --reps blocks per arm, the
           arms alternating; --warmup blocks of each first
  arm A    the path without patterns: the ring with occupancy, the fetch (packed bytes), then the NumPy definition on the
           host (patterns.Patterns.evaluate) on the first --host-rows rows of the block, its time scaled to all rows (the
           work is one gather and one bincount per row and set); the line says so
  arm B    patterns on the device, no occupancy column

  wall time per sample of both arms (host clock from the queueing of the block to the arrays in hand, median and range
  over the blocks), the observables kernel's own time (HIP events around its one launch), its share of the block's MC kernel
  time (the events of smolmc_last_kernel_ms), bytes downloaded per sample.

python tools/patterns_timing.py [--samples 4] [--reps 5] [--out ...]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from smol_amd import synth, workloads  # noqa: E402
from smol_amd.engine import Engine  # noqa: E402
from smol_amd.observables import Observables  # noqa: E402
from smol_amd.patterns import Patterns  # noqa: E402
from tools.observables_timing import block_bytes, stats_ms  # noqa: E402


def patterns_of(wl, dim, quad_cutoff):
    """(observables without shells, the pattern spec): the triplet orbits of the workload's expansion and the
    nearest-neighbour tetrahedra of a second model on the same prim."""
    kinds = Observables.from_supercell(wl.sc, tables=wl.tables)
    obs = Observables(kinds.kind_base, kinds.n_kinds, site_ncodes=kinds.site_ncodes)
    triplets = Patterns.from_supercell(wl.sc, obs)
    wide = synth.build_supercell(synth.build_cluster_model(wl.sc.model.prim, {2: quad_cutoff, 3: quad_cutoff, 4: quad_cutoff}),
                                 [dim, dim, dim])
    quads = [o.id for o in wide.model.orbits if o.size == 4]
    tetra = Patterns.from_supercell(wide, obs, orbits=quads[:1])
    return obs, Patterns(obs, triplets.sets + tetra.sets)


def measure(args):
    kw = dict(count=args.replicas) if args.replicas else {}
    if args.dim:
        kw["dim"] = args.dim
    wl = workloads.BUILDERS[2](**kw)
    dim = round(wl.sc.num_sites ** (1.0 / 3.0))
    eng = Engine(wl.tables, wl.make_config())
    eng.set_state(wl.occupancy, wl.seeds, wl.temperature)
    obs, spec = patterns_of(wl, dim, args.quad_cutoff)
    eng.set_observables(obs)
    eng.set_patterns(spec)
    R, N, ns = eng.R, eng.N, args.samples
    thin = N  # one sweep
    eng.run(20 * N, sync=True)
    host_rows = min(args.host_rows, ns * R)

    def arm_a():
        t0 = time.perf_counter()
        eng.run_sampled_async(ns, thin, occupancy=True)
        nbytes = block_bytes(eng)
        smp = eng.fetch_samples(packed=True)
        t1 = time.perf_counter()
        spec.evaluate(smp["occupancy"].reshape(ns * R, N)[:host_rows])
        t2 = time.perf_counter()
        return dict(ring=t1 - t0, host_scaled=(t2 - t1) * (ns * R / host_rows), mc_ms=eng.last_kernel_ms(), bytes=nbytes)

    def arm_b():
        t0 = time.perf_counter()
        eng.run_sampled_async(ns, thin, occupancy=False, patterns=True)
        nbytes = block_bytes(eng)
        eng.fetch_samples()
        t1 = time.perf_counter()
        return dict(wall=t1 - t0, mc_ms=eng.last_kernel_ms(), obs_ms=eng.observables_kernel_ms(), bytes=nbytes)

    A, B = [], []
    for i in range(args.warmup + args.reps):
        a, b = arm_a(), arm_b()
        if i >= args.warmup:
            A.append(a)
            B.append(b)
    # the two arms count the same thing: one more block, both ways, on the same rows
    eng.run_sampled_async(1, thin, occupancy=True, patterns=True)
    smp = eng.fetch_samples(packed=True)
    same = bool(np.array_equal(smp["pattern_counts"][0, :host_rows], spec.evaluate(smp["occupancy"][0, :host_rows])))
    obs_ms = np.array([x["obs_ms"] for x in B])
    mc_ms = np.array([x["mc_ms"] for x in B])
    out = dict(what="patterns", config=2, name=wl.name, kernel=eng.kernel_info(), walkers=R, sites=N, n_kinds=obs.n_kinds,
               arity=[s.arity for s in spec.sets], n_classes=[s.n_classes for s in spec.sets],
               tuples=[s.n_tuples for s in spec.sets], n_cells=spec.n_cells, samples_per_block=ns, thin_by=thin, reps=args.reps,
               device_equals_definition=same,
               arm_a=dict(ring_and_fetch_per_sample=stats_ms([x["ring"] / ns for x in A]),
                          with_host_patterns_per_sample=stats_ms([(x["ring"] + x["host_scaled"]) / ns for x in A]),
                          host_patterns_scaled_from_rows=host_rows, bytes_per_sample=A[0]["bytes"] // ns,
                          mc_kernel_ms_per_block=float(np.median([x["mc_ms"] for x in A]))),
               arm_b=dict(per_sample=stats_ms([x["wall"] / ns for x in B]), bytes_per_sample=B[0]["bytes"] // ns,
                          observables_kernel_ms_per_block=stats_ms(obs_ms / 1e3),
                          observables_kernel_ms_per_sample=float(np.median(obs_ms)) / ns,
                          mc_kernel_ms_per_block=float(np.median(mc_ms)), observables_share_of_mc_kernel=float(np.median(obs_ms / mc_ms))))
    out["a_over_b"] = out["arm_a"]["with_host_patterns_per_sample"]["median_ms"] / out["arm_b"]["per_sample"]["median_ms"]
    out["b_faster_beyond_spread"] = bool(out["arm_b"]["per_sample"]["max_ms"] < out["arm_a"]["with_host_patterns_per_sample"]["min_ms"])
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--replicas", type=int, default=0, help="walkers (default: the configuration's)")
    ap.add_argument("--dim", type=int, default=0, help="supercell size (default: the configuration's)")
    ap.add_argument("--samples", type=int, default=4, help="samples per block")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-rows", type=int, default=64, help="rows on which arm A evaluates the definition")
    ap.add_argument("--quad-cutoff", type=float, default=3.0, help="cutoff of the second model: nearest-neighbour tetrahedra")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "patterns_timing.jsonl"))
    args = ap.parse_args()
    line = json.dumps(measure(args))
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
