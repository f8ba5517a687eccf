#!/usr/bin/env python3
"""What the coordination environments of sampled states cost, counted on the device against counted on the host (DESIGN
4.23), one JSON line into profiles/environments_timing.jsonl:

  shape    config 2 (the headline: R = 4096 walkers of N = 4096 sites) with the nearest-neighbour shell: every site a
           centre with its 12 neighbours, centre and neighbour classes the two species (338 cells)
  blocks   --samples samples per block, one sample per sweep (thin_by = N steps per walker); --reps blocks per arm, the
           arms alternating; --warmup blocks of each first
  arm A    the path without environments: the ring with occupancy, the fetch (packed bytes), then the NumPy definition
           on the host (environments.Environments.evaluate) on the first --host-rows rows of the block, its time scaled to
           all rows (the work is one gather and one bincount per row); the line says so
  arm B    environments on the device, no occupancy column
  arm C    the same launch without the environment sets (the kind counts alone, no shells): what the phase adds

  wall time per sample of arms A and B (host clock from the queueing of the block to the arrays in hand, median and range
  over the blocks), the observables kernel's own time (HIP events around its one launch) with and without the sets, its
  share of the block's MC kernel time (the events of smolmc_last_kernel_ms), bytes downloaded per sample.

python tools/environments_timing.py [--samples 4] [--reps 5] [--out ...]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from smol_amd import workloads  # noqa: E402
from smol_amd.engine import Engine  # noqa: E402
from smol_amd.environments import Environments  # noqa: E402
from smol_amd.observables import Observables  # noqa: E402
from tools.observables_timing import block_bytes, stats_ms  # noqa: E402


def environments_of(wl):
    """(observables without shells, the environment spec): the shortest pair orbit of the workload's expansion, read in
    both directions."""
    kinds = Observables.from_supercell(wl.sc, tables=wl.tables)
    obs = Observables(kinds.kind_base, kinds.n_kinds, site_ncodes=kinds.site_ncodes)
    for orbit in kinds.shell_orbit_ids:
        spec = Environments.from_supercell(wl.sc, obs, orbits=[orbit])
        if spec.sets[0].width == 12:
            return obs, spec
    raise RuntimeError("the expansion has no pair orbit with 12 neighbours a site")


def measure(args):
    kw = dict(count=args.replicas) if args.replicas else {}
    if args.dim:
        kw["dim"] = args.dim
    wl = workloads.BUILDERS[2](**kw)
    eng = Engine(wl.tables, wl.make_config())
    eng.set_state(wl.occupancy, wl.seeds, wl.temperature)
    obs, spec = environments_of(wl)
    eng.set_observables(obs)
    eng.set_environments(spec)
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
        eng.run_sampled_async(ns, thin, occupancy=False, environments=True)
        nbytes = block_bytes(eng)
        eng.fetch_samples()
        t1 = time.perf_counter()
        return dict(wall=t1 - t0, mc_ms=eng.last_kernel_ms(), obs_ms=eng.observables_kernel_ms(), bytes=nbytes)

    def arm_c():
        eng.run_sampled_async(ns, thin, occupancy=False, observables=True)
        eng.fetch_samples()
        return dict(obs_ms=eng.observables_kernel_ms())

    A, B, Cc = [], [], []
    for i in range(args.warmup + args.reps):
        a, b, c = arm_a(), arm_b(), arm_c()
        if i >= args.warmup:
            A.append(a)
            B.append(b)
            Cc.append(c)
    # the two arms count the same thing: one more block, both ways, on the same rows
    eng.run_sampled_async(1, thin, occupancy=True, environments=True)
    smp = eng.fetch_samples(packed=True)
    same = bool(np.array_equal(smp["environment_counts"][0, :host_rows], spec.evaluate(smp["occupancy"][0, :host_rows])))
    obs_ms = np.array([x["obs_ms"] for x in B])
    mc_ms = np.array([x["mc_ms"] for x in B])
    st = spec.sets[0]
    out = dict(what="environments", config=2, name=wl.name, kernel=eng.kernel_info(), walkers=R, sites=N, n_kinds=obs.n_kinds,
               width=st.width, n_centres=st.n_centres, n_centre_classes=st.n_centre_classes, n_neigh_classes=st.n_neigh_classes,
               n_cells=spec.n_cells, samples_per_block=ns, thin_by=thin, reps=args.reps, device_equals_definition=same,
               arm_a=dict(ring_and_fetch_per_sample=stats_ms([x["ring"] / ns for x in A]),
                          with_host_environments_per_sample=stats_ms([(x["ring"] + x["host_scaled"]) / ns for x in A]),
                          host_environments_scaled_from_rows=host_rows, bytes_per_sample=A[0]["bytes"] // ns,
                          mc_kernel_ms_per_block=float(np.median([x["mc_ms"] for x in A]))),
               arm_b=dict(per_sample=stats_ms([x["wall"] / ns for x in B]), bytes_per_sample=B[0]["bytes"] // ns,
                          observables_kernel_ms_per_block=stats_ms(obs_ms / 1e3),
                          observables_kernel_ms_per_sample=float(np.median(obs_ms)) / ns,
                          mc_kernel_ms_per_block=float(np.median(mc_ms)), observables_share_of_mc_kernel=float(np.median(obs_ms / mc_ms))),
               arm_c=dict(observables_kernel_ms_per_block_kinds_only=stats_ms(np.array([x["obs_ms"] for x in Cc]) / 1e3)))
    out["a_over_b"] = out["arm_a"]["with_host_environments_per_sample"]["median_ms"] / out["arm_b"]["per_sample"]["median_ms"]
    out["b_faster_beyond_spread"] = bool(out["arm_b"]["per_sample"]["max_ms"] < out["arm_a"]["with_host_environments_per_sample"]["min_ms"])
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "environments_timing.jsonl"))
    args = ap.parse_args()
    line = json.dumps(measure(args))
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
