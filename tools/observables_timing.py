#!/usr/bin/env python3
"""What the observables of sampled states cost, counted on the device against counted on the host, one JSON
line per shape into profiles/observables_timing.jsonl:

  shapes   config 2 (the headline: R = 4096 walkers of N = 4096 sites, its four pair shells) and config 14 (the mu-T grid of
           config 3 in one handle: the kind counts and one pair shell)
  blocks   --samples samples per block, one sample per sweep (thin_by = N steps per walker); --reps blocks per arm, the
           arms alternating; --warmup blocks of each first
  arm A    the path without observables: the ring with occupancy, the fetch (packed bytes), then the NumPy definition on
           the host (observables.Observables.evaluate).  The kind counts are evaluated for every row.  The pair counts of
           the definition take minutes per block at these shapes: they are evaluated on the first --host-rows rows of the
           block and the time is scaled to all rows (the work is one gather and one bincount per row); the line says so.
  arm B    observables on the device, no occupancy column

  wall time per sample of both arms (host clock from the queueing of the block to the arrays in hand, median and range
  over the blocks), the observables kernel's own time (HIP events around its launch), its share of the block's MC kernel
  time (the events of smolmc_last_kernel_ms), bytes downloaded per sample.

python tools/observables_timing.py [--configs 2,14] [--samples 4] [--reps 5] [--out ...]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from smol_amd import capi, workloads  # noqa: E402
from smol_amd.engine import Engine  # noqa: E402
from smol_amd.observables import Observables  # noqa: E402


def stats_ms(samples):
    a = np.asarray(samples) * 1e3
    return dict(median_ms=float(np.median(a)), min_ms=float(a.min()), max_ms=float(a.max()), n=len(a))


def observables_of(config, wl):
    """config 2: default kinds and every pair shell of the expansion; config 14: the kind counts and the first shell."""
    full = Observables.from_supercell(wl.sc, tables=wl.tables)
    if config == 14:
        return Observables.from_supercell(wl.sc, tables=wl.tables, orbits=full.shell_orbit_ids[:1])
    return full


def block_bytes(eng):
    fn = eng._lib.smolmc_debug_block_bytes
    import ctypes as C

    fn.restype, fn.argtypes = C.c_longlong, [C.c_void_p]
    return int(fn(eng._h))


def measure(config, args):
    kw = dict(count=args.replicas) if args.replicas else {}
    if args.dim:
        kw["dim"] = args.dim
    wl = workloads.BUILDERS[config](**kw)
    eng = Engine(wl.tables, wl.make_config())
    if "walker_mu" in wl.extras:
        eng.set_walker_mu(wl.extras["walker_mu"])
    eng.set_state(wl.occupancy, wl.seeds, wl.temperature)
    obs = observables_of(config, wl)
    eng.set_observables(obs)
    counts_only = Observables(obs.kind_base, obs.n_kinds, site_ncodes=obs.site_ncodes)
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
        occ = smp["occupancy"].reshape(ns * R, N)
        counts, _ = counts_only.evaluate(occ)
        t2 = time.perf_counter()
        _, pairs = obs.evaluate(occ[:host_rows])
        t3 = time.perf_counter()
        return dict(ring=t1 - t0, counts=t2 - t1, pairs_scaled=(t3 - t2) * (ns * R / host_rows), mc_ms=eng.last_kernel_ms(),
                    bytes=nbytes, check=(counts, pairs))

    def arm_b():
        t0 = time.perf_counter()
        eng.run_sampled_async(ns, thin, occupancy=False, observables=True)
        nbytes = block_bytes(eng)
        smp = eng.fetch_samples()
        t1 = time.perf_counter()
        return dict(wall=t1 - t0, mc_ms=eng.last_kernel_ms(), obs_ms=eng.observables_kernel_ms(), bytes=nbytes,
                    check=(smp["species_counts"], smp["pair_counts"]))

    A, B = [], []
    for i in range(args.warmup + args.reps):
        a, b = arm_a(), arm_b()
        if i >= args.warmup:
            A.append(a)
            B.append(b)
    # the two arms count the same thing: one more block, both ways, on the same rows
    eng.run_sampled_async(1, thin, occupancy=True, observables=True)
    smp = eng.fetch_samples(packed=True)
    want = obs.evaluate(smp["occupancy"][0, :host_rows])
    same = bool(np.array_equal(smp["species_counts"][0, :host_rows], want[0]) and np.array_equal(smp["pair_counts"][0, :host_rows], want[1]))
    a_counts = [(x["ring"] + x["counts"]) / ns for x in A]
    a_pairs = [(x["ring"] + x["counts"] + x["pairs_scaled"]) / ns for x in A]
    b_wall = [x["wall"] / ns for x in B]
    obs_ms = np.array([x["obs_ms"] for x in B])
    mc_ms = np.array([x["mc_ms"] for x in B])
    out = dict(what="observables", config=config, name=wl.name, kernel=eng.kernel_info(), walkers=R, sites=N, n_kinds=obs.n_kinds,
               n_shells=obs.n_shells, bonds=[int(len(b)) for b in obs.shells], samples_per_block=ns, thin_by=thin, reps=args.reps,
               device_equals_definition=same,
               arm_a=dict(ring_and_fetch_per_sample=stats_ms([x["ring"] / ns for x in A]),
                          with_host_kind_counts_per_sample=stats_ms(a_counts),
                          with_host_pair_counts_per_sample=stats_ms(a_pairs),
                          host_pair_counts_scaled_from_rows=host_rows, bytes_per_sample=A[0]["bytes"] // ns,
                          mc_kernel_ms_per_block=float(np.median([x["mc_ms"] for x in A]))),
               arm_b=dict(per_sample=stats_ms(b_wall), bytes_per_sample=B[0]["bytes"] // ns,
                          observables_kernel_ms_per_block=float(np.median(obs_ms)), observables_kernel_ms_per_sample=float(np.median(obs_ms)) / ns,
                          mc_kernel_ms_per_block=float(np.median(mc_ms)), observables_share_of_mc_kernel=float(np.median(obs_ms / mc_ms))))
    out["a_counts_over_b"] = out["arm_a"]["with_host_kind_counts_per_sample"]["median_ms"] / out["arm_b"]["per_sample"]["median_ms"]
    out["b_faster_beyond_spread"] = bool(out["arm_b"]["per_sample"]["max_ms"] < out["arm_a"]["with_host_kind_counts_per_sample"]["min_ms"])
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", default="2,14")
    ap.add_argument("--replicas", type=int, default=0, help="walkers (default: the configuration's)")
    ap.add_argument("--dim", type=int, default=0, help="supercell size (default: the configuration's)")
    ap.add_argument("--samples", type=int, default=4, help="samples per block")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-rows", type=int, default=64, help="rows on which arm A evaluates the pair counts of the definition")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "observables_timing.jsonl"))
    args = ap.parse_args()
    for config in (int(c) for c in args.configs.split(",")):
        line = json.dumps(measure(config, args))
        print(line, flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
