#!/usr/bin/env python3
"""What keeping the lowest sampled states costs, on the device against on the host, one JSON line per shape
into profiles/minima_timing.jsonl:

  shapes   config 2 (the headline: R = 4096 walkers of N = 4096 sites, canonical: every row of a block has one
           composition, every wave of pass 1 is slot-uniform when keyed by composition) and config 14 (the mu-T grid in
           one handle: the compositions differ from row to row)
  blocks   --samples samples per block, one sample per sweep (thin_by = N steps per walker); --reps blocks per arm, the
           arms alternating; --warmup blocks of each first
  arm A    the path without a record: the ring with occupancy, the fetch (packed bytes), then the per-walker argmin over
           the block on the host and the pick of its occupancy row
  arm B    the record on the device, no occupancy column: once per walker, once keyed by composition (the kind counts are
           then counted on the device for every row, behind the downloaded part)

  wall time per sample of the arms (host clock from the queueing of the block to the arrays in hand, median and range
  over the blocks), the three kernels' own times (HIP events around their launches), their share of the block's MC kernel
  time (the events of smolmc_last_kernel_ms), bytes downloaded per sample.

python tools/minima_timing.py [--configs 2,14] [--samples 4] [--reps 5] [--out ...]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from smol_amd import capi, workloads  # noqa: E402,F401
from smol_amd.engine import Engine  # noqa: E402
from smol_amd.minima import Minima, MinimaRecord  # noqa: E402
from smol_amd.observables import Observables  # noqa: E402


def stats_ms(samples):
    a = np.asarray(samples) * 1e3
    return dict(median_ms=float(np.median(a)), min_ms=float(a.min()), max_ms=float(a.max()), n=len(a))


def block_bytes(eng):
    fn = eng._lib.smolmc_debug_block_bytes
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
    full = Observables.from_supercell(wl.sc, tables=wl.tables)
    obs = Observables(full.kind_base, full.n_kinds, site_ncodes=full.site_ncodes)  # (the kind counts, no shells)
    R, N, ns = eng.R, eng.N, args.samples
    thin = N  # one sweep
    eng.run(20 * N, sync=True)
    specs = dict(per_walker=Minima.per_walker(), by_composition=Minima.by_composition(obs, [1], extents=[N + 1]))
    host_best = dict(value=np.full(R, np.inf), occupancy=np.zeros((R, N), dtype=np.uint8))

    def arm_a():
        t0 = time.perf_counter()
        eng.run_sampled_async(ns, thin, occupancy=True)
        nbytes = block_bytes(eng)
        smp = eng.fetch_samples(packed=True)
        t1 = time.perf_counter()
        H = smp["enthalpy"]
        where = H.argmin(axis=0)
        low = H[where, np.arange(R)]
        better = low < host_best["value"]
        host_best["value"][better] = low[better]
        host_best["occupancy"][better] = smp["occupancy"][where[better], np.flatnonzero(better)]
        t2 = time.perf_counter()
        return dict(ring=t1 - t0, wall=t2 - t0, mc_ms=eng.last_kernel_ms(), bytes=nbytes)

    def arm_b():
        t0 = time.perf_counter()
        eng.run_sampled_async(ns, thin, occupancy=False, minima=True)
        nbytes = block_bytes(eng)
        eng.fetch_samples()
        t1 = time.perf_counter()
        return dict(wall=t1 - t0, mc_ms=eng.last_kernel_ms(), min_ms=eng.minima_kernel_ms(), bytes=nbytes)

    out = dict(what="minima", config=config, name=wl.name, kernel=eng.kernel_info(), walkers=R, sites=N, n_kinds=obs.n_kinds,
               samples_per_block=ns, thin_by=thin, reps=args.reps)
    for what, spec in specs.items():
        if spec.n_axes:
            eng.set_observables(obs)
        eng.set_minima(spec)
        A, B = [], []
        for i in range(args.warmup + args.reps):
            a, b = arm_a(), arm_b()
            if i >= args.warmup:
                A.append(a)
                B.append(b)
        # the record is the definition's: one more block with every column, offered on the host
        eng.reset_minima()
        eng.run_sampled_async(ns, thin, occupancy=True, observables=bool(spec.n_axes), minima=True)
        smp = eng.fetch_samples()
        want = MinimaRecord(spec, R, eng.F, N, obs.n_kinds if spec.n_axes else 0)
        want.offer(smp["enthalpy"], smp["features"], smp["occupancy"], smp.get("species_counts"))
        got = eng.minima()
        same = all(np.array_equal(getattr(got, f), getattr(want, f)) for f in ("value", "enthalpy", "features", "occupancy", "walker", "sample"))
        k = np.array([b["min_ms"] for b in B])
        mc = np.array([b["mc_ms"] for b in B])
        a_wall, b_wall = stats_ms([x["wall"] / ns for x in A]), stats_ms([x["wall"] / ns for x in B])
        out[what] = dict(
            n_slots=spec.n_slots(R), filled=int(got.filled.sum()), device_equals_definition=bool(same),
            arm_a=dict(per_sample=a_wall, ring_and_fetch_per_sample=stats_ms([x["ring"] / ns for x in A]), bytes_per_sample=A[0]["bytes"] // ns,
                       mc_kernel_ms_per_block=float(np.median([x["mc_ms"] for x in A]))),
            arm_b=dict(per_sample=b_wall, bytes_per_sample=B[0]["bytes"] // ns,
                       rows_winners_copy_kernel_ms_per_block=[float(x) for x in np.median(k, axis=0)],
                       mc_kernel_ms_per_block=float(np.median(mc)), minima_share_of_mc_kernel=float(np.median(k.sum(axis=1) / mc))),
            a_over_b=a_wall["median_ms"] / b_wall["median_ms"], b_not_slower_beyond_spread=bool(b_wall["median_ms"] <= a_wall["max_ms"]))
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "minima_timing.jsonl"))
    args = ap.parse_args()
    for config in (int(c) for c in args.configs.split(",")):
        line = json.dumps(measure(config, args))
        print(line, flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
