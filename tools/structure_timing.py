#!/usr/bin/env python3
"""What structure factors of every sample cost, on the device against on the host, one JSON line per set of
wave vectors into profiles/structure_timing.jsonl:

  shape    config 2 (the headline: R = 4096 walkers of N = 4096 sites, two kinds)
  points   "superlattice": Gamma and the three X points (the L1_0 / L1_2 reflections): 4 points of at most 2 phase
           classes, 4 cells
           "grid": g = 4 (i, j, k), i, j, k < 4: 64 points of at most 4 classes, 8 cells
           "plane": g = (i, j, 0), i, j < 8: 64 points of up to 16 classes, 32 cells
           every kind pair of every point is an intensity; the kernel each spec takes is reported (capi.structure_plan)
  blocks   --samples samples per block, one sample per sweep (thin_by = N steps per walker); --reps blocks, --warmup first
  device   the block with SMOLMC_SAMPLE_STRUCTURE and without the occupancy column: wall time per sample from the queueing
           of the block to the columns in hand, the kernel's own time (HIP events around its launch) and its share of the
           block's MC kernel time (the events of smolmc_last_kernel_ms)
  host     one sample with the occupancy column, fetched packed, then StructureFactor.evaluate in NumPy (one thread)

python tools/structure_timing.py [--sets superlattice,grid,plane] [--samples 16] [--reps 3] [--out ...]"""
import argparse
import itertools
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from smol_amd import capi, workloads  # noqa: E402,F401
from smol_amd.engine import Engine  # noqa: E402
from smol_amd.structure import StructureFactor  # noqa: E402


def point_sets(dim):
    h, q = dim // 2, dim // 4
    return {
        "superlattice": np.array([[0, 0, 0], [h, h, 0], [h, 0, h], [0, h, h]]),
        "grid": np.array([[q * i, q * j, q * k] for i, j, k in itertools.product(range(4), repeat=3)]),
        "plane": np.array([[i, j, 0] for i, j in itertools.product(range(8), repeat=2)]),
    }


def stats_ms(samples):
    a = np.asarray(samples) * 1e3
    return dict(median_ms=float(np.median(a)), min_ms=float(a.min()), max_ms=float(a.max()), n=len(a))


def measure(which, args):
    kw = dict(count=args.replicas) if args.replicas else {}
    if args.dim:
        kw["dim"] = args.dim
    wl = workloads.BUILDERS[2](**kw)
    eng = Engine(wl.tables, wl.make_config())
    eng.set_state(wl.occupancy, wl.seeds, wl.temperature)
    R, N, ns = eng.R, eng.N, args.samples
    thin = N  # one sweep
    g = point_sets(int(round(N ** (1 / 3))))[which]
    K = 2
    its = [(p, a, b) for p in range(len(g)) for a in range(K) for b in range(a, K)]
    sf = StructureFactor.from_supercell(wl.sc, g, intensities=its)
    eng.set_structure_factor(sf)
    eng.run(20 * N, sync=True)

    def device():
        t0 = time.perf_counter()
        eng.run_sampled_async(ns, thin, occupancy=False, structure=True)
        eng.fetch_samples()
        t1 = time.perf_counter()
        return dict(wall=t1 - t0, mc_ms=eng.last_kernel_ms(), sf_ms=eng.structure_kernel_ms())

    D = [device() for _ in range(args.warmup + args.reps)][args.warmup:]
    # the host path, one sample: the occupancies come back, NumPy evaluates the definition
    t0 = time.perf_counter()
    eng.run_sampled_async(1, thin, occupancy=True, structure=True)
    smp = eng.fetch_samples(packed=True)
    t1 = time.perf_counter()
    want = sf.evaluate(smp["occupancy"])
    t2 = time.perf_counter()
    same = bool(np.array_equal(want[0], smp["structure_amplitudes"]) and np.array_equal(want[1], smp["structure_intensities"]))
    k = np.array([d["sf_ms"] for d in D])
    mc = np.array([d["mc_ms"] for d in D])
    dev = stats_ms([d["wall"] / ns for d in D])
    host_ms = (t2 - t0) * 1e3
    out = dict(what="structure", config=2, name=wl.name, kernel=eng.kernel_info(), walkers=R, sites=N, points=which,
               n_points=sf.n_points, n_kinds=sf.n_kinds, n_phases=sf.n_phases, n_intensities=sf.n_intensities,
               cells_per_point=sf.n_kinds * sf.n_phases,
               counting=capi.structure_plan(N, (N + 15) // 16 * 16, sf.n_kinds, sf.n_phases, sf.n_points)[0],
               samples_per_block=ns, thin_by=thin, reps=args.reps, device_equals_definition=same,
               device=dict(per_sample=dev, structure_kernel_ms_per_block=float(np.median(k)),
                           structure_kernel_us_per_sample=float(np.median(k)) * 1e3 / ns,
                           mc_kernel_ms_per_block=float(np.median(mc)), structure_share_of_mc_kernel=float(np.median(k / mc))),
               host=dict(per_sample_ms=host_ms, ring_and_fetch_ms=(t1 - t0) * 1e3, evaluate_ms=(t2 - t1) * 1e3, n=1),
               host_over_device=host_ms / dev["median_ms"])
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sets", default="superlattice,grid,plane")
    ap.add_argument("--replicas", type=int, default=0, help="walkers (default: the configuration's)")
    ap.add_argument("--dim", type=int, default=0, help="supercell size (default: the configuration's)")
    ap.add_argument("--samples", type=int, default=16, help="samples per block")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "structure_timing.jsonl"))
    args = ap.parse_args()
    for which in args.sets.split(","):
        line = json.dumps(measure(which, args))
        print(line, flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
