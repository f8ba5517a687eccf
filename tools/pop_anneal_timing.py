#!/usr/bin/env python3
"""One population-annealing resampling step on config 2 (4096 walkers) and config 3 (2048 walkers, Ewald
potential field), device path against host path in the same process, alternating between them; one JSON line per
configuration into profiles/pop_anneal_timing.jsonl.

  device          Engine.anneal_resample with its outputs: weights, resampling and clone on the device, the map, the
                  weights and their sums read back
  device_queued   the same with outputs=False, then a stream synchronisation: what a driver that needs no outputs pays
  host            the body of run_population_annealing(host_decide=True): get_state, PopulationAnnealing.step,
                  set_state(occupancy[parent], reset_aux=False) + set_counters

Wall clock from a synchronised stream to a synchronised stream.  The populations alternate between the configuration's
temperature T and T / --factor, so every step reweights (db of either sign) and clones; the clones per step are
recorded.  --steps Metropolis steps run between two measurements.

python tools/pop_anneal_timing.py [--configs 2,3] [--reps 10] [--out ...]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from smol_amd import parallel, workloads  # noqa: E402
from smol_amd.engine import Engine  # noqa: E402

REPLICAS = {2: 4096, 3: 2048}


def stats_ms(samples):
    a = np.asarray(samples) * 1e3
    return dict(median_ms=float(np.median(a)), min_ms=float(a.min()), max_ms=float(a.max()), n=len(a))


def measure(config, args):
    wl = workloads.BUILDERS[config](count=REPLICAS[config])
    eng = Engine(wl.tables, wl.make_config())
    R, P = wl.n_walkers, args.populations
    T = float(np.asarray(wl.temperature).reshape(-1)[0])
    eng.set_state(wl.occupancy, wl.seeds, T)
    eng.run(args.steps, sync=True)
    temps = [T, T / args.factor]
    at = 0  # index into temps of the temperature in force
    times = dict(device=[], device_queued=[], host=[])
    clones = dict(device=[], device_queued=[], host=[])
    attempt = 0
    dummy_seeds = np.zeros(R, dtype=np.uint64)
    for rep in range(args.reps + 1):  # (the first round warms up: allocations, first launches)
        for path in ("device", "host", "device_queued"):
            eng.run(args.steps, sync=True)
            pa = parallel.PopulationAnnealing([temps[at], temps[1 - at]], populations=P, seed=args.seed + attempt)
            t0 = time.perf_counter()
            if path == "host":
                st = eng.get_state()
                parent = pa.step(st["enthalpy"], 0)["parent"]
                eng.set_state(st["occupancy"][parent], dummy_seeds, np.full(R, temps[1 - at]), reset_aux=False)
                eng.set_counters(st["n_steps"], st["n_accepted"])
                eng.sync()
            elif path == "device":
                parent = eng.anneal_resample(np.full(P, temps[1 - at]), pa.offset_words(0), npop=P)["parent"]
            else:
                eng.anneal_resample(np.full(P, temps[1 - at]), pa.offset_words(0), npop=P, outputs=False)
                eng.sync()
                parent = None
            dt = time.perf_counter() - t0
            at, attempt = 1 - at, attempt + 1
            if rep:
                times[path].append(dt)
                if parent is not None:
                    clones[path].append(int((np.asarray(parent) != np.arange(R)).sum()))
    st = eng.get_state()
    drift = eng.audit_drift()
    row_bytes = eng.N + 8 * eng.F + 9
    out = dict(config=wl.name, kernel=eng.kernel_info(), replicas=R, populations=P, temperatures=temps,
               steps_between=args.steps, clones_per_step=dict(device=float(np.mean(clones["device"])), host=float(np.mean(clones["host"]))),
               device=stats_ms(times["device"]), device_queued=stats_ms(times["device_queued"]), host=stats_ms(times["host"]),
               host_over_device=float(np.median(times["host"]) / np.median(times["device"])),
               host_over_device_queued=float(np.median(times["host"]) / np.median(times["device_queued"])),
               state_bytes_per_walker_without_field=row_bytes, drift_after=dict(features=drift[0], enthalpy=drift[1]),
               acceptance=float(st["n_accepted"].sum()) / float(st["n_steps"].sum()))
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="2,3")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--factor", type=float, default=1.02)
    ap.add_argument("--populations", type=int, default=1)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pop_anneal_timing.jsonl"))
    args = ap.parse_args()
    lines = []
    for config in (int(x) for x in args.configs.split(",")):
        row = measure(config, args)
        print(json.dumps(row), flush=True)
        lines.append(json.dumps(row))
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
