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

With --against LIB the tool measures instead whether the fixed-schedule step pays for the search phase of
pop_parent_kernel: device_queued of this build against that of another build of the library (the parent commit's), three
handles on the same chains, calls alternating in one process; the other build against a second handle of itself gives
the spread of such a comparison.

With --adaptive the tool times the adaptive step (Engine.anneal_adaptive) on config 2 for every population
count of --populations (a list), alternating between
  adaptive        Engine.anneal_adaptive: search, resampling and clone on the device
  read_enthalpy   Engine.get_state(occupancy=False): what a host search has to read first
  host_search     PopulationAnnealing.next_temperature on those enthalpies (the host's part alone)
  fixed           Engine.anneal_resample to the temperature the adaptive step of the round chose
and, with --scheme, runs the whole scheme on the enumerable case of tests/pop_anneal_case.py for the overlaps of
--overlaps: steps to reach 300 K and the error of ln Z per population.

python tools/pop_anneal_timing.py [--configs 2,3] [--reps 10] [--against LIB] [--adaptive] [--populations 1,4,64]
                                  [--scheme] [--overlaps 0.7,0.85,0.95] [--out ...]"""
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
    R, P = wl.n_walkers, args.populations[0]
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


def other_engine(path, wl):
    """A handle served by another build of the library (one that may lack the newest entry points)."""
    import ctypes as C

    from smol_amd import engine

    lib = C.CDLL(path)
    for name, (res, argtypes) in engine.SYMBOLS.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, argtypes
    ours, engine._LIB = engine.load_library(), lib
    try:
        return Engine(wl.tables, wl.make_config())
    finally:
        engine._LIB = ours


def measure_against(config, args):
    """The fixed-schedule step, queued and synchronised, of this build against another build: the same chains in three
    handles, one call each per round."""
    wl = workloads.BUILDERS[config](count=REPLICAS[config])
    P = args.populations[0]
    engines = dict(other=other_engine(args.against, wl), other_again=other_engine(args.against, wl), this=Engine(wl.tables, wl.make_config()))
    R = wl.n_walkers
    T = float(np.asarray(wl.temperature).reshape(-1)[0])
    temps = [T, T / args.factor]
    for eng in engines.values():
        eng.set_state(wl.occupancy, wl.seeds, T)
        eng.run(args.steps, sync=True)
    times = {k: [] for k in engines}
    at = 0
    for rep in range(args.reps + 1):  # (the first round warms up)
        pa = parallel.PopulationAnnealing([temps[at], temps[1 - at]], populations=P, seed=args.seed + rep)
        words, parents = pa.offset_words(0), {}
        for k, eng in engines.items():
            eng.run(args.steps, sync=True)
            t0 = time.perf_counter()
            eng.anneal_resample(np.full(P, temps[1 - at]), words, npop=P, outputs=False)
            eng.sync()
            dt = time.perf_counter() - t0
            if rep:
                times[k].append(dt)
            parents[k] = eng.get_state(occupancy=False)["enthalpy"]
        assert all(np.array_equal(v, parents["this"]) for v in parents.values()), "the builds took different steps"
        at = 1 - at
    med = {k: float(np.median(v)) for k, v in times.items()}
    out = dict(what="fixed_step_this_build_against_another", config=wl.name, kernel=engines["this"].kernel_info(), replicas=R,
               populations=P, temperatures=temps, steps_between=args.steps, against=os.path.basename(os.path.dirname(os.path.abspath(args.against))),
               device_queued={k: stats_ms(v) for k, v in times.items()},
               spread_other_against_itself=med["other_again"] / med["other"] - 1.0,
               this_against_other=med["this"] / med["other"] - 1.0, same_states=True)
    for eng in engines.values():
        eng.close()
    return out


def measure_adaptive(P, args):
    """The adaptive step on config 2 with P populations: the device call against the pieces of a host search."""
    wl = workloads.BUILDERS[2](count=REPLICAS[2])
    eng = Engine(wl.tables, wl.make_config())
    R = wl.n_walkers
    T = float(np.asarray(wl.temperature).reshape(-1)[0])
    eng.set_state(wl.occupancy, wl.seeds, T)
    eng.run(args.steps, sync=True)
    PA = parallel.PopulationAnnealing
    target = PA.target_word(args.overlap)
    limit = T / 3  # (every round cools from T towards T / 3 and goes back to T by the fixed step)
    paths = ("adaptive", "read_enthalpy", "host_search", "fixed")
    times = {k: [] for k in paths}
    chosen, agree = [], []
    for rep in range(args.reps + 1):
        pa = PA([T], populations=P, seed=args.seed + rep)
        words = pa.offset_words(0)
        eng.run(args.steps, sync=True)
        t_now = T  # (the fixed step below ends every round where it began)
        t0 = time.perf_counter()
        H = eng.get_state(occupancy=False)["enthalpy"]
        t1 = time.perf_counter()
        t_host = PA.next_temperature(H.reshape(P, R // P), 1.0 / (parallel.kB * t_now), limit, target, args.n_iter)
        t2 = time.perf_counter()
        res = eng.anneal_adaptive(limit, args.overlap, words, npop=P, n_iter=args.n_iter)
        t3 = time.perf_counter()
        eng.run(args.steps, sync=True)
        t4 = time.perf_counter()
        eng.anneal_resample(np.full(P, t_now), words, npop=P)  # a fixed step of the same size, back to where the round began
        t5 = time.perf_counter()
        if rep:
            for k, dt in zip(paths, (t3 - t2, t1 - t0, t2 - t1, t5 - t4)):
                times[k].append(dt)
            chosen.append(res["temperature"] / t_now)
            agree.append(bool(t_host[0] == res["temperature"]))
    out = dict(what="adaptive_step", config=wl.name, kernel=eng.kernel_info(), replicas=R, populations=P, walkers_per_population=R // P,
               overlap=args.overlap, n_iter=args.n_iter, steps_between=args.steps, **{k: stats_ms(v) for k, v in times.items()},
               temperature_ratio_chosen=dict(min=float(np.min(chosen)), max=float(np.max(chosen))),
               host_search_chose_the_same=int(np.sum(agree)), rounds=len(agree),
               adaptive_over_fixed=float(np.median(times["adaptive"]) / np.median(times["fixed"])),
               host_pieces_over_adaptive=float((np.median(times["read_enthalpy"]) + np.median(times["host_search"]) + np.median(times["fixed"]))
                                               / np.median(times["adaptive"])))
    eng.close()
    return out


def measure_scheme(overlap, args):
    """The whole scheme on the enumerable case for one target overlap: steps and errors per seed."""
    from tests import pop_anneal_case as pc
    from tests import wl_windows_case as wc

    rows = []
    for seed in pc.SEEDS:
        R = pc.WALKERS * pc.POPULATIONS
        eng = Engine(wc.case()["tab"], pc.config(R))
        pa = parallel.PopulationAnnealing.adaptive(pc.TEMPERATURES[0], pc.TEMPERATURES[-1], overlap, populations=pc.POPULATIONS,
                                                   seed=seed, n_iter=args.n_iter)
        eng.set_state(pc.start_occupancies(seed, R), pc.walker_seeds(seed, R), pc.TEMPERATURES[0])
        parallel.run_population_annealing(eng, pa, pc.STEPS)
        emean = eng.get_state()["enthalpy"].reshape(pc.POPULATIONS, pc.WALKERS).mean(axis=1)
        rows.append(dict(seed=seed, steps=pa.n_steps, temperatures=[round(float(t), 2) for t in pa.temperatures],
                         lnz_error=[round(float(x), 5) for x in pa.log_partition_ratio() - pc.LNZ_EXACT],
                         emean_error=[round(float(x), 6) for x in emean - pc.EMEAN_EXACT]))
        eng.close()
    return dict(what="adaptive_scheme", case="tests/pop_anneal_case.py", overlap=overlap, n_iter=args.n_iter, fixed_ladder_steps=len(pc.TEMPERATURES) - 1,
                steps=[r["steps"] for r in rows], largest_lnz_error=max(abs(x) for r in rows for x in r["lnz_error"]),
                largest_emean_error=max(abs(x) for r in rows for x in r["emean_error"]), seeds=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="2,3")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--factor", type=float, default=1.02)
    ap.add_argument("--populations", default="1", help="population counts; --adaptive measures each, the other modes take the first")
    ap.add_argument("--against", default=None, help="another build of libsmolmc_hip.so: time the fixed step of this build against it")
    ap.add_argument("--adaptive", action="store_true", help="time the adaptive step on config 2")
    ap.add_argument("--scheme", action="store_true", help="the whole adaptive scheme on the enumerable case, per overlap")
    ap.add_argument("--overlap", type=float, default=0.85)
    ap.add_argument("--overlaps", default="0.7,0.85,0.95")
    ap.add_argument("--n-iter", type=int, default=16)
    ap.add_argument("--append", action="store_true", help="append to --out")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pop_anneal_timing.jsonl"))
    args = ap.parse_args()
    args.populations = [int(x) for x in str(args.populations).split(",")]
    jobs = []
    if args.adaptive or args.scheme:
        if args.adaptive:
            jobs += [(measure_adaptive, P) for P in args.populations]
        if args.scheme:
            jobs += [(measure_scheme, float(x)) for x in args.overlaps.split(",")]
    else:
        jobs = [(measure_against if args.against else measure, int(x)) for x in args.configs.split(",")]
    lines = []
    for fn, arg in jobs:
        row = fn(arg, args)
        print(json.dumps(row), flush=True)
        lines.append(json.dumps(row))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
