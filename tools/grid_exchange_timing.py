#!/usr/bin/env python3
"""What one exchange attempt across the mu-T grid costs: config 14 (32 T x 64 mu, 2048 walkers of 3456
sites in one handle), one attempt decided and applied on the device (Engine.exchange_grid) against the same attempt on
the host (read the state back, parallel.GridExchange.decide, set_temperature + set_walker_mu: only calls the engine had
before the device move), and against the kernel time of one sweep.  Wall clock from a synchronised stream to a
synchronised stream, the four moves in turn; warm-up attempts first, then median / min / max over the repetitions.
python tools/grid_exchange_timing.py [--reps 40] [--out profiles/grid_exchange_timing.jsonl]"""
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


def stats_ms(samples):
    a = np.asarray(samples) * 1e3
    return dict(median_ms=float(np.median(a)), min_ms=float(a.min()), max_ms=float(a.max()), n=len(a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grid_exchange_timing.jsonl"))
    args = ap.parse_args()

    wl = workloads.config14()
    nT, nMu = wl.extras["grid"]
    rows = wl.extras["walker_mu"]
    gx = parallel.GridExchange(wl.temperature[::nMu], rows[:nMu], seed=14)
    assert np.array_equal(gx.point_rows, rows) and np.array_equal(gx.point_temperatures, wl.temperature)
    eng = Engine(wl.tables, wl.make_config())
    eng.set_walker_mu(rows)
    eng.set_state(wl.occupancy, wl.seeds, wl.temperature)
    sweep = int(sum(len(sites) for sites in wl.tables.active_sites()))  # one flip attempt per active site
    eng.run(20 * sweep, sync=True)

    # kernel time of one sweep
    sweeps = []
    for _ in range(10):
        eng.run(sweep, sync=True)
        sweeps.append(eng.last_kernel_ms() * 1e-3)
    out = dict(config="config14", walkers=wl.n_walkers, grid=[int(nT), int(nMu)], sites=int(wl.sc.num_sites),
               steps_per_sweep=int(sweep), kernel=eng.kernel_info(), sweep_kernel=stats_ms(sweeps))

    def device_attempt(attempt, with_stats):
        move = gx.move_of(attempt)
        pairs = gx.pairs(move)
        log_u = gx.log_u(attempt, len(pairs))
        stats = np.zeros((len(pairs), 2), dtype=np.int64) if with_stats else None
        t0 = time.perf_counter()
        eng.exchange_grid(pairs, log_u, stats)
        eng.sync()
        return time.perf_counter() - t0, (int(stats[:, 1].sum()) if with_stats else 0), len(pairs)

    def host_attempt(attempt, point_of):
        move = gx.move_of(attempt)
        t0 = time.perf_counter()
        st = eng.get_state()
        res = gx.decide(st["enthalpy"], eng.species_counts(st["occupancy"]), point_of, move, attempt, record=False)
        eng.set_temperature(gx.point_temperatures[res["point_of"]])
        eng.set_walker_mu(gx.point_rows[res["point_of"]])
        eng.sync()
        return time.perf_counter() - t0, int(res["accept"].sum()), res["point_of"]

    # the walkers keep moving between attempts (a fifth of a sweep), so that attempts keep being accepted
    attempt = 0
    for name, with_stats in (("device_attempt", False), ("device_attempt_with_stats", True)):
        times, acc, att = [], 0, 0
        for i in range(args.warmup + args.reps):
            eng.run(sweep // 5, sync=True)
            dt, a, n = device_attempt(attempt, with_stats)
            attempt += 1
            if i >= args.warmup:
                times.append(dt)
                acc, att = acc + a, att + n
        out[name] = stats_ms(times)
        if with_stats:
            out[name]["acceptance"] = acc / max(att, 1)
    # host path: the engine's points are named anew by every set call; the grid's map is kept here
    point_of = eng.state_points()[0].astype(np.int64)
    times, acc = [], 0
    for i in range(max(2, args.warmup // 4) + max(5, args.reps // 4)):
        eng.run(sweep // 5, sync=True)
        dt, a, point_of = host_attempt(attempt, point_of)
        attempt += 1
        if i >= max(2, args.warmup // 4):
            times.append(dt)
            acc += a
    out["host_attempt"] = stats_ms(times)
    out["host_over_device"] = out["host_attempt"]["median_ms"] / out["device_attempt"]["median_ms"]
    out["device_attempt_over_sweep"] = out["device_attempt"]["median_ms"] / out["sweep_kernel"]["median_ms"]
    out["host_attempt_over_sweep"] = out["host_attempt"]["median_ms"] / out["sweep_kernel"]["median_ms"]
    # the state is still priced right after all of it
    st = eng.get_state()
    out["max_work_error"] = float(np.max(np.abs(st["features"][:, -1] - eng.chemical_work(st["occupancy"], eng.get_walker_mu()))))
    eng.close()
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
