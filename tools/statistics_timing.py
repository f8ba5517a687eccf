#!/usr/bin/env python3
"""What keeping the statistics record costs, on the device against on the host, one JSON line per shape
into profiles/statistics_timing.jsonl:

  shapes   config 2 (the headline: R = 4096 walkers of N = 4096 sites, keyed by walker) and config 14 (the mu-T grid in
           one handle, keyed by state point)
  blocks   --samples samples per block, one sample per sweep (thin_by = N steps per walker); --reps blocks per arm, the
           arms alternating; --warmup blocks of each first
  arm A    the existing path: the ring without occupancy, the fetch, then NumPy: the columns of the block, on config 14
           regrouped by state point, and their running sums of x and of x x^T
  arm B    the record on the device: the same block with SMOLMC_SAMPLE_STATISTICS (the trace columns still come back,
           nobody has to look at them)
  record   enthalpy, the first features and the energy -- --columns in all -- with 16 blocking levels and a histogram of
           256 bins on the enthalpy

  wall time per sample of the arms (host clock from the queueing of the block to the result in hand, median and range
  over the blocks), the reduction kernel's own time (HIP events around its launch) and its share of the block's MC kernel
  time (the events of smolmc_last_kernel_ms).

python tools/statistics_timing.py [--configs 2,14] [--samples 16] [--reps 5] [--columns 8] [--out ...]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from smol_amd import capi, workloads  # noqa: E402,F401
from smol_amd import statistics as st  # noqa: E402
from smol_amd.engine import Engine  # noqa: E402
from smol_amd.statistics import Statistics, StatisticsRecord  # noqa: E402


def stats_ms(samples):
    a = np.asarray(samples) * 1e3
    return dict(median_ms=float(np.median(a)), min_ms=float(a.min()), max_ms=float(a.max()), n=len(a))


def measure(config, args):
    kw = dict(count=args.replicas) if args.replicas else {}
    if args.dim:
        kw["dim"] = args.dim
    wl = workloads.BUILDERS[config](**kw)
    eng = Engine(wl.tables, wl.make_config())
    keyed = "walker_mu" in wl.extras
    if keyed:
        eng.set_walker_mu(wl.extras["walker_mu"])
    eng.set_state(wl.occupancy, wl.seeds, wl.temperature)
    R, N, ns = eng.R, eng.N, args.samples
    thin = N  # one sweep
    eng.run(20 * N, sync=True)
    H0 = eng.get_state()["enthalpy"]
    span = max(float(H0.max() - H0.min()), 1.0)
    nfeat = max(0, min(eng.F, args.columns - 2))
    cols = [st.ENTHALPY] + [st.feature(i) for i in range(nfeat)] + [st.ENERGY]
    spec = Statistics(st.BY_STATE_POINT if keyed else st.BY_WALKER, cols, weights=eng.natural_parameters[:max(1, eng.F - 1)],
                      n_levels=16, hist=(st.ENTHALPY, 256, float(H0.min()) - span, 3.0 * span / 256))
    eng.set_statistics(spec)
    Cn = spec.n_columns
    host = dict(n=0, s1=np.zeros((R, Cn)), s2=np.zeros((R, Cn, Cn)))

    def arm_a():
        t0 = time.perf_counter()
        eng.run_sampled_async(ns, thin, occupancy=False)
        smp = eng.fetch_samples()
        t1 = time.perf_counter()
        x = spec.column_values(smp["enthalpy"], smp["features"])  # (ns, R, C)
        if keyed:  # regroup: row r of a sample belongs to the state point walker r holds
            point_of = eng.state_points()[0]
            by = np.empty_like(x)
            by[:, point_of] = x
            x = by
        host["n"] += ns
        host["s1"] += x.sum(axis=0)
        host["s2"] += np.einsum("sra,srb->rab", x, x)
        t2 = time.perf_counter()
        return dict(ring=t1 - t0, wall=t2 - t0, mc_ms=eng.last_kernel_ms())

    def arm_b():
        t0 = time.perf_counter()
        eng.run_sampled_async(ns, thin, occupancy=False, statistics=True)
        eng.fetch_samples()
        t1 = time.perf_counter()
        return dict(wall=t1 - t0, mc_ms=eng.last_kernel_ms(), stat_ms=eng.statistics_kernel_ms())

    A, B = [], []
    for i in range(args.warmup + args.reps):
        a, b = arm_a(), arm_b()
        if i >= args.warmup:
            A.append(a)
            B.append(b)
    # the record is the definition's: one more block, offered on the host
    eng.reset_statistics()
    key = eng.state_points()[0] if keyed else None
    smp = eng.run_sampled(ns, thin, occupancy=False, statistics=True)
    want = StatisticsRecord(spec, R).offer(smp["enthalpy"], smp["features"], None, key)
    same = eng.statistics().equals(want)
    k = np.array([b["stat_ms"] for b in B])
    mc = np.array([b["mc_ms"] for b in B])
    a_wall, b_wall = stats_ms([x["wall"] / ns for x in A]), stats_ms([x["wall"] / ns for x in B])
    out = dict(what="statistics", config=config, name=wl.name, kernel=eng.kernel_info(), walkers=R, sites=N,
               key="state point" if keyed else "walker", columns=Cn, n_levels=spec.n_levels, n_bins=spec.n_bins,
               samples_per_block=ns, thin_by=thin, reps=args.reps, device_equals_definition=bool(same),
               arm_a=dict(per_sample=a_wall, ring_and_fetch_per_sample=stats_ms([x["ring"] / ns for x in A]),
                          mc_kernel_ms_per_block=float(np.median([x["mc_ms"] for x in A]))),
               arm_b=dict(per_sample=b_wall, statistics_kernel_ms_per_block=float(np.median(k)),
                          statistics_kernel_us_per_sample=float(np.median(k)) * 1e3 / ns,
                          mc_kernel_ms_per_block=float(np.median(mc)), statistics_share_of_mc_kernel=float(np.median(k / mc))),
               a_over_b=a_wall["median_ms"] / b_wall["median_ms"])
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", default="2,14")
    ap.add_argument("--replicas", type=int, default=0, help="walkers (default: the configuration's)")
    ap.add_argument("--dim", type=int, default=0, help="supercell size (default: the configuration's)")
    ap.add_argument("--samples", type=int, default=16, help="samples per block")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--columns", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "statistics_timing.jsonl"))
    args = ap.parse_args()
    for config in (int(c) for c in args.configs.split(",")):
        line = json.dumps(measure(config, args))
        print(line, flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
