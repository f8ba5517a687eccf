#!/usr/bin/env python3
"""What a statistics record keyed by bins of a column costs, one JSON line per shape into
profiles/statistics_bins_timing.jsonl:

  shapes   config 2 (the headline: R = 4096 walkers of N = 4096 sites, 16-sample blocks = 65536 rows) with
             bins256      256 bins of the enthalpy over the range the equilibrated walkers span
             composition  Statistics.by_composition, 4097 keys (a canonical run: every row meets in one key)
             thin         65536 bins over the same range: the rows spread thin, the worst case of the scan
           config 15 (16 windows x 64 copies of replica-exchange Wang-Landau) with Statistics.on_wl_levels on the global
           grid
  blocks   --samples samples per block, one sample per sweep; --reps blocks per arm, the arms alternating block by
           block (a new spec starts an empty record, which costs no device time in the block); --warmup rounds first
  arms     walker       the per-walker record of the same columns (statistics_kernel: the parent's kernel), the yardstick
           <shape>      the binned record: the device times of its two launches of statistics_kernel, the key pass and the
                        reduction per key (HIP events)
           host         the path the record replaces: the ring without occupancy (with the counts where the key needs
                        them), the fetch, then grouping by key in NumPy: n, sum x and sum x x^T per key

  device time per block and per sample, its share of the block's MC kernel time, wall time per sample of every arm, and
  whether the device record of one more block equals the definition.

python tools/statistics_bins_timing.py [--configs 2,15] [--samples 16] [--reps 5] [--out ...]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from smol_amd import capi, workloads  # noqa: E402,F401
from smol_amd import statistics as st  # noqa: E402
from smol_amd.engine import Engine  # noqa: E402
from smol_amd.observables import Observables  # noqa: E402
from smol_amd.statistics import Statistics, StatisticsRecord  # noqa: E402


def stats_ms(samples):
    a = np.asarray(samples) * 1e3
    return dict(median_ms=float(np.median(a)), min_ms=float(a.min()), max_ms=float(a.max()), n=len(a))


def host_group(spec, smp):
    """Fetch-and-group: n, sum x and sum x x^T per key of a fetched block, in NumPy."""
    x = spec.column_values(smp["enthalpy"], smp["features"], smp.get("species_counts")).reshape(-1, spec.n_columns)
    q = st.bin_of(x[:, spec.key_column], spec.key_min, spec.key_bin)
    ok = np.isfinite(q) & (q >= 0) & (q < spec.n_keys)
    k, x = q[ok].astype(np.int64), x[ok]
    n = np.bincount(k, minlength=spec.n_keys)
    s1 = np.stack([np.bincount(k, weights=x[:, c], minlength=spec.n_keys) for c in range(spec.n_columns)], axis=1)
    ia, ib = np.triu_indices(spec.n_columns)
    s2 = np.stack([np.bincount(k, weights=x[:, a] * x[:, b], minlength=spec.n_keys) for a, b in zip(ia, ib)], axis=1)
    return n, s1, s2


def measure(config, eng, shapes, walker_spec, args, name, extra):
    R, N, ns = eng.R, eng.N, args.samples
    thin = N  # one sweep
    arms = {what: [] for what in shapes}
    arms["walker"], host = [], {what: [] for what in shapes}
    for i in range(args.warmup + args.reps):
        keep = i >= args.warmup
        eng.set_statistics(walker_spec)
        t0 = time.perf_counter()
        eng.run_sampled_async(ns, thin, occupancy=False, statistics=True)
        eng.fetch_samples()
        t1 = time.perf_counter()
        if keep:
            arms["walker"].append(dict(wall=t1 - t0, mc_ms=eng.last_kernel_ms(), stat_ms=eng.statistics_kernel_ms()))
        for what, spec in shapes.items():
            eng.set_statistics(spec)
            t0 = time.perf_counter()
            eng.run_sampled_async(ns, thin, occupancy=False, statistics=True)
            eng.fetch_samples()
            t1 = time.perf_counter()
            keys_ms, reduce_ms = eng.statistics_bins_kernel_ms()
            if keep:
                arms[what].append(dict(wall=t1 - t0, mc_ms=eng.last_kernel_ms(), keys_ms=keys_ms, reduce_ms=reduce_ms))
            eng.set_statistics(None)
            t0 = time.perf_counter()
            eng.run_sampled_async(ns, thin, occupancy=False, observables=bool(spec.count_columns()))
            host_group(spec, eng.fetch_samples())
            t1 = time.perf_counter()
            if keep:
                host[what].append(t1 - t0)
    out = []
    wk = np.array([b["stat_ms"] for b in arms["walker"]])
    for what, spec in shapes.items():
        eng.set_statistics(spec)  # the record is the definition's: one more block, offered on the host
        smp = eng.run_sampled(ns, thin, occupancy=False, statistics=True, observables=bool(spec.count_columns()))
        got = eng.statistics()
        same = got.equals(StatisticsRecord(spec).offer(smp["enthalpy"], smp["features"], smp.get("species_counts")))
        B = arms[what]
        keys, red, mc = (np.array([b[f] for b in B]) for f in ("keys_ms", "reduce_ms", "mc_ms"))
        both = keys + red
        wall = stats_ms([b["wall"] / ns for b in B])
        hwall = stats_ms([t / ns for t in host[what]])
        out.append(dict(
            what="statistics_bins", config=config, name=name, kernel=eng.kernel_info(), walkers=R, sites=N, shape=what,
            n_keys=spec.n_keys, columns=spec.n_columns, samples_per_block=ns, rows_per_block=ns * R, thin_by=thin, reps=args.reps,
            keys_with_rows=int((got.n > 0).sum()), rows_outside=int(got.key_under + got.key_over), device_equals_definition=bool(same),
            key_pass_us_per_block=float(np.median(keys)) * 1e3,
            reduction_us_per_block=float(np.median(red)) * 1e3,
            both_passes_us_per_block=float(np.median(both)) * 1e3, both_passes_us_per_sample=float(np.median(both)) * 1e3 / ns,
            both_passes_us_per_block_range=[float(both.min()) * 1e3, float(both.max()) * 1e3],
            per_walker_statistics_kernel_us_per_block=float(np.median(wk)) * 1e3,
            per_walker_statistics_kernel_us_per_sample=float(np.median(wk)) * 1e3 / ns,
            binned_over_per_walker=float(np.median(both) / np.median(wk)),
            mc_kernel_ms_per_block=float(np.median(mc)), share_of_mc_kernel=float(np.median(both / mc)),
            wall_per_sample=wall, wall_per_sample_per_walker_record=stats_ms([b["wall"] / ns for b in arms["walker"]]),
            wall_per_sample_fetch_and_group=hwall, fetch_and_group_over_record=hwall["median_ms"] / wall["median_ms"], **extra))
    return out


def config2(args):
    kw = dict(count=args.replicas) if args.replicas else {}
    if args.dim:
        kw["dim"] = args.dim
    wl = workloads.BUILDERS[2](**kw)
    eng = Engine(wl.tables, wl.make_config())
    obs = Observables.from_supercell(wl.sc, tables=wl.tables)
    eng.set_observables(obs)
    eng.set_state(wl.occupancy, wl.seeds, wl.temperature)
    eng.run(20 * eng.N, sync=True)
    H0 = eng.get_state()["enthalpy"]
    lo, hi = float(H0.min()), float(H0.max())
    span = max(hi - lo, 1e-6)
    cols = [st.ENTHALPY] + [st.feature(i) for i in range(min(eng.F, args.columns - 2))] + [st.kind(obs, 1)]
    shapes = {
        "bins256": Statistics.by_bin(st.ENTHALPY, 256, lo - 0.5 * span, 2.0 * span / 256, columns=cols),
        "composition": Statistics.by_composition(obs, 1, eng.N, columns=cols),
        "thin": Statistics.by_bin(st.ENTHALPY, 65536, lo - 0.5 * span, 2.0 * span / 65536, columns=cols),
    }
    out = measure(2, eng, shapes, Statistics.per_walker(cols), args, wl.name, {})
    eng.close()
    return out


def config15(args):
    from bench_configs import windowed_engine

    kw = dict(count=args.replicas) if args.replicas else {}
    wl = workloads.BUILDERS[15](**kw)
    probe = Engine(wl.tables, capi.make_config(1))
    h0 = float(probe.natural_parameters @ probe.eval_full(wl.occupancy[:1])[0])
    probe.close()
    wl = workloads.BUILDERS[15](h0=h0, **kw)
    eng, wx, seed_steps = windowed_engine(wl)
    cols = [st.ENTHALPY] + [st.feature(i) for i in range(min(eng.F, args.columns - 1))]
    shapes = {"wl_levels": Statistics.on_wl_levels(wx.min_enthalpy, wx.bin_size, wx.L, columns=cols)}
    out = measure(15, eng, shapes, Statistics.per_walker(cols), args, wl.name,
                  dict(windows=wx.n_windows, copies=wx.copies, seed_steps_per_walker=seed_steps))
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", default="2,15")
    ap.add_argument("--replicas", type=int, default=0, help="walkers (default: the configuration's)")
    ap.add_argument("--dim", type=int, default=0, help="supercell size of config 2 (default: the configuration's)")
    ap.add_argument("--samples", type=int, default=16, help="samples per block")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--columns", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "statistics_bins_timing.jsonl"))
    args = ap.parse_args()
    for config in (int(c) for c in args.configs.split(",")):
        for row in {2: config2, 15: config15}[config](args):
            line = json.dumps(row)
            print(line, flush=True)
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
