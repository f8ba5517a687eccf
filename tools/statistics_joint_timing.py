#!/usr/bin/env python3
"""What the joint field of a statistics record costs, one JSON line per shape into
profiles/statistics_joint_timing.jsonl:

  shapes   config 2 (the headline: R = 4096 walkers of N = 4096 sites, 16-sample blocks = 65536 rows), 64 x 64 cells of
           the enthalpy and feature 1, with the record keyed
             walker    by walker: one thread per key, the only owner of its cells, no atomics
             bins256   by 256 bins of the enthalpy over the range the equilibrated walkers span: one thread per row,
                       neighbouring rows in different keys and cells
             one       by one bin that takes every row, the cells so wide that every row meets in ONE of them: the rows of a
                       wave are merged into one atomic
  blocks   --samples samples per block, one sample per sweep; --reps blocks per arm, the arms alternating block by
           block; --warmup rounds first
  arms     field     the block with the record and its field, nothing fetched but the record: the device time of the
                     field's launch and of the record's own launches (HIP events) and the wall time
           plain     the same record WITHOUT a joint field: its launches' device time, the figure to hold against another
                     build's (tools/statistics_timing.py measures the per-walker record alone)
           host      the path the field replaces: the two columns fetched with the block, then np.add.at per key and cell

  device time of the field's launch per block, its share of the block's MC kernel time, the record's launches with and
  without the field, wall time per sample of the arms, and whether the device field of one more block equals the NumPy
  sums.

python tools/statistics_joint_timing.py [--samples 16] [--reps 5] [--replicas R] [--dim D] [--out ...]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from smol_amd import workloads  # noqa: E402
from smol_amd import statistics as st  # noqa: E402
from smol_amd.engine import Engine  # noqa: E402
from smol_amd.statistics import Statistics  # noqa: E402


def stats_ms(samples):
    a = np.asarray(samples) * 1e3
    return dict(median_ms=float(np.median(a)), min_ms=float(a.min()), max_ms=float(a.max()), n=len(a))


def record_ms(eng, spec):
    """Device time of the record's own launches of the last block: the reduction, or the key pass and the reduction."""
    return float(sum(eng.statistics_bins_kernel_ms())) if spec.binned else float(eng.statistics_kernel_ms())


def host_field(spec, smp, n_keys):
    """(joint (n_keys, n_a, n_b), joint_out (n_keys,)) of a fetched block: the key and the cell of every row, then one
    np.add.at."""
    H = smp["enthalpy"]
    ns, R = H.shape
    x = spec.column_values(H, smp["features"]).reshape(ns * R, -1)
    if spec.binned:
        q = st.bin_of(x[:, spec.key_column], spec.key_min, spec.key_bin)
        ok = np.isfinite(q) & (q >= 0) & (q < n_keys)
        keys = np.where(ok, np.nan_to_num(q, nan=0.0, posinf=0.0, neginf=0.0), -1).astype(np.int64)
    else:
        keys = np.tile(np.arange(R), ns)
    offered = keys >= 0
    inside, cell = offered.copy(), np.zeros(len(x), dtype=np.int64)
    for i in (0, 1):
        xv = x[:, spec.joint_columns[i]]
        q = st.bin_of(xv, spec.joint_min[i], spec.joint_bin[i])
        ok = np.isfinite(xv) & np.isfinite(q) & (q >= 0) & (q < spec.joint_n[i])
        inside &= ok
        cell = cell * spec.joint_n[i] + np.where(ok, np.nan_to_num(q, nan=0.0, posinf=0.0, neginf=0.0), 0.0).astype(np.int64)
    joint = np.zeros((n_keys, spec.joint_n[0] * spec.joint_n[1]), dtype=np.int64)
    np.add.at(joint, (keys[inside], cell[inside]), 1)
    out = np.bincount(keys[offered & ~inside], minlength=n_keys).astype(np.int64)
    return joint.reshape((n_keys,) + tuple(spec.joint_n)), out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--replicas", type=int, default=0, help="walkers (default: the configuration's)")
    ap.add_argument("--dim", type=int, default=0, help="supercell size of config 2 (default: the configuration's)")
    ap.add_argument("--samples", type=int, default=16, help="samples per block")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cells", type=int, default=64, help="cells per axis")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "statistics_joint_timing.jsonl"))
    args = ap.parse_args()
    kw = dict(count=args.replicas) if args.replicas else {}
    if args.dim:
        kw["dim"] = args.dim
    wl = workloads.BUILDERS[2](**kw)
    eng = Engine(wl.tables, wl.make_config())
    eng.set_state(wl.occupancy, wl.seeds, wl.temperature)
    eng.run(20 * eng.N, sync=True)
    s0 = eng.get_state(occupancy=False)
    H0, f0 = s0["enthalpy"], s0["features"][:, 1]
    lo, span = float(H0.min()), max(float(H0.max() - H0.min()), 1e-6)
    flo, fspan = float(f0.min()), max(float(f0.max() - f0.min()), 1e-6)
    R, N, ns, n = eng.R, eng.N, args.samples, args.cells
    thin = N  # one sweep
    cols = [st.ENTHALPY, st.feature(1)]
    spread = ((st.ENTHALPY, n, lo - 0.5 * span, 2.0 * span / n), (st.feature(1), n, flo - 0.5 * fspan, 2.0 * fspan / n))
    meet = ((st.ENTHALPY, n, lo - 32e3 * span, 1e3 * span), (st.feature(1), n, flo - 32e3 * fspan, 1e3 * fspan))
    shapes = {
        "walker": lambda joint: Statistics.per_walker(cols, joint=joint and spread),
        "bins256": lambda joint: Statistics.by_bin(st.ENTHALPY, 256, lo - 0.5 * span, 2.0 * span / 256, columns=cols, joint=joint and spread),
        "one": lambda joint: Statistics.by_bin(st.ENTHALPY, 1, lo - 1e3 * span, 2e3 * span, columns=cols, joint=joint and meet),
    }
    arms = {what: [] for what in shapes}
    plain = {what: [] for what in shapes}
    host = {what: [] for what in shapes}
    for i in range(args.warmup + args.reps):
        keep = i >= args.warmup
        for what, make in shapes.items():
            spec = make(True)
            eng.set_statistics(spec)
            t0 = time.perf_counter()
            eng.run_sampled_async(ns, thin, occupancy=False, statistics=True)
            eng.fetch_samples()
            t1 = time.perf_counter()
            rec = eng.statistics()  # (a run downloads the record once, at its end)
            t2 = time.perf_counter()
            if keep:
                arms[what].append(dict(wall=t1 - t0, download=t2 - t1, mc_ms=eng.last_kernel_ms(), joint_ms=eng.statistics_joint_kernel_ms(),
                                       record_ms=record_ms(eng, spec)))
            del rec
            bare = make(None)
            eng.set_statistics(bare)
            eng.run_sampled_async(ns, thin, occupancy=False, statistics=True)
            eng.fetch_samples()
            if keep:
                plain[what].append(record_ms(eng, bare))
            eng.set_statistics(None)
            t0 = time.perf_counter()
            eng.run_sampled_async(ns, thin, occupancy=False)
            smp = eng.fetch_samples()
            host_field(spec, smp, spec.n_keys if spec.binned else R)
            t1 = time.perf_counter()
            if keep:
                host[what].append(t1 - t0)
    for what, make in shapes.items():
        spec = make(True)
        n_keys = spec.n_keys if spec.binned else R
        eng.set_statistics(spec)  # one more block, its columns fetched: the device field against the definition
        smp = eng.run_sampled(ns, thin, occupancy=False, statistics=True)
        got = eng.statistics()
        want, want_out = host_field(spec, smp, n_keys)
        same = bool(np.array_equal(got.joint, want) and np.array_equal(got.joint_out, want_out)
                    and np.array_equal(got.joint.sum(axis=(1, 2)) + got.joint_out, got.n))
        B = arms[what]
        dev, mc, own = (np.array([b[f] for b in B]) for f in ("joint_ms", "mc_ms", "record_ms"))
        bare = np.array(plain[what])
        wall = stats_ms([b["wall"] / ns for b in B])
        hwall = stats_ms([t / ns for t in host[what]])
        row = dict(
            what="statistics_joint", config=2, name=wl.name, kernel=eng.kernel_info(), walkers=R, sites=N, cells=[n, n], shape=what,
            n_keys=n_keys, samples_per_block=ns, rows_per_block=ns * R, thin_by=thin, reps=args.reps,
            keys_with_rows=int((got.n > 0).sum()), rows_outside_keys=int(got.key_under + got.key_over),
            cells_with_rows=int((got.joint > 0).sum()), rows_outside_cells=int(got.joint_out.sum()), device_equals_numpy=same,
            field_MiB=float(got.joint.nbytes) / 2**20,
            field_launch_us_per_block=float(np.median(dev)) * 1e3, field_launch_us_per_block_range=[float(dev.min()) * 1e3, float(dev.max()) * 1e3],
            mc_kernel_ms_per_block=float(np.median(mc)), share_of_mc_kernel=float(np.median(dev / mc)),
            record_launches_us_with_field=float(np.median(own)) * 1e3, record_launches_us_without_field=float(np.median(bare)) * 1e3,
            record_launches_us_without_field_range=[float(bare.min()) * 1e3, float(bare.max()) * 1e3],
            wall_per_sample=wall, record_download=stats_ms([b["download"] for b in B]), wall_per_sample_fetch_and_bin=hwall)
        line = json.dumps(row)
        print(line, flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
