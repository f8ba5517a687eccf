#!/usr/bin/env python3
"""What the site field of a statistics record costs, one JSON line per shape into
profiles/statistics_sites_timing.jsonl:

  shapes   config 2 (the headline: R = 4096 walkers of N = 4096 sites, 16-sample blocks = 65536 rows), all sites tracked,
           two codes, with the record keyed
             walker    by walker: one owner per counter, no atomics
             bins256   by 256 bins of the enthalpy over the range the equilibrated walkers span: neighbouring rows
                       in different keys, an atomic per row and site
             one       by one bin that takes every row: long runs of one key, few atomics
  blocks   --samples samples per block, one sample per sweep; --reps blocks per arm, the arms alternating block by
           block; --warmup rounds first
  arms     field     the block with the record and its field, occupancies left on the device: the device time of the
                     field's launch (HIP events) and the wall time
           host      the path the field replaces: the ring with the occupancies (uint8), the fetch, then the one-hot sums
                     per key in NumPy

  device time of the field's launch per block, its share of the block's MC kernel time, wall time per sample of both
  arms, the time of one download of the record (a run needs one, at its end), the field's memory, and whether the device
  field of one more block equals the NumPy sums.

python tools/statistics_sites_timing.py [--samples 16] [--reps 5] [--replicas R] [--dim D] [--out ...]"""
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


def host_field(spec, smp, n_keys, S):
    """site_counts (n_keys, N, S) of a fetched block: the rows sorted by key, one sum per key and code."""
    H = smp["enthalpy"]
    ns, R = H.shape
    occ = smp["occupancy"].reshape(ns * R, -1)
    if spec.binned:
        q = st.bin_of(H.reshape(-1), spec.key_min, spec.key_bin)
        ok = np.isfinite(q) & (q >= 0) & (q < n_keys)
        keys = np.where(ok, np.nan_to_num(q, nan=0.0, posinf=0.0, neginf=0.0), -1).astype(np.int64)
    else:
        keys = np.tile(np.arange(R), ns)
    order = np.argsort(keys, kind="stable")
    order = order[keys[order] >= 0]
    out = np.zeros((n_keys, occ.shape[1], S), dtype=np.int64)
    if not len(order):
        return out
    sk = keys[order]
    starts = np.flatnonzero(np.r_[True, sk[1:] != sk[:-1]])
    rows = occ[order]
    for c in range(S):
        out[sk[starts], :, c] = np.add.reduceat(rows == c, starts, axis=0, dtype=np.int64)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--replicas", type=int, default=0, help="walkers (default: the configuration's)")
    ap.add_argument("--dim", type=int, default=0, help="supercell size of config 2 (default: the configuration's)")
    ap.add_argument("--samples", type=int, default=16, help="samples per block")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "statistics_sites_timing.jsonl"))
    args = ap.parse_args()
    kw = dict(count=args.replicas) if args.replicas else {}
    if args.dim:
        kw["dim"] = args.dim
    wl = workloads.BUILDERS[2](**kw)
    eng = Engine(wl.tables, wl.make_config())
    eng.set_state(wl.occupancy, wl.seeds, wl.temperature)
    eng.run(20 * eng.N, sync=True)
    H0 = eng.get_state(occupancy=False)["enthalpy"]
    lo, hi = float(H0.min()), float(H0.max())
    span = max(hi - lo, 1e-6)
    R, N, ns, S = eng.R, eng.N, args.samples, 2
    thin = N  # one sweep
    field = dict(sites=None, site_codes=S)
    shapes = {
        "walker": Statistics.per_walker([st.ENTHALPY], **field),
        "bins256": Statistics.by_bin(st.ENTHALPY, 256, lo - 0.5 * span, 2.0 * span / 256, **field),
        "one": Statistics.by_bin(st.ENTHALPY, 1, lo - 1e3 * span, 2e3 * span, **field),
    }
    arms = {what: [] for what in shapes}
    host = {what: [] for what in shapes}
    for i in range(args.warmup + args.reps):
        keep = i >= args.warmup
        for what, spec in shapes.items():
            eng.set_statistics(spec)
            t0 = time.perf_counter()
            eng.run_sampled_async(ns, thin, occupancy=False, statistics=True)
            eng.fetch_samples()
            t1 = time.perf_counter()
            rec = eng.statistics()  # (a run downloads the record once, at its end)
            t2 = time.perf_counter()
            if keep:
                arms[what].append(dict(wall=t1 - t0, download=t2 - t1, mc_ms=eng.last_kernel_ms(),
                                       sites_ms=eng.statistics_sites_kernel_ms()))
            del rec
            eng.set_statistics(None)
            t0 = time.perf_counter()
            eng.run_sampled_async(ns, thin, occupancy=True)
            host_field(spec, eng.fetch_samples(packed=True), spec.n_keys if spec.binned else R, S)
            t1 = time.perf_counter()
            if keep:
                host[what].append(t1 - t0)
    for what, spec in shapes.items():
        n_keys = spec.n_keys if spec.binned else R
        eng.set_statistics(spec)  # one more block, its occupancies fetched: the device field against the NumPy sums
        smp = eng.run_sampled(ns, thin, occupancy=True, packed=True, statistics=True)
        got = eng.statistics()
        same = bool(np.array_equal(got.site_counts, host_field(spec, smp, n_keys, S)) and not got.site_over.any()
                    and np.array_equal(got.site_counts.sum(axis=(1, 2)), N * got.n))
        B = arms[what]
        dev, mc = (np.array([b[f] for b in B]) for f in ("sites_ms", "mc_ms"))
        wall = stats_ms([b["wall"] / ns for b in B])
        hwall = stats_ms([t / ns for t in host[what]])
        row = dict(
            what="statistics_sites", config=2, name=wl.name, kernel=eng.kernel_info(), walkers=R, sites=N, codes=S, shape=what,
            n_keys=n_keys, samples_per_block=ns, rows_per_block=ns * R, thin_by=thin, reps=args.reps,
            keys_with_rows=int((got.n > 0).sum()), rows_outside=int(got.key_under + got.key_over), device_equals_numpy=same,
            field_bytes=int(got.site_counts.nbytes + got.site_over.nbytes), field_MiB=float(got.site_counts.nbytes) / 2**20,
            field_launch_us_per_block=float(np.median(dev)) * 1e3, field_launch_us_per_sample=float(np.median(dev)) * 1e3 / ns,
            field_launch_us_per_block_range=[float(dev.min()) * 1e3, float(dev.max()) * 1e3],
            mc_kernel_ms_per_block=float(np.median(mc)), share_of_mc_kernel=float(np.median(dev / mc)),
            wall_per_sample=wall, record_download=stats_ms([b["download"] for b in B]), wall_per_sample_fetch_and_sum=hwall,
            fetch_and_sum_over_field=hwall["median_ms"] / wall["median_ms"])
        line = json.dumps(row)
        print(line, flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
