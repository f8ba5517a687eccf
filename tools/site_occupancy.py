#!/usr/bin/env python3
"""Which sublattice orders, without naming the ordering beforehand.

The small binary fcc alloy of tools/wl_order_parameter.py (``workloads.config2`` on dim^3 primitive cells, 50 / 50) is
cooled through its ordering transition by canonical swap walkers, every walker on its own.  The handle keeps a statistics
record per walker with a SITE FIELD on all sites (``Statistics.per_walker(..., sites=None, site_codes=2)``): how often every
site held every species.  At each temperature the walkers equilibrate, the record is emptied, and every sample of the
measuring sweeps is offered on the device; the blocks are discarded unread and the record is the only download.

Printed per temperature, as the mean over the walkers (with the smallest and the largest walker for the first):
  frozen    ``record.frozen_order()``: mean_m sum_s p_m(s)^2 less the same for the walker's composition; 0 while a walker's
            sites are alike, 1 - sum x^2 = 0.5 here when it sits in one ordering variant
  B-rich    the share of the sites with p_m(B) > 1/2 -- the sublattice found by thresholding the field -- and the mean
            p(B) on those sites and on the others (``record.sublattice_occupancy``)
One JSON line at the end.

python tools/site_occupancy.py [--dim 4] [--walkers 64] [--sweeps 400] [--equilibrate 200] [--temperatures 3000,...]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from smol_amd import workloads  # noqa: E402
from smol_amd import statistics as st  # noqa: E402
from smol_amd.engine import Engine  # noqa: E402
from smol_amd.statistics import Statistics  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dim", type=int, default=4, help="primitive cells along each axis (4: 64 sites)")
    ap.add_argument("--walkers", type=int, default=64)
    ap.add_argument("--sweeps", type=int, default=400, help="measuring sweeps per temperature, one sample each")
    ap.add_argument("--equilibrate", type=int, default=200, help="sweeps at every temperature before the record is emptied")
    ap.add_argument("--temperatures", default="3000,2000,1500,1200,1000,800,600,400,300,200", help="in K, in the order of the run")
    args = ap.parse_args()

    wl = workloads.config2(count=args.walkers, dim=args.dim)
    eng = Engine(wl.tables, wl.make_config())
    N, W = eng.N, args.walkers
    temps = [float(x) for x in args.temperatures.split(",")]
    eng.set_state(wl.occupancy, wl.seeds, temps[0])
    eng.set_statistics(Statistics.per_walker([st.ENTHALPY], sites=None, site_codes=2))
    rows = []
    print(f"# {N} sites, {W} walkers, {args.equilibrate} + {args.sweeps} sweeps per temperature")
    print("      T / K   <H> / eV    frozen (min .. max)         B-rich share   p(B) there   p(B) elsewhere")
    for T in temps:
        eng.set_temperature(T)
        eng.run(args.equilibrate * N)
        eng.reset_statistics()
        left = args.sweeps
        while left > 0:  # blocks of samples offered on the device and discarded unread
            ns = min(left, 64)
            eng.run_sampled_async(ns, N, occupancy=False, statistics=True)
            eng.discard_samples()
            left -= ns
        rec = eng.statistics()
        assert (rec.n == args.sweeps).all() and (rec.site_counts.sum(axis=(1, 2)) == N * rec.n).all()
        frozen = rec.frozen_order()
        p_b = rec.site_occupancy()[:, :, 1]  # (W, N)
        rich = p_b > 0.5
        share = rich.mean(axis=1)
        there, elsewhere = np.full(W, np.nan), np.full(W, np.nan)
        for w in range(W):  # the classes differ from walker to walker: each found its own variant
            classes = [np.flatnonzero(rich[w]), np.flatnonzero(~rich[w])]
            if all(len(c) for c in classes):
                sub = rec.sublattice_occupancy(classes)[w]  # (2 classes, 2 codes)
                there[w], elsewhere[w] = sub[0, 1], sub[1, 1]
        row = dict(T=T, mean_enthalpy=float(rec.mean()[:, 0].mean()), frozen_order=float(frozen.mean()),
                   frozen_order_range=[float(frozen.min()), float(frozen.max())], b_rich_share=float(share.mean()),
                   p_b_on_b_rich=float(np.nanmean(there)), p_b_elsewhere=float(np.nanmean(elsewhere)))
        rows.append(row)
        print(f"{T:11.1f} {row['mean_enthalpy']:10.4f} {row['frozen_order']:9.4f} ({frozen.min():.4f} .. {frozen.max():.4f})"
              f" {row['b_rich_share']:14.4f} {row['p_b_on_b_rich']:12.4f} {row['p_b_elsewhere']:16.4f}")
    print(json.dumps(dict(what="site_occupancy", sites=N, walkers=W, sweeps=args.sweeps, equilibrate=args.equilibrate, rows=rows)))
    eng.close()


if __name__ == "__main__":
    main()
