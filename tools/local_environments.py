#!/usr/bin/env python3
"""Like nearest neighbours of an annealed binary fcc alloy, measured on the device.

The alloy is the headline workload (``workloads.config2``: binary fcc, point + 4 pair + 2 triplet orbits, canonical swaps).
Its environment spec has every site as a centre with its 12 nearest neighbours, centre and neighbour classes the two
species: cell (a, n_0, n_1) counts the sites of species a with n_0 neighbours of species 0 and n_1 of species 1.  The handle
is cooled through --temperatures; at each one it equilibrates, empties its statistics record and feeds it on the device
from every sample.  The record's columns are the 2 x 13 cells with n_0 + n_1 = 12 and the two kind counts; the occupancies
never leave the device, and the record is the only download.  Printed per temperature and species: the share of its sites
with n = 0 .. 12 LIKE neighbours next to the share in a random alloy of the same composition
(``Environments.random_alloy``: binomial in the species' own concentration).  Ordering shows as weight moved to few like
neighbours, clustering as weight moved to many.

python tools/local_environments.py [--dim 16] [--walkers 16] [--temperatures 4000,2500,1500,1000] [--samples 32]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from smol_amd import statistics as st  # noqa: E402
from smol_amd import workloads  # noqa: E402
from smol_amd.engine import Engine  # noqa: E402
from smol_amd.environments import Environments  # noqa: E402
from smol_amd.observables import Observables  # noqa: E402
from smol_amd.statistics import Statistics  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dim", type=int, default=16, help="primitive cells along each axis (16: 4096 sites)")
    ap.add_argument("--walkers", type=int, default=16)
    ap.add_argument("--temperatures", default="4000,2500,1500,1000", help="the cooling schedule, in K")
    ap.add_argument("--samples", type=int, default=32, help="samples per walker and temperature, one per sweep")
    ap.add_argument("--equilibrate", type=int, default=50, help="sweeps at a temperature before its first sample")
    args = ap.parse_args()

    wl = workloads.config2(count=args.walkers, dim=args.dim)
    sc, N, W = wl.sc, wl.sc.num_sites, args.walkers
    eng = Engine(wl.tables, wl.make_config())
    eng.set_state(wl.occupancy, wl.seeds, wl.temperature)
    kinds = Observables.from_supercell(sc, tables=wl.tables)
    obs = Observables(kinds.kind_base, kinds.n_kinds, site_ncodes=kinds.site_ncodes)  # (no shells: the kinds alone)
    spec = next(s for s in (Environments.from_supercell(sc, obs, orbits=[i]) for i in kinds.shell_orbit_ids) if s.sets[0].width == 12)
    z = spec.sets[0].width
    eng.set_observables(obs)
    eng.set_environments(spec)
    like = [[spec.cell(0, a, (n, z - n) if a == 0 else (z - n, n)) for n in range(z + 1)] for a in range(2)]
    record = Statistics.per_walker([st.environment(c) for row in like for c in row] + [st.kind(obs, 0), st.kind(obs, 1)])
    eng.set_statistics(record)
    print(f"# {N} sites, {W} walkers, {args.samples} samples per walker and temperature; the record is the only download")
    for T in [float(x) for x in args.temperatures.split(",")]:
        eng.set_temperature(T)
        eng.run(args.equilibrate * N, sync=True)
        eng.reset_statistics()
        left = args.samples
        while left > 0:
            ns = min(left, 16)
            eng.run_sampled(ns, N, occupancy=False, statistics=True)
            left -= ns
        mean = eng.statistics().mean().mean(axis=0)  # (columns,) over the walkers
        counts = mean[-2:]
        alloy = spec.random_alloy(counts, 0)
        print(f"T = {T:g} K, composition {counts[0] / counts.sum():.4f} / {counts[1] / counts.sum():.4f}")
        print("   n like   " + "  ".join(f"species {a}: sampled  random" for a in range(2)))
        out = dict(what="local_environments", sites=N, temperature=T, walkers=W, samples=args.samples, sampled=[], random=[])
        rows = []
        for a in range(2):
            got = mean[a * (z + 1):(a + 1) * (z + 1)] / counts[a]
            want = np.array([alloy[(a, n, z - n) if a == 0 else (a, z - n, n)] for n in range(z + 1)]) / counts[a]
            rows.append((got, want))
            out["sampled"].append(got.tolist())
            out["random"].append(want.tolist())
        for n in range(z + 1):
            print(f"   {n:6d}   " + "  ".join(f"           {got[n]:7.4f} {want[n]:7.4f}" for got, want in rows))
        print(json.dumps(out), file=sys.stderr)
    eng.close()


if __name__ == "__main__":
    main()
