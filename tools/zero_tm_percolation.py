#!/usr/bin/env python3
"""0-TM percolation of a disordered rocksalt, measured on the device.

The cation lattice of a rocksalt is fcc: ``synth.fcc_prim`` with two species, Li (code 0) and a transition metal (code 1).
A Li ion hops between two neighbouring octahedral sites through a tetrahedral site; the hop is fast when the two other
cations on that tetrahedron are Li too -- the 0-TM channel of Urban, Lee and Ceder (Adv. Energy Mater. 4, 1400478).  So the
graph is: members Li, bonds the nearest neighbours, every bond gated by its two tetrahedra, ``max_blocked = 0`` (or 1 with
--max-blocked 1: 0-TM or 1-TM).

One handle holds --walkers walkers per state point: a composition scan (--fractions, the Li share of the cation sites, kept by
the canonical swaps) or, with --temperatures, a temperature scan at the one composition of --fractions.  A statistics
record with the columns connectivity(0, WRAPPING_SITES), connectivity(0, N_MEMBERS) and connectivity(0, WRAP_AXES) and a
histogram of the axis mask is fed on the device from every sample; the occupancies never leave it, and the record is the
only download.  Printed per state point: the percolation strength <wrapping sites> / <members> and the probability that a
component wraps the cell.  With a random alloy (high temperature) the 0-TM threshold of the infinite lattice lies near a Li
share of 0.55.

python tools/zero_tm_percolation.py [--dim 16] [--fractions 0.40,...,0.70] [--temperatures T1,T2,...] [--samples 64]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from smol_amd import capi, synth  # noqa: E402
from smol_amd import connectivity as cn  # noqa: E402
from smol_amd import statistics as st  # noqa: E402
from smol_amd.connectivity import Connectivity  # noqa: E402
from smol_amd.engine import Engine  # noqa: E402
from smol_amd.statistics import Statistics  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dim", type=int, default=16, help="primitive cells along each axis (16: 4096 cation sites)")
    ap.add_argument("--fractions", default="0.40,0.45,0.50,0.55,0.60,0.65,0.70", help="Li share of the cation sites")
    ap.add_argument("--temperatures", default=None, help="a temperature scan at the first of --fractions instead")
    ap.add_argument("--temperature", type=float, default=5000.0, help="of a composition scan (high: a nearly random alloy)")
    ap.add_argument("--walkers", type=int, default=16, help="walkers per state point")
    ap.add_argument("--samples", type=int, default=64, help="samples per walker, one per sweep")
    ap.add_argument("--equilibrate", type=int, default=20, help="sweeps before the first sample")
    ap.add_argument("--max-blocked", type=int, default=0, help="transition metals a channel may have (0: 0-TM)")
    ap.add_argument("--scale", type=float, default=0.002, help="scale of the random pair interactions")
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()

    a = 4.2
    model = synth.build_cluster_model(synth.fcc_prim(a=a), {2: a + 0.01})
    sc = synth.build_supercell(model, [args.dim] * 3)
    tab = capi.TableSet.from_synth(sc, synth.random_coefs(model, seed=args.seed, scale=args.scale), feature_mode=capi.FEATURES_INTERACTIONS)
    N = sc.num_sites
    fractions = [float(x) for x in args.fractions.split(",")]
    if args.temperatures:
        temps = [float(x) for x in args.temperatures.split(",")]
        points = [(fractions[0], t) for t in temps]
    else:
        points = [(x, args.temperature) for x in fractions]
    W = args.walkers
    R = W * len(points)
    rng = np.random.default_rng(args.seed)
    occ = np.ones((R, N), dtype=np.int32)
    for r in range(R):  # exactly round(x N) Li (code 0) in every row of the point
        occ[r, rng.permutation(N)[: int(round(points[r // W][0] * N))]] = 0
    eng = Engine(tab, capi.make_config(R, capi.KERNEL_METROPOLIS, capi.STEP_SWAP))
    eng.set_state(occ, np.arange(R, dtype=np.uint64) + np.uint64(args.seed), np.repeat([t for _, t in points], W))
    spec = Connectivity.from_supercell(sc, [dict(members=[0], cutoff=a / np.sqrt(2.0) + 0.01,
                                                 gate=dict(kinds=[0], corners=2, max_blocked=args.max_blocked))])
    eng.set_connectivity(spec)
    axes = st.connectivity(0, cn.WRAP_AXES)
    record = Statistics.per_walker([st.connectivity(0, cn.WRAPPING_SITES), st.connectivity(0, cn.N_MEMBERS), axes], n_levels=4,
                                   hist=(axes, 8, 0.0, 1.0))
    eng.set_statistics(record)
    eng.run(args.equilibrate * N, sync=True)
    left = args.samples
    while left > 0:  # nothing but the record comes back
        ns = min(left, 16)
        eng.run_sampled(ns, N, occupancy=False, statistics=True)
        left -= ns
    rec = eng.statistics()
    mean = rec.mean()
    print(f"# {N} cation sites, {spec.graphs[0].bonds.shape[0]} channel rows, max_blocked = {args.max_blocked}, "
          f"{W} walkers x {args.samples} samples per point; kernel {eng.connectivity_kernel_ms():.3f} ms for the last block")
    print("#  x_Li  temperature  percolation_strength  wrapping_probability")
    for p, (x, t) in enumerate(points):
        rows = slice(p * W, (p + 1) * W)
        strength = mean[rows, 0].sum() / mean[rows, 1].sum()
        wrapping = 1.0 - rec.hist[rows, 0].sum() / rec.n[rows].sum()
        print(f"  {x:5.3f}  {t:11.1f}  {strength:20.4f}  {wrapping:20.4f}")
        print(json.dumps(dict(what="zero_tm_percolation", sites=N, x_li=x, temperature=t, max_blocked=args.max_blocked,
                              percolation_strength=float(strength), wrapping_probability=float(wrapping), samples=int(rec.n[rows].sum()))),
              file=sys.stderr)
    eng.close()


if __name__ == "__main__":
    main()
