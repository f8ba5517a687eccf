#!/usr/bin/env python3
"""Ground states of every composition from ONE semigrand anneal: the walkers of one handle are spread over a grid of
chemical potentials (smolmc_set_walker_mu), annealed down a temperature ladder, and every recorded sample is offered to a
minima record keyed by composition (smolmc_set_minima: the count of the scanned species selects the slot, the ENERGY --
the enthalpy without the chemical work -- is minimised).  Nothing but the record is ever downloaded: no occupancy column,
no observables column.  Prints one JSON line per filled composition (x, energy, formation energy against the end members,
on_hull, the offer and walker that found it) and one summary line with the vertices of the lower convex hull.

    python tools/ground_state_search.py --config 3 --dim 6 --mu=-2:2:64 --T 40000 20000 10000 5000 2000
    python tools/ground_state_search.py --mson model.mson --supercell 4 --species Li+ --mu=-0.5:0.5:64 --T 1500 800 300 --out-npz gs.npz
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def parse_args(argv=None):
    import mu_scan

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--config", type=int, choices=mu_scan.SEMIGRAND_CONFIGS, help="a semigrand configuration of smol_amd.workloads")
    src.add_argument("--mson", help="a cluster expansion serialized by smol (.mson / .json[.gz])")
    ap.add_argument("--dim", type=int, default=0, help="--config: supercell size (default: the configuration's)")
    ap.add_argument("--supercell", type=int, default=4, help="--mson: n of the n x n x n supercell")
    ap.add_argument("--mu-base", default="", help="--mson: chemical potentials the grid is an offset to (default 0)")
    ap.add_argument("--species", default="", help="--mson: the species whose count is the composition axis")
    ap.add_argument("--scan", default="0:1", help="--config: sublattice:code of that species (default 0:1)")
    ap.add_argument("--T", nargs="+", type=float, required=True, help="the temperature ladder, highest first (K)")
    ap.add_argument("--mu", required=True, help="lo:hi:n offsets of the scanned chemical potential (eV); write --mu=-1:1:9 when lo is negative")
    ap.add_argument("--walkers", type=int, default=1, help="walkers per chemical potential")
    ap.add_argument("--samples", type=int, default=64, help="samples per temperature")
    ap.add_argument("--thin", type=int, default=0, help="steps between samples (default: one sweep)")
    ap.add_argument("--seed", type=int, default=777)
    ap.add_argument("--out-npz", default="", help="write the record's arrays here")
    a = ap.parse_args(argv)
    lo, hi, n = a.mu.split(":")
    a.mu_values = np.linspace(float(lo), float(hi), int(n))
    return a


def main(argv=None):
    import mu_scan
    from smol_amd import capi
    from smol_amd.engine import Engine
    from smol_amd.minima import Minima, formation_energies, lower_hull

    a = parse_args(argv)
    R = len(a.mu_values) * a.walkers
    tables, step, occ, (k, code) = mu_scan.build(a, R)
    eng = Engine(tables, capi.make_config(R, capi.KERNEL_METROPOLIS, step))
    base = eng.get_walker_mu()
    W = base.shape[2]
    sites = tables.active_sites()
    obs = mu_scan.composition_observables(tables, W)
    eng.set_observables(obs)
    n_sub = len(sites[k])
    nat = eng.natural_parameters
    eng.set_minima(Minima.by_composition(obs, [k * W + code], extents=[n_sub + 1], weights=nat[:-1]))  # (all but the chemical work)
    rows = base.copy()
    rows[:, k, code] += np.repeat(a.mu_values, a.walkers)
    eng.set_walker_mu(rows)
    eng.set_state(occ, np.arange(R, dtype=np.uint64) + np.uint64(a.seed), a.T[0])
    thin = a.thin or eng.N
    for T in a.T:
        eng.set_temperature(T)
        eng.run_sampled_async(a.samples, thin, occupancy=False, minima=True)
        eng.fetch_samples()
    rec = eng.minima()
    slots = np.flatnonzero(rec.filled)
    x = slots / float(n_sub)
    ef = formation_energies(x, rec.value[slots])
    hull = lower_hull(x, ef)
    for i, s in enumerate(slots):
        print(json.dumps(dict(n=int(s), x=float(x[i]), energy=float(rec.value[s]), formation_energy=float(ef[i]),
                              on_hull=bool(i in set(hull.tolist())), offer=int(rec.sample[s]), walker=int(rec.walker[s]),
                              step=int(rec.step[s]))), flush=True)
    print(json.dumps(dict(kernel=eng.kernel_info(), walkers=R, sites=int(eng.N), sublattice_sites=int(n_sub), offers=int(len(a.T) * a.samples),
                          compositions_filled=int(len(slots)), of=int(n_sub + 1), hull=[float(v) for v in x[hull]])))
    if a.out_npz:
        np.savez_compressed(a.out_npz, slots=slots, **{f: getattr(rec, f)[slots] for f in ("value", "enthalpy", "features", "occupancy",
                                                                                            "counts", "walker", "sample", "step")})
    eng.close()


if __name__ == "__main__":
    main()
