#!/usr/bin/env python3
"""A T x mu grid of a semigrand model in ONE engine handle (per-walker chemical potentials, smolmc_set_walker_mu):
composition isotherms, mu-T diagrams and hysteresis loops without one handle per chemical potential.

Every grid point (T_i, mu_j) gets `--walkers` walkers.  The chemical potential of ONE species (`--scan
sublattice:code`, or `--species NAME` on an .mson model) runs over `--mu lo:hi:n` as an offset to the model's own
table; the walkers equilibrate, then record `--samples` samples `--thin` steps apart through the device ring.  One JSON
line per grid point: T, mu, mean composition per active sublattice, acceptance.  The compositions are counted on the
device (smolmc_set_observables: one kind per active sublattice and species code); no occupancy is downloaded.

    python tools/mu_scan.py --config 3 --dim 6 --T 30000 40000 --mu=-2:2:16
    python tools/mu_scan.py --mson model.mson --supercell 6 --species Li+ --mu=-0.5:0.5:32 --T 600 900
    python tools/mu_scan.py --config 3 --T 40000 --mu=-2:2:8 --sweep up,down    # hysteresis loop

`--sweep up,down`: after the first pass every column moves one mu step per stage (up: to the next value, the last
column stays; down: back again), carrying its occupancies along; every stage prints its lines with "stage": k.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SEMIGRAND_CONFIGS = (3, 5, 9, 13)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--config", type=int, choices=SEMIGRAND_CONFIGS, help="a semigrand configuration of smol_amd.workloads")
    src.add_argument("--mson", help="a cluster expansion serialized by smol (.mson / .json[.gz])")
    ap.add_argument("--dim", type=int, default=0, help="--config: supercell size (default: the configuration's)")
    ap.add_argument("--supercell", type=int, default=4, help="--mson: n of the n x n x n supercell")
    ap.add_argument("--mu-base", default="", help="--mson: 'Li+=0.1,Ni3+=0' chemical potentials the scan is an offset to (default 0)")
    ap.add_argument("--species", default="", help="--mson: the species whose chemical potential is scanned")
    ap.add_argument("--scan", default="0:1", help="--config: sublattice:code of the scanned species (default 0:1)")
    ap.add_argument("--T", nargs="+", type=float, required=True, help="temperatures (K)")
    ap.add_argument("--mu", required=True, help="lo:hi:n offsets of the scanned chemical potential (eV); write --mu=-1:1:9 when lo is negative")
    ap.add_argument("--walkers", type=int, default=1, help="walkers per grid point")
    ap.add_argument("--equil", type=int, default=20000, help="equilibration steps per walker (each stage)")
    ap.add_argument("--samples", type=int, default=50)
    ap.add_argument("--thin", type=int, default=200)
    ap.add_argument("--sweep", default="", help="'up', 'down' or 'up,down': move every column one mu step per stage")
    ap.add_argument("--seed", type=int, default=777)
    ap.add_argument("--dry-run", action="store_true", help="print the grid and stop (no GPU)")
    a = ap.parse_args(argv)
    lo, hi, n = a.mu.split(":")
    a.mu_values = np.linspace(float(lo), float(hi), int(n))
    a.sweep_stages = [s for s in a.sweep.split(",") if s]
    if any(s not in ("up", "down") for s in a.sweep_stages):
        ap.error("--sweep takes 'up', 'down' or 'up,down'")
    if a.mson and not a.species:
        ap.error("--mson needs --species")
    return a


def grid_of(a):
    """(temperature, index of the mu value) of every walker: mu fastest, then the walkers of a point, then T."""
    nmu = len(a.mu_values)
    T = np.repeat(np.asarray(a.T, dtype=float), nmu * a.walkers)
    j = np.tile(np.repeat(np.arange(nmu), a.walkers), len(a.T))
    return T, j


def stages_of(a):
    """Per stage the index into mu_values of every column: the first pass, then one step per sweep stage."""
    nmu = len(a.mu_values)
    col = np.arange(nmu)
    out = [col.copy()]
    for s in a.sweep_stages:
        for _ in range(nmu - 1):
            col = np.minimum(col + 1, nmu - 1) if s == "up" else np.maximum(col - 1, 0)
            out.append(col.copy())
    return out


def build(a, R):
    """tables, step type, start occupancies, the handle's own rows (n_sublattices, W) and the scanned (sublattice, code)."""
    from smol_amd import capi, workloads

    if a.config:
        kw = dict(count=R)
        if a.dim:
            kw["dim"] = a.dim
        wl = workloads.BUILDERS[a.config](**kw)
        k, code = (int(x) for x in a.scan.split(":"))
        return wl.tables, wl.config_kwargs["step"], wl.occupancy, (k, code)
    from smol_amd import moca, mson

    ce = mson.load_mson(a.mson)
    ens = moca.Ensemble.from_mson(ce, np.diag([a.supercell] * 3))
    base = {sp: 0.0 for sp in ens.species}
    for item in filter(None, a.mu_base.split(",")):
        name, val = item.split("=")
        base[name] = float(val)
    ens.chemical_potentials = base
    hit = [(k, int(s.encoding[list(map(str, s.species)).index(a.species)])) for k, s in enumerate(ens.active_sublattices)
           if a.species in map(str, s.species)]
    if not hit:
        raise SystemExit(f"--species {a.species}: not on an active sublattice (species: {[str(s) for s in ens.species]})")
    rng = np.random.default_rng(a.seed)
    occ = np.zeros((R, ens.num_sites), dtype=np.int32)
    for s in ens.sublattices:
        occ[:, s.sites] = rng.choice(s.encoding, size=(R, len(s.sites)))
    return ens.make_tables(), capi.STEP_FLIP, occ, hit[0]


def composition_observables(tables, width):
    """Kind = active sublattice q x ``width`` + species code on the sites of the active sublattices, no bond shells: the
    species counts of every walker in the layout of its chemical-potential rows."""
    from smol_amd.observables import Observables

    sites = tables.active_sites()
    kind_base = np.full(tables.struct.num_sites, -1, dtype=np.int32)
    for q, st in enumerate(sites):
        kind_base[st] = q * width
    return Observables(kind_base, len(sites) * width)


def main(argv=None):
    a = parse_args(argv)
    T, j = grid_of(a)
    R = len(T)
    stages = stages_of(a)
    if a.dry_run:
        print(json.dumps(dict(walkers=R, temperatures=list(map(float, a.T)), mu=a.mu_values.tolist(), stages=len(stages))))
        return
    from smol_amd import capi
    from smol_amd.engine import Engine

    tables, step, occ, (k, code) = build(a, R)
    eng = Engine(tables, capi.make_config(R, capi.KERNEL_METROPOLIS, step))
    base = eng.get_walker_mu()
    sites = tables.active_sites()
    eng.set_observables(composition_observables(tables, base.shape[2]))
    seeds = np.arange(R, dtype=np.uint64) + np.uint64(a.seed)
    for stage, col in enumerate(stages):
        rows = base.copy()
        rows[:, k, code] += a.mu_values[col[j]]
        eng.set_walker_mu(rows)
        if stage == 0:
            eng.set_state(occ, seeds, T)
        eng.run(a.equil)
        s0 = eng.get_state(occupancy=False)
        smp = eng.run_sampled(a.samples, a.thin, occupancy=False, observables=True)
        s1 = eng.get_state(occupancy=False)
        acc = (s1["n_accepted"] - s0["n_accepted"]) / float(a.samples * a.thin)
        n = smp["species_counts"].sum(axis=0).reshape(R, len(sites), base.shape[2])  # (R, sublattices, codes) over the samples
        comp = [n[:, q, :] / float(a.samples * len(st)) for q, st in enumerate(sites)]
        npt = len(a.mu_values)
        for p in range(len(a.T) * npt):
            w = slice(p * a.walkers, (p + 1) * a.walkers)
            print(json.dumps(dict(stage=stage, T=float(T[w][0]), mu=float(a.mu_values[col[p % npt]]),
                                  composition=[c[w].mean(axis=0).round(6).tolist() for c in comp],
                                  acceptance=float(acc[w].mean()), kernel=eng.kernel_info() if p == 0 else None)), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
