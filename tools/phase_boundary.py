#!/usr/bin/env python3
"""A phase boundary mu_coex(T) from ONE semigrand mu-T grid and nothing but its statistics record.

The 256-site binary fcc model of the golden case ``fcc_conv444_pairs`` runs on a grid of temperatures x chemical
potentials in one engine handle (per-walker chemical potentials, one walker per state point) with replica exchange across
the grid on the device (``Engine.exchange_grid``).  The handle keeps a statistics record keyed by STATE POINT with a JOINT
FIELD: H_k(E, N), the energy (the weighted sum of the features with weight 0 on the chemical work: ``statistics.ENERGY``,
not the enthalpy) against the count of species 1.  A pilot record (moments only) places the energy axis; then every sample
is offered on the device, the blocks are discarded unread, and the record is the only download.

From the record:
  ln g(E, N)   ``record.wham_joint(betas, fields)``: the state points joined by the multiple-histogram method
  mu_coex(T)   ``record.coexistence(ln_g, beta, bracket, split)``: the chemical potential at which P(N) has equal weight
               below and above half filling, at every temperature of the grid and between them
  the jump     the plain isotherm <N>(mu) of the grid's own state points: the middle of the two neighbouring chemical
               potentials between which <N> crosses half filling, and those two values -- what a grid of isolated state points
               gives, no finer than its spacing
One table, then one JSON line.

python tools/phase_boundary.py [--temperatures 1500,2000,2500] [--mu=-0.4:0.4:12] [--exchanges 200] [--samples 8]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from smol_amd import capi, parallel  # noqa: E402
from smol_amd import statistics as st  # noqa: E402
from smol_amd.engine import Engine  # noqa: E402
from smol_amd.observables import Observables  # noqa: E402
from smol_amd.statistics import KB, Statistics  # noqa: E402
from tests.cases import load_case, tables_for  # noqa: E402

CASE = "fcc_conv444_pairs"


def offer_blocks(eng, gx, n_exchanges, samples, thin, attempt):
    """``n_exchanges`` rounds of one block offered on the device and discarded unread, then one exchange attempt."""
    for _ in range(n_exchanges):
        eng.run_sampled_async(samples, thin, occupancy=False, statistics=True)
        eng.discard_samples()
        pairs = gx.pairs(gx.move_of(attempt))
        if len(pairs):
            eng.exchange_grid(pairs, gx.log_u(attempt, len(pairs)))
        attempt += 1
    return attempt


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--temperatures", default="1500,2000,2500", help="in K")
    ap.add_argument("--mu", default="-0.4:0.4:12", help="lo:hi:n chemical potentials of species 1 (eV); write --mu=-1:1:9 when lo is negative")
    ap.add_argument("--exchanges", type=int, default=200, help="measuring rounds: one block, then one exchange attempt")
    ap.add_argument("--equilibrate", type=int, default=50, help="rounds before the record is emptied")
    ap.add_argument("--samples", type=int, default=8, help="samples per block, one sweep apart")
    ap.add_argument("--energy-cells", type=int, default=128)
    ap.add_argument("--between", type=int, default=1, help="temperatures between two of the grid at which mu_coex is printed as well")
    ap.add_argument("--seed", type=int, default=5)
    args = ap.parse_args()
    temps = np.array([float(x) for x in args.temperatures.split(",")])
    lo, hi, n = args.mu.split(":")
    mus = np.linspace(float(lo), float(hi), int(n))

    sc = load_case(CASE)["sc"]
    Ns, nsp = sc.num_sites, max(sc.model.prim.nspecies)
    tab = tables_for(CASE, capi.FEATURES_INTERACTIONS, mu_table=np.zeros((Ns, nsp)))
    R = len(temps) * len(mus)
    eng = Engine(tab, capi.make_config(R, capi.KERNEL_METROPOLIS, capi.STEP_FLIP))
    obs = Observables.from_supercell(sc, tables=tab)
    eng.set_observables(obs)
    rows = np.zeros((len(mus),) + tuple(eng._mu_shape()[1:]))
    rows[:, 0, 1] = mus
    gx = parallel.GridExchange(temps, rows, seed=args.seed)
    rng = np.random.default_rng(args.seed)
    occ = (rng.random((R, Ns)) < 0.5).astype(np.int32)
    eng.set_walker_mu(gx.point_rows)  # (state point p is walker p from here on; the exchanges move the walkers)
    eng.set_state(occ, np.arange(R, dtype=np.uint64) + np.uint64(args.seed), gx.point_temperatures)
    weights = eng.natural_parameters[:-1]  # (weight 0 on the last feature, the chemical work)
    cols = [st.ENERGY, st.kind(obs, 1)]

    # the pilot: moments only, to place the energy axis
    eng.set_statistics(Statistics.by_state_point(cols, weights=weights))
    attempt = offer_blocks(eng, gx, args.equilibrate, args.samples, Ns, 0)
    eng.reset_statistics()
    attempt = offer_blocks(eng, gx, args.equilibrate, args.samples, Ns, attempt)
    pilot = eng.statistics()
    mean, sd = pilot.mean()[:, 0], np.sqrt(pilot.variance()[:, 0])
    e_lo, e_hi = float((mean - 6.0 * sd).min()), float((mean + 6.0 * sd).max())
    joint = ((st.ENERGY, args.energy_cells, e_lo, (e_hi - e_lo) / args.energy_cells), (st.kind(obs, 1), Ns + 1, -0.5, 1.0))

    # the measurement: nothing but the record comes back
    eng.set_statistics(Statistics.by_state_point(cols, weights=weights, joint=joint))
    attempt = offer_blocks(eng, gx, args.exchanges, args.samples, Ns, attempt)
    rec = eng.statistics()
    eng.close()
    assert (rec.joint.sum(axis=(1, 2)) + rec.joint_out == rec.n).all() and (rec.n == args.exchanges * args.samples).all()
    betas, fields = 1.0 / (KB * gx.point_temperatures), gx.point_rows[:, 0, 1]
    ln_g, f = rec.wham_joint(betas, fields, tol=1e-9, max_iter=50000)

    n_mean = rec.mean()[:, 1].reshape(len(temps), len(mus))  # the plain isotherms, state point by state point
    split = Ns // 2
    out = []
    listed = []
    for i, T in enumerate(temps):
        listed.append((float(T), i))
        if i + 1 < len(temps):
            listed += [(float(T + (temps[i + 1] - T) * (j + 1) / (args.between + 1)), None) for j in range(args.between)]
    print(f"# {Ns} sites, {len(temps)} x {len(mus)} state points, {args.exchanges} x {args.samples} samples each, "
          f"{int(rec.joint_out.sum())} of {int(rec.n.sum())} rows outside the cells")
    print("      T / K   mu_coex / eV   <N> there   the isotherm crosses half filling between")
    for T, i in listed:
        beta = 1.0 / (KB * T)
        try:
            mu_coex = rec.coexistence(ln_g, beta, (float(mus[0]), float(mus[-1])), split, tol=1e-9)
            n_there = float(rec.from_ln_g(ln_g, beta, mu_coex)[0][1])
        except ValueError:
            mu_coex, n_there = float("nan"), float("nan")
        jump = None
        if i is not None:
            above = np.flatnonzero(n_mean[i] >= split)
            if len(above) and above[0] > 0:
                jump = [float(mus[above[0] - 1]), float(mus[above[0]])]
        out.append(dict(T=T, mu_coex=mu_coex, mean_count_at_mu_coex=n_there, isotherm_crossing=jump))
        tail = "(between the grid's temperatures)" if i is None else "not inside the grid" if jump is None else \
            f"{jump[0]:.4f} and {jump[1]:.4f}: {0.5 * (jump[0] + jump[1]):.4f}"
        print(f"{T:11.1f} {mu_coex:14.5f} {n_there:11.2f}   {tail}")
    print(json.dumps(dict(what="phase_boundary", case=CASE, sites=Ns, temperatures=temps.tolist(), mu=mus.tolist(),
                          exchanges=args.exchanges, samples=args.samples, rows_outside=int(rec.joint_out.sum()),
                          exchange_attempts=attempt, rows=out)))


if __name__ == "__main__":
    main()
