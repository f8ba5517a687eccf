#!/usr/bin/env python3
"""Short-range order against temperature from ONE Wang-Landau run.

A small binary fcc alloy at 50 / 50 (the headline Hamiltonian, ``workloads.config2``, on dim^3 primitive cells) is walked
by Wang-Landau walkers over an enthalpy window found by two short Metropolis runs.  The handle keeps a statistics record
keyed by the Wang-Landau levels (``Statistics.on_wl_levels``): per level the mean enthalpy, the four species patterns
A-A, A-B, B-A, B-B on the nearest-neighbour pairs (a pattern spec: pair counts per level) and the two kind counts.  Every
sample is offered on the device; the blocks are discarded unread, and the record and ln g are the only downloads.

Printed per temperature: the Warren-Cowley parameter of the first shell, alpha = 1 - P(AB) / (2 c_A c_B), from
``record.canonical(ln g, T)``, and the heat capacity per site from ``record.canonical_heat_capacity(ln g, T)``; one JSON
line at the end.  alpha < 0 is ordering, alpha > 0 clustering, 0 the random alloy.

python tools/wl_order_parameter.py [--dim 4] [--walkers 64] [--levels 64] [--sweeps 4000] [--temperatures 300,...]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from smol_amd import capi, workloads  # noqa: E402
from smol_amd import statistics as st  # noqa: E402
from smol_amd.engine import Engine  # noqa: E402
from smol_amd.observables import Observables  # noqa: E402
from smol_amd.patterns import Patterns  # noqa: E402
from smol_amd.statistics import Statistics  # noqa: E402


def enthalpy_window(wl, n_levels):
    """(min, bin) of a window from the coldest and the hottest enthalpies two short Metropolis runs reach."""
    eng = Engine(wl.tables, wl.make_config())
    N = eng.N
    seen = []
    for T in (50000.0, 200.0):
        eng.set_state(wl.occupancy, wl.seeds, T)
        eng.run(200 * N, sync=True)
        seen.append(eng.get_state(occupancy=False)["enthalpy"])
    cold = eng.get_state()["occupancy"]
    eng.close()
    lo, hi = float(np.min(seen)), float(np.max(seen))
    pad = 0.02 * (hi - lo)
    lo, hi = lo - pad, hi + pad
    return lo, (hi - lo) / n_levels * (1.0 + 1e-12), cold


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dim", type=int, default=4, help="primitive cells along each axis (4: 64 sites)")
    ap.add_argument("--walkers", type=int, default=64)
    ap.add_argument("--levels", type=int, default=64, help="Wang-Landau levels = keys of the record")
    ap.add_argument("--sweeps", type=int, default=4000, help="sweeps per walker, one sample each")
    ap.add_argument("--temperatures", default="300,600,1000,1500,2500,5000,20000", help="in K")
    args = ap.parse_args()

    wl = workloads.config2(count=args.walkers, dim=args.dim)
    sc, N, W, L = wl.sc, wl.sc.num_sites, args.walkers, args.levels
    lo, bin_size, cold = enthalpy_window(wl, L)
    cfg = capi.make_config(W, capi.KERNEL_WANGLANDAU, capi.STEP_SWAP, min_enthalpy=lo, max_enthalpy=lo + L * bin_size / (1.0 + 1e-12),
                           bin_size=bin_size, check_period=10 * N, flatness=0.8)
    eng = Engine(wl.tables, cfg)
    assert eng.L == L, (eng.L, L)
    # half of the walkers start hot (random), half from the cold end, all inside the window
    occ = wl.occupancy.copy()
    occ[W // 2:] = cold[W // 2:]
    eng.set_state(occ, wl.seeds, 0.0)
    kinds = Observables.from_supercell(sc, tables=wl.tables)
    obs = Observables(kinds.kind_base, kinds.n_kinds, site_ncodes=kinds.site_ncodes)  # (no shells: the kinds alone)
    pairs = next(np.asarray(rows, dtype=np.int32) for orb, rows in zip(sc.model.orbits, sc.full_indices) if orb.size == 2)
    pat = Patterns.from_tuples(obs, [pairs], classes="kind")  # the nearest-neighbour pairs: cells AA, AB, BA, BB
    eng.set_observables(obs)
    eng.set_patterns(pat)
    cells = [pat.cell(0, (a, b)) for a in range(2) for b in range(2)]
    cols = [st.ENTHALPY] + [st.pattern(c) for c in cells] + [st.kind(obs, 0), st.kind(obs, 1)]
    eng.set_statistics(Statistics.on_wl_levels(lo, bin_size, L, columns=cols))
    left = args.sweeps
    while left > 0:  # blocks of samples offered on the device and discarded unread
        ns = min(left, 64)
        eng.run_sampled_async(ns, N, occupancy=False, statistics=True)
        eng.discard_samples()
        left -= ns
    rec = eng.statistics()
    wlz = eng.get_wl()
    S = wlz["entropy"]
    seen = S > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        ln_g = np.where(seen.any(axis=0), np.where(seen, S, 0.0).sum(axis=0) / seen.sum(axis=0), np.nan)
    print(f"# {N} sites, {W} walkers, {args.sweeps} sweeps each; {int((rec.n > 0).sum())} of {L} levels hold samples, "
          f"{rec.key_under + rec.key_over} rows outside; modification factor {wlz['mod_factor'].min():.3g} .. {wlz['mod_factor'].max():.3g}")
    temps = np.array([float(x) for x in args.temperatures.split(",")])
    mean = rec.canonical(ln_g, temps)                # (nT, C)
    heat = rec.canonical_heat_capacity(ln_g, temps)  # (nT,) in eV / K
    n_pairs = mean[:, 1:5].sum(axis=1)
    p_ab = (mean[:, 2] + mean[:, 3]) / n_pairs
    c_a, c_b = mean[:, 5] / N, mean[:, 6] / N
    alpha = 1.0 - p_ab / (2.0 * c_a * c_b)
    print("      T / K    <H> / eV     alpha_1    C / (N kB)")
    for i, T in enumerate(temps):
        print(f"{T:11.1f} {mean[i, 0]:11.5f} {alpha[i]:11.5f} {heat[i] / (N * st.KB):13.5f}")
    print(json.dumps(dict(what="wl_order_parameter", sites=N, walkers=W, levels=L, sweeps=args.sweeps, temperatures=temps.tolist(),
                          mean_enthalpy=mean[:, 0].tolist(), warren_cowley_1=alpha.tolist(),
                          heat_capacity_per_site_kB=(heat / (N * st.KB)).tolist(), levels_with_samples=int((rec.n > 0).sum()))))
    eng.close()


if __name__ == "__main__":
    main()
