#!/usr/bin/env python3
"""Golden data for the distance objective (special quasirandom structures): the REFERENCE's compiled
ClusterSpaceEvaluator.corr_distances_from_occupancies / interaction_distances_from_occupancies
(smol/utils/cluster/evaluator.pyx:319-437), built out of tree with Cython by make_golden.build_reference_core.

Run in the build container only (needs /root/reference, Cython, gcc):

    python tests/golden/make_distance_golden.py

Cases: binary fcc {2: 7, 3: 5} in diag(4,4,4); the same model in the aliased diag(2,2,2) cell; a ternary fcc
with quadruplets {2: 6, 3: 4.5, 4: 4.2} in diag(3,3,3); the rocksalt model with two active sublattices in
diag(3,3,3).  For each: random occupancies with single and double flips, the target set to the correlations
(interactions) of an ordered occupancy that fits the cell (so that rows match it exactly and the L term is
non-zero), the distance rows of both feature modes, and the exact-match diameter L with match_weight 0 and 1.

Restated (pymatgen is absent, so ClusterSubspace.orbits_by_diameter cannot be imported):
    exact_match_max_diameter          distance.py:307-332 (correlations), :454-472 (interactions)
    orbits_by_diameter grouping       clusterspace.py:368-381 (rounded to 6 decimals, ascending)
and a reference-order Metropolis swap trajectory at kB = 1 (kernel/base.py:145-166, metropolis.py:31-49,
mcusher.py:176-200 with numpy's Generator) whose enthalpies come from corr_distances_from_occupancies.

Output: tests/golden/distance_v1.npz (data only).
"""

import os
import sys
from itertools import groupby

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402


def groups_of(model):
    """clusterspace.py:368-381: {round(diameter, 6): orbits}, ascending."""
    orbs = sorted(model.orbits, key=lambda o: np.round(o.diameter, 6))
    return [(d, list(g)) for d, g in groupby(orbs, key=lambda o: np.round(o.diameter, 6))]


def exact_match_max_diameter(groups, d, tol, corr):
    """distance.py:307-332 / :454-472."""
    L = 0.0
    for diameter, orbits in groups:
        idx = [i for o in orbits for i in (range(o.bit_id, o.bit_id + len(o.bit_combos)) if corr else [o.id])]
        if np.all(d[idx] <= tol):
            L = diameter
        else:
            break
    return L


def case(core, name, prim, cutoffs, mat, ordered, rng, out):
    from smol_amd import synth

    model = synth.build_cluster_model(prim, cutoffs)
    sc = synth.build_supercell(model, np.asarray(mat))
    ones = np.ones(model.num_corr_functions)
    proc = mg.RefProcessor(core, model, sc, ones)
    nsp = np.array([prim.nspecies[b] for b in sc.site_b])
    active = np.flatnonzero(nsp > 1)
    occ_o = ordered(sc).astype(np.int32)
    t_corr = proc.ev_corr.correlations_from_occupancy(occ_o, proc.full_cont)
    t_int = proc.ev_int.interactions_from_occupancy(occ_o, proc.full_cont)
    occ_i, occ_f = [], []
    for k in range(12):
        o = occ_o.copy() if k == 0 else (rng.random(sc.num_sites) * nsp).astype(np.int32)
        for nfl in (1, 2):
            f = o.copy()
            for s in rng.choice(active, nfl, replace=False):
                f[s] = (f[s] + 1 + rng.integers(0, nsp[s] - 1)) % nsp[s]
            occ_i.append(o)
            occ_f.append(f)
    occ_i, occ_f = np.array(occ_i, np.int32), np.array(occ_f, np.int32)
    dc = np.array([proc.ev_corr.corr_distances_from_occupancies(f, i, t_corr, proc.full_cont)
                   for i, f in zip(occ_i, occ_f)])
    di = np.array([proc.ev_int.interaction_distances_from_occupancies(f, i, t_int, proc.full_cont)
                   for i, f in zip(occ_i, occ_f)])
    gr = groups_of(model)
    tol = 1e-5
    Lc = np.array([[exact_match_max_diameter(gr, r, tol, True) for r in rows] for rows in dc])
    Li = np.array([[exact_match_max_diameter(gr, r, tol, False) for r in rows] for rows in di])
    out.update({f"{name}/occ_i": occ_i, f"{name}/occ_f": occ_f, f"{name}/target_corr": t_corr,
                f"{name}/target_int": t_int, f"{name}/dist_corr": dc, f"{name}/dist_int": di,
                f"{name}/L_corr": Lc, f"{name}/L_int": Li, f"{name}/match_tol": np.array(tol)})
    return model, sc, proc, t_corr


def trajectory(proc, sc, target, rng, out, R=4, n=300, T=0.1):
    """Reference-order Metropolis swap chain at kB = 1 on the correlation distance, match_weight 1."""
    model = proc.model
    gr = groups_of(model)
    w = np.concatenate([[-1.0], np.ones(model.num_corr_functions - 1)])
    steps = np.full((R, n, 4), -1, np.int32)
    us, acc, H = np.zeros((R, n)), np.zeros((R, n), np.uint8), np.zeros((R, n))
    occ0 = np.array([rng.permutation(np.repeat([0, 1], sc.num_sites // 2)) for _ in range(R)], np.int32)
    for r in range(R):
        occ = occ0[r].copy()
        for i in range(n):
            s1 = rng.integers(sc.num_sites)  # Swap.propose_step: site, then one of another species
            others = np.flatnonzero(occ != occ[s1])
            s2 = others[rng.integers(len(others))]
            f = occ.copy()
            f[s1], f[s2] = occ[s2], occ[s1]
            d = proc.ev_corr.corr_distances_from_occupancies(f, occ, target, proc.full_cont)
            d[0, 0] = exact_match_max_diameter(gr, d[0], 1e-5, True)
            d[1, 0] = exact_match_max_diameter(gr, d[1], 1e-5, True)
            dE = float(w @ (d[1] - d[0]))
            expo = -dE / T
            if expo >= 0:
                u, a = np.nan, True
            else:
                u = rng.random()
                a = expo > np.log(u)
            steps[r, i] = [s1, occ[s2], s2, occ[s1]]
            us[r, i], acc[r, i] = u, a
            if a:
                occ = f
            dd = proc.ev_corr.corr_distances_from_occupancies(occ, occ, target, proc.full_cont)[0]
            dd[0] = exact_match_max_diameter(gr, dd, 1e-5, True)
            H[r, i] = float(w @ dd)
    out.update({"traj/occ0": occ0, "traj/steps": steps, "traj/uniforms": us, "traj/accepted": acc,
                "traj/enthalpy": H, "traj/T": np.array(T)})


def main():
    from smol_amd import synth

    core = mg.build_reference_core()
    rng = np.random.default_rng(20261016)
    out = {}
    l10 = lambda sc: (sc.lattice_points[sc.site_t][:, 2] % 2)  # noqa: E731
    _, sc, proc, t = case(core, "binary444", synth.fcc_prim(), {2: 7.0, 3: 5.0}, np.diag([4, 4, 4]), l10, rng, out)
    trajectory(proc, sc, t, rng, out)
    case(core, "binary222", synth.fcc_prim(), {2: 7.0, 3: 5.0}, np.diag([2, 2, 2]), l10, rng, out)
    tern = lambda sc: (sc.lattice_points[sc.site_t][:, 2] % 3)  # noqa: E731
    case(core, "ternary333", synth.fcc_prim(nspecies=3), {2: 6.0, 3: 4.5, 4: 4.2}, np.diag([3, 3, 3]), tern, rng, out)
    rs = lambda sc: np.where(np.array([sc.model.prim.nspecies[b] for b in sc.site_b]) > 1,  # noqa: E731
                             sc.lattice_points[sc.site_t][:, 2] % 2, 0)
    case(core, "rocksalt333", synth.rocksalt_prim(anion_charges=(-2.0, -1.0)), {2: 4.5, 3: 3.2},
         np.diag([3, 3, 3]), rs, rng, out)
    np.savez_compressed(os.path.join(HERE, "distance_v1.npz"), **out)


if __name__ == "__main__":
    main()
