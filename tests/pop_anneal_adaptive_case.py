"""The adaptive schedule on the model of tests/pop_anneal_case.py (the 16-site fcc cell, 4 populations of 256 walkers, 160
swap steps per temperature, seeds 5, 6, 7): from 3000 K to 300 K with a target overlap of 0.85 and 16 bisections per step,
instead of the 15 steps of the fixed geometric ladder.  tests/test_pop_anneal_adaptive_host.py runs it on the CPU oracle,
tests/test_gpu_pop_anneal_adaptive.py on the device."""

import numpy as np

from smol_amd import parallel
from tests import pop_anneal_case as pc
from tests import wl_windows_case as wc

T_START, T_END = 3000.0, 300.0
OVERLAP, N_ITER = 0.85, 16
FIXED_STEPS = len(pc.TEMPERATURES) - 1  # 15: what the adaptive schedule has to beat

# The bounds: 3 x the largest |error| of the scheme on the CPU ORACLE, seeds 5, 6, 7 with four populations each (twelve
# estimates; run_annealing(oracle, seed, host_decide=True), measured by oracle_errors below).  Every seed took 6 steps:
#   seed 5: 3000 1857.2 991.8 648.8 466.5 325.5 300 K
#   seed 6: 3000 1949.3 992.8 646.9 463.1 338.2 300 K
#   seed 7: 3000 2174.6 1093.5 709.0 511.0 367.9 300 K
#   sum ln Q - 4.18461
#     seed 5: +0.0257 +0.0046 -0.0299 -0.0245
#     seed 6: +0.0624 +0.0072 -0.0116 +0.0528
#     seed 7: -0.0914 -0.0264 +0.0352 -0.0569
#     largest 0.0914 -> bound 0.2742
#   final mean enthalpy + 0.153544
#     seed 5: +0.00193 +0.00034 +0.00066 -0.00092
#     seed 6: +0.00352 +0.00034 +0.00352 -0.00029
#     seed 7: -0.00029 +0.00003 +0.00161 -0.00219
#     largest 0.00352 -> bound 0.01056
# (The fixed ladder of pop_anneal_case.py: 0.0972 and 0.00410.)
LNZ_BOUND = 3 * 0.0914
EMEAN_BOUND = 3 * 0.00352


def schedule(seed):
    return parallel.PopulationAnnealing.adaptive(T_START, T_END, OVERLAP, populations=pc.POPULATIONS, seed=seed, n_iter=N_ITER)


def run_annealing(engine, seed, host_decide, history=None):
    """The scheme on ``engine`` (an Engine or an OracleMC of WALKERS * POPULATIONS walkers): returns (pa, final mean
    enthalpy per population)."""
    R = pc.WALKERS * pc.POPULATIONS
    pa = schedule(seed)
    engine.set_state(pc.start_occupancies(seed, R), pc.walker_seeds(seed, R), T_START)
    parallel.run_population_annealing(engine, pa, pc.STEPS, host_decide=host_decide, history=history)
    return pa, engine.get_state()["enthalpy"].reshape(pc.POPULATIONS, pc.WALKERS).mean(axis=1)


def oracle_errors(seed):
    """(pa, sum ln Q - exact (P,), final mean enthalpy - exact (P,), parent maps) of the scheme on the CPU oracle."""
    from oracle import oracle as orc

    ora = orc.OracleMC(wc.case()["tab"], pc.config(pc.WALKERS * pc.POPULATIONS))
    history = []
    pa, emean = run_annealing(ora, seed, host_decide=True, history=history)
    return pa, pa.log_partition_ratio() - pc.LNZ_EXACT, emean - pc.EMEAN_EXACT, history


def chain_enthalpies(model, R, steps=300):
    """The enthalpies of R walkers of a model of tests/test_gpu_pop_anneal.py after ``steps`` steps on the CPU oracle: the
    same chains as the device's, on which the cases of the device tests are chosen."""
    from oracle import oracle as orc

    ora = orc.OracleMC(model.tables, model.config(R))
    occ, seeds = model.starts(R)
    ora.set_state(occ, seeds, model.T)
    ora.run(steps)
    return np.array(ora.get_state()["enthalpy"])
