"""The small model of the population-annealing statistics tests (tests/test_pop_anneal_host.py on the CPU oracle,
tests/test_gpu_pop_anneal.py on the device): the 16-site fcc cell of tests/wl_windows_case.py, whose 12870 states are
enumerated exactly, cooled from 3000 K to 300 K in 15 resampling steps, 256 walkers per population, 160 swap steps
per temperature, start states drawn from the exact Boltzmann distribution at 3000 K."""

import functools

import numpy as np

from smol_amd import capi, parallel
from tests import wl_windows_case as wc

TEMPERATURES = np.geomspace(3000.0, 300.0, 16)
WALKERS, POPULATIONS, STEPS = 256, 4, 160
SEEDS = (5, 6, 7)

# Exact values from the enumeration (exact()): ln Z(300 K) - ln Z(3000 K) and <E>(300 K).
LNZ_EXACT, EMEAN_EXACT = 4.18461, -0.153544

# The bounds: 3 x the largest |error| of the scheme on the CPU ORACLE, seeds 5, 6, 7 with four populations each (twelve
# estimates; run_annealing(oracle, seed, host_decide=True), measured by tests/pop_anneal_case.py: oracle_errors):
#   sum ln Q - 4.18461
#     seed 5: -0.0384 +0.0270 -0.0066 +0.0032
#     seed 6: -0.0245 +0.0197 -0.0972 -0.0365
#     seed 7: -0.0170 -0.0534 +0.0552 -0.0333
#     largest 0.0972 -> bound 0.2916
#   final mean enthalpy + 0.153544
#     seed 5: -0.00124 +0.00130 +0.00161 +0.00003
#     seed 6: +0.00257 -0.00410 -0.00092 -0.00092
#     seed 7: +0.00193 +0.00130 -0.00061 +0.00066
#     largest 0.00410 -> bound 0.01230
# The signal is 4.18: a wrong sign of db or a dropped -db * H_ref misses by order 4 - 5.
LNZ_BOUND = 3 * 0.0972
EMEAN_BOUND = 3 * 0.00410


@functools.lru_cache(maxsize=None)
def exact():
    """(ln Z(T_K) - ln Z(T_0), <E>(T_K)) from the enumeration."""
    E = wc.case()["E"]
    b0, b1 = 1.0 / (parallel.kB * TEMPERATURES[0]), 1.0 / (parallel.kB * TEMPERATURES[-1])
    e0 = E.min()
    z0, z1 = np.exp(-b0 * (E - e0)), np.exp(-b1 * (E - e0))
    return float(np.log(z1.sum()) - np.log(z0.sum()) - (b1 - b0) * e0), float((E * z1).sum() / z1.sum())


def config(R):
    return capi.make_config(R, capi.KERNEL_METROPOLIS, capi.STEP_SWAP)


def start_occupancies(seed, R):
    """R states drawn from the exact Boltzmann distribution at TEMPERATURES[0]."""
    c = wc.case()
    w = np.exp(-(c["E"] - c["E"].min()) / (parallel.kB * TEMPERATURES[0]))
    rng = np.random.default_rng(2000 + seed)
    return c["states"][rng.choice(len(w), size=R, p=w / w.sum())]


def walker_seeds(seed, R):
    return np.arange(R, dtype=np.uint64) + np.uint64(1000 * seed + 1)


def run_annealing(engine, seed, host_decide, history=None):
    """The scheme on ``engine`` (an Engine or an OracleMC of WALKERS * POPULATIONS walkers): returns (pa, final mean
    enthalpy per population)."""
    R = WALKERS * POPULATIONS
    pa = parallel.PopulationAnnealing(TEMPERATURES, populations=POPULATIONS, seed=seed)
    engine.set_state(start_occupancies(seed, R), walker_seeds(seed, R), TEMPERATURES[0])
    parallel.run_population_annealing(engine, pa, STEPS, host_decide=host_decide, history=history)
    return pa, engine.get_state()["enthalpy"].reshape(POPULATIONS, WALKERS).mean(axis=1)


def oracle_errors(seed):
    """(sum ln Q - exact (P,), final mean enthalpy - exact (P,), parent maps) of the scheme on the CPU oracle."""
    from oracle import oracle as orc

    ora = orc.OracleMC(wc.case()["tab"], config(WALKERS * POPULATIONS))
    history = []
    pa, emean = run_annealing(ora, seed, host_decide=True, history=history)
    return pa.log_partition_ratio() - LNZ_EXACT, emean - EMEAN_EXACT, history
