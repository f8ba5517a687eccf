"""The small model of the replica-exchange Wang-Landau statistics tests (tests/test_wl_windows_host.py on the CPU
oracle, tests/test_gpu_wl_windows.py on the device): a 16-site fcc cell at 8 / 8 whose 12870 states are enumerated
exactly, 24 global bins, three windows of 12 bins at a stride of 6, two copies."""

import functools
import itertools

import numpy as np

from smol_amd import capi, parallel, synth

CELL = [2, 2, 4]
N_BINS, N_WINDOWS, COPIES = 24, 3, 2
CHECK_PERIOD, ROUNDS, STEPS = 500, 400, 500

# The bound on the RMS deviation of a joined ln g from the log of the exact counts (over the occupied bins, after
# removing the mean difference): 3 x the largest RMS of PLAIN single-window Wang-Landau walkers on the same oracle,
# same 200 000 steps per walker, same check period -- four walkers for each of the seeds 5, 6, 7 (twelve in all).
# Measured on the CPU oracle (tests/wl_windows_case.py: single_window_rms):
#   seed 5: 0.0682 0.0449 0.0519 0.0280    seed 6: 0.0583 0.0499 0.0629 0.0476    seed 7: 0.0452 0.0398 0.0674 0.0470
#   largest 0.0682 -> bound 0.2046
# The joined copies of the replica-exchange runs on the oracle (seeds 5, 6, 7): see test_wl_windows_host.py.
# ln g spans 1.4 .. 7.6 over the occupied bins: a join without the shifts, or a wrong sign in the exchange exponent,
# misses by order 1.
RMS_BOUND = 3 * 0.0682


@functools.lru_cache(maxsize=None)
def case():
    """dict(sc, coefs, tab, N, E (12870,), states (12870, N) int32, lo, hi, bin, exact_counts (24,), occupied (24,) bool)."""
    from oracle import oracle as orc

    model = synth.build_cluster_model(synth.fcc_prim(), {2: 6.0, 3: 5.0})
    sc = synth.build_supercell(model, CELL)
    coefs = synth.random_coefs(model, seed=11, scale=0.05)
    tab = capi.TableSet.from_synth(sc, coefs)
    N = sc.num_sites
    rows = [c for c in itertools.combinations(range(N), N // 2)]
    states = np.zeros((len(rows), N), dtype=np.int32)
    states[np.arange(len(rows))[:, None], np.asarray(rows)] = 1
    ev = orc.OracleEvaluator(tab)
    nat = ev.natural_parameters()
    E = np.array([ev.feature_vector(o) @ nat for o in states])
    lo, hi = float(E.min() - 1e-3), float(E.max() + 1e-3)
    bin_size = (hi - lo) / N_BINS * (1.0 + 1e-12)  # (24 bins by the ceil rule, whatever the division rounds to)
    counts = np.bincount(np.clip(np.floor_divide(E - lo, bin_size).astype(int), 0, N_BINS - 1), minlength=N_BINS)
    return dict(sc=sc, coefs=coefs, tab=tab, N=N, E=E, states=states, lo=lo, hi=hi, bin=bin_size, exact_counts=counts, occupied=counts > 0)


def windows(seed):
    c = case()
    wx = parallel.WLWindows(c["lo"], c["hi"], c["bin"], N_WINDOWS, overlap=0.5, copies=COPIES, seed=seed)
    assert (wx.L, wx.Lw, wx.Ls) == (N_BINS, 12, 6)
    return wx


def config(R, vmin, vmax):
    return capi.make_config(R, capi.KERNEL_WANGLANDAU, capi.STEP_SWAP, min_enthalpy=float(vmin), max_enthalpy=float(vmax),
                            bin_size=case()["bin"], check_period=CHECK_PERIOD)


def start_occupancies(wx, seed):
    """One state inside every estimator's window, drawn from the enumeration (the middle third of the window)."""
    c = case()
    rng = np.random.default_rng(1000 + seed)
    out = np.zeros((wx.R, c["N"]), dtype=np.int32)
    for e in range(wx.R):
        third = (wx.vmax[e] - wx.vmin[e]) / 3.0
        inside = np.flatnonzero((c["E"] >= wx.vmin[e] + third) & (c["E"] < wx.vmax[e] - third))
        out[e] = c["states"][rng.choice(inside)]
    return out


def rms_vs_exact(ln_g, visited=None):
    """RMS of ln g - log(exact counts) over the occupied bins after removing the mean difference."""
    c = case()
    m = c["occupied"] if visited is None else (c["occupied"] & visited)
    d = ln_g[m] - np.log(c["exact_counts"][m])
    return float(np.sqrt(np.mean((d - d.mean()) ** 2)))


def single_window_rms(seed, walkers=4):
    """Plain Wang-Landau on the oracle over the global window: the RMS of every walker (the yardstick of RMS_BOUND)."""
    from oracle import oracle as orc

    c = case()
    ora = orc.OracleMC(c["tab"], config(walkers, c["lo"], c["hi"]))
    rng = np.random.default_rng(1000 + seed)
    ora.set_state(c["states"][rng.choice(len(c["states"]), walkers)], np.arange(walkers, dtype=np.uint64) + np.uint64(100 * seed), 0.0)
    ora.run(ROUNDS * STEPS)
    S = ora.get_wl()["entropy"]
    return [rms_vs_exact(S[r], S[r] > 0) for r in range(walkers)]
