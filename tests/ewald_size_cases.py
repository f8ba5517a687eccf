"""Chains on rocksalt cells chosen for the GROUP COUNT of their Ewald potential field (tests/test_gpu_ewald_sizes.py on the
device, tests/test_ewald_sizes_host.py on the oracle alone).  The field sweeps of smolmc_common.h switch code on the number
of changeable sites na = 64 groups + tail; every cell here puts a call site of the kernels on one side of such a switch.

All cases: synth.rocksalt_prim() with pair cutoff 4.5 and ewald_coef = 0.2, 3 walkers, launches of 1, 40 and 160 steps;
Metropolis at T = 2e5 K, where most steps are accepted (each accepted step is one sweep)."""

import functools
from collections import namedtuple

import numpy as np

from smol_amd import capi, ewald, synth

R = 3
CHUNKS = (1, 40, 160)
NSTEPS = sum(CHUNKS)
MIN_ACCEPTED = 60   # per walker: fewer and the sweeps barely ran
TEMPERATURE = 2.0e5
FLIP_TABLE = np.array([[1, -3, 2]])  # the cation table of tests/test_gpu_table_flip.py: 3 Mn3+ <-> 1 Li+ + 2 Ti4+

# dims -> (changeable sites, full groups, tail); two: the anion sublattice is active too (O2- / F-)
Cell = namedtuple("Cell", "dims two na groups tail")
CELLS = {
    "4x9x10": Cell((4, 9, 10), False, 360, 5, 40),
    "8x8x10": Cell((8, 8, 10), False, 640, 10, 0),
    "11x12x13": Cell((11, 12, 13), False, 1716, 26, 52),
    "8x14x16": Cell((8, 14, 16), False, 1792, 28, 0),
    "9x14x15": Cell((9, 14, 15), False, 1890, 29, 34),
    "8x8x15-two": Cell((8, 8, 15), True, 1920, 30, 0),
    "8x8x16-two": Cell((8, 8, 16), True, 2048, 32, 0),
    "8x8x8-two": Cell((8, 8, 8), True, 1024, 16, 0),
    "7x8x9-two": Cell((7, 8, 9), True, 1008, 15, 48),
}

# name, cell, step, kernel ("metropolis" / "wang-landau"), environment switches, words kernel_info must start with / hold /
# must not hold, and the sweep branch the case is there for
Case = namedtuple("Case", "name cell step kernel env starts has hasnot branch")
NOGX, GEN = {"SMOLMC_NO_EWALD_GX": "1"}, {"SMOLMC_FORCE_GENERAL": "1"}
HBM, LDS = {"SMOLMC_MULTI_PHI_HBM": "1"}, {"SMOLMC_MULTI_PHI_LDS": "1"}
FLIP, SWAP, TABLE = capi.STEP_FLIP, capi.STEP_SWAP, capi.STEP_TABLE_FLIP


def _c(name, cell, step, branch, kernel="metropolis", env=None, starts="lean ", has=("field=1", "gx="), hasnot=()):
    return Case(name, cell, step, kernel, dict(env or {}), starts, tuple(has), tuple(hasnot), branch)


CASES = [
    _c("360-flip", "4x9x10", FLIP, "gx_small<1,4>: 5 groups + 40, two rounds of four slots, masked lanes"),
    _c("360-swap", "4x9x10", SWAP, "gx_small<2,4>: the same for two flips"),
    _c("360-table", "4x9x10", TABLE, "gx_sized<3,9,4> below its first batch: group by group + ragged tail (swap steps: gx_small<2,4>)"),
    _c("640-swap-rows", "8x8x10", SWAP, "field_sweep<true> (U = 14) below its first batch: batches of 4, 4, 1, 1",
       env=NOGX, has=("field=1",), hasnot=("gx=",)),
    _c("1716-flip", "11x12x13", FLIP, "last size below the 27-batch: gx_sized<1,9,4>, two batches + shifted nine-batch + tail"),
    _c("1792-flip", "8x14x16", FLIP, "gx_pre27 + its tail call: the shifted 27-batch (26 groups rewritten)"),
    _c("1792-swap", "8x14x16", SWAP, "gx_sized<2,9,4>: three batches + shifted batch in one chunk"),
    _c("1792-table", "8x14x16", TABLE, "gx_sized<3,9,4>: three batches, then one group alone (no shifted batch for three flips)"),
    _c("1792-flip-rows", "8x14x16", FLIP, "field_sweep<false> (U = 9): three batches + shifted batch", env=NOGX,
       has=("field=1",), hasnot=("gx=",)),
    _c("1792-swap-rows", "8x14x16", SWAP, "field_sweep<true> (U = 14): two batches, no remainder", env=NOGX,
       has=("field=1",), hasnot=("gx=",)),
    _c("1792-flip-general", "8x14x16", FLIP, "field_sweep<false,6>: four batches + shifted batch", env=GEN, starts="general",
       has=(), hasnot=("field=0", "gx=")),
    _c("1792-swap-general", "8x14x16", SWAP, "field_sweep<true,4>: seven batches", env=GEN, starts="general", has=(),
       hasnot=("field=0", "gx=")),
    _c("1890-flip", "9x14x15", FLIP, "gx_pre27 + tail call: shifted 27-batch (25 rewritten) and ragged tail of 34"),
    _c("1920-flip-hbm", "8x8x15-two", FLIP, "field in HBM, pending list OFF (na < 2048): gx_multi<1,0> per accepted flip",
       env=HBM, starts="lean-multi", has=("field=2", "gx=")),
    _c("1920-swap-hbm", "8x8x15-two", SWAP, "field in HBM, pending list OFF: gx_multi<2,0> per accepted swap", env=HBM,
       starts="lean-multi", has=("field=2", "gx=")),
    _c("2048-flip-hbm", "8x8x16-two", FLIP, "pending list ON: gx_multi<4,-1> flushes, launches end on a partly filled list",
       env=HBM, starts="lean-multi", has=("field=2", "gx=")),
    _c("2048-swap-hbm", "8x8x16-two", SWAP, "pending list ON: gx_multi<4,0> flushes, launches end on a partly filled list",
       env=HBM, starts="lean-multi", has=("field=2", "gx=")),
    _c("1024-flip-wl", "8x8x8-two", FLIP, "gx_groups<1,16>: all 16 groups from registers (Wang-Landau, field in LDS)",
       kernel="wang-landau", env=LDS, starts="lean-multi", has=("field=1", "gx=", "wl=multi")),
    _c("1024-swap-wl", "8x8x8-two", SWAP, "gx_groups<2,16>", kernel="wang-landau", env=LDS, starts="lean-multi",
       has=("field=1", "gx=", "wl=multi")),
    _c("1008-flip-wl", "7x8x9-two", FLIP, "the neighbour that does NOT take the register sweep: gx_multi<1,1>, 15 groups + 48",
       kernel="wang-landau", env=LDS, starts="lean-multi", has=("field=1", "gx=", "wl=multi")),
    _c("1008-swap-wl", "7x8x9-two", SWAP, "... gx_multi<2,1>", kernel="wang-landau", env=LDS, starts="lean-multi",
       has=("field=1", "gx=", "wl=multi")),
]
CASE_IDS = [c.name for c in CASES]
DISPATCH_ENV = ("SMOLMC_FORCE_GENERAL", "SMOLMC_FORCE_UNIVERSAL", "SMOLMC_NO_EWALD_GX", "SMOLMC_NO_EWALD_FIELD",
                "SMOLMC_DENSE_EWALD", "SMOLMC_MULTI_PHI_HBM", "SMOLMC_MULTI_PHI_LDS", "SMOLMC_NO_LEAN_MULTI", "SMOLMC_NO_WL_MULTI",
                "SMOLMC_NO_SITE_RELABEL", "SMOLMC_LAUNCH_CHUNK")


@functools.lru_cache(maxsize=None)
def cell_tables(cell_name):
    """(supercell, coefficients, Ewald tables) of a cell: built once per process (the Ewald matrix of 8x14x16 takes seconds)."""
    cell = CELLS[cell_name]
    prim = synth.rocksalt_prim(anion_charges=(-2.0, -1.0)) if cell.two else synth.rocksalt_prim()
    model = synth.build_cluster_model(prim, {2: 4.5})
    sc = synth.build_supercell(model, list(cell.dims))
    return sc, synth.random_coefs(model, seed=3), ewald.supercell_ewald(sc)


@functools.lru_cache(maxsize=None)
def table_set(cell_name, table_flip):
    sc, coefs, ew = cell_tables(cell_name)
    kw = dict(flip_table=FLIP_TABLE, swap_weight=0.2) if table_flip else {}
    return capi.TableSet.from_synth(sc, coefs, ewald=ew, ewald_coef=0.2, **kw)


def changeable_sites(sc):
    prim = sc.model.prim
    return int(sum(prim.nspecies[b] > 1 for b in sc.site_b))


def start_state(case):
    """(occupancies, seeds) of the case's three walkers: random species, or charge neutral for the TableFlip cases."""
    sc = cell_tables(case.cell)[0]
    rng = np.random.default_rng(sum(CELLS[case.cell].dims) + 17 * CASE_IDS.index(case.name))
    if case.step == TABLE:
        P = sc.size  # cations 0 .. P-1 against fixed O2-: 2 n_Mn + 3 n_Ti = P
        occ = np.zeros((R, sc.num_sites), dtype=np.int32)
        for r in range(R):
            n_ti = 2 * (P // 18 + r)
            n_mn = (P - 3 * n_ti) // 2
            assert 2 * n_mn + 3 * n_ti == P
            perm = rng.permutation(P)
            occ[r, perm[:n_mn]] = 1
            occ[r, perm[n_mn:n_mn + n_ti]] = 2
    else:
        nsp = np.array([sc.model.prim.nspecies[b] for b in sc.site_b])
        occ = (rng.random((R, sc.num_sites)) * nsp).astype(np.int32)
    seeds = rng.integers(1, 2 ** 62, size=R).astype(np.uint64)
    return occ, seeds


def config(case, tab, occ):
    if case.kernel == "metropolis":
        return capi.make_config(R, capi.KERNEL_METROPOLIS, case.step), TEMPERATURE
    # window and bins of tests/test_gpu_wl_multi.py::test_two_sublattices_with_ewald
    from oracle import oracle as orc

    ev = orc.OracleEvaluator(tab)
    h = np.array([ev.feature_vector(o) @ ev.natural_parameters() for o in occ])
    cfg = capi.make_config(R, capi.KERNEL_WANGLANDAU, case.step, min_enthalpy=float(h.min() - 3.371),
                           max_enthalpy=float(h.max() + 2.193), bin_size=0.0517, check_period=50, update_period=1, flatness=0.2)
    return cfg, 0.0


def setup(case):
    """(tables, config, occupancies, seeds, temperature) of a case."""
    tab = table_set(case.cell, case.step == TABLE)
    occ, seeds = start_state(case)
    cfg, temp = config(case, tab, occ)
    return tab, cfg, occ, seeds, temp
