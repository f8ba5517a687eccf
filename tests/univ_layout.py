"""The LDS layout of the universal kernel (mc_univ.h), restated in plain Python, and the cases that reach each of its
switches (tests/test_univ_layout_host.py on the rules alone, tests/test_gpu_univ_layout.py on the device).

engine.hip chooses the layout per handle (univ_pack_records: which dictionaries fit; univ_lds_layout: everything else) and
univ.hip the instantiation (smolmc_univ_selector).  ``layout`` below is written from those rules, not from the code:

* shadow copies of the step's feature cells: ``cells`` = Fce rounded up to even (none for Fce > 1024), each
  ``1 << dshift`` times with the largest dshift <= 3 that keeps ``cells << dshift`` <= 512;
* accepted-step cells: F rounded up to even while there are feature cells;
* per-wave scratch: 128 B (TableFlip: 2464 B) + 8 B per cell; the occupancy (Npad bytes) follows it, rounded to 16;
* dictionaries in LDS (12 800 B per workgroup): <= 64 distinct records, <= 1024 tensor entries, F <= 128;
* occupancy in LDS: scratch + occupancy <= 160 KiB - 256 and no SMOLMC_UNIV_OCC_HBM; where it fits a CU's 160 KiB alone
  but not behind the dictionaries, the dictionaries go (the window fallback) -- the request never exceeds 163 840 B;
* waves per workgroup: 4, halved while the workgroup exceeds 64 KiB;
* crowded launches (more than 3072 walkers) of four-wave workgroups above 40 KiB: dshift is lowered step by step, then the
  dictionaries are dropped;
* K1 (every record has one function), TABLE (TableFlip handle) and dense (more than 8 walkers per CU) pick the instantiation."""

import collections
import functools

import numpy as np

DICT_RECS, DICT_TENS, DICT_NAT = 64, 1024, 128
DICT_BYTES = DICT_RECS * 56 + DICT_TENS * 8 + DICT_NAT * 8  # 12 800
SCRATCH, SCRATCH_TABLE = 128, 2464
CU_LDS = 160 * 1024
OCC_LDS_MAX = CU_LDS - 256     # scratch + occupancy of one wave
WORKGROUP_MAX = 64 * 1024      # more than one wave per workgroup
CROWDED_R, CROWDED_BYTES = 12 * 256, 40 * 1024
CUS = 256                      # compute units of an MI355X


class Layout(collections.namedtuple(
        "Layout", "dfeat_cells dshift acc_cells occ_lds occ_off lds_per_wave wpb dict lds_shared total k1 table R dict_off crowded")):
    """dict_off: the reasons the dictionaries are not in LDS (subset of records / tensors / features / crowding / window);
    crowded: 'no' (not a crowded launch, or nothing to shrink), 'shift' (dshift lowered, dictionaries kept), 'drop'
    (dshift 0 and the dictionaries dropped); occ_off: offset of the occupancy inside the workgroup's LDS (wave 0)."""

    def dense(self, cus=CUS):
        return int(self.R > 2 * 4 * cus)

    def words(self, cus=CUS):
        """The words smolmc_kernel_info prints after lds=."""
        cells = f"dshift={self.dshift}" if self.dfeat_cells else "dcells=0"
        return f"lds={self.total} wpb={self.wpb} {cells} dict={self.dict} k1={self.k1} table={self.table} dense={self.dense(cus)}"

    def symbol(self, cus=CUS):
        b = lambda x: "true" if x else "false"
        return (f"void mc_univ_kernel<{b(self.occ_lds)}, {b(self.k1)}, {b(self.table)}, {4 if self.dense(cus) else 2}, {b(self.dict)}>"
                "(UParams, int)")


def layout(Fce, F, Npad, R, table, n_recs, tens_len, occ_hbm_env=False, all_k1=True):
    cells = (Fce + 1) // 2 * 2 if Fce <= 1024 else 0
    acc = (F + 1) // 2 * 2 if cells else 0
    dshift = 0
    while cells and dshift < 3 and cells << (dshift + 1) <= 512:
        dshift += 1
    off = [why for why, bad in (("records", n_recs > DICT_RECS), ("tensors", tens_len > DICT_TENS), ("features", F > DICT_NAT)) if bad]
    dicts = not off

    def lay_out():
        nonlocal dicts
        scratch = (SCRATCH_TABLE if table else SCRATCH) + ((cells << dshift) + acc) * 8
        with_occ = (scratch + Npad + 15) // 16 * 16
        occ_lds = with_occ <= OCC_LDS_MAX and not occ_hbm_env
        per_wave = with_occ if occ_lds else scratch
        if occ_lds and dicts and DICT_BYTES + with_occ > CU_LDS:  # the occupancy fits a CU alone, not behind the dictionaries
            dicts = False
            off.append("window")
        shared = DICT_BYTES if dicts else 0
        wpb = 4
        while wpb > 1 and shared + per_wave * wpb > WORKGROUP_MAX:
            wpb //= 2
        return scratch, occ_lds, per_wave, shared, wpb

    scratch, occ_lds, per_wave, shared, wpb = lay_out()
    crowded = "no"
    too_big = lambda: R > CROWDED_R and wpb == 4 and shared + per_wave * 4 > CROWDED_BYTES
    while too_big() and dshift > 0:
        dshift -= 1
        crowded = "shift"
        scratch, occ_lds, per_wave, shared, wpb = lay_out()
    if too_big() and dicts:
        dicts = False
        off.append("crowding")
        crowded = "drop"
        scratch, occ_lds, per_wave, shared, wpb = lay_out()
    return Layout(cells, dshift, acc, int(occ_lds), shared + scratch, per_wave, wpb, int(dicts), shared, shared + per_wave * wpb,
                  int(bool(all_k1)), int(bool(table)), R, tuple(off), crowded)


def info_words(info):
    """The layout words of a universal handle's kernel_info(), as ``Layout.words`` spells them ('' for an older text)."""
    head = info.split(" (")[0]
    at = head.find(" lds=")
    return head[at + 1:] if at >= 0 and " wpb=" in head else ""


def args_of(tab, R, table=None, occ_hbm_env=False):
    """The arguments of ``layout`` from a capi.TableSet: feature counts, the distinct records of the enthalpy pass (equal
    in strides, functions, tensor, feature, scale and natural parameter: per orbit everything but the scale is fixed, and
    the features of two orbits differ), the tensor entries they reach and whether every record has one function."""
    from smol_amd import capi

    k, t = tab._keep, tab.struct
    cm = t.feature_mode == capi.FEATURES_CORRELATIONS
    Fce = int(t.num_corr if cm else t.num_orbits)
    orb = k["loc_orbit"].astype(np.int64)
    scale = float(t.size) / k["loc_ratio"] / k["loc_nrows"].astype(np.float64)
    n_recs = max(1, len(np.unique(np.stack([orb.astype(np.float64), scale]), axis=1).T)) if len(orb) else 1
    used = np.unique(orb)
    K = k["orb_nfunc"][used].astype(np.int64) if cm else np.ones(len(used), dtype=np.int64)
    t_off = (k["orb_ctensor_off"] if cm else k["orb_itensor_off"])[used]
    tens_len = int((t_off + K * k["orb_tensor_len"][used]).max(initial=0))
    return dict(Fce=Fce, F=int(tab.num_features), Npad=(int(t.num_sites) + 15) // 16 * 16, R=int(R),
                table=bool(t.n_flip_vectors) if table is None else bool(table), n_recs=int(n_recs), tens_len=tens_len,
                occ_hbm_env=bool(occ_hbm_env), all_k1=bool((K == 1).all()))


# ---------------------------------------------------------------------------------------------------------------------
# the cases: the smallest shapes that reach each state of the layout
# ---------------------------------------------------------------------------------------------------------------------
# prim: ("fcc", species), ("tri", species) (a triclinic one-site cell) or "salt" (rocksalt, three cation species, inert anions); mode "int" / "corr"; step "swap" / "flip" /
# "table"; env: SMOLMC_FORCE_UNIVERSAL unless the model reaches the kernel by itself; extra: also one run_sampled block
# and one Wang-Landau handle (both read the features through the accepted-step cells).
# args: layout()'s arguments as the tables give them (the device test derives them again and compares); want: the state
# the case is there for, checked against layout(**args) on the host.
Case = collections.namedtuple("Case", "name prim cutoffs dims mode step R env extra args want")
FORCE, HBM = "SMOLMC_FORCE_UNIVERSAL", "SMOLMC_UNIV_OCC_HBM"
PAIR = {2: 3.0}


def _a(Fce, F, Npad, R, table, n_recs, tens_len, occ_hbm_env=False, all_k1=True):
    return dict(Fce=Fce, F=F, Npad=Npad, R=R, table=table, n_recs=n_recs, tens_len=tens_len, occ_hbm_env=occ_hbm_env, all_k1=all_k1)


CASES = []  # filled below


def _case(name, prim, cutoffs, dims, mode, step, R, env, extra, args, **want):
    CASES.append(Case(name, prim, dict(cutoffs), tuple(dims), mode, step, R, tuple(env), extra, args, want))


@functools.lru_cache(maxsize=None)
def model_of(prim, cutoffs):
    """The cluster model of a case (cutoffs as a sorted tuple of items): built once per process -- twelve species take seconds."""
    from smol_amd import synth

    if prim == "salt":
        p = synth.rocksalt_prim()
    elif prim[0] == "tri":  # one site, inversion the only point symmetry: every pair of lattice vectors +-v is an orbit
        p = synth.PrimCell(np.array([[3.0, 0, 0], [0.4, 3.3, 0], [0.3, 0.5, 3.7]]), [[0, 0, 0]], [prim[1]])
    else:
        p = synth.fcc_prim(nspecies=prim[1])
    return synth.build_cluster_model(p, dict(cutoffs))


@functools.lru_cache(maxsize=None)
def tables_of(name):
    """(supercell, TableSet) of a case."""
    from smol_amd import capi, synth

    c = BY_NAME[name]
    model = model_of(c.prim, tuple(sorted(c.cutoffs.items())))
    sc = synth.build_supercell(model, list(c.dims))
    kw = {}
    if c.step == "table":  # the cation table of tests/test_gpu_table_flip.py: 3 Mn3+ <-> 1 Li+ + 2 Ti4+
        kw = dict(flip_table=np.array([[1, -3, 2]]), swap_weight=0.3)
    mode = capi.FEATURES_CORRELATIONS if c.mode == "corr" else capi.FEATURES_INTERACTIONS
    return sc, capi.TableSet.from_synth(sc, synth.random_coefs(model, seed=6), feature_mode=mode, **kw)


def start_state(name):
    """(occupancies, seeds, temperatures) of a case's walkers: random species; charge neutral for the TableFlip case."""
    c = BY_NAME[name]
    sc, _ = tables_of(name)
    rng = np.random.default_rng(1000 + [k.name for k in CASES].index(name))
    if c.step == "table":
        P = sc.size  # cations 0 .. P-1 against fixed O2-: n_Li + 3 n_Mn + 4 n_Ti = 2 P
        occ = np.zeros((c.R, sc.num_sites), dtype=np.int32)
        for r in range(c.R):
            n_ti = 2 * (P // 18 + r % 7)
            n_mn = (P - 3 * n_ti) // 2
            perm = rng.permutation(P)
            occ[r, perm[:n_mn]] = 1
            occ[r, perm[n_mn:n_mn + n_ti]] = 2
    else:
        nsp = np.array([sc.model.prim.nspecies[b] for b in sc.site_b])
        occ = (rng.random((c.R, sc.num_sites)) * nsp).astype(np.int32)
    return occ, rng.integers(1, 2 ** 62, size=c.R).astype(np.uint64), np.linspace(1500.0, 6000.0, c.R)


FCC2, TRIPLETS = ("fcc", 2), {2: 4.5, 3: 3.0}
# -- the feature-cell classes (each also sampled and under Wang-Landau): 64 sites, 5 walkers
_case("dshift3", FCC2, TRIPLETS, (4, 4, 4), "int", "swap", 5, [FORCE], True, _a(5, 5, 64, 5, False, 4, 18),
      dshift=3, dict=1, wpb=4, lds=15296)
_case("dshift2", ("fcc", 5), {2: 6.0, 3: 3.0}, (4, 4, 4), "corr", "flip", 5, [FORCE], True,
      _a(65, 65, 64, 5, False, 6, 3520, all_k1=False), dshift=2, dict=0, dict_off=("tensors",), lds=11328)
_case("dshift1", ("fcc", 6), {2: 6.0, 3: 4.2}, (4, 4, 4), "corr", "flip", 5, [FORCE], True,
      _a(176, 176, 64, 5, False, 7, 25950, all_k1=False), dshift=1, dict=0, dict_off=("tensors", "features"), lds=17664)
_case("dshift0", ("fcc", 9), {2: 6.0, 3: 3.0}, (4, 4, 4), "corr", "flip", 5, [FORCE], True,
      _a(273, 273, 64, 5, False, 6, 99216, all_k1=False), dshift=0, dict=0, dict_off=("tensors", "features"), lds=18304)
_case("no-cells", ("fcc", 12), {2: 6.0, 3: 4.2}, (4, 4, 4), "corr", "flip", 3, [FORCE], True,
      _a(1288, 1288, 64, 3, False, 7, 1786884, all_k1=False), dfeat_cells=0, dict=0, lds=768)
# -- more than 64 distinct records on small tensors and few features: 65 pair orbits of a triclinic cell
_case("dict-records", ("tri", 2), {2: 10.5}, (4, 4, 4), "int", "swap", 5, [FORCE], False, _a(67, 67, 64, 5, False, 66, 262),
      dict=0, dict_off=("records",))
# -- waves per workgroup and the large workgroups: binary fcc with nearest-neighbour pairs, 3 walkers (the last workgroup
#    of the two-wave layout has one live wave behind the dictionary barrier)
_case("wpb2", FCC2, PAIR, (26, 26, 26), "int", "swap", 3, [FORCE], False, _a(3, 3, 17584, 3, False, 2, 6), wpb=2, dict=1, lds=48800)
_case("wpb1-above-64k", FCC2, PAIR, (40, 40, 40), "int", "swap", 3, [FORCE], False, _a(3, 3, 64000, 3, False, 2, 6),
      wpb=1, dict=1, lds=77216)
_case("largest-with-dict", FCC2, PAIR, (53, 53, 53), "int", "swap", 3, [FORCE], False, _a(3, 3, 148880, 3, False, 2, 6),
      wpb=1, dict=1, occ_lds=1, lds=162096)
# -- the window: occupancy + dictionaries exceed a CU's LDS, the occupancy alone does not (no switch: the model reaches
#    the universal kernel by itself, "occupancy does not fit LDS")
_case("window", FCC2, PAIR, (54, 54, 55), "int", "swap", 3, [], False, _a(3, 3, 160384, 3, False, 2, 6),
      wpb=1, dict=0, dict_off=("window",), occ_lds=1, lds=160800)
# -- crowded launches (3073 walkers): no shrink, dshift lowered with the dictionaries kept, dshift 0 and dictionaries dropped
_case("crowded-control", FCC2, PAIR, (18, 18, 18), "int", "swap", 3073, [FORCE], False, _a(3, 3, 5840, 3073, False, 2, 6),
      crowded="no", dshift=3, dict=1, wpb=4, lds=37824)
_case("crowded-shift", FCC2, PAIR, (16, 20, 21), "int", "swap", 3073, [FORCE], False, _a(3, 3, 6720, 3073, False, 2, 6),
      crowded="shift", dshift=2, dict=1, wpb=4, lds=40832)
_case("crowded-drop", FCC2, PAIR, (20, 20, 20), "int", "swap", 3073, [FORCE], False, _a(3, 3, 8000, 3073, False, 2, 6),
      crowded="drop", dshift=0, dict=0, dict_off=("crowding",), wpb=4, lds=32768)
# -- a TableFlip handle (scratch 2464 B) at a shrunk crowded layout: rocksalt cations, 12x12x15 = 4320 sites
_case("crowded-table", "salt", {2: 4.5}, (12, 12, 15), "int", "table", 3073, [FORCE], False, _a(4, 4, 4320, 3073, True, 3, 21),
      crowded="shift", dshift=2, dict=1, wpb=4, table=1, lds=40576)
# -- dense launches meet K1 = 0 and the occupancy in HBM
_case("dense-k0", ("fcc", 3), TRIPLETS, (4, 4, 4), "corr", "flip", 3073, [FORCE], False,
      _a(13, 13, 64, 3073, False, 4, 168, all_k1=False), k1=0, dict=1, lds=17600)
_case("dense-hbm", FCC2, TRIPLETS, (4, 4, 4), "int", "swap", 3073, [FORCE, HBM], False,
      _a(5, 5, 64, 3073, False, 4, 18, occ_hbm_env=True), occ_lds=0, dict=1, lds=15040)
# -- the two instantiations of the Flip / Swap handles with the occupancy in LDS that the cases above leave out
_case("k0-dict", ("fcc", 3), TRIPLETS, (4, 4, 4), "corr", "flip", 5, [FORCE], False, _a(13, 13, 64, 5, False, 4, 168, all_k1=False),
      k1=0, dict=1, lds=17600)
_case("dense-k0-nodict", ("fcc", 5), {2: 6.0, 3: 3.0}, (4, 4, 4), "corr", "flip", 3073, [FORCE], False,
      _a(65, 65, 64, 3073, False, 6, 3520, all_k1=False), k1=0, dict=0, dshift=2, lds=11328)
BY_NAME = {c.name: c for c in CASES}
CASE_IDS = list(BY_NAME)
assert len(BY_NAME) == len(CASES)
# the models whose tables a host test may build (the others take seconds: the device test derives their arguments)
CHEAP = ("dshift3", "dshift2", "dshift1", "dict-records", "wpb2", "crowded-shift", "crowded-table", "dense-k0", "dense-hbm", "k0-dict",
         "dense-k0-nodict")


def case_layout(name):
    return layout(**BY_NAME[name].args)


# every value of every switch: what the case table must reach (tests/test_univ_layout_host.py)
STATES = ["dshift=3", "dshift=2", "dshift=1", "dshift=0", "no cells", "dict on", "dict off: records", "dict off: tensors",
          "dict off: features", "dict off: crowding", "dict off: window", "occ lds", "occ hbm", "wpb=4", "wpb=2", "wpb=1",
          "crowded: no shrink", "crowded: shift lowered, dictionaries kept", "crowded: shift 0, dictionaries dropped",
          "one wave above 64 KiB", "k1=0", "k1=1", "table=0", "table=1", "dense=0", "dense=1"]


def states_of(L):
    """The STATES a layout is a case of.  dshift counts where nothing shrank it (the crowded outcomes are states of their own)."""
    s = {"dict on" if L.dict else None, "occ lds" if L.occ_lds else "occ hbm", f"wpb={L.wpb}", f"k1={L.k1}", f"table={L.table}",
         f"dense={L.dense()}"}
    s |= {f"dict off: {why}" for why in L.dict_off}
    if not L.dfeat_cells:
        s.add("no cells")
    elif L.crowded == "no":
        s.add(f"dshift={L.dshift}")
    if L.R > CROWDED_R and L.wpb == 4:
        s.add({"no": "crowded: no shrink", "shift": "crowded: shift lowered, dictionaries kept",
               "drop": "crowded: shift 0, dictionaries dropped"}[L.crowded])
    if L.wpb == 1 and L.total > WORKGROUP_MAX:
        s.add("one wave above 64 KiB")
    return s - {None}
