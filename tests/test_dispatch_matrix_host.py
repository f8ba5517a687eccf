"""The dispatch matrix on the built library's symbol table (no device): every kernel classified, every case's cell a
kernel of the library, the reduced-matrix coverage rule with its teeth, and predict() against expectations derived by
hand from the launchers (launch.h, the ends of mc_lean.h, mc_lean_multi.h, mc_wl.h, mc_general.h; engine.hip:
lean_families, lean_launcher, family_of)."""

import collections
import itertools
import os

import pytest

from smol_amd import codeobj, engine
from tests import dispatch_matrix as dm

pytestmark = pytest.mark.skipif(not os.path.exists(engine.LIB_PATH), reason="libsmolmc_hip.so not built")
BOUNDS = os.path.join(os.path.dirname(engine.LIB_PATH), "libsmolmc_hip_bounds.so")


@pytest.fixture(scope="module")
def symbols():
    return sorted(codeobj.kernel_digests(engine.LIB_PATH))


def test_every_symbol_falls_into_exactly_one_class(symbols):
    cls = dm.classify(symbols)  # (raises on a kernel that is neither a known template nor a HELPERS entry)
    count = collections.Counter(cls.values())
    print(dict(count))
    assert set(cls) == set(symbols) and sum(count.values()) == len(symbols)
    assert count["helper"] == len(dm.HELPERS), sorted(set(dm.HELPERS) - {dm.helper_name(s) for s in symbols})
    for module in set(dm.HELPERS.values()):
        assert os.path.exists(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), module)), module
    # the classes partition the Monte-Carlo instantiations; a cell is one symbol
    shown = [dm.show(dm.coords(s)) for s in symbols if dm.coords(s) is not None]
    assert len(set(shown)) == len(shown)
    assert count["covered"] == len(set(dm.TARGETS.values())) + len(set(dm.UNIV_TARGETS.values()))
    assert not set(dm.TARGETS.values()) & set(dm.UNIV_TARGETS.values())
    # the entries of NEVER_DISPATCHED that name symbols of this library (the others guard against additions)
    named = collections.Counter(dm.never_dispatched(dm.coords(s)) for s in symbols if dm.coords(s) is not None)
    assert named["lean LV_WL"] == 8 and named["mc_kernel MM outside its index type"] == 32, named


def test_the_bounds_library_has_the_same_kernels(symbols):
    if not os.path.exists(BOUNDS):
        pytest.skip("libsmolmc_hip_bounds.so not built")
    assert sorted(codeobj.kernel_digests(BOUNDS)) == symbols


def test_every_case_names_a_kernel_of_the_library(symbols):
    by_show = {dm.show(dm.coords(s)): s for s in symbols if dm.coords(s) is not None}
    assert len({c.id for c in dm.CASES}) == len(dm.CASES)
    for name, target in dm.UNIV_TARGETS.items():  # the universal kernel's cells: the layout cases
        assert target in by_show and dm.coords(by_show[target]).template == "mc_univ_kernel", (name, target)
    for case in dm.CASES:
        target = dm.TARGETS[case.id]
        assert target in by_show, (case.id, target)
        assert dm.never_dispatched(dm.coords(by_show[target])) is None, (case.id, target)


def test_coverage_rule_and_its_teeth(symbols):
    """Among dispatchable symbols every (F, V) pair and every (F, NSLOT, MM, STEP) tuple has a case or an UNREACHED entry;
    and the rule bites: without any one case that is the sole cover of a coordinate, the assertion fails."""
    need = dm.required(symbols)
    targets = [dm.TARGETS[c.id] for c in dm.CASES] + sorted(set(dm.UNIV_TARGETS.values()))
    names = [c.id for c in dm.CASES] + sorted(set(dm.UNIV_TARGETS.values()))
    cover = [dm.covered_by([t], symbols) for t in targets]  # (each case's two coordinates)

    def uncovered(covers):
        return {q for q in need - set().union(*covers) if dm.unreached(q) is None}

    assert not uncovered(cover), sorted(uncovered(cover), key=str)[:10]
    left = need - set().union(*cover)
    mc = {q for q in need if q[1] not in ("univ", "univ-dict", "dist", "dist-replay")}
    print(f"required {len(need)}, covered {len(need) - len(left)}, unreached {len(left)} = {100.0 * len(left) / len(need):.1f} % "
          f"({len(left - mc)} of them on the universal kernel, whose cells are the layout cases, and the distance kernels, which the matrix "
          f"does not model; {len(left & mc)} of {len(mc)} planner refusals)")
    univ = {q for q in need if q[1] in ("univ", "univ-dict")}
    assert len(univ) == 36 and len(univ & left) == 23  # (10 cells = 10 (F, V) pairs and 3 shapes; the rest by the two entries)
    # no case covers an UNREACHED coordinate: an entry that a case reaches must be deleted
    assert all(dm.unreached(q) is None for q in set().union(*cover)), "an UNREACHED entry is covered by a case"
    cover_count = collections.Counter(q for c in cover for q in c)
    sole = [i for i, c in enumerate(cover) if any(cover_count[q] == 1 for q in c)]
    assert len(sole) > len(targets) // 2  # (the matrix is a greedy cover: most cases are the only one on a coordinate)
    for i in sole:  # the rule on a copy of the cases without case i
        assert uncovered(cover[:i] + cover[i + 1:]), names[i]


F = dm.Facts
FLIP, SWAP, TABLE = 0, 1, 2
LEAN, MULTI = "void mc_lean_kernel<%s>(LeanParams)", "void mc_lean_multi_kernel<%s>(LeanParams)"
TAB, TABM, WL = "void mc_table_kernel<%s>(LeanParams)", "void mc_table_multi_kernel<%s>(LeanParams)", "void mc_wl_kernel<%s>(LeanParams)"
# One handle description per launcher list, with the kernel read off the C++ by hand:
#   mc_lean_kernel<NSLOT, MM, STEP, MU, EWX, WL, BIAS, SOLO, KF, OCC, REPLAY>      (EWX: Ewald mode | 4 with per-walker mu)
#   mc_lean_multi_kernel<NSLOT, MM, STEP, MU, EWX, REG, BIAS, REPLAY, WLX>         (WLX: 1 WL, 2 WL_KF, | 4 with windows)
#   mc_table_kernel<NSLOT, MM, EWX, REPLAY, BIAS, WL>    mc_table_multi_kernel<NSLOT, MM, EWX, REPLAY, WL, BIAS>
#   mc_wl_kernel<NSLOT, MM, STEP | 16 with windows, REPLAY, MU, EW>                mc_kernel<IdxT, NSLOT, MM, GENERIC, WL>
EXPECTED = [
    # launch_lean_nslot: the solo layouts, and lean_key's `ew_field ? 2 : 1`
    ("lean nslot=2 mm=2 field=0 lds=1280 solo=1 occ=6", F(SWAP), LEAN % "2, 2, 1, false, 0, false, false, true, 0, 6, false"),
    ("lean nslot=4 mm=3 field=1 lds=9000 gx=1x3x3x3", F(FLIP, mu=True, ewald=True), LEAN % "4, 3, 0, true, 2, false, false, false, 0, 0, false"),
    # launch_lean_mu_ew<LV_BIAS>: an Ewald term without the field in LDS is mode 1
    ("lean nslot=2 mm=3 field=0 lds=9000", F(FLIP, bias=True, mu=True, ewald=True), LEAN % "2, 3, 0, true, 1, false, true, false, 0, 0, false"),
    ("lean nslot=2 mm=2 field=0 lds=9000", F(SWAP, bias=True, replay=True), LEAN % "2, 2, 1, false, 0, false, true, false, 0, 0, true"),
    ("lean nslot=4 mm=2 field=0 lds=10400 kf=1", F(SWAP), LEAN % "4, 2, 1, false, 0, false, false, false, 6, 0, false"),
    # launch_lean_replay_kf: LV_OCC6 is masked out of the key, the rows variants do not replay; KF has no solo layout
    ("lean nslot=2 mm=2 field=0 lds=1280 solo=1 occ=6 rows=21", F(FLIP, mu=True, replay=True),
     LEAN % "2, 2, 0, true, 0, false, false, true, 0, 0, true"),
    ("lean nslot=2 mm=3 field=1 lds=9000 kf=1", F(SWAP, ewald=True, replay=True), LEAN % "2, 3, 1, false, 2, false, false, false, 6, 0, true"),
    # per-walker chemical potentials: launch_lean_wmu_nslot, launch_lean_wmu_mu_ew<LV_BIAS / LV_KF>
    ("lean nslot=2 mm=2 field=0 lds=1280 solo=1 walker_mu=1 mu_max=0.5", F(FLIP, mu=True), LEAN % "2, 2, 0, true, 4, false, false, true, 0, 0, false"),
    ("lean nslot=4 mm=2 field=1 lds=9000 walker_mu=1 mu_max=0.5", F(FLIP, bias=True, mu=True, ewald=True),
     LEAN % "4, 2, 0, true, 6, false, true, false, 0, 0, false"),
    ("lean nslot=2 mm=2 field=0 lds=9000 kf=1 walker_mu=1 mu_max=0.5", F(FLIP, mu=True), LEAN % "2, 2, 0, true, 4, false, false, false, 6, 0, false"),
    # launch_lean_rows_nslot: MM is the rows shape
    ("lean nslot=2 mm=2 field=0 lds=1280 solo=1 rows=11", F(SWAP), LEAN % "2, 11, 1, false, 0, false, false, true, 0, 0, false"),
    # launch_table_nslot: lists <0, 2, 1> and, for Wang-Landau, <0, 2>
    ("lean nslot=2 mm=2 field=0 lds=9000", F(TABLE, mu=True, ewald=True), TAB % "2, 2, 1, false, false, false"),
    ("lean nslot=4 mm=3 field=1 lds=9000 wl=table", F(TABLE, wl=True, ewald=True), TAB % "4, 3, 2, false, false, true"),
    ("lean nslot=2 mm=2 field=1 lds=9000", F(TABLE, bias=True, ewald=True), TAB % "2, 2, 2, false, true, false"),
    ("lean nslot=2 mm=3 field=0 lds=9000", F(TABLE, replay=True), TAB % "2, 3, 0, true, false, false"),
    ("lean nslot=2 mm=2 field=1 lds=9000 walker_mu=1 mu_max=1", F(TABLE, mu=True, ewald=True), TAB % "2, 2, 6, false, false, false"),
    ("lean nslot=2 mm=2 field=1 lds=9000 walker_mu=1 mu_max=1", F(TABLE, bias=True, mu=True, ewald=True), TAB % "2, 2, 6, false, true, false"),
    # launch_wl_variant<0 / WV_REPLAY / WV_WIN>
    ("lean nslot=2 mm=2 field=1 lds=9000 wl=v3", F(SWAP, wl=True, mu=True, ewald=True), WL % "2, 2, 1, false, true, true"),
    ("lean nslot=4 mm=2 field=0 lds=9000 wl=v3", F(FLIP, wl=True, replay=True), WL % "4, 2, 0, true, false, false"),
    ("lean nslot=2 mm=3 field=0 lds=9000 wl=v3 wl_windows=1", F(SWAP, wl=True), WL % "2, 3, 17, false, false, false"),
    # launch_multi_variant: ew_field 1 / 2 straight through; MV_REG at NSLOT 8 on one site class
    ("lean-multi nslot=8 mm=2 field=2 lds=9000", F(FLIP, mu=True, ewald=True, ncls1=True), MULTI % "8, 2, 0, true, 2, true, false, false, 0"),
    ("lean-multi nslot=8 mm=3 field=1 lds=9000", F(SWAP, ewald=True), MULTI % "8, 3, 1, false, 1, false, false, false, 0"),
    ("lean-multi nslot=2 mm=2 field=0 lds=9000", F(SWAP, bias=True, replay=True), MULTI % "2, 2, 1, false, 0, false, true, true, 0"),
    ("lean-multi nslot=4 mm=2 field=1 lds=9000 wl=multi-mean", F(FLIP, wl=True, mu=True, ewald=True), MULTI % "4, 2, 0, true, 1, false, false, false, 1"),
    ("lean-multi nslot=4 mm=2 field=1 lds=9000 wl=multi-mean", F(FLIP, wl=True, mu=True, ewald=True, replay=True),
     MULTI % "4, 2, 0, true, 1, false, false, true, 1"),
    ("lean-multi nslot=4 mm=3 field=0 lds=9000 kf=1 wl=multi", F(SWAP, wl=True), MULTI % "4, 3, 1, false, 0, false, false, false, 2"),
    ("lean-multi nslot=2 mm=2 field=2 lds=9000 wl=multi wl_windows=1", F(SWAP, wl=True, ewald=True), MULTI % "2, 2, 1, false, 2, false, false, false, 5"),
    # launch_multi_wmu_variant<0 / MV_BIAS>
    ("lean-multi nslot=2 mm=2 field=1 lds=9000 walker_mu=1 mu_max=1", F(FLIP, mu=True, ewald=True), MULTI % "2, 2, 0, true, 5, false, false, false, 0"),
    ("lean-multi nslot=8 mm=2 field=0 lds=9000 walker_mu=1 mu_max=1", F(FLIP, bias=True, mu=True, ncls1=True),
     MULTI % "8, 2, 0, true, 4, true, true, false, 0"),
    # launch_table_multi_nslot: list <2, 0, 1>
    ("lean-multi nslot=2 mm=2 field=2 lds=9000", F(TABLE, ewald=True), TABM % "2, 2, 2, false, false, false"),
    ("lean-multi nslot=8 mm=2 field=0 lds=9000 wl=multi", F(TABLE, wl=True), TABM % "8, 2, 0, false, true, false"),
    ("lean-multi nslot=4 mm=3 field=1 lds=9000 walker_mu=1 mu_max=1", F(TABLE, bias=True, mu=True, ewald=True), TABM % "4, 3, 5, false, false, true"),
    ("lean-multi nslot=2 mm=2 field=0 lds=9000", F(TABLE, replay=True), TABM % "2, 2, 0, true, false, false"),
    # launch_general_nslot: GENERIC rows run MM 3 or 6, the others 2, 3 or 5
    ("general nslot=4 mm=6 field=0 lds=15616 env=SMOLMC_FORCE_GENERAL | not lean: environment override", F(SWAP, aliased=True),
     "void mc_kernel<int, 4, 6, true, false>(KParams, int)"),
    ("general nslot=16 mm=3 field=0 lds=58368 | not lean: more than 512 clusters per site", F(FLIP, wl=True),
     "void mc_kernel<unsigned short, 16, 3, false, true>(KParams, int)"),
]


@pytest.mark.parametrize("k", range(len(EXPECTED)))
def test_predict_against_hand_derived_expectations(k, symbols):
    info, facts, want = EXPECTED[k]
    assert dm.predict(info, facts) == want
    assert want in symbols, want


def test_keys_that_name_no_variant_take_the_last_entry(symbols):
    """first_match gives every other key to the LAST entry.  No handle produces such a key (below); a description that
    does shows what would run: per-walker chemical potentials on a solo handle WITHOUT a mu table (smolmc_set_walker_mu
    refuses it: walker_mu_refused, has_mu) would key LV_WMU | LV_SOLO, which names no entry of launch_lean_wmu_nslot's list,
    and launch the four-walker kernel (the list's last entry, LV_WMU | LV_MU) on the solo handle's grid."""
    info = "lean nslot=2 mm=2 field=0 lds=1280 solo=1 walker_mu=1 mu_max=0"
    symbol, key, variants = dm.trace(info, F(SWAP, mu=False))
    assert dm.falls_through(key, variants) and key == dm.LV_WMU | dm.LV_SOLO
    assert symbol == LEAN % "2, 2, 1, true, 4, false, false, false, 0, 0, false" and symbol in symbols
    # a TableFlip step on with_mm_step's <SWAP, FLIP> list would take FLIP: family_of keeps TableFlip handles off those launchers
    assert dm._mm_step(dm.parse_info("lean nslot=2 mm=2 field=0"), F(TABLE)) == (2, FLIP)


def test_families_without_a_launcher_are_refused_not_guessed():
    with pytest.raises(dm.NoLeanLauncher):  # K_TABLE_BIAS has no replay instantiation: smolmc_replay takes the universal kernel
        dm.predict("lean nslot=2 mm=2 field=0 lds=9000", F(TABLE, bias=True, replay=True))
    with pytest.raises(dm.NoLeanLauncher):  # K_MULTI_WL_KF takes no windows
        dm.predict("lean-multi nslot=2 mm=2 field=0 lds=9000 kf=1 wl=multi wl_windows=1", F(SWAP, wl=True))
    with pytest.raises(dm.NoLeanLauncher):  # (a text without the selector words is not guessed at)
        dm.predict("universal occ=lds field=0 lds=27392 (TableFlip outside the lean families)", F(TABLE))


UNIV = "void mc_univ_kernel<%s>(UParams, int)"
# smolmc_univ_selector's bits as kernel_info prints them -> mc_univ_kernel<OCC_LDS, K1, TABLE, WPS, DICT> (univ_select)
UNIV_EXPECTED = [
    ("universal occ=lds field=0 lds=27392 wpb=4 dshift=3 dict=1 k1=1 table=1 dense=0 (TableFlip outside the lean families)",
     UNIV % "true, true, true, 2, true"),
    ("universal occ=hbm field=2 lds=13312 wpb=4 dshift=2 dict=0 k1=0 table=0 dense=1 (more than 64 features) env=SMOLMC_UNIV_OCC_HBM",
     UNIV % "false, false, false, 4, false"),
    ("universal occ=lds field=0 lds=768 wpb=4 dcells=0 dict=0 k1=0 table=0 dense=0 (environment override) env=SMOLMC_FORCE_UNIVERSAL",
     UNIV % "true, false, false, 2, false"),
    ("universal occ=lds field=0 lds=160800 wpb=1 dshift=3 dict=0 k1=1 table=0 dense=0 (occupancy does not fit LDS)",
     UNIV % "true, true, false, 2, false"),
]


@pytest.mark.parametrize("k", range(len(UNIV_EXPECTED)))
def test_predict_the_universal_kernel_from_its_words(k, symbols):
    info, want = UNIV_EXPECTED[k]
    symbol, key, variants = dm.trace(info, F(SWAP))
    assert symbol == want and want in symbols and not dm.falls_through(key, variants)


def test_every_universal_instantiation_is_predicted_by_its_words(symbols):
    reached = {dm.predict(f"universal occ={occ} field=0 lds=1 wpb=4 dshift=0 dict={dl} k1={k1} table={tb} dense={dn} (x)", F(SWAP))
               for occ, dl, k1, tb, dn in itertools.product(("lds", "hbm"), *[(0, 1)] * 4)}
    assert reached == {s for s in symbols if dm.template_of(s) == "mc_univ_kernel"} and len(reached) == 32


def test_no_plausible_handle_reaches_an_else_or_leaves_the_library(symbols):
    """Every handle description the planners can produce (their exclusions restated below) predicts a symbol of the
    library through an entry that its key names; and every dispatchable symbol of the lean families is predicted by one."""
    lib, reached = set(symbols), set()
    for fam, nslot, mm, field, solo, occ6, kf, rows, wmu, win in itertools.product(
            ("lean", "lean-multi"), (2, 4, 8), (2, 3), (0, 1, 2), (False, True), (False, True), (False, True), (0, 21, 11), (False, True),
            (False, True)):
        multi = fam == "lean-multi"
        if (not multi and (nslot == 8 or field == 2)) or (solo and (multi or field or kf)) or (occ6 and not solo) or (rows and not solo):
            continue  # (decide_lean: NSLOT <= 4, the field in LDS only; solo without Ewald / KF; rows and occ=6 on solo handles)
        k = dm.Info(fam, nslot, mm, field, solo, occ6, kf, rows, wmu, win, None)
        for step, wl, bias, mu, ewald, replay, ncls1 in itertools.product((FLIP, SWAP, TABLE), *[(False, True)] * 6):
            if multi and ewald != bool(field):
                continue  # (plan_lean_multi: ew_field is 1 or 2 exactly when the model has an Ewald term)
            if (not multi and (field and not ewald or not ncls1)) or (solo and (wl or ewald or bias or step == TABLE)):
                continue
            if kf and (step == TABLE or bias or (wl != multi)) or (wl and bias) or (wl and not multi and ewald and not field):
                continue  # (lean_mode: KF is Metropolis on one class or Wang-Landau on the multi layout; no biased Wang-Landau)
            if (wmu and (not mu or wl or rows)) or (win and (not wl or wmu)):
                continue  # (walker_mu_refused, wl_windows_refused; kernel_info hides rows= while per-walker mu is set)
            try:
                symbol, key, variants = dm.trace(k, F(step, wl, bias, mu, ewald, replay, ncls1))
            except dm.NoLeanLauncher:
                continue
            assert symbol in lib, (k, step, symbol)
            assert not dm.falls_through(key, variants), (k, step, key, variants)
            reached.add(symbol)
    lean = {s for s in symbols if (c := dm.coords(s)) is not None and c.template not in ("mc_kernel", "mc_univ_kernel", "mc_dist_kernel")
            and dm.never_dispatched(c) is None}
    assert lean <= reached, sorted(lean - reached)[:5]
