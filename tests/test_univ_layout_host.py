"""The LDS layout of the universal kernel, on the host: the restated rule (tests/univ_layout.py) keeps every request
inside a CU's LDS where the rule before it did not, the case table reaches every value of every switch, and the
pinned arguments of the cheap cases are what their tables give."""

import itertools
import os

import pytest

from smol_amd import codeobj, engine
from tests import univ_layout as ul

KIB = 1024


def _scratch(Fce, F, table, dshift):
    cells = (Fce + 1) // 2 * 2 if Fce <= 1024 else 0
    return (ul.SCRATCH_TABLE if table else ul.SCRATCH) + ((cells << dshift) + ((F + 1) // 2 * 2 if cells else 0)) * 8


def _npads(Fce, table):
    """16 ... 176 000: every multiple of 16 where a threshold of the rule can fall for this model (whatever dshift the
    crowded branch leaves), every 1024 elsewhere."""
    lo, hi = _scratch(Fce, Fce, table, 0), _scratch(Fce, Fce, table, 3)
    edges = [q - s for q in (40 * KIB, 64 * KIB, 160 * KIB, 160 * KIB - 256) for s in (0, ul.DICT_BYTES)]
    edges = [e // w for e in edges for w in (1, 2, 4)]
    fine = set()
    for e in edges:
        fine.update(range(max(16, (e - hi - 64) // 16 * 16), min(176000, e - lo + 64) + 1, 16))
    return sorted(fine | set(range(16, 176001, 1024)))


def parent_total(scratch, Npad, shared):
    """The rule before the window fallback: the occupancy stays in LDS whenever it fits WITHOUT the dictionaries."""
    with_occ = (scratch + Npad + 15) // 16 * 16
    per_wave = with_occ if with_occ <= 160 * KIB - 256 else scratch
    return shared + per_wave * next(w for w in (4, 2, 1) if w == 1 or shared + per_wave * w <= 64 * KIB)


SWEEP = list(itertools.product((2, 64, 66, 256, 258, 1024, 1026), (False, True), (False, True), (5, 3073)))


@pytest.mark.parametrize("Fce,table,dicts,R", SWEEP, ids=[f"Fce{a}-{'table' if b else 'flip'}-{'dict' if c else 'nodict'}-R{d}" for a, b, c, d in SWEEP])
def test_budget_property(Fce, table, dicts, R):
    n_recs, tens = (2, 6) if dicts else (65, 6)
    over = []
    for Npad in _npads(Fce, table):
        L = ul.layout(Fce, Fce, Npad, R, table, n_recs, tens)
        assert L.total <= 160 * KIB, (Npad, L)
        assert L.wpb == 1 or L.total <= 64 * KIB, (Npad, L)
        assert L.total == L.lds_shared + L.lds_per_wave * L.wpb
        assert L.occ_off % 16 == 0 and L.lds_per_wave % 16 == 0 and L.lds_shared % 16 == 0, (Npad, L)
        assert not L.occ_lds or L.occ_off - L.lds_shared + Npad <= L.lds_per_wave  # the occupancy ends inside the wave's block
        if L.dict:
            assert Fce <= ul.DICT_NAT and dicts
        # the rule before the fix, at the shadow copies this layout has (crowding lowers them only in four-wave workgroups,
        # far below the window): above a CU's LDS exactly where the window fallback acts
        scratch = _scratch(Fce, Fce, table, L.dshift)
        if parent_total(scratch, Npad, ul.DICT_BYTES if dicts and Fce <= ul.DICT_NAT else 0) > 160 * KIB:
            over.append((scratch + Npad + 15) // 16 * 16)
            assert L.dict_off == ("window",) and L.occ_lds and L.dict == 0 and L.wpb == 1, (Npad, L)
        else:
            assert "window" not in L.dict_off, (Npad, L)
    if dicts and Fce <= ul.DICT_NAT:
        # the defect stays documented: with the dictionaries on, the old rule asks for more than 163 840 B exactly where
        # scratch + occupancy lies in (160 KiB - 12 800, 160 KiB - 256]
        assert over and min(over) == 160 * KIB - ul.DICT_BYTES + 16 and max(over) == 160 * KIB - 256, (min(over, default=0), max(over, default=0))
    else:
        assert not over


def test_the_examples_of_the_defect():
    """Binary fcc with nearest-neighbour pairs (three features): 54x54x55 reaches the kernel by itself, 54x54x54 under
    SMOLMC_FORCE_UNIVERSAL; the old rule asked for 173 600 B and 170 688 B."""
    for sites, old, new in ((54 * 54 * 55, 173600, 160800), (54 ** 3, 170688, 157888)):
        Npad = (sites + 15) // 16 * 16
        assert parent_total(_scratch(3, 3, False, 3), Npad, ul.DICT_BYTES) == old > 160 * KIB
        L = ul.layout(3, 3, Npad, 3, False, 2, 6)
        assert (L.total, L.dict, L.occ_lds, L.wpb, L.dict_off) == (new, 0, 1, 1, ("window",))
    # one cell below the window the dictionaries stay, above it the occupancy leaves LDS
    assert ul.layout(3, 3, 160 * KIB - ul.DICT_BYTES - 416, 3, False, 2, 6).dict == 1
    L = ul.layout(3, 3, 160 * KIB - 256 - 416 + 16, 3, False, 2, 6)
    assert (L.occ_lds, L.dict, L.wpb) == (0, 1, 4)


@pytest.mark.parametrize("name", ul.CASE_IDS)
def test_a_case_is_in_the_state_it_is_there_for(name):
    c, L = ul.BY_NAME[name], ul.case_layout(name)
    for key, want in c.want.items():
        assert {"lds": L.total}.get(key, getattr(L, key, None)) == want, (key, L)
    assert c.args["R"] == c.R and c.args["table"] == (c.step == "table") and c.args["occ_hbm_env"] == (ul.HBM in c.env)


def test_coverage_rule_and_its_teeth():
    """Every value of every switch has a case; and the rule bites: a state that one case alone reaches is missed without it."""
    reached = {name: ul.states_of(ul.case_layout(name)) for name in ul.CASE_IDS}
    assert set().union(*reached.values()) >= set(ul.STATES), sorted(set(ul.STATES) - set().union(*reached.values()))
    assert set().union(*reached.values()) <= set(ul.STATES)
    sole = [n for n in ul.CASE_IDS if any(sum(s in r for r in reached.values()) == 1 for s in reached[n])]
    assert {"dshift1", "dshift0", "no-cells", "dict-records", "wpb2", "window", "crowded-drop", "dense-hbm"} <= set(sole)
    for n in sole:
        rest = set().union(*(r for m, r in reached.items() if m != n))
        assert not rest >= set(ul.STATES), n
    assert [c.name for c in ul.CASES if c.extra] == ["dshift3", "dshift2", "dshift1", "dshift0", "no-cells"]


@pytest.mark.parametrize("name", ul.CHEAP)
def test_pinned_arguments_are_what_the_tables_give(name):
    c = ul.BY_NAME[name]
    _, tab = ul.tables_of(name)
    assert ul.args_of(tab, c.R, occ_hbm_env=ul.HBM in c.env) == c.args


def test_words_round_trip():
    L = ul.case_layout("crowded-table")
    info = f"universal occ=lds field=0 {L.words()} (environment override) env=SMOLMC_FORCE_UNIVERSAL"
    assert ul.info_words(info) == "lds=40576 wpb=4 dshift=2 dict=1 k1=1 table=1 dense=1"
    assert ul.case_layout("no-cells").words() == "lds=768 wpb=4 dcells=0 dict=0 k1=0 table=0 dense=0"
    assert ul.info_words("universal occ=lds field=0 lds=27392 (TableFlip outside the lean families)") == ""
    assert L.symbol() == "void mc_univ_kernel<true, true, true, 4, true>(UParams, int)"


def test_both_libraries_hold_the_same_universal_kernels():
    """The bounds build traps gathers of other kernels only: its 32 mc_univ_kernel instantiations are the release
    library's, byte for byte -- which is why tests/test_gpu_univ_layout.py runs the release library alone."""
    bounds = os.path.join(os.path.dirname(engine.LIB_PATH), "libsmolmc_hip_bounds.so")
    if not (os.path.exists(engine.LIB_PATH) and os.path.exists(bounds)):
        pytest.skip("the libraries are not built")
    a, b = ({n: d for n, d in codeobj.kernel_digests(p).items() if "mc_univ_kernel<" in n} for p in (engine.LIB_PATH, bounds))
    assert len(a) == 32 and a == b
